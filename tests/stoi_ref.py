"""numpy restatement of STOI (Taal, Hendriks, Heusdens, Jensen 2011, extended=False) at 10 kHz,
written from the definition in include/encx.h; the tests' reference for csrc/stoi.hip.

`stoi_ref(x, y, dtype)` runs every step in `dtype`: float64 is the reference, plain float32 the
error yardstick (what the same chain costs in the kernel's number format). It returns the score
together with F (frames), n (frames kept), M (analysis frames) and the margin: the smallest
|e_i - (max e - 40)| over the frames, in dB, i.e. how far the closest frame is from changing
sides of the silent-frame threshold."""
import collections

import numpy as np

FS, NF, HOP, NFFT, J, N, DYN = 10000, 256, 128, 512, 15, 30, 40.0
MINFREQ = 150.0
EPS = float(np.finfo(np.float64).eps)  # 2^-52
CLIP = 10.0 ** (15.0 / 20.0)

Result = collections.namedtuple('Result', 'score F n M margin')


def band_edges():
    """(lo, hi) bin ranges [lo, hi) of the 15 third-octave bands: the bins nearest to
    sqrt(cf_k cf_{k-+1}), cf_k = 150 * 2^(k/3), on the grid k * 10000 / 512."""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    k = np.arange(J, dtype=np.float64)
    fl = MINFREQ * 2.0 ** ((2 * k - 1) / 6)
    fh = MINFREQ * 2.0 ** ((2 * k + 1) / 6)
    lo = [int(np.argmin((f - a) ** 2)) for a in fl]
    hi = [int(np.argmin((f - a) ** 2)) for a in fh]
    return lo, hi


def window():
    return np.hanning(NF + 2)[1:-1]


def frames(length):
    """len(range(0, length - NF, HOP))"""
    return len(range(0, int(length) - NF, HOP))


def stoi_ref(x, y, dtype=np.float64):
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype)
    y = np.asarray(y, dtype)
    assert x.ndim == 1 and x.shape == y.shape
    w = window().astype(dtype)
    eps = dt(EPS)
    starts = list(range(0, len(x) - NF, HOP))
    F = len(starts)
    if F == 0:
        return Result(1e-5, 0, 0, 0, float('inf'))
    idx = np.asarray(starts)[:, None] + np.arange(NF)[None]
    xf, yf = w * x[idx], w * y[idx]
    e = dt(20) * np.log10(np.sqrt((xf * xf).sum(1, dtype=dtype)) + eps)
    thr = e.max() - dt(DYN)
    keep = e > thr
    margin = float(np.abs(e.astype(np.float64) - float(thr)).min())
    xf, yf = xf[keep], yf[keep]
    n = int(keep.sum())
    xs = np.zeros((n - 1) * HOP + NF, dtype)
    ys = np.zeros_like(xs)
    for i in range(n):  # overlap-add of the kept windowed frames
        xs[i * HOP:i * HOP + NF] += xf[i]
        ys[i * HOP:i * HOP + NF] += yf[i]
    M = len(range(0, (n - 1) * HOP, HOP))
    if M < N:
        return Result(1e-5, F, n, M, margin)
    lo, hi = band_edges()

    def bands(sig):
        fr = w * sig[np.arange(M)[:, None] * HOP + np.arange(NF)[None]]
        # numpy >= 2 transforms float32 input in single precision (complex64 out); an older one
        # computes in fp64, and its output is then rounded
        spec = np.fft.rfft(fr, NFFT, axis=1)
        p = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
        return np.stack([np.sqrt(p[:, a:b].sum(1, dtype=dtype)) for a, b in zip(lo, hi)])  # [J][M]

    X, Y = bands(xs), bands(ys)
    # every 30-frame run of every band, 4096 runs at a time: [J][runs][N]
    xw = np.lib.stride_tricks.sliding_window_view(X, N, axis=1)
    yw = np.lib.stride_tricks.sliding_window_view(Y, N, axis=1)
    total = dt(0)
    for s0 in range(0, M - N + 1, 4096):
        xseg, yseg = xw[:, s0:s0 + 4096], yw[:, s0:s0 + 4096]
        alpha = np.sqrt((xseg * xseg).sum(-1, dtype=dtype, keepdims=True)) / \
            (np.sqrt((yseg * yseg).sum(-1, dtype=dtype, keepdims=True)) + eps)
        yp = np.minimum(alpha * yseg, (dt(1) + dt(CLIP)) * xseg)
        xc = xseg - xseg.mean(-1, dtype=dtype, keepdims=True)
        yc = yp - yp.mean(-1, dtype=dtype, keepdims=True)
        xc = xc / (np.sqrt((xc * xc).sum(-1, dtype=dtype, keepdims=True)) + eps)
        yc = yc / (np.sqrt((yc * yc).sum(-1, dtype=dtype, keepdims=True)) + eps)
        total = total + (xc * yc).sum(dtype=dtype)
    return Result(float(total / dt(J * (M - N + 1))), F, n, M, margin)


def gated_signal(T, seed=0):
    """A harmonic tone (f0 140 Hz, 30 partials up to 4.2 kHz, random phases, 1/sqrt(h) amplitudes)
    gated on and off at 3 Hz with smooth flanks, plus a noise floor 60 dB below it: speech-like
    in that the silent-frame removal drops a non-contiguous third of its frames."""
    g = np.random.default_rng(seed)
    t = np.arange(T) / FS
    s = np.zeros(T)
    for h in range(1, 31):
        s += np.sin(2 * np.pi * 140.0 * h * t + g.uniform(0, 2 * np.pi)) / np.sqrt(h)
    gate = np.clip((np.sin(2 * np.pi * 3.0 * t + 0.3) + 0.25) / 0.2, 0.0, 1.0)
    gate = 0.5 - 0.5 * np.cos(np.pi * gate)
    s = s * gate + 1e-3 * g.standard_normal(T)
    return 0.3 * s / np.abs(s).max()


def block_gated_signal(T, seed=0):
    """A long row at little cost: 10000 samples of the harmonic tone (140 whole periods) tiled,
    under a slow 4 dB amplitude swing, switched on for 20 hops and off for 9 at hop boundaries,
    plus the -60 dB floor. A frame is then whole, half or not at all inside a burst, so every
    frame energy stays far from the silent-frame threshold however many frames there are."""
    g = np.random.default_rng(seed)
    t = np.arange(10000) / FS
    base = np.zeros(10000)
    for h in range(1, 31):
        base += np.sin(2 * np.pi * 140.0 * h * t + g.uniform(0, 2 * np.pi)) / np.sqrt(h)
    s = np.tile(base, T // 10000 + 1)[:T] * (0.8 + 0.2 * np.sin(2 * np.pi * np.arange(T) / 777777.0))
    s *= ((np.arange(T) // HOP) % 29 < 20)
    s = s / np.abs(s).max() + 1e-3 * g.standard_normal(T)
    return 0.3 * s


def add_noise(x, snr_db, seed=1):
    g = np.random.default_rng(seed)
    nz = g.standard_normal(len(x))
    nz *= np.sqrt((x * x).mean() / (nz * nz).mean()) * 10.0 ** (-snr_db / 20.0)
    return x + nz
