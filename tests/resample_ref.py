"""fp64 restatement of torchaudio.transforms.Resample(orig, new) with its defaults
(sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), written from the definition in
include/encx.h; the reference of tests/test_resample.py. numpy only."""
import math

import numpy as np

# rate pairs of the tests and their reduced (o, n)
PAIRS = [(16000, 24000), (44100, 24000), (48000, 24000), (24000, 16000), (44100, 48000), (48000, 44100),
         (8000, 48000)]


def geometry(orig, new):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    width = math.ceil(6 * o / base)
    return o, n, base, width, 2 * width + o


def table64(orig, new):
    """table[p][t] in fp64, [n][taps]."""
    o, n, base, width, taps = geometry(orig, new)
    t = np.arange(taps, dtype=np.float64)[None, :]
    p = np.arange(n, dtype=np.float64)[:, None]
    tau = np.clip(((t - width) / o - p / n) * base, -6.0, 6.0)
    a = np.pi * tau
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    return sinc * np.cos(np.pi * tau / 12.0) ** 2 * (base / o)


def out_len(L, orig, new):
    o, n, _, _, _ = geometry(orig, new)
    return -((-n * L) // o)


def resample64(x, table, orig, new, absolute=False):
    """y[i n + p] = sum_t table[p][t] x[i o + t - width] over rows x [..., L] in fp64 (x = 0
    outside the row); `table` [n][taps] of any float type. With `absolute`, the same sum of
    |table| |x| (the scale of the rounding-error bound)."""
    o, n, _, width, taps = geometry(orig, new)
    x = np.asarray(x, np.float64)
    tab = np.asarray(table, np.float64)
    if absolute:
        x, tab = np.abs(x), np.abs(tab)
    L = x.shape[-1]
    Lout = out_len(L, orig, new)
    frames = -(-Lout // n)
    xp = np.zeros(x.shape[:-1] + (width + (frames - 1) * o + taps + L,), np.float64)
    xp[..., width:width + L] = x
    idx = np.arange(frames)[:, None] * o + np.arange(taps)[None, :]        # [frames][taps]
    y = np.einsum('...ft,pt->...fp', xp[..., idx], tab)                      # [..., frames, n]
    return y.reshape(x.shape[:-1] + (frames * n,))[..., :Lout]
