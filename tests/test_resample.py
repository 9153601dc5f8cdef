"""Sample-rate conversion (csrc/resample.hip, encx.ops.resample, encx.utils, encx.data): the host
table and the fp64 restatement (CPU), the HIP kernel against the fp64 sum, and the any-rate
dataset (GPU, through the C ABI)."""
import math
import random
import types
import wave

import numpy as np
import pytest
import torch

import resample_ref as R
from oracle import data_oracle as D

DEV = 'cuda:0'
TILE = 1024  # outputs per workgroup of resample_kernel (RS_TILE) at every rate pair used here
U = 2.0 ** -24


def write_wav(path, x, sr):
    """x int16 [C][T] -> PCM16 file."""
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(x.shape[0])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(x.T).astype('<i2').tobytes())


def mid(y):
    n = y.shape[-1]
    return y[..., n // 10: n - n // 10]


# ------------------------------------------------------------------------------ CPU: table
@pytest.mark.parametrize('orig,new', R.PAIRS)
def test_table_matches_fp64_definition(orig, new):
    from encx import ops
    o, n, base, width, taps = R.geometry(orig, new)
    assert ops.resample_geometry(orig, new) == (o, n, width, taps, 2 * width + 1)
    _, coef, start = ops.resample_table(orig, new)
    assert coef.shape == (n, 2 * width + 1) and start.min() >= 0 and start.max() + 2 * width + 1 <= taps
    full = ops.resample_table(orig, new, full=True)
    ref = R.table64(orig, new)
    assert full.shape == ref.shape == (n, taps)
    err = np.abs(full.astype(np.float64) - ref).max()
    print(f'{orig}->{new}: (o, n) = ({o}, {n}), taps {taps}, kept {2 * width + 1}, max |table - fp64| = {err:.3g}')
    assert err <= 2.0 ** -23


@pytest.mark.parametrize('orig,new', R.PAIRS)
def test_out_len(orig, new):
    from encx import ops
    o, n, _, _, _ = R.geometry(orig, new)
    for L in sorted({1, 5, max(o - 1, 1), o, 5003}):
        assert ops.resample_out_len(L, orig, new) == math.ceil(n * L / o) == R.out_len(L, orig, new)


# ------------------------------------------------------------------------------ CPU: restatement
@pytest.mark.parametrize('orig,new', R.PAIRS)
@pytest.mark.parametrize('frac', [0.05, 0.25])
def test_restatement_resamples_a_sine(orig, new, frac):
    """A sine at `frac` of the lower rate's Nyquist frequency, 4000 input samples, against the
    analytic sine at the new rate over the middle 80 %: independent of torchaudio's formula."""
    f = frac * min(orig, new) / 2
    x = np.sin(2 * np.pi * f * np.arange(4000) / orig)
    y = R.resample64(x, R.table64(orig, new), orig, new)
    ref = np.sin(2 * np.pi * f * np.arange(y.shape[-1]) / new)
    err = np.abs(mid(y) - mid(ref)).max()
    print(f'{orig}->{new} sine at {frac} Nyquist: max err {err:.3g}')
    assert err <= 1e-3


@pytest.mark.parametrize('orig,new', R.PAIRS)
def test_restatement_against_scipy_resample_poly(orig, new):
    from scipy.signal import resample_poly
    o, n, _, _, _ = R.geometry(orig, new)
    t = np.arange(4000) / orig
    ny = min(orig, new) / 2
    x = (0.5 * np.sin(2 * np.pi * 0.05 * ny * t) + 0.3 * np.sin(2 * np.pi * 0.2 * ny * t + 1.0)
         + 0.2 * np.sin(2 * np.pi * 0.4 * ny * t + 2.0))
    y = R.resample64(x, R.table64(orig, new), orig, new)
    ref = resample_poly(x, n, o)
    assert ref.shape == y.shape
    err = np.abs(mid(y) - mid(ref)).max()
    print(f'{orig}->{new} vs resample_poly: max err {err:.3g}')
    assert err <= 1e-2


# ------------------------------------------------------------------------------ CPU: files
def test_read_wav_save_audio_round_trip(tmp_path):
    from encx.data import read_wav
    from encx.utils import save_audio
    g = np.random.default_rng(3)
    lim = int(0.99 * 32768) - 1
    x = g.integers(-lim, lim + 1, size=(2, 777)).astype(np.int16)
    x[0, :4] = [lim, -lim, 0, 1]
    a, b = tmp_path / 'a.wav', tmp_path / 'b.wav'
    write_wav(a, x, 16000)
    wav, sr = read_wav(str(a))
    assert sr == 16000 and wav.dtype == np.float32 and wav.shape == (2, 777)
    np.testing.assert_array_equal(wav, x.astype(np.float32) / 32768.0)
    save_audio(torch.from_numpy(wav), b, sr)
    assert a.read_bytes() == b.read_bytes()


def test_save_audio_clamp_and_rescale(tmp_path):
    from encx.data import read_wav
    from encx.utils import save_audio
    wav = torch.tensor([[0.5, -2.0, 1.5, 0.25, 0.0]])
    save_audio(wav, tmp_path / 'c.wav', 24000)
    got, sr = read_wav(str(tmp_path / 'c.wav'))
    assert sr == 24000
    q = lambda v: np.clip(np.round(np.asarray(v, np.float64) * 32768.0), -32768, 32767) / 32768.0  # noqa: E731
    np.testing.assert_array_equal(got[0], q(wav.clamp(-0.99, 0.99)[0].numpy()).astype(np.float32))
    save_audio(wav, tmp_path / 'r.wav', 24000, rescale=True)
    got, _ = read_wav(str(tmp_path / 'r.wav'))
    np.testing.assert_array_equal(got[0], q((wav * (0.99 / 2.0))[0].numpy()).astype(np.float32))
    assert np.abs(got).max() <= 0.99
    quiet = torch.tensor([[0.5, -0.25]])
    save_audio(quiet, tmp_path / 'q.wav', 24000, rescale=True)   # min(0.99 / max, 1) = 1: unchanged
    np.testing.assert_array_equal(read_wav(str(tmp_path / 'q.wav'))[0], quiet.numpy())
    # round half to even of x * 32768
    half = torch.tensor([[0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768]], dtype=torch.float64)
    save_audio(half, tmp_path / 'h.wav', 24000)
    np.testing.assert_array_equal(read_wav(str(tmp_path / 'h.wav'))[0][0] * 32768, [0, 2, 2, 0])


def test_load_wav_still_refuses_another_rate(tmp_path):
    from encx.data import load_wav, read_wav
    write_wav(tmp_path / 'a.wav', np.zeros((1, 10), np.int16), 16000)
    with pytest.raises(ValueError):
        load_wav(str(tmp_path / 'a.wav'), 24000, mono=True)
    assert load_wav(str(tmp_path / 'a.wav'), 16000, mono=True).shape == (1, 10)
    assert read_wav(str(tmp_path / 'a.wav'))[1] == 16000


# ------------------------------------------------------------------------------ CPU: errors
def test_bad_rates_and_channels_are_refused_before_any_device_call():
    from encx import ops
    from encx._lib import lib
    from encx.utils import convert_audio
    EINVAL = 9001
    # the C ABI: the argument check comes before any pointer is touched
    for B, Cin, Cout, L, orig, new in [(1, 1, 1, 5, 0, 24000), (1, 1, 1, 5, 16000, 0), (1, 1, 1, 5, -1, 24000),
                                       (1, 2, 3, 5, 16000, 24000), (1, 3, 2, 5, 16000, 24000),
                                       (1, 1, 3, 5, 16000, 24000), (1, 1, 1, 5, 24000, 24000)]:
        assert lib.encx_resample(None, None, None, B, Cin, Cout, L, orig, new, None) == EINVAL
    assert lib.encx_resample(None, None, None, 1, 2, 1, 5, 16000, 24000, None) == EINVAL   # null pointers
    assert lib.encx_resample_out_len(5, 0, 24000) == -1 and lib.encx_resample_table_floats(16000, 0) == -1
    assert lib.encx_resample_table(None, 16000, 24000) == EINVAL
    # a pair encx_resample refuses (table above 2^26 words, input span above the LDS budget) has no
    # table either: nothing of its size is allocated on the way to the error
    buf = np.zeros(4, np.float32)
    for orig, new in [(2 ** 31 - 1, 1), (1, 2 ** 31 - 1), (48000, 1000)]:
        assert lib.encx_resample_table_floats(orig, new) == -1
        assert lib.encx_resample_table(buf.ctypes.data, orig, new) == EINVAL
        assert lib.encx_resample(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 1, 1, 1, 4, orig, new, None) == EINVAL
        with pytest.raises(ValueError):
            ops.resample_table(orig, new)
    x = torch.zeros(2, 8)   # a CPU tensor: the rate and channel errors come first
    for orig, new in [(0, 24000), (16000, 0), (16000.5, 24000), (16000, 24000.0), (-3, 1)]:
        with pytest.raises(ValueError):
            ops.resample(x, orig, new)
    for C, Cout in [(2, 3), (3, 2), (1, 3)]:
        with pytest.raises(ValueError):
            ops.resample(torch.zeros(C, 8), 16000, 24000, channels=Cout)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.resample(x, 16000, 24000)
    with pytest.raises(AssertionError):
        convert_audio(torch.zeros(3, 8), 16000, 24000, 1)      # mono or stereo only
    with pytest.raises(RuntimeError, match='Impossible to convert'):
        convert_audio(torch.zeros(2, 8), 16000, 24000, 3)


# ------------------------------------------------------------------------------ GPU: kernel
# (orig, new) with reduced (o, n) = (2,3), (147,80), (160,147), (2,1), (1,6); the last pair's
# table (441 phases) is too large for LDS, so the kernel reads it from memory
GPU_PAIRS = [(16000, 24000), (44100, 24000), (48000, 44100), (48000, 24000), (8000, 48000), (16000, 22050)]


def past_tile_length(orig, new):
    """The shortest L whose last output is one sample past the first output tile: Lout = TILE + 1."""
    o, n, _, _, _ = R.geometry(orig, new)
    L = (TILE * o) // n + 1
    while R.out_len(L, orig, new) < TILE + 1:
        L += 1
    while R.out_len(L - 1, orig, new) >= TILE + 1:
        L -= 1
    return L


def check_against_fp64(orig, new, x, channels):
    """ops.resample(x [B][C][L]) against the fp64 sum over the full [n][taps] table: the product's
    own fp32 coefficients inside each phase's window, the definition's (rounded to fp32) at the
    taps the product drops."""
    from encx import ops
    o, n, _, width, taps = R.geometry(orig, new)
    _, coef, start = ops.resample_table(orig, new)
    tab = R.table64(orig, new).astype(np.float32)
    for p in range(n):
        tab[p, start[p]:start[p] + coef.shape[1]] = coef[p]
    B, Cin, L = x.shape
    y = ops.resample(torch.from_numpy(x).to(DEV), orig, new, channels=channels).cpu().numpy()
    Cout = Cin if channels is None else channels
    assert y.shape == (B, Cout, R.out_len(L, orig, new)) and y.dtype == np.float32
    x64 = x.astype(np.float64)
    if Cout == 1 and Cin > 1:
        src, asrc = x64.mean(1, keepdims=True), np.abs(x64).mean(1, keepdims=True)
    else:
        src = asrc = x64
    y64 = R.resample64(src, tab, orig, new)
    scale = R.resample64(asrc, tab, orig, new, absolute=True)
    if Cin == 1 and Cout == 2:
        y64, scale = np.repeat(y64, 2, 1), np.repeat(scale, 2, 1)
    m = taps + Cin
    gamma = m * U / (1 - m * U)
    bound = gamma * scale + U * np.abs(y64) + taps * 1e-30 * np.abs(x).max()
    err = np.abs(y.astype(np.float64) - y64)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'{orig}->{new} B {B} C {Cin}->{Cout} L {L}: max err {err.max() if err.size else 0:.3g}, '
          f'{worst:.3f} of the bound')
    assert np.all(err <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize('orig,new', GPU_PAIRS)
def test_gpu_resample_matches_fp64_sum(orig, new):
    o = R.geometry(orig, new)[0]
    g = np.random.default_rng(orig + new)
    lengths = sorted({1, 5, max(o - 1, 1), 5003, past_tile_length(orig, new)})
    for L in lengths:
        for B, Cin, channels in [(1, 1, None), (5, 1, None), (2, 2, None), (3, 2, 1), (2, 1, 2)]:
            x = g.uniform(-1, 1, size=(B, Cin, L)).astype(np.float32)
            check_against_fp64(orig, new, x, channels)


@pytest.mark.gpu
@pytest.mark.parametrize('orig,new', [(44100, 24000), (16000, 24000)])
def test_gpu_resample_rows_are_independent(orig, new):
    from encx import ops
    g = np.random.default_rng(11)
    x = torch.from_numpy(g.uniform(-1, 1, size=(5, 2, 5003)).astype(np.float32)).to(DEV)
    for channels in (None, 1):
        y = ops.resample(x, orig, new, channels=channels)
        assert torch.equal(y, ops.resample(x, orig, new, channels=channels))
        for b in range(x.shape[0]):
            assert torch.equal(ops.resample(x[b], orig, new, channels=channels), y[b])
            if channels is None:   # a channel by itself, and as a plain [1][L] row
                assert torch.equal(ops.resample(x[b, 1:2].contiguous(), orig, new), y[b, 1:2])
    mono = x[:, :1].contiguous()
    y2 = ops.resample(mono, orig, new, channels=2)
    assert torch.equal(y2[:, 0], y2[:, 1]) and torch.equal(y2[:, :1], ops.resample(mono, orig, new))


@pytest.mark.gpu
def test_gpu_resample_same_rate_keeps_the_samples():
    from encx import ops
    from encx.utils import convert_audio
    g = np.random.default_rng(12)
    x = torch.from_numpy(g.uniform(-1, 1, size=(2, 2, 301)).astype(np.float32)).to(DEV)
    assert torch.equal(ops.resample(x, 24000, 24000), x)
    assert torch.equal(convert_audio(x, 24000, 24000, 2), x)
    assert torch.equal(convert_audio(x, 24000, 24000, 1), x.mean(-2, keepdim=True))
    assert torch.equal(convert_audio(x[:, :1], 24000, 24000, 2), x[:, :1].expand(2, 2, 301))


# ------------------------------------------------------------------------------ GPU: dataset
def cfg(csv, cut, channels=1, sample_rate=24000):
    return types.SimpleNamespace(
        datasets=types.SimpleNamespace(fixed_length=0, tensor_cut=cut, train_csv_path=str(csv),
                                       test_csv_path=str(csv)),
        model=types.SimpleNamespace(sample_rate=sample_rate, channels=channels))


def make_files(tmp_path, specs):
    g = np.random.default_rng(21)
    files = []
    for i, (sr, ch, T) in enumerate(specs):
        p = tmp_path / f'clip{i}.wav'
        write_wav(p, g.integers(-20000, 20000, size=(ch, T)).astype(np.int16), sr)
        files.append(str(p))
    csv = tmp_path / 'files.csv'
    csv.write_text('path\n' + '\n'.join(files) + '\n')
    return csv, files


def pool_clips(pool):
    flat = pool.data.cpu().numpy()
    return [flat[o:o + c * n].reshape(c, n) for o, c, n in zip(pool.offsets, pool.channels, pool.lengths)]


@pytest.mark.gpu
def test_gpu_dataset_resamples_files_of_other_rates(tmp_path):
    from encx.data import CustomAudioDataset, read_wav
    from encx.utils import convert_audio
    specs = [(16000, 2, 4000), (24000, 1, 5000), (16000, 2, 2100), (24000, 1, 900), (16000, 2, 3333)]
    csv, files = make_files(tmp_path, specs)
    ds = CustomAudioDataset(cfg(csv, 1500), device=DEV)
    want = []
    for f in files:
        x, sr = read_wav(f)
        want.append(convert_audio(torch.from_numpy(x).to(DEV), sr, 24000, 1).cpu().numpy())
    assert want[0].shape == (1, 6000) and want[1].shape == (1, 5000)
    got = pool_clips(ds.pool)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    order = [3, 0, 4, 1, 2, 0]
    random.seed(77)
    out = ds.make_batch(order).cpu().numpy()
    random.seed(77)
    ref = D.collate([D.crop(D.expand(want[i], 1), 1500)[0] for i in order])
    np.testing.assert_array_equal(out, ref)


@pytest.mark.gpu
def test_gpu_dataset_at_the_model_rate_is_unchanged(tmp_path):
    from encx.data import AudioPool, CustomAudioDataset, load_wav
    csv, files = make_files(tmp_path, [(24000, 1, 3000), (24000, 2, 1234), (24000, 1, 10)])
    ds = CustomAudioDataset(cfg(csv, 1000), device=DEV)
    ref = AudioPool([load_wav(f, 24000, True) for f in files], device=DEV)
    assert torch.equal(ds.pool.data, ref.data)
    for k in ('channels', 'lengths', 'offsets'):
        np.testing.assert_array_equal(getattr(ds.pool, k), getattr(ref, k))
