"""bench.py's command line and its --dump-outputs writer (host logic only: no GPU, no library)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    return bench.parse()


def test_plain_run_is_lean_and_full_is_opt_in(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, '--full', '--dump-outputs', 'd', '--no-cpu-baseline')
    assert a.full and a.dump_outputs == 'd' and a.no_cpu_baseline and not a.no_roofline


def _fake_trainer(n_gen, n_disc):
    g = torch.Generator().manual_seed(5)
    opt = types.SimpleNamespace(flat=torch.randn(n_gen, generator=g))
    opt_d = types.SimpleNamespace(flat=torch.randn(n_disc, generator=g)) if n_disc else None
    codes = [(torch.arange(12).reshape(2, 6), None), (torch.arange(12, 24).reshape(2, 6), None)]
    return types.SimpleNamespace(last_y=torch.randn(3, 1, 50, generator=g), opt=opt, opt_d=opt_d,
                                 model=types.SimpleNamespace(seg_codes=codes))


def test_dump_outputs_files_dtype_and_fixed_sample(tmp_path):
    n = bench.DUMP_SAMPLE + 1234
    tr = _fake_trainer(n, 100)
    losses = {'l_t': torch.tensor(0.25), 'l_d': torch.tensor([2.0])}
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    bench.dump_outputs(a, tr, losses)
    bench.dump_outputs(b, tr, losses)
    names = sorted(os.listdir(a))
    assert names == ['codes.npy', 'loss_l_d.npy', 'loss_l_t.npy', 'params_disc.npy', 'params_gen.npy', 'y.npy']
    total = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float32 and np.array_equal(x, y), f
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(a, 'loss_l_t.npy')).tolist() == [0.25]
    assert np.array_equal(np.load(os.path.join(a, 'y.npy')), tr.last_y.numpy())
    assert np.array_equal(np.load(os.path.join(a, 'codes.npy')),
                          np.concatenate([np.arange(12).reshape(2, 6), np.arange(12, 24).reshape(2, 6)], 1))
    # small buffers whole, large ones as the same PCG64(4321) draw of positions every time
    assert np.array_equal(np.load(os.path.join(a, 'params_disc.npy')), tr.opt_d.flat.numpy())
    idx = np.random.Generator(np.random.PCG64(4321)).integers(0, n, bench.DUMP_SAMPLE)
    assert np.array_equal(np.load(os.path.join(a, 'params_gen.npy')), tr.opt.flat.numpy()[idx])


def test_dump_outputs_without_discriminator(tmp_path):
    bench.dump_outputs(str(tmp_path), _fake_trainer(10, 0), {'l_f': torch.tensor(1.5)})
    assert sorted(os.listdir(tmp_path)) == ['codes.npy', 'loss_l_f.npy', 'params_gen.npy', 'y.npy']
