"""STOI (csrc/stoi.hip, encx.metrics): the numpy restatement the GPU tests compare against
(tests/stoi_ref.py) checked on its own, and the library's host-side entry points. No GPU."""
import numpy as np
import pytest

import stoi_ref as R

LO = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
HI = [9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]


def test_band_edges():
    lo, hi = R.band_edges()
    assert lo == LO and hi == HI


def test_identical_signals_score_one():
    x = R.gated_signal(10000)
    assert abs(R.stoi_ref(x, x).score - 1.0) <= 1e-12


def test_score_falls_with_snr():
    x = R.gated_signal(10000)
    d = [R.stoi_ref(x, R.add_noise(x, snr)).score for snr in (20, 5, -5)]
    print('stoi at +20 / +5 / -5 dB:', d)
    assert 1.0 > d[0] > d[1] > d[2] > 0.0
    assert d[0] > 0.95 and d[2] < 0.7


@pytest.mark.parametrize('T,F,n,M,segments', [(4224, 31, 31, 30, 1), (4225, 32, 32, 31, 2), (4096, 30, 30, 29, 0)])
def test_frame_counts(T, F, n, M, segments):
    g = np.random.default_rng(T)
    x = 0.1 * g.standard_normal(T)  # continuous noise: no frame is silent
    r = R.stoi_ref(x, R.add_noise(x, 5, seed=T + 1))
    assert (r.F, r.n, r.M) == (F, n, M)
    assert max(0, r.M - R.N + 1) == segments
    if segments == 0:
        assert r.score == 1e-5
    else:
        assert 0.0 < r.score < 1.0


def test_library_frame_count():
    from encx._lib import lib
    for T in (0, 1, 255, 256, 257, 384, 385, 4224, 4225, 1 << 22):
        assert lib.encx_stoi_frames(T) == R.frames(T), T
    assert lib.encx_stoi_frames(-1) == -1


def test_library_rejects_bad_arguments_on_the_host():
    from encx._lib import lib
    EINVAL = 9001
    assert lib.encx_stoi(None, None, None, None, None, 1, 10000, None) == EINVAL
    assert lib.encx_stoi(None, None, None, None, None, -1, 10000, None) == EINVAL
    assert lib.encx_stoi(None, None, None, None, None, 1, (1 << 22) + 1, None) == EINVAL
    assert lib.encx_stoi_workspace_floats(1, (1 << 22) + 1) == -1
    assert lib.encx_stoi_workspace_floats(-1, 100) == -1
    # counts, fp64 tile sums, norms + kept indices, two band maps: B + 2 B tiles + 2 B F + 30 B (F - 1)
    F = R.frames(10000)
    assert lib.encx_stoi_workspace_floats(3, 10000) == 4 + 2 * 3 * 1 + 2 * 3 * F + 30 * 3 * (F - 1)
    assert lib.encx_stoi_workspace_floats(2, 200) == 2


def test_metrics_refuses_cpu_tensors_and_extended():
    import torch
    from encx import metrics
    x = torch.zeros(10000)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        metrics.stoi(x, x, 10000)
    with pytest.raises(NotImplementedError):
        metrics.stoi(x, x, 10000, extended=True)


@pytest.mark.parametrize('n,world', [(10, 1), (10, 2), (7, 4), (3, 4), (0, 2)])
def test_validation_order_matches_torch_samplers(n, world):
    """The test loader of the reference: dataset order, DistributedSampler(shuffle=False) shards."""
    from torch.utils.data import BatchSampler, DistributedSampler, SequentialSampler
    from encx.train_multi_gpu import validation_order
    ds = list(range(n))
    if world == 1:
        assert validation_order(n, 0, 1, 3) == list(BatchSampler(SequentialSampler(ds), 3, False))
    for rank in range(world):
        ref = list(BatchSampler(DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=False), 3, False))
        assert validation_order(n, rank, world, 3) == ref
