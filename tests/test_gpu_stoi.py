"""STOI on the GPU (csrc/stoi.hip through encx.metrics), the validation epoch of
encx.train_multi_gpu and the cal_metrics command line.

Tolerance (the project's rule): |d_hip - d_64| <= max(4 |d_32 - d_64|, 1e-6), d_64 the numpy
restatement (tests/stoi_ref.py) in float64 and d_32 the same chain in plain float32. Every compared
row must sit at least 0.1 dB (fp64 margin) away from the silent-frame threshold: a frame within
rounding of that discrete threshold may legitimately fall on either side of it."""
import functools
import logging
import os
import random
import wave

import numpy as np
import pytest
import torch

import stoi_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NO_SCORE = float(np.float32(1e-5))


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, y) float32 arrays at 10 kHz, made once and shared."""
    g = np.random.default_rng(sum(map(ord, name)))
    if name.startswith('gated'):            # gated<T>@<snr>
        T, snr = name[5:].split('@')
        x = R.gated_signal(int(T))
        y = R.add_noise(x, float(snr))
    elif name.startswith('block'):          # block<T>: bursts switched at hop boundaries (long rows)
        x = R.block_gated_signal(int(name[5:]))
        y = R.add_noise(x, 5, seed=4)
    elif name.startswith('noise'):          # noise<T>: no silent frame
        T = int(name[5:])
        x = 0.1 * g.standard_normal(T)
        y = R.add_noise(x, 5, seed=T + 1)
    elif name == 'yzero':
        x = R.gated_signal(10000)
        y = np.zeros_like(x)
    elif name == 'xzero':
        y = R.gated_signal(10000)
        x = np.zeros_like(y)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


@functools.lru_cache(maxsize=None)
def refs(name):
    """(fp64 result, float32 result) of the restatement for a case."""
    x, y = case(name)
    return R.stoi_ref(x, y, np.float64), R.stoi_ref(x, y, np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(d_hip, r64, r32, what):
    tol = max(4 * abs(r32.score - r64.score), 1e-6)
    err = abs(float(d_hip) - r64.score)
    print(f'{what}: hip {float(d_hip):.9f} fp64 {r64.score:.9f} |err| {err:.3g} |fp32 - fp64| '
          f'{abs(r32.score - r64.score):.3g} tol {tol:.3g} (F {r64.F} n {r64.n} M {r64.M} margin {r64.margin:.3g} dB)')
    assert r64.margin >= 0.1
    assert err <= tol


# ---------------------------------------------------------------------------- kernel at 10 kHz
# block40000: 311 frames, a second pass of the kept-frame scan (256 frames per pass); block4194304:
# the longest row the library takes (2^22 samples, 32766 frames, 371 segment tiles: the finish
# kernel's second stride, the largest indices)
@pytest.mark.parametrize('name', ['gated10000@20', 'gated10000@5', 'gated10000@-5', 'gated25000@30', 'noise7000',
                                  'block40000', 'block4194304'])
def test_kernel_matches_fp64(name):
    from encx import metrics
    x, y = case(name)
    r64, r32 = refs(name)
    d, kept = metrics.stoi_10k(dev(x)[None], dev(y)[None], return_kept=True)
    assert int(kept[0]) == r64.n
    if not name.startswith('noise'):
        assert r64.n < r64.F  # the kept set has holes
    check(d[0], r64, r32, name)


@pytest.mark.parametrize('name', ['noise4224', 'noise4225', 'yzero', 'xzero'])
def test_edges_against_fp64(name):
    from encx import metrics
    x, y = case(name)
    r64, r32 = refs(name)
    if name == 'noise4224':
        assert (r64.F, r64.M) == (31, 30)  # one segment
    if name == 'xzero':
        assert r64.n == r64.F              # every frame ties at the maximum: all kept
    d, kept = metrics.stoi_10k(dev(x)[None], dev(y)[None], return_kept=True)
    assert int(kept[0]) == r64.n
    check(d[0], r64, r32, name)


@pytest.mark.parametrize('T', [4096, 256, 257, 100, 1])
def test_too_short_rows_score_1e_5(T):
    from encx import metrics
    g = np.random.default_rng(T)
    x = dev(g.standard_normal(T).astype(np.float32))
    d = metrics.stoi(x, x.clone(), 10000)
    assert d.dim() == 0 and d.dtype == torch.float32
    assert float(d) == NO_SCORE == metrics.NO_SCORE


def test_batch_rows_are_bit_identical_to_single_rows():
    from encx import metrics
    names = ['gated10000@5', 'noise4225', 'noise7000', 'noise4096']
    T = 10000
    g = np.random.default_rng(9)
    X = g.standard_normal((4, T)).astype(np.float32)  # whatever follows a row's samples is ignored
    Y = g.standard_normal((4, T)).astype(np.float32)
    lens = []
    for i, nm in enumerate(names):
        x, y = case(nm)
        X[i, :len(x)], Y[i, :len(y)] = x, y
        lens.append(len(x))
    assert lens == [10000, 4225, 7000, 4096]
    d = metrics.stoi(dev(X), dev(Y), 10000, lengths=torch.tensor(lens, device=DEV))
    assert d.shape == (4,)
    for i, nm in enumerate(names):
        x, y = case(nm)
        alone = metrics.stoi(dev(x), dev(y), 10000)
        assert d[i].view(torch.int32).item() == alone.view(torch.int32).item(), nm
    assert float(d[3]) == NO_SCORE


# ---------------------------------------------------------------------------- other rates
@pytest.mark.parametrize('sr', [24000, 16000])
def test_other_rates_go_through_resample(sr):
    from encx import metrics, ops
    g = np.random.default_rng(sr)
    t = np.arange(sr) / sr
    x = np.zeros(sr)
    for h in range(1, 25):
        x += np.sin(2 * np.pi * 150.0 * h * t + g.uniform(0, 2 * np.pi)) / np.sqrt(h)
    x = (0.05 * x * (1.2 + np.sin(2 * np.pi * 2.0 * t))).astype(np.float32)  # 1 s, modulated, never silent
    y = R.add_noise(x.astype(np.float64), 5, seed=3).astype(np.float32)
    xd, yd = dev(x), dev(y)
    d = metrics.stoi(xd, yd, sr)
    xr = ops.resample(xd[None, None], sr, 10000)[0, 0]
    yr = ops.resample(yd[None, None], sr, 10000)[0, 0]
    assert xr.shape[0] == 10000
    d10 = metrics.stoi_10k(xr[None].contiguous(), yr[None].contiguous())[0]
    assert d.view(torch.int32).item() == d10.view(torch.int32).item()
    xr, yr = xr.cpu().numpy(), yr.cpu().numpy()
    check(d, R.stoi_ref(xr, yr, np.float64), R.stoi_ref(xr, yr, np.float32), f'{sr} Hz')
    # batched with lengths: row 1 is the first 0.7 s of the clip, scored as that clip alone
    L = int(0.7 * sr)
    X, Y = torch.stack([xd, xd]), torch.stack([yd, yd])
    db = metrics.stoi(X, Y, sr, lengths=torch.tensor([sr, L], device=DEV))
    alone = metrics.stoi(xd[:L].contiguous(), yd[:L].contiguous(), sr)
    assert db[0].view(torch.int32).item() == d.view(torch.int32).item()
    assert db[1].view(torch.int32).item() == alone.view(torch.int32).item()


def test_argument_errors():
    from encx import metrics
    x = torch.zeros(10000)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        metrics.stoi(x, x, 10000)
    xd = x.to(DEV)
    with pytest.raises(NotImplementedError):
        metrics.stoi(xd, xd, 10000, extended=True)
    with pytest.raises(ValueError):
        metrics.stoi(xd, xd[:-1], 10000)


# ---------------------------------------------------------------------------- the validation epoch
CFG = {
    'common': {'save_interval': 1, 'test_interval': 5, 'log_interval': 1, 'max_epoch': 1, 'seed': 3401,
               'amp': False},
    'datasets': {'train_csv_path': None, 'test_csv_path': None, 'batch_size': 2, 'tensor_cut': 4800,
                 'num_workers': 0, 'fixed_length': 0, 'pin_memory': True},
    'checkpoint': {'resume': False, 'checkpoint_path': '', 'disc_checkpoint_path': '',
                   'save_folder': None,
                   'save_location': '${checkpoint.save_folder}/bs${datasets.batch_size}_cut${datasets.tensor_cut}_'},
    'optimization': {'lr': 3e-4, 'disc_lr': 3e-4},
    'lr_scheduler': {'warmup_epoch': 0},
    'model': {'target_bandwidths': [1.5, 3., 6., 12., 24.], 'sample_rate': 24000, 'channels': 1,
              'train_discriminator': True, 'audio_normalize': True, 'filters': 32, 'ratios': [8, 5, 4, 2],
              'disc_win_lengths': [1024, 2048, 512], 'disc_hop_lengths': [256, 512, 128],
              'disc_n_ffts': [1024, 2048, 512], 'causal': False, 'norm': 'time_group_norm',
              'segment': 'None', 'name': 'my_encodec'},
    'distributed': {'data_parallel': False, 'world_size': 1, 'find_unused_parameters': False,
                    'torch_distributed_debug': False, 'init_method': 'tcp'},
    'balancer': {'weights': {'l_t': 0.1, 'l_f': 1, 'l_g': 3, 'l_feat': 3}},
}


def config(tmp_path, **over):
    from encx.train_multi_gpu import load_config
    d = {k: dict(v) for k, v in CFG.items()}
    d['checkpoint']['save_folder'] = str(tmp_path / 'ck')
    for k, v in over.items():
        sec, key = k.split('__')
        d[sec][key] = v
    return load_config(d)


def snapshot(trainer):
    """Every piece of training state the validation epoch must leave alone, cloned."""
    s = {}
    for k, v in trainer.model.state_dict().items():
        s['model.' + k] = v.detach().clone()
    for k, v in trainer.disc.state_dict().items():
        s['disc.' + k] = v.detach().clone()
    for name, obj in (('opt', trainer.opt.state_dict()), ('opt_d', trainer.opt_d.state_dict()),
                      ('sched', trainer.sched.state_dict()), ('sched_d', trainer.sched_d.state_dict()),
                      ('balancer', vars(trainer.balancer))):
        def walk(prefix, o):
            if torch.is_tensor(o):
                s[prefix] = o.detach().clone()
            elif isinstance(o, dict):
                for kk, vv in o.items():
                    walk(f'{prefix}.{kk}', vv)
            elif isinstance(o, (list, tuple)):
                for i, vv in enumerate(o):
                    walk(f'{prefix}.{i}', vv)
            elif isinstance(o, (int, float, bool, str, type(None))):
                s[prefix] = o
        walk(name, obj)
    return s


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert torch.equal(a[k].contiguous().reshape(-1).view(torch.uint8),
                               b[k].contiguous().reshape(-1).view(torch.uint8)), k  # bitwise
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


# 0.2 - 0.3 s clips are too short for a score (fewer than 30 analysis frames at 10 kHz): stoi is
# NaN there; the 0.5 - 0.6 s set has a score for every row
@pytest.mark.parametrize('lengths', [(4800, 6000, 7200), (12000, 13200, 14400)])
def test_validation_epoch(tmp_path, lengths, caplog):
    import encx.train_multi_gpu as tm
    from encx import metrics
    from encx.data import CustomAudioDataset, read_wav
    from encx.losses import disc_loss, total_loss
    from encx.train import Trainer
    cfg = config(tmp_path, datasets__tensor_cut=24000)
    torch.manual_seed(5)
    model, disc = tm.build(cfg, torch.device(DEV))
    trainer = Trainer(model, disc, max_iter=10)
    g = np.random.default_rng(11)
    clips = [(0.1 * g.standard_normal(n)).astype(np.float32) for n in lengths]
    testset = CustomAudioDataset(cfg, mode='test', clips=clips, device=DEV)
    assert torch.equal(testset.get(1), dev(clips[1])[None])
    trainer.step(testset.make_batch([0, 1]))  # codebooks initialised, balancer and Adam state non-trivial
    model.train()
    disc.train()
    before = snapshot(trainer)
    random.seed(21)
    with caplog.at_level(logging.INFO, logger='encx.train'):
        out = tm.test(3, model, disc, testset, cfg)
    assert any('| TEST | epoch: 3 |' in r.getMessage() for r in caplog.records)
    assert model.training and disc.training
    same(before, snapshot(trainer))
    # the same calls by hand: batches [0, 1] and [2]; the last one's losses are reported
    scores = []
    model.eval()
    with torch.no_grad():
        for ids in ([0, 1], [2]):
            x = testset.make_batch(ids)
            y = model(x)
            lr, fr = disc(x)
            lf, ff = disc(y)
            want = dict(total_loss(fr, lf, ff, x, y, 24000), loss_disc=disc_loss(lr, lf))
            lens = torch.tensor([lengths[i] for i in ids], device=DEV)
            scores.append(metrics.stoi(x[:, 0].contiguous(), y[:, 0].contiguous(), 24000, lengths=lens))
    model.train()
    assert set(out) == {'l_t', 'l_f', 'l_g', 'l_feat', 'loss_disc', 'stoi'}
    for k, v in want.items():
        assert np.float32(out[k]).tobytes() == v.reshape(-1)[:1].cpu().numpy().tobytes(), k
    scores = torch.cat(scores).cpu().numpy()
    print('row scores', scores, 'reported', out['stoi'])
    ok = scores != np.float32(1e-5)
    if lengths[0] == 4800:
        assert not ok.any() and np.isnan(out['stoi'])
    else:
        assert ok.all()
        assert abs(out['stoi'] - float(scores.astype(np.float64).mean())) <= 1e-6
        assert -1.0 <= out['stoi'] <= 1.0
    # the dumped pair: the clip random.randrange picked, uncropped, and its reconstruction
    random.seed(21)
    pick = random.randrange(3)
    for name in ('GT.wav', 'Reconstruction.wav'):
        w, sr = read_wav(str(tmp_path / 'ck' / name))
        assert sr == 24000 and w.shape == (1, lengths[pick]), name
    gt, _ = read_wav(str(tmp_path / 'ck' / 'GT.wav'))
    assert np.abs(gt[0] - np.clip(clips[pick], -0.99, 0.99)).max() <= 1.0 / 32768


def write_wavs(folder, lengths, seed, name):
    g = np.random.default_rng(seed)
    paths = []
    os.makedirs(folder, exist_ok=True)
    for i, n in enumerate(lengths):
        x = (0.1 * g.standard_normal(n) * 32767).astype(np.int16)
        p = os.path.join(folder, f'{name}{i}.wav')
        with wave.open(p, 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(24000)
            w.writeframes(x.tobytes())
        paths.append(p)
    csv = os.path.join(folder, f'{name}.csv')
    with open(csv, 'w') as fh:
        fh.write('path\n' + '\n'.join(paths) + '\n')
    return csv


@pytest.mark.parametrize('graphs', [False, True])
def test_training_is_unchanged_by_validation(tmp_path, graphs, monkeypatch):
    """train() with a test set runs test() at epochs 0, 1, 2 and ends with bit-identical weights to
    train() without one. Training draws from Python's `random` every step (the bandwidth, the
    discriminator coin), and so does test() (the clip it dumps), so the wrapper puts the
    generator's state back after each validation epoch: what is compared is everything else."""
    import encx.train_multi_gpu as tm
    train_csv = write_wavs(str(tmp_path / 'wav'), (4800, 4000, 4400, 3600), 0, 'train')  # none above tensor_cut
    test_csv = write_wavs(str(tmp_path / 'wav'), (4800, 6000, 7200), 1, 'test')
    calls = []
    real = tm.test

    def wrapped(epoch, *a, **k):
        state = random.getstate()
        try:
            out = real(epoch, *a, **k)
        finally:
            random.setstate(state)
        calls.append((epoch, out))
        return out
    monkeypatch.setattr(tm, 'test', wrapped)
    finals = []
    for csv in (test_csv, None):
        sub = tmp_path / ('with' if csv else 'without')
        cfg = config(sub, datasets__train_csv_path=train_csv, datasets__test_csv_path=csv,
                     common__max_epoch=2, common__test_interval=1, common__hip_graphs=graphs)
        n0 = len(calls)
        tr = tm.train(0, 1, cfg)
        torch.cuda.synchronize()
        if csv:
            assert [c[0] for c in calls[n0:]] == [0, 1, 2]
            assert all(set(c[1]) == {'l_t', 'l_f', 'l_g', 'l_feat', 'loss_disc', 'stoi'} for c in calls[n0:])
            assert os.path.exists(sub / 'ck' / 'GT.wav') and os.path.exists(sub / 'ck' / 'Reconstruction.wav')
        else:
            assert len(calls) == n0 and not os.path.exists(sub / 'ck' / 'GT.wav')
        assert tr.sched.last_epoch == 4  # 2 epochs x 2 steps
        finals.append({**{'m.' + k: v.detach().clone() for k, v in tr.model.state_dict().items()},
                       **{'d.' + k: v.detach().clone() for k, v in tr.disc.state_dict().items()}})
    same(finals[0], finals[1])


# ---------------------------------------------------------------------------- cal_metrics
def test_cal_metrics_cli(tmp_path, capsys):
    from encx import cal_metrics, metrics
    from encx.data import read_wav
    from encx.utils import convert_audio, save_audio
    sr = 16000
    g = np.random.default_rng(4)
    pairs = []
    for rel, ref_name, deg_name, n in (('a', 'x.wav', 'x_bw6.0.wav', 16000), ('a/b', 'y.wav', 'y.wav', 14000)):
        t = np.arange(n) / sr
        x = sum(np.sin(2 * np.pi * 170.0 * h * t + g.uniform(0, 6.28)) / np.sqrt(h) for h in range(1, 20))
        x = 0.05 * x * (1.2 + np.sin(2 * np.pi * 2.0 * t))
        y = R.add_noise(x, 10, seed=n)[:n - 500]  # the degraded file is the shorter one
        for root, name, sig in (('ref', ref_name, x), ('deg', deg_name, y)):
            os.makedirs(tmp_path / root / rel, exist_ok=True)
            save_audio(torch.from_numpy(sig.astype(np.float32))[None], tmp_path / root / rel / name, sr)
        pairs.append((tmp_path / 'ref' / rel / ref_name, tmp_path / 'deg' / rel / deg_name))
    out = tmp_path / 'res'
    mean, nb, wb = cal_metrics.main(['-r', str(tmp_path / 'ref'), '-d', str(tmp_path / 'deg'), '-s', str(sr),
                                     '-b', '6.0', '-o', str(out)])
    assert np.isnan(nb) and np.isnan(wb)
    want = []
    for ref, deg in pairs:
        a, b = (convert_audio(dev(read_wav(str(p))[0]), sr, sr, 1)[0] for p in (ref, deg))
        m = min(len(a), len(b))
        want.append(float(metrics.stoi(a[:m].contiguous(), b[:m].contiguous(), sr)))
    assert all(0.3 < w < 1.0 for w in want)
    lines = (out / 'stoi_scores.txt').read_text().splitlines()
    assert sorted(lines) == sorted(f'{r}\t{d}\t{w}' for (r, d), w in zip(pairs, want))
    assert mean == sum(want) / 2 or abs(mean - sum(want) / 2) < 1e-15
    printed = capsys.readouterr().out
    assert f'STOI: {mean}' in printed and 'PESQ: not available' in printed
    assert not (out / 'pesq_scores.txt').exists()
