"""STOI throughput: encx.metrics.stoi (csrc/stoi.hip) on 64 rows x 10 s, at 10 kHz (the kernels
alone) and at 24 kHz (ops.resample to 10 kHz, then the kernels), against a CPU baseline.

The baseline is the tests' numpy restatement (tests/stoi_ref.py) in float32, one row per task
over a pool of 16 worker processes (the CPUs a job may use), on the 10 kHz rows. It is NOT the
reference's route: the reference scores files with the CPU library pystoi (cal_metrics.py:57-63),
one core per file, and that library is not in the image; the restatement runs the same chain with
numpy's vectorised framing, FFT and 30-frame segment windows. The 24 kHz
variant is compared with the same baseline (its resampled rows would cost the CPU route a
resampler on top, which is left out).

GPU timing: device events around blocks of calls after a warm-up, each variant >= 0.5 s of work
in total, 7 rounds; median and the rounds' min / max (the run-to-run spread), and the first
variant measured twice. `hbm_frac` is the algorithmic bytes 4 * 2 * B * T (x and y read once)
over the time, as a share of HBM peak: a whole-call figure over five launches (plus two resample
launches at 24 kHz), not one kernel's share. Prints one JSON line and writes it, indented, to --out
(default profiles/stoi/stoi_bench.json).

python tools/stoi_bench.py [--rows 64] [--seconds 10] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'encodec-pytorch_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_PEAK_GBS = 8000.0
WORKERS = 16


def make_rows(rows, seconds, sr):
    """Clean / degraded pairs: a harmonic tone gated on and off at 3 Hz (so a third of the frames
    is dropped as silent), white noise at +5 dB for the degraded row. float32 [rows][T]."""
    T = int(seconds * sr)
    t = np.arange(T) / sr
    X, Y = np.empty((rows, T), np.float32), np.empty((rows, T), np.float32)
    for i in range(rows):
        g = np.random.default_rng(i)
        s = np.zeros(T)
        for h in range(1, 31):
            s += np.sin(2 * np.pi * (120.0 + i) * h * t + g.uniform(0, 2 * np.pi)) / np.sqrt(h)
        gate = np.clip((np.sin(2 * np.pi * 3.0 * t + 0.1 * i) + 0.25) / 0.2, 0.0, 1.0)
        s = s * (0.5 - 0.5 * np.cos(np.pi * gate)) + 1e-3 * g.standard_normal(T)
        s *= 0.3 / np.abs(s).max()
        nz = g.standard_normal(T)
        nz *= np.sqrt((s * s).mean() / (nz * nz).mean()) * 10.0 ** (-5 / 20.0)
        X[i], Y[i] = s, s + nz
    return X, Y


def _baseline_row(xy):
    import stoi_ref
    return stoi_ref.stoi_ref(xy[0], xy[1], np.float32).score


def stats(ms):
    return {'ms': round(statistics.median(ms), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'stoi', 'stoi_bench.json'))
    args = ap.parse_args()

    X10, Y10 = make_rows(args.rows, args.seconds, 10000)
    # the CPU baseline first, in worker processes started before this one touches the GPU
    import multiprocessing as mp
    base_ms, base_scores = [], None
    with mp.get_context('spawn').Pool(WORKERS) as pool:
        pairs = list(zip(X10, Y10))
        pool.map(_baseline_row, pairs[:WORKERS])  # warm-up: imports, numpy's FFT plans
        for _ in range(3):
            t0 = time.perf_counter()
            base_scores = pool.map(_baseline_row, pairs, chunksize=1)
            base_ms.append((time.perf_counter() - t0) * 1e3)
    base = stats(base_ms)

    import torch
    from encx import metrics
    if not torch.cuda.is_available():
        raise SystemExit('stoi_bench needs the GPU: nothing is measured without one')
    dev = torch.device('cuda')

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def measure(fn, rounds, min_seconds=0.5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters = max(3, int(np.ceil(min_seconds * 1e3 / rounds / timed(fn, 3))))
        return [timed(fn, iters) for _ in range(rounds)], iters

    variants = []
    for sr in (10000, 24000):
        X, Y = (X10, Y10) if sr == 10000 else make_rows(args.rows, args.seconds, sr)
        xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
        fn = lambda xd=xd, yd=yd, sr=sr: metrics.stoi(xd, yd, sr)  # noqa: E731
        scores = fn().cpu().numpy()
        ms, iters = measure(fn, args.rounds)
        a = stats(ms)
        gb = 4.0 * 2 * X.shape[0] * X.shape[1] / 1e9
        v = {'sr': sr, 'rows': X.shape[0], 'T': X.shape[1], 'encx': a, 'calls_per_round': iters,
             'spread_rel': round((a['max'] - a['min']) / a['ms'], 4),
             'audio_seconds_per_second': round(X.shape[0] * args.seconds / (a['ms'] * 1e-3), 1),
             'algorithmic_GB': round(gb, 5), 'GBs': round(gb / (a['ms'] * 1e-3), 1),
             'hbm_frac': round(gb / (a['ms'] * 1e-3) / HBM_PEAK_GBS, 5),
             'speedup_vs_cpu_baseline': round(base['ms'] / a['ms'], 1),
             'mean_score': round(float(scores.mean()), 6)}
        if sr == 10000:
            v['max_abs_diff_vs_baseline_scores'] = float(np.abs(scores - np.asarray(base_scores)).max())
            again, _ = measure(fn, args.rounds)
            v['repeat'] = {'second': stats(again),
                           'rel_diff': round(abs(statistics.median(again) - a['ms']) / a['ms'], 4)}
        variants.append(v)

    res = {'metric': f'metrics.stoi ms per call, {args.rows} rows x {args.seconds:g} s',
           'device': torch.cuda.get_device_name(0), 'hbm_peak_GBs': HBM_PEAK_GBS, 'rounds': args.rounds,
           'timing': 'device events around blocks of calls, >= 0.5 s per variant, after warm-up',
           'variants': variants,
           'cpu_baseline': dict(base, what='tests/stoi_ref.py in float32 numpy on the 10 kHz rows, one row per '
                                'task over 16 worker processes, host clock, 3 runs after a warm-up; not the '
                                'reference\'s pystoi route (that library is not in the image)',
                                audio_seconds_per_second=round(args.rows * args.seconds / (base['ms'] * 1e-3), 1)),
           'bound': 'not HBM bandwidth (see hbm_frac): five short dependent launches; the per-kernel times '
                    'are a trace of its own (profiles/stoi/kernel_trace.md)',
           'data': 'synthetic gated harmonic rows, white noise at +5 dB'}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
