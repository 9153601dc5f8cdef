"""Resampler throughput: encx.ops.resample (csrc/resample.hip) against the same algorithm as
torchaudio runs it, F.conv1d(pad(x), table[:, None], stride=o) over the full [n][taps] table
through PyTorch-ROCm, in one process with alternating timed blocks.

Shapes: 64 rows x 30 s at 16 -> 24, 44.1 -> 24, 48 -> 24 and 48 -> 44.1 kHz, and the mono case
(64 x 2 channels -> 1) fused against torch's downmix followed by the resampler. Every block is
timed with device events after a warm-up and runs long enough that a shape gets >= 0.5 s of
work per variant. Per shape: ms per call of both (median over the rounds, and the rounds' min /
max as the run-to-run spread), the ratio, and the algorithmic bytes 4 (Cin L + Cout Lout) per row
over the kernel's time as a share of HBM peak (the kernel is HBM-bound: W multiply-adds per 8
bytes is far below the machine's flop/byte). Prints one JSON line and writes it, indented, to --out
(default profiles/resample/resample_bench.json).

python tools/resample_bench.py [--rows 64] [--seconds 30] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'encodec-pytorch_amd'))

HBM_PEAK_GBS = 8000.0
PAIRS = [(16000, 24000), (44100, 24000), (48000, 24000), (48000, 44100)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(a, b, rounds, min_seconds=0.5):
    """Alternating blocks of a and b -> (ms list of a, ms list of b)."""
    for fn in (a, b):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    iters = []
    for fn in (a, b):
        ms = timed(fn, 3)
        iters.append(max(3, int(np.ceil(min_seconds * 1e3 / rounds / ms))))
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(a, iters[0]))
        tb.append(timed(b, iters[1]))
    return ta, tb


def stats(ms):
    return {'ms': round(statistics.median(ms), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=30.0)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'resample', 'resample_bench.json'))
    args = ap.parse_args()
    from encx import ops
    dev = torch.device('cuda')
    g = torch.Generator(device='cpu').manual_seed(0)
    shapes = []
    for orig, new in PAIRS:
        o, n, width, taps, W = ops.resample_geometry(orig, new)
        L = int(args.seconds * orig)
        Lout = ops.resample_out_len(L, orig, new)
        x = (0.1 * torch.randn(args.rows, 1, L, generator=g)).to(dev)
        full = torch.from_numpy(ops.resample_table(orig, new, full=True)).to(dev)[:, None]   # [n][1][taps]

        def ours(x=x, orig=orig, new=new):
            return ops.resample(x, orig, new)

        def base(x=x, full=full, o=o, width=width, Lout=Lout):
            y = F.conv1d(F.pad(x, (width, width + o)), full, stride=o)           # [rows][n][frames]
            return y.transpose(1, 2).reshape(x.shape[0], 1, -1)[..., :Lout]

        ya, yb = ours(), base()
        diff = float((ya - yb).abs().max())
        ta, tb = compare(ours, base, args.rounds)
        a, b = stats(ta), stats(tb)
        gb = 4.0 * args.rows * (L + Lout) / 1e9
        shapes.append({
            'pair': f'{orig}->{new}', 'o_n': [o, n], 'taps_full': taps, 'taps_kept': W, 'rows': args.rows, 'L': L,
            'Lout': Lout, 'encx': a, 'conv1d_baseline': b, 'speedup': round(b['ms'] / a['ms'], 3),
            'spread_rel': round(max((a['max'] - a['min']) / a['ms'], (b['max'] - b['min']) / b['ms']), 4),
            'algorithmic_GB': round(gb, 4), 'GBs': round(gb / (a['ms'] * 1e-3), 1),
            'hbm_frac': round(gb / (a['ms'] * 1e-3) / HBM_PEAK_GBS, 4), 'bound': 'HBM bandwidth',
            'max_abs_diff_vs_baseline': diff})
        del x, full, ya, yb
        torch.cuda.empty_cache()

    # stereo -> mono: the mean fused into the staging, against torch's mean and then the kernel
    orig, new = 44100, 24000
    L = int(args.seconds * orig)
    Lout = ops.resample_out_len(L, orig, new)
    x2 = (0.1 * torch.randn(args.rows, 2, L, generator=g)).to(dev)
    fused = lambda: ops.resample(x2, orig, new, channels=1)                         # noqa: E731
    split = lambda: ops.resample(x2.mean(-2, keepdim=True), orig, new)              # noqa: E731
    diff = float((fused() - split()).abs().max())
    ta, tb = compare(fused, split, args.rounds)
    a, b = stats(ta), stats(tb)
    gb = 4.0 * args.rows * (2 * L + Lout) / 1e9
    mono = {'pair': f'{orig}->{new}', 'rows': args.rows, 'channels': '2->1', 'L': L, 'fused': a,
            'downmix_then_resample': b, 'speedup': round(b['ms'] / a['ms'], 3), 'algorithmic_GB': round(gb, 4),
            'GBs': round(gb / (a['ms'] * 1e-3), 1), 'hbm_frac': round(gb / (a['ms'] * 1e-3) / HBM_PEAK_GBS, 4),
            'max_abs_diff': diff}

    # the first shape again: the spread of a repeated measurement
    orig, new = PAIRS[0]
    x = (0.1 * torch.randn(args.rows, 1, int(args.seconds * orig), generator=g)).to(dev)
    fn = lambda: ops.resample(x, orig, new)                                         # noqa: E731
    ra, rb = compare(fn, fn, args.rounds)
    repeat = {'pair': f'{orig}->{new}', 'first': stats(ra), 'second': stats(rb),
              'rel_diff': round(abs(statistics.median(ra) - statistics.median(rb)) / statistics.median(ra), 4)}

    res = {'metric': 'ops.resample ms per call, 64 rows x 30 s, vs F.conv1d over the full table',
           'device': torch.cuda.get_device_name(0), 'hbm_peak_GBs': HBM_PEAK_GBS, 'rounds': args.rounds,
           'timing': 'device events around alternating blocks, >= 0.5 s per shape and variant, after warm-up',
           'shapes': shapes, 'mono': mono, 'repeat': repeat,
           'data': 'synthetic 0.1*N(0,1) rows'}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
