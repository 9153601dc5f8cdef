"""Where the time of the register-window Conv2d forward / bwd-data kernels goes (csrc/conv2d_fwd.hip
c2_fwd_rw_kernel, csrc/conv2d_dgrad.hip c2_dgrad_rw_kernel): needs a library built with
-DENCX_C2_TRACE, e.g.
  make -C encodec-pytorch_amd trace   (-> encodec-pytorch_amd/ab/trace.so)
  ENCX_LIB=encodec-pytorch_amd/ab/trace.so python tools/c2_trace.py
One layer call at B 32 for three config-3 shapes of the 32 -> 32 3x9 stride-2 layers. Prints, per
kernel: the prologue (kernel entry -> after the weight-staging barrier), the main loop and the
epilogue per item (medians over waves and items), the share of the kernel's time in which both
waves of a SIMD (waves w and w + 4 of a workgroup) are outside their main loops at once -- over
the whole kernel, and between the pair's first main-loop start and last main-loop end, which leaves
only epilogues and item hand-overs -- and the tail after the first wave has finished."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'encodec-pytorch_amd'))

W, NWV = 32, 8           # int64 per wave (conv2d.h C2_TR_W), waves per workgroup
US = 10.0 / 1000.0       # 100 MHz ticks -> us
# (T2, Fi, dilation) of the layer input; Fo = (Fi - 1) / 2 + 1
SHAPES = [(184, 257, 1), (43, 1025, 1), (184, 65, 4)]


def union(iv):
    """Total length of the union of [a, b) intervals."""
    tot, end = 0.0, -np.inf
    for a, b in sorted(iv):
        if b > end:
            tot += b - max(a, end)
            end = b
    return tot


def report(name, raw, dt_us):
    tr = raw.reshape(-1, W)
    tr = tr[tr[:, 0] != 0]
    n = tr[:, 2].astype(int)
    t = tr.astype(np.float64) * US
    t0 = t[:, 0].min()
    last = np.array([t[i, 2 + 3 * n[i]] if n[i] else t[i, 1] for i in range(len(t))])
    span = last.max() - t0
    main, epi, gaps = [], [], []
    for i in range(len(t)):
        for k in range(n[i]):
            s, e, d = t[i, 3 + 3 * k: 6 + 3 * k]
            main.append(e - s)
            epi.append(d - e)
            if k:
                gaps.append(s - t[i, 2 + 3 * k])
    both_all, both_in, pairs = 0.0, 0.0, 0
    for w0 in range(0, len(t) - NWV + 1, NWV):
        for w in range(NWV // 2):
            a, b = w0 + w, w0 + w + NWV // 2
            iv = [(t[i, 3 + 3 * k], t[i, 4 + 3 * k]) for i in (a, b) for k in range(n[i])]
            if not iv or not n[a] or not n[b]:
                continue
            u = union(iv)
            lo, hi = min(x for x, _ in iv), max(y for _, y in iv)
            both_all += span - u
            both_in += (hi - lo) - u
            pairs += 1
    start = np.array([t[i, 3] for i in range(len(t)) if n[i]])
    print(f'{name}: {len(t)} waves, {int(n.sum())} items (max {n.max()} per wave), kernel {span:.1f} us by the '
          f'stamps ({dt_us:.1f} us by events)')
    print(f'  prologue {np.median(t[:, 1] - t[:, 0]):.2f} us (max {np.max(t[:, 1] - t[:, 0]):.2f}), first main-loop '
          f'start {np.median(start - t0):.2f} us after the first entry')
    print(f'  main loop {np.median(main):.2f} us / item (min {np.min(main):.2f}, max {np.max(main):.2f}), epilogue '
          f'{np.median(epi):.2f} us / item (min {np.min(epi):.2f}, max {np.max(epi):.2f})'
          + (f', epilogue end -> next main-loop start {np.median(gaps):.2f}' if gaps else ''))
    if pairs:
        print(f'  both waves of a SIMD outside their main loops: {100 * both_all / (pairs * span):.1f} % of the kernel '
              f'({both_all / pairs:.1f} us), of which between the first start and last end of their main loops '
              f'{100 * both_in / (pairs * span):.1f} % ({both_in / pairs:.1f} us)')
    print(f'  tail after the first wave finishes: {last.max() - last.min():.1f} us; sum per wave: prologue '
          f'{100 * np.sum(t[:, 1] - t[:, 0]) / (len(t) * span):.1f} %, main {100 * np.sum(main) / (len(t) * span):.1f} %, '
          f'epilogue {100 * np.sum(epi) / (len(t) * span):.1f} % of wave time')


def main():
    from encx import ops
    from encx._lib import call, ptr, stream
    dev = torch.device('cuda', 0)
    B, Ci, Co, k, s = 32, 32, 32, (3, 9), (1, 2)
    buf = torch.zeros(256 * NWV * W, dtype=torch.int64, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)

    def traced(name, fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        buf.zero_()
        call('encx_conv2d_trace', ptr(buf), buf.numel())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        call('encx_conv2d_trace', None, 0)
        report(name, buf.cpu().numpy(), e0.elapsed_time(e1) * 1000.0)

    for T2, Fi, dil in SHAPES:
        KT, KF, sf, dt, pt, pf, Fo = ops.conv2d_geometry(Fi, k, s, (dil, 1), (dil, 4))
        dims = (B, Ci, T2, Fi, Co, Fo, KT, KF, sf, dt, pt, pf)
        x = torch.randn(B, Ci, T2, Fi, generator=g, device=dev)
        fr = x + 0.3 * torch.randn(B, Ci, T2, Fi, generator=g, device=dev)
        wf = 0.1 * torch.randn(Co * Ci * KT * KF, generator=g, device=dev)
        bias = 0.1 * torch.randn(Co, generator=g, device=dev)
        wp = ops._wpoly(wf, Co, Ci, KT, KF, sf, x)
        y = torch.empty(B, Co, T2, Fo, device=dev)
        dy = torch.randn(B, Co, T2, Fo, generator=g, device=dev)
        dx = torch.empty_like(x)
        den = torch.rand(1, generator=g, device=dev) + 0.5
        fg = torch.rand(1, generator=g, device=dev) + 0.5
        code = torch.empty(x.numel(), device=dev, dtype=torch.uint8)
        outs, dens = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        ws = torch.empty(ops.lib.encx_disc_loss_workspace() // 4, device=dev)
        call('encx_feat_loss_code', ptr(fr), ptr(x), x.numel(), 3.0, ptr(outs), ptr(dens), 0, ptr(ws), ptr(code),
             stream())
        prev = ops.lib.encx_conv2d_select(1)
        try:
            print(f'== T2 {T2}, F {Fi} -> {Fo}, dilation {dil}, B {B}')
            traced('forward', lambda: call('encx_conv2d_fwd', ptr(x), ptr(wf), ptr(bias), ptr(y), *dims, 1, stream()))
            traced('bwd-data, LeakyReLU\'(y) mask, plain epilogue',
                   lambda: call('encx_conv2d_bwd_data', ptr(dy), ptr(y), ptr(wp), None, ptr(dx), 0, *dims, stream()))
            traced('bwd-data, y mask, feature code + x mask epilogue (premasking)',
                   lambda: call('encx_conv2d_bwd_data_feat', ptr(dy), ptr(y), ptr(wp), ptr(x), ptr(dx), 0, ptr(fr),
                                ptr(x), ptr(den), ptr(fg), 3.0, ptr(code), *dims, stream()))
            traced('bwd-data, premasked dy, feature code epilogue',
                   lambda: call('encx_conv2d_bwd_data_feat', ptr(dy), None, ptr(wp), None, ptr(dx), 0, ptr(fr),
                                ptr(x), ptr(den), ptr(fg), 3.0, ptr(code), *dims, stream()))
        finally:
            ops.lib.encx_conv2d_select(prev)


if __name__ == '__main__':
    main()
