"""The persistent LSTM backward with the K-split as the unit of work (lstm_bwd_pers, csrc/lstm.hip:
workgroup (l, bg, nt, s) contracts one split of a 64-column tile from a copy of DA staged in LDS,
the four workgroups of a tile exchange their partials through a two-slot ring) against the
launch-per-step form (option LSTM_PERSIST 0), at the smallest shapes that reach each of its paths.
Both forms keep one summation order, so the gate grads DA and the input grad dx must be the same
bits: no tolerance. Every case proves by encx_lstm_bwd_form that the persistent kernel ran, and
reuses its buffers (the ring among them) over two rounds of fresh inputs."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# B, H, T, L
SHAPES = {
    # T 1: no frame contracts in the recurrent tiles, so the exchange is skipped in all four
    # workgroups of a tile alike; one row: clamped row addresses; G 2
    't1_one_row': (1, 128, 1, 1),
    # the first exchanged frame, the XP hand-off between layers, both ring slots used once
    't2_two_layers': (2, 128, 2, 2),
    # the G 6 instantiation; the third frame rewrites ring slot 0; exactly one full row group
    'g6_slot_reuse': (16, 384, 3, 1),
    # three layers, a ragged second row group (4 of 16 rows), ring reuse over several frames
    'three_layers_ragged': (20, 256, 9, 3),
    # the workload's widths and its 256-workgroup grid (every CU, the co-residency edge), short T
    'full_grid': (32, 512, 4, 2),
}
CASES = [pytest.param(*shape, acc, False, id=f'{name}-acc{acc}') for name, shape in SHAPES.items() for acc in (0, 1)]
# dx NULL: layer 0's input tiles store nothing but still take part in the exchange
CASES.append(pytest.param(*SHAPES['three_layers_ragged'], 0, True, id='three_layers_ragged-nodx'))


@pytest.mark.parametrize('B,H,Tn,L,acc_x,no_dx', CASES)
def test_lstm_bwd_split_bit_identical(B, H, Tn, L, acc_x, no_dx):
    from encx._lib import call, ptr, option, lib, lstm_sync_errors
    gen = torch.Generator().manual_seed(31 * B + H + Tn)
    k = H ** -0.5
    f = lambda *s: ((torch.rand(*s, generator=gen) * 2 - 1) * k).to(DEV)
    e = lambda n: torch.empty(n, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    wcat, wcatT, bsum = e(L * 8 * H * H), e(L * 8 * H * H), e(L * 4 * H)
    for l in range(L):
        call('encx_lstm_pack', *(ptr(f(*s)) for s in [(4 * H, H), (4 * H, H), (4 * H,), (4 * H,)]),
             ptr(wcat), ptr(wcatT), ptr(bsum), H, l, st)
    with option(LSTM_PERSIST=1):
        assert lib.encx_lstm_bwd_form(B, Tn, H, L) == 1, 'the persistent form does not admit this shape here'
    with option(LSTM_PERSIST=0):
        assert lib.encx_lstm_bwd_form(B, Tn, H, L) == 0
    x, dout = torch.empty(B, H, Tn, device=DEV), torch.empty(B, H, Tn, device=DEV)
    assert lstm_sync_errors() == 0
    bufs = {}
    for rnd in range(2):
        x.copy_(torch.randn(B, H, Tn, generator=gen))
        dout.copy_(torch.randn(B, H, Tn, generator=gen))
        dx0 = torch.randn(B, H, Tn, generator=gen).to(DEV)  # what dx holds before an accumulating call
        res = []
        for persist in (0, 1):
            if persist not in bufs:
                bufs[persist] = (e(B * Tn * H), e(L * B * Tn * H), e(L * B * Tn * H), e(L * B * Tn * 4 * H),
                                 torch.empty_like(x), e(L * B * Tn * 4 * H), torch.empty_like(x),
                                 torch.empty(lib.encx_lstm_bwd_workspace(B, Tn, H, L), dtype=torch.uint8, device=DEV))
            xt, Y, Cs, Gs, out, DA, dx, ws = bufs[persist]
            dx.copy_(dx0)
            with option(LSTM_PERSIST=persist):
                call('encx_lstm_fwd', ptr(x), ptr(wcat), ptr(bsum), ptr(xt), ptr(Y), ptr(Cs), ptr(Gs), ptr(out), 1,
                     B, Tn, H, L, st)
                call('encx_lstm_bwd', ptr(dout), ptr(wcatT), ptr(Cs), ptr(Gs), ptr(DA), None if no_dx else ptr(dx),
                     acc_x, ptr(ws), B, Tn, H, L, st)
            torch.cuda.synchronize()
            res.append((DA.clone(), dx.clone()))
        assert lstm_sync_errors() == 0, (rnd, 'hand-off spins timed out or a counter ended off its count')
        (da0, dxs0), (da1, dxs1) = res
        assert torch.equal(da0, da1), (rnd, 'DA', float((da0 - da1).abs().max()))
        assert torch.equal(dxs0, dxs1), (rnd, 'dx', float((dxs0 - dxs1).abs().max()))
        if no_dx:
            assert torch.equal(dxs1, dx0), (rnd, 'dx was NULL and must stay untouched')
        else:
            assert not torch.equal(dxs1, dx0), (rnd, 'dx was not written')
