"""Both sides of option BLAS for the short-T convolutions, each against fp64 and each with proof
of the route it took.

The plain GEMMs of the im2col'd convs (csrc/conv1d.hip blas_flat_run / blas_wgrad_run) go to
hipBLASLt when their predicate holds (blas_flat_ok: 256+ rows, a reduction of 512+, 1e9+
multiply-adds; bits 4 and 8 of BLAS for T > 128), and silently to the library's own flattened
GEMM (gemm.h gemm_launch with its k-splits) when the option is off or hipBLASLt declines. The
shapes here are the smallest that cross the predicate, chosen so that the helper kernels
(im2col_kernel, gemm_epi_kernel, wg_transpose_kernel, wg_colsum_part / fin, the slab reduces)
meet ragged tiles and every chunk count blas_chunks can return (8, 6, 4, 3, 2, and the uneven cut
it makes where none of them divides the reduction).

Reference: the oracle's sconv1d / sconvtr1d (oracle/encodec_oracle.py; reference
modules/conv.py:195-252) evaluated by torch on the GPU in float64 from the same fp32 operands
(test_gpu_fullsize._fp64_layer), and the same restatement in plain float32 (MIOpen off: torch's
own im2col + GEMM, as steputil.oracle_step runs the full-size step). Error of a tensor: max |a -
ref| / max |ref|. Bound, the project's rule: within 4x the plain-fp32 restatement's error (floor
1e-6, test_lstm_vs_oracle) and below 2e-5 (test_gpu_fullsize).

Route proof: encx_blas_stats is read before and after every forward + backward. With the bit on,
`launched` rises by the GEMMs the case is meant to hand to the library and `declined` stays; with
BLAS 0 neither moves. A shape that misses its predicate, or a hipBLASLt that has no algorithm,
fails the case instead of testing the other kernel."""
import functools

import pytest
import torch

from test_gpu_fullsize import _fp64_layer, _rel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# name -> (layer, Cin, Cout, K, stride, causal, pre-ELU, B, T_in, library GEMMs under its option)
CASES = {
    # aligned baseline. fwd 256 x 7680 x 512 in KB 2 chunks; the strided bwd-data is the polyphase
    # GEMM 256 x 7744 x 512 (121 columns per item); weight grad over 7680 positions, KB 8
    'a': ('conv', 64, 256, 8, 4, True, 'elu', 64, 480, 3),
    # ragged in everything: reduction 525 (% 64 != 0); M 260 (% 32 != 0); N 7777 (odd: % 16 != 0);
    # T 77 (% 4 != 0); non-causal reflect padding. No chunk count divides 525 or 7777, where
    # blas_chunks used to return 1: one library chain over the 7777 positions of the weight grad
    # measured dweight_v 3.4e-6 against plain fp32's 4.0e-7 (8.6x) and dweight_g 1.5e-6 against
    # 2.2e-7. Now the reduction is cut unevenly, each cut two library GEMMs: forward 263 + 262,
    # weight grad 7 x 973 + 966. Its bwd-data has 75 rows: the own GEMM under either option
    'b': ('conv', 75, 260, 7, 1, False, None, 101, 77, 4),
    'c': ('conv', 96, 256, 8, 4, True, None, 44, 480, 3),   # fwd reduction 768: KB 3
    'd': ('conv', 192, 256, 8, 4, True, None, 22, 480, 3),  # fwd reduction 1536: KB 6
    # polyphase 256 x 7700 x 512, bwd-data as a forward conv of dy, weight grad over 7700
    # positions: KB 4 (7700 % 8 != 0), the transposed L with N % 32 != 0
    'e': ('convtr', 256, 64, 8, 4, True, 'elu', 77, 100, 3),
    # config 3's stride-1 k7 layer at its own shape, for the own GEMM's split path (BLAS 0 only)
    'f': ('conv', 512, 128, 7, 1, True, 'elu', 32, 75, 0),
    # T_out 160 > 128: bits 4 (fwd 512 x 7680 x 1024, 4.03e9 multiply-adds, a 31 MB im2col; the
    # polyphase bwd-data) and 8 (the weight grad)
    'big_conv': ('conv', 128, 512, 8, 4, True, 'elu', 48, 640, 3),
    'big_convtr': ('convtr', 512, 128, 8, 4, True, 'elu', 48, 160, 3),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's module, input, output grad, fp64 results and plain-fp32 errors: computed once,
    shared by every test of the case, never written again."""
    from encx.modules.conv import SConv1d, SConvTranspose1d
    kind, cin, cout, k, s, causal, act, B, T, _ = CASES[name]
    torch.manual_seed(100 + sorted(CASES).index(name))
    if kind == 'conv':
        m = SConv1d(cin, cout, k, stride=s, causal=causal, norm='weight_norm', pad_mode='reflect')
    else:
        m = SConvTranspose1d(cin, cout, k, stride=s, causal=causal, norm='weight_norm')
    # weight-norm gains away from ||v|| so the norm's scale and its grad are exercised
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, prm in m.named_parameters():
            if n.endswith('weight_g'):
                prm.mul_(0.5 + torch.rand(prm.shape, generator=g))
    m = m.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(3000 + len(name) + B)
    x = torch.randn((B, cin, T), generator=gen, device=DEV)
    ref, err32 = {}, {}
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype, copy=True).requires_grad_(True)  # (a plain .to(float32) would hand back x itself)
        with torch.backends.cudnn.flags(enabled=False):
            yr, pr = _fp64_layer(m, xr, act, dtype)
            if dtype == torch.float64:
                dy = torch.randn(yr.shape, generator=gen, device=DEV)
            yr.backward(dy.to(dtype))
        out = {'y': yr.detach(), 'dx': xr.grad}
        out.update({'d' + n.split('.')[-1]: pr['m.' + n].grad for n, _ in m.named_parameters()})
        if dtype == torch.float64:
            ref = out
        else:
            err32 = {n: _rel(v, ref[n]) for n, v in out.items()}
    assert set(ref) == {'y', 'dx', 'dweight_v', 'dweight_g', 'dbias'}, sorted(ref)
    return m, x, dy, act, ref, err32


def _run(name, **opts):
    """One forward + backward of the case's encx module under the options -> (its outputs, the
    rise of encx_blas_stats' (launched, declined) over it)."""
    from encx._lib import blas_stats, option
    m, x0, dy, act, _, _ = _case(name)
    x = x0.detach().clone().requires_grad_(True)
    for prm in m.parameters():
        prm.grad = None
    torch.cuda.synchronize()
    before = blas_stats()
    with option(**opts):
        y = m(x, act=act)
        y.backward(dy)
        torch.cuda.synchronize()
    after = blas_stats()
    out = {'y': y.detach(), 'dx': x.grad}
    out.update({'d' + n.split('.')[-1]: prm.grad for n, prm in m.named_parameters()})
    return out, (after[0] - before[0], after[1] - before[1])


def _check(name, label, want_gemms, **opts):
    _, _, _, _, ref, err32 = _case(name)
    out, moved = _run(name, **opts)
    errs = {n: _rel(v, ref[n]) for n, v in out.items()}
    print(f'{name} {label}: library GEMMs {moved[0]}, declined {moved[1]}; encx / plain fp32: ' +
          ', '.join(f'{n} {errs[n]:.1e}/{err32[n]:.1e}' for n in errs))
    assert moved == (want_gemms, 0), (f'case {name} {label}: encx_blas_stats moved by (launched, declined) = '
                                      f'{moved}, the intended route moves it by ({want_gemms}, 0)')
    bad = [(n, e, err32[n]) for n, e in errs.items() if not (e <= max(4 * err32[n], 1e-6) and e < 2e-5)]
    assert not bad, (name, label, bad)


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'e'])
def test_short_t_library_route(name):
    """BLAS at its default: the case's GEMMs run in hipBLASLt, none handed back."""
    _check(name, 'BLAS default', CASES[name][-1])


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'e', 'f'])
def test_short_t_own_gemm_route(name):
    """BLAS 0: the same layers on the flattened implicit GEMM and its k-split slabs (gemm_splits /
    gemm_slabs, conv_fwd_reduce / conv_poly_reduce) and the hand-written weight grads; the
    library is not offered anything."""
    _check(name, 'BLAS 0', 0, BLAS=0)


def test_library_route_bit_identical():
    """Case (a) twice under the default: every output bit for bit the same (the plan cache hands
    the second call the first call's algorithm, and the slabs are summed in a fixed order)."""
    first, moved1 = _run('a')
    second, moved2 = _run('a')
    assert moved1 == moved2 == (CASES['a'][-1], 0), (moved1, moved2)
    for n in first:
        assert torch.equal(first[n], second[n]), (n, float((first[n] - second[n]).abs().max()))


@pytest.mark.parametrize('name', ['big_conv', 'big_convtr'])
def test_long_t_opt_in_route(name):
    """BLAS 15: the opt-in bits 4 (forward / polyphase of a T > 128 layer through im2col +
    hipBLASLt) and 8 (its weight grad), DESIGN §4's recorded A/B, under the same bound and proof."""
    _check(name, 'BLAS 15', CASES[name][-1], BLAS=15)
