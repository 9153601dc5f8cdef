"""The hand-over from item to item in the persistent register-window Conv2d forward and
backward-data kernels (c2_fwd_rw_kernel, c2_dgrad_rw_kernel): the small shapes of test_gpu_disc
give a wave at most one item, so the next-item window prefetch and the first item's window load
ahead of the quad-staged weight copy never met a second item there, nor the feature-code epilogue's
clamped loads at row edges a ragged last tile.
Here options FWR / DGR shrink the launch to 1 and 2 workgroups, so every wave of the one-workgroup
launch takes 3 or more items in turn (2 or more at two workgroups: the shapes have 18 to 49 items
and a workgroup 8 waves) -- computed below by the planner's formula and asserted. The forward
output and the backward-data dx are checked against torch.nn.functional.conv2d in fp64 on the CPU
under the bound of test_gpu_disc.test_conv2d_vs_torch_fp64 (1e-5 of the tensor's largest
magnitude), and bit for bit against the same call at the default FWR / DGR: who computes an item
must not change a bit. Backward-data runs in every epilogue combination of the training step:
plain, LeakyReLU'(x) mask, feature term from the two float maps or from the 1-byte code, each
accumulating or not, with and without the LeakyReLU'(y) mask (premasked dy); the code epilogue
must equal the float one bit for bit (test_gpu_disc.test_feat_code_epilogue_bit_identical)."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NWV = 8  # waves per workgroup of both kernels

# (Ci, Co, kernel, stride, dilation, padding): the DiscriminatorSTFT layers (msstftd.py:67-84)
LAYERS = {
    'first': (2, 32, (3, 9), (1, 1), (1, 1), (1, 4)),
    'd1': (32, 32, (3, 9), (1, 2), (1, 1), (1, 4)),
    'd2': (32, 32, (3, 9), (1, 2), (2, 1), (2, 4)),
    'd4': (32, 32, (3, 9), (1, 2), (4, 1), (4, 4)),
    'k3': (32, 32, (3, 3), (1, 1), (1, 1), (1, 1)),
}
# (B, T2, Fi): 26 tiles of the stride-2 layers on 8 waves; a ragged last tile and partial f edges
SHAPES = [(4, 23, 65), (3, 11, 129), (5, 23, 33)]
WGS = [(1, 3), (2, 2)]  # (workgroups, items the busiest wave must at least take)


def cdiv(a, b):
    return -(-a // b)


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def lrelu_grad(t):
    return torch.where(t > 0, 1.0, 0.2).double()


def items_per_wave(items, wgs):
    """Items of the busiest wave (run_fwd_rw / run_dgrad_rw: grid = min(wgs, ceil(items / 8)), item j
    of a round to wave j / grid of workgroup j % grid)."""
    grid = min(wgs, cdiv(items, NWV))
    return cdiv(items, grid * NWV)


@pytest.fixture(autouse=True)
def regwin_family():
    from encx._lib import lib
    prev = lib.encx_conv2d_select(1)
    yield
    lib.encx_conv2d_select(prev)


@functools.lru_cache(maxsize=None)
def problem(layer, shape):
    """Inputs and fp64 references (shared by every run of the case, never modified): the forward
    pre-activation, and the plain input grad of dy with and without the LeakyReLU'(y) mask, y being
    a given map (no sign flips to allow for)."""
    import torch.nn.functional as F
    Ci, Co, k, s, d, pad = LAYERS[layer]
    B, T2, Fi = shape
    g = torch.Generator().manual_seed(sum(map(ord, layer)) * 1000 + B * 100 + Fi)
    x = torch.randn(B, Ci, T2, Fi, generator=g)
    v = 0.2 * torch.randn((Co, Ci) + k, generator=g)
    b = 0.1 * torch.randn(Co, generator=g)
    x64 = x.double().requires_grad_(True)
    p64 = F.conv2d(x64, v.double(), b.double(), stride=s, dilation=d, padding=pad)
    dy = torch.randn(p64.shape, generator=g)
    y = torch.randn(p64.shape, generator=g)
    fr = x + 0.3 * torch.randn(x.shape, generator=g)
    fr.view(-1)[::97] = x.view(-1)[::97]  # ties: sign 0
    dx0 = torch.randn(x.shape, generator=g)
    den = torch.rand(1, generator=g) + 0.5
    fg = torch.rand(1, generator=g) + 0.5
    gx = {ym: torch.autograd.grad(p64, x64, dy.double() * (lrelu_grad(y) if ym else 1.0), retain_graph=True)[0]
          for ym in (False, True)}
    return dict(x=x, v=v, b=b, p64=p64.detach(), dy=dy, y=y, fr=fr, dx0=dx0, den=den, fg=fg, gx=gx)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'b%d_t%d_f%d' % s)
@pytest.mark.parametrize('layer', list(LAYERS))
def test_forward_items(layer, shape):
    import torch.nn.functional as F
    from encx import ops
    from encx._lib import call, ptr, stream, get_option, set_option
    Ci, Co, k, s, d, pad = LAYERS[layer]
    B, T2, Fi = shape
    KT, KF, sf, dt, pt, pf, Fo = ops.conv2d_geometry(Fi, k, s, d, pad)
    items = cdiv(B * T2 * cdiv(Fo, 4), 32)
    P = problem(layer, shape)
    x, b = P['x'].to(DEV), P['b'].to(DEV)
    wf = P['v'].permute(1, 2, 3, 0).contiguous().view(-1).to(DEV)  # [(ci,kt)][kf][co]
    want = F.leaky_relu(P['p64'], 0.2)

    def run():
        y = torch.empty(B, Co, T2, Fo, device=DEV)
        call('encx_conv2d_fwd', ptr(x), ptr(wf), ptr(b), ptr(y), B, Ci, T2, Fi, Co, Fo, KT, KF, sf, dt, pt, pf, 1,
             stream())
        return y

    base = run()
    assert rel(base, want) < 1e-5, rel(base, want)
    default = get_option('FWR')
    try:
        for wgs, least in WGS:
            assert items_per_wave(items, wgs) >= least, (items, wgs)
            set_option('FWR', wgs)
            y = run()
            print(f'{layer} {shape} FWR {wgs}: {items} items, {items_per_wave(items, wgs)} on the busiest wave, '
                  f'rel {rel(y, want):.2e}')
            assert rel(y, want) < 1e-5, rel(y, want)
            assert torch.equal(y, base), (wgs, float((y - base).abs().max()))
    finally:
        set_option('FWR', default)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'b%d_t%d_f%d' % s)
@pytest.mark.parametrize('layer', ['d1', 'd2', 'd4', 'k3'])
def test_bwd_data_items(layer, shape):
    from encx import ops
    from encx._lib import lib, call, ptr, stream, get_option, set_option
    Ci, Co, k, s, d, pad = LAYERS[layer]
    B, T2, Fi = shape
    KT, KF, sf, dt, pt, pf, Fo = ops.conv2d_geometry(Fi, k, s, d, pad)
    U = (Fi - 1 + pf) // sf + 1
    items = cdiv(B * T2 * cdiv(U, 4), 32)
    P = problem(layer, shape)
    x, dy, y, fr, dx0, den, fg = (P[n].to(DEV) for n in ('x', 'dy', 'y', 'fr', 'dx0', 'den', 'fg'))
    wf = P['v'].permute(1, 2, 3, 0).contiguous().view(-1).to(DEV)
    wp = ops._wpoly(wf, Co, Ci, KT, KF, sf, x)
    dims = (B, Ci, T2, Fi, Co, Fo, KT, KF, sf, dt, pt, pf)
    n = x.numel()
    code = torch.empty(n, device=DEV, dtype=torch.uint8)
    outs, dens = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ws = torch.empty(lib.encx_disc_loss_workspace() // 4, device=DEV)
    call('encx_feat_loss_code', ptr(fr), ptr(x), n, 3.0, ptr(outs), ptr(dens), 0, ptr(ws), ptr(code), stream())
    fc = float(P['fg'].double() * 3.0 / P['den'].double())
    sign = torch.sign(P['x'].double() - P['fr'].double())

    def run(ym, xm, feat, acc):
        dx = dx0.clone()
        if feat is None:
            call('encx_conv2d_bwd_data', ptr(dy), ptr(y if ym else None), ptr(wp), ptr(x if xm else None), ptr(dx),
                 acc, *dims, stream())
        else:
            call('encx_conv2d_bwd_data_feat', ptr(dy), ptr(y if ym else None), ptr(wp), ptr(x if xm else None),
                 ptr(dx), acc, ptr(fr), ptr(x), ptr(den), ptr(fg), 3.0, ptr(code if feat == 'code' else None), *dims,
                 stream())
        return dx

    def want(ym, xm, feat, acc):
        u = P['gx'][ym]
        if feat is not None:
            u = u + fc * sign
        if xm:
            u = u * lrelu_grad(P['x'])
        return P['dx0'].double() + u if acc else u

    combos = list(itertools.product((False, True), (False, True), (None, 'float', 'code'), (0, 1)))
    base = {c: run(*c) for c in combos}
    for c in combos:
        assert rel(base[c], want(*c)) < 1e-5, (c, rel(base[c], want(*c)))
    default = get_option('DGR')
    try:
        for wgs, least in WGS:
            assert items_per_wave(items, wgs) >= least, (items, wgs)
            set_option('DGR', wgs)
            worst = 0.0
            for c in combos:
                dx = run(*c)
                worst = max(worst, rel(dx, want(*c)))
                assert rel(dx, want(*c)) < 1e-5, (wgs, c, rel(dx, want(*c)))
                assert torch.equal(dx, base[c]), (wgs, c, float((dx - base[c]).abs().max()))
                if c[2] == 'code':  # the 1-byte code against both float maps
                    other = run(c[0], c[1], 'float', c[3])
                    assert torch.equal(dx, other), (wgs, c, float((dx - other).abs().max()))
            print(f'{layer} {shape} DGR {wgs}: {items} items, {items_per_wave(items, wgs)} on the busiest wave, '
                  f'worst rel {worst:.2e} over {len(combos)} epilogue combinations')
    finally:
        set_option('DGR', default)
