"""The register-window weight grad of the strided Conv2d (c2_wgrad_rw_kernel,
csrc/conv2d_wgrad.hip), at the smallest shapes that reach each of its paths: interior items (no fix-up, loads at a scalar
base), row-edge chunks, kt rows outside the input, partial channel tiles, the tensor's first and
last quads, odd tails of the two-stage item loop and splits with fewer items than waves; with and
without the LeakyReLU' mask, in the 8-wave workgroup form and the one-wave form. Weight and bias
grads against torch.nn.functional.conv2d in fp64 under the bounds of
test_gpu_disc.test_conv2d_vs_torch_fp64, and bit-identical from run to run."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# kernel, stride, dilation, padding of the layers the kernel serves (msstftd.py:67-84)
D1 = ((3, 9), (1, 2), (1, 1), (1, 4))
D2 = ((3, 9), (1, 2), (2, 1), (2, 4))
D4 = ((3, 9), (1, 2), (4, 1), (4, 4))
K3 = ((3, 3), (1, 1), (1, 1), (1, 1))

# name: (layer, Ci, Co, B, T2, F_in, act)
CASES = {
    # F_in 65 -> F_out 33: 5 chunks, the last partial, the first and the fourth at a row edge
    'd1_f65': (D1, 32, 32, 2, 5, 65, True),
    'd2_f65': (D2, 32, 32, 2, 5, 65, True),
    'd4_f65_t9': (D4, 32, 32, 2, 9, 65, True),      # kt 0 / 2 rows inside for some t only
    'd4_f65_t3': (D4, 32, 32, 2, 3, 65, True),      # every kt != 1 row outside for every t
    'k3_f33': (K3, 32, 32, 2, 5, 33, True),
    # F_in 9 -> F_out 5: one partial chunk, both halves at an edge; B 1: the tensor's first and last
    # quads belong to the first and the last item, and the splits have fewer items than waves
    'd1_f9': (D1, 32, 32, 2, 3, 9, True),
    'd1_f9_b1': (D1, 32, 32, 1, 3, 9, True),
    'd4_f9_b1': (D4, 32, 32, 1, 3, 9, True),
    'k3_f9_b1': (K3, 32, 32, 1, 3, 9, True),
    'd1_f65_b1': (D1, 32, 32, 1, 5, 65, True),
    'd1_f9_t2': (D1, 32, 32, 2, 2, 9, True),        # planes too small for the scalar-base loads
    'k3_f9_t1_b1': (K3, 32, 32, 1, 1, 9, True),
    # the middle chunks of the interior rows are interior items only
    'd1_f129_t12': (D1, 32, 32, 2, 12, 129, True),
    'k3_f65_t12': (K3, 32, 32, 2, 12, 65, True),
    # channels below the 32 x 32 tile
    'd1_ci16': (D1, 16, 32, 2, 5, 65, True),
    'd2_ci48': (D2, 48, 32, 2, 5, 65, True),
    'd1_co8': (D1, 32, 8, 2, 5, 65, True),
    'k3_ci48_co8': (K3, 48, 8, 2, 5, 33, True),
    # no LeakyReLU' mask
    'd1_f65_noact': (D1, 32, 32, 2, 5, 65, False),
    'k3_f33_noact': (K3, 32, 32, 2, 5, 33, False),
    'd1_f129_t12_noact': (D1, 32, 32, 2, 12, 129, False),
}


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(autouse=True)
def regwin_family():
    from encx._lib import lib
    prev = lib.encx_conv2d_select(1)
    yield
    lib.encx_conv2d_select(prev)


@functools.lru_cache(maxsize=None)
def problem(name):
    """Inputs in fp64 (shared by every run of the case, never modified)."""
    import torch.nn.functional as F
    (k, s, d, pad), Ci, Co, B, T2, Fi, act = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x64 = torch.randn(B, Ci, T2, Fi, generator=g, dtype=torch.float64).requires_grad_(True)
    v64 = (0.2 * torch.randn((Co, Ci) + k, generator=g, dtype=torch.float64)).requires_grad_(True)
    b64 = (0.1 * torch.randn(Co, generator=g, dtype=torch.float64)).requires_grad_(True)
    p64 = F.conv2d(x64, v64, b64, stride=s, dilation=d, padding=pad)  # pre-activation
    dy64 = torch.randn(p64.shape, generator=g, dtype=torch.float64)
    return x64, v64, b64, p64, dy64


def run(name):
    from encx import ops
    (k, s, d, pad), Ci, Co, B, T2, Fi, act = CASES[name]
    x64, v64, b64, p64, dy64 = problem(name)
    x = x64.detach().float().to(DEV).requires_grad_(True)
    v = v64.detach().float().to(DEV).requires_grad_(True)
    b = b64.detach().float().to(DEV).requires_grad_(True)
    y = ops.conv2d(x, v, None, b, k, s, d, pad, act)
    y.backward(dy64.float().to(DEV))
    return y.detach(), v.grad, b.grad


def check(name, wgs):
    from encx._lib import set_option
    prev = set_option('WGR_WGS', wgs) if wgs is not None else None
    try:
        y, gv, gb = run(name)
        _, gv2, gb2 = run(name)
    finally:
        if prev is not None:
            set_option('WGR_WGS', prev)
    assert torch.equal(gv, gv2) and torch.equal(gb, gb2)
    act = CASES[name][-1]
    x64, v64, b64, p64, dy64 = problem(name)
    # the reference grads use OUR LeakyReLU' mask (test_conv2d_vs_torch_fp64: the fp32
    # pre-activation may take the other sign than fp64's only within fp32 rounding of 0)
    mask = 1.0
    if act:
        mine = y.double().cpu() > 0
        flips = mine != (p64.detach() > 0)
        assert bool((p64.detach().abs()[flips] <= 1e-5 * float(p64.detach().abs().max())).all())
        mask = torch.where(mine, 1.0, 0.2).double()
    dyl = dy64 * mask
    gv64, gb64 = torch.autograd.grad(p64, (v64, b64), dyl, retain_graph=True)
    rv, rb = rel(gv, gv64), rel(gb, gb64)
    bscale = float(dyl.abs().sum(dim=(0, 2, 3)).max())
    berr = float((gb.double().cpu() - gb64).abs().max())
    print(f'{name} wgs {wgs}: dw rel {rv:.2e}, db rel {rb:.2e}, db err {berr:.2e} (scale {bscale:.2e})')
    assert rv < 1e-5, rv
    assert rb < 1e-5 or berr <= 1e-7 * bscale, (rb, berr, bscale)


@pytest.mark.parametrize('wgs', [None, 0], ids=['wg8', 'wave1'])
@pytest.mark.parametrize('name', list(CASES))
def test_wgrad_rw_vs_torch_fp64(name, wgs):
    """Each case in the 8-wave workgroup form (WGR_WGS at its default) and the one-wave form."""
    check(name, wgs)


# few workgroups: per_split is no multiple of 16 (an odd tail in the two-stage loop of the 8
# waves): d1_f129_t12 has 216 items in 1 (WGS 3) or 2 (WGS 7) splits, k3_f33 50 items in 3 or 7
@pytest.mark.parametrize('wgs', [3, 7])
@pytest.mark.parametrize('name', ['d1_f129_t12', 'd4_f65_t9', 'k3_f33', 'd1_f9_b1', 'd1_f129_t12_noact'])
def test_wgrad_rw_odd_tails(name, wgs):
    check(name, wgs)
