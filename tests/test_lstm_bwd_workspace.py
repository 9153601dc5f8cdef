"""encx_lstm_bwd_workspace (a host-only query, no device): shapes the persistent backward admits
count its split-exchange ring behind the input-grad tiles; shapes it does not admit keep the step
form's size."""
import pytest


def _ws(B, T, H, L):
    from encx._lib import lib
    return lib.encx_lstm_bwd_workspace(B, T, H, L)


def _step_floats(B, H, L):
    groups = H // 4  # k-splits of the step GEMM: <= 4, dividing the groups, >= 8 groups each
    ns = max(1, min(4, groups // 8))
    while groups % ns:
        ns -= 1
    return L * B * H + L * ns * B * 2 * H + (L + 1) * (H // 16)


@pytest.mark.parametrize('B,H,T,L', [(1, 128, 1, 1), (2, 128, 2, 2), (16, 384, 3, 1), (20, 256, 9, 3), (32, 512, 4, 2),
                                     (32, 512, 75, 2)])
def test_persistent_shapes_count_the_ring(B, H, T, L):
    nwg = L * -(-B // 16) * (H // 8)           # 4 K-splits of every 64-column tile
    ring = 2 * nwg * 16 * 64 * 4               # two [16][64] fp32 slots per workgroup
    xp = max(L - 1, 1) * B * T * H * 4
    assert _ws(B, T, H, L) >= xp + ring
    assert _ws(B, T, H, L) == max(xp + ring, _step_floats(B, H, L) * 4)


@pytest.mark.parametrize('B,H,T,L', [(4, 64, 5, 2), (32, 1024, 3, 1), (8, 192, 7, 2), (3, 16, 2, 1)])
def test_step_only_shapes_keep_their_size(B, H, T, L):
    """H % 128 != 0 or H > 512: only the step form runs; the size is what it was (the larger of the
    step form's buffers and the persistent form's input-grad tiles)."""
    assert _ws(B, T, H, L) == max(_step_floats(B, H, L), max(L - 1, 1) * B * T * H) * 4
