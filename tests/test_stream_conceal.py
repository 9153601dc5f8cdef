"""Loss concealment of the streaming decoder, the host side (encx/streaming.py): the closed-form
fade against a per-sample loop of its rule, the refusals, packet_frames. No GPU."""
import numpy as np
import pytest

from encx.streaming import (MAX_FADE, check_lost, fade_gains, fade_positions, fade_span, fade_step,
                            packet_frames)

HOP = 320


def loop(p, r, kind, samples, hold, fade, recover, M):
    """The rule, one sample at a time -> (positions after each sample, p, r)."""
    out = []
    for _ in range(samples):
        if kind == 'lost':
            r += 1
            if r > hold:
                p = max(0, p - recover)
        else:
            p = min(M, p + fade)
        out.append(p)
    if kind != 'lost' and samples:
        r = 0
    return out, p, r


def follow(schedule, hold_frames, fade_frames, recover_frames, hop=HOP):
    """Run a schedule of (kind, frames) through the closed form and the loop side by side ->
    per step (positions, p, r) of the closed form. kind: 'lost', 'ok' or 'out' (the slot sits out)."""
    M = fade_span(hold_frames, fade_frames, recover_frames, hop)
    hold = hold_frames * hop
    p = pl = M
    r = rl = 0
    steps = []
    for kind, n in schedule:
        samples = 0 if kind == 'out' else n * hop
        pos = fade_positions(p, r, kind == 'lost', samples, hold, fade_frames, recover_frames, M)
        p, r = fade_step(p, r, kind == 'lost', samples, hold, fade_frames, recover_frames, M)
        want, pl, rl = loop(pl, rl, kind, samples, hold, fade_frames, recover_frames, M)
        assert pos.dtype == np.int64 and pos.tolist() == want, (kind, n)
        assert (p, r) == (pl, rl), (kind, n)
        g = fade_gains(pos, M)
        assert g.dtype == np.float32
        inv = np.float32(1) / np.float32(M)
        assert all(g[i] == np.float32(want[i]) * inv for i in range(0, len(want), 37))
        steps.append((pos, p, r))
    return steps, M


def test_a_loss_inside_the_hold_changes_nothing():
    steps, M = follow([('ok', 7), ('lost', 1), ('lost', 1), ('ok', 3)], 2, 6, 1)
    assert all((pos == M).all() for pos, _, _ in steps)
    assert [r for _, _, r in steps] == [0, HOP, 2 * HOP, 0]


def test_the_fade_reaches_zero_and_recovers_within_a_step():
    # hold 1, fade 2, recover 1: M = 640. Four lost frames: one held, two down, the last at 0.
    steps, M = follow([('ok', 7), ('lost', 4), ('ok', 1), ('ok', 2)], 1, 2, 1)
    assert M == 2 * HOP
    pos = steps[1][0]
    assert (pos[:HOP] == M).all() and pos[HOP] == M - 1 and pos[3 * HOP - 1] == 0 and not pos[3 * HOP:].any()
    assert steps[1][1:] == (0, 4 * HOP)
    up = steps[2][0]
    assert up[0] == 2 and up[-1] == M and up[-2] == M - 2  # full level exactly at the step's end
    assert steps[2][1:] == (M, 0) and (steps[3][0] == M).all()


def test_recovery_carried_over_two_steps():
    steps, M = follow([('ok', 7), ('lost', 2), ('lost', 2), ('ok', 1), ('ok', 1), ('ok', 1)], 1, 2, 2)
    assert M == 4 * HOP
    assert steps[1][1:] == (M - 2 * HOP, 2 * HOP) and steps[2][1:] == (0, 4 * HOP)
    assert steps[3][1:] == (2 * HOP, 0) and steps[4][1:] == (M, 0) and steps[4][0][-2] == M - 2
    assert (steps[5][0] == M).all()


def test_a_slot_that_sits_out_in_mid_fade_keeps_its_state():
    steps, M = follow([('ok', 7), ('lost', 2), ('out', 3), ('lost', 1), ('out', 1), ('ok', 1), ('out', 2), ('ok', 8)],
                      1, 3, 2)
    assert steps[2][1:] == steps[1][1:] and len(steps[2][0]) == 0
    assert steps[4][1:] == steps[3][1:] and steps[6][1:] == steps[5][1:]
    assert 0 < steps[5][1] < M and steps[7][1:] == (M, 0)


def test_odd_parameters_and_a_hold_of_zero():
    follow([('ok', 7), ('lost', 1), ('ok', 1), ('lost', 3), ('lost', 8), ('ok', 2), ('lost', 1), ('ok', 8)], 0, 5, 3,
           hop=7)
    follow([('ok', 7), ('lost', 8), ('lost', 8), ('ok', 8)], 255, 255, 255, hop=3)


def test_fade_span_refusals():
    assert fade_span(2, 6, 1, 320) == 1920
    assert fade_span(0, 255, 255, 258) <= MAX_FADE
    for bad in ((-1, 6, 1), (256, 6, 1), (2, 0, 1), (2, 256, 1), (2, 6, 0), (2, 6, 256)):
        with pytest.raises(ValueError, match='conceal_'):
            fade_span(*bad, 320)
    with pytest.raises(ValueError, match='2\\^24'):
        fade_span(2, 255, 255, 259)


def test_check_lost_refusals_and_pass_through():
    started = [True, False, True]
    assert check_lost(started, [1, 7, 0], None) is None
    assert check_lost(started, [1, 7, 0], [False] * 3) is None
    assert check_lost(started, [1, 7, 0], (0, 0, 0)) is None
    assert check_lost(started, [3, 7, 0], [True, False, False], 1920) == [True, False, False]
    with pytest.raises(ValueError, match='first chunk'):
        check_lost(started, [3, 7, 0], [False, True, False])
    with pytest.raises(ValueError, match='0 frames'):
        check_lost(started, [3, 0, 0], [False, False, True])
    with pytest.raises(ValueError, match='lost for 2 slots'):
        check_lost(started, [3, 7, 0], [True, False])
    with pytest.raises(ValueError, match='sequence of bools'):
        check_lost(started, [3, 7, 0], True)
    with pytest.raises(ValueError, match='2\\^24'):
        check_lost(started, [3, 7, 0], [True, False, False], MAX_FADE + 1)
    assert check_lost(started, [3, 7, 0], [True, False, False], MAX_FADE) == [True, False, False]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """ENCX_EINVAL (9001) for a NULL pointer or a bad dimension; nothing is launched, so the
    non-NULL pointers here are never followed."""
    from encx._lib import lib
    L = lib.load()
    p = 1 << 20  # stands for a device pointer
    fill = lambda **kw: L.encx_stream_conceal_fill(*[{**dict(win=p, w_b=128 * 14, w_d=14, B=2, D=128, P=6, n=8, slots=p,
                                                              conceal=p), **kw}[k]
                                                     for k in ('win', 'w_b', 'w_d', 'B', 'D', 'P', 'n', 'slots', 'conceal')],
                                                   None)
    for kw in (dict(win=None), dict(slots=None), dict(conceal=None), dict(B=0), dict(B=65), dict(D=0), dict(P=0),
               dict(P=65), dict(n=0), dict(n=256), dict(w_d=13), dict(w_b=128 * 14 - 1)):
        assert fill(**kw) == 9001, kw
    base = dict(x=p, x_b=2560, x_c=2560, out=p, B=2, C=1, hop=320, n=8, slots=p, conceal=p, hold=2, fade=6, recover=1)
    out = lambda **kw: L.encx_stream_conceal_out(*[{**base, **kw}[k] for k in base], None)
    for kw in (dict(x=None), dict(out=None), dict(slots=None), dict(conceal=None), dict(B=0), dict(B=65), dict(C=0),
               dict(hop=0), dict(n=0), dict(n=256), dict(hold=-1), dict(hold=256), dict(fade=0), dict(fade=256),
               dict(recover=0), dict(recover=256), dict(fade=255, recover=255), dict(x_c=2559), dict(x_b=2559, C=2)):
        assert out(**kw) == 9001, kw
    base = dict(codes=p, c_b=64, c_k=8, c_t=1, packed=p, B=2, K=8, bins=1024, D=128, n=8, slots=p, nq=p, conceal=p,
                held=p, out=p, o_b=128 * 14, o_d=14, o_t=1)
    dec = lambda **kw: L.encx_stream_rvq_decode_slots_conceal(*[{**base, **kw}[k] for k in base], None)
    for kw in (dict(codes=None), dict(packed=None), dict(slots=None), dict(nq=None), dict(conceal=None),
               dict(held=None), dict(out=None), dict(B=65), dict(K=65), dict(bins=1022), dict(D=12), dict(n=0)):
        assert dec(**kw) == 9001, kw


def test_lose_is_host_bookkeeping():
    """On a model that never saw a device: with an LM the slots join `failed` and their packets
    are dropped unread until restart; a slot that failed on a bad packet still refuses; without an
    LM lose() only checks its indices."""
    import torch
    from encx.lm import LMModel
    from encx.model import EncodecModel
    from encx.streaming import StreamUnpacker
    m = EncodecModel._get_model([1.5, 24.], 24000, 1, causal=True, model_norm='weight_norm',
                                audio_normalize=False).eval()
    lm = LMModel(8, 1024, dim=64, num_heads=4, num_layers=1, past_context=5).eval()
    raw, coded = StreamUnpacker(m, 3, 8), StreamUnpacker(m, 3, 8, use_lm=True, lm=lm)
    for u in (raw, coded):
        for bad in ([3], [-1], [0.5]):
            with pytest.raises(ValueError):
                u.lose(bad)
        assert u.failed == []
    raw.lose([1])
    assert raw.failed == [] and not raw._lost
    coded.lose([1])
    assert coded.failed == [1]
    # slot 1's packet is dropped unread; it was the only one, so nothing is left to decode
    codes, frames = coded.unpack_slots([b'', bytes([3, 1, 2]), b''])
    assert frames == [0, 0, 0] and codes.shape == (3, 8, 0) and codes.dtype == torch.int64
    # beside a live slot the step goes on to the device (this model has none): the drop came first
    with pytest.raises(RuntimeError, match='no CPU fallback|on the GPU'):
        coded.unpack_slots([bytes([1, 0]), bytes([3, 1, 2]), b''])
    coded._lm.failed.add(0)  # the state a bad packet leaves: still a refusal, as before
    with pytest.raises(ValueError, match='restart'):
        coded.unpack_slots([bytes([1, 0]), bytes([3, 1, 2]), b''])
    coded.restart([0, 1])
    assert coded.failed == [] and not coded._lost
    coded.lose([2])
    coded.reset()
    assert coded.failed == [] and not coded._lost


def test_packet_frames():
    assert packet_frames(b'') == 0
    assert packet_frames(bytes([5, 1, 2, 3])) == 5
    assert packet_frames(bytearray([255])) == 255
    assert packet_frames(bytes([8, 2])) == 8  # the two-byte header's byte 0
