"""CPU checks of the streaming codec's per-slot lifecycle (encx/streaming.py): the pure host
validation of a step's frame counts and of restart(), and the argument validation of the two
slot-table entry points (ENCX_EINVAL before any device call)."""
import numpy as np
import pytest

MIN_FIRST, MAX_FRAMES = 7, 8


def check(started, frames):
    from encx.streaming import check_frames
    return check_frames(started, frames, MIN_FIRST, MAX_FRAMES)


def test_check_frames_accepts_and_returns_n_max_and_any_first():
    assert check([False] * 3, [7, 7, 7]) == (7, True)
    assert check([True] * 3, [1, 1, 1]) == (1, False)
    assert check([True, False, False], [1, 7, 0]) == (7, True)      # a join beside a short chunk
    assert check([True, True, False], [1, 8, 0]) == (8, False)      # a slot that never started sits out
    assert check([True, False, True], [0, 0, 3]) == (3, False)
    assert check([False], [8]) == (8, True)
    assert check([True, False], [6, 0]) == (6, False)               # below min_first, but not a first chunk
    assert check([False, True], (7, 8)) == (8, True)                # any sequence
    assert check([True, True], np.array([2, 5])) == (5, False)      # of anything that is an int


def test_check_frames_refusals():
    for started, frames in (
            ([True] * 3, [1, 1]),                # wrong length
            ([True] * 3, [1, 1, 1, 1]),
            ([True] * 2, [1, 9]),                # above max_frames
            ([True] * 2, [-1, 1]),               # below 0
            ([True, False], [1, 1]),             # a first chunk of 1..min_first_frames - 1 frames
            ([True, False], [1, 6]),
            ([False, False], [6, 6]),
            ([True, True], [0, 0]),              # nobody delivers
            ([False, False], [0, 0]),
            ([True, True], [1.0, 1]),            # not an int
            ([True], 'x')):
        with pytest.raises(ValueError):
            check(started, frames)


def test_check_restart():
    from encx.streaming import check_restart
    assert check_restart([0, 63], 64) == [0, 63]
    assert check_restart([], 2) == []
    assert check_restart((1,), 2) == [1]
    for slots, batch in (([2], 2), ([-1], 2), ([0, 64], 64), ([0.5], 2)):
        with pytest.raises(ValueError):
            check_restart(slots, batch)


def test_slot_entry_points_validate_before_any_device_call():
    """As test_stream.py does for their neighbours: NULL pointers, zero sizes and each bad shape
    -> ENCX_EINVAL (9001); the non-NULL pointers are never dereferenced."""
    from encx._lib import lib
    l = lib.load()
    p = 4096
    roll, lstm = l.encx_stream_roll_slots, l.encx_stream_lstm_slots
    assert roll(*([None] + [0] * 3 + [None, 0, None])) == 9001
    assert roll(None, 1, 4, 0, p, 1, None) == 9001     # no window table
    assert roll(p, 1, 4, 0, None, 1, None) == 9001     # no slot table
    assert roll(p, 0, 4, 0, p, 1, None) == 9001        # no windows
    assert roll(p, 1, 0, 0, p, 1, None) == 9001        # no rows
    assert roll(p, 1, 4, 0, p, 0, None) == 9001        # B outside 1..64
    assert roll(p, 1, 4, 0, p, 65, None) == 9001
    assert roll(p, 1, 4, 3, p, 1, None) == 9001        # mode outside shift / reflect / zero
    assert roll(p, 1, 4, -1, p, 1, None) == 9001
    assert lstm(*([None] * 7 + [0] * 9 + [None, None])) == 9001
    good = [p] * 7 + [1, 2, 1, 32, 2, 32, 1, 32, 1, p, None]   # skip, B, n_max, H, L, strides, slots
    for i in range(7):                                  # each NULL pointer
        assert lstm(*(good[:i] + [None] + good[i + 1:])) == 9001
    assert lstm(*(good[:16] + [None, None])) == 9001    # no slot table
    bad = lambda **kw: lstm(*[kw.get(k, v) for k, v in zip(
        ('x', 'w', 'b', 'hz', 'c', 'g', 'out', 'skip', 'B', 'n_max', 'H', 'L', 'xbs', 'xrs', 'obs', 'ors', 'slots',
         'st'), good)])
    assert bad(B=0) == 9001 and bad(B=65) == 9001       # B outside 1..64
    assert bad(n_max=0) == 9001 and bad(n_max=-1) == 9001
    assert bad(H=24, xbs=24, obs=24) == 9001            # H % 16
    assert bad(n_max=2) == 9001                         # rows shorter than n_max columns
