"""Host side of the per-slot bandwidth (n_q) of the streaming codec: the n_q check, the
variable-bandwidth packet length, and the ABI of the new entry points (declared in encx.h, bound
by encx._lib, refusing bad arguments before any launch). No GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('encx_stream_rvq_prepare', 'encx_stream_rvq_encode_slots', 'encx_stream_rvq_decode_slots',
       'encx_bitpack_slots_nq', 'encx_bitunpack_slots_nq')
EINVAL = 9001


def test_check_n_q_accepts():
    from encx.streaming import check_n_q
    assert check_n_q([7, 1, 8], [1, 3, 8], 8) == [1, 3, 8]
    assert check_n_q([1], (32,), 32) == [32]
    # a slot with 0 frames: whatever stands there is ignored, the table gets 0
    assert check_n_q([0, 2, 0, 0], [99, 2, None, 'x'], 8) == [0, 2, 0, 0]
    assert check_n_q([0, 2], [0, 8], 8) == [0, 8]
    import numpy as np
    assert check_n_q([3, 3], np.array([2, 4]), 8) == [2, 4]  # anything with __index__


@pytest.mark.parametrize('frames, n_q', [
    ([1, 1], [8]), ([1, 1], [8, 8, 8]), ([1], []),      # wrong length
    ([1, 1], [8, 2.0]), ([1, 1], ['2', 8]), ([1], [None]),  # a non-int in a delivering slot
    ([1, 1], [0, 8]), ([1, 1], [8, 9]), ([0, 1], [8, -1]),  # 0, K_max + 1, negative
    ([1, 1], 8),                                         # not a sequence
])
def test_check_n_q_refuses(frames, n_q):
    from encx.streaming import check_n_q
    with pytest.raises(ValueError):
        check_n_q(frames, n_q, 8)


def test_only_steps_with_n_q_depend_on_the_fused_quantizers_shapes():
    """The fused quantizer takes bins % 4 == 0 and D % 8 == 0 (8..256), up to 64 codebooks; the
    per-layer kernels take any bins and D <= 256. The rule is host arithmetic, and it refuses a
    step that passes n_q (NotImplementedError), never the construction of a session."""
    from encx.ops import stream_rvq_supports
    from encx.streaming import check_rvq_shape
    for ok in ((8, 1024, 128), (1, 4, 8), (64, 1 << 20, 256), (32, 1024, 128), (2, 1000, 64)):
        assert stream_rvq_supports(*ok), ok
        check_rvq_shape(*ok)
    for bad in ((8, 1001, 128), (8, 1022, 128), (8, 1024, 100), (8, 1024, 132), (8, 1024, 264), (8, 1024, 4),
                (65, 1024, 128), (0, 1024, 128), (8, 0, 128), (8, (1 << 20) + 4, 128)):
        assert not stream_rvq_supports(*bad), bad
        with pytest.raises(NotImplementedError, match='per-slot n_q'):
            check_rvq_shape(*bad)


def test_packet_bytes_nq_by_hand():
    from encx.streaming import packet_bytes_nq, packet_bytes
    # 2 header bytes + ceil(n K bits / 8)
    assert packet_bytes_nq(1, 1, 10) == 2 + 2      # 10 bits
    assert packet_bytes_nq(1, 8, 10) == 2 + 10     # 80 bits
    assert packet_bytes_nq(7, 3, 10) == 2 + 27     # 210 bits -> 26.25
    assert packet_bytes_nq(8, 32, 10) == 2 + 320
    assert packet_bytes_nq(255, 64, 10) == 2 + 20400
    assert packet_bytes_nq(3, 5, 7) == 2 + 14      # 105 bits -> 13.125
    for n, K, bits in ((1, 1, 10), (5, 3, 10), (8, 32, 10), (3, 5, 7)):
        assert packet_bytes_nq(n, K, bits) == packet_bytes(n, K, bits) + 1


def test_new_entry_points_declared_and_bound():
    from encx._lib import parse_header, lib, LIB_PATH
    sigs = parse_header()
    src = open(os.path.join(ROOT, 'include', 'encx.h')).read()
    declared = set(re.findall(r'\b(encx_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    for name in NEW:
        assert name in declared and name in sigs and name in lib.sigs, name
        res, args = lib.sigs[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p  # int f(..., encx_stream_t)
    assert len(sigs['encx_stream_rvq_encode_slots'][1]) == 19
    assert len(sigs['encx_stream_rvq_decode_slots'][1]) == 17
    assert len(sigs['encx_bitpack_slots_nq'][1]) == len(sigs['encx_bitpack_slots'][1]) + 1
    assert len(sigs['encx_bitunpack_slots_nq'][1]) == len(sigs['encx_bitunpack_slots'][1]) + 1
    assert 'VARIABLE-BANDWIDTH PACKET' in src
    assert os.path.exists(LIB_PATH), 'build first: __graft_entry__.build()'
    cdll = ctypes.CDLL(LIB_PATH)
    assert not [n for n in NEW if not hasattr(cdll, n)]


def test_new_entry_points_refuse_before_any_launch():
    """NULL pointers and out-of-range sizes are ENCX_EINVAL; nothing is launched (no device is
    touched: the pointers below are never dereferenced)."""
    from encx._lib import lib
    L = lib.load()
    p = 4096  # a non-NULL pointer value that is never followed
    ok = dict(B=2, K=8, bins=1024, D=128, n=7)

    def enc(x=p, E=p, ET=p, ee=p, slots=p, nq=p, codes=p, **kw):
        d = dict(ok, **kw)
        return L.encx_stream_rvq_encode_slots(x, 128 * 8, 8, 1, E, ET, ee, d['B'], d['K'], d['bins'], d['D'], d['n'],
                                              slots, nq, codes, 8 * 7, 7, 1, None)

    def dec(codes=p, E=p, slots=p, nq=p, out=p, **kw):
        d = dict(ok, **kw)
        return L.encx_stream_rvq_decode_slots(codes, 56, 7, 1, E, d['B'], d['K'], d['bins'], d['D'], d['n'], slots,
                                              nq, out, 1024, 8, 1, None)

    for f, ptrs in ((enc, ('x', 'E', 'ET', 'ee', 'slots', 'nq', 'codes')), (dec, ('codes', 'E', 'slots', 'nq', 'out'))):
        for name in ptrs:
            assert f(**{name: None}) == EINVAL, (f.__name__, name)
        for bad in (dict(B=0), dict(B=65), dict(K=0), dict(K=65), dict(bins=0), dict(bins=1022), dict(D=0),
                    dict(D=132), dict(D=264), dict(n=0), dict(n=256)):
            assert f(**bad) == EINVAL, (f.__name__, bad)

    def prep(embed=p, E=p, ET=p, ee=p, k=0, K=8, bins=1024, D=128):
        return L.encx_stream_rvq_prepare(embed, k, K, bins, D, E, ET, ee, None)
    for name in ('embed', 'E', 'ET', 'ee'):
        assert prep(**{name: None}) == EINVAL, name
    for bad in (dict(k=-1), dict(k=8), dict(K=0), dict(K=65), dict(bins=6), dict(D=4)):
        assert prep(**bad) == EINVAL, bad

    def pack(codes=p, slots=p, nq=p, out=p, nbytes=p, err=p, B=2, K=8, n=7, bits=10, stride=2 + 70):
        return L.encx_bitpack_slots_nq(codes, 56, 7, 1, B, K, n, bits, slots, nq, out, stride, nbytes, err, None)

    def unpack(data=p, slots=p, nq=p, codes=p, B=2, K=8, n=7, bits=10, stride=70):
        return L.encx_bitunpack_slots_nq(data, stride, B, K, n, bits, slots, nq, codes, 56, 7, 1, None)

    for name in ('codes', 'slots', 'nq', 'out', 'nbytes', 'err'):
        assert pack(**{name: None}) == EINVAL, name
    for name in ('data', 'slots', 'nq', 'codes'):
        assert unpack(**{name: None}) == EINVAL, name
    for bad in (dict(B=0), dict(B=65), dict(K=0), dict(K=65), dict(n=0), dict(n=256), dict(bits=0), dict(bits=33)):
        assert pack(**bad) == EINVAL and unpack(**bad) == EINVAL, bad
    assert pack(stride=2 + 69) == EINVAL    # the two header bytes count
    assert unpack(stride=69) == EINVAL
