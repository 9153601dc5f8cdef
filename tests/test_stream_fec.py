"""Host side of the redundant packets (in-band FEC) and the key packets of the streaming codec:
the packet length, the fec check, every constructor and header refusal on a model that never saw a
device, the ABI of encx_bitpack_slots_fec (declared in encx.h, bound by encx._lib, refusing bad
arguments before any launch) and the choices of StreamReceiver with stub sessions. No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 9001
B, K, BITS, MAXF, R = 3, 8, 10, 8, 2


@pytest.fixture(scope='module')
def model():
    from encx.model import EncodecModel
    m = EncodecModel._get_model([1.5, 24.], 24000, 1, causal=True, model_norm='weight_norm', audio_normalize=False)
    assert m.bits_per_codebook == BITS
    return m.eval()


@pytest.fixture(scope='module')
def lm():
    from encx.lm import LMModel
    return LMModel(K, 1024, dim=64, num_heads=4, num_layers=1, past_context=5).eval()


def test_packet_bytes_fec_by_hand():
    from encx.streaming import packet_bytes_fec, packet_bytes_nq
    assert packet_bytes_fec(1, 1, 0, 0, 10) == 4 + 2
    assert packet_bytes_fec(7, 3, 1, 1, 10) == 4 + 27 + 2      # 210 bits -> 26.25, then 10 bits on a byte boundary
    assert packet_bytes_fec(8, 32, 8, 2, 10) == 4 + 320 + 20
    assert packet_bytes_fec(3, 5, 2, 3, 7) == 4 + 14 + 6       # 105 and 42 bits
    for n, k, bits in ((1, 1, 10), (5, 3, 10), (8, 32, 10), (3, 5, 7)):
        # without a copy: the variable-bandwidth packet and two more header bytes
        assert packet_bytes_fec(n, k, 0, 0, bits) == packet_bytes_nq(n, k, bits) + 2


def test_check_fec_accepts():
    from encx.slots import check_fec
    import encx.streaming
    assert encx.streaming.check_fec is check_fec
    assert check_fec([7, 1, 8], [0, 1, 2], 2) == [0, 1, 2]
    assert check_fec([7, 0, 8], None, 2) == [2, 0, 2]          # None: the most everywhere a packet goes
    assert check_fec([1], (32,), 32) == [32]
    # a slot with 0 frames: whatever stands there is ignored
    assert check_fec([0, 2, 0, 0], [99, 2, None, 'x'], 2) == [0, 2, 0, 0]
    import numpy as np
    assert check_fec([3, 3], np.array([2, 0]), 2) == [2, 0]    # anything with __index__


@pytest.mark.parametrize('frames, fec', [
    ([1, 1], [2]), ([1, 1], [2, 2, 2]), ([1], []),          # wrong length
    ([1, 1], [2, 1.0]), ([1, 1], ['1', 2]), ([1], [None]),  # a non-int in a delivering slot
    ([1, 1], [3, 2]), ([0, 1], [2, -1]),                    # R + 1, negative
    ([1, 1], 2),                                            # not a sequence
])
def test_check_fec_refuses(frames, fec):
    from encx.slots import check_fec
    with pytest.raises(ValueError):
        check_fec(frames, fec, 2)


def test_constructor_refusals(model, lm):
    from encx.streaming import StreamPacker, StreamUnpacker
    for cls in (StreamPacker, StreamUnpacker):
        with pytest.raises(ValueError, match='slot_n_q'):
            cls(model, B, K, fec=R)                                    # fec without slot_n_q
        for bad in (0, K + 1, -1):
            with pytest.raises(ValueError):
                cls(model, B, K, slot_n_q=True, fec=bad)
        with pytest.raises((ValueError, TypeError)):
            cls(model, B, K, slot_n_q=True, fec=1.5)
        for kw in (dict(), dict(lm_format=2)):
            with pytest.raises(NotImplementedError, match='LM'):
                cls(model, B, K, use_lm=True, lm=lm, fec=R, **kw)
        for ok in (1, K):
            assert cls(model, B, K, slot_n_q=True, fec=ok).fec == ok
        assert cls(model, B, K, slot_n_q=True).fec is None
    # key packets exist in packet format 2 only
    for kw in (dict(), dict(slot_n_q=True), dict(use_lm=True, lm=lm), dict(use_lm=True, lm=lm, lm_format=1)):
        with pytest.raises(ValueError, match='key'):
            StreamPacker(model, B, K, key_interval=3, **kw)
    for bad in (0, -2):
        with pytest.raises(ValueError, match='key_interval'):
            StreamPacker(model, B, K, use_lm=True, lm=lm, lm_format=2, key_interval=bad)
    assert StreamPacker(model, B, K, use_lm=True, lm=lm, lm_format=2, key_interval=1).key_interval == 1
    with pytest.raises(TypeError):
        StreamUnpacker(model, B, K, use_lm=True, lm=lm, lm_format=2, key_interval=3)   # a sender's argument


def test_pack_refusals_are_host_only(model, lm):
    """The model is on the CPU: a call that passed its host checks raises RuntimeError (no CPU
    fallback), so ValueError shows the refusal came first."""
    from encx.streaming import StreamPacker
    codes = torch.zeros(B, K, MAXF, dtype=torch.int64)
    frames, nq = (1, 8, 0), (8, 3, 0)
    p = StreamPacker(model, B, K, slot_n_q=True, fec=R)
    for bad in ([1, 1], [1, 1, 1, 1], [3, 0, 0], [0, -1, 0], [1.0, 1, 1], 2):
        with pytest.raises(ValueError, match='fec'):
            p.pack_slots(codes, frames, nq, fec=bad)
    with pytest.raises(ValueError):
        p.pack_slots(codes, frames)                                    # fec needs n_q too
    with pytest.raises(ValueError, match='key'):
        p.pack_slots(codes, frames, nq, key=[True, False, False])      # a raw packet has no key bit
    for ok in (None, [2, 0, 'idle'], [0, 0, 0]):
        with pytest.raises(RuntimeError, match='no CPU fallback'):     # valid: reaches the device check
            p.pack_slots(codes, frames, nq, fec=ok)
    assert p._prev == [(0, 0)] * B and p._par == [0] * B and p._dev is None
    with pytest.raises(ValueError, match='fec'):
        StreamPacker(model, B, K, slot_n_q=True).pack_slots(codes, frames, nq, fec=[1, 1, 1])
    # key with format 1, and a key list of the wrong shape with format 2
    with pytest.raises(ValueError, match='key'):
        StreamPacker(model, B, K, use_lm=True, lm=lm).pack_slots(codes, frames, key=[True] * B)
    p2 = StreamPacker(model, B, K, use_lm=True, lm=lm, lm_format=2)
    for bad in ([True], [True] * 4, 1):
        with pytest.raises(ValueError, match='key'):
            p2.pack_slots(codes, frames, nq, key=bad)
    assert p2._lm.started == [False] * B and not p2._owed


def fec_packet(n, k, n_r, k_r, extra=0):
    from encx.streaming import packet_bytes_fec
    return bytes([n, k, n_r, k_r]) + bytes(packet_bytes_fec(n, k, n_r, k_r, BITS) - 4 + extra)


def test_unpack_header_refusals_are_host_only(model):
    from encx.streaming import StreamUnpacker
    u = StreamUnpacker(model, B, K, slot_n_q=True, fec=R)
    good = fec_packet(7, 3, 1, 1)
    assert len(good) == 4 + 27 + 2
    for packets in ([good] * 2, [good] * 4,                          # wrong length
                    [b'', b'', b''],                                  # nobody delivers
                    [good, 'abc', b''], [good, None, b''],
                    [good[:3], b'', b''],                             # no header
                    [good[:-1], b'', b''], [good + b'\0', b'', b''],  # length != packet_bytes_fec
                    [fec_packet(7, 3, 1, 1)[:31], b'', b''],          # the main section alone
                    [fec_packet(0, 3, 0, 0), b'', b''],               # n 0
                    [fec_packet(9, 3, 0, 0), b'', b''],               # n above max_frames
                    [fec_packet(7, 3, 9, 1), b'', b''],               # n_r above max_frames
                    [fec_packet(7, 0, 0, 0), b'', b''],               # K 0
                    [fec_packet(7, 9, 0, 0), b'', b''],               # K above the session's n_q
                    [fec_packet(7, 3, 1, 9), b'', b''],               # K_r above the session's n_q
                    [bytes([7, 3, 1, 0]) + bytes(27), b'', b''],      # K_r 0 but n_r 1
                    [bytes([7, 3, 0, 1]) + bytes(27), b'', b'']):     # n_r 0 but K_r 1
        with pytest.raises(ValueError):
            u.unpack_slots(packets)
        with pytest.raises(ValueError):
            u.unpack_slots(packets, recover=[True, False, False])
    for bad in ([True], [True] * 4, 1):
        with pytest.raises(ValueError, match='recover'):
            u.unpack_slots([good, b'', b''], recover=bad)
    for recover in (None, [True, False, False]):
        with pytest.raises(RuntimeError, match='on the GPU'):         # valid: reaches the device check
            u.unpack_slots([good, fec_packet(8, 8, 8, 2), b''], recover)
    # a copy that no packet carries: (0, 0) and zero codes, with no device call at all
    codes, frames, nq = u.unpack_slots([fec_packet(7, 3, 0, 0), b'', b''], recover=[True, False, False])
    assert frames == [0, 0, 0] and nq == [0, 0, 0] and codes.shape == (B, K, 0) and u._dev is None
    with pytest.raises(ValueError, match='recover'):
        StreamUnpacker(model, B, K, slot_n_q=True).unpack_slots([bytes([1, 1, 0, 0]), b'', b''], recover=[False] * B)


def test_the_key_bit_is_masked_before_the_k_check(model, lm):
    from encx.streaming import StreamUnpacker, KEY_BIT
    u = StreamUnpacker(model, B, K, use_lm=True, lm=lm, lm_format=2)
    assert KEY_BIT == 0x80
    assert u._headers([bytes([3, 5 | KEY_BIT, 1, 2]), bytes([1, K]), b'']) == ([3, 1, 0], [5, K, 0])
    assert u._key_slots([bytes([3, 5 | KEY_BIT, 1, 2]), bytes([1, K]), b'']) == [0]
    for bad in (bytes([3, KEY_BIT]), bytes([3, (K + 1) | KEY_BIT])):   # K 0 and K_max + 1 under the bit
        with pytest.raises(ValueError):
            u._headers([bad, b'', b''])
    # format 1 has no spare bit: byte 1 is payload there, and the raw two-byte header has no key bit
    assert StreamUnpacker(model, B, K, use_lm=True, lm=lm)._key_slots([bytes([3, 0xff]), b'', b'']) == []
    raw = StreamUnpacker(model, B, K, slot_n_q=True)
    assert raw._key_slots([bytes([1, 1 | KEY_BIT]) + bytes(2), b'', b'']) == []
    with pytest.raises(ValueError):
        raw.unpack_slots([bytes([1, 1 | KEY_BIT]) + bytes(2), b'', b''])
    # a flagged packet takes a lost and failed slot back in on the host, before any device call
    u.lose([0, 1])
    assert u.failed == [0, 1]
    with pytest.raises(RuntimeError):                                  # the LM is on the CPU
        u.unpack_slots([bytes([3, 5 | KEY_BIT, 1, 2]), bytes([1, K, 9]), b''])
    assert u.failed == [1] and u._lost == {1}


def test_entry_point_declared_and_bound():
    from encx._lib import parse_header, lib, LIB_PATH
    name = 'encx_bitpack_slots_fec'
    sigs = parse_header()
    src = open(os.path.join(ROOT, 'include', 'encx.h')).read()
    declared = set(re.findall(r'\b(encx_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    assert name in declared and name in sigs and name in lib.sigs
    res, args = lib.sigs[name]
    assert res is ctypes.c_int and args[-1] is ctypes.c_void_p  # int f(..., encx_stream_t)
    assert len(args) == len(sigs['encx_bitpack_slots_nq'][1]) + 4  # R, h_max, the fec table, the history
    assert 'REDUNDANT PACKET' in src and 'KEY PACKET' in src
    assert os.path.exists(LIB_PATH), 'build first: __graft_entry__.build()'
    assert hasattr(ctypes.CDLL(LIB_PATH), name)


def test_entry_point_refuses_before_any_launch():
    """NULL pointers, sizes out of range and a short stride are ENCX_EINVAL; nothing is launched (no
    device is touched: the pointers below are never dereferenced)."""
    from encx._lib import lib
    L = lib.load()
    p = 4096  # a non-NULL pointer value that is never followed

    def pack(codes=p, slots=p, nq=p, fec=p, hist=p, out=p, nbytes=p, err=p, B=2, K=8, n=7, bits=10, R=2, h=8,
             stride=4 + 70 + 20):
        return L.encx_bitpack_slots_fec(codes, 56, 7, 1, B, K, n, bits, R, h, slots, nq, fec, hist, out, stride,
                                        nbytes, err, None)

    for name in ('codes', 'slots', 'nq', 'fec', 'hist', 'out', 'nbytes', 'err'):
        assert pack(**{name: None}) == EINVAL, name
    big = 1 << 20
    for bad in (dict(B=0), dict(B=65), dict(K=0), dict(K=65, stride=big), dict(n=0), dict(n=256, h=255, stride=big),
                dict(bits=0), dict(bits=33, stride=big), dict(R=0), dict(R=9, stride=big), dict(R=-1),
                dict(h=6), dict(h=256, stride=big)):
        assert pack(**bad) == EINVAL, bad
    assert pack(stride=4 + 70 + 19) == EINVAL       # four header bytes and both sections count
    assert pack(stride=2 + 70 + 20) == EINVAL
    assert pack(stride=-1) == EINVAL
    assert pack(B=64, K=32, n=8, R=32, h=8, stride=4 + 320 + 319) == EINVAL


# ---------------------------------------------------------------- StreamReceiver, pure host logic
class StubUnpacker:
    """Answers from the headers alone: frames and n_q of the section asked for, and codes whose
    value names the slot."""

    def __init__(self):
        self.calls = []

    def unpack_slots(self, packets, recover=None):
        self.calls.append((list(packets), list(recover)))
        frames, nq = [], []
        for p, r in zip(packets, recover):
            n, k, n_r, k_r = p[:4] if len(p) else (0, 0, 0, 0)
            frames.append(n_r if r else n)
            nq.append(k_r if r else k)
        codes = torch.zeros(len(packets), K, max(frames), dtype=torch.int64)
        for b, f in enumerate(frames):
            codes[b, :, :f] = b + 1
        return codes, frames, nq


class StubDecoder:
    def __init__(self):
        self.calls = []

    def decode_slots(self, codes, frames, n_q=None, lost=None):
        self.calls.append((codes, list(frames), list(n_q), lost))
        return 'wave'


def receiver():
    from encx.streaming import StreamReceiver
    rx = StreamReceiver(StubDecoder(), StubUnpacker())
    return rx, rx.decoder.calls, rx.unpacker.calls


def test_receiver_chooses_main_recovered_concealed_idle():
    rx, dec, unp = receiver()
    this, nxt, bare = fec_packet(3, 8, 0, 0), fec_packet(2, 8, 5, 2), fec_packet(2, 8, 0, 0)
    wav, status = rx.step([this, b'', None, None, None], [None, None, nxt, None, bare], [9, 9, 9, 6, 4])
    assert wav == 'wave' and status == ['main', 'idle', 'recovered', 'concealed', 'concealed']
    assert unp == [([this, b'', nxt, b'', bare], [False, False, True, False, True])]
    (codes, frames, nq, lost), = dec
    assert frames == [3, 0, 5, 6, 4] and nq == [8, 0, 2, 0, 0]
    assert lost == [False, False, False, True, True]
    # padded to the longest concealed slot; what the unpacker gave is untouched
    assert codes.shape == (5, K, 6) and codes[0, :, :3].eq(1).all() and codes[2, :, :5].eq(3).all()
    assert not codes[:, :, 5:].any()


def test_receiver_passes_no_lost_list_when_nothing_is_concealed():
    rx, dec, unp = receiver()
    a, nxt = fec_packet(8, 1, 0, 0), fec_packet(1, 1, 8, 1)
    _, status = rx.step([a, None], [nxt, nxt], [1, 8])      # ahead of a slot that delivered is not used
    assert status == ['main', 'recovered'] and unp[0] == ([a, nxt], [False, True])
    (codes, frames, nq, lost), = dec
    assert lost is None and frames == [8, 8] and nq == [1, 1] and codes.shape == (2, K, 8)


def test_receiver_conceals_without_codes_when_nothing_decodes():
    rx, dec, unp = receiver()
    bare = fec_packet(2, 8, 0, 0)
    _, status = rx.step([None, b'', None], [None, None, bare], [3, 0, 2])
    assert status == ['concealed', 'idle', 'concealed'] and len(unp) == 1   # the copy was asked for: none there
    assert dec == [(None, [3, 0, 2], [0, 0, 0], [True, False, True])]
    rx, dec, unp = receiver()
    rx.step([None, b''], [None, None], [3, 0])
    assert unp == [] and dec == [(None, [3, 0], [0, 0], [True, False])]   # no packet at all: no unpack call
    for bad in (([b''], [None, None], [0]), ([b''], [None], [0, 0])):
        with pytest.raises(ValueError):
            rx.step(*bad)
