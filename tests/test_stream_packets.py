"""CPU checks of the streaming packet layer (encx/streaming.py StreamPacker / StreamUnpacker,
encx/lm.py LMStreamEncoder / LMStreamDecoder): the packet length rule, every host-only refusal on
a model that never saw a device (ValueError before any launch or copy, the session still usable),
and the argument validation of the new entry points (ENCX_EINVAL before any device call), after
the pattern of tests/test_stream_slots.py."""
import pytest
import torch

B, K, BITS, MAXF = 3, 8, 10, 8


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


def test_packet_length_rule():
    from encx.streaming import packet_bytes
    from encx._lib import lib
    l = lib.load()
    for n in (1, 2, 7, 8, 255):
        for k in (1, 3, 8, 32):
            for bits in (1, 7, 10, 32):
                want = 1 + -(-n * k * bits // 8)
                assert packet_bytes(n, k, bits) == want == 1 + l.encx_bitpack_bytes(n * k, bits)
    assert packet_bytes(1, 8, 10) == 11 and packet_bytes(8, 8, 10) == 81


def test_constructor_refusals(model, lm):
    from encx.streaming import StreamPacker, StreamUnpacker
    from encx.lm import LMStreamEncoder, LMStreamDecoder
    for cls in (StreamPacker, StreamUnpacker):
        for kw in (dict(batch=0), dict(batch=65), dict(n_q=0), dict(n_q=33), dict(max_frames=0),
                   dict(max_frames=256)):
            with pytest.raises(ValueError):
                cls(model, **{**dict(batch=B, n_q=K), **kw})
        cls(model, 64, 32, max_frames=255)
    for cls in (LMStreamEncoder, LMStreamDecoder):
        for kw in (dict(batch=0), dict(batch=65), dict(K=0), dict(K=K + 1), dict(max_frames=0), dict(max_frames=256)):
            with pytest.raises(ValueError):
                cls(lm, **{**dict(batch=B, K=K), **kw})
        assert cls(lm, 64, K, max_frames=255).R == 5 + 255


BAD_FRAMES = ((1, 1), (1, 1, 1, 1),        # wrong length
              (9, 0, 0), (-1, 1, 1),       # outside 0..max_frames
              (0, 0, 0),                   # nobody delivers
              (1.0, 1, 1), 'xyz')          # not ints


def test_pack_refusals_are_host_only(model, lm):
    """The model and the LM are on the CPU: a call that passed its host checks would raise
    RuntimeError (no CPU fallback), so ValueError shows the refusal came first."""
    from encx.streaming import StreamPacker
    from encx.lm import LMStreamEncoder
    codes = torch.zeros(B, K, MAXF, dtype=torch.int64)
    for p in (StreamPacker(model, B, K), StreamPacker(model, B, K, use_lm=True, lm=lm)):
        for frames in BAD_FRAMES:
            with pytest.raises(ValueError):
                p.pack_slots(codes, frames)
        with pytest.raises(ValueError):
            p.pack_slots(codes[:, :, :3], (1, 8, 0))               # the tensor is not max(frames) long
        with pytest.raises(ValueError):
            p.pack_slots(codes.to(torch.int32), (1, 8, 0))
        for bad in ([3], [-1], [0.5]):
            with pytest.raises(ValueError):
                p.restart(bad)
        p.restart([0, 2])
        p.reset()
        with pytest.raises(RuntimeError, match='no CPU fallback'):  # valid: reaches the device check
            p.pack_slots(codes, (1, 8, 0))
    e = LMStreamEncoder(lm, B, K)
    for frames in BAD_FRAMES:
        with pytest.raises(ValueError):
            e.encode_slots(codes, frames)
    assert e.started == [False] * B and not e._ready


def test_unpack_refusals_are_host_only(model, lm):
    from encx.streaming import StreamUnpacker, packet_bytes
    from encx.lm import LMStreamDecoder
    good = lambda n: bytes([n]) + bytes(packet_bytes(n, K, BITS) - 1)
    raw = StreamUnpacker(model, B, K)
    coded = StreamUnpacker(model, B, K, use_lm=True, lm=lm)
    for u in (raw, coded):
        for packets in ([good(1)] * 2, [good(1)] * 4,             # wrong length
                        [b'', b'', b''],                          # nobody delivers
                        [bytes([0]) + bytes(10), b'', b''],       # a header byte of 0
                        [bytes([9]) + bytes(90), b'', b''],       # above max_frames
                        [good(1), 'abc', b''], [good(1), None, b'']):
            with pytest.raises(ValueError):
                u.unpack_slots(packets)
        assert u.failed == []
        with pytest.raises(RuntimeError, match='no CPU fallback|on the GPU'):
            u.unpack_slots([good(1), good(8), b''])
    for packets in ([good(1)[:-1], b'', b''], [good(1) + b'\0', b'', b''], [good(2)[:11], b'', b''],
                    [bytes([1]), b'', b'']):                      # a raw payload of the wrong length
        with pytest.raises(ValueError):
            raw.unpack_slots(packets)
    d = LMStreamDecoder(lm, B, K)
    for frames in BAD_FRAMES:
        with pytest.raises(ValueError):
            d.decode_slots([b'x'] * B, frames)
    for payloads, frames in (([b'x'] * 2, (1, 1, 1)), ([b'x', b'x', b'x'], (1, 1, 0)),   # bytes for 0 frames
                             ([b'x', 'x', b''], (1, 1, 0)), ([bytes(d.cap + 1), b'', b''], (8, 0, 0))):
        with pytest.raises(ValueError):
            d.decode_slots(payloads, frames)
    # a slot that failed refuses packets until it is restarted (the state a bad packet leaves)
    d.failed.add(1)
    with pytest.raises(ValueError, match='restart'):
        d.decode_slots([b'x', b'x', b''], (1, 1, 0))
    d.restart([1])
    assert not d.failed and not d._ready


def test_packet_entry_points_validate_before_any_device_call():
    """NULL pointers, B outside 1..64, n_max < 1, K outside 1..64, bits outside 1..32 and
    R < past_context + n_max -> ENCX_EINVAL (9001); the non-NULL pointers are never dereferenced."""
    from encx._lib import lib
    l = lib.load()
    p = 4096

    def sweep(fn, names, good, ptrs, bad):
        """each pointer NULL in turn, then each bad value of a named size"""
        for n in ptrs:
            args = [None if k == n else v for k, v in zip(names, good)]
            assert fn(*args) == 9001, (fn.__name__, n)
        for n, values in bad.items():
            for v in values:
                args = [v if k == n else g for k, g in zip(names, good)]
                assert fn(*args) == 9001, (fn.__name__, n, v)

    sizes = dict(B=(0, 65, -1), K=(0, 65), n_max=(0, -1, 256))
    sweep(l.encx_bitpack_slots,
          ('codes', 'sb', 'sk', 'st', 'B', 'K', 'n_max', 'bits', 'slots', 'out', 'stride', 'nbytes', 'err', 'stream'),
          [p, 64, 8, 1, 3, 8, 8, 10, p, p, 81, p, p, None], ('codes', 'slots', 'out', 'nbytes', 'err'),
          dict(sizes, bits=(0, 33), stride=(80, 0)))
    sweep(l.encx_bitunpack_slots,
          ('in', 'stride', 'B', 'K', 'n_max', 'bits', 'slots', 'codes', 'sb', 'sk', 'st', 'stream'),
          [p, 80, 3, 8, 8, 10, p, p, 64, 8, 1, None], ('in', 'slots', 'codes'),
          dict(sizes, bits=(0, 33), stride=(79, 0)))
    sweep(l.encx_lm_input_slots,
          ('codes', 'sb', 'sk', 'st', 'B', 'K', 'T', 'n_max', 'slots', 'pos', 'prev', 'dstep', 'emb', 'card1', 'D',
           'ln_w', 'ln_b', 'period', 'x', 'stream'),
          [p, 64, 8, 1, 3, 8, 8, 8, p, p, p, None, p, 65, 64, p, p, 10000., p, None],
          ('slots', 'pos', 'prev', 'emb', 'ln_w', 'ln_b', 'x'), dict(sizes, T=(0, 9), D=(0, 3, 514), card1=(0,)))
    layer = ('x', 'y', 'B', 'T', 'n_max', 'kv', 'R', 'slots', 'pos', 'dstep', 'P', 'D', 'heads', 'F') + \
        tuple(f'w{i}' for i in range(12)) + ('work', 'stream')
    sweep(l.encx_lm_layer_slots, layer, [p, p, 3, 8, 8, p, 13, p, p, None, 5, 64, 4, 256] + [p] * 12 + [p, None],
          ('x', 'y', 'kv', 'slots', 'pos', 'work') + tuple(f'w{i}' for i in range(12)),
          dict(B=(0, 65), n_max=(0, 256), T=(0, 9), R=(12, 0), P=(-1, 6), heads=(0, 3), D=(0, 520)))
    sweep(l.encx_lm_slots_advance,
          ('slots', 'B', 'K', 'n_max', 'pos', 'prev', 'codes', 'sb', 'sk', 'st', 'card1', 'stream'),
          [p, 3, 8, 8, p, p, None, 0, 0, 0, 65, None], ('slots', 'pos', 'prev'), dict(sizes, card1=(0,)))
    sweep(l.encx_ac_encode_slots,
          ('lohi', 'B', 'n_max', 'K', 'slots', 'bits', 'out', 'stride', 'nbytes', 'err', 'stream'),
          [p, 3, 8, 8, p, 24, p, 209, p, p, None], ('lohi', 'slots', 'out', 'nbytes', 'err'),
          dict(sizes, bits=(0, 31), stride=(0,)))
    sweep(l.encx_ac_decode_slots,
          ('data', 'stride', 'nbytes', 'B', 'state', 'cdf', 'K', 'card', 'bits', 'codes', 'cs', 'ck', 'ct', 'n_max',
           'dstep', 'slots', 'prev', 'err', 'stream'),
          [p, 208, p, 3, p, p, 8, 1024, 24, p, 64, 8, 1, 8, p, p, p, p, None],
          ('data', 'nbytes', 'state', 'cdf', 'codes', 'dstep', 'slots', 'prev', 'err'),
          dict(sizes, bits=(0, 31), card=(0,), stride=(0,)))
