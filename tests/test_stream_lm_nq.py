"""CPU checks of LM-coded packets with a codebook count per slot and step (packet format 2 of
include/encx.h; encx/lm.py LMStreamEncoder / LMStreamDecoder(lm_format=2), encx/streaming.py
StreamPacker / StreamUnpacker(use_lm=True, lm_format=2)):

  * the short flush, on a restatement of oracle/ac_oracle.encode's loop (tests/ac_short_ref.py) that
    is first pinned to the oracle byte for byte with the reference's flush;
  * every host-only refusal on a model that never saw a device, the header parse, the pinned
    NotImplementedError of use_lm=True with slot_n_q=True;
  * ENCX_EINVAL from each new entry point before any device call."""
import numpy as np
import pytest
import torch

from oracle import ac_oracle as A
from fixtures import load, g12_ac_rows
import ac_short_ref as S

B, K, BITS, MAXF = 3, 8, 10, 8


# ============================================================================ the short flush
def random_case(g, card, n, bits=24):
    """n (symbol, cdf) pairs of a peaky random pdf through the oracle's own quantizer."""
    syms, cdfs = [], []
    for _ in range(n):
        p = g.random(card).astype(np.float32) ** 8 + 1e-9
        p = (p / (p.sum(dtype=np.float64) * (1 + 1e-5))).astype(np.float32)   # a total the coder accepts
        cdfs.append(A.quantized_cdf(p, bits))
        syms.append(int(g.choice(card, p=p.astype(np.float64) / p.astype(np.float64).sum())))
    return syms, cdfs


def coder_cases():
    out = []
    for card, bits, pdf, cdf, sym, data, eof in g12_ac_rows(load('g12_lm.npz')):
        out.append((f'g12 card {card}', [int(s) for s in sym], list(cdf), bits, data if not eof else None))
    g = np.random.default_rng(2024)
    for card in (2, 5, 64, 1024):
        for n in (1, 2, 3, 8, 17, 39):
            syms, cdfs = random_case(g, card, n)
            out.append((f'random card {card} n {n}', syms, cdfs, 24, None))
    return out


CASES = coder_cases()


def test_restatement_with_the_reference_flush_is_the_oracle():
    for name, syms, cdfs, bits, data in CASES:
        want = A.encode(syms, cdfs, bits)
        assert S.encode(syms, cdfs, bits) == want, name
        if data is not None:
            assert want == data, name


def test_short_flush_decodes_is_minimal_and_never_longer():
    saved = []
    for name, syms, cdfs, bits, _ in CASES:
        ref, short = S.encode(syms, cdfs, bits), S.encode(syms, cdfs, bits, short=True)
        assert S.decode_padded(short, cdfs, bits) == syms, name
        assert len(short) <= len(ref), name
        if short:
            assert short[-1] != 0, name
            try:   # a value below `low`: other symbols, or no interval at all
                assert S.decode_padded(short[:-1], cdfs, bits) != syms, name
            except RuntimeError as err:
                assert 'Binary search failed' in str(err)
        saved.append(len(ref) - len(short))
    assert min(saved) >= 0 and max(saved) >= 1
    print(f'short flush: {np.mean(saved):.2f} bytes saved per run on average over {len(saved)} runs')


def test_short_flush_of_all_zero_symbols_is_empty():
    """Every symbol 0 with range_low 0: low stays 0, so v = 0 and every byte is dropped."""
    g = np.random.default_rng(5)
    for card, n in ((2, 1), (64, 7), (1024, 16)):
        _, cdfs = random_case(g, card, n)
        syms = [0] * n
        assert S.encode(syms, cdfs, short=True) == b''
        assert S.decode_padded(b'', cdfs) == syms
        assert len(S.encode(syms, cdfs)) >= 3


# ============================================================================ host logic
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


def test_constructor_refusals_and_the_pinned_combination(model, lm):
    from encx.streaming import StreamPacker, StreamUnpacker
    from encx.lm import LMStreamEncoder, LMStreamDecoder
    for cls in (StreamPacker, StreamUnpacker):
        with pytest.raises(NotImplementedError, match='lm_format=2'):
            cls(model, B, K, use_lm=True, lm=lm, slot_n_q=True)
        with pytest.raises(ValueError, match='use_lm=True'):
            cls(model, B, K, lm_format=2)
        with pytest.raises(ValueError, match='use_lm=True'):
            cls(model, B, K, slot_n_q=True, lm_format=2)
        for bad in (0, 3, '2'):
            with pytest.raises(ValueError, match='lm_format'):
                cls(model, B, K, use_lm=True, lm=lm, lm_format=bad)
        s = cls(model, B, K, use_lm=True, lm=lm, lm_format=2)
        assert s.lm_format == 2 and s._lm.lm_format == 2 and s._lm.K == K
        assert cls(model, B, K, use_lm=True, lm=lm)._lm.lm_format == 1
    for cls in (LMStreamEncoder, LMStreamDecoder):
        for bad in (0, 3):
            with pytest.raises(ValueError, match='lm_format'):
                cls(lm, B, K, lm_format=bad)
        assert cls(lm, B, K).lm_format == 1


BAD_NQ = ((8, 8), (8, 8, 8, 8),        # wrong length
          (0, 8, 8), (9, 8, 8), (-1, 8, 8),   # outside 1..K for a slot that delivers
          (1.5, 8, 8), 5)              # not ints, not a sequence


def test_pack_refusals_are_host_only(model, lm):
    """Model and LM are on the CPU: a call that passed its host checks would raise RuntimeError
    (no CPU fallback), so ValueError shows that the refusal came first."""
    from encx.streaming import StreamPacker
    from encx.lm import LMStreamEncoder
    codes = torch.zeros(B, K, MAXF, dtype=torch.int64)
    p = StreamPacker(model, B, K, use_lm=True, lm=lm, lm_format=2)
    e = LMStreamEncoder(lm, B, K, lm_format=2)
    for call in (p.pack_slots, e.packets, e.encode_slots):
        with pytest.raises(ValueError, match='n_q'):
            call(codes, (8, 8, 8))                       # format 2 without n_q
        for nq in BAD_NQ:
            with pytest.raises(ValueError):
                call(codes, (8, 8, 8), nq)
        with pytest.raises(ValueError):
            call(codes, (9, 8, 8), (8, 8, 8))
        with pytest.raises(ValueError):
            call(codes[:, :, :3], (8, 8, 8), (8, 8, 8))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call(codes, (1, 8, 0), (1, 8, 'ignored at a slot that sits out'))
    assert e.started == [False] * B and not e._ready
    for s in (StreamPacker(model, B, K, use_lm=True, lm=lm), LMStreamEncoder(lm, B, K)):
        with pytest.raises(ValueError, match='n_q'):     # format 1 takes no n_q
            (s.pack_slots if hasattr(s, 'pack_slots') else s.packets)(codes, (8, 8, 8), (8, 8, 8))


def test_unpack_header_parse_and_refusals_are_host_only(model, lm):
    from encx.streaming import StreamUnpacker
    from encx.lm import LMStreamDecoder
    u = StreamUnpacker(model, B, K, use_lm=True, lm=lm, lm_format=2)
    cap = u._lm.cap
    pk = lambda n, k, size=3: bytes([n, k]) + bytes(size)
    assert u._headers_nq([pk(1, 8), b'', pk(8, 1, 0)]) == ([1, 0, 8], [8, 0, 1])   # an empty payload is a packet
    assert u._headers_nq([pk(8, 8, cap), b'', b'']) == ([8, 0, 0], [8, 0, 0])
    for packets in ([pk(1, 8)] * 2, [pk(1, 8)] * 4,              # wrong length
                    [b'', b'', b''],                             # nobody delivers
                    [bytes([1]), b'', b''],                      # no (n, K) header
                    [pk(0, 8), b'', b''], [pk(9, 8), b'', b''],  # n outside 1..max_frames
                    [pk(1, 0), b'', b''], [pk(1, 9), b'', b''],  # K outside 1..K_max
                    [pk(8, 8, cap + 1), b'', b''],               # above the capacity
                    [pk(1, 8), 'abc', b''], [pk(1, 8), None, b'']):
        with pytest.raises(ValueError):
            u.unpack_slots(packets)
    assert u.failed == []
    with pytest.raises(RuntimeError, match='no CPU fallback|on the GPU'):
        u.unpack_slots([pk(1, 8), pk(8, 2), b''])
    d = LMStreamDecoder(lm, B, K, lm_format=2)
    with pytest.raises(ValueError, match='n_q'):
        d.decode_slots([b'x'] * B, (1, 1, 1))
    for nq in BAD_NQ:
        with pytest.raises(ValueError):
            d.decode_slots([b'x'] * B, (1, 1, 1), nq)
    for payloads, frames in (([b'x'] * 2, (1, 1, 1)), ([b'x', b'x', b'x'], (1, 1, 0)),
                             ([bytes(d.cap + 1), b'', b''], (8, 0, 0))):
        with pytest.raises(ValueError):
            d.decode_slots(payloads, frames, (8, 8, 8))
    d.failed.add(1)
    with pytest.raises(ValueError, match='restart'):
        d.decode_slots([b'x', b'', b''], (1, 1, 0), (8, 8, 8))
    d.restart([1])
    assert not d.failed and not d._ready
    with pytest.raises(ValueError, match='n_q'):
        LMStreamDecoder(lm, B, K).decode_slots([b'x'] * B, (1, 1, 1), (8, 8, 8))


# ============================================================================ the entry points
def test_new_entry_points_are_declared_and_bound():
    from encx._lib import lib, parse_header
    sigs = parse_header()
    l = lib.load()
    for name, nargs in (('encx_lm_input_slots_nq', 21), ('encx_lm_slots_advance_nq', 13), ('encx_lm_heads_slots', 25),
                        ('encx_ac_encode_slots_nq', 12), ('encx_ac_decode_slots_nq', 20)):
        assert name in sigs and len(sigs[name][1]) == nargs, name
        assert getattr(l, name).argtypes == sigs[name][1]


def test_new_entry_points_validate_before_any_device_call():
    """NULL pointers and sizes outside their ranges -> ENCX_EINVAL (9001); the non-NULL pointers
    are never dereferenced (they point nowhere)."""
    from encx._lib import lib
    l = lib.load()
    p = 4096

    def sweep(fn, names, good, ptrs, bad):
        for n in ptrs:
            args = [None if k == n else v for k, v in zip(names, good)]
            assert fn(*args) == 9001, (fn.__name__, n)
        for n, values in bad.items():
            for v in values:
                args = [v if k == n else g for k, g in zip(names, good)]
                assert fn(*args) == 9001, (fn.__name__, n, v)

    sizes = dict(B=(0, 65, -1), K=(0, 65), n_max=(0, -1, 256))
    sweep(l.encx_lm_input_slots_nq,
          ('codes', 'sb', 'sk', 'st', 'B', 'K', 'T', 'n_max', 'slots', 'nq', 'pos', 'prev', 'dstep', 'emb', 'card1', 'D',
           'ln_w', 'ln_b', 'period', 'x', 'stream'),
          [p, 64, 8, 1, 3, 8, 8, 8, p, p, p, p, None, p, 65, 64, p, p, 10000., p, None],
          ('slots', 'nq', 'pos', 'prev', 'emb', 'ln_w', 'ln_b', 'x'),
          dict(sizes, T=(0, 9), D=(0, 3, 514), card1=(0,)))
    sweep(l.encx_lm_slots_advance_nq,
          ('slots', 'nq', 'B', 'K', 'n_max', 'pos', 'prev', 'codes', 'sb', 'sk', 'st', 'card1', 'stream'),
          [p, p, 3, 8, 8, p, p, None, 0, 0, 0, 65, None], ('slots', 'nq', 'pos', 'prev'), dict(sizes, card1=(0,)))
    sweep(l.encx_lm_heads_slots,
          ('x', 'B', 'T', 'n_max', 'D', 'w', 'bias', 'K', 'card', 'slots', 'nq', 'dstep', 'work', 'probas', 'cdf',
           'bits', 'roundoff', 'min_range', 'sym', 'sb', 'sk', 'st', 'lohi', 'err', 'stream'),
          [p, 3, 8, 8, 64, p, p, 8, 64, p, p, None, p, None, p, 24, 1e-8, 2, p, 64, 8, 1, p, p, None],
          ('x', 'w', 'bias', 'slots', 'nq', 'work', 'cdf', 'lohi'),
          dict(sizes, T=(0, 9), D=(0,), card=(0, 65537), bits=(0, 31), min_range=(1,)))
    sweep(l.encx_ac_encode_slots_nq,
          ('lohi', 'B', 'n_max', 'K', 'slots', 'nq', 'bits', 'out', 'stride', 'nbytes', 'err', 'stream'),
          [p, 3, 8, 8, p, p, 24, p, 210, p, p, None], ('lohi', 'slots', 'nq', 'out', 'nbytes', 'err'),
          dict(sizes, bits=(0, 31), stride=(0, 1)))
    sweep(l.encx_ac_decode_slots_nq,
          ('data', 'stride', 'nbytes', 'B', 'state', 'cdf', 'K', 'card', 'bits', 'codes', 'cs', 'ck', 'ct', 'n_max',
           'dstep', 'slots', 'nq', 'prev', 'err', 'stream'),
          [p, 208, p, 3, p, p, 8, 1024, 24, p, 64, 8, 1, 8, p, p, p, p, p, None],
          ('data', 'nbytes', 'state', 'cdf', 'codes', 'dstep', 'slots', 'nq', 'prev', 'err'),
          dict(sizes, bits=(0, 31), card=(0,), stride=(0,)))
