"""The streaming packet layer on the GPU: one self-contained packet per delivering slot and step,
raw (bit-packed) or arithmetic-coded under an LM whose state is carried across a slot's packets
(encx/streaming.py StreamPacker / StreamUnpacker, encx/lm.py LMStreamEncoder / LMStreamDecoder;
the format: include/encx.h).

Every comparison is == on bytes or torch.equal on codes, against references outside the new code:
oracle/ecdc_oracle.bitpack for the raw form; for the LM form the EXISTING one-pass LM path
(lm._body + lm._heads over each slot's whole stream) with oracle/ac_oracle.encode over its cdf
rows, and lm.encode_streams for a stream's first packet. The one tolerance: the probabilities
behind the streamed cdfs against oracle/lm_oracle.lm_step driven chunk by chunk, under the
project's LM bound of tests/test_lm.py (rtol 2e-4, atol 1e-6), no extra margin.

Every feed poisons what a slot does not deliver (codes +-2^40 past its count): the packets equal
references that never saw the tail, so the tail changes no byte."""
import numpy as np
import pytest
import torch
from torch import nn

from oracle import ecdc_oracle as E, ac_oracle as A
from test_lm import _lm
from test_gpu_stream_slots import RUN1
from test_gpu_stream import build, DEV, HOP, FRAMES

pytestmark = pytest.mark.gpu

POISON = 1 << 40


def feed(codes, off, frames, n_max):
    """[B, K, n_max] on the device: slot b's next frames[b] columns, the rest poisoned."""
    B, K, _ = codes.shape
    x = torch.empty(B, K, n_max, dtype=torch.int64)
    for b, f in enumerate(frames):
        x[b] = POISON if b % 2 else -POISON
        x[b, :, :f] = codes[b, :, off[b]:off[b] + f]
    return x.to(DEV)


# ============================================================================ raw packets
class Codec(nn.Module):
    """What the packet layer reads of a model: the code width, the codebook count, a device."""

    def __init__(self, bits, n_q):
        super().__init__()
        self.bits_per_codebook = bits
        self.quantizer = type('Q', (), {'n_q': n_q})()
        self.w = nn.Parameter(torch.zeros(1))


def raw_run(B, K, bits, schedule, seed):
    from encx.streaming import StreamPacker, StreamUnpacker
    m = Codec(bits, K).to(DEV)
    packer, unpacker = StreamPacker(m, B, K), StreamUnpacker(m, B, K)
    total = [sum(f[b] for f in schedule) for b in range(B)]
    g = np.random.default_rng(seed)
    codes = torch.from_numpy(g.integers(0, 1 << bits, size=(B, K, max(total) + 1)))
    codes[:, :, 0] = (1 << bits) - 1  # every bit of a code set: the top of the range
    off = [0] * B
    for frames in schedule:
        n = max(frames)
        x = feed(codes, off, frames, n)
        packets = packer.pack_slots(x, frames)
        back, fr = unpacker.unpack_slots(packets)
        assert fr == list(frames) and back.shape == (B, K, n) and back.dtype == torch.int64 and back.is_cuda
        for b, f in enumerate(frames):
            mine = codes[b, :, off[b]:off[b] + f]
            want = bytes([f]) + E.bitpack(mine.t().reshape(-1).numpy(), bits) if f else b''
            assert packets[b] == want, (b, frames)
            assert len(want) == (1 + -(-f * K * bits // 8) if f else 0)
            assert torch.equal(back[b, :, :f].cpu(), mine) and not back[b, :, f:].any(), (b, frames)
            off[b] += f
    return packer, codes


def test_raw_packets_over_run1_equal_the_oracle_and_unpack():
    """B = 3, K = 8, 10 bits, run 1 of test_gpu_stream_slots: (1, 8, 0), joins, idle steps; tails
    poisoned. A delivered code that does not fit raises; the same value in a tail does not."""
    packer, codes = raw_run(3, 8, 10, RUN1, 11)
    x = feed(codes, [0, 0, 0], (2, 8, 0), 8)
    assert len(packer.pack_slots(x, (2, 8, 0))[1]) == 81
    x[0, 3, 2] = 1 << 10          # slot 0 delivers 2 frames: column 2 is its tail
    packer.pack_slots(x, (2, 8, 0))
    x[0, 3, 1] = 1 << 10
    with pytest.raises(ValueError, match='10 bits'):
        packer.pack_slots(x, (2, 8, 0))
    x[0, 3, 1] = -1
    with pytest.raises(ValueError, match='10 bits'):
        packer.pack_slots(x, (2, 8, 0))
    x[0, 3, 1] = 5
    assert packer.pack_slots(x, (2, 8, 0))[0][0] == 2  # the session is still usable


@pytest.mark.parametrize('bits', (1, 7, 32))
@pytest.mark.parametrize('K', (1, 3))
def test_raw_packets_partial_bytes(bits, K):
    raw_run(3, K, bits, ((1, 8, 0), (7, 0, 3), (2, 5, 8), (0, 0, 1)), 100 * bits + K)


def test_raw_packets_slots_0_and_63_of_64():
    fr = lambda first, last: (first,) + (0,) * 62 + (last,)
    raw_run(64, 8, 10, (fr(3, 0), fr(1, 8), fr(0, 5), fr(8, 8)), 13)


# ============================================================================ LM packets
LM_RUN = ((7, 0, 0), (1, 7, 0), (8, 0, 0), (1, 8, 0), (2, 0, 0), (8, 1, 0), (8, 3, 7), (5, 8, 1), (0, 8, 8),
          (0, 5, 8), (0, 0, 8), (0, 0, 8))
LM_T = 40


def one_pass_cdf(lm, codes):
    """The existing one-pass path over whole streams [B, K, T] -> cdf rows [B][T][K][card]."""
    B, K, Tn = codes.shape
    lm._packed()
    full = torch.zeros_like(codes)
    full[:, :, 1:] = codes[:, :, :-1] + 1
    x = lm._body(full, full.stride(), B, K, Tn, False, lm.new_state(B, Tn + 1))
    cdf = torch.empty(B, Tn, K, lm.card, device=DEV, dtype=torch.int32)
    lm._heads(x, B, Tn, K, cdf=cdf)
    return cdf.cpu().numpy().astype(np.int64)


def oracle_payload(codes, cdf, b, t0, n):
    """ac_oracle.encode of slot b's frames [t0, t0 + n), t-major then codebook, over those rows."""
    K = codes.shape[1]
    rows = [(t, k) for t in range(t0, t0 + n) for k in range(K)]
    return A.encode([int(codes[b, k, t]) for t, k in rows], [cdf[b, t, k] for t, k in rows])


def lm_drive(lm, codes, schedule, graphs=True, enc=None, dec=None, off=None):
    """Code the streams codes [B, K, T] (host) along `schedule`, every payload decoded at once ->
    per slot the list of (first frame, frames, payload)."""
    from encx.lm import LMStreamEncoder, LMStreamDecoder
    B, K, _ = codes.shape
    enc = enc or LMStreamEncoder(lm, B, K, graphs=graphs)
    dec = dec or LMStreamDecoder(lm, B, K, graphs=graphs)
    off = off if off is not None else [0] * B
    out = [[] for _ in range(B)]
    for frames in schedule:
        n = max(frames)
        x = feed(codes, off, frames, n)
        pay = enc.encode_slots(x, frames)
        got, failed = dec.decode_slots(pay, frames)
        assert failed == [] and got.shape == (B, K, n)
        for b, f in enumerate(frames):
            assert (len(pay[b]) > 0) == (f > 0)
            assert torch.equal(got[b, :, :f], x[b, :, :f]) and not got[b, :, f:].any(), (b, frames)
            if f:
                out[b].append((off[b], f, pay[b]))
                off[b] += f
    return out, enc, dec


@pytest.fixture(scope='module')
def small():
    """LM 'b' (past_context 5: the ring of 13 rows wraps every other step), three streams of 40
    frames, their one-pass cdfs, and the run with graphs; computed once, left unchanged."""
    ns = type('Ctx', (), {})()
    ns.lm, ns.cfg, _ = _lm('b')
    g = np.random.default_rng(17)
    ns.codes = torch.from_numpy(g.integers(0, ns.cfg.card, size=(3, 4, LM_T)))
    ns.cdf = one_pass_cdf(ns.lm, ns.codes.to(DEV))
    assert [sum(f[b] for f in LM_RUN) for b in range(3)] == [LM_T] * 3 and (1, 8, 0) in LM_RUN
    ns.run, ns.enc, ns.dec = lm_drive(ns.lm, ns.codes, LM_RUN)
    return ns


def test_lm_first_packet_is_the_existing_coder(small):
    for b in range(3):
        t0, n, pay = small.run[b][0]
        assert t0 == 0 and pay == small.lm.encode_streams(small.codes[b:b + 1, :, :n].to(DEV))[0]


def test_lm_chunking_never_changes_a_cdf(small):
    """Every packet = the oracle coder over the ONE-PASS cdf rows of its frames: the ring wraps
    many times, prev is carried, dead rows write nothing, the window is read in order."""
    assert small.enc.R == 13 and len(small.enc._graphs) > 1 and len(small.dec._graphs) == 1
    for b in range(3):
        assert sum(n for _, n, _ in small.run[b]) == LM_T
        for t0, n, pay in small.run[b]:
            assert pay == oracle_payload(small.codes, small.cdf, b, t0, n), (b, t0, n)


def test_lm_graph_equals_eager_round_trip(small):
    """lm_drive decodes every payload and compares the codes; eager gives the graphs' bytes."""
    eager, enc, dec = lm_drive(small.lm, small.codes, LM_RUN, graphs=False)
    assert not enc._graphs and not dec._graphs
    assert eager == small.run


def test_lm_slot_independence(small):
    for b in range(3):
        solo, _, _ = lm_drive(small.lm, small.codes[b:b + 1], [(f[b],) for f in LM_RUN if f[b]])
        assert solo[0] == small.run[b]


def test_lm_restart_beside_a_continuing_neighbour(small):
    """B = 2. Slot 0: 15 frames of stream 0, restart in mid-clip, stream 1 from its start. Slot 1:
    stream 2 without a break. Slot 0's second clip must be coded as a fresh session codes it
    (stale pos or prev would change its first packet and all after it), slot 1 as alone."""
    c = small.codes
    first = torch.stack([c[0], c[2]])
    out1, enc, dec = lm_drive(small.lm, first, ((7, 7), (8, 1)))
    enc.restart([0])
    dec.restart([0])
    sched2 = ((1, 8), (8, 8), (8, 0), (3, 8), (8, 8), (8, 0), (4, 0))
    assert [sum(f[b] for f in sched2) for b in range(2)] == [LM_T, LM_T - 8]
    out2, _, _ = lm_drive(small.lm, torch.stack([c[1], c[2]]), sched2, enc=enc, dec=dec, off=[0, 8])
    fresh, _, _ = lm_drive(small.lm, c[1:2], [(f[0],) for f in sched2])
    assert out2[0] == fresh[0]
    alone, _, _ = lm_drive(small.lm, c[2:3], [(f[1],) for f in ((7, 7), (8, 1)) + sched2 if f[1]])
    assert out1[1] + out2[1] == alone[0]
    for t0, n, pay in out2[0]:
        assert pay == oracle_payload(c, small.cdf, 1, t0, n)


def test_lm_packet_cut_in_half(small):
    from encx.lm import LMStreamEncoder, LMStreamDecoder
    lm, c = small.lm, small.codes
    enc, dec = LMStreamEncoder(lm, 3, 4), LMStreamDecoder(lm, 3, 4)
    off = [0, 0, 0]

    def step(frames, cut=None):
        x = feed(c, off, frames, max(frames))
        pay = enc.encode_slots(x, frames)
        if cut is not None:
            pay[cut] = pay[cut][:len(pay[cut]) // 2]
        got, failed = dec.decode_slots(pay, frames)
        for b, f in enumerate(frames):
            if b not in failed:
                assert torch.equal(got[b, :, :f], x[b, :, :f]) and not got[b, :, f:].any()
            off[b] += f
        return got, failed

    assert step((7, 8, 3))[1] == []
    got, failed = step((2, 8, 8), cut=1)
    assert failed == [1] and dec.failed == {1} and not got[1].any()
    with pytest.raises(ValueError, match='restart'):
        dec.decode_slots([b'', b'\0\0', b''], (0, 1, 0))
    assert step((8, 0, 1))[1] == [] and step((1, 0, 8))[1] == []   # the others, this step and after
    enc.restart([1])
    dec.restart([1])
    off[1] = 0
    assert step((8, 8, 8))[1] == [] and step((3, 1, 2))[1] == [] and not dec.failed


def test_lm_real_size_ring_wraps_and_probabilities_vs_oracle():
    """LM 'a' (dim 200, 5 layers, past_context 262), B = 2, K = 4, 300 frames in chunks of 8: the
    ring of 270 rows wraps. Round trip exact (lm_drive); payloads = the oracle coder over the
    one-pass cdfs; the probabilities of the last chunks (frames 256..299) against
    lm_oracle.lm_step driven chunk by chunk with its own truncated states (rtol 2e-4, atol 1e-6).
    Measured on an MI355X: the worst element is at 0.077 of that bound."""
    from oracle import lm_oracle as L
    from encx.lm import LMStreamEncoder
    lm, cfg, st = _lm('a')
    B, K, Tn = 2, 4, 300
    g = np.random.default_rng(19)
    codes = torch.from_numpy(g.integers(0, cfg.card, size=(B, K, Tn)))
    sched = [(8, 8)] * 37 + [(4, 4)]
    enc = LMStreamEncoder(lm, B, K, probas=True)
    assert enc.R == 270
    # the oracle, chunk by chunk
    inp = torch.zeros_like(codes)
    inp[:, :, 1:] = codes[:, :, :-1] + 1
    states, o, ref = None, 0, {}
    for t0 in range(0, Tn, 8):
        n = min(8, Tn - t0)
        p, states, o = L.lm_step(st, inp[:, :, t0:t0 + n], states, o, cfg)
        if t0 >= 256:
            ref[t0] = p.permute(0, 3, 2, 1).numpy()   # [B, n, K, card]
    # the stream, every packet decoded; the probabilities of the late chunks
    from encx.lm import LMStreamDecoder
    dec = LMStreamDecoder(lm, B, K)
    cdf = one_pass_cdf(lm, codes.to(DEV))
    off, worst = [0, 0], 0.
    for frames in sched:
        t0 = off[0]
        out, _, _ = lm_drive(lm, codes, [frames], enc=enc, dec=dec, off=off)
        for b in range(B):
            (s0, n, pay), = out[b]
            assert s0 == t0 and pay == oracle_payload(codes, cdf, b, t0, n), (b, t0)
        if t0 in ref:
            mine = enc.last_probas.cpu().numpy()
            worst = max(worst, float(np.max(np.abs(mine - ref[t0]) / (1e-6 + 2e-4 * np.abs(ref[t0])))))
            np.testing.assert_allclose(mine, ref[t0], rtol=2e-4, atol=1e-6)
    assert off == [Tn, Tn] and sorted(ref) == list(range(256, 300, 8))
    print(f'streamed probabilities vs lm_oracle.lm_step: worst error / bound = {worst:.3f}')


# ============================================================================ end to end
@pytest.fixture(scope='module')
def codec():
    from synth import synth_wave
    from fixtures import T
    m, _, _, _ = build(1, 1)
    return m, T(synth_wave((3, 1, FRAMES * HOP), 4331))


@pytest.mark.parametrize('use_lm', (False, True))
def test_end_to_end_encode_pack_bytes_unpack_decode(codec, use_lm):
    """encode_slots -> pack_slots -> bytes -> unpack_slots -> decode_slots over run 1: the wave
    equals the one obtained by handing the codes over directly. LM-coded: a random-weight
    LMModel(n_q, 1024) installed through set_lm_model."""
    from encx.streaming import StreamEncoder, StreamDecoder, StreamPacker, StreamUnpacker
    from encx.lm import LMModel
    m, x = codec
    enc = StreamEncoder(m, 3)
    if use_lm:
        torch.manual_seed(5)
        m.set_lm_model(LMModel(enc.n_q, 1024).to(DEV).eval())
    dec, direct = StreamDecoder(m, 3, enc.n_q), StreamDecoder(m, 3, enc.n_q)
    packer, unpacker = StreamPacker(m, 3, enc.n_q, use_lm=use_lm), StreamUnpacker(m, 3, enc.n_q, use_lm=use_lm)
    off, sizes = [0, 0, 0], []
    for frames in RUN1:
        n = max(frames)
        chunk = torch.zeros(3, 1, n * HOP)
        for b, f in enumerate(frames):
            chunk[b, :, :f * HOP] = x[b, :, off[b] * HOP:(off[b] + f) * HOP]
            off[b] += f
        codes = enc.encode_slots(chunk.to(DEV), frames)
        packets = [bytes(p) for p in packer.pack_slots(codes, frames)]
        assert [p[0] if p else 0 for p in packets] == list(frames)
        sizes.append(sum(map(len, packets)))
        back, fr = unpacker.unpack_slots(packets)
        assert fr == list(frames) and torch.equal(back, codes)
        assert torch.equal(dec.decode_slots(back, fr), direct.decode_slots(codes, frames)), frames
    assert off == [FRAMES] * 3 and unpacker.failed == []
    if not use_lm:
        assert sizes == [sum(1 + -(-f * enc.n_q * 10 // 8) for f in fr if f) for fr in RUN1]
        return
    # a packet cut in half: its slot comes back empty and refuses packets until it is restarted
    codes = torch.randint(0, 1024, (3, enc.n_q, 8), device=DEV)
    packets = packer.pack_slots(codes, (8, 8, 2))
    packets[1] = packets[1][:len(packets[1]) // 2]
    back, fr = unpacker.unpack_slots(packets)
    assert fr == [8, 0, 2] and unpacker.failed == [1] and not back[1].any()
    assert torch.equal(back[0], codes[0]) and torch.equal(back[2, :, :2], codes[2, :, :2])
    with pytest.raises(ValueError, match='restart'):
        unpacker.unpack_slots(packets)
    more = packer.pack_slots(codes[:, :, :3].contiguous(), (3, 0, 1))
    back, fr = unpacker.unpack_slots(more)
    assert fr == [3, 0, 1] and torch.equal(back[0], codes[0, :, :3])
    packer.restart([1])
    unpacker.restart([1])
    back, fr = unpacker.unpack_slots(packer.pack_slots(codes, (1, 8, 0)))
    assert fr == [1, 8, 0] and unpacker.failed == [] and torch.equal(back[1], codes[1])
