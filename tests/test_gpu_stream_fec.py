"""Redundant packets (in-band FEC, raw form) and key packets (LM-coded, format 2) on the GPU.

The reference in every comparison is what exists without the feature: the variable-bandwidth
packer (StreamPacker(slot_n_q=True) / encx_bitpack_slots_nq) called on this step's codes and again
on the kept codes of the slot's previous packet, a plain StreamDecoder fed the codes directly, the
decoder's concealment, and a fresh format-2 packer for the first packet of a stream. Everything is
== on bytes and torch.equal on codes and waves.

The model is test_gpu_stream.build(1, 1) (24 kHz causal, 32 codebooks, 10 bits), sessions have
K_max = 8 and at most 4 slots, clips are 27 frames; the LM is 'b' of test_lm (K_max 4, card 64)."""
import numpy as np
import pytest
import torch

from fixtures import T
from synth import synth_wave
from test_lm import _lm
from test_gpu_stream import build, DEV, HOP, FRAMES

pytestmark = pytest.mark.gpu
KMAX, BITS, POISON = 8, 10, 1 << 40


@pytest.fixture(scope='module')
def ctx():
    m, _, _, _ = build(1, 1)
    ns = type('Ctx', (), {})()
    ns.m = m
    ns.x = T(synth_wave((3, 1, FRAMES * HOP), 4361))
    return ns


def bp(n, bits=BITS):
    return (n * bits + 7) // 8


def poisoned(codes, frames, nq):
    """codes with everything a packer must not read replaced: columns >= frames[b], rows >= nq[b]."""
    out = codes.clone()
    for b, (f, q) in enumerate(zip(frames, nq)):
        out[b, :, f:] = POISON
        out[b, q:] = -POISON
    return out


# ---------------------------------------------------------------- 1. bytes against the parent's packer
R = 3
# per step: (frames, n_q, fec, slots restarted before the step). Slot 0 delivers every step: main
# sections that end inside a byte ((1, 1): 10 bits, (7, 3): 210 bits), copies with K_r < the
# previous K (8 -> 3), a previous K below R (1 -> K_r 1) and fec[b] capping it (step 2). Slot 1
# sits out steps 2 and 3: its packet of step 4 repeats step 1. Slot 2 has fec 0 at step 2 and is
# restarted before step 3. Slot 3 joins at step 2, where slot 1 leaves, and leaves at step 5.
FEC_RUN = (
    ((7, 7, 8, 0), (8, 3, 8, 0), None, ()),
    ((1, 2, 8, 0), (1, 8, 8, 0), None, ()),
    ((7, 0, 4, 7), (3, 0, 1, 8), (1, 3, 0, 3), ()),
    ((8, 0, 7, 1), (8, 0, 3, 2), None, (2,)),
    ((3, 1, 1, 8), (2, 1, 8, 8), (3, 2, 3, 3), ()),
    ((5, 8, 1, 0), (8, 5, 1, 0), None, ()),
)
# what the headers must say: (n_r, K_r) per slot and step, worked out by hand from the rules
FEC_COPIES = (
    ((0, 0), (0, 0), (0, 0), None),
    ((7, 3), (7, 3), (8, 3), None),
    ((1, 1), None, (0, 0), (0, 0)),
    ((7, 3), None, (0, 0), (7, 3)),
    ((8, 3), (2, 2), (7, 3), (1, 2)),
    ((3, 2), (1, 1), (1, 3), None),
)


@pytest.fixture(scope='module')
def fec_run(ctx):
    """FEC_RUN through a packer with fec=R, once: per step (codes, frames, n_q, packets)."""
    from encx.streaming import StreamPacker
    packer = StreamPacker(ctx.m, 4, KMAX, slot_n_q=True, fec=R)
    g = torch.Generator().manual_seed(11)
    steps = []
    for frames, nq, fec, restarted in FEC_RUN:
        if restarted:
            packer.restart(list(restarted))
        nq = [q if f else 0 for f, q in zip(frames, nq)]
        codes = torch.randint(0, 1 << BITS, (4, KMAX, max(frames)), generator=g).to(DEV)
        packets = packer.pack_slots(poisoned(codes, frames, nq), frames, nq, fec=fec)
        steps.append((codes, list(frames), nq, packets))
    return steps, packer


def test_packets_are_header_main_and_the_previous_packet_at_k_r(ctx, fec_run):
    from encx.streaming import StreamPacker, packet_bytes_fec
    steps, _ = fec_run
    old = StreamPacker(ctx.m, 4, KMAX, slot_n_q=True)      # the packer this change leaves untouched
    prev = [None] * 4                                      # per slot (codes [K, n], n, K) of its last packet
    for i, (codes, frames, nq, packets) in enumerate(steps):
        for b in FEC_RUN[i][3]:
            prev[b] = None
        main = old.pack_slots(codes, frames, nq)
        copies = [FEC_COPIES[i][b] or (0, 0) for b in range(4)]
        red = [b''] * 4
        if any(n_r for n_r, _ in copies):
            # the parent's packer again, on the kept codes of each slot's previous packet at K_r rows
            kept = torch.full((4, KMAX, max(n_r for n_r, _ in copies)), POISON, dtype=torch.int64, device=DEV)
            for b, (n_r, K_r) in enumerate(copies):
                if n_r:
                    pc, pn, pK = prev[b]
                    assert n_r == pn and K_r <= min(R, pK), (i, b)
                    kept[b, :K_r, :n_r] = pc[:K_r]
            red = [p[2:] for p in old.pack_slots(kept, [c[0] for c in copies], [c[1] for c in copies])]
        for b, (f, q) in enumerate(zip(frames, nq)):
            if not f:
                assert FEC_COPIES[i][b] is None and packets[b] == b'', (i, b)
                continue
            n_r, K_r = copies[b]
            assert packets[b] == bytes([f, q, n_r, K_r]) + main[b][2:] + red[b], (i, b)
            assert len(packets[b]) == packet_bytes_fec(f, q, n_r, K_r, BITS) == 4 + bp(f * q) + bp(n_r * K_r)
            prev[b] = (codes[b, :, :f].clone(), f, q)
    # the shapes the schedule is there for did occur
    sizes = {(f, q) for _, frames, nq, _ in steps for f, q in zip(frames, nq) if f}
    assert {(1, 1), (7, 3)} <= sizes and (7 * 3 * BITS) % 8 and BITS % 8


def test_round_trip_of_both_sections(ctx, fec_run):
    from encx.streaming import StreamUnpacker
    steps, _ = fec_run
    u = StreamUnpacker(ctx.m, 4, KMAX, slot_n_q=True, fec=R)
    seen = 0
    for i, (codes, frames, nq, packets) in enumerate(steps):
        got, fr, q = u.unpack_slots(packets)
        want = torch.zeros_like(codes)
        for b, (f, k) in enumerate(zip(frames, nq)):
            want[b, :k, :f] = codes[b, :k, :f]
        assert fr == frames and q == nq and torch.equal(got, want), i
        if not i:
            continue
        # every packet of this step taken as the NEXT packet of a slot whose previous one was lost
        recover = [bool(f) for f in frames]
        got, fr, q = u.unpack_slots(packets, recover)
        copies = [FEC_COPIES[i][b] or (0, 0) for b in range(4)]
        assert fr == [c[0] for c in copies] and q == [c[1] for c in copies], i
        assert got.shape == (4, KMAX, max(fr))
        for b, (n_r, K_r) in enumerate(copies):
            if n_r:
                j = max(s for s in range(i) if steps[s][1][b])      # the slot's previous delivered step
                assert torch.equal(got[b, :K_r, :n_r], steps[j][0][b, :K_r, :n_r]), (i, b)
                seen += 1
            assert not got[b, K_r:].any() and not got[b, :, n_r:].any(), (i, b)
        # a mix: slot 0's copy beside the main sections of the others
        got, fr, q = u.unpack_slots(packets, [True, False, False, False])
        assert fr[1:] == frames[1:] and q[1:] == nq[1:] and (fr[0], q[0]) == copies[0]
        for b in range(1, 4):
            assert torch.equal(got[b, :nq[b], :frames[b]], codes[b, :nq[b], :frames[b]])
    assert seen == 13


def test_a_code_that_does_not_fit_leaves_the_last_good_packet_in_the_history(ctx):
    from encx.streaming import StreamPacker, StreamUnpacker
    packer = StreamPacker(ctx.m, 2, KMAX, slot_n_q=True, fec=2)
    u = StreamUnpacker(ctx.m, 2, KMAX, slot_n_q=True, fec=2)
    g = torch.Generator().manual_seed(13)
    c = [torch.randint(0, 1 << BITS, (2, KMAX, 8), generator=g).to(DEV) for _ in range(4)]
    packer.pack_slots(c[0][:, :, :3], [3, 2], [8, 1])
    good = packer.pack_slots(c[1][:, :, :5], [5, 0], [4, 0])
    state = (list(packer._prev), list(packer._par))
    bad = c[2].clone()
    bad[0, 1, 6] = 1 << BITS        # delivered: row 1 < n_q 2, column 6 < 7 frames; it would be kept, too
    for _ in range(2):              # twice: a second refused step must not reach the good copy either
        with pytest.raises(ValueError, match='does not fit'):
            packer.pack_slots(bad[:, :, :7], [7, 1], [2, 8])
        assert (packer._prev, packer._par) == state
    nxt = packer.pack_slots(c[3][:, :, :7], [7, 1], [2, 8])
    assert tuple(nxt[0][:4]) == (7, 2, 5, 2) and tuple(nxt[1][:4]) == (1, 8, 2, 1)
    got, fr, q = u.unpack_slots(nxt, [True, True])
    assert fr == [5, 2] and q == [2, 1]
    assert torch.equal(got[0, :2, :5], c[1][0, :2, :5]) and torch.equal(got[1, :1, :2], c[0][1, :1, :2])
    # and the step before the refused one is what a fresh run of the good steps alone gives
    again = StreamPacker(ctx.m, 2, KMAX, slot_n_q=True, fec=2)
    again.pack_slots(c[0][:, :, :3], [3, 2], [8, 1])
    assert again.pack_slots(c[1][:, :, :5], [5, 0], [4, 0]) == good
    assert again.pack_slots(c[3][:, :, :7], [7, 1], [2, 8]) == nxt


# ---------------------------------------------------------------- 2. the ABI directly
def i32(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('B, K, Rr, h_max, bits, ns', [
    (3, 5, 2, 6, 7, (6, 4)),          # bits 7: no section but the empty one ends on a byte; h_max above n_max
    (64, 32, 32, 8, 10, (8, 8)),      # the stride bound: every slot full, the copy as large as the packet
    (2, 8, 3, 255, 32, (255, 1)),     # the longest packet, 32-bit codes
])
def test_entry_point_against_the_nq_packer_called_twice(B, K, Rr, h_max, bits, ns):
    from encx._lib import call, stream
    g = np.random.default_rng(B * 1000 + bits)
    stride = 4 + bp(h_max * K, bits) + bp(h_max * Rr, bits)
    hist = torch.zeros(2, B, Rr, h_max, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)

    def nq_packer(codes, n_max, frames, nq):
        """encx_bitpack_slots_nq as the parent runs it -> per slot the payload."""
        out = torch.zeros(B, 2 + bp(n_max * K, bits), dtype=torch.uint8, device=DEV)
        nb = torch.zeros(B, dtype=torch.int64, device=DEV)
        slots, nq_t = i32([(f, 0) for f in frames]), i32(nq)
        call('encx_bitpack_slots_nq', codes.data_ptr(), *codes.stride(), B, K, n_max, bits, slots.data_ptr(),
             nq_t.data_ptr(), out.data_ptr(), out.shape[1], nb.data_ptr(), err.data_ptr(), stream())
        host, nb = out.cpu().numpy(), nb.tolist()
        return [host[b, 2:nb[b]].tobytes() for b in range(B)]

    prev, par = [(0, 0, None)] * B, [0] * B
    for step, n_max in enumerate(ns):
        frames = [int(v) for v in g.integers(0, n_max + 1, B)]
        nq = [int(v) for v in g.integers(1, K + 1, B)]
        if B == 64:
            frames, nq = [n_max] * B, [K] * B
        frames[0], nq[0] = n_max, K
        if step and B == 3:
            frames[1] = 0                                        # sits out: nothing written, history kept
        codes = torch.from_numpy(g.integers(0, 1 << bits, (B, K, n_max))).to(DEV)
        fec = [(n, min(Rr, q), p, 0) for (n, q, _), p in zip(prev, par)]
        out = torch.full((B, stride), 0xAA, dtype=torch.uint8, device=DEV)
        nb = torch.full((B,), -1, dtype=torch.int64, device=DEV)
        before = hist.clone()
        src, slots, nq_t, fec_t = poisoned(codes, frames, nq), i32([(f, 0) for f in frames]), i32(nq), i32(fec)
        call('encx_bitpack_slots_fec', src.data_ptr(), *src.stride(), B, K, n_max, bits, Rr, h_max, slots.data_ptr(),
             nq_t.data_ptr(), fec_t.data_ptr(), hist.data_ptr(), out.data_ptr(), stride, nb.data_ptr(),
             err.data_ptr(), stream())
        host, nb = out.cpu().numpy(), nb.tolist()
        main = nq_packer(codes, n_max, frames, nq)
        red = [b''] * B
        if any(r[0] for r in fec):
            # the kept codes of every slot's previous packet at K_r rows, through the same packer
            m_r = max(r[0] for r in fec)
            kept = torch.full((B, K, m_r), POISON, dtype=torch.int64, device=DEV)
            for b, (n_r, K_r, _, _) in enumerate(fec):
                if n_r:
                    kept[b, :K_r, :n_r] = prev[b][2][:K_r]
            red = nq_packer(kept, m_r, [r[0] for r in fec], [r[1] for r in fec])
        for b, (f, q) in enumerate(zip(frames, nq)):
            n_r, K_r, p, _ = fec[b]
            if not f:
                assert nb[b] == 0 and (host[b] == 0xAA).all(), (step, b)
                assert torch.equal(hist[:, b], before[:, b]), (step, b)
                continue
            want = bytes([f, q, n_r, K_r]) + main[b] + red[b]
            assert nb[b] == len(want) == 4 + bp(f * q, bits) + bp(n_r * K_r, bits), (step, b)
            assert host[b, :nb[b]].tobytes() == want, (step, b)
            assert (host[b, nb[b]:] == 0xAA).all(), (step, b)       # nothing past the packet
            # the history: the copy it read is untouched, the other holds rows < min(R, K) of this step
            keep = min(Rr, q)
            assert torch.equal(hist[p, b], before[p, b]), (step, b)
            assert torch.equal(hist[p ^ 1, b, :keep, :f], codes[b, :keep, :f]), (step, b)
            prev[b], par[b] = (f, q, codes[b, :, :f].clone()), p ^ 1
    assert int(err.item()) == 0
    if B == 64:
        assert max(nb) == stride        # the bound is met exactly


# ---------------------------------------------------------------- 3. the wave
WAVE_RUN = ((7, 7, 7), (3, 1, 8), (8, 2, 1), (1, 8, 3), (8, 8, 8))
WAVE_NQ = ((8, 4, 1), (8, 8, 3), (2, 8, 8), (5, 3, 8), (8, 8, 8))
LOST_STEP, LOST_SLOT = 2, 1
WAVE_R = 1    # the test model has two codebooks that are not zero: one fewer is another wave


@pytest.fixture(scope='module')
def sent(ctx):
    """The sender's side of WAVE_RUN, once: per step the codes and the redundant packets (R = WAVE_R), and
    the wave of a receiver that loses nothing."""
    from encx.streaming import StreamEncoder, StreamDecoder, StreamPacker
    m = ctx.m
    enc = StreamEncoder(m, 3, n_q=KMAX)
    packer = StreamPacker(m, 3, KMAX, slot_n_q=True, fec=WAVE_R)
    clean = StreamDecoder(m, 3, KMAX)
    off, steps = [0] * 3, []
    for frames, nq in zip(WAVE_RUN, WAVE_NQ):
        chunk = torch.zeros(3, 1, max(frames) * HOP)
        for b, f in enumerate(frames):
            chunk[b, :, :f * HOP] = ctx.x[b, :, off[b] * HOP:(off[b] + f) * HOP]
            off[b] += f
        codes = enc.encode_slots(chunk.to(DEV), frames, n_q=nq)
        packets = packer.pack_slots(codes, frames, list(nq))
        steps.append((codes, packets, clean.decode_slots(codes, frames, n_q=nq)))
    return steps


def receive(ctx, sent, with_ahead):
    """A StreamReceiver over the packets with LOST_SLOT's packet of LOST_STEP gone -> waves, statuses."""
    from encx.streaming import StreamReceiver, StreamDecoder, StreamUnpacker
    rx = StreamReceiver(StreamDecoder(ctx.m, 3, KMAX), StreamUnpacker(ctx.m, 3, KMAX, slot_n_q=True, fec=WAVE_R))
    waves, statuses = [], []
    for i, (_, packets, _) in enumerate(sent):
        packets, ahead = list(packets), [None] * 3
        if i == LOST_STEP:
            packets[LOST_SLOT] = None
            if with_ahead:
                ahead = list(sent[i + 1][1])    # the jitter buffer holds the next step; only the lost slot's is used
        wav, status = rx.step(packets, ahead, [0 if p is not None else WAVE_RUN[i][b] for b, p in enumerate(packets)])
        waves.append(wav)
        statuses.append(status)
    return waves, statuses


def test_a_lost_step_is_decoded_from_the_next_packet_at_k_r(ctx, sent):
    from encx.streaming import StreamDecoder
    waves, statuses = receive(ctx, sent, True)
    assert statuses == [['main'] * 3 if i != LOST_STEP else ['main', 'recovered', 'main'] for i in range(len(sent))]
    n_r, K_r = sent[LOST_STEP + 1][1][LOST_SLOT][2:4]
    assert (n_r, K_r) == (WAVE_RUN[LOST_STEP][LOST_SLOT], WAVE_R) and K_r < WAVE_NQ[LOST_STEP][LOST_SLOT]
    ref = StreamDecoder(ctx.m, 3, KMAX)     # a plain decoder fed the codes, the lost step at n_q = K_r
    for i, (codes, _, clean) in enumerate(sent):
        nq = list(WAVE_NQ[i])
        if i == LOST_STEP:
            nq[LOST_SLOT] = K_r
        assert torch.equal(waves[i], ref.decode_slots(codes, WAVE_RUN[i], n_q=nq)), i
        for b in range(3):
            if b != LOST_SLOT:
                assert torch.equal(waves[i][b], clean[b]), (i, b)      # the neighbours never notice
    # fewer codebooks is another wave: the recovered step is not the clean one
    assert not torch.equal(waves[LOST_STEP][LOST_SLOT], sent[LOST_STEP][2][LOST_SLOT])


def test_without_the_next_packet_the_step_is_concealed_as_before(ctx, sent):
    from encx.streaming import StreamDecoder
    waves, statuses = receive(ctx, sent, False)
    assert statuses[LOST_STEP] == ['main', 'concealed', 'main']
    ref = StreamDecoder(ctx.m, 3, KMAX)
    for i, (codes, _, clean) in enumerate(sent):
        lost = [i == LOST_STEP and b == LOST_SLOT for b in range(3)]
        assert torch.equal(waves[i], ref.decode_slots(codes, WAVE_RUN[i], n_q=WAVE_NQ[i], lost=lost)), i
        for b in range(3):
            if b != LOST_SLOT:
                assert torch.equal(waves[i][b], clean[b]), (i, b)


# ---------------------------------------------------------------- 4. key packets
KEY_RUN = ((7, 2), (1, 8), (3, 0), (8, 1), (2, 2), (5, 3), (1, 1), (4, 4))
KEY_NQ = ((4, 2), (4, 3), (1, 0), (4, 4), (2, 4), (4, 1), (3, 4), (4, 4))
# key_interval 3: every third delivered packet of a slot, its first included (slot 1 sits step 2 out)
KEY_AT = ((1, 1), (0, 0), (0, 0), (1, 0), (0, 1), (0, 0), (1, 0), (0, 1))
KEY = 0x80


@pytest.fixture(scope='module')
def keyed(ctx):
    """KEY_RUN through a format-2 packer with key_interval=3, once: per step (codes, n_q, packets)."""
    from encx.streaming import StreamPacker
    ns = type('Ctx', (), {})()
    ns.lm, cfg, _ = _lm('b')
    ns.args = dict(use_lm=True, lm=ns.lm, lm_format=2)
    packer = StreamPacker(ctx.m, 2, 4, key_interval=3, **ns.args)
    g = torch.Generator().manual_seed(17)
    ns.steps = []
    for frames, nq in zip(KEY_RUN, KEY_NQ):
        codes = torch.randint(0, cfg.card, (2, 4, max(frames)), generator=g).to(DEV)
        for b, (f, q) in enumerate(zip(frames, nq)):    # what the LM path zeroes or ignores
            codes[b, q:] = 0
            codes[b, :, f:] = 0
        ns.steps.append((codes, list(nq), packer.pack_slots(codes, frames, list(nq))))
    return ns


def flags(packets):
    return tuple(int(bool(p) and bool(p[1] & KEY)) for p in packets)


def unflag(p):
    return p[:1] + bytes([p[1] & ~KEY & 0xff]) + p[2:]


def check_sent(got, fr, q, codes, frames, nq, slots):
    for b in slots:
        assert (fr[b], q[b]) == (frames[b], nq[b] if frames[b] else 0), b
        assert torch.equal(got[b, :, :frames[b]], codes[b, :, :frames[b]]), b


def test_key_packets_are_first_packets_and_need_no_restart(ctx, keyed):
    from encx.streaming import StreamPacker, StreamUnpacker
    fresh = StreamPacker(ctx.m, 2, 4, **keyed.args)
    u = StreamUnpacker(ctx.m, 2, 4, **keyed.args)
    carried = False
    for i, (codes, nq, packets) in enumerate(keyed.steps):
        frames = KEY_RUN[i]
        assert flags(packets) == KEY_AT[i], i
        assert [tuple(unflag(p)[:2]) if p else (0, 0) for p in packets] == [(f, q if f else 0) for f, q in zip(frames, nq)]
        fresh.reset()
        first = fresh.pack_slots(codes, frames, nq)
        for b, is_key in enumerate(KEY_AT[i]):
            if is_key:
                assert unflag(packets[b]) == first[b], (i, b)
            elif packets[b]:
                carried |= packets[b] != first[b]
        got, fr, q = u.unpack_slots(packets)        # the receiver follows every restart by itself
        check_sent(got, fr, q, codes, frames, nq, (0, 1))
    assert u.failed == []
    assert carried    # between key packets the context is kept: some unflagged packet is no first packet


@pytest.mark.parametrize('corrupt', (False, True))
def test_a_loss_heals_at_the_next_key_packet(ctx, keyed, corrupt):
    """Slot 0 loses its packet 1 (corrupt: it arrives damaged instead, and the transport's checksum
    says so; format 2 cannot tell by itself unless no interval holds the value). Packet 2 is dropped
    unread, packet 3 is a key packet: from there on the codes are the sender's, with no restart
    call on either side. Slot 1 is exact throughout."""
    from encx.streaming import StreamUnpacker
    u = StreamUnpacker(ctx.m, 2, 4, **keyed.args)
    for i, (codes, nq, packets) in enumerate(keyed.steps):
        frames, packets = KEY_RUN[i], list(packets)
        if i == 1:
            if corrupt:
                damaged = packets[0][:2] + bytes(b ^ 0x5a for b in packets[0][2:])
                got, fr, q = u.unpack_slots([damaged, packets[1]])
                check_sent(got, fr, q, codes, frames, nq, (1,))
            u.lose([0])
            assert u.failed == [0]
            if corrupt:
                continue
            packets[0] = b''
        got, fr, q = u.unpack_slots(packets)
        check_sent(got, fr, q, codes, frames, nq, (1,))
        if i in (1, 2):
            assert (fr[0], q[0]) == (0, 0) and not got[0].any(), i
            assert u.failed == [0]
        else:
            check_sent(got, fr, q, codes, frames, nq, (0,))
            assert u.failed == []


def test_a_packer_that_never_keys_sends_what_it_always_sent(ctx, keyed):
    from encx.streaming import StreamPacker
    plain = StreamPacker(ctx.m, 2, 4, **keyed.args)
    never = StreamPacker(ctx.m, 2, 4, **keyed.args)
    named = StreamPacker(ctx.m, 2, 4, **keyed.args)
    for i, (codes, nq, _) in enumerate(keyed.steps):
        want = plain.pack_slots(codes, KEY_RUN[i], nq)
        assert never.pack_slots(codes, KEY_RUN[i], nq, key=[False, False]) == want
        assert flags(want) == (0, 0)
        # key=[...] alone: the named slot's packet is a first packet, the other slot's is untouched
        got = named.pack_slots(codes, KEY_RUN[i], nq, key=[i == 4, False])
        assert flags(got) == (int(i == 4), 0) and got[1] == want[1], i
        if i < 4:
            assert got[0] == want[0]
    assert never._sent == [0, 0] and not never._owed
