"""LM-coded packets with a codebook count per slot and step, on the GPU (packet format 2 of
include/encx.h: encx_lm_heads_slots, encx_lm_input_slots_nq / encx_lm_slots_advance_nq,
encx_ac_encode_slots_nq / encx_ac_decode_slots_nq; encx/lm.py LMStreamEncoder / LMStreamDecoder
(lm_format=2); encx/streaming.py StreamPacker / StreamUnpacker(use_lm=True, lm_format=2)).

Every comparison is == on bytes or torch.equal on integers against references outside the new
code: encx_lm_heads for the heads kernel; for a session the EXISTING linear-cache path one stream
at a time (lm._body + lm._heads with the chunk's own K, the input indices following the rule of
encx.h: 0 where the previous frame lacked the codebook) and tests/ac_short_ref.py (pinned to
oracle/ac_oracle.py by tests/test_stream_lm_nq.py) over its cdf rows. The one tolerance: the
probabilities of the real-size run against oracle/lm_oracle.lm_step, under the project's LM bound
of tests/test_lm.py (rtol 2e-4, atol 1e-6), no extra margin.

Every feed poisons what a slot does not deliver (codes +-2^40 past its count and in rows k >=
n_q[b]); the references never saw those values."""
import numpy as np
import pytest
import torch

from oracle import ac_oracle as A
from fixtures import load, g12_ac_rows
from test_lm import _lm
from test_gpu_stream import build, DEV, HOP, FRAMES
from test_gpu_stream_slots import RUN1
from test_gpu_stream_packets import POISON, LM_RUN, LM_T, one_pass_cdf
import ac_short_ref as S

pytestmark = pytest.mark.gpu

BITS, ROUNDOFF, MIN_RANGE = 24, 1e-8, 2
SENT = -7   # what the outputs of a kernel hold before it runs


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def tables(counts, nq):
    return i32([(c, 0) for c in counts]), i32(list(nq))


# ============================================================================ the heads kernel alone
def heads_both(lm, B, T, n_max, counts, nq, dstep, seed):
    """encx_lm_heads on every row, encx_lm_heads_slots under the tables on sentinel-filled outputs,
    the same x, weights and (where wanted) symbols -> the (row, k) mask and the three output pairs."""
    from encx._lib import call, lib, stream
    lm._packed()
    K, card, D = lm.n_q, lm.card, lm.dim
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, D, generator=g).to(DEV)
    sym = torch.randint(0, card, (B, K, T), generator=g)
    want = torch.zeros(B, T, K, dtype=torch.bool)
    for b in range(B):
        live = max(0, min(counts[b] - dstep, T))
        want[b, :live, :nq[b]] = True
    poisoned = torch.where(want.permute(0, 2, 1), sym, torch.full_like(sym, POISON)).to(DEV)
    poisoned[1::2] = torch.where(want.permute(0, 2, 1)[1::2].to(DEV), poisoned[1::2], -POISON)
    sym = sym.to(DEV)
    mk = lambda fill: (torch.full((B, T, K, card), float(fill), device=DEV),
                       torch.full((B, T, K, card), fill, dtype=torch.int32, device=DEV),
                       torch.full((B, T, K, 2), fill, dtype=torch.int32, device=DEV))
    ref, new = mk(0), mk(SENT)
    err = torch.zeros(2, dtype=torch.int32, device=DEV)
    work = torch.empty((int(lib.encx_lm_heads_workspace(B * T, K, card)) + 3) // 4, device=DEV)
    call('encx_lm_heads', x.data_ptr(), B, T, D, lm._lin_w.data_ptr(), lm._lin_b.data_ptr(), K, card,
         work.data_ptr(), ref[0].data_ptr(), ref[1].data_ptr(), BITS, ROUNDOFF, MIN_RANGE, sym.data_ptr(),
         *sym.stride(), ref[2].data_ptr(), err[:1].data_ptr(), stream())
    slots, nqt = tables(counts, nq)
    step = torch.tensor([dstep], dtype=torch.int64, device=DEV)
    work.fill_(float('nan'))
    call('encx_lm_heads_slots', x.data_ptr(), B, T, n_max, D, lm._lin_w.data_ptr(), lm._lin_b.data_ptr(), K, card,
         slots.data_ptr(), nqt.data_ptr(), step.data_ptr() if dstep else None, work.data_ptr(), new[0].data_ptr(),
         new[1].data_ptr(), BITS, ROUNDOFF, MIN_RANGE, poisoned.data_ptr(), *poisoned.stride(), new[2].data_ptr(),
         err[1:].data_ptr(), stream())
    assert err.tolist() == [0, 0]
    return want.to(DEV), ref, new


def check_heads(lm, B, T, n_max, counts, nq, dstep=0, seed=0):
    want, ref, new = heads_both(lm, B, T, n_max, counts, nq, dstep, seed)
    assert bool(want.any()) and (B * T == 1 or not bool(want.all()))
    for name, r, n in zip(('probas', 'cdf', 'lohi'), ref, new):
        assert torch.equal(n[want], r[want]), name              # a computed (row, k): encx_lm_heads's bits
        assert bool((n[~want] == SENT).all()), name             # a skipped one: never written


def test_heads_slots_small_shapes():
    """LM 'b' (K_max 4, card 64, D 64): (B, T) = (1, 1) and (3, 7) with ragged counts and nq, and
    the decoder's form (T = 1, the step in a device counter)."""
    lm, _, _ = _lm('b')
    check_heads(lm, 1, 1, 1, [1], [4])
    check_heads(lm, 1, 1, 1, [1], [2], seed=1)
    check_heads(lm, 3, 7, 7, [7, 3, 0], [1, 4, 2], seed=2)
    check_heads(lm, 3, 7, 8, [2, 7, 5], [3, 2, 4], seed=3)
    check_heads(lm, 3, 1, 7, [7, 2, 3], [2, 4, 3], dstep=2, seed=4)   # step 2: slot 1 is done


def test_heads_slots_column_tiles_that_straddle_codebooks():
    """card 48: the 32- and 64-column tiles straddle two codebooks, and are computed if either is
    wanted. A randomly initialised LM; only its heads are used."""
    from encx.lm import LMModel
    torch.manual_seed(48)
    lm = LMModel(4, 48, dim=64, num_heads=4, num_layers=1).to(DEV).eval()
    check_heads(lm, 3, 7, 7, [7, 3, 0], [1, 4, 3], seed=5)
    check_heads(lm, 3, 1, 7, [1, 1, 1], [3, 1, 2], seed=6)
    check_heads(lm, 24, 7, 7, [(5 * b) % 8 for b in range(24)], [1 + b % 4 for b in range(24)], seed=7)   # MFMA route


@pytest.mark.parametrize('T', (1, 8))
def test_heads_slots_real_size_both_row_routes(T):
    """(64, 1): 64 rows, the VALU kernel; (64, 8): 512 rows, the MFMA tiles. K_max 32, card 1024,
    D 200, nq cycling 1..32, ragged counts."""
    from encx.lm import LMModel
    torch.manual_seed(32)
    lm = LMModel(32, 1024, dim=200, num_layers=1).to(DEV).eval()
    counts = [(3 * b) % (T + 1) for b in range(64)]
    counts[0] = T
    check_heads(lm, 64, T, T, counts, [1 + b % 32 for b in range(64)], seed=8 + T)


# ============================================================================ the coder kernels alone
def coder_layout(card, bits, cdf, sym):
    """Slots over one g12 coder case: (frames, nq) and the (symbol, cdf row) list each slot codes.
    K_max 4; slot 0 at K_max, slot 1 at 1, slot 2 sits out, slot 3 codes zeros with range_low 0 (an
    empty payload), slot 4 at 3."""
    steps = len(sym)
    n_max = min(8, steps // 4)
    assert n_max >= 1
    plan = [(n_max, 4), (min(n_max, 5), 1), (0, 0), (min(n_max, 2), 2), (max(1, n_max // 3), 3)]
    out = []
    for b, (f, q) in enumerate(plan):
        rows = [(0 if b == 3 else int(sym[i]), cdf[i]) for i in range(f * q)]
        out.append((f, q, rows))
    return n_max, out


@pytest.mark.parametrize('case', range(8))
def test_coder_kernels_on_the_g12_cases(case):
    """Intervals and cdfs straight from the g12 coder cases, no LM: the packets are (n, K) + the
    restatement's short payload, and decode back; unread lohi / cdf entries hold garbage."""
    from encx._lib import call, lib, stream
    from encx.ac import new_decoder_state
    card, bits, pdf, cdf, sym, data, eof = g12_ac_rows(load('g12_lm.npz'))[case]
    n_max, plan = coder_layout(card, bits, cdf, sym)
    B, K = len(plan), 4
    lohi = torch.full((B, n_max, K, 2), 0x7fffffff, dtype=torch.int32)
    for b, (f, q, rows) in enumerate(plan):
        for i, (s, c) in enumerate(rows):
            lohi[b, i // q, i % q, 0] = int(c[s - 1]) if s else 0
            lohi[b, i // q, i % q, 1] = int(c[s]) - 1
    lohi = lohi.to(DEV)
    slots, nq = tables([f for f, _, _ in plan], [q for _, q, _ in plan])
    stride = 2 + int(lib.encx_ac_encode_capacity(n_max * K, bits))
    out = torch.full((B, stride), 0xAA, dtype=torch.uint8, device=DEV)
    nbytes = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    err = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    call('encx_ac_encode_slots_nq', lohi.data_ptr(), B, n_max, K, slots.data_ptr(), nq.data_ptr(), bits,
         out.data_ptr(), stride, nbytes.data_ptr(), err.data_ptr(), stream())
    host, nb = out.cpu(), nbytes.tolist()
    assert err.tolist() == [0] * B
    packets = [host[b, :nb[b]].numpy().tobytes() for b in range(B)]
    for b, (f, q, rows) in enumerate(plan):
        want = bytes([f, q]) + S.encode([s for s, _ in rows], [c for _, c in rows], bits, short=True) if f else b''
        assert packets[b] == want, (case, b)
    assert packets[3] == bytes([plan[3][0], 2]) and packets[2] == b''   # an empty payload, a slot that sits out
    # decode: one launch per frame, the step in a device counter, this frame's cdf rows on the device
    cap = stride - 2
    buf = torch.zeros(B, cap, dtype=torch.uint8)
    for b, p in enumerate(packets):
        if len(p) > 2:
            buf[b, :len(p) - 2] = torch.frombuffer(bytearray(p[2:]), dtype=torch.uint8)
    buf, lens = buf.to(DEV), torch.tensor([max(0, len(p) - 2) for p in packets], dtype=torch.int64, device=DEV)
    state, derr = new_decoder_state(B, DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    codes = torch.full((B, K, n_max), 99, dtype=torch.int64, device=DEV)
    prev = torch.full((B, K), 99, dtype=torch.int64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for t in range(n_max):
        rowsd = torch.full((B, K, card), -1, dtype=torch.int32)
        for b, (f, q, rows) in enumerate(plan):
            if t < f:
                for k in range(q):
                    rowsd[b, k] = torch.from_numpy(np.asarray(rows[t * q + k][1], dtype=np.int32))
        rowsd = rowsd.to(DEV)
        call('encx_ac_decode_slots_nq', buf.data_ptr(), cap, lens.data_ptr(), B, state.data_ptr(), rowsd.data_ptr(),
             K, card, bits, codes.data_ptr(), K * n_max, n_max, 1, n_max, step.data_ptr(), slots.data_ptr(),
             nq.data_ptr(), prev.data_ptr(), derr.data_ptr(), stream())
        call('encx_lm_step_advance', step.data_ptr(), 1, stream())
    assert derr.tolist() == [0] * B
    codes, prev = codes.cpu(), prev.cpu()
    for b, (f, q, rows) in enumerate(plan):
        if not f:
            assert bool((codes[b] == 99).all()) and bool((prev[b] == 99).all())
            continue
        got = codes[b, :q, :f].t().reshape(-1).tolist()
        assert got == [s for s, _ in rows], (case, b)
        assert not codes[b, q:, :f].any() and bool((codes[b, :, f:] == 99).all())
        assert prev[b, :q].tolist() == [s + 1 for s, _ in rows[-q:]] and not prev[b, q:].any()


# ============================================================================ sessions
def feed_nq(codes, off, frames, nq, n_max):
    """[B, K, n_max] on the device: slot b's next frames[b] columns of its first nq[b] rows, every
    other element poisoned."""
    B, K, _ = codes.shape
    x = torch.empty(B, K, n_max, dtype=torch.int64)
    for b, (f, q) in enumerate(zip(frames, nq)):
        x[b] = POISON if b % 2 else -POISON
        x[b, :q, :f] = codes[b, :q, off[b]:off[b] + f]
    return x.to(DEV)


def drive(lm, codes, schedule, nqs, graphs=True, enc=None, dec=None, off=None, cut=None):
    """Code the streams codes [B, K, T] (host) along schedule / nqs through format-2 sessions, every
    packet decoded at once -> per slot the list of (first frame, frames, K, packet, cdf rows
    [n][K][card] of the encoder)."""
    from encx.lm import LMStreamEncoder, LMStreamDecoder
    B, K, _ = codes.shape
    enc = enc or LMStreamEncoder(lm, B, K, graphs=graphs, lm_format=2)
    dec = dec or LMStreamDecoder(lm, B, K, graphs=graphs, lm_format=2)
    off = off if off is not None else [0] * B
    out = [[] for _ in range(B)]
    for frames, nq in zip(schedule, nqs):
        n = max(frames)
        x = feed_nq(codes, off, frames, nq, n)
        packets = enc.packets(x, frames, nq)
        assert [p[:2] for p in packets] == [bytes([f, q]) if f else b'' for f, q in zip(frames, nq)]
        cdf = enc.last_cdf.cpu()
        got, failed = dec.decode_slots([p[2:] for p in packets], frames, nq)
        assert failed == [] and got.shape == (B, K, n)
        for b, (f, q) in enumerate(zip(frames, nq)):
            assert torch.equal(got[b, :q, :f], x[b, :q, :f]), (b, frames, nq)
            assert not got[b, q:].any() and not got[b, :, f:].any(), (b, frames, nq)
            if f:
                out[b].append((off[b], f, q, packets[b], cdf[b, :f, :q].clone()))
                off[b] += f
    return out, enc, dec


def lm_inputs(codes, kframe):
    """The LM input indices of one stream, codes [K, T] with kframe[t] codebooks in frame t (encx.h):
    idx[k, t] = 1 + codes[k, t - 1] if frame t - 1 carried k, else 0 (and 0 at t = 0)."""
    K, Tn = codes.shape
    idx = torch.zeros(K, Tn, dtype=torch.int64)
    for t in range(1, Tn):
        q = kframe[t - 1]
        idx[:q, t] = codes[:q, t - 1] + 1
    return idx


def linear_cdfs(lm, codes, chunks):
    """The existing path for one stream, chunk by chunk: lm._body on a linear state with the
    chunk's own K, then lm._heads -> per chunk the cdf rows [n][K_c][card] (host)."""
    lm._packed()
    kframe = [q for n, q in chunks for _ in range(n)]
    idx = lm_inputs(codes[:, :len(kframe)], kframe)
    state, t0, out = lm.new_state(1, len(kframe) + 2), 0, []
    for n, q in chunks:
        ic = idx[:q, t0:t0 + n].unsqueeze(0).contiguous().to(DEV)
        x = lm._body(ic, ic.stride(), 1, q, n, False, state)
        cdf = torch.empty(1, n, q, lm.card, device=DEV, dtype=torch.int32)
        lm._heads(x, 1, n, q, cdf=cdf)
        out.append(cdf[0].cpu())
        t0 += n
    return out


def short_packet(codes, cdf, t0, n, q):
    """(n, q) + the restatement's short payload of frames [t0, t0 + n) over cdf rows [n][q][card]."""
    rows = [(t, k) for t in range(n) for k in range(q)]
    return bytes([n, q]) + S.encode([int(codes[k, t0 + t]) for t, k in rows],
                                    [cdf[t, k].numpy().astype(np.int64) for t, k in rows], BITS, short=True)


def check_against_linear(lm, codes, run):
    """Every packet of every slot of a drive() against the linear path of its own stream."""
    for b, packets in enumerate(run):
        ref = linear_cdfs(lm, codes[b], [(n, q) for _, n, q, _, _ in packets])
        for (t0, n, q, packet, cdf), want in zip(packets, ref):
            assert torch.equal(cdf, want), (b, t0, n, q)
            assert packet == short_packet(codes[b], want, t0, n, q), (b, t0, n, q)


@pytest.fixture(scope='module')
def small():
    """LM 'b' (K_max 4, card 64, past_context 5: the ring of 13 rows wraps) and three streams of 40
    frames; computed once, left unchanged."""
    ns = type('Ctx', (), {})()
    ns.lm, ns.cfg, _ = _lm('b')
    g = np.random.default_rng(23)
    ns.codes = torch.from_numpy(g.integers(0, ns.cfg.card, size=(3, 4, LM_T)))
    return ns


CONST_K = (1, 3, 4)


def test_constant_k_is_the_session_of_that_k(small):
    """Slots at k = 1, 3, 4 of K_max = 4 along LM_RUN: last_cdf[b, t, :k] is the one-pass path of a
    K = k model call over the whole stream, bit for bit; the packets are its short payloads."""
    lm, c = small.lm, small.codes
    nqs = [[q if f else 0 for f, q in zip(frames, CONST_K)] for frames in LM_RUN]
    run, enc, dec = drive(lm, c, LM_RUN, nqs)
    assert enc.R == 13 and len(dec._graphs) == 1 and sorted(enc._graphs) == sorted({max(f) for f in LM_RUN})
    for b, k in enumerate(CONST_K):
        want = torch.from_numpy(one_pass_cdf(lm, c[b:b + 1, :k].contiguous().to(DEV)))[0].to(torch.int32)   # [T][k][card]
        assert sum(n for _, n, _, _, _ in run[b]) == LM_T
        for t0, n, q, packet, cdf in run[b]:
            assert q == k and torch.equal(cdf, want[t0:t0 + n]), (b, t0)
            assert packet == short_packet(c[b], want[t0:t0 + n], t0, n, k), (b, t0)


# slot 0: 4 -> 1 -> 4 -> 2 at packet borders; slot 1 joins later at 2, then 3; slot 2 sits out, then 4
CHANGE_RUN = ((7, 0, 0), (1, 0, 0), (8, 7, 0), (3, 1, 0), (8, 8, 0), (2, 8, 7), (5, 0, 8), (0, 3, 8), (0, 8, 8))
CHANGE_NQ = ((4, 0, 0), (1, 0, 0), (1, 2, 0), (4, 2, 0), (4, 3, 0), (2, 3, 4), (2, 0, 4), (0, 3, 4), (0, 2, 4))


@pytest.fixture(scope='module')
def changing(small):
    return drive(small.lm, small.codes, CHANGE_RUN, CHANGE_NQ)


def test_changing_k_equals_the_linear_path_chunk_by_chunk(small, changing):
    run, enc, dec = changing
    assert [q for _, _, q, _, _ in run[0]] == [4, 1, 1, 4, 4, 2, 2]
    check_against_linear(small.lm, small.codes, run)


def test_graphs_equal_eager_and_replay_under_another_table(small, changing):
    run, enc, dec = changing
    # one graph per n_max on the encoder, one on the decoder: n_max = 8 was replayed under 5 tables
    assert sorted(enc._graphs) == [1, 3, 7, 8] and len(dec._graphs) == 1
    eager, e2, d2 = drive(small.lm, small.codes, CHANGE_RUN, CHANGE_NQ, graphs=False)
    assert not e2._graphs and not d2._graphs
    for b in range(3):
        assert len(eager[b]) == len(run[b])
        for p, q in zip(eager[b], run[b]):
            assert p[:4] == q[:4] and torch.equal(p[4], q[4]), (b, p[:3])
    # the same graphs again, from the start, under other tables
    for s in (enc, dec):
        s.reset()
    nq2 = [[(5 - q) if q else 0 for q in nq] for nq in CHANGE_NQ]
    again, _, _ = drive(small.lm, small.codes, CHANGE_RUN, nq2, enc=enc, dec=dec)
    assert sorted(enc._graphs) == [1, 3, 7, 8]
    check_against_linear(small.lm, small.codes, again)


def test_each_slot_equals_its_stream_alone(small, changing):
    run, _, _ = changing
    for b in range(3):
        sched = [((f[b],), (q[b],)) for f, q in zip(CHANGE_RUN, CHANGE_NQ) if f[b]]
        solo, _, _ = drive(small.lm, small.codes[b:b + 1], [s for s, _ in sched], [q for _, q in sched])
        assert [p[:4] for p in solo[0]] == [p[:4] for p in run[b]]


def test_restart_beside_a_continuing_neighbour(small):
    """B = 2. Slot 0: 15 frames of stream 0 at K 4 then 2, restart, stream 1 from its start at K 3
    (prev rows >= 2 were zeroed, rows < 2 hold stale codes, pos is stale: all must be ignored).
    Slot 1: stream 2 without a break."""
    lm, c = small.lm, small.codes
    out1, enc, dec = drive(lm, torch.stack([c[0], c[2]]), ((7, 7), (8, 1)), ((4, 2), (2, 2)))
    enc.restart([0])
    dec.restart([0])
    sched2, nq2 = ((1, 8), (8, 8), (8, 0), (3, 8)), ((3, 4), (3, 4), (1, 0), (4, 1))
    out2, _, _ = drive(lm, torch.stack([c[1], c[2]]), sched2, nq2, enc=enc, dec=dec, off=[0, 8])
    check_against_linear(lm, torch.stack([c[1], c[2]]), [out2[0], out1[1] + out2[1]])


def test_packet_cut_in_half(small):
    """The cut slot fails or returns other codes (format 2 cannot run dry); the other slots are
    exact in that step and after; after restart([b]) on both sides the slot round-trips again."""
    from encx.lm import LMStreamEncoder, LMStreamDecoder
    lm, c = small.lm, small.codes
    enc, dec = LMStreamEncoder(lm, 3, 4, lm_format=2), LMStreamDecoder(lm, 3, 4, lm_format=2)
    off = [0, 0, 0]

    def step(frames, nq, cut=None):
        x = feed_nq(c, off, frames, nq, max(frames))
        pay = enc.encode_slots(x, frames, nq)
        if cut is not None:
            assert len(pay[cut]) >= 2
            pay[cut] = pay[cut][:len(pay[cut]) // 2]
        got, failed = dec.decode_slots(pay, frames, nq)
        for b, (f, q) in enumerate(zip(frames, nq)):
            same = torch.equal(got[b, :q, :f], x[b, :q, :f]) and not got[b, q:].any() and not got[b, :, f:].any()
            if b == cut:
                assert failed in ([], [b]) and (not got[b].any() if failed else not same)
            else:
                assert same and b not in failed
            off[b] += f
        return failed

    assert step((7, 8, 3), (4, 3, 2)) == []
    failed = step((2, 8, 8), (4, 3, 2), cut=1)
    assert dec.failed == set(failed)
    if failed:
        with pytest.raises(ValueError, match='restart'):
            dec.decode_slots([b'', b'\0', b''], (0, 1, 0), (0, 1, 0))
    assert step((8, 0, 1), (1, 0, 4)) == [] and step((1, 0, 8), (2, 0, 4)) == []   # the others, this step and after
    enc.restart([1])
    dec.restart([1])
    off[1] = 0
    assert step((8, 8, 8), (2, 4, 4)) == [] and step((3, 1, 2), (4, 1, 3)) == [] and not dec.failed


def test_real_size_ring_wraps_and_probabilities_vs_oracle():
    """LM 'a' (dim 200, 5 layers, past_context 262), B = 2, K_max = 8, nq (8, 2) swapped to (2, 8) at
    frame 152, 300 frames in chunks of 8: the ring of 270 rows wraps. Round trip exact (drive); the
    probabilities of the last chunks (frames 256..299), [:, :, :nq[b]], against lm_oracle.lm_step
    driven chunk by chunk per stream with the zero-index rule (rtol 2e-4, atol 1e-6).
    Measured on an MI355X: the worst element is at 0.073 of that bound."""
    from oracle import lm_oracle as L
    from encx.lm import LMStreamEncoder, LMStreamDecoder
    lm, cfg, st = _lm('a')
    B, K, Tn = 2, 8, 300
    g = np.random.default_rng(29)
    codes = torch.from_numpy(g.integers(0, cfg.card, size=(B, K, Tn)))
    sched = [(8, 8)] * 37 + [(4, 4)]
    nq_at = lambda t0: (8, 2) if t0 < 152 else (2, 8)
    ref = {}
    for b in range(B):
        kframe = [nq_at(t)[b] for t in range(Tn)]
        idx = lm_inputs(codes[b], kframe)
        states, o = None, 0
        for t0 in range(0, Tn, 8):
            n, q = min(8, Tn - t0), nq_at(t0)[b]
            p, states, o = L.lm_step(st, idx[:q, t0:t0 + n].unsqueeze(0), states, o, cfg)
            if t0 >= 256:
                ref[b, t0] = p.permute(0, 3, 2, 1)[0].numpy()   # [n, q, card]
    enc, dec = LMStreamEncoder(lm, B, K, probas=True, lm_format=2), LMStreamDecoder(lm, B, K, lm_format=2)
    assert enc.R == 270
    off, worst, seen = [0, 0], 0., 0
    for frames in sched:
        t0 = off[0]
        drive(lm, codes, [frames], [nq_at(t0)], enc=enc, dec=dec, off=off)
        for b in range(B):
            if (b, t0) in ref:
                q = nq_at(t0)[b]
                mine, want = enc.last_probas[b, :frames[b], :q].cpu().numpy(), ref[b, t0]
                worst = max(worst, float(np.max(np.abs(mine - want) / (1e-6 + 2e-4 * np.abs(want)))))
                print(f'slot {b} frames {t0}..: worst error / bound so far = {worst:.3f}')
                np.testing.assert_allclose(mine, want, rtol=2e-4, atol=1e-6)
                seen += 1
    assert off == [Tn, Tn] and seen == 2 * len(range(256, 300, 8))
    print(f'streamed probabilities vs lm_oracle.lm_step: worst error / bound = {worst:.3f}')


# ============================================================================ end to end
def test_end_to_end_encode_pack_bytes_unpack_decode():
    """The model of test_gpu_stream_nq.py (24 kHz causal, 32 codebooks) over run 1, nq changing every
    step: encode_slots -> pack_slots (LM, format 2) -> bytes -> unpack_slots -> decode_slots; the wave
    equals the decode of the encoder's own codes. The LM is a small random one over 32 codebooks."""
    from synth import synth_wave
    from fixtures import T
    from encx.streaming import StreamEncoder, StreamDecoder, StreamPacker, StreamUnpacker
    from encx.lm import LMModel
    m, _, _, _ = build(1, 1)
    x = T(synth_wave((3, 1, FRAMES * HOP), 4351))
    torch.manual_seed(7)
    lm = LMModel(32, 1024, dim=64, num_heads=4, num_layers=1, past_context=5).to(DEV).eval()
    enc = StreamEncoder(m, 3, n_q=32)
    dec, direct = StreamDecoder(m, 3, 32), StreamDecoder(m, 3, 32)
    packer = StreamPacker(m, 3, 32, use_lm=True, lm=lm, lm_format=2)
    unpacker = StreamUnpacker(m, 3, 32, use_lm=True, lm=lm, lm_format=2)
    cycle = (32, 2, 8, 1, 16, 4, 31)
    off = [0, 0, 0]
    for i, frames in enumerate(RUN1):
        n = max(frames)
        nq = [cycle[(i + 2 * b) % len(cycle)] for b in range(3)]
        chunk = torch.zeros(3, 1, n * HOP)
        for b, f in enumerate(frames):
            chunk[b, :, :f * HOP] = x[b, :, off[b] * HOP:(off[b] + f) * HOP]
            off[b] += f
        codes = enc.encode_slots(chunk.to(DEV), frames, n_q=nq)
        packets = [bytes(p) for p in packer.pack_slots(codes, frames, nq)]
        assert [tuple(p[:2]) if p else (0, 0) for p in packets] == [(f, q if f else 0) for f, q in zip(frames, nq)]
        back, fr, nq_back = unpacker.unpack_slots(packets)
        assert fr == list(frames) and nq_back == [q if f else 0 for f, q in zip(frames, nq)]
        assert torch.equal(back, codes)
        assert torch.equal(dec.decode_slots(back, fr, n_q=nq_back), direct.decode_slots(codes, frames, n_q=nq)), frames
    assert off == [FRAMES] * 3 and unpacker.failed == []
