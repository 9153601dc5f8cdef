"""A bandwidth (n_q) per slot and step in the streaming codec, on the GPU (encode_slots /
decode_slots with n_q, the fused quantizer of csrc/stream_rvq.hip, the variable-bandwidth packets).

The reference in every comparison is the path that exists without the feature: ops.rvq_encode /
ops.rvq_decode layer by layer, StreamEncoder / StreamDecoder steps without n_q, StreamPacker with a
fixed K. Code k depends only on layers < k, so the codes a slot must produce at n_q = k are rows
[:k] of the codes at the session's K_max with zeros below, and its wave is that of a decoder built
for k codebooks: all torch.equal. The one anchor outside bit-equality (a stream that changes
bandwidth against the offline decoder) uses the offline wave bound of test_gpu_stream.py, 1e-3.

The model is test_gpu_stream.build(1, 1) (24 kHz causal, 32 codebooks), sessions have K_max = 8,
clips are 27 frames."""
import pytest
import torch

from fixtures import T
from synth import synth_wave
from test_gpu_stream import build, rel, DEV, HOP, FRAMES
from test_gpu_stream_slots import RUN1

pytestmark = pytest.mark.gpu
KMAX = 8


def embeds_of(m, K):
    return [l._codebook.embed for l in m.quantizer.vq.layers[:K]]


def tables(counts, nq):
    slots = torch.tensor([(c, 0) for c in counts], dtype=torch.int32, device=DEV)
    return slots, torch.tensor(list(nq), dtype=torch.int32, device=DEV)


def masked(codes, counts, nq):
    """codes [B, K, n] with rows >= nq[b] and columns >= counts[b] zeroed."""
    out = codes.clone()
    for b, (c, q) in enumerate(zip(counts, nq)):
        out[b, q:] = 0
        out[b, :, c:] = 0
    return out


@pytest.fixture(scope='module')
def ctx():
    m, cfg, p, cbs = build(1, 1)
    ns = type('Ctx', (), {})()
    ns.m = m
    ns.x = T(synth_wave((3, 1, FRAMES * HOP), 4351))
    ns.clips = [ns.x[b:b + 1] for b in range(3)]
    return ns


# ---------------------------------------------------------------- 1. the kernels alone
def shape_case(B, n, K):
    nq = [(3, K, 1)[b % 3] for b in range(B)] if B > 1 else [K]
    counts = [(n - b) % (n + 1) for b in range(B)]
    if B == 3:
        counts[2] = 0
    return counts, nq


@pytest.mark.parametrize('B, n, K', [(1, 1, KMAX), (3, 7, KMAX), (64, 8, KMAX), (2, 7, 32)])
def test_fused_kernels_equal_the_per_layer_kernels(ctx, B, n, K):
    from encx import ops
    embeds = embeds_of(ctx.m, K)
    books = ops.StreamRVQBooks(embeds)
    counts, nq = shape_case(B, n, K)
    assert B < 3 or (0 in counts and {1, 3, K} <= set(nq))
    slots, nqt = tables(counts, nq)
    g = torch.Generator().manual_seed(100 * B + n)
    scale = float(embeds[0].std())
    clean = (torch.randn(B, 128, n, generator=g) * 2 * scale).to(DEV)
    # the latent as a window holds it: strided, and NaN wherever a slot does not deliver
    win = torch.full((B, 128, n + 5), float('nan'), device=DEV)
    for b, c in enumerate(counts):
        win[b, :, 3:3 + c] = clean[b, :, :c]
    codes = ops.stream_rvq_encode_slots(win[:, :, 3:3 + n], books, slots, nqt)
    ref = ops.rvq_encode(clean, embeds).permute(1, 0, 2).contiguous()  # [B, K, n]
    want = masked(ref, counts, nq)
    assert codes.shape == (B, K, n) and codes.dtype == torch.int64
    assert torch.equal(codes, want)
    assert int(want.count_nonzero()) or B == 1

    # decode: poison what must not be read (a slot's tail, its rows >= nq), one read code outside
    # the codebook (clamped, as StreamDecoder clamps today)
    cin = want.clone()
    for b, (c, q) in enumerate(zip(counts, nq)):
        cin[b, q:] = 1 << 40
        cin[b, :, c:] = -(1 << 40)
    clamped = want.clone()
    if counts[0]:
        cin[0, 0, 0], clamped[0, 0, 0] = 5000, 1023
    out = torch.full((B, 128, n + 5), float('nan'), device=DEV)
    ops.stream_rvq_decode_slots(cin, books, slots, nqt, out[:, :, 3:3 + n])
    assert bool(out[:, :, :3].isnan().all()) and bool(out[:, :, 3 + n:].isnan().all())
    got = out[:, :, 3:3 + n]
    for k in sorted(set(nq)):
        q = ops.rvq_decode(clamped[:, :k].permute(1, 0, 2).contiguous(), embeds[:k])
        for b in range(B):
            if nq[b] == k:
                assert torch.equal(got[b, :, :counts[b]], q[b, :, :counts[b]]), (b, k)
                assert not got[b, :, counts[b]:].any(), b


def test_equidistant_codes_go_to_the_lower_index(ctx):
    from encx import ops
    embeds = [e.clone() for e in embeds_of(ctx.m, 2)]
    embeds[0][700] = embeds[0][5]  # a duplicated row: codes 5 and 700 are exactly equidistant
    books = ops.StreamRVQBooks(embeds)
    x = torch.stack([embeds[0][5], embeds[0][5] * 1.001], 1).unsqueeze(0).contiguous()  # [1, D, 2]
    slots, nqt = tables([2], [2])
    codes = ops.stream_rvq_encode_slots(x, books, slots, nqt)
    ref = ops.rvq_encode(x, embeds).permute(1, 0, 2)
    assert torch.equal(codes, ref)
    assert codes[0, 0].tolist() == [5, 5]


# ---------------------------------------------------------------- sessions
def drive(m, clips, schedule, nqs, graphs=True, kmax=KMAX):
    """A session of len(clips) slots over `schedule` (frames per step); nqs: the n_q of every step,
    or None for the path without n_q. -> per slot (codes [1, K, T], wave [1, C, T * HOP]) of its
    own columns, and the sessions."""
    from encx.streaming import StreamEncoder, StreamDecoder
    B = len(clips)
    enc = StreamEncoder(m, B, graphs=graphs, n_q=kmax)
    dec = StreamDecoder(m, B, kmax, graphs=graphs)
    off = [0] * B
    got = [([], []) for _ in range(B)]
    for i, frames in enumerate(schedule):
        n = max(frames)
        x = torch.full((B, m.channels, n * HOP), float('nan'))
        for b, f in enumerate(frames):
            if f:
                x[b, :, :f * HOP] = clips[b][0, :, off[b] * HOP:(off[b] + f) * HOP]
        nq = None if nqs is None else nqs[i]
        codes = enc.encode_slots(x.to(DEV), frames, n_q=nq)
        assert codes.shape == (B, kmax, n) and codes.dtype == torch.int64
        cin = codes.clone()
        for b, f in enumerate(frames):  # what the decoder must not read
            cin[b, :, f:] = 1 << 40
            if nq is not None and f:
                cin[b, nq[b]:] = -(1 << 40)
        y = dec.decode_slots(cin, frames, n_q=nq)
        assert y.shape == (B, m.channels, n * HOP) and bool(torch.isfinite(y).all())
        for b, f in enumerate(frames):
            assert not codes[b, :, f:].any() and not y[b, :, f * HOP:].any()
            if f:
                assert nq is None or not codes[b, nq[b]:].any()
                got[b][0].append(codes[b:b + 1, :, :f])
                got[b][1].append(y[b:b + 1, :, :f * HOP])
                off[b] += f
    return [(torch.cat(c, 2), torch.cat(y, 2)) if c else None for c, y in got], enc, dec


def solo(m, clip, chunks, k):
    """The clip streamed alone through a session built for k codebooks, on the path without n_q."""
    out, _, _ = drive(m, [clip[:, :, :sum(chunks) * HOP]], [(f,) for f in chunks], None, kmax=k)
    return out[0]


@pytest.fixture(scope='module')
def run1(ctx):
    """RUN1 at constant n_q (1, 3, 8), and the parent's codes at K_max on the same schedule."""
    nq = (1, 3, 8)
    got, enc, dec = drive(ctx.m, ctx.clips, RUN1, [nq] * len(RUN1))
    parent, _, _ = drive(ctx.m, ctx.clips, RUN1, None)
    return nq, got, parent, enc, dec


def test_session_at_constant_per_slot_n_q(ctx, run1):
    nq, got, parent, enc, dec = run1
    for b, k in enumerate(nq):
        codes, wave = got[b]
        want = parent[b][0].clone()
        want[:, k:] = 0
        assert codes.shape == (1, KMAX, FRAMES) and torch.equal(codes, want), b
        s_codes, s_wave = solo(ctx.m, ctx.clips[b], [f[b] for f in RUN1 if f[b]], k)
        assert torch.equal(codes[:, :k], s_codes), b
        assert torch.equal(wave, s_wave), b
    # keyed apart from the graphs of the path without n_q
    assert not enc._s.graph_keys('slots') and not dec._s.graph_keys('slots')
    assert enc._s.graph_keys('nq') and dec._s.graph_keys('nq')


def test_bandwidth_change_mid_stream(ctx):
    """Slot 0 goes 8 -> 2 -> 8 -> 1 while slot 1 joins and slot 2 sits out."""
    from encx import ops
    m = ctx.m
    schedule = ((7, 0, 0), (3, 7, 0), (8, 1, 0), (2, 8, 0))
    nqs = ((8, 0, 0), (2, 3, 0), (8, 3, 7), (1, 5, 'idle'))
    got, _, _ = drive(m, ctx.clips, schedule, nqs)
    assert got[2] is None
    chunks, ks = [f[0] for f in schedule], [q[0] for q in nqs]
    alone, _, _ = drive(m, ctx.clips[:1], [(f,) for f in chunks], [(k,) for k in ks])
    codes, wave = got[0]
    assert torch.equal(codes, alone[0][0]) and torch.equal(wave, alone[0][1])
    parent = solo(m, ctx.clips[0], chunks, KMAX)[0]
    want, segs, off = parent.clone(), [], 0
    embeds = embeds_of(m, KMAX)
    for f, k in zip(chunks, ks):
        want[:, k:, off:off + f] = 0
        segs.append(ops.rvq_decode(parent[:, :k, off:off + f].permute(1, 0, 2).contiguous(), embeds[:k]))
        off += f
    assert torch.equal(codes, want)
    with torch.no_grad():
        y_off = m.decoder(torch.cat(segs, 2))
    r = rel(wave, y_off)
    print(f'bandwidth change 8 -> 2 -> 8 -> 1: wave rel {r:.3e} vs the offline decoder')
    assert r < 1e-3, r
    # slot 1 joined at 3 codebooks and moved to 5
    want1 = solo(m, ctx.clips[1], [7, 1, 8], KMAX)[0].clone()
    want1[:, 3:, :8] = 0
    want1[:, 5:, 8:] = 0
    assert torch.equal(got[1][0], want1)


def test_graph_replay_reads_the_nq_table_on_the_device(ctx):
    """(3, 3, 3) runs three times: the capture, then two replays under other nq tables."""
    schedule = ((7, 7, 7), (3, 3, 3), (3, 3, 3), (3, 3, 3))
    nqs = ((8, 8, 8), (1, 3, 8), (8, 2, 5), (4, 8, 1))
    eager, e_enc, _ = drive(ctx.m, ctx.clips, schedule, nqs, graphs=False)
    graph, g_enc, g_dec = drive(ctx.m, ctx.clips, schedule, nqs)
    assert not e_enc._s.graph_keys('nq')
    assert g_enc._s.graph_keys('nq') == [(3, False, False), (7, True, False)]
    assert g_dec._s.graph_keys('nq') == [(3, False), (7, True)]
    for b in range(3):
        assert torch.equal(graph[b][0], eager[b][0]) and torch.equal(graph[b][1], eager[b][1]), b
        assert int(graph[b][0][:, :, 10:13].count_nonzero())


# ---------------------------------------------------------------- 5. packets
def test_variable_bandwidth_packets(ctx):
    from encx.streaming import StreamPacker, StreamUnpacker
    m, B, n = ctx.m, 4, 7
    frames, nq = [7, 0, 3, 1], [8, 5, 1, 3]
    g = torch.Generator().manual_seed(7)
    codes = torch.randint(0, 1024, (B, KMAX, n), generator=g).to(DEV)
    want = masked(codes, frames, [8, 0, 1, 3])
    poisoned = codes.clone()
    for b, (f, q) in enumerate(zip(frames, nq)):
        poisoned[b, :, f:] = 1 << 40
        poisoned[b, q:] = 1 << 40     # a code >= 2^bits in a row k >= n_q[b] is not read
    packer = StreamPacker(m, B, KMAX, slot_n_q=True)
    unpacker = StreamUnpacker(m, B, KMAX, slot_n_q=True)
    packets = packer.pack_slots(poisoned, frames, nq)
    assert packets[1] == b''
    for K in (8, 1, 3):
        old = StreamPacker(m, B, K).pack_slots(codes[:, :K], frames)
        for b in range(B):
            if frames[b] and nq[b] == K:
                assert packets[b] == bytes([frames[b], K]) + old[b][1:], b
    got, fr, q = unpacker.unpack_slots(packets)
    assert fr == frames and q == [8, 0, 1, 3]
    assert got.shape == (B, KMAX, n) and torch.equal(got, want)
    bad = codes.clone()
    bad[2, 0, 2] = 1024           # delivered: row 0 < n_q 1, column 2 < 3 frames
    with pytest.raises(ValueError, match='does not fit'):
        packer.pack_slots(bad, frames, nq)
    assert packer.pack_slots(poisoned, frames, nq) == packets
    # the unpacker's refusals are host checks
    p0 = packets[0]
    for broken in (bytes([7, 0]) + p0[2:], bytes([7, 9]) + p0[2:], p0[:-1], p0 + b'\0', bytes([7, 7]) + p0[2:],
                   bytes([9, 8]) + p0[2:], p0[:1]):
        with pytest.raises(ValueError):
            unpacker.unpack_slots([broken] + packets[1:])
    with pytest.raises(ValueError):
        packer.pack_slots(codes, frames)            # slot_n_q=True needs n_q
    with pytest.raises(ValueError):
        StreamPacker(m, B, KMAX).pack_slots(codes, frames, nq)


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_session_untouched(ctx):
    from encx.streaming import StreamEncoder, StreamDecoder, StreamPacker, StreamUnpacker
    m = ctx.m
    enc, dec = StreamEncoder(m, 2, n_q=KMAX), StreamDecoder(m, 2, KMAX)
    x = ctx.x[:2, :, :8 * HOP].to(DEV)
    codes = enc.encode_slots(x[:, :, :7 * HOP], [7, 0], n_q=[8, 0])
    dec.decode_slots(codes, [7, 0], n_q=[8, 0])
    torch.cuda.synchronize()
    state = [(s._arena.clone(), s._slots.clone(), s._nq.clone()) for s in (enc._s, dec._s)]
    c8 = torch.zeros(2, KMAX, 8, device=DEV, dtype=torch.int64)
    for frames, n, nq in (((1, 0), 1, (8,)), ((1, 0), 1, (8, 8, 8)),     # wrong length
                          ((1, 0), 1, (0, 8)), ((1, 0), 1, (9, 8)),      # outside 1..K_max
                          ((1, 0), 1, (2.5, 8)), ((1, 0), 1, 8),         # not ints
                          ((1, 3), 3, (8, 8)),                           # slot 1's first chunk is too short
                          ((0, 0), 1, (8, 8))):                          # nobody delivers
        with pytest.raises(ValueError):
            enc.encode_slots(x[:, :, :n * HOP], frames, n_q=nq)
        with pytest.raises(ValueError):
            dec.decode_slots(c8[:, :, :n], frames, n_q=nq)
    with pytest.raises(ValueError):
        enc.n_q_for(12.0)
    assert [enc.n_q_for(bw) for bw in (1.5, 3.0, 6.0)] == [2, 4, 8]
    with pytest.raises(ValueError):
        StreamEncoder(m, 2, n_q=33)
    torch.cuda.synchronize()
    for s, (a, t, q) in zip((enc._s, dec._s), state):
        assert torch.equal(s._arena, a) and torch.equal(s._slots, t) and torch.equal(s._nq, q)
        assert s.started == [True, False]
    for cls in (StreamPacker, StreamUnpacker):
        with pytest.raises(NotImplementedError):
            cls(m, 2, KMAX, use_lm=True, slot_n_q=True)
    # and the session goes on
    codes = enc.encode_slots(x[:, :, :7 * HOP], [1, 7], n_q=[2, 8])
    assert int(codes[0, :2, :1].count_nonzero()) and not codes[0, 2:].any()


def test_a_codebook_shape_the_fused_kernel_does_not_take_still_streams(ctx):
    """1001 bins: the per-layer kernels take them, the fused quantizer does not (bins % 4). The
    session is built and streams without n_q as ever; only a step that passes n_q is refused, on
    the host, with the session untouched."""
    import copy
    from encx import ops
    from encx.streaming import StreamEncoder, StreamDecoder
    m = copy.deepcopy(ctx.m)
    for l in m.quantizer.vq.layers:
        l._codebook.embed = l._codebook.embed[:1001].clone()
    m.quantizer.bins = 1001
    enc, dec = StreamEncoder(m, 2, n_q=KMAX), StreamDecoder(m, 2, KMAX)
    assert enc._books is None and dec._books is None
    x = ctx.x[:2, :, :7 * HOP].to(DEV)
    codes, emb = enc.encode_slots(x, [7, 7], return_latent=True)
    assert torch.equal(codes, ops.rvq_encode(emb, embeds_of(m, KMAX)).permute(1, 0, 2))
    assert int(codes.max()) <= 1000 and int(codes.count_nonzero())
    y = dec.decode_slots(codes, [7, 7])
    torch.cuda.synchronize()
    state = [s._arena.clone() for s in (enc._s, dec._s)]
    x1 = ctx.x[:2, :, 7 * HOP:8 * HOP].to(DEV)
    with pytest.raises(NotImplementedError, match='per-slot n_q'):
        enc.encode_slots(x1, [1, 1], n_q=[8, 2])
    with pytest.raises(NotImplementedError, match='per-slot n_q'):
        dec.decode_slots(codes[:, :, :1], [1, 1], n_q=[8, 2])
    torch.cuda.synchronize()
    assert all(torch.equal(s._arena, a) for s, a in zip((enc._s, dec._s), state))
    enc.refresh_weights(), dec.refresh_weights()
    c1 = enc.encode(x1)
    assert c1.shape == (2, KMAX, 1) and dec.decode(c1).shape == (2, 1, HOP) and bool(torch.isfinite(y).all())


# ---------------------------------------------------------------- 7. the path without n_q
def test_steps_without_n_q_are_not_disturbed(ctx):
    """Two steps without n_q in a fresh session; the same second step after a per-slot step (at
    the full count, so that the decoder carries the same state) in another."""
    from encx.streaming import StreamEncoder, StreamDecoder
    m, x = ctx.m, ctx.x[:2].to(DEV)
    a, b = x[:, :, :7 * HOP], x[:, :, 7 * HOP:10 * HOP]
    enc0, dec0 = StreamEncoder(m, 2, n_q=KMAX), StreamDecoder(m, 2, KMAX)
    c0, e0 = enc0.encode_slots(a, [7, 7], return_latent=True)
    y0 = dec0.decode_slots(c0, [7, 7])
    c1, e1 = enc0.encode_slots(b, [3, 2], return_latent=True)
    y1 = dec0.decode_slots(c1, [3, 2])
    enc, dec = StreamEncoder(m, 2, n_q=KMAX), StreamDecoder(m, 2, KMAX)
    cq, eq = enc.encode_slots(a, [7, 7], return_latent=True, n_q=[KMAX, KMAX])
    yq = dec.decode_slots(cq, [7, 7], n_q=[KMAX, KMAX])
    assert torch.equal(cq, c0) and torch.equal(eq, e0) and torch.equal(yq, y0)
    c2, e2 = enc.encode_slots(b, [3, 2], return_latent=True)
    y2 = dec.decode_slots(c2, [3, 2])
    assert torch.equal(c2, c1) and torch.equal(e2, e1) and torch.equal(y2, y1)
    assert enc._s.graph_keys('slots') == [(3, False)] and enc0._s.graph_keys('slots') == [(3, False), (7, True)]
