"""Loss concealment of the streaming decoder on the GPU (decode_slots with `lost`, StreamUnpacker.lose).

A lost slot decodes its last latent frame again, which is, bit for bit, decoding its last delivered
code column again; the output fades under the integer rule of encx/streaming.py. So everything is
torch.equal against a decoder that is simply FED the repeated column (and, for the fade, that wave
times the gains of a per-sample Python loop of the rule, multiplied on the device). The one anchor
outside the project's own rule is the offline decoder on the repeated codes, within
test_gpu_stream.py's wave bound (1e-3), no extra margin.

The model is test_gpu_stream.build (24 kHz causal, hop 320, bandwidth 1.5: 2 codebooks), the clips 27
frames. Lost slots are handed codes far outside the codebook (1 << 40) and, with a per-slot n_q, 0
codebooks: neither may be used."""
import numpy as np
import pytest
import torch

from fixtures import T
from synth import synth_wave
from test_gpu_stream import build, run, rel, stream_decode, DEV, HOP, FRAMES, SCHEDULE

pytestmark = pytest.mark.gpu

OK, LOST, OUT = 'ok', 'lost', 'out'
# test 1's schedule, and one that holds every case of the fade (test 2)
S1 = ((OK, 7), (OK, 1), (LOST, 3), (OK, 8), (LOST, 1), (LOST, 2), (OK, 5))
S2 = ((OK, 7), (OK, 1), (LOST, 1), (OK, 2), (LOST, 4), (OK, 1), (OK, 1), (LOST, 2), (OK, 8))
POISON = 1 << 40


@pytest.fixture(scope='module')
def ctx():
    """The model, three clips and each clip streamed alone without loss (computed once)."""
    m, _, _, _ = build(1, 1)
    ns = type('Ctx', (), {})()
    ns.m = m
    ns.x = T(synth_wave((3, 1, FRAMES * HOP), 4331))
    ns.solo = [run(m, ns.x[b:b + 1], SCHEDULE) for b in range(3)]  # (latent, codes, wave)
    ns.codes = [s[1] for s in ns.solo]                              # [1, n_q, 27] each, on the GPU
    ns.n_q = ns.codes[0].shape[1]
    ns.base = {}
    return ns


def decoder(m, B, n_q, **kw):
    from encx.streaming import StreamDecoder
    return StreamDecoder(m, B, n_q, **kw)


def repeated(codes, sched):
    """The slot's codes with every lost span replaced by the last delivered column."""
    out, off = codes.clone(), 0
    for kind, n in sched:
        if kind == LOST:
            out[:, :, off:off + n] = out[:, :, off - 1:off]
        off += n
    return out


def drive(dec, codes, steps, n_q=None, none_ok=False):
    """steps: per step a tuple over slots of (kind, frames). A slot's timeline advances through its
    own codes whether its frames arrive or not. What a slot does not deliver is POISON. -> the wave
    of each slot, its own samples only."""
    B = len(codes)
    off, waves = [0] * B, [[] for _ in range(B)]
    for i, step in enumerate(steps):
        frames = [0 if kind == OUT else n for kind, n in step]
        lost = [kind == LOST for kind, _ in step]
        n_max = max(frames)
        cin = torch.full((B, codes[0].shape[1], n_max), POISON, dtype=torch.int64, device=DEV)
        for b, (kind, n) in enumerate(step):
            if kind == OK:
                cin[b, :, :n] = codes[b][0, :, off[b]:off[b] + n]
        if none_ok and not any(kind == OK for kind, _ in step):
            cin = None
        y = dec.decode_slots(cin, frames, lost=lost) if n_q is None else \
            dec.decode_slots(cin, frames, n_q=n_q[i], lost=lost)
        assert y.shape == (B, 1, n_max * HOP) and bool(torch.isfinite(y).all())
        for b, f in enumerate(frames):
            assert not y[b, :, f * HOP:].any(), (b, step)
            if f:
                waves[b].append(y[b:b + 1, :, :f * HOP])
                off[b] += f
    return [torch.cat(w, 2) if w else None for w in waves]


def solo_conceal(ctx, b, sched, **kw):
    dec = decoder(ctx.m, 1, ctx.n_q, **kw)
    return drive(dec, [ctx.codes[b]], [(s,) for s in sched])[0]


def held(ctx, sched):
    """Clip 0 under a schedule with the hold longer than any loss: no fade (computed once)."""
    key = tuple(sched)
    if key not in ctx.base:
        ctx.base[key] = solo_conceal(ctx, 0, sched, conceal_hold=255)
    return ctx.base[key]


def rule(sched, hold_frames, fade, recover):
    """The fade position after every sample of a schedule, by the rule one sample at a time."""
    M, hold = fade * recover * HOP, hold_frames * HOP
    p, r, out = M, 0, []
    for kind, n in sched:
        for _ in range(n * HOP if kind != OUT else 0):
            if kind == LOST:
                r += 1
                if r > hold:
                    p = max(0, p - recover)
            else:
                p = min(M, p + fade)
            out.append(p)
        if kind == OK:
            r = 0
    return np.array(out, dtype=np.int64), M


def faded(wave, pos, M):
    """wave times the rule's gains, in fp32 on the device: x where p == M, x * (float(p) * invM)."""
    p = torch.as_tensor(pos, device=DEV)
    inv = torch.tensor(np.float32(1) / np.float32(M), device=DEV, dtype=torch.float32)
    return torch.where(p == M, wave, wave * (p.to(torch.float32) * inv))


# ---------------------------------------------------------------------------- 1
def test_held_latent_equals_repeated_codes(ctx):
    assert sum(n for _, n in S1) == FRAMES
    wave = held(ctx, S1)
    rep = repeated(ctx.codes[0], S1)
    assert not torch.equal(rep, ctx.codes[0])
    plain, _ = stream_decode(ctx.m, rep, [n for _, n in S1])
    assert wave.shape == plain.shape == (1, 1, FRAMES * HOP)
    assert torch.equal(wave, plain)
    assert not torch.equal(wave, ctx.solo[0][2])  # and it is not the loss-free wave
    with torch.no_grad():
        y_off = ctx.m.decode([(rep.to(DEV), None)])
    r = rel(wave, y_off)
    print(f'concealed wave vs the offline decoder on the repeated codes: rel {r:.3e}')
    assert r < 1e-3, r


# ---------------------------------------------------------------------------- 2
@pytest.mark.parametrize('recover', (1, 2))
@pytest.mark.parametrize('sched', (S1, S2), ids=('s1', 's2'))
def test_fade(ctx, sched, recover):
    assert sum(n for _, n in sched) == FRAMES
    base = held(ctx, sched)
    pos, M = rule(sched, 1, 2, recover)
    wave = solo_conceal(ctx, 0, sched, conceal_hold=1, conceal_fade=2, conceal_recover=recover)
    assert torch.equal(wave, faded(base, pos, M))
    assert (pos < M).any() and not torch.equal(wave, base)
    if sched is not S2:
        return
    at = np.cumsum([0] + [n for _, n in sched]) * HOP  # the first sample of each step
    # the one-frame loss ends inside the hold: test 1's bits
    assert (pos[at[2]:at[3]] == M).all() and torch.equal(wave[:, :, at[2]:at[3]], base[:, :, at[2]:at[3]])
    # the four-frame loss: its last 320 samples are exactly 0 (and the held wave is not)
    assert not wave[:, :, at[5] - HOP:at[5]].any() and base[:, :, at[5] - HOP:at[5]].any()
    assert pos[at[5] - HOP - 2] > 0 or recover == 2  # with recover 1 it gets there only then
    if recover == 1:  # back at full level exactly at the end of the next step
        assert pos[at[6] - 2] == M - 2 and pos[at[6] - 1] == M
    else:             # the way up is carried over two steps
        assert pos[at[6] - 1] == M // 2 and pos[at[7] - 2] == M - 2 and pos[at[7] - 1] == M
    assert (pos[at[7]:at[7] + HOP] == M).all() and pos[at[8] - 1] < M and pos[-1] == M


# ---------------------------------------------------------------------------- 3
def test_neighbours_are_not_disturbed(ctx):
    """Slot 0 loses steps, one of them the very step of slot 1's first chunk, and fades back in
    during slot 2's; slot 2 sits out until then."""
    steps = (((OK, 7), (OUT, 0), (OUT, 0)), ((LOST, 1), (OK, 7), (OUT, 0)), ((OK, 8), (OK, 1), (OUT, 0)),
             ((LOST, 2), (OK, 8), (OUT, 0)), ((OK, 1), (OUT, 0), (OK, 7)), ((OK, 8), (OK, 3), (OK, 8)),
             ((OUT, 0), (OK, 8), (OK, 8)), ((OUT, 0), (OUT, 0), (OK, 4)))
    kw = dict(conceal_hold=1, conceal_fade=2, conceal_recover=1)
    waves = drive(decoder(ctx.m, 3, ctx.n_q, **kw), ctx.codes, steps)
    mine = [s[0] for s in steps if s[0][0] != OUT]
    pos, M = rule(mine, 1, 2, 1)
    assert (pos < M).any() and pos[16 * HOP + 1] == M and pos[18 * HOP] < M  # fading in at slot 2's first chunk
    assert torch.equal(waves[0], solo_conceal(ctx, 0, mine, **kw))
    for b in (1, 2):
        assert torch.equal(waves[b], ctx.solo[b][2]), b


# ---------------------------------------------------------------------------- 4
def test_per_slot_n_q_on_the_fused_kernel(ctx):
    """Slot 0 goes from 8 to 2 codebooks, then loses two steps (n_q 0 passed, codes POISON or None):
    the same as repeating its last column with n_q = 2. Slot 1 is not disturbed. build() leaves the
    codebooks past the second at zero, where the count could not show: a model of its own, with
    codebooks 2..7 drawn at the scale of the first."""
    g = torch.Generator().manual_seed(11)
    m, _, _, _ = build(1, 1)
    layers = m.quantizer.vq.layers
    with torch.no_grad():
        scale = float(layers[0]._codebook.embed.std())
        for layer in layers[2:8]:
            layer._codebook.embed.copy_((torch.randn(1024, 128, generator=g) * scale).to(DEV))
    ctx = type('Ctx', (), {'m': m})()
    codes = [torch.randint(0, 1024, (1, 8, FRAMES), generator=g).to(DEV) for _ in range(2)]
    steps = (((OK, 7), (OK, 7)), ((OK, 2), (OK, 1)), ((OK, 3), (OK, 8)), ((LOST, 2), (OK, 2)), ((LOST, 1), (OUT, 0)),
             ((OK, 8), (OK, 8)), ((OK, 4), (OK, 1)))
    nq = ((8, 8), (8, 4), (2, 8), (0, 3), (0, 0), (8, 5), (8, 8))
    got = drive(decoder(ctx.m, 2, 8, conceal_hold=255), codes, steps, n_q=nq, none_ok=True)
    # the reference: no loss, the column repeated, n_q = 2 in its place
    rep = [repeated(codes[0], [s[0] for s in steps]), codes[1]]
    plain_steps = tuple(tuple((OK, n) if kind == LOST else (kind, n) for kind, n in s) for s in steps)
    plain_nq = ((8, 8), (8, 4), (2, 8), (2, 3), (2, 0), (8, 5), (8, 8))
    want = drive(decoder(ctx.m, 2, 8), rep, plain_steps, n_q=plain_nq)
    for b in range(2):
        assert torch.equal(got[b], want[b]), b
    # and the codebook count matters: the held column is not that of 8 codebooks
    other = drive(decoder(ctx.m, 2, 8), rep, plain_steps, n_q=((8, 8), (8, 4), (2, 8), (8, 3), (8, 0), (8, 5), (8, 8)))
    assert not torch.equal(got[0], other[0])


# ---------------------------------------------------------------------------- 5
@pytest.mark.parametrize('fused', (False, True), ids=('layers', 'fused'))
def test_one_graph_serves_every_loss_pattern(ctx, fused):
    steps = (((OK, 7), (OK, 7)), ((LOST, 1), (OK, 1)), ((OK, 1), (LOST, 1)), ((LOST, 1), (LOST, 1)), ((OK, 1), (OK, 1)),
             ((OK, 3), (LOST, 2)))
    nq = [(2, 2)] * len(steps) if fused else None
    kw = dict(conceal_hold=0, conceal_fade=1, conceal_recover=2)
    dec = decoder(ctx.m, 2, ctx.n_q, **kw)
    got = drive(dec, ctx.codes[:2], steps, n_q=nq, none_ok=True)
    assert dec._s.graph_keys('conceal') == [(1, False, fused), (3, False, fused)]
    want = drive(decoder(ctx.m, 2, ctx.n_q, graphs=False, **kw), ctx.codes[:2], steps, n_q=nq, none_ok=True)
    for b in range(2):
        assert torch.equal(got[b], want[b]), b
        assert torch.equal(got[b], solo_conceal(ctx, b, [s[b] for s in steps], **kw)), b


# ---------------------------------------------------------------------------- 6
def test_sessions_that_never_lose_are_untouched(ctx):
    frames = ((7, 7), (1, 8), (3, 0), (8, 2))
    a, b = decoder(ctx.m, 2, ctx.n_q), decoder(ctx.m, 2, ctx.n_q)
    off = [0, 0]
    for fr in frames:
        cin = torch.zeros(2, ctx.n_q, max(fr), dtype=torch.int64, device=DEV)
        for s, f in enumerate(fr):
            cin[s, :, :f] = ctx.codes[s][0, :, off[s]:off[s] + f]
            off[s] += f
        ya, yb = a.decode_slots(cin, fr), b.decode_slots(cin, fr, lost=[False, False])
        assert torch.equal(ya, yb)
        for s, f in enumerate(fr):
            assert torch.equal(ya[s:s + 1, :, :f * HOP], ctx.solo[s][2][:, :, (off[s] - f) * HOP:off[s] * HOP])
    assert a._s.graph_keys('conceal') == [] and b._s.graph_keys('conceal') == [] and not b._dirty
    # a loss, the way back to full level, and then the old path again
    dec = decoder(ctx.m, 1, ctx.n_q, conceal_hold=0, conceal_fade=1, conceal_recover=1)
    sched = ((OK, 7), (LOST, 1), (OK, 1), (OK, 5), (OK, 1))
    codes = [ctx.codes[0]]
    w = drive(dec, codes, [(s,) for s in sched[:3]])[0]
    assert dec._p == [dec._M] and not dec._dirty and dec._s.graph_keys('conceal') == [(1, False, False)]
    assert (5, False) not in dec._s.graph_keys('slots')
    rep = repeated(ctx.codes[0], sched)
    y = dec.decode_slots(rep[:, :, 9:14], [5], lost=[False])
    assert (5, False) in dec._s.graph_keys('slots') and dec._s.graph_keys('conceal') == [(1, False, False)]
    plain, _ = stream_decode(ctx.m, rep[:, :, :14], (7, 1, 1, 5))
    assert torch.equal(y, plain[:, :, 9 * HOP:])
    pos, M = rule(sched[:3], 0, 1, 1)
    assert torch.equal(w, faded(plain[:, :, :9 * HOP], pos, M))


# ---------------------------------------------------------------------------- 7
def test_refusals_leave_the_session_untouched(ctx):
    from encx.streaming import StreamDecoder
    with pytest.raises(ValueError, match='2\\^24'):
        StreamDecoder(ctx.m, 1, ctx.n_q, conceal_fade=255, conceal_recover=255)
    with pytest.raises(ValueError, match='conceal_hold'):
        StreamDecoder(ctx.m, 1, ctx.n_q, conceal_hold=256)
    dec, twin = decoder(ctx.m, 2, ctx.n_q, conceal_hold=0), decoder(ctx.m, 2, ctx.n_q, conceal_hold=0)
    c = torch.cat(ctx.codes[:2], 0)
    first = torch.cat([c[:1, :, :7], torch.full_like(c[:1, :, :7], POISON)], 0)
    assert torch.equal(dec.decode_slots(first, [7, 0]), twin.decode_slots(first, [7, 0]))
    state = dec._s._arena.clone()
    bad = ((c[:, :, :7], [1, 7], [False, True], 'first chunk'),      # lost before its first chunk
           (c[:, :, :1], [1, 0], [False, True], '0 frames'),          # lost with nothing to conceal
           (c[:, :, :1], [1, 0], [True], 'lost for 1 slots'),         # a wrong length
           (c[:, :, :1], [1, 0], [True, False, False], 'lost for 3 slots'),
           (None, [1, 7], [True, False], 'codes may be None'),        # a delivering slot without codes
           (None, [1, 0], None, 'codes may be None'))
    for codes, frames, lost, what in bad:
        with pytest.raises(ValueError, match=what):
            dec.decode_slots(codes, frames, lost=lost)
        assert torch.equal(dec._s._arena, state) and dec._s.started == [True, False]
        assert dec._p == twin._p and dec._r == twin._r and dec._s.graph_keys('conceal') == []
    for codes, frames, lost in ((None, [2, 0], [True, False]), (c[:, :, 9:16], [1, 7], [False, False])):
        assert torch.equal(dec.decode_slots(codes, frames, lost=lost), twin.decode_slots(codes, frames, lost=lost))


# ---------------------------------------------------------------------------- 8
def test_lm_recipe_lose_conceal_restart_the_lm_only(ctx):
    from encx.lm import LMModel
    from encx.streaming import StreamPacker, StreamUnpacker, packet_frames
    m, K = ctx.m, ctx.n_q
    torch.manual_seed(5)
    m.set_lm_model(LMModel(K, 1024).to(DEV).eval())
    packer, unpacker = StreamPacker(m, 2, K, use_lm=True), StreamUnpacker(m, 2, K, use_lm=True)
    kw = dict(conceal_hold=1, conceal_fade=2, conceal_recover=1)
    dec = decoder(m, 2, K, **kw)
    off, waves = [0, 0], [[], []]

    def step(frames, drop=(), restart=()):
        if restart:
            packer.restart(list(restart))
            unpacker.restart(list(restart))
        sent = torch.zeros(2, K, max(frames), dtype=torch.int64, device=DEV)
        for b, f in enumerate(frames):
            sent[b, :, :f] = ctx.codes[b][0, :, off[b]:off[b] + f]
            off[b] += f
        packets = packer.pack_slots(sent, frames)
        arrived = [b'' if b in drop else p for b, p in enumerate(packets)]
        back, fr = unpacker.unpack_slots(arrived)
        # what the transport knows: a missing packet's frames from timing, a held one's from its header
        conceal = [f if b in drop else packet_frames(arrived[b]) for b, f in enumerate(frames)]
        lost = [fr[b] == 0 and conceal[b] > 0 for b in range(2)]
        n = max(conceal)
        cin = torch.full((2, K, n), POISON, dtype=torch.int64, device=DEV)
        cin[:, :, :back.shape[2]] = back
        y = dec.decode_slots(cin, conceal, lost=lost)
        for b, f in enumerate(conceal):
            waves[b].append(y[b:b + 1, :, :f * HOP])
        return sent, back, fr, lost

    sent, back, fr, lost = step((7, 7))
    assert fr == [7, 7] and torch.equal(back, sent) and lost == [False, False]
    # slot 0's packet does not arrive
    unpacker.lose([0])
    sent, back, fr, lost = step((2, 3), drop=(0,))
    assert fr == [0, 3] and lost == [True, False] and unpacker.failed == [0]
    assert torch.equal(back[1], sent[1]) and not back[0].any()
    # its next packet arrives, but under a context the sender does not share: dropped, concealed
    sent, back, fr, lost = step((1, 1))
    assert fr == [0, 1] and lost == [True, False] and unpacker.failed == [0]
    assert torch.equal(back[1], sent[1]) and not back[0].any()
    # the sender has learnt of it: the LM context restarts on both sides, nothing else does
    sent, back, fr, lost = step((8, 8), restart=(0,))
    assert fr == [8, 8] and lost == [False, False] and unpacker.failed == [] and torch.equal(back, sent)
    sent, back, fr, lost = step((3, 2))
    assert fr == [3, 2] and torch.equal(back, sent)
    assert dec._s.started == [True, True]
    mine = ((OK, 7), (LOST, 2), (LOST, 1), (OK, 8), (OK, 3))
    assert torch.equal(torch.cat(waves[0], 2), solo_conceal(ctx, 0, mine, **kw))
    assert torch.equal(torch.cat(waves[1], 2), ctx.solo[1][2][:, :, :21 * HOP])
