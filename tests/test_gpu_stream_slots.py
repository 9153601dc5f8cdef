"""Per-slot lifecycle of the streaming codec on the GPU (encode_slots / decode_slots / restart):
slots that join late, sit steps out, deliver ragged frame counts and are restarted must each
produce, bit for bit, what the same clip produces streamed ALONE in a session of one. That is
the project's own rule (slicing and batch never change bits), so the comparisons are torch.equal
on latents, codes and wave; the one anchor outside it (the offline model) uses the offline
bounds of test_gpu_stream.py / test_gpu_long.py (latent 1e-4, wave 1e-3), no extra margin.

The model is test_gpu_stream.build (24 kHz causal, bandwidth 1.5), the clips 27 frames.

Run 1 (B = 3), frames per step for slots (0, 1, 2):
    (7,0,0) (1,7,0) (8,0,0) (1,8,0) (2,0,0) (8,1,0) (0,3,7) (0,8,1) (0,0,8) (0,0,8) (0,0,3)
Slot 0 streams 7, 1, 8, 1, 2, 8 from step 0. Slot 1 joins with 7 while slot 0 delivers 1 and then
takes ragged counts including steps of 0; (1, 8, 0) is the roll's overlapping case next to the long
one. Slot 2 joins (again a step of n_max 7 with a first chunk) only after slot 0 has finished.
Slot 0 delivers 1 only twice, and the second time is needed for (1, 8, 0), so slot 1 sits out one
step before it joins and two more after, not two before."""
import pytest
import torch

from fixtures import T
from synth import synth_wave
from test_gpu_stream import build, run, rel, DEV, HOP, FRAMES, SCHEDULE

pytestmark = pytest.mark.gpu

RUN1 = ((7, 0, 0), (1, 7, 0), (8, 0, 0), (1, 8, 0), (2, 0, 0), (8, 1, 0), (0, 3, 7), (0, 8, 1), (0, 0, 8), (0, 0, 8),
        (0, 0, 3))
NAMES = ('latent', 'codes', 'wave')


class Drive:
    """Feeds a session of B slots step by step. feeds[b] is the list of clips [1, C, T] slot b
    streams one after the other (restart(b) moves it to the next); done[b] collects, per clip,
    the (latent, codes, wave) of the slot's own columns. Every step checks the result shapes and
    that the columns past each slot's count are zero. poison: what the slot does not deliver is
    NaN (samples) or far outside the codebook (codes) instead of zero."""

    def __init__(self, m, feeds, graphs=True, poison=False, n_q=None):
        from encx.streaming import StreamEncoder, StreamDecoder
        self.B, self.C, self.poison = len(feeds), m.channels, poison
        self.enc = StreamEncoder(m, self.B, graphs=graphs)
        self.dec = StreamDecoder(m, self.B, self.enc.n_q, graphs=graphs)
        self.feeds = [list(f) for f in feeds]
        self.off = [0] * self.B
        self.done = [[] for _ in range(self.B)]
        self.cur = [[] for _ in range(self.B)]

    def restart(self, slots):
        self.enc.restart(slots)
        self.dec.restart(slots)
        for b in slots:
            self._close(b)
            self.feeds[b].pop(0)
            self.off[b] = 0

    def _close(self, b):
        if self.cur[b]:
            self.done[b].append(tuple(torch.cat([c[i] for c in self.cur[b]], 2) for i in range(3)))
            self.cur[b] = []

    def step(self, frames):
        n = max(frames)
        x = torch.full((self.B, self.C, n * HOP), float('nan') if self.poison else 0.)
        for b, f in enumerate(frames):
            if f:
                x[b, :, :f * HOP] = self.feeds[b][0][0, :, self.off[b] * HOP:(self.off[b] + f) * HOP]
        codes, emb = self.enc.encode_slots(x.to(DEV), frames, return_latent=True)
        assert codes.shape == (self.B, self.enc.n_q, n) and codes.dtype == torch.int64 and emb.shape[2] == n
        cin = codes.clone()
        if self.poison:
            for b, f in enumerate(frames):
                cin[b, :, f:] = (1 << 40) if b % 2 else -(1 << 40)
        y = self.dec.decode_slots(cin, frames)
        assert y.shape == (self.B, self.C, n * HOP)
        assert bool(torch.isfinite(emb).all()) and bool(torch.isfinite(y).all())
        for b, f in enumerate(frames):
            assert not emb[b, :, f:].any() and not codes[b, :, f:].any() and not y[b, :, f * HOP:].any(), (b, frames)
            if f:
                self.cur[b].append((emb[b:b + 1, :, :f], codes[b:b + 1, :, :f], y[b:b + 1, :, :f * HOP]))
                self.off[b] += f
        return self

    def steps(self, schedule):
        for frames in schedule:
            self.step(frames)
        return self

    def result(self):
        for b in range(self.B):
            self._close(b)
        return self.done


def equal(got, want, frames=None):
    """got = want (a solo run), on the first `frames` frames when given, named when not."""
    for name, g, w, rate in zip(NAMES, got, want, (1, 1, HOP)):
        w = w if frames is None else w[:, :, :frames * rate]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert torch.equal(g, w), name


@pytest.fixture(scope='module')
def ctx():
    """The model, three clips, each clip streamed ALONE in a B = 1 session (computed once, left
    unchanged), and run 1 with graphs."""
    m, cfg, p, cbs = build(1, 1)
    ns = type('Ctx', (), {})()
    ns.m = m
    ns.x = T(synth_wave((3, 1, FRAMES * HOP), 4331))
    assert float(ns.x[0].abs().max()) > 0.05  # clip a is not silent: stale state would show
    ns.clips = [ns.x[b:b + 1] for b in range(3)]
    ns.solo = [run(m, c, SCHEDULE) for c in ns.clips]
    assert not torch.equal(ns.solo[0][0], ns.solo[1][0])
    ns.run1 = Drive(m, [[c] for c in ns.clips]).steps(RUN1).result()
    return ns


def test_late_join_idle_slots_and_ragged_chunks_equal_solo(ctx):
    assert [sum(f[b] for f in RUN1) for b in range(3)] == [FRAMES] * 3 and (1, 8, 0) in RUN1
    for b in range(3):
        assert len(ctx.run1[b]) == 1
        equal(ctx.run1[b][0], ctx.solo[b])


def test_restart_does_not_disturb_the_neighbour(ctx):
    """B = 2. Slot 0: clip a to the end, restart, 15 frames of clip b, restart in mid-clip, clip b
    from its start to its end. Slot 1: clip c without a break across both restarts. Encoder and
    decoder both: stale LSTM state, a stale transposed-conv column or a stale conv history of
    the previous stream would change slot 0's later runs; a disturbed neighbour, slot 1."""
    (a, b, c), solo = ctx.clips, ctx.solo
    d = Drive(ctx.m, [[a, b, b], [c]])
    d.steps(((7, 0), (8, 7), (8, 1), (4, 1)))
    d.restart([0])
    d.steps(((7, 1), (8, 2)))
    d.restart([0])
    d.steps(((7, 1), (8, 8), (8, 5), (4, 1)))
    s0, s1 = d.result()
    assert len(s0) == 3 and len(s1) == 1
    equal(s0[0], solo[0])
    equal(s0[1], solo[1], frames=15)
    equal(s0[2], solo[1])
    equal(s1[0], solo[2])


def test_unread_tail_may_hold_anything(ctx):
    """Run 1 again with NaN in every sample position and a code far outside the codebook in every
    code position past each slot's count: identical results, nothing non-finite (Drive.step)."""
    again = Drive(ctx.m, [[c] for c in ctx.clips], poison=True).steps(RUN1).result()
    for b in range(3):
        equal(again[b][0], ctx.run1[b][0])


def test_graph_equals_eager_and_one_graph_serves_both_joins(ctx):
    eager = Drive(ctx.m, [[c] for c in ctx.clips], graphs=False).steps(RUN1)
    assert not eager.enc._s.graph_keys('slots') and not eager.dec._s.graph_keys('slots')
    d = Drive(ctx.m, [[c] for c in ctx.clips])
    d.steps(RUN1[:6])  # slot 1 joined in step 1: (n_max 7, a first chunk)
    caught = [s.graph('slots', (7, True)) for s in (d.enc._s, d.dec._s)]
    keys = set(d.enc._s.graph_keys('slots'))
    d.steps(RUN1[6:])  # slot 2 joins in step 6
    for s, g in zip((d.enc._s, d.dec._s), caught):
        assert s.graph('slots', (7, True)) is g
        assert s.graph_keys('slots') == sorted({(max(f), any(f[b] and not any(e[b] for e in RUN1[:i])
                                                             for b in range(3))) for i, f in enumerate(RUN1)})
    assert keys <= set(d.enc._s.graph_keys('slots'))
    for b, (e, g) in enumerate(zip(eager.result(), d.result())):
        equal(g[0], e[0])
        equal(g[0], ctx.solo[b])  # both joins equal solo


def test_uniform_counts_equal_encode_and_decode(ctx):
    from encx.streaming import StreamEncoder, StreamDecoder
    m, x = ctx.m, ctx.x[:2].to(DEV)
    enc, twin = StreamEncoder(m, 2), StreamEncoder(m, 2)
    dec, dtwin = StreamDecoder(m, 2, enc.n_q), StreamDecoder(m, 2, enc.n_q)
    off = 0
    for n in (7, 1, 3, 8):
        chunk = x[:, :, off * HOP:(off + n) * HOP]
        c0, e0 = twin.encode(chunk, return_latent=True)
        c1, e1 = enc.encode_slots(chunk, [n] * 2, return_latent=True)
        assert torch.equal(e0, e1) and torch.equal(c0, c1), n
        assert torch.equal(dtwin.decode(c0), dec.decode_slots(c1, [n] * 2)), n
        off += n


def test_index_extremes_of_64_slots(ctx):
    """Slots 0 and 63 of 64 join at different steps, 9 frames each, while the rest sit out."""
    feeds = [[ctx.clips[0]]] + [[] for _ in range(62)] + [[ctx.clips[1]]]
    fr = lambda first, last: (first,) + (0,) * 62 + (last,)
    out = Drive(ctx.m, feeds).steps((fr(7, 0), fr(2, 7), fr(0, 2))).result()
    equal(out[0][0], ctx.solo[0], frames=9)
    equal(out[63][0], ctx.solo[1], frames=9)
    assert not any(out[1:63])


def test_stereo_model_one_join():
    """C = 2: a window's row -> slot index is row / channels."""
    m, _, _, _ = build(2, 3)
    x = T(synth_wave((2, 2, 10 * HOP), 4333))
    solo = [run(m, x[b:b + 1], (7, 3)) for b in range(2)]
    out = Drive(m, [[x[:1]], [x[1:]]]).steps(((7, 0), (1, 7), (2, 3))).result()
    for b in range(2):
        equal(out[b][0], solo[b])


def test_refusals_leave_a_live_session_usable(ctx):
    d = Drive(ctx.m, [[ctx.clips[0]], [ctx.clips[1]]])
    d.step((7, 0))
    enc, dec = d.enc, d.dec
    state = [s._arena.clone() for s in (enc._s, dec._s)]
    tables = [s._slots.clone() for s in (enc._s, dec._s)]
    x = torch.zeros(2, 1, 8 * HOP, device=DEV)
    codes = torch.zeros(2, enc.n_q, 8, device=DEV, dtype=torch.int64)
    for frames, n in (((1,), 1), ((1, 1, 1), 1),      # wrong length
                      ((9, 0), 8), ((-1, 1), 1),      # outside 0..max_frames
                      ((1, 3), 3), ((0, 6), 6),       # slot 1 has not started: 1..6 frames
                      ((0, 0), 1),                    # nobody delivers
                      ((1, 0), 2)):                   # the tensors are longer than max(frames)
        with pytest.raises(ValueError):
            enc.encode_slots(x[:, :, :n * HOP], frames)
        with pytest.raises(ValueError):
            dec.decode_slots(codes[:, :, :n], frames)
    for bad in ([2], [-1], [0, 5]):
        with pytest.raises(ValueError):
            enc.restart(bad)
        with pytest.raises(ValueError):
            dec.restart(bad)
    with pytest.raises(ValueError, match='first chunk'):
        enc.encode(x[:, :, :HOP])  # the uniform call is validated per slot: slot 1 has not started
    torch.cuda.synchronize()
    for s, a, t in zip((enc._s, dec._s), state, tables):
        assert torch.equal(s._arena, a) and torch.equal(s._slots, t) and s.started == [True, False]
    out = d.steps(((1, 7), (8, 1), (2, 0))).result()
    equal(out[0][0], ctx.solo[0], frames=18)
    equal(out[1][0], ctx.solo[1], frames=8)


def test_a_late_joiner_against_the_offline_model(ctx):
    """The anchor outside bit-equality: slot 1 of run 1 (joined in step 1, ragged counts) against
    m.encoder / m.decoder on the whole clip, under the offline bounds."""
    emb, codes, y = ctx.run1[1][0]
    with torch.no_grad():
        emb_off = ctx.m.encoder(ctx.clips[1].to(DEV))
        y_off = ctx.m.decode([(codes, None)])
    r_emb, r_y = rel(emb, emb_off), rel(y, y_off)
    print(f'late joiner: latent rel {r_emb:.3e}, wave rel {r_y:.3e} vs the offline model')
    assert r_emb < 1e-4, r_emb
    assert r_y < 1e-3, r_y


def test_roll_skips_a_row_whose_count_would_leave_it():
    """encx_stream_roll_slots over a small buffer of sentinels: a table whose count would leave
    the row (shift: n_cols + P > rstride; reflect: n_cols <= P) changes nothing and returns
    ENCX_OK; the rows of a slot with a count that fits move, so the launch is seen to act. The
    buffer is larger than the window, so even the refused addresses lie inside it."""
    from encx._lib import lib, stream, ensure_device
    ensure_device(torch.device(DEV))
    l = lib.load()
    B, C, W, P = 2, 2, 16, 4
    fresh = lambda: torch.arange(1, 1 + (B * C + 2) * W, device=DEV, dtype=torch.float32).view(B * C + 2, W)
    buf = fresh()
    tab = torch.tensor([[buf.data_ptr(), B * C, P, 0, W, 0, C, 1]], dtype=torch.int64).to(DEV)

    def roll(mode, slots):
        s = torch.tensor(slots, dtype=torch.int32).to(DEV)
        rc = l.encx_stream_roll_slots(tab.data_ptr(), 1, B * C, mode, s.data_ptr(), B, stream())
        torch.cuda.synchronize()
        return rc

    want = fresh()
    assert roll(0, [13, 0, 1 << 30, 0]) == 0 and torch.equal(buf, want)   # 13 + 4 > 16; far too many
    assert roll(1, [4, 1, 3, 1]) == 0 and torch.equal(buf, want)          # reflect needs n_cols > P
    assert roll(1, [13, 1, -1, 1]) == 0 and torch.equal(buf, want)
    assert roll(0, [12, 0, 0, 0]) == 0                                    # 12 + 4 = 16 fits: slot 0 moves
    want[:C, :P] = want[:C, 12:16]
    assert torch.equal(buf, want)
    assert roll(1, [0, 1, 5, 1]) == 0                                     # slot 1 reflects, slot 0 sits out
    want[C:2 * C, :P] = want[C:2 * C, P + 1:2 * P + 1].flip(1)
    assert torch.equal(buf, want)
    assert roll(2, [3, 0, 1, 1]) == 0                                     # zero: only the first-chunk slot
    want[C:2 * C, :P] = 0
    assert torch.equal(buf, want)


@pytest.mark.parametrize('width', (2, 1))
def test_device_table_uploads_on_change_through_rotating_staging(width):
    """encx.slots.DeviceTable at B = 3: the same rows twice are one upload; nine different tables
    (more than twice the four staging buffers) put back to back without a host synchronisation,
    the device tensor cloned on the stream after each, all arrive as put; clear() zeroes the
    table and the rows held before it upload again."""
    from encx._lib import ensure_device
    from encx.slots import DeviceTable
    ensure_device(torch.device(DEV))
    B = 3
    rows = lambda i: tuple(10 * i + b if width == 1 else tuple(100 * i + 10 * b + w for w in range(width))
                           for b in range(B))
    t = DeviceTable(B, width, torch.device(DEV))
    assert t.t.shape == ((B,) if width == 1 else (B, width)) and t.t.dtype == torch.int32
    assert t.data_ptr() == t.t.data_ptr() and t.uploads == 0 and t.host is None
    t.put(rows(0))
    t.put(list(rows(0)))
    assert t.uploads == 1 and t.host == rows(0)
    clones = []
    for i in range(1, 10):
        t.put(rows(i))
        clones.append(t.t.clone())
    assert t.uploads == 10
    torch.cuda.synchronize()
    for i, c in enumerate(clones, 1):
        assert torch.equal(c.cpu(), torch.tensor(rows(i), dtype=torch.int32)), i
    t.clear()
    assert t.host is None and not t.t.any().item()
    t.put(rows(9))
    assert t.uploads == 11 and torch.equal(t.t.cpu(), torch.tensor(rows(9), dtype=torch.int32))
