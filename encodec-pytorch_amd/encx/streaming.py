"""Streaming codec: stateful chunked encode / decode of the causal EnCodec model.

A causal codec can run live: delivered in chunks, it produces exactly what the offline model
produces on the whole clip. `StreamEncoder` / `StreamDecoder` keep the state that makes this so
between calls, for `batch` live streams, one step per chunk. Streams that advance together:

    enc = StreamEncoder(model, batch=64)            # n_q from model.bandwidth
    dec = StreamDecoder(model, batch=64, n_q=enc.n_q)
    codes = enc.encode(x)      # x [B, C, n * hop_length] -> codes [B, n_q, n]
    wav = dec.decode(codes)    # -> [B, C, n * hop_length]

A chunk is n latent frames (n * hop_length samples). For such lengths no layer's
`extra_padding` is ever non-zero (ops.conv_geometry), so no layer needs the future. The first
chunk of a session must hold at least `min_first_frames` frames (every layer's first input must
be longer than its reflect padding); later chunks may hold 1..max_frames. A trailing partial hop
is the caller's to zero-pad: the result then equals the offline model on the padded clip.

State, per tensor between two layers (a WINDOW [B][C][P + columns], csrc/stream.hip):
  SConv1d (K, s, d)        the last P = (K-1)*d - (s-1) input columns, pre-activation (the ELU
                           is applied by the consumer as it loads, as in the offline kernels);
  SConvTranspose1d (K=2s)  the previous input column;
  SLSTM                    h, c per layer.
A stream's first chunk fills each conv history by reflection of its own first columns
(x[P], x[P-1], .., x[1]), exactly as pad1d does; the transposed conv's previous column is zero.

Bit-exact slicing: the kernels' reduction order depends on the layer only, never on the batch
or on the chunk length, so the latents, codes and waveform of a stream are identical however its
audio was cut into chunks and whichever streams share its batch.

Slots. The `batch` streams of a session are slots with a life of their own: calls begin and end
at different times, and a late packet sits a step out.

    codes = enc.encode_slots(x, frames)      # x [B, C, max(frames) * hop]; frames: B ints
    wav = dec.decode_slots(codes, frames)    # codes [B, n_q, max(frames)]
    enc.restart([5]); dec.restart([5])       # slot 5's caller hung up: its next chunk is a first chunk

Slot b delivers the first frames[b] frames of its row (0: it sits the step out and keeps its
state); the rest of the row is not read (it may hold anything, NaN included), and the matching
columns of the results are zero. A slot that has not started, or was restarted, needs a first
chunk of `min_first_frames`; the other slots are not disturbed, whatever they deliver in the same
step. A step computes max(frames) columns for every slot and costs what the uniform step of that
length costs: every layer is causal, so the columns past a slot's count influence nothing that is
carried, and only the two places that carry state look at the per-slot counts (a slot table in
device memory, read by the kernels): the window roll / first-chunk fill and the LSTM's h and c
(csrc/stream.hip). encode(x) / decode(codes) are the uniform case. A slot's results are
bit-identical to the same stream alone in a session of one. Not supported: more than 64 slots,
an `.ecdc` container for live streams.

Bandwidth per slot. One model serves every bandwidth by keeping the first n_q codebooks, and no
state a session carries depends on n_q, so every slot may use its own count, and change it from
one step to the next:

    enc = StreamEncoder(model, 64, n_q=32)            # the session's largest count (24 kbps)
    dec = StreamDecoder(model, 64, n_q=32)
    nq = [enc.n_q_for(6.0)] * 64                      # per slot and step, 1..enc.n_q
    codes = enc.encode_slots(x, frames, n_q=nq)       # [B, 32, n_max], rows k >= nq[b] zero
    wav = dec.decode_slots(codes, frames, n_q=nq)     # rows k >= nq[b] are not read

The counts live in a device table beside the slot table, so one captured graph serves every mix.
The quantizer of such a step is one launch for all slots and layers (csrc/stream_rvq.hip): a
column's whole residual chain runs in one workgroup with n_q[b] as its loop bound, and the codes
are, bit for bit, rows [:n_q[b]] of the codes at the session's full bandwidth. Packets of such a
step carry a second header byte with K: raw with StreamPacker / StreamUnpacker(..., slot_n_q=True),
LM-coded with (..., use_lm=True, lm_format=2):

    packer = StreamPacker(model, 64, 32, use_lm=True, lm_format=2)     # and the StreamUnpacker alike
    packets = packer.pack_slots(codes, frames, nq)    # bytes (n, K) + one coder run, short flush
    codes, frames, nq = unpacker.unpack_slots(packets)   # ready for dec.decode_slots(codes, frames, n_q=nq)

The LM of such a stream (include/encx.h, packet format 2): the row of a frame sums the embeddings
of the K codebooks its packet carries; codebook k enters with 1 + its code in the previous frame,
or with the start index 0 where the previous frame did not carry k (or at the stream's start);
heads, cdfs and coder symbols exist for k < K only. A stream that stays at K = k is coded with the
cdf rows of a K = k session, bit for bit. The coder run ends with the short flush (the shortest
value inside the final interval, trailing zero bytes dropped; the decoder reads zero bits past
the end), so a truncated packet is not detected as "ran dry": it fails only if no interval holds
the value, and otherwise decodes to wrong codes; integrity is the transport's job. The fused quantizer takes codebooks of bins a multiple
of 4 and a latent dimension a multiple of 8 (up to 256); a session of any other model is built
and streams as before, and only its steps that pass n_q are refused (NotImplementedError, a
host check: check_rvq_shape).

Packets. What goes on the wire is one self-contained packet per delivering slot and step
(`StreamPacker` / `StreamUnpacker`; the format is documented in include/encx.h): a header byte
with the frame count, then the codes bit-packed (one launch for all slots) or, with use_lm=True,
arithmetic-coded under the entropy-coding LM. The coder is flushed at the end of every packet,
so a packet decodes when it arrives; the LM's context is carried from packet to packet, per slot,
on a ring cache, for a stream of any length (encx/lm.py LMStreamEncoder / LMStreamDecoder).

    packer, unpacker = StreamPacker(model, 64, enc.n_q), StreamUnpacker(model, 64, enc.n_q)
    packets = packer.pack_slots(codes, frames)        # list of bytes, b'' for a slot with 0 frames
    codes, frames = unpacker.unpack_slots(packets)    # ready for dec.decode_slots(codes, frames)

Lost packets. The packets are meant for a lossy link, and the decoder conceals a packet that
did not arrive, per slot and on the device:

    wav = dec.decode_slots(codes, frames, lost=[b in gone for b in range(64)])   # frames[b] to conceal
    unpacker.lose([5])                       # LM-coded streams: slot 5's context is out of step

A lost slot decodes its last latent frame again for frames[b] frames (the transport knows the
count from timing; packet_frames(p) reads it from a packet that is held but cannot be decoded).
That frame is column P-1 of the decoder's first window, where the end-of-step roll left it, so
nothing is kept on the host and the result is, bit for bit, that of repeating the slot's last
delivered code column with the codebook count it was decoded with. Everything behind the first
window runs as in any step, so the slot's state stays continuous and it simply goes on with its
next packet: no restart, no first chunk. Its codes and n_q[b] are not used.
The output fades. Per slot two integers, p in 0..M (M = conceal_fade * conceal_recover * hop,
starting at M) and r, the samples concealed in the current run; per output sample of a step
    concealed   r += 1, and p = max(0, p - conceal_recover) once r > conceal_hold * hop
    delivered   p = min(M, p + conceal_fade); r = 0 at the end of the step
and a slot that sits out changes neither. The sample is x where p == M (after the sample's
update), x * (float(p) * (1 / M)) in fp32 otherwise. With the defaults (hold 2, fade 6, recover 1
frames: 27 ms held, 80 ms down, 13 ms back up at 75 frames/s) these are design choices, not
tuned by ear. restart and reset put a slot back to p = M, r = 0. Steps with a lost slot, or with
a slot below M, run graphs of their own, one per (n_max, any_first) whatever the loss pattern;
every other step runs what it ran before. Refused: a lost slot that has not started or has 0
frames (ValueError), a decoder whose first window keeps no history (NotImplementedError).
LM-coded streams: after a lost packet the receiver's LM context differs from the sender's.
unpacker.lose([b]) marks the slot failed and drops its packets unread (0 frames) while the decoder
conceals; once the sender knows, packer.restart([b]) and unpacker.restart([b]) restart the LM
context only. Encoder and decoder are NOT restarted. Not here: codes predicted by the LM for the
lost frames, sequence numbers (detecting a loss is the transport's job).

Redundant packets (raw form). The first K_r codebooks of a frame are a coarser description of the
same frame, so a packet may repeat them for the slot's previous packet (in-band FEC; the format is
REDUNDANT PACKET in include/encx.h). A receiver that holds the next packet decodes a lost step at
K_r codebooks with the decoder it has, instead of concealing it:

    packer = StreamPacker(model, 64, 32, slot_n_q=True, fec=2)          # up to 2 codebooks repeated
    unpacker = StreamUnpacker(model, 64, 32, slot_n_q=True, fec=2)
    packets = packer.pack_slots(codes, frames, nq)                  # fec=[...]: 0..2 per slot, 0 = no copy
    codes, frames, nq = unpacker.unpack_slots(packets)              # the main sections
    codes, frames, nq = unpacker.unpack_slots(next_packets, recover=[b == 5 for b in range(64)])
    wav, status = StreamReceiver(dec, unpacker).step(packets, ahead, lost_frames)   # the recipe as code

The packer is still one launch per step: it keeps rows < R of each slot's last packet on the
device, in two copies that a slot alternates between, so the launch that reads a copy never
writes it, and a step that raises leaves the last good one in place. A copy costs 2 header bytes
and ceil(n_r K_r bits / 8). "Previous" is the slot's last step with frames; restart([b]) and
reset() drop it. Not here: redundancy for LM-coded packets, more than one step of lookback.

Key packets (LM-coded, lm_format=2). Bit 7 of header byte 1 says "this slot's LM context starts
anew with this packet"; the unpacker then restarts the context itself, and takes the slot out of
the lost and failed sets. The context is worth little (the packets table), so on a
one-way link (broadcast, a recording tap) the sender sets the bit every few packets and a loss
heals itself: unpacker.lose([b]), conceal while the slot's packets are dropped, and rejoin at the
next key packet, with no word from the receiver.

    packer = StreamPacker(model, 64, 32, use_lm=True, lm_format=2, key_interval=8)
    packets = packer.pack_slots(codes, frames, nq, key=[...])       # key: B bools, OR-ed with the interval

Inference only. Weight-normed weights are prepared once, at construction; call
refresh_weights() after changing the model. reset() restarts every slot.
"""
import dataclasses
import operator
import typing as tp

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import call, stream, ensure_device
from .lm import LMStreamEncoder, LMStreamDecoder
from .slots import DeviceTable, _ints, check_fec, check_frames, check_n_q, check_restart  # noqa: F401 (re-exported)
from .modules.conv import SConv1d, SConvTranspose1d
from .modules.lstm import SLSTM
from .modules.seanet import SEANetEncoder, SEANetResnetBlock

MAX_BATCH = ops.LSTM_MAX_BATCH
MAX_HISTORY = 64  # encx_stream_roll moves a window row as one wave
ROLL_SHIFT, ROLL_REFLECT, ROLL_ZERO = 0, 1, 2  # encx.h ENCX_ROLL_*


# ---------------------------------------------------------------------------- the layer plan
@dataclasses.dataclass
class Window:
    """A tensor between two layers. rate = its columns per latent frame; P = the history its
    consumers need (the largest of theirs); fill = how a stream's first chunk fills it."""
    C: int
    rate: int
    P: int = 0
    fill: str = 'reflect'


@dataclasses.dataclass
class Layer:
    kind: str            # 'conv' | 'convtr' | 'lstm'
    name: str            # module path inside the SEANet stack
    module: tp.Any
    src: int             # index of the window it reads
    dst: int             # index of the window it writes
    Cin: int
    Cout: int
    K: int = 1
    stride: int = 1
    dilation: int = 1
    P: int = 0           # history columns THIS layer reads before the chunk
    act: tp.Optional[str] = None
    add: bool = False    # adds into dst (the residual sum of a SEANetResnetBlock)
    final: bool = True   # dst is complete after this layer


@dataclasses.dataclass
class Plan:
    layers: tp.List[Layer]
    windows: tp.List[Window]
    hop_length: int

    @property
    def min_first_frames(self) -> int:
        """Smallest first chunk: every reflect-filled history needs n * rate > P columns."""
        return max([w.P // w.rate + 1 for w in self.windows if w.P and w.fill == 'reflect'] + [1])


def _refuse(what):
    raise NotImplementedError(f'encx streaming: {what}')


def _check_conv(m, name):
    inner = m.conv if isinstance(m, SConv1d) else m.convtr
    if not m.causal:
        _refuse(f'{name} is not causal (a non-causal layer needs the future)')
    if inner.norm_type != 'weight_norm':
        _refuse(f"{name} has norm {inner.norm_type!r}; only 'weight_norm' streams (GroupNorm is not causal)")
    if isinstance(m, SConv1d) and m.pad_mode != 'reflect':
        _refuse(f"{name} has pad_mode {m.pad_mode!r}; only 'reflect' is supported")
    if isinstance(m, SConvTranspose1d):
        if m.trim_right_ratio != 1.0:
            _refuse(f'{name} has trim_right_ratio {m.trim_right_ratio}; only 1.0 is supported')
        if inner.kernel_size != 2 * inner.stride:
            _refuse(f'{name}: transposed conv with kernel_size != 2 * stride')


def layer_plan(seanet, in_rate: int) -> Plan:
    """Host-only geometry of a SEANetEncoder (in_rate = hop_length) or SEANetDecoder (in_rate = 1):
    the layers in execution order and the windows between them. Refuses (NotImplementedError)
    what cannot stream. Touches no device."""
    is_encoder = isinstance(seanet, SEANetEncoder)
    windows = [Window(int(seanet.channels if is_encoder else seanet.dimension), int(in_rate))]
    layers: tp.List[Layer] = []

    def new_window(C, rate):
        windows.append(Window(int(C), int(rate)))
        return len(windows) - 1

    def conv(m, name, src, act, dst=None, add=False, final=True):
        _check_conv(m, name)
        c = m.conv
        K, s, d = c.kernel_size, c.stride, c.dilation
        w = windows[src]
        if w.rate % s:
            _refuse(f'{name}: stride {s} does not divide the {w.rate} columns of a frame')
        if dst is None:
            dst = new_window(c.out_channels, w.rate // s)
        P = (K - 1) * d - (s - 1)
        if P < 0 or P > MAX_HISTORY:
            _refuse(f'{name}: history of {P} columns')
        w.P = max(w.P, P)
        layers.append(Layer('conv', name, m, src, dst, c.in_channels, c.out_channels, K, s, d, P, act, add, final))
        return dst

    cur, pending = 0, None
    for idx, m in seanet.model.named_children():
        name = f'model.{idx}'
        if isinstance(m, nn.ELU):
            pending = 'elu'
        elif isinstance(m, SConv1d):
            cur, pending = conv(m, name, cur, pending), None
        elif isinstance(m, SConvTranspose1d):
            _check_conv(m, name)
            c = m.convtr
            w = windows[cur]
            w.P, w.fill = 1, 'zero'
            dst = new_window(c.out_channels, w.rate * c.stride)
            layers.append(Layer('convtr', name, m, cur, dst, c.in_channels, c.out_channels, c.kernel_size,
                                c.stride, 1, 1, pending))
            cur, pending = dst, None
        elif isinstance(m, SEANetResnetBlock):
            assert pending is None
            if not isinstance(m.shortcut, SConv1d):
                _refuse(f'{name}: identity shortcut (true_skip=True)')
            convs = [(f'{name}.block.{i}', c) for i, c in m.block.named_children() if isinstance(c, SConv1d)]
            # the shortcut conv writes the block's output window; the last conv adds into it
            out = conv(m.shortcut, f'{name}.shortcut', cur, None, final=False)
            h = cur
            for i, (cname, c) in enumerate(convs):
                if i == len(convs) - 1:
                    conv(c, cname, h, m.act, dst=out, add=True)
                else:
                    h = conv(c, cname, h, m.act)
            cur = out
        elif isinstance(m, SLSTM):
            assert pending is None
            H = m.lstm.hidden_size
            if H % 16 or H > 1024 or m.lstm.input_size != H:
                _refuse(f'{name}: LSTM of {m.lstm.input_size} -> {H} units')
            dst = new_window(H, windows[cur].rate)
            layers.append(Layer('lstm', name, m, cur, dst, H, H))
            cur = dst
        else:
            _refuse(f'{name}: {type(m).__name__}')
    assert pending is None and layers[-1].dst == cur
    hop = in_rate if is_encoder else windows[cur].rate
    if windows[cur].rate != (1 if is_encoder else hop):
        _refuse('the strides do not multiply to the hop length')
    return Plan(layers, windows, int(hop))


def check_model(model):
    """The refusals that concern the whole model (NotImplementedError); no device call."""
    if model.normalize:
        _refuse('audio_normalize=True (the scale needs the whole clip)')
    if model.segment is not None:
        _refuse('segmented models (segment is not None)')
    if model.channels not in (1, 2):
        _refuse(f'{model.channels} channels')


def encoder_plan(model) -> Plan:
    check_model(model)
    return layer_plan(model.encoder, int(model.encoder.hop_length))


def decoder_plan(model) -> Plan:
    check_model(model)
    return layer_plan(model.decoder, 1)


# ---------------------------------------------------------------------------- concealment, the host side
MAX_FADE = 1 << 24  # the fade position is multiplied as an fp32: exact up to 2^24
_R_CAP = 1 << 30    # r saturates here: past the hold only r > hold is ever asked of it


def fade_span(hold_frames: int, fade_frames: int, recover_frames: int, hop: int) -> int:
    """M = fade_frames * recover_frames * hop, the full level of the fade position p. A concealed
    sample past the hold lowers p by recover_frames, a delivered one raises it by fade_frames, so the
    way down takes fade_frames frames and the way up recover_frames. Raises ValueError; host only."""
    hold_frames, fade_frames, recover_frames = (operator.index(v) for v in (hold_frames, fade_frames, recover_frames))
    if not 0 <= hold_frames <= 255:
        raise ValueError(f'encx streaming: conceal_hold {hold_frames} (0..255 frames)')
    if not 1 <= fade_frames <= 255:
        raise ValueError(f'encx streaming: conceal_fade {fade_frames} (1..255 frames)')
    if not 1 <= recover_frames <= 255:
        raise ValueError(f'encx streaming: conceal_recover {recover_frames} (1..255 frames)')
    M = fade_frames * recover_frames * int(hop)
    if M > MAX_FADE:
        raise ValueError(f'encx streaming: a fade of {fade_frames} x {recover_frames} frames of {hop} samples has '
                         f'{M} levels (at most 2^24)')
    return M


def check_lost(started: tp.Sequence[bool], frames: tp.Sequence[int], lost, M: int = 0) -> tp.Optional[tp.List[bool]]:
    """lost[b]: slot b's packet of this step did not arrive, and frames[b] (1..max_frames, known to
    the transport from timing) frames are concealed. -> the flags as bools, or None when no slot is
    lost (lost=None, or all False). M: the session's fade span. Raises ValueError; host data only."""
    if lost is None:
        return None
    try:
        lost = [bool(v) for v in lost]
    except TypeError:
        raise ValueError('encx streaming: lost must be a sequence of bools') from None
    if len(lost) != len(started) or len(frames) != len(started):
        raise ValueError(f'encx streaming: lost for {len(lost)} slots, the session has {len(started)}')
    if not any(lost):
        return None
    if M > MAX_FADE:
        raise ValueError(f'encx streaming: a fade of {M} levels (at most 2^24)')
    for b, (on, f, gone) in enumerate(zip(started, frames, lost)):
        if not gone:
            continue
        if not f:
            raise ValueError(f'encx streaming: slot {b} is lost with 0 frames (pass the frames to conceal)')
        if not on:
            raise ValueError(f'encx streaming: slot {b} is lost before its first chunk: there is nothing to repeat')
    return lost


def fade_positions(p: int, r: int, lost: bool, samples: int, hold: int, fade: int, recover: int, M: int):
    """The fade position after each of a step's `samples` samples of one slot, in closed form, from
    the slot's (p, r) at the start of the step; hold in samples. int64 [samples]. Per sample the
    rule is: concealed r += 1, and p = max(0, p - recover) once r > hold; delivered p = min(M, p +
    fade). The kernel (csrc/stream_conceal.hip) evaluates the same expressions."""
    j1 = np.arange(1, samples + 1, dtype=np.int64)
    if lost:
        dec = np.maximum(r + j1 - hold, 0) - max(r - hold, 0)
        return np.maximum(p - recover * dec, 0)
    return np.minimum(p + fade * j1, M)


def fade_step(p: int, r: int, lost: bool, samples: int, hold: int, fade: int, recover: int, M: int):
    """(p, r) of a slot after a step of `samples` samples (0: it sat out, nothing changes)."""
    if not samples:
        return p, r
    if lost:
        dec = max(r + samples - hold, 0) - max(r - hold, 0)
        return max(p - recover * dec, 0), min(r + samples, _R_CAP)
    return min(p + fade * samples, M), 0


def fade_gains(positions, M: int):
    """The fp32 factor of each sample: float(p) * invM with invM = fp32(1) / fp32(M); where p == M
    the sample is written unscaled (the factor is then not used)."""
    return positions.astype(np.float32) * (np.float32(1) / np.float32(M))


# ---------------------------------------------------------------------------- a running session
class _Session:
    """The device side of one SEANet stack: windows, prepared weights, LSTM state, roll tables
    and the captured graphs."""

    def __init__(self, model, plan: Plan, batch: int, max_frames: int, graphs: bool):
        if not 1 <= batch <= MAX_BATCH:
            _refuse(f'batch {batch} (1..{MAX_BATCH})')
        if max_frames < plan.min_first_frames:
            raise ValueError(f'encx streaming: max_frames {max_frames} is below the first chunk\'s minimum '
                             f'of {plan.min_first_frames} frames')
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('encx streaming runs on the GPU (no CPU fallback): move the model first')
        ensure_device(dev)
        self.model, self.plan, self.dev = model, plan, dev
        self.B, self.max_frames, self.graphs = int(batch), int(max_frames), bool(graphs)
        self.hop_length = plan.hop_length
        self.min_first_frames = plan.min_first_frames
        # every window and the LSTM state in one arena, so reset() is one fill
        self._W = [w.P + max_frames * w.rate for w in plan.windows]
        sizes = [self.B * w.C * W for w, W in zip(plan.windows, self._W)]
        lstm_sizes = []
        for L in plan.layers:
            if L.kind == 'lstm':
                nl = L.module.lstm.num_layers
                lstm_sizes += [nl * self.B * 2 * L.Cin, nl * self.B * L.Cin]
        self._arena = torch.zeros(sum(sizes) + sum(lstm_sizes), device=dev, dtype=torch.float32)
        off, self.bufs = 0, []
        for w, W, sz in zip(plan.windows, self._W, sizes):
            self.bufs.append(self._arena[off:off + sz].view(self.B, w.C, W))
            off += sz
        self._lstm = {}
        for i, L in enumerate(plan.layers):
            if L.kind != 'lstm':
                continue
            nl, H = L.module.lstm.num_layers, L.Cin
            hz = self._arena[off:off + nl * self.B * 2 * H]
            off += hz.numel()
            c = self._arena[off:off + nl * self.B * H]
            off += c.numel()
            self._lstm[i] = dict(hz=hz, c=c, gates=torch.empty(self.B * 4 * H, device=dev),
                                 wcat=torch.empty(nl * 8 * H * H, device=dev),
                                 wcatT=torch.empty(nl * 8 * H * H, device=dev),
                                 bsum=torch.empty(nl * 4 * H, device=dev))
        self._weights: tp.Dict[int, torch.Tensor] = {}
        self._bias: tp.Dict[int, torch.Tensor] = {}
        self._tables: tp.Dict[tp.Optional[int], tuple] = {}
        # the captured steps, keyed (variant, n, first, *extra): a variant's graphs never replace
        # another's
        self._graphs: tp.Dict[tuple, tuple] = {}
        self.started = [False] * self.B  # per slot: it has had its first chunk
        self._fresh = True               # the arena is as reset() left it
        # the slot table the kernels read (encx.h), refilled before each step of a slots call, and
        # beside it the codebook count per slot (encx.h: nq[B]) of a per-slot-bandwidth step
        self.slot_table = DeviceTable(self.B, 2, dev)
        self.nq_table = DeviceTable(self.B, 1, dev)
        self._slots, self._nq = self.slot_table.t, self.nq_table.t
        self._cols = torch.arange(max(self._W), device=dev, dtype=torch.int32)
        self._table(None)
        self.refresh_weights()

    # ---- weights
    @torch.no_grad()
    def refresh_weights(self):
        """(Re)prepare every layer's weights from the model's current parameters, into the
        buffers the kernels (and any captured graph) already point at."""
        st = stream()
        for i, L in enumerate(self.plan.layers):
            if L.kind == 'lstm':
                s, H = self._lstm[i], L.Cin
                ws = L.module._weights()
                for l in range(L.module.lstm.num_layers):
                    w_ih, w_hh, b_ih, b_hh = (w.detach().contiguous() for w in ws[4 * l:4 * l + 4])
                    call('encx_lstm_pack', w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(),
                         s['wcat'].data_ptr(), s['wcatT'].data_ptr(), s['bsum'].data_ptr(), H, l, st)
                continue
            params = L.module.conv.conv if L.kind == 'conv' else L.module.convtr.convtr
            v, g = params.wv()
            wf, wp = ops._weight_prep(v.detach().contiguous(), g.detach().contiguous(), L.K, L.stride,
                                      L.kind == 'conv', L.kind == 'convtr')
            w = wf if L.kind == 'conv' else wp
            if i in self._weights:
                self._weights[i].copy_(w)
            else:
                self._weights[i] = w
            # the bias too is a copy, so that a session is one snapshot of the model
            if params.bias is not None:
                if i in self._bias:
                    self._bias[i].copy_(params.bias)
                else:
                    self._bias[i] = params.bias.detach().clone()

    # ---- state
    @torch.no_grad()
    def reset(self):
        """Start a new session: every slot restarted, every history and LSTM state cleared."""
        self._arena.zero_()
        self.started = [False] * self.B
        self._fresh = True

    def restart(self, slots):
        """The named slots' next non-empty chunk is a first chunk. Host bookkeeping only: the
        `first` flag of the slot table makes the kernels refill the slot's histories and start its
        LSTM from zero on that chunk."""
        slots = check_restart(slots, self.B)
        for b in slots:
            self.started[b] = False
        return slots

    def check_frames(self, frames):
        return check_frames(self.started, frames, self.min_first_frames, self.max_frames)

    def uniform(self):
        """Whether a step of n frames for every slot can run without the slot table: all slots
        are past their first chunk, or none has started and the arena is clear (a restarted slot
        holds the state of its previous stream, which only the table's `first` flag clears)."""
        return all(self.started) or self._fresh

    def put_slots(self, frames):
        """Fill the device slot table for this step: per slot its frames and whether this is its
        first chunk."""
        self.slot_table.put((int(f), int(f > 0 and not on)) for f, on in zip(frames, self.started))

    def keep(self, cols, rate):
        """[B, 1, cols] bool, from the slot table on the device (capturable): the columns of a
        tensor with `rate` columns per frame that belong to each slot's chunk."""
        return (self._cols[:cols] < self._slots[:, :1] * rate).unsqueeze(1)

    # ---- roll tables
    def _table(self, n):
        """Device tables of encx_stream_win (48-byte entries) for chunks of n frames: all windows
        that carry a history (the end-of-step roll) and the same entries one by one (the first
        chunk's reflect fills). n None: the same for a slots step, as encx_stream_slot_win
        (64-byte entries): the columns a row moves come from the slot table, so one table serves
        every step. Built on the host, so outside any capture."""
        t = self._tables.get(n)
        if t is None:
            rows, full, single, index = 0, [], [], {}
            for wi, (w, W, buf) in enumerate(zip(self.plan.windows, self._W, self.bufs)):
                if not w.P:
                    continue
                index[wi] = len(full)
                e = [buf.data_ptr(), self.B * w.C, w.P, 0 if n is None else n * w.rate, W]
                per_slot = [w.C, w.rate] if n is None else []
                full.append(e + [rows] + per_slot)
                single.append(e + [0] + per_slot)
                rows += self.B * w.C
            tab = torch.tensor(np.array(full + single, dtype=np.int64)).to(self.dev) if full else None
            t = self._tables[n] = (tab, len(full), rows, index)
        return t

    def _reflect(self, n, wi, st, slots=False):
        """The first-chunk fill of window wi, right after its producer ran. Without the slot table
        every row is reflected (a 'zero' window is zero already: the arena is clear); with it,
        the rows of the slots on their first chunk are reflected or cleared."""
        w = self.plan.windows[wi]
        if not w.P:
            return
        if slots:
            tab, nfull, _, index = self._table(None)
            call('encx_stream_roll_slots', tab.data_ptr() + 64 * (nfull + index[wi]), 1, self.B * w.C,
                 ROLL_REFLECT if w.fill == 'reflect' else ROLL_ZERO, self._slots.data_ptr(), self.B, st)
        elif w.fill == 'reflect':
            tab, nfull, _, index = self._table(n)
            call('encx_stream_roll', tab.data_ptr() + 48 * (nfull + index[wi]), 1, self.B * w.C, 1, st)

    # ---- one step
    def _layers(self, n, first, slots=False):
        """The layers and the end-of-step roll for n columns per slot; first: the first-chunk
        fills run too. slots: masked by the device slot table (n = n_max, first = any slot's)."""
        st = stream()
        ws, Ws, bufs, B = self.plan.windows, self._W, self.bufs, self.B
        if first:
            self._reflect(n, 0, st, slots)
        for i, L in enumerate(self.plan.layers):
            s, d = ws[L.src], ws[L.dst]
            Ws_, Wd = Ws[L.src], Ws[L.dst]
            y = bufs[L.dst].data_ptr() + 4 * d.P
            b = self._bias.get(i)
            if L.kind == 'conv':
                call('encx_stream_conv1d', bufs[L.src].data_ptr() + 4 * (s.P - L.P), self._weights[i].data_ptr(),
                     None if b is None else b.data_ptr(), y, B, L.Cin, L.Cout, n * d.rate, L.K, L.stride,
                     L.dilation, s.C * Ws_, Ws_, d.C * Wd, Wd, ops.ACT[L.act], int(L.add), st)
            elif L.kind == 'convtr':
                call('encx_stream_convtr1d', bufs[L.src].data_ptr() + 4 * (s.P - 1), self._weights[i].data_ptr(),
                     None if b is None else b.data_ptr(), y, B, L.Cin, L.Cout, n * s.rate, L.stride,
                     s.C * Ws_, Ws_, d.C * Wd, Wd, ops.ACT[L.act], st)
            else:
                m = self._lstm[i]
                args = (bufs[L.src].data_ptr() + 4 * s.P, m['wcatT'].data_ptr(),
                        m['bsum'].data_ptr(), m['hz'].data_ptr(), m['c'].data_ptr(), m['gates'].data_ptr(), y,
                        int(bool(L.module.skip)), B, n * s.rate, L.Cin, L.module.lstm.num_layers, s.C * Ws_, Ws_,
                        d.C * Wd, Wd)
                if slots:
                    if s.rate != 1:  # the table counts frames, the recurrence columns
                        _refuse(f'{L.name}: per-slot steps of an LSTM at {s.rate} columns per frame')
                    call('encx_stream_lstm_slots', *args, self._slots.data_ptr(), st)
                else:
                    call('encx_stream_lstm', *args, st)
            if first and L.final:
                self._reflect(n, L.dst, st, slots)
        tab, nfull, rows, _ = self._table(None if slots else n)
        if not nfull:
            return
        if slots:
            call('encx_stream_roll_slots', tab.data_ptr(), nfull, rows, ROLL_SHIFT, self._slots.data_ptr(), B, st)
        else:
            call('encx_stream_roll', tab.data_ptr(), nfull, rows, 0, st)

    def _run(self, key, body):
        """body(*key) eagerly, or as the graph captured for key the first time."""
        if not self.graphs:
            return body(*key)
        ent = self._graphs.get(key)
        if ent is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):  # one stream: the graph has no parallel branches
                res = body(*key)
            ent = self._graphs[key] = (g, res)
        ent[0].replay()
        return tuple(t.clone() for t in ent[1])  # the graph's outputs are rewritten by its next replay

    def step(self, body, variant, frames, n, first, *extra):
        """One step of `frames` (checked: n, first = check_frames(frames)): body(variant, n, first,
        *extra), and a graph per such key. variant 'uniform' runs without the slot table (see
        uniform()); 'slots', 'nq' and 'conceal' run under it (already filled: put_slots), and it is
        read by the kernels, so one graph serves whichever slots join, sit out or deliver fewer
        frames."""
        if variant == 'uniform':
            self._table(n)  # built on the host, so before any capture
        out = self._run((variant, n, first) + extra, body)
        if first:
            self.started = [on or f > 0 for on, f in zip(self.started, frames)]
        self._fresh = False
        return out

    def graph_keys(self, variant):
        """The keys (n, first, *extra) of the variant's captured steps, sorted."""
        return sorted(k[1:] for k in self._graphs if k[0] == variant)

    def graph(self, variant, key):
        """The captured step (graph, outputs) of a key of graph_keys(variant)."""
        return self._graphs[(variant,) + tuple(key)]

    def first_and_one(self, variant, fill=None, *extra):
        """The usual steps of warm(): one first chunk and one later chunk of a single frame."""
        return [(variant, self.min_first_frames, fill) + extra, (variant, 1, fill) + extra]

    def warm(self, body, runs):
        """Load every kernel of a step before any capture. Each of `runs` starts on the zero state
        and is a list of steps (variant, n, fill, *extra), taken eagerly with n frames for every
        slot; fill() puts the step's tables beyond the slot table. Then back to a clean session."""
        graphs, self.graphs = self.graphs, False
        try:
            for steps in runs:
                for variant, n, fill, *extra in steps:
                    frames = [n] * self.B
                    if variant != 'uniform':
                        self.put_slots(frames)
                    if fill is not None:
                        fill()
                    self.step(body, variant, frames, *self.check_frames(frames), *extra)
                self.reset()
        finally:
            self.graphs = graphs


def check_rvq_shape(n_q: int, bins: int, D: int):
    """A step with a per-slot n_q runs the fused quantizer, which takes fewer codebook shapes
    than the per-layer kernels of every other step (ops.stream_rvq_supports). Raises
    NotImplementedError; host arithmetic only, so a session of any model the per-layer path
    streams is still built, and only its steps that pass n_q are refused."""
    if not ops.stream_rvq_supports(n_q, bins, D):
        _refuse(f'a per-slot n_q with {n_q} codebooks of {bins} x {D} (at most 64 codebooks, bins a multiple '
                'of 4, a latent dimension that is a multiple of 8 up to 256); steps without n_q run')


def _books(embeds, encode):
    """The packed codebooks of the fused quantizer, or None where it does not take their shape
    (check_rvq_shape then refuses the steps that would need them)."""
    bins, D = embeds[0].shape
    return ops.StreamRVQBooks(embeds, encode) if ops.stream_rvq_supports(len(embeds), bins, D) else None


def _embeds(model, n_q):
    layers = model.quantizer.vq.layers
    if not 1 <= n_q <= len(layers):
        raise ValueError(f'encx streaming: n_q {n_q} (the model has {len(layers)} codebooks)')
    return [l._codebook.embed for l in layers[:n_q]]


class _Stream:
    """What StreamEncoder and StreamDecoder share: the session of their SEANet stack (self._s),
    the codebooks of their n_q (set before _open), and the life cycle of the slots."""

    def _open(self, model, plan, batch, max_frames, graphs, encode):
        self._s = _Session(model, plan, batch, max_frames, graphs)
        self.channels = model.channels
        self._embeds = _embeds(model, self.n_q)
        self._books = _books(self._embeds, encode)  # a decoder gathers rows: no transpose, no |e|^2

    def _fill_nq(self):
        """warm(): every slot at the session's full codebook count."""
        self._s.nq_table.put([self.n_q] * self._s.B)

    hop_length = property(lambda self: self._s.hop_length)
    min_first_frames = property(lambda self: self._s.min_first_frames)
    plan = property(lambda self: self._s.plan)

    def reset(self):
        self._s.reset()

    def restart(self, slots):
        """The named slots (indices 0..batch-1) start a new stream with their next non-empty
        chunk; the other slots are not disturbed. Legal between any two steps; launches nothing."""
        self._s.restart(slots)

    def refresh_weights(self):
        self._s.refresh_weights()
        self._embeds = _embeds(self._s.model, self.n_q)
        if self._books is not None:
            self._books.prepare(self._embeds)


class StreamEncoder(_Stream):
    """Chunked encoder of a causal model for `batch` streams: encode(x [B, C, n*hop]) -> codes
    [B, n_q, n] (int64). n_q, the session's codebook count (the largest a slot may use with a
    per-slot n_q), is the constructor's argument or, by default, follows from model.bandwidth. See
    the module docstring."""

    def __init__(self, model, batch: int, max_frames: int = 8, graphs: bool = True, n_q: tp.Optional[int] = None):
        plan = encoder_plan(model)
        if n_q is None:
            n_q = model.quantizer.get_num_quantizers_for_bandwidth(model.frame_rate, model.bandwidth)
        self.n_q = operator.index(n_q)  # the session's largest codebook count
        _embeds(model, self.n_q)        # refused here, before any device call
        self._open(model, plan, batch, max_frames, graphs, True)
        s = self._s
        runs = [s.first_and_one('uniform'), s.first_and_one('slots')]
        if self._books is not None:
            runs.append(s.first_and_one('nq', self._fill_nq, False))
        with torch.no_grad():
            s.warm(self._body, runs)

    def n_q_for(self, bandwidth_kbps: float) -> int:
        """The codebook count of this model at a bandwidth (kbps), for encode_slots(n_q=...).
        ValueError when the session was built for fewer codebooks."""
        m = self._s.model
        q = m.quantizer.get_num_quantizers_for_bandwidth(m.frame_rate, bandwidth_kbps)
        if q > self.n_q:
            raise ValueError(f'encx streaming: {bandwidth_kbps} kbps needs {q} codebooks, the session has {self.n_q}')
        return q

    def _body(self, variant, n, first, latent=True):
        """One step -> (codes, latent). 'uniform': the layers without the slot table, the
        per-layer quantizer. 'slots': under the table, the columns past a slot's count zero.
        'nq': under the table, the quantizer the fused kernel under the nq table, which reads the
        latent in place from the last window, all slots and layers in one launch; the latent is
        returned only when asked for."""
        s = self._s
        s._layers(n, first, variant != 'uniform')
        dst = s.plan.layers[-1].dst
        P = s.plan.windows[dst].P
        win = s.bufs[dst][:, :, P:P + n]
        if variant == 'uniform':
            # a copy, never a view: the window is rewritten by the next step
            emb = win.clone(memory_format=torch.contiguous_format)
            return ops.rvq_encode(emb, self._embeds).permute(1, 0, 2).contiguous(), emb
        if variant == 'nq':
            codes = ops.stream_rvq_encode_slots(win, self._books, s._slots, s._nq)
            return (codes, torch.where(s.keep(n, 1), win, 0.).contiguous()) if latent else (codes,)
        keep = s.keep(n, 1)
        # the columns past a slot's count are zero (and a copy, as above)
        emb = torch.where(keep, win, 0.).contiguous()
        return torch.where(keep, ops.rvq_encode(emb, self._embeds).permute(1, 0, 2), 0).contiguous(), emb

    def _samples(self, x):
        s = self._s
        if x.dim() != 3 or x.shape[0] != s.B or x.shape[1] != self.channels or x.shape[2] % s.hop_length:
            raise ValueError(f'encx streaming: expected [{s.B}, {self.channels}, n * {s.hop_length}] samples, '
                             f'got {tuple(x.shape)}')
        return x.shape[2] // s.hop_length

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_latent: bool = False):
        """x [B, C, n * hop_length] float32 on the model's device -> codes [B, n_q, n] (and the
        latent [B, D, n] with return_latent). Equals the offline model on the audio so far. The
        uniform case of encode_slots: every slot delivers n frames."""
        s = self._s
        n = self._samples(x)
        frames = [n] * s.B
        n, first = s.check_frames(frames)
        ops._check(x)
        if not s.uniform():  # some slots are on their first chunk, others not
            return self.encode_slots(x, frames, return_latent)
        P = s.plan.windows[0].P
        s.bufs[0][:, :, P:P + x.shape[2]].copy_(x)
        codes, emb = s.step(self._body, 'uniform', frames, n, first)
        return (codes, emb) if return_latent else codes

    @torch.no_grad()
    def encode_slots(self, x: torch.Tensor, frames: tp.Sequence[int], return_latent: bool = False,
                     n_q: tp.Optional[tp.Sequence[int]] = None):
        """x [B, C, n_max * hop_length], frames[b] = the frames slot b delivers (0: it sits out),
        n_max = max(frames) -> codes [B, n_q, n_max] (and the latent [B, D, n_max]). Slot b's
        samples past frames[b] * hop_length are not read; its result columns past frames[b] are
        zero. Each slot equals the same stream alone.

        n_q: B ints, the codebooks each slot uses THIS step (1..self.n_q for a slot that delivers
        frames; ignored for the others); it may differ from the slot's last step, which is how a
        stream changes bandwidth. Rows k >= n_q[b] of slot b's codes are zero, rows k < n_q[b] are
        those of the session's full bandwidth (code k depends only on layers < k). The quantizer
        then runs as one launch for all slots and layers (csrc/stream_rvq.hip)."""
        s = self._s
        n = self._samples(x)
        frames = _ints(frames, 'frames')
        n_max, any_first = s.check_frames(frames)
        if n != n_max:
            raise ValueError(f'encx streaming: {n} frames of samples for max(frames) = {n_max}')
        if n_q is not None:
            check_rvq_shape(self.n_q, *self._embeds[0].shape)
            n_q = check_n_q(frames, n_q, self.n_q)
        ops._check(x)
        s.put_slots(frames)
        P = s.plan.windows[0].P
        s.bufs[0][:, :, P:P + x.shape[2]].copy_(torch.where(s.keep(x.shape[2], s.hop_length), x, 0.))
        if n_q is not None:
            s.nq_table.put(n_q)
            out = s.step(self._body, 'nq', frames, n_max, any_first, bool(return_latent))
        else:
            out = s.step(self._body, 'slots', frames, n_max, any_first)
        return out if return_latent else out[0]


class StreamDecoder(_Stream):
    """Chunked decoder of a causal model for `batch` streams: decode(codes [B, n_q, n]) -> wav
    [B, C, n * hop_length]. See the module docstring."""

    def __init__(self, model, batch: int, n_q: int, max_frames: int = 8, graphs: bool = True,
                 conceal_hold: int = 2, conceal_fade: int = 6, conceal_recover: int = 1):
        plan = decoder_plan(model)
        self.n_q = int(n_q)
        if not 1 <= self.n_q <= model.quantizer.n_q:
            raise ValueError(f'encx streaming: n_q {n_q} (the model has {model.quantizer.n_q} codebooks)')
        # the fade of a concealed slot (module docstring): frames held, frames down, frames back up
        self._M = fade_span(conceal_hold, conceal_fade, conceal_recover, plan.hop_length)
        self._hold, self._fade, self._recover = int(conceal_hold), int(conceal_fade), int(conceal_recover)
        self._open(model, plan, batch, max_frames, graphs, False)
        self.bins = model.quantizer.bins
        self._codes: tp.Dict[tuple, torch.Tensor] = {}
        # concealment: per slot the fade position p (0..M) and the samples r of the current loss run,
        # advanced here exactly as the kernels do, and the table they read (encx.h: conceal[B][4])
        s = self._s
        self._p, self._r = [self._M] * s.B, [0] * s.B
        self._dirty = False  # some slot has p < M or r > 0
        self._conceal = DeviceTable(s.B, 4, s.dev)
        runs = [s.first_and_one('uniform'), s.first_and_one('slots')]
        if self._books is not None:
            runs.append(s.first_and_one('nq', self._fill_nq))
        if plan.windows[0].P:
            # the concealed step: a first chunk, then one concealed frame for every slot on either
            # dequantizer
            steps = [('slots', s.min_first_frames, None),
                     ('conceal', 1, lambda: self._put_conceal([True] * s.B), False)]
            if self._books is not None:
                steps.append(('conceal', 1, self._fill_nq, True))
            runs.append(steps)
        with torch.no_grad():
            s.warm(self._body, runs)

    def reset(self):
        self._s.reset()
        self._p, self._r, self._dirty = [self._M] * self._s.B, [0] * self._s.B, False

    def restart(self, slots):
        """As StreamEncoder.restart; the slots' fade starts over at full level."""
        for b in self._s.restart(slots):
            self._p[b], self._r[b] = self._M, 0
        self._dirty = any(p < self._M or r for p, r in zip(self._p, self._r))

    # ---- concealment
    def _put_conceal(self, lost):
        """Fill the device concealment table for this step: lost flag, p and r at its start."""
        self._conceal.put((int(l), p, r, 0) for l, p, r in zip(lost, self._p, self._r))

    def _advance(self, frames, lost):
        """p and r of every slot after the step, by the rule the output kernel applies per sample."""
        if lost is None and not self._dirty:
            return
        hop = self._s.hop_length
        for b, f in enumerate(frames):
            self._p[b], self._r[b] = fade_step(self._p[b], self._r[b], bool(lost and lost[b]), f * hop,
                                               self._hold * hop, self._fade, self._recover, self._M)
        self._dirty = any(p < self._M or r for p, r in zip(self._p, self._r))

    def _code_buf(self, n, fused=False):
        """The codes of a step, the graph's own input: [n_q, B, n] for the per-layer dequantizer,
        clamped and zero past a slot's count; fused, [B, n_q, n] as the caller passed them (the
        kernel clamps them and reads neither a slot's tail nor its rows k >= n_q[b])."""
        c = self._codes.get((n, fused))
        if c is None:
            shape = (self._s.B, self.n_q, n) if fused else (self.n_q, self._s.B, n)
            c = self._codes[n, fused] = torch.zeros(shape, device=self._s.dev, dtype=torch.int64)
        return c

    def _body(self, variant, n, first, fused=False):
        """One step -> (wav,). The dequantizer writes into the first window behind its history:
        per layer, or ('nq', and 'conceal' with fused) the fused kernel under the nq table. Then the
        layers, without the slot table ('uniform') or under it, and the output, a copy of the last
        window, zero past a slot's count under the table. 'conceal': a slots step with lost or
        fading slots. The latent of a lost slot is its held column (P-1 of the first window), set
        by the fused dequantizer itself or, after the per-layer one, by the fill kernel; the output
        kernel reads the last window in place, zeroes the samples past each slot's count and
        applies the fade."""
        s = self._s
        P, win, hop = s.plan.windows[0].P, s.bufs[0], s.hop_length
        conceal = variant == 'conceal'
        if fused or variant == 'nq':
            held = (self._conceal.t, win[:, :, P - 1:P]) if conceal else ()
            ops.stream_rvq_decode_slots(self._code_buf(n, True), self._books, s._slots, s._nq, win[:, :, P:P + n],
                                        *held)
        else:
            win[:, :, P:P + n].copy_(ops.rvq_decode(self._code_buf(n), self._embeds))
            if conceal:
                ops.stream_conceal_fill(win, P, n, s._slots, self._conceal.t)
        s._layers(n, first, variant != 'uniform')
        out = s.bufs[s.plan.layers[-1].dst]
        if conceal:
            return (ops.stream_conceal_out(out, hop, n, s._slots, self._conceal.t, self._hold, self._fade,
                                           self._recover),)
        out = out[:, :, :n * hop]
        if variant == 'uniform':
            # a copy, never a view: the window is rewritten by the next step
            return (out.clone(memory_format=torch.contiguous_format),)
        return (torch.where(s.keep(n * hop, hop), out, 0.).contiguous(),)

    def _frames(self, codes):
        s = self._s
        if codes.dim() != 3 or codes.shape[0] != s.B or codes.shape[1] != self.n_q or codes.dtype != torch.int64:
            raise ValueError(f'encx streaming: expected int64 codes [{s.B}, {self.n_q}, n], got '
                             f'{codes.dtype} {tuple(codes.shape)}')
        return codes.shape[2]

    @torch.no_grad()
    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [B, n_q, n] int64 on the model's device -> wav [B, C, n * hop_length]. Equals
        the offline decoder on the codes so far. Codes are clamped to the codebook size. The
        uniform case of decode_slots: every slot delivers n frames."""
        s = self._s
        frames = [self._frames(codes)] * s.B
        n, first = s.check_frames(frames)
        if not codes.is_cuda:
            raise RuntimeError('encx streaming takes device tensors (no CPU fallback)')
        if not s.uniform() or self._dirty:  # some slots are on their first chunk, or in a fade
            return self.decode_slots(codes, frames)
        buf = self._code_buf(n)
        buf.copy_(codes.permute(1, 0, 2))
        buf.clamp_(0, self.bins - 1)  # an index outside the codebook must never reach the gather
        return s.step(self._body, 'uniform', frames, n, first)[0]

    @torch.no_grad()
    def decode_slots(self, codes: tp.Optional[torch.Tensor], frames: tp.Sequence[int],
                     n_q: tp.Optional[tp.Sequence[int]] = None, lost=None) -> torch.Tensor:
        """codes [B, n_q, n_max], frames[b] = the frames slot b delivers (0: it sits out), n_max =
        max(frames) -> wav [B, C, n_max * hop_length]. Slot b's codes past frames[b] are not read
        (code 0 is decoded in their place); its samples past frames[b] * hop_length are zero.
        Each slot equals the same stream alone.

        n_q: as StreamEncoder.encode_slots: B ints, the codebooks of each slot this step; rows
        k >= n_q[b] of slot b's codes are not read, and the slot's wave is that of a decoder built
        for n_q[b] codebooks.

        lost: B bools. A lost slot's packet did not arrive: frames[b] (1..max_frames, which the
        transport knows from timing) frames are concealed by decoding the slot's last latent frame
        again, bit for bit what repeating its last delivered code column would give, and its output
        fades out after conceal_hold frames and back in once it delivers (module docstring). The
        codes and n_q[b] of a lost slot are not used (anything may stand there); codes may be None
        when every slot with frames is lost. The slot must have had its first chunk."""
        s = self._s
        n = None if codes is None else self._frames(codes)
        frames = _ints(frames, 'frames')
        n_max, any_first = s.check_frames(frames)
        lost = check_lost(s.started, frames, lost, self._M)
        if n is None:
            if lost is None or any(f and not gone for f, gone in zip(frames, lost)):
                raise ValueError('encx streaming: codes may be None only when every slot with frames is lost')
        elif n != n_max:
            raise ValueError(f'encx streaming: {n} frames of codes for max(frames) = {n_max}')
        if lost is not None and not s.plan.windows[0].P:
            _refuse('concealment for a decoder whose first layer keeps no history (no held column to repeat)')
        if n_q is not None:
            check_rvq_shape(self.n_q, *self._embeds[0].shape)
            n_q = check_n_q([0 if gone else f for f, gone in zip(frames, lost)] if lost else frames, n_q, self.n_q)
        if codes is not None and not codes.is_cuda:
            raise RuntimeError('encx streaming takes device tensors (no CPU fallback)')
        s.put_slots(frames)
        # the concealed step: its own graphs, taken only while a slot is lost or below full level
        conceal = lost is not None or any(p < self._M for p in self._p)
        if conceal:
            self._put_conceal(lost or [False] * s.B)
        fused = n_q is not None
        if fused:
            s.nq_table.put(n_q)
        buf = self._code_buf(n_max, fused)
        if codes is None:
            buf.zero_()
        elif fused:
            buf.copy_(codes)
        else:
            # clamped as in decode(); past a slot's count whatever the caller left becomes code 0
            buf.copy_(torch.where(s.keep(n_max, 1).squeeze(1), codes.permute(1, 0, 2).clamp(0, self.bins - 1), 0))
        variant, extra = ('conceal', (fused,)) if conceal else ('nq' if fused else 'slots', ())
        out = s.step(self._body, variant, frames, n_max, any_first, *extra)[0]
        self._advance(frames, lost)
        return out


# ---------------------------------------------------------------------------- packets
MAX_PACKET_FRAMES = 255  # the header byte (include/encx.h: the packet format)


def packet_frames(packet: bytes) -> int:
    """The frame count a packet announces (header byte 0 of every packet form), 0 for b''. For a
    packet that is held but cannot be decoded (StreamUnpacker.lose): the frames to conceal."""
    return int(packet[0]) if len(packet) else 0


def packet_bytes(n: int, K: int, bits: int) -> int:
    """Length of a raw packet of n frames of K codes: the header byte and ceil(n K bits / 8)."""
    return 1 + (n * K * bits + 7) // 8


def packet_bytes_nq(n: int, K: int, bits: int) -> int:
    """Length of a variable-bandwidth packet of n frames of K codes: the two header bytes (n, K)
    and ceil(n K bits / 8)."""
    return 2 + (n * K * bits + 7) // 8


def packet_bytes_fec(n: int, K: int, n_r: int, K_r: int, bits: int) -> int:
    """Length of a redundant packet: the four header bytes (n, K, n_r, K_r), ceil(n K bits / 8) for
    this step and, from the next byte on, ceil(n_r K_r bits / 8) for the copy of the previous one."""
    return 4 + (n * K * bits + 7) // 8 + (n_r * K_r * bits + 7) // 8


KEY_BIT = 0x80  # header byte 1 of packet format 2 (include/encx.h: KEY PACKET)


def check_key(use_lm: bool, lm_format: int):
    """Key packets exist in packet format 2 only: format 1 is the reference's header byte and has
    no spare bit, and a raw packet carries no context to restart. Raises ValueError; host only."""
    if not use_lm or lm_format != 2:
        raise ValueError('encx streaming: key packets (key, key_interval) go with use_lm=True, lm_format=2')


class _Packets:
    """What StreamPacker and StreamUnpacker share: the arguments, the LM session behind the
    LM-coded form, and for the raw form a slot table and byte buffers on the device, made at the
    first valid step (every refusal of a step's arguments is a pure host check). slot_n_q: the
    variable-bandwidth packets (two header bytes, K per slot from an nq table); n_q is then the
    largest K. fec: the redundant packets (four header bytes, a copy of up to fec codebooks of the
    slot's previous packet)."""

    def __init__(self, model, batch, n_q, use_lm, lm, max_frames, graphs, lm_session, slot_n_q=False, lm_format=1,
                 fec=None):
        if fec is not None:
            if use_lm:
                _refuse('redundant packets under the LM (a redundant copy would need an LM context of its own)')
            if not slot_n_q:
                raise ValueError('encx streaming: fec goes with slot_n_q=True (the copy has a codebook count of its own)')
            fec = operator.index(fec)
            if not 1 <= fec <= n_q:
                raise ValueError(f'encx streaming: fec {fec} (1..n_q={n_q})')
        self.fec = fec
        if use_lm and slot_n_q:
            _refuse('LM-coded packets with a per-slot n_q are not slot_n_q=True (the raw two-byte-header form) '
                    'with use_lm=True: pass use_lm=True, lm_format=2')
        if lm_format not in (1, 2):
            raise ValueError(f'encx streaming: lm_format {lm_format!r} (1 or 2)')
        if lm_format == 2 and not use_lm:
            raise ValueError('encx streaming: lm_format=2 is an LM-coded packet: it goes with use_lm=True')
        self.slot_n_q, self.lm_format = bool(slot_n_q), int(lm_format)
        # the header: the byte n, or the bytes (n, K) of the packets with a codebook count per slot
        self._hdr = 2 if self.slot_n_q or self.lm_format == 2 else 1
        self._packet_bytes = packet_bytes_nq if self._hdr == 2 else packet_bytes
        if not 1 <= batch <= MAX_BATCH:
            raise ValueError(f'encx streaming: batch {batch} (1..{MAX_BATCH})')
        if not 1 <= n_q <= min(model.quantizer.n_q, 64):
            raise ValueError(f'encx streaming: n_q {n_q} (the model has {model.quantizer.n_q} codebooks; at most 64)')
        if not 1 <= max_frames <= MAX_PACKET_FRAMES:
            raise ValueError(f'encx streaming: max_frames {max_frames} (1..{MAX_PACKET_FRAMES})')
        self.model, self.B, self.n_q = model, int(batch), int(n_q)
        self.max_frames, self.use_lm = int(max_frames), bool(use_lm)
        self.bits = int(model.bits_per_codebook)
        self._lm = None
        if self.use_lm:
            self._lm = lm_session(lm if lm is not None else model.get_lm_model(), self.B, self.n_q,
                                  self.max_frames, graphs, lm_format=self.lm_format)
        self._dev = None
        self._lost: tp.Set[int] = set()  # StreamUnpacker.lose: slots whose packets are dropped unread

    def reset(self):
        """Every slot starts a new stream with its next packet (the raw form carries no state)."""
        self._lost.clear()
        if self._lm is not None:
            self._lm.reset()

    def restart(self, slots):
        """As StreamEncoder.restart: the named slots' next packet begins a stream."""
        slots = check_restart(slots, self.B)
        self._lost.difference_update(slots)
        if self._lm is not None:
            self._lm.restart(slots)

    def _ensure(self):
        if self._dev is None:
            dev = next(self.model.parameters()).device
            if dev.type != 'cuda':
                raise RuntimeError('encx streaming runs on the GPU (no CPU fallback): move the model first')
            ensure_device(dev)
            self._stride = self._packet_bytes(self.max_frames, self.n_q, self.bits)
            if self.fec is not None:
                self._stride = packet_bytes_fec(self.max_frames, self.n_q, self.max_frames, self.fec, self.bits)
            self._slots = DeviceTable(self.B, 2, dev)
            self._nq = DeviceTable(self.B, 1, dev)
            self._bytes = torch.zeros(self.B, self._stride, dtype=torch.uint8, device=dev)
            self._nbytes = torch.zeros(self.B, dtype=torch.int64, device=dev)
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
            self._dev = dev

    def _put(self, frames, n_q):
        """The raw form's tables for this step: the slot table (no first-chunk flag: it carries
        no state) and, for variable-bandwidth packets, nq -> the kernel's nq argument, if any."""
        self._slots.put([(f, 0) for f in frames])
        if n_q is None:
            return ()
        self._nq.put(n_q)
        return (self._nq.data_ptr(),)


class StreamPacker(_Packets):
    """The codes of a slots step as one self-contained packet per delivering slot:

        packer = StreamPacker(model, batch=64, n_q=enc.n_q)            # or use_lm=True
        packets = packer.pack_slots(enc.encode_slots(x, frames), frames)   # list of bytes, b'' for 0 frames

    Raw: header byte + the bit-packed codes, ONE launch for all slots whatever their counts.
    use_lm=True: header byte + one arithmetic-coder run under `lm` (model.get_lm_model() when
    None), the LM's context carried across a slot's packets (encx.lm.LMStreamEncoder). The
    packet format is documented in include/encx.h. Slot b's codes past frames[b] are not read.
    use_lm=True, lm_format=2: pack_slots(codes, frames, n_q), the LM-coded packet with a codebook
    count per slot and step (two header bytes, short flush; n_q is then the session's largest);
    key_interval=N: every N-th packet of a slot, its first included, is a key packet.
    slot_n_q=True, fec=R (1..n_q): redundant packets, each with a copy of up to R codebooks of the
    slot's previous packet (module docstring)."""

    def __init__(self, model, batch: int, n_q: int, use_lm: bool = False, lm=None, max_frames: int = 8,
                 graphs: bool = True, slot_n_q: bool = False, lm_format: int = 1, fec: tp.Optional[int] = None,
                 key_interval: tp.Optional[int] = None):
        if key_interval is not None:
            check_key(use_lm, lm_format)
            key_interval = operator.index(key_interval)
            if key_interval < 1:
                raise ValueError(f'encx streaming: key_interval {key_interval} (at least 1 packet)')
        super().__init__(model, batch, n_q, use_lm, lm, max_frames, graphs, LMStreamEncoder, slot_n_q, lm_format, fec)
        self.key_interval = key_interval
        self._sent = [0] * self.B              # key packets: the slot's packets since its stream began
        self._owed: tp.Set[int] = set()        # key packets: slots restarted by a step that then raised
        self._prev = [(0, 0)] * self.B         # fec: (frames, K) of the slot's previous packet, (0, 0) for none
        self._par = [0] * self.B               # fec: the copy of the history that holds it (encx.h: fec[B][4])

    def reset(self):
        super().reset()
        self._sent, self._prev = [0] * self.B, [(0, 0)] * self.B
        self._owed.clear()

    def restart(self, slots):
        """As StreamEncoder.restart: the named slots' next packet begins a stream; it carries no
        redundant copy, and it counts as the first of its stream for key_interval."""
        super().restart(slots)
        for b in check_restart(slots, self.B):
            self._sent[b], self._prev[b] = 0, (0, 0)
            self._owed.discard(b)

    def _ensure(self):
        fresh = self._dev is None
        super()._ensure()
        if fresh and self.fec is not None:
            self._fec = DeviceTable(self.B, 4, self._dev)
            self._hist = torch.zeros(2, self.B, self.fec, self.max_frames, dtype=torch.int64, device=self._dev)

    def _keys(self, frames, key):
        """The slots whose packet of this step is a key packet: every key_interval-th of a stream,
        its first included, and those the caller names. Host data only."""
        if key is None and self.key_interval is None:
            return []
        check_key(self.use_lm, self.lm_format)
        frames = _ints(frames, 'frames')
        if key is not None:
            try:
                key = [bool(v) for v in key]
            except TypeError:
                raise ValueError('encx streaming: key must be a sequence of bools') from None
            if len(key) != self.B or len(frames) != self.B:
                raise ValueError(f'encx streaming: key for {len(key)} slots, the session has {self.B}')
        N = self.key_interval
        return [b for b, f in enumerate(frames[:self.B])
                if f and ((key is not None and key[b]) or (N is not None and self._sent[b] % N == 0)
                          or b in self._owed)]

    @torch.no_grad()
    def pack_slots(self, codes: torch.Tensor, frames: tp.Sequence[int], n_q: tp.Optional[tp.Sequence[int]] = None,
                   fec: tp.Optional[tp.Sequence[int]] = None, key: tp.Optional[tp.Sequence[bool]] = None) -> tp.List[bytes]:
        """slot_n_q=True: pack_slots(codes, frames, n_q) -> variable-bandwidth packets (include/encx.h):
        bytes (frames[b], n_q[b]) and the payload of codes[b, :n_q[b], :frames[b]]; rows k >= n_q[b]
        are not read.

        A packer built with fec=R: redundant packets. Each carries, behind its own codes, the first
        K_r = min(R, the K of the slot's previous packet) codebooks of that packet; fec: B ints in
        0..R, K_r = min(fec[b], previous K) instead, 0 for no copy (entries at slots with 0 frames
        are ignored). One launch per step; a step that raises leaves the history as it was.

        lm_format=2: key: B bools; a slot's packet is a key packet where key[b] is set or the
        packer's key_interval says so: its LM context is restarted first and bit 7 of byte 1 set."""
        if (self.slot_n_q or self.lm_format == 2) != (n_q is not None):
            raise ValueError('encx streaming: n_q goes with slot_n_q=True or lm_format=2, and only with them')
        if fec is not None and self.fec is None:
            raise ValueError('encx streaming: fec goes with a packer built with fec=R')
        keys = self._keys(frames, key)
        if self._lm is not None:
            if keys:
                # restarted here, flagged below: a step that raises in between still owes the flag
                self._lm.restart(keys)
                self._owed.update(keys)
            packets = self._lm.packets(codes, frames, n_q)
            for b in keys:
                packets[b] = packets[b][:1] + bytes([packets[b][1] | KEY_BIT]) + packets[b][2:]
            self._owed.difference_update(keys)
            if self.key_interval is not None:
                self._sent = [c + bool(p) for c, p in zip(self._sent, packets)]
            return packets
        frames = _ints(frames, 'frames')
        n_max, _ = check_frames([True] * self.B, frames, 1, self.max_frames)
        if n_q is not None:
            n_q = check_n_q(frames, n_q, self.n_q)
        if self.fec is not None:
            fec = check_fec(frames, fec, self.fec)
        if codes.dim() != 3 or tuple(codes.shape) != (self.B, self.n_q, n_max) or codes.dtype != torch.int64:
            raise ValueError(f'encx streaming: expected int64 codes [{self.B}, {self.n_q}, max(frames) = {n_max}], '
                             f'got {codes.dtype} {tuple(codes.shape)}')
        if not codes.is_cuda:
            raise RuntimeError('encx streaming takes device tensors (no CPU fallback)')
        self._ensure()
        nq = self._put(frames, n_q)
        self._err.zero_()
        sb, sk, s_t = codes.stride()
        if self.fec is not None:
            # the copy: the previous packet's frames at min(fec[b], its K) codebooks, none at 0
            red = [(n, min(r, K)) if min(r, K) else (0, 0) for r, (n, K) in zip(fec, self._prev)]
            self._fec.put((n_r, K_r, par, 0) for (n_r, K_r), par in zip(red, self._par))
            call('encx_bitpack_slots_fec', codes.data_ptr(), sb, sk, s_t, self.B, self.n_q, n_max, self.bits,
                 self.fec, self.max_frames, self._slots.data_ptr(), *nq, self._fec.data_ptr(),
                 self._hist.data_ptr(), self._bytes.data_ptr(), self._stride, self._nbytes.data_ptr(),
                 self._err.data_ptr(), stream())
        else:
            call('encx_bitpack_slots_nq' if nq else 'encx_bitpack_slots', codes.data_ptr(), sb, sk, s_t, self.B,
                 self.n_q, n_max, self.bits, self._slots.data_ptr(), *nq, self._bytes.data_ptr(), self._stride,
                 self._nbytes.data_ptr(), self._err.data_ptr(), stream())
        host = self._bytes.cpu()
        if int(self._err.item()):
            raise ValueError(f'encx streaming: a delivered code does not fit in {self.bits} bits')
        bits = self.bits
        if self.fec is not None:
            # the slots that delivered now read the copy of the history this step wrote
            for b, (f, q) in enumerate(zip(frames, n_q)):
                if f:
                    self._prev[b], self._par[b] = (f, q), self._par[b] ^ 1
            return [host[b, :packet_bytes_fec(f, q, n_r, K_r, bits)].numpy().tobytes() if f else b''
                    for b, (f, q, (n_r, K_r)) in enumerate(zip(frames, n_q, red))]
        size = self._packet_bytes
        return [host[b, :size(f, q, bits)].numpy().tobytes() if f else b''
                for b, (f, q) in enumerate(zip(frames, n_q or [self.n_q] * self.B))]


class StreamUnpacker(_Packets):
    """The inverse of StreamPacker: unpack_slots(packets) -> (codes [B, n_q, max(frames)] int64 on
    the GPU, zero past each slot's count, and frames), ready for StreamDecoder.decode_slots. A slot
    with nothing to deliver passes b''. A bad LM packet is data: its slot comes back with 0 frames
    and zero codes, is listed in `failed`, and refuses packets until restart([b]).
    use_lm=True, lm_format=2: -> (codes [B, n_q, max(frames)], frames, n_q) from the LM-coded
    packets with a count per slot, ready for StreamDecoder.decode_slots(codes, frames, n_q=n_q); a
    failed slot comes back with 0 frames, 0 codebooks and zero codes; a key packet restarts its
    slot's LM context in band.
    slot_n_q=True, fec=R: redundant packets; unpack_slots(packets, recover=[...]) decodes the copy
    of a lost step from the slot's next packet."""

    def __init__(self, model, batch: int, n_q: int, use_lm: bool = False, lm=None, max_frames: int = 8,
                 graphs: bool = True, slot_n_q: bool = False, lm_format: int = 1, fec: tp.Optional[int] = None):
        super().__init__(model, batch, n_q, use_lm, lm, max_frames, graphs, LMStreamDecoder, slot_n_q, lm_format, fec)

    @property
    def failed(self) -> tp.List[int]:
        return sorted(self._lm.failed) if self._lm is not None else []

    def lose(self, slots):
        """A packet of each named slot did not arrive. With use_lm=True the slot's LM context no
        longer matches the sender's, so the slot joins `failed`, and until restart([b]) its
        packets are dropped unread: they come back with 0 frames and zero codes, the other slots
        decode, and nothing is decoded under a context the sender does not share (packet_frames
        tells how many frames to conceal for such a packet). A raw packet carries no state:
        without an LM this only checks the indices. Recovery: packer.restart([b]) and
        unpacker.restart([b]) once the sender knows, which restarts the LM context only; the
        encoder and the decoder go on (module docstring)."""
        slots = check_restart(slots, self.B)
        if self._lm is not None:
            self._lost.update(slots)
            self._lm.lose(slots)

    def _key_slots(self, packets):
        """The slots whose packet has the key bit set (packet format 2 only; a packet that is not
        bytes, or has no byte 1, is left to _headers)."""
        if self.lm_format != 2:
            return []
        return [b for b, p in enumerate(packets)
                if isinstance(p, (bytes, bytearray)) and len(p) >= 2 and p[1] & KEY_BIT]

    def _drop_lost(self, packets, keys=()):
        """The packets with those of the lost slots replaced by b'' (unread), or None when that
        leaves no packet at all. keys: slots whose packet is a key packet; it is read."""
        if not self._lost or len(packets) != self.B:
            return packets
        kept = [b'' if b in self._lost and b not in keys else p for b, p in enumerate(packets)]
        if any(len(p) for p in packets if isinstance(p, (bytes, bytearray))) and \
                not any(len(p) for p in kept if isinstance(p, (bytes, bytearray))):
            return None
        return kept

    def _headers(self, packets):
        """The headers of a step's packets, the byte n or the bytes (n, K) -> (frames, n_q), 0 and
        0 for b''. With the one-byte header K is the session's n_q."""
        if len(packets) != self.B:
            raise ValueError(f'encx streaming: packets for {len(packets)} slots, the session has {self.B}')
        frames, n_q = [], []
        hdr, K_max, raw = self._hdr, self.n_q, not self.use_lm
        for b, p in enumerate(packets):
            if not isinstance(p, (bytes, bytearray)):
                raise ValueError(f'encx streaming: the packet of slot {b} is not bytes')
            n = K = 0
            if len(p):
                if len(p) < hdr:
                    raise ValueError(f'encx streaming: the packet of slot {b} has no (n, K) header')
                n, K = p[0], p[1] if hdr == 2 else K_max
                if self.lm_format == 2:
                    K &= ~KEY_BIT
                if not 1 <= n <= self.max_frames:
                    raise ValueError(f'encx streaming: the packet of slot {b} announces {n} frames '
                                     f'(1..max_frames={self.max_frames})')
                if not 1 <= K <= K_max:
                    raise ValueError(f'encx streaming: the packet of slot {b} announces {K} codebooks '
                                     f'(1..n_q={K_max})')
                if raw and len(p) != self._packet_bytes(n, K, self.bits):
                    raise ValueError(f'encx streaming: a raw packet of {n} frames of {K} codebooks in slot {b} has '
                                     f'{self._packet_bytes(n, K, self.bits)} bytes, not {len(p)}')
                if self.lm_format == 2 and len(p) - 2 > self._lm.cap:
                    raise ValueError(f'encx streaming: a payload of {len(p) - 2} bytes in slot {b}; no packet of '
                                     f'up to {self.max_frames} frames has more than {self._lm.cap}')
            frames.append(n)
            n_q.append(K)
        if not any(frames):
            raise ValueError('encx streaming: no slot delivers a frame')
        return frames, n_q

    _headers_nq = _headers  # its name for the (n, K) form

    def _upload(self, packets):
        host = torch.zeros(self.B, self._stride, dtype=torch.uint8)
        for b, p in enumerate(packets):
            if len(p):
                host[b, :len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8)
        self._bytes.copy_(host)

    def _sections(self, packets, recover):
        """The headers (n, K, n_r, K_r) of a step's redundant packets -> (frames, n_q, payloads):
        per slot the section asked for, the main one or with recover[b] the copy of the slot's
        previous packet, as the payload of a variable-bandwidth packet; (0, 0, b'') for b'' and for
        a copy the packet does not carry. Raises ValueError; host data only."""
        if len(packets) != self.B:
            raise ValueError(f'encx streaming: packets for {len(packets)} slots, the session has {self.B}')
        if recover is None:
            recover = [False] * self.B
        else:
            try:
                recover = [bool(v) for v in recover]
            except TypeError:
                raise ValueError('encx streaming: recover must be a sequence of bools') from None
            if len(recover) != self.B:
                raise ValueError(f'encx streaming: recover for {len(recover)} slots, the session has {self.B}')
        frames, n_q, payloads = [], [], []
        bits = self.bits
        for b, p in enumerate(packets):
            if not isinstance(p, (bytes, bytearray)):
                raise ValueError(f'encx streaming: the packet of slot {b} is not bytes')
            n = K = 0
            pay = b''
            if len(p):
                if len(p) < 4:
                    raise ValueError(f'encx streaming: the packet of slot {b} has no (n, K, n_r, K_r) header')
                n, K, n_r, K_r = p[:4]
                if not 1 <= n <= self.max_frames or n_r > self.max_frames:
                    raise ValueError(f'encx streaming: the packet of slot {b} announces {n} frames and a copy of '
                                     f'{n_r} (1..max_frames={self.max_frames})')
                if not 1 <= K <= self.n_q or K_r > self.n_q:
                    raise ValueError(f'encx streaming: the packet of slot {b} announces {K} codebooks and a copy of '
                                     f'{K_r} (1..n_q={self.n_q})')
                if (n_r == 0) != (K_r == 0):
                    raise ValueError(f'encx streaming: the packet of slot {b} announces a copy of {n_r} frames of '
                                     f'{K_r} codebooks')
                if len(p) != packet_bytes_fec(n, K, n_r, K_r, bits):
                    raise ValueError(f'encx streaming: a redundant packet of {n} x {K} and {n_r} x {K_r} codes in slot '
                                     f'{b} has {packet_bytes_fec(n, K, n_r, K_r, bits)} bytes, not {len(p)}')
                split = 4 + (n * K * bits + 7) // 8
                if recover[b]:
                    n, K, pay = n_r, K_r, bytes(p[split:])
                else:
                    pay = bytes(p[4:split])
            frames.append(n)
            n_q.append(K)
            payloads.append(pay)
        if not any(len(p) for p in packets):
            raise ValueError('encx streaming: no slot delivers a frame')
        return frames, n_q, payloads

    @torch.no_grad()
    def unpack_slots(self, packets: tp.Sequence[bytes], recover: tp.Optional[tp.Sequence[bool]] = None):
        """slot_n_q=True: -> (codes [B, n_q, max(frames)], frames, n_q) from variable-bandwidth
        packets, n_q[b] = 0 for an empty packet and zero rows at k >= n_q[b]: ready for
        StreamDecoder.decode_slots(codes, frames, n_q).

        An unpacker built with fec=R takes redundant packets and decodes their main sections.
        recover: B bools; recover[b] says packets[b] is the slot's NEXT packet and the step before
        it, which was lost, is wanted: the slot comes back with the frames, n_q and codes of the
        redundant copy, (0, 0) and zero codes when the packet carries none.

        lm_format=2: a key packet (bit 7 of byte 1) restarts the slot's LM context before it is
        decoded and takes the slot out of the lost and failed sets, whether it was lost or not."""
        if self.fec is not None:
            return self._unpack_fec(packets, recover)
        if recover is not None:
            raise ValueError('encx streaming: recover goes with an unpacker built with fec=R')
        keys = self._key_slots(packets)
        packets = self._drop_lost(packets, keys)
        if packets is None:  # every packet of the step belongs to a lost slot: nothing to decode
            codes = torch.zeros(self.B, self.n_q, 0, dtype=torch.int64, device=next(self.model.parameters()).device)
            return (codes, [0] * self.B, [0] * self.B) if self.lm_format == 2 else (codes, [0] * self.B)
        frames, n_q = self._headers(packets)
        if keys:  # an in-band restart([b]): the sender did restart, so this side does too
            self.restart(keys)
        if self._lm is not None:
            codes, failed = self._lm.decode_slots([bytes(p[self._hdr:]) for p in packets], frames,
                                                  n_q if self._hdr == 2 else None)
            frames, n_q = ([0 if b in failed else v for b, v in enumerate(vs)] for vs in (frames, n_q))
        else:
            n_max = max(frames)
            self._ensure()
            self._upload(packets)
            nq = self._put(frames, n_q if self._hdr == 2 else None)
            codes = torch.empty(self.B, self.n_q, n_max, dtype=torch.int64, device=self._dev)
            sb, sk, s_t = codes.stride()
            call('encx_bitunpack_slots_nq' if nq else 'encx_bitunpack_slots', self._bytes.data_ptr() + self._hdr,
                 self._stride, self.B, self.n_q, n_max, self.bits, self._slots.data_ptr(), *nq, codes.data_ptr(),
                 sb, sk, s_t, stream())
        return (codes, frames, n_q) if self._hdr == 2 else (codes, frames)

    def _unpack_fec(self, packets, recover):
        """unpack_slots for redundant packets: the host copies the section each slot asked for to
        the start of its row of the staging buffer, and the variable-bandwidth unpacker reads it."""
        frames, n_q, payloads = self._sections(packets, recover)
        n_max = max(frames)
        dev = next(self.model.parameters()).device
        if not n_max:  # only copies were asked for, and no packet carries one
            return torch.zeros(self.B, self.n_q, 0, dtype=torch.int64, device=dev), frames, n_q
        self._ensure()
        self._upload(payloads)
        nq = self._put(frames, n_q)
        codes = torch.empty(self.B, self.n_q, n_max, dtype=torch.int64, device=self._dev)
        sb, sk, s_t = codes.stride()
        call('encx_bitunpack_slots_nq', self._bytes.data_ptr(), self._stride, self.B, self.n_q, n_max, self.bits,
             self._slots.data_ptr(), *nq, codes.data_ptr(), sb, sk, s_t, stream())
        return codes, frames, n_q


# ---------------------------------------------------------------------------- the receiver's recipe
class StreamReceiver:
    """What a receiver with a one-step jitter buffer does with redundant packets, as code:

        rx = StreamReceiver(StreamDecoder(model, B, n_q), StreamUnpacker(model, B, n_q, slot_n_q=True, fec=R))
        wav, status = rx.step(packets, ahead, lost_frames)

    Per slot packets[b] is this step's packet, b'' for a slot that sits out, None for a packet
    that did not arrive; ahead[b] is the slot's next packet where the jitter buffer already holds
    it, else None; lost_frames[b] is the number of frames to conceal when nothing recovers the step
    (the transport knows it from timing). A packet that is there is decoded from its main section;
    a lost one from the redundant copy in ahead[b], at the copy's codebook count; where there is
    none the decoder conceals lost_frames[b] frames. At most one unpack_slots and one decode_slots
    call per step. -> (wav [B, C, max frames * hop], status): per slot 'main', 'recovered',
    'concealed' or 'idle'. Sequence numbers and detecting a loss stay the transport's job."""

    def __init__(self, decoder, unpacker):
        self.decoder, self.unpacker = decoder, unpacker

    def step(self, packets, ahead, lost_frames):
        B = len(packets)
        if len(ahead) != B or len(lost_frames) != B:
            raise ValueError(f'encx streaming: packets for {B} slots, ahead for {len(ahead)}, lost_frames for '
                             f'{len(lost_frames)}')
        status = ['idle'] * B
        chosen, recover = [b''] * B, [False] * B
        for b, p in enumerate(packets):
            if p is None:
                status[b] = 'concealed'
                if ahead[b] is not None and len(ahead[b]):
                    chosen[b], recover[b] = ahead[b], True
            elif len(p):
                status[b], chosen[b] = 'main', p
        codes, frames, n_q = None, [0] * B, [0] * B
        if any(len(p) for p in chosen):
            codes, frames, n_q = self.unpacker.unpack_slots(chosen, recover)
            frames, n_q = list(frames), list(n_q)
        lost = [False] * B
        for b in range(B):
            if recover[b] and frames[b]:
                status[b] = 'recovered'
            elif status[b] == 'concealed':
                frames[b], n_q[b], lost[b] = operator.index(lost_frames[b]), 0, True
        n_max = max(frames)
        if codes is not None and not any(f and not gone for f, gone in zip(frames, lost)):
            codes = None  # every slot with frames is concealed
        elif codes is not None and codes.shape[2] < n_max:
            # a concealed slot has more frames than any packet of the step: its columns are not read
            codes = torch.nn.functional.pad(codes, (0, n_max - codes.shape[2]))
        wav = self.decoder.decode_slots(codes, frames, n_q=n_q, lost=lost if any(lost) else None)
        return wav, status
