"""Streaming codec: stateful chunked encode / decode of the causal EnCodec model.

A causal codec can run live: delivered in chunks, it produces exactly what the offline model
produces on the whole clip. `StreamEncoder` / `StreamDecoder` keep the state that makes this so
between calls, for `batch` live streams that advance together, one step per chunk:

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

Inference only. Weight-normed weights are prepared once, at construction; call
refresh_weights() after changing the model. All streams of a session start together (reset());
restarting one slot is not supported.
"""
import dataclasses
import typing as tp

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import call, stream, ensure_device
from .modules.conv import SConv1d, SConvTranspose1d
from .modules.lstm import SLSTM
from .modules.seanet import SEANetEncoder, SEANetResnetBlock

MAX_BATCH = ops.LSTM_MAX_BATCH
MAX_HISTORY = 64  # encx_stream_roll moves a window row as one wave


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
        self._tables: tp.Dict[int, tuple] = {}
        self._graphs: tp.Dict[tuple, tuple] = {}
        self.started = False
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
        """Start a new session: every stream's history and LSTM state cleared."""
        self._arena.zero_()
        self.started = False

    def _check_chunk(self, n):
        if n < 1 or n > self.max_frames:
            raise ValueError(f'encx streaming: a chunk of {n} frames (1..max_frames={self.max_frames})')
        if not self.started and n < self.min_first_frames:
            raise ValueError(f'encx streaming: the first chunk of a session needs at least '
                             f'{self.min_first_frames} frames (got {n})')

    # ---- roll tables
    def _table(self, n):
        """Device tables of encx_stream_win for chunks of n frames: all windows that carry a
        history (the end-of-step roll) and the same entries one by one (the first chunk's
        reflect fills). Built on the host, so outside any capture."""
        t = self._tables.get(n)
        if t is None:
            rows, full, single, index = 0, [], [], {}
            for wi, (w, W, buf) in enumerate(zip(self.plan.windows, self._W, self.bufs)):
                if not w.P:
                    continue
                index[wi] = len(full)
                e = [buf.data_ptr(), self.B * w.C, w.P, n * w.rate, W]
                full.append(e + [rows])
                single.append(e + [0])
                rows += self.B * w.C
            tab = torch.tensor(np.array(full + single, dtype=np.int64)).to(self.dev)
            t = self._tables[n] = (tab, len(full), rows, index)
        return t

    def _reflect(self, n, wi, st):
        w = self.plan.windows[wi]
        if not w.P or w.fill != 'reflect':
            return
        tab, nfull, _, index = self._table(n)
        call('encx_stream_roll', tab.data_ptr() + 48 * (nfull + index[wi]), 1, self.B * w.C, 1, st)

    # ---- one step
    def _layers(self, n, first):
        st = stream()
        ws, Ws, bufs, B = self.plan.windows, self._W, self.bufs, self.B
        if first:
            self._reflect(n, 0, st)
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
                call('encx_stream_lstm', bufs[L.src].data_ptr() + 4 * s.P, m['wcatT'].data_ptr(),
                     m['bsum'].data_ptr(), m['hz'].data_ptr(), m['c'].data_ptr(), m['gates'].data_ptr(), y,
                     int(bool(L.module.skip)), B, n * s.rate, L.Cin, L.module.lstm.num_layers, s.C * Ws_, Ws_,
                     d.C * Wd, Wd, st)
            if first and L.final:
                self._reflect(n, L.dst, st)
        tab, nfull, rows, _ = self._table(n)
        if nfull:
            call('encx_stream_roll', tab.data_ptr(), nfull, rows, 0, st)

    def _step(self, n, body):
        """Run body(n, first) eagerly, or as the graph captured for (n, first) the first time."""
        first = not self.started
        self._table(n)
        if not self.graphs:
            out = body(n, first)
        else:
            ent = self._graphs.get((n, first))
            if ent is None:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):  # one stream: the graph has no parallel branches
                    res = body(n, first)
                ent = self._graphs[(n, first)] = (g, res)
            ent[0].replay()
            out = tuple(t.clone() for t in ent[1])  # the graph's outputs are rewritten by its next replay
        self.started = True
        return out

    def _warm(self, body):
        """Load every kernel of a step before any capture: one first chunk and one later chunk on
        the zero state, eagerly; then back to a clean session."""
        graphs, self.graphs = self.graphs, False
        try:
            self._step(self.min_first_frames, body)
            self._step(1, body)
        finally:
            self.graphs = graphs
        self.reset()


def _embeds(model, n_q):
    layers = model.quantizer.vq.layers
    if not 1 <= n_q <= len(layers):
        raise ValueError(f'encx streaming: n_q {n_q} (the model has {len(layers)} codebooks)')
    return [l._codebook.embed for l in layers[:n_q]]


class StreamEncoder:
    """Chunked encoder of a causal model for `batch` streams: encode(x [B, C, n*hop]) -> codes
    [B, n_q, n] (int64), n_q from model.bandwidth at construction. See the module docstring."""

    def __init__(self, model, batch: int, max_frames: int = 8, graphs: bool = True):
        plan = encoder_plan(model)
        self.n_q = model.quantizer.get_num_quantizers_for_bandwidth(model.frame_rate, model.bandwidth)
        self._s = _Session(model, plan, batch, max_frames, graphs)
        self.channels = model.channels
        self._embeds = _embeds(model, self.n_q)
        with torch.no_grad():
            self._s._warm(self._body)

    hop_length = property(lambda self: self._s.hop_length)
    min_first_frames = property(lambda self: self._s.min_first_frames)
    plan = property(lambda self: self._s.plan)

    def reset(self):
        self._s.reset()

    def refresh_weights(self):
        self._s.refresh_weights()
        self._embeds = _embeds(self._s.model, self.n_q)

    def _body(self, n, first):
        s = self._s
        s._layers(n, first)
        # a copy, never a view: the window is rewritten by the next step
        emb = s.bufs[s.plan.layers[-1].dst][:, :, :n].clone(memory_format=torch.contiguous_format)
        codes = ops.rvq_encode(emb, self._embeds).permute(1, 0, 2).contiguous()
        return codes, emb

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_latent: bool = False):
        """x [B, C, n * hop_length] float32 on the model's device -> codes [B, n_q, n] (and the
        latent [B, D, n] with return_latent). Equals the offline model on the audio so far."""
        s = self._s
        if x.dim() != 3 or x.shape[0] != s.B or x.shape[1] != self.channels or x.shape[2] % s.hop_length:
            raise ValueError(f'encx streaming: expected [{s.B}, {self.channels}, n * {s.hop_length}] samples, '
                             f'got {tuple(x.shape)}')
        n = x.shape[2] // s.hop_length
        s._check_chunk(n)
        ops._check(x)
        P = s.plan.windows[0].P
        s.bufs[0][:, :, P:P + x.shape[2]].copy_(x)
        codes, emb = s._step(n, self._body)
        return (codes, emb) if return_latent else codes


class StreamDecoder:
    """Chunked decoder of a causal model for `batch` streams: decode(codes [B, n_q, n]) -> wav
    [B, C, n * hop_length]. See the module docstring."""

    def __init__(self, model, batch: int, n_q: int, max_frames: int = 8, graphs: bool = True):
        plan = decoder_plan(model)
        self.n_q = int(n_q)
        if not 1 <= self.n_q <= model.quantizer.n_q:
            raise ValueError(f'encx streaming: n_q {n_q} (the model has {model.quantizer.n_q} codebooks)')
        self._s = _Session(model, plan, batch, max_frames, graphs)
        self.channels = model.channels
        self.bins = model.quantizer.bins
        self._embeds = _embeds(model, self.n_q)
        self._codes: tp.Dict[int, torch.Tensor] = {}
        with torch.no_grad():
            self._s._warm(self._body)

    hop_length = property(lambda self: self._s.hop_length)
    min_first_frames = property(lambda self: self._s.min_first_frames)
    plan = property(lambda self: self._s.plan)

    def reset(self):
        self._s.reset()

    def refresh_weights(self):
        self._s.refresh_weights()
        self._embeds = _embeds(self._s.model, self.n_q)

    def _code_buf(self, n):
        c = self._codes.get(n)
        if c is None:
            c = self._codes[n] = torch.zeros(self.n_q, self._s.B, n, device=self._s.dev, dtype=torch.int64)
        return c

    def _body(self, n, first):
        s = self._s
        q = ops.rvq_decode(self._code_buf(n), self._embeds)
        P = s.plan.windows[0].P
        s.bufs[0][:, :, P:P + n].copy_(q)
        s._layers(n, first)
        # a copy, never a view: the window is rewritten by the next step
        out = s.bufs[s.plan.layers[-1].dst][:, :, :n * s.hop_length]
        return (out.clone(memory_format=torch.contiguous_format),)

    @torch.no_grad()
    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [B, n_q, n] int64 on the model's device -> wav [B, C, n * hop_length]. Equals
        the offline decoder on the codes so far. Codes are clamped to the codebook size."""
        s = self._s
        if codes.dim() != 3 or codes.shape[0] != s.B or codes.shape[1] != self.n_q or codes.dtype != torch.int64:
            raise ValueError(f'encx streaming: expected int64 codes [{s.B}, {self.n_q}, n], got '
                             f'{codes.dtype} {tuple(codes.shape)}')
        n = codes.shape[2]
        s._check_chunk(n)
        if not codes.is_cuda:
            raise RuntimeError('encx streaming takes device tensors (no CPU fallback)')
        buf = self._code_buf(n)
        buf.copy_(codes.permute(1, 0, 2))
        buf.clamp_(0, self.bins - 1)  # an index outside the codebook must never reach the gather
        return s._step(n, self._body)[0]
