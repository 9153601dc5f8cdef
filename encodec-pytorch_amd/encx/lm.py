"""LMModel of the reference (model.py:27-65) over StreamingTransformerEncoder
(modules/transformer.py:62-119), on the encx HIP kernels (csrc/lm.hip, csrc/ac.hip).

The module tree (and so the state dict) is the reference's: `transformer.norm_in`,
`transformer.layers.{i}.self_attn.{in_proj_weight,in_proj_bias,out_proj}`, `linear1`,
`linear2`, `norm1`, `norm2`, `emb.{k}`, `linears.{k}`; torch modules serve only as parameter
holders and no torch arithmetic runs. `forward(indices, states, offset)` keeps the reference's
streaming contract; `states` is an opaque `LMState` (each layer's key/value cache) instead of
the list of past layer inputs, and is passed back the same way.

`encode_streams` / `decode_streams` are the entropy coder of compress.py:67-89 / 128-155 for a
batch of equal-shape frames: the encoder runs all T steps of a frame as one pass (every code
is known), the decoder one step per launch sequence; csrc/lm.hip computes every row in a
fixed order that does not depend on the rows sharing the launch, so both sides produce the
same cdfs bit for bit.

`LMStreamEncoder` / `LMStreamDecoder` are the same coder for live streams (the slots of
encx/streaming.py): one flushed coder run per slot and step, the LM's position, last codes and
key/value ring carried per slot on the device, so a stream has no length limit and a captured
step replays whatever the slots deliver. With lm_format=2 every slot and step has its own
codebook count n_q[b] <= K (packet format 2 of include/encx.h: the LM row sums the embeddings of
the codebooks the packet carries, a codebook the previous frame lacked enters with the start
index, and the coder run ends with the short flush); the counts are a second device table, so
the same graphs serve any mix.

`nll(codes)` trains the LM (csrc/lm_train.hip): the teacher-forced forward is the encoder's own
pass, so the loss is the log-probability the arithmetic coder will see, and one autograd Function
runs the hand-written backward and hands every parameter its gradient.
"""
import typing as tp

import torch
from torch import nn

from ._lib import call, lib, stream, ensure_device, ENCX_AC_POS
from .ac import new_decoder_state
from .slots import DeviceTable, _ints, check_frames, check_n_q, check_restart

TOTAL_RANGE_BITS = 24   # ArithmeticCoder default (ac.py:96), as compress.py uses it
ROUNDOFF = 1e-8         # build_stable_quantized_cdf defaults (ac.py:18-20)
MIN_RANGE = 2

# The limits of csrc/lm.hip. The reference builds an LM of any size; these are this port's.
MAX_DIM = 512           # LayerNorm holds a row in one wave, 8 values per lane
MAX_HEAD_DIM = 64       # the attention kernels' widest instantiation
MAX_CARD = 65536        # encx_lm_heads
MAX_CODEBOOKS = 64      # the input stage fetches one index per lane
MAX_ATTN_LDS = 150 * 1024   # the few-row attention kernel keeps its window's weights and values in LDS


def _check_window(tr, rows):
    """The few-row attention kernel holds `rows` key positions x (1 + head dim) floats in LDS."""
    hd = tr.dim // tr.num_heads
    need = rows * (hd + 1) * 4
    if need > MAX_ATTN_LDS:
        raise ValueError(f'encx LM: an attention window of {rows} positions at head dim {hd} needs {need} bytes of '
                         f'LDS, above this port\'s limit of {MAX_ATTN_LDS} (the reference has none): past_context '
                         f'{tr.past_context} is too long for dim {tr.dim} with {tr.num_heads} heads')


class StreamingTransformerEncoderLayer(nn.Module):
    """Parameter holder with nn.TransformerEncoderLayer's names (transformer.py:30)."""

    def __init__(self, d_model, nhead, dim_feedforward):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, batch_first=True)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)


class StreamingTransformerEncoder(nn.Module):
    """transformer.py:62-99 (post-norm layers, GELU, LayerNorm input, no dropout)."""

    def __init__(self, dim, hidden_scale: float = 4., num_heads: int = 8, num_layers: int = 5,
                 max_period: float = 10000, past_context: int = 1000, gelu: bool = True,
                 norm_in: bool = True, dropout: float = 0., **kwargs):
        super().__init__()
        if dim < 4 or dim > MAX_DIM or dim % 2:
            raise ValueError(f'encx LM: dim {dim}; this port takes an even dim in 4..{MAX_DIM} (the reference any)')
        assert dim % num_heads == 0
        if dim // num_heads > MAX_HEAD_DIM:
            raise ValueError(f'encx LM: head dim {dim // num_heads} (dim {dim} / {num_heads} heads); this port takes '
                             f'head dims up to {MAX_HEAD_DIM} (the reference any)')
        if past_context < 0:
            raise ValueError(f'encx LM: past_context {past_context} is negative')
        if not gelu or not norm_in or dropout or kwargs:
            raise NotImplementedError('encx LM: GELU, norm_in and dropout 0 only (the configuration '
                                      'EncodecModel.get_lm_model builds, model.py:224-225)')
        self.dim, self.num_heads = dim, num_heads
        self.hidden = int(dim * hidden_scale)
        self.max_period = max_period
        self.past_context = past_context
        self.norm_in = nn.LayerNorm(dim)
        self.layers = nn.ModuleList([StreamingTransformerEncoderLayer(dim, num_heads, self.hidden)
                                     for _ in range(num_layers)])


class LMState:
    """Streaming state: per layer a key/value cache [B][capacity][2*dim] of sequence positions
    0 (the zero initial state, transformer.py:106) .. offset, and the step offset."""

    def __init__(self, B, num_layers, dim, capacity, device):
        self.B, self.dim = B, dim
        self.kv = [torch.empty(B, capacity, 2 * dim, device=device) for _ in range(num_layers)]
        self.offset = 0

    @property
    def capacity(self):
        return self.kv[0].shape[1]

    def reserve(self, n):
        if n > self.capacity:
            cap = max(n, 2 * self.capacity)
            for i, kv in enumerate(self.kv):
                nkv = torch.empty(self.B, cap, 2 * self.dim, device=kv.device)
                nkv[:, :self.offset + 1] = kv[:, :self.offset + 1]
                self.kv[i] = nkv


class _NLLFn(torch.autograd.Function):
    """LMModel.nll: the coding forward with every layer's workspace and cache kept, the fused
    cross-entropy + gradient and the heads backward chunk by chunk in the forward (the logits
    never exist whole), the layers and the input stage in the backward."""

    @staticmethod
    def forward(ctx, lm, codes, chunk_floats, *params):
        tr = lm.transformer
        B, K, T = codes.shape
        N, D, Fh, card = B * T, lm.dim, tr.hidden, lm.card
        dev = codes.device
        st = stream()
        f32 = lambda nbytes: torch.empty((int(nbytes) + 3) // 4, device=dev)
        need = any(ctx.needs_input_grad)  # False under no_grad: the loss alone
        sb, sk, s_t = codes.stride()
        state = lm.new_state(B, T + 1)
        x = torch.empty(N, D, device=dev)
        call('encx_lm_input', codes.data_ptr(), sb, sk, s_t, B, K, T, 1, lm._emb.data_ptr(), card + 1, D,
             tr.norm_in.weight.data_ptr(), tr.norm_in.bias.data_ptr(), 0, None, float(tr.max_period),
             x.data_ptr(), st)
        xs, works = [x], []
        for i, layer in enumerate(tr.layers):
            if need or not works:
                works.append(f32(lib.encx_lm_layer_workspace(N, D, Fh)))
            y = torch.empty_like(x)
            call('encx_lm_layer', x.data_ptr(), y.data_ptr(), B, T, state.kv[i].data_ptr(), state.capacity, 1, None,
                 tr.past_context, D, tr.num_heads, Fh, *_layer_ptrs(layer), works[-1].data_ptr(), st)
            xs.append(y)
            x = y
        # heads, loss and dlogits, heads backward: row chunks of whole rows
        rows = max(1, min(N, chunk_floats // (K * card)))
        logits = f32(lib.encx_lm_heads_workspace(rows, K, card))
        probas = torch.empty(rows * K * card, device=dev)
        ce = f32(lib.encx_lm_ce_workspace(N, K))
        scale = 1.0 / (N * K)
        if need:
            hw = f32(lib.encx_lm_heads_bwd_workspace(rows, D, K, card))
            dx = torch.empty(N, D, device=dev)
            g_w = torch.zeros(lm.n_q, card, D, device=dev) if K < lm.n_q else torch.empty(K, card, D, device=dev)
            g_b = torch.zeros(lm.n_q, card, device=dev) if K < lm.n_q else torch.empty(K, card, device=dev)
        for n0 in range(0, N, rows):
            r = min(rows, N - n0)
            xc = x.data_ptr() + n0 * D * 4
            call('encx_lm_heads', xc, 1, r, D, lm._lin_w.data_ptr(), lm._lin_b.data_ptr(), K, card,
                 logits.data_ptr(), probas.data_ptr(), None, TOTAL_RANGE_BITS, ROUNDOFF, MIN_RANGE, None, 0, 0, 0,
                 None, None, st)
            call('encx_lm_ce', logits.data_ptr(), n0, r, N, T, K, card, codes.data_ptr(), sb, sk, s_t, scale,
                 ce.data_ptr(), st)
            if need:
                call('encx_lm_heads_bwd', logits.data_ptr(), xc, r, D, lm._lin_w.data_ptr(), K, card,
                     dx.data_ptr() + n0 * D * 4, g_w.data_ptr(), g_b.data_ptr(), int(n0 > 0), hw.data_ptr(), st)
        out = torch.empty((), device=dev)
        # codes were range-checked before the first launch (LMModel.nll): the count is not read
        err = torch.empty(1, device=dev, dtype=torch.int32)
        call('encx_lm_ce_finish', ce.data_ptr(), N, K, scale, out.data_ptr(), err.data_ptr(), st)
        if need:
            ctx.lm, ctx.codes, ctx.xs, ctx.works, ctx.kv = lm, codes, xs, works, state.kv
            ctx.emb = lm._emb  # the stack this forward read (an optimiser step may follow)
            ctx.head_grads = (dx, g_w, g_b)
            # the backward reads the layers' live parameters (nothing is copied): see backward
            ctx.versions = [(p.data_ptr(), p._version) for p in params]
        return out

    @staticmethod
    def backward(ctx, g):
        lm, codes = ctx.lm, ctx.codes
        if ctx.head_grads is None:
            raise RuntimeError('encx LM: nll can be differentiated once (its saved activations are released by '
                               'the first backward; retain_graph is not supported): call nll again')
        if ctx.versions != [(p.data_ptr(), p._version) for p in lm._train_params()]:
            raise RuntimeError('encx LM: a parameter changed between nll() and backward(); the backward reads the '
                               'live parameters, so run backward before the optimiser step')
        tr = lm.transformer
        B, K, T = codes.shape
        N, D, Fh, card = B * T, lm.dim, tr.hidden, lm.card
        dev = codes.device
        st = stream()
        f32 = lambda nbytes: torch.empty((int(nbytes) + 3) // 4, device=dev)
        dy, g_w, g_b = ctx.head_grads
        # the loss's own scale 1 / (N K) is inside the kernels; the incoming grad multiplies on top.
        # Everything below is linear in the heads' three results, so scaling them scales every grad.
        dy, g_w, g_b = dy * g, g_w * g, g_b * g
        work = f32(lib.encx_lm_layer_bwd_workspace(B, T, D, tr.num_heads, Fh))
        layer_grads = []
        for i in reversed(range(len(tr.layers))):
            layer = tr.layers[i]
            a = layer.self_attn
            ps = [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, layer.linear1.weight,
                  layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm1.weight,
                  layer.norm1.bias, layer.norm2.weight, layer.norm2.bias]
            gs = [torch.empty_like(p) for p in ps]
            dx = torch.empty(N, D, device=dev)
            call('encx_lm_layer_bwd', dy.data_ptr(), dx.data_ptr(), ctx.xs[i].data_ptr(), B, T, ctx.kv[i].data_ptr(),
                 ctx.kv[i].shape[1], tr.past_context, D, tr.num_heads, Fh, a.in_proj_weight.data_ptr(),
                 a.in_proj_bias.data_ptr(), a.out_proj.weight.data_ptr(), layer.linear1.weight.data_ptr(),
                 layer.linear1.bias.data_ptr(), layer.linear2.weight.data_ptr(), layer.norm1.weight.data_ptr(),
                 layer.norm2.weight.data_ptr(), ctx.works[i].data_ptr(), *[t.data_ptr() for t in gs],
                 work.data_ptr(), st)
            layer_grads.append(gs)
            dy = dx
        g_nw, g_nb = torch.empty(D, device=dev), torch.empty(D, device=dev)
        g_emb = torch.zeros(lm.n_q, card + 1, D, device=dev) if K < lm.n_q \
            else torch.empty(K, card + 1, D, device=dev)
        sb, sk, s_t = codes.stride()
        iw = f32(lib.encx_lm_input_bwd_workspace(B, T, D, K))
        call('encx_lm_input_bwd', dy.data_ptr(), codes.data_ptr(), sb, sk, s_t, B, K, T, ctx.emb.data_ptr(), card + 1,
             D, tr.norm_in.weight.data_ptr(), g_emb.data_ptr(), g_nw.data_ptr(), g_nb.data_ptr(), iw.data_ptr(), st)
        grads = [g_nw, g_nb]
        for gs in reversed(layer_grads):
            grads += gs
        grads += list(g_emb.unbind(0)) + list(g_w.unbind(0)) + list(g_b.unbind(0))
        ctx.xs = ctx.works = ctx.kv = ctx.head_grads = None
        return (None, None, None, *grads)


def _layer_ptrs(layer):
    a = layer.self_attn
    return [t.data_ptr() for t in (a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                                   layer.linear1.weight, layer.linear1.bias, layer.linear2.weight,
                                   layer.linear2.bias, layer.norm1.weight, layer.norm1.bias, layer.norm2.weight,
                                   layer.norm2.bias)]


class LMModel(nn.Module):
    """model.py:27-45."""

    def __init__(self, n_q: int = 32, card: int = 1024, dim: int = 200, **kwargs):
        super().__init__()
        if not 1 <= card <= MAX_CARD:
            raise ValueError(f'encx LM: card {card}; this port takes 1..{MAX_CARD} (the reference any)')
        self.card = card
        self.n_q = n_q
        self.dim = dim
        self.transformer = StreamingTransformerEncoder(dim=dim, **kwargs)
        self.emb = nn.ModuleList([nn.Embedding(card + 1, dim) for _ in range(n_q)])
        self.linears = nn.ModuleList([nn.Linear(dim, card) for _ in range(n_q)])
        self._packed_key = None

    # ------------------------------------------------------------------ weights
    def invalidate_packed(self):
        """Forget the stacked copies of the embeddings and heads: the next call restacks them.
        The cache key below (data_ptr, _version) cannot see an optimiser that writes through raw
        pointers (FlatAdam / encx_adam_step), so `nll` restacks on every call and leaves the
        cache invalid behind it; call this after such a step taken without an `nll` since the
        last use of the model."""
        self._packed_key = None

    def _packed(self):
        """The K embedding tables and output heads stacked into contiguous [n_q][.][dim]
        buffers (rebuilt only when a parameter changes, see invalidate_packed)."""
        ps = [e.weight for e in self.emb] + [l.weight for l in self.linears] + [l.bias for l in self.linears]
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key != self._packed_key:
            with torch.no_grad():
                self._emb = torch.stack([e.weight for e in self.emb]).contiguous()
                self._lin_w = torch.stack([l.weight for l in self.linears]).contiguous()
                self._lin_b = torch.stack([l.bias for l in self.linears]).contiguous()
            self._packed_key = key
        return self._emb, self._lin_w, self._lin_b

    def _check_device(self):
        p = self._emb
        if not p.is_cuda or p.dtype != torch.float32:
            raise RuntimeError('encx LM: parameters must be float32 on the GPU (no CPU fallback)')
        ensure_device(p.device)
        for t in self.parameters():
            if not t.is_contiguous():
                raise RuntimeError('encx LM: parameters must be contiguous')

    def _check_codebooks(self, K):
        if K > self.n_q:
            raise ValueError(f'{K} codebooks for an LM of n_q={self.n_q}')
        if not 1 <= K <= MAX_CODEBOOKS:
            raise ValueError(f'encx LM: {K} codebooks in one call; this port takes 1..{MAX_CODEBOOKS} '
                             '(the reference any)')

    def new_state(self, B, capacity=64):
        tr = self.transformer
        return LMState(B, len(tr.layers), self.dim, max(int(capacity), 2), self._emb.device)

    # ------------------------------------------------------------------ core
    def _body(self, idx, strides, B, K, T, shifted, state: LMState, dev_step=None):
        """input + transformer over rows [B][T] continuing `state` -> x [B*T][dim]. With
        dev_step (an int64 device counter) the step offset is read on the device and the host
        offset stays put (a graph-captured decode step; the caller reserved the cache)."""
        tr = self.transformer
        D, Fh = self.dim, tr.hidden
        dev = self._emb.device
        st = stream()
        dptr = dev_step.data_ptr() if dev_step is not None else None
        # the few-row attention kernel (csrc/lm.hip lm_layer_run): its window is sized for the whole
        # past_context when the step is read on the device
        if dev_step is not None:
            _check_window(tr, tr.past_context + 1)
        elif B * T * tr.num_heads <= 4096:
            _check_window(tr, min(tr.past_context + 1, state.offset + 1 + T))
        if dev_step is None:
            state.reserve(state.offset + T + 1)
        x = torch.empty(B * T, D, device=dev)
        call('encx_lm_input', idx.data_ptr(), strides[0], strides[1], strides[2], B, K, T, int(shifted),
             self._emb.data_ptr(), self.card + 1, D, tr.norm_in.weight.data_ptr(), tr.norm_in.bias.data_ptr(),
             state.offset, dptr, float(tr.max_period), x.data_ptr(), st)
        work = torch.empty((int(lib.encx_lm_layer_workspace(B * T, D, Fh)) + 3) // 4, device=dev)
        for i, layer in enumerate(tr.layers):
            y = torch.empty_like(x)
            a = layer.self_attn
            call('encx_lm_layer', x.data_ptr(), y.data_ptr(), B, T, state.kv[i].data_ptr(), state.capacity,
                 state.offset + 1, dptr, tr.past_context, D, tr.num_heads, Fh,
                 a.in_proj_weight.data_ptr(), a.in_proj_bias.data_ptr(),
                 a.out_proj.weight.data_ptr(), a.out_proj.bias.data_ptr(),
                 layer.linear1.weight.data_ptr(), layer.linear1.bias.data_ptr(),
                 layer.linear2.weight.data_ptr(), layer.linear2.bias.data_ptr(),
                 layer.norm1.weight.data_ptr(), layer.norm1.bias.data_ptr(),
                 layer.norm2.weight.data_ptr(), layer.norm2.bias.data_ptr(), work.data_ptr(), st)
            x = y
        if dev_step is None:
            state.offset += T
        return x

    def _heads(self, x, B, T, K, probas=None, cdf=None, sym=None, lohi=None, err=None):
        dev = x.device
        work = torch.empty((int(lib.encx_lm_heads_workspace(B * T, K, self.card)) + 3) // 4, device=dev)
        s = sym.stride() if sym is not None else (0, 0, 0)
        call('encx_lm_heads', x.data_ptr(), B, T, self.dim, self._lin_w.data_ptr(), self._lin_b.data_ptr(),
             K, self.card, work.data_ptr(), probas.data_ptr() if probas is not None else None,
             cdf.data_ptr() if cdf is not None else None, TOTAL_RANGE_BITS, ROUNDOFF, MIN_RANGE,
             sym.data_ptr() if sym is not None else None, s[0], s[1], s[2],
             lohi.data_ptr() if lohi is not None else None, err.data_ptr() if err is not None else None,
             stream())

    # ------------------------------------------------------------------ training
    def _train_params(self):
        """Parameters in the order _NLLFn takes and returns them."""
        tr = self.transformer
        ps = [tr.norm_in.weight, tr.norm_in.bias]
        for layer in tr.layers:
            a = layer.self_attn
            ps += [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                   layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias,
                   layer.norm1.weight, layer.norm1.bias, layer.norm2.weight, layer.norm2.bias]
        ps += [e.weight for e in self.emb] + [l.weight for l in self.linears] + [l.bias for l in self.linears]
        return ps

    def nll(self, codes: torch.Tensor, chunk_floats: int = 1 << 25) -> torch.Tensor:
        """Mean negative log-likelihood (nats per code) of codes int64 [B, K, T] under the
        teacher-forced LM: exactly the probabilities `encode_streams` codes them with.
        Differentiable with respect to every parameter; heads and embeddings k >= K get zero
        gradients. The heads run in row chunks of at most `chunk_floats` logits.

        Limits: the backward reads the live parameters, so it must run before anything changes
        them (an in-place change is refused; a write through raw pointers, as FlatAdam's step
        makes, cannot be seen and gives wrong layer gradients); and the loss can be
        differentiated once (no retain_graph: the saved activations are released)."""
        self.invalidate_packed()
        self._packed()
        self.invalidate_packed()  # an optimiser step follows: never trust this stack again
        self._check_device()
        if codes.dtype != torch.int64 or codes.dim() != 3 or not codes.is_cuda:
            raise RuntimeError('encx LM: codes must be int64 [B, K, T] on the GPU')
        if codes.device != self._emb.device:
            raise RuntimeError(f'encx LM: codes on {codes.device}, parameters on {self._emb.device}')
        B, K, T = codes.shape
        self._check_codebooks(K)
        if B < 1 or T < 1:
            raise ValueError('encx LM: nll needs at least one code')
        # the input stage reads the embedding table at the code: check before any launch
        lo, hi = codes.aminmax()
        if int(lo) < 0 or int(hi) >= self.card:
            raise ValueError(f'a code is outside [0, {self.card})')
        return _NLLFn.apply(self, codes, int(chunk_floats), *self._train_params())

    @torch.no_grad()
    def forward(self, indices: torch.Tensor, states: tp.Optional[LMState] = None, offset: int = 0):
        """model.py:47-65: indices [B, n_q, T] (1 + code, 0 = missing) -> (probabilities
        [B, card, n_q, T], states, offset + T)."""
        self._packed()
        self._check_device()
        if indices.dtype != torch.int64 or indices.dim() != 3 or not indices.is_cuda:
            raise RuntimeError('encx LM: indices must be int64 [B, K, T] on the GPU')
        B, K, T = indices.shape
        self._check_codebooks(K)
        if states is None:
            states = self.new_state(B, T + 1)
            states.offset = int(offset)
            if states.offset:
                raise ValueError('encx LM: a fresh state starts at offset 0')
        elif states.offset != int(offset):
            raise ValueError(f'encx LM: offset {offset} does not continue the state (at {states.offset})')
        x = self._body(indices, indices.stride(), B, K, T, False, states)
        probas = torch.empty(B, T, K, self.card, device=x.device)
        self._heads(x, B, T, K, probas=probas)
        return probas.permute(0, 3, 2, 1), states, states.offset

    # ------------------------------------------------------------------ entropy coder
    @torch.no_grad()
    def encode_streams(self, codes: torch.Tensor) -> tp.List[bytes]:
        """compress.py:67-89 (use_lm=True) for B frames [B, K, T] of codes: the arithmetic
        coded payload of each frame. One LM pass over all T steps, the coding intervals from the
        fused softmax + cdf kernel, then one coder thread per stream."""
        self._packed()
        self._check_device()
        if codes.dtype != torch.int64 or codes.dim() != 3 or not codes.is_cuda:
            raise RuntimeError('encx LM: codes must be int64 [B, K, T] on the GPU')
        B, K, T = codes.shape
        self._check_codebooks(K)
        dev = codes.device
        state = self.new_state(B, T + 1)
        x = self._body(codes, codes.stride(), B, K, T, True, state)
        lohi = torch.empty(B, T, K, 2, device=dev, dtype=torch.int32)
        err = torch.zeros(1, device=dev, dtype=torch.int32)
        self._heads(x, B, T, K, sym=codes, lohi=lohi, err=err,
                    cdf=torch.empty(B, T, K, self.card, device=dev, dtype=torch.int32))
        cap = int(lib.encx_ac_encode_capacity(T * K, TOTAL_RANGE_BITS))
        out = torch.empty(B, cap, device=dev, dtype=torch.uint8)
        nbytes = torch.empty(B, device=dev, dtype=torch.int64)
        serr = torch.empty(B, device=dev, dtype=torch.int32)
        call('encx_ac_encode', lohi.data_ptr(), B, T * K, TOTAL_RANGE_BITS, out.data_ptr(), cap,
             nbytes.data_ptr(), serr.data_ptr(), stream())
        host, nb, e, e0 = out.cpu(), nbytes.cpu().tolist(), serr.cpu().tolist(), int(err.item())
        if e0 & 2:
            raise ValueError(f'a code is outside [0, {self.card})')
        if e0 & 1 or any(v == 1 for v in e):
            raise AssertionError('quantized cdf total above 2^total_range_bits (ac.py:50, 116)')
        if any(e):
            raise RuntimeError(f'encx arithmetic coder failed: {e}')
        return [host[b, :nb[b]].numpy().tobytes() for b in range(B)]

    @torch.no_grad()
    def decode_streams(self, datas: tp.Sequence[bytes], K: int, T: int, graph: bool = True,
                       dev_span=None):
        """compress.py:128-155 (use_lm=True) for B streams of K codebooks x T steps: ->
        (codes int64 [B, K, T] on the GPU, bytes consumed per stream). Raises EOFError where
        the reference's decoder runs dry, RuntimeError where its binary search fails.

        One step = LM input, 5 layers, heads + cdf, arithmetic decode of the K codes (whose
        + 1 is the next step's input, compress.py:154-155). With graph=True the step's ~40
        launches are captured once into a HIP graph (offsets from a device-side step counter)
        and replayed T times, with one host sync at the end.
        dev_span = (uint8 device tensor, byte offset, byte count): decode ONE stream of that many
        bytes at that offset of a buffer already on the device (datas is then ignored), so a
        file's segments are decoded from one upload of the file."""
        self._packed()
        self._check_device()
        self._check_codebooks(K)
        dev = self._emb.device
        if dev_span is not None:
            src, off, count = dev_span
            if off < 0 or count < 0 or off + count > src.numel():
                raise ValueError('encx decode_streams: dev_span outside its buffer')
            B, stride = 1, max(count, 1)
            data_ptr = src.data_ptr() + off
            nbytes = torch.tensor([count], dtype=torch.int64).to(dev)
        else:
            B = len(datas)
            stride = max([len(d) for d in datas] + [1])
            buf = torch.zeros(B, stride, dtype=torch.uint8)
            for b, d in enumerate(datas):
                if len(d):
                    buf[b, :len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8)
            data = buf.to(dev)
            data_ptr = data.data_ptr()
            nbytes = torch.tensor([len(d) for d in datas], dtype=torch.int64).to(dev)
        dstate = new_decoder_state(B, dev)
        err = torch.zeros(B, dtype=torch.int32, device=dev)
        codes = torch.zeros(B, K, T, dtype=torch.int64, device=dev)
        idx = torch.zeros(B, K, dtype=torch.int64, device=dev)      # step input, 0 at t = 0
        cdf = torch.empty(B, 1, K, self.card, device=dev, dtype=torch.int32)
        state = self.new_state(B, T + 1)
        step = torch.zeros(1, dtype=torch.int64, device=dev)

        def one_step(t, dstep):
            st = stream()
            x = self._body(idx, (K, 1, 1), B, K, 1, False, state, dev_step=dstep)
            self._heads(x, B, 1, K, cdf=cdf)
            call('encx_ac_decode', data_ptr, stride, nbytes.data_ptr(), B, dstate.data_ptr(),
                 cdf.data_ptr(), K, self.card, TOTAL_RANGE_BITS, codes.data_ptr(), K * T, T, 1, t,
                 dstep.data_ptr() if dstep is not None else None, idx.data_ptr(), err.data_ptr(), st)
            if dstep is not None:
                call('encx_lm_step_advance', dstep.data_ptr(), 1, st)

        if graph and T > 2:
            one_step(0, step)                    # eager first step (loads every kernel)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                one_step(0, step)
            for _ in range(T - 1):
                g.replay()
        else:
            for t in range(T):
                one_step(t, None)
        e = err.cpu().tolist()
        if any(v == 1 for v in e):
            raise EOFError("The stream ended sooner than expected.")
        if any(v == 2 for v in e):
            raise RuntimeError("Binary search failed")
        if any(e):
            raise RuntimeError(f'encx arithmetic decoder failed: {e}')
        return codes, [(p + 7) // 8 for p in dstate[:, ENCX_AC_POS].cpu().tolist()]


# ---------------------------------------------------------------------------- live streams
MAX_SLOTS = 64          # encx.h: the slot table's B
MAX_PACKET_FRAMES = 255  # the packet's header byte


class _LMSlots:
    """What LMStreamEncoder and LMStreamDecoder share: the per-slot LM state on the device
    (pos [B], prev [B][K], one key/value ring [B][R][2 dim] per layer, R = past_context +
    max_frames), the slot table the kernels read (encx.h) and the host's view of each slot.
    Nothing touches the device before the first valid step, so every refusal of a step's
    arguments is a pure host check. A session is a snapshot of the LM's stacked heads and
    embeddings: build a new one after changing the LM's weights."""

    def __init__(self, lm: 'LMModel', batch: int, K: int, max_frames: int, graphs: bool, lm_format: int = 1):
        if lm_format not in (1, 2):
            raise ValueError(f'encx LM streaming: lm_format {lm_format!r} (1: a fixed K, 2: n_q per slot and step)')
        self.lm_format = int(lm_format)
        if not 1 <= batch <= MAX_SLOTS:
            raise ValueError(f'encx LM streaming: batch {batch} (1..{MAX_SLOTS})')
        if not 1 <= K <= min(lm.n_q, 64):
            raise ValueError(f'encx LM streaming: {K} codebooks for an LM of n_q={lm.n_q} (at most 64)')
        if not 1 <= max_frames <= MAX_PACKET_FRAMES:
            raise ValueError(f'encx LM streaming: max_frames {max_frames} (1..{MAX_PACKET_FRAMES})')
        _check_window(lm.transformer, int(lm.transformer.past_context) + 1)
        self.lm, self.B, self.K = lm, int(batch), int(K)
        self.max_frames, self.graphs = int(max_frames), bool(graphs)
        self.R = int(lm.transformer.past_context) + self.max_frames
        self.started = [False] * self.B
        self.failed: tp.Set[int] = set()
        self._ready = False
        self._graphs: tp.Dict[int, tp.Any] = {}

    def reset(self):
        """Every slot starts a new stream with its next packet."""
        self.started = [False] * self.B
        self.failed.clear()

    def restart(self, slots):
        """The named slots start a new stream with their next packet: the LM's position and
        context are taken as empty by the kernels on that packet (the slot table's first-chunk
        flag), so this launches nothing and disturbs no other slot."""
        for b in check_restart(slots, self.B):
            self.started[b] = False
            self.failed.discard(b)

    def _check_frames(self, frames):
        frames = _ints(frames, 'frames')
        n_max, _ = check_frames(self.started, frames, 1, self.max_frames)
        for b, f in enumerate(frames):
            if f and b in self.failed:
                raise ValueError(f'encx LM streaming: slot {b} failed on a bad packet; restart([{b}]) it first')
        return frames, n_max

    def _check_n_q(self, frames, n_q):
        """n_q goes with lm_format=2 and only with it -> the nq table (slots.check_n_q), or None."""
        if (self.lm_format == 2) != (n_q is not None):
            raise ValueError('encx LM streaming: n_q goes with lm_format=2, and only with it')
        return check_n_q(frames, n_q, self.K) if n_q is not None else None

    def _ensure(self):
        if self._ready:
            return
        lm = self.lm
        self._packed = lm._packed()  # kept: the captured graphs point at these stacks
        lm._check_device()
        dev = self.dev = lm._emb.device
        tr = lm.transformer
        B, K = self.B, self.K
        self._kv = [torch.zeros(B, self.R, 2 * lm.dim, device=dev) for _ in tr.layers]
        self._pos = torch.zeros(B, dtype=torch.int64, device=dev)
        self._prev = torch.zeros(B, K, dtype=torch.int64, device=dev)
        self._slots = DeviceTable(B, 2, dev)
        self._nq = DeviceTable(B, 1, dev)  # lm_format 2
        self._cols = torch.arange(self.max_frames, device=dev, dtype=torch.int32)
        self._ready = True

    def _put(self, frames, n_q):
        """This step's tables; a sustained step repeats them: no upload."""
        self._slots.put([(int(f), int(f > 0 and not on)) for f, on in zip(frames, self.started)])
        if n_q is not None:
            self._nq.put(n_q)

    def _rows(self, T, n_max, codes, dstep):
        """The LM input and every layer for T rows per slot under the slot table -> x [B*T][dim]."""
        lm, tr = self.lm, self.lm.transformer
        B, K, D, Fh = self.B, self.K, lm.dim, tr.hidden
        st = stream()
        cs = codes.stride() if codes is not None else (0, 0, 0)
        dptr = dstep.data_ptr() if dstep is not None else None
        x = torch.empty(B * T, D, device=self.dev)
        nq = (self._nq.data_ptr(),) if self.lm_format == 2 else ()
        call('encx_lm_input_slots_nq' if nq else 'encx_lm_input_slots',
             codes.data_ptr() if codes is not None else None, cs[0], cs[1], cs[2], B, K, T,
             n_max, self._slots.data_ptr(), *nq, self._pos.data_ptr(), self._prev.data_ptr(), dptr,
             lm._emb.data_ptr(), lm.card + 1, D, tr.norm_in.weight.data_ptr(), tr.norm_in.bias.data_ptr(),
             float(tr.max_period), x.data_ptr(), st)
        work = torch.empty((int(lib.encx_lm_layer_workspace(B * T, D, Fh)) + 3) // 4, device=self.dev)
        for i, layer in enumerate(tr.layers):
            y = torch.empty_like(x)
            call('encx_lm_layer_slots', x.data_ptr(), y.data_ptr(), B, T, n_max, self._kv[i].data_ptr(), self.R,
                 self._slots.data_ptr(), self._pos.data_ptr(), dptr, tr.past_context, D, tr.num_heads, Fh,
                 *_layer_ptrs(layer), work.data_ptr(), st)
            x = y
        return x

    def _advance(self, n_max, codes):
        cs = codes.stride() if codes is not None else (0, 0, 0)
        nq = (self._nq.data_ptr(),) if self.lm_format == 2 else ()
        call('encx_lm_slots_advance_nq' if nq else 'encx_lm_slots_advance', self._slots.data_ptr(), *nq, self.B,
             self.K, n_max, self._pos.data_ptr(), self._prev.data_ptr(),
             codes.data_ptr() if codes is not None else None, cs[0], cs[1], cs[2], self.lm.card + 1, stream())

    def _heads_nq(self, x, T, n_max, dstep, probas=None, cdf=None, sym=None, lohi=None, err=None):
        """lm._heads for the live rows and the codebooks k < nq[b] of a slots step (lm_format 2)."""
        lm = self.lm
        work = torch.empty((int(lib.encx_lm_heads_workspace(self.B * T, self.K, lm.card)) + 3) // 4, device=self.dev)
        s = sym.stride() if sym is not None else (0, 0, 0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        call('encx_lm_heads_slots', x.data_ptr(), self.B, T, n_max, lm.dim, lm._lin_w.data_ptr(),
             lm._lin_b.data_ptr(), self.K, lm.card, self._slots.data_ptr(), self._nq.data_ptr(), ptr(dstep),
             work.data_ptr(), ptr(probas), ptr(cdf), TOTAL_RANGE_BITS, ROUNDOFF, MIN_RANGE, ptr(sym), s[0], s[1], s[2],
             ptr(lohi), ptr(err), stream())

    def _run(self, key, body, frames, n_q=None):
        """Fill this step's slot table; -> the graph of body(key) to replay, or None (run the body
        eagerly). The first step of a key runs the body once eagerly under an EMPTY table (every
        row dead: each kernel is loaded, no state moves), then captures it; the table is device
        memory, so the graph replays for any counts."""
        g = None
        if self.graphs:
            g = self._graphs.get(key)
            if g is None:
                self._slots.clear()
                body(key)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):  # one stream: no parallel branches
                    body(key)
                self._graphs[key] = g
        self._put(frames, n_q)
        return g


class LMStreamEncoder(_LMSlots):
    """Arithmetic-codes the chunks of `batch` live streams (the slots of a StreamEncoder) under
    `lm`, one self-contained packet per delivering slot and step, the LM's context carried from
    packet to packet for a stream of any length (the packet format: include/encx.h).

        enc = LMStreamEncoder(lm, batch=64, K=8)
        payloads = enc.encode_slots(codes, frames)   # codes [B, K, max(frames)] int64 on the GPU

    payloads[b] is the coded chunk of slot b (b'' for a slot with 0 frames); packets(...) returns
    the same with the header byte in front. Slot b's columns past frames[b] are not read. A slot's
    bytes are those of the same stream alone in a session of one. probas=True keeps the
    probabilities of the last step's rows in last_probas [B, n_max, K, card].

    lm_format=2: K is the session's largest count and every step names the count of each slot,

        payloads = enc.encode_slots(codes, frames, n_q)   # rows k >= n_q[b] of codes are not read

    packets(...) then carries the two header bytes (n, n_q[b]) of packet format 2. The rows of
    last_probas / last_cdf that a step skipped (dead frames, k >= n_q[b]) hold whatever they held."""

    def __init__(self, lm, batch: int, K: int, max_frames: int = 8, graphs: bool = True, probas: bool = False,
                 lm_format: int = 1):
        super().__init__(lm, batch, K, max_frames, graphs, lm_format)
        self._want_probas = bool(probas)
        self._bufs: tp.Dict[int, tp.Any] = {}
        self.last_probas = self.last_cdf = None

    def _buf(self, n):
        b = self._bufs.get(n)
        if b is None:
            dev, B, K, card = self.dev, self.B, self.K, self.lm.card
            stride = self.lm_format + int(lib.encx_ac_encode_capacity(n * K, TOTAL_RANGE_BITS))
            b = self._bufs[n] = dict(
                codes=torch.zeros(B, K, n, dtype=torch.int64, device=dev),
                lohi=torch.zeros(B, n, K, 2, dtype=torch.int32, device=dev),
                cdf=torch.empty(B, n, K, card, dtype=torch.int32, device=dev),
                probas=torch.empty(B, n, K, card, device=dev) if self._want_probas else None,
                out=torch.zeros(B, stride, dtype=torch.uint8, device=dev),
                nbytes=torch.zeros(B, dtype=torch.int64, device=dev),
                serr=torch.zeros(B, dtype=torch.int32, device=dev),
                err=torch.zeros(1, dtype=torch.int32, device=dev))
        return b

    def _body(self, n):
        b = self._buf(n)
        x = self._rows(n, n, b['codes'], None)
        b['err'].zero_()
        if self.lm_format == 2:
            self._heads_nq(x, n, n, None, probas=b['probas'], cdf=b['cdf'], sym=b['codes'], lohi=b['lohi'],
                           err=b['err'])
            call('encx_ac_encode_slots_nq', b['lohi'].data_ptr(), self.B, n, self.K, self._slots.data_ptr(),
                 self._nq.data_ptr(), TOTAL_RANGE_BITS, b['out'].data_ptr(), b['out'].shape[1],
                 b['nbytes'].data_ptr(), b['serr'].data_ptr(), stream())
        else:
            self.lm._heads(x, self.B, n, self.K, probas=b['probas'], cdf=b['cdf'], sym=b['codes'], lohi=b['lohi'],
                           err=b['err'])
            call('encx_ac_encode_slots', b['lohi'].data_ptr(), self.B, n, self.K, self._slots.data_ptr(),
                 TOTAL_RANGE_BITS, b['out'].data_ptr(), b['out'].shape[1], b['nbytes'].data_ptr(),
                 b['serr'].data_ptr(), stream())
        self._advance(n, b['codes'])

    @torch.no_grad()
    def packets(self, codes: torch.Tensor, frames: tp.Sequence[int],
                n_q: tp.Optional[tp.Sequence[int]] = None) -> tp.List[bytes]:
        """One packet (header + coded payload) per slot, b'' for a slot with 0 frames. The header is
        the byte n, and with lm_format=2 the bytes (n, n_q[b])."""
        frames, n_max = self._check_frames(frames)
        n_q = self._check_n_q(frames, n_q)
        if codes.dim() != 3 or tuple(codes.shape) != (self.B, self.K, n_max) or codes.dtype != torch.int64:
            raise ValueError(f'encx LM streaming: expected int64 codes [{self.B}, {self.K}, max(frames) = {n_max}], '
                             f'got {codes.dtype} {tuple(codes.shape)}')
        if not codes.is_cuda:
            raise RuntimeError('encx LM streaming takes device tensors (no CPU fallback)')
        self._ensure()
        b = self._buf(n_max)
        g = self._run(n_max, self._body, frames, n_q)
        # the graph's own input; past a slot's count whatever the caller left becomes code 0
        keep = (self._cols[:n_max] < self._slots.t[:, :1]).unsqueeze(1)
        b['codes'].copy_(torch.where(keep, codes, 0))
        if g is not None:
            g.replay()
        else:
            self._body(n_max)
        self.last_probas, self.last_cdf = b['probas'], b['cdf']
        host, nb = b['out'].cpu(), b['nbytes'].cpu().tolist()
        e, e0 = b['serr'].cpu().tolist(), int(b['err'].item())
        for s, f in enumerate(frames):
            if f:
                self.started[s] = True
        if e0 & 2:
            raise ValueError(f'a code is outside [0, {self.lm.card})')
        if e0 & 1 or any(v == 1 for v in e):
            raise AssertionError('quantized cdf total above 2^total_range_bits (ac.py:50, 116)')
        if any(e):
            raise RuntimeError(f'encx arithmetic coder failed: {e}')
        return [host[s, :nb[s]].numpy().tobytes() for s in range(self.B)]

    def encode_slots(self, codes: torch.Tensor, frames: tp.Sequence[int],
                     n_q: tp.Optional[tp.Sequence[int]] = None) -> tp.List[bytes]:
        """The coded payloads (the packets without their header: one byte, two with lm_format=2)."""
        return [p[self.lm_format:] for p in self.packets(codes, frames, n_q)]


class LMStreamDecoder(_LMSlots):
    """The inverse of LMStreamEncoder: decode_slots(payloads, frames) -> (codes [B, K, max(frames)]
    int64 on the GPU, zero past each slot's count, and the list of slots that failed in this
    step). One step of the chunk = LM input, layers, heads + cdf, arithmetic decode of the K
    codes, for one row per slot; it is captured once and replayed max(frames) times with the step
    in a device counter. A packet the coder cannot decode (it runs dry, or no interval holds the
    value) is data, not an error: that slot comes back with zero codes, is listed in `failed`, and
    refuses further packets until restart([b]); the other slots are not disturbed.

    lm_format=2: decode_slots(payloads, frames, n_q), the payloads without their two header bytes;
    rows k >= n_q[b] of the codes are zero. A payload may be empty, and bits past its end read as
    zero, so the coder never runs dry: a truncated packet either fails (no interval holds the value)
    or decodes to other codes, and integrity is the transport's job (include/encx.h)."""

    def __init__(self, lm, batch: int, K: int, max_frames: int = 8, graphs: bool = True, lm_format: int = 1):
        super().__init__(lm, batch, K, max_frames, graphs, lm_format)
        self.cap = int(lib.encx_ac_encode_capacity(self.max_frames * self.K, TOTAL_RANGE_BITS))

    def lose(self, slots):
        """A packet of each named slot did not arrive: its context no longer matches the
        sender's, so the slot is failed, exactly as after a bad packet, until restart([b])."""
        self.failed.update(check_restart(slots, self.B))

    def _ensure(self):
        if self._ready:
            return
        super()._ensure()
        dev, B, K, M = self.dev, self.B, self.K, self.max_frames
        self._data = torch.zeros(B, self.cap, dtype=torch.uint8, device=dev)
        self._nbytes = torch.zeros(B, dtype=torch.int64, device=dev)
        self._dstate = new_decoder_state(B, dev)
        self._err = torch.zeros(B, dtype=torch.int32, device=dev)
        self._codes = torch.zeros(B, K, M, dtype=torch.int64, device=dev)
        self._cdf = torch.empty(B, 1, K, self.lm.card, dtype=torch.int32, device=dev)
        self._step = torch.zeros(1, dtype=torch.int64, device=dev)

    def _body(self, _key):
        B, K, M = self.B, self.K, self.max_frames
        x = self._rows(1, M, None, self._step)
        st = stream()
        if self.lm_format == 2:
            self._heads_nq(x, 1, M, self._step, cdf=self._cdf)
            call('encx_ac_decode_slots_nq', self._data.data_ptr(), self.cap, self._nbytes.data_ptr(), B,
                 self._dstate.data_ptr(), self._cdf.data_ptr(), K, self.lm.card, TOTAL_RANGE_BITS,
                 self._codes.data_ptr(), K * M, M, 1, M, self._step.data_ptr(), self._slots.data_ptr(),
                 self._nq.data_ptr(), self._prev.data_ptr(), self._err.data_ptr(), st)
        else:
            self.lm._heads(x, B, 1, K, cdf=self._cdf)
            call('encx_ac_decode_slots', self._data.data_ptr(), self.cap, self._nbytes.data_ptr(), B,
                 self._dstate.data_ptr(), self._cdf.data_ptr(), K, self.lm.card, TOTAL_RANGE_BITS,
                 self._codes.data_ptr(), K * M, M, 1, M, self._step.data_ptr(), self._slots.data_ptr(),
                 self._prev.data_ptr(), self._err.data_ptr(), st)
        call('encx_lm_step_advance', self._step.data_ptr(), 1, st)

    @torch.no_grad()
    def decode_slots(self, payloads: tp.Sequence[bytes], frames: tp.Sequence[int],
                     n_q: tp.Optional[tp.Sequence[int]] = None):
        frames, n_max = self._check_frames(frames)
        n_q = self._check_n_q(frames, n_q)
        if len(payloads) != self.B:
            raise ValueError(f'encx LM streaming: payloads for {len(payloads)} slots, the session has {self.B}')
        for b, (p, f) in enumerate(zip(payloads, frames)):
            if not isinstance(p, (bytes, bytearray)):
                raise ValueError(f'encx LM streaming: the payload of slot {b} is not bytes')
            if len(p) and not f:
                raise ValueError(f'encx LM streaming: slot {b} has a payload but 0 frames')
            if len(p) > self.cap:
                raise ValueError(f'encx LM streaming: a payload of {len(p)} bytes in slot {b}; no packet of up to '
                                 f'{self.max_frames} frames has more than {self.cap}')
        self._ensure()
        host = torch.zeros(self.B, self.cap, dtype=torch.uint8)
        for b, p in enumerate(payloads):
            if len(p):
                host[b, :len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8)
        g = self._run(0, self._body, frames, n_q)
        self._data.copy_(host)
        self._nbytes.copy_(torch.tensor([len(p) for p in payloads], dtype=torch.int64))
        self._codes.zero_()
        self._err.zero_()
        self._step.zero_()
        for _ in range(n_max):
            if g is not None:
                g.replay()
            else:
                self._body(0)
        self._advance(self.max_frames, None)
        codes = self._codes[:, :, :n_max].clone()
        failed = [b for b, v in enumerate(self._err.cpu().tolist()) if v]
        for b, f in enumerate(frames):
            if b in failed:
                codes[b] = 0
                self.failed.add(b)
            elif f:
                self.started[b] = True
        return codes, failed
