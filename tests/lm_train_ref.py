"""Differentiable restatement of the LM's teacher-forced training loss -- TEST INFRASTRUCTURE.

`nll(st, codes, cfg)` is the body of oracle.lm_oracle.lm_all without no_grad, through the
oracle's own `_input` / `_layer` / `_heads` pieces (so it is pinned to the reference by the same
fixtures as lm_all), then F.cross_entropy over the codebook axis: the mean over (b, k, t) of
-log p[code], in the dtype of the state dict. tests/test_lm_train_ref.py checks it against lm_all
and with gradcheck; tests/test_gpu_lm_train.py checks encx.lm.LMModel.nll against it.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import lm_oracle as O


@contextlib.contextmanager
def _default_dtype(dtype):
    """The oracle's sin_embedding builds its phases from integer tensors, so they come out in
    torch's DEFAULT dtype whatever the state dict's: an "fp64" run would carry fp32 position
    embeddings (up to 3.3e-6 of the input's largest entry at position 300, all of it shared with
    the fp32 run and so invisible in |g32 - g64|). With the default dtype set to the state's, the
    fp64 restatement is fp64 throughout and the fp32 one is unchanged bit for bit."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(prev)


def logits(st, codes, cfg):
    """lm_all's body up to the heads' logits [B, card, K, T] (softmax of these = lm_all)."""
    B, K, T = codes.shape
    inp = torch.zeros_like(codes)
    inp[:, :, 1:] = codes[:, :, :-1] + 1
    with _default_dtype(st['transformer.norm_in.weight'].dtype):
        x = O._input(st, inp, 0, cfg)
    P = cfg.past_context
    s = torch.arange(1, T + 1).view(-1, 1)
    j = torch.arange(T + 1).view(1, -1)
    valid = (j <= s) & (j >= s - P)
    for i in range(cfg.num_layers):
        keys_in = torch.cat([torch.zeros_like(x[:, :1]), x], dim=1)
        x = O._layer(st, i, x, keys_in, ~valid, cfg)
    return torch.stack([F.linear(x, st[f'linears.{k}.weight'], st[f'linears.{k}.bias'])
                        for k in range(K)], dim=1).permute(0, 3, 1, 2)


def nll(st, codes, cfg):
    """Mean nats per code, differentiable with respect to every tensor of st."""
    return F.cross_entropy(logits(st, codes, cfg), codes)


def state(st, dtype, requires_grad=True):
    """A detached copy of a state dict in `dtype`, leaves that require grad."""
    return {k: v.detach().to(dtype).clone().requires_grad_(requires_grad) for k, v in st.items()}


def loss_and_grads(st, codes, cfg, dtype):
    """-> (loss as a Python float, {name: grad}) of nll in `dtype` on the host; parameters the
    loss does not reach (heads / embeddings k >= K) get zeros."""
    p = state(st, dtype)
    loss = nll(p, codes, cfg)
    names = list(p)
    gs = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    return float(loss.detach()), {k: (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(names, gs)}


def synth(cfg, seed):
    """Synthetic LM weights for cfg (tests/golden/synth.py, as the g12 fixture's)."""
    import numpy as np
    from synth import synth_lm_state
    return {k: torch.from_numpy(np.ascontiguousarray(v))
            for k, v in synth_lm_state(O.lm_param_shapes(cfg), seed).items()}


def adam_steps(st, batches, cfg, dtype, lr, steps=None, eps=1e-8):
    """torch.optim.Adam on nll over `batches` (a list of code tensors, cycled) -> (losses before
    each step, the final state dict)."""
    p = state(st, dtype)
    opt = torch.optim.Adam(list(p.values()), lr=lr, eps=eps)
    losses = []
    for i in range(steps if steps is not None else len(batches)):
        opt.zero_grad()
        loss = nll(p, batches[i % len(batches)], cfg)
        loss.backward()
        for v in p.values():
            if v.grad is None:
                v.grad = torch.zeros_like(v)
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in p.items()}
