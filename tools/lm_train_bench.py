"""LM training throughput on one MI355X: encx.lm.LMModel.nll + backward + FlatAdam (the
hand-written HIP path, csrc/lm_train.hip) against the same model written with torch.nn through
PyTorch-ROCm autograd, fp32, in the same process.

The 24 kHz LM at its real size (card 1024, dim 200, 8 heads, 5 layers, past_context 262,
model.py:221-226) with random-init weights, K = 8 and K = 32 codebooks, B 32 x T 150 random
codes. One step = loss, full backward, Adam. The torch baseline: F.embedding sums,
F.layer_norm, a masked F.scaled_dot_product_attention over [phantom zero input, x] (boolean
window mask), F.gelu, the K heads as one stacked F.linear, F.cross_entropy over its rows,
torch.optim.Adam; same parameters, same loss.

Method: every variant is warmed up, then timed with device events over windows of at least
--min-seconds each; --rounds rounds alternate the variants; the median and the min..max spread
of the per-round step time are reported, with steps/s and codes/s from the median. The share of
the FP32 MFMA peak (157.3 TFLOP/s) is for the heads' three GEMMs (forward, dX, dW: 3 x 2 N K card
D flop) from a per-kernel profile, not from this run.

python tools/lm_train_bench.py [--K 8 32] [--batch 32] [--steps-T 150] [--rounds 5] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'encodec-pytorch_amd'))
sys.path.insert(0, ROOT)

DEV = 'cuda:0'
DIM, HEADS, LAYERS, CARD, PAST = 200, 8, 5, 1024, 262


class TorchLM(torch.nn.Module):
    """The same LM in torch.nn ops (the baseline); takes an encx LMModel's state dict."""

    def __init__(self, lm, K):
        super().__init__()
        self.K = K
        sd = lm.state_dict()
        self.p = torch.nn.ParameterDict({k.replace('.', '/'): torch.nn.Parameter(v.detach().clone())
                                         for k, v in sd.items()
                                         if not k.startswith('linears.') and
                                         not (k.startswith('emb.') and int(k.split('.')[1]) >= K)})
        # the K heads as ONE [K card][dim] projection: a single GEMM, no per-head launches, no
        # stack copy of the logits (the baseline's best form, not the reference's K nn.Linear)
        self.head_w = torch.nn.Parameter(torch.cat([sd[f'linears.{k}.weight'] for k in range(K)]).clone())
        self.head_b = torch.nn.Parameter(torch.cat([sd[f'linears.{k}.bias'] for k in range(K)]).clone())

    def g(self, k):
        return self.p[k.replace('.', '/')]

    def forward(self, codes):
        B, K, T = codes.shape
        D, H = DIM, HEADS
        inp = torch.zeros_like(codes)
        inp[:, :, 1:] = codes[:, :, :-1] + 1
        x = sum(F.embedding(inp[:, k], self.g(f'emb.{k}.weight')) for k in range(K))
        x = F.layer_norm(x, (D,), self.g('transformer.norm_in.weight'), self.g('transformer.norm_in.bias'))
        half = D // 2
        pos = torch.arange(T, device=x.device, dtype=torch.float32).view(1, -1, 1)
        ph = pos / (10000.0 ** (torch.arange(half, device=x.device, dtype=torch.float32) / (half - 1)))
        x = x + torch.cat([ph.cos(), ph.sin()], -1)
        s = torch.arange(1, T + 1, device=x.device).view(-1, 1)
        j = torch.arange(T + 1, device=x.device).view(1, -1)
        mask = (j <= s) & (j >= s - PAST)                           # True = attend
        for i in range(LAYERS):
            pre = f'transformer.layers.{i}.'
            W, b = self.g(pre + 'self_attn.in_proj_weight'), self.g(pre + 'self_attn.in_proj_bias')
            kin = torch.cat([torch.zeros_like(x[:, :1]), x], 1)
            q = F.linear(x, W[:D], b[:D]).view(B, T, H, D // H).transpose(1, 2)
            kv = F.linear(kin, W[D:], b[D:]).view(B, T + 1, 2, H, D // H)
            a = F.scaled_dot_product_attention(q, kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2),
                                               attn_mask=mask)
            a = a.transpose(1, 2).reshape(B, T, D)
            x = F.layer_norm(x + F.linear(a, self.g(pre + 'self_attn.out_proj.weight'),
                                          self.g(pre + 'self_attn.out_proj.bias')),
                             (D,), self.g(pre + 'norm1.weight'), self.g(pre + 'norm1.bias'))
            ff = F.linear(F.gelu(F.linear(x, self.g(pre + 'linear1.weight'), self.g(pre + 'linear1.bias'))),
                          self.g(pre + 'linear2.weight'), self.g(pre + 'linear2.bias'))
            x = F.layer_norm(x + ff, (D,), self.g(pre + 'norm2.weight'), self.g(pre + 'norm2.bias'))
        logits = F.linear(x, self.head_w, self.head_b)              # [B, T, K card], rows (b, t, k) of card
        return F.cross_entropy(logits.view(B * T * K, CARD), codes.transpose(1, 2).reshape(-1))


def window(step, min_seconds):
    """Device-event time per step of a window of at least min_seconds."""
    n = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            step()
        b.record()
        b.synchronize()
        dt = a.elapsed_time(b) / 1e3
        if dt >= min_seconds:
            return dt / n
        n = max(n + 1, int(math.ceil(n * min_seconds / max(dt, 1e-4) * 1.1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps-T', type=int, default=150)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=['encx', 'torch'], default=None, help='one side only (for a kernel profile)')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    from encx.lm import LMModel
    from encx.optim import FlatAdam
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'B': args.batch, 'T': args.steps_T,
           'dim': DIM, 'layers': LAYERS, 'card': CARD, 'rounds': args.rounds, 'min_seconds': args.min_seconds,
           'variants': []}
    for K in args.K:
        torch.manual_seed(0)
        lm = LMModel(K, CARD, dim=DIM, num_heads=HEADS, num_layers=LAYERS, past_context=PAST).to(DEV)
        ref = TorchLM(lm, K).to(DEV)
        codes = torch.randint(0, CARD, (args.batch, K, args.steps_T), device=DEV)
        with torch.no_grad():
            l_encx, l_torch = float(lm.nll(codes)), float(ref(codes))
        opt = FlatAdam(lm.parameters(), lr=1e-4)
        topt = torch.optim.Adam(ref.parameters(), lr=1e-4)

        def step_encx():
            opt.zero_grad()
            lm.nll(codes).backward()
            opt.step()

        def step_torch():
            topt.zero_grad(set_to_none=True)
            ref(codes).backward()
            topt.step()
        sides = [(n, f) for n, f in (('encx', step_encx), ('torch', step_torch)) if args.only in (None, n)]
        for _, f in sides:
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        times = {n: [] for n, _ in sides}
        for _ in range(args.rounds):
            for n, f in sides:
                times[n].append(window(f, args.min_seconds))
        n_codes = args.batch * K * args.steps_T
        heads_flop = 3 * 2 * args.batch * args.steps_T * K * CARD * DIM
        row = {'K': K, 'loss_encx_at_init': l_encx, 'loss_torch_at_init': l_torch, 'heads_gflop_per_step': heads_flop / 1e9}
        for n, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            row[n] = {'step_ms_median': med * 1e3, 'step_ms_min': ts[0] * 1e3, 'step_ms_max': ts[-1] * 1e3,
                      'steps_per_s': 1 / med, 'codes_per_s': n_codes / med}
        if 'encx' in row and 'torch' in row:
            row['encx_over_torch_speed'] = row['torch']['step_ms_median'] / row['encx']['step_ms_median']
        res['variants'].append(row)
        print(json.dumps(row), flush=True)
        del lm, ref, opt, topt
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
