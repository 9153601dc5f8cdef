"""Training the entropy-coding LM on the GPU: encx.lm.LMModel.nll (csrc/lm_train.hip) against the
fp64 restatement tests/lm_train_ref.py.

The rule is the project's 4x rule (tests/steputil.py check_grads): per tensor, max |g - g64| /
max |g64| within 4x what the same restatement achieves in plain fp32 on the host (or 4x the
fp32 restatement's median over the tensors where that is larger), and the median ratio at most 4.
FLOOR, the smallest bound, is 16 u = 2^-20 (u = 2^-24, fp32's unit roundoff): on the smallest
cases (T 1, a handful of terms per sum) the fp32 restatement gets whole tensors exact to within
a rounding or two, |g32 - g64| ~ u, and 4 u bounds no fp32 computation that sums more than four
terms in another order; every gradient entry here is at least one dot product of >= 48 terms
(dim 50, card 48), whose rounding in any order is up to ~sqrt(48) u = 7 u, times the two or more
GEMMs between it and the loss. The loss is held to the same rule with the same floor relative
to max(1, loss).
"""
import functools
import math
import wave

import numpy as np
import pytest
import torch

import lm_train_ref as R
from oracle import lm_oracle as O
from steputil import check_grads

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FLOOR = 2.0 ** -20


def _cfg(dim, heads, layers, card, P, n_q=4):
    return O.LMConfig(n_q=n_q, card=card, dim=dim, num_heads=heads, num_layers=layers, past_context=P)


# name -> (cfg, B, K, T, nll keyword arguments). Smallest shapes at which each path can go wrong:
# hd 25 and 64 (the two attention instantiations), 1 and 2 layers, K 1 and 3 of n_q 4, card 48 (no
# multiple of 32 or 64) and 1024, B 1 and 3, T 1 / 7 / 70 (70: two 64-query and two 64-key blocks;
# N = 210 rows: 27 eight-row LayerNorm partials, the last one short, and three split-K slabs in
# the weight grads, which split from 128 rows up), past_context 3 (most rows lose the phantom key
# and older ones) and T + 5 (every row sees it), and the heads in four row chunks (chunk: the
# accumulate path of the heads' weight grad). chunk_tail: 650 rows in chunks of 330 + 320, where the
# shorter last chunk splits its weight grad into MORE slabs than the first (5 of 64 rows against
# 4 of 96: the k chunk rounds up to 32) out of the one work buffer sized for the first.
CASES = {
    'hd25_T1': (_cfg(50, 2, 1, 48, 3), 1, 1, 1, {}),
    'hd25_T7_2layers': (_cfg(50, 2, 2, 48, 3), 3, 3, 7, {}),
    'hd25_T7_sees0': (_cfg(50, 2, 1, 48, 12), 1, 3, 7, {}),
    'hd25_T70_P3': (_cfg(50, 2, 1, 48, 3), 3, 3, 70, {}),
    'hd25_T70_chunks': (_cfg(50, 2, 1, 48, 3), 3, 3, 70, dict(chunk_floats=64 * 3 * 48)),
    'hd25_chunk_tail': (_cfg(50, 2, 1, 48, 3), 5, 3, 130, dict(chunk_floats=330 * 3 * 48)),
    'hd25_T70_sees0_card1024': (_cfg(50, 2, 2, 1024, 75), 3, 3, 70, {}),
    'hd64_T7_sees0': (_cfg(128, 2, 1, 48, 12), 1, 3, 7, {}),
    'hd64_T70_P3_card1024': (_cfg(128, 2, 2, 1024, 3), 3, 1, 70, {}),
    'real_size': (_cfg(200, 8, 5, 1024, 262, n_q=8), 2, 8, 300, {}),
}


def _codes(cfg, B, K, T, seed):
    return torch.randint(0, cfg.card, (B, K, T), generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(state, codes, loss64, grads64, loss32, grads32), computed once per case."""
    cfg, B, K, T, _ = CASES[name]
    st = R.synth(cfg, 200 + len(name))
    codes = _codes(cfg, B, K, T, 7)
    nt = torch.get_num_threads()
    torch.set_num_threads(8)   # a fixed summation order for the fp32 restatement (steputil.ORACLE_THREADS)
    try:
        l64, g64 = R.loss_and_grads(st, codes, cfg, torch.float64)
        l32, g32 = R.loss_and_grads(st, codes, cfg, torch.float32)
    finally:
        torch.set_num_threads(nt)
    return st, codes, l64, g64, l32, g32


def _lm(cfg, st):
    from encx.lm import LMModel
    lm = LMModel(cfg.n_q, cfg.card, dim=cfg.dim, num_heads=cfg.num_heads, num_layers=cfg.num_layers,
                 past_context=cfg.past_context)
    lm.load_state_dict(st)
    return lm.to(DEV)


def _run(lm, codes, **kw):
    lm.zero_grad(set_to_none=True)
    loss = lm.nll(codes.to(DEV), **kw)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {k: p.grad.detach().cpu() for k, p in lm.named_parameters()}


def _check_loss(mine, l64, l32, what):
    err, e32 = abs(mine - l64), abs(l32 - l64)
    bound = max(4 * e32, FLOOR * max(1.0, abs(l64)))
    print(f'{what}: loss {mine:.9g} fp64 {l64:.9g} err {err:.3e} fp32 restatement {e32:.3e} bound {bound:.3e}')
    assert err <= bound, (what, mine, l64, err, bound)


@pytest.mark.parametrize('name', list(CASES))
def test_gpu_nll_loss_and_grads_match_fp64(name):
    cfg, B, K, T, kw = CASES[name]
    st, codes, l64, g64, l32, g32 = _reference(name)
    loss, g = _run(_lm(cfg, st), codes, **kw)
    _check_loss(loss, l64, l32, name)
    assert set(g) == set(g64)
    check_grads(g, g64, g32, f'nll grads {name}', floor=FLOOR)
    D = cfg.dim
    for i in range(cfg.num_layers):
        # the value half of in_proj_bias: the rows' column sums PLUS the phantom key's dv (position
        # 0, whose value is this bias); the key half is zero up to rounding (a shift of every key
        # by the same vector leaves the softmax as it is) and is held by the whole-tensor check
        k = f'transformer.layers.{i}.self_attn.in_proj_bias'
        check_grads({k: g[k][2 * D:]}, {k: g64[k][2 * D:]}, {k: g32[k][2 * D:]}, f'{name} in_proj_bias[2D:3D]',
                    floor=FLOOR)
        check_grads({k: g[k][D:]}, {k: g64[k][D:]}, {k: g32[k][D:]}, f'{name} in_proj_bias[D:3D]', floor=FLOOR)
    for k in range(cfg.n_q):
        if k < K:
            assert float(g[f'emb.{k}.weight'][0].abs().max()) > 0, f'emb.{k} row 0 (the t = 0 token)'
        else:
            for n in (f'emb.{k}.weight', f'linears.{k}.weight', f'linears.{k}.bias'):
                assert float(g[n].abs().max()) == 0, n


def test_gpu_phantom_key_changes_the_bias_grad():
    """With every row seeing position 0 the value-bias grad is not the plain column sum of dv over
    the real positions: the same codes under past_context 0 (nobody sees the phantom, every row
    attends itself alone) give another one, and both match fp64 (the cases above); here only that
    the window is honoured at all: P 0 against P T + 5 differ."""
    cfg, B, K, T, _ = CASES['hd25_T7_sees0']
    st, codes, *_ = _reference('hd25_T7_sees0')
    _, g = _run(_lm(cfg, st), codes)
    cfg0 = _cfg(50, 2, 1, 48, 0)
    _, g0 = _run(_lm(cfg0, st), codes)
    l64, g64 = R.loss_and_grads(st, codes, cfg0, torch.float64)
    l32, g32 = R.loss_and_grads(st, codes, cfg0, torch.float32)
    check_grads(g0, g64, g32, 'past_context 0', floor=FLOOR)
    k = 'transformer.layers.0.self_attn.in_proj_bias'
    assert not torch.allclose(g[k][100:], g0[k][100:], rtol=1e-3, atol=0)


def test_gpu_nll_is_the_loss_the_coder_sees():
    """nll = -mean log of forward()'s probabilities at the codes (teacher-forced inputs), to fp32
    summation accuracy, on the g12 LM."""
    from fixtures import g12_lm_config
    cfg, st = g12_lm_config('b')
    lm = _lm(cfg, st).eval()
    codes = _codes(cfg, 3, 4, 40, 11).to(DEV)
    inp = torch.zeros_like(codes)
    inp[:, :, 1:] = codes[:, :, :-1] + 1
    probas, _, _ = lm(inp)                       # [B, card, K, T]
    want = float(-torch.log(probas.double().gather(1, codes[:, None])).mean())
    with torch.no_grad():
        got = float(lm.nll(codes))
    # 480 terms of magnitude <~ 30 summed in fp32-rounded pieces: each term carries <= 4 u of the
    # largest logit (log-softmax against log of the rounded probability)
    assert abs(got - want) <= 8 * 2.0 ** -24 * 30, (got, want)


def test_gpu_nll_is_deterministic():
    cfg, B, K, T, _ = CASES['hd25_T70_sees0_card1024']
    st, codes, *_ = _reference('hd25_T70_sees0_card1024')
    lm = _lm(cfg, st)
    a = _run(lm, codes)
    b = _run(lm, codes)
    assert a[0] == b[0]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_gpu_bad_code_raises_and_leaves_grads_alone():
    cfg, B, K, T, _ = CASES['hd25_T7_2layers']
    st, codes, *_ = _reference('hd25_T7_2layers')
    lm = _lm(cfg, st)
    _, g = _run(lm, codes)
    for bad in (cfg.card, -1):
        c = codes.clone()
        c[1, 2, 3] = bad
        with pytest.raises(ValueError, match='outside'):
            lm.nll(c.to(DEV))
    for k, p in lm.named_parameters():
        assert torch.equal(p.grad.cpu(), g[k]), k


def test_gpu_backward_refuses_changed_parameters_and_a_second_pass():
    cfg, B, K, T, _ = CASES['hd25_T7_2layers']
    st, codes, *_ = _reference('hd25_T7_2layers')
    lm = _lm(cfg, st)
    loss = lm.nll(codes.to(DEV))
    with torch.no_grad():
        lm.transformer.layers[0].linear1.bias.add_(1.0)
    with pytest.raises(RuntimeError, match='changed between'):
        loss.backward()
    loss = lm.nll(codes.to(DEV))
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='differentiated once'):
        loss.backward()
    # an incoming grad other than 1 scales every gradient
    _, g1 = _run(lm, codes)
    lm.zero_grad(set_to_none=True)
    (lm.nll(codes.to(DEV)) * 0.5).backward()
    for k, p in lm.named_parameters():
        assert torch.equal(p.grad.cpu(), (g1[k] * 0.5)) or torch.allclose(p.grad.cpu(), g1[k] * 0.5, rtol=1e-6, atol=0), k


def test_gpu_ce_kernel_counts_bad_codes():
    """encx_lm_ce on its own: a code outside [0, card) is counted in the error word, its gradient
    row is zero, and the other rows are (softmax - onehot) * scale."""
    from encx._lib import call, lib, stream
    N, K, card = 5, 2, 48
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(N, K, card, generator=g).to(DEV)
    codes = torch.randint(0, card, (1, K, N), generator=g)
    codes[0, 1, 2] = card
    codes[0, 0, 4] = -3
    cd = codes.to(DEV)
    work = torch.empty(int(lib.encx_lm_ce_workspace(N, K)) // 4, device=DEV)
    d = logits.clone()
    out = torch.empty((), device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    scale = 1.0 / (N * K)
    call('encx_lm_ce', d.data_ptr(), 0, N, N, N, K, card, cd.data_ptr(), *cd.stride(), scale, work.data_ptr(), stream())
    call('encx_lm_ce_finish', work.data_ptr(), N, K, scale, out.data_ptr(), err.data_ptr(), stream())
    assert int(err.item()) == 2
    ok = torch.ones(N, K, dtype=torch.bool)
    ok[2, 1] = ok[4, 0] = False
    assert float(d.cpu()[~ok].abs().max()) == 0
    ls = torch.log_softmax(logits.double().cpu(), -1)
    tgt = codes[0].t().clamp(0, card - 1)                                  # [N, K]
    want = torch.exp(ls) - torch.nn.functional.one_hot(tgt, card)
    np.testing.assert_allclose(d.cpu()[ok].numpy(), (want[ok] * scale).numpy(), atol=16 * 2.0 ** -24 * scale)  # expf 2 ulp, a 48-term sum, a divide
    wl = float(-(ls.gather(-1, tgt[..., None])[..., 0][ok]).sum() * scale)
    assert abs(float(out) - wl) <= 16 * 2.0 ** -24 * 8


def test_gpu_forward_after_flat_adam_step_is_not_stale():
    """FlatAdam writes the parameters through raw pointers, which the (data_ptr, _version) key of
    the stacked embeddings / heads cannot see: forward() after a step must use the new weights,
    and equal the fp64 restatement after the same Adam step within the rule."""
    from encx.optim import FlatAdam
    cfg, B, K, T, _ = CASES['hd25_T7_2layers']
    st, codes, *_ = _reference('hd25_T7_2layers')
    lr, eps = 1e-2, 1e-3   # a smooth Adam step: no sign decisions on gradients that are rounding
    lm = _lm(cfg, st)
    opt = FlatAdam(lm.parameters(), lr=lr, eps=eps)
    inp = torch.zeros_like(codes)
    inp[:, :, 1:] = codes[:, :, :-1] + 1
    before = lm(inp.to(DEV))[0].cpu()
    opt.zero_grad()
    lm.nll(codes.to(DEV)).backward()
    opt.step()
    after = lm(inp.to(DEV))[0].cpu()
    assert float((after - before).abs().max()) > 1e-4, 'forward() still sees the weights from before the step'
    _, st64 = R.adam_steps(st, [codes], cfg, torch.float64, lr, eps=eps)
    _, st32 = R.adam_steps(st, [codes], cfg, torch.float32, lr, eps=eps)
    with torch.no_grad():
        p64 = O.lm_all(st64, codes, cfg)
        p32 = O.lm_all(st32, codes, cfg)
    check_grads({'probas': after}, {'probas': p64}, {'probas': p32}, 'forward after one FlatAdam step', floor=FLOOR)


# ------------------------------------------------------------------------------ it learns
LEARN_CFG = O.LMConfig(n_q=1, card=64, dim=64, num_heads=2, num_layers=1, past_context=20)
LEARN_LR, LEARN_EPS = 3e-3, 1e-5
LEARN_STEPS, LEARN_LOG = 60, 10


def markov_batches(n=30, B=8, T=48, seed=0):
    """First-order Markov code streams: the next code is perm[code] with probability 0.9, else
    uniform (entropy ~0.74 nats per code against ln 64 = 4.16 un-modelled)."""
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(1234))   # the chain: one for every seed
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        c = torch.empty(B, 1, T, dtype=torch.int64)
        c[:, 0, 0] = torch.randint(0, 64, (B,), generator=g)
        for t in range(1, T):
            jump = torch.rand(B, generator=g) < 0.1
            c[:, 0, t] = torch.where(jump, torch.randint(0, 64, (B,), generator=g), perm[c[:, 0, t - 1]])
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def learn_reference(dtype):
    st = R.synth(LEARN_CFG, 77)
    return R.adam_steps(st, markov_batches(), LEARN_CFG, dtype, LEARN_LR, steps=LEARN_STEPS, eps=LEARN_EPS)


def test_gpu_lm_learns_and_files_shrink():
    from encx._lib import lib
    from encx.optim import FlatAdam
    l64, _ = learn_reference(torch.float64)
    l32, _ = learn_reference(torch.float32)
    assert l64[-1] < 0.5 * math.log(LEARN_CFG.card), l64[-1]    # the step count was chosen for this
    batches = [b.to(DEV) for b in markov_batches()]
    lm = _lm(LEARN_CFG, R.synth(LEARN_CFG, 77))
    opt = FlatAdam(lm.parameters(), lr=LEARN_LR, eps=LEARN_EPS)
    mine = []
    for i in range(LEARN_STEPS):
        opt.zero_grad()
        loss = lm.nll(batches[i % len(batches)])
        loss.backward()
        opt.step()
        mine.append(loss.detach())
    mine = torch.stack(mine).cpu().tolist()
    for i in list(range(0, LEARN_STEPS, LEARN_LOG)) + [LEARN_STEPS - 1]:
        _check_loss(mine[i], l64[i], l32[i], f'learning step {i}')
    lm.eval()
    codes = markov_batches(1, 4, 48, seed=9)[0].to(DEV)       # streams the LM did not train on
    datas = lm.encode_streams(codes)
    raw = int(lib.encx_bitpack_bytes(codes.shape[1] * codes.shape[2], 6))
    assert all(len(d) < raw for d in datas), ([len(d) for d in datas], raw)
    back, _ = lm.decode_streams(datas, 1, 48)
    assert torch.equal(back, codes)


# ------------------------------------------------------------------------------ command line
def _write_wav(path, seed):
    """1 s of 24 kHz mono PCM16: two tones and a little noise."""
    g = np.random.default_rng(seed)
    t = np.arange(24000) / 24000.0
    x = 0.4 * np.sin(2 * np.pi * (300 + 40 * seed) * t) + 0.2 * np.sin(2 * np.pi * 1300 * t + seed)
    x = x + 0.02 * g.standard_normal(x.shape)
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(24000)
        w.writeframes((x * 32768).round().astype('<i2').tobytes())


def test_gpu_train_lm_cli_round_trip(tmp_path):
    """train_lm.py for a few steps on synthetic WAVs, --merge-into, then main.py -l -c merged:
    compress + decompress gives the use_lm=False wave bit for bit, through the trained LM."""
    from test_cli import run
    from fixtures import load, model_state, codebooks_from_stats
    from oracle import encodec_oracle as EO
    from encx import train_lm
    from encx.model import EncodecModel
    cfg = EO.Config(sample_rate=24000, channels=1, causal=False, norm='time_group_norm', audio_normalize=True,
                    target_bandwidths=(1.5, 3., 6., 12., 24.))
    sd = dict(model_state(cfg, 131))
    for i, cb in enumerate(codebooks_from_stats(load('g1_eval24k.npz')['stats'], 133, 2, cfg.n_q)):
        for k, v in cb.items():
            sd[f'quantizer.vq.layers.{i}._codebook.{k}'] = v
    ckpt = tmp_path / 'codec.pt'
    torch.save({'epoch': 0, 'model_state_dict': sd}, ckpt)
    for i in range(3):
        _write_wav(tmp_path / f'{i}.wav', i)
    (tmp_path / 'files.csv').write_text('path\n' + ''.join(f'{tmp_path / f"{i}.wav"}\n' for i in range(3)))
    merged = tmp_path / 'codec_lm.pt'
    args = train_lm.get_parser().parse_args(
        ['-c', str(ckpt), '--csv', str(tmp_path / 'files.csv'), '-b', '1.5', '--batch-size', '3', '--crop', '12000',
         '--epochs', '3', '--lr', '1e-3', '--dim', '48', '--layers', '1', '--heads', '2', '--log-every', '1',
         '--out', str(tmp_path / 'lm.pt'), '--merge-into', str(merged), '-d', DEV])
    lm, last = train_lm.train(args)
    assert math.isfinite(last)
    saved = torch.load(tmp_path / 'lm.pt', map_location='cpu', weights_only=True)
    assert set(saved) == {'lm_state_dict', 'lm_config'} and saved['lm_config']['dim'] == 48
    common = ['-m', 'my_encodec', '-d', DEV, '-b', '1.5']
    run(*common, '-c', merged, '-l', tmp_path / '0.wav', tmp_path / 'lm.ecdc')
    run(*common, '-c', merged, tmp_path / 'lm.ecdc', tmp_path / 'lm.wav')
    run(*common, '-c', ckpt, tmp_path / '0.wav', tmp_path / 'plain.ecdc')
    run(*common, '-c', ckpt, tmp_path / 'plain.ecdc', tmp_path / 'plain.wav')
    assert (tmp_path / 'lm.wav').read_bytes() == (tmp_path / 'plain.wav').read_bytes()
    assert (tmp_path / 'lm.ecdc').read_bytes() != (tmp_path / 'plain.ecdc').read_bytes()
    m = EncodecModel.my_encodec_model(str(merged))
    assert m.get_lm_model().dim == 48
    for k, v in lm.state_dict().items():
        assert torch.equal(m.get_lm_model().state_dict()[k], v.cpu()), k
