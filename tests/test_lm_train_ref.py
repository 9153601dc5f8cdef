"""CPU checks for LM training: the differentiable restatement (tests/lm_train_ref.py) against
the oracle's lm_all and against finite differences, and the host side of the new entry points."""
import torch

import lm_train_ref as R
from fixtures import g12_lm_config
from oracle import lm_oracle as O


def test_restatement_probabilities_equal_lm_all_exactly():
    """fp32, the g12 LMs: softmax of the restatement's logits is lm_all's output bit for bit
    (same pieces, same order), so its cross-entropy is -log of the probabilities the oracle --
    and through it the reference -- assigns."""
    for name, (B, K, T) in (('b', (2, 3, 9)), ('a', (1, 2, 4))):
        cfg, st = g12_lm_config(name)
        g = torch.Generator().manual_seed(5)
        codes = torch.randint(0, cfg.card, (B, K, T), generator=g)
        with torch.no_grad():
            lg = R.logits(st, codes, cfg)
            assert torch.equal(torch.softmax(lg, dim=1), O.lm_all(st, codes, cfg))
            want = -torch.log(O.lm_all(st, codes, cfg).double().gather(1, codes[:, None])).mean()
            assert abs(float(R.nll(st, codes, cfg)) - float(want)) <= 1e-5 * float(want)


def test_restatement_gradcheck_fp64():
    cfg = O.LMConfig(n_q=2, card=5, dim=8, num_heads=2, num_layers=1, past_context=2)
    st = R.state(R.synth(cfg, 3), torch.float64)
    codes = torch.tensor([[[1, 4, 0, 2], [3, 3, 1, 0]]])
    names = list(st)

    def f(*ts):
        return R.nll(dict(zip(names, ts)), codes, cfg)
    assert torch.autograd.gradcheck(f, [st[k] for k in names], eps=1e-6, atol=1e-6, rtol=1e-4)


def test_loss_and_grads_zero_past_K():
    cfg = O.LMConfig(n_q=3, card=6, dim=8, num_heads=2, num_layers=1, past_context=4)
    st = R.synth(cfg, 4)
    codes = torch.randint(0, 6, (2, 2, 5), generator=torch.Generator().manual_seed(1))
    loss, g = R.loss_and_grads(st, codes, cfg, torch.float64)
    assert loss > 0 and float(g['emb.2.weight'].abs().max()) == 0 and float(g['linears.2.bias'].abs().max()) == 0
    assert float(g['emb.0.weight'][0].abs().max()) > 0     # the t = 0 "missing" token's row


def test_lm_train_host_checks():
    """The new entry points refuse bad arguments (9001) before any device call, and the
    workspace queries return their formulas (-1 out of range)."""
    from encx._lib import lib
    lib.load()
    assert lib.encx_lm_ce_workspace(10, 3) == 2 * 10 * 3 * 4
    assert lib.encx_lm_ce_workspace(10, 0) == -1
    N, D, K = 70, 50, 3
    assert lib.encx_lm_input_bwd_workspace(2, 35, D, K) == (N * D + 9 * 2 * D + K * N) * 4   # 9 = ceil(70 / 8) LayerNorm partials
    assert lib.encx_lm_input_bwd_workspace(2, 35, 0, K) == -1
    # fewer than 128 rows: one slab of [K card][D + 1] (the bias grad is its last column)
    assert lib.encx_lm_heads_bwd_workspace(100, 50, 3, 48) == 3 * 48 * 51 * 4
    assert lib.encx_lm_heads_bwd_workspace(0, 50, 3, 48) == -1
    # one buffer sized for a pass's largest chunk serves its shorter last chunk: the query never
    # shrinks with the rows, also where the shorter chunk runs MORE slabs (320 rows: 5 of 64, 330
    # rows: 4 of 96; 2048: 32, 2100: 22) -- it covers the 5 (32) slabs of [K card][D + 1]
    for big, small, slabs in ((330, 320, 5), (2100, 2048, 32)):
        assert lib.encx_lm_heads_bwd_workspace(big, 50, 3, 48) >= lib.encx_lm_heads_bwd_workspace(small, 50, 3, 48) \
            >= slabs * 3 * 48 * 51 * 4
    sizes = [lib.encx_lm_heads_bwd_workspace(n, 50, 3, 48) for n in range(1, 2200)]
    assert sizes == sorted(sizes)
    sizes = [lib.encx_lm_heads_bwd_workspace(n, 200, 8, 1024) for n in range(1, 5000, 7)]
    assert sizes == sorted(sizes)
    w = lib.encx_lm_layer_bwd_workspace(2, 35, D, 2, 4 * D)
    fixed = N * (7 * D + 4 * D) + 2 * 2 * D + N * 2 * 3 + 9 * 2 * D
    assert w >= (fixed + 3 * D * (D + 1)) * 4 and w % 4 == 0
    assert lib.encx_lm_layer_bwd_workspace(2, 35, D, 0, 4 * D) == -1
    assert lib.encx_lm_ce(None, 0, 4, 4, 2, 1, 48, None, 0, 0, 0, 1.0, None, None) == 9001      # null pointers
    assert lib.encx_lm_ce(None, 3, 4, 4, 2, 1, 48, None, 0, 0, 0, 1.0, None, None) == 9001      # rows past N
    assert lib.encx_lm_ce_finish(None, 4, 1, 1.0, None, None, None) == 9001
    assert lib.encx_lm_heads_bwd(*([None] * 2 + [4, 50] + [None] + [3, 48] + [None] * 3 + [0, None, None])) == 9001
    # 7 heads do not divide dim 200; then null pointers
    bad = [None] * 3 + [1, 4, None, 5, 3, 200, 7, 800] + [None] * 23
    assert lib.encx_lm_layer_bwd(*bad) == 9001
    bad[9] = 8
    assert lib.encx_lm_layer_bwd(*bad) == 9001
    assert lib.encx_lm_input_bwd(*([None] * 2 + [0, 0, 0, 1, 2, 4] + [None] + [49, 50] + [None] * 6)) == 9001
    assert lib.encx_lm_input_bwd(*([None] * 2 + [0, 0, 0, 1, 2, 4] + [None] + [49, 7] + [None] * 6)) == 9001  # odd dim


def test_nll_refuses_cpu_and_bad_shapes():
    from encx.lm import LMModel
    import pytest
    lm = LMModel(2, 16, dim=8, num_heads=2, num_layers=1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        lm.nll(torch.zeros(1, 2, 3, dtype=torch.long))
