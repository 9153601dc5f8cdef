"""The LM inference kernels (csrc/lm.hip, the softmax / cdf / coder kernels of csrc/ac.hip, encx/lm.py)
beyond the shapes of the g12 fixture: head dims 2..64 on both attention kernels and both of their
instantiations, dims 4..512, past_context 0, 1 and longer than the sequence, attention windows above
64 KB of LDS with and without slots, card above one pass of the decoder's symbol search (up to the
limit of 65536), n_q 64, the border between the two GEMM kernels, and the refusals just past each limit.

References, all outside the code under test: oracle/lm_oracle.lm_all in fp64 for the probabilities
(weights of synth.synth_lm_state, a fixed seed per case), oracle/ac_oracle for the cdf rows and the
coded bytes, and for a streaming session the linear-cache path one stream at a time (drive /
check_against_linear of tests/test_gpu_stream_lm_nq.py).

Tolerance: the project's LM bound of tests/test_lm.py against fp64, rtol 2e-4 and atol 1e-6, no extra
margin. Everything else is torch.equal / == : the same row computed by another kernel, in another
launch or from another call split, cdf rows, bytes, codes.

Measured on an MI355X, worst error / bound per case, then max|p - p64| / max|p64| of the GPU and of
lm_all in fp32 on the host (printed by every run, the second pair not asserted):
    hd2         0.005 (3.5e-07, 4.4e-07)    hd32        0.024 (1.0e-06, 1.2e-06)    hd33        0.025 (1.5e-06, 2.2e-06)
    hd48_sees0  0.014 (9.2e-07, 6.6e-07)    hd64        0.032 (1.6e-06, 1.6e-06)    P0          0.014 (6.0e-07, 8.7e-07)
    P1          0.014 (5.8e-07, 7.6e-07)    dim512      0.094 (4.7e-06, 3.7e-06)    block_hd33  0.174 (8.3e-06, 8.6e-06)
    block_hd64  0.142 (8.1e-06, 5.8e-06)    card 1500   0.018 (1.2e-06, 3.0e-06)    card 2049   0.018 (1.3e-06, 1.8e-06)
    n_q 64      0.028 (1.1e-06, 8.9e-07)    card 65536  0.004 (3.7e-07, 7.5e-05)
    slots (against lm_step in fp64): dim 66 0.019, dim 128 0.041, dim 512 0.028
"""
import numpy as np
import pytest
import torch

from oracle import ac_oracle as A
from oracle import lm_oracle as L
from fixtures import T as tensor
from synth import synth_lm_state
from test_gpu_stream_lm_nq import drive, check_against_linear, lm_inputs, CHANGE_RUN, CHANGE_NQ, DEV
from test_gpu_stream_packets import LM_T

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 1e-6   # tests/test_lm.py


def make_lm(seed, dim, heads, past_context, layers=1, card=48, n_q=3):
    """-> (the LM on the GPU, its LMConfig, its state dict on the host)."""
    from encx.lm import LMModel
    cfg = L.LMConfig(n_q=n_q, card=card, dim=dim, num_heads=heads, num_layers=layers, past_context=past_context)
    st = {k: tensor(v) for k, v in synth_lm_state(L.lm_param_shapes(cfg), seed).items()}
    lm = LMModel(n_q, card, dim=dim, num_heads=heads, num_layers=layers, past_context=past_context)
    lm.load_state_dict(st)
    return lm.to(DEV).eval(), cfg, st


def draw(seed, B, K, Tn, card):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, card, size=(B, K, Tn)))


def teacher_forced(codes):
    full = torch.zeros_like(codes)
    full[:, :, 1:] = codes[:, :, :-1] + 1
    return full


def oracle_probs(st, codes, cfg, dtype):
    """lm_all with every tensor it makes (the sin embedding too) in `dtype` -> [B, card, K, T]."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return L.lm_all({k: v.to(dtype) for k, v in st.items()}, codes, cfg)
    finally:
        torch.set_default_dtype(prev)


def check_vs_fp64(name, mine, st, codes, cfg):
    """mine [B, card, K, T] (host) within the LM bound of lm_all in fp64; prints the figures first."""
    p64 = oracle_probs(st, codes, cfg, torch.float64).numpy()
    p32 = oracle_probs(st, codes, cfg, torch.float32).numpy()
    mine = mine.numpy()
    worst = float(np.max(np.abs(mine - p64) / (ATOL + RTOL * np.abs(p64))))
    top = float(np.abs(p64).max())
    print(f'{name}: worst error / bound = {worst:.3f}; max|p - p64| / max|p64| = '
          f'{float(np.abs(mine - p64).max()) / top:.2e} (GPU), {float(np.abs(p32 - p64).max()) / top:.2e} (lm_all in fp32)')
    np.testing.assert_allclose(mine, p64, rtol=RTOL, atol=ATOL)


def in_pieces(lm, full, p_all, pieces):
    """The same sequence in calls of the given lengths: every call's probabilities bit for bit."""
    assert sum(pieces) == full.shape[2]
    states, off = None, 0
    for n in pieces:
        p, states, new_off = lm(full[:, :, off:off + n].contiguous(), states, off)
        assert new_off == off + n
        assert torch.equal(p, p_all[..., off:off + n]), (off, n)
        off = new_off


# ============================================================================ 1. one pass, and in pieces
#        name: dim, heads, past_context, layers, card, (B, K, T), row-kernel split of a block-route case
CASES = {
    'hd2': (4, 2, 3, 1, 48, (2, 2, 9), None),               # the smallest dim the input stage takes
    'hd32': (64, 2, 3, 1, 48, (3, 3, 70), None),            # upper edge of <32>
    'hd33': (66, 2, 3, 1, 48, (3, 3, 70), None),            # first of <64>; dim % 4 != 0: one row on the MFMA GEMM too
    'hd48_sees0': (96, 2, 75, 1, 48, (1, 3, 7), None),      # every row sees position 0
    'hd64': (128, 2, 12, 2, 48, (3, 1, 70), None),          # upper edge of <64>
    'P0': (64, 4, 0, 1, 48, (2, 2, 9), None),               # a row sees only itself
    'P1': (64, 4, 1, 1, 48, (2, 2, 9), None),               # and one back
    'dim512': (512, 8, 262, 1, 64, (1, 2, 300), None),      # LayerNorm's limit; 68380 bytes of LDS, no slots
    'block_hd33': (264, 8, 70, 1, 48, (1, 2, 513), (256, 256, 1)),   # 4104 (row, head) pairs; one live lane at the end
    'block_hd64': (128, 2, 3, 1, 48, (5, 1, 411), (200, 200, 11)),   # 4110 pairs; 27 live lanes at the end
}


BLOCK_CASES = [name for name, c in CASES.items() if c[-1]]


@pytest.fixture(scope='module')
def one_pass():
    """one_pass(name) -> (lm, cfg, st, codes, full, p_all): the case's LM, its teacher-forced input and the
    probabilities of one call over the whole sequence; computed at first use, shared, left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            dim, heads, P, layers, card, (B, K, Tn), split = CASES[name]
            seed = 300 + list(CASES).index(name)
            lm, cfg, st = make_lm(seed, dim, heads, P, layers=layers, card=card, n_q=K)
            codes = draw(seed, B, K, Tn, card)
            assert (B * Tn * heads > 4096) == bool(split)   # which attention kernel the one pass takes
            full = teacher_forced(codes).to(DEV)
            p_all, _, off = lm(full)
            assert off == Tn and p_all.shape == (B, card, K, Tn)
            cache[name] = (lm, cfg, st, codes, full, p_all)
        return cache[name]
    return get


@pytest.fixture(scope='module')
def dim512(one_pass):
    """The dim-512, 8-head LM (head dim 64, past_context 262, card 64, n_q 2) that parts 1, 4 and 5 share."""
    return one_pass('dim512')[:3]


@pytest.mark.parametrize('name', list(CASES))
def test_one_pass_vs_fp64_oracle(name, one_pass):
    lm, cfg, st, codes, full, p_all = one_pass(name)
    check_vs_fp64(name, p_all.cpu(), st, codes, cfg)


@pytest.mark.parametrize('name', list(CASES))
def test_steps_equal_the_one_pass(name, one_pass):
    """T - 5 steps in one call, then 5 single steps, bit for bit."""
    lm, cfg, st, codes, full, p_all = one_pass(name)
    in_pieces(lm, full, p_all, [codes.shape[2] - 5] + [1] * 5)


@pytest.mark.parametrize('name', BLOCK_CASES)
def test_block_and_row_attention_agree(name, one_pass):
    """The one pass took the many-row (block) kernel; calls of at most 4096 (row, head) pairs take the few-row
    kernel: the same bits at head dims above 32."""
    lm, cfg, st, codes, full, p_all = one_pass(name)
    split = CASES[name][-1]
    assert all(codes.shape[0] * n * cfg.num_heads <= 4096 for n in split)
    in_pieces(lm, full, p_all, list(split))


# ============================================================================ 2. the two GEMM kernels
@pytest.mark.parametrize('dim, heads', [(64, 4), (200, 8)])
def test_rows_64_and_65_give_the_same_bits(dim, heads):
    """65 streams: at T = 1 every linear layer and the heads run on the MFMA GEMM; the first 64 of the same
    streams alone run on the VALU kernel (dim 200: a k tail of 72 in a chunk of 128). Then 3 more steps."""
    lm, cfg, _ = make_lm(320 + dim, dim, heads, 5, n_q=2)
    inp = teacher_forced(draw(321, 65, 2, 4, cfg.card)).to(DEV)
    out = []
    for B in (65, 64):
        p1, states, off = lm(inp[:B, :, :1].contiguous())
        p3, _, _ = lm(inp[:B, :, 1:].contiguous(), states, off)
        out.append((p1, p3))
    assert torch.equal(out[0][0][:64], out[1][0])
    assert torch.equal(out[0][1][:64], out[1][1])


# ============================================================================ 3. card > 1024, n_q 64
def round_trip(lm, cfg, st, codes, row_stride):
    """The checks of test_lm.test_gpu_lm_coder_round_trip_and_oracle_bytes, and the probabilities
    against lm_all in fp64."""
    B, K, Tn = codes.shape
    dcodes = codes.to(DEV)
    datas = lm.encode_streams(dcodes)
    for graph in (True, False):
        back, used = lm.decode_streams(datas, K, Tn, graph=graph)
        assert torch.equal(back, dcodes), graph
        assert used == [len(x) for x in datas], graph
    full = teacher_forced(dcodes)
    x = lm._body(full, full.stride(), B, K, Tn, False, lm.new_state(B, Tn + 1))
    probas = torch.empty(B, Tn, K, cfg.card, device=DEV)
    cdf = torch.empty(B, Tn, K, cfg.card, device=DEV, dtype=torch.int32)
    lm._heads(x, B, Tn, K, probas=probas, cdf=cdf)
    probas, cdf = probas.cpu(), cdf.cpu().numpy().astype(np.int64)
    for b in range(B):
        rows = [(t, k) for t in range(Tn) for k in range(K)]
        for t, k in rows[::row_stride]:
            np.testing.assert_array_equal(A.quantized_cdf(probas[b, t, k].numpy(), 24, check=False), cdf[b, t, k])
        assert A.encode([int(codes[b, k, t]) for t, k in rows], [cdf[b, t, k] for t, k in rows]) == datas[b]
    check_vs_fp64(f'card {cfg.card} n_q {cfg.n_q}', probas.permute(0, 3, 2, 1), st, codes, cfg)


@pytest.mark.parametrize('card', [1500, 2049])
def test_card_above_one_pass_of_the_symbol_search(card):
    """The decoder scans the cdf 1024 entries a pass: codes from every pass, and the last entry."""
    lm, cfg, st = make_lm(330 + card, 64, 4, 5, card=card, n_q=2)
    codes = draw(card, 2, 2, 12, card)
    for p in range(-(-card // 1024)):   # every pass of the search finds a symbol: its 8th entry and its last
        codes[0, p % 2, 2 + p] = min(card - 1, 1024 * p + 7)
        codes[1, 0, 2 + p] = min(card - 1, 1024 * p + 1023)
    assert bool((codes < 1024).any()) and bool((codes >= 1024).any()) and int(codes.max()) == card - 1
    if card == 2049:
        assert bool((codes == 2048).any()) and bool(((codes >= 1024) & (codes < 2048)).any())
    round_trip(lm, cfg, st, codes, 5)


def test_n_q_64():
    lm, cfg, st = make_lm(340, 64, 4, 5, card=48, n_q=64)
    round_trip(lm, cfg, st, draw(341, 2, 64, 6, 48), 37)


def test_card_65536():
    lm, cfg, st = make_lm(350, 8, 2, 5, card=65536, n_q=1)
    codes = draw(351, 1, 1, 3, 65536)
    codes[0, 0, 1] = 65535
    round_trip(lm, cfg, st, codes, 1)


# ============================================================================ 4. > 64 KB of LDS, no slots
def decode_round_trip(lm, codes):
    datas = lm.encode_streams(codes)
    for graph in (True, False):
        back, used = lm.decode_streams(datas, codes.shape[1], codes.shape[2], graph=graph)
        assert torch.equal(back, codes), graph
        assert used == [len(x) for x in datas], graph


def test_default_lm_decodes_with_a_window_of_104104_bytes():
    """LMModel's own defaults (dim 200, 8 heads, 5 layers, past_context 1000): the captured decode step
    sizes the attention window for the whole past_context, 1001 x 26 floats."""
    from encx.lm import LMModel
    cfg = L.LMConfig(n_q=4, card=64, past_context=1000)
    lm = LMModel(4, 64)
    tr = lm.transformer
    assert (lm.dim, tr.num_heads, len(tr.layers), tr.past_context) == (200, 8, 5, 1000)
    lm.load_state_dict({k: tensor(v) for k, v in synth_lm_state(L.lm_param_shapes(cfg), 360).items()})
    decode_round_trip(lm.to(DEV).eval(), draw(361, 2, 4, 6, 64).to(DEV))


def test_dim512_decodes_with_a_window_of_68380_bytes(dim512):
    lm, cfg, _ = dim512
    decode_round_trip(lm, draw(362, 2, 2, 6, cfg.card).to(DEV))


# ============================================================================ 5. slots at head dims > 32
def session(name, lm, cfg, st, codes, schedule, nqs, R):
    """drive() over the schedule, then check_against_linear: cdf rows with torch.equal and packets byte for
    byte against the linear-cache path, one stream at a time. The linear path runs the same attention
    arithmetic, so the encoder's probabilities of every step are also held against lm_step in fp64, driven
    chunk by chunk per stream, under the LM bound."""
    from encx.lm import LMStreamEncoder, LMStreamDecoder
    B, K, _ = codes.shape
    enc = LMStreamEncoder(lm, B, K, probas=True, lm_format=2)
    dec = LMStreamDecoder(lm, B, K, lm_format=2)
    assert enc.R == R
    off, run, probs = [0] * B, [[] for _ in range(B)], [[] for _ in range(B)]
    for frames, nq in zip(schedule, nqs):
        out, _, _ = drive(lm, codes, [frames], [nq], enc=enc, dec=dec, off=off)
        for b, (f, q) in enumerate(zip(frames, nq)):
            run[b] += out[b]
            if f:
                probs[b].append(enc.last_probas[b, :f, :q].cpu().numpy())
    check_against_linear(lm, codes, run)
    st64, worst = {k: v.double() for k, v in st.items()}, 0.
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)   # the oracle's own sin embedding in fp64 too
    try:
        for b in range(B):
            chunks = [(n, q) for _, n, q, _, _ in run[b]]
            kframe = [q for n, q in chunks for _ in range(n)]
            idx = lm_inputs(codes[b][:, :len(kframe)], kframe)
            states, o = None, 0
            for (n, q), mine in zip(chunks, probs[b]):
                p, states, nxt = L.lm_step(st64, idx[:q, o:o + n].unsqueeze(0), states, o, cfg)
                want = p.permute(0, 3, 2, 1)[0].numpy()   # [n, q, card]
                worst = max(worst, float(np.max(np.abs(mine - want) / (ATOL + RTOL * np.abs(want)))))
                np.testing.assert_allclose(mine, want, rtol=RTOL, atol=ATOL, err_msg=f'slot {b} frames {o}..')
                o = nxt
    finally:
        torch.set_default_dtype(prev)
        print(f'{name}: streamed probabilities vs lm_step in fp64, worst error / bound = {worst:.3f}')


@pytest.mark.parametrize('dim', [66, 128])
def test_slots_at_head_dims_33_and_64(dim):
    """past_context 5: the ring of 13 rows wraps; three streams with a changing n_q."""
    lm, cfg, st = make_lm(370 + dim, dim, 2, 5, card=64, n_q=4)
    session(f'slots dim {dim}', lm, cfg, st, draw(371, 3, 4, LM_T, 64), CHANGE_RUN, CHANGE_NQ, 13)


def test_slots_dim512_window_of_68380_bytes(dim512):
    """Two steps of 8 frames on two slots: the hd > 32 slots kernel above 64 KB of LDS."""
    lm, cfg, st = dim512
    session('slots dim 512', lm, cfg, st, draw(372, 2, 2, 16, cfg.card), ((8, 8), (8, 8)), ((2, 1), (1, 2)), 270)


# ============================================================================ 6. refusals
def test_refusals_just_past_the_limits():
    """Each is a ValueError that names the limit, raised on the host; the process stays usable."""
    from encx.lm import LMModel, LMStreamEncoder, LMStreamDecoder
    lm, cfg, _ = make_lm(380, 64, 4, 5, n_q=2)
    inp = teacher_forced(draw(381, 2, 2, 5, cfg.card)).to(DEV)
    p0 = lm(inp)[0].clone()

    def still_fine():
        assert torch.equal(lm(inp)[0], p0)

    for kw, msg in ((dict(dim=130, num_heads=2), 'head dim 65'),
                    (dict(dim=514, num_heads=257), 'dim 514'),
                    (dict(dim=65, num_heads=5), 'dim 65'),
                    (dict(dim=2, num_heads=1), 'dim 2')):
        with pytest.raises(ValueError, match=msg + '.*this port'):
            LMModel(2, 48, num_layers=1, **kw)
        still_fine()
    with pytest.raises(ValueError, match='card 65537.*this port'):
        LMModel(1, 65537, dim=8, num_heads=2, num_layers=1)
    still_fine()
    # n_q 65: the model exists (its first 64 codebooks can be used); a call or a session of 65 is refused
    torch.manual_seed(65)
    lm65 = LMModel(65, 48, dim=64, num_heads=4, num_layers=1, past_context=5).to(DEV).eval()
    for session in (LMStreamEncoder, LMStreamDecoder):
        with pytest.raises(ValueError, match='at most 64'):
            session(lm65, 1, 65, lm_format=2)
    with pytest.raises(ValueError, match='65 codebooks.*this port'):
        lm65(torch.zeros(1, 65, 1, dtype=torch.int64, device=DEV))
    still_fine()
    assert lm65(torch.zeros(1, 64, 1, dtype=torch.int64, device=DEV))[0].shape == (1, 48, 64, 1)
    # 601 positions x 65 floats = 156260 bytes, above the 150 KB the window may take: the decode step
    # with its device-side counter and a session are refused, the calls with a short window still run
    torch.manual_seed(600)
    lm600 = LMModel(2, 64, dim=512, num_heads=8, num_layers=1, past_context=600).to(DEV).eval()
    codes = draw(382, 1, 2, 4, 64).to(DEV)
    datas = lm600.encode_streams(codes)
    with pytest.raises(ValueError, match='LDS.*this port'):
        lm600.decode_streams(datas, 2, 4)
    still_fine()
    with pytest.raises(ValueError, match='LDS.*this port'):
        LMStreamEncoder(lm600, 1, 2)
    assert torch.equal(lm600.decode_streams(datas, 2, 4, graph=False)[0], codes)
    LMStreamEncoder(LMModel(2, 64, dim=512, num_heads=8, num_layers=1, past_context=589), 1, 2)   # 153400 bytes
    still_fine()
