"""SEANet beyond the default architecture on the GPU, offline and streamed.

Every other test builds n_residual_layers=1, true_skip=False, compress=2, n_filters=32,
ratios=(8,5,4,2), lstm=2, kernels 7/7/3. Here the product's SEANetEncoder / SEANetDecoder run the
three architectures of fixtures.ARCHS (the g14 fixture pins the oracle's restatement of them to the
reference): several residual blocks per stage with dilations 1, 2, 4 (a fused j = 0 block beside
linked unfused dilated blocks in one autograd graph), the identity shortcut with its 'head' /
'tail' gradient hand-over, compress 4 with a hidden width of 3, channel widths that are no
multiple of 16, strides 3 and 6, kernel sizes 5/3/5, lstm 0 / 1 / 3, GroupNorm with an odd tail.

Bounds. Whole stacks and single blocks: the project's rule steputil.check_grads -- per tensor the
error against the fp64 oracle within 4x the plain fp32 oracle's (floor 1e-6); outputs through the
same helper. The dilated bwd-data with accumulate: the bound test_gpu_kernels uses for dx. The
public `ratios` model and the streamed arch A: the offline bounds of test_gpu_long.py (latent 1e-4,
wave 1e-3, codes equal wherever fp64 certifies them); slicing, batching, graphs and slots bit for bit.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encodec_oracle as O
from fixtures import load, T, model_state, codebooks_from_stats, rvq_certified, arch_cfg, arch_modules
from synth import synth_state, synth_wave
from steputil import check_grads, ORACLE_THREADS
from test_gpu_kernels import DILATED_LAYERS, _case_params, close, G
from test_gpu_long import check_segments, load_model
from test_gpu_stream import stream_decode, run, same, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def oracle_run(fn, p, x, gy, dtype):
    """fn(x, params) -> list of outputs, the last one backpropagated with gy -> name -> tensor:
    the outputs ('out0', ..), 'dx' and every parameter grad. fp32 on a fixed thread count."""
    nt = torch.get_num_threads()
    torch.set_num_threads(ORACLE_THREADS)
    try:
        pp = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items()}
        xx = x.detach().to(dtype).requires_grad_(True)
        outs = fn(xx, pp)
        outs[-1].backward(gy.to(dtype))
    finally:
        torch.set_num_threads(nt)
    res = {f'out{i}': o.detach() for i, o in enumerate(outs)}
    res['dx'] = xx.grad
    res.update({k: v.grad for k, v in pp.items()})
    return res


_ORACLE = {}  # key -> the oracle's (fp64, fp32) results: computed once, shared, left unchanged


def check(mine, p, fn, x, gy, what, key=None):
    """The 4x rule on the outputs and on dx + every parameter grad -> the worst err / bound."""
    res = _ORACLE.get(key)
    if res is None:
        res = oracle_run(fn, p, x, gy, torch.float64), oracle_run(fn, p, x, gy, torch.float32)
        if key is not None:
            _ORACLE[key] = res
    r64, r32 = res
    assert set(mine) == set(r64), set(mine) ^ set(r64)
    outs = [k for k in r64 if k.startswith('out')]
    grads = [k for k in r64 if not k.startswith('out')]
    assert all(v is not None for v in r64.values()) and all(mine[k] is not None for k in grads)
    table = check_grads({k: mine[k] for k in outs}, {k: r64[k] for k in outs}, {k: r32[k] for k in outs}, what + ' outputs')
    table += check_grads({k: mine[k] for k in grads}, {k: r64[k] for k in grads}, {k: r32[k] for k in grads},
                         what + ' grads')
    worst = max(table, key=lambda r: r[1] / r[3])
    print(f'{what}: worst err / bound {worst[1] / worst[3]:.3f} ({worst[0]})')
    return worst[1] / worst[3]


# --------------------------------------------------------------------------- whole stacks
def build_stack(name):
    import encx.modules as M
    cfg, seed = arch_cfg(name)
    p = model_state(cfg, seed)
    enc, dec = arch_modules(name, M)
    for pre, mod in (('encoder.', enc), ('decoder.', dec)):
        mod.load_state_dict({k[len(pre):]: v for k, v in p.items() if k.startswith(pre)})
    return cfg, p, enc.to(DEV), dec.to(DEV)


def stack_run(name, Tn, seed):
    """The product's encoder -> decoder with a seeded output grad -> (cfg, p, x, gy, mine, gy on
    the device, its clone taken before the backward)."""
    cfg, p, enc, dec = build_stack(name)
    x0 = T(synth_wave((2, cfg.channels, Tn), seed))
    x = x0.to(DEV).requires_grad_(True)
    emb = enc(x)
    y = dec(emb)
    gy0 = T(synth_wave(tuple(y.shape), seed + 1, amp=1.0))
    gy = gy0.to(DEV)
    keep = gy.clone()
    y.backward(gy)
    mine = {'out0': emb.detach(), 'out1': y.detach(), 'dx': x.grad}
    for pre, mod in (('encoder.', enc), ('decoder.', dec)):
        mine.update({pre + k: v.grad for k, v in mod.named_parameters()})
    return cfg, p, x0, gy0, mine, gy, keep


def stack_fn(cfg):
    def fn(x, p):
        emb = O.run_plan(x, p, cfg.enc_plan, cfg.causal, cfg.norm)
        return [emb, O.run_plan(emb, p, cfg.dec_plan, cfg.causal, cfg.norm)]
    return fn


@pytest.fixture
def fused_calls(monkeypatch):
    """Counts the blocks that take the fused kernel (ops.resblock -> ops.ResBlockFn) and all blocks."""
    from encx import ops
    from encx.modules.seanet import SEANetResnetBlock
    n = {'fused': 0, 'blocks': 0}
    orig, fwd = ops.resblock, SEANetResnetBlock.forward

    def counted(*a, **kw):
        n['fused'] += 1
        return orig(*a, **kw)

    def block(self, x):
        n['blocks'] += 1
        return fwd(self, x)
    monkeypatch.setattr(ops, 'resblock', counted)
    monkeypatch.setattr(SEANetResnetBlock, 'forward', block)
    return n


@pytest.mark.parametrize('name,Tn,fused', [('A', 4800, 2), ('A', 360, 0), ('B', 1200, 0), ('C', 607, 0)])
def test_stack_grads_vs_oracle(name, Tn, fused, fused_calls):
    """A at T = 4800: the dim-32 stages run at 2400 >= RESBLOCK_TMIN, so their j = 0 block is the
    fused kernel and the dilated j = 1, 2 blocks beside it (and every dim-16 block) the linked
    convs; at 60 hops nothing fuses. B: 24 * 50 samples. C: 15 * 40 + 7, an odd tail, so the
    strided convs' extra_padding is non-zero. (C's last conv has one output channel under
    GroupNorm(1, 1), which removes its bias: that grad is 0 in exact arithmetic, ~1e-12 in fp64 and
    rounding noise in fp32, so its row of the table is bounded by the fp32 oracle's noise alone.)"""
    from encx import ops
    cfg, p, x0, gy0, mine, gy, keep = stack_run(name, Tn, 1500 + ord(name))
    hop = int(np.prod(cfg.ratios))
    assert mine['out0'].shape == (2, cfg.dimension, -(-Tn // hop))
    if name == 'A' and Tn == 4800:
        assert Tn // 2 >= ops.RESBLOCK_TMIN
    if name == 'C':
        assert O.extra_padding_for_conv1d(Tn, 6, 3, 3) > 0
    assert fused_calls == {'fused': fused, 'blocks': sum(L[0] == 'res' for L in cfg.enc_plan + cfg.dec_plan)}
    check(mine, p, stack_fn(cfg), x0, gy0, f'arch {name} T {Tn}', key=(name, Tn))
    # the caller's output grad is the caller's: no backward writes into it (the identity-shortcut
    # tail used to hand it to the head conv's accumulating bwd-data)
    assert torch.equal(gy, keep)


def test_stack_fused_blocks_off_gives_the_same_within_the_rule(monkeypatch, fused_calls):
    """A at T = 4800 with ENCX_RESBLOCK=0, a fresh construction: no fused block, same bounds."""
    monkeypatch.setenv('ENCX_RESBLOCK', '0')
    cfg, p, x0, gy0, mine, _, _ = stack_run('A', 4800, 1500 + ord('A'))
    assert fused_calls == {'fused': 0, 'blocks': 12}
    check(mine, p, stack_fn(cfg), x0, gy0, 'arch A T 4800, fused blocks off', key=('A', 4800))


# --------------------------------------------------------------------------- single blocks
BLOCKS = [
    # dim, T, compress, K, dilation, true_skip, causal
    (24, 97, 2, 3, 4, False, True),
    (12, 5, 4, 5, 2, True, True),     # T <= the reflect pad of 8: pad1d's zero extension
    (32, 300, 2, 3, 2, False, False),
]


def build_block(dim, comp, K, d, skip, causal, seed):
    from encx.modules.seanet import SEANetResnetBlock
    shapes = {}
    O._conv_shapes(shapes, 'm.block.1', dim, dim // comp, K, 'weight_norm')
    O._conv_shapes(shapes, 'm.block.3', dim // comp, dim, 1, 'weight_norm')
    if not skip:
        O._conv_shapes(shapes, 'm.shortcut', dim, dim, 1, 'weight_norm')
    p = {k: T(v) for k, v in synth_state(shapes, seed).items()}
    blk = SEANetResnetBlock(dim, kernel_sizes=[K, 1], dilations=[d, 1], norm='weight_norm', causal=causal,
                            compress=comp, true_skip=skip)
    blk.load_state_dict({k[2:]: v for k, v in p.items()})
    return blk.to(DEV), p


@pytest.mark.parametrize('bi', range(len(BLOCKS)))
def test_resblock_vs_oracle(bi):
    dim, Tn, comp, K, d, skip, causal = BLOCKS[bi]
    blk, p = build_block(dim, comp, K, d, skip, causal, 1600 + bi)
    assert not blk._fuse
    x0 = T(synth_wave((2, dim, Tn), 1610 + bi, amp=1.0))
    gy0 = T(synth_wave((2, dim, Tn), 1620 + bi, amp=1.0))
    x = x0.to(DEV).requires_grad_(True)
    y = blk(x)
    gy = gy0.to(DEV)
    y.backward(gy)
    mine = {'out0': y.detach(), 'dx': x.grad, **{'m.' + k: v.grad for k, v in blk.named_parameters()}}
    check(mine, p, lambda xx, pp: [O.resblock(xx, pp, 'm', dim, K, comp, causal=causal, dilation=d, true_skip=skip)],
          x0, gy0, f'block dim {dim} T {Tn} c{comp} K{K} d{d} skip {skip} causal {causal}')
    assert torch.equal(gy, gy0.to(DEV))


def test_identity_block_leaves_the_output_grad_alone():
    """blk(x).backward(gy) with the identity shortcut: gy is the caller's tensor and y.grad (kept by
    retain_grad) is autograd's; the skip gradient must reach x without either being written."""
    dim, Tn, comp, K, d, skip, causal = 12, 50, 4, 5, 2, True, True
    blk, _ = build_block(dim, comp, K, d, skip, causal, 1630)
    x = T(synth_wave((2, dim, Tn), 1631, amp=1.0)).to(DEV).requires_grad_(True)
    gy = T(synth_wave((2, dim, Tn), 1632, amp=1.0)).to(DEV)
    keep = gy.clone()
    seen = []
    y = blk(x)
    y.retain_grad()
    y.register_hook(lambda g: seen.append(g))  # the tensor autograd hands on, not a copy of it
    y.backward(gy)
    torch.cuda.synchronize()
    assert torch.equal(gy, keep)
    assert torch.equal(y.grad, keep)
    assert len(seen) == 1 and torch.equal(seen[0], keep)
    # and the skip path did arrive: dx = gy + (the conv branch's grad), which is not gy
    assert not torch.equal(x.grad, keep)
    # a block inside a graph: the grad of the tensor between two blocks, seen by a hook
    x2 = x.detach().requires_grad_(True)
    mid = blk(x2)
    mid.retain_grad()
    out = blk(mid)
    out.backward(gy)
    x3 = x.detach().requires_grad_(True)
    mid3 = blk(x3)
    g_mid, = torch.autograd.grad(blk(mid3), mid3, gy)
    assert torch.equal(mid.grad, g_mid) and torch.equal(gy, keep)


# --------------------------------------------------------------------------- dilated bwd-data, accumulate
@pytest.mark.parametrize('li', range(len(DILATED_LAYERS)))
def test_dilated_bwd_data_accumulates_vs_oracle(li):
    """encx_conv1d_bwd_data_dilated(accumulate=1) through the ABI, the 'join' of a conv-shortcut
    block whose head conv is dilated: dx pre-filled with seeded values must come back as fp64
    (dx0 + dgrad), under the bound test_dilated_conv1d_vs_oracle holds dx to."""
    from encx import ops
    cin, cout, K, s, d, causal, pad, pre_elu, Tin = DILATED_LAYERS[li]
    v0, g0, b0 = _case_params(700 + li, 'conv', cin, cout, K)
    x0 = synth_wave((3, cin, Tin), 720 + li, amp=1.0)
    pl, pr, e, tout = ops.conv_geometry(Tin, K, s, d, causal, pad)
    gy0 = synth_wave((3, cout, tout), 740 + li, amp=1.0)
    dx0 = synth_wave((3, cin, Tin), 760 + li, amp=1.0)
    x, gy, dx = G(x0), G(gy0), G(dx0)
    with torch.no_grad():
        wf, _ = ops._weight_prep(v0.detach(), g0.detach(), K, s, True, False)
        ws = ops._f32(3 * cin * (pl + pr) + 1, x)
        ops.call('encx_conv1d_bwd_data_dilated', ops.ptr(gy), ops.ptr(wf), ops.ptr(x), ops.ptr(dx), ops.ptr(ws),
                 3, cin, Tin, cout, tout, K, s, d, pl, pr, e, ops.PAD[pad], ops.ACT['elu' if pre_elu else None], 1,
                 ops.stream())
    torch.cuda.synchronize()
    p = {'m.conv.conv.weight_v': v0.detach().cpu().double(), 'm.conv.conv.weight_g': g0.detach().cpu().double(),
         'm.conv.conv.bias': b0.detach().cpu().double()}
    xc = T(x0).double().requires_grad_(True)
    yc = O.sconv1d(F.elu(xc) if pre_elu else xc, p, 'm', K, s, d, causal, pad)
    assert yc.shape == gy0.shape
    yc.backward(T(gy0).double())
    want = T(dx0).double() + xc.grad
    close(dx, want, 1e-4, 1e-5 * float(want.abs().max()), f'{cin}->{cout} K{K} s{s} d{d} {pad} dx0 + dx')


# --------------------------------------------------------------------------- ratios through _get_model
def test_ratios_through_the_public_constructor():
    from encx.model import EncodecModel
    d = load('g1_eval24k.npz')
    cfg = O.Config(ratios=(6, 4, 2), target_bandwidths=(6.0,), audio_normalize=False)
    assert cfg.n_q == 1 and cfg.frame_rate == 500
    p = model_state(cfg, 1701)
    cbs = codebooks_from_stats(d['stats'], 77, 1, cfg.n_q)
    m = load_model(EncodecModel._get_model([6.0], 24000, 1, causal=True, model_norm='weight_norm',
                                           ratios=[6, 4, 2]), p, cbs)
    assert m.quantizer.n_q == 1 and int(m.encoder.hop_length) == 48
    m.set_target_bandwidth(6.0)
    x = T(synth_wave((1, 1, 40 * 48), 1702))
    frames = check_segments(m, x, p, cbs, cfg, 6.0)
    assert frames[0][0].shape == (1, 1, 40)


# --------------------------------------------------------------------------- arch A streamed
FRAMES = 27
SCHEDULE = (7, 1, 1, 3, 8, 2, 5)
BW = 80.0  # 4000 frames/s x 10 bits: 40 kbps per codebook, n_q 2


@pytest.fixture(scope='module')
def arch_a():
    """Arch A as an EncodecModel (dimension 128: the g1 codebooks serve; no normalisation, no
    segments), three clips of 27 frames (162 samples), the oracle's latent / codes / wave of clip 0
    and each clip streamed alone, computed once and left unchanged."""
    import encx.modules as M
    from encx.model import EncodecModel
    from encx.quantization import ResidualVectorQuantizer
    cfg, seed = arch_cfg('A')
    p = model_state(cfg, seed)
    cbs = codebooks_from_stats(load('g1_eval24k.npz')['stats'], 77, 2, cfg.n_q)
    enc, dec = arch_modules('A', M)
    m = EncodecModel(enc, dec, ResidualVectorQuantizer(dimension=128, n_q=cfg.n_q, bins=1024), [BW], 24000, 1,
                     normalize=False, segment=None)
    m = load_model(m, p, cbs)
    m.set_target_bandwidth(BW)
    ns = type('Ctx', (), {})()
    ns.m, ns.cfg, ns.p, ns.cbs = m, cfg, p, cbs
    ns.hop = int(m.encoder.hop_length)
    assert ns.hop == 6 and m.frame_rate == cfg.frame_rate == 4000
    ns.n_q = O.rvq_num_quantizers(BW, cfg.frame_rate, n_q_max=cfg.n_q)
    assert ns.n_q == 2
    ns.x = T(synth_wave((3, 1, FRAMES * ns.hop), 1801))
    with torch.no_grad():
        (codes_o, _, emb_o), = O.encodec_encode_eval(ns.x[:1], p, cbs, cfg, BW)
        ns.codes_o = torch.as_tensor(codes_o).long()
        ns.emb_o = emb_o
        ns.y_o = O.encodec_decode_eval([(codes_o, None)], p, cbs, cfg, ns.x.shape[-1])
        p64 = {k: v.double() for k, v in p.items()}
        ns.emb_64 = O.run_plan(ns.x[:1].double(), p64, cfg.enc_plan)
        q = O.rvq_decode(ns.codes_o.transpose(0, 1), [{'embed': cb['embed'].double()} for cb in cbs])
        ns.y_64 = O.run_plan(q, p64, cfg.dec_plan)
    ns.solo = [run(m, ns.x[b:b + 1], SCHEDULE) for b in range(3)]
    return ns


def test_arch_a_streamed_against_the_oracle_and_the_offline_model(arch_a):
    ns = arch_a
    m, x = ns.m, ns.x[:1]
    emb, codes, _ = ns.solo[0]
    with torch.no_grad():
        emb_off = m.encoder(x.to(DEV))
    r64, r32, roff = rel(emb, ns.emb_64), rel(emb, ns.emb_o), rel(emb, emb_off)
    print(f'arch A latent: rel vs fp64 oracle {r64:.3e}, vs fp32 oracle {r32:.3e}, vs the offline encoder {roff:.3e}; '
          f'fp32 oracle vs fp64 {rel(ns.emb_o, ns.emb_64):.3e}')
    assert r64 < 1e-4 and roff < 1e-4, (r64, roff)
    embeds = [cb['embed'] for cb in ns.cbs[:ns.n_q]]
    mine = codes.transpose(0, 1).cpu()
    assert mine.shape == (ns.n_q, 1, FRAMES)
    for factor in (256, 32):
        want, cert = rvq_certified(emb, embeds, factor)
        print(f'certified at {factor}: {float(cert.float().mean()):.3f} of the codes')
        assert cert.any()
        assert torch.equal(mine[cert], want[cert]), (factor, int((mine[cert] != want[cert]).sum()))
    y, _ = stream_decode(m, ns.codes_o, SCHEDULE)
    with torch.no_grad():
        y_off = m.decode([(ns.codes_o.to(DEV), None)])
    r64, r32, roff = rel(y, ns.y_64), rel(y, ns.y_o), rel(y, y_off)
    print(f'arch A wave: rel vs fp64 oracle {r64:.3e}, vs fp32 oracle {r32:.3e}, vs the offline decoder {roff:.3e}; '
          f'fp32 oracle vs fp64 {rel(ns.y_o, ns.y_64):.3e}')
    assert y.shape == ns.y_o.shape == (1, 1, FRAMES * ns.hop)
    assert r64 < 1e-3 and roff < 1e-3, (r64, roff)


def test_arch_a_schedule_invariance_bit_for_bit(arch_a):
    """7 + 20 x 1 (one-frame chunks: the roll moves 3 columns under the 8-column history of the
    d = 4 blocks at 3 columns per frame, 6 under 8 at 6 per frame), 8 + 8 + 8 + 3 and all 27 at once."""
    m, x = arch_a.m, arch_a.x[:1]
    a = run(m, x, (7,) + (1,) * 20)
    b = run(m, x, (8, 8, 8, 3))
    c = run(m, x, (27,), max_frames=27)
    for name, i in (('latent', 0), ('codes', 1), ('wave', 2)):
        assert torch.equal(a[i], b[i]), name
        assert torch.equal(a[i], c[i]), name
        assert torch.equal(a[i], arch_a.solo[0][i]), name


def test_arch_a_batch_independence(arch_a):
    both = run(arch_a.m, arch_a.x, SCHEDULE)
    assert not torch.equal(arch_a.solo[0][0], arch_a.solo[1][0])
    for b in range(3):
        for name, i in (('latent', 0), ('codes', 1), ('wave', 2)):
            assert torch.equal(both[i][b:b + 1], arch_a.solo[b][i]), (b, name)


def test_arch_a_graph_equals_eager(arch_a):
    eager = run(arch_a.m, arch_a.x[:1], SCHEDULE, graphs=False)
    assert same(eager, arch_a.solo[0])  # solo ran with graphs


def test_arch_a_slots_equal_each_stream_alone(arch_a):
    """frames [7,0,7] -> [1,7,2] -> [3,1,0]: a late join beside a one-frame chunk, ragged counts, a
    slot that sits out; each slot equals its clip streamed alone (the num_layers = 1 LSTM under the
    slot table)."""
    from encx.streaming import StreamEncoder, StreamDecoder
    ns = arch_a
    m, hop = ns.m, ns.hop
    enc = StreamEncoder(m, 3)
    dec = StreamDecoder(m, 3, enc.n_q)
    off, got = [0, 0, 0], [[] for _ in range(3)]
    for frames in ([7, 0, 7], [1, 7, 2], [3, 1, 0]):
        n = max(frames)
        x = torch.zeros(3, 1, n * hop)
        for b, f in enumerate(frames):
            x[b, :, :f * hop] = ns.x[b, :, off[b] * hop:(off[b] + f) * hop]
        codes, emb = enc.encode_slots(x.to(DEV), frames, return_latent=True)
        y = dec.decode_slots(codes, frames)
        assert codes.shape == (3, enc.n_q, n) and emb.shape == (3, 128, n) and y.shape == (3, 1, n * hop)
        for b, f in enumerate(frames):
            assert not emb[b, :, f:].any() and not codes[b, :, f:].any() and not y[b, :, f * hop:].any(), (b, frames)
            if f:
                got[b].append((emb[b:b + 1, :, :f], codes[b:b + 1, :, :f], y[b:b + 1, :, :f * hop]))
                off[b] += f
    assert off == [11, 8, 9]
    for b in range(3):
        for i, (name, rate) in enumerate((('latent', 1), ('codes', 1), ('wave', hop))):
            mine = torch.cat([g[i] for g in got[b]], 2)
            assert torch.equal(mine, ns.solo[b][i][:, :, :off[b] * rate]), (b, name)
