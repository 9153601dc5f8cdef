"""The RVQ kernels (csrc/rvq.hip, csrc/stream_rvq.hip) at codebook shapes other than 1024 x 128.

ResidualVectorQuantizer(dimension, n_q, bins) takes any latent width and codebook size; every other
RVQ test runs D = 128, Kc = 1024. Here: D from 5 to 256 (odd, D % 4 != 0, below and above a wave),
Kc from 1 to 2048 (ragged code tiles), N from 1 to 2400. References are fp64 on the CPU
(oracle.encodec_oracle and numpy); only the fused streaming quantizer is compared with the per-layer
kernels, bit for bit, as test_gpu_stream_nq does.

Two rules.

Certification. A frame's code is settled when its fp64 top-2 distance gap exceeds
factor * eps32 * (|x|^2 max + |e|^2 max) (fixtures.certified) with factor = 2 D + 8: twice the
worst-case rounding of a D-term fp32 dot product (the existing 256 = 2 * 128) plus the three extra
roundings of (xx - 2 dot) + ee. On certified frames the code must EQUAL the fp64 argmin; on every
other frame the fp64 distance of the GPU's pick may exceed the fp64 minimum by at most that margin.
Each case asserts, before the GPU is consulted, that at least 0.99 of its frames are certified.

Accuracy. steputil.check_grads: per tensor, max|mine - ref64| / max|ref64| at most
max(4 x the same error of the oracle run in plain fp32, 1e-6)."""
import numpy as np
import pytest
import torch

from oracle import encodec_oracle as O
from fixtures import T, certified, rvq_certified
from steputil import check_grads, code_impose, check_code_ties

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS32 = float(np.finfo(np.float32).eps)


def G(a):
    return (a if torch.is_tensor(a) else T(a)).to(DEV)


def gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def factor(D):
    return 2 * D + 8


def rows_of(x):
    """[B, D, T] -> [B*T, D] ('b d n -> (b n) d')."""
    x = np.asarray(x)
    return x.transpose(0, 2, 1).reshape(-1, x.shape[1])


def dist64(rows, E, exact=False):
    """fp64 squared distances [N, Kc]: the expanded form, or (exact) the sum of squared differences,
    which is 0 for equal rows and equal for equal codes."""
    r, e = np.asarray(rows, np.float64), np.asarray(E, np.float64)
    if exact:
        return np.stack([((r - ek[None]) ** 2).sum(1) for ek in e], 1)
    return (r ** 2).sum(1)[:, None] - 2 * r @ e.T + (e ** 2).sum(1)[None]


def certify(rows, E, scale=1.0):
    """-> (dist [N, Kc], cert [N] bool, margin): the certification rule of the module docstring.
    scale 2 for the direct form, whose terms are bounded by |x - e|^2 <= 2 (|x|^2 + |e|^2)."""
    d = dist64(rows, E)
    D = np.asarray(rows).shape[1]
    srt = np.sort(d, 1)
    gap = srt[:, 1] - srt[:, 0] if d.shape[1] > 1 else np.full(d.shape[0], np.inf)
    x2 = float((np.asarray(rows, np.float64) ** 2).sum(1).max())
    e2 = float((np.asarray(E, np.float64) ** 2).sum(1).max())
    f = scale * factor(D)
    return d, certified(gap, x2, e2, f), f * EPS32 * (x2 + e2)


def check_codes(idx, d, cert, margin, what):
    """Equal to the fp64 argmin where certified; within the margin of the fp64 minimum elsewhere."""
    idx = np.asarray(idx).reshape(-1)
    assert idx.shape[0] == d.shape[0] and idx.min() >= 0 and idx.max() < d.shape[1], what
    ref = d.argmin(1)
    assert (idx[cert] == ref[cert]).all(), (what, int((idx[cert] != ref[cert]).sum()), 'certified codes differ')
    excess = d[np.arange(len(idx)), idx] - d.min(1)
    assert (excess[~cert] <= margin).all(), (what, float(excess[~cert].max()), margin)
    return float(excess.max() / margin)


def accuracy(mine, r64, r32, what):
    table = check_grads({k: torch.as_tensor(v) for k, v in mine.items()}, r64, r32, what)
    return max(r[1] / r[3] for r in table)


# ---------------------------------------------------------------- a. nearest code, MFMA form
ARGMIN = [  # (B, D, T, Kc)
    (2, 64, 75, 1024),
    (3, 40, 50, 100),     # D < 64; quad staging
    (1, 256, 130, 2048),  # the largest D, 130 KB of LDS; Kc above 1024
    (2, 6, 97, 1024), (2, 10, 97, 1001),  # D % 4 != 0: scalar staging
    (3, 5, 33, 7), (2, 7, 100, 65), (2, 129, 40, 64),  # odd D; Kc one past a code tile
    (1, 8, 63, 4),
    (2, 96, 65, 63),      # N one past a frame tile; a tile that straddles two batch items
    (1, 128, 1, 1024),    # N = 1
    (1, 128, 64, 1),      # a single code: every index 0
]


def argmin_inputs(i):
    B, D, Tn, Kc = ARGMIN[i]
    r = gen(2000 + i)
    return r.standard_normal((B, D, Tn)).astype(np.float32), r.standard_normal((Kc, D)).astype(np.float32)


@pytest.mark.parametrize('i', range(len(ARGMIN)), ids=['x'.join(map(str, s)) for s in ARGMIN])
def test_argmin_vs_fp64(i):
    from encx import ops
    x, E = argmin_inputs(i)
    d, cert, margin = certify(rows_of(x), E)
    assert cert.mean() >= 0.99, cert.mean()
    ref = O.codebook_quantize(T(rows_of(x)).double(), T(E).double()).numpy()
    assert (ref[cert] == d.argmin(1)[cert]).all()  # the oracle's own quantize, in fp64
    idx = ops.rvq_argmin(G(x), G(E)).cpu().numpy()
    worst = check_codes(idx, d, cert, margin, ARGMIN[i])
    if ARGMIN[i][3] == 1:
        assert not idx.any()
    print(f'argmin {ARGMIN[i]}: certified {cert.mean():.4f}, worst excess / margin {worst:.3f}')


@pytest.mark.parametrize('D, Kc', [(128, 1024), (40, 100), (7, 65), (5, 7)])
def test_argmin_of_a_codebook_row_is_that_row(D, Kc):
    """x = rows of a codebook of large norm: the fp32 distance (xx - 2 x.e) + ee of the exact row is
    rounding noise on either side of zero (ord_key's negative branch), every other far above it."""
    from encx import ops
    r = gen(2100 + D)
    E = (30 * r.standard_normal((Kc, D))).astype(np.float32)
    pick = r.integers(0, Kc, size=(2, 75))
    pick[0, :min(Kc, 75)] = np.arange(Kc)[:75]  # every code of a small codebook at least once
    x = np.ascontiguousarray(E[pick].transpose(0, 2, 1))  # [2, D, 75]
    d = dist64(rows_of(x), E, exact=True)
    assert (np.sort(d, 1)[:, 1] > 1.0).all() and (d.min(1) == 0).all()  # distinct rows
    for direct in (False, True):
        idx = ops.rvq_argmin(G(x), G(E), direct=direct).cpu().numpy()
        assert (idx == pick.reshape(-1)).all(), (direct, int((idx != pick.reshape(-1)).sum()))


TIES = [  # (Kc, lower, upper): where the duplicated row sits
    (64, 3, 20),     # inside one 32-column MFMA tile
    (64, 3, 40),     # across the two column waves of a workgroup
    (100, 10, 99),   # across workgroups, the second a ragged last tile
    (300, 10, 299),  # across the direct form's 256-code blocks
]


@pytest.mark.parametrize('direct', [False, True], ids=['mfma', 'direct'])
@pytest.mark.parametrize('Kc, lo, hi', TIES)
@pytest.mark.parametrize('D', [40, 7])
def test_argmin_ties_go_to_the_lower_index(D, Kc, lo, hi, direct):
    from encx import ops
    r = gen(2200 + Kc + hi)
    E = r.standard_normal((Kc, D)).astype(np.float32)
    E[hi] = E[lo]
    x = (E[lo][None, :, None] + 0.01 * r.standard_normal((1, D, 70))).astype(np.float32)
    d = dist64(rows_of(x), E, exact=True)
    srt = np.sort(d, 1)
    assert (d.argmin(1) == lo).all() and (srt[:, 1] == srt[:, 0]).all()
    assert (srt[:, 2] - srt[:, 0] > 1e-2).all()  # no third code near
    idx = ops.rvq_argmin(G(x), G(E), direct=direct).cpu().numpy()
    assert (idx == lo).all(), np.unique(idx)


# ---------------------------------------------------------------- b. direct form, one kmeans step
KMEANS = [  # (N, D, Kc)
    (600, 40, 300),    # two code blocks
    (33, 128, 1024),   # four code blocks; N one past the 32-row tile; most clusters empty
    (2400, 256, 64),   # D above 141: the chunked kernel
    (300, 5, 16),
]


def kmeans_inputs(i):
    """Well-separated samples: seeded start means, each sample a start mean plus small noise."""
    N, D, Kc = KMEANS[i]
    r = gen(2300 + i)
    means = r.standard_normal((Kc, D)).astype(np.float32)
    samples = (means[r.integers(0, Kc, size=N)] + 0.05 * r.standard_normal((N, D))).astype(np.float32)
    return samples, means


def kmeans_step_gpu(samples, means):
    from encx._lib import call, ptr, stream, lib
    N, D = samples.shape
    Kc = means.shape[0]
    s, m = G(samples), G(means).contiguous()
    bins = torch.zeros(Kc, dtype=torch.int64, device=DEV)
    idx = torch.empty(N, dtype=torch.int64, device=DEV)
    keys = torch.empty(N, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.encx_rvq_bucket_workspace(N, D, Kc) // 4 + 1, device=DEV)
    call('encx_kmeans_step', ptr(s), ptr(m), ptr(bins), ptr(idx), ptr(keys), ptr(ws), N, D, Kc, stream())
    return m.cpu(), bins.cpu(), idx.cpu()


@pytest.mark.parametrize('i', range(len(KMEANS)), ids=['x'.join(map(str, s)) for s in KMEANS])
def test_kmeans_step_vs_fp64(i):
    samples, means = kmeans_inputs(i)
    N, D, Kc = KMEANS[i]
    s64, s32 = T(samples).double(), T(samples)
    start = T(means)
    worst = 0.0
    for step in range(4):  # one step from the given means, then three more, each from the fp64 means
        d, cert, margin = certify(samples, start.numpy(), scale=2.0)
        assert cert.all(), (step, cert.mean())
        m64, b64 = O.kmeans(s64, Kc, 1, None, means=start.double())
        m32, _ = O.kmeans(s32, Kc, 1, None, means=start)
        m, bins, idx = kmeans_step_gpu(samples, start)
        assert (idx.numpy() == d.argmin(1)).all(), step
        assert torch.equal(bins, b64), step
        empty = b64 == 0
        assert torch.equal(m[empty], start[empty]), step  # bit-unchanged
        assert step or i != 1 or int(empty.sum()) > Kc // 2
        worst = max(worst, accuracy({'means': m}, {'means': m64}, {'means': m32}, f'kmeans {KMEANS[i]} step {step}'))
        start = m64.float()
    print(f'kmeans {KMEANS[i]}: worst err / bound {worst:.3f}')


def test_sample_rows_with_replacement():
    """num > N (core_vq.py:74-75, randint): every row is a sample row, and the seed matters."""
    from encx._lib import call, ptr, stream
    s = G(gen(2400).standard_normal((33, 6)).astype(np.float32))
    outs = []
    for seed in (12345, 12346):
        out = torch.full((100, 6), float('nan'), device=DEV)
        call('encx_sample_rows', ptr(s), ptr(out), 33, 6, 100, seed, stream())
        assert bool((out[:, None, :] == s[None]).all(-1).any(1).all())
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])


def test_bdt_to_nd():
    from encx import ops
    x = G(gen(2401).standard_normal((3, 40, 50)).astype(np.float32))
    assert torch.equal(ops.rvq_to_rows(x), x.permute(0, 2, 1).reshape(-1, 40))


# ---------------------------------------------------------------- c. EMA update
EMA = [  # (B, D, T, Kc)
    (2, 40, 75, 100), (2, 64, 75, 1024), (2, 96, 75, 1001), (2, 100, 75, 300), (2, 160, 75, 1024),
    (1, 256, 130, 2048), (3, 5, 33, 7),
    (2, 128, 15, 1024),   # N = 30: one k-slab, nearly every code empty
    (8, 128, 300, 1024),  # N = 2400: several slabs
]


def ema_assignments(r, N, Kc):
    half = max(1, Kc // 2)
    return {'uniform': r.integers(0, Kc, size=N),
            'one code': np.full(N, Kc - 1),
            'skewed': np.minimum((half * r.random(N) ** 3).astype(np.int64), half - 1)}  # codes >= Kc/2 empty


@pytest.mark.parametrize('i', range(len(EMA)), ids=['x'.join(map(str, s)) for s in EMA])
def test_ema_vs_fp64(i):
    from encx import ops
    from encx._lib import call, ptr, stream, lib
    B, D, Tn, Kc = EMA[i]
    N = B * Tn
    r = gen(2500 + i)
    x = r.standard_normal((B, D, Tn)).astype(np.float32)
    cb = {'inited': torch.ones(1), 'cluster_size': T(r.uniform(0.5, 4.0, size=Kc).astype(np.float32)),
          'embed_avg': T(r.standard_normal((Kc, D)).astype(np.float32)),
          'embed': T(r.standard_normal((Kc, D)).astype(np.float32))}
    xr = T(rows_of(x))
    xg = G(x)
    ws = ops._ws(lib.encx_rvq_bucket_workspace(N, D, Kc), xg)
    worst = 0.0
    for name, ind in ema_assignments(r, N, Kc).items():
        ind = T(ind.astype(np.int64))
        if name == 'skewed' and Kc > 1:
            assert int(ind.max()) < max(1, Kc // 2)
        for decay in (0.99, 0.8):
            what = f'ema {EMA[i]} {name} decay {decay}'
            r64 = O.codebook_ema(xr.double(), ind, {k: v.double() for k, v in cb.items()}, decay, 1e-5)
            r32 = O.codebook_ema(xr, ind, cb, decay, 1e-5)
            mine = {k: G(cb[k]).clone() for k in ('cluster_size', 'embed_avg', 'embed')}
            ig = G(ind)
            call('encx_rvq_ema', ptr(xg), ptr(ig), ptr(mine['cluster_size']), ptr(mine['embed_avg']),
                 ptr(mine['embed']), ptr(ws), B, D, Tn, Kc, decay, 1e-5, stream())
            keys = ('cluster_size', 'embed_avg', 'embed')
            worst = max(worst, accuracy(mine, {k: r64[k] for k in keys}, {k: r32[k] for k in keys}, what))
            # the two halves (the data-parallel sync's path) from the same starting buffers
            two = {k: G(cb[k]).clone() for k in keys}
            sums = torch.full((Kc, D + 1), float('nan'), device=DEV)
            call('encx_rvq_code_sums', ptr(xg), ptr(ig), ptr(sums), ptr(ws), B, D, Tn, Kc, stream())
            assert torch.equal(sums[:, D].cpu(), torch.bincount(ind, minlength=Kc).float()), what
            call('encx_rvq_ema_from_sums', ptr(sums), ptr(two['cluster_size']), ptr(two['embed_avg']),
                 ptr(two['embed']), D, Kc, decay, 1e-5, stream())
            for k in keys:
                assert torch.equal(two[k], mine[k]), (what, k)
    print(f'ema {EMA[i]}: worst err / bound {worst:.3f}')


# ---------------------------------------------------------------- d. the train function, the eval pair
class _CB:
    def __init__(self, d):
        for k, v in d.items():
            setattr(self, k, v)
        self.training = True
        self.decay, self.epsilon = 0.99, 1e-5

    def init_embed_(self, x):
        pass


TRAIN = [  # (B, D, T, Kc), n_q 3
    (2, 40, 75, 100), (3, 96, 50, 1001), (2, 5, 33, 7),
    (4, 256, 300, 64),  # 307 200 elements: rvq_apply's grid-stride loop, the 1024-part commit reduce
]
N_Q = 3


def train_inputs(i):
    B, D, Tn, Kc = TRAIN[i]
    r = gen(2600 + i)
    emb = r.standard_normal((B, D, Tn)).astype(np.float32)
    gq = r.standard_normal((B, D, Tn)).astype(np.float32)
    cbs = []
    for _ in range(N_Q):
        cbs.append({'inited': torch.ones(1), 'embed': T(r.standard_normal((Kc, D)).astype(np.float32)),
                    'cluster_size': T(r.uniform(0.5, 4.0, size=Kc).astype(np.float32)),
                    'embed_avg': T(r.standard_normal((Kc, D)).astype(np.float32))})
    return emb, gq, cbs


def audit_chain(emb, embeds, codes, what):
    """Every layer's codes along the residual chain the GPU's own codes define (fp64): equal to the
    fp64 argmin where certified, within the margin elsewhere. -> worst excess / margin."""
    res = np.asarray(rows_of(emb), np.float64)
    worst = 0.0
    for k, E in enumerate(embeds):
        E = np.asarray(E, np.float64)
        d, cert, margin = certify(res, E)
        idx = np.asarray(codes[k]).reshape(-1)
        worst = max(worst, check_codes(idx, d, cert, margin, (what, 'layer', k)))
        res = res - E[idx]
    return worst


def oracle_train(emb, gq, cbs, codes, dtype, log=False):
    """O.rvq_train with our codes imposed -> (tensors by name, audit log)."""
    x = T(emb).to(dtype).requires_grad_(True)
    seg = [(codes, T(emb))]
    with code_impose(seg) as audit:
        q, c, pen, new = O.rvq_train(x, [{k: v.to(dtype) for k, v in cb.items()} for cb in cbs], len(cbs))
    torch.autograd.backward([q, pen], [T(gq).to(dtype), torch.ones((), dtype=pen.dtype)])
    out = {'quantized': q.detach(), 'penalty': pen.detach().reshape(1), 'demb': x.grad}
    for i, cb in enumerate(new):
        for k in ('cluster_size', 'embed_avg', 'embed'):
            out[f'{k}{i}'] = cb[k]
    return out, (audit if log else None)


def run_train_case(emb, gq, cbs, what, fn=None):
    """RVQTrainFn (or fn: a module's forward) from the given buffers against O.rvq_train."""
    from encx import ops
    n_q = len(cbs)
    holders = [_CB({k: G(v).clone().contiguous() for k, v in cb.items()}) for cb in cbs]
    x = G(emb).requires_grad_(True)
    q, codes, pen = fn(x) if fn else ops.RVQTrainFn.apply(x, holders, 0.99, 1e-5)
    assert codes.shape == (n_q,) + (emb.shape[0], emb.shape[2]) and codes.dtype == torch.int64
    torch.autograd.backward([q, pen], [G(gq), torch.ones((), device=DEV)])
    return x, q, codes, pen, holders


def check_train_case(emb, gq, cbs, x, q, codes, pen, bufs, what):
    n_q = len(cbs)
    codes = codes.cpu()
    r64, log = oracle_train(emb, gq, cbs, codes, torch.float64, log=True)
    r32, _ = oracle_train(emb, gq, cbs, codes, torch.float32)
    n_imp = check_code_ties(log, [(codes, T(emb))], n_q, what)
    mine = {'quantized': q.detach(), 'penalty': pen.detach().reshape(1), 'demb': x.grad}
    for i in range(n_q):
        for k in ('cluster_size', 'embed_avg', 'embed'):
            mine[f'{k}{i}'] = bufs[i][k]
    worst = accuracy(mine, r64, r32, what)
    print(f'{what}: worst err / bound {worst:.3f}, {n_imp} near-tie codes imposed')
    return worst


@pytest.mark.parametrize('i', range(len(TRAIN)), ids=['x'.join(map(str, s)) for s in TRAIN])
def test_train_fn_vs_fp64(i):
    emb, gq, cbs = train_inputs(i)
    what = f'rvq train {TRAIN[i]}'
    x, q, codes, pen, holders = run_train_case(emb, gq, cbs, what)
    audit_chain_train(emb, cbs, codes.cpu(), what)
    bufs = [{k: getattr(h, k) for k in ('cluster_size', 'embed_avg', 'embed')} for h in holders]
    check_train_case(emb, gq, cbs, x, q, codes, pen, bufs, what)


def audit_chain_train(emb, cbs, codes, what):
    """The train chain subtracts x + (q - x) (core_vq.py:309), q up to one rounding: the eval chain's
    audit holds with that rounding far inside the margin."""
    return audit_chain(emb, [cb['embed'].numpy() for cb in cbs], codes.numpy(), what)


@pytest.mark.parametrize('i', range(len(TRAIN)), ids=['x'.join(map(str, s)) for s in TRAIN])
def test_encode_decode_vs_fp64(i):
    from encx import ops
    emb, _, cbs = train_inputs(i)
    B, D, Tn, Kc = TRAIN[i]
    embeds = [cb['embed'] for cb in cbs]
    ref, cert = rvq_certified(T(emb), embeds, factor(D))
    assert float(cert[-1].float().mean()) >= 0.99, cert.float().mean((1, 2))
    codes = ops.rvq_encode(G(emb), [G(e) for e in embeds]).cpu()
    assert codes.shape == (N_Q, B, Tn)
    assert torch.equal(codes[cert], ref[cert])
    worst = audit_chain(emb, [e.numpy() for e in embeds], codes.numpy(), f'rvq encode {TRAIN[i]}')
    # decode, every layer count (layers 2+ accumulate)
    for k in range(1, N_Q + 1):
        out = ops.rvq_decode(G(codes[:k]).contiguous(), [G(e) for e in embeds[:k]])
        r64 = O.rvq_decode(codes[:k], [{'embed': e.double()} for e in embeds[:k]])
        r32 = O.rvq_decode(codes[:k], [{'embed': e} for e in embeds[:k]])
        accuracy({'decoded': out}, {'decoded': r64}, {'decoded': r32}, f'rvq decode {TRAIN[i]} {k} layers')
    print(f'rvq encode {TRAIN[i]}: certified {float(cert[-1].float().mean()):.4f} (all layers), '
          f'worst excess / margin {worst:.3f}')


@pytest.mark.parametrize('kw, n_q', [(dict(dimension=96, n_q=3, bins=100), 3), (dict(), 2)],
                         ids=['96x100', 'default'])
def test_module_kmeans_init_then_train_step(kw, n_q):
    """ResidualVectorQuantizer in train mode: the first forward runs the kmeans init of each layer
    (D = 256 by default: the chunked direct argmin), the second is a train step from known buffers."""
    from encx.quantization import ResidualVectorQuantizer
    torch.manual_seed(7)
    m = ResidualVectorQuantizer(**kw).to(DEV).train()
    D, bins = m.dimension, m.bins
    r = gen(2700 + D)
    emb = r.standard_normal((2, D, 75)).astype(np.float32)
    gq = r.standard_normal((2, D, 75)).astype(np.float32)
    q, codes, pen = m.vq(G(emb), n_q=n_q)
    layers = m.vq.layers[:n_q]
    keys = ('cluster_size', 'embed_avg', 'embed')
    for layer in layers:
        c = layer._codebook
        assert float(c.inited) == 1.0
        assert all(bool(torch.isfinite(getattr(c, k)).all()) for k in keys)
        assert abs(float(c.cluster_size.sum()) - 150.0) < 1e-2  # kmeans' bins (every sample in one cluster), one EMA
    assert int(codes.min()) >= 0 and int(codes.max()) < bins and bool(torch.isfinite(q).all())
    snap = [{'inited': torch.ones(1), **{k: getattr(layer._codebook, k).detach().cpu().clone() for k in keys}}
            for layer in layers]
    what = f'module {D} x {bins} second forward'
    emb2 = r.standard_normal((2, D, 75)).astype(np.float32)
    x, q, codes, pen, _ = run_train_case(emb2, gq, snap, what, fn=lambda x: m.vq(x, n_q=n_q))
    bufs = [{k: getattr(layer._codebook, k) for k in keys} for layer in layers]
    check_train_case(emb2, gq, snap, x, q, codes, pen, bufs, what)


# ---------------------------------------------------------------- e. the fused streaming quantizer
def tables(counts, nq):
    slots = torch.tensor([(c, 0) for c in counts], dtype=torch.int32, device=DEV)
    return slots, torch.tensor(list(nq), dtype=torch.int32, device=DEV)


def masked(codes, counts, nq):
    out = codes.clone()
    for b, (c, q) in enumerate(zip(counts, nq)):
        out[b, q:] = 0
        out[b, :, c:] = 0
    return out


FUSED = [  # (bins, D)
    (4, 8),        # the smallest: one valid code thread
    (100, 40),
    (1028, 64),    # bins / 4 = 257: a second round with one valid thread
    (2048, 256),   # the largest D; two full rounds
]


@pytest.mark.parametrize('n', [1, 7])
@pytest.mark.parametrize('bins, D', FUSED)
def test_fused_quantizer_equals_the_per_layer_kernels(bins, D, n):
    """test_gpu_stream_nq.test_fused_kernels_equal_the_per_layer_kernels at other codebook shapes: a
    strided NaN-poisoned window, ragged counts, a codebook count per slot, torch.equal."""
    from encx import ops
    K = B = 3
    r = gen(2800 + bins + n)
    embeds = [G((0.6 ** k * r.standard_normal((bins, D))).astype(np.float32)) for k in range(K)]
    books = ops.StreamRVQBooks(embeds)
    nq = [3, 2, 1]
    counts = [n, n - 1, 0] if n > 1 else [1, 1, 0]
    slots, nqt = tables(counts, nq)
    clean = G(r.standard_normal((B, D, n)).astype(np.float32))
    win = torch.full((B, D, n + 5), float('nan'), device=DEV)
    for b, c in enumerate(counts):
        win[b, :, 3:3 + c] = clean[b, :, :c]
    codes = ops.stream_rvq_encode_slots(win[:, :, 3:3 + n], books, slots, nqt)
    ref = ops.rvq_encode(clean, embeds).permute(1, 0, 2).contiguous()  # [B, K, n]
    want = masked(ref, counts, nq)
    assert codes.shape == (B, K, n) and codes.dtype == torch.int64
    assert torch.equal(codes, want), int((codes != want).sum())
    assert int(want.count_nonzero()) or bins == 4

    cin = want.clone()
    for b, (c, q) in enumerate(zip(counts, nq)):
        cin[b, q:] = 1 << 40
        cin[b, :, c:] = -(1 << 40)
    clamped = want.clone()
    cin[0, 0, 0], clamped[0, 0, 0] = bins + 7, bins - 1  # a read code outside the codebook: clamped
    out = torch.full((B, D, n + 5), float('nan'), device=DEV)
    ops.stream_rvq_decode_slots(cin, books, slots, nqt, out[:, :, 3:3 + n])
    assert bool(out[:, :, :3].isnan().all()) and bool(out[:, :, 3 + n:].isnan().all())
    got = out[:, :, 3:3 + n]
    for b in range(B):
        k = nq[b]
        q = ops.rvq_decode(clamped[:, :k].permute(1, 0, 2).contiguous(), embeds[:k])
        assert torch.equal(got[b, :, :counts[b]], q[b, :, :counts[b]]), (b, k)
        assert not got[b, :, counts[b]:].any(), b


SUPPORT = [  # (K, bins, D): both sides of every bound of the fused quantizer
    (1, 4, 8), (64, 4, 8), (65, 4, 8), (0, 4, 8),
    (1, 0, 8), (1, 2, 8), (1, 6, 8), (1, 8, 8), (1, 1001, 8), (1, 1 << 20, 8), (1, (1 << 20) + 4, 8),
    (1, 4, 0), (1, 4, 4), (1, 4, 12), (1, 4, 16), (1, 4, 40), (1, 4, 100), (1, 4, 256), (1, 4, 264),
    (3, 1028, 64), (3, 100, 40),
]


@pytest.mark.parametrize('K, bins, D', SUPPORT)
def test_stream_rvq_supports_is_what_the_entry_points_accept(K, bins, D):
    """A refusal happens on the host, before any launch (ENCX_EINVAL); an accepted call runs."""
    from encx import ops
    from encx._lib import lib, ptr, stream
    want = ops.stream_rvq_supports(K, bins, D)
    n = max(1, K * bins * D)
    E, ET, e = (torch.zeros(n, device=DEV) for _ in range(3))
    ee = torch.zeros(max(1, K * bins), device=DEV)
    rc = lib.encx_stream_rvq_prepare(ptr(e), 0, K, bins, D, ptr(E), ptr(ET), ptr(ee), stream())
    assert (rc == 0) == want, ('prepare', rc)
    x = torch.zeros(1, max(D, 1), 1, device=DEV)
    codes = torch.zeros(1, max(K, 1), 1, dtype=torch.int64, device=DEV)
    slots, nq = tables([1], [max(K, 1)])
    rc = lib.encx_stream_rvq_encode_slots(x.data_ptr(), *x.stride(), ptr(E), ptr(ET), ptr(ee), 1, K, bins, D, 1,
                                          ptr(slots), ptr(nq), codes.data_ptr(), *codes.stride(), stream())
    assert (rc == 0) == want, ('encode', rc)
    rc = lib.encx_stream_rvq_decode_slots(codes.data_ptr(), *codes.stride(), ptr(E), 1, K, bins, D, 1, ptr(slots),
                                          ptr(nq), x.data_ptr(), *x.stride(), stream())
    assert (rc == 0) == want, ('decode', rc)
    torch.cuda.synchronize()
    if want:
        ops.StreamRVQBooks([torch.zeros(bins, D, device=DEV)] * K)
    elif K > 0 and bins > 0 and D > 0:
        with pytest.raises(ValueError):
            ops.StreamRVQBooks([torch.zeros(bins, D, device=DEV)] * K)
