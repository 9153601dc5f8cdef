// NormConv2d forward (conv2d.h) on gfx950: the tiled kernel, its column-aligned register-pipelined
// form, the register-window form and the single-output-channel kernel; encx_conv2d_fwd picks one
// per layer. Also the one definition of the kernel family selection (encx_conv2d_select) that the
// backward passes read.
#include "common.h"
#include "conv2d.h"
#include "prof.h"

namespace {

struct C2Fwd {
    C2Geo g;
    const float* x;
    const float* wf;  // [(ci,kt)][kf][co]
    const float* bias;
    float* y;
    int act;
    int CK, NR, RL;
};

template <int BM, int BN, int WM, int WN, int KFC = 0>
__global__ __launch_bounds__(NT) void c2_fwd_kernel(C2Fwd a) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    extern __shared__ float smem[];
    const C2Geo g = a.g;
    const int CK = a.CK, NR = a.NR, RL = a.RL, KF = g.KF, S = g.sf;
    const int VC = g.Ci * g.KT, XR = NR * RL;
    float* Xs = smem;           // [CK][NR][RL]
    float* Ws = smem + CK * XR; // [CK][KF][BM]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / WN) * TM * 32, wn0 = (wave % WN) * TN * 32;
    const int h = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.z, n0 = blockIdx.x * BN, co0 = blockIdx.y * BM;
    const int Nall = g.T2 * g.Fo, nend = min(Nall, n0 + BN);
    const int tf = n0 / g.Fo, f0 = n0 - tf * g.Fo;
    const int nr = (nend - 1) / g.Fo - tf + 1;
    int boff[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn0 + j * 32 + l32;
        boff[j] = 0;
        if (n < nend) {
            const int tr = n / g.Fo, f = n - tr * g.Fo, rs = tr - tf;
            boff[j] = rs * RL + (f - (rs ? 0 : f0)) * S;
        }
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};
    const float* xb = a.x + (int64_t)b * g.Ci * g.T2 * g.Fi;
    // Staging without per-element division: a table of the window rows (global row
    // gr = vc*NR + rs -> source offset of column 0, first column position or "invalid"), built
    // once; each thread walks its items (row r, column w) by a fixed step of NT; the weight
    // items keep their column (NT is a multiple of BM) and step the (kf, cl) row.
    int2* rtab = (int2*)(Ws + KF * CK * BM);  // {source offset of column 0, first position}
    for (int gr = tid; gr < VC * NR; gr += NT) {
        const int vc = gr / NR, rs = gr - vc * NR, ci = vc / g.KT, kt = vc - ci * g.KT;
        const int row = tf + rs + kt * g.dt - g.pt, pos0 = (rs ? 0 : f0) * S - g.pf;
        const bool ok = rs < nr && row >= 0 && row < g.T2;
        rtab[gr] = make_int2(ok ? (ci * g.T2 + row) * g.Fi + pos0 : 0, ok ? pos0 : -(1 << 30));
    }
    const int dr = NT / RL, dw = NT - dr * RL, r_init = tid / RL, w_init = tid - r_init * RL;
    const int wcol = tid & (BM - 1);
    for (int c0 = 0; c0 < VC; c0 += CK) {
        __syncthreads();
        {
            const int nrows = min(CK, VC - c0) * NR, items = CK * XR;
            int r = r_init, w = w_init;
            for (int i0 = 0; i0 < items; i0 += NT * DPER) {
                // (row, column) of the DPER items, then their table entries, then the loads
                int rq[DPER], wq[DPER];
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    rq[q] = r;
                    wq[q] = w;
                    w += dw;
                    r += dr;
                    if (w >= RL) {
                        w -= RL;
                        ++r;
                    }
                }
                int2 e[DPER];
#pragma unroll
                for (int q = 0; q < DPER; ++q) e[q] = rtab[c0 * NR + (rq[q] < nrows ? rq[q] : 0)];
                float v[DPER];
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int pos = e[q].y + wq[q];
                    const bool ok = rq[q] < nrows && pos >= 0 && pos < g.Fi;
                    const float t = xb[ok ? e[q].x + wq[q] : 0];
                    v[q] = ok ? t : 0.f;
                }
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int i = i0 + q * NT + tid;
                    if (i < items) Xs[i] = v[q];
                }
            }
        }
        {
            // Ws[cl][kf][col] = wf[(c0 + cl, kf)][co0 + col]: rows (cl, kf) are consecutive rows
            // of wf, so an item's source needs no division
            const int items = KF * CK * BM, rows = (VC - c0) * KF, co = co0 + wcol;
            const float* wsrc = a.wf + (int64_t)c0 * KF * g.Co + co;
            for (int i0 = 0; i0 < items; i0 += NT * DPER) {
                float v[DPER];
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int rr = (i0 + q * NT + tid) / BM;
                    const bool ok = rr < rows && co < g.Co;
                    const float t = wsrc[ok ? (int64_t)rr * g.Co : 0];
                    v[q] = ok ? t : 0.f;
                }
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int i = i0 + q * NT + tid;
                    if (i < items) Ws[i] = v[q];
                }
            }
        }
        __syncthreads();
        if constexpr (KFC > 0) {
            // k-pairs = combo pairs (cp, cp+1); the KF taps of a pair unrolled, so every
            // accumulator sees KFC independent MFMAs per loop trip and the loads run ahead
            for (int cp = 0; cp < CK; cp += 2) {
                const float* wk = Ws + (cp + h) * KFC * BM + wm0 + l32;
                const float* xk = Xs + (cp + h) * XR;
#pragma unroll
                for (int kf = 0; kf < KFC; ++kf) {
                    float av[TM], bv[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) av[i] = wk[kf * BM + i * 32];
#pragma unroll
                    for (int j = 0; j < TN; ++j) bv[j] = xk[boff[j] + kf];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(av[i], bv[j], acc[i][j]);
                }
            }
        } else {
            for (int kf = 0; kf < KF; ++kf) {
                const float* wk = Ws + (h * KF + kf) * BM + wm0 + l32;
                const float* xk = Xs + h * XR + kf;
                for (int cp = 0; cp < CK; cp += 2) {
                    float av[TM], bv[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) av[i] = wk[cp * KF * BM + i * 32];
#pragma unroll
                    for (int j = 0; j < TN; ++j) bv[j] = xk[cp * XR + boff[j]];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(av[i], bv[j], acc[i][j]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn0 + j * 32 + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm0 + i * 32 + mfma_row(r, lane);
                const float bco = a.bias ? a.bias[co < g.Co ? co : g.Co - 1] : 0.f;  // unconditional load
                if (co < g.Co && n < nend) {
                    float v = acc[i][j][r] + bco;
                    if (a.act) v = lrelu(v);
                    a.y[((int64_t)b * g.Co + co) * Nall + n] = v;
                }
            }
        }
}

// Forward with column-aligned window quads. A window row holds input columns [base, base + RLp)
// of one input row, base = the row's first needed column rounded DOWN to a multiple of 4 (the
// compute reads at an offset of col - base), so every quad is aligned to input columns: a quad
// is entirely padding (left of column 0, or a row outside the input: a select, no load),
// entirely interior, or the one quad holding column Fi - 1 whose tail lanes are masked. The
// loads are issued for the next chunk before the current chunk's MFMAs (MQ quads per thread),
// and the commit is a masked select + ds_write_b128: no per-element paths, no shifts.
template <int BN, int KFC, int MQ, int CKM, int OCC = 1>  // OCC: min waves per SIMD (register cap)
__global__ __launch_bounds__(NT, OCC) void c2_fwdr_kernel(C2Fwd a) {
    constexpr int BM = 32, TN = BN / 128, MW = (KFC * CKM * BM / 4 + NT - 1) / NT;
    extern __shared__ float smem[];
    const C2Geo g = a.g;
    const int CK = a.CK, NR = a.NR, RL = a.RL, S = g.sf;
    const int RLp = (RL + 3) & ~3, NQ = RLp >> 2;
    const int VC = g.Ci * g.KT, XR = NR * RLp, WQ = KFC * CK * BM / 4;
    float* Xs = smem;                      // [CK][NR][RLp]
    float* Ws = smem + CK * XR;            // [CK][KFC][BM]
    int2* rtab = (int2*)(Ws + KFC * CK * BM);  // [VC*NR]: {offset of column `base`, base} / invalid
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l32 = lane & 31;
    const TileId tile = xcd_tile();
    const int b = tile.z, n0 = tile.x * BN, co0 = tile.y * BM;
    const int wn0 = wave * TN * 32;
    const int Nall = g.T2 * g.Fo, nend = min(Nall, n0 + BN);
    const int tf = n0 / g.Fo, f0 = n0 - tf * g.Fo;
    const int nr = (nend - 1) / g.Fo - tf + 1;
    const int base0 = ((f0 * S - g.pf) & ~3), baseN = ((-g.pf) & ~3);  // floor to a multiple of 4
    int boff[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn0 + j * 32 + l32;
        boff[j] = 0;
        if (n < nend) {
            const int tr = n / g.Fo, f = n - tr * g.Fo, rs = tr - tf;
            boff[j] = rs * RLp + f * S - g.pf - (rs ? baseN : base0);
        }
    }
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[j] = (f32x16){0};
    const int64_t xtot = (int64_t)g.B * g.Ci * g.T2 * g.Fi;
    const float* xb = a.x + (int64_t)b * g.Ci * g.T2 * g.Fi;
    const int64_t xleft = xtot - (int64_t)b * g.Ci * g.T2 * g.Fi;  // floats from xb to the tensor end
    for (int gr = tid; gr < VC * NR; gr += NT) {
        const int vc = gr / NR, rs = gr - vc * NR, ci = vc / g.KT, kt = vc - ci * g.KT;
        const int row = tf + rs + kt * g.dt - g.pt, base = rs ? baseN : base0;
        const bool ok = rs < nr && row >= 0 && row < g.T2;
        rtab[gr] = make_int2(ok ? (ci * g.T2 + row) * g.Fi + base : 0, ok ? base : -(1 << 30));
    }
    __syncthreads();
    const int rows = CK * NR;
    const int dr = NT / NQ, dq = NT - dr * NQ, r_init = tid / NQ, q_init = tid - r_init * NQ;
    f32x4 xv[MQ], wv[MW];
    int xmask[MQ], xdst[MQ];
    auto fetch = [&](int c0) {
        const int nrows = min(CK, VC - c0) * NR;
        int r = r_init, q = q_init;
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            const bool live = r < nrows;
            const int2 e = rtab[c0 * NR + (live ? r : 0)];
            const int col = e.y + 4 * q;  // first input column of the quad
            const bool any = live && col >= 0 && col < g.Fi;  // e.y = -2^30 for rows outside
            int off = any ? e.x + 4 * q : 0;
            // the last quad of the tensor may run past its end: read it one quad earlier
            // (only columns < Fi are kept, and those are then at lanes shifted... see mask)
            if (off > xleft - 4) off = (int)xleft - 4;
            xv[u] = ld4u(xb + off);
            const int sh = (any ? e.x + 4 * q : 0) - off;  // 0 except at the tensor's very end
            xmask[u] = any ? (min(g.Fi - col, 4) | (sh << 4)) : 0;  // valid lanes, shift
            xdst[u] = r < rows ? r * RLp + 4 * q : -1;
            q += dq;
            r += dr;
            if (q >= NQ) {
                q -= NQ;
                ++r;
            }
        }
        const float* wsrc = a.wf + (int64_t)c0 * KFC * g.Co + co0;
        const int wrows = (VC - c0) * KFC;
#pragma unroll
        for (int u = 0; u < MW; ++u) {
            const int j = u * NT + tid, rr = j >> 3, col = (j & 7) * 4;
            const bool ok = j < WQ && rr < wrows && co0 + col + 3 < g.Co;
            wv[u] = ld4u(wsrc + (ok ? (int64_t)rr * g.Co + col : 0));
            if (!ok) wv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < VC; c0 += CK) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            const int m = xmask[u], nv = m & 15, sh = m >> 4;
            f32x4 v = xv[u];
            if (sh) {  // the tensor's last quad, read shifted back by sh lanes (one quad in all)
                const f32x4 t = v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = k + sh < 4 ? (k + sh == 1 ? t[1] : k + sh == 2 ? t[2] : t[3]) : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < nv ? v[k] : 0.f;
            if (xdst[u] >= 0) *(f32x4*)(Xs + xdst[u]) = v;
        }
#pragma unroll
        for (int u = 0; u < MW; ++u) {
            const int j = u * NT + tid, rr = j >> 3, col = (j & 7) * 4;
            if (j < WQ && rr < (VC - c0) * KFC && co0 + col + 3 >= g.Co)  // partial co tile (Co % 4)
                for (int k = 0; k < 4; ++k)
                    wv[u][k] = co0 + col + k < g.Co ? a.wf[((int64_t)c0 * KFC + rr) * g.Co + co0 + col + k] : 0.f;
            if (j < WQ) *(f32x4*)(Ws + rr * BM + col) = wv[u];
        }
        __syncthreads();
        if (c0 + CK < VC) fetch(c0 + CK);
#pragma unroll 2
        for (int cp = 0; cp < CK; cp += 2) {
            const float* wk = Ws + (cp + h) * KFC * BM + l32;
            const float* xk = Xs + (cp + h) * XR;
#pragma unroll
            for (int kf = 0; kf < KFC; ++kf) {
                const float av = wk[kf * BM];
                float bv[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) bv[j] = xk[boff[j] + kf];
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[j] = mfma32(av, bv[j], acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn0 + j * 32 + l32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + mfma_row(r, lane);
            const float bco = a.bias ? a.bias[co < g.Co ? co : g.Co - 1] : 0.f;
            if (co < g.Co && n < nend) {
                float v = acc[j][r] + bco;
                if (a.act) v = lrelu(v);
                a.y[((int64_t)b * g.Co + co) * Nall + n] = v;
            }
        }
    }
}

// Forward, register-window form. The 32 x (Ci*KT*KF) weights of the layer are staged ONCE per
// workgroup into LDS ([(ci,kt)][kf][32 co], the wf layout), then each wave loops over tiles of
// 32 output-position QUADS (128 positions; rows padded to whole quads, F4 = ceil(Fo/4) quads
// per row). Lane l of a wave owns quad l: its 4 consecutive output columns f0..f0+3 are the
// MFMA columns of its 4 accumulators (jb = 0..3). The MFMA's two k slots are two input channels
// (ci = 2c + h), so per (c, kt) step each lane loads ONE contiguous input window
// x[ci][t + kt*dt - pt][S*f0 - pf .. + 3S + KF - 1] (WQ quads, straight from global memory into
// registers) which holds the operand of all KF taps x 4 columns: 4 * KF MFMAs per step, each
// with no address arithmetic, the A operand (weights) one ds_read_b32 per tap shared by the 4
// columns. The next step's window is loaded before this step's MFMAs. Window elements outside
// the input (padding, rows outside [0, T2), the tensor's ends) are zeroed by a per-lane
// element mask, only in waves that have such a lane. Bias + LeakyReLU(0.2) in the epilogue.
struct C2FwdR {
    C2Geo g;
    const float* x;
    const float* wf;  // [(ci,kt)][kf][co]
    const float* bias;
    float* y;
    int act;
    int F4;     // quads per output row
    int tiles;  // ceil(B * T2 * F4 / 32)
    C2_TRACE_ARG
};
template <int KF, int S, int WQ, int NWV>
__global__ __launch_bounds__(NWV * 64) void c2_fwd_rw_kernel(C2FwdR a) {
    constexpr int NE = 4 * WQ, KT = 3;  // window elements per lane; kernel rows (host-checked)
    extern __shared__ float smem[];
    const C2Geo g = a.g;
    const int tslot = blockIdx.x * NWV + (threadIdx.x >> 6);  // (trace builds only)
    int titem = 0;
    (void)titem;
    C2_TRACE(a.tr, tslot, 0);
    float* Ws = smem;                          // [Ci*KT][KF][32]
    float* Bs = smem + g.Ci * KT * KF * 32;    // [32] bias
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, l = lane & 31;
    // element offsets fit in 32 bits (checked on the host)
    const int quads = g.B * g.T2 * a.F4;
    const int plane = g.T2 * g.Fi, xlast = g.B * g.Ci * plane - 4;
    const int CP = g.Ci >> 1;  // channel pairs
    const int cstride = 2 * plane;
    // one item's geometry: window element e of step (c, kt) is x[b][2c + h][row(kt)][col0 + e]
    struct Geo {
        int t, b, f0;
        int rb[KT];
        uint32_t msk[KT];
        bool fix;  // wave-uniform: some lane's window leaves the input
    };
    auto geo = [&](int tile) {
        Geo q;
        const int qd = min(tile * 32 + l, quads - 1);
        const int fq = qd % a.F4, bt = qd / a.F4;
        q.t = bt % g.T2;
        q.b = bt / g.T2;
        q.f0 = 4 * fq;
        const int col0 = S * q.f0 - g.pf;
        uint32_t cmask = 0;
#pragma unroll
        for (int e = 0; e < NE; ++e) cmask |= (col0 + e >= 0 && col0 + e < g.Fi) ? (1u << e) : 0u;
        bool clean = true;  // every element of every window of this lane is in the input
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            const int row = q.t + kt * g.dt - g.pt;
            const bool ok = row >= 0 && row < g.T2;
            q.rb[kt] = (q.b * g.Ci + h) * plane + (ok ? row : 0) * g.Fi + col0;
            q.msk[kt] = ok ? cmask : 0u;
            clean = clean && q.msk[kt] == (1u << NE) - 1;
        }
        q.fix = !__all(clean);
        return q;
    };
    auto load = [&](f32x4* w, const Geo& q, int c, int kt) {
        const int base = q.rb[kt] + c * cstride;
#pragma unroll
        for (int w4 = 0; w4 < WQ; ++w4) w[w4] = ld4u(a.x + min(max(base + 4 * w4, 0), xlast));
    };
    // three register windows, one per kt: step (c, kt) multiplies window kt with the weight
    // columns of (c, kt), read from LDS just in time, while the next step's window is in flight
    // (the prefetch is unconditional, so every wait is exact). The last step of an item loads the
    // NEXT item's first window, so it is in flight during this item's epilogue stores and the
    // next item does not start by waiting out a memory round trip behind them (vmcnt counts the
    // stores too). Measured against reading the weights a step ahead or one tap ahead: none is
    // faster (profiles/r05).
    f32x4 wb[KT][WQ];
    auto wcol = [&](int c, int kt) { return Ws + ((2 * c + h) * KT + kt) * KF * 32 + l; };
    const int stride = gridDim.x * NWV;
    int tile = rw_first_slot(wave);
    // the first item's window goes out ahead of the weights, so it arrives under their staging
    if (tile < a.tiles) load(wb[0], geo(tile), 0, 0);
    // the weights, once per workgroup. Co == 32 (every layer of the discriminator): wf is the LDS
    // layout, copied as quads, RW_SQ of them in flight per thread ahead of their LDS writes (one
    // memory round trip for the 32-channel layers' 108 KB at 512 threads; loaded dword by dword,
    // eight in flight, it was seven).
    if (g.Co == 32) {
        const int nq = g.Ci * KT * KF * 8;
        for (int i0 = 0; i0 < nq; i0 += NWV * 64 * RW_SQ) {
            f32x4 sv[RW_SQ];
#pragma unroll
            for (int u = 0; u < RW_SQ; ++u)
                sv[u] = ld4u(a.wf + 4 * min(i0 + u * NWV * 64 + (int)threadIdx.x, nq - 1));
#pragma unroll
            for (int u = 0; u < RW_SQ; ++u) {
                const int i = i0 + u * NWV * 64 + (int)threadIdx.x;
                if (i < nq) *(f32x4*)(Ws + 4 * i) = sv[u];
            }
        }
    } else {
        for (int i = threadIdx.x; i < g.Ci * KT * KF * 32; i += NWV * 64) {
            const int co = i & 31, r = i >> 5;
            Ws[i] = co < g.Co ? a.wf[r * g.Co + co] : 0.f;
        }
    }
    if (threadIdx.x < 32) Bs[threadIdx.x] = (a.bias && (int)threadIdx.x < g.Co) ? a.bias[threadIdx.x] : 0.f;
    __syncthreads();
    C2_TRACE(a.tr, tslot, 1);
    for (; tile < a.tiles; tile += stride) {
        const Geo cur = geo(tile);  // (recomputed: cheaper than holding the next item's in registers)
        const int t = cur.t, b = cur.b, f0 = cur.f0;
        f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (f32x16){0};
        C2_TRACE(a.tr, tslot, 3 + 3 * titem);
        for (int c = 0; c < CP; ++c) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const int nk = kt + 1 < KT ? kt + 1 : 0;
                if (kt + 1 < KT) load(wb[nk], cur, c, nk);
                else if (c + 1 < CP) load(wb[0], cur, c + 1, 0);
                else load(wb[0], geo(tile + stride < a.tiles ? tile + stride : tile), 0, 0);  // (past the last: own)
                f32x4* w = wb[kt];
                if (cur.fix) {
                    const int base = cur.rb[kt] + c * cstride;
#pragma unroll
                    for (int q = 0; q < WQ; ++q) {
                        const int o = base + 4 * q;
                        if (__any(o < 0 || o > xlast)) w[q] = quad_abs(w[q], o, xlast);  // tensor ends
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (!((cur.msk[kt] >> (4 * q + e)) & 1u)) w[q][e] = 0.f;
                    }
                }
                const float* wk = wcol(c, kt);
#pragma unroll
                for (int kf = 0; kf < KF; ++kf) {
                    const float av = wk[kf * 32];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = S * j + kf;
                        acc[j] = mfma32(av, w[r >> 2][r & 3], acc[j]);
                    }
                }
            }
        }
        C2_TRACE(a.tr, tslot, 4 + 3 * titem);
        // ---- epilogue: rows co, columns f0 + j of this lane's quad
        if (tile * 32 + l < quads) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = mfma_row(r, lane);
                if (co >= g.Co) continue;
                const float bco = Bs[co];
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float u = acc[j][r] + bco;
                    v[j] = a.act ? lrelu(u) : u;
                }
                float* dst = a.y + (((int64_t)b * g.Co + co) * g.T2 + t) * g.Fo + f0;
                if (f0 + 4 <= g.Fo) {
                    *(f32x4u*)dst = v;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (f0 + j < g.Fo) dst[j] = v[j];
                }
            }
        }
        C2_TRACE(a.tr, tslot, 5 + 3 * titem);
        ++titem;
        C2_TRACE_VAL(a.tr, tslot, 2, titem);
    }
}

// ------------------------------------------------------------- single output channel (Co = 1)
// The post conv of each DiscriminatorSTFT (msstftd.py:80-81, 32 -> 1, 3x3) has one output
// channel, so an MFMA tile would idle 31 of its 32 rows. c2_co1_fwd, c2_co1_dgrad and c2_co1_wgrad
// are VALU kernels with the taps unrolled (KT, KF, stride compile-time) and clamped loads, so
// every lane keeps its KT*KF loads in flight; lanes run along the frequency axis (coalesced). Each
// input element is read KT*KF times through L1/L2; the HBM traffic is the algorithmic
// |x| + |y| (+ |dx|).

// y[b][0][t][fo]: block = 64 output columns x 4 ci groups of one (b, t); the 4 partial sums meet
// in LDS in a fixed order.
template <int KT, int KF, int S>
__global__ __launch_bounds__(256) void c2_co1_fwd(C2Fwd a) {
    const C2Geo g = a.g;
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, cg = threadIdx.x >> 6;
    const int plane = g.T2 * g.Fo, p = blockIdx.x * 64 + lane, b = blockIdx.y;
    const int pc = p < plane ? p : plane - 1;
    const int t = pc / g.Fo, fo = pc - t * g.Fo;
    const int64_t xplane = (int64_t)g.T2 * g.Fi;
    const int cper = (g.Ci + 3) >> 2, c0 = cg * cper, c1 = min(g.Ci, c0 + cper);
    const int fb = fo * S - g.pf;
    float acc = 0.f;
    for (int ci = c0; ci < c1; ++ci) {
        const float* xc = a.x + ((int64_t)b * g.Ci + ci) * xplane;
        const float* w = a.wf + ci * KT * KF;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            const int tr = t + kt * g.dt - g.pt;
            const bool rok = tr >= 0 && tr < g.T2;
            const float* row = xc + (int64_t)(rok ? tr : 0) * g.Fi;
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) {
                const int f = fb + kf;
                const bool ok = rok && f >= 0 && f < g.Fi;
                const float v = row[ok ? f : 0];
                acc = fmaf(w[kt * KF + kf], ok ? v : 0.f, acc);
            }
        }
    }
    part[cg][lane] = acc;
    __syncthreads();
    if (cg == 0 && p < plane) {
        float v = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        if (a.bias) v += a.bias[0];
        a.y[(int64_t)b * plane + p] = a.act ? lrelu(v) : v;
    }
}

// ---------------------------------------------------------------------------- planning
template <int BM, int BN, int WM, int WN, int KFC = 0>
int launch_fwd(C2Fwd a, hipStream_t st) {
    const size_t lds = ((size_t)a.CK * a.NR * a.RL + (size_t)a.g.KF * a.CK * BM +
                        (size_t)2 * a.g.Ci * a.g.KT * a.NR + 2) * sizeof(float);
    dim3 grid((unsigned)cdiv((int64_t)a.g.T2 * a.g.Fo, BN), (unsigned)cdiv(a.g.Co, BM), (unsigned)a.g.B);
    hipLaunchKernelGGL((c2_fwd_kernel<BM, BN, WM, WN, KFC>), grid, dim3(NT), lds, st, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

// planned launches: window geometry and LDS chunking for the column tile BN
template <int BM, int BN, int WM, int WN, int KFC = 0>
int run_fwd(C2Fwd a, hipStream_t st, int budget = 12288) {
    a.NR = c2_rows(BN, a.g.Fo);
    a.RL = (min(BN, a.g.Fo) - 1) * a.g.sf + a.g.KF;
    a.CK = c2_ck(a.g.Ci * a.g.KT, a.NR * a.RL + a.g.KF * BM, budget);
    return launch_fwd<BM, BN, WM, WN, KFC>(a, st);
}

// register-window forward (c2_fwd_rw_kernel): 32-wide output-channel tile, even Ci, KT <= 3,
// the layer's weights in LDS (<= 128 KB)
static bool fwr_ok(const C2Geo& g) {
    if (g.Co > 32 || (g.Ci & 1) || g.KT != 3 || g.Fo < 1 || g.Fi < 4) return false;
    if ((int64_t)g.B * g.Ci * g.T2 * g.Fi >= (1ll << 31) || (int64_t)g.B * g.T2 * cdiv(g.Fo, 4) >= (1ll << 31) - 64)
        return false;
    if (!((g.KF == 9 && (g.sf == 2 || g.sf == 1)) || (g.KF == 3 && g.sf == 1))) return false;
    return (size_t)g.Ci * g.KT * g.KF * 32 * sizeof(float) <= 128 * 1024;
}
// wgs: workgroups (one per CU holds the layer's weights) of 8 waves
static int run_fwd_rw(const C2Fwd& f, int wgs, hipStream_t st) {
    if (!fwr_ok(f.g)) return ENCX_EINVAL;
    constexpr int NWV = 8;
    const C2Geo& g = f.g;
    C2FwdR a{g, f.x, f.wf, f.bias, f.y, f.act, (int)cdiv(g.Fo, 4), 0};
    a.tiles = (int)cdiv((int64_t)g.B * g.T2 * a.F4, 32);
    C2_TRACE_SET(a);
    const size_t lds = ((size_t)g.Ci * g.KT * g.KF * 32 + 32) * sizeof(float);
    const int grid = (int)min((int64_t)wgs, cdiv(a.tiles, NWV));
    if (g.KF == 9 && g.sf == 2)
        hipLaunchKernelGGL((c2_fwd_rw_kernel<9, 2, 4, NWV>), dim3(grid), dim3(NWV * 64), lds, st, a);
    else if (g.KF == 9)
        hipLaunchKernelGGL((c2_fwd_rw_kernel<9, 1, 3, NWV>), dim3(grid), dim3(NWV * 64), lds, st, a);
    else
        hipLaunchKernelGGL((c2_fwd_rw_kernel<3, 1, 2, NWV>), dim3(grid), dim3(NWV * 64), lds, st, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}
template <int BN, int KFC, int MQ, int CKM, int OCC = 1>
int run_fwdr(C2Fwd a, hipStream_t st) {
    a.NR = c2_rows(BN, a.g.Fo);
    a.RL = (min(BN, a.g.Fo) - 1) * a.g.sf + a.g.KF + 3;  // + alignment slack of the column base
    a.CK = quad_ck(a.g.Ci * a.g.KT, a.NR, a.RL, MQ, CKM);
    if (a.g.KF != KFC || a.CK < 2 || a.g.Fi < 4 || a.g.pf > 4) return ENCX_EINVAL;
    const int RLp = (a.RL + 3) & ~3;
    const size_t lds = ((size_t)a.CK * a.NR * RLp + (size_t)KFC * a.CK * 32 + (size_t)2 * a.g.Ci * a.g.KT * a.NR) *
                       sizeof(float);
    dim3 grid((unsigned)cdiv((int64_t)a.g.T2 * a.g.Fo, BN), (unsigned)cdiv(a.g.Co, 32), (unsigned)a.g.B);
    hipLaunchKernelGGL((c2_fwdr_kernel<BN, KFC, MQ, CKM, OCC>), grid, dim3(NT), lds, st, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// Register-window or tiled kernel for a layer. The register-window kernels hand whole 128-position
// items to SIMDs (rw_first_slot), so their time follows ceil(items / SIMDs) item rounds; the tiled
// kernels' time follows the positions. Per round / per 128 x SIMDs positions, measured on the
// config-3 layers (tools/mb/c2_mb, profiles/r03/mb_rw.md): forward 66 vs 87 us, bwd-data 78 vs 92
// us -- so the register-window form loses on layers whose last round is mostly idle (Fo 65 at
// T2 90, Fo 65 at T2 184) and wins everywhere else. `ratio` = tiled / register-window cost.
int g_c2_select = [] {  // encx_conv2d_select; ENCX_C2 sets the initial mode
    const char* v = getenv("ENCX_C2");
    return v ? atoi(v) : 0;
}();
bool rw_pays(int64_t items, int64_t positions, double ratio) {
    if (g_c2_select != 0) return g_c2_select == 1;
    static const int simds = [] {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) cus = 256;
        return 4 * cus;
    }();
    const double rounds = std::ceil((double)items / simds), tiled = (double)positions / (128.0 * simds);
    return rounds < ratio * tiled;
}

#ifdef ENCX_C2_TRACE
C2Trace g_c2_trace{nullptr, 0};
#endif

extern "C" {

int encx_conv2d_trace(int64_t* buf, int64_t n) {
#ifdef ENCX_C2_TRACE
    ENCX_REQUIRE(n >= 0 && (buf || n == 0));
    g_c2_trace = C2Trace{(long long*)buf, (int)std::min<int64_t>(n / C2_TR_W, 1 << 20)};
    return 0;
#else
    (void)buf;
    (void)n;
    return ENCX_EINVAL;
#endif
}

int encx_conv2d_select(int mode) {
    const int prev = g_c2_select;
    if (mode >= 0 && mode <= 2) g_c2_select = mode;
    return prev;
}

int encx_conv2d_fwd(const float* x, const float* wf, const float* bias, float* y, int64_t B, int64_t Ci,
                    int64_t T2, int64_t Fi, int64_t Co, int64_t Fo, int64_t KT, int64_t KF, int64_t sf,
                    int64_t dt, int64_t pt, int64_t pf, int act, encx_stream_t stream) {
    ENCX_REQUIRE(x && wf && y);
    C2Geo g{(int)B, (int)Ci, (int)T2, (int)Fi, (int)Co, (int)Fo, (int)KT, (int)KF, (int)sf, (int)dt, (int)pt, (int)pf};
    ENCX_REQUIRE(geo_ok(g));
    hipStream_t st = (hipStream_t)stream;
    encx_prof_scope ps(st, 2.0 * B * Co * T2 * Fo * Ci * KT * KF, 4.0 * (B * Ci * T2 * Fi + B * Co * T2 * Fo), "c2_fwd");
    ps.tag(" %ldx%ld %ldx%ld s%ld T%ld F%ld", (long)Ci, (long)Co, (long)KT, (long)KF, (long)sf, (long)T2, (long)Fo);
    C2Fwd a{g, x, wf, bias, y, act, 0, 0, 0};
    // register-window form (c2_fwd_rw_kernel); option FWR = workgroups (0: off)
    const int fw_wgs = (int)encx_opt(OPT_FWR);
    if (fw_wgs > 0 && fwr_ok(g) &&
        ((Ci * KT < 16 && g_c2_select != 2) || rw_pays(cdiv(B * T2 * cdiv(Fo, 4), 32), B * T2 * Fo, 87.0 / 66.0)) &&
        run_fwd_rw(a, fw_wgs, st) == 0)
        return 0;
    if (Co == 1 && KT == 3 && KF == 3 && (sf == 1 || sf == 2)) {
        dim3 grid((unsigned)cdiv(T2 * Fo, 64), (unsigned)B);
        if (sf == 1) hipLaunchKernelGGL((c2_co1_fwd<3, 3, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((c2_co1_fwd<3, 3, 2>), grid, dim3(256), 0, st, a);
        ENCX_CHECK_LAUNCH();
        return 0;
    }
    // column-aligned, register-pipelined staging (c2_fwdr_kernel) for the 32-channel layers; the
    // 2-channel first layer (K = 54) keeps the round-1 kernel, which is faster there
    if (Co <= 32 && Ci * KT >= 16) {
        if (KF == 9 && run_fwdr<256, 9, 6, 16>(a, st) == 0) return 0;
        if (KF == 3 && run_fwdr<256, 3, 6, 32>(a, st) == 0) return 0;
    }
    if (Co <= 32) return run_fwd<32, 128, 1, 4>(a, st);
    return run_fwd<64, 128, 2, 2>(a, st);
}

}  // extern "C"
