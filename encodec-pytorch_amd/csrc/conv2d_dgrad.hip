// NormConv2d backward-data (conv2d.h) on gfx950: the tiled polyphase kernel, its column-aligned
// register-pipelined form, the register-window form, the narrow first-layer kernel and the
// single-output-channel kernel; encx_conv2d_bwd_data[_feat] picks one per layer. Also the
// polyphase weight layout they read (encx_conv2d_wpoly).
#include "common.h"
#include "conv2d.h"
#include "prof.h"

namespace {

struct C2Dg {
    C2Geo g;
    const float* dy;    // [B][Co][T2][Fo]
    const float* yact;  // post-activation output (LeakyReLU' mask of dy) or null
    const float* wp;    // [(co,kt)][J][ci*S + r]
    const float* xact;  // input (LeakyReLU' of the previous layer) or null
    float* dx;          // [B][Ci][T2][Fi]
    int J, U, CK, NR, RL, accumulate;
    // optional feature-matching term added to dx (FeatFn's grad of this input map, fused here
    // instead of a separate grad tensor + add): c * sign(ffx - ffr), c = fg[0] * fscale / fden[0]
    const float* ffr;   // real map [B][Ci][T2][Fi] or null
    const float* ffx;   // fake map (this layer's input)
    const float* fden;  // mean |fr| of the pair
    const float* fg;    // upstream grad of the loss (null: 1)
    float fscale;
    // optional per-element code of the pair (encx_feat_loss_code): bit 0 ffx > ffr, bit 1
    // ffx < ffr, bit 2 ffx > 0. The register-window and tiled epilogues read it (1 byte) instead
    // of ffx / ffr (8 bytes) when the mask comes from ffx or is absent
    const uint8_t* fcode;
};
ENCX_DEV float code_term(uint32_t c, float fc) { return (c & 1u) ? fc : ((c & 2u) ? -fc : 0.f); }
ENCX_DEV float code_mask(uint32_t c) { return (c & 4u) ? 1.f : 0.2f; }

ENCX_DEV float feat_coef(const C2Dg& a) {
    return a.ffr ? (a.fg ? a.fg[0] : 1.f) * a.fscale / a.fden[0] : 0.f;
}
// same value as feat_grad_kernel's dff (disc.hip) for element o. In every epilogue the grad of the input map
// is completed by the feature term first; xact then turns it into the grad of the input's
// pre-activation, so the producing layer reads dy without its mask.
ENCX_DEV float feat_term(const C2Dg& a, float c, int64_t o) {
    const float d = a.ffx[o] - a.ffr[o];
    return d > 0.f ? c : (d < 0.f ? -c : 0.f);
}
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));

template <int BM, int BN, int WM, int WN, int JC = 0>
__global__ __launch_bounds__(NT) void c2_dgrad_kernel(C2Dg a) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    extern __shared__ float smem[];
    const C2Geo g = a.g;
    const int CK = a.CK, NR = a.NR, RL = a.RL, J = a.J, U = a.U, S = g.sf;
    const int VC = g.Co * g.KT, XR = NR * RL, M = g.Ci * S;
    float* Xs = smem;            // [CK][NR][RL]
    float* As = smem + CK * XR;  // [CK][J][BM]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / WN) * TM * 32, wn0 = (wave % WN) * TN * 32;
    const int h = lane >> 5, l32 = lane & 31;
    const int b = blockIdx.z, n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
    const int Nall = g.T2 * U, nend = min(Nall, n0 + BN);
    const int tf = n0 / U, u0 = n0 - tf * U;
    const int nr = (nend - 1) / U - tf + 1;
    int boff[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn0 + j * 32 + l32;
        boff[j] = J - 1;  // in-range LDS reads for masked columns
        if (n < nend) {
            const int tr = n / U, u = n - tr * U, rs = tr - tf;
            boff[j] = rs * RL + (u - (rs ? 0 : u0)) + (J - 1);
        }
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};
    const int64_t plane = (int64_t)g.T2 * g.Fo;
    const float* dyb = a.dy + (int64_t)b * g.Co * plane;
    const float* yab = a.yact ? a.yact + (int64_t)b * g.Co * plane : nullptr;
    // staging as in c2_fwd_kernel: window-row table {offset, first position}, items walked by
    // a fixed step, weights in source order As[cl][q][m]
    int2* rtab = (int2*)(As + J * CK * BM);
    for (int gr = tid; gr < VC * NR; gr += NT) {
        const int vc = gr / NR, rs = gr - vc * NR, co = vc / g.KT, kt = vc - co * g.KT;
        const int row = tf + rs + g.pt - kt * g.dt, pos0 = (rs ? 0 : u0) - (J - 1);
        const bool ok = rs < nr && row >= 0 && row < g.T2;
        rtab[gr] = make_int2(ok ? co * (int)plane + row * g.Fo + pos0 : 0, ok ? pos0 : -(1 << 30));
    }
    const int dr = NT / RL, dw = NT - dr * RL, r_init = tid / RL, w_init = tid - r_init * RL;
    const int wcol = tid & (BM - 1);
    const float* ysrc = yab ? yab : dyb;
    for (int c0 = 0; c0 < VC; c0 += CK) {
        __syncthreads();
        {
            const int nrows = min(CK, VC - c0) * NR, items = CK * XR;
            int r = r_init, w = w_init;
            for (int i0 = 0; i0 < items; i0 += NT * DPER) {
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
                float v[DPER], ym[DPER];
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int pos = e[q].y + wq[q];
                    const bool ok = rq[q] < nrows && pos >= 0 && pos < g.Fo;
                    const int o = ok ? e[q].x + wq[q] : 0;
                    const float t = dyb[o];
                    if (yab) ym[q] = ysrc[o];
                    v[q] = ok ? t : 0.f;
                }
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int i = i0 + q * NT + tid;
                    if (i < items) Xs[i] = yab ? v[q] * lrelu_grad(ym[q]) : v[q];
                }
            }
        }
        {
            const int items = J * CK * BM, rows = (VC - c0) * J, m = m0 + wcol;
            const float* wsrc = a.wp + (int64_t)c0 * J * M + m;
            for (int i0 = 0; i0 < items; i0 += NT * DPER) {
                float v[DPER];
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int rr = (i0 + q * NT + tid) / BM;
                    const bool ok = rr < rows && m < M;
                    const float t = wsrc[ok ? (int64_t)rr * M : 0];
                    v[q] = ok ? t : 0.f;
                }
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int i = i0 + q * NT + tid;
                    if (i < items) As[i] = v[q];
                }
            }
        }
        __syncthreads();
        if constexpr (JC > 0) {
            for (int cp = 0; cp < CK; cp += 2) {
                const float* aq = As + (cp + h) * JC * BM + wm0 + l32;
                const float* xq = Xs + (cp + h) * XR;
#pragma unroll
                for (int q = 0; q < JC; ++q) {
                    float av[TM], bv[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) av[i] = aq[q * BM + i * 32];
#pragma unroll
                    for (int j = 0; j < TN; ++j) bv[j] = xq[boff[j] - q];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(av[i], bv[j], acc[i][j]);
                }
            }
        } else {
            for (int q = 0; q < J; ++q) {
                const float* aq = As + (h * J + q) * BM + wm0 + l32;
                const float* xq = Xs + h * XR - q;
                for (int cp = 0; cp < CK; cp += 2) {
                    float av[TM], bv[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) av[i] = aq[cp * J * BM + i * 32];
#pragma unroll
                    for (int j = 0; j < TN; ++j) bv[j] = xq[cp * XR + boff[j]];
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
            if (n >= nend) continue;
            const int tr = n / U, u = n - tr * U;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + i * 32 + mfma_row(r, lane);
                if (m >= M) continue;
                const int ci = m / S, rr = m - ci * S;
                const int f = u * S + rr - g.pf;
                if (f < 0 || f >= g.Fi) continue;
                const int64_t o = (((int64_t)b * g.Ci + ci) * g.T2 + tr) * g.Fi + f;
                float v = acc[i][j][r];
                if (a.ffr) v += feat_term(a, feat_coef(a), o);
                if (a.xact) v *= lrelu_grad(a.xact[o]);
                a.dx[o] = a.accumulate ? a.dx[o] + v : v;
            }
        }
}

// Backward-data with column-aligned quads and register pipelining (c2_fwdr_kernel's staging
// applied to c2_dgrad_kernel's polyphase GEMM): rows m = (ci, r) (BM = 32 * TM), columns
// (t, u), reduction (co, kt) pairs x JC taps; the staged B image is dy * LeakyReLU'(y), both
// read as aligned quads (dy columns [base, base + RLp), base = the window start rounded down to
// a multiple of 4) and masked in the commit.
// c2_dgradr_kernel's epilogue, its terms fixed at compile time (MODE bits as rw_dg_epi): no
// branches around the loads, and the output never aliases the maps read, so the 8 row pairs of a
// (row tile, column tile) are loaded together, then combined and stored.
template <int TM, int TN, int MODE, bool PS = false>
ENCX_DEV void dgr_epi(const C2Dg& a, const f32x16 (&acc)[TM][TN], int b, int m0, int nl, int nend, int U, int M,
                      int S, int lane, float fc, bool ps = false) {
    constexpr bool C = MODE & 16, F = (MODE & 1) && !C, XM = (MODE & 2) && !C, XL = MODE & 4, A = MODE & 8,
                   LX = F || XL, CX = C && (MODE & 2);
    const C2Geo& g = a.g;
    const float* __restrict__ xs = XL ? a.xact : a.ffx;
    const float* __restrict__ rs = a.ffr;
    const uint8_t* __restrict__ cs = a.fcode;
    float* __restrict__ dx = a.dx;
    auto combine = [&](float u, float x, float r, float d, uint32_t c) {
        if (F) {
            const float e = x - r;
            u += e > 0.f ? fc : (e < 0.f ? -fc : 0.f);
        }
        if (XM) u *= lrelu_grad(x);
        if (C) u += code_term(c, fc);
        if (CX) u *= code_mask(c);
        return A ? d + u : u;
    };
    if (PS && ps) {
        // phase-major rows (c2_dgradr_kernel with TM 2 at the 3x9 stride-2 layers): tile 0 holds
        // phase 0 and tile 1 phase 1 of the 32 ci, register r of both the same ci
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = nl + j * 32;
            if (n >= nend) continue;
            const int tr = n / U, u = n - tr * U, f = 2 * u - g.pf;
            if (f >= 0 && f + 1 < g.Fi) {
#pragma unroll
                for (int h8 = 0; h8 < 16; h8 += 8) {
                    int64_t o[8];
                    f32x2u X[8], R[8], D[8];
                    uint32_t Cc[8][2];
#pragma unroll
                    for (int p = 0; p < 8; ++p) {
                        o[p] = (((int64_t)b * g.Ci + mfma_row(h8 + p, lane)) * g.T2 + tr) * g.Fi + f;
                        if (LX) X[p] = *(const f32x2u*)(xs + o[p]);
                        if (F) R[p] = *(const f32x2u*)(rs + o[p]);
                        if (A) D[p] = *(const f32x2u*)(dx + o[p]);
                        if (C) {
                            Cc[p][0] = cs[o[p]];
                            Cc[p][1] = cs[o[p] + 1];
                        }
                    }
#pragma unroll
                    for (int p = 0; p < 8; ++p) {
                        f32x2u s2;
#pragma unroll
                        for (int e = 0; e < 2; ++e)
                            s2[e] = combine(acc[e][j][h8 + p], LX ? X[p][e] : 0.f, F ? R[p][e] : 0.f,
                                            A ? D[p][e] : 0.f, C ? Cc[p][e] : 0u);
                        *(f32x2u*)(dx + o[p]) = s2;
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int fe = f + e;
                        if (fe < 0 || fe >= g.Fi) continue;
                        const int64_t q = (((int64_t)b * g.Ci + mfma_row(r, lane)) * g.T2 + tr) * g.Fi + fe;
                        dx[q] = combine(acc[e][j][r], LX ? xs[q] : 0.f, F ? rs[q] : 0.f, A ? dx[q] : 0.f,
                                        C ? (uint32_t)cs[q] : 0u);
                    }
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = nl + j * 32;
            if (n >= nend) continue;
            const int tr = n / U, u = n - tr * U;
            if (S == 2) {
                // rows m, m + 1 (registers r, r + 1) are phases 0 / 1 of the same ci: the two
                // adjacent f of this column, one 8-byte access
                const int f = 2 * u - g.pf;
                if (f >= 0 && f + 1 < g.Fi && m0 + i * 32 + 32 <= M) {
                    int64_t o[8];
                    f32x2u X[8], R[8], D[8];
                    uint32_t Cc[8][2];
#pragma unroll
                    for (int p = 0; p < 8; ++p) {
                        const int m = m0 + i * 32 + mfma_row(2 * p, lane);
                        o[p] = (((int64_t)b * g.Ci + (m >> 1)) * g.T2 + tr) * g.Fi + f;
                        if (LX) X[p] = *(const f32x2u*)(xs + o[p]);
                        if (F) R[p] = *(const f32x2u*)(rs + o[p]);
                        if (A) D[p] = *(const f32x2u*)(dx + o[p]);
                        if (C) {
                            Cc[p][0] = cs[o[p]];
                            Cc[p][1] = cs[o[p] + 1];
                        }
                    }
#pragma unroll
                    for (int p = 0; p < 8; ++p) {
                        f32x2u s2;
#pragma unroll
                        for (int e = 0; e < 2; ++e)
                            s2[e] = combine(acc[i][j][2 * p + e], LX ? X[p][e] : 0.f, F ? R[p][e] : 0.f,
                                            A ? D[p][e] : 0.f, C ? Cc[p][e] : 0u);
                        *(f32x2u*)(dx + o[p]) = s2;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = m0 + i * 32 + mfma_row(r, lane);
                        const int fe = f + (r & 1);
                        if (m >= M || fe < 0 || fe >= g.Fi) continue;
                        const int64_t q = (((int64_t)b * g.Ci + (m >> 1)) * g.T2 + tr) * g.Fi + fe;
                        dx[q] = combine(acc[i][j][r], LX ? xs[q] : 0.f, F ? rs[q] : 0.f, A ? dx[q] : 0.f,
                                        C ? (uint32_t)cs[q] : 0u);
                    }
                }
                continue;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + i * 32 + mfma_row(r, lane);
                if (m >= M) continue;
                const int ci = m / S, rr = m - ci * S;
                const int f = u * S + rr - g.pf;
                if (f < 0 || f >= g.Fi) continue;
                const int64_t q = (((int64_t)b * g.Ci + ci) * g.T2 + tr) * g.Fi + f;
                dx[q] = combine(acc[i][j][r], LX ? xs[q] : 0.f, F ? rs[q] : 0.f, A ? dx[q] : 0.f,
                                C ? (uint32_t)cs[q] : 0u);
            }
        }
}

template <int TM, int BN, int JC, int MQ, int CKM, int OCC = 1, bool YM = true>
__global__ __launch_bounds__(NT, OCC) void c2_dgradr_kernel(C2Dg a) {
    constexpr int BM = 32 * TM, TN = BN / 128, MW = (JC * CKM * BM / 4 + NT - 1) / NT;
    // phase-major rows at the 3x9 stride-2 layers (both 32-row tiles in one workgroup): the fifth
    // polyphase tap, zero for every phase-1 row (kf = 2 q + 1 = 9), is skipped for tile 1
    constexpr bool PS = TM == 2 && JC == 5;
    extern __shared__ float smem[];
    const C2Geo g = a.g;
    const int CK = a.CK, NR = a.NR, RL = a.RL, U = a.U, S = g.sf;
    const int RLp = (RL + 3) & ~3, NQ = RLp >> 2;
    const int VC = g.Co * g.KT, XR = NR * RLp, M = g.Ci * S, WQ = JC * CK * BM / 4;
    float* Xs = smem;                     // [CK][NR][RLp]
    float* As = smem + CK * XR;           // [CK][JC][BM]
    int2* rtab = (int2*)(As + JC * CK * BM);  // [VC*NR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l32 = lane & 31;
    const TileId tile = xcd_tile();
    const int b = tile.z, n0 = tile.x * BN, m0 = tile.y * BM;
    const bool ps = PS && S == 2 && M == 64 && m0 == 0;
    const int wn0 = wave * TN * 32;
    const int Nall = g.T2 * U, nend = min(Nall, n0 + BN);
    const int tf = n0 / U, u0 = n0 - tf * U;
    const int nr = (nend - 1) / U - tf + 1;
    const int base0 = (u0 - (JC - 1)) & ~3, baseN = (-(JC - 1)) & ~3;
    int boff[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn0 + j * 32 + l32;
        boff[j] = JC - 1;  // in-range reads for masked columns
        if (n < nend) {
            const int tr = n / U, u = n - tr * U, rs = tr - tf;
            boff[j] = rs * RLp + u - (rs ? baseN : base0);
        }
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};
    const int64_t plane = (int64_t)g.T2 * g.Fo;
    const float* dyb = a.dy + (int64_t)b * g.Co * plane;
    const float* yab = YM ? a.yact + (int64_t)b * g.Co * plane : dyb;
    const int64_t left = (int64_t)(g.B - b) * g.Co * plane;  // floats from dyb to the tensor end
    const float fc = feat_coef(a);
    for (int gr = tid; gr < VC * NR; gr += NT) {
        const int vc = gr / NR, rs = gr - vc * NR, co = vc / g.KT, kt = vc - co * g.KT;
        const int row = tf + rs + g.pt - kt * g.dt, base = rs ? baseN : base0;
        const bool ok = rs < nr && row >= 0 && row < g.T2;
        rtab[gr] = make_int2(ok ? co * (int)plane + row * g.Fo + base : 0, ok ? base : -(1 << 30));
    }
    __syncthreads();
    const int rows = CK * NR;
    const int dr = NT / NQ, dq = NT - dr * NQ, r_init = tid / NQ, q_init = tid - r_init * NQ;
    f32x4 xv[MQ], yv[MQ], wv[MW];
    int xmask[MQ], xdst[MQ];
    auto fetch = [&](int c0) {
        const int nrows = min(CK, VC - c0) * NR;
        int r = r_init, q = q_init;
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            const bool live = r < nrows;
            const int2 e = rtab[c0 * NR + (live ? r : 0)];
            const int col = e.y + 4 * q;
            const bool any = live && col >= 0 && col < g.Fo;
            int off = any ? e.x + 4 * q : 0;
            if (off > left - 4) off = (int)left - 4;
            xv[u] = ld4u(dyb + off);
            if (YM) yv[u] = ld4u(yab + off);
            const int sh = (any ? e.x + 4 * q : 0) - off;
            xmask[u] = any ? (min(g.Fo - col, 4) | (sh << 4)) : 0;
            xdst[u] = r < rows ? r * RLp + 4 * q : -1;
            q += dq;
            r += dr;
            if (q >= NQ) {
                q -= NQ;
                ++r;
            }
        }
        const float* wsrc = a.wp + (int64_t)c0 * JC * M + m0;
        const int wrows = (VC - c0) * JC;
#pragma unroll
        for (int u = 0; u < MW; ++u) {
            const int j = u * NT + tid, rr = j / (BM / 4), col = (j % (BM / 4)) * 4;
            const bool ok = j < WQ && rr < wrows && m0 + col + 3 < M;
            wv[u] = ld4u(wsrc + (ok ? (int64_t)rr * M + col : 0));
            if (!ok) wv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    auto commit = [&](int c0, float* X, float* A) {
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            const int m = xmask[u], nv = m & 15, sh = m >> 4;
            f32x4 v = xv[u], y = yv[u];
            if (sh) {
                const f32x4 t = v, ty = y;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = k + sh < 4 ? (k + sh == 1 ? t[1] : k + sh == 2 ? t[2] : t[3]) : 0.f;
                    y[k] = k + sh < 4 ? (k + sh == 1 ? ty[1] : k + sh == 2 ? ty[2] : ty[3]) : 0.f;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < nv ? (YM ? v[k] * lrelu_grad(y[k]) : v[k]) : 0.f;
            if (xdst[u] >= 0) *(f32x4*)(X + xdst[u]) = v;
        }
#pragma unroll
        for (int u = 0; u < MW; ++u) {
            const int j = u * NT + tid, rr = j / (BM / 4), col = (j % (BM / 4)) * 4;
            if (j < WQ && rr < (VC - c0) * JC && m0 + col + 3 >= M)
                for (int k = 0; k < 4; ++k)
                    wv[u][k] = m0 + col + k < M ? a.wp[((int64_t)c0 * JC + rr) * M + m0 + col + k] : 0.f;
            if (j < WQ) {
                if (PS && ps) {  // rows col .. col + 3 = (ci, 0), (ci, 1), (ci + 1, 0), (ci + 1, 1)
                    const int ci = col >> 1;
                    *(f32x2*)(A + rr * BM + ci) = (f32x2){wv[u][0], wv[u][2]};
                    *(f32x2*)(A + rr * BM + 32 + ci) = (f32x2){wv[u][1], wv[u][3]};
                } else {
                    *(f32x4*)(A + rr * BM + col) = wv[u];
                }
            }
        }
    };
    auto compute = [&](const float* X, const float* A) {
#pragma unroll 2
        for (int cp = 0; cp < CK; cp += 2) {
            const float* aq = A + (cp + h) * JC * BM + l32;
            const float* xq = X + (cp + h) * XR;
#pragma unroll
            for (int q = 0; q < JC; ++q) {
                float av[TM], bv[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) av[i] = aq[q * BM + i * 32];
#pragma unroll
                for (int j = 0; j < TN; ++j) bv[j] = xq[boff[j] - q];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    if (!(PS && ps && i == 1 && q == JC - 1))
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(av[i], bv[j], acc[i][j]);
            }
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < VC; c0 += CK) {
        __syncthreads();
        commit(c0, Xs, As);
        __syncthreads();
        if (c0 + CK < VC) fetch(c0 + CK);
        compute(Xs, As);
    }
    // epilogue (dgr_epi): the feature-matching term, LeakyReLU'(x), accumulate
    const bool ldx = a.xact && !(a.ffr && a.ffx == a.xact);
    const int mode = (a.ffr ? 1 : 0) | (a.xact ? 2 : 0) | (ldx ? 4 : 0) | (a.accumulate ? 8 : 0) |
                     (a.fcode && a.ffr && !ldx ? 16 : 0);
    switch (mode) {
#define ENCX_EPI(m) \
    case m: dgr_epi<TM, TN, m, PS>(a, acc, b, m0, n0 + wn0 + l32, nend, U, M, S, lane, fc, ps); break;
        ENCX_EPI(0) ENCX_EPI(1) ENCX_EPI(3) ENCX_EPI(6) ENCX_EPI(7)
        ENCX_EPI(8) ENCX_EPI(9) ENCX_EPI(11) ENCX_EPI(14) ENCX_EPI(15)
        ENCX_EPI(17) ENCX_EPI(19) ENCX_EPI(25) ENCX_EPI(27)
#undef ENCX_EPI
        default: break;
    }
}

// Backward-data, register-window form (c2_fwd_rw_kernel's scheme on c2_dgradr_kernel's
// polyphase GEMM): rows m = (ci, r) (M = Ci*S: TM tiles of 32), columns = output-column QUADS
// of the polyphase grid (t, u), rows padded to whole quads (U4 per row); lane l of a wave owns
// quad l, its 4 accumulators per row tile are the columns u0..u0+3. The k slots are two output
// channels (co = 2c + h): per (c, kt) step each lane loads ONE window of the output grad
// dy[co][t + pt - kt*dt][u0 - J + 1 .. u0 + 3] (+ the same window of y for LeakyReLU'(y)),
// which holds the operand of all J taps x 4 columns: J * 4 * TM MFMAs per step, the polyphase
// weights (staged once per workgroup in LDS, wp layout) one ds_read_b32 per tap and row tile.
// Epilogue: the feature-matching term, LeakyReLU'(x), accumulate, as c2_dgradr_kernel; the
// 2S consecutive input columns a lane holds per ci are written as quads.
struct C2DgR {
    C2Dg d;
    int U4;     // quads per polyphase row
    int tiles;  // column tiles (32 quads each): ceil(B * T2 * U4 / 32)
    C2_TRACE_ARG
};
// c2_dgrad_rw_kernel's epilogue for one item, the combination of its terms fixed at compile time
// (MODE bits: 1 feature term, 2 LeakyReLU'(x), 4 x read from xact (else from ffx), 8 accumulate),
// so the per-quad code has no branches around its loads: with them, every load sat in its own
// basic block behind a wait, one memory round trip per quad. The output never aliases the maps
// read here, so the loads of EP rows are issued together, then combined and stored.
template <int S, int TM, int MODE>
ENCX_DEV void rw_dg_epi(const C2Dg& a, const f32x16 (&acc)[TM][4], int rt, int lane, int b, int t, int u0, float fc) {
    // MODE 16: the feature term (and LeakyReLU'(ffx)) from the 1-byte pair code
    constexpr bool C = MODE & 16, F = (MODE & 1) && !C, XM = (MODE & 2) && !C, XL = MODE & 4, A = MODE & 8,
                   LX = F || XL, CX = C && (MODE & 2);
    constexpr int EP = 2;  // S == 2: ci rows (2 phases x 2 quads each) per batch; S == 1: 2 EP rows
    const C2Geo& g = a.g;
    const float* __restrict__ xs = XL ? a.xact : a.ffx;
    const float* __restrict__ rs = a.ffr;
    const uint8_t* __restrict__ cs = a.fcode;
    float* __restrict__ dx = a.dx;
    auto combine = [&](float u, float x, float r, float d, uint32_t c) {
        if (F) {
            const float e = x - r;
            u += e > 0.f ? fc : (e < 0.f ? -fc : 0.f);
        }
        if (XM) u *= lrelu_grad(x);
        if (C) u += code_term(c, fc);
        if (CX) u *= code_mask(c);
        return A ? d + u : u;
    };
    if (S == 2) {
        // TM == 2 (phase-split rows, c2_dgrad_rw_kernel): tile 0 holds phase 0 and tile 1 phase 1
        // of the same 32 ci, register r of both the same ci; otherwise registers r, r + 1 of a tile
        // are phases 0 / 1 of one ci. Either way the 4 columns give 8 consecutive f.
        constexpr bool PS = TM == 2;
        const int f = 2 * u0 - g.pf;
        const bool inb = f >= 0 && f + 8 <= g.Fi;
        if constexpr (PS && C && !LX && !F && !A) {
            // the premasked feature-code epilogue (the map's only input is its 1-byte code), for
            // EVERY lane, the ones at a row's edges included: a tile of 32 quads spans a row edge in
            // nearly every wave (33 quads per row at F 257), and such a wave then also ran the
            // per-element path below for its edge lanes, eight chunks of byte loads, a wait and
            // scalar stores each: 84 us per item against the plain epilogue's 19 at T 184 / F 257
            // (profiles/c2_items). Here the codes of a half quad are one unaligned dword loaded from
            // min(max(column, 0), Fi - 4), inside the row, and shifted into place (the bytes of
            // columns outside the row fall out or are never stored); four row pairs' loads are
            // issued together, then combined and stored: quads where the half lies inside the row,
            // single elements at the edges. The rows of a lane are row_stride apart.
            {
                typedef uint32_t u32u __attribute__((aligned(1)));
                const int64_t orow = (((int64_t)b * g.Ci + mfma_row(0, lane)) * g.T2 + t) * g.Fi;
                const int64_t row_stride = (int64_t)g.T2 * g.Fi;
                int cl[2], sh[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    cl[h] = min(max(f + 4 * h, 0), g.Fi - 4);
                    sh[h] = f + 4 * h - cl[h];  // 0: the half lies inside the row
                }
#pragma unroll
                for (int hb = 0; hb < 16; hb += 4 * EP) {
                    uint32_t cw[4 * EP][2];
#pragma unroll
                    for (int j = 0; j < 4 * EP; ++j)
#pragma unroll
                        for (int h = 0; h < 2; ++h)
                            cw[j][h] = *(const u32u*)(cs + orow + (mfma_row(hb + j, 0) - mfma_row(0, 0)) * row_stride + cl[h]);
#pragma unroll
                    for (int j = 0; j < 4 * EP; ++j)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int r = hb + j, n = sh[h];
                            const uint32_t c4 = n == 0 ? cw[j][h]
                                                : n > 0 ? (n < 4 ? cw[j][h] >> (8 * n) : 0u)
                                                        : (n > -4 ? cw[j][h] << (-8 * n) : 0u);
                            f32x4 s4;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int e8 = 4 * h + e;
                                s4[e] = combine(acc[e8 & 1][e8 >> 1][r], 0.f, 0.f, 0.f, (c4 >> (8 * e)) & 255u);
                            }
                            float* dr = dx + orow + (mfma_row(r, 0) - mfma_row(0, 0)) * row_stride + f + 4 * h;
                            if (n == 0) {
                                *(f32x4u*)dr = s4;
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (f + 4 * h + e >= 0 && f + 4 * h + e < g.Fi) dr[e] = s4[e];
                            }
                        }
                }
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < (PS ? 1 : TM); ++i)
#pragma unroll
            for (int r0 = 0; r0 < 16; r0 += PS ? EP : 2 * EP) {
                int64_t o[EP];
#pragma unroll
                for (int p = 0; p < EP; ++p) {
                    const int ci = PS ? mfma_row(r0 + p, lane) : ((rt * TM + i) * 32 + mfma_row(r0 + 2 * p, lane)) >> 1;
                    o[p] = (((int64_t)b * g.Ci + ci) * g.T2 + t) * g.Fi + f;
                }
                auto val = [&](int p, int e8) {
                    return PS ? acc[e8 & 1][e8 >> 1][r0 + p] : acc[i][e8 >> 1][r0 + 2 * p + (e8 & 1)];
                };
                if (inb) {
                    f32x4 X[EP][2], R[EP][2], D[EP][2];
                    uint32_t Cc[EP][8];
#pragma unroll
                    for (int p = 0; p < EP; ++p) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            if (LX) X[p][h] = ld4u(xs + o[p] + 4 * h);
                            if (F) R[p][h] = ld4u(rs + o[p] + 4 * h);
                            if (A) D[p][h] = ld4u(dx + o[p] + 4 * h);
                        }
                        if (C) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) Cc[p][e] = cs[o[p] + e];
                        }
                    }
#pragma unroll
                    for (int p = 0; p < EP; ++p)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            f32x4 s4;
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                s4[e] = combine(val(p, 4 * h + e), LX ? X[p][h][e] : 0.f, F ? R[p][h][e] : 0.f,
                                                A ? D[p][h][e] : 0.f, C ? Cc[p][4 * h + e] : 0u);
                            *(f32x4u*)(dx + o[p] + 4 * h) = s4;
                        }
                } else {
#pragma unroll
                    for (int p = 0; p < EP; ++p)
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (f + e >= 0 && f + e < g.Fi) {
                                const int64_t q = o[p] + e;
                                dx[q] = combine(val(p, e), LX ? xs[q] : 0.f, F ? rs[q] : 0.f, A ? dx[q] : 0.f,
                                                C ? (uint32_t)cs[q] : 0u);
                            }
                }
            }
    } else {
        const int f = u0 - g.pf;
        const bool inb = f >= 0 && f + 4 <= g.Fi;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r0 = 0; r0 < 16; r0 += 2 * EP) {
                int64_t o[2 * EP];
#pragma unroll
                for (int p = 0; p < 2 * EP; ++p) {
                    const int ci = (rt * TM + i) * 32 + mfma_row(r0 + p, lane);
                    o[p] = (((int64_t)b * g.Ci + ci) * g.T2 + t) * g.Fi + f;
                }
                if (inb) {
                    f32x4 X[2 * EP], R[2 * EP], D[2 * EP];
                    uint32_t Cc[2 * EP][4];
#pragma unroll
                    for (int p = 0; p < 2 * EP; ++p) {
                        if (LX) X[p] = ld4u(xs + o[p]);
                        if (F) R[p] = ld4u(rs + o[p]);
                        if (A) D[p] = ld4u(dx + o[p]);
                        if (C) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) Cc[p][e] = cs[o[p] + e];
                        }
                    }
#pragma unroll
                    for (int p = 0; p < 2 * EP; ++p) {
                        f32x4 s4;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            s4[e] = combine(acc[i][e][r0 + p], LX ? X[p][e] : 0.f, F ? R[p][e] : 0.f, A ? D[p][e] : 0.f,
                                            C ? Cc[p][e] : 0u);
                        *(f32x4u*)(dx + o[p]) = s4;
                    }
                } else {
#pragma unroll
                    for (int p = 0; p < 2 * EP; ++p)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (f + e >= 0 && f + e < g.Fi) {
                                const int64_t q = o[p] + e;
                                dx[q] = combine(acc[i][e][r0 + p], LX ? xs[q] : 0.f, F ? rs[q] : 0.f, A ? dx[q] : 0.f,
                                                C ? (uint32_t)cs[q] : 0u);
                            }
                }
            }
    }
}

template <int J, int S, int RT, int WQ, bool YM, int NWV, int TM>
__global__ __launch_bounds__(NWV * 64) void c2_dgrad_rw_kernel(C2DgR R) {
    // RT row tiles of 32 (M = Ci*S = 32 RT); a work item is (column tile, TM row tiles); the
    // weight columns are read from LDS just in time (measured against reading them a step ahead,
    // one tap ahead, and one row tile per item: none is faster, profiles/r05)
    constexpr int NE = 4 * WQ, KT = 3, M = 32 * RT, RG = RT / TM;
    const C2Dg& a = R.d;
    extern __shared__ float smem[];
    const C2Geo g = a.g;
    const int tslot = blockIdx.x * NWV + (threadIdx.x >> 6);  // (trace builds only)
    int titem = 0;
    (void)titem;
    C2_TRACE(R.tr, tslot, 0);
    // phase-split rows (the 3x9 stride-2 layers with both row tiles per item): tile 0 = phase 0,
    // tile 1 = phase 1 of the 32 ci, so the fifth polyphase tap, zero for every phase-1 row
    // (kf = 2 q + 1 = 9 >= KF), is skipped for tile 1: 10 % fewer MFMAs
    constexpr bool PS = S == 2 && J == 5 && RT == 2 && TM == 2;
    float* As = smem;  // [(co,kt)][J][M]: the wp layout (M == Ci*S, host-checked), rows phase-major if PS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, l = lane & 31;
    // element offsets fit in 32 bits (checked on the host)
    const int quads = g.B * g.T2 * R.U4;
    const int plane = g.T2 * g.Fo, ylast = g.B * g.Co * plane - 4;
    const int CP = g.Co >> 1, cstride = 2 * plane;
    const float fc = feat_coef(a);
    // one item's geometry: window element e of step (c, kt) is dy[b][2c + h][row(kt)][e0 + e]
    struct Geo {
        int rt, tile, t, b, u0;
        int rb[KT];
        uint32_t msk[KT];
        bool fix;  // wave-uniform: some lane's window leaves the map
    };
    auto geo = [&](int item) {
        Geo q;
        q.rt = item % RG;
        q.tile = item / RG;  // rows rt*TM*32 .. + TM*32
        const int qd = min(q.tile * 32 + l, quads - 1);
        const int uq = qd % R.U4, bt = qd / R.U4;
        q.t = bt % g.T2;
        q.b = bt / g.T2;
        q.u0 = 4 * uq;
        const int e0 = q.u0 - (J - 1);  // dy column of window element 0
        uint32_t cmask = 0;
#pragma unroll
        for (int e = 0; e < NE; ++e) cmask |= (e0 + e >= 0 && e0 + e < g.Fo) ? (1u << e) : 0u;
        bool clean = true;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            const int row = q.t + g.pt - kt * g.dt;
            const bool ok = row >= 0 && row < g.T2;
            q.rb[kt] = (q.b * g.Co + h) * plane + (ok ? row : 0) * g.Fo + e0;
            q.msk[kt] = ok ? cmask : 0u;
            clean = clean && q.msk[kt] == (1u << NE) - 1;
        }
        q.fix = !__all(clean);
        return q;
    };
    // two register buffers of windows, alternating over the (c, kt) steps: step s + 1 is in
    // flight while step s multiplies. The loop body is 2 channel pairs x 3 kt = 6 steps, so
    // every buffer / kt index is a compile-time constant (Co % 4 == 0). The last step of an item
    // loads the NEXT item's first window, so it is in flight during this item's epilogue and the
    // next item does not start by waiting out a round trip behind the epilogue's stores.
    f32x4 wb[2][WQ], yb[2][WQ];
    auto load = [&](int k, const Geo& q, int c, int kt) {
        const int base = q.rb[kt] + c * cstride;
#pragma unroll
        for (int w4 = 0; w4 < WQ; ++w4) {
            const int o = min(max(base + 4 * w4, 0), ylast);
            wb[k][w4] = ld4u(a.dy + o);
            if (YM) yb[k][w4] = ld4u(a.yact + o);
        }
    };
    const int stride = gridDim.x * NWV, nitems = R.tiles * RG;
    int item = rw_first_slot(wave);
    // the first item's window goes out ahead of the weights, so it arrives under their staging
    if (item < nitems) load(0, geo(item), 0, 0);
    // the weights, once per workgroup: wp copied as quads, RW_SQ of them in flight per thread ahead
    // of their LDS writes (one memory round trip for the 3x9 layers' 120 KB at 512 threads; loaded
    // dword by dword, eight in flight, it was eight). Phase-split rows: the quad (ci, 0), (ci, 1),
    // (ci + 1, 0), (ci + 1, 1) of wp goes to columns ci, ci + 1 of tile 0 and of tile 1.
    {
        const int nq = g.Co * KT * J * (M / 4);
        for (int i0 = 0; i0 < nq; i0 += NWV * 64 * RW_SQ) {
            f32x4 sv[RW_SQ];
#pragma unroll
            for (int u = 0; u < RW_SQ; ++u)
                sv[u] = ld4u(a.wp + 4 * min(i0 + u * NWV * 64 + (int)threadIdx.x, nq - 1));
#pragma unroll
            for (int u = 0; u < RW_SQ; ++u) {
                const int i = i0 + u * NWV * 64 + (int)threadIdx.x;
                if (i >= nq) continue;
                if (PS) {
                    const int col = (4 * i) % M, ci = col >> 1;
                    *(f32x2*)(As + 4 * i - col + ci) = (f32x2){sv[u][0], sv[u][2]};
                    *(f32x2*)(As + 4 * i - col + 32 + ci) = (f32x2){sv[u][1], sv[u][3]};
                } else {
                    *(f32x4*)(As + 4 * i) = sv[u];
                }
            }
        }
    }
    __syncthreads();
    C2_TRACE(R.tr, tslot, 1);
    for (; item < nitems; item += stride) {
        const Geo cur = geo(item);  // (recomputed: cheaper than holding the next item's in registers)
        const int rt = cur.rt, tile = cur.tile, t = cur.t, b = cur.b, u0 = cur.u0;
        auto acol = [&](int c, int kt) { return As + ((2 * c + h) * KT + kt) * J * M + rt * TM * 32 + l; };
        f32x16 acc[TM][4];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x16){0};
        C2_TRACE(R.tr, tslot, 3 + 3 * titem);
        for (int c0 = 0; c0 < CP; c0 += 2) {
#pragma unroll
            for (int u = 0; u < 2 * KT; ++u) {
                const int kt = u % KT, c = c0 + u / KT, k = u & 1;
                // the next step: within the item, or the next item's first (past the last item
                // its own first again, never used)
                const int nu = u + 1 < 2 * KT ? u + 1 : 0;
                if (u + 1 < 2 * KT || c0 + 2 < CP) load(k ^ 1, cur, u + 1 < 2 * KT ? c0 + nu / KT : c0 + 2, nu % KT);
                else load(k ^ 1, geo(item + stride < nitems ? item + stride : item), 0, 0);
                // keep the next step's loads HERE, a whole step ahead of their use: without the
                // barrier the scheduler sinks them to the end of the step (one register buffer
                // instead of two) and every step waits out the load latency (measured: the
                // round-3 kernel without it is slower, profiles/r05)
                __builtin_amdgcn_sched_barrier(0);
                f32x4* w = wb[k];
                if (YM) {
#pragma unroll
                    for (int q = 0; q < WQ; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[q][e] *= lrelu_grad(yb[k][q][e]);
                }
                if (cur.fix) {
                    const int base = cur.rb[kt] + c * cstride;
#pragma unroll
                    for (int q = 0; q < WQ; ++q) {
                        const int o = base + 4 * q;
                        if (__any(o < 0 || o > ylast)) w[q] = quad_abs(w[q], o, ylast);  // tensor ends
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (!((cur.msk[kt] >> (4 * q + e)) & 1u)) w[q][e] = 0.f;
                    }
                }
                const float* ak = acol(c, kt);
#pragma unroll
                for (int q = 0; q < J; ++q) {
                    float av[TM];
#pragma unroll
                    for (int i = 0; i < TM; ++i) av[i] = (PS && i == 1 && q == J - 1) ? 0.f : ak[q * M + i * 32];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = j - q + J - 1;  // window element of column u0 + j, tap q
#pragma unroll
                        for (int i = 0; i < TM; ++i)
                            if (!(PS && i == 1 && q == J - 1)) acc[i][j] = mfma32(av[i], w[r >> 2][r & 3], acc[i][j]);
                    }
                }
            }
        }
        C2_TRACE(R.tr, tslot, 4 + 3 * titem);
        // ---- epilogue (rw_dg_epi): the feature-matching term, LeakyReLU'(x), accumulate
        const bool live = tile * 32 + l < quads;
        const bool ldx = a.xact && !(a.ffr && a.ffx == a.xact);  // x from xact (else from ffx)
        const int mode = (a.ffr ? 1 : 0) | (a.xact ? 2 : 0) | (ldx ? 4 : 0) | (a.accumulate ? 8 : 0) |
                         (a.fcode && a.ffr && !ldx ? 16 : 0);
        switch (mode) {
#define ENCX_EPI(m) \
    case m: if (live) rw_dg_epi<S, TM, m>(a, acc, rt, lane, b, t, u0, fc); break;
            ENCX_EPI(0) ENCX_EPI(1) ENCX_EPI(3) ENCX_EPI(6) ENCX_EPI(7)
            ENCX_EPI(8) ENCX_EPI(9) ENCX_EPI(11) ENCX_EPI(14) ENCX_EPI(15)
            ENCX_EPI(17) ENCX_EPI(19) ENCX_EPI(25) ENCX_EPI(27)
#undef ENCX_EPI
            default: break;  // (xact without its own load needs ffr: modes 2, 10 do not occur)
        }
        C2_TRACE(R.tr, tslot, 5 + 3 * titem);
        ++titem;
        C2_TRACE_VAL(R.tr, tslot, 2, titem);
    }
}

// Narrow backward-data (M = Ci <= 4 rows, stride 1 along f: the first layer's grad into the
// spectrogram). A 32-row MFMA tile would carry 2 useful rows, so this runs on the vector ALU:
// a workgroup owns 16 t rows x 64 f columns of one batch item; the masked output grad for
// NC_CO channels is staged in LDS with its (KT-1)*dt row and KF-1 column halo; a thread keeps
// CI x 4 accumulators for 4 adjacent f and slides a 4+KF-1 window over its LDS row per tap;
// the weights are wave-uniform (scalar loads).
#ifndef ENCX_DN_QP
#define ENCX_DN_QP 4  // staging quads in flight per thread and tensor (compile-time A/B knob)
#endif
constexpr int DN_ROWS = 16, DN_COLS = 64, DN_FPT = 4, DN_CC = 8, DN_MAXHALO = 4;
// DT: the time dilation at compile time (the staging's index splits then divide by constants:
// with a runtime row count they were integer divisions, and the staging's VALU work rivalled the
// FMAs'); interior quads (the whole quad inside the row) skip the edge shift / mask.
template <int CI, int KT, int KF, bool YM = true, int DT = 1>
__global__ __launch_bounds__(NT) void c2_dgrad_narrow(C2Dg a) {
    constexpr int RC = (DN_COLS + KF - 1 + 3) & ~3;  // LDS row length (float4 aligned)
    constexpr int WIN4 = (DN_FPT + KF - 1 + 3) / 4;
    __shared__ float Xs[DN_CC * (DN_ROWS + DN_MAXHALO) * RC];
    const C2Geo g = a.g;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int f0 = blockIdx.x * DN_COLS, t0 = blockIdx.y * DN_ROWS, b = blockIdx.z;
    constexpr int halo = (KT - 1) * DT, NRW = DN_ROWS + halo;
    const int tbase = t0 + g.pt - halo, fbase = f0 + g.pf - (KF - 1);
    const int64_t plane = (int64_t)g.T2 * g.Fo;
    const float* dyb = a.dy + (int64_t)b * g.Co * plane;
    const float* yab = YM ? a.yact + (int64_t)b * g.Co * plane : dyb;
    // accumulators as (ci, ci + 1) pairs: one packed FMA (v_pk_fma_f32, the weight pair from
    // SGPRs) per two channels
    static_assert(CI % 2 == 0, "channel pairs");
    f32x2 acc[CI / 2][DN_FPT];
#pragma unroll
    for (int c = 0; c < CI / 2; ++c)
#pragma unroll
        for (int e = 0; e < DN_FPT; ++e) acc[c][e] = (f32x2){0.f, 0.f};
    // the tile is staged as quads along f (ld4u; lanes outside [0, Fo) or outside the
    // tensor masked), one index split per 4 elements instead of per element
    constexpr int RQ = RC / 4, QP = ENCX_DN_QP;
    constexpr int nq = DN_CC * NRW * RQ;
    const int64_t left = (int64_t)(g.B - b) * g.Co * plane;  // floats from dyb to the tensor end
    for (int c0 = 0; c0 < g.Co; c0 += DN_CC) {
        __syncthreads();
        for (int i0 = 0; i0 < nq; i0 += NT * QP) {
            f32x4 v[QP], ym[QP];
            int mk[QP];
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                const int i = i0 + q * NT + tid;
                const int cl = i / (NRW * RQ), rem = i - cl * (NRW * RQ), r = rem / RQ, cq = rem - r * RQ;
                const int tr = tbase + r, fc = fbase + 4 * cq;
                const bool ok = i < nq && c0 + cl < g.Co && tr >= 0 && tr < g.T2 && fc + 4 > 0 && fc < g.Fo;
                const int64_t o = ok ? (int64_t)(c0 + cl) * plane + (int64_t)tr * g.Fo + fc : 0;
                int64_t oc = o < 0 ? 0 : o;
                if (oc > left - 4) oc = left - 4;
                v[q] = ld4u(dyb + oc);
                if (YM) ym[q] = ld4u(yab + oc);
                // lanes [lo, hi) hold columns inside [0, Fo); sh = the shift of a clamped load
                const int lo = fc < 0 ? -fc : 0, hi = min(g.Fo - fc, 4), sh = (int)(o - oc);
                // 1: the plain quad (inside the row and the tensor), no shift or mask
                mk[q] = ok ? ((lo == 0 && hi == 4 && sh == 0) ? 1 : (lo | (hi << 4) | ((sh + 4) << 8))) : 0;
            }
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                const int i = i0 + q * NT + tid;
                if (i >= nq) continue;
                const int m = mk[q];
                if (m == 1) {
                    f32x4 u = v[q];
                    if (YM)
#pragma unroll
                        for (int k = 0; k < 4; ++k) u[k] *= lrelu_grad(ym[q][k]);
                    *(f32x4*)(Xs + i * 4) = u;
                    continue;
                }
                const int lo = m & 15, hi = (m >> 4) & 15, sh = (m >> 8) - 4;
                f32x4 t = v[q], ty = ym[q], u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int src = k + sh;  // lane of the loaded quad holding column fc + k
                    float dv = 0.f, yv = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (src == j) {
                            dv = t[j];
                            if (YM) yv = ty[j];
                        }
                    const bool in = m && k >= lo && k < hi && src >= 0 && src < 4;
                    u[k] = in ? (YM ? dv * lrelu_grad(yv) : dv) : 0.f;
                }
                *(f32x4*)(Xs + i * 4) = u;
            }
        }
        __syncthreads();
        for (int cl = 0; cl < DN_CC; ++cl) {
            const int co = c0 + cl;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const float* row = Xs + (cl * NRW + ty + (KT - 1 - kt) * DT) * RC + 4 * tx;
                float win[WIN4 * 4];
#pragma unroll
                for (int j = 0; j < WIN4; ++j) {
                    const f32x4 t = *(const f32x4*)(row + 4 * j);
                    win[4 * j] = t[0];
                    win[4 * j + 1] = t[1];
                    win[4 * j + 2] = t[2];
                    win[4 * j + 3] = t[3];
                }
                const float* wr = a.wp + (int64_t)(co * KT + kt) * KF * CI;
#pragma unroll
                for (int kf = 0; kf < KF; ++kf)
#pragma unroll
                    for (int c = 0; c < CI / 2; ++c) {
                        const f32x2 w = {wr[kf * CI + 2 * c], wr[kf * CI + 2 * c + 1]};
#pragma unroll
                        for (int e = 0; e < DN_FPT; ++e) {
                            const float xv = win[e + KF - 1 - kf];
                            acc[c][e] = __builtin_elementwise_fma(w, (f32x2){xv, xv}, acc[c][e]);
                        }
                    }
            }
        }
    }
    const int t = t0 + ty;
    if (t >= g.T2) return;
#pragma unroll
    for (int c = 0; c < CI; ++c)
#pragma unroll
        for (int e = 0; e < DN_FPT; ++e) {
            const int f = f0 + 4 * tx + e;
            if (f >= g.Fi) continue;
            const int64_t o = (((int64_t)b * CI + c) * g.T2 + t) * g.Fi + f;
            float v = acc[c / 2][e][c % 2];
            if (a.ffr) v += feat_term(a, feat_coef(a), o);
            if (a.xact) v *= lrelu_grad(a.xact[o]);
            a.dx[o] = a.accumulate ? a.dx[o] + v : v;
        }
}

// wp[(co,kt)][q][ci*S + r] = W[co][ci][kt][q*S + r] from wf[((ci,kt))*KF + kf][co]
__global__ void c2_wpoly_kernel(const float* wf, float* wp, int Co, int Ci, int KT, int KF, int S, int J) {
    const int64_t total = (int64_t)Co * KT * J * Ci * S;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int M = Ci * S;
    const int m = (int)(i % M);
    const int64_t rq = i / M;
    const int q = (int)(rq % J), vc = (int)(rq / J);
    const int co = vc / KT, kt = vc - co * KT;
    const int ci = m / S, r = m - ci * S, kf = q * S + r;
    wp[i] = kf < KF ? wf[(((int64_t)ci * KT + kt) * KF + kf) * Co + co] : 0.f;
}

// Single output channel (Co = 1, the VALU kernels described at c2_co1_fwd):
// dx[b][ci][ti][fi] = sum_{kt,kf} W[ci][kt][kf] * dy'[b][ti - kt*dt + pt][(fi - kf + pf)/S]
// (terms whose output column is fractional or out of range drop), dy' = dy * LeakyReLU'(yact).
// Block = 64 columns x 4 rows of one (b, ci) plane.
// CPT input channels per thread share the KT*KF loads of dy' (blockIdx.y = (b, channel group));
// per channel the taps are summed in the same order as one channel per thread.
template <int KT, int KF, int S, int CPT = 1>
__global__ __launch_bounds__(256) void c2_co1_dgrad(C2Dg a) {
    const C2Geo g = a.g;
    const int xplane = g.T2 * g.Fi, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= xplane) return;
    const int ti = p / g.Fi, fi = p - ti * g.Fi;
    const int groups = g.Ci / CPT, b = blockIdx.y / groups, ci0 = (blockIdx.y - b * groups) * CPT;
    const int64_t plane = (int64_t)g.T2 * g.Fo;
    const float* dyb = a.dy + (int64_t)b * plane;
    const float* yab = a.yact ? a.yact + (int64_t)b * plane : dyb;
    const int M = g.Ci * S;
    float dv[KT * KF];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        const int to = ti - kt * g.dt + g.pt;
        const bool rok = to >= 0 && to < g.T2;
#pragma unroll
        for (int kf = 0; kf < KF; ++kf) {
            const int fs = fi - kf + g.pf;
            const int fo = fs / S;  // S is 1 or 2: a shift
            const bool ok = rok && fs >= 0 && (S == 1 || fs % S == 0) && fo < g.Fo;
            const int64_t o = ok ? (int64_t)to * g.Fo + fo : 0;
            float d = dyb[o];
            if (a.yact) d *= lrelu_grad(yab[o]);
            dv[kt * KF + kf] = ok ? d : 0.f;
        }
    }
    const float fc = feat_coef(a);
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        const int ci = ci0 + c;
        float acc = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int kf = 0; kf < KF; ++kf)
                acc = fmaf(a.wp[(kt * a.J + kf / S) * M + ci * S + kf % S], dv[kt * KF + kf], acc);
        const int64_t i = ((int64_t)b * g.Ci + ci) * xplane + p;
        if (a.ffr) acc += feat_term(a, fc, i);
        if (a.xact) acc *= lrelu_grad(a.xact[i]);
        a.dx[i] = a.accumulate ? a.dx[i] + acc : acc;
    }
}

// ---------------------------------------------------------------------------- planning
template <int BM, int BN, int WM, int WN, int JC = 0>
int launch_dgrad(C2Dg a, hipStream_t st) {
    const size_t lds = ((size_t)a.CK * a.NR * a.RL + (size_t)a.J * a.CK * BM +
                        (size_t)2 * a.g.Co * a.g.KT * a.NR + 2) * sizeof(float);
    dim3 grid((unsigned)cdiv((int64_t)a.g.T2 * a.U, BN), (unsigned)cdiv(a.g.Ci * a.g.sf, BM), (unsigned)a.g.B);
    hipLaunchKernelGGL((c2_dgrad_kernel<BM, BN, WM, WN, JC>), grid, dim3(NT), lds, st, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

template <int BM, int BN, int WM, int WN, int JC = 0>
int run_dgrad(C2Dg a, hipStream_t st, int budget = 12288) {
    a.J = (int)cdiv(a.g.KF, a.g.sf);
    a.U = (a.g.Fi - 1 + a.g.pf) / a.g.sf + 1;
    a.NR = c2_rows(BN, a.U);
    a.RL = min(BN, a.U) - 1 + a.J;
    a.CK = c2_ck(a.g.Co * a.g.KT, a.NR * a.RL + a.J * BM, budget);
    return launch_dgrad<BM, BN, WM, WN, JC>(a, st);
}

// register-window backward-data (c2_dgrad_rw_kernel): 3x9 stride 2 (M = 64) and 3x3 stride 1
// (M = 32) layers with Co % 4 == 0; the polyphase weights in LDS
static bool dgr_ok(const C2Geo& g) {
    if ((g.Co & 3) || g.KT != 3 || g.Fi < 4 || g.Fo < 4) return false;
    if (!((g.KF == 9 && g.sf == 2 && g.Ci == 32) || (g.KF == 3 && g.sf == 1 && g.Ci == 32))) return false;
    if ((int64_t)g.B * g.Co * g.T2 * g.Fo >= (1ll << 31) - 64) return false;
    const int J = (g.KF + g.sf - 1) / g.sf;
    return (size_t)g.Co * 3 * J * g.Ci * g.sf * sizeof(float) <= 150 * 1024;
}
static void launch_dgrad_rw(const C2DgR& R, int grid, size_t lds, hipStream_t st) {
    constexpr int NWV = 8;
    const bool ym = R.d.yact != nullptr;
    if (R.d.g.KF == 9) {
        if (ym) hipLaunchKernelGGL((c2_dgrad_rw_kernel<5, 2, 2, 2, true, NWV, 2>), dim3(grid), dim3(NWV * 64), lds, st, R);
        else hipLaunchKernelGGL((c2_dgrad_rw_kernel<5, 2, 2, 2, false, NWV, 2>), dim3(grid), dim3(NWV * 64), lds, st, R);
    } else {
        if (ym) hipLaunchKernelGGL((c2_dgrad_rw_kernel<3, 1, 1, 2, true, NWV, 1>), dim3(grid), dim3(NWV * 64), lds, st, R);
        else hipLaunchKernelGGL((c2_dgrad_rw_kernel<3, 1, 1, 2, false, NWV, 1>), dim3(grid), dim3(NWV * 64), lds, st, R);
    }
}
// 8 waves per workgroup, items of both row tiles of the 3x9 layers (TM = 2). Measured and
// dropped (round 5): a half-full last round of items handed to a second launch as one-row-tile
// items (TM = 1, twice the items at half the work): 799.0 vs 802.0 audio-s/s.
static int run_dgrad_rw(const C2Dg& d, int wgs, hipStream_t st) {
    if (!dgr_ok(d.g)) return ENCX_EINVAL;
    constexpr int NWV = 8;
    const C2Geo& g = d.g;
    C2DgR R{d, 0, 0};
    R.d.U = (g.Fi - 1 + g.pf) / g.sf + 1;
    R.U4 = (int)cdiv(R.d.U, 4);
    const int tiles = (int)cdiv((int64_t)g.B * g.T2 * R.U4, 32);
    const int J = (g.KF + g.sf - 1) / g.sf;
    const size_t lds = (size_t)g.Co * 3 * J * g.Ci * g.sf * sizeof(float);
    const int grid = (int)min((int64_t)wgs, cdiv((int64_t)tiles, NWV));
    R.tiles = tiles;
    C2_TRACE_SET(R);
    launch_dgrad_rw(R, grid, lds, st);
    ENCX_CHECK_LAUNCH();
    return 0;
}

template <int TM, int BN, int JC, int MQ, int CKM, int OCC = 1>
int run_dgradr(C2Dg a, hipStream_t st) {
    a.J = (int)cdiv(a.g.KF, a.g.sf);
    a.U = (a.g.Fi - 1 + a.g.pf) / a.g.sf + 1;
    a.NR = c2_rows(BN, a.U);
    a.RL = min(BN, a.U) - 1 + a.J + 3;
    a.CK = quad_ck(a.g.Co * a.g.KT, a.NR, a.RL, MQ, CKM);
    if (a.J != JC || a.CK < 2 || a.g.Fo < 4 || JC > 5 || a.g.Ci * a.g.sf > 32 * TM) return ENCX_EINVAL;
    const int RLp = (a.RL + 3) & ~3;
    const size_t lds = ((size_t)a.CK * a.NR * RLp + (size_t)JC * a.CK * 32 * TM +
                        (size_t)2 * a.g.Co * a.g.KT * a.NR) * sizeof(float);
    dim3 grid((unsigned)cdiv((int64_t)a.g.T2 * a.U, BN), 1, (unsigned)a.g.B);
    if (a.yact) hipLaunchKernelGGL((c2_dgradr_kernel<TM, BN, JC, MQ, CKM, OCC, true>), grid, dim3(NT), lds, st, a);
    else hipLaunchKernelGGL((c2_dgradr_kernel<TM, BN, JC, MQ, CKM, OCC, false>), grid, dim3(NT), lds, st, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

/* The polyphase weights wp of a layer from its forward layout wf (c2_wpoly_kernel). */
int encx_conv2d_wpoly(const float* wf, float* wp, int64_t Co, int64_t Ci, int64_t KT, int64_t KF, int64_t sf,
                      encx_stream_t stream) {
    ENCX_REQUIRE(wf && wp && Co > 0 && Ci > 0 && KT > 0 && KF > 0 && sf > 0);
    const int J = (int)cdiv(KF, sf);
    const int64_t total = Co * KT * J * Ci * sf;
    hipLaunchKernelGGL(c2_wpoly_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, wf,
                       wp, (int)Co, (int)Ci, (int)KT, (int)KF, (int)sf, J);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_conv2d_bwd_data(const float* dy, const float* yact, const float* wp, const float* xact, float* dx,
                         int accumulate, int64_t B, int64_t Ci, int64_t T2, int64_t Fi, int64_t Co, int64_t Fo,
                         int64_t KT, int64_t KF, int64_t sf, int64_t dt, int64_t pt, int64_t pf,
                         encx_stream_t stream) {
    return encx_conv2d_bwd_data_feat(dy, yact, wp, xact, dx, accumulate, nullptr, nullptr, nullptr, nullptr, 0.0,
                                     nullptr, B,
                                     Ci, T2, Fi, Co, Fo, KT, KF, sf, dt, pt, pf, stream);
}

int encx_conv2d_bwd_data_feat(const float* dy, const float* yact, const float* wp, const float* xact, float* dx,
                              int accumulate, const float* feat_real, const float* feat_fake, const float* feat_denom,
                              const float* feat_g, double feat_scale, const uint8_t* feat_code, int64_t B, int64_t Ci,
                              int64_t T2, int64_t Fi, int64_t Co, int64_t Fo, int64_t KT, int64_t KF, int64_t sf,
                              int64_t dt, int64_t pt, int64_t pf, encx_stream_t stream) {
    ENCX_REQUIRE(dy && wp && dx);
    ENCX_REQUIRE(!feat_real || (feat_fake && feat_denom));
    // the epilogues with a feature term take sign(x - feat_real) from the map they load as x: the
    // xact map when there is one (the compile-time epilogues dgr_epi / rw_dg_epi), so it must BE
    // the fake map
    ENCX_REQUIRE(!feat_real || !xact || xact == feat_fake);
    C2Geo g{(int)B, (int)Ci, (int)T2, (int)Fi, (int)Co, (int)Fo, (int)KT, (int)KF, (int)sf, (int)dt, (int)pt, (int)pf};
    ENCX_REQUIRE(geo_ok(g));
    hipStream_t st = (hipStream_t)stream;
    encx_prof_scope ps(st, 2.0 * B * Co * T2 * Fo * Ci * KT * KF,
                       4.0 * (B * Ci * T2 * Fi * (feat_real ? 3 : 1) + 2 * B * Co * T2 * Fo), "c2_dgrad");
    ps.tag(" %ldx%ld %ldx%ld s%ld T%ld F%ld", (long)Ci, (long)Co, (long)KT, (long)KF, (long)sf, (long)T2, (long)Fo);
    C2Dg a{g, dy, yact, wp, xact, dx, 0, 0, 0, 0, 0, accumulate, feat_real, feat_fake, feat_denom, feat_g,
           (float)feat_scale, feat_real && encx_opt(OPT_FEAT_CODE) ? feat_code : nullptr};
    a.J = (int)cdiv(KF, sf);              // c2_co1_dgrad's tap stride in wp
    a.U = (int)((Fi - 1 + pf) / sf + 1);  // polyphase columns per row (the family choice below)
    const int M = (int)(Ci * sf);
    if (Co == 1 && KT == 3 && KF == 3 && (sf == 1 || sf == 2)) {
        dim3 grid((unsigned)cdiv(T2 * Fi, 256), (unsigned)(B * Ci));
        if (Ci % 4 == 0) {
            const dim3 g4((unsigned)cdiv(T2 * Fi, 256), (unsigned)(B * Ci / 4));
            if (sf == 1) hipLaunchKernelGGL((c2_co1_dgrad<3, 3, 1, 4>), g4, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((c2_co1_dgrad<3, 3, 2, 4>), g4, dim3(256), 0, st, a);
        } else if (sf == 1) hipLaunchKernelGGL((c2_co1_dgrad<3, 3, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((c2_co1_dgrad<3, 3, 2>), grid, dim3(256), 0, st, a);
        ENCX_CHECK_LAUNCH();
        return 0;
    }
    // register-window form (c2_dgrad_rw_kernel); option DGR = workgroups (0: off)
    const int dg_wgs = (int)encx_opt(OPT_DGR);
    if (dg_wgs > 0 && dgr_ok(g) && rw_pays(cdiv(B * T2 * cdiv(a.U, 4), 32), B * T2 * a.U, 92.0 / 78.0) &&
        run_dgrad_rw(a, dg_wgs, st) == 0)
        return 0;
    // tile choice from tools/mb/c2_mb sweeps: 128-column tiles for the narrowest layers (Fo 33;
    // at Fo 65 the 256-column tile is 4-7 % faster), 8-combo
    // chunks + a 3-waves/SIMD register cap for the wide ones
    if (M == 64 && KF == 9 && sf == 2) {
        if (Fo <= 33 ? run_dgradr<2, 128, 5, 4, 16, 3>(a, st) == 0 : run_dgradr<2, 256, 5, 4, 8, 3>(a, st) == 0)
            return 0;
    }
    if (M <= 32 && KF == 3 && sf == 1 && run_dgradr<1, 256, 3, 6, 32>(a, st) == 0) return 0;
    if (sf == 1 && KT == 3 && KF == 9 && (Ci == 2 || Ci == 4) && Co % DN_CC == 0 && (KT - 1) * dt <= DN_MAXHALO) {
        dim3 grid((unsigned)cdiv(Fi, DN_COLS), (unsigned)cdiv(T2, DN_ROWS), (unsigned)B);
#define ENCX_DN(ci, ym, dt) hipLaunchKernelGGL((c2_dgrad_narrow<ci, 3, 9, ym, dt>), grid, dim3(NT), 0, st, a)
        if (dt == 1) {
            if (Ci == 2 && yact) ENCX_DN(2, true, 1);
            else if (Ci == 2) ENCX_DN(2, false, 1);
            else if (yact) ENCX_DN(4, true, 1);
            else ENCX_DN(4, false, 1);
        } else {
            if (Ci == 2 && yact) ENCX_DN(2, true, 2);
            else if (Ci == 2) ENCX_DN(2, false, 2);
            else if (yact) ENCX_DN(4, true, 2);
            else ENCX_DN(4, false, 2);
        }
#undef ENCX_DN
        ENCX_CHECK_LAUNCH();
        return 0;
    }
    if (M <= 32) return run_dgrad<32, 128, 1, 4>(a, st);
    return run_dgrad<64, 128, 2, 2>(a, st);
}

}  // extern "C"
