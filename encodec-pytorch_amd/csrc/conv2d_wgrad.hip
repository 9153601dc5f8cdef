// NormConv2d weight and bias grad (conv2d.h) on gfx950: the tiled kernel, the column-group
// kernel with quad staging, the register-window kernel (one-wave and 8-wave forms), the
// single-output-channel kernel and the fixed-order slab reductions;
// encx_conv2d_bwd_weight picks one per layer.
#include "common.h"
#include "conv2d.h"
#include "prof.h"

namespace {

constexpr int WG_BT = 64;  // c2_wgrad_kernel: output positions per work item

struct C2Wg {
    C2Geo g;
    const float* dy;
    const float* yact;
    const float* x;
    float* ws;  // [S][Co][N], N = VC*KF + 1 (bias column last)
    int BT, NR, RL, NCmax, items, per_split, chunks;
};

template <int BM, int BN, int WM, int WN, int WK, bool YM = true>
__global__ __launch_bounds__(NT) void c2_wgrad_kernel(C2Wg a) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    static_assert(WM * WN * WK == 4, "4 waves");
    extern __shared__ float smem[];
    const C2Geo g = a.g;
    constexpr int BT = WG_BT;
    const int NR = a.NR, RL = a.RL, KF = g.KF, S = g.sf;
    const int VC = g.Ci * g.KT, Nw = VC * KF, N = Nw + 1, XR = NR * RL;
    int4* rtab = (int4*)smem;                         // [NCmax*NR]: window-row table
    float* Ls = smem + 4 * a.NCmax * NR;              // [BT][BM]
    float* Rs = Ls + BT * BM;                         // [NCmax][NR][RL]
    int* poff = (int*)(Rs + a.NCmax * XR);            // [BT]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave % WK, wmn = wave / WK;
    const int wm0 = (wmn / WN) * TM * 32, wn0 = (wmn % WN) * TN * 32;
    const int h = lane >> 5, l32 = lane & 31;
    const int co0 = blockIdx.y * BM, n0 = blockIdx.x * BN, split = blockIdx.z;
    const int c_first = n0 / KF;
    const int Nall = g.T2 * g.Fo;
    const int64_t plane_y = (int64_t)Nall, plane_x = (int64_t)g.T2 * g.Fi;
    int cbase[TN];
    bool isb[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn0 + j * 32 + l32;
        const int vc = n / KF, kf = n - vc * KF;
        isb[j] = n == Nw;
        cbase[j] = (n < Nw) ? (vc - c_first) * XR + kf : 0;
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};
    // rows r = cl*NR + rs of the x window: {offset relative to row tf, row relative to tf, rs,
    // vc in range}; per item only tf / f0 / nr change, so the staging needs no division
    for (int r = tid; r < a.NCmax * NR; r += NT) {
        const int cl = r / NR, rs = r - cl * NR, vc = c_first + cl, ci = vc / g.KT, kt = vc - ci * g.KT;
        const int rrel = rs + kt * g.dt - g.pt;
        rtab[r] = make_int4(ci * (int)plane_x + rrel * g.Fi, rrel, rs, vc < VC);
    }
    const int dr = NT / RL, dw = NT - dr * RL, r_init = tid / RL, w_init = tid - r_init * RL;
    const int it_beg = split * a.per_split, it_end = min(a.items, it_beg + a.per_split);
    const int tw = BT / WK;
    for (int it = it_beg; it < it_end; ++it) {
        const int b = it / a.chunks, p0 = (it - b * a.chunks) * BT;
        const int pend = min(Nall, p0 + BT);
        const int tf = p0 / g.Fo, f0 = p0 - tf * g.Fo;
        const int nr = (pend - 1) / g.Fo - tf + 1;
        const float* dyb = a.dy + (int64_t)b * g.Co * plane_y;
        const float* yab = YM ? a.yact + (int64_t)b * g.Co * plane_y : nullptr;
        const float* xb = a.x + (int64_t)b * g.Ci * plane_x;
        __syncthreads();
        const float* ysrc = yab ? yab : dyb;
        for (int i0 = 0; i0 < BT * BM; i0 += NT * DPER) {
            float v[DPER], ym[DPER];
#pragma unroll
            for (int q = 0; q < DPER; ++q) {
                const int i = i0 + q * NT + tid;
                const int tl = i % BT, col = i / BT, p = p0 + tl, co = co0 + col;
                const bool ok = i < BT * BM && p < pend && co < g.Co;
                const int64_t o = ok ? (int64_t)co * plane_y + p : 0;
                const float t = dyb[o];
                if (YM) ym[q] = ysrc[o];
                v[q] = ok ? t : 0.f;
            }
#pragma unroll
            for (int q = 0; q < DPER; ++q) {
                const int i = i0 + q * NT + tid;
                if (i < BT * BM) {
                    const int tl = i % BT, col = i / BT;
                    Ls[tl * BM + col] = YM ? v[q] * lrelu_grad(ym[q]) : v[q];
                }
            }
        }
        {
            const int items = a.NCmax * XR, nrows = a.NCmax * NR, tfo = tf * g.Fi;
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
                int4 e[DPER];
#pragma unroll
                for (int q = 0; q < DPER; ++q) e[q] = rtab[rq[q] < nrows ? rq[q] : 0];
                float v[DPER];
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int row = tf + e[q].y, pos = (e[q].z ? 0 : f0) * S - g.pf + wq[q];
                    const bool ok = rq[q] < nrows && e[q].w && e[q].z < nr && row >= 0 && row < g.T2 && pos >= 0 &&
                                    pos < g.Fi;
                    const float t = xb[ok ? e[q].x + tfo + pos : 0];
                    v[q] = ok ? t : 0.f;
                }
#pragma unroll
                for (int q = 0; q < DPER; ++q) {
                    const int i = i0 + q * NT + tid;
                    if (i < items) Rs[i] = v[q];
                }
            }
        }
        for (int tl = tid; tl < BT; tl += NT) {
            const int p = p0 + tl;
            int off = 0;
            if (p < pend) {
                const int tr = p / g.Fo, f = p - tr * g.Fo, rs = tr - tf;
                off = rs * RL + (f - (rs ? 0 : f0)) * S;
            }
            poff[tl] = off;
        }
        __syncthreads();
        for (int tp = wk * tw; tp < (wk + 1) * tw; tp += 2) {
            const int tl = tp + h;
            const int po = poff[tl];
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = Ls[tl * BM + wm0 + i * 32 + l32];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = isb[j] ? 1.f : Rs[cbase[j] + po];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma32(av[i], bv[j], acc[i][j]);
        }
    }
    if (WK > 1) {
        __syncthreads();
        float* red = smem;  // [WM*WN][WK][TM*TN*16][64]
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    red[(((wmn * WK + wk) * TM * TN + i * TN + j) * 16 + r) * 64 + lane] = acc[i][j][r];
        __syncthreads();
        if (wk != 0) return;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = red[(((wmn * WK) * TM * TN + i * TN + j) * 16 + r) * 64 + lane];
                    for (int w = 1; w < WK; ++w)
                        v += red[(((wmn * WK + w) * TM * TN + i * TN + j) * 16 + r) * 64 + lane];
                    acc[i][j][r] = v;
                }
    }
    float* wsb = a.ws + (int64_t)split * g.Co * N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn0 + j * 32 + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm0 + i * 32 + mfma_row(r, lane);
                if (co < g.Co && n < N) wsb[(int64_t)co * N + n] = acc[i][j][r];
            }
        }
}

// Weight grad, column-group form with vectorised staging. dW[co][n] (n = vc*KF + kf,
// vc = ci*KT + kt) as a GEMM over the positions (b, t, f). A workgroup owns GC combos = GC*KF
// columns = NW * NTW tiles of 32 and all Co <= 32 rows; wave w keeps NTW column tiles, so the
// masked dy value a lane reads once per k-pair (the A operand) feeds NTW independent MFMA chains.
// Positions are staged W3_P at a time (one batch item per chunk), every staged value moving in
// aligned quads: dy' = dy * LeakyReLU'(y) along the positions, then transposed into Ls[p][33]
// by four ds_write_b32 (the pad keeps the transposing store conflict-free), and the x window of
// the GC combos, Rs[GC][NR][RLp], as column-aligned quads (as c2_fwdr_kernel). All of a chunk's
// loads are issued before any of its LDS stores. A workgroup walks a contiguous range of chunks
// and writes one partial slab [Co][N + 1] (column Nw = the bias, summed by wave 0 of group 0 on
// the vector ALU); c2_wg_reduce adds the slabs in a fixed order.
constexpr int W3_P = 64;
struct C2Wg3 {
    C2Geo g;
    const float* dy;
    const float* yact;
    const float* x;
    float* ws;  // [splits][Co][N], N = VC*KF + 1
    int NR, RL, GC, items, per_split, chunks;
};
template <int KF, int NTW, int NW, int MQ, int ML, int OCC = 1, bool YM = true>
__global__ __launch_bounds__(NW * 64, OCC) void c2_wgrad3_kernel(C2Wg3 a) {
    constexpr int NTH = NW * 64, P = W3_P, LDA = 33, PQ = P / 4;
    extern __shared__ float smem[];
    const C2Geo g = a.g;
    const int NR = a.NR, RL = a.RL, GC = a.GC, S = g.sf;
    const int RLp = (RL + 3) & ~3, NQ = RLp >> 2, XR = NR * RLp;
    const int VC = g.Ci * g.KT, Nw = VC * KF, N = Nw + 1;
    int4* rtab = (int4*)smem;                  // [GC*NR]: {offset at row tf, row - tf, rs, valid}
    float* Ls = smem + 4 * GC * NR;            // [P][LDA]
    int* poff = (int*)(Ls + P * LDA);          // [P]
    float* Rs = (float*)(poff + P);            // [GC][NR][RLp] (16-byte aligned: see plan_wg3r)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l32 = lane & 31;
    const TileId tile = xcd_tile();  // the combo groups of one split share its dy chunks
    const int vc0 = tile.x * GC, split = tile.y;
    const int n0 = vc0 * KF + wave * NTW * 32;
    const int Nall = g.T2 * g.Fo;
    const int64_t plane_y = (int64_t)Nall, plane_x = (int64_t)g.T2 * g.Fi;
    const int64_t ytot = (int64_t)g.B * g.Co * plane_y, xtot = (int64_t)g.B * g.Ci * plane_x;
    const bool do_bias = tile.x == 0 && wave == 0;
    const int baseN = (-g.pf) & ~3;
    int cbase[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int n = n0 + j * 32 + l32;
        const int vc = n / KF, kf = n - vc * KF;
        cbase[j] = (n < Nw) ? (vc - vc0) * XR + kf : 0;
    }
    f32x16 acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[j] = (f32x16){0};
    float bsum = 0.f;
    for (int r = tid; r < GC * NR; r += NTH) {
        const int cl = r / NR, rs = r - cl * NR, vc = vc0 + cl, ci = vc / g.KT, kt = vc - ci * g.KT;
        const int rrel = rs + kt * g.dt - g.pt;
        rtab[r] = make_int4(ci * (int)plane_x + rrel * g.Fi, rrel, rs, vc < VC);
    }
    const int dr = NTH / NQ, dq = NTH - dr * NQ, r_init = tid / NQ, q_init = tid - r_init * NQ;
    const int it_beg = split * a.per_split, it_end = min(a.items, it_beg + a.per_split);
    __syncthreads();
    f32x4 dv[ML], yv[ML], xv[MQ];
    int dmask[ML], xmask[MQ];
    // ---- loads of chunk it: dy / y quads along positions, x window quads
    auto load = [&](int it) {
        const int b = it / a.chunks, p0 = (it - b * a.chunks) * P;
        const int pend = min(Nall, p0 + P);
        const int tf = p0 / g.Fo, f0 = p0 - tf * g.Fo;
        const int nr = (pend - 1) / g.Fo - tf + 1;
        const int base0 = (f0 * S - g.pf) & ~3;
        const int64_t yb = (int64_t)b * g.Co * plane_y, xbo = (int64_t)b * g.Ci * plane_x;
#pragma unroll
        for (int u = 0; u < ML; ++u) {
            const int i = u * NTH + tid, co = i / PQ, k = i - co * PQ, p = p0 + 4 * k;
            const bool any = i < 32 * PQ && co < g.Co && p < pend;
            int64_t off = any ? yb + (int64_t)co * plane_y + p : 0;
            const int64_t offc = off > ytot - 4 ? ytot - 4 : off;
            dv[u] = ld4u(a.dy + offc);
            if (YM) yv[u] = ld4u(a.yact + offc);
            dmask[u] = any ? (min(pend - p, 4) | ((int)(off - offc) << 4)) : 0;
        }
        int r = r_init, q = q_init;
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            const int rr = r < GC * NR ? r : 0;
            const int4 e = rtab[rr];
            const int base = e.z ? baseN : base0, col = base + 4 * q;
            const int row = tf + e.y;
            const bool any = r < GC * NR && e.w && e.z < nr && row >= 0 && row < g.T2 && col >= 0 && col < g.Fi;
            int64_t off = any ? xbo + e.x + (int64_t)tf * g.Fi + col : 0;
            const int64_t offc = off > xtot - 4 ? xtot - 4 : off;
            xv[u] = ld4u(a.x + offc);
            xmask[u] = any ? (min(g.Fi - col, 4) | ((int)(off - offc) << 4)) : 0;
            q += dq;
            r += dr;
            if (q >= NQ) {
                q -= NQ;
                ++r;
            }
        }
    };
    // ---- LDS image of chunk it from the loaded registers
    auto store = [&](int it) {
        const int b = it / a.chunks, p0 = (it - b * a.chunks) * P;
        const int pend = min(Nall, p0 + P);
        const int tf = p0 / g.Fo, f0 = p0 - tf * g.Fo;
        const int base0 = (f0 * S - g.pf) & ~3;
#pragma unroll
        for (int u = 0; u < ML; ++u) {
            const int i = u * NTH + tid, co = i / PQ, k = i - co * PQ;
            if (i < 32 * PQ) {
                const int m = dmask[u], nv = m & 15, sh = m >> 4;
                f32x4 v = dv[u], y = yv[u];
                if (sh) {
                    const f32x4 t = v, ty = y;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        v[c] = c + sh < 4 ? (c + sh == 1 ? t[1] : c + sh == 2 ? t[2] : t[3]) : 0.f;
                        y[c] = c + sh < 4 ? (c + sh == 1 ? ty[1] : c + sh == 2 ? ty[2] : ty[3]) : 0.f;
                    }
                }
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    Ls[(4 * k + c) * LDA + co] = c < nv ? (YM ? v[c] * lrelu_grad(y[c]) : v[c]) : 0.f;
            }
        }
        int r = r_init, q = q_init;
#pragma unroll
        for (int u = 0; u < MQ; ++u) {
            const int m = xmask[u], nv = m & 15, sh = m >> 4;
            f32x4 v = xv[u];
            if (sh) {
                const f32x4 t = v;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = c + sh < 4 ? (c + sh == 1 ? t[1] : c + sh == 2 ? t[2] : t[3]) : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = c < nv ? v[c] : 0.f;
            if (r < GC * NR) *(f32x4*)(Rs + r * RLp + 4 * q) = v;
            q += dq;
            r += dr;
            if (q >= NQ) {
                q -= NQ;
                ++r;
            }
        }
        for (int tl = tid; tl < P; tl += NTH) {
            const int p = p0 + tl;
            int off = 0;
            if (p < pend) {
                const int tr = p / g.Fo, f = p - tr * g.Fo, rs = tr - tf;
                off = rs * RLp + f * S - g.pf - (rs ? baseN : base0);
            }
            poff[tl] = off;
        }
    };
    for (int it = it_beg; it < it_end; ++it) {
        load(it);
        __syncthreads();  // the previous chunk's MFMAs are done with Ls / Rs
        store(it);
        __syncthreads();
#pragma unroll 4
        for (int kp = 0; kp < P / 2; ++kp) {
            const int tl = 2 * kp + h;
            const int po = poff[tl];
            const float av = Ls[tl * LDA + l32];
            bsum += av;  // every wave (no branch in the loop); only the bias wave stores it
            float bv[NTW];
#pragma unroll
            for (int j = 0; j < NTW; ++j) bv[j] = Rs[cbase[j] + po];
#pragma unroll
            for (int j = 0; j < NTW; ++j) acc[j] = mfma32(av, bv[j], acc[j]);
        }
    }
    float* wsb = a.ws + (int64_t)split * g.Co * N;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int n = n0 + j * 32 + l32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = mfma_row(r, lane);
            if (co < g.Co && n < Nw) wsb[(int64_t)co * N + n] = acc[j][r];
        }
    }
    if (do_bias) {
        bsum += __shfl_xor(bsum, 32, 64);
        if (h == 0 && l32 < g.Co) wsb[(int64_t)l32 * N + Nw] = bsum;
    }
}

// Weight grad, register-window form: no LDS, no staging. The GEMM's reduction index is the
// output position, and the MFMA's two k slots are two positions, so the 32 x 32 tile of one tap
// (kt, kf) is D[co][ci] = sum_p dy'[co][p] x[ci][row(p, kt)][S p + kf - pf]. A wave owns 9 taps
// (one kt of a 3x9 layer, or all of a 3x3 layer) and walks (b, t, 8-position chunk) items; half
// h of the wave takes positions f0 + 4h .. f0 + 4h + 3 of a chunk, so
//   A: lane (h, co) needs dy'[co][t][f0 + 4h + q], q < 4: ONE quad load (+ the y quad for
//      LeakyReLU'(y)),
//   B: lane (h, ci) needs, for all 9 taps and the 4 positions, x[ci][row][S (f0 + 4h) - pf + r],
//      r < 3S + KF: one contiguous window of WQ quads per kt row,
// and a chunk is 9 taps x 4 positions = 36 MFMAs on 9 accumulator chains (one per tap), with
// no LDS read and no address arithmetic between them. The next item's quads are loaded before the
// current item's MFMAs (register double buffer). Each wave writes its 32 x 32 x 9 partial to
// the split slab ws[split][co][n] (c2_wg_reduce sums the slabs in a fixed order).
struct C2WgR {
    C2Geo g;
    const float* dy;
    const float* yact;
    const float* x;
    float* ws;      // [splits][Co][N], N = Ci*KT*KF + 1
    int NC;         // 8-position chunks per output row
    int items;      // B * T2 * NC
    int per_split;  // items per wave
    int ktg;        // kt groups (tasks per split per ci block): KT for KF = 9, 1 for KF = 3
    int cib;        // 32-channel ci blocks
    int SW, NCS;    // item order: strips of SW chunks (SW | NC, NCS = NC / SW), t within a strip
};
template <int KTW, int WQ>
struct RwStage {  // one item's operands, loaded a whole item ahead of their MFMAs
    f32x4 av, yv, xw[KTW][WQ];
};
// Quad load at a wave-uniform base plus a 32-bit byte offset per lane (plus a constant). The base
// is formed on the scalar unit; the lane's part is one 64-bit add per base (the compiler keeps the
// zero-extended lane offset in a register pair), and the constant goes into the instruction.
ENCX_DEV f32x4 ld4_sv(const float* base, uint32_t lane_bytes, int imm = 0) {
    typedef const __attribute__((address_space(1))) char* gptr;
    const uint64_t b = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    const gptr p = (gptr)(((uint64_t)hi << 32) | lo);
    return *(const __attribute__((address_space(1))) f32x4u*)(p + (uint64_t)lane_bytes + imm);
}
// An item's geometry is the same for every lane of the wave, so it lives in scalar registers and
// is advanced from item to item (RwPos: + NW chunks, carrying at SW, T2, NCS; no division). A
// lane's element offsets are these scalars plus a per-lane constant computed once per wave.
struct RwPos {
    int cs, t, strip, b;  // chunk in strip, row, strip, batch
};
template <int KTW>
struct RwItem {
    int f0;         // first position of the chunk
    int sy;         // element offset of dy[b][0][t][f0]
    int sx[KTW];    // element offset of x[b][0][row(k)][S f0 - pf] (row 0 if row(k) is outside)
    bool edge;      // some element of this item lies outside its row
    bool rok[KTW];  // kt row k is inside the input
    bool ends;      // some lane's quad may start outside the tensor (its first / last quads only)
};
// NW > 1 (c2_wgrad_rwg): NW waves per workgroup share one (kt group, ci block, split) task and
// take its items interleaved (wave w: items it_beg + w, + NW, ...; neighbouring waves read
// neighbouring windows), then sum their 32 x 32 x NTAP accumulators through LDS in a fixed
// order (waves 0..3 store, waves 4..7 add, one pass sums the four) and store ONE task partial,
// contiguous, in the task-major slab ws[split][kt group][ci block][co][ci][tap] (+ 32 biases),
// which c2_wgr_reduce sums: NW x fewer slab bytes than the one-wave form, and coalesced.
template <int KF, int S, int KTW, int WQ, bool YM, int NW = 1>
__global__ __launch_bounds__(NW * 64, NW == 1 ? 2 : 1) void c2_wgrad_rw_kernel(C2WgR a) {
    constexpr int NTAP = KTW * KF;
    static_assert(NW == 1 || NW == 8, "one-wave or 8-wave workgroups");
    const C2Geo g = a.g;
    const int lane = threadIdx.x & 63, h = lane >> 5, l = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform, and known to be
    const int id = xcd_linear_id();
    const int kg = id % a.ktg, rest = id / a.ktg, cb = rest % a.cib, split = rest / a.cib;
    const int kt0 = kg * KTW, ci = cb * 32 + l;
    const bool ci_ok = ci < g.Ci, co_ok = l < g.Co;
    const bool full = g.Co >= 32 && (cb + 1) * 32 <= g.Ci;  // every lane's row and column exist
    const int it_beg = split * a.per_split, it_end = min(a.items, it_beg + a.per_split);
    // element offsets fit in 32 bits (checked on the host)
    const int plane_y = g.T2 * g.Fo, plane_x = g.T2 * g.Fi;
    const int ylast = g.B * g.Co * plane_y - 4, xlast = g.B * g.Ci * plane_x - 4;
    f32x16 acc[NTAP];
#pragma unroll
    for (int j = 0; j < NTAP; ++j) acc[j] = (f32x16){0};
    float bsum = 0.f;
    // Items run (b, strip, t, chunk in strip), the chunk fastest: the kt-group workgroups of a
    // task (same ci block and split, same XCD) read the same dy / y quads at the same time and
    // x rows one or two steps of t apart, a reuse distance of a strip's bytes, not a row's
    auto advance = [&](RwPos& q) {  // the wave's next item: NW chunks on
        q.cs += NW;
        while (q.cs >= a.SW) {
            q.cs -= a.SW;
            if (++q.t == g.T2) {
                q.t = 0;
                if (++q.strip == a.NCS) {
                    q.strip = 0;
                    ++q.b;
                }
            }
        }
    };
    // this lane's constant part of its offsets: dy / y quad at it.sy + ly, window k at it.sx[k] + lx
    const int ly = (co_ok ? l : 0) * plane_y + 4 * h;
    const int lx = (ci_ok ? ci : 0) * plane_x + 4 * S * h;
    // their largest values over the wave (scalars), for RwItem::ends
    const int ly_max = (min(g.Co, 32) - 1) * plane_y + 4;
    const int lx_max = min(g.Ci - 1, cb * 32 + 31) * plane_x + 4 * S;
    // load_in's form (scalar base + 32-bit lane byte offset) needs the byte offsets of one image's
    // lanes to fit in 32 bits; and its stand-in loads of an `ends` item (base 0, see step) stay
    // inside the tensor if a plane holds the lanes' last quads. Otherwise: no lane offsets, and
    // every item counts as `ends` (stand-in at the tensor's start, then load_any).
    const bool sv_ok = g.Co * plane_y < (1 << 29) && g.Ci * plane_x < (1 << 29) && plane_y >= 8 &&
                       plane_x >= 4 * S + 4 * WQ;
    const uint32_t lyb = sv_ok ? 4u * (uint32_t)ly : 0u, lxb = sv_ok ? 4u * (uint32_t)lx : 0u;
    auto item = [&](const RwPos& q) {
        RwItem<KTW> it;
        const int f0 = (q.strip * a.SW + q.cs) * 8;
        it.f0 = f0;
        it.sy = q.b * g.Co * plane_y + q.t * g.Fo + f0;
        const int xb = q.b * g.Ci * plane_x + S * f0 - g.pf;
#pragma unroll
        for (int k = 0; k < KTW; ++k) {
            const int row = q.t + (kt0 + k) * g.dt - g.pt;
            it.rok[k] = row >= 0 && row < g.T2;
            it.sx[k] = xb + (it.rok[k] ? row : 0) * g.Fi;
        }
        it.edge = f0 + 8 > g.Fo || S * f0 - g.pf < 0 || S * (f0 + 4) - g.pf + 4 * WQ > g.Fi;
        it.ends = !sv_ok || it.sy + ly_max > ylast;
#pragma unroll
        for (int k = 0; k < KTW; ++k) it.ends = it.ends || it.sx[k] < 0 || it.sx[k] + lx_max + 4 * (WQ - 1) > xlast;
        return it;
    };
    // ---- issue the loads of an item; nothing waits for them until its compute. Every quad is one
    // (unaligned) load at its own address, so every item issues the same loads: elements past a
    // row's ends read the neighbouring row (in bounds) and compute() zeroes them; only a quad
    // past the END of the tensor is read from a clamped address and shifted (load_any).
    // An item with no edge reads only inside its rows: no clamp, and the address is the item's
    // scalar base plus the lane's constant offset (no per-lane address arithmetic).
    auto load_in = [&](RwStage<KTW, WQ>& st, const RwItem<KTW>& it) {
        const int sy = it.ends ? 0 : it.sy;
        st.av = ld4_sv(a.dy + sy, lyb);
        if (YM) st.yv = ld4_sv(a.yact + sy, lyb);
#pragma unroll
        for (int k = 0; k < KTW; ++k) {
            const int sx = it.ends ? 0 : it.sx[k];
#pragma unroll
            for (int w = 0; w < WQ; ++w) st.xw[k][w] = ld4_sv(a.x + sx, lxb, 16 * w);
        }
    };
    auto load_any = [&](RwStage<KTW, WQ>& st, const RwItem<KTW>& it) {
        const int oac = min(it.sy + ly, ylast);
        st.av = ld4u(a.dy + oac);
        if (YM) st.yv = ld4u(a.yact + oac);
#pragma unroll
        for (int k = 0; k < KTW; ++k) {
            const int rb = it.sx[k] + lx;
#pragma unroll
            for (int w = 0; w < WQ; ++w) st.xw[k][w] = ld4u(a.x + min(max(rb + 4 * w, 0), xlast));
        }
    };
    // ---- what an item that is not interior needs before its MFMAs: the tensor's end quads moved
    // into place, elements outside their row and the lanes of absent channels zeroed
    auto fix = [&](RwStage<KTW, WQ>& st, const RwItem<KTW>& it) {
        if (it.edge) {
            const int p = it.f0 + 4 * h, col0 = S * p - g.pf;
            const int oa = it.sy + ly;
            if (__any(oa > ylast)) {  // (only at the very end of the tensor)
                st.av = quad_abs(st.av, oa, ylast);
                if (YM) st.yv = quad_abs(st.yv, oa, ylast);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e >= g.Fo) st.av[e] = 0.f;
#pragma unroll
            for (int w = 0; w < WQ; ++w) {
#pragma unroll
                for (int k = 0; k < KTW; ++k) {  // the tensor's first / last quad
                    const int o = it.sx[k] + lx + 4 * w;
                    if (__any(o < 0 || o > xlast)) st.xw[k][w] = quad_abs(st.xw[k][w], o, xlast);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int col = col0 + 4 * w + e;
                    if (col < 0 || col >= g.Fi) {
#pragma unroll
                        for (int k = 0; k < KTW; ++k) st.xw[k][w][e] = 0.f;
                    }
                }
            }
        }
        if (!full) {
            if (!co_ok) st.av = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KTW; ++k)
#pragma unroll
                for (int w = 0; w < WQ; ++w)
                    if (!ci_ok) st.xw[k][w] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    // ---- dy' = dy LeakyReLU'(y) and the bias sum of one item. Not contracted: the sum adds the
    // ROUNDED products, as it does when the producer has already applied the mask (YM false);
    // beside the MFMAs of the same block the compiler otherwise fuses them (test_premask_bit_identical)
    auto grad = [&](const RwStage<KTW, WQ>& st) {
#pragma clang fp contract(off)
        f32x4 ca = st.av;
        if (YM) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ca[e] *= lrelu_grad(st.yv[e]);
        }
        bsum += (ca[0] + ca[1]) + (ca[2] + ca[3]);
        return ca;
    };
    // ---- the KF taps x 4 positions of kt row k
    auto taps = [&](const RwStage<KTW, WQ>& st, const f32x4& ca, int k) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int kf = 0; kf < KF; ++kf) {
                const int r = S * q + kf;
                acc[k * KF + kf] = mfma32(ca[q], st.xw[k][r >> 2][r & 3], acc[k * KF + kf]);
            }
    };
    // One step: issue the loads of item nx into stage sn, then the MFMAs of item cu in stage sc.
    // With the middle kt row inside the input that is ONE basic block: the six loads (scalar base
    // + lane offset), the LeakyReLU' products and the bias adds, then the row's MFMAs, with one
    // wait for exactly the older item's loads. An item at an end of the tensor (nx.ends; a handful
    // per launch) gets stand-in loads there (base 0, in bounds) and its own clamped loads after.
    auto step = [&](RwStage<KTW, WQ>& sc, const RwItem<KTW>& cu, RwStage<KTW, WQ>& sn, const RwItem<KTW>& nx) {
        if (cu.edge || !full) fix(sc, cu);  // (an interior item has nothing to fix)
        constexpr int KM = KTW / 2;  // the middle row goes first, with the loads (the rows' chains are apart)
        f32x4 ca;
        // (the fence and the scheduling barrier emit nothing; they keep the compiler from sinking
        // the loads below the MFMAs, towards the step that uses them, which would undo the prefetch)
        if (cu.rok[KM]) {
            load_in(sn, nx);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_sched_barrier(0);
            ca = grad(sc);
            taps(sc, ca, KM);
        } else {  // a kt row outside the input contributes zero
            load_in(sn, nx);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_sched_barrier(0);
            ca = grad(sc);
        }
#pragma unroll
        for (int k = 0; k < KTW; ++k)
            if (k != KM && cu.rok[k]) taps(sc, ca, k);
        if (nx.ends) load_any(sn, nx);  // (load_in read a stand-in)
    };
    // two register stages, alternating: item it + NW is in flight while item it computes.
    // The prefetches are unconditional (past the end they re-load the wave's last item and are
    // never used).
    RwStage<KTW, WQ> s0, s1;
    const int it0 = it_beg + wv;
    if (it0 < it_end) {
        RwPos pos;  // the only divisions: once per wave
        const int r1 = it0 / a.SW, r2 = r1 / g.T2;
        pos.cs = it0 - r1 * a.SW;
        pos.t = r1 - r2 * g.T2;
        pos.b = r2 / a.NCS;
        pos.strip = r2 - pos.b * a.NCS;
        RwItem<KTW> i0 = item(pos), i1;
        load_any(s0, i0);
        for (int it = it0;; it += 2 * NW) {
            if (it + NW < it_end) advance(pos);
            i1 = item(pos);
            step(s0, i0, s1, i1);
            if (it + NW >= it_end) break;
            if (it + 2 * NW < it_end) advance(pos);
            i0 = item(pos);
            step(s1, i1, s0, i0);
            if (it + 2 * NW >= it_end) break;
        }
    }
    if constexpr (NW > 1) {
        // ---- fixed-order workgroup sum through LDS, then one contiguous task partial
        extern __shared__ float red[];  // [4][32 co][32 ci][NTAP] + [NW][32] biases
        constexpr int TS = 32 * 32 * NTAP;
        float* bred = red + 4 * TS;
        bsum += __shfl_xor(bsum, 32, 64);
        if (h == 0) bred[wv * 32 + l] = bsum;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if ((wv >> 2) == pass) {
                float* reg = red + (wv & 3) * TS;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = mfma_row(r, lane);
#pragma unroll
                    for (int j = 0; j < NTAP; ++j) {
                        float* q = reg + (co * 32 + l) * NTAP + j;
                        *q = pass == 0 ? acc[j][r] : *q + acc[j][r];
                    }
                }
            }
            __syncthreads();
        }
        const int64_t SZ = (int64_t)a.ktg * a.cib * TS + 32;
        float* dst = a.ws + (int64_t)split * SZ + (int64_t)(kg * a.cib + cb) * TS;
        for (int d = threadIdx.x; d < TS; d += NW * 64)
            dst[d] = ((red[d] + red[TS + d]) + red[2 * TS + d]) + red[3 * TS + d];
        if (kg == 0 && cb == 0 && threadIdx.x < 32) {
            float b = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) b += bred[w * 32 + threadIdx.x];
            a.ws[(int64_t)split * SZ + (SZ - 32) + threadIdx.x] = b;
        }
        return;
    }
    // ---- the partial: D[co][ci] of tap (kt0 + k, kf) -> ws[split][co][(ci*KT + kt)*KF + kf]
    const int N = g.Ci * g.KT * KF + 1;
    float* wsb = a.ws + (int64_t)split * g.Co * N;
    if (ci_ok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = mfma_row(r, lane);
            if (co < g.Co) {
                float* dst = wsb + (int64_t)co * N + (ci * g.KT + kt0) * KF;
#pragma unroll
                for (int j = 0; j < NTAP; ++j) dst[j] = acc[j][r];
            }
        }
    }
    if (kg == 0 && cb == 0) {
        bsum += __shfl_xor(bsum, 32, 64);
        if (h == 0 && co_ok) wsb[(int64_t)l * N + N - 1] = bsum;
    }
}

// part[g][i] = sum of slabs s in [g*G, (g+1)*G) of ws[s][i], ascending: the first stage of a
// two-stage slab sum when the slabs far outnumber the outputs (c2_wg_reduce alone would run a
// few dozen workgroups, each adding hundreds of slabs in sequence)
__global__ __launch_bounds__(256) void c2_slab_group_sum(const float* ws, int S, int G, int64_t n, float* part) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int g = blockIdx.y, s0 = g * G, cnt = min(G, S - s0);
    part[(int64_t)g * n + i] = (float)sum_strided_d(ws + (int64_t)s0 * n + i, cnt, n);
}

// dw[co][n] (+)= sum_s ws[s][co][n] for n < Nw; db[co] (+)= sum_s ws[s][co][Nw]. Fixed order
// (slab_sum_256_d: 64 outputs per block, 4 split slices, fp64 accumulation: at B 32 the bias
// grads sum ~10^5 positions through up to ~1500 slabs, and an fp32 sum of the slabs lost ~4x the
// accuracy of a pairwise fp32 sum, test_config3_b32_step_vs_oracle_fp64).
__global__ __launch_bounds__(256) void c2_wg_reduce(const float* ws, int S, int Co, int N, float* dw, float* db,
                                                    int acc_w, int acc_b) {
    __shared__ double red[256];
    const int64_t i = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const bool valid = i < (int64_t)Co * N;
    const float v = slab_sum_256_d(ws + (valid ? i : 0), S, (int64_t)Co * N, valid, red);
    if (threadIdx.x >= 64 || !valid) return;
    const int co = (int)(i / N), n = (int)(i - (int64_t)co * N);
    const int Nw = N - 1;
    if (n < Nw) {
        if (dw) {
            float* p = dw + (int64_t)co * Nw + n;
            *p = acc_w ? *p + v : v;
        }
    } else if (db) {
        db[co] = acc_b ? db[co] + v : v;
    }
}

// dw[co][(ci*KT + kt)*KF + kf] (+)= sum_s of the task-major slabs of c2_wgrad_rw_kernel<.., NW > 1>
// (ws[s][kg][cb][co][ci % 32][k*KF + kf], kt = kg*KTW + k, cb = ci / 32; the biases at SZ - 32 + co),
// db[co] likewise. Fixed order (slab_sum_256_d).
__global__ __launch_bounds__(256) void c2_wgr_reduce(const float* ws, int S, int64_t SZ, int Co, int Ci, int KT,
                                                     int KF, int KTW, int cib, float* dw, float* db, int acc_w,
                                                     int acc_b) {
    __shared__ double red[256];
    const int N = Ci * KT * KF + 1;
    const int64_t i = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const bool valid = i < (int64_t)Co * N;
    int64_t off = 0;
    int co = 0, n = 0;
    if (valid) {
        co = (int)(i / N);
        n = (int)(i - (int64_t)co * N);
        if (n < N - 1) {
            const int ci = n / (KT * KF), kt = (n / KF) % KT, kf = n % KF;
            const int kg = kt / KTW, k = kt % KTW, NTAP = KTW * KF;
            off = ((((int64_t)kg * cib + ci / 32) * 32 + co) * 32 + (ci & 31)) * NTAP + k * KF + kf;
        } else {
            off = SZ - 32 + co;
        }
    }
    const float v = slab_sum_256_d(ws + off, S, SZ, valid, red);
    if (threadIdx.x >= 64 || !valid) return;
    if (n < N - 1) {
        if (dw) {
            float* p = dw + (int64_t)co * (N - 1) + n;
            *p = acc_w ? *p + v : v;
        }
    } else if (db) {
        db[co] = acc_b ? db[co] + v : v;
    }
}

// Single output channel (Co = 1, the VALU kernels described at c2_co1_fwd):
// ws[s][0][n], s = (b, row chunk): n =(ci*KT + kt)*KF + kf -> sum over the chunk's output
// positions of dy'[b][to][fo] * x[b][ci][to + kt*dt - pt][fo*S + kf - pf]; n = Ci*KT*KF -> the
// chunk's sum of dy' (bias). Block = 4 waves (one ci each, blockIdx.z picks the ci group) x 64
// lanes along fo; per-lane partials are summed over the wave in a fixed order through LDS.
template <int KT, int KF, int S>
__global__ __launch_bounds__(256) void c2_co1_wgrad(C2Wg a) {
    constexpr int K = KT * KF;
    const C2Geo g = a.g;
    __shared__ float red[4][K + 1][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rc = blockIdx.x, b = blockIdx.y, ci = blockIdx.z * 4 + wave;
    const int N = g.Ci * K + 1, rows = a.BT;
    const int to0 = rc * rows, to1 = min(g.T2, to0 + rows);
    const int64_t plane = (int64_t)g.T2 * g.Fo, xplane = (int64_t)g.T2 * g.Fi;
    const float* dyb = a.dy + (int64_t)b * plane;
    const float* yab = a.yact ? a.yact + (int64_t)b * plane : dyb;
    const float* xc = a.x + ((int64_t)b * g.Ci + (ci < g.Ci ? ci : 0)) * xplane;
    float acc[K], bacc = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.f;
    const int p1 = to1 * g.Fo;
    for (int base = to0 * g.Fo; base < p1; base += 64) {
        {
            const int p = base + lane;
            const bool cok = p < p1;
            const int pc = cok ? p : p1 - 1;
            const int to = pc / g.Fo, fo = pc - to * g.Fo;
            const int64_t o = pc;
            float d = dyb[o];
            if (a.yact) d *= lrelu_grad(yab[o]);
            d = cok ? d : 0.f;
            bacc += d;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const int tr = to + kt * g.dt - g.pt;
                const bool rok = tr >= 0 && tr < g.T2;
                const float* row = xc + (int64_t)(rok ? tr : 0) * g.Fi;
#pragma unroll
                for (int kf = 0; kf < KF; ++kf) {
                    const int f = fo * S + kf - g.pf;
                    const bool ok = rok && f >= 0 && f < g.Fi;
                    const float v = row[ok ? f : 0];
                    acc[kt * KF + kf] = fmaf(d, ok ? v : 0.f, acc[kt * KF + kf]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][k][lane] = acc[k];
    red[wave][K][lane] = bacc;
    __syncthreads();
    if (lane <= K) {
        float v = 0.f;
        for (int l = 0; l < 64; ++l) v += red[wave][lane][l];
        float* out = a.ws + ((int64_t)b * gridDim.x + rc) * N;
        if (lane < K && ci < g.Ci) out[ci * K + lane] = v;
        if (lane == K && blockIdx.z == 0 && wave == 0) out[N - 1] = v;
    }
}

// ---------------------------------------------------------------------------- planning
// weight grad, column-group form (c2_wgrad3_kernel)
struct WgPlan3 {
    int NR, RL, GC, chunks, items, splits, per_split;
    size_t lds;
};
static WgPlan3 plan_wg3r(const C2Geo& g, int GC, int target = 1024) {
    WgPlan3 p;
    const int P = W3_P, Nall = g.T2 * g.Fo;
    p.GC = GC;
    p.NR = c2_rows(P, g.Fo);
    p.RL = (min(P, g.Fo) - 1) * g.sf + g.KF + 3;
    p.chunks = (int)cdiv(Nall, P);
    p.items = g.B * p.chunks;
    const int groups = (int)cdiv(g.Ci * g.KT, GC);
    int sp = (int)cdiv(target, groups);
    if (sp > p.items) sp = p.items;
    p.per_split = (int)cdiv(p.items, sp);
    p.splits = (int)cdiv(p.items, p.per_split);
    // rtab int4 [GC*NR] + Ls [P][33] + poff [P]: P*33 + P = 34*64 floats keeps Rs 16-byte aligned
    p.lds = ((size_t)4 * GC * p.NR + (size_t)P * 33 + P + (size_t)GC * p.NR * (((p.RL + 3) & ~3))) * sizeof(float);
    return p;
}
// workgroups per launch: 768 = 3 combo groups x 256 splits, whole rounds over the 256 CUs
// (tools/mb/c2_mb sweep: 768 within 2 % of the best target on all nine strided layers; targets
// that leave a partial last round, 512 = 3 x 171, lose up to 35 %)
static int wg3r_target(const C2Geo& g) {
    (void)g;
    return 768;
}
// the layers c2_wgrad3_kernel<9, 1, 9, *, 1> serves: 3x9 taps, 32-combo groups, <= 32 rows
static bool wg3r_ok(const C2Geo& g) {
    if (g.KF != 9 || (g.Ci * g.KT) % 32 != 0 || g.Co > 32 || g.Fi < 4 || g.pf > 4) return false;
    const WgPlan3 q = plan_wg3r(g, 32, 512);
    return q.GC * q.NR * (((q.RL + 3) & ~3) >> 2) <= 4 * 9 * 64;
}
// the narrow first layer (Ci*KT <= 14 combos, 3x9 taps): all combos in one column group of
// 2 or 4 waves (tools/mb/c2_mb: 1536 workgroups, 4 waves/SIMD cap; 1.5x the generic kernel)
static bool wg3n_ok(const C2Geo& g) {
    return g.KF == 9 && g.Ci * g.KT <= 14 && g.Co <= 32 && g.Fi >= 4 && g.pf <= 4;
}
static WgPlan3 plan_wg3n(const C2Geo& g) { return plan_wg3r(g, g.Ci * g.KT, 1536); }
template <int KF, int NTW, int NW, int MQ, int ML, int OCC = 1>
int run_wgrad3(const C2Geo& g, const float* dy, const float* yact, const float* x, float* ws, const WgPlan3& p,
               hipStream_t st) {
    const int quads = p.GC * p.NR * (((p.RL + 3) & ~3) >> 2);
    if (quads > MQ * NW * 64 || 32 * (W3_P / 4) > ML * NW * 64 || g.Co > 32 || g.Fi < 4 || g.pf > 4) return ENCX_EINVAL;
    C2Wg3 a{g, dy, yact, x, ws, p.NR, p.RL, p.GC, p.items, p.per_split, p.chunks};
    dim3 grid((unsigned)cdiv(g.Ci * g.KT, p.GC), (unsigned)p.splits);
    if (yact) hipLaunchKernelGGL((c2_wgrad3_kernel<KF, NTW, NW, MQ, ML, OCC, true>), grid, dim3(NW * 64), p.lds, st, a);
    else hipLaunchKernelGGL((c2_wgrad3_kernel<KF, NTW, NW, MQ, ML, OCC, false>), grid, dim3(NW * 64), p.lds, st, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

// register-window weight grad (c2_wgrad_rw_kernel): 3x9 stride-2 and 3x3 stride-1 layers with
// 32-channel blocks of input channels and <= 32 output channels
struct WgPlanR {
    int NC, items, ktg, cib, splits, per_split, SW, NCS;
};
static bool wgr_ok(const C2Geo& g) {
    if (g.Co > 32 || g.Ci < 16 || g.KT != 3 || g.Fo < 4 || g.Fi < 4) return false;
    if ((int64_t)g.B * g.Ci * g.T2 * g.Fi >= (1ll << 31) - 64 || (int64_t)g.B * g.Co * g.T2 * g.Fo >= (1ll << 31) - 64)
        return false;
    return (g.KF == 9 && g.sf == 2) || (g.KF == 3 && g.sf == 1);
}
// waves: the one-wave form's wave count; wgs > 0: the 8-wave workgroup form with at most that
// many workgroups (one per CU: its 144 KB of reduction LDS), whole rounds over the CUs
static WgPlanR plan_wgr(const C2Geo& g, int waves = 2048, int wgs = 0) {
    WgPlanR p;
    p.NC = (int)cdiv(g.Fo, 8);
    p.items = g.B * g.T2 * p.NC;
    // strip width: NC itself up to 17 chunks, else its largest divisor <= 16 (65 -> 13, 33 -> 11)
    p.SW = p.NC;
    if (p.NC > 17)
        for (int w = 16; w >= 1; --w)
            if (p.NC % w == 0) {
                p.SW = w;
                break;
            }
    p.NCS = p.NC / p.SW;
    p.ktg = g.KF == 9 ? g.KT : 1;
    p.cib = (int)cdiv(g.Ci, 32);
    const int per = p.ktg * p.cib;
    int sp = wgs > 0 ? max(1, wgs / per) : (int)cdiv(waves, per);
    if (sp > p.items) sp = p.items;
    p.per_split = (int)cdiv(p.items, sp);
    p.splits = (int)cdiv(p.items, p.per_split);
    return p;
}
static int64_t wgr_slab(const C2Geo& g, const WgPlanR& p) {  // task-major slab floats (8-wave form)
    return (int64_t)p.ktg * p.cib * 32 * 32 * 9 + 32;  // NTAP = 9 taps per task (1 x 9 or 3 x 3)
}
static int run_wgrad_rw(const C2Geo& g, const float* dy, const float* yact, const float* x, float* ws,
                        const WgPlanR& p, hipStream_t st, bool wg8 = false) {
    if (!wgr_ok(g)) return ENCX_EINVAL;
    C2WgR a{g, dy, yact, x, ws, p.NC, p.items, p.per_split, p.ktg, p.cib, p.SW, p.NCS};
    const dim3 grid((unsigned)(p.splits * p.ktg * p.cib));
    if (wg8) {
        const size_t lds = (4 * 32 * 32 * 9 + 8 * 32) * sizeof(float);
        if (g.KF == 9) {
            if (yact) hipLaunchKernelGGL((c2_wgrad_rw_kernel<9, 2, 1, 4, true, 8>), grid, dim3(512), lds, st, a);
            else hipLaunchKernelGGL((c2_wgrad_rw_kernel<9, 2, 1, 4, false, 8>), grid, dim3(512), lds, st, a);
        } else {
            if (yact) hipLaunchKernelGGL((c2_wgrad_rw_kernel<3, 1, 3, 2, true, 8>), grid, dim3(512), lds, st, a);
            else hipLaunchKernelGGL((c2_wgrad_rw_kernel<3, 1, 3, 2, false, 8>), grid, dim3(512), lds, st, a);
        }
        ENCX_CHECK_LAUNCH();
        return 0;
    }
    const dim3 blk(64);
    if (g.KF == 9) {
        if (yact) hipLaunchKernelGGL((c2_wgrad_rw_kernel<9, 2, 1, 4, true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((c2_wgrad_rw_kernel<9, 2, 1, 4, false>), grid, blk, 0, st, a);
    } else {
        if (yact) hipLaunchKernelGGL((c2_wgrad_rw_kernel<3, 1, 3, 2, true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((c2_wgrad_rw_kernel<3, 1, 3, 2, false>), grid, blk, 0, st, a);
    }
    ENCX_CHECK_LAUNCH();
    return 0;
}

struct WgPlan2 {
    int BT, NR, RL, NCmax, chunks, items, splits, per_split, narrow;
};
static WgPlan2 plan_wg2(const C2Geo& g) {
    WgPlan2 p;
    p.BT = WG_BT;
    const int Nall = g.T2 * g.Fo;
    p.NR = c2_rows(p.BT, g.Fo);
    p.RL = (min(p.BT, g.Fo) - 1) * g.sf + g.KF;
    const int N = g.Ci * g.KT * g.KF + 1;
    p.narrow = N <= 64;
    const int BN = p.narrow ? 64 : 128;
    p.NCmax = (BN - 1) / g.KF + 2;
    p.chunks = (int)cdiv(Nall, p.BT);
    p.items = g.B * p.chunks;
    const int tiles = (int)(cdiv(N, BN) * cdiv(g.Co, 32));
    int sp = (int)cdiv(1024, tiles);
    if (sp > p.items) sp = p.items;
    p.per_split = (int)cdiv(p.items, sp);
    p.splits = (int)cdiv(p.items, p.per_split);
    return p;
}

// Co = 1 wgrad: splits = (b, row chunk), about 512 of them
struct WgPlanC1 {
    int rows, chunks, splits;
};
static bool co1_ok(const C2Geo& g) { return g.Co == 1 && g.KT == 3 && g.KF == 3 && (g.sf == 1 || g.sf == 2); }
static WgPlanC1 plan_co1(const C2Geo& g) {
    WgPlanC1 p;
    const int per_b = max(1, 512 / g.B);
    p.rows = (int)cdiv(g.T2, per_b);
    p.chunks = (int)cdiv(g.T2, p.rows);
    p.splits = g.B * p.chunks;
    return p;
}

}  // namespace

extern "C" {

size_t encx_conv2d_bwd_weight_workspace(int64_t B, int64_t Ci, int64_t T2, int64_t Fi, int64_t Co, int64_t Fo,
                                        int64_t KT, int64_t KF, int64_t sf, int64_t dt, int64_t pt, int64_t pf) {
    C2Geo g{(int)B, (int)Ci, (int)T2, (int)Fi, (int)Co, (int)Fo, (int)KT, (int)KF, (int)sf, (int)dt, (int)pt, (int)pf};
    WgPlan2 p = plan_wg2(g);
    int splits = p.splits;
    if (wg3r_ok(g)) splits = max(splits, plan_wg3r(g, 32, wg3r_target(g)).splits);
    if (wgr_ok(g)) splits = max(splits, plan_wgr(g, 4096).splits);  // ENCX_WGR up to 4096 waves
    if (co1_ok(g)) splits = max(splits, plan_co1(g).splits);
    if (wg3n_ok(g)) splits = max(splits, plan_wg3n(g).splits + (int)cdiv(plan_wg3n(g).splits, 32));
    size_t bytes = (size_t)splits * Co * (Ci * KT * KF + 1) * sizeof(float);
    if (wgr_ok(g)) {  // the 8-wave form's task-major slabs (ENCX_WGR_WGS up to 1024 workgroups)
        const WgPlanR q = plan_wgr(g, 0, 1024);
        bytes = max(bytes, (size_t)q.splits * wgr_slab(g, q) * sizeof(float));
    }
    return bytes;
}

/* dw [Co][Ci][KT][KF] and db [Co] (either may be NULL) of the layer whose output grad is dy,
 * masked by LeakyReLU'(yact) when yact != NULL. acc_w / acc_b: add into dw / db. */
int encx_conv2d_bwd_weight(const float* dy, const float* yact, const float* x, float* dw, float* db,
                           int acc_w, int acc_b, float* ws, int64_t B, int64_t Ci, int64_t T2, int64_t Fi, int64_t Co,
                           int64_t Fo, int64_t KT, int64_t KF, int64_t sf, int64_t dt, int64_t pt, int64_t pf,
                           encx_stream_t stream) {
    ENCX_REQUIRE(dy && x && ws);
    C2Geo g{(int)B, (int)Ci, (int)T2, (int)Fi, (int)Co, (int)Fo, (int)KT, (int)KF, (int)sf, (int)dt, (int)pt, (int)pf};
    ENCX_REQUIRE(geo_ok(g));
    hipStream_t st = (hipStream_t)stream;
    encx_prof_scope ps(st, 2.0 * B * Co * T2 * Fo * Ci * KT * KF, 4.0 * (B * Ci * T2 * Fi + 2 * B * Co * T2 * Fo), "c2_wgrad");
    ps.tag(" %ldx%ld %ldx%ld s%ld T%ld F%ld", (long)Ci, (long)Co, (long)KT, (long)KF, (long)sf, (long)T2, (long)Fo);
    const int N = (int)(Ci * KT * KF + 1);
    if (co1_ok(g)) {
        const WgPlanC1 q = plan_co1(g);
        C2Wg a{g, dy, yact, x, ws, q.rows, 0, 0, 0, 0, 0, 0};
        dim3 grid((unsigned)q.chunks, (unsigned)B, (unsigned)cdiv(Ci, 4));
        if (sf == 1) hipLaunchKernelGGL((c2_co1_wgrad<3, 3, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((c2_co1_wgrad<3, 3, 2>), grid, dim3(256), 0, st, a);
        ENCX_CHECK_LAUNCH();
        hipLaunchKernelGGL(c2_wg_reduce, dim3((unsigned)cdiv(N, 64)), dim3(256), 0, st, ws, q.splits, 1, N, dw, db,
                           acc_w, acc_b);
        ENCX_CHECK_LAUNCH();
        return 0;
    }
    const int rw_waves = (int)min(encx_opt(OPT_WGR), (int64_t)4096);
    // 8-wave workgroups summing their partials in LDS (one per CU); option WGR_WGS = 0: one-wave form
    const int rw_wgs = (int)min(encx_opt(OPT_WGR_WGS), (int64_t)1024);
    if (rw_waves > 0 && rw_wgs > 0 && wgr_ok(g) && g_c2_select != 2) {
        const WgPlanR q = plan_wgr(g, 0, rw_wgs);
        if (run_wgrad_rw(g, dy, yact, x, ws, q, st, true) == 0) {
            hipLaunchKernelGGL(c2_wgr_reduce, dim3((unsigned)cdiv(Co * N, 64)), dim3(256), 0, st, ws, q.splits,
                               wgr_slab(g, q), (int)Co, (int)Ci, (int)KT, (int)KF, KF == 9 ? 1 : 3, q.cib, dw, db,
                               acc_w, acc_b);
            ENCX_CHECK_LAUNCH();
            return 0;
        }
    }
    if (rw_waves > 0 && wgr_ok(g) && g_c2_select != 2) {  // register-window form (c2_wgrad_rw_kernel); ENCX_WGR=0 off
        const WgPlanR q = plan_wgr(g, rw_waves);
        if (run_wgrad_rw(g, dy, yact, x, ws, q, st) == 0) {
            hipLaunchKernelGGL(c2_wg_reduce, dim3((unsigned)cdiv(Co * N, 64)), dim3(256), 0, st, ws, q.splits, (int)Co,
                               N, dw, db, acc_w, acc_b);
            ENCX_CHECK_LAUNCH();
            return 0;
        }
    }
    if (wg3r_ok(g)) {  // 9 waves x one 32-column tile each, vectorised staging (c2_wgrad3_kernel)
        const WgPlan3 q = plan_wg3r(g, 32, wg3r_target(g));
        if (run_wgrad3<9, 1, 9, 4, 1, 5>(g, dy, yact, x, ws, q, st) == 0) {
            hipLaunchKernelGGL(c2_wg_reduce, dim3((unsigned)cdiv(Co * N, 64)), dim3(256), 0, st, ws, q.splits, (int)Co,
                               N, dw, db, acc_w, acc_b);
            ENCX_CHECK_LAUNCH();
            return 0;
        }
    }
    if (wg3n_ok(g)) {
        const WgPlan3 q = plan_wg3n(g);
        const int rc = Ci * KT <= 7 ? run_wgrad3<9, 1, 2, 2, 4, 4>(g, dy, yact, x, ws, q, st)
                                    : run_wgrad3<9, 1, 4, 2, 2, 4>(g, dy, yact, x, ws, q, st);
        if (rc == 0) {
            // ~1500 slabs of Co x N outputs: groups of 32 slabs first, then the fixed-order sum
            const int G = 32, S2 = (int)cdiv(q.splits, G);
            const int64_t n = Co * N;
            float* part = ws + (int64_t)q.splits * n;
            hipLaunchKernelGGL(c2_slab_group_sum, dim3((unsigned)cdiv(n, 256), (unsigned)S2), dim3(256), 0, st, ws,
                               q.splits, G, n, part);
            hipLaunchKernelGGL(c2_wg_reduce, dim3((unsigned)cdiv(n, 64)), dim3(256), 0, st, part, S2, (int)Co, N, dw,
                               db, acc_w, acc_b);
            ENCX_CHECK_LAUNCH();
            return 0;
        }
    }
    WgPlan2 p = plan_wg2(g);
    C2Wg a{g, dy, yact, x, ws, p.BT, p.NR, p.RL, p.NCmax, p.items, p.per_split, p.chunks};
    const size_t lds = ((size_t)4 * p.NCmax * p.NR + (size_t)p.BT * 32 + (size_t)p.NCmax * p.NR * p.RL) * sizeof(float) +
                       p.BT * sizeof(int);
    if (p.narrow) {
        const size_t red = (size_t)4 * 16 * 64 * sizeof(float);  // all 4 waves' tiles
        const dim3 grid((unsigned)cdiv(N, 64), (unsigned)cdiv(Co, 32), p.splits);
        if (yact) hipLaunchKernelGGL((c2_wgrad_kernel<32, 64, 1, 2, 2, true>), grid, dim3(NT), lds > red ? lds : red, st, a);
        else hipLaunchKernelGGL((c2_wgrad_kernel<32, 64, 1, 2, 2, false>), grid, dim3(NT), lds > red ? lds : red, st, a);
    } else {
        const dim3 grid((unsigned)cdiv(N, 128), (unsigned)cdiv(Co, 32), p.splits);
        if (yact) hipLaunchKernelGGL((c2_wgrad_kernel<32, 128, 1, 4, 1, true>), grid, dim3(NT), lds, st, a);
        else hipLaunchKernelGGL((c2_wgrad_kernel<32, 128, 1, 4, 1, false>), grid, dim3(NT), lds, st, a);
    }
    ENCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(c2_wg_reduce, dim3((unsigned)cdiv(Co * N, 64)), dim3(256), 0, st, ws, p.splits, (int)Co, N,
                       dw, db, acc_w, acc_b);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
