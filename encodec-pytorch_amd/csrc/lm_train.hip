// encx -- teacher-forced training of the entropy-coding LM (csrc/lm.hip): the next-code
// cross-entropy fused with its gradient, and the backward of the heads, of one transformer layer
// and of the input stage.
//
// The forward is lm.hip's own (encx_lm_input shifted, encx_lm_layer, encx_lm_heads), so the loss
// is the log-probability the arithmetic coder sees. Each layer keeps its encx_lm_layer workspace
// (q, ctx, h1, x1, ff, h2) and its k | v cache until the backward; everything else is recomputed
// here: the linear1 pre-activation (one GEMM whose epilogue applies GELU'), the LayerNorm
// statistics, and the attention's softmax rows from q and k | v.
//
// Every reduction has a fixed order and there is no atomic: weight grads are split-K GEMMs into
// per-split slabs summed by a second pass in slab order (the bias grad rides along as a column of
// ones), LayerNorm parameter grads are per-block partials summed in block order, attention dk / dv
// have one owner lane per key that walks its queries in ascending order, and each embedding row
// (k, code) has one owner wave that adds its rows in ascending row order. Two runs give the same
// bits.
#include "common.h"
#include "gemm.h"

namespace {

constexpr int LN_MAXV = 8;   // D <= 64 * 8, as lm.hip
constexpr int LN_ROWS = 8;   // rows per LayerNorm-backward wave (one partial of dw / db each)

// ---- GEMM operands -------------------------------------------------------------------------
// y = x W^T recomputed (the forward's operand order): x [M][K], W [N][K]
struct LdRows {
    static constexpr bool A_K_FAST = true, B_N_FAST = false;
    const float* x;
    const float* w;
    int ldx, ldw;
    ENCX_DEV float a(int m, int k) const { return x[(int64_t)m * ldx + k]; }
    ENCX_DEV float b(int k, int n) const { return w[(int64_t)n * ldw + k]; }
};
// dX = dY W: dY [M][K] rows, W [K][N] (nn.Linear's [out][in])
struct LdDgrad {
    static constexpr bool A_K_FAST = true, B_N_FAST = true;
    const float* dy;
    const float* w;
    int ldy, ldw;
    ENCX_DEV float a(int m, int k) const { return dy[(int64_t)m * ldy + k]; }
    ENCX_DEV float b(int k, int n) const { return w[(int64_t)k * ldw + n]; }
};
// (dW | db) = dY^T (X | 1): reduction over the rows; column I of the product is the bias grad
struct LdWgrad {
    static constexpr bool A_K_FAST = false, B_N_FAST = true;
    const float* dy;
    const float* x;
    int ldy, ldx, I;
    ENCX_DEV float a(int m, int k) const { return dy[(int64_t)k * ldy + m]; }
    ENCX_DEV float b(int k, int n) const {
        const float t = x[(int64_t)k * ldx + (n < I ? n : I - 1)];
        return n < I ? t : 1.f;
    }
};

struct EpStore {  // out = acc (+ res)
    const float* res;  // nullable
    float* out;
    int ldo;
    ENCX_DEV void operator()(int m, int n, float v) const {
        if (res) v += res[(int64_t)m * ldo + n];
        out[(int64_t)m * ldo + n] = v;
    }
};
struct EpSlab {  // split z's partial product into its own slab
    float* slab;
    int64_t MN;
    int ldn;
    ENCX_DEV void operator()(int m, int n, float v) const {
        slab[(int64_t)blockIdx.z * MN + (int64_t)m * ldn + n] = v;
    }
};
// d[m][n] *= GELU'(acc + bias[n]) (erf form: Phi(u) + u phi(u)), d holding dL/d gelu(u)
struct EpGeluGrad {
    const float* bias;
    float* d;
    int ld;
    ENCX_DEV void operator()(int m, int n, float v) const {
        const float u = v + bias[n];
        const float cdf = 0.5f * (1.f + erff(u * 0.70710678118654752f));
        const float pdf = 0.39894228040143268f * expf(-0.5f * u * u);
        d[(int64_t)m * ld + n] *= cdf + u * pdf;
    }
};

constexpr int WG_MIN_K = 64;  // rows per split at the least

int wgrad_splits(int O, int I, int rows) { return gemm_splits(O, I + 1, rows, WG_MIN_K, 32); }
// Slab floats that suffice for every row count up to `rows`: the split count requested never
// shrinks as the rows grow, and a launch uses at most that many slabs. (The slabs a launch does use,
// gemm_slabs, are NOT monotone in the rows -- the k chunk is rounded up to 32, so 320 rows make 5
// slabs of 64 where 330 make 4 of 96 -- and a buffer sized for one row count is reused for the
// shorter last chunk of a pass.)
int64_t wgrad_slab_floats(int64_t rows, int64_t O, int64_t I) {
    return (int64_t)wgrad_splits((int)O, (int)I, (int)rows) * O * (I + 1);
}

// second pass: slabs summed in slab order; column I goes to the bias grad
__global__ __launch_bounds__(256) void lm_wgrad_reduce_kernel(const float* __restrict__ slab, int S, int O, int I1,
                                                              float* __restrict__ dw, float* __restrict__ db,
                                                              int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)O * I1) return;
    const int m = (int)(i / I1), n = (int)(i - (int64_t)m * I1);
    const float v = sum_strided(slab + i, S, (int64_t)O * I1);
    float* dst = n < I1 - 1 ? dw + (int64_t)m * (I1 - 1) + n : db + m;
    *dst = accumulate ? *dst + v : v;
}

// dw [O][I] (=|+=) dy^T x, db [O] (=|+=) column sums of dy; dy [rows][O] (ld ldy), x [rows][I]
int lm_wgrad(const float* dy, int ldy, const float* x, int ldx, int rows, int O, int I, float* dw, float* db,
             int accumulate, float* slab, hipStream_t st) {
    const int sp = wgrad_splits(O, I, rows);
    const int S = gemm_slabs(rows, sp);
    int rc = gemm_launch(LdWgrad{dy, x, ldy, ldx, I}, EpSlab{slab, (int64_t)O * (I + 1), I + 1}, O, I + 1, rows, st, sp);
    if (rc) return rc;
    hipLaunchKernelGGL(lm_wgrad_reduce_kernel, dim3((unsigned)cdiv((int64_t)O * (I + 1), 256)), dim3(256), 0, st, slab,
                       S, O, I + 1, dw, db, accumulate);
    ENCX_CHECK_LAUNCH();
    return 0;
}

// The heads' dX = dlogits W reduces over k = K card (8192 at K 8): one fmaf chain that long loses
// ~sqrt(k) u of the result (4e-6, which every gradient below the heads inherits) and leaves few
// workgroups, so k is split into chains of about HEADS_DX_CHAIN and the slabs are summed in slab
// order in fp64.
constexpr int HEADS_DX_CHAIN = 512;
int heads_dx_splits(int kc) { return (int)std::min<int64_t>(32, cdiv(kc, HEADS_DX_CHAIN)); }
int64_t heads_dx_slab_floats(int64_t N, int64_t D, int64_t kc) {
    const int S = gemm_slabs((int)kc, heads_dx_splits((int)kc));
    return S > 1 ? S * N * D : 0;
}
__global__ __launch_bounds__(256) void lm_slab_sum_kernel(const float* __restrict__ slab, int S, int64_t n,
                                                          float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)sum_strided_d(slab + i, S, n);
}

// ---- cross-entropy fused with its gradient -------------------------------------------------
// one wave per (row, k): the logits row becomes (softmax - onehot) * scale in place
__global__ __launch_bounds__(256) void lm_ce_kernel(float* __restrict__ logits, int64_t rows, int card,
                                                    const int64_t* __restrict__ sym, int64_t s_b, int64_t s_k,
                                                    int64_t s_t, int K, int T, int64_t n0, float scale,
                                                    float* __restrict__ rowloss, float* __restrict__ rowbad) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t n = n0 + r / K;
    const int k = (int)(r % K);
    const int64_t b = n / T, t = n - b * T;
    const int64_t code = sym[b * s_b + k * s_k + t * s_t];
    const bool bad = code < 0 || code >= card;
    float* l = logits + r * card;
    float mx = -INFINITY, lc = 0.f;
    for (int c = lane; c < card; c += 64) {
        const float v = l[c];
        mx = fmaxf(mx, v);
        if (c == code) lc = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    lc = wave_sum(lc);  // one lane holds the code's logit, the rest 0
    float S = 0.f;
    for (int c = lane; c < card; c += 64) S += expf(l[c] - mx);
    S = wave_sum(S);
    for (int c = lane; c < card; c += 64) {
        const float p = expf(l[c] - mx) / S;
        l[c] = bad ? 0.f : (p - (c == code ? 1.f : 0.f)) * scale;
    }
    if (lane == 0) {
        rowloss[n0 * K + r] = bad ? 0.f : (mx + logf(S)) - lc;
        rowbad[n0 * K + r] = bad ? 1.f : 0.f;
    }
}

// loss = scale * sum of the row losses, *err = number of bad codes: thread i adds rows i, i + 256,
// ... in fp64, then a fixed LDS tree
__global__ __launch_bounds__(256) void lm_ce_finish_kernel(const float* __restrict__ rowloss,
                                                           const float* __restrict__ rowbad, int64_t n, float scale,
                                                           float* loss, int* err) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    double a = 0.0, c = 0.0;
    for (int64_t i = tid; i < n; i += 256) {
        a += (double)rowloss[i];
        c += (double)rowbad[i];
    }
    red[0][tid] = a;
    red[1][tid] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        *loss = (float)(red[0][0] * (double)scale);
        *err = (int)red[1][0];
    }
}

// ---- LayerNorm backward --------------------------------------------------------------------
// One wave per LN_ROWS consecutive rows. Statistics recomputed from the LayerNorm's input row
// (h, or with GATHER the embedding sum of the LM input, summed over k in the forward's order);
// dh = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w. The wave's sums of dy xhat and dy over
// its rows (ascending) go to part[block][2][D].
template <bool GATHER>
__global__ __launch_bounds__(64) void lm_ln_bwd_kernel(const float* __restrict__ h, const int32_t* __restrict__ idx,
                                                       const float* __restrict__ emb, int64_t card1, int K,
                                                       const float* __restrict__ dy, const float* __restrict__ w,
                                                       int N, int D, float* __restrict__ dh,
                                                       float* __restrict__ part) {
    const int lane = threadIdx.x;
    const int r0 = blockIdx.x * LN_ROWS, r1 = min(N, r0 + LN_ROWS);
    double gw[LN_MAXV], gb[LN_MAXV];  // the wave's rows, then the partials: fp64, rounded once each
    float wv[LN_MAXV];
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        gw[i] = gb[i] = 0.0;
        wv[i] = (lane + 64 * i < D) ? w[lane + 64 * i] : 0.f;
    }
    for (int r = r0; r < r1; ++r) {
        float v[LN_MAXV], g[LN_MAXV];
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) v[i] = 0.f;
        if (GATHER) {
            for (int k = 0; k < K; ++k) {
                const float* er = emb + ((int64_t)k * card1 + idx[(int64_t)k * N + r]) * D;
#pragma unroll
                for (int i = 0; i < LN_MAXV; ++i)
                    if (lane + 64 * i < D) v[i] += er[lane + 64 * i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < LN_MAXV; ++i)
                if (lane + 64 * i < D) v[i] = h[(int64_t)r * D + lane + 64 * i];
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i)
            if (lane + 64 * i < D) s += v[i];
        const float mean = wave_sum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i)
            if (lane + 64 * i < D) {
                v[i] -= mean;
                q += v[i] * v[i];
            }
        const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) {
            const int d = lane + 64 * i;
            g[i] = 0.f;
            if (d < D) {
                const float dyv = dy[(int64_t)r * D + d];
                v[i] *= rstd;  // xhat
                g[i] = dyv * wv[i];
                s1 += g[i];
                s2 += g[i] * v[i];
                gw[i] += (double)(dyv * v[i]);
                gb[i] += (double)dyv;
            }
        }
        s1 = wave_sum(s1) / (float)D;
        s2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i) {
            const int d = lane + 64 * i;
            if (d < D) dh[(int64_t)r * D + d] = rstd * (g[i] - s1 - v[i] * s2);
        }
    }
    float* p = part + (int64_t)blockIdx.x * 2 * D;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int d = lane + 64 * i;
        if (d < D) {
            p[d] = (float)gw[i];
            p[D + d] = (float)gb[i];
        }
    }
}

// gw [D], gb [D] = the partials summed in block order (in fp64)
__global__ __launch_bounds__(256) void lm_ln_param_kernel(const float* __restrict__ part, int nblk, int D,
                                                          float* __restrict__ gw, float* __restrict__ gb) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= 2 * D) return;
    const float v = (float)sum_strided_d(part + j, nblk, 2 * (int64_t)D);
    if (j < D) gw[j] = v;
    else gb[j - D] = v;
}

template <bool GATHER>
int lm_ln_bwd(const float* h, const int32_t* idx, const float* emb, int64_t card1, int K, const float* dy,
              const float* w, int N, int D, float* dh, float* part, float* gw, float* gb, hipStream_t st) {
    const int nblk = (int)cdiv(N, LN_ROWS);
    hipLaunchKernelGGL(lm_ln_bwd_kernel<GATHER>, dim3((unsigned)nblk), dim3(64), 0, st, h, idx, emb, card1, K, dy, w,
                       N, D, dh, part);
    ENCX_CHECK_LAUNCH();
    hipLaunchKernelGGL(lm_ln_param_kernel, dim3((unsigned)cdiv(2 * D, 256)), dim3(256), 0, st, part, nblk, D, gw, gb);
    ENCX_CHECK_LAUNCH();
    return 0;
}

// ---- attention backward --------------------------------------------------------------------
// Forward (lm.hip): query s = t + 1 attends keys j in [max(0, s - P), s] of [phantom, x_0, ...];
// p = softmax(scale q.k_j), ctx = sum_j p_j v_j. With dp_j = dctx.v_j and delta = dctx.ctx
// (= sum_j p_j dp_j), ds_j = p_j (dp_j - delta):
//   dq = scale sum_j ds_j k_j,  dk_j = scale sum_s ds_sj q_s,  dv_j = sum_s p_sj dctx_s.
ENCX_DEV int dcl(int d, int hd) { return d < hd ? d : hd - 1; }
ENCX_DEV const float* kv_row(const float* kv, const float* in_b, int64_t base, int64_t pos, int D, int hoff, int v) {
    return pos == 0 ? in_b + D + v * D + hoff : kv + (base + pos) * (2 * D) + v * D + hoff;
}

// dq: one wave per (stream, head, 64 consecutive queries), lane = query, walking the union of the
// windows key by key (each lane taking the keys of its own window). Also leaves each (row, head)'s softmax
// max, sum and delta in stats [N][H][3] for the dk / dv kernel.
template <int HD>
__global__ __launch_bounds__(64) void lm_attn_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                           const float* __restrict__ in_b,
                                                           const float* __restrict__ ctx,
                                                           const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                           float* __restrict__ stats, int T, int D, int H, int64_t L,
                                                           int64_t P, int tblocks) {
    const int lane = threadIdx.x;
    int id = blockIdx.x;
    const int tb = id % tblocks;
    id /= tblocks;
    const int h = id % H, b = id / H;
    const int hd = D / H, hoff = h * hd;
    const int t0 = tb * 64;
    const int t = t0 + lane;
    const bool live = t < T;
    const int64_t sfirst = 1 + t0;
    const int64_t slast = min(T, t0 + 64);
    const int64_t u0 = sfirst - P > 0 ? sfirst - P : 0;
    const int64_t base = (int64_t)b * L;
    const int64_t s = 1 + (live ? t : t0);
    const int64_t s0 = s - P > 0 ? s - P : 0;
    const float scale = 1.f / sqrtf((float)hd);
    const int64_t row = (int64_t)b * T + (live ? t : t0);
    const float* qr = q + row * D + hoff;
    const float* cr = ctx + row * D + hoff;
    const float* dr = dctx + row * D + hoff;
    float qv[HD], dc[HD], dq[HD];
    float delta = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
        qv[d] = d < hd ? qr[dcl(d, hd)] : 0.f;
        dc[d] = d < hd ? dr[dcl(d, hd)] : 0.f;
        delta = fmaf(dc[d], cr[dcl(d, hd)], delta);
        dq[d] = 0.f;
    }
    // The walk stages 64 key positions at a time in LDS: every lane fetches its share of the 64
    // k and v head slices with all loads in flight together, then the wave reads them back as
    // broadcasts. (Walking the keys straight from memory costs one load round trip per key.)
    __shared__ float ks[64 * HD], vs[64 * HD];
    constexpr int RPI = 64 / HD;  // key rows per staging iteration
    const int sd = lane % HD, sj = lane / HD;
    auto stage = [&](int64_t c0, int n) {
        float tk[HD], tv[HD];
#pragma unroll
        for (int u = 0; u < HD; ++u) {
            const int j = u * RPI + sj;
            const int64_t pos = c0 + (j < n ? j : 0);
            tk[u] = kv_row(kv, in_b, base, pos, D, hoff, 0)[dcl(sd, hd)];
            tv[u] = kv_row(kv, in_b, base, pos, D, hoff, 1)[dcl(sd, hd)];
        }
        __syncthreads();  // the previous chunk's reads are done
#pragma unroll
        for (int u = 0; u < HD; ++u) {
            const int j = u * RPI + sj;  // < 64; rows past n hold a copy of the chunk's first row, never read
            ks[j * HD + sd] = sd < hd ? tk[u] : 0.f;
            vs[j * HD + sd] = sd < hd ? tv[u] : 0.f;
        }
        __syncthreads();
    };
    // softmax statistics in one walk (running max, the sum rescaled when the max moves)
    float mx = -INFINITY, S = 0.f;
    for (int64_t c0 = u0; c0 <= slast; c0 += 64) {
        const int n = (int)min((int64_t)64, slast - c0 + 1);
        stage(c0, n);
        for (int j = 0; j < n; ++j) {
            const int64_t pos = c0 + j;
            const float* kp = ks + j * HD;
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc = fmaf(qv[d], kp[d], acc);
            const float sc = acc * scale;
            if (pos >= s0 && pos <= s) {
                const float m2 = fmaxf(mx, sc);
                S = S * expf(mx - m2) + expf(sc - m2);   // expf(-inf) = 0 at the first key
                mx = m2;
            }
        }
    }
    for (int64_t c0 = u0; c0 <= slast; c0 += 64) {
        const int n = (int)min((int64_t)64, slast - c0 + 1);
        stage(c0, n);
        for (int j = 0; j < n; ++j) {
            const int64_t pos = c0 + j;
            const float* kp = ks + j * HD;
            const float* vp = vs + j * HD;
            float kk[HD];
            float acc = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) {
                kk[d] = kp[d];
                acc = fmaf(qv[d], kk[d], acc);
                dp = fmaf(dc[d], vp[d], dp);
            }
            const float p = expf(acc * scale - mx) / S;
            const float ds = p * (dp - delta);
            if (pos >= s0 && pos <= s) {
#pragma unroll
                for (int d = 0; d < HD; ++d) dq[d] = fmaf(ds, kk[d], dq[d]);
            }
        }
    }
    if (live) {
        float* out = dqkv + row * (3 * (int64_t)D) + hoff;
#pragma unroll
        for (int d = 0; d < HD; ++d)
            if (d < hd) out[d] = dq[d] * scale;
        float* sp = stats + (row * H + h) * 3;
        sp[0] = mx;
        sp[1] = S;
        sp[2] = delta;
    }
}

// dk / dv: one wave per (stream, head, 64 consecutive key positions of 0..T), lane = key, which
// owns its dk and dv and adds its queries s in [max(1, j), min(T, j + P)] in ascending order; the
// wave walks the union of those ranges, so each query's q / dctx / stats address is wave-uniform.
// Key j >= 1 belongs to row (b, j - 1): dk | dv go to columns [D, 3D) of that row of dqkv; key 0,
// the phantom whose k | v are the in_proj biases, goes to dkv0 [B][2D].
template <int HD>
__global__ __launch_bounds__(64) void lm_attn_bwd_kv_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                            const float* __restrict__ in_b,
                                                            const float* __restrict__ dctx,
                                                            const float* __restrict__ stats, float* __restrict__ dqkv,
                                                            float* __restrict__ dkv0, int T, int D, int H, int64_t L,
                                                            int64_t P, int kblocks) {
    const int lane = threadIdx.x;
    int id = blockIdx.x;
    const int kb = id % kblocks;
    id /= kblocks;
    const int h = id % H, b = id / H;
    const int hd = D / H, hoff = h * hd;
    const int j0 = kb * 64;
    const bool live = j0 + lane <= T;
    const int64_t j = live ? j0 + lane : j0;
    const int64_t base = (int64_t)b * L;
    const float scale = 1.f / sqrtf((float)hd);
    const float* kr = kv_row(kv, in_b, base, j, D, hoff, 0);
    const float* vr = kv_row(kv, in_b, base, j, D, hoff, 1);
    float kk[HD], vv[HD], dk[HD], dv[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) {
        kk[d] = kr[dcl(d, hd)];
        vv[d] = vr[dcl(d, hd)];
        dk[d] = dv[d] = 0.f;
    }
    const int64_t jl = min((int64_t)T, (int64_t)j0 + 63);
    const int64_t sq0 = j0 > 1 ? j0 : 1;
    const int64_t sq1 = min((int64_t)T, jl + P);
    for (int64_t s = sq0; s <= sq1; ++s) {
        const int64_t row = (int64_t)b * T + s - 1;
        const float* qr = q + row * D + hoff;
        const float* dr = dctx + row * D + hoff;
        const float* sp = stats + (row * H + h) * 3;
        const float mx = sp[0], S = sp[1], delta = sp[2];
        float qd[HD], dd[HD];
        float acc = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            qd[d] = d < hd ? qr[dcl(d, hd)] : 0.f;
            dd[d] = d < hd ? dr[dcl(d, hd)] : 0.f;
            acc = fmaf(qd[d], kk[d], acc);
            dp = fmaf(dd[d], vv[d], dp);
        }
        const float p = expf(acc * scale - mx) / S;
        const float ds = p * (dp - delta) * scale;
        if (live && s >= j && s - j <= P) {
#pragma unroll
            for (int d = 0; d < HD; ++d) {
                dv[d] = fmaf(p, dd[d], dv[d]);
                dk[d] = fmaf(ds, qd[d], dk[d]);
            }
        }
    }
    if (live) {
        float* ok = j == 0 ? dkv0 + (int64_t)b * 2 * D + hoff
                           : dqkv + ((int64_t)b * T + j - 1) * (3 * (int64_t)D) + D + hoff;
#pragma unroll
        for (int d = 0; d < HD; ++d)
            if (d < hd) {
                ok[d] = dk[d];
                ok[D + d] = dv[d];
            }
    }
}

// in_proj_bias[D:3D] grad += the phantom key's dk | dv summed over the streams in order
__global__ __launch_bounds__(256) void lm_phantom_bias_kernel(const float* __restrict__ dkv0, int B, int D2,
                                                              float* __restrict__ gb) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D2) return;
    gb[j] += sum_strided(dkv0 + j, B, D2);
}

// ---- input stage ---------------------------------------------------------------------------
// idx [K][N] int32: the teacher-forced input of row n = (b, t): 0 at t = 0, else 1 + codes[b][k][t-1]
// (clamped into the table)
__global__ __launch_bounds__(256) void lm_train_idx_kernel(const int64_t* __restrict__ codes, int64_t s_b, int64_t s_k,
                                                           int64_t s_t, int K, int T, int N, int64_t card1,
                                                           int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)K * N) return;
    const int k = (int)(i / N), n = (int)(i - (int64_t)k * N);
    const int b = n / T, t = n - b * T;
    int64_t v = t == 0 ? 0 : codes[b * s_b + k * s_k + (int64_t)(t - 1) * s_t] + 1;
    v = v < 0 ? 0 : (v >= card1 ? card1 - 1 : v);
    idx[i] = (int32_t)v;
}

// demb[k][id][:] = sum of dsum rows n with idx[k][n] == id, ascending n: one owner wave per (k, id)
__global__ __launch_bounds__(64) void lm_emb_scatter_kernel(const int32_t* __restrict__ idx,
                                                            const float* __restrict__ dsum, int N, int D,
                                                            int64_t card1, float* __restrict__ demb) {
    const int lane = threadIdx.x;
    const int64_t owner = blockIdx.x;
    const int k = (int)(owner / card1);
    const int id = (int)(owner - (int64_t)k * card1);
    const int32_t* ik = idx + (int64_t)k * N;
    float acc[LN_MAXV];
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) acc[i] = 0.f;
    for (int n0 = 0; n0 < N; n0 += 64) {
        const int n = n0 + lane;
        const bool hit = n < N && ik[n < N ? n : N - 1] == id;
        unsigned long long mask = __ballot(hit);
        while (mask) {
            const int r = n0 + __ffsll((long long)mask) - 1;
            mask &= mask - 1;
#pragma unroll
            for (int i = 0; i < LN_MAXV; ++i)
                if (lane + 64 * i < D) acc[i] += dsum[(int64_t)r * D + lane + 64 * i];
        }
    }
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i)
        if (lane + 64 * i < D) demb[owner * D + lane + 64 * i] = acc[i];
}

int64_t max4(int64_t a, int64_t b, int64_t c, int64_t d) { return std::max(std::max(a, b), std::max(c, d)); }

}  // namespace

extern "C" {

int64_t encx_lm_ce_workspace(int64_t N, int64_t K) {
    if (N < 0 || K < 1) return -1;
    return 2 * N * K * (int64_t)sizeof(float);
}

int encx_lm_ce(float* logits, int64_t n0, int64_t rows, int64_t N, int64_t T, int64_t K, int64_t card,
               const int64_t* sym, int64_t s_b, int64_t s_k, int64_t s_t, float scale, float* work,
               encx_stream_t stream) {
    ENCX_REQUIRE(n0 >= 0 && rows >= 0 && N >= 0 && n0 + rows <= N && T >= 1 && N % T == 0);
    ENCX_REQUIRE(K >= 1 && K <= INT32_MAX && card >= 1 && card <= 65536 && N * K <= INT32_MAX);
    if (rows == 0) return 0;
    ENCX_REQUIRE(logits && sym && work);
    hipLaunchKernelGGL(lm_ce_kernel, dim3((unsigned)cdiv(rows * K, 4)), dim3(256), 0, (hipStream_t)stream, logits,
                       rows * K, (int)card, sym, s_b, s_k, s_t, (int)K, (int)T, n0, scale, work, work + N * K);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_lm_ce_finish(const float* work, int64_t N, int64_t K, float scale, float* loss, int* err,
                      encx_stream_t stream) {
    ENCX_REQUIRE(N >= 0 && K >= 1 && N * K <= INT32_MAX && work && loss && err);
    hipLaunchKernelGGL(lm_ce_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, work, work + N * K, N * K,
                       scale, loss, err);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int64_t encx_lm_heads_bwd_workspace(int64_t N, int64_t D, int64_t K, int64_t card) {
    if (N < 1 || D < 1 || K < 1 || card < 1 || N > INT32_MAX || K * card > INT32_MAX || D >= INT32_MAX) return -1;
    return std::max(wgrad_slab_floats(N, K * card, D), heads_dx_slab_floats(N, D, K * card)) * (int64_t)sizeof(float);
}

int encx_lm_heads_bwd(const float* dlogits, const float* x, int64_t N, int64_t D, const float* w, int64_t K,
                      int64_t card, float* dx, float* dw, float* db, int accumulate, float* work,
                      encx_stream_t stream) {
    ENCX_REQUIRE(N >= 0 && D >= 1 && K >= 1 && card >= 1 && N <= INT32_MAX && K * card <= INT32_MAX && D < INT32_MAX);
    if (N == 0) return 0;
    ENCX_REQUIRE(dlogits && x && w && dx && dw && db && work);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)N, d = (int)D, kc = (int)(K * card);
    const int sp = heads_dx_splits(kc), S = gemm_slabs(kc, sp);
    int rc;
    if (S > 1) {
        rc = gemm_launch(LdDgrad{dlogits, w, kc, d}, EpSlab{work, N * D, d}, n, d, kc, st, sp);
        if (rc) return rc;
        hipLaunchKernelGGL(lm_slab_sum_kernel, dim3((unsigned)cdiv(N * D, 256)), dim3(256), 0, st, work, S, N * D, dx);
        ENCX_CHECK_LAUNCH();
    } else {
        rc = gemm_launch(LdDgrad{dlogits, w, kc, d}, EpStore{nullptr, dx, d}, n, d, kc, st);
        if (rc) return rc;
    }
    return lm_wgrad(dlogits, kc, x, d, n, kc, d, dw, db, accumulate, work, st);
}

int64_t encx_lm_layer_bwd_workspace(int64_t B, int64_t T, int64_t D, int64_t heads, int64_t F) {
    if (B < 1 || T < 1 || D < 1 || heads < 1 || F < 1 || B * T > INT32_MAX || 3 * D >= INT32_MAX || F >= INT32_MAX)
        return -1;
    const int64_t N = B * T;
    const int64_t slab = max4(wgrad_slab_floats(N, D, F), wgrad_slab_floats(N, F, D), wgrad_slab_floats(N, D, D),
                              wgrad_slab_floats(N, 3 * D, D));
    return (N * (7 * D + F) + B * 2 * D + N * heads * 3 + cdiv(N, LN_ROWS) * 2 * D + slab) * (int64_t)sizeof(float);
}

int encx_lm_layer_bwd(const float* dy, float* dx, const float* x, int64_t B, int64_t T, const float* kv, int64_t L,
                      int64_t past_context, int64_t D, int64_t heads, int64_t F, const float* in_w,
                      const float* in_b, const float* out_w, const float* l1_w, const float* l1_b,
                      const float* l2_w, const float* n1_w, const float* n2_w, const float* fwd_work, float* g_in_w,
                      float* g_in_b, float* g_out_w, float* g_out_b, float* g_l1_w, float* g_l1_b, float* g_l2_w,
                      float* g_l2_b, float* g_n1_w, float* g_n1_b, float* g_n2_w, float* g_n2_b, float* work,
                      encx_stream_t stream) {
    ENCX_REQUIRE(B >= 1 && T >= 0 && D >= 1 && heads >= 1 && D % heads == 0 && D <= 64 * LN_MAXV);
    ENCX_REQUIRE(D / heads <= 64 && F >= 1 && F < INT32_MAX && past_context >= 0 && T + 1 <= L);
    const int64_t N = B * T;
    if (N == 0) return 0;
    ENCX_REQUIRE(N <= INT32_MAX && N * heads * 3 <= INT32_MAX && B * heads * cdiv(T + 1, 64) <= INT32_MAX);
    ENCX_REQUIRE(dy && dx && x && kv && in_w && in_b && out_w && l1_w && l1_b && l2_w && n1_w && n2_w && fwd_work);
    ENCX_REQUIRE(g_in_w && g_in_b && g_out_w && g_out_b && g_l1_w && g_l1_b && g_l2_w && g_l2_b);
    ENCX_REQUIRE(g_n1_w && g_n1_b && g_n2_w && g_n2_b && work);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)N, d = (int)D, f = (int)F, H = (int)heads;
    // the forward's buffers (encx_lm_layer)
    const float* q = fwd_work;
    const float* ctx = q + N * D;
    const float* h1 = ctx + N * D;
    const float* x1 = h1 + N * D;
    const float* ff = x1 + N * D;
    const float* h2 = ff + N * F;
    float* dh2 = work;
    float* dff = dh2 + N * D;
    float* dx1 = dff + N * F;
    float* dh1 = dx1 + N * D;
    float* dctx = dh1 + N * D;
    float* dqkv = dctx + N * D;
    float* dkv0 = dqkv + N * 3 * D;
    float* stats = dkv0 + B * 2 * D;
    float* part = stats + N * heads * 3;
    float* slab = part + cdiv(N, LN_ROWS) * 2 * D;
    int rc;
    // norm2, linear2
    if ((rc = lm_ln_bwd<false>(h2, nullptr, nullptr, 0, 0, dy, n2_w, n, d, dh2, part, g_n2_w, g_n2_b, st))) return rc;
    if ((rc = lm_wgrad(dh2, d, ff, f, n, d, f, g_l2_w, g_l2_b, 0, slab, st))) return rc;
    if ((rc = gemm_launch(LdDgrad{dh2, l2_w, d, f}, EpStore{nullptr, dff, f}, n, f, d, st))) return rc;
    // u = x1 W1^T + b1 recomputed, dff *= GELU'(u) in its epilogue; linear1; the residual join
    if ((rc = gemm_launch(LdRows{x1, l1_w, d, d}, EpGeluGrad{l1_b, dff, f}, n, f, d, st))) return rc;
    if ((rc = lm_wgrad(dff, f, x1, d, n, f, d, g_l1_w, g_l1_b, 0, slab, st))) return rc;
    if ((rc = gemm_launch(LdDgrad{dff, l1_w, f, d}, EpStore{dh2, dx1, d}, n, d, f, st))) return rc;
    // norm1, out_proj
    if ((rc = lm_ln_bwd<false>(h1, nullptr, nullptr, 0, 0, dx1, n1_w, n, d, dh1, part, g_n1_w, g_n1_b, st))) return rc;
    if ((rc = lm_wgrad(dh1, d, ctx, d, n, d, d, g_out_w, g_out_b, 0, slab, st))) return rc;
    if ((rc = gemm_launch(LdDgrad{dh1, out_w, d, d}, EpStore{nullptr, dctx, d}, n, d, d, st))) return rc;
    // attention: dq and the softmax statistics, then dk | dv per key position
    const int hd = d / H;
    const int tblocks = (int)cdiv(T, 64), kblocks = (int)cdiv(T + 1, 64);
    const int64_t P = past_context < T + 1 ? past_context : T + 1;
    if (hd <= 32) {
        hipLaunchKernelGGL(lm_attn_bwd_q_kernel<32>, dim3((unsigned)(B * H * tblocks)), dim3(64), 0, st, q, kv, in_b,
                           ctx, dctx, dqkv, stats, (int)T, d, H, L, P, tblocks);
        ENCX_CHECK_LAUNCH();
        hipLaunchKernelGGL(lm_attn_bwd_kv_kernel<32>, dim3((unsigned)(B * H * kblocks)), dim3(64), 0, st, q, kv, in_b,
                           dctx, stats, dqkv, dkv0, (int)T, d, H, L, P, kblocks);
    } else {
        hipLaunchKernelGGL(lm_attn_bwd_q_kernel<64>, dim3((unsigned)(B * H * tblocks)), dim3(64), 0, st, q, kv, in_b,
                           ctx, dctx, dqkv, stats, (int)T, d, H, L, P, tblocks);
        ENCX_CHECK_LAUNCH();
        hipLaunchKernelGGL(lm_attn_bwd_kv_kernel<64>, dim3((unsigned)(B * H * kblocks)), dim3(64), 0, st, q, kv, in_b,
                           dctx, stats, dqkv, dkv0, (int)T, d, H, L, P, kblocks);
    }
    ENCX_CHECK_LAUNCH();
    // in_proj: rows (dq | dk | dv); the phantom key's dk | dv join the bias grad; the residual join
    if ((rc = lm_wgrad(dqkv, 3 * d, x, d, n, 3 * d, d, g_in_w, g_in_b, 0, slab, st))) return rc;
    hipLaunchKernelGGL(lm_phantom_bias_kernel, dim3((unsigned)cdiv(2 * D, 256)), dim3(256), 0, st, dkv0, (int)B,
                       2 * d, g_in_b + D);
    ENCX_CHECK_LAUNCH();
    return gemm_launch(LdDgrad{dqkv, in_w, 3 * d, d}, EpStore{dh1, dx, d}, n, d, 3 * d, st);
}

int64_t encx_lm_input_bwd_workspace(int64_t B, int64_t T, int64_t D, int64_t K) {
    if (B < 0 || T < 0 || D < 1 || K < 1 || B * T > INT32_MAX) return -1;
    const int64_t N = B * T;
    return (N * D + cdiv(N, LN_ROWS) * 2 * D + K * N) * (int64_t)sizeof(float);
}

int encx_lm_input_bwd(const float* dx, const int64_t* codes, int64_t s_b, int64_t s_k, int64_t s_t, int64_t B,
                      int64_t K, int64_t T, const float* emb, int64_t card1, int64_t D, const float* ln_w,
                      float* g_emb, float* g_ln_w, float* g_ln_b, float* work, encx_stream_t stream) {
    ENCX_REQUIRE(B >= 0 && K >= 1 && K <= 64 && T >= 0 && D >= 4 && D % 2 == 0 && D <= 64 * LN_MAXV && card1 >= 1);
    const int64_t N = B * T;
    if (N == 0) return 0;
    ENCX_REQUIRE(N <= INT32_MAX && K * card1 <= INT32_MAX && K * N <= INT32_MAX * (int64_t)256);
    ENCX_REQUIRE(dx && codes && emb && ln_w && g_emb && g_ln_w && g_ln_b && work);
    hipStream_t st = (hipStream_t)stream;
    float* dsum = work;
    float* part = dsum + N * D;
    int32_t* idx = (int32_t*)(part + cdiv(N, LN_ROWS) * 2 * D);
    hipLaunchKernelGGL(lm_train_idx_kernel, dim3((unsigned)cdiv(K * N, 256)), dim3(256), 0, st, codes, s_b, s_k, s_t,
                       (int)K, (int)T, (int)N, card1, idx);
    ENCX_CHECK_LAUNCH();
    // norm_in (the sin embedding has no parameters: d(sum + pos) = d(sum))
    int rc = lm_ln_bwd<true>(nullptr, idx, emb, card1, (int)K, dx, ln_w, (int)N, (int)D, dsum, part, g_ln_w, g_ln_b, st);
    if (rc) return rc;
    hipLaunchKernelGGL(lm_emb_scatter_kernel, dim3((unsigned)(K * card1)), dim3(64), 0, st, idx, dsum, (int)N, (int)D,
                       card1, g_emb);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
