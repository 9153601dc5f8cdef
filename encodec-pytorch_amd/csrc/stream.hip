// Streaming (stateful, chunked) forward of the causal SEANet codec: encx/streaming.py.
//
// A live session delivers n latent frames per step for up to 64 streams, so every layer is a
// small GEMM: M = Cout (32..2048), N = B * columns from 1 to ~10^5, reduction Cin*K up to 8192,
// weight-bound and launch-bound. Each layer reads a per-tensor WINDOW [B][C][P + columns] whose
// first P columns are the history carried from the previous step, and writes its output straight
// into its consumer's window behind that window's history (explicit row strides), so a step has
// no concat and no pad launch.
//
// Determinism: the reduction order of an output element is a function of the
// layer alone. stream_gemm gives reduction group g (4 consecutive reduction elements, one
// v_mfma_f32_16x16x4_f32) to wave g / ceil(G/4) of a 4-wave workgroup, G = ceil(Cin*K/4); each
// wave chains its groups in ascending order into one accumulator per 16x16 output tile (padded
// with exact zero products to a whole number of 4-group trips), and the four partials are
// added in wave order, then the bias, then the residual. Neither B, nor the
// columns of the step, nor the position of a column in its tile enters: an MFMA computes every
// element of its tile alike. So a stream's result does not depend on how its audio was sliced or
// on which streams share its batch. No floating-point atomics anywhere.
//
//  stream_gemm   Conv1d over a window (valid conv, optional pre-ELU, bias, residual) and, with
//                the polyphase weight layout, ConvTranspose1d (K = 2 stride) over [prev | chunk];
//                also the LSTM's gate pre-activations ([x_t | h_{t-1}] . wcatT + bsum).
//  lstm_stage / lstm_cell   the recurrence around that GEMM: a launch boundary is the only
//                grid-wide dependency (no inter-workgroup waiting, no counters).
//  roll_kernel   end of step: every window's last P columns move to its front, ONE launch driven
//                by a device table; first chunk: the reflected columns x[P] .. x[1] instead.
//
// Slots (encx_stream_roll_slots, encx_stream_lstm_slots): the streams of a session join, leave,
// sit a step out and deliver their own frame counts. A step computes max(frames) columns for
// every slot: every layer is causal, so the columns past a slot's count influence nothing that is
// carried, and stream_gemm needs no mask. Only what carries state reads the per-slot counts from a
// slot table in device memory: roll_kernel and lstm_stage / lstm_cell, the same kernels, which
// run without a table for the uniform step.
#include "common.h"

namespace {

typedef float f32x4s __attribute__((ext_vector_type(4)));
ENCX_DEV f32x4s mfma16s(float a, float b, f32x4s c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// y[b][m / ms][t * ms + m % ms] (+)= bias[m / ms] + sum_r w[r][m] act(x[b][r / K][t * s + (r % K) * d])
// for rows m < M, columns j = b * n_out + t < N. Conv1d: M = Cout, ms = 1, w = wf [Cin][K][Cout].
// ConvTranspose1d: M = Cout * stride, ms = stride, K = 2, s = 1, d = -1, x at the chunk's first
// column (tap 1 reads the column before it), w = wp [Cin][2][Cout * stride].
struct GemmP {
    const float* x;
    const float* w;
    const float* bias;
    float* y;
    int64_t xbs, xrs, ybs, yrs;  // element strides of a batch item / a channel row
    int R, K, M, ms, s, d, n_out, N, add;
};

constexpr int GW = 4;    // waves per workgroup: the reduction split
constexpr int GT = 4;    // 16-column tiles per workgroup
constexpr int GM = 16;   // output rows per workgroup
constexpr int GU = 4;    // reduction groups whose loads are in flight together

template <bool ELU>
__global__ __launch_bounds__(GW * 64) void stream_gemm(GemmP p) {
    __shared__ float red[GW][GT][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int m0 = blockIdx.x * GM, c0 = blockIdx.y * (GT * 16);
    const int G = (p.R + 3) >> 2, per = (G + GW - 1) / GW;
    const int g0 = wave * per, g1 = min(G, g0 + per);
    const int nt = min(GT, (p.N - c0 + 15) >> 4);  // column tiles of this workgroup that hold columns
    const int m = m0 + li;
    const bool mv = m < p.M;
    const float* wcol = p.w + (mv ? m : 0);
    const float* xc[GT];
    bool cv[GT];
#pragma unroll
    for (int q = 0; q < GT; ++q) {
        const int j = c0 + q * 16 + li;
        cv[q] = j < p.N;
        const int jj = cv[q] ? j : 0;
        const int b = jj / p.n_out, t = jj - b * p.n_out;
        xc[q] = p.x + (int64_t)b * p.xbs + (int64_t)t * p.s;
    }
    // reduction element of this lane in group g: r = 4 g + lk = ci * K + k, advanced by 4 per group
    int r = g0 * 4 + lk;
    int ci = r / p.K, k = r - ci * p.K;
    const int q4 = 4 / p.K, r4 = 4 - q4 * p.K;
    f32x4s acc[GT];
#pragma unroll
    for (int q = 0; q < GT; ++q) acc[q] = (f32x4s){0.f, 0.f, 0.f, 0.f};
    // GU groups per trip: every load of the trip is issued before the first MFMA waits for one.
    // Branch-free: an element past the wave's share, the reduction, the rows or the columns is
    // loaded from a clamped (valid) address and replaced by 0, and 0 * 0 leaves the chain as it
    // is, so a wave always runs ceil(per / GU) * GU MFMAs per tile: a function of Cin * K alone.
    for (int g = g0; g < g1; g += GU) {
        float a[GU], v[GU][GT];
        bool rv[GU];
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            rv[u] = g + u < g1 && r < p.R;
            const int64_t wo = rv[u] ? (int64_t)r * p.M : 0;
            const int64_t xo = rv[u] ? (int64_t)ci * p.xrs + (int64_t)k * p.d : 0;
            a[u] = wcol[wo];
#pragma unroll
            for (int q = 0; q < GT; ++q) v[u][q] = xc[q][xo];
            r += 4;
            k += r4;
            ci += q4;
            if (k >= p.K) {
                k -= p.K;
                ++ci;
            }
        }
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const float av = rv[u] && mv ? a[u] : 0.f;
#pragma unroll
            for (int q = 0; q < GT; ++q) {
                const float xv = ELU ? elu(v[u][q]) : v[u][q];
                acc[q] = mfma16s(av, rv[u] && cv[q] ? xv : 0.f, acc[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < GT; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wave][q][i][lane] = acc[q][i];
    __syncthreads();
    // wave q finishes column tile q: partials in wave order, bias, residual
    if (wave < nt) {
        const int j = c0 + wave * 16 + li;
        if (j < p.N) {
            const int b = j / p.n_out, t = j - b * p.n_out;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + 4 * lk + i;
                if (row < p.M) {
                    float v = red[0][wave][i][lane];
#pragma unroll
                    for (int w = 1; w < GW; ++w) v += red[w][wave][i][lane];
                    const int co = row / p.ms, ph = row - co * p.ms;
                    float* dst = p.y + (int64_t)b * p.ybs + (int64_t)co * p.yrs + (int64_t)t * p.ms + ph;
                    if (p.bias) v += p.bias[co];
                    if (p.add) v += *dst;
                    *dst = v;
                }
            }
        }
    }
}

int launch_gemm(const GemmP& p, int act, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(p.M, GM), (unsigned)cdiv(p.N, GT * 16));
    if (grid.y > 65535u) return ENCX_EINVAL;
    if (act == ENCX_ACT_ELU) hipLaunchKernelGGL(stream_gemm<true>, grid, dim3(GW * 64), 0, st, p);
    else hipLaunchKernelGGL(stream_gemm<false>, grid, dim3(GW * 64), 0, st, p);
    ENCX_CHECK_LAUNCH();
    return ENCX_OK;
}

// ------------------------------------------------------------------------- LSTM around the GEMM
ENCX_DEV float sigm_s(float x) { return 1.f / (1.f + expf(-x)); }

// The slot table (encx.h): slots[2b] = frames slot b delivers this step (0: it sits out),
// slots[2b + 1] = 1 on the slot's first chunk. NULL: every slot delivers every frame of the call.

// hz[0][b][u] = x[b][u][t]: layer 0's input of step t. A slot's first chunk starts from h = c = 0
// in every layer: cleared here, before the first gate GEMM reads h, so a restarted slot costs no
// launch of its own.
__global__ void lstm_stage(const float* x, int64_t xbs, int64_t xrs, int t, float* hz, float* c, int B, int H,
                           int L, const int32_t* slots) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, u = i - b * H;
    hz[(int64_t)b * 2 * H + u] = x[(int64_t)b * xbs + (int64_t)u * xrs + t];
    if (slots && t == 0 && slots[2 * b + 1] && slots[2 * b] > 0) {
        for (int l = 0; l < L; ++l) {
            hz[((int64_t)l * B + b) * 2 * H + H + u] = 0.f;
            c[((int64_t)l * B + b) * H + u] = 0.f;
        }
    }
}

// layer l, one (b, u) per thread: gates i, f, g, o from pre [B][4H]; c and h carried in place
// (h in the second half of the layer's own step input hz[l]); h also becomes the next layer's
// input, or the output column t (+ x, the skip) after the last layer. A slot that has no frame t
// keeps c, h and its output column as they are.
__global__ void lstm_cell(const float* pre, float* hz, float* c, const float* x, int64_t xbs, int64_t xrs,
                          float* out, int64_t obs, int64_t ors, int t, int skip, int last, int B, int H,
                          const int32_t* slots) {
#pragma clang fp contract(on)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, u = i - b * H;
    if (slots && t >= slots[2 * b]) return;
    const float* pr = pre + (int64_t)b * 4 * H + u;
    const float ig = sigm_s(pr[0]), fg = sigm_s(pr[H]), gg = tanhf(pr[2 * H]), og = sigm_s(pr[3 * H]);
    const float cn = fg * c[i] + ig * gg;
    const float h = og * tanhf(cn);
    c[i] = cn;
    hz[(int64_t)b * 2 * H + H + u] = h;
    if (!last) {
        hz[(int64_t)(B + b) * 2 * H + u] = h;  // hz[l + 1][b][u]
    } else {
        float v = h;
        if (skip) v += x[(int64_t)b * xbs + (int64_t)u * xrs + t];
        out[(int64_t)b * obs + (int64_t)u * ors + t] = v;
    }
}

// ------------------------------------------------------------------------- window roll
// One wave per window row. Shift: columns [n_cols, n_cols + P) -> [0, P); the two ranges overlap
// when n_cols < P, so every lane loads its column before any lane stores (one load instruction,
// then one store instruction, for the whole wave: P <= 64). Reflect (a stream's first chunk):
// column c <- column 2P - c, i.e. the history is x[P], x[P-1], .., x[1] as pad1d writes it.
// Zero (a first chunk whose history is the transposed conv's previous column): columns [0, P) <- 0.
//
// The table holds entries of esz bytes that begin with an encx_stream_win. Without a slot table
// (encx_stream_roll) every row moves the entry's n_cols. With one (encx_stream_roll_slots) the
// entries are encx_stream_slot_win: row r of a window belongs to slot b = r / chans and moves
// slots[2b] * rate columns; a slot that sits out keeps its history, and reflect / zero touch
// only the rows of slots on their first chunk. A row whose move would leave the row is skipped:
// whatever the tables hold, no address outside [0, rstride) of a row is formed.
__global__ __launch_bounds__(256) void roll_kernel(const char* tab, int esz, int n, int64_t rows_total, int mode,
                                                   const int32_t* slots, int B) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_total) return;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (((const encx_stream_win*)(tab + (int64_t)mid * esz))->row0 <= row) lo = mid;
        else hi = mid - 1;
    }
    const encx_stream_win e = *(const encx_stream_win*)(tab + (int64_t)lo * esz);
    const int P = (int)e.P;
    if (lane >= P || row < e.row0 || row - e.row0 >= e.rows) return;
    int64_t n_cols = e.n_cols;
    if (slots) {
        const encx_stream_slot_win* s = (const encx_stream_slot_win*)(tab + (int64_t)lo * esz);
        const int64_t chans = s->chans, rate = s->rate;
        // rows_total < 2^32 (the launch): a 32-bit division; rate < 2^31 keeps frames * rate exact
        if (chans <= 0 || chans >= (1ll << 31) || rate <= 0 || rate >= (1ll << 31)) return;
        const unsigned b = (unsigned)(row - e.row0) / (unsigned)chans;
        if (b >= (unsigned)B) return;
        const int frames = slots[2 * b], first = slots[2 * b + 1];
        if (frames <= 0 || (mode != ENCX_ROLL_SHIFT && !first)) return;
        n_cols = frames * rate;
    }
    float* p = e.ptr + (row - e.row0) * e.rstride;
    if (mode == ENCX_ROLL_ZERO) {
        if (P <= e.rstride) p[lane] = 0.f;
        return;
    }
    if (n_cols < 0 || n_cols + P > e.rstride || (mode == ENCX_ROLL_REFLECT && n_cols <= P)) return;
    const int64_t src = mode == ENCX_ROLL_REFLECT ? 2 * (int64_t)P - lane : n_cols + lane;
    const float v = p[src];
    p[lane] = v;
}

// the recurrence behind encx_stream_lstm (slots == NULL) and encx_stream_lstm_slots
int lstm_run(const float* x, const float* wcatT, const float* bsum, float* hz, float* c, float* gates, float* out,
             int skip, int64_t B, int64_t n, int64_t H, int64_t L, int64_t x_bstride, int64_t x_rstride,
             int64_t out_bstride, int64_t out_rstride, const int32_t* slots, hipStream_t st) {
    ENCX_REQUIRE(x && wcatT && bsum && hz && c && gates && out);
    ENCX_REQUIRE(B > 0 && B <= 64 && n > 0 && L > 0 && H >= 16 && (H % 16) == 0 && H <= 1024);
    ENCX_REQUIRE(x_rstride >= n && out_rstride >= n && x_bstride >= H * x_rstride && out_bstride >= H * out_rstride);
    const unsigned pw = (unsigned)cdiv(B * H, 256);
    for (int64_t t = 0; t < n; ++t) {
        hipLaunchKernelGGL(lstm_stage, dim3(pw), dim3(256), 0, st, x, x_bstride, x_rstride, (int)t, hz, c, (int)B,
                           (int)H, (int)L, slots);
        ENCX_CHECK_LAUNCH();
        for (int64_t l = 0; l < L; ++l) {
            float* hzl = hz + l * B * 2 * H;
            GemmP p;
            p.x = hzl; p.w = wcatT + l * 8 * H * H; p.bias = bsum + l * 4 * H; p.y = gates;
            p.xbs = 2 * H; p.xrs = 1; p.ybs = 4 * H; p.yrs = 1;
            p.R = (int)(2 * H); p.K = 1; p.M = (int)(4 * H); p.ms = 1; p.s = 1; p.d = 1;
            p.n_out = 1; p.N = (int)B; p.add = 0;
            const int rc = launch_gemm(p, ENCX_ACT_NONE, st);
            if (rc) return rc;
            hipLaunchKernelGGL(lstm_cell, dim3(pw), dim3(256), 0, st, (const float*)gates, hzl, c + l * B * H, x,
                               x_bstride, x_rstride, out, out_bstride, out_rstride, (int)t, skip, (int)(l == L - 1),
                               (int)B, (int)H, slots);
            ENCX_CHECK_LAUNCH();
        }
    }
    return ENCX_OK;
}

int roll_run(const void* tab, size_t esz, int64_t n_wins, int64_t rows_total, int mode, const int32_t* slots,
             int64_t B, hipStream_t st) {
    ENCX_REQUIRE(tab && n_wins > 0 && n_wins < (1ll << 31) && rows_total > 0 && rows_total < (1ll << 32));
    hipLaunchKernelGGL(roll_kernel, dim3((unsigned)cdiv(rows_total, 4)), dim3(256), 0, st, (const char*)tab,
                       (int)esz, (int)n_wins, rows_total, mode, slots, (int)B);
    ENCX_CHECK_LAUNCH();
    return ENCX_OK;
}

}  // namespace

extern "C" {

int encx_stream_conv1d(const float* win, const float* wf, const float* bias, float* y, int64_t B, int64_t Cin,
                       int64_t Cout, int64_t n_out, int64_t K, int64_t stride, int64_t dilation,
                       int64_t win_bstride, int64_t win_rstride, int64_t y_bstride, int64_t y_rstride, int pre_act,
                       int add_into_y, encx_stream_t stream) {
    ENCX_REQUIRE(win && wf && y);
    ENCX_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && n_out > 0 && K > 0 && stride > 0 && dilation > 0);
    ENCX_REQUIRE(pre_act == ENCX_ACT_NONE || pre_act == ENCX_ACT_ELU);
    // the rows must hold every column the conv reads and writes
    ENCX_REQUIRE(win_rstride >= (n_out - 1) * stride + (K - 1) * dilation + 1 && y_rstride >= n_out);
    ENCX_REQUIRE(win_bstride >= Cin * win_rstride && y_bstride >= Cout * y_rstride);
    ENCX_REQUIRE(Cin * K < (1 << 30) && B * n_out < (1ll << 31) && Cout < (1 << 30));
    GemmP p;
    p.x = win; p.w = wf; p.bias = bias; p.y = y;
    p.xbs = win_bstride; p.xrs = win_rstride; p.ybs = y_bstride; p.yrs = y_rstride;
    p.R = (int)(Cin * K); p.K = (int)K; p.M = (int)Cout; p.ms = 1; p.s = (int)stride; p.d = (int)dilation;
    p.n_out = (int)n_out; p.N = (int)(B * n_out); p.add = add_into_y != 0;
    return launch_gemm(p, pre_act, (hipStream_t)stream);
}

int encx_stream_convtr1d(const float* win, const float* wp, const float* bias, float* y, int64_t B, int64_t Cin,
                         int64_t Cout, int64_t n_in, int64_t stride, int64_t win_bstride, int64_t win_rstride,
                         int64_t y_bstride, int64_t y_rstride, int pre_act, encx_stream_t stream) {
    ENCX_REQUIRE(win && wp && y);
    ENCX_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && n_in > 0 && stride > 0);
    ENCX_REQUIRE(pre_act == ENCX_ACT_NONE || pre_act == ENCX_ACT_ELU);
    ENCX_REQUIRE(win_rstride >= n_in + 1 && y_rstride >= n_in * stride);
    ENCX_REQUIRE(win_bstride >= Cin * win_rstride && y_bstride >= Cout * y_rstride);
    ENCX_REQUIRE(Cin * 2 < (1 << 30) && B * n_in < (1ll << 31) && Cout * stride < (1 << 30));
    GemmP p;
    p.x = win + 1; p.w = wp; p.bias = bias; p.y = y;  // tap 0 reads the chunk column, tap 1 the one before
    p.xbs = win_bstride; p.xrs = win_rstride; p.ybs = y_bstride; p.yrs = y_rstride;
    p.R = (int)(Cin * 2); p.K = 2; p.M = (int)(Cout * stride); p.ms = (int)stride; p.s = 1; p.d = -1;
    p.n_out = (int)n_in; p.N = (int)(B * n_in); p.add = 0;
    return launch_gemm(p, pre_act, (hipStream_t)stream);
}

int encx_stream_lstm(const float* x, const float* wcatT, const float* bsum, float* hz, float* c, float* gates,
                     float* out, int skip, int64_t B, int64_t n, int64_t H, int64_t L, int64_t x_bstride,
                     int64_t x_rstride, int64_t out_bstride, int64_t out_rstride, encx_stream_t stream) {
    return lstm_run(x, wcatT, bsum, hz, c, gates, out, skip, B, n, H, L, x_bstride, x_rstride, out_bstride,
                    out_rstride, nullptr, (hipStream_t)stream);
}

int encx_stream_lstm_slots(const float* x, const float* wcatT, const float* bsum, float* hz, float* c, float* gates,
                           float* out, int skip, int64_t B, int64_t n_max, int64_t H, int64_t L, int64_t x_bstride,
                           int64_t x_rstride, int64_t out_bstride, int64_t out_rstride, const int32_t* slots,
                           encx_stream_t stream) {
    ENCX_REQUIRE(slots);
    return lstm_run(x, wcatT, bsum, hz, c, gates, out, skip, B, n_max, H, L, x_bstride, x_rstride, out_bstride,
                    out_rstride, slots, (hipStream_t)stream);
}

int encx_stream_roll(const encx_stream_win* wins, int64_t n_wins, int64_t rows_total, int reflect,
                     encx_stream_t stream) {
    return roll_run(wins, sizeof(encx_stream_win), n_wins, rows_total, reflect ? ENCX_ROLL_REFLECT : ENCX_ROLL_SHIFT,
                    nullptr, 0, (hipStream_t)stream);
}

int encx_stream_roll_slots(const encx_stream_slot_win* wins, int64_t n_wins, int64_t rows_total, int mode,
                           const int32_t* slots, int64_t B, encx_stream_t stream) {
    ENCX_REQUIRE(slots && B > 0 && B <= 64);
    ENCX_REQUIRE(mode == ENCX_ROLL_SHIFT || mode == ENCX_ROLL_REFLECT || mode == ENCX_ROLL_ZERO);
    return roll_run(wins, sizeof(encx_stream_slot_win), n_wins, rows_total, mode, slots, B, (hipStream_t)stream);
}

}  // extern "C"
