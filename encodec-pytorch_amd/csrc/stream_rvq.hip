// encx -- the residual quantizer of a streaming slots step with a codebook count per slot
// (encx/streaming.py: encode_slots / decode_slots with n_q). A step holds at most 64 x 8 latent
// columns of D = 128 floats: far too few for the per-layer kernels of rvq.hip (sized for
// training's 2400 columns, four launches a layer). Columns are independent and code k depends
// only on layers < k, so the whole residual chain of a column runs inside ONE workgroup, and a
// slot's layer count nq[b] is a loop bound.
//
//  stream_rvq_prepare  one layer's codebook into the session's packed buffers: E [K][bins][D]
//                      (rows: the gather of the decode and of the residual update), ET [K][D][bins]
//                      (its transpose: the operand of the distance loop, read coalesced along the
//                      codes) and ee [K][bins] = |e|^2, rvq_argmin_mfma's ascending-d fmaf chain.
//  stream_rvq_encode   grid (tiles of COLS columns of one slot, B). 256 threads own four adjacent
//                      codes each (bins / 4 = 256 at 1024 bins) and keep 4 x COLS running dot
//                      products in registers: per d one 16-byte load of ET (1 KB per wave-
//                      instruction, eight in flight, double buffered) against the COLS residual
//                      values broadcast from LDS. Every (column, code) product is ONE thread's fmaf
//                      chain in ascending d from 0, bitwise the v_mfma_f32_32x32x2_f32 chain of
//                      rvq_argmin_mfma (MI355X_MICROARCH.md, the FP32 matrix row; lm.hip
//                      lm_gemv_kernel), so it does not depend on B, n_max, the other slots or the
//                      tile. A fifth wave computes |x|^2 of the residual (rvq_argmin_mfma's xx
//                      chain) beside the dot products. Then v = (xx - 2 dot) + ee, the minimum of
//                      ord_key(v) << 32 | code over the thread, the wave and the four waves (ties
//                      to the lowest code, as the 64-bit atomicMin of rvq.hip), and x -= E[code]
//                      exactly (rvq_apply with ste = 0). Three barriers a layer.
//  stream_rvq_decode   grid (n_max, B): out[b][d][t] = ((E_0[c_0] + E_1[c_1]) + ...)[d] in
//                      ascending k < nq[b], rvq_gather's order. With a concealment table
//                      (encx_stream_rvq_decode_slots_conceal) the columns t < count of a lost slot
//                      are copies of its held column instead, its codes and nq[b] unread.
// Both read the slot table (count, first flag) and the nq table, clamp them, and never form an
// address from a slot's unread tail (columns >= its count).
#include "common.h"
#include "prof.h"

namespace {

constexpr int SR_NT = 256;           // threads that own codes
constexpr int SR_NTX = SR_NT + 64;   // plus the |x|^2 wave
constexpr int SR_U = 8;              // 16-byte loads in flight per thread and buffer
constexpr int SR_DMAX = 256;

ENCX_DEV uint32_t ord_key(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ENCX_DEV uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
ENCX_DEV uint64_t shfl_xor64(uint64_t v, int o) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl_xor(lo, o, 64);
    hi = __shfl_xor(hi, o, 64);
    return ((uint64_t)hi << 32) | lo;
}
ENCX_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void stream_rvq_prepare_kernel(const float* __restrict__ embed, float* __restrict__ E,
                                          float* __restrict__ ET, float* __restrict__ ee, int bins, int D) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= bins) return;
    float s = 0.f;
    for (int d = 0; d < D; ++d) {
        const float v = embed[(int64_t)c * D + d];
        E[(int64_t)c * D + d] = v;
        if (ET) ET[(int64_t)d * bins + c] = v;
        s = fmaf(v, v, s);
    }
    if (ee) ee[c] = s;
}

struct SrEnc {
    const float* x;
    int64_t x_b, x_d, x_t;
    const float* E;
    const float* ET;
    const float* ee;
    int K_max, bins, D, n_max;
    const int32_t* slots;
    const int32_t* nq;
    int64_t* codes;
    int64_t c_b, c_k, c_t;
};

template <int COLS>
__global__ __launch_bounds__(SR_NTX) void stream_rvq_encode_kernel(SrEnc a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float xs[SR_DMAX * COLS];  // the residual, [d][column]
    __shared__ float xxs[COLS];
    __shared__ uint64_t part[COLS][SR_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool dots = wave < SR_NT / 64;
    const int b = blockIdx.y, t0 = blockIdx.x * COLS;
    const int D = a.D, bins = a.bins, bins4 = bins >> 2;
    const int count = clampi(a.slots[2 * b], 0, a.n_max);
    const int nq = clampi(a.nq[b], 0, a.K_max);
    const int live = count - t0 < COLS ? count - t0 : COLS;  // columns of this tile the slot delivers
    int64_t* cb = a.codes + b * a.c_b;
    // the zeros: every row of a column the slot does not deliver, rows >= nq of the others
    for (int i = tid; i < a.K_max * COLS; i += SR_NTX) {
        const int k = i / COLS, j = i - k * COLS;
        if (t0 + j < a.n_max && (j >= live || k >= nq)) cb[k * a.c_k + (t0 + j) * a.c_t] = 0;
    }
    if (live <= 0 || nq == 0) return;  // the whole workgroup leaves: no barrier was reached
    for (int i = tid; i < D * COLS; i += SR_NTX) {
        const int j = i / D, d = i - j * D;
        xs[d * COLS + j] = j < live ? a.x[b * a.x_b + d * a.x_d + (t0 + j) * a.x_t] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < nq; ++k) {
        uint64_t best[COLS];
#pragma unroll
        for (int j = 0; j < COLS; ++j) best[j] = ~0ull;
        const float* et = a.ET + (int64_t)k * D * bins;
        for (int c40 = 0; c40 < bins4; c40 += SR_NT) {  // one round at 1024 bins; uniform trip count
            const bool valid = dots && c40 + tid < bins4;
            const int c4 = valid ? c40 + tid : bins4 - 1;
            float acc[COLS][4];
#pragma unroll
            for (int j = 0; j < COLS; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = 0.f;
            if (dots) {
                const float* p = et + 4 * c4;
                f32x4 cur[SR_U], nxt[SR_U];
#pragma unroll
                for (int u = 0; u < SR_U; ++u) cur[u] = *(const f32x4*)(p + (int64_t)u * bins);
                for (int d0 = 0; d0 < D; d0 += SR_U) {
                    // the last round reloads its own rows (in range, unused) rather than branch
                    const float* pn = p + (int64_t)(d0 + SR_U < D ? d0 + SR_U : d0) * bins;
#pragma unroll
                    for (int u = 0; u < SR_U; ++u) nxt[u] = *(const f32x4*)(pn + (int64_t)u * bins);
#pragma unroll
                    for (int u = 0; u < SR_U; ++u) {
                        float xv[COLS];
#pragma unroll
                        for (int j = 0; j < COLS; ++j) xv[j] = xs[(d0 + u) * COLS + j];
#pragma unroll
                        for (int j = 0; j < COLS; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(xv[j], cur[u][e], acc[j][e]);
                    }
#pragma unroll
                    for (int u = 0; u < SR_U; ++u) cur[u] = nxt[u];
                }
            } else if (c40 == 0 && lane < COLS) {
                // |x|^2 of the residual: ascending d from 0, one lane per column
                float v = 0.f;
                for (int d = 0; d < D; ++d) v = fmaf(xs[d * COLS + lane], xs[d * COLS + lane], v);
                xxs[lane] = v;
            }
            if (c40 == 0) __syncthreads();  // xxs visible
            if (valid) {
                const f32x4 e2 = *(const f32x4*)(a.ee + (int64_t)k * bins + 4 * c4);
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const float xx = xxs[j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = (xx - 2.f * acc[j][e]) + e2[e];
                        best[j] = umin64(best[j], ((uint64_t)ord_key(v) << 32) | (uint32_t)(4 * c4 + e));
                    }
                }
            }
        }
        if (dots) {
#pragma unroll
            for (int j = 0; j < COLS; ++j) {
                uint64_t v = best[j];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v = umin64(v, shfl_xor64(v, o));
                if (lane == 0) part[j][wave] = v;
            }
        }
        __syncthreads();
        int code[COLS];
#pragma unroll
        for (int j = 0; j < COLS; ++j) {
            uint64_t v = part[j][0];
#pragma unroll
            for (int w = 1; w < SR_NT / 64; ++w) v = umin64(v, part[j][w]);
            code[j] = (int)(uint32_t)(v & 0xffffffffull);  // < bins: every thread offered a real code
        }
        if (tid < COLS && tid < live) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < COLS; ++j) c = tid == j ? code[j] : c;
            cb[k * a.c_k + (t0 + tid) * a.c_t] = c;
        }
        if (k + 1 < nq) {  // residual - q, the exact q
            const float* Ek = a.E + (int64_t)k * bins * D;
            for (int i = tid; i < D * COLS; i += SR_NTX) {
                const int jj = i / D, d = i - jj * D;
                int c = 0;
#pragma unroll
                for (int j = 0; j < COLS; ++j) c = jj == j ? code[j] : c;
                xs[d * COLS + jj] = xs[d * COLS + jj] - Ek[(int64_t)c * D + d];
            }
        }
        __syncthreads();
    }
}

struct SrDec {
    const int64_t* codes;
    int64_t c_b, c_k, c_t;
    const float* E;
    int K_max, bins, D, n_max;
    const int32_t* slots;
    const int32_t* nq;
    float* out;
    int64_t o_b, o_d, o_t;
    const int32_t* conceal;  // nullable: the concealment table [B][4] (encx.h), word 0 = the step is lost
    const float* held;       // with it: held[b*o_b + d*o_d], the slot's last decoded latent column
};

constexpr int SR_KU = 8;  // gathers in flight per thread

// One workgroup per (column t, slot b), a thread per d. The codes of a column are uniform over the
// workgroup; the SR_KU rows of a round are loaded before they are added, in ascending k.
__global__ __launch_bounds__(128) void stream_rvq_decode_kernel(SrDec a) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int count = clampi(a.slots[2 * b], 0, a.n_max);
    const int nq = clampi(a.nq[b], 0, a.K_max);
    float* o = a.out + b * a.o_b + t * a.o_t;
    const bool lost = a.conceal && t < count && a.conceal[4 * b] != 0;
    if (lost) {  // the held latent: neither the slot's codes nor its nq are looked at
        const float* h = a.held + b * a.o_b;
        for (int d = threadIdx.x; d < a.D; d += blockDim.x) o[d * a.o_d] = h[d * a.o_d];
        return;
    }
    if (t >= count || nq == 0) {
        for (int d = threadIdx.x; d < a.D; d += blockDim.x) o[d * a.o_d] = 0.f;
        return;
    }
    const int64_t* cp = a.codes + b * a.c_b + t * a.c_t;
    for (int d = threadIdx.x; d < a.D; d += blockDim.x) {
        float acc = 0.f;
        for (int k0 = 0; k0 < nq; k0 += SR_KU) {
            float q[SR_KU];
#pragma unroll
            for (int u = 0; u < SR_KU; ++u) {
                const int k = k0 + u < nq ? k0 + u : nq - 1;  // clamped: rows >= nq are never read
                int64_t c = cp[k * a.c_k];
                c = c < 0 ? 0 : (c > a.bins - 1 ? a.bins - 1 : c);
                q[u] = a.E[((int64_t)k * a.bins + c) * a.D + d];
            }
#pragma unroll
            for (int u = 0; u < SR_KU; ++u)
                if (k0 + u < nq) acc = k0 + u ? acc + q[u] : q[u];
        }
        o[d * a.o_d] = acc;
    }
}

bool sr_dims_ok(int64_t B, int64_t K_max, int64_t bins, int64_t D, int64_t n_max) {
    return B >= 1 && B <= 64 && K_max >= 1 && K_max <= 64 && bins >= 4 && bins <= (1 << 20) && bins % 4 == 0 &&
           D >= SR_U && D <= SR_DMAX && D % SR_U == 0 && n_max >= 1 && n_max <= 255;
}

}  // namespace

extern "C" {

int encx_stream_rvq_prepare(const float* embed, int64_t k, int64_t K_max, int64_t bins, int64_t D, float* packed,
                            float* packed_t, float* ee, encx_stream_t stream) {
    ENCX_REQUIRE(embed && packed && (packed_t != nullptr) == (ee != nullptr));  // a decoder needs neither
    ENCX_REQUIRE(sr_dims_ok(1, K_max, bins, D, 1) && k >= 0 && k < K_max);
    encx_prof_scope ps((hipStream_t)stream, 2.0 * bins * D, 4.0 * bins * (3 * D + 1), "stream_rvq_prepare", false);
    hipLaunchKernelGGL(stream_rvq_prepare_kernel, dim3((unsigned)cdiv(bins, 64)), dim3(64), 0, (hipStream_t)stream,
                       embed, packed + k * bins * D, packed_t ? packed_t + k * bins * D : nullptr,
                       ee ? ee + k * bins : nullptr, (int)bins, (int)D);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_stream_rvq_encode_slots(const float* x, int64_t x_b, int64_t x_d, int64_t x_t, const float* packed,
                                 const float* packed_t, const float* ee, int64_t B, int64_t K_max, int64_t bins,
                                 int64_t D, int64_t n_max, const int32_t* slots, const int32_t* nq, int64_t* codes,
                                 int64_t c_b, int64_t c_k, int64_t c_t, encx_stream_t stream) {
    ENCX_REQUIRE(x && packed && packed_t && ee && slots && nq && codes);
    ENCX_REQUIRE(sr_dims_ok(B, K_max, bins, D, n_max));
    encx_prof_scope ps((hipStream_t)stream, 2.0 * B * n_max * K_max * bins * D,
                       4.0 * (B * D * n_max + 2.0 * K_max * bins * D) + 8.0 * B * K_max * n_max, "stream_rvq_encode");
    ps.tag("B %lld n %lld K %lld", (long long)B, (long long)n_max, (long long)K_max);
    SrEnc a{x, x_b, x_d, x_t, packed, packed_t, ee, (int)K_max, (int)bins, (int)D, (int)n_max,
            slots, nq, codes, c_b, c_k, c_t};
    // Two columns per workgroup: at 64 slots x 8 frames that is one workgroup per CU (one column:
    // twice the codebook traffic, L2-bound; four: half the CUs idle). A one-frame
    // step has one column per slot. A column's bits do not depend on its tile.
    if (n_max > 1) {
        hipLaunchKernelGGL(stream_rvq_encode_kernel<2>, dim3((unsigned)cdiv(n_max, 2), (unsigned)B), dim3(SR_NTX), 0,
                           (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(stream_rvq_encode_kernel<1>, dim3((unsigned)n_max, (unsigned)B), dim3(SR_NTX), 0,
                           (hipStream_t)stream, a);
    }
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_stream_rvq_decode_slots(const int64_t* codes, int64_t c_b, int64_t c_k, int64_t c_t, const float* packed,
                                 int64_t B, int64_t K_max, int64_t bins, int64_t D, int64_t n_max,
                                 const int32_t* slots, const int32_t* nq, float* out, int64_t o_b, int64_t o_d,
                                 int64_t o_t, encx_stream_t stream) {
    ENCX_REQUIRE(codes && packed && slots && nq && out);
    ENCX_REQUIRE(sr_dims_ok(B, K_max, bins, D, n_max));
    encx_prof_scope ps((hipStream_t)stream, 1.0 * B * n_max * K_max * D,
                       4.0 * B * D * n_max * (K_max + 1) + 8.0 * B * K_max * n_max, "stream_rvq_decode", false);
    SrDec a{codes, c_b, c_k, c_t, packed, (int)K_max, (int)bins, (int)D, (int)n_max, slots, nq, out, o_b, o_d, o_t,
            nullptr, nullptr};
    hipLaunchKernelGGL(stream_rvq_decode_kernel, dim3((unsigned)n_max, (unsigned)B), dim3(128), 0,
                       (hipStream_t)stream, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_stream_rvq_decode_slots_conceal(const int64_t* codes, int64_t c_b, int64_t c_k, int64_t c_t,
                                         const float* packed, int64_t B, int64_t K_max, int64_t bins, int64_t D,
                                         int64_t n_max, const int32_t* slots, const int32_t* nq,
                                         const int32_t* conceal, const float* held, float* out, int64_t o_b,
                                         int64_t o_d, int64_t o_t, encx_stream_t stream) {
    ENCX_REQUIRE(codes && packed && slots && nq && conceal && held && out);
    ENCX_REQUIRE(sr_dims_ok(B, K_max, bins, D, n_max));
    encx_prof_scope ps((hipStream_t)stream, 1.0 * B * n_max * K_max * D,
                       4.0 * B * D * n_max * (K_max + 1) + 8.0 * B * K_max * n_max, "stream_rvq_decode_conceal", false);
    SrDec a{codes, c_b, c_k, c_t, packed, (int)K_max, (int)bins, (int)D, (int)n_max, slots, nq, out, o_b, o_d, o_t,
            conceal, held};
    hipLaunchKernelGGL(stream_rvq_decode_kernel, dim3((unsigned)n_max, (unsigned)B), dim3(128), 0,
                       (hipStream_t)stream, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
