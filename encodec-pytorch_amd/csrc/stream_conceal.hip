// encx -- packet-loss concealment of the streaming decoder (encx/streaming.py: decode_slots with
// `lost`). A slot whose packet did not arrive decodes its last latent frame again, and its output
// fades out (and, once packets arrive again, back in) under an integer ramp the host can mirror.
//
// The concealment table, int32 conceal[B][4], beside the slot table and the nq table (encx.h):
//   word 0  lost   non-zero: the slot's step is concealed (its `count` frames repeat the held latent)
//   word 1  p      the fade position at the START of the step, 0..M (M: full level)
//   word 2  r      the samples concealed so far in the current loss run, at the start of the step
//   word 3  0
//
//  stream_conceal_fill  the per-layer dequantizer's path: after encx_rvq_gather has written the
//                       step's columns [P, P + n_max) of the decoder's first window, the rows of the
//                       lost slots get columns [P, P + count) <- column P-1 (the last latent frame the
//                       slot decoded: what the end-of-step roll left there). A row per wave.
//  stream_conceal_out   the step's output: the decoder's last window read in place, written as
//                       [B][C][n_max * hop] contiguous, zero past a slot's count, and sample j of a
//                       slot scaled by its fade position after that sample's update:
//                         concealed   p_j = max(0, p - recover * (max(0, r + j + 1 - hold) - max(0, r - hold)))
//                         delivered   p_j = min(M, p + fade * (j + 1))
//                       written as x where p_j == M, else x * (float(p_j) * invM). Closed form per
//                       sample: nothing is carried from one lane to the next. Quads (16-byte loads
//                       and stores) where the hop, the strides and the pointers allow, dwords
//                       otherwise; hop % 4 == 0 puts a whole quad on one side of count * hop.
// Neither forms an address from a column a slot does not own: past count * hop the window is not read.
#include "common.h"
#include "prof.h"

namespace {

ENCX_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void stream_conceal_fill_kernel(float* __restrict__ win, int64_t w_b, int64_t w_d,
                                                                   int B, int D, int P, int n_max,
                                                                   const int32_t* __restrict__ slots,
                                                                   const int32_t* __restrict__ conceal) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)B * D) return;
    const int b = (int)(row / D), d = (int)(row - (int64_t)b * D);
    if (conceal[4 * b] == 0) return;
    const int count = clampi(slots[2 * b], 0, n_max);
    float* r = win + b * w_b + d * w_d;
    const float v = r[P - 1];
    for (int t = lane; t < count; t += 64) r[P + t] = v;
}

struct ScOut {
    const float* x;
    int64_t x_b, x_c;
    float* out;
    int C, hop, n_max;
    const int32_t* slots;
    const int32_t* conceal;
    int hold, fade, recover, M;  // hold in samples
    float invM;
};

template <int V>
__global__ __launch_bounds__(256) void stream_conceal_out_kernel(ScOut a) {
    const int row = blockIdx.y, b = row / a.C, c = row - b * a.C;
    const int S = a.n_max * a.hop;
    const int i = (blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= S) return;
    const int live = clampi(a.slots[2 * b], 0, a.n_max) * a.hop;
    float* o = a.out + (int64_t)row * S + i;
    float v[V];
    if (i >= live) {  // hop % V == 0: the whole quad lies past the slot's count, and nothing is read
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = 0.f;
    } else {
        const float* x = a.x + b * a.x_b + c * a.x_c + i;
        if constexpr (V == 4) {
            const f32x4 q = *(const f32x4*)x;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = q[e];
        } else {
            v[0] = x[0];
        }
        const bool lost = a.conceal[4 * b] != 0;
        const int64_t p0 = clampi(a.conceal[4 * b + 1], 0, a.M);
        const int64_t r0 = a.conceal[4 * b + 2] < 0 ? 0 : a.conceal[4 * b + 2];
        const int64_t before = r0 > a.hold ? r0 - a.hold : 0;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int64_t j1 = (int64_t)(i + e) + 1;
            int64_t p;
            if (lost) {
                const int64_t r = r0 + j1;
                const int64_t dec = (r > a.hold ? r - a.hold : 0) - before;
                p = p0 - a.recover * dec;
                p = p < 0 ? 0 : p;
            } else {
                p = p0 + a.fade * j1;
                p = p > a.M ? a.M : p;
            }
            if (p != a.M) v[e] = v[e] * ((float)p * a.invM);
        }
    }
    if constexpr (V == 4) {
        f32x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = v[e];
        *(f32x4*)o = q;
    } else {
        o[0] = v[0];
    }
}

}  // namespace

extern "C" {

int encx_stream_conceal_fill(float* win, int64_t w_b, int64_t w_d, int64_t B, int64_t D, int64_t P, int64_t n_max,
                             const int32_t* slots, const int32_t* conceal, encx_stream_t stream) {
    ENCX_REQUIRE(win && slots && conceal);
    ENCX_REQUIRE(B >= 1 && B <= 64 && D >= 1 && D <= (1 << 20) && P >= 1 && P <= 64 && n_max >= 1 && n_max <= 255);
    ENCX_REQUIRE(w_d >= P + n_max && w_b >= D * w_d);
    encx_prof_scope ps((hipStream_t)stream, 0.0, 4.0 * B * D * (n_max + 1), "stream_conceal_fill", false);
    hipLaunchKernelGGL(stream_conceal_fill_kernel, dim3((unsigned)cdiv(B * D, 4)), dim3(256), 0, (hipStream_t)stream,
                       win, w_b, w_d, (int)B, (int)D, (int)P, (int)n_max, slots, conceal);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_stream_conceal_out(const float* x, int64_t x_b, int64_t x_c, float* out, int64_t B, int64_t C, int64_t hop,
                            int64_t n_max, const int32_t* slots, const int32_t* conceal, int64_t hold_frames,
                            int64_t fade_frames, int64_t recover_frames, encx_stream_t stream) {
    ENCX_REQUIRE(x && out && slots && conceal);
    ENCX_REQUIRE(B >= 1 && B <= 64 && C >= 1 && C <= 1024 && hop >= 1 && hop <= (1 << 16) && n_max >= 1 &&
                 n_max <= 255);
    ENCX_REQUIRE(hold_frames >= 0 && hold_frames <= 255 && fade_frames >= 1 && fade_frames <= 255 &&
                 recover_frames >= 1 && recover_frames <= 255);
    const int64_t M = fade_frames * recover_frames * hop, S = n_max * hop;
    ENCX_REQUIRE(M <= (1 << 24));  // float(p) is exact for every p in 0..M
    ENCX_REQUIRE(x_c >= S && x_b >= C * x_c);
    encx_prof_scope ps((hipStream_t)stream, 2.0 * B * C * S, 8.0 * B * C * S, "stream_conceal_out", false);
    ScOut a{x, x_b, x_c, out, (int)C, (int)hop, (int)n_max, slots, conceal, (int)(hold_frames * hop),
            (int)fade_frames, (int)recover_frames, (int)M, 1.0f / (float)M};
    const bool quads = hop % 4 == 0 && x_b % 4 == 0 && x_c % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (quads) {
        hipLaunchKernelGGL(stream_conceal_out_kernel<4>, dim3((unsigned)cdiv(S / 4, 256), (unsigned)(B * C)), dim3(256),
                           0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(stream_conceal_out_kernel<1>, dim3((unsigned)cdiv(S, 256), (unsigned)(B * C)), dim3(256), 0,
                           (hipStream_t)stream, a);
    }
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
