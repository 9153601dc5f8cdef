// MS-STFT discriminator (msstftd.py:28-149): its spectrogram and its losses (losses.py:44-80) on
// gfx950. Its NormConv2d layers are in conv2d.h and conv2d_{fwd,dgrad,wgrad}.hip.
//
//   spectrogram  torchaudio Spectrogram(normalized, center=False, power=None) as a DFT GEMM:
//                frames gathered from the waveform while staging, [w cos | -w sin] table
//                shared with the mel loss; the epilogue writes the cat([re, im]) and
//                'b c w t -> b c t w' layout directly. Backward: the transposed GEMM + a
//                fixed-order overlap-add.
//   losses       the hinge and feature-matching losses as fixed-order two-stage reductions, and
//                their grads.
#include "common.h"
#include "gemm.h"
#include "fft.h"
#include "prof.h"

namespace {

// ---------------------------------------------------------------------------- spectrogram
struct LdSpecD {  // A(m = (bc, fr), k) = x[bc][fr*hop + k]; B = DFT table [n][2nb]
    // (scalar staging: the quad form measured 4 % slower here)
    static constexpr bool A_K_FAST = true, B_N_FAST = true, VEC = false;
    const float* x;
    const float* bt;
    int T, Fr, hop, nb2;
    FastDiv fFr;
    ENCX_DEV float a(int m, int k) const {
        const int bc = (int)fdiv((uint32_t)m, fFr), fr = m - bc * Fr;
        return x[(int64_t)bc * T + (int64_t)fr * hop + k];
    }
    ENCX_DEV float b(int k, int n) const { return bt[(int64_t)k * nb2 + n]; }
    ENCX_DEV f32x4 a4(int m, int k) const {  // k..k+3 of one frame (k + 3 < n_fft)
        const int bc = (int)fdiv((uint32_t)m, fFr), fr = m - bc * Fr;
        return ld4u(x + (int64_t)bc * T + (int64_t)fr * hop + k);
    }
    ENCX_DEV f32x4 b4(int k, int n) const { return ld4u(bt + (int64_t)k * nb2 + n); }
};
struct EpSpecD {  // z[b][ch][fr][k], ch = c (re) or C + c (im)
    float* z;
    int C, Fr, nb;
    float inv;
    ENCX_DEV void operator()(int m, int n, float v) const {
        const int bc = m / Fr, fr = m - bc * Fr, b = bc / C, c = bc - b * C;
        const int im = n >= nb, k = im ? n - nb : n, ch = im ? C + c : c;
        z[(((int64_t)b * 2 * C + ch) * Fr + fr) * nb + k] = v * inv;
    }
};
struct LdSpecDB {  // A(m = (bc, fr), col) = dz at col; B(col, t) = bt[t][col]
    static constexpr bool A_K_FAST = true, B_N_FAST = false, VEC = true;
    const float* dz;
    const float* bt;
    int C, Fr, nb, nb2;
    float inv;
    ENCX_DEV float a(int m, int col) const {
        const int bc = m / Fr, fr = m - bc * Fr, b = bc / C, c = bc - b * C;
        const int im = col >= nb, k = im ? col - nb : col, ch = im ? C + c : c;
        return dz[(((int64_t)b * 2 * C + ch) * Fr + fr) * nb + k] * inv;
    }
    ENCX_DEV float b(int col, int t) const { return bt[(int64_t)t * nb2 + col]; }
    ENCX_DEV f32x4 a4(int m, int col) const {
        if (col < nb && col + 3 >= nb) {  // the quad straddles the re / im boundary
            f32x4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = a(m, col + q);
            return v;
        }
        const int bc = m / Fr, fr = m - bc * Fr, b = bc / C, c = bc - b * C;
        const int im = col >= nb, k = im ? col - nb : col, ch = im ? C + c : c;
        const f32x4 v = ld4u(dz + (((int64_t)b * 2 * C + ch) * Fr + fr) * nb + k);
        return (f32x4){v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv};
    }
    ENCX_DEV f32x4 b4(int col, int t) const { return ld4u(bt + (int64_t)t * nb2 + col); }
};
struct EpFrames {
    float* out;
    int n;
    ENCX_DEV void operator()(int m, int t, float v) const { out[(int64_t)m * n + t] = v; }
};
// dx[bc][t] (+)= sum_{fr: 0 <= t - fr*hop < n} frames[bc*Fr + fr][t - fr*hop], fr ascending
__global__ void spec_overlap_add(const float* frames, float* dx, int BC, int T, int Fr, int n, int hop,
                                 int acc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)BC * T) return;
    const int bc = (int)(i / T), t = (int)(i - (int64_t)bc * T);
    int lo = t - n + 1;
    lo = lo <= 0 ? 0 : (lo + hop - 1) / hop;
    const int hi = min(Fr - 1, t / hop);
    float s = 0.f;
    for (int fr = lo; fr <= hi; ++fr) s += frames[((int64_t)bc * Fr + fr) * n + (t - fr * hop)];
    dx[i] = acc ? dx[i] + s : s;
}

// ---------------------------------------------------------------------------- losses
// sums[0] += sum relu(1 + s*x) over n (s = -1: generator / real term, +1: fake term)
__global__ __launch_bounds__(256) void hinge_kernel(const float* x, int64_t n, float s, float* parts) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        acc += fmaxf(1.f + s * x[i], 0.f);
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = acc;
}
// parts[b] = (sum |fr - ff|, sum |fr|) over a grid-stride slice: float4 loads, 4 in flight per
// operand and thread (n % 4 == 0, 16-byte aligned maps: torch allocations of 32-channel maps)
template <bool CODE>
__global__ __launch_bounds__(256) void feat_kernel(const float* fr, const float* ff, int64_t n, float* parts,
                                                   uint32_t* code) {
    __shared__ float red[16];
    const f32x4* r4 = (const f32x4*)fr;
    const f32x4* f4 = (const f32x4*)ff;
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
    float s1 = 0.f, s2 = 0.f;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += 4 * stride) {
        f32x4 rv[4], fv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * stride;
            const int64_t ic = i < n4 ? i : 0;
            rv[u] = r4[ic];
            fv[u] = f4[ic];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u * stride < n4) {
                uint32_t cw = 0;  // CODE: 4 bytes, one per element (conv2d_dgrad.hip: code_term / code_mask)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = fv[u][c] - rv[u][c];
                    s1 += fabsf(rv[u][c] - fv[u][c]);
                    s2 += fabsf(rv[u][c]);
                    cw |= ((d > 0.f ? 1u : (d < 0.f ? 2u : 0u)) | (fv[u][c] > 0.f ? 4u : 0u)) << (8 * c);
                }
                if (CODE) code[i0 + u * stride] = cw;
            }
        }
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        parts[2 * blockIdx.x] = s1;
        parts[2 * blockIdx.x + 1] = s2;
    }
}
constexpr int LP = 512;  // partial blocks of the loss reductions
// out[0] (+)= scale * sum(parts[0::stride]) / (stride == 2 ? sum(parts[1::2]) : n)
__global__ __launch_bounds__(256) void loss_finish(const float* parts, int np, int stride, double n,
                                                   float scale, float* out, float* denom, int acc) {
    __shared__ float red[16];
    float a = 0.f, d = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) {
        a += parts[i * stride];
        if (stride == 2) d += parts[i * stride + 1];
    }
    a = block_sum(a, red);
    d = block_sum(d, red);
    if (threadIdx.x == 0) {
        const float den = stride == 2 ? d : (float)n;
        const float v = scale * (a / den);
        out[0] = acc ? out[0] + v : v;
        if (denom) denom[0] = den;
    }
}
// grad of scale * mean(relu(1 + s*x)): scale * s / n where 1 + s*x > 0; g0 = upstream scalar
__global__ void hinge_grad_kernel(const float* x, int64_t n, float s, float scale, const float* g0,
                                  float* dx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = (g0 ? g0[0] : 1.f) * scale * s / (float)n;
    dx[i] = (1.f + s * x[i] > 0.f) ? g : 0.f;
}
// grad wrt ff of scale * sum|fr - ff| / sum|fr| (the reference's l1 / mean|fr| ratio)
__global__ void feat_grad_kernel(const float* fr, const float* ff, int64_t n, float scale,
                                 const float* denom, const float* g0, float* dff) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = (g0 ? g0[0] : 1.f) * scale / denom[0];
    const float d = ff[i] - fr[i];
    dff[i] = d > 0.f ? g : (d < 0.f ? -g : 0.f);
}

}  // namespace

extern "C" {

/* Spectrogram of DiscriminatorSTFT (msstftd.py:62-64, 97-99): x [B][C][T] -> z [B][2C][Fr][nb]
 * (channels re_0..re_{C-1}, im_0..im_{C-1}), Fr = (T - n)/hop + 1, nb = n/2 + 1, scaled by
 * 1/sqrt(sum w^2) (normalized=True). tables: the mel-table layout of n (encx_mel_tables_init). */
// option FFT = 0: the spectrogram as the framed DFT GEMM (round 3) instead of the real FFT (fft.h)
static bool disc_fft(int64_t n) {
    return encx_opt(OPT_FFT) != 0 && encx_fft::fft_ok(n);
}

static double hann_norm(int64_t n) { return 1.0 / sqrt(3.0 * (double)n / 8.0); }  // sum of periodic hann^2 = 3n/8

int encx_disc_spec_fwd(const float* x, const float* tables, float* z, int64_t B, int64_t C, int64_t T,
                       int64_t n_fft, int64_t hop, encx_stream_t stream) {
    return encx_disc_spec_fwd_scaled(x, tables, z, B, C, T, n_fft, hop, hann_norm(n_fft), stream);
}

int encx_disc_spec_fwd_scaled(const float* x, const float* tables, float* z, int64_t B, int64_t C, int64_t T,
                              int64_t n_fft, int64_t hop, double scale, encx_stream_t stream) {
    ENCX_REQUIRE(x && tables && z && T >= n_fft && hop > 0);
    hipStream_t st = (hipStream_t)stream;
    const int Fr = (int)((T - n_fft) / hop + 1), nb = (int)(n_fft / 2 + 1);
    const float inv = (float)scale;
    const int M = (int)(B * C * Fr), N = 2 * nb, K = (int)n_fft;
    const bool fft = disc_fft(n_fft);
    encx_prof_scope ps(st, fft ? 2.5 * M * K * log2((double)K) : 2.0 * M * N * K, 4.0 * (B * C * T + (int64_t)M * N), "spec_fwd");
    ps.tag(" n%ld", (long)n_fft);
    if (fft) {  // real FFT of each hann-windowed frame (fft.h), written in the (t, f) channel layout
        encx_fft::FftArgs a{x, tables, N, z, (int)T, Fr, (int)hop, 0, M, 1, (int)C, inv};
        return encx_fft::r2c(a, (int)n_fft, st);
    }
    return gemm_launch(LdSpecD{x, tables, (int)T, Fr, (int)hop, N, make_fastdiv((uint32_t)Fr)}, EpSpecD{z, (int)C, Fr, nb, inv}, M, N, K, st);
}

size_t encx_disc_spec_bwd_workspace(int64_t B, int64_t C, int64_t T, int64_t n_fft, int64_t hop) {
    const int64_t Fr = (T - n_fft) / hop + 1;
    return (size_t)(B * C * Fr * n_fft) * sizeof(float);
}

/* dx (+)= d spectrogram^T dz (accumulate: add into dx). ws: encx_disc_spec_bwd_workspace. */
int encx_disc_spec_bwd(const float* dz, const float* tables, float* dx, float* ws, int accumulate, int64_t B,
                       int64_t C, int64_t T, int64_t n_fft, int64_t hop, encx_stream_t stream) {
    return encx_disc_spec_bwd_scaled(dz, tables, dx, ws, accumulate, B, C, T, n_fft, hop, hann_norm(n_fft), stream);
}

int encx_disc_spec_bwd_scaled(const float* dz, const float* tables, float* dx, float* ws, int accumulate,
                              int64_t B, int64_t C, int64_t T, int64_t n_fft, int64_t hop, double scale,
                              encx_stream_t stream) {
    ENCX_REQUIRE(dz && tables && dx && ws && T >= n_fft && hop > 0);
    hipStream_t st = (hipStream_t)stream;
    const int Fr = (int)((T - n_fft) / hop + 1), nb = (int)(n_fft / 2 + 1);
    const float inv = (float)scale;
    const int M = (int)(B * C * Fr), N = (int)n_fft, K = 2 * nb;
    {
        const bool fft = disc_fft(n_fft);
        encx_prof_scope ps(st, fft ? 2.5 * M * N * log2((double)N) : 2.0 * M * N * K,
                           4.0 * ((int64_t)M * K + (int64_t)M * N), "spec_bwd");
        ps.tag(" n%ld", (long)n_fft);
        int rc;
        if (fft) {  // the transpose of the windowed real DFT per frame (fft.h c2r)
            encx_fft::FftArgs a{dz, tables, K, ws, (int)T, Fr, (int)hop, 0, M, 1, (int)C, inv};
            rc = encx_fft::c2r(a, (int)n_fft, st);
        } else {
            rc = gemm_launch(LdSpecDB{dz, tables, (int)C, Fr, nb, K, inv}, EpFrames{ws, N}, M, N, K, st);
        }
        if (rc) return rc;
    }
    const int64_t tot = B * C * T;
    hipLaunchKernelGGL(spec_overlap_add, dim3((unsigned)cdiv(tot, 256)), dim3(256), 0, st, ws, dx, (int)(B * C),
                       (int)T, Fr, (int)n_fft, (int)hop, accumulate);
    ENCX_CHECK_LAUNCH();
    return 0;
}

size_t encx_disc_loss_workspace(void) { return (size_t)2 * LP * sizeof(float); }

/* out[0] (+)= scale * mean(relu(1 + s*x)) over n elements (losses.py:48, 78-79). */
int encx_hinge_loss(const float* x, int64_t n, double s, double scale, float* out, int accumulate, float* ws,
                    encx_stream_t stream) {
    ENCX_REQUIRE(x && out && ws && n > 0);
    encx_prof_scope ps((hipStream_t)stream, 2.0 * n, 4.0 * n, "hinge", false);
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)min((int64_t)LP, cdiv(n, 256));
    hipLaunchKernelGGL(hinge_kernel, dim3(nb), dim3(256), 0, st, x, n, (float)s, ws);
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(256), 0, st, ws, nb, 1, (double)n, (float)scale, out,
                       (float*)nullptr, accumulate);
    ENCX_CHECK_LAUNCH();
    return 0;
}

/* out[0] (+)= scale * mean|fr - ff| / mean|fr| (losses.py:53); denom[0] = sum|fr| for the
 * backward. */
int encx_feat_loss(const float* fr, const float* ff, int64_t n, double scale, float* out, float* denom,
                   int accumulate, float* ws, encx_stream_t stream) {
    ENCX_REQUIRE(fr && ff && out && ws && n > 0 && n % 4 == 0 && ((uintptr_t)fr & 15) == 0 && ((uintptr_t)ff & 15) == 0);
    encx_prof_scope ps((hipStream_t)stream, 4.0 * n, 8.0 * n, "feat", false);
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)min((int64_t)LP, cdiv(n, 1024));
    hipLaunchKernelGGL(feat_kernel<false>, dim3(nb), dim3(256), 0, st, fr, ff, n, ws, (uint32_t*)nullptr);
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(256), 0, st, ws, nb, 2, (double)n, (float)scale, out, denom,
                       accumulate);
    ENCX_CHECK_LAUNCH();
    return 0;
}

/* encx_feat_loss + the pair's per-element code (code[i] = [ff > fr] | 2 [ff < fr] | 4 [ff > 0], one
 * byte per element, 4-byte aligned), which encx_conv2d_bwd_data_feat reads instead of the two maps. */
int encx_feat_loss_code(const float* fr, const float* ff, int64_t n, double scale, float* out, float* denom,
                        int accumulate, float* ws, uint8_t* code, encx_stream_t stream) {
    ENCX_REQUIRE(fr && ff && out && ws && code && n > 0 && n % 4 == 0 && ((uintptr_t)fr & 15) == 0 &&
                 ((uintptr_t)ff & 15) == 0 && ((uintptr_t)code & 3) == 0);
    encx_prof_scope ps((hipStream_t)stream, 4.0 * n, 9.0 * n, "feat", false);
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)min((int64_t)LP, cdiv(n, 1024));
    hipLaunchKernelGGL(feat_kernel<true>, dim3(nb), dim3(256), 0, st, fr, ff, n, ws, (uint32_t*)code);
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(256), 0, st, ws, nb, 2, (double)n, (float)scale, out, denom,
                       accumulate);
    ENCX_CHECK_LAUNCH();
    return 0;
}

/* dx = g0[0] * scale * s / n * [1 + s*x > 0]  (g0 may be NULL: 1) */
int encx_hinge_loss_bwd(const float* x, int64_t n, double s, double scale, const float* g0, float* dx,
                        encx_stream_t stream) {
    ENCX_REQUIRE(x && dx && n > 0);
    encx_prof_scope ps((hipStream_t)stream, 2.0 * n, 8.0 * n, "hinge_bwd", false);
    hipLaunchKernelGGL(hinge_grad_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n,
                       (float)s, (float)scale, g0, dx);
    ENCX_CHECK_LAUNCH();
    return 0;
}

/* dff = g0[0] * scale * sign(ff - fr) / denom[0] */
int encx_feat_loss_bwd(const float* fr, const float* ff, int64_t n, double scale, const float* denom,
                       const float* g0, float* dff, encx_stream_t stream) {
    ENCX_REQUIRE(fr && ff && denom && dff && n > 0);
    encx_prof_scope ps((hipStream_t)stream, 2.0 * n, 12.0 * n, "feat_bwd", false);
    hipLaunchKernelGGL(feat_grad_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, fr, ff, n,
                       (float)scale, denom, g0, dff);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"

