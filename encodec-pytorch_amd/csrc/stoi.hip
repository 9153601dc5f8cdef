// encx -- short-time objective intelligibility (STOI; Taal, Hendriks, Heusdens, Jensen 2011), the
// measure cal_metrics.py:57-63 takes from a CPU library, for a batch of (clean x, degraded y) rows
// at 10 kHz. Per row (len samples; NF 256, HOP 128, NFFT 512, J 15 bands, N 30 frames, DYN 40 dB,
// w = hanning(258)[1:-1]):
//   1. F = ceil((len - NF) / HOP) frames at i HOP; e_i = 20 log10(||w x_i|| + EPS);
//   2. frames with e_i > max e - DYN are kept (k_0 < ... < k_{n-1}); the compacted x and y are the
//      overlap-add of their kept windowed frames at spacing HOP;
//   3. M = n - 1 frames of the compacted signals, windowed again, 512-point real FFT, and the
//      square root of the power summed over each third-octave band -> X[j][m], Y[j][m];
//   4. for every 30-frame segment and band the correlation of x_s with the clipped, rescaled y_s;
//      the score is their mean, or 1e-5 when M < N.
// Five launches, none of which waits for the host: the kept count stays on the device, grids are
// sized from the upper bound F(T) and surplus workgroups leave.
//   stoi_energy  one wave per frame: ||w x_i||
//   stoi_mask    one workgroup per row: the row maximum, then the kept indices by an ordered scan
//   stoi_bands   2 analysis frames of x and the same 2 of y per workgroup, the four as one call of
//                the LDS real FFT of fft.h (m = 256); the power spectra go to the FFT's idle
//                buffer. The compacted signal is never stored: with the same hop
//                and window in steps 2 and 3, sample t of analysis frame m is
//                  t < 128:  w[t + 128] x[k_{m-1} HOP + t + 128] + w[t] x[k_m HOP + t]   (no first term at m = 0)
//                  t >= 128: w[t] x[k_m HOP + t] + w[t - 128] x[k_{m+1} HOP + t - 128]
//   stoi_score   64 segments x 15 bands per workgroup from an LDS tile of X and Y; one thread per
//                (segment, band) holds its 30 + 30 values in registers and works in fp64
//   stoi_finish  one workgroup per row: the tile sums in tile order, the mean
// Step 2's test is done on the norms, (||w x_i|| + EPS) > (max + EPS) 10^(-DYN/20): the same
// inequality without two logarithms' roundings. Every sum runs in a fixed order (per-lane runs,
// then xor butterflies; tile partials in fp64 in tile order), there are no atomics, and a tile's
// extent never depends on T or B, so a row's bits do not depend on the batch around it.
#include "common.h"
#include "fft.h"

#include <cmath>

namespace {

constexpr int NF = 256, HOP = 128, NBAND = 15, NSEG = 30;
constexpr int64_t STOI_TMAX = (int64_t)1 << 22;
constexpr float STOI_EPS = 2.220446049250313e-16f;   // 2^-52
constexpr double STOI_EPS_D = 2.220446049250313e-16;
constexpr float STOI_DYN = 0.01f;                     // 10^(-40 / 20)
constexpr double STOI_CLIP = 1.0 + 5.623413251903491; // 1 + 10^(15 / 20)
constexpr int NT = 256;
static_assert(NT == NF, "stoi_bands_kernel: one thread per frame sample");
// analysis frames per stoi_bands workgroup: their x and y frames are 4 transforms of 256 complex
// points, one radix-4 butterfly per thread and stage, in 19.5 KiB of LDS (8 workgroups per CU).
// Measured at 64 rows x 10 s: 4 per workgroup (35 KiB, 4 workgroups per CU) is 24 % slower
constexpr int FPW = 2;
constexpr int SEG_TILE = 64;  // segments per stoi_score workgroup
constexpr int SEG_SPAN = SEG_TILE + NSEG - 1;  // band frames a tile reads (93)
constexpr int SEG_LD = 96;

// band j sums the power of bins [BAND_LO[j], BAND_HI[j]): the bins nearest to
// 150 * 2^((2j -+ 1) / 6) Hz on the 10000 / 512 Hz grid
__device__ const int BAND_LO[NBAND] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
__device__ const int BAND_HI[NBAND] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// w[t] = hanning(258)[1 + t], from fp64 once per device (a setup launch before the first call)
__device__ float g_win[NF];
__global__ void stoi_win_kernel() {
    const int t = threadIdx.x;
    g_win[t] = (float)(0.5 - 0.5 * cospi(2.0 * (double)(t + 1) / 257.0));
}
int stoi_ready(hipStream_t st) {
    static bool done[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return ENCX_EINVAL;
    if (done[dev]) return 0;
    hipLaunchKernelGGL(stoi_win_kernel, dim3(1), dim3(NF), 0, st);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) done[dev] = true;
    return (int)e;
}

inline int64_t stoi_frames(int64_t len) { return len <= NF ? 0 : (len - NF + HOP - 1) / HOP; }

struct StoiArgs {
    const float* x;
    const float* y;
    const int64_t* lengths;  // null: T for every row
    int* cnt;      // [B] kept frames n
    float* nrm;    // [B][F] ||w x_i||
    int* kept;     // [B][F] kept frame indices, ascending
    float* bands;  // [B][2][NBAND][Mp] X, then Y
    double* part;  // [B][nseg_tiles] tile sums of the segment correlations
    float* out;    // [B]
    int T, F, Mp, frame_tiles, band_tiles, seg_tiles;
};

ENCX_DEV int row_len(const StoiArgs& a, int row) {
    if (!a.lengths) return a.T;
    const int64_t l = a.lengths[row];
    return l < 0 ? 0 : (l > a.T ? a.T : (int)l);
}
ENCX_DEV int row_frames(int len) { return len <= NF ? 0 : (len - NF + HOP - 1) / HOP; }

// one wave per frame: lane l sums (w x)^2 at t = l, l + 64, l + 128, l + 192 in that order, then
// the xor butterfly (every lane ends with the same bits)
__global__ __launch_bounds__(NT) void stoi_energy_kernel(StoiArgs a) {
    const int row = blockIdx.x / a.frame_tiles, tile = blockIdx.x - row * a.frame_tiles;
    const int Fb = row_frames(row_len(a, row));
    const int i = tile * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= Fb) return;  // wave-uniform
    const float* xr = a.x + (int64_t)row * a.T + (int64_t)i * HOP;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < NF / 64; ++q) {
        const float v = g_win[lane + 64 * q] * xr[lane + 64 * q];
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) a.nrm[(int64_t)row * a.F + i] = sqrtf(s);
}

// one workgroup per row: max of the norms (exact in any order), the threshold, then the kept
// indices in ascending order, 256 frames per pass (ballot + popcount within a wave, the four
// wave totals through LDS)
__global__ __launch_bounds__(NT) void stoi_mask_kernel(StoiArgs a) {
    __shared__ float smax[NT / 64];
    __shared__ int stot[NT / 64];
    const int row = blockIdx.x;
    const int Fb = row_frames(row_len(a, row));
    const float* nr = a.nrm + (int64_t)row * a.F;
    int* kp = a.kept + (int64_t)row * a.F;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float mx = 0.f;
    for (int i = threadIdx.x; i < Fb; i += NT) mx = fmaxf(mx, nr[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) smax[w] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    const float thr = (mx + STOI_EPS) * STOI_DYN;
    int run = 0;
    for (int base = 0; base < Fb; base += NT) {  // Fb is uniform over the workgroup
        const int i = base + threadIdx.x;
        const bool keep = i < Fb && nr[i] + STOI_EPS > thr;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();  // the previous pass's reads of stot are done
        if (lane == 0) stot[w] = __popcll(bal);
        __syncthreads();
        int off = run;
        for (int q = 0; q < w; ++q) off += stot[q];
        if (keep) kp[off + before] = i;  // off + before < number kept so far <= Fb
        run += stot[0] + stot[1] + stot[2] + stot[3];
    }
    if (threadIdx.x == 0) a.cnt[row] = run;
}

// analysis frames m0 .. m0 + AF - 1 of the row: x's frames and y's frames are the 2 AF transforms of
// one stockham call (frames [0, AF) x, [AF, 2 AF) y)
template <int AF>
__global__ __launch_bounds__(NT) void stoi_bands_kernel(StoiArgs a) {
    using namespace encx_fft;
    constexpr int M = 256, N = 512, NB = M + 1, NFR = 2 * AF;
    constexpr int LANES = NT / (NFR * 16);  // lanes per (frame, band) sum; 16 band slots per frame
    static_assert(LANES == 2 || LANES == 4, "stoi_bands_kernel: AF is 2 or 4");
    static_assert(NFR * NB * sizeof(float) <= NFR * M * sizeof(f2v), "the spectra fit the idle FFT buffer");
    __shared__ f2v buf[2 * NFR * M];
    __shared__ f2v tw[M + 1];
    __shared__ float Win[NF];
    __shared__ int Kp[AF + 2];  // k_{m0-1} .. k_{m0+AF}
    const int row = blockIdx.x / a.band_tiles, tile = blockIdx.x - row * a.band_tiles;
    const int n = a.cnt[row], Mb = n > 0 ? n - 1 : 0, m0 = tile * AF;
    if (m0 >= Mb) return;  // uniform: before any barrier
    make_twiddles<M>(tw, -1.f);
    Win[threadIdx.x] = g_win[threadIdx.x];
    if (threadIdx.x < AF + 2) {
        const int m = m0 - 1 + (int)threadIdx.x;
        Kp[threadIdx.x] = (m >= 0 && m < n) ? a.kept[(int64_t)row * a.F + m] : 0;
    }
    __syncthreads();
    float* bufr = reinterpret_cast<float*>(buf);
    {
        // thread t fills sample t of every frame (NT == NF) and zeroes sample NF + t. All 2 NFR
        // loads go out before the first is used: each address is inside the row whatever m is
        // (a kept frame k ends at k HOP + NF - 1 < len <= T, and Kp is 0 past the kept list), and
        // what a frame past Mb or a missing neighbour loaded is dropped by a select
        const int t = threadIdx.x;
        const bool first = t < HOP;  // wave-uniform
        const int t2 = first ? t + HOP : t - HOP;
        const float wc = Win[t], wo = Win[t2];
        float cv[NFR], ov[NFR];
#pragma unroll
        for (int fr = 0; fr < NFR; ++fr) {
            const int f = fr % AF;
            const float* src = (fr < AF ? a.x : a.y) + (int64_t)row * a.T;
            cv[fr] = src[Kp[f + 1] * HOP + t];
            ov[fr] = src[Kp[first ? f : f + 2] * HOP + t2];
        }
#pragma unroll
        for (int fr = 0; fr < NFR; ++fr) {
            const int f = fr % AF, m = m0 + f;
            const float c = wc * cv[fr];
            const float o = (first && m == 0) ? 0.f : wo * ov[fr];  // m + 1 <= n - 1 for m < Mb
            bufr[fr * N + t] = m < Mb ? (o + c) * wc : 0.f;  // packed z[j] = v[2j] + i v[2j + 1]
            bufr[fr * N + NF + t] = 0.f;                     // zeros past the frame
        }
    }
    __syncthreads();
    const int res = stockham<M, NFR>(buf, tw);
    const f2v* Z = buf + res * (NFR * M);
    // power spectra into the FFT's idle buffer; the odd row stride spreads the band runs over the banks
    float* Ps = reinterpret_cast<float*>(buf + (res ^ 1) * (NFR * M));
    for (int q = threadIdx.x; q < NFR * NB; q += NT) {
        const int fr = q / NB, k = q - fr * NB;
        const f2v zk = Z[fr * M + (k & (M - 1))], zm = cconj(Z[fr * M + ((M - k) & (M - 1))]);
        const f2v e = (zk + zm) * 0.5f, o = (zk - zm) * 0.5f;
        const f2v tt = cmul(tw[k], o);
        const float re = e[0] + tt[1], im = e[1] - tt[0];
        Ps[q] = re * re + im * im;
    }
    __syncthreads();
    // one (frame, band) sum per LANES lanes: an equal run of the band's bins in bin order per
    // lane, then the xor butterfly
    const int task = threadIdx.x / LANES, part = threadIdx.x % LANES;
    const int fr = task >> 4, j = task & 15, f = fr % AF;
    const bool on = j < NBAND;
    float s = 0.f;
    if (on) {
        const int lo = BAND_LO[j], wd = BAND_HI[j] - lo, ch = (wd + LANES - 1) / LANES;
        const int k1 = min(wd, (part + 1) * ch);
        for (int k = part * ch; k < k1; ++k) s += Ps[fr * NB + lo + k];
    }
#pragma unroll
    for (int o = 1; o < LANES; o <<= 1) s += __shfl_xor(s, o, 64);
    if (on && part == 0 && m0 + f < Mb)
        a.bands[(((int64_t)row * 2 + (fr < AF ? 0 : 1)) * NBAND + j) * a.Mp + m0 + f] = sqrtf(s);
}

// segments q0 .. q0 + 63 of the row (segment q covers band frames [q, q + 30))
__global__ __launch_bounds__(NT) void stoi_score_kernel(StoiArgs a) {
    __shared__ float Xs[NBAND * SEG_LD], Ys[NBAND * SEG_LD];
    __shared__ double Ds[NBAND * SEG_TILE];
    const int row = blockIdx.x / a.seg_tiles, tile = blockIdx.x - row * a.seg_tiles;
    const int n = a.cnt[row], Mb = n > 0 ? n - 1 : 0, S = Mb - NSEG + 1, q0 = tile * SEG_TILE;
    if (q0 >= S) return;  // uniform (also S <= 0)
    const float* bx = a.bands + (int64_t)row * 2 * NBAND * a.Mp;
    const float* by = bx + (int64_t)NBAND * a.Mp;
    for (int i = threadIdx.x; i < NBAND * SEG_LD; i += NT) {
        const int j = i / SEG_LD, m = q0 + (i - j * SEG_LD);
        const bool in = m < Mb;  // Mb <= Mp
        Xs[i] = in ? bx[(int64_t)j * a.Mp + m] : 0.f;
        Ys[i] = in ? by[(int64_t)j * a.Mp + m] : 0.f;
    }
    __syncthreads();
    const int sl = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = w; j < NBAND; j += NT / 64) {
        double d = 0.0;
        if (q0 + sl < S) {
            double xs[NSEG], ys[NSEG];
            double sx = 0.0, sy = 0.0;
#pragma unroll
            for (int i = 0; i < NSEG; ++i) {
                xs[i] = (double)Xs[j * SEG_LD + sl + i];
                ys[i] = (double)Ys[j * SEG_LD + sl + i];
                sx = fma(xs[i], xs[i], sx);
                sy = fma(ys[i], ys[i], sy);
            }
            const double alpha = sqrt(sx) / (sqrt(sy) + STOI_EPS_D);
            double mx = 0.0, my = 0.0;
#pragma unroll
            for (int i = 0; i < NSEG; ++i) {
                ys[i] = fmin(alpha * ys[i], STOI_CLIP * xs[i]);
                mx += xs[i];
                my += ys[i];
            }
            mx /= NSEG;
            my /= NSEG;
            double nx = 0.0, ny = 0.0, xy = 0.0;
#pragma unroll
            for (int i = 0; i < NSEG; ++i) {
                const double xc = xs[i] - mx, yc = ys[i] - my;
                nx = fma(xc, xc, nx);
                ny = fma(yc, yc, ny);
                xy = fma(xc, yc, xy);
            }
            d = xy / ((sqrt(nx) + STOI_EPS_D) * (sqrt(ny) + STOI_EPS_D));
        }
        Ds[j * SEG_TILE + sl] = d;
    }
    __syncthreads();
    if (w == 0) {  // the tile's sum: each segment's bands in band order, then the butterfly
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NBAND; ++j) s += Ds[j * SEG_TILE + sl];
        s = wave_sum_d(s);
        if (sl == 0) a.part[(int64_t)row * a.seg_tiles + tile] = s;
    }
}

// one workgroup per row: thread t sums tiles t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(NT) void stoi_finish_kernel(StoiArgs a) {
    __shared__ double red[NT / 64];
    const int row = blockIdx.x;
    const int n = a.cnt[row], Mb = n > 0 ? n - 1 : 0, S = Mb - NSEG + 1;
    if (S <= 0) {  // fewer than N frames: the published implementation's warning value
        if (threadIdx.x == 0) a.out[row] = 1e-5f;
        return;
    }
    const int tiles = (S + SEG_TILE - 1) / SEG_TILE;  // <= seg_tiles: the ones stoi_score wrote
    double s = 0.0;
    for (int t = threadIdx.x; t < tiles; t += NT) s += a.part[(int64_t)row * a.seg_tiles + t];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        a.out[row] = (float)(((red[0] + red[1]) + (red[2] + red[3])) / ((double)NBAND * (double)S));
}

// workspace layout in 4-byte words: cnt [B] | pad to even | part [B][seg_tiles] fp64 |
// nrm [B][F] | kept [B][F] | bands [B][2][15][Mp]
struct StoiPlan {
    int64_t F, Mp, seg_tiles, o_part, o_nrm, o_kept, o_bands, total;
};
bool stoi_plan(int64_t B, int64_t T, StoiPlan& p) {
    if (B < 0 || T < 0 || T > STOI_TMAX || B > INT32_MAX / 2) return false;
    p.F = stoi_frames(T);
    p.Mp = p.F > 0 ? p.F - 1 : 0;
    const int64_t S = p.Mp - NSEG + 1;
    p.seg_tiles = S > 0 ? cdiv(S, SEG_TILE) : 0;
    p.o_part = (B + 1) & ~(int64_t)1;
    p.o_nrm = p.o_part + 2 * B * p.seg_tiles;
    p.o_kept = p.o_nrm + B * p.F;
    p.o_bands = p.o_kept + B * p.F;
    p.total = p.o_bands + B * 2 * NBAND * p.Mp;
    // every launch's grid (rows x tiles) must fit 31 bits; stoi_bands has the most tiles
    static_assert(FPW <= NT / 64, "stoi_plan: the bands grid is the largest");
    return B * std::max<int64_t>(cdiv(p.F, FPW), 1) <= INT32_MAX;
}

}  // namespace

extern "C" {

int64_t encx_stoi_frames(int64_t len) { return len < 0 ? -1 : stoi_frames(len); }

int64_t encx_stoi_workspace_floats(int64_t B, int64_t T) {
    StoiPlan p;
    return stoi_plan(B, T, p) ? p.total : -1;
}

int encx_stoi(const float* x, const float* y, const int64_t* lengths, float* ws, float* out, int64_t B, int64_t T,
              encx_stream_t stream) {
    StoiPlan p;
    ENCX_REQUIRE(stoi_plan(B, T, p));
    if (B == 0) return 0;
    ENCX_REQUIRE(x && y && ws && out && ((uintptr_t)ws & 7) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = stoi_ready(st)) return rc;
    if (const int rc = encx_fft::tw_ready(st)) return rc;
    StoiArgs a;
    a.x = x; a.y = y; a.lengths = lengths; a.out = out;
    a.cnt = reinterpret_cast<int*>(ws);
    a.part = reinterpret_cast<double*>(ws + p.o_part);
    a.nrm = ws + p.o_nrm;
    a.kept = reinterpret_cast<int*>(ws + p.o_kept);
    a.bands = ws + p.o_bands;
    a.T = (int)T; a.F = (int)p.F; a.Mp = (int)p.Mp;
    a.frame_tiles = (int)cdiv(p.F, NT / 64);
    a.band_tiles = (int)cdiv(p.Mp, FPW);
    a.seg_tiles = (int)p.seg_tiles;
    const unsigned b = (unsigned)B;
    if (a.frame_tiles > 0) {
        hipLaunchKernelGGL(stoi_energy_kernel, dim3(b * a.frame_tiles), dim3(NT), 0, st, a);
        ENCX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(stoi_mask_kernel, dim3(b), dim3(NT), 0, st, a);
    ENCX_CHECK_LAUNCH();
    if (a.seg_tiles > 0) {  // a row shorter than N + 1 frames scores 1e-5 whatever its bands are
        hipLaunchKernelGGL(stoi_bands_kernel<FPW>, dim3(b * a.band_tiles), dim3(NT), 0, st, a);
        ENCX_CHECK_LAUNCH();
        hipLaunchKernelGGL(stoi_score_kernel, dim3(b * a.seg_tiles), dim3(NT), 0, st, a);
        ENCX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(stoi_finish_kernel, dim3(b), dim3(NT), 0, st, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
