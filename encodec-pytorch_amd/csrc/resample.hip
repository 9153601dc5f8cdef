// encx -- sample-rate conversion with the channel conversion of convert_audio fused
// (utils.py:84-97: mean / expand, then torchaudio.transforms.Resample(sr, target_sr) with its
// defaults: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).
//
// With g = gcd(orig, new), o = orig/g, n = new/g, base = min(o, n) * 0.99, width = ceil(6 o / base)
// and taps = 2 width + o, torchaudio runs a stride-o conv1d with n output channels of `taps`
// coefficients each:  y[i n + p] = sum_t table[p][t] x[i o + t - width]  (x = 0 outside the row),
//   table[p][t] = sinc(pi tau) cos^2(pi tau / 12) base / o,  tau = clamp(((t - width)/o - p/n) base, -6, 6).
// For a phase p only the taps with |tau| < 6 differ from cos^2(pi/2) ~ 4e-33: at most
// W = 2 width + 1 consecutive ones of the 2 width + o (25 of 171 at 44.1 -> 24 kHz, 15 of 174 at
// 48 -> 44.1 kHz). The table here is that compact form: per phase W coefficients and the tap
// `start[p]` of the first, so the sum costs W multiply-adds per output and the kernel is a
// streaming copy: each workgroup stages the input span of its output tile in LDS once (the channel
// mean taken while staging), reads every coefficient from LDS, and writes its outputs coalesced.
// Each output is one fmaf chain over its own W inputs in tap order, whatever the batch or the tile.
#include "common.h"

#include <cmath>

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;      // outputs per workgroup (halved while the input span does not fit)
constexpr int RS_XS_MAX = 10240;   // floats of LDS for the staged input span
constexpr int RS_TAB_MAX = 6144;   // floats of LDS for the table; a larger one is read through L2
constexpr int64_t RS_TAB_LIMIT = (int64_t)1 << 26;  // floats of any table (keeps fdiv's operands below 2^31)
// the launch asks for at most this much dynamic LDS, the limit without hipFuncSetAttribute
static_assert((RS_XS_MAX + RS_TAB_MAX) * sizeof(float) <= 65536, "resample_kernel's LDS request");

struct RsGeo {
    int64_t o, n, width, taps, W;
};
static bool rs_geo(int64_t orig, int64_t neu, RsGeo& g) {
    if (orig <= 0 || neu <= 0 || orig > INT32_MAX || neu > INT32_MAX) return false;
    int64_t a = orig, b = neu;
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    g.o = orig / a;
    g.n = neu / a;
    const double base = (double)std::min(g.o, g.n) * 0.99;
    g.width = (int64_t)std::ceil(6.0 * (double)g.o / base);
    g.taps = 2 * g.width + g.o;
    g.W = 2 * g.width + 1;
    return true;
}
static double rs_tau(const RsGeo& g, int64_t p, int64_t t) {
    const double base = (double)std::min(g.o, g.n) * 0.99;
    return ((double)(t - g.width) / (double)g.o - (double)p / (double)g.n) * base;
}
static float rs_coef(const RsGeo& g, int64_t p, int64_t t) {
    const double base = (double)std::min(g.o, g.n) * 0.99;
    const double tau = std::min(6.0, std::max(-6.0, rs_tau(g, p, t)));
    const double c = std::cos(M_PI * tau / 12.0), a = M_PI * tau;
    return (float)((a == 0.0 ? 1.0 : std::sin(a) / a) * c * c * (base / (double)g.o));
}

struct RsPlan {
    int tile, span, tab_lds;
};
// the largest tile whose input span fits the LDS budget: outputs [j0, j0 + tile) come from at most
// ndi = (tile + n - 2) / n + 1 consecutive input frames i, i.e. (ndi - 1) o + taps samples
static bool rs_plan(const RsGeo& g, RsPlan& pl) {
    if (g.n * (g.W + 1) > RS_TAB_LIMIT) return false;
    pl.tab_lds = g.n * (g.W + 1) <= RS_TAB_MAX;
    for (int tile = RS_TILE; tile >= RS_THREADS; tile >>= 1) {
        const int64_t ndi = (tile + g.n - 2) / g.n + 1, span = (ndi - 1) * g.o + g.taps;
        if (span <= RS_XS_MAX) {
            pl.tile = tile;
            pl.span = (int)span;
            return true;
        }
    }
    return false;
}

struct RsArgs {
    const float* x;
    const float* tab;
    float* y;
    int64_t L, Lout;
    int rows, cin, cout;  // row groups; channels read (averaged) / written (copies) per group
    int o, n, width, W, tile, span;
    FastDiv fn;
};

template <bool TAB_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_sm[];
    float* xs = rs_sm;
    const int nW = a.n * a.W;
    const float* coef = a.tab;
    const int* start = reinterpret_cast<const int*>(a.tab + nW);
    if (TAB_LDS) {
        uint32_t* ts = reinterpret_cast<uint32_t*>(rs_sm + ((a.span + 3) & ~3));
        const uint32_t* tg = reinterpret_cast<const uint32_t*>(a.tab);
        for (int k = threadIdx.x; k < nW + a.n; k += RS_THREADS) ts[k] = tg[k];
        coef = reinterpret_cast<const float*>(ts);
        start = reinterpret_cast<const int*>(ts + nW);
    }
    const int64_t j0 = (int64_t)blockIdx.x * a.tile;
    const int64_t i0 = j0 / a.n;
    const int64_t in0 = i0 * a.o - a.width;            // input position of xs[0]
    const uint32_t jr = (uint32_t)(j0 - i0 * a.n);     // < n
    const int64_t left = a.Lout - j0;
    const int cnt = left < a.tile ? (int)left : a.tile;
    const float fcin = (float)a.cin;
    for (int row = blockIdx.y; row < a.rows; row += gridDim.y) {
        __syncthreads();  // the previous row's reads of xs (and the table's stores) are done
        const float* xr = a.x + (int64_t)row * a.cin * a.L;
        for (int k = threadIdx.x; k < a.span; k += RS_THREADS) {
            const int64_t pos = in0 + k;
            float v = 0.f;
            if (pos >= 0 && pos < a.L) {
                v = xr[pos];
                if (a.cin > 1) {  // wav.mean(-2): the channels summed in order, then / Cin
                    for (int c = 1; c < a.cin; ++c) v += xr[(int64_t)c * a.L + pos];
                    v /= fcin;
                }
            }
            xs[k] = v;
        }
        __syncthreads();
        float* yr = a.y + (int64_t)row * a.cout * a.Lout + j0;
        for (int q = threadIdx.x; q < cnt; q += RS_THREADS) {
            const uint32_t jj = jr + (uint32_t)q;
            const uint32_t di = fdiv(jj, a.fn), p = jj - di * (uint32_t)a.n;
            const float* c = coef + p * a.W;
            const float* xx = xs + di * a.o + start[p];
            float acc = 0.f;
#pragma unroll 5
            for (int k = 0; k < a.W; ++k) acc = fmaf(c[k], xx[k], acc);
            for (int ch = 0; ch < a.cout; ++ch) yr[(int64_t)ch * a.Lout + q] = acc;
        }
    }
}

}  // namespace

extern "C" {

int64_t encx_resample_out_len(int64_t L, int64_t orig, int64_t neu) {
    RsGeo g;
    if (L < 0 || !rs_geo(orig, neu, g)) return -1;
    if (L > INT64_MAX / g.n - 1) return -1;
    return (g.n * L + g.o - 1) / g.o;
}

int64_t encx_resample_table_floats(int64_t orig, int64_t neu) {
    RsGeo g;
    RsPlan pl;
    if (!rs_geo(orig, neu, g) || !rs_plan(g, pl)) return -1;  // a pair encx_resample refuses has no table
    return g.n * (g.W + 1);
}

int encx_resample_table(float* host_table, int64_t orig, int64_t neu) {
    RsGeo g;
    RsPlan pl;
    ENCX_REQUIRE(host_table && rs_geo(orig, neu, g) && rs_plan(g, pl));
    int32_t* start = reinterpret_cast<int32_t*>(host_table + g.n * g.W);
    for (int64_t p = 0; p < g.n; ++p) {
        int64_t s = 0;  // the first tap of phase p inside the window, |tau| < 6
        while (s < g.taps - g.W && !(std::fabs(rs_tau(g, p, s)) < 6.0)) ++s;
        start[p] = (int32_t)s;
        for (int64_t k = 0; k < g.W; ++k) host_table[p * g.W + k] = rs_coef(g, p, s + k);
    }
    return 0;
}

int encx_resample(const float* x, const float* table, float* y, int64_t B, int64_t Cin, int64_t Cout, int64_t L,
                  int64_t orig, int64_t neu, encx_stream_t stream) {
    RsGeo g;
    RsPlan pl;
    ENCX_REQUIRE(rs_geo(orig, neu, g) && orig != neu);
    ENCX_REQUIRE(B >= 0 && L >= 0 && Cin >= 1 && Cout >= 1 && Cin <= 64 && Cout <= 64);
    ENCX_REQUIRE(Cout == Cin || Cout == 1 || (Cin == 1 && Cout == 2));
    ENCX_REQUIRE(rs_plan(g, pl));
    const int64_t Lout = encx_resample_out_len(L, orig, neu);
    ENCX_REQUIRE(Lout >= 0 && B * std::max(Cin, Cout) <= INT32_MAX);
    if (B == 0 || Lout == 0) return 0;
    ENCX_REQUIRE(x && table && y);
    RsArgs a;
    a.x = x; a.tab = table; a.y = y;
    a.L = L; a.Lout = Lout;
    if (Cout == Cin) {  // every channel a row of its own
        a.rows = (int)(B * Cin); a.cin = 1; a.cout = 1;
    } else {            // mean over Cin -> 1, or 1 -> 2 copies
        a.rows = (int)B; a.cin = (int)Cin; a.cout = (int)Cout;
    }
    a.o = (int)g.o; a.n = (int)g.n; a.width = (int)g.width; a.W = (int)g.W;
    a.tile = pl.tile; a.span = pl.span;
    a.fn = make_fastdiv((uint32_t)g.n);
    const int64_t tiles = cdiv(Lout, pl.tile);
    ENCX_REQUIRE(tiles <= INT32_MAX);
    const dim3 grid((unsigned)tiles, (unsigned)std::min(a.rows, 65535));
    const size_t lds = sizeof(float) * (size_t)(((pl.span + 3) & ~3) + (pl.tab_lds ? g.n * (g.W + 1) : 0));
    if (pl.tab_lds)
        hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
