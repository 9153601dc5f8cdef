// NormConv2d of the MS-STFT discriminator (modules/conv.py:125-139): what more than one of its
// three passes uses. The kernels and entry points are in conv2d_fwd.hip, conv2d_dgrad.hip and
// conv2d_wgrad.hip, three implicit GEMMs over v_mfma_f32_32x32x2_f32:
//     fwd    Y[co][(t,f)]  = sum_{(ci,kt),kf} W * X[ci][t+kt*dt-pt][f*sf+kf-pf]; the (t, f)
//            output positions of a batch item are flattened into one GEMM column space so
//            narrow late layers (F = 33..65) still fill 32-wide MFMA tiles; every tile stages
//            the input rows it touches (one window per (ci, kt) and output row) in LDS.
//            Bias + LeakyReLU(0.2) fused in the epilogue.
//     dgrad  polyphase along f (rows (ci, r), columns (t, u), reduction ((co, kt), q)), the
//            output-grad mask LeakyReLU'(y) applied while staging, the input's LeakyReLU'
//            applied in the epilogue; every dX element is written exactly once.
//     wgrad  dW[co][((ci,kt),kf)] + the bias as a ones column, split over (b, position chunk)
//            work items into slabs, summed in a fixed order (deterministic).
#pragma once
#include "common.h"

constexpr int NT = 256;
constexpr int DPER = 8;  // staging loads in flight per thread

/* NormConv2d geometry as used by DiscriminatorSTFT (msstftd.py:67-84): input [B][Ci][T2][Fi]
 * (time frames x freq bins), kernel (KT, KF), stride (1, sf), dilation (dt, 1), zero padding
 * (pt, pf) with T2 preserved; Fo = (Fi + 2 pf - KF)/sf + 1. */
struct C2Geo {
    int B, Ci, T2, Fi, Co, Fo, KT, KF, sf, dt, pt, pf;
};
static inline bool geo_ok(const C2Geo& g) {
    return g.B > 0 && g.Ci > 0 && g.T2 > 0 && g.Fi > 0 && g.Co > 0 && g.Fo > 0 && g.KT > 0 && g.KF > 0 &&
           g.sf > 0 && g.dt > 0 && g.pt >= 0 && g.pf >= 0 &&
           g.Fo == (g.Fi + 2 * g.pf - g.KF) / g.sf + 1 && g.T2 + 2 * g.pt - g.dt * (g.KT - 1) == g.T2;
}

// ---------------------------------------------------------------------------- planning
// window rows a column tile of BN flattened positions touches, rows of `len` positions
static inline int c2_rows(int BN, int len) { return (len + BN - 2) / len + 1; }

// channels per LDS chunk: even, <= VC rounded up to even, LDS <= budget floats
static inline int c2_ck(int VC, int per_ch, int budget = 12288) {
    int ck = budget / per_ch;
    if (ck > 32) ck = 32;
    int vce = (VC + 1) & ~1;
    if (ck > vce) ck = vce;
    ck &= ~1;
    if (ck < 2) ck = 2;
    // prefer an exact (even) divisor of VC near ck
    for (int c = ck; c >= 2; c -= 2)
        if (VC % c == 0 && c * 2 >= ck) return c;
    return ck;
}

// CK for the quad-staged kernels (c2_fwdr_kernel, c2_dgradr_kernel): the largest even combo
// count (<= CKM, <= VC rounded up to even) whose window of NR rows x RL columns fits MQ quads
// per thread; 0 when not even 2 combos fit
static inline int quad_ck(int VC, int NR, int RL, int MQ, int CKM) {
    const int quads = NR * (((RL + 3) & ~3) >> 2);
    int ck = MQ * NT / quads;
    ck = std::min(ck, CKM);
    ck = std::min(ck, (VC + 1) & ~1);
    ck &= ~1;
    return ck;
}

// Kernel family of a layer (conv2d_fwd.hip). g_c2_select: 0 the cost model, 1 the register-window
// kernels wherever they apply, 2 the tiled ones (encx_conv2d_select; ENCX_C2 sets the initial
// mode). rw_pays: whether the register-window form is the cheaper one under that mode.
extern int g_c2_select;
bool rw_pays(int64_t items, int64_t positions, double ratio);

// ---------------------------------------------------------------------- device helpers
// A quad meant to start at element offset o of a tensor whose last quad starts at `last` is
// loaded from min(max(o, 0), last) (never outside the tensor); quad_abs moves it into place:
// o[e] = v[e + sh], sh = o - clamped, zero where e + sh leaves the quad. Only the tensor's first
// and last quads are ever clamped, and there |sh| < 4 matters: the rest is padding, masked by
// the caller. Two select layers on the bits of |sh| (a select chain on sh == k compiles to
// branches).
ENCX_DEV f32x4 quad_abs(f32x4 v, int o, int last) {
    const int sh = o < 0 ? o : (o > last ? o - last : 0);
    const int n = sh < 0 ? -sh : sh;
    const bool b1 = n & 1, b2 = n & 2;
    f32x4 r;
    if (sh >= 0) {  // down: r[e] = v[e + n]
        const float t0 = b1 ? v[1] : v[0], t1 = b1 ? v[2] : v[1], t2 = b1 ? v[3] : v[2], t3 = b1 ? 0.f : v[3];
        r[0] = b2 ? t2 : t0;
        r[1] = b2 ? t3 : t1;
        r[2] = b2 ? 0.f : t2;
        r[3] = b2 ? 0.f : t3;
    } else {  // up: r[e] = v[e - n]
        const float t0 = b1 ? 0.f : v[0], t1 = b1 ? v[0] : v[1], t2 = b1 ? v[1] : v[2], t3 = b1 ? v[2] : v[3];
        r[0] = b2 ? 0.f : t0;
        r[1] = b2 ? 0.f : t1;
        r[2] = b2 ? t0 : t2;
        r[3] = b2 ? t1 : t3;
    }
    return r;
}

// Slot order of the persistent register-window loops (one NWV-wave workgroup per CU): item j of
// a round goes to wave j / gridDim.x of the j % gridDim.x-th workgroup in XCD order. A partial last
// round thus hands out one item per SIMD (waves w and w + 4 share one) before any SIMD takes a second
// -- the workgroup-major order piled it onto the first CUs, costing a whole extra round on layers
// with 1.5x or 2.9x as many items as wave slots -- and neighbouring items still share an XCD's L2.
ENCX_DEV int rw_first_slot(int wave) { return wave * (int)gridDim.x + xcd_linear_id(); }

// Staging quads in flight per thread of the register-window kernels' weight copy: every load of a
// thread is issued before its first LDS write (15 quads cover the 120 KB of the 3x9 layers at 512
// threads; the registers are free before the first item).
constexpr int RW_SQ = 15;

// Development tracing of the register-window forward / bwd-data kernels (build with
// -DENCX_C2_TRACE: `make trace`; tools/c2_trace.py reads it). Lane 0 of every wave stamps the
// steady clock (100 MHz) into the buffer given to encx_conv2d_trace, C2_TR_W int64 per wave
// (wave = block * NWV + wave in block): [0] kernel entry, [1] after the staging barrier, [2] items
// done, then per item [3 + 3 i ..] main-loop start, main-loop end, epilogue end.
constexpr int C2_TR_W = 32, C2_TR_ITEMS = (C2_TR_W - 3) / 3;
struct C2Trace {
    long long* buf;
    int waves;  // capacity of buf in waves
};
#ifdef ENCX_C2_TRACE
extern C2Trace g_c2_trace;
#define C2_TRACE_ARG C2Trace tr;
#define C2_TRACE_SET(s) (s).tr = g_c2_trace
#define C2_TRACE_VAL(tr, slot, k, v)                                                     \
    do {                                                                                 \
        if ((tr).buf && (threadIdx.x & 63) == 0 && (slot) < (tr).waves && (k) < C2_TR_W) \
            (tr).buf[(int64_t)(slot) * C2_TR_W + (k)] = (long long)(v);                  \
    } while (0)
#define C2_TRACE(tr, slot, k) C2_TRACE_VAL(tr, slot, k, wall_clock64())
#else
#define C2_TRACE_ARG
#define C2_TRACE_SET(s) \
    do {                \
    } while (0)
#define C2_TRACE_VAL(tr, slot, k, v) \
    do {                             \
    } while (0)
#define C2_TRACE(tr, slot, k) \
    do {                      \
    } while (0)
#endif
