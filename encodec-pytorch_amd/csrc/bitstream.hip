// encx -- `.ecdc` payload bit packing (binary.py:55-123) for whole encoded frames.
//
// The reference pushes the codes of a frame one at a time, t-major then codebook
// (compress.py:88-98): value v = t*K + k occupies bits [v*bits, (v+1)*bits) of a little-endian
// bit stream (BitPacker.push adds value << current_bits, binary.py:69-78), and flush() emits the
// final partial byte (binary.py:80-88), so a frame of n values is exactly ceil(n*bits/8) bytes.
// BitUnpacker.pull (binary.py:105-123) is the inverse. Both are pure byte/integer work and
// HBM-bound: no LDS, no MFMA.
// Several frames of equal (K, T) are handled by one launch at a fixed byte stride per frame.
// The slots of a streaming step deliver unequal frame counts: encx_bitpack_slots /
// encx_bitunpack_slots handle them in one launch too, each slot's count read from the device
// slot table, one packet (header byte + payload) per slot (encx.h: the packet format).
// encx_bitpack_slots_fec adds, in the same launch, a copy of the first codebooks of each slot's
// previous packet from a history it keeps on the device (encx.h: REDUNDANT PACKET).
#include "common.h"
#include "prof.h"

namespace {

// Eight consecutive codes are exactly `bits` whole bytes of the stream, so lane g owns codes
// 8g..8g+7 and bytes [g*bits, (g+1)*bits): no byte is shared between lanes, and (v -> t, k) is
// one division per lane, then a carried increment. The tail lane (n % 8 codes) emits the
// flush's partial byte. Reads: each of the K codebook rows is walked contiguously across the
// wave (t advances with the lane); writes: the wave covers 64*bits contiguous bytes.
__global__ void bitpack_kernel(const int64_t* __restrict__ codes, int64_t s_item, int64_t s_k,
                               int64_t s_t, int K, int64_t n, int bits, uint8_t* __restrict__ out,
                               int64_t groups, int64_t out_stride, int64_t total,
                               int* __restrict__ err) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const int64_t b = j / groups;
    const int64_t g = j - b * groups;
    const int64_t v0 = g * 8;
    const int cnt = (int)((n - v0) < 8 ? (n - v0) : 8);
    int64_t t = v0 / K;
    int k = (int)(v0 - t * K);
    const int64_t* src = codes + b * s_item;
    uint8_t* dst = out + b * out_stride + g * bits;
    uint64_t acc = 0;
    int nb = 0;
    uint64_t bad = 0;
    for (int i = 0; i < cnt; ++i) {
        const uint64_t val = (uint64_t)src[k * s_k + t * s_t];
        // the reference adds without masking; a code >= 2^bits would corrupt its neighbours
        bad |= val >> bits;
        acc |= val << nb;
        nb += bits;
        while (nb >= 8) {
            *dst++ = (uint8_t)(acc & 0xff);
            acc >>= 8;
            nb -= 8;
        }
        if (++k == K) { k = 0; ++t; }
    }
    if (nb) *dst = (uint8_t)(acc & 0xff);  // flush (binary.py:80-85); only the tail lane
    if (bad) atomicOr(err, 1);
}

// The inverse: lane g reads its `bits` bytes (fewer on the tail) and emits codes 8g..8g+7.
__global__ void bitunpack_kernel(const uint8_t* __restrict__ in, int64_t in_stride, int K, int64_t n,
                                 int bits, int64_t* __restrict__ codes, int64_t s_item, int64_t s_k,
                                 int64_t s_t, int64_t groups, int64_t total) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const int64_t b = j / groups;
    const int64_t g = j - b * groups;
    const int64_t v0 = g * 8;
    const int cnt = (int)((n - v0) < 8 ? (n - v0) : 8);
    int64_t t = v0 / K;
    int k = (int)(v0 - t * K);
    const uint8_t* src = in + b * in_stride + g * bits;
    int64_t* dst = codes + b * s_item;
    const uint64_t mask = (1ull << bits) - 1;
    uint64_t acc = 0;
    int nb = 0;
    for (int i = 0; i < cnt; ++i) {
        while (nb < bits) {
            acc |= (uint64_t)(*src++) << nb;
            nb += 8;
        }
        dst[k * s_k + t * s_t] = (int64_t)(acc & mask);
        acc >>= bits;
        nb -= bits;
        if (++k == K) { k = 0; ++t; }
    }
}

// ---- one packet per slot of a streaming step (encx.h: the slot table and the packet format)
// The frames a slot delivers, from the slot table: clamped to 0..n_max, so whatever the table
// holds no column past the call's n_max (and none past the slot's own count) is addressed.
ENCX_DEV int slot_frames(const int32_t* slots, int b, int n_max) {
    const int f = slots[2 * b];
    return f < 0 ? 0 : (f > n_max ? n_max : f);
}

// bitpack_kernel's lane layout over a slot's own sequence of n values (t-major, K codebooks):
// the lane owns codes v0..v0+cnt-1 (v0 = 8g) and the payload bytes from dst = payload + g*bits.
// -> the OR of the bits that do not fit. Shared by the fixed-K and the per-slot-K packers.
ENCX_DEV uint64_t pack_group(const int64_t* __restrict__ src, int64_t s_k, int64_t s_t, int K, int v0, int cnt,
                             int bits, uint8_t* __restrict__ dst) {
    int t = v0 / K, k = v0 - t * K;
    uint64_t acc = 0, bad = 0;
    int nb = 0;
    for (int i = 0; i < cnt; ++i) {
        const uint64_t val = (uint64_t)src[k * s_k + t * s_t];
        bad |= val >> bits;
        acc |= val << nb;
        nb += bits;
        while (nb >= 8) {
            *dst++ = (uint8_t)(acc & 0xff);
            acc >>= 8;
            nb -= 8;
        }
        if (++k == K) { k = 0; ++t; }
    }
    if (nb) *dst = (uint8_t)(acc & 0xff);
    return bad;
}

// The inverse: positions v0..v0+cnt-1 of a (t-major, K) grid; those below n are read from the
// lane's bytes at src, the others are written as 0.
ENCX_DEV void unpack_group(const uint8_t* __restrict__ src, int64_t* __restrict__ dst, int64_t s_k, int64_t s_t,
                           int K, int v0, int cnt, int n, int bits) {
    int t = v0 / K, k = v0 - t * K;
    const uint64_t mask = (1ull << bits) - 1;
    uint64_t acc = 0;
    int nb = 0;
    for (int i = 0; i < cnt; ++i) {
        int64_t val = 0;
        if (v0 + i < n) {
            while (nb < bits) {
                acc |= (uint64_t)(*src++) << nb;
                nb += 8;
            }
            val = (int64_t)(acc & mask);
            acc >>= bits;
            nb -= bits;
        }
        dst[k * s_k + t * s_t] = val;
        if (++k == K) { k = 0; ++t; }
    }
}

// A slot's codebook count from the nq table of a per-slot-bandwidth step, clamped to 0..K.
ENCX_DEV int slot_nq(const int32_t* nq, int b, int K) {
    const int q = nq[b];
    return q < 0 ? 0 : (q > K ? K : q);
}

// One packet per slot: lane g of slot b owns codes 8g..8g+7 of the slot's t-major sequence of
// n = frames * K values and the payload bytes [g*bits, (g+1)*bits) behind the header. Lanes past
// the slot's count leave without forming an address, so the unread tail of a row (columns >=
// frames) may hold anything. Lane 0 writes the header and the packet length (0 for a slot that
// sits out: no header either). NQ: K is the slot's own nq[b] (rows >= nq[b] are not read) and
// the header is two bytes, (frames, K); a slot whose table says nq 0 delivers nothing.
template <bool NQ>
__global__ void bitpack_slots_kernel(const int64_t* __restrict__ codes, int64_t s_b, int64_t s_k, int64_t s_t, int B,
                                     int K, int n_max, int bits, const int32_t* __restrict__ slots,
                                     const int32_t* __restrict__ nq, uint8_t* __restrict__ out, int64_t out_stride,
                                     int64_t* __restrict__ nbytes, int groups, int* __restrict__ err) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B * groups) return;
    const int b = j / groups, g = j - b * groups;
    const int Kb = NQ ? slot_nq(nq, b, K) : K;
    const int frames = Kb ? slot_frames(slots, b, n_max) : 0;
    const int n = frames * Kb, hdr = NQ ? 2 : 1;
    if (g == 0) {
        nbytes[b] = frames ? hdr + ((int64_t)n * bits + 7) / 8 : 0;
        if (frames) out[b * out_stride] = (uint8_t)frames;
        if (NQ && frames) out[b * out_stride + 1] = (uint8_t)Kb;
    }
    const int v0 = g * 8;
    if (v0 >= n) return;
    const uint64_t bad = pack_group(codes + b * s_b, s_k, s_t, Kb, v0, n - v0 < 8 ? n - v0 : 8, bits,
                                    out + b * out_stride + hdr + (int64_t)g * bits);
    if (bad) atomicOr(err, 1);
}

// A slot's row of the fec table (encx.h: fec[B][4]), clamped: the copy's frames 0..h_max and
// codebooks 0..R, both 0 when either is, and the copy of the history that holds the slot's
// previous packet (this launch writes the other one).
struct fec_row {
    int n_r, K_r, par;
};
ENCX_DEV fec_row slot_fec(const int32_t* fec, int b, int h_max, int R) {
    int n = fec[4 * b], q = fec[4 * b + 1];
    n = n < 0 ? 0 : (n > h_max ? h_max : n);
    q = q < 0 ? 0 : (q > R ? R : q);
    if (!n || !q) n = q = 0;
    return {n, q, fec[4 * b + 2] & 1};
}

// One redundant packet per slot (encx.h: REDUNDANT PACKET). Slot b has gm lanes for its main
// section, which pack as bitpack_slots_kernel<true> behind a four-byte header, and gr lanes for
// the copy of its previous packet: lane g of those packs codes 8g..8g+7 of the K_r x n_r grid
// kept in hist[par] at the first byte after the main section. A main lane also keeps what it
// packed: the codes of rows k < min(R, K_b) go to hist[par ^ 1]. The two copies are disjoint,
// so no lane reads a cell this launch writes; the host flips par only when the slot delivered
// and no code was refused. A slot that sits out writes nothing, neither packet nor history.
__global__ void bitpack_slots_fec_kernel(const int64_t* __restrict__ codes, int64_t s_b, int64_t s_k, int64_t s_t,
                                         int B, int K, int n_max, int bits, int R, int h_max,
                                         const int32_t* __restrict__ slots, const int32_t* __restrict__ nq,
                                         const int32_t* __restrict__ fec, int64_t* hist,
                                         uint8_t* __restrict__ out, int64_t out_stride,
                                         int64_t* __restrict__ nbytes, int gm, int gr, int* __restrict__ err) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B * (gm + gr)) return;
    const int b = j / (gm + gr), g = j - b * (gm + gr);
    const int Kb = slot_nq(nq, b, K);
    const int frames = Kb ? slot_frames(slots, b, n_max) : 0;
    if (!frames) {
        if (g == 0) nbytes[b] = 0;
        return;
    }
    const fec_row f = slot_fec(fec, b, h_max, R);
    const int n = frames * Kb, nr = f.n_r * f.K_r;
    const int64_t main_bytes = ((int64_t)n * bits + 7) / 8;
    uint8_t* pkt = out + b * out_stride;
    const int64_t plane = (int64_t)B * R * h_max;  // one copy of the history, [B][R][h_max]
    const int64_t row0 = (int64_t)b * R * h_max;
    uint64_t bad = 0;
    if (g < gm) {
        if (g == 0) {
            nbytes[b] = 4 + main_bytes + ((int64_t)nr * bits + 7) / 8;
            pkt[0] = (uint8_t)frames;
            pkt[1] = (uint8_t)Kb;
            pkt[2] = (uint8_t)f.n_r;
            pkt[3] = (uint8_t)f.K_r;
        }
        const int v0 = g * 8;
        if (v0 >= n) return;
        const int cnt = n - v0 < 8 ? n - v0 : 8;
        const int64_t* src = codes + b * s_b;
        bad = pack_group(src, s_k, s_t, Kb, v0, cnt, bits, pkt + 4 + (int64_t)g * bits);
        int64_t* keep = hist + (f.par ^ 1) * plane + row0;
        int t = v0 / Kb, k = v0 - t * Kb;
        for (int i = 0; i < cnt; ++i) {
            if (k < R) keep[(int64_t)k * h_max + t] = src[k * s_k + t * s_t];
            if (++k == Kb) { k = 0; ++t; }
        }
    } else {
        const int v0 = (g - gm) * 8;
        if (v0 >= nr) return;
        bad = pack_group(hist + f.par * plane + row0, h_max, 1, f.K_r, v0, nr - v0 < 8 ? nr - v0 : 8, bits,
                         pkt + 4 + main_bytes + (int64_t)(g - gm) * bits);
    }
    if (bad) atomicOr(err, 1);
}

// The inverse over all n_max * K code positions of every slot: lane g reads its bytes of the
// payload only where the slot delivers the code, and writes 0 past the slot's count.
__global__ void bitunpack_slots_kernel(const uint8_t* __restrict__ in, int64_t in_stride, int B, int K, int n_max,
                                       int bits, const int32_t* __restrict__ slots, int64_t* __restrict__ codes,
                                       int64_t s_b, int64_t s_k, int64_t s_t, int groups) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B * groups) return;
    const int b = j / groups, g = j - b * groups;
    const int n = slot_frames(slots, b, n_max) * K, total = n_max * K;
    const int v0 = g * 8;
    unpack_group(in + b * in_stride + (int64_t)g * bits, codes + b * s_b, s_k, s_t, K, v0,
                 total - v0 < 8 ? total - v0 : 8, n, bits);
}

// With K per slot: lane g unpacks codes 8g..8g+7 of the slot's own sequence (frames * nq[b]
// values) into rows < nq[b], then writes the zeros of its share of the [K][n_max] grid: rows >=
// nq[b] and columns >= frames. The two sets of positions are disjoint.
__global__ void bitunpack_slots_nq_kernel(const uint8_t* __restrict__ in, int64_t in_stride, int B, int K, int n_max,
                                          int bits, const int32_t* __restrict__ slots,
                                          const int32_t* __restrict__ nq, int64_t* __restrict__ codes, int64_t s_b,
                                          int64_t s_k, int64_t s_t, int groups) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B * groups) return;
    const int b = j / groups, g = j - b * groups;
    const int Kb = slot_nq(nq, b, K);
    const int frames = Kb ? slot_frames(slots, b, n_max) : 0;
    const int n = frames * Kb, total = n_max * K;
    const int v0 = g * 8;
    int64_t* dst = codes + b * s_b;
    if (v0 < n)
        unpack_group(in + b * in_stride + (int64_t)g * bits, dst, s_k, s_t, Kb, v0, n - v0 < 8 ? n - v0 : 8, n, bits);
    for (int v = v0; v < total && v < v0 + 8; ++v) {
        const int t = v / K, k = v - t * K;
        if (t >= frames || k >= Kb) dst[k * s_k + t * s_t] = 0;
    }
}

}  // namespace

extern "C" {

int encx_bitpack_slots(const int64_t* codes, int64_t s_b, int64_t s_k, int64_t s_t, int64_t B, int64_t K,
                       int64_t n_max, int bits, const int32_t* slots, uint8_t* out, int64_t out_stride,
                       int64_t* nbytes, int* err, encx_stream_t stream) {
    ENCX_REQUIRE(codes && slots && out && nbytes && err);
    ENCX_REQUIRE(B >= 1 && B <= 64 && K >= 1 && K <= 64 && n_max >= 1 && n_max <= 255 && bits >= 1 && bits <= 32);
    ENCX_REQUIRE(out_stride >= 1 + encx_bitpack_bytes(n_max * K, bits));
    const int groups = (int)cdiv(n_max * K, 8);
    hipLaunchKernelGGL(bitpack_slots_kernel<false>, dim3((unsigned)cdiv(B * groups, 256)), dim3(256), 0,
                       (hipStream_t)stream, codes, s_b, s_k, s_t, (int)B, (int)K, (int)n_max, bits, slots,
                       (const int32_t*)nullptr, out, out_stride, nbytes, groups, err);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_bitunpack_slots(const uint8_t* in, int64_t in_stride, int64_t B, int64_t K, int64_t n_max, int bits,
                         const int32_t* slots, int64_t* codes, int64_t s_b, int64_t s_k, int64_t s_t,
                         encx_stream_t stream) {
    ENCX_REQUIRE(in && slots && codes);
    ENCX_REQUIRE(B >= 1 && B <= 64 && K >= 1 && K <= 64 && n_max >= 1 && n_max <= 255 && bits >= 1 && bits <= 32);
    ENCX_REQUIRE(in_stride >= encx_bitpack_bytes(n_max * K, bits));
    const int groups = (int)cdiv(n_max * K, 8);
    hipLaunchKernelGGL(bitunpack_slots_kernel, dim3((unsigned)cdiv(B * groups, 256)), dim3(256), 0,
                       (hipStream_t)stream, in, in_stride, (int)B, (int)K, (int)n_max, bits, slots, codes, s_b, s_k,
                       s_t, groups);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_bitpack_slots_nq(const int64_t* codes, int64_t s_b, int64_t s_k, int64_t s_t, int64_t B, int64_t K,
                          int64_t n_max, int bits, const int32_t* slots, const int32_t* nq, uint8_t* out,
                          int64_t out_stride, int64_t* nbytes, int* err, encx_stream_t stream) {
    ENCX_REQUIRE(codes && slots && nq && out && nbytes && err);
    ENCX_REQUIRE(B >= 1 && B <= 64 && K >= 1 && K <= 64 && n_max >= 1 && n_max <= 255 && bits >= 1 && bits <= 32);
    ENCX_REQUIRE(out_stride >= 2 + encx_bitpack_bytes(n_max * K, bits));
    encx_prof_scope ps((hipStream_t)stream, 0.0, 9.0 * B * K * n_max, "bitpack_slots_nq", false);
    const int groups = (int)cdiv(n_max * K, 8);
    hipLaunchKernelGGL(bitpack_slots_kernel<true>, dim3((unsigned)cdiv(B * groups, 256)), dim3(256), 0,
                       (hipStream_t)stream, codes, s_b, s_k, s_t, (int)B, (int)K, (int)n_max, bits, slots, nq, out,
                       out_stride, nbytes, groups, err);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_bitpack_slots_fec(const int64_t* codes, int64_t s_b, int64_t s_k, int64_t s_t, int64_t B, int64_t K,
                           int64_t n_max, int bits, int64_t R, int64_t h_max, const int32_t* slots, const int32_t* nq,
                           const int32_t* fec, int64_t* hist, uint8_t* out, int64_t out_stride, int64_t* nbytes,
                           int* err, encx_stream_t stream) {
    ENCX_REQUIRE(codes && slots && nq && fec && hist && out && nbytes && err);
    ENCX_REQUIRE(B >= 1 && B <= 64 && K >= 1 && K <= 64 && n_max >= 1 && n_max <= 255 && bits >= 1 && bits <= 32);
    ENCX_REQUIRE(R >= 1 && R <= K && h_max >= n_max && h_max <= 255);
    ENCX_REQUIRE(out_stride >= 4 + encx_bitpack_bytes(n_max * K, bits) + encx_bitpack_bytes(h_max * R, bits));
    encx_prof_scope ps((hipStream_t)stream, 0.0, 9.0 * B * (K * n_max + 2 * R * h_max), "bitpack_slots_fec", false);
    const int gm = (int)cdiv(n_max * K, 8), gr = (int)cdiv(h_max * R, 8);
    hipLaunchKernelGGL(bitpack_slots_fec_kernel, dim3((unsigned)cdiv(B * (gm + gr), 256)), dim3(256), 0,
                       (hipStream_t)stream, codes, s_b, s_k, s_t, (int)B, (int)K, (int)n_max, bits, (int)R,
                       (int)h_max, slots, nq, fec, hist, out, out_stride, nbytes, gm, gr, err);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_bitunpack_slots_nq(const uint8_t* in, int64_t in_stride, int64_t B, int64_t K, int64_t n_max, int bits,
                            const int32_t* slots, const int32_t* nq, int64_t* codes, int64_t s_b, int64_t s_k,
                            int64_t s_t, encx_stream_t stream) {
    ENCX_REQUIRE(in && slots && nq && codes);
    ENCX_REQUIRE(B >= 1 && B <= 64 && K >= 1 && K <= 64 && n_max >= 1 && n_max <= 255 && bits >= 1 && bits <= 32);
    ENCX_REQUIRE(in_stride >= encx_bitpack_bytes(n_max * K, bits));
    encx_prof_scope ps((hipStream_t)stream, 0.0, 9.0 * B * K * n_max, "bitunpack_slots_nq", false);
    const int groups = (int)cdiv(n_max * K, 8);
    hipLaunchKernelGGL(bitunpack_slots_nq_kernel, dim3((unsigned)cdiv(B * groups, 256)), dim3(256), 0,
                       (hipStream_t)stream, in, in_stride, (int)B, (int)K, (int)n_max, bits, slots, nq, codes, s_b,
                       s_k, s_t, groups);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int64_t encx_bitpack_bytes(int64_t n_values, int bits) {
    if (n_values < 0 || bits < 1 || bits > 32) return -1;
    return (n_values * bits + 7) / 8;
}

int encx_bitpack(const int64_t* codes, int64_t s_item, int64_t s_k, int64_t s_t, int64_t items,
                 int64_t K, int64_t T, int bits, uint8_t* out, int64_t out_stride, int* err,
                 encx_stream_t stream) {
    ENCX_REQUIRE(bits >= 1 && bits <= 32 && items >= 0 && K >= 0 && T >= 0);
    const int64_t n = K * T;
    const int64_t nbytes = encx_bitpack_bytes(n, bits);
    ENCX_REQUIRE(out_stride >= nbytes);
    const int64_t groups = cdiv(n, 8);
    const int64_t total = items * groups;
    if (total == 0) return 0;  // BitPacker.flush with nothing pushed writes nothing
    ENCX_REQUIRE(codes && out && err && K <= INT32_MAX);
    hipLaunchKernelGGL(bitpack_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, codes, s_item, s_k, s_t, (int)K, n, bits, out, groups,
                       out_stride, total, err);
    ENCX_CHECK_LAUNCH();
    return 0;
}

int encx_bitunpack(const uint8_t* in, int64_t in_stride, int64_t items, int64_t K, int64_t T,
                   int bits, int64_t* codes, int64_t s_item, int64_t s_k, int64_t s_t,
                   encx_stream_t stream) {
    ENCX_REQUIRE(bits >= 1 && bits <= 32 && items >= 0 && K >= 0 && T >= 0);
    const int64_t n = K * T;
    ENCX_REQUIRE(in_stride >= encx_bitpack_bytes(n, bits));
    const int64_t groups = cdiv(n, 8);
    const int64_t total = items * groups;
    if (total == 0) return 0;
    ENCX_REQUIRE(in && codes && K <= INT32_MAX);
    hipLaunchKernelGGL(bitunpack_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0,
                       (hipStream_t)stream, in, in_stride, (int)K, n, bits, codes, s_item, s_k, s_t,
                       groups, total);
    ENCX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
