// Host-side argument validation of the per-slot bandwidth entry points (include/encx.h), as a
// stand-alone program for a sanitizer build: `make -C encodec-pytorch_amd san-stream-nq` compiles
// the host code of csrc/stream_rvq.hip, csrc/bitstream.hip and csrc/api.hip with
// -fsanitize=address,undefined, links this main() and runs it on the CPU. Every call below must
// return ENCX_EINVAL before any launch: the non-NULL pointers are host arrays that a kernel could
// not even read, so a launch would be an error too. No device is needed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/encx.h"

static int failures = 0;
#define EXPECT_EINVAL(call)                                                 \
    do {                                                                    \
        const int rc_ = (call);                                             \
        if (rc_ != ENCX_EINVAL) {                                           \
            std::printf("line %d: %s -> %d\n", __LINE__, #call, rc_);       \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

int main() {
    std::vector<float> f(16, 0.f);
    std::vector<int64_t> c(16, 0);
    std::vector<int32_t> t(16, 0);
    std::vector<uint8_t> by(16, 0);
    int err = 0;
    float* F = f.data();
    int64_t* C = c.data();
    int32_t* S = t.data();
    uint8_t* Y = by.data();
    const float* N = nullptr;

    // encx_stream_rvq_prepare(embed, k, K_max, bins, D, packed, packed_t, ee, stream)
    EXPECT_EINVAL(encx_stream_rvq_prepare(N, 0, 8, 1024, 128, F, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 8, 1024, 128, nullptr, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 8, 1024, 128, F, nullptr, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 8, 1024, 128, F, F, nullptr, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, -1, 8, 1024, 128, F, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 8, 8, 1024, 128, F, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 0, 1024, 128, F, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 65, 1024, 128, F, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 8, 1023, 128, F, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 8, INT64_MAX, 128, F, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 8, 1024, 4, F, F, F, nullptr));
    EXPECT_EINVAL(encx_stream_rvq_prepare(F, 0, 8, 1024, 264, F, F, F, nullptr));

    // encx_stream_rvq_encode_slots(x, x_b, x_d, x_t, packed, packed_t, ee, B, K_max, bins, D, n_max,
    //                              slots, nq, codes, c_b, c_k, c_t, stream)
#define ENC(x, E, ET, ee, B, K, bins, D, n, sl, nq, co) \
    encx_stream_rvq_encode_slots(x, 1024, 8, 1, E, ET, ee, B, K, bins, D, n, sl, nq, co, 56, 7, 1, nullptr)
    EXPECT_EINVAL(ENC(N, F, F, F, 2, 8, 1024, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, N, F, F, 2, 8, 1024, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, N, F, 2, 8, 1024, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, N, 2, 8, 1024, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 1024, 128, 7, nullptr, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 1024, 128, 7, S, nullptr, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 1024, 128, 7, S, S, nullptr));
    EXPECT_EINVAL(ENC(F, F, F, F, 0, 8, 1024, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 65, 8, 1024, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 0, 1024, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 65, 1024, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 0, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 1026, 128, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 1024, 0, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 1024, 132, 7, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 1024, 128, 0, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, 2, 8, 1024, 128, 256, S, S, C));
    EXPECT_EINVAL(ENC(F, F, F, F, INT64_MIN, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX, S, S, C));

    // encx_stream_rvq_decode_slots(codes, c_b, c_k, c_t, packed, B, K_max, bins, D, n_max, slots, nq,
    //                              out, o_b, o_d, o_t, stream)
#define DEC(co, E, B, K, bins, D, n, sl, nq, out) \
    encx_stream_rvq_decode_slots(co, 56, 7, 1, E, B, K, bins, D, n, sl, nq, out, 1024, 8, 1, nullptr)
    EXPECT_EINVAL(DEC(nullptr, F, 2, 8, 1024, 128, 7, S, S, F));
    EXPECT_EINVAL(DEC(C, N, 2, 8, 1024, 128, 7, S, S, F));
    EXPECT_EINVAL(DEC(C, F, 2, 8, 1024, 128, 7, nullptr, S, F));
    EXPECT_EINVAL(DEC(C, F, 2, 8, 1024, 128, 7, S, nullptr, F));
    EXPECT_EINVAL(DEC(C, F, 2, 8, 1024, 128, 7, S, S, nullptr));
    EXPECT_EINVAL(DEC(C, F, 0, 8, 1024, 128, 7, S, S, F));
    EXPECT_EINVAL(DEC(C, F, 65, 8, 1024, 128, 7, S, S, F));
    EXPECT_EINVAL(DEC(C, F, 2, 0, 1024, 128, 7, S, S, F));
    EXPECT_EINVAL(DEC(C, F, 2, 65, 1024, 128, 7, S, S, F));
    EXPECT_EINVAL(DEC(C, F, 2, 8, 2, 128, 7, S, S, F));
    EXPECT_EINVAL(DEC(C, F, 2, 8, 1024, 257, 7, S, S, F));
    EXPECT_EINVAL(DEC(C, F, 2, 8, 1024, 128, -1, S, S, F));
    EXPECT_EINVAL(DEC(C, F, 2, 8, 1024, 128, 256, S, S, F));

    // encx_bitpack_slots_nq(codes, s_b, s_k, s_t, B, K, n_max, bits, slots, nq, out, out_stride, nbytes, err, stream)
#define PACK(co, B, K, n, bits, sl, nq, out, stride, nb, e) \
    encx_bitpack_slots_nq(co, 56, 7, 1, B, K, n, bits, sl, nq, out, stride, nb, e, nullptr)
    EXPECT_EINVAL(PACK(nullptr, 2, 8, 7, 10, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 10, nullptr, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 10, S, nullptr, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 10, S, S, nullptr, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 10, S, S, Y, 72, nullptr, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 10, S, S, Y, 72, C, nullptr));
    EXPECT_EINVAL(PACK(C, 0, 8, 7, 10, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 65, 8, 7, 10, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 0, 7, 10, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 65, 7, 10, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 0, 10, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 256, 10, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 0, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 33, S, S, Y, 72, C, &err));
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 10, S, S, Y, 71, C, &err));  // 2 header bytes + 70
    EXPECT_EINVAL(PACK(C, 2, 8, 7, 10, S, S, Y, -1, C, &err));

    // encx_bitunpack_slots_nq(in, in_stride, B, K, n_max, bits, slots, nq, codes, s_b, s_k, s_t, stream)
#define UNPACK(in, stride, B, K, n, bits, sl, nq, co) \
    encx_bitunpack_slots_nq(in, stride, B, K, n, bits, sl, nq, co, 56, 7, 1, nullptr)
    EXPECT_EINVAL(UNPACK(nullptr, 70, 2, 8, 7, 10, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 8, 7, 10, nullptr, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 8, 7, 10, S, nullptr, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 8, 7, 10, S, S, nullptr));
    EXPECT_EINVAL(UNPACK(Y, 70, 0, 8, 7, 10, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 65, 8, 7, 10, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 0, 7, 10, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 65, 7, 10, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 8, 0, 10, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 8, 256, 10, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 8, 7, 0, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 70, 2, 8, 7, 33, S, S, C));
    EXPECT_EINVAL(UNPACK(Y, 69, 2, 8, 7, 10, S, S, C));

    if (failures) {
        std::printf("%d call(s) were not refused\n", failures);
        return 1;
    }
    std::printf("stream_nq_args: every bad call refused before any launch\n");
    return 0;
}
