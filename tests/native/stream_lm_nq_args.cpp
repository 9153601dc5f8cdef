// Host-side argument validation of the entry points behind LM-coded packets with a codebook count
// per slot (packet format 2, include/encx.h), as a stand-alone program for a sanitizer build:
// `make -C encodec-pytorch_amd san-stream-lm-nq` compiles the host code of csrc/lm.hip, csrc/ac.hip
// and csrc/api.hip with -fsanitize=address,undefined, links this main() and runs it on the CPU.
// Every call below must return ENCX_EINVAL before any launch: the non-NULL pointers are host
// arrays that a kernel could not even read, so a launch would be an error too. No device is needed.
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
    const float* NF = nullptr;
    const int32_t* NS = nullptr;
    int64_t* NC = nullptr;

    // encx_lm_input_slots_nq(codes, s_b, s_k, s_t, B, K, T, n_max, slots, nq, pos, prev, dev_step, emb, card1, D,
    //                        ln_w, ln_b, max_period, x, stream)
#define INP(B, K, T, n, sl, nq, pos, prev, emb, card1, D, lw, lb, x) \
    encx_lm_input_slots_nq(C, 64, 8, 1, B, K, T, n, sl, nq, pos, prev, nullptr, emb, card1, D, lw, lb, 10000.f, x, nullptr)
    EXPECT_EINVAL(INP(3, 8, 8, 8, NS, S, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, NS, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, NC, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, C, NC, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, C, C, NF, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, C, C, F, 65, 64, NF, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, C, C, F, 65, 64, F, NF, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, C, C, F, 65, 64, F, F, nullptr));
    EXPECT_EINVAL(INP(0, 8, 8, 8, S, S, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(65, 8, 8, 8, S, S, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 0, 8, 8, S, S, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 65, 8, 8, S, S, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 0, 8, S, S, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 9, 8, S, S, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 256, S, S, C, C, F, 65, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, C, C, F, 0, 64, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, C, C, F, 65, 3, F, F, F));
    EXPECT_EINVAL(INP(3, 8, 8, 8, S, S, C, C, F, 65, 514, F, F, F));
    EXPECT_EINVAL(INP(INT64_MIN, INT64_MAX, INT64_MAX, INT64_MAX, S, S, C, C, F, INT64_MAX, INT64_MAX, F, F, F));

    // encx_lm_slots_advance_nq(slots, nq, B, K, n_max, pos, prev, codes, s_b, s_k, s_t, card1, stream)
#define ADV(sl, nq, B, K, n, pos, prev, card1) \
    encx_lm_slots_advance_nq(sl, nq, B, K, n, pos, prev, nullptr, 0, 0, 0, card1, nullptr)
    EXPECT_EINVAL(ADV(NS, S, 3, 8, 8, C, C, 65));
    EXPECT_EINVAL(ADV(S, NS, 3, 8, 8, C, C, 65));
    EXPECT_EINVAL(ADV(S, S, 3, 8, 8, NC, C, 65));
    EXPECT_EINVAL(ADV(S, S, 3, 8, 8, C, NC, 65));
    EXPECT_EINVAL(ADV(S, S, 0, 8, 8, C, C, 65));
    EXPECT_EINVAL(ADV(S, S, 65, 8, 8, C, C, 65));
    EXPECT_EINVAL(ADV(S, S, 3, 0, 8, C, C, 65));
    EXPECT_EINVAL(ADV(S, S, 3, 65, 8, C, C, 65));
    EXPECT_EINVAL(ADV(S, S, 3, 8, 0, C, C, 65));
    EXPECT_EINVAL(ADV(S, S, 3, 8, 256, C, C, 65));
    EXPECT_EINVAL(ADV(S, S, 3, 8, 8, C, C, 0));

    // encx_lm_heads_slots(x, B, T, n_max, D, w, bias, K, card, slots, nq, dev_step, work, probas, cdf, bits,
    //                     roundoff, min_range, sym, s_b, s_k, s_t, lohi, err, stream)
#define HEADS(x, B, T, n, D, w, bias, K, card, sl, nq, work, probas, cdf, bits, minr, sym, lohi) \
    encx_lm_heads_slots(x, B, T, n, D, w, bias, K, card, sl, nq, nullptr, work, probas, cdf, bits, 1e-8f, minr, sym, \
                        64, 8, 1, lohi, &err, nullptr)
    EXPECT_EINVAL(HEADS(NF, 3, 8, 8, 64, F, F, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, NF, F, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, NF, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, NS, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, S, NS, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, S, S, nullptr, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, S, S, F, nullptr, nullptr, 24, 2, nullptr, nullptr));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, S, S, F, F, nullptr, 24, 2, C, S));   // sym needs cdf
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, S, S, F, F, S, 24, 2, C, nullptr));   // and lohi
    EXPECT_EINVAL(HEADS(F, 0, 8, 8, 64, F, F, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 65, 8, 8, 64, F, F, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 0, 8, 64, F, F, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 9, 8, 64, F, F, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 256, 64, F, F, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 0, F, F, 8, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 0, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 65, 64, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 0, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 65537, S, S, F, F, S, 24, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, S, S, F, F, S, 0, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, S, S, F, F, S, 31, 2, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 64, S, S, F, F, S, 24, 1, C, S));
    EXPECT_EINVAL(HEADS(F, 3, 8, 8, 64, F, F, 8, 1024, S, S, F, F, S, 10, 2, C, S));       // alpha > 1
    EXPECT_EINVAL(HEADS(F, 64, 255, 255, 64, F, F, 64, 65536, S, S, F, F, S, 24, 2, C, S)); // B T K card past int32

    // encx_ac_encode_slots_nq(lohi, B, n_max, K, slots, nq, bits, out, out_stride, nbytes, err, stream)
#define ENC(lh, B, n, K, sl, nq, bits, out, stride, nb, e) \
    encx_ac_encode_slots_nq(lh, B, n, K, sl, nq, bits, out, stride, nb, e, nullptr)
    EXPECT_EINVAL(ENC(NS, 3, 8, 8, S, S, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 8, NS, S, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 8, S, NS, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 8, S, S, 24, nullptr, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 8, S, S, 24, Y, 210, NC, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 8, S, S, 24, Y, 210, C, nullptr));
    EXPECT_EINVAL(ENC(S, 0, 8, 8, S, S, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 65, 8, 8, S, S, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 0, 8, S, S, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 256, 8, S, S, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 0, S, S, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 65, S, S, 24, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 8, S, S, 0, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 8, S, S, 31, Y, 210, C, &err));
    EXPECT_EINVAL(ENC(S, 3, 8, 8, S, S, 24, Y, 1, C, &err));   // no room for the two header bytes
    EXPECT_EINVAL(ENC(S, 3, 8, 8, S, S, 24, Y, -1, C, &err));

    // encx_ac_decode_slots_nq(data, stride, nbytes, B, state, cdf, K, card, bits, codes, c_s, c_k, c_t, n_max,
    //                         dev_step, slots, nq, prev, err, stream)
#define DEC(data, stride, nb, B, st, cdf, K, card, bits, co, n, step, sl, nq, prev, e) \
    encx_ac_decode_slots_nq(data, stride, nb, B, st, cdf, K, card, bits, co, 64, 8, 1, n, step, sl, nq, prev, e, nullptr)
    EXPECT_EINVAL(DEC(nullptr, 208, C, 3, C, S, 8, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, NC, 3, C, S, 8, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, NC, S, 8, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, NS, 8, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 24, NC, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 24, C, 8, NC, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 24, C, 8, C, NS, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 24, C, 8, C, S, NS, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 24, C, 8, C, S, S, NC, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 24, C, 8, C, S, S, C, nullptr));
    EXPECT_EINVAL(DEC(Y, 0, C, 3, C, S, 8, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 0, C, S, 8, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 65, C, S, 8, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 0, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 65, 1024, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 0, 24, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 0, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 31, C, 8, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 24, C, 0, C, S, S, C, &err));
    EXPECT_EINVAL(DEC(Y, 208, C, 3, C, S, 8, 1024, 24, C, 256, C, S, S, C, &err));

    if (failures) {
        std::printf("%d call(s) were not refused\n", failures);
        return 1;
    }
    std::printf("stream_lm_nq_args: every bad call refused before any launch\n");
    return 0;
}
