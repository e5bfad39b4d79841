// weight_drop.h -- the rule of lstm_hip_set_weight_drop (include/lstm_hip.h), compiled by host and
// device code alike: Philox4x32-10 and the keep decision of one element of the logical 4N x N matrix U.  The mask kernel
// (kernels.hip, k_weight_drop) and lstm_hip_weight_drop_mask on the CPU both run exactly this text.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WD_FN __host__ __device__ inline
#else
#define WD_FN inline
#endif

namespace weight_drop {

struct Words {
    uint32_t w[4];
};

// Philox4x32-10: counter (c0, c1, c2, c3), key (k0, k1).  Per round c <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1,
// lo(M0*c0)), then the key is bumped; ten rounds.
WD_FN Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

// the four words of quad q = e >> 2 (elements 4q .. 4q + 3) under (seed, t)
WD_FN Words quad_words(uint64_t q, uint64_t seed, uint64_t t) {
    return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)t, (uint32_t)(t >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}
WD_FN bool keep_word(uint32_t word, uint32_t thr) { return word >= thr; }

// host numbers of a rate 0 < rate < 1, in double: thr = floor(rate * 2^32), scale = 1 / (1 - rate) narrowed
inline uint32_t threshold(double rate) { return (uint32_t)(rate * 4294967296.0); }
inline float scale(double rate) { return (float)(1.0 / (1.0 - rate)); }

} // namespace weight_drop
#undef WD_FN
