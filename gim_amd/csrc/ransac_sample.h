// The RANSAC sampler of csrc/ransac_sample.hip, as functions that compile for the host and for the device: the kernel runs
// gim_rs_sample on one lane per sample, tools/rs_host_check.cpp runs it on the CPU, pose.device_samples is the same arithmetic in
// numpy.  32- and 64-bit unsigned integers only, no floating point, no loop whose length depends on a random word; the contract is
// next to gim_ransac_sample in include/gim_hip.h.
//
// Sample number n of a run (the 0-based ordinal over the whole run, 64 bits) depends on (seed, n, P, m) alone:
//   words    Philox4x32-10 (Salmon et al., SC'11) under the key (seed & 0xffffffff, seed >> 32): the counters (n & 0xffffffff,
//            n >> 32, 0, 0) and (.., .., 1, 0) give r[0..3] and r[4..7];
//   indices  Floyd's algorithm, exactly m draws: for i = 0 .. m-1, j = P - m + i, t = (r[i] * (j + 1)) >> 32 (a uniform word scaled
//            to [0, j]); out[i] = t unless t occurs in out[0..i-1], else out[i] = j.  The set is uniform over the m-subsets of
//            [0, P) up to the bias of the multiply-shift: a value of [0, j] is hit by floor or ceil of 2^32 / (j + 1) words, so its
//            probability is off by at most (j + 1) / 2^32 relative (5e-7 at P = 2 000, one half at P = 2^31).  The ORDER inside a
//            sample is not uniform (j can only enter at place i); the minimal solvers do not depend on it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GIM_RS_FN __host__ __device__ inline
#else
#define GIM_RS_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GIM_RS_UNROLL _Pragma("unroll")
#else
#define GIM_RS_UNROLL
#endif

constexpr uint32_t GIM_RS_M0 = 0xD2511F53u, GIM_RS_M1 = 0xCD9E8D57u;   // the round multipliers
constexpr uint32_t GIM_RS_W0 = 0x9E3779B9u, GIM_RS_W1 = 0xBB67AE85u;   // the Weyl increments of the key
constexpr int GIM_RS_MAX_M = 7;                                        // one counter block pair gives 8 words

GIM_RS_FN bool gim_rs_supported(int m) { return m == 4 || m == 5 || m == 7; }

GIM_RS_FN uint32_t gim_rs_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// Philox4x32-10: ctr [4] is replaced by its output
GIM_RS_FN void gim_rs_philox(uint32_t* ctr, uint32_t k0, uint32_t k1) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    GIM_RS_UNROLL
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = gim_rs_mulhi(GIM_RS_M0, c0), l0 = GIM_RS_M0 * c0;
        const uint32_t h1 = gim_rs_mulhi(GIM_RS_M1, c2), l1 = GIM_RS_M1 * c2;
        c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
        k0 += GIM_RS_W0, k1 += GIM_RS_W1;
    }
    ctr[0] = c0, ctr[1] = c1, ctr[2] = c2, ctr[3] = c3;
}

// sample n of the run `seed` over P points: out[0 .. m-1] distinct indices of [0, P), or all -1 when P < m.  m <= GIM_RS_MAX_M.
template <int M>
GIM_RS_FN void gim_rs_sample_m(uint64_t seed, uint64_t n, int32_t P, int32_t* out) {
    static_assert(M >= 1 && M <= GIM_RS_MAX_M, "one sample takes at most 8 words");
    if (P < M) {
        GIM_RS_UNROLL
        for (int i = 0; i < M; ++i) out[i] = -1;
        return;
    }
    uint32_t r[8];
    GIM_RS_UNROLL
    for (int blk = 0; blk < (M > 4 ? 2 : 1); ++blk) {
        uint32_t c[4] = {(uint32_t)n, (uint32_t)(n >> 32), (uint32_t)blk, 0u};
        gim_rs_philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        GIM_RS_UNROLL
        for (int i = 0; i < 4; ++i) r[4 * blk + i] = c[i];
    }
    GIM_RS_UNROLL
    for (int i = 0; i < M; ++i) {
        const uint32_t j = (uint32_t)(P - M + i);                 // j + 1 <= P <= 2^31 - 1: no overflow
        const uint32_t t = gim_rs_mulhi(r[i], j + 1u);
        bool seen = false;
        GIM_RS_UNROLL
        for (int q = 0; q < i; ++q) seen = seen || out[q] == (int32_t)t;
        out[i] = (int32_t)(seen ? j : t);
    }
}

// run-time m (4, 5 or 7; anything else leaves `out` untouched and returns false)
GIM_RS_FN bool gim_rs_sample(uint64_t seed, uint64_t n, int32_t P, int m, int32_t* out) {
    if (m == 4) gim_rs_sample_m<4>(seed, n, P, out);
    else if (m == 5) gim_rs_sample_m<5>(seed, n, P, out);
    else if (m == 7) gim_rs_sample_m<7>(seed, n, P, out);
    else return false;
    return true;
}
