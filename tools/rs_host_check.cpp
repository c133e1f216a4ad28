// The RANSAC sampler of gim_amd/csrc/ransac_sample.h on the CPU, as plain C++ (no HIP, no Python): the Philox4x32-10 known answers,
// then a few thousand samples for every m at the edge point counts (m, m + 1, 9, 2 000, 4 097, 2^31 - 1), with ordinals that cross
// 2^32; every sample must hold m distinct indices of [0, P), P < m must give -1 everywhere, a refused m must leave the output
// untouched.  A checksum per (m, P) is printed; tests/test_ransac_sampler_cpu.py compares it with pose.device_samples'.  Meant to
// be built with a host sanitizer:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gim_amd/csrc tools/rs_host_check.cpp -o rs_host_check
//     ./rs_host_check
#include <cstdint>
#include <cstdio>

#include "ransac_sample.h"

namespace {

int failures = 0;

void known_answer(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o0, uint32_t o1, uint32_t o2,
                  uint32_t o3) {
    uint32_t c[4] = {c0, c1, c2, c3};
    gim_rs_philox(c, k0, k1);
    if (c[0] != o0 || c[1] != o1 || c[2] != o2 || c[3] != o3)
        printf("FAIL: philox gives %08x %08x %08x %08x, expected %08x %08x %08x %08x\n", c[0], c[1], c[2], c[3], o0, o1, o2, o3), ++failures;
}

constexpr uint64_t SEED = 0x0123456789ABCDEFull, FIRST = 0xFFFFFFFFull - 1000ull;   // the run crosses ordinal 2^32
constexpr int N = 4000;

// N samples from FIRST on; -> sum of (i + 1) * idx over all of them, modulo 2^64
uint64_t run(int m, int32_t P) {
    uint64_t sum = 0;
    for (int s = 0; s < N; ++s) {
        int32_t out[GIM_RS_MAX_M + 2];
        for (int i = 0; i < GIM_RS_MAX_M + 2; ++i) out[i] = -7;                     // guards behind the m places
        if (!gim_rs_sample(SEED, FIRST + (uint64_t)s, P, m, out)) printf("FAIL: m=%d refused\n", m), ++failures;
        for (int i = m; i < GIM_RS_MAX_M + 2; ++i)
            if (out[i] != -7) printf("FAIL: m=%d wrote place %d\n", m, i), ++failures;
        for (int i = 0; i < m; ++i) {
            if (P < m) {
                if (out[i] != -1) printf("FAIL: m=%d P=%d gives %d, not -1\n", m, P, out[i]), ++failures;
            } else {
                if (out[i] < 0 || out[i] >= P) printf("FAIL: m=%d P=%d index %d\n", m, P, out[i]), ++failures;
                for (int q = 0; q < i; ++q)
                    if (out[q] == out[i]) printf("FAIL: m=%d P=%d sample %d repeats %d\n", m, P, s, out[i]), ++failures;
            }
            sum += (uint64_t)(i + 1) * (uint64_t)(int64_t)out[i];
        }
        if (failures > 20) return sum;
    }
    return sum;
}

}  // namespace

int main() {
    known_answer(0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u);
    known_answer(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u,
                 0x6d5451fdu);
    known_answer(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u,
                 0x24126ea1u);
    const int ms[3] = {4, 5, 7};
    for (int mi = 0; mi < 3; ++mi) {
        const int m = ms[mi];
        const int32_t Ps[8] = {0, m - 1, m, m + 1, 9, 2000, 4097, 0x7fffffff};
        for (int pi = 0; pi < 8; ++pi) printf("m %d P %d checksum %016llx\n", m, Ps[pi], (unsigned long long)run(m, Ps[pi]));
    }
    int32_t out[GIM_RS_MAX_M] = {-7, -7, -7, -7, -7, -7, -7};
    for (int m = -1; m <= 9; ++m)
        if (!gim_rs_supported(m)) {
            if (gim_rs_sample(SEED, 0, 100, m, out) || out[0] != -7) printf("FAIL: m=%d was not refused\n", m), ++failures;
        }
    printf(failures == 0 ? "OK\n" : "FAIL\n");
    return failures == 0 ? 0 : 1;
}
