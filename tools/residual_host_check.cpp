// The two residuals of gim_amd/csrc/two_view_residual.h on the CPU, as plain C++ (no HIP, no Python): 200 seeded model and point
// pairs per kind and the edge cases of the contract (the all-zero model, a NaN entry, a denominator below the clamp, w == 0, a
// projection that overflows, an error exactly at the threshold).  One line per case: the inputs, both residuals and both verdicts,
// every double as its 64 bits in hexadecimal; tests/test_residual_cpu.py restates the expressions in Python floats and asks for
// equal bits, so build with -ffp-contract=off.  Also meant to be built with a host sanitizer:
//
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I gim_amd/csrc tools/residual_host_check.cpp -o residual_host_check
//     ./residual_host_check
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "two_view_residual.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
double uniform() {   // xorshift64*, in [0, 1)
    state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
    return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}
double sym() { return 2.0 * uniform() - 1.0; }

uint64_t bits(double x) {
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return b;
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) printf("FAIL: %s\n", what), ++failures;
}

struct Verdict {
    double s, t;
    bool in1, in0;
};

// label: the kind the case was made for (0 / 1) or the name of an edge case
Verdict emit(const char* label, const double* M, const double* p, double thr2) {
    Verdict v;
    v.s = gim_tv_error(GIM_TV_EPIPOLAR, M, p[0], p[1], p[2], p[3]);
    v.t = gim_tv_error(GIM_TV_HOMOGRAPHY, M, p[0], p[1], p[2], p[3]);
    v.in1 = gim_tv_inlier(GIM_TV_EPIPOLAR, M, p[0], p[1], p[2], p[3], thr2);
    v.in0 = gim_tv_inlier(GIM_TV_HOMOGRAPHY, M, p[0], p[1], p[2], p[3], thr2);
    expect(v.in1 == gim_tv_within(GIM_TV_EPIPOLAR, v.s, thr2) && v.in0 == gim_tv_within(GIM_TV_HOMOGRAPHY, v.t, thr2),
           "inlier == within(error)");
    expect(v.s == gim_tv_sampson(M, p[0], p[1], p[2], p[3]) || (std::isnan(v.s) && std::isnan(gim_tv_sampson(M, p[0], p[1], p[2], p[3]))),
           "error(kind 1) is the Sampson error");
    printf("case %s", label);
    for (int i = 0; i < 9; ++i) printf(" %016" PRIx64, bits(M[i]));
    for (int i = 0; i < 4; ++i) printf(" %016" PRIx64, bits(p[i]));
    printf(" %016" PRIx64 " -> %016" PRIx64 " %016" PRIx64 " %d %d\n", bits(thr2), bits(v.s), bits(v.t), v.in1 ? 1 : 0, v.in0 ? 1 : 0);
    return v;
}

}  // namespace

int main() {
    // kind 1: a random 3 x 3 matrix and two points of [-1, 1]^2; the Sampson error is of order 0.1, the threshold of [0, 0.5)
    for (int i = 0; i < 200; ++i) {
        double M[9], p[4];
        for (double& m : M) m = sym();
        for (double& x : p) x = sym();
        emit("1", M, p, 0.5 * uniform());
    }
    // kind 0: a homography near the identity, b = proj(H a) moved by up to 0.2 per axis, the threshold of [0, 0.04)
    for (int i = 0; i < 200; ++i) {
        double H[9], p[4];
        for (int k = 0; k < 9; ++k) H[k] = (k % 4 == 0 ? 1.0 : 0.0) + 0.3 * sym();
        p[0] = sym(), p[1] = sym();
        const double w = H[6] * p[0] + H[7] * p[1] + H[8];
        p[2] = (H[0] * p[0] + H[1] * p[1] + H[2]) / w + 0.2 * sym();
        p[3] = (H[3] * p[0] + H[4] * p[1] + H[5]) / w + 0.2 * sym();
        emit("0", H, p, 0.04 * uniform());
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double pt[4] = {0.25, -0.5, 0.75, 0.125};
    {
        const double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const Verdict v = emit("zero", Z, pt, 0.0);
        expect(v.s == 0.0 && v.in1, "the all-zero model: Sampson 0, an inlier at thr2 = 0");
        expect(std::isnan(v.t) && !v.in0, "the all-zero model: w == 0, no transfer error, an outlier");
    }
    for (int k = 0; k < 9; ++k) {
        double M[9] = {1.0, 0.1, 0.2, -0.1, 1.0, 0.3, 0.01, 0.02, 1.0};
        M[k] = nan;
        const Verdict v = emit("nan", M, pt, std::numeric_limits<double>::infinity());
        expect(!v.in1 && !v.in0, "a model with a NaN entry: never an inlier");
    }
    {
        const double T[9] = {1e-160, 0, 0, 0, 1e-160, 0, 0, 0, 1e-160};       // den about 1e-320, below the clamp
        const Verdict v = emit("den", T, pt, 1.0);
        expect(std::isfinite(v.s) && v.s > 0.0, "den below 1e-300: the error is e^2 / 1e-300");
    }
    {
        const double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 0};                      // w == 0 for every point
        const Verdict v = emit("w0", H, pt, std::numeric_limits<double>::infinity());
        expect(std::isnan(v.t) && !v.in0, "w == 0: NaN, an outlier");
    }
    {
        const double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1e-320};                 // w so small that the projection overflows
        const Verdict v = emit("overflow", H, pt, std::numeric_limits<double>::infinity());
        expect(!std::isfinite(v.t) && !v.in0, "a projection that overflows: an outlier");
    }
    {
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        const double p[4] = {0.0, 0.0, 3.0, 4.0};                             // |b - a|^2 = 25 exactly
        const Verdict v = emit("at", I, p, 25.0);
        expect(v.t == 25.0 && v.in0, "the transfer error exactly at thr2: an inlier");
    }
    printf(failures == 0 ? "OK\n" : "FAIL\n");
    return failures == 0 ? 0 : 1;
}
