// The seven-point solver of gim_amd/csrc/fundamental_solve.h on the CPU, as plain C++ (no HIP, no Python): a few hundred seeded
// samples of a synthetic two-view scene plus the degenerate ones the tests plant, every valid model checked against its seven points,
// a checksum printed.  Meant to be built with a host sanitizer:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gim_amd/csrc tools/f7_host_check.cpp -o f7_host_check
//     ./f7_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fundamental_solve.h"
#include "two_view_residual.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
double uniform() {   // xorshift64*, in [0, 1)
    state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
    return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

// a point in front of both cameras and its two pixel positions; planar: the point lies on the plane z = 5 + 0.1 x
void correspondence(bool planar, double* a, double* b) {
    const double X = -2.0 + 4.0 * uniform(), Y = -2.0 + 4.0 * uniform();
    const double Z = planar ? 5.0 + 0.1 * X : 4.0 + 4.0 * uniform();
    const double c = cos(0.2), s = sin(0.2);
    const double X1 = c * X + s * Z + 0.5, Y1 = Y + 0.1, Z1 = -s * X + c * Z + 0.05;
    a[0] = 500.0 * X / Z + 320.0, a[1] = 500.0 * Y / Z + 240.0;
    b[0] = 500.0 * X1 / Z1 + 320.0, b[1] = 500.0 * Y1 / Z1 + 240.0;
}

struct Tally {
    int samples = 0, models = 0, rejected = 0;
    double worst = 0.0, sum = 0.0;
};

// solves one sample; returns the number of valid models; checks what the contract promises of every slot
int run(const double* p0, const double* p1, Tally* t) {
    double A[63], F[27];
    bool ok[3];
    gim_f7_solve(p0, p1, A, F, ok);
    int n = 0;
    for (int j = 0; j < 3; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < 9; ++i) n2 += F[9 * j + i] * F[9 * j + i];
        if (!ok[j]) {
            if (n2 != 0.0) printf("FAIL: an invalid slot is not zero\n"), t->rejected = -1000000;
            continue;
        }
        ++n;
        if (fabs(n2 - 1.0) > 1e-12) printf("FAIL: |F| = %.17g\n", sqrt(n2)), t->rejected = -1000000;
        for (int i = 0; i < 7; ++i) {
            // a point exactly on its epipolar line has Sampson error 0: thr2 = 1e-12 px^2 accepts rounding only
            if (!gim_tv_inlier(GIM_TV_EPIPOLAR, F + 9 * j, p0[2 * i], p0[2 * i + 1], p1[2 * i], p1[2 * i + 1], 1e-12)) t->worst = 1.0;
        }
        for (int i = 0; i < 9; ++i) t->sum += fabs(F[9 * j + i]) * (double)(1 + i + 9 * j);
    }
    t->samples += 1, t->models += n, t->rejected += n == 0;
    return n;
}

}  // namespace

int main() {
    Tally t;
    double p0[14], p1[14];
    for (int s = 0; s < 300; ++s) {
        for (int i = 0; i < 7; ++i) correspondence(false, p0 + 2 * i, p1 + 2 * i);
        if (run(p0, p1, &t) == 0) printf("note: general sample %d rejected\n", s);
    }
    const int general = t.models;
    int bad = 0;
    for (int s = 0; s < 20; ++s) {                                                      // a planar scene: rank 6
        for (int i = 0; i < 7; ++i) correspondence(true, p0 + 2 * i, p1 + 2 * i);
        bad += run(p0, p1, &t);
    }
    for (int s = 0; s < 20; ++s) {                                                      // seven collinear points on side 0
        for (int i = 0; i < 7; ++i) correspondence(false, p0 + 2 * i, p1 + 2 * i), p0[2 * i + 1] = 2.0 * p0[2 * i] + 3.0;
        bad += run(p0, p1, &t);
    }
    for (int s = 0; s < 20; ++s) {                                                      // seven coincident points on side 1
        for (int i = 0; i < 7; ++i) correspondence(false, p0 + 2 * i, p1 + 2 * i), p1[2 * i] = 123.456, p1[2 * i + 1] = 78.9;
        bad += run(p0, p1, &t);
    }
    for (int s = 0; s < 20; ++s) {                                                      // three matches share their point on side 1
        for (int i = 0; i < 7; ++i) correspondence(false, p0 + 2 * i, p1 + 2 * i);
        p1[2] = p1[4] = p1[0], p1[3] = p1[5] = p1[1];
        bad += run(p0, p1, &t);
    }
    for (int i = 0; i < 7; ++i) correspondence(false, p0 + 2 * i, p1 + 2 * i);          // a repeated point, a NaN, an infinity, all zero
    p0[12] = p0[0], p0[13] = p0[1], p1[12] = p1[0], p1[13] = p1[1];
    bad += run(p0, p1, &t);
    p0[3] = NAN;
    bad += run(p0, p1, &t);
    p0[3] = INFINITY;
    bad += run(p0, p1, &t);
    memset(p0, 0, sizeof p0), memset(p1, 0, sizeof p1);
    bad += run(p0, p1, &t);
    printf("samples %d, models of the 300 general samples %d, models of the %d degenerate samples %d, rejected %d\n", t.samples, general,
           t.samples - 300, bad, t.rejected);
    printf("checksum %.12e\n", t.sum);
    const bool pass = general >= 300 && bad == 0 && t.worst == 0.0 && t.rejected >= 0;
    printf(pass ? "OK\n" : "FAIL\n");
    return pass ? 0 : 1;
}
