// The five-point solver of gim_amd/csrc/essential_solve.h on the CPU, as plain C++ (no HIP, no Python): a few hundred seeded samples
// of a synthetic two-view scene in normalised camera coordinates plus the degenerate ones the tests plant; every valid model is
// checked against its five points (epipolar residual), for unit norm and for the ok flags, the true E must be among the models of
// every general sample, a checksum is printed.  Meant to be built with a host sanitizer:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gim_amd/csrc tools/e5_host_check.cpp -o e5_host_check
//     ./e5_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "essential_solve.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
double uniform() {   // xorshift64*, in [0, 1)
    state ^= state >> 12, state ^= state << 25, state ^= state >> 27;
    return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

const double CS = cos(0.2), SN = sin(0.2), T[3] = {0.5, 0.1, 0.05};

// a point in front of both cameras (a turn of 0.2 rad about y, a sideways step) and its two normalised image positions
void correspondence(double* a, double* b) {
    const double X = -2.0 + 4.0 * uniform(), Y = -2.0 + 4.0 * uniform(), Z = 4.0 + 4.0 * uniform();
    const double X1 = CS * X + SN * Z + T[0], Y1 = Y + T[1], Z1 = -SN * X + CS * Z + T[2];
    a[0] = X / Z, a[1] = Y / Z;
    b[0] = X1 / Z1, b[1] = Y1 / Z1;
}

// E = [t]x R of that scene, unit Frobenius norm
void truth(double* E) {
    const double R[9] = {CS, 0.0, SN, 0.0, 1.0, 0.0, -SN, 0.0, CS};
    const double K[9] = {0.0, -T[2], T[1], T[2], 0.0, -T[0], -T[1], T[0], 0.0};
    double n2 = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            E[3 * i + j] = K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j] + K[3 * i + 2] * R[6 + j];
            n2 += E[3 * i + j] * E[3 * i + j];
        }
    for (int i = 0; i < 9; ++i) E[i] /= sqrt(n2);
}

struct Tally {
    int samples = 0, models = 0, rejected = 0, failures = 0;
    double worst_res = 0.0, worst_truth = 0.0, sum = 0.0;
};

// solves one sample; returns the number of valid models; checks what the contract promises of every slot.  Et: the true E or NULL.
int run(const double* p0, const double* p1, const double* Et, Tally* t) {
    static double work[GIM_E5_WORK];
    double E[90];
    bool ok[10];
    for (int i = 0; i < GIM_E5_WORK; ++i) work[i] = NAN;                                 // the solver may rely on nothing left in it
    gim_e5_solve(p0, p1, work, E, ok);
    int n = 0;
    double nearest = 1e300;
    for (int j = 0; j < 10; ++j) {
        const double* m = E + 9 * j;
        double n2 = 0.0;
        for (int i = 0; i < 9; ++i) n2 += m[i] * m[i];
        if (!ok[j]) {
            if (n2 != 0.0) printf("FAIL: an invalid slot is not zero\n"), t->failures += 1;
            continue;
        }
        ++n;
        if (!(fabs(n2 - 1.0) <= 1e-12)) printf("FAIL: |E| = %.17g\n", sqrt(n2)), t->failures += 1;
        for (int i = 0; i < 5; ++i) {
            const double x = p0[2 * i], y = p0[2 * i + 1], u = p1[2 * i], v = p1[2 * i + 1];
            const double r = u * (m[0] * x + m[1] * y + m[2]) + v * (m[3] * x + m[4] * y + m[5]) + (m[6] * x + m[7] * y + m[8]);
            if (!(fabs(r) <= t->worst_res)) t->worst_res = fabs(r);
        }
        if (Et) {
            double dm = 0.0, dp = 0.0;
            for (int i = 0; i < 9; ++i) dm += (m[i] - Et[i]) * (m[i] - Et[i]), dp += (m[i] + Et[i]) * (m[i] + Et[i]);
            const double d = sqrt(dm < dp ? dm : dp);
            if (d < nearest) nearest = d;
        }
        for (int i = 0; i < 9; ++i) t->sum += fabs(m[i]) * (double)(1 + i + 9 * j);
    }
    if (Et && n && nearest > t->worst_truth) t->worst_truth = nearest;
    t->samples += 1, t->models += n, t->rejected += n == 0;
    return n;
}

}  // namespace

int main() {
    Tally t;
    double p0[10], p1[10], Et[9];
    truth(Et);
    int general_valid = 0;
    for (int s = 0; s < 300; ++s) {
        for (int i = 0; i < 5; ++i) correspondence(p0 + 2 * i, p1 + 2 * i);
        if (run(p0, p1, Et, &t) == 0) printf("note: general sample %d rejected\n", s);
        else ++general_valid;
    }
    const int general = t.models;
    for (int s = 0; s < 100; ++s) {                                                      // general 5-tuples that belong to no one scene
        for (int i = 0; i < 5; ++i) correspondence(p0 + 2 * i, p1 + 2 * i), p1[2 * i] = -0.5 + uniform(), p1[2 * i + 1] = -0.4 + 0.8 * uniform();
        run(p0, p1, nullptr, &t);
    }
    const int before = t.models;
    int bad = 0;
    for (int s = 0; s < 20; ++s) {                                                      // five coincident points on both sides
        for (int i = 0; i < 5; ++i) correspondence(p0 + 2 * i, p1 + 2 * i);
        for (int i = 1; i < 5; ++i) p0[2 * i] = p0[0], p0[2 * i + 1] = p0[1], p1[2 * i] = p1[0], p1[2 * i + 1] = p1[1];
        bad += run(p0, p1, nullptr, &t);
    }
    for (int s = 0; s < 20; ++s) {                                                      // a repeated correspondence: rank 4
        for (int i = 0; i < 5; ++i) correspondence(p0 + 2 * i, p1 + 2 * i);
        p0[8] = p0[2], p0[9] = p0[3], p1[8] = p1[2], p1[9] = p1[3];
        bad += run(p0, p1, nullptr, &t);
    }
    for (int i = 0; i < 5; ++i) correspondence(p0 + 2 * i, p1 + 2 * i);                  // a NaN, an infinity, all zero
    p0[3] = NAN;
    bad += run(p0, p1, nullptr, &t);
    p0[3] = INFINITY;
    bad += run(p0, p1, nullptr, &t);
    p0[3] = 0.1, p1[6] = -INFINITY;
    bad += run(p0, p1, nullptr, &t);
    memset(p0, 0, sizeof p0), memset(p1, 0, sizeof p1);
    bad += run(p0, p1, nullptr, &t);
    printf("samples %d; 300 exact samples: %d with a model, %d models, the true E within %.3e of one of them; 100 general samples: %d models; "
           "%d degenerate samples: %d models; samples without a model %d\n",
           t.samples, general_valid, general, t.worst_truth, before - general, t.samples - 400, bad, t.rejected);
    printf("largest |p1^T E p0| over all valid models %.3e\n", t.worst_res);
    printf("checksum %.12e\n", t.sum);
    // the distance to the truth is printed for the record; its bar here only says "the truth was found" (this scene, a sideways step
    // with a small turn, has samples on which pose.five_point itself is 1e-9 away)
    const bool pass = general_valid == 300 && bad == 0 && t.failures == 0 && t.worst_res <= 1e-12 && t.worst_truth <= 1e-6;
    printf(pass ? "OK\n" : "FAIL\n");
    return pass ? 0 : 1;
}
