// The five-point essential-matrix solver of csrc/essential.hip, as functions that compile for the host and for the device: the kernel
// runs gim_e5_roots on one lane and gim_e5_model on one lane per root, tools/e5_host_check.cpp runs gim_e5_solve on the CPU (the
// arithmetic can be read against pose.five_point_ge without a GPU).  fp64, plain C++, real arithmetic only, every loop bounded; the
// contract is next to gim_essential_step in include/gim_hip.h.
//
// Everything that is indexed at run time lives in the work memory `w` (LDS on the device), GIM_E5_WORK doubles:
//   basis [4][9]    X, Y, Z, W of the null space, E = x X + y Y + z Z + W
//   M     [10][20]  the ten cubic constraints over the 20 monomials; after the reduction [I | B]
//   rows  [5][9]    the epipolar rows          } dead once M is built: the 10 x 10 Hessenberg matrix and the Householder vector of
//   EEt   [6][10], tr [10], tmp [10]           } its reduction take their place
//   roots [10]      the real eigenvalues, ascending
//   sys   [10][100] one 10 x 10 system Act - x I per root
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GIM_E5_FN __host__ __device__ inline
#else
#define GIM_E5_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GIM_E5_UNROLL _Pragma("unroll")
#else
#define GIM_E5_UNROLL
#endif

constexpr double GIM_E5_RANK_EPS = 1e-12;    // smallest fifth pivot of the 5 x 9 elimination, relative to the first
constexpr double GIM_E5_PIVOT_EPS = 1e-12;   // smallest pivot of the 10 x 10 cubic block, relative to the largest |entry| of the 10 x 20 matrix
constexpr double GIM_E5_W_EPS = 1e-14;       // smallest |v[9]| relative to max |v| of a root's null vector (pose.five_point's 1e-14)
constexpr double GIM_E5_QR_EPS = 2.220446049250313e-16;   // the deflation tests of the QR iteration
constexpr int GIM_E5_QR_ITS = 30;            // QR sweeps allowed per eigenvalue; exceptional shifts at sweeps 10 and 20

constexpr int GIM_E5_BASIS = 0, GIM_E5_M = 36, GIM_E5_ROWS = 236, GIM_E5_EET = 281, GIM_E5_TR = 341, GIM_E5_TMP = 351;
constexpr int GIM_E5_H = 236, GIM_E5_ORT = 336, GIM_E5_ROOTS = 362, GIM_E5_SYS = 372, GIM_E5_WORK = 1372;

// monomials: a linear polynomial has coefficients over (x, y, z, 1); degree <= 2 over pose._MONO2 = (x2, xy, xz, y2, yz, z2, x, y, z,
// 1); degree <= 3 over pose._MONO.  t12: (linear a) * (linear b) -> index in _MONO2; t23: (_MONO2 m) * (linear b) -> index in _MONO.
GIM_E5_FN int gim_e5_t12(int a, int b) {
    static constexpr uint8_t T[16] = {0, 1, 2, 6, 1, 3, 4, 7, 2, 4, 5, 8, 6, 7, 8, 9};
    return T[4 * a + b];
}
GIM_E5_FN int gim_e5_t23(int m, int b) {
    static constexpr uint8_t T[40] = {0,  1,  2,  10, 1,  3,  4,  11, 2,  4,  5,  12, 3,  6,  7,  13, 4,  7,  8,  14,
                                      5,  8,  9,  15, 10, 11, 12, 16, 11, 13, 14, 17, 12, 14, 15, 18, 16, 17, 18, 19};
    return T[4 * m + b];
}

// P2 += sg * e[ca] * e[cb]: the entries ca, cb of E as linear polynomials (column c of the basis), the product over _MONO2
GIM_E5_FN void gim_e5_acc11(double* P2, double sg, const double* Bs, int ca, int cb) {
    GIM_E5_UNROLL
    for (int a = 0; a < 4; ++a) {
        GIM_E5_UNROLL
        for (int b = 0; b < 4; ++b) P2[gim_e5_t12(a, b)] += sg * (Bs[9 * a + ca] * Bs[9 * b + cb]);
    }
}

// row += sg * P2 * e[c]: a polynomial of degree <= 2 times an entry of E, the product over _MONO
GIM_E5_FN void gim_e5_acc21(double* row, double sg, const double* P2, const double* Bs, int c) {
    GIM_E5_UNROLL
    for (int m = 0; m < 10; ++m) {
        GIM_E5_UNROLL
        for (int b = 0; b < 4; ++b) row[gim_e5_t23(m, b)] += sg * (P2[m] * Bs[9 * b + c]);
    }
}

// phase 1: the 5 x 9 epipolar rows, Gauss-Jordan with full pivoting, the basis of the four free columns.  false: refused.
GIM_E5_FN bool gim_e5_nullspace(const double p0[10], const double p1[10], double* w) {
    double* A = w + GIM_E5_ROWS;
    double* Bs = w + GIM_E5_BASIS;
    bool fin = true;
    GIM_E5_UNROLL
    for (int i = 0; i < 10; ++i) fin = fin && isfinite(p0[i]) && isfinite(p1[i]);
    if (!fin) return false;
    GIM_E5_UNROLL
    for (int i = 0; i < 5; ++i) {
        const double x = p0[2 * i], y = p0[2 * i + 1], u = p1[2 * i], v = p1[2 * i + 1];
        double* r = A + 9 * i;
        r[0] = u * x, r[1] = u * y, r[2] = u, r[3] = v * x, r[4] = v * y, r[5] = v, r[6] = x, r[7] = y, r[8] = 1.0;
    }
    // the largest |a| over the rows k.. and all columns; the lowest row, then the lowest column, wins a tie.  rowof: four bits per
    // column, the row whose pivot sits in it, 15 for a free column.
    uint64_t rowof = 0xFFFFFFFFFull;
    double first = 0.0;
    for (int k = 0; k < 5; ++k) {
        int pr = k, pc = 0;
        double best = 0.0;
        for (int r = k; r < 5; ++r)
            for (int c = 0; c < 9; ++c) {
                const double a = fabs(A[r * 9 + c]);
                if (a > best) best = a, pr = r, pc = c;
            }
        if (k == 0) first = best;
        if (!(best > 0.0) || !isfinite(best)) return false;
        if (k == 4 && !(best >= GIM_E5_RANK_EPS * first)) return false;                       // rank-deficient sample
        if (pr != k)
            for (int c = 0; c < 9; ++c) {
                const double t = A[k * 9 + c];
                A[k * 9 + c] = A[pr * 9 + c];
                A[pr * 9 + c] = t;
            }
        const double d = A[k * 9 + pc];
        for (int c = 0; c < 9; ++c) A[k * 9 + c] = A[k * 9 + c] / d;
        for (int r = 0; r < 5; ++r) {
            if (r == k) continue;
            const double f = A[r * 9 + pc];
            for (int c = 0; c < 9; ++c) A[r * 9 + c] -= f * A[k * 9 + c];
        }
        rowof = (rowof & ~(0xFull << (4 * pc))) | ((uint64_t)k << (4 * pc));
    }
    int f0 = -1, f1 = -1, f2 = -1, f3 = -1;                                                   // the four free columns, ascending
    for (int c = 0; c < 9; ++c)
        if (((rowof >> (4 * c)) & 15) == 15) {
            if (f0 < 0) f0 = c;
            else if (f1 < 0) f1 = c;
            else if (f2 < 0) f2 = c;
            else f3 = c;
        }
    for (int c = 0; c < 9; ++c) {
        const int r = (int)((rowof >> (4 * c)) & 15);
        const bool piv = r != 15;
        const double* row = A + 9 * (piv ? r : 0);
        Bs[c] = c == f0 ? 1.0 : (piv ? -row[f0] : 0.0);
        Bs[9 + c] = c == f1 ? 1.0 : (piv ? -row[f1] : 0.0);
        Bs[18 + c] = c == f2 ? 1.0 : (piv ? -row[f2] : 0.0);
        Bs[27 + c] = c == f3 ? 1.0 : (piv ? -row[f3] : 0.0);
    }
    return true;
}

// phase 2: det E = 0 and the nine entries of 2 E E^T E - tr(E E^T) E, rows in the order pose.five_point stacks them
GIM_E5_FN void gim_e5_constraints(double* w) {
    const double* Bs = w + GIM_E5_BASIS;
    double* M = w + GIM_E5_M;
    double* EEt = w + GIM_E5_EET;                                                             // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    double* tr = w + GIM_E5_TR;
    double* tmp = w + GIM_E5_TMP;
    for (int i = 0; i < 60; ++i) EEt[i] = 0.0;
    for (int i = 0; i < 200; ++i) M[i] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double* P = EEt + 10 * (3 * i - (i * (i - 1)) / 2 + (j - i));
            for (int k = 0; k < 3; ++k) gim_e5_acc11(P, 1.0, Bs, 3 * i + k, 3 * j + k);
        }
    for (int t = 0; t < 10; ++t) tr[t] = (EEt[t] + EEt[30 + t]) + EEt[50 + t];
    // det E by the cofactors of the first row: e00 (e11 e22 - e12 e21) - e01 (e10 e22 - e12 e20) + e02 (e10 e21 - e11 e20)
    for (int t = 0; t < 10; ++t) tmp[t] = 0.0;
    gim_e5_acc11(tmp, 1.0, Bs, 4, 8), gim_e5_acc11(tmp, -1.0, Bs, 5, 7);
    gim_e5_acc21(M, 1.0, tmp, Bs, 0);
    for (int t = 0; t < 10; ++t) tmp[t] = 0.0;
    gim_e5_acc11(tmp, 1.0, Bs, 3, 8), gim_e5_acc11(tmp, -1.0, Bs, 5, 6);
    gim_e5_acc21(M, -1.0, tmp, Bs, 1);
    for (int t = 0; t < 10; ++t) tmp[t] = 0.0;
    gim_e5_acc11(tmp, 1.0, Bs, 3, 7), gim_e5_acc11(tmp, -1.0, Bs, 4, 6);
    gim_e5_acc21(M, 1.0, tmp, Bs, 2);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double* row = M + 20 * (1 + 3 * i + j);
            for (int k = 0; k < 3; ++k) {
                const int lo = i < k ? i : k, hi = i < k ? k : i;
                gim_e5_acc21(row, 1.0, EEt + 10 * (3 * lo - (lo * (lo - 1)) / 2 + (hi - lo)), Bs, 3 * k + j);
            }
            for (int t = 0; t < 20; ++t) row[t] = 2.0 * row[t];
            gim_e5_acc21(row, -1.0, tr, Bs, 3 * i + j);
        }
}

// phase 3: Gauss-Jordan with partial pivoting on the cubic block, M -> [I | B].  false: refused.
GIM_E5_FN bool gim_e5_reduce(double* w) {
    double* M = w + GIM_E5_M;
    double mmax = 0.0;
    bool fin = true;
    for (int i = 0; i < 200; ++i) {
        const double a = fabs(M[i]);
        fin = fin && isfinite(a);
        if (a > mmax) mmax = a;
    }
    if (!fin || !(mmax > 0.0)) return false;
    for (int k = 0; k < 10; ++k) {
        int pr = k;
        double best = 0.0;
        for (int r = k; r < 10; ++r) {
            const double a = fabs(M[r * 20 + k]);
            if (a > best) best = a, pr = r;
        }
        if (!(best >= GIM_E5_PIVOT_EPS * mmax) || !isfinite(best)) return false;
        if (pr != k)
            for (int c = k; c < 20; ++c) {
                const double t = M[k * 20 + c];
                M[k * 20 + c] = M[pr * 20 + c];
                M[pr * 20 + c] = t;
            }
        const double d = M[k * 20 + k];
        for (int c = k; c < 20; ++c) M[k * 20 + c] = M[k * 20 + c] / d;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = M[r * 20 + k];
            for (int c = k; c < 20; ++c) M[r * 20 + c] -= f * M[k * 20 + c];
        }
    }
    return true;
}

// entry (r, c) of the action matrix of multiplication by x on the basis (x2, xy, xz, y2, yz, z2, x, y, z, 1), as pose.five_point
// builds it from B
GIM_E5_FN double gim_e5_act(const double* M, int r, int c) {
    if (r < 6) return -M[r * 20 + 10 + c];
    return ((r == 6 && c == 0) || (r == 7 && c == 1) || (r == 8 && c == 2) || (r == 9 && c == 6)) ? 1.0 : 0.0;
}

// phase 4: the real eigenvalues of the action matrix, ascending, into w[GIM_E5_ROOTS ..]; their number is returned.  Householder
// reduction to Hessenberg form (EISPACK orthes), then the real Francis double-shift QR iteration (EISPACK hqr, eigenvalues only).
GIM_E5_FN int gim_e5_eigenvalues(double* w) {
    const double* M = w + GIM_E5_M;
    double* a = w + GIM_E5_H;
    double* ort = w + GIM_E5_ORT;
    double* roots = w + GIM_E5_ROOTS;
    for (int r = 0; r < 10; ++r)
        for (int c = 0; c < 10; ++c) a[r * 10 + c] = gim_e5_act(M, r, c);
    for (int m = 1; m < 9; ++m) {
        double scale = 0.0;
        for (int i = m; i < 10; ++i) scale += fabs(a[i * 10 + m - 1]);
        if (scale == 0.0) continue;
        double h = 0.0;
        for (int i = 9; i >= m; --i) {
            ort[i] = a[i * 10 + m - 1] / scale;
            h += ort[i] * ort[i];
        }
        const double g = -copysign(sqrt(h), ort[m]);
        h -= ort[m] * g;
        ort[m] -= g;
        for (int j = m; j < 10; ++j) {                                                        // (I - u u^T / h) A
            double f = 0.0;
            for (int i = 9; i >= m; --i) f += ort[i] * a[i * 10 + j];
            f /= h;
            for (int i = m; i < 10; ++i) a[i * 10 + j] -= f * ort[i];
        }
        for (int i = 0; i < 10; ++i) {                                                        // A (I - u u^T / h)
            double f = 0.0;
            for (int j = 9; j >= m; --j) f += ort[j] * a[i * 10 + j];
            f /= h;
            for (int j = m; j < 10; ++j) a[i * 10 + j] -= f * ort[j];
        }
        a[m * 10 + m - 1] = scale * g;
        for (int i = m + 1; i < 10; ++i) a[i * 10 + m - 1] = 0.0;
    }
    double anorm = 0.0;
    for (int i = 0; i < 10; ++i)
        for (int j = i > 0 ? i - 1 : 0; j < 10; ++j) anorm += fabs(a[i * 10 + j]);
    if (!isfinite(anorm)) return 0;
    int nr = 0, nn = 9, its = 0;
    double t = 0.0;
    for (int guard = 0; guard < 10 * (GIM_E5_QR_ITS + 1) && nn >= 0; ++guard) {
        int l = nn;
        for (; l > 0; --l) {                                                                  // a small subdiagonal element
            double s = fabs(a[(l - 1) * 10 + l - 1]) + fabs(a[l * 10 + l]);
            if (s == 0.0) s = anorm;
            if (fabs(a[l * 10 + l - 1]) <= GIM_E5_QR_EPS * s) {
                a[l * 10 + l - 1] = 0.0;
                break;
            }
        }
        double x = a[nn * 10 + nn];
        if (l == nn) {                                                                        // one root
            roots[nr++] = x + t;
            nn -= 1, its = 0;
            continue;
        }
        double y = a[(nn - 1) * 10 + nn - 1];
        double ww = a[nn * 10 + nn - 1] * a[(nn - 1) * 10 + nn];
        if (l == nn - 1) {                                                                    // a 2 x 2 block: two real roots or a complex pair
            const double p = 0.5 * (y - x);
            const double q = p * p + ww;
            double z = sqrt(fabs(q));
            x += t;
            if (q >= 0.0) {
                z = p + copysign(z, p);
                roots[nr] = x + z;
                roots[nr + 1] = z != 0.0 ? x - ww / z : x + z;
                nr += 2;
            }
            nn -= 2, its = 0;
            continue;
        }
        if (its == GIM_E5_QR_ITS) break;                                                      // no convergence: what is left has no models
        if (its == 10 || its == 20) {                                                         // exceptional shift
            t += x;
            for (int i = 0; i <= nn; ++i) a[i * 10 + i] -= x;
            const double s = fabs(a[nn * 10 + nn - 1]) + fabs(a[(nn - 1) * 10 + nn - 2]);
            y = x = 0.75 * s;
            ww = -0.4375 * s * s;
        }
        ++its;
        double p = 0.0, q = 0.0, r = 0.0, z = 0.0;
        int m = nn - 2;
        for (; m >= l; --m) {                                                                 // two consecutive small subdiagonal elements
            z = a[m * 10 + m];
            r = x - z;
            double s = y - z;
            p = (r * s - ww) / a[(m + 1) * 10 + m] + a[m * 10 + m + 1];
            q = a[(m + 1) * 10 + m + 1] - z - r - s;
            r = a[(m + 2) * 10 + m + 1];
            s = fabs(p) + fabs(q) + fabs(r);
            p /= s, q /= s, r /= s;
            if (m == l) break;
            const double u = fabs(a[m * 10 + m - 1]) * (fabs(q) + fabs(r));
            const double v = fabs(p) * (fabs(a[(m - 1) * 10 + m - 1]) + fabs(z) + fabs(a[(m + 1) * 10 + m + 1]));
            if (u <= GIM_E5_QR_EPS * v) break;
        }
        for (int i = m; i < nn - 1; ++i) {
            a[(i + 2) * 10 + i] = 0.0;
            if (i != m) a[(i + 2) * 10 + i - 1] = 0.0;
        }
        for (int k = m; k < nn; ++k) {                                                        // the double QR step on rows l .. nn, columns m .. nn
            if (k != m) {
                p = a[k * 10 + k - 1];
                q = a[(k + 1) * 10 + k - 1];
                r = k + 1 != nn ? a[(k + 2) * 10 + k - 1] : 0.0;
                x = fabs(p) + fabs(q) + fabs(r);
                if (x != 0.0) p /= x, q /= x, r /= x;
            }
            const double s = copysign(sqrt(p * p + q * q + r * r), p);
            if (s == 0.0 || !isfinite(s)) continue;
            if (k == m) {
                if (l != m) a[k * 10 + k - 1] = -a[k * 10 + k - 1];
            } else {
                a[k * 10 + k - 1] = -s * x;
            }
            p += s;
            x = p / s, y = q / s, z = r / s;
            q /= p, r /= p;
            for (int j = k; j <= nn; ++j) {
                p = a[k * 10 + j] + q * a[(k + 1) * 10 + j];
                if (k + 1 != nn) {
                    p += r * a[(k + 2) * 10 + j];
                    a[(k + 2) * 10 + j] -= p * z;
                }
                a[(k + 1) * 10 + j] -= p * y;
                a[k * 10 + j] -= p * x;
            }
            const int mmin = nn < k + 3 ? nn : k + 3;
            for (int i = l; i <= mmin; ++i) {
                p = x * a[i * 10 + k] + y * a[i * 10 + k + 1];
                if (k + 1 != nn) {
                    p += z * a[i * 10 + k + 2];
                    a[i * 10 + k + 2] -= p * r;
                }
                a[i * 10 + k + 1] -= p * q;
                a[i * 10 + k] -= p;
            }
        }
    }
    for (int i = 1; i < nr; ++i) {                                                            // ascending; NaN never moves
        const double v = roots[i];
        int j = i;
        for (; j > 0 && roots[j - 1] > v; --j) roots[j] = roots[j - 1];
        roots[j] = v;
    }
    return nr;
}

// phases 1-4 on one sample: the number of real roots (0: the sample is refused or has none), the roots ascending in w[GIM_E5_ROOTS ..]
GIM_E5_FN int gim_e5_roots(const double p0[10], const double p1[10], double* w) {
    if (!gim_e5_nullspace(p0, p1, w)) return 0;
    gim_e5_constraints(w);
    if (!gim_e5_reduce(w)) return 0;
    return gim_e5_eigenvalues(w);
}

// phase 5 on one root: the null vector v of Act - x I by Gauss-Jordan with full pivoting in S [10][10] (the free column is 1),
// (x, y, z) = v[6..8] / v[9], E = x X + y Y + z Z + W scaled to unit Frobenius norm.  false: the slot is refused (E is then untouched).
GIM_E5_FN bool gim_e5_model(const double* w, double lam, double* S, double E[9]) {
    const double* M = w + GIM_E5_M;
    const double* Bs = w + GIM_E5_BASIS;
    for (int r = 0; r < 10; ++r)
        for (int c = 0; c < 10; ++c) {
            const double v = gim_e5_act(M, r, c);
            S[r * 10 + c] = r == c ? v - lam : v;
        }
    uint64_t rowof = 0xFFFFFFFFFFull;
    for (int k = 0; k < 9; ++k) {
        int pr = k, pc = 0;
        double best = 0.0;
        for (int r = k; r < 10; ++r)
            for (int c = 0; c < 10; ++c) {
                const double a = fabs(S[r * 10 + c]);
                if (a > best) best = a, pr = r, pc = c;
            }
        if (!(best > 0.0) || !isfinite(best)) return false;
        if (pr != k)
            for (int c = 0; c < 10; ++c) {
                const double t = S[k * 10 + c];
                S[k * 10 + c] = S[pr * 10 + c];
                S[pr * 10 + c] = t;
            }
        const double d = S[k * 10 + pc];
        for (int c = 0; c < 10; ++c) S[k * 10 + c] = S[k * 10 + c] / d;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = S[r * 10 + pc];
            for (int c = 0; c < 10; ++c) S[r * 10 + c] -= f * S[k * 10 + c];
        }
        rowof = (rowof & ~(0xFull << (4 * pc))) | ((uint64_t)k << (4 * pc));
    }
    int fc = 0;
    for (int c = 0; c < 10; ++c)
        if (((rowof >> (4 * c)) & 15) == 15) fc = c;
    double v6 = 0.0, v7 = 0.0, v8 = 0.0, v9 = 0.0, vmax = 0.0;
    for (int c = 0; c < 10; ++c) {
        const int r = (int)((rowof >> (4 * c)) & 15);
        const double v = c == fc ? 1.0 : -S[(r % 10) * 10 + fc];
        if (fabs(v) > vmax) vmax = fabs(v);
        if (c == 6) v6 = v;
        if (c == 7) v7 = v;
        if (c == 8) v8 = v;
        if (c == 9) v9 = v;
    }
    if (!(fabs(v9) > GIM_E5_W_EPS * vmax) || !isfinite(vmax)) return false;
    const double x = v6 / v9, y = v7 / v9, z = v8 / v9;
    double e[9];
    double n2 = 0.0;
    GIM_E5_UNROLL
    for (int i = 0; i < 9; ++i) {
        e[i] = ((x * Bs[i] + y * Bs[9 + i]) + z * Bs[18 + i]) + Bs[27 + i];
        n2 += e[i] * e[i];
    }
    const double nrm = sqrt(n2);
    if (!(nrm > 0.0) || !isfinite(nrm)) return false;
    GIM_E5_UNROLL
    for (int i = 0; i < 9; ++i) E[i] = e[i] / nrm;
    return true;
}

// p0, p1 [5][2] in normalised camera coordinates -> up to ten E [10][9] row-major with p1^T E p0 = 0, unit Frobenius norm, ordered by
// the root x ascending; ok[j] = false and a zero matrix for an unused or rejected slot.  w: GIM_E5_WORK doubles of work memory.
GIM_E5_FN void gim_e5_solve(const double p0[10], const double p1[10], double* w, double E[90], bool ok[10]) {
    for (int i = 0; i < 90; ++i) E[i] = 0.0;
    for (int j = 0; j < 10; ++j) ok[j] = false;
    const int nr = gim_e5_roots(p0, p1, w);
    for (int j = 0; j < nr; ++j) ok[j] = gim_e5_model(w, w[GIM_E5_ROOTS + j], w + GIM_E5_SYS + 100 * j, E + 9 * j);
}
