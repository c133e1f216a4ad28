"""The numpy-only half of gim_amd/pose.py (no torch, no gim_amd.ops): the LAPACK minimal solvers and errors, the line-for-line
restatements of the device kernels that serve as their CPU oracles (the `*_ge` functions, `homography_4pt`), the counter-based sampler,
the per-step record reductions and the MAGSAC++ gain.  pose.py imports this module, never the reverse, and re-exports its public names."""
import itertools

import numpy as np

# ---- polynomial bookkeeping for the five-point constraints -------------------------------------------------------------
# monomials of degree <= 3 in (x, y, z): the ten cubic ones first (eliminated by Gauss-Jordan), then the basis of the quotient ring
_MONO = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
         (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_IDX = {m: i for i, m in enumerate(_MONO)}


# degree <= 2 monomials (products of two linear polynomials), in _MONO's order of them
_MONO2 = [m for m in _MONO if sum(m) <= 2]
_IDX2 = {m: i for i, m in enumerate(_MONO2)}
_LIN1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]                          # a linear polynomial is (x, y, z, 1) coefficients


def _tables():
    t12 = np.zeros((4, 4, len(_MONO2)))                                      # linear x linear -> degree <= 2
    for (i, a), (j, b) in itertools.product(enumerate(_LIN1), repeat=2):
        t12[i, j, _IDX2[(a[0] + b[0], a[1] + b[1], a[2] + b[2])]] = 1.0
    t23 = np.zeros((len(_MONO2), 4, 20))                                     # degree <= 2 x linear -> degree <= 3
    for (i, a), (j, b) in itertools.product(enumerate(_MONO2), enumerate(_LIN1)):
        t23[i, j, _IDX[(a[0] + b[0], a[1] + b[1], a[2] + b[2])]] = 1.0
    return t12.reshape(16, -1), t23.reshape(4 * len(_MONO2), 20)


_T12, _T23 = _tables()


def _mul11(a, b):
    """linear x linear (coefficients over x, y, z, 1) -> coefficients over _MONO2; batched over leading axes"""
    return (a[..., :, None] * b[..., None, :]).reshape(*a.shape[:-1], 16) @ _T12


def _mul21(a, b):
    """degree <= 2 (over _MONO2) x linear -> coefficients over _MONO"""
    return (a[..., :, None] * b[..., None, :]).reshape(*a.shape[:-1], a.shape[-1] * 4) @ _T23


def _nullspace(A, k):
    """last k right singular vectors of every matrix of the batch A [N, r, 9] (r < 9: full_matrices gives the whole basis)"""
    _, _, vt = np.linalg.svd(A, full_matrices=True)
    return vt[:, 9 - k:, :]


def _epipolar_rows(x0, x1):
    """rows of the linear system x1^T M x0 = 0 in the row-major entries of M; x0, x1 [..., 2] (homogeneous 1 appended)"""
    o = np.ones_like(x0[..., :1])
    h0 = np.concatenate([x0, o], -1)
    h1 = np.concatenate([x1, o], -1)
    return (h1[..., :, None] * h0[..., None, :]).reshape(*x0.shape[:-1], 9)


def five_point(x0, x1):
    """Essential matrices through 5 correspondences.  x0, x1: [N, 5, 2] normalised image points (x1^T E x0 = 0).
    -> (E [N, 10, 3, 3], valid [N, 10]): up to ten real solutions per sample, each scaled to unit Frobenius norm."""
    x0 = np.asarray(x0, dtype=np.float64)
    x1 = np.asarray(x1, dtype=np.float64)
    n = x0.shape[0]
    basis = _nullspace(_epipolar_rows(x0, x1), 4).reshape(n, 4, 3, 3)       # X, Y, Z, W
    # E = x X + y Y + z Z + W: every entry a linear polynomial, coefficients (x, y, z, 1)
    Ep = np.moveaxis(basis, 1, -1)                                           # [N, 3, 3, 4]
    e = lambda i, j: Ep[:, i, j]   # noqa: E731

    def m2(a, b, c, d):   # a b - c d
        return _mul11(a, b) - _mul11(c, d)
    det = (_mul21(m2(e(1, 1), e(2, 2), e(1, 2), e(2, 1)), e(0, 0)) -
           _mul21(m2(e(1, 0), e(2, 2), e(1, 2), e(2, 0)), e(0, 1)) +
           _mul21(m2(e(1, 0), e(2, 1), e(1, 1), e(2, 0)), e(0, 2)))
    # E E^T (degree 2), its trace, then 2 (E E^T) E - tr(E E^T) E
    EEt = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            EEt[i][j] = EEt[j][i] = _mul11(e(i, 0), e(j, 0)) + _mul11(e(i, 1), e(j, 1)) + _mul11(e(i, 2), e(j, 2))
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    rows = [det]
    for i in range(3):
        for j in range(3):
            sij = _mul21(EEt[i][0], e(0, j)) + _mul21(EEt[i][1], e(1, j)) + _mul21(EEt[i][2], e(2, j))
            rows.append(2.0 * sij - _mul21(tr, e(i, j)))
    M = np.stack(rows, 1)                                                   # [N, 10, 20]
    # Gauss-Jordan on the cubic block: [I | B]
    A, Bm = M[:, :, :10], M[:, :, 10:]
    ok = np.ones(n, dtype=bool)
    try:
        B = np.linalg.solve(A, Bm)
    except np.linalg.LinAlgError:
        B = np.zeros_like(Bm)
        for s in range(n):
            try:
                B[s] = np.linalg.solve(A[s], Bm[s])
            except np.linalg.LinAlgError:
                ok[s] = False
    ok &= np.isfinite(B).all((1, 2))
    B = np.where(ok[:, None, None], B, 0.0)
    # action matrix of multiplication by x on the basis [x^2, xy, xz, y^2, yz, z^2, x, y, z, 1]
    Act = np.zeros((n, 10, 10))
    Act[:, :6] = -B[:, :6]
    Act[:, 6, 0] = Act[:, 7, 1] = Act[:, 8, 2] = Act[:, 9, 6] = 1.0
    ev, vec = np.linalg.eig(Act)                                            # columns of vec: the basis evaluated at a solution
    real = (np.abs(ev.imag) < 1e-9 * (1.0 + np.abs(ev.real))) & ok[:, None]
    v = vec.real
    w = v[:, 9, :]
    real &= np.abs(w) > 1e-14
    w = np.where(real, w, 1.0)
    xyz = np.stack([v[:, 6, :] / w, v[:, 7, :] / w, v[:, 8, :] / w], -1)    # [N, 10, 3]
    E = (xyz[..., 0, None, None] * basis[:, None, 0] + xyz[..., 1, None, None] * basis[:, None, 1] +
         xyz[..., 2, None, None] * basis[:, None, 2] + basis[:, None, 3])
    nrm = np.linalg.norm(E.reshape(n, 10, 9), axis=-1)
    real &= np.isfinite(nrm) & (nrm > 0)
    E = np.where(real[..., None, None], E / np.where(real, nrm, 1.0)[..., None, None], 0.0)
    return E, real


def seven_point(x0, x1):
    """Fundamental matrices through 7 correspondences.  x0, x1: [N, 7, 2] (any units; x1^T F x0 = 0).
    -> (F [N, 3, 3, 3], valid [N, 3]): the real roots of det(a F1 + (1 - a) F2) = 0."""
    x0 = np.asarray(x0, dtype=np.float64)
    x1 = np.asarray(x1, dtype=np.float64)
    n = x0.shape[0]
    ns = _nullspace(_epipolar_rows(x0, x1), 2).reshape(n, 2, 3, 3)
    F1, F2 = ns[:, 0], ns[:, 1]
    # det(a F1 + (1 - a) F2) is a cubic in a: interpolate it at four abscissae
    aa = np.array([0.0, 1.0, -1.0, 2.0])
    d = np.stack([np.linalg.det(a * F1 + (1.0 - a) * F2) for a in aa], -1)  # [N, 4]
    V = np.vander(aa, 4, increasing=True)                                   # d = V c
    c = np.linalg.solve(V, d.T).T                                           # c0 + c1 a + c2 a^2 + c3 a^3
    lead = c[:, 3]
    good = np.abs(lead) > 1e-14 * (np.abs(c).max(1) + 1e-300)
    cm = np.zeros((n, 3, 3))
    ld = np.where(good, lead, 1.0)
    cm[:, 0, 2] = -c[:, 0] / ld
    cm[:, 1, 2] = -c[:, 1] / ld
    cm[:, 2, 2] = -c[:, 2] / ld
    cm[:, 1, 0] = cm[:, 2, 1] = 1.0
    roots = np.linalg.eigvals(cm)                                           # [N, 3]
    real = (np.abs(roots.imag) < 1e-9 * (1.0 + np.abs(roots.real))) & good[:, None]
    a = roots.real
    F = a[..., None, None] * F1[:, None] + (1.0 - a)[..., None, None] * F2[:, None]
    nrm = np.linalg.norm(F.reshape(n, 3, 9), axis=-1)
    real &= np.isfinite(nrm) & (nrm > 0)
    F = np.where(real[..., None, None], F / np.where(real, nrm, 1.0)[..., None, None], 0.0)
    return F, real


F7_SCALE_EPS = 1e-12    # smallest mean distance of a side's seven points from their centre
F7_RANK_EPS = 1e-12     # smallest seventh pivot of the 7 x 9 elimination, relative to the first
F7_CUBIC_EPS = 1e-12    # smallest max |c| of the cubic: below it every matrix a F1 + (1 - a) F2 is singular, the cubic is noise
F7_LEAD_EPS = 1e-14     # smallest |c3| relative to max |c| (seven_point's rule)
F7_DISC_EPS = 1e-9      # |discriminant| / scale below which one real root and three cannot be told apart


def _f7_normalise(p):
    """[N, 7, 2] -> (q with zero mean and mean distance sqrt(2), centre [N, 2], scale [N], ok [N]); q = (p - c) * s"""
    c = ((((((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]) + p[:, 4]) + p[:, 5]) + p[:, 6]) / 7.0
    q = p - c[:, None]
    d = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1])
    md = ((((((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]) + d[:, 4]) + d[:, 5]) + d[:, 6]) / 7.0
    ok = np.isfinite(md) & (md >= F7_SCALE_EPS)
    s = np.sqrt(2.0) / np.where(ok, md, 1.0)
    return q * s[:, None, None], c, s, ok


def _f7_det3(m):
    return (m[..., 0] * (m[..., 4] * m[..., 8] - m[..., 5] * m[..., 7]) - m[..., 1] * (m[..., 3] * m[..., 8] - m[..., 5] * m[..., 6]) +
            m[..., 2] * (m[..., 3] * m[..., 7] - m[..., 4] * m[..., 6]))


def seven_point_ge(x0, x1, detail=False):
    """Fundamental matrices through 7 correspondences by elimination.  x0, x1: [N, 7, 2] in any units (x1^T F x0 = 0)
    -> (F [N, 3, 3, 3] of unit Frobenius norm, valid [N, 3]), the models ordered by their root a ascending, an unused slot zero.
    The arithmetic and the validity rules of gim_fundamental_step (include/gim_hip.h; csrc/fundamental_solve.h is the same code for
    the device), batched over the samples: each side shifted to zero mean and scaled to mean distance sqrt(2) per sample; the 7 x 9
    rows of `_epipolar_rows` reduced by Gauss-Jordan elimination with full pivoting; the two free columns give F1, F2; the cubic
    det(a F1 + (1 - a) F2) interpolated at a = 0, 1, -1, 2 as in `seven_point`, solved in closed form (Cardano for one real root, the
    trigonometric form for three) and polished by two Newton steps; F = T1^T (a F1 + (1 - a) F2) T0.  All three slots are invalid
    when the seven points of a side coincide (mean distance below 1e-12), the seventh pivot is below 1e-12 times the first (collinear
    points, a planar scene), max |c| is below 1e-12 (every matrix of the pencil is singular -- three matches that share a point on
    one side do that -- and the cubic is rounding noise), or |c3| <= 1e-14 max |c|; a slot is invalid when its model's norm is zero
    or not finite.
    detail=True adds a dict: ok_scale, ok_rank, ok_cubic, ok_lead [N] (the four rules, each True where an earlier rule already
    failed), pivot_ratio [N] (seventh pivot / first), cubic_scale [N] (max |c|), lead_ratio [N] (|c3| / max |c|), disc_rel [N]
    (discriminant / its scale, > 0: one root), roots [N, 3] -- what a test needs to see how far a sample is from a rule."""
    x0 = np.asarray(x0, dtype=np.float64)
    x1 = np.asarray(x1, dtype=np.float64)
    n = x0.shape[0]
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        q0, c0, s0, ok0 = _f7_normalise(x0)
        q1, c1, s1, ok1 = _f7_normalise(x1)
        ok_scale = ok0 & ok1
        A = _epipolar_rows(q0, q1)                                              # [N, 7, 9]
        alive = ok_scale.copy()
        rowof = np.full((n, 9), -1, dtype=np.int64)
        first = last = np.zeros(n)
        for k in range(7):
            sub = np.abs(A[:, k:, :]).reshape(n, -1)
            j = np.where(np.isnan(sub).any(1), 0, sub.argmax(1))                # argmax: the lowest row, then the lowest column
            best = sub[rows, j]
            pr, pc = j // 9 + k, j % 9
            if k == 0:
                first = best
            alive &= np.isfinite(best) & (best > 0.0)
            if k == 6:
                last = best
                alive &= best >= F7_RANK_EPS * first
            tmp = A[rows, k].copy()
            A[rows, k] = A[rows, pr]
            A[rows, pr] = tmp
            A[:, k] = A[:, k] / np.where(alive, A[rows, k, pc], 1.0)[:, None]
            f = A[rows, :, pc]                                                  # [N, 7] (a copy: fancy indexing)
            f[:, k] = 0.0
            A -= f[:, :, None] * A[:, None, k, :]
            rowof[rows, pc] = k
        ok_rank = alive | ~ok_scale
        free = np.argsort(rowof >= 0, axis=1, kind="stable")[:, :2]             # the two free columns, ascending
        f1 = np.where(alive, free[:, 0], 7)
        f2 = np.where(alive, free[:, 1], 8)
        r = np.where(rowof >= 0, rowof, 0)
        F1 = -A[rows[:, None], r, f1[:, None]]
        F2 = -A[rows[:, None], r, f2[:, None]]
        F1[rows, f1], F1[rows, f2], F2[rows, f2], F2[rows, f1] = 1.0, 0.0, 1.0, 0.0
        d0, d1, dm, d2 = _f7_det3(F2), _f7_det3(F1), _f7_det3(2.0 * F2 - F1), _f7_det3(2.0 * F1 - F2)
        k0 = d0
        k2 = (d1 + dm) * 0.5 - k0
        sum13 = (d1 - dm) * 0.5
        sum143 = ((d2 - k0) - 4.0 * k2) * 0.5
        k3 = (sum143 - sum13) / 3.0
        k1 = sum13 - k3
        cmax = np.fmax(np.fmax(np.abs(k0), np.abs(k1)), np.fmax(np.abs(k2), np.abs(k3)))
        ok_cubic = cmax >= F7_CUBIC_EPS
        ok_lead = np.abs(k3) > F7_LEAD_EPS * (cmax + 1e-300)
        alive &= ok_cubic & ok_lead
        ld = np.where(alive, k3, 1.0)
        b2, b1, b0 = k2 / ld, k1 / ld, k0 / ld
        sh = b2 / 3.0
        p = b1 - b2 * sh
        q = (2.0 * sh * sh - b1) * sh + b0
        hq, tp = 0.5 * q, p / 3.0
        D = hq * hq + tp * tp * tp
        one = D > 0.0
        alive &= one | (D <= 0.0)
        # one real root: Cardano, no cancellation under the cube root
        sD = np.sqrt(np.where(one, D, 0.0))
        u = np.where(hq >= 0.0, -np.cbrt(hq + sD), np.cbrt(sD - hq))
        v = np.where(u != 0.0, -tp / np.where(u != 0.0, u, 1.0), 0.0)
        a1 = (u + v) - sh
        # three real roots: trigonometric form
        m = np.sqrt(np.where(one, 0.0, -tp))
        w = np.clip(-hq / np.where(m > 0.0, m * m * m, 1.0), -1.0, 1.0)
        th = np.arccos(w) / 3.0
        tw = 2.0943951023931954923
        a3 = np.stack([2.0 * m * np.cos(th), 2.0 * m * np.cos(th - tw), 2.0 * m * np.cos(th - 2.0 * tw)], 1)
        a3 = np.where((m > 0.0)[:, None], a3, 0.0) - sh[:, None]
        a = np.where(one[:, None], np.stack([a1, np.zeros(n), np.zeros(n)], 1), a3)
        for _ in range(2):                                                       # Newton on a^3 + b2 a^2 + b1 a + b0
            fa = ((a + b2[:, None]) * a + b1[:, None]) * a + b0[:, None]
            ga = (3.0 * a + 2.0 * b2[:, None]) * a + b1[:, None]
            da = fa / ga
            a = np.where(np.isfinite(da), a - da, a)
        a = np.where(one[:, None], a, np.sort(a, axis=1))
        slot = alive[:, None] & (~one[:, None] | (np.arange(3) == 0))
        a = np.where(slot, a, 0.0)
        N = a[:, :, None] * F1[:, None] + (1.0 - a)[:, :, None] * F2[:, None]     # [N, 3, 9]
        N = N.reshape(n, 3, 3, 3)
        G = np.empty_like(N)
        G[..., 0] = N[..., 0] * s0[:, None, None]
        G[..., 1] = N[..., 1] * s0[:, None, None]
        G[..., 2] = N[..., 2] - s0[:, None, None] * (N[..., 0] * c0[:, None, None, 0] + N[..., 1] * c0[:, None, None, 1])
        P = np.empty_like(G)
        P[:, :, 0] = s1[:, None, None] * G[:, :, 0]
        P[:, :, 1] = s1[:, None, None] * G[:, :, 1]
        P[:, :, 2] = G[:, :, 2] - s1[:, None, None] * (c1[:, None, None, 0] * G[:, :, 0] + c1[:, None, None, 1] * G[:, :, 1])
        Pf = P.reshape(n, 3, 9)
        n2 = np.zeros((n, 3))
        for i in range(9):
            n2 = n2 + Pf[..., i] * Pf[..., i]
        nrm = np.sqrt(n2)
        valid = slot & np.isfinite(nrm) & (nrm > 0.0)
        F = np.where(valid[..., None, None], P / np.where(valid, nrm, 1.0)[..., None, None], 0.0)
    if detail:
        with np.errstate(all="ignore"):
            before = ok_scale & ok_rank
            info = dict(ok_scale=ok_scale, ok_rank=ok_rank, ok_cubic=ok_cubic | ~before, ok_lead=ok_lead | ~(before & ok_cubic),
                        pivot_ratio=last / first, cubic_scale=cmax, lead_ratio=np.abs(k3) / (cmax + 1e-300), disc_rel=D / (hq * hq + np.abs(tp * tp * tp)), roots=a)
        return F, valid, info
    return F, valid


E5_RANK_EPS = 1e-12     # smallest fifth pivot of the 5 x 9 elimination, relative to the first
E5_PIVOT_EPS = 1e-12    # smallest pivot of the 10 x 10 cubic block, relative to the largest |entry| of the 10 x 20 matrix
E5_W_EPS = 1e-14        # smallest |v[9]| relative to max |v| of a root's null vector (five_point's 1e-14)
E5_QR_EPS = 2.220446049250313e-16   # the deflation tests of the QR iteration
E5_QR_ITS = 30          # QR sweeps allowed per eigenvalue; exceptional shifts at sweeps 10 and 20
_E5_T12 = _T12.reshape(4, 4, -1).argmax(-1)          # (linear a) * (linear b) -> index in _MONO2: gim_e5_t12
_E5_T23 = _T23.reshape(len(_MONO2), 4, 20).argmax(-1)   # (_MONO2 m) * (linear b) -> index in _MONO: gim_e5_t23


def _e5_acc11(P2, sg, Bs, ca, cb):
    """P2 [N, 10] += sg * e[ca] * e[cb], the entries of E as linear polynomials (Bs [N, 4, 9]): gim_e5_acc11"""
    for a in range(4):
        for b in range(4):
            P2[:, _E5_T12[a, b]] += sg * (Bs[:, a, ca] * Bs[:, b, cb])


def _e5_acc21(row, sg, P2, Bs, c):
    """row [N, 20] += sg * P2 [N, 10] * e[c]: gim_e5_acc21"""
    for m in range(10):
        for b in range(4):
            row[:, _E5_T23[m, b]] += sg * (P2[:, m] * Bs[:, b, c])


def _e5_eigenvalues(act):
    """gim_e5_eigenvalues on one 10 x 10 matrix (nested lists of Python floats: IEEE doubles, no contraction), statement by
    statement: Householder reduction to Hessenberg form (EISPACK orthes), the real double-shift QR iteration (EISPACK hqr,
    eigenvalues only) -> (real roots ascending, smallest |discriminant| of a 2 x 2 block relative to its scale, most sweeps
    spent on one eigenvalue, all sweeps, converged)"""
    import math
    a = [list(map(float, r)) for r in act]
    ort = [0.0] * 10
    roots, disc, its_max, sweeps = [], math.inf, 0, 0
    try:
        for m in range(1, 9):
            scale = 0.0
            for i in range(m, 10):
                scale += abs(a[i][m - 1])
            if scale == 0.0:
                continue
            h = 0.0
            for i in range(9, m - 1, -1):
                ort[i] = a[i][m - 1] / scale
                h += ort[i] * ort[i]
            g = -math.copysign(math.sqrt(h), ort[m])
            h -= ort[m] * g
            ort[m] -= g
            for j in range(m, 10):
                f = 0.0
                for i in range(9, m - 1, -1):
                    f += ort[i] * a[i][j]
                f /= h
                for i in range(m, 10):
                    a[i][j] -= f * ort[i]
            for i in range(10):
                f = 0.0
                for j in range(9, m - 1, -1):
                    f += ort[j] * a[i][j]
                f /= h
                for j in range(m, 10):
                    a[i][j] -= f * ort[j]
            a[m][m - 1] = scale * g
            for i in range(m + 1, 10):
                a[i][m - 1] = 0.0
        anorm = 0.0
        for i in range(10):
            for j in range(max(i - 1, 0), 10):
                anorm += abs(a[i][j])
        if not math.isfinite(anorm):
            return [], disc, 0, 0, False
        nn, its, t = 9, 0, 0.0
        for _ in range(10 * (E5_QR_ITS + 1)):
            if nn < 0:
                break
            l = nn
            while l > 0:
                s = abs(a[l - 1][l - 1]) + abs(a[l][l])
                if s == 0.0:
                    s = anorm
                if abs(a[l][l - 1]) <= E5_QR_EPS * s:
                    a[l][l - 1] = 0.0
                    break
                l -= 1
            x = a[nn][nn]
            if l == nn:
                roots.append(x + t)
                nn, its = nn - 1, 0
                continue
            y = a[nn - 1][nn - 1]
            ww = a[nn][nn - 1] * a[nn - 1][nn]
            if l == nn - 1:
                p = 0.5 * (y - x)
                q = p * p + ww
                z = math.sqrt(abs(q))
                x += t
                den = p * p + abs(ww)
                disc = min(disc, abs(q) / den if den > 0.0 else 0.0)
                if q >= 0.0:
                    z = p + math.copysign(z, p)
                    roots.append(x + z)
                    roots.append(x - ww / z if z != 0.0 else x + z)
                nn, its = nn - 2, 0
                continue
            if its == E5_QR_ITS:
                return sorted(roots), disc, its_max, sweeps, False
            if its in (10, 20):
                t += x
                for i in range(nn + 1):
                    a[i][i] -= x
                s = abs(a[nn][nn - 1]) + abs(a[nn - 1][nn - 2])
                y = x = 0.75 * s
                ww = -0.4375 * s * s
            its += 1
            sweeps += 1
            its_max = max(its_max, its)
            p = q = r = z = 0.0
            m = nn - 2
            while m >= l:
                z = a[m][m]
                r = x - z
                s = y - z
                p = (r * s - ww) / a[m + 1][m] + a[m][m + 1]
                q = a[m + 1][m + 1] - z - r - s
                r = a[m + 2][m + 1]
                s = abs(p) + abs(q) + abs(r)
                p, q, r = p / s, q / s, r / s
                if m == l:
                    break
                u = abs(a[m][m - 1]) * (abs(q) + abs(r))
                v = abs(p) * (abs(a[m - 1][m - 1]) + abs(z) + abs(a[m + 1][m + 1]))
                if u <= E5_QR_EPS * v:
                    break
                m -= 1
            for i in range(m, nn - 1):
                a[i + 2][i] = 0.0
                if i != m:
                    a[i + 2][i - 1] = 0.0
            for k in range(m, nn):
                if k != m:
                    p = a[k][k - 1]
                    q = a[k + 1][k - 1]
                    r = a[k + 2][k - 1] if k + 1 != nn else 0.0
                    x = abs(p) + abs(q) + abs(r)
                    if x != 0.0:
                        p, q, r = p / x, q / x, r / x
                s = math.copysign(math.sqrt(p * p + q * q + r * r), p)
                if s == 0.0 or not math.isfinite(s):
                    continue
                if k == m:
                    if l != m:
                        a[k][k - 1] = -a[k][k - 1]
                else:
                    a[k][k - 1] = -s * x
                p += s
                x, y, z = p / s, q / s, r / s
                q /= p
                r /= p
                ak, ak1 = a[k], a[k + 1]
                ak2 = a[k + 2] if k + 1 != nn else None
                for j in range(k, nn + 1):
                    p = ak[j] + q * ak1[j]
                    if ak2 is not None:
                        p += r * ak2[j]
                        ak2[j] -= p * z
                    ak1[j] -= p * y
                    ak[j] -= p * x
                for i in range(l, min(nn, k + 3) + 1):
                    ai = a[i]
                    p = x * ai[k] + y * ai[k + 1]
                    if ak2 is not None:
                        p += z * ai[k + 2]
                        ai[k + 2] -= p * r
                    ai[k + 1] -= p * q
                    ai[k] -= p
        return sorted(roots), disc, its_max, sweeps, nn < 0
    except (ZeroDivisionError, ValueError, OverflowError):   # where C++ goes on with an infinity or a NaN: no further roots
        return sorted(r for r in roots if math.isfinite(r)), disc, its_max, sweeps, False


def five_point_ge(x0, x1, detail=False):
    """Essential matrices through 5 correspondences by elimination and a real QR iteration.  x0, x1: [N, 5, 2] normalised image points
    (x1^T E x0 = 0) -> (E [N, 10, 3, 3] of unit Frobenius norm, valid [N, 10]), the models ordered by their root x ascending, an
    unused or refused slot zero.  The arithmetic and the validity rules of gim_essential_step (include/gim_hip.h;
    csrc/essential_solve.h is the same code for the device), batched over the samples, with one exception: the eigenvalue
    iteration has a data-dependent course and runs sample by sample on Python floats (`_e5_eigenvalues`).
      1. the 5 x 9 rows of `_epipolar_rows`, Gauss-Jordan with full pivoting; the four free columns give X, Y, Z, W.  Refused: an
         input that is not finite, a fifth pivot below 1e-12 times the first (a repeated correspondence, coincident points);
      2. the ten cubic constraints of `five_point` over `_MONO`, accumulated term by term in the order of the header;
      3. Gauss-Jordan with partial pivoting on the cubic block -> [I | B].  Refused: a pivot below 1e-12 times the largest |entry|;
      4. the action matrix of `five_point`; Hessenberg form by Householder reflections, eigenvalues by the real double-shift QR
         iteration: at most 30 sweeps per eigenvalue, exceptional shifts at sweeps 10 and 20, a 2 x 2 block with a negative
         discriminant is a complex pair (no models), no convergence leaves the slots not yet found invalid;
      5. per real root the null vector v of Act - x I by Gauss-Jordan with full pivoting, (x, y, z) = v[6..8] / v[9], refused when
         |v[9]| <= 1e-14 max |v|; E = x X + y Y + z Z + W over its norm, refused when that is zero or not finite.
    detail=True adds a dict: ok_input, ok_rank, ok_pivot [N] (the three sample rules, each True where an earlier rule already
    failed), rank_ratio [N] (fifth pivot / first), pivot_ratio [N] (smallest pivot of step 3 / largest |entry|), disc_rel [N]
    (smallest |discriminant| of a 2 x 2 block relative to its scale; inf without such a block), gap_rel [N] (smallest gap between
    two real roots relative to 1 + |x|; inf with fewer than two), w_ratio [N] (smallest |v[9]| / max |v| over the roots; inf
    without a root), qr_its [N] (most sweeps spent on one eigenvalue), qr_sweeps [N] (all sweeps), qr_ok [N] (the iteration
    converged), nroots [N], roots [N, 10] (NaN in an unused slot) -- what a test needs to see how far a sample is from a rule."""
    x0 = np.asarray(x0, dtype=np.float64)
    x1 = np.asarray(x1, dtype=np.float64)
    n = x0.shape[0]
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        ok_input = np.isfinite(x0).all((1, 2)) & np.isfinite(x1).all((1, 2))
        A = _epipolar_rows(x0, x1)                                              # [N, 5, 9]
        alive = ok_input.copy()
        rowof = np.full((n, 9), -1, dtype=np.int64)
        first = last = np.zeros(n)
        for k in range(5):
            sub = np.abs(A[:, k:, :]).reshape(n, -1)
            j = np.where(np.isnan(sub).any(1), 0, sub.argmax(1))                # argmax: the lowest row, then the lowest column
            best = sub[rows, j]
            pr, pc = j // 9 + k, j % 9
            if k == 0:
                first = best
            alive &= np.isfinite(best) & (best > 0.0)
            if k == 4:
                last = best
                alive &= best >= E5_RANK_EPS * first
            tmp = A[rows, k].copy()
            A[rows, k] = A[rows, pr]
            A[rows, pr] = tmp
            A[:, k] = A[:, k] / np.where(alive, A[rows, k, pc], 1.0)[:, None]
            f = A[rows, :, pc]
            f[:, k] = 0.0
            A -= f[:, :, None] * A[:, None, k, :]
            rowof[rows, pc] = k
        ok_rank = alive | ~ok_input
        free = np.argsort(rowof >= 0, axis=1, kind="stable")[:, :4]             # the four free columns, ascending
        r = np.where(rowof >= 0, rowof, 0)
        Bs = np.empty((n, 4, 9))
        for k in range(4):
            fk = free[:, k]
            Bs[:, k] = np.where(rowof >= 0, -A[rows[:, None], r, fk[:, None]], 0.0)
            Bs[rows, k, fk] = 1.0
        Bs = np.where(alive[:, None, None], Bs, 0.0)
        # the constraints
        EEt = np.zeros((6, n, 10))
        sym = lambda i, j: 3 * min(i, j) - (min(i, j) * (min(i, j) - 1)) // 2 + abs(j - i)   # noqa: E731
        for i in range(3):
            for j in range(i, 3):
                for k in range(3):
                    _e5_acc11(EEt[sym(i, j)], 1.0, Bs, 3 * i + k, 3 * j + k)
        tr = (EEt[0] + EEt[3]) + EEt[5]
        M = np.zeros((n, 10, 20))
        for sg, (c1, c2, c3, c4), c in ((1.0, (4, 8, 5, 7), 0), (-1.0, (3, 8, 5, 6), 1), (1.0, (3, 7, 4, 6), 2)):
            tmp = np.zeros((n, 10))
            _e5_acc11(tmp, 1.0, Bs, c1, c2)
            _e5_acc11(tmp, -1.0, Bs, c3, c4)
            _e5_acc21(M[:, 0], sg, tmp, Bs, c)
        for i in range(3):
            for j in range(3):
                row = M[:, 1 + 3 * i + j]
                for k in range(3):
                    _e5_acc21(row, 1.0, EEt[sym(i, k)], Bs, 3 * k + j)
                row *= 2.0
                _e5_acc21(row, -1.0, tr, Bs, 3 * i + j)
        # [I | B]
        mmax = np.abs(M).reshape(n, -1).max(1)
        alive &= np.isfinite(M).all((1, 2)) & (mmax > 0.0)
        minpiv = np.full(n, np.inf)
        for k in range(10):
            col = np.abs(M[:, k:, k])
            pr = np.where(np.isnan(col).any(1), 0, col.argmax(1)) + k
            best = col[rows, pr - k]
            minpiv = np.fmin(minpiv, np.where(alive, best, np.inf))
            alive &= np.isfinite(best) & (best >= E5_PIVOT_EPS * mmax)
            tmp = M[rows, k, k:].copy()
            M[rows, k, k:] = M[rows, pr, k:]
            M[rows, pr, k:] = tmp
            M[:, k, k:] = M[:, k, k:] / np.where(alive, M[:, k, k], 1.0)[:, None]
            f = M[:, :, k].copy()
            f[:, k] = 0.0
            M[:, :, k:] -= f[:, :, None] * M[:, None, k, k:]
        ok_pivot = alive | ~(ok_input & ok_rank)
        Act = np.zeros((n, 10, 10))
        Act[:, :6] = -M[:, :6, 10:]
        Act[:, 6, 0] = Act[:, 7, 1] = Act[:, 8, 2] = Act[:, 9, 6] = 1.0
        Act = np.where(alive[:, None, None], Act, 0.0)
        # the eigenvalues, sample by sample
        lam = np.full((n, 10), np.nan)
        nroots = np.zeros(n, dtype=np.int64)
        disc_rel, gap_rel = np.full(n, np.inf), np.full(n, np.inf)
        qr_its, qr_sweeps, qr_ok = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool)
        for s in np.flatnonzero(alive):
            rts, disc_rel[s], qr_its[s], qr_sweeps[s], qr_ok[s] = _e5_eigenvalues(Act[s].tolist())
            nroots[s] = len(rts)
            lam[s, :len(rts)] = rts
            if len(rts) > 1:
                rt = np.array(rts)
                gap_rel[s] = (np.diff(rt) / (1.0 + np.abs(rt[:-1]))).min()
        slot = np.arange(10)[None] < nroots[:, None]
        # one system per root
        S = np.broadcast_to(Act[:, None], (n, 10, 10, 10)).copy()
        d = np.arange(10)
        S[:, :, d, d] -= np.where(slot, lam, 0.0)[..., None]
        NS = n * 10
        S = S.reshape(NS, 10, 10)
        srow = np.arange(NS)
        sl = slot.reshape(NS).copy()
        rof = np.full((NS, 10), -1, dtype=np.int64)
        for k in range(9):
            sub = np.abs(S[:, k:, :]).reshape(NS, -1)
            j = np.where(np.isnan(sub).any(1), 0, sub.argmax(1))
            best = sub[srow, j]
            pr, pc = j // 10 + k, j % 10
            sl &= np.isfinite(best) & (best > 0.0)
            tmp = S[srow, k].copy()
            S[srow, k] = S[srow, pr]
            S[srow, pr] = tmp
            S[:, k] = S[:, k] / np.where(sl, S[srow, k, pc], 1.0)[:, None]
            f = S[srow, :, pc]
            f[:, k] = 0.0
            S -= f[:, :, None] * S[:, None, k, :]
            rof[srow, pc] = k
        fc = 9 - np.argmax((rof < 0)[:, ::-1], axis=1)                          # the free column (the last one, as the header takes it)
        v = -S[srow[:, None], np.where(rof >= 0, rof, 0), fc[:, None]]
        v[srow, fc] = 1.0
        vmax = np.abs(v).max(1)
        sl &= np.isfinite(vmax) & (np.abs(v[:, 9]) > E5_W_EPS * vmax)
        w9 = np.where(sl, v[:, 9], 1.0)
        x, y, z = (v[:, 6] / w9).reshape(n, 10, 1), (v[:, 7] / w9).reshape(n, 10, 1), (v[:, 8] / w9).reshape(n, 10, 1)
        Em = ((x * Bs[:, None, 0] + y * Bs[:, None, 1]) + z * Bs[:, None, 2]) + Bs[:, None, 3]   # [N, 10, 9]
        n2 = np.zeros((n, 10))
        for i in range(9):
            n2 = n2 + Em[..., i] * Em[..., i]
        nrm = np.sqrt(n2)
        valid = sl.reshape(n, 10) & np.isfinite(nrm) & (nrm > 0.0)
        E = np.where(valid[..., None], Em / np.where(valid, nrm, 1.0)[..., None], 0.0).reshape(n, 10, 3, 3)
    if detail:
        with np.errstate(all="ignore"):
            wr = np.where(slot, (np.abs(v[:, 9]) / vmax).reshape(n, 10), np.inf)
            info = dict(ok_input=ok_input, ok_rank=ok_rank, ok_pivot=ok_pivot, rank_ratio=last / first, pivot_ratio=minpiv / mmax,
                        disc_rel=disc_rel, gap_rel=gap_rel, w_ratio=np.where(np.isnan(wr), 0.0, wr).min(1), qr_its=qr_its,
                        qr_sweeps=qr_sweeps, qr_ok=qr_ok, nroots=nroots, roots=lam)
        return E, valid, info
    return E, valid


def sampson_error(M, x0, x1):
    """(x1^T M x0)^2 / (|M x0|_xy^2 + |M^T x1|_xy^2) for models M [..., 3, 3] and points [P, 2] -> [..., P]
    (EMEstimatorCallback::computeError / FMEstimatorCallback::computeError)"""
    o = np.ones((x0.shape[0], 1))
    h0t = np.concatenate([x0, o], 1).T                                      # [3, P]
    h1t = np.concatenate([x1, o], 1).T
    Mx0 = M @ h0t                                                           # [..., 3, P]
    Mtx1 = np.swapaxes(M, -1, -2) @ h1t
    num = (Mx0 * h1t).sum(-2) ** 2
    den = Mx0[..., 0, :] ** 2 + Mx0[..., 1, :] ** 2 + Mtx1[..., 0, :] ** 2 + Mtx1[..., 1, :] ** 2
    return num / np.maximum(den, 1e-300)


def _count_inliers(Ms, valid, x0, x1, thr2, chunk=128, error=None):
    """inlier counts of the models Ms [K, 3, 3] over all points, in chunks whose temporaries stay cache-resident"""
    error = sampson_error if error is None else error
    out = np.zeros(Ms.shape[0], dtype=np.int64)
    for c0 in range(0, Ms.shape[0], chunk):
        out[c0:c0 + chunk] = (error(Ms[c0:c0 + chunk], x0, x1) <= thr2).sum(1)
    return np.where(valid, out, 0)


# ---- counter-based sampling and the per-step reduction (csrc/ransac_sample.h, csrc/ransac_records.hip restated) -----------------
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_U32, _SH32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): counter [..., 4] and key [..., 2] of 32-bit words (broadcast against each
    other) -> uint32 [..., 4].  uint64 products, the high and low halves taken by shift and mask."""
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> _SH32) ^ c1 ^ k0, p1 & _U32, (p0 >> _SH32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _PHILOX_W0) & _U32, (k1 + _PHILOX_W1) & _U32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def _check_seed64(seed):
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed={seed}: the philox / device samplers take a seed of 64 unsigned bits")
    return seed


def device_samples(seed, first, n, P, m):
    """The samples number first .. first + n - 1 of the run `seed` over P points, m in (4, 5, 7) indices each -> int32 [n, m]: what
    gim_ransac_sample writes (csrc/ransac_sample.h), in numpy.  Sample number N (the 0-based ordinal over the whole run, modulo
    2^64) depends on (seed, N, P, m) alone: r[0..7] = philox4x32((N & 0xffffffff, N >> 32, blk, 0), (seed & 0xffffffff, seed >> 32))
    for blk = 0, 1; Floyd's algorithm with exactly m draws: j = P - m + i, t = (r[i] * (j + 1)) >> 32, out[i] = t unless t is
    among out[:i], then j.  Distinct indices of [0, P); the set is uniform over the m-subsets up to the multiply-shift bias (a value
    of [0, j] is off by at most (j + 1) / 2^32 relative: 5e-7 at P = 2 000); the order inside a sample is not uniform.
    P < m: every index is -1."""
    seed, n, P, m = _check_seed64(seed), int(n), int(P), int(m)
    if m not in (4, 5, 7):
        raise ValueError(f"m={m}: 4, 5 or 7")
    if not 0 <= P < 1 << 31 or n < 0:
        raise ValueError(f"P={P}, n={n}: 0 <= P < 2^31, n >= 0")
    if P < m:
        return np.full((n, m), -1, dtype=np.int32)
    with np.errstate(over="ignore"):
        N = np.uint64(int(first) & ((1 << 64) - 1)) + np.arange(n, dtype=np.uint64)          # wraps modulo 2^64
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = N & _U32, N >> _SH32
    r = [philox4x32(ctr, key)]
    if m > 4:
        ctr[:, 2] = 1
        r.append(philox4x32(ctr, key))
    r = np.concatenate(r, 1).astype(np.uint64)
    out = np.empty((n, m), dtype=np.int64)
    for i in range(m):
        j = P - m + i
        t = ((r[:, i] * np.uint64(j + 1)) >> _SH32).astype(np.int64)
        out[:, i] = np.where((out[:, :i] == t[:, None]).any(1), j, t)
    return out.astype(np.int32)


def step_records(counts, nb, floor):
    """The samples of a step that set a new strict maximum -- what gim_ransac_records writes (csrc/ransac_records.hip), in numpy.
    counts int [B, K, k], nb [B] (samples in use, clamped to [0, K]), floor [B] (the count to beat: max(best so far, m - 1)) ->
    int32 [B, 1 + 3 K]: n_rec, then the triples (s, j_s, c_s) in ascending s with c_s = counts[b, s].max(), j_s = its argmax (the
    lowest slot) and c_s > max(floor[b], c_0 .. c_{s-1}); zeros beyond the last triple (the device leaves those words unwritten)."""
    counts = np.asarray(counts)
    B, K, _ = counts.shape
    out = np.zeros((B, 1 + 3 * K), dtype=np.int32)
    for b in range(B):
        n = min(max(int(nb[b]), 0), K)
        c, j = counts[b, :n].max(1), counts[b, :n].argmax(1)
        before = np.maximum.accumulate(np.concatenate([[int(floor[b])], c]))[:n]
        s = np.flatnonzero(c > before)
        out[b, 0] = len(s)
        out[b, 1:1 + 3 * len(s)] = np.stack([s, j[s], c[s]], 1).reshape(-1)
    return out


# ---- MAGSAC++ scoring (csrc/magsac_loss.h, csrc/ransac_score.hip restated) -----------------------------------------------------------------
MAGSAC_K = 3.64                                  # the 0.99 quantile of chi(4): OpenCV's two-view USAC constant
MAGSAC_UK = 3.64 * 3.64 / 2.0                    # u = r^2 / (2 sigma^2) at r = k sigma
MAGSAC_GK = 0.0036572608340910747                # Gamma(3/2, u_k), upper incomplete gamma
MAGSAC_LK = 1.3012265540498873                   # gamma(5/2, u_k), lower incomplete gamma
MAGSAC_UNITS = 4294967296.0                      # 2^32 quantisation units per point
_MAGSAC_C_ERF, _MAGSAC_C_ERFC = 1.3293403881791370, 0.88622692545275801      # 3 sqrt(pi) / 4, sqrt(pi) / 2


def _erf_erfc(t):
    try:
        from scipy.special import erf, erfc
        return erf(t), erfc(t)
    except ImportError:                          # the C library's, one value at a time
        import math
        return np.frompyfunc(math.erf, 1, 1)(t).astype(np.float64), np.frompyfunc(math.erfc, 1, 1)(t).astype(np.float64)


def magsac_n(u):
    """N(u) = gamma(5/2, u) + u (Gamma(3/2, u) - G_k) in closed form: (3 sqrt(pi)/4) erf(t) - 1.5 t exp(-u) + (sqrt(pi)/2) u erfc(t)
    - u G_k with t = sqrt(u); u >= 0, any shape"""
    u = np.asarray(u, dtype=np.float64)
    t = np.sqrt(u)
    ef, efc = _erf_erfc(t)
    return _MAGSAC_C_ERF * ef - 1.5 * t * np.exp(-u) + _MAGSAC_C_ERFC * u * efc - u * MAGSAC_GK


def magsac_gain(u):
    """The MAGSAC++ gain of a point with u = r^2 / (2 sigma^2), sigma = max_threshold / 3.64 (include/gim_hip.h, gim_magsac_score;
    gim_ms_gain of csrc/magsac_loss.h in numpy): 1 - N(u) / g_k clamped to [0, 1] for 0 <= u < u_k, 0 otherwise (beyond k sigma,
    negative, NaN, infinite).  1 at 0, 0 at u_k, continuous and non-increasing."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(all="ignore"):
        inside = (u >= 0.0) & (u < MAGSAC_UK)
        g = 1.0 - magsac_n(np.where(inside, u, 0.0)) / MAGSAC_LK
        return np.where(inside, np.clip(g, 0.0, 1.0), 0.0)


def magsac_units(r2, max_thr2):
    """q = llrint(gain * 2^32) of squared residuals r2 under the band max_thr2 = max_threshold^2 -> int64 of [0, 2^32]"""
    with np.errstate(all="ignore"):
        u = np.asarray(r2, dtype=np.float64) / (float(max_thr2) / MAGSAC_UK)
    return np.rint(magsac_gain(u) * MAGSAC_UNITS).astype(np.int64)


def magsac_quality(kind, Ms, valid, a, b, thr2, max_thr2, chunk=128):
    """What gim_magsac_score writes for one pair, in numpy: models Ms [K, 3, 3], valid [K] or None, points a, b [P, 2]; kind 1 the
    Sampson error (`sampson_error`), kind 0 the forward transfer error b ~ M a (`transfer_error`) -> (quality int64 [K]: the sum of
    `magsac_units` over the points, counts int64 [K]: the points with error <= thr2).  A model with valid == 0 or with an entry that
    is not finite: 0 and 0; a point with a NaN coordinate adds nothing to either."""
    if kind not in (0, 1):
        raise ValueError(f"kind={kind!r}: 0 (homography) or 1 (fundamental matrix)")
    max_thr2 = float(max_thr2)
    if not (np.isfinite(max_thr2) and max_thr2 > 0.0):
        raise ValueError(f"max_thr2={max_thr2}: finite and positive")
    Ms = np.asarray(Ms, dtype=np.float64).reshape(-1, 3, 3)
    a = np.asarray(a, dtype=np.float64).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 2)
    K = Ms.shape[0]
    ok = np.isfinite(Ms).all((1, 2)) & (np.ones(K, dtype=bool) if valid is None else np.asarray(valid).reshape(-1) != 0)
    error = transfer_error if kind == 0 else sampson_error
    q, c = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    for c0 in range(0, K, chunk):
        with np.errstate(all="ignore"):
            r2 = error(np.where(ok[c0:c0 + chunk, None, None], Ms[c0:c0 + chunk], 0.0), a, b)
            c[c0:c0 + chunk] = (r2 <= thr2).sum(1)
            q[c0:c0 + chunk] = magsac_units(r2, max_thr2).sum(1)
    return np.where(ok, q, 0), np.where(ok, c, 0)


def step_records64(quality, counts, nb, floor_q, min_count):
    """What gim_ransac_records64 writes (csrc/ransac_records.hip), in numpy.  quality int64 [B, K, k], counts int [B, K, k], nb [B],
    floor_q int64 [B], min_count: a slot is eligible iff its count is at least min_count, an ineligible slot has key 0 -> int64
    [B, 1 + 4 K]: n_rec, then (s, j_s, c_s, Q_s) in ascending s with Q_s the largest key of the sample, j_s the lowest slot that
    holds it, c_s that slot's count, and Q_s > max(floor_q[b], Q_0 .. Q_{s-1}); zeros beyond the last record (the device leaves
    those words unwritten)."""
    quality, counts = np.asarray(quality, dtype=np.int64), np.asarray(counts)
    B, K, _ = quality.shape
    out = np.zeros((B, 1 + 4 * K), dtype=np.int64)
    for b in range(B):
        n = min(max(int(nb[b]), 0), K)
        key = np.where(counts[b, :n] >= min_count, quality[b, :n], 0)
        Q, j = key.max(1), key.argmax(1)
        before = np.maximum.accumulate(np.concatenate([[int(floor_q[b])], Q]))[:n]
        s = np.flatnonzero(Q > before)
        out[b, 0] = len(s)
        out[b, 1:1 + 4 * len(s)] = np.stack([s, j[s], counts[b, s, j[s]], Q[s]], 1).reshape(-1)
    return out


# ---- homography: four-point minimal solver, transfer error, DLT re-fit, RANSAC (demo.py:180-227 cv2.findHomography) ------------
H4_PIVOT_EPS = 1e-12     # smallest pivot of the normalised 8 x 8 system
H4_AREA_EPS = 1e-9       # smallest doubled triangle area in normalised coordinates
_H4_TRI = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))   # the triples of HomographyEstimatorCallback::checkSubset


def _h4_normalise(p):
    """[N, 4, 2] -> (q [N, 4, 2] with zero mean and mean distance sqrt(2), centre [N, 2], scale [N], ok [N]); q = (p - c) * s"""
    c = (((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]) * 0.25
    q = p - c[:, None]
    d = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1])
    md = (((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]) * 0.25
    ok = np.isfinite(md) & (md > 0.0)
    s = np.sqrt(2.0) / np.where(ok, md, 1.0)
    return q * s[:, None, None], c, s, ok


def _h4_area2(q, i, j, k):
    return (q[:, j, 0] - q[:, i, 0]) * (q[:, k, 1] - q[:, i, 1]) - (q[:, j, 1] - q[:, i, 1]) * (q[:, k, 0] - q[:, i, 0])


def homography_4pt(x_src, x_dst, detail=False):
    """Homographies through 4 correspondences, x_dst ~ H x_src.  x_src, x_dst: [N, 4, 2] -> (H [N, 1, 3, 3], valid [N, 1]).
    The arithmetic and the validity rules of gim_homography_step (include/gim_hip.h; csrc/homography_solve.h is the same code for
    the device), batched over the samples: each side shifted to zero mean and scaled to mean distance sqrt(2); the 8 x 9 augmented
    system of the eight equations with h33 = 1 reduced by Gaussian elimination with partial pivoting; H de-normalised and scaled to
    h33 = 1.  valid = 0 (and a zero model) when the four points of a side coincide, three points of a side are collinear (doubled
    area below 1e-9 in normalised coordinates -- a repeated point is such a triple), the orientation test of
    HomographyEstimatorCallback::checkSubset (fundam.cpp) fails, a pivot is below 1e-12, or the result is not finite.
    detail=True adds a dict: min_area [N] (smallest |doubled area| over both sides), min_pivot [N] (smallest pivot reached),
    orient_ok [N], and the normalisations (qs, qd, cs, cd, ss, sd) -- what a test needs to see how far a sample is from a rule."""
    x_src = np.asarray(x_src, dtype=np.float64)
    x_dst = np.asarray(x_dst, dtype=np.float64)
    n = x_src.shape[0]
    with np.errstate(all="ignore"):
        qs, cs, ss, ok_s = _h4_normalise(x_src)
        qd, cd, sd, ok_d = _h4_normalise(x_dst)
        valid = ok_s & ok_d
        min_area = np.full(n, np.inf)
        negative = np.zeros(n, dtype=np.int64)
        for i, j, k in _H4_TRI:
            a_s, a_d = _h4_area2(qs, i, j, k), _h4_area2(qd, i, j, k)
            min_area = np.fmin(min_area, np.fmin(np.abs(a_s), np.abs(a_d)))
            valid &= (np.abs(a_s) >= H4_AREA_EPS) & (np.abs(a_d) >= H4_AREA_EPS)
            negative += (a_s < 0.0) != (a_d < 0.0)
        orient_ok = (negative == 0) | (negative == 4)
        valid &= orient_ok
        x, y, u, v = qs[..., 0], qs[..., 1], qd[..., 0], qd[..., 1]                    # [N, 4]
        o, z = np.ones_like(x), np.zeros_like(x)
        A = np.empty((n, 8, 9))
        A[:, 0::2] = np.stack([x, y, o, z, z, z, -u * x, -u * y, u], -1)
        A[:, 1::2] = np.stack([z, z, z, x, y, o, -v * x, -v * y, v], -1)
        rows = np.arange(n)
        min_pivot = np.full(n, np.inf)
        for k in range(8):
            col = np.abs(A[:, k:, k])
            piv = np.where(np.isnan(col).any(1), 0, col.argmax(1)) + k            # argmax: the first row of the largest magnitude
            best = col[rows, piv - k]
            min_pivot = np.fmin(min_pivot, np.where(valid, best, np.inf))
            valid &= best >= H4_PIVOT_EPS
            tmp = A[rows, k].copy()
            A[rows, k] = A[rows, piv]
            A[rows, piv] = tmp
            dk = np.where(valid, A[:, k, k], 1.0)
            f = A[:, k + 1:, k] / dk[:, None]
            A[:, k + 1:, k + 1:] -= f[:, :, None] * A[:, None, k, k + 1:]
        h = np.ones((n, 9))
        for k in range(7, -1, -1):
            acc = A[:, k, 8].copy()
            for c in range(k + 1, 8):
                acc -= A[:, k, c] * h[:, c]
            h[:, k] = acc / np.where(valid, A[:, k, k], 1.0)
        h = h.reshape(n, 3, 3)
        # H = Td^-1 Hn Ts, Ts = [ss 0 -ss cs.x; 0 ss -ss cs.y; 0 0 1], Td^-1 = [1/sd 0 cd.x; 0 1/sd cd.y; 0 0 1]
        g = np.empty((n, 3, 3))
        g[:, :, 0] = h[:, :, 0] * ss[:, None]
        g[:, :, 1] = h[:, :, 1] * ss[:, None]
        g[:, :, 2] = h[:, :, 2] - ss[:, None] * (h[:, :, 0] * cs[:, None, 0] + h[:, :, 1] * cs[:, None, 1])
        isd = 1.0 / sd
        H = np.empty((n, 3, 3))
        H[:, 0] = g[:, 0] * isd[:, None] + cd[:, None, 0] * g[:, 2]
        H[:, 1] = g[:, 1] * isd[:, None] + cd[:, None, 1] * g[:, 2]
        H[:, 2] = g[:, 2]
        H = H / H[:, 2:, 2:]
        valid &= np.isfinite(H).all((1, 2))
        H[:, 2, 2] = 1.0
    H = np.where(valid[:, None, None], H, 0.0)[:, None]
    if detail:
        return H, valid[:, None], dict(min_area=min_area, min_pivot=min_pivot, orient_ok=orient_ok, qs=qs, qd=qd, cs=cs, cd=cd, ss=ss, sd=sd)
    return H, valid[:, None]


def transfer_error(H, src, dst):
    """|dst - proj(H src)|^2 for models H [..., 3, 3] and points [P, 2] -> [..., P]: the forward transfer error of
    HomographyEstimatorCallback::computeError (fp64, IEEE division).  inf where w = h31 x + h32 y + h33 is 0 or the error is not
    finite, so that such a point fails every `<= thr2`."""
    H = np.asarray(H, dtype=np.float64)
    ht = np.concatenate([src, np.ones((src.shape[0], 1))], 1).T                     # [3, P]
    q = H @ ht                                                                      # [..., 3, P]
    w = q[..., 2, :]
    with np.errstate(all="ignore"):
        e = (dst[:, 0] - q[..., 0, :] / w) ** 2 + (dst[:, 1] - q[..., 1, :] / w) ** 2
    return np.where((w != 0.0) & np.isfinite(e), e, np.inf)


def homography_dlt(src, dst):
    """Normalised DLT over n >= 4 correspondences, dst ~ H src: Hartley scaling of both sides, the right singular vector of the
    smallest singular value of the 2n x 9 system, de-normalised and scaled to h33 = 1.  Runs on the host, once per call (the re-fit
    on the final inliers).  -> H [3, 3], or None for fewer than 4 points or a degenerate set."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 2)
    dst = np.asarray(dst, dtype=np.float64).reshape(-1, 2)
    if src.shape[0] < 4:
        return None

    def norm_T(p):
        c = p.mean(0)
        md = np.sqrt(((p - c) ** 2).sum(1)).mean()
        s = np.sqrt(2.0) / md if md > 0 else 0.0
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])

    Ts, Td = norm_T(src), norm_T(dst)
    if Ts[0, 0] == 0.0 or Td[0, 0] == 0.0 or not (np.isfinite(Ts).all() and np.isfinite(Td).all()):
        return None
    a = src * Ts[0, 0] + Ts[:2, 2]
    b = dst * Td[0, 0] + Td[:2, 2]
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    o, z = np.ones_like(x), np.zeros_like(x)
    A = np.concatenate([np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], 1), np.stack([z, z, z, x, y, o, -v * x, -v * y, -v], 1)])
    _, _, vt = np.linalg.svd(A)
    H = np.linalg.inv(Td) @ vt[-1].reshape(3, 3) @ Ts
    with np.errstate(all="ignore"):
        H = H / H[2, 2]
    return H if np.isfinite(H).all() else None


def decompose_essential(E):
    """cv::decomposeEssentialMat -> (R1, R2, t)"""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2].copy()


def _triangulate(P0, P1, x0, x1):
    """DLT triangulation (cv::triangulatePoints) -> homogeneous points [P, 4]"""
    A = np.stack([x0[:, 0, None] * P0[2] - P0[0], x0[:, 1, None] * P0[2] - P0[1],
                  x1[:, 0, None] * P1[2] - P1[0], x1[:, 1, None] * P1[2] - P1[1]], 1)      # [P, 4, 4]
    _, _, vt = np.linalg.svd(A)
    return vt[:, -1, :]


def recover_pose_host(E, x0, x1, distance_thresh=1e9, mask=None):
    """the host half of pose.recover_pose: cv2.recoverPose(E, x0, x1, eye(3), distanceThresh, mask=mask) with LAPACK's SVDs"""
    x0 = np.asarray(x0, dtype=np.float64)
    x1 = np.asarray(x1, dtype=np.float64)
    m_in = np.ones(x0.shape[0], dtype=bool) if mask is None else np.asarray(mask).ravel() > 0
    R1, R2, t = decompose_essential(np.asarray(E, dtype=np.float64))
    P0 = np.eye(3, 4)
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    goods = []
    for R, tt in cands:
        P1 = np.concatenate([R, tt[:, None]], 1)
        Q = _triangulate(P0, P1, x0, x1)
        w = np.where(np.abs(Q[:, 3]) > 1e-300, Q[:, 3], 1e-300)
        X = Q[:, :3] / w[:, None]
        z0 = X[:, 2]
        z1 = (X @ R.T + tt)[:, 2]
        goods.append(m_in & (z0 > 0) & (z0 < distance_thresh) & (z1 > 0) & (z1 < distance_thresh))
    n = [int(g.sum()) for g in goods]
    k = 0 if (n[0] >= n[1] and n[0] >= n[2] and n[0] >= n[3]) else 1 if (n[1] >= n[2] and n[1] >= n[3]) else 2 if n[2] >= n[3] else 3
    R, tt = cands[k]
    return n[k], R, tt, goods[k]


# ---- recoverPose as the device computes it (csrc/recover_pose_solve.h) -----------------------------------------------------------
RP_SWEEPS3 = 8           # cyclic Jacobi sweeps over E^T E
RP_SWEEPS4 = 8           # cyclic Jacobi sweeps over A^T A of a point
RP_W_TINY = 1e-300       # recover_pose's clamp of the homogeneous coordinate


def _rp_jacobi(a, sweeps):
    """gim_rp_jacobi3 / gim_rp_jacobi4 on a stack of symmetric matrices a [..., N, N] (only the upper triangle is read; it is changed
    in place) -> (diagonal [..., N], eigenvectors as columns [..., N, N])"""
    N = a.shape[-1]
    v = np.broadcast_to(np.eye(N), a.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(N):
                for q in range(p + 1, N):
                    apq = a[..., p, q].copy()
                    go = apq != 0.0
                    theta = (a[..., q, q] - a[..., p, p]) / (2.0 * np.where(go, apq, 1.0))
                    t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    t = np.where(go, t, 0.0)             # a skipped rotation is the identity: c = 1, s = tau = 0
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    tau = s / (1.0 + c)
                    a[..., p, p] -= t * apq
                    a[..., q, q] += t * apq
                    a[..., p, q] = np.where(go, 0.0, apq)
                    for r in range(N):
                        if r in (p, q):
                            continue
                        ip, iq = ((r, p) if r < p else (p, r)), ((r, q) if r < q else (q, r))
                        g, h = a[(..., *ip)].copy(), a[(..., *iq)].copy()
                        a[(..., *ip)] = np.where(go, g - s * (h + tau * g), g)
                        a[(..., *iq)] = np.where(go, h + s * (g - tau * h), h)
                    g, h = v[..., p].copy(), v[..., q].copy()
                    v[..., p] = np.where(go[..., None], g - s[..., None] * (h + tau[..., None] * g), g)
                    v[..., q] = np.where(go[..., None], h + s[..., None] * (g - tau[..., None] * h), h)
    return np.stack([a[..., i, i] for i in range(N)], -1), v


def _rp_dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def decompose_essential_ge(E):
    """gim_rp_decompose in numpy -> the four candidates [(R, t)] in the order of `recover_pose`, or None for an E with an entry
    that is not finite or all zero.  cv::decomposeEssentialMat with a fixed-sweep Jacobi SVD: det U = det V = +1 by construction."""
    E = np.asarray(E, dtype=np.float64).reshape(3, 3)
    big = np.abs(E).max() if np.isfinite(E).all() else 0.0
    if not big > 0.0:
        return None
    e = E / big
    a = np.array([[(e[0, i] * e[0, j] + e[1, i] * e[1, j]) + e[2, i] * e[2, j] for j in range(3)] for i in range(3)])
    d, v = _rp_jacobi(a, RP_SWEEPS3)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        if d[j] > d[i]:
            d[[i, j]] = d[[j, i]]
            v[:, [i, j]] = v[:, [j, i]]
    v0, v1 = v[:, 0].copy(), v[:, 1].copy()
    v0 = v0 / np.sqrt(_rp_dot3(v0, v0))
    v1 = v1 - _rp_dot3(v0, v1) * v0
    v1 = v1 / np.sqrt(_rp_dot3(v1, v1))
    cross = lambda p, q: np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])   # noqa: E731
    v2 = cross(v0, v1)
    u0 = np.array([_rp_dot3(e[i], v0) for i in range(3)])
    u1 = np.array([_rp_dot3(e[i], v1) for i in range(3)])
    u0 = u0 / np.sqrt(_rp_dot3(u0, u0))
    u1 = u1 - _rp_dot3(u0, u1) * u0
    n = np.sqrt(_rp_dot3(u1, u1))
    if not n > 1e-150:                   # rank one
        u1 = cross(u0, np.eye(3)[int(np.argmin(np.abs(u0)))])
        n = np.sqrt(_rp_dot3(u1, u1))
    u1 = u1 / n
    u2 = cross(u0, u1)
    R1 = np.array([[(u0[i] * v1[j] - u1[i] * v0[j]) + u2[i] * v2[j] for j in range(3)] for i in range(3)])
    R2 = np.array([[(u1[i] * v0[j] - u0[i] * v1[j]) + u2[i] * v2[j] for j in range(3)] for i in range(3)])
    return [(R1, u2), (R2, u2), (R1, -u2), (R2, -u2)]


def recover_pose_ge(E, x0, x1, distance_thresh=1e9, mask=None, detail=False):
    """`recover_pose` in the arithmetic of gim_recover_pose (include/gim_hip.h; csrc/recover_pose_solve.h is the code), vectorised
    over the points -- the CPU oracle of ops.recover_pose: Jacobi iterations with fixed sweep counts in place of LAPACK's SVDs, a
    point's null vector as the smallest eigenvector of A^T A.  -> (n_good, R, t, mask_out) as `recover_pose`; detail=True adds
    (counts int [4], best): the good points of each candidate in the device's candidate order and the winner's index.  An invalid
    E: (0, zero R, zero t, all-False) and best = -1."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 2)
    x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 2)
    P = x0.shape[0]
    m_in = np.ones(P, dtype=bool) if mask is None else np.asarray(mask).ravel() > 0
    cands = decompose_essential_ge(E)
    if cands is None:
        out = (0, np.zeros((3, 3)), np.zeros(3), np.zeros(P, dtype=bool))
        return out + (np.zeros(4, dtype=np.int64), -1) if detail else out
    goods = []
    x, y, u, w1 = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    zero, one = np.zeros(P), np.ones(P)
    for R, tt in cands:
        c = np.concatenate([R.ravel(), tt])
        A = np.stack([np.stack([-one, zero, x, zero], -1), np.stack([zero, -one, y, zero], -1),
                      np.stack([u * c[6] - c[0], u * c[7] - c[1], u * c[8] - c[2], u * c[11] - c[9]], -1),
                      np.stack([w1 * c[6] - c[3], w1 * c[7] - c[4], w1 * c[8] - c[5], w1 * c[11] - c[10]], -1)], 1)   # [P, 4, 4]
        a = np.zeros((P, 4, 4))
        for i in range(4):
            for j in range(i, 4):
                a[:, i, j] = ((A[:, 0, i] * A[:, 0, j] + A[:, 1, i] * A[:, 1, j]) + A[:, 2, i] * A[:, 2, j]) + A[:, 3, i] * A[:, 3, j]
        d, v = _rp_jacobi(a, RP_SWEEPS4)
        k = np.argmin(d, -1) if P else np.zeros(0, dtype=np.int64)         # the first smallest, as the device's strict <
        Q = np.take_along_axis(v, k[:, None, None], 2)[:, :, 0]
        with np.errstate(all="ignore"):
            w = np.where(np.abs(Q[:, 3]) > RP_W_TINY, Q[:, 3], RP_W_TINY)
            X = Q[:, :3] / w[:, None]
            z0 = X[:, 2]
            z1 = ((X[:, 0] * c[6] + X[:, 1] * c[7]) + X[:, 2] * c[8]) + c[11]
            goods.append(m_in & (z0 > 0) & (z0 < distance_thresh) & (z1 > 0) & (z1 < distance_thresh))
    n = np.array([int(g.sum()) for g in goods], dtype=np.int64)
    k = 0 if (n[0] >= n[1] and n[0] >= n[2] and n[0] >= n[3]) else 1 if (n[1] >= n[2] and n[1] >= n[3]) else 2 if n[2] >= n[3] else 3
    out = (int(n[k]), cands[k][0], cands[k][1].copy(), goods[k])
    return out + (n, k) if detail else out


# ---- least-squares refit on the inliers as the device computes it (csrc/model_refit_solve.h) -------------------------------------
MR_SWEEPS9 = 8           # cyclic Jacobi sweeps over the 9 x 9 normal matrix
MR_LANES = 256           # the lanes whose partial sums fix the summation order
MR_MIN_POINTS = (4, 8)   # inliers a refit needs: homography, fundamental matrix
MR_MAX_ROUNDS = 8


def _mr_block_sum(terms, inl):
    """the kernel's sum of terms [P, K] over the inliers `inl` [P]: lane l adds its points l, l + 256, ... in ascending order, a wave's
    64 lanes are combined by the tree x[l] += x[l + o], o = 32 .. 1, the four wave totals are added in wave order -> [K]"""
    P, K = terms.shape
    rows = max(1, -(-P // MR_LANES))
    pad = np.zeros((rows * MR_LANES, K))
    pad[:P] = np.where(inl[:, None], terms, 0.0)             # a point outside the mask is never read: its NaN stays out
    pad = pad.reshape(rows, MR_LANES, K)
    acc = np.zeros((MR_LANES, K))
    for r in range(rows):
        acc = acc + pad[r]
    w = acc.reshape(4, 64, K)
    for o in (32, 16, 8, 4, 2, 1):
        w = w[:, :o] + w[:, o:2 * o]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def _mr_solve(kind, a, b, inl, sweeps=MR_SWEEPS9, detail=False):
    """steps 2 to 6 of gim_model_refit on the points a, b [P, 2] whose `inl` [P] is set (at least one, all finite) -> the model
    [3, 3] or None (a side without extent, a result that is not finite, a zero norm or h33 == 0).  detail=True: (model, off) with
    off = the largest off-diagonal |entry| of the 9 x 9 matrix after the sweeps over its largest diagonal |entry|."""
    n = int(inl.sum())
    with np.errstate(all="ignore"):
        s4 = _mr_block_sum(np.concatenate([a, b], 1), inl)
        ca, cb = s4[:2] / n, s4[2:] / n
        pa, pb = a - ca, b - cb
        dist = np.stack([np.sqrt(pa[:, 0] * pa[:, 0] + pa[:, 1] * pa[:, 1]), np.sqrt(pb[:, 0] * pb[:, 0] + pb[:, 1] * pb[:, 1])], 1)
        md = _mr_block_sum(dist, inl) / n
        if not (md[0] > 0.0 and md[1] > 0.0 and np.isfinite(md).all()):
            return (None, 0.0) if detail else None
        sa, sb = np.sqrt(2.0) / md[0], np.sqrt(2.0) / md[1]
        x, y, u, v = pa[:, 0] * sa, pa[:, 1] * sa, pb[:, 0] * sb, pb[:, 1] * sb
        o, z = np.ones_like(x), np.zeros_like(x)
        if kind == 0:
            r1 = [x, y, o, z, z, z, -u * x, -u * y, -u]
            r2 = [z, z, z, x, y, o, -v * x, -v * y, -v]
            terms = np.stack([r1[i] * r1[j] + r2[i] * r2[j] for i in range(9) for j in range(i, 9)], 1)
        else:
            r = [u * x, u * y, u, v * x, v * y, v, x, y, o]
            terms = np.stack([r[i] * r[j] for i in range(9) for j in range(i, 9)], 1)
        A = np.zeros((9, 9))
        A[np.triu_indices(9)] = _mr_block_sum(terms, inl)
        d, vec = _rp_jacobi(A, sweeps)
        off = np.abs(np.triu(A, 1)).max() / max(np.abs(d).max(), 1e-300)
        f = vec[:, int(np.argmin(d))].reshape(3, 3).copy()                  # the first smallest, as the device's strict <
        if kind == 1:
            g = np.array([[(f[0, i] * f[0, j] + f[1, i] * f[1, j]) + f[2, i] * f[2, j] for j in range(3)] for i in range(3)])
            d3, v3 = _rp_jacobi(g, RP_SWEEPS3)
            for i, j in ((0, 1), (0, 2), (1, 2)):
                if d3[j] > d3[i]:
                    d3[[i, j]] = d3[[j, i]]
                    v3[:, [i, j]] = v3[:, [j, i]]
            v2 = v3[:, 2] / np.sqrt(_rp_dot3(v3[:, 2], v3[:, 2]))
            for i in range(3):
                f[i] = f[i] - _rp_dot3(f[i], v2) * v2
        m = np.stack([f[:, 0] * sa, f[:, 1] * sa, f[:, 2] - sa * (f[:, 0] * ca[0] + f[:, 1] * ca[1])], 1)          # f Ta
        if kind == 0:
            out = np.stack([m[0] / sb + cb[0] * m[2], m[1] / sb + cb[1] * m[2], m[2]])                              # Tb^-1 (f Ta)
            scale = out[2, 2]
        else:
            out = np.stack([sb * m[0], sb * m[1], m[2] - sb * (cb[0] * m[0] + cb[1] * m[1])])                       # Tb^T (f Ta)
            ss = 0.0
            for e in out.ravel():
                ss = ss + e * e
            scale = np.sqrt(ss)
        if not (scale != 0.0 and np.isfinite(scale)):
            return (None, off) if detail else None
        out = out / scale
    if not np.isfinite(out).all():
        out = None
    return (out, off) if detail else out


def _mr_points(a, b, n_min):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 2)
    if a.shape[0] < n_min or not (np.isfinite(a).all() and np.isfinite(b).all()):
        return None
    return a, b


def homography_dlt_ge(src, dst):
    """`homography_dlt` in the arithmetic of gim_model_refit (kind 0): the 9 x 9 normal matrix of the normalised system summed in
    the kernel's order, the eigenvector of its smallest eigenvalue by cyclic Jacobi with MR_SWEEPS9 sweeps in place of LAPACK's SVD
    -> H [3, 3] with h33 = 1, or None (fewer than 4 points, a coordinate that is not finite, a degenerate set)."""
    pts = _mr_points(src, dst, 4)
    return None if pts is None else _mr_solve(0, pts[0], pts[1], np.ones(pts[0].shape[0], dtype=bool))


def eight_point_ge(x0, x1):
    """The normalised eight-point algorithm (Hartley 1997; OpenCV's run8Point) in the arithmetic of gim_model_refit (kind 1):
    x1^T F x0 = 0 over n >= 8 correspondences, F of rank 2 and unit Frobenius norm, or None."""
    pts = _mr_points(x0, x1, 8)
    return None if pts is None else _mr_solve(1, pts[0], pts[1], np.ones(pts[0].shape[0], dtype=bool))


def refit_ge(kind, a, b, model, thr2, mask=None, rounds=1, detail=False):
    """gim_model_refit for one pair in numpy (include/gim_hip.h is the contract, csrc/model_refit_solve.h the code) -- the CPU oracle
    of ops.model_refit.  kind 0: b ~ H a under `transfer_error`; kind 1: b^T F a = 0 under `sampson_error`.  Starting from `model`
    and `mask` (None: the model's own mask under thr2), up to `rounds` times: refit on the current inliers (`_mr_solve`), take the
    candidate's mask, keep the candidate iff it has no fewer inliers; stop at the first candidate that cannot be made, is rejected or
    reproduces the current mask.  -> (model [3, 3], mask bool [P], counts (start, final), accepted); a model that is all zero or not
    finite: (zeros, all-False, (0, 0), -1).
    detail=True adds a dict: `models` the models whose error was compared with thr2 (the start when mask is None, then every
    candidate), `counts` their inlier counts, `margin` [P] = the smallest |error - thr2| / thr2 of each point under those models (a
    point is decidable when it is at least 1e-6), `off` the Jacobi off-diagonal mass of every solve, `stop` why the loop ended."""
    if kind not in (0, 1):
        raise ValueError(f"kind={kind!r}: 0 (homography) or 1 (fundamental matrix)")
    rounds = int(rounds)
    if not 1 <= rounds <= MR_MAX_ROUNDS:
        raise ValueError(f"rounds={rounds}: 1 <= rounds <= {MR_MAX_ROUNDS}")
    a = np.asarray(a, dtype=np.float64).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 2)
    P = a.shape[0]
    model = np.asarray(model, dtype=np.float64).reshape(3, 3)
    thr2 = float(thr2)
    error = transfer_error if kind == 0 else sampson_error
    info = dict(models=[], counts=[], margin=np.full(P, np.inf), off=[], stop="skipped")

    def score(M):
        with np.errstate(all="ignore"):
            e = error(M, a, b)
            info["margin"] = np.fmin(info["margin"], np.where(np.isfinite(e), np.abs(e - thr2) / max(thr2, 1e-300), np.inf))
            m = e <= thr2
        info["models"].append(M)
        info["counts"].append(int(m.sum()))
        return m

    if not (np.isfinite(model).all() and (model != 0.0).any()):
        out = (np.zeros((3, 3)), np.zeros(P, dtype=bool), (0, 0), -1)
        return out + (info,) if detail else out
    cur = model.copy()
    cur_mask = score(cur) if mask is None else np.asarray(mask).ravel() != 0
    n = n0 = int(cur_mask.sum())
    accepted, info["stop"] = 0, "rounds"
    for _ in range(rounds):
        if n < MR_MIN_POINTS[kind]:
            info["stop"] = "few"
            break
        if not (np.isfinite(a[cur_mask]).all() and np.isfinite(b[cur_mask]).all()):
            info["stop"] = "nonfinite"
            break
        cand, off = _mr_solve(kind, a, b, cur_mask, detail=True)
        info["off"].append(off)
        if cand is None:
            info["stop"] = "degenerate"
            break
        cand_mask = score(cand)
        nc = int(cand_mask.sum())
        if nc < n:
            info["stop"] = "rejected"
            break
        fixed = np.array_equal(cand_mask, cur_mask)
        cur, cur_mask, n, accepted = cand, cand_mask, nc, accepted + 1
        if fixed:
            info["stop"] = "fixed"
            break
    out = (cur, cur_mask, (n0, n), accepted)
    return out + (info,) if detail else out
