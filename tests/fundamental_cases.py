"""Seeded inputs shared by tests/test_fundamental_cpu.py (which judges them with the host code alone) and the GPU tests
tests/test_gpu_fundamental.py.  Nothing here touches a device; every case is built once and frozen.  Every case carries the host
answer pose.seven_point_ge(..., detail=True) and a `band` flag per sample: set when a rule of the solver is within a factor 10 of its
threshold (seventh pivot ratio, size of the cubic, leading coefficient, discriminant), where the host's and the device's rounding may decide differently."""
import functools

import numpy as np

from gim_amd import pose, pose_math

THR2 = 1.0                       # (1 px)^2, the demo's threshold
W, H_IMG = 640.0, 480.0
_K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def two_views(rng, n, planar=False):
    """n exact correspondences in pixels of a 640 x 480 camera pair (a turn of 0.2 rad about y, a sideways step) -> (x0, x1 [n, 2],
    F [3, 3] of unit norm with x1^T F x0 = 0).  planar: the scene points lie on one plane (the epipolar rows then have rank 6)."""
    X = np.concatenate([rng.uniform(-2.0, 2.0, (n, 2)), rng.uniform(4.0, 8.0, (n, 1))], 1)
    if planar:
        X[:, 2] = 5.0 + 0.1 * X[:, 0] - 0.2 * X[:, 1]
    c, s = np.cos(0.2), np.sin(0.2)
    R, t = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]), np.array([0.5, 0.1, 0.05])
    x0, x1 = X @ _K.T, (X @ R.T + t) @ _K.T
    Ki = np.linalg.inv(_K)
    F = Ki.T @ _skew(t) @ R @ Ki
    return x0[:, :2] / x0[:, 2:], x1[:, :2] / x1[:, 2:], F / np.linalg.norm(F)


def sampson(F, x0, x1):
    """the fp64 numpy oracle of the inlier rule: (x1^T F x0)^2 / max(|F x0|_xy^2 + |F^T x1|_xy^2, 1e-300), F [..., 3, 3] -> [..., P]"""
    h0 = np.concatenate([x0, np.ones((x0.shape[0], 1))], 1)
    h1 = np.concatenate([x1, np.ones((x1.shape[0], 1))], 1)
    a = np.einsum("...ij,pj->...pi", F, h0)                       # F x0
    b = np.einsum("...ji,pj->...pi", F, h1)                       # F^T x1
    num = np.einsum("...pi,pi->...p", a, h1) ** 2
    return num / np.maximum(a[..., 0] ** 2 + a[..., 1] ** 2 + b[..., 0] ** 2 + b[..., 1] ** 2, 1e-300)


def sin_dist(A, B):
    """sine of the angle between the 9-vectors of A [..., 3, 3] and B [..., 3, 3] (sign-free), accurate at small angles: the norm of
    the part of A / |A| that is orthogonal to B / |B|"""
    a = A.reshape(*A.shape[:-2], 9)
    b = np.broadcast_to(B.reshape(*B.shape[:-2], 9), a.shape)
    a = a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-300)
    b = b / np.maximum(np.linalg.norm(b, axis=-1, keepdims=True), 1e-300)
    return np.linalg.norm(a - (a * b).sum(-1, keepdims=True) * b, axis=-1)


def residuals(F, x0s, x1s):
    """F [N, 3, 3, 3] (unit norm), samples x0s, x1s [N, 7, 2] -> (largest |row . f| over the seven unit-norm epipolar rows [N, 3],
    |det F| [N, 3])"""
    rows = pose_math._epipolar_rows(x0s, x1s)
    rows = rows / np.linalg.norm(rows, axis=-1, keepdims=True)
    r = np.abs(np.einsum("nik,nmk->nmi", rows, F.reshape(F.shape[0], 3, 9))).max(-1)
    return r, np.abs(np.linalg.det(F))


def in_band(info):
    """samples within a factor 10 of a threshold of the solver, each rule judged only where the rules before it passed"""
    with np.errstate(all="ignore"):
        p, m, l, d = info["pivot_ratio"], info["cubic_scale"], info["lead_ratio"], np.abs(info["disc_rel"])
        s1 = info["ok_scale"]
        s2 = s1 & info["ok_rank"]
        s3 = s2 & info["ok_cubic"]
        s4 = s3 & info["ok_lead"]
        return ((s1 & (p >= pose.F7_RANK_EPS / 10) & (p <= pose.F7_RANK_EPS * 10)) |
                (s2 & (m >= pose.F7_CUBIC_EPS / 10) & (m <= pose.F7_CUBIC_EPS * 10)) |
                (s3 & (l >= pose.F7_LEAD_EPS / 10) & (l <= pose.F7_LEAD_EPS * 10)) | (s4 & ~(d > pose.F7_DISC_EPS * 10)))


@functools.lru_cache(maxsize=None)
def ransac_scene(seed=7, P=300, inliers=180, min_dist=5.0):
    """the decidable scene of the find_fundamental_mat tests (host and device): P matches, `inliers` exact ones, every other one at
    least min_dist px (Sampson) from the true epipolar geometry -> (F, p0, p1, truth)"""
    rng = np.random.default_rng(seed)
    p0, p1, F = two_views(rng, P)
    truth = np.zeros(P, dtype=bool)
    truth[rng.permutation(P)[:inliers]] = True
    for i in np.flatnonzero(~truth):
        while True:
            p1[i] = rng.uniform([0.0, 0.0], [W, H_IMG])
            if np.sqrt(sampson(F, p0[i:i + 1], p1[i:i + 1]))[0] >= min_dist:
                break
    for a in (F, p0, p1, truth):
        a.setflags(write=False)
    return F, p0, p1, truth


# planted samples of `step_case`, by row of idx
ROW_REPEAT, ROW_PAST, ROW_NEG, ROW_COLLINEAR, ROW_COINCIDE, ROW_PLANAR = 3, 5, 6, 40, 41, 42


class StepCase:
    """Three pairs with ragged offsets [0, 1000, 1000, 1065] (the middle one empty, the last shorter than one 256-point pass) and
    K = 257 samples each.  A pair: exact two-view matches with 0.3 px of noise, 50 % uniform outliers.  Three blocks of seven points
    near the pair's end are overwritten: n-30.. on a planar scene, n-20.. collinear on side 0, n-13.. coincident on side 1.  Samples:
    random distinct 7-tuples; planted rows: a repeated index, an index equal to n, an index -1, the three blocks.
    Host answers (pose.seven_point_ge): models, valid, info, and the band of undecidable samples."""

    def __init__(self, seed=21):
        rng = np.random.default_rng(seed)
        self.offsets = np.array([0, 1000, 1000, 1065], dtype=np.int32)
        x0, x1 = [], []
        for n in (1000, 0, 65):
            a, b, _ = two_views(rng, n)
            b = b + rng.normal(size=(n, 2)) * 0.3
            out = rng.random(n) < 0.5
            b[out] = rng.uniform([0.0, 0.0], [W, H_IMG], (int(out.sum()), 2))
            if n:
                a[n - 30:n - 23], b[n - 30:n - 23], _ = two_views(rng, 7, planar=True)
                a[n - 20:n - 13, 1] = 0.5 * a[n - 20:n - 13, 0] + 40.0
                b[n - 13:n - 6] = b[n - 13]
            x0.append(a)
            x1.append(b)
        self.x0, self.x1 = np.ascontiguousarray(np.concatenate(x0)), np.ascontiguousarray(np.concatenate(x1))
        K = 257
        self.idx = np.zeros((3, K, 7), dtype=np.int32)
        self.models, self.valid, self.band, self.info = {}, {}, {}, {}
        for b, n in ((0, 1000), (2, 65)):
            idx = np.stack([rng.choice(n, 7, replace=False) for _ in range(K)]).astype(np.int32)
            idx[ROW_REPEAT, 4] = idx[ROW_REPEAT, 1]
            idx[ROW_PAST, 2] = n
            idx[ROW_NEG, 6] = -1
            idx[ROW_PLANAR] = np.arange(n - 30, n - 23)
            idx[ROW_COLLINEAR] = np.arange(n - 20, n - 13)
            idx[ROW_COINCIDE] = np.arange(n - 13, n - 6)
            self.idx[b] = idx
            a, c = self.pair(b)
            safe = np.clip(idx, 0, n - 1)
            F, v, info = pose.seven_point_ge(a[safe], c[safe], detail=True)
            refused = ((idx < 0) | (idx >= n)).any(1) | np.array([len(set(r)) < 7 for r in idx.tolist()])   # the kernel's index rule
            F[refused], v[refused] = 0.0, False
            self.models[b], self.valid[b], self.band[b], self.info[b] = F, v, in_band(info) & ~refused, info
        self.idx[1] = self.idx[0]                                # the empty pair: every index is outside it
        self.valid[1], self.band[1] = np.zeros((K, 3), dtype=bool), np.zeros(K, dtype=bool)
        for a in (self.x0, self.x1, self.idx, self.offsets):
            a.setflags(write=False)

    def pair(self, b):
        return self.x0[self.offsets[b]:self.offsets[b + 1]], self.x1[self.offsets[b]:self.offsets[b + 1]]


@functools.lru_cache(maxsize=None)
def step_case():
    return StepCase()


@functools.lru_cache(maxsize=None)
def tiny_case():
    """one pair of exactly 7 exact matches, K = 1: the smallest problem the kernel accepts -> (x0, x1, idx [1, 7], F, valid, info, band)"""
    x0, x1, _ = two_views(np.random.default_rng(22), 7)
    idx = np.arange(7, dtype=np.int32)[None]
    F, v, info = pose.seven_point_ge(x0[idx], x1[idx], detail=True)
    return x0, x1, idx, F, v, info, in_band(info)


@functools.lru_cache(maxsize=None)
def batch_pairs():
    """the five pairs of the lockstep test: the decidable scene, 6 points (no model), 7 points, and the two pairs of `step_case`"""
    _, p0, p1, _ = ransac_scene()
    t0, t1 = tiny_case()[:2]
    c = step_case()
    return [(p0, p1), (t0[:6], t1[:6]), (t0, t1), c.pair(2), c.pair(0)]
