"""Seeded inputs shared by tests/test_essential_cpu.py (which judges them with the host code alone) and the GPU tests
tests/test_gpu_essential.py.  Nothing here touches a device; every case is built once and frozen.  Every case carries the host answer
pose.five_point_ge(..., detail=True) and a `band` flag per sample: set when a diagnostic of the solver is within a factor 10 of its
threshold (the two pivot ratios, |v[9]| / max |v|), when two real roots are closer than 1e-6 relative, when a 2 x 2 block's
discriminant is below 1e-6 relative (real pair or complex pair: undecidable), or when the QR iteration did not converge -- where the
host's and the device's rounding may decide differently."""
import functools

import numpy as np

from fundamental_cases import sampson   # noqa: F401  (the fp64 numpy oracle of the inlier rule, the same for E and F)
from gim_amd import pose

THR = 1e-3                       # 0.5 px at a focal length of 500 px: the ZEB threshold in normalised coordinates
THR2 = THR * THR
FOCAL, CENTRE = 500.0, np.array([320.0, 240.0])
K_PIX = np.array([[FOCAL, 0.0, CENTRE[0]], [0.0, FOCAL, CENTRE[1]], [0.0, 0.0, 1.0]])
_C, _S = np.cos(0.2), np.sin(0.2)
R_TRUE = np.array([[_C, 0.0, _S], [0.0, 1.0, 0.0], [-_S, 0.0, _C]])
T_TRUE = np.array([0.5, 0.1, 0.05])


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def two_views(rng, n):
    """n exact correspondences in normalised camera coordinates (a turn of 0.2 rad about y, a sideways step) -> (x0, x1 [n, 2],
    E [3, 3] of unit norm with x1^T E x0 = 0)"""
    X = np.concatenate([rng.uniform(-2.0, 2.0, (n, 2)), rng.uniform(4.0, 8.0, (n, 1))], 1)
    Y = X @ R_TRUE.T + T_TRUE
    E = _skew(T_TRUE) @ R_TRUE
    return X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:], E / np.linalg.norm(E)


def noisy_pair(rng, n, noise=2e-4):
    """n matches: exact ones with `noise` (0.1 px at f = 500) on side 1, 50 % replaced by uniform outliers"""
    a, b, _ = two_views(rng, n)
    b = b + rng.normal(size=(n, 2)) * noise
    out = rng.random(n) < 0.5
    b[out] = rng.uniform([-0.64, -0.48], [0.64, 0.48], (int(out.sum()), 2))
    return a, b


def dist(A, B):
    """sign-aligned Frobenius distance min(|a - b|, |a + b|) of A [..., 3, 3] and B [..., 3, 3]"""
    f = lambda M: np.linalg.norm(M.reshape(*M.shape[:-2], 9), axis=-1)   # noqa: E731
    return np.minimum(f(A - B), f(A + B))


def set_dist(A, va, B, vb):
    """two sets of models of one sample, A [10, 3, 3] / va [10] and B / vb with equally many valid ones -> the largest distance of a
    model of A to its nearest model of B, and of one of B to its nearest of A (0 for two empty sets)"""
    if not va.any():
        return 0.0
    D = dist(A[va][:, None], B[vb][None])
    return float(max(D.min(1).max(), D.min(0).max()))


def residuals(E, x0s, x1s):
    """E [N, 10, 3, 3] (unit norm), samples x0s, x1s [N, 5, 2] -> (largest |p1^T E p0| over the five points [N, 10], largest entry of
    |2 E E^T E - tr(E E^T) E| [N, 10])"""
    o = np.ones((*x0s.shape[:-1], 1))
    h0, h1 = np.concatenate([x0s, o], -1), np.concatenate([x1s, o], -1)
    r = np.abs(np.einsum("npi,nmij,npj->nmp", h1, E, h0)).max(-1)
    EEt = E @ np.swapaxes(E, -1, -2)
    tr = np.trace(EEt, axis1=-2, axis2=-1)
    c = np.abs(2.0 * EEt @ E - tr[..., None, None] * E).reshape(*E.shape[:-2], 9).max(-1)
    return r, c


def in_band(info):
    """samples within a factor 10 of a threshold of the solver (each rule judged only where the rules before it passed), or with a
    root gap or a discriminant below 1e-6 relative, or whose QR iteration ran out of sweeps"""
    with np.errstate(all="ignore"):
        p, m, w = info["rank_ratio"], info["pivot_ratio"], info["w_ratio"]
        s1 = info["ok_input"]
        s2 = s1 & info["ok_rank"]
        s3 = s2 & info["ok_pivot"]
        return ((s1 & (p >= pose.E5_RANK_EPS / 10) & (p <= pose.E5_RANK_EPS * 10)) |
                (s2 & (m >= pose.E5_PIVOT_EPS / 10) & (m <= pose.E5_PIVOT_EPS * 10)) |
                (s3 & ((w <= pose.E5_W_EPS * 10) | (info["gap_rel"] < 1e-6) | (info["disc_rel"] < 1e-6) | ~info["qr_ok"])))


@functools.lru_cache(maxsize=None)
def ransac_scene(seed=7, P=300, inliers=180, min_dist=10.0 * THR):
    """the decidable scene of the find_essential_mat tests (host and device): P matches, `inliers` exact ones, every other one at
    least min_dist (Sampson, 10 x the threshold) from the true epipolar geometry -> (E, x0, x1, truth)"""
    rng = np.random.default_rng(seed)
    x0, x1, E = two_views(rng, P)
    truth = np.zeros(P, dtype=bool)
    truth[rng.permutation(P)[:inliers]] = True
    for i in np.flatnonzero(~truth):
        while True:
            x1[i] = rng.uniform([-0.64, -0.48], [0.64, 0.48])
            if np.sqrt(sampson(E, x0[i:i + 1], x1[i:i + 1]))[0] >= min_dist:
                break
    for a in (E, x0, x1, truth):
        a.setflags(write=False)
    return E, x0, x1, truth


def to_pixels(x):
    return x * FOCAL + CENTRE


# planted samples of `step_case`, by row of idx
ROW_REPEAT, ROW_PAST, ROW_NEG, ROW_COINCIDE, ROW_RANK4, ROW_NONFINITE = 3, 5, 6, 40, 41, 42
PLANTED = (ROW_REPEAT, ROW_PAST, ROW_NEG, ROW_COINCIDE, ROW_RANK4, ROW_NONFINITE)


class StepCase:
    """Three pairs with ragged offsets [0, 1000, 1000, 1065] (the middle one empty, the last shorter than one 256-point pass) and
    K = 257 samples each.  A pair: `noisy_pair`.  Near the pair's end: the five matches n-20.. are one and the same point on both
    sides, the match n-12 repeats the match n-13, the match n-1 has a NaN on side 1.  Samples: random distinct 5-tuples; planted
    rows: a repeated index, an index equal to n, an index -1, the coincident block, the block with the repeated match (rank 4),
    a sample that holds the NaN.  Host answers (pose.five_point_ge): models, valid, info, and the band of undecidable samples."""

    def __init__(self, seed=21):
        rng = np.random.default_rng(seed)
        self.offsets = np.array([0, 1000, 1000, 1065], dtype=np.int32)
        x0, x1 = [], []
        for n in (1000, 0, 65):
            a, b = noisy_pair(rng, n)
            if n:
                a[n - 20:n - 15], b[n - 20:n - 15] = a[n - 20], b[n - 20]
                a[n - 12], b[n - 12] = a[n - 13], b[n - 13]
                b[n - 1, 1] = np.nan
            x0.append(a)
            x1.append(b)
        self.x0, self.x1 = np.ascontiguousarray(np.concatenate(x0)), np.ascontiguousarray(np.concatenate(x1))
        K = 257
        self.idx = np.zeros((3, K, 5), dtype=np.int32)
        self.models, self.valid, self.band, self.info = {}, {}, {}, {}
        for b, n in ((0, 1000), (2, 65)):
            idx = np.stack([rng.choice(n - 1, 5, replace=False) for _ in range(K)]).astype(np.int32)
            idx[ROW_REPEAT, 4] = idx[ROW_REPEAT, 1]
            idx[ROW_PAST, 2] = n
            idx[ROW_NEG, 3] = -1
            idx[ROW_COINCIDE] = np.arange(n - 20, n - 15)
            idx[ROW_RANK4] = np.arange(n - 13, n - 8)
            idx[ROW_NONFINITE] = [0, 1, n - 1, 2, 3]
            self.idx[b] = idx
            a, c = self.pair(b)
            safe = np.clip(idx, 0, n - 1)
            E, v, info = pose.five_point_ge(a[safe], c[safe], detail=True)
            refused = ((idx < 0) | (idx >= n)).any(1) | np.array([len(set(r)) < 5 for r in idx.tolist()])   # the kernel's index rule
            E[refused], v[refused] = 0.0, False
            self.models[b], self.valid[b], self.band[b], self.info[b] = E, v, in_band(info) & ~refused, info
        self.idx[1] = self.idx[0]                                # the empty pair: every index is outside it
        self.valid[1], self.band[1] = np.zeros((K, 10), dtype=bool), np.zeros(K, dtype=bool)
        for a in (self.x0, self.x1, self.idx, self.offsets):
            a.setflags(write=False)

    def pair(self, b):
        return self.x0[self.offsets[b]:self.offsets[b + 1]], self.x1[self.offsets[b]:self.offsets[b + 1]]


@functools.lru_cache(maxsize=None)
def step_case():
    return StepCase()


@functools.lru_cache(maxsize=None)
def tiny_case():
    """one pair of exactly 5 exact matches, K = 1: the smallest problem the kernel accepts -> (x0, x1, idx [1, 5], E truth, models,
    valid, info, band)"""
    x0, x1, Et = two_views(np.random.default_rng(22), 5)
    idx = np.arange(5, dtype=np.int32)[None]
    E, v, info = pose.five_point_ge(x0[idx], x1[idx], detail=True)
    return x0, x1, idx, Et, E, v, info, in_band(info)


@functools.lru_cache(maxsize=None)
def batch_pairs():
    """the five pairs of the lockstep test: the decidable scene, 4 points (no model), 5 points, and noisy pairs of 65 and 1000"""
    _, x0, x1, _ = ransac_scene()
    t0, t1 = tiny_case()[:2]
    rng = np.random.default_rng(23)
    return [(x0, x1), (t0[:4], t1[:4]), (t0, t1), noisy_pair(rng, 65), noisy_pair(rng, 1000)]
