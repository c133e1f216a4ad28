"""Seeded two-view scenes shared by test_model_refit_cpu.py and test_gpu_model_refit.py: planar scenes for the homography refit
(kind 0) and general scenes for the fundamental-matrix refit (kind 1), in pixels of a 640 x 480 image pair.  Every scene comes with
the plain-RANSAC model the refit starts from.  Nothing here needs a GPU."""
import functools

import numpy as np

from gim_amd import pose

W, H_IMG = 640.0, 480.0
K_CAM = np.array([[520.0, 0.0, 320.0], [0.0, 520.0, 240.0], [0.0, 0.0, 1.0]])
THR = 1.0                   # pixels: the demo's threshold
THR2 = THR * THR
DECIDE = 1e-6               # a point is decidable when its error is at least this far (relative) from thr2 under every model visited

# ---- bars -------------------------------------------------------------------------------------------------------------------------
EXACT_BAR = 1e-9            # recovery of the true model from noise-free points, of scale (test_fundamental_cpu / test_essential_cpu)
# The largest entry difference between the Jacobi restatement (homography_dlt_ge / eight_point_ge) and LAPACK (homography_dlt / an
# SVD eight-point) on the inliers of every problem() below, both noisy seeds, every size of SIZES that can be fitted, as
# test_model_refit_cpu.py::test_against_lapack measures, prints and caps it.  H (h33 = 1) relative to its largest |entry|: 8.4e-15
# (five points); F (unit norm, up to sign): 1.6e-13 (nine points), 4.2e-14 on 2 000.  The bar is 8 x the measured difference.
H_MEASURED = 8.5e-15
F_MEASURED = 1.6e-13
H_BAR = 8.0 * H_MEASURED
F_BAR = 8.0 * F_MEASURED
UNDECIDABLE_CAP = 0.01      # of a scene's points; the seeds below leave none

NOISY_SEEDS = (11, 12)
EXACT_SEEDS = (21, 22)


def _rot(rng, deg):
    w = rng.normal(size=3)
    w = w / np.linalg.norm(w) * np.deg2rad(deg)
    t = np.linalg.norm(w)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / t
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * k @ k


def _project(Kc, X):
    x = X @ Kc.T
    return x[:, :2] / x[:, 2:]


@functools.lru_cache(maxsize=None)
def scene(kind, seed, n=2000, outliers=0.5, noise=0.3):
    """-> (a [n, 2], b [n, 2], true model, true-inlier mask [n]); kind 0: b ~ H a on a plane, kind 1: b^T F a = 0 in general position.
    The arrays are shared between tests: read-only."""
    rng = np.random.default_rng(1000 * kind + seed)
    R = _rot(rng, 12.0)
    t = np.array([0.4, -0.1, 0.15]) + 0.05 * rng.normal(size=3)
    a = np.stack([rng.uniform(20, W - 20, n), rng.uniform(20, H_IMG - 20, n)], 1)
    rays = np.concatenate([a, np.ones((n, 1))], 1) @ np.linalg.inv(K_CAM).T
    if kind == 0:
        nrm, d = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0]), 5.0
        depth = d / (rays @ nrm)
        M = K_CAM @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(K_CAM)
        M = M / M[2, 2]
    else:
        depth = rng.uniform(3.0, 9.0, n)
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        M = np.linalg.inv(K_CAM).T @ tx @ R @ np.linalg.inv(K_CAM)
        M = M / np.linalg.norm(M)
    X = rays * depth[:, None]
    b = _project(K_CAM, X @ R.T + t)
    inl = np.ones(n, dtype=bool)
    n_out = int(round(outliers * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        b[bad] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H_IMG, n_out)], 1)
    if noise:
        a = a + noise * rng.normal(size=a.shape) * inl[:, None]
        b = b + noise * rng.normal(size=b.shape) * inl[:, None]
    for arr in (a, b, M, inl):
        arr.setflags(write=False)
    return a, b, M, inl


def noisy(kind, seed):
    return scene(kind, seed)


def exact(kind, seed):
    return scene(kind, seed, n=64, outliers=0.0, noise=0.0)


@functools.lru_cache(maxsize=None)
def start_model(kind, seed, n=2000):
    """the plain RANSAC's best minimal-sample model on scene(kind, seed, n): what the refit starts from"""
    a, b, _, _ = scene(kind, seed, n)
    if kind == 0:
        M, _ = pose._ransac(a, b, pose.homography_4pt, 4, THR, 0.999999, 2000, np.random.default_rng(seed), error=pose.transfer_error)
    else:
        M, _ = pose.find_fundamental_mat(a, b, THR, max_iters=2000, seed=seed, solve="ge", sampler="philox")
    assert M is not None
    M = np.array(M)
    M.setflags(write=False)
    return M


SIZES = {0: (0, 3, 4, 5, 255, 256, 257, 2000), 1: (0, 7, 8, 9, 255, 256, 257, 2000)}   # the GPU test's point counts
SEED = NOISY_SEEDS[0]


@functools.lru_cache(maxsize=None)
def problem(kind, seed, n=2000):
    """n points of the noisy scene with the start model of the whole scene and that model's own mask -> (a, b, M, mask).  n >= 255:
    the first n matches, half of them outliers.  n <= 9: the n true inliers the start model fits best, in scene order -- all of
    them inliers of the start model, so the minimum-count rule is what decides at 3 / 4 and 7 / 8."""
    a, b, _, inl = scene(kind, seed)
    M = start_model(kind, seed)
    if n <= 9:
        e = np.where(inl, error(kind)(M, a, b), np.inf)
        idx = np.sort(np.argsort(e, kind="stable")[:n])
    else:
        idx = np.arange(n)
    a, b = np.array(a[idx]), np.array(b[idx])
    mask = error(kind)(M, a, b) <= THR2
    assert n > 9 or mask.all()
    for arr in (a, b, mask):
        arr.setflags(write=False)
    return a, b, M, mask


@functools.lru_cache(maxsize=None)
def oracle(kind, seed, rounds, with_mask, n=2000):
    """refit_ge(detail=True) on problem(kind, seed, n); with_mask: the model's own mask is passed in (the same start as mask=None,
    through the other entrance)"""
    a, b, M, mask = problem(kind, seed, n)
    return pose.refit_ge(kind, a, b, M, THR2, mask=mask if with_mask else None, rounds=rounds, detail=True)


def error(kind):
    return pose.transfer_error if kind == 0 else pose.sampson_error


def model_diff(kind, A, B):
    """the largest entry difference: H relative to the largest |entry| (both have h33 = 1), F up to sign (both have unit norm)"""
    A, B = np.asarray(A), np.asarray(B)
    if kind == 0:
        return np.abs(A - B).max() / np.abs(B).max()
    return min(np.abs(A - B).max(), np.abs(A + B).max())


def bar(kind):
    return H_BAR if kind == 0 else F_BAR


def decidable(info):
    return info["margin"] >= DECIDE
