"""Seeded inputs and the shared measures of tests/test_recover_pose_cpu.py and tests/test_gpu_recover_pose.py: two-view scenes with
outliers and noise, the decidability rule of a (point, candidate) pair, and the comparison of a pose with the host's up to the
candidate order.  Numpy only; every reference is computed once per process and never changed."""
import functools

import numpy as np

from gim_amd import pose, pose_math

NOISE = 5e-4
# |R - R'| and |t - t'| of pose.recover_pose_ge against pose.recover_pose (LAPACK): the largest over the five scenes of P = 2 000 was
# 7.008e-16 for R and 2.220e-16 for t on the machine that wrote this (test_recover_pose_cpu.py measures it again and prints it); the bar
# is 8 x that, the margin the sibling solver tests give a re-rounded algorithm.  The device against recover_pose_ge uses the same
# bar: they differ by FMA contraction alone.
RT_MEASURED = 7.008e-16
RT_BAR = 8.0 * RT_MEASURED
UNDECIDABLE_CAP = 0.01
K_PIX = np.array([[800.0, 0.0, 320.0], [0.0, 800.0, 240.0], [0.0, 0.0, 1.0]])


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def rotation(axis, angle):
    k = skew(axis / np.linalg.norm(axis))
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


@functools.lru_cache(maxsize=None)
def scene(seed, P, outliers=0.5):
    """P points with x in [-2, 2], y in [-1.5, 1.5], z in [2, 10] in camera 0, a rotation of about 0.15 rad about a random axis, a unit
    translation, `outliers` of the x1 replaced by uniform points of [-1, 1]^2, NOISE on both sides -> (E = [t]x R, x0, x1 [P,2], R, t)"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, P), rng.uniform(-1.5, 1.5, P), rng.uniform(2, 10, P)], 1)
    R = rotation(rng.normal(size=3), 0.15 * (1.0 + 0.1 * rng.normal()))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    Y = X @ R.T + t
    x0 = X[:, :2] / X[:, 2:]
    x1 = Y[:, :2] / Y[:, 2:]
    out = rng.permutation(P)[:int(round(outliers * P))]
    x1[out] = rng.uniform(-1, 1, (len(out), 2))
    x0 = x0 + NOISE * rng.normal(size=x0.shape)
    x1 = x1 + NOISE * rng.normal(size=x1.shape)
    for a in (x0, x1):
        a.setflags(write=False)
    return skew(t) @ R, x0, x1, R, t


SCENE_SEEDS = (101, 102, 103, 104, 105)


def scenes():
    return [scene(s, 2000) for s in SCENE_SEEDS]


def mask_with_holes(P, seed=7):
    m = np.random.default_rng(seed).random(P) < 0.7
    if P:
        m[0] = False
    return m


def host_detail(E, x0, x1):
    R1, R2, t = pose.decompose_essential(np.asarray(E, dtype=np.float64))
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    q3, z0, z1 = [], [], []
    for R, tt in cands:
        Q = pose_math._triangulate(np.eye(3, 4), np.concatenate([R, tt[:, None]], 1), x0, x1)
        w = np.where(np.abs(Q[:, 3]) > 1e-300, Q[:, 3], 1e-300)
        X = Q[:, :3] / w[:, None]
        q3.append(Q[:, 3]), z0.append(X[:, 2]), z1.append((X @ R.T + tt)[:, 2])
    return cands, np.array(q3).reshape(4, -1), np.array(z0).reshape(4, -1), np.array(z1).reshape(4, -1)


def decidable(E, x0, x1, dthr=1e9):
    """[P] bool: the point is decidable under ALL four candidates, in the host recover_pose's own fp64 values: |Q[3]| >= 1e-6 for the
    unit null vector, 1e-6 <= |z0|, |z1| <= 1e8, both depths at least 1e-6 away from the distance threshold"""
    _, q3, z0, z1 = host_detail(E, x0, x1)
    ok = np.abs(q3) >= 1e-6
    for z in (z0, z1):
        ok &= (np.abs(z) >= 1e-6) & (np.abs(z) <= 1e8) & (np.abs(z - dthr) >= 1e-6)
    return ok.all(0)


def same_pose(Ra, ta, Rb, tb, bar=RT_BAR):
    return float(np.abs(Ra - Rb).max()) <= bar and float(np.abs(ta - tb).max()) <= bar


def match_candidates(ge_cands, host_cands):
    """the permutation that maps the device's candidate order to the host's (LAPACK may exchange R1 / R2 and negate t):
    perm[j] = the host candidate nearest to device candidate j; it must be a permutation"""
    perm = []
    for R, t in ge_cands:
        d = [max(np.abs(R - Rh).max(), np.abs(t - th).max()) for Rh, th in host_cands]
        perm.append(int(np.argmin(d)))
    assert sorted(perm) == [0, 1, 2, 3], perm
    return perm


@functools.lru_cache(maxsize=None)
def behind_scene(P=200, seed=11):
    """every match triangulates behind a camera under every candidate.  A match on the epipolar geometry is in front of both cameras
    under exactly one of the four candidates, so these are matches off it: uniform pairs of [-1, 1]^2, kept when the HOST's own
    values (`host_detail`) put them behind a camera under all four candidates, decidably -> (E, x0, x1 [P,2])"""
    E = scene(seed, 1)[0]
    rng = np.random.default_rng(seed)
    x0, x1 = rng.uniform(-1, 1, (40 * P, 2)), rng.uniform(-1, 1, (40 * P, 2))
    _, _, z0, z1 = host_detail(E, x0, x1)
    keep = np.flatnonzero(~((z0 > 0) & (z1 > 0)).any(0) & decidable(E, x0, x1))[:P]
    assert len(keep) == P
    return E, x0[keep], x1[keep]


def ragged_batch():
    """B = 4 with (300, 0, 257, 64) points, E[3] zero, a mask with holes -> (E [4,3,3], x0, x1 [621,2], offsets int32 [5], mask [621])"""
    sizes = (300, 0, 257, 64)
    parts = [scene(200 + b, n) for b, n in enumerate(sizes)]
    E = np.stack([p[0] for p in parts])
    E[3] = 0.0
    x0 = np.concatenate([p[1] for p in parts])
    x1 = np.concatenate([p[2] for p in parts])
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return E, x0, x1, offsets, mask_with_holes(int(offsets[-1]))


def to_pixels(x):
    return x * K_PIX[[0, 1], [0, 1]] + K_PIX[[0, 1], [2, 2]]


def ransac_pairs():
    """pixel matches for the zeb tests: a 300-match and a 120-match scene (30 % outliers), a pair of four matches (no RANSAC) and a
    pair of eight coincident matches (every five-point sample is refused: no model) -> [(kpts0, kpts1, K0, K1)]"""
    out = []
    for seed, P in ((301, 300), (302, 120)):
        _, x0, x1, _, _ = scene(seed, P, outliers=0.3)
        out.append((to_pixels(x0), to_pixels(x1), K_PIX, K_PIX))
    _, x0, x1, _, _ = scene(303, 4, outliers=0.0)
    out.append((to_pixels(x0), to_pixels(x1), K_PIX, K_PIX))
    out.append((np.tile(to_pixels(x0[:1]), (8, 1)), np.tile(to_pixels(x1[:1]), (8, 1)), K_PIX, K_PIX))
    return out
