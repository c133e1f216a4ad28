"""Seeded inputs shared by tests/test_ransac_sampler_cpu.py and tests/test_gpu_ransac_sampler.py: inlier-count arrays for the record
reduction (pose.step_records / gim_ransac_records), whole runs of counts for the bookkeeping, and the two-view scenes of the
end-to-end tests.  Nothing here touches a device; every case is built once and frozen."""
import functools

import numpy as np

import essential_cases as EC
import fundamental_cases as FC
import homography_oracle as HO

K = 257                          # one sample more than a 256-lane chunk


@functools.lru_cache(maxsize=None)
def count_case(k):
    """counts int32 [6, K, k], nb [6], floor [6] for k models per sample.  Pair 0: random small counts with many slot ties and equal
    maxima across samples; pair 1: a strictly increasing run of 40 records (more than one read-back of 32), then
    smaller counts; pair 2: records on both sides of the 256-lane chunk edge and of every 64-lane wave edge; pair 3: a floor above
    every count; pair 4: nb = 100 < K with larger counts beyond nb that must not be seen; pair 5: nb = 0."""
    rng = np.random.default_rng(40 + k)
    c = rng.integers(0, 12, (6, K, k)).astype(np.int32)
    c[0, 5] = c[0, 5].max()                                     # every slot of a sample ties
    c[0, 9] = c[0, 5]                                           # and a later sample equals it: no record
    c[1] = rng.integers(0, 5, (K, k))
    run = 50 + np.arange(40)
    c[1, 10:50, k - 1] = run                                    # the last slot wins
    c[1, 10:50, 0] = np.where(np.arange(40) % 2 == 0, run, 0) if k > 1 else run   # every other sample: slot 0 ties, argmax is 0
    c[1, 60:, :] = np.minimum(c[1, 60:, :], 89)
    c[2] = 0
    for i, s in enumerate((0, 63, 64, 127, 128, 191, 192, 255, 256)):
        c[2, s, i % k] = 20 + i
    c[3] = rng.integers(0, 30, (K, k))
    c[4, 100:] += 1000
    nb = np.array([K, K, K, K, 100, 0], dtype=np.int32)
    floor = np.array([6, 6, 3, 30, 4, 6], dtype=np.int32)
    for a in (c, nb, floor):
        a.setflags(write=False)
    return c, nb, floor


def check_records(rec, ref):
    """the specified part of two record buffers [B, 1 + 3 K] agrees: n_rec and the first n_rec triples of every pair"""
    rec, ref = np.asarray(rec), np.asarray(ref)
    assert rec.shape == ref.shape and rec.dtype == np.int32
    assert np.array_equal(rec[:, 0], ref[:, 0]), (rec[:, 0], ref[:, 0])
    for b in range(len(ref)):
        n = 1 + 3 * int(ref[b, 0])
        assert np.array_equal(rec[b, :n], ref[b, :n]), (b, rec[b, :n], ref[b, :n])


@functools.lru_cache(maxsize=None)
def run_cases():
    """whole runs for the bookkeeping: (name, P, m, conf, max_iters, counts [N, k]) with counts[n] those of sample number n"""
    rng = np.random.default_rng(50)
    out = []
    low = rng.integers(0, 40, (1100, 3))
    out.append(("no shrinking, max_iters = 1100 is no multiple of 250", 2000, 7, 0.999999, 1100, low))
    c = rng.integers(0, 40, (1000, 10))
    c[30, 4] = 1900            # 95 % inliers: the bound drops to a few samples inside the first step ...
    c[100, 2] = 1950           # ... so this larger count is never reached
    out.append(("the bound shrinks inside the first step", 2000, 5, 0.999, 1000, c))
    c = rng.integers(0, 20, (10000, 3))
    c[300:340, 1] = 600 + 10 * np.arange(40)                    # 40 records in a row in the second step
    c[300:340:2, 0] = c[300:340:2, 1]                           # with slot ties
    c[700, 2] = c[339, 1]                                       # an equal maximum later: not a record
    out.append(("a strictly increasing run longer than 32, ties", 2000, 7, 0.999999, 10000, c))
    out.append(("a floor above every count", 2000, 7, 0.999999, 600, rng.integers(0, 7, (600, 3))))
    c = rng.integers(0, 3, (500, 1))
    c[260] = 300               # every point an inlier: den < 1e-12, the run ends at this sample
    out.append(("all points are inliers in the second step", 300, 4, 0.999999, 500, c))
    c = rng.integers(0, 30, (2000, 10))
    c[249, 9], c[250, 0], c[499, 3] = 500, 700, 900             # records on the step edges
    out.append(("records on the step edges", 2000, 5, 0.999, 2000, c))
    for _, _, _, _, _, a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def quality_run_cases():
    """whole runs for the quality walk (score="magsac"), k = 3: {name: (P, m, conf, max_iters, counts [N, 3], quality int64 [N, 3], the
    best (sample, slot) and final bound that the plant implies)}.  The background is ineligible (counts below m) with large random
    qualities, so only the planted samples can be accepted."""
    rng = np.random.default_rng(51)
    out = {}

    def background(N, m):
        return rng.integers(0, m, (N, 3)), rng.integers(1, 1 << 60, (N, 3)).astype(np.int64)

    # two samples of equal quality: the earlier one is kept (strictly above)
    c, q = background(300, 7)
    c[20, 1], q[20, 1] = 100, 1 << 40
    c[60, 2], q[60, 2] = 120, 1 << 40
    out["two samples of equal quality"] = (2000, 7, 0.999999, 300, c, q, (20, 1), 300)
    # the highest quality sits in a slot with count < m; another slot of that sample is eligible
    c, q = background(300, 7)
    c[30], q[30] = (3, 0, 50), (1 << 61, 5, 1 << 30)
    out["the highest quality is ineligible"] = (2000, 7, 0.999999, 300, c, q, (30, 2), 300)
    # the accepted slot is not the slot with the most inliers: the bound comes from 1 200 inliers (487), not from 1 900 (a dozen)
    c, q = background(600, 7)
    c[40], q[40] = (1200, 1900, 0), (1 << 35, 1 << 30, 7)
    out["the accepted slot has fewer inliers than another"] = (2000, 7, 0.999999, 600, c, q, (40, 0), 487)
    # the bound shrinks inside the first step to before a better later sample
    c, q = background(500, 5)
    c[30, 1], q[30, 1] = 1900, 1 << 40
    c[100, 2], q[100, 2] = 1950, 1 << 45
    out["the bound shrinks inside the first step"] = (2000, 5, 0.999, 500, c, q, (30, 1), 31)
    # c == P: den < 1e-12, the run ends at that sample
    c, q = background(500, 4)
    c[260, 0], q[260, 0] = 300, 1 << 40
    out["all points are inliers in the second step"] = (300, 4, 0.999999, 500, c, q, (260, 0), 261)
    # max_iters is no multiple of 250, increasing records across the step edges
    c, q = background(610, 7)
    for i, s in enumerate((5, 249, 250, 499, 500, 609)):
        c[s, i % 3], q[s, i % 3] = 20 + i, (1 << 40) + i
    out["max_iters = 610 is no multiple of 250"] = (2000, 7, 0.999999, 610, c, q, (609, 2), 610)
    for case in out.values():
        case[4].setflags(write=False), case[5].setflags(write=False)
    return out


# ---- scenes of the end-to-end tests ------------------------------------------------------------------------------------------------
def _outliers(rng, b, share, lo, hi):
    out = rng.random(len(b)) < share
    b[out] = rng.uniform(lo, hi, (int(out.sum()), 2))
    return b


@functools.lru_cache(maxsize=None)
def scenes(kind):
    """kind "F" (pixels), "E" (normalised coordinates) or "H" (pixels) -> {name: (a, b)}: 2 000 matches with 50 % outliers, a 95 %-inlier
    scene (the bound shrinks inside the first step), an all-outlier scene, fewer points than a sample, and an empty pair"""
    rng = np.random.default_rng({"F": 61, "E": 62, "H": 63}[kind])
    m = {"F": 7, "E": 5, "H": 4}[kind]

    def make(n, share):
        if kind == "F":
            a, b, _ = FC.two_views(rng, n)
            return a, _outliers(rng, b + rng.normal(size=(n, 2)) * 0.3, share, [0.0, 0.0], [640.0, 480.0])
        if kind == "E":
            a, b, _ = EC.two_views(rng, n)
            return a, _outliers(rng, b + rng.normal(size=(n, 2)) * 2e-4, share, [-0.64, -0.48], [0.64, 0.48])
        H = HO.general_h(rng)
        a = rng.uniform([0, 0], [HO.W, HO.H_IMG], (n, 2))
        return a, _outliers(rng, HO.proj(H, a) + rng.normal(size=(n, 2)) * 0.3, share, [0.0, 0.0], [HO.W, HO.H_IMG])

    out = {"half outliers": make(2000, 0.5), "mostly inliers": make(400, 0.05), "all outliers": make(120, 1.0)}
    few = make(m - 1, 0.0)
    out["fewer than a sample"] = few
    out["empty"] = (np.zeros((0, 2)), np.zeros((0, 2)))
    for a, b in out.values():
        a.setflags(write=False), b.setflags(write=False)
    return out


THRESHOLD = {"F": 1.0, "E": EC.THR, "H": 1.0}
