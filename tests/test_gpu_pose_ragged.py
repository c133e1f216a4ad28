"""GPU test of the pose entry ladder at the smallest ragged batch: for each of E, F and H the pairs of 0, m - 1, m, m + 1 and 40
points (exact correspondences of the case builders, a few outliers in the 40-point pair) with max_iters = 500 -- the sizes at which
the control-block layout of `pose._ransac_on_device`, the offsets and the walk's first and last record can go wrong.  With
sampler="device" the batch equals, byte for byte, the single-pair call of every pair and the sampler="philox" run on the same
device; for F and H also with score="magsac".  Homographies have no public batch call: their batch is the driver itself and their
philox run the loop underneath `find_homography` (which would re-fit)."""
import functools

import numpy as np
import pytest

import essential_cases as EC
import fundamental_cases as FC
import homography_oracle as HO
from gim_amd import pose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, ITERS = 0x9E3779B97F4A7C15, 500
M = {"E": 5, "F": 7, "H": 4}
THR = {"E": EC.THR, "F": 1.0, "H": 1.0}


@functools.lru_cache(maxsize=None)
def pairs(kind):
    rng = np.random.default_rng({"E": 71, "F": 72, "H": 73}[kind])
    m, out = M[kind], []
    for n in (0, m - 1, m, m + 1, 40):
        if kind == "H":
            a = rng.uniform([0, 0], [HO.W, HO.H_IMG], (max(n, 1), 2))
            b = HO.proj(HO.general_h(rng), a)
        else:
            a, b, _ = (EC if kind == "E" else FC).two_views(rng, max(n, 1))
        a, b = a[:n], b[:n]
        if n == 40:
            b = b.copy()
            b[:5] = b[:5][::-1] + (0.05 if kind == "E" else 30.0)          # five gross outliers
        out.append((np.ascontiguousarray(a), np.ascontiguousarray(b)))
    return out


def _band(score):
    return None if score == "count" else THR["H"] ** 2


def run_batch(kind, ps, sampler, score):
    if kind == "E":
        return pose.find_essential_mat_batch(ps, THR[kind], max_iters=ITERS, seed=SEED, device=DEV, solve="device", sampler=sampler)
    if kind == "F":
        return pose.find_fundamental_mat_batch(ps, THR[kind], max_iters=ITERS, seed=SEED, device=DEV, sampler=sampler, score=score)
    if sampler == "device":
        return pose._ransac_on_device(ps, pose.DeviceHomography, THR[kind], 0.999999, ITERS, SEED, DEV, max_thr2=_band(score))[0]
    out = []
    for a, b in ps:                                    # sampler="philox": the loop underneath find_homography, pair by pair
        dev = pose.DeviceHomography(a, b, THR[kind] ** 2, DEV, max_thr2=_band(score)) if len(a) >= 4 else None
        H, mask = pose._ransac(a, b, None, 4, THR[kind], 0.999999, ITERS, None, scorer=dev, solve_idx=dev and dev.solve,
                               error=pose.transfer_error, draw=pose._draw("philox", SEED, len(a), 4), max_thr2=_band(score), kind=0)
        out.append((H, np.asarray(mask, dtype=bool)))
    return out


def run_single(kind, a, b, score):
    if kind == "E":
        return pose.find_essential_mat(a, b, THR[kind], max_iters=ITERS, seed=SEED, device=DEV, solve="device", sampler="device")
    if kind == "F":
        return pose.find_fundamental_mat(a, b, THR[kind], max_iters=ITERS, seed=SEED, device=DEV, solve="device", sampler="device", score=score)
    return run_batch(kind, [(a, b)], "device", score)[0]


def _same(x, y, what):
    (Ma, ma), (Mb, mb) = x, y
    assert (Ma is None) == (Mb is None), what
    assert Ma is None or np.asarray(Ma).tobytes() == np.asarray(Mb).tobytes(), what
    assert ma.dtype == mb.dtype == bool and ma.tobytes() == mb.tobytes(), what


@pytest.mark.parametrize("kind,score", [("E", "count"), ("F", "count"), ("H", "count"), ("F", "magsac"), ("H", "magsac")])
def test_ragged_device_batch_equals_single_calls_and_philox(kind, score):
    ps, m = pairs(kind), M[kind]
    got = run_batch(kind, ps, "device", score)
    philox = run_batch(kind, ps, "philox", score)
    assert len(got) == len(philox) == len(ps)
    for i, ((a, b), r) in enumerate(zip(ps, got)):
        assert r[1].shape == (len(a),) and r[1].dtype == bool
        if len(a) < m:
            assert r[0] is None and not r[1].any(), i
        _same(r, run_single(kind, a, b, score), (kind, score, i, "single"))
        _same(r, philox[i], (kind, score, i, "philox"))
    E, mask = got[-1]
    print(f"{kind} {score}: models {[r[0] is not None for r in got]}, inliers of the 40-point pair {int(mask.sum())}")
    assert E is not None and mask[5:].all() and mask.sum() >= 35          # the planted geometry of the 40-point pair is found
