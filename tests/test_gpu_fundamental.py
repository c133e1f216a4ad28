"""GPU tests of the fused fundamental-matrix RANSAC step (gim_amd/csrc/fundamental.hip, ops.fundamental_step,
pose.find_fundamental_mat(solve="device"), pose.find_fundamental_mat_batch, the demo's --ransac-solve) against the host:
pose.seven_point_ge for validity and models (the same arithmetic apart from FMA contraction), the fp64 numpy Sampson oracle of
tests/fundamental_cases.py and the merged scorer ops.ransac_score for counts.  Inputs: tests/fundamental_cases.py, whose caps
tests/test_fundamental_cpu.py checks with the host code alone.

Bars.  Validity: equal to the host's flags on every sample outside the band (a factor 10 around each threshold of the solver).  Models:
sin-distance to the host model of the same slot at most 1e-9, and the residual bar of the CPU test (8 x pose.seven_point's own maximum
on the same samples, floored at 1e-15).  Counts: EXACTLY the oracle's on the device's own models, after checking that no error lies
within 1e-9 relative of thr2, and exactly ops.ransac_score's."""
import os

import numpy as np
import pytest
import torch

import fundamental_cases as C
from gim_amd import ops, pose
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = (C.ROW_REPEAT, C.ROW_PAST, C.ROW_NEG, C.ROW_PLANAR, C.ROW_COLLINEAR, C.ROW_COINCIDE)


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def step():
    """one launch over the three pairs of the step case, shared by the tests below -> (case, models, valid, counts) as numpy"""
    case = C.step_case()
    m, v, c = ops.fundamental_step(d(case.x0), d(case.x1), d(case.idx), C.THR2, offsets=d(case.offsets))
    assert m.shape == (3, 257, 3, 3, 3) and v.shape == (3, 257, 3) and c.shape == (3, 257, 3)
    assert m.dtype == torch.float64 and v.dtype == torch.bool and c.dtype == torch.int32
    return case, m.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy()


def test_step_validity_against_the_host(step):
    case, m, v, c = step
    assert not v[1].any() and not m[1].any() and not c[1].any()                       # the empty pair: every index is outside it
    for b in (0, 2):
        keep = ~case.band[b]
        assert np.array_equal(v[b][keep], case.valid[b][keep]), np.flatnonzero((v[b] != case.valid[b]).any(1) & keep)
        for row in PLANTED:
            assert not v[b, row].any() and not m[b, row].any() and not c[b, row].any(), (b, row)
        assert not m[b][~v[b]].any() and not c[b][~v[b]].any()                         # an invalid slot: zero matrix, count 0


def test_step_models_against_the_host(step):
    """every valid device model against the host model of the same slot, and the residual bar of the CPU test on the device's models.
    First GPU run (MI355X), 1 259 models: sin-distance to the host at most 2.235e-12; epipolar residual seven_point 8.066e-17, device
    8.674e-19; |det F| seven_point 1.841e-19, device 2.984e-19."""
    case, m, v, c = step
    worst_sin, worst = 0.0, {"svd": [0.0, 0.0], "dev": [0.0, 0.0]}
    n = 0
    for b in (0, 2):
        a, x = case.pair(b)
        both = v[b] & case.valid[b] & ~case.band[b][:, None]
        worst_sin = max(worst_sin, C.sin_dist(m[b], case.models[b])[both].max())
        nrm = np.linalg.norm(m[b].reshape(-1, 9), axis=-1)[v[b].reshape(-1)]
        assert np.abs(nrm - 1.0).max() <= 1e-14
        keep = both.any(1)
        idx = case.idx[b][keep]
        Fs, vs = pose.seven_point(a[idx], x[idx])
        for name, F, ok in (("svd", Fs, vs), ("dev", m[b][keep], both[keep])):
            r, det = C.residuals(F, a[idx], x[idx])
            worst[name][0], worst[name][1] = max(worst[name][0], r[ok].max()), max(worst[name][1], det[ok].max())
        n += int(both.sum())
    print(f"{n} models: sin-distance to the host {worst_sin:.3e}; residual svd {worst['svd'][0]:.3e} device {worst['dev'][0]:.3e}; "
          f"|det| svd {worst['svd'][1]:.3e} device {worst['dev'][1]:.3e}")
    assert n > 900 and worst_sin <= 1e-9
    assert worst["dev"][0] <= max(8.0 * worst["svd"][0], 1e-15) and worst["dev"][1] <= max(8.0 * worst["svd"][1], 1e-15)


def test_step_counts_against_the_oracle_and_the_merged_scorer(step):
    case, m, v, c = step
    for b in (0, 2):
        a, x = case.pair(b)
        e = C.sampson(m[b][v[b]], a, x)
        assert int((np.abs(e - C.THR2) <= 1e-9 * C.THR2).sum()) == 0                   # the condition for exact equality
        want = (e <= C.THR2).sum(1)
        assert np.array_equal(c[b][v[b]], want) and want.max() > 15 and (want >= 7).all()
    score = ops.ransac_score(d(m.reshape(3, 257 * 3, 3, 3)), d(case.x0), d(case.x1), C.THR2, valid=d(v.reshape(3, 257 * 3)),
                             offsets=d(case.offsets))
    assert np.array_equal(score.cpu().numpy().reshape(3, 257, 3), c)


def test_tiny_case():
    x0, x1, idx, F, valid, info, band = C.tiny_case()
    m, v, c = ops.fundamental_step(d(x0), d(x1), d(idx), C.THR2)
    m, v, c = m.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy()
    assert m.shape == (1, 3, 3, 3) and np.array_equal(v, valid) and v.any()
    assert (C.sampson(m[0][v[0]], x0, x1) <= 1e-12).all() and (c[0][v[0]] == 7).all() and not c[0][~v[0]].any()
    assert C.sin_dist(m[0], F[0])[v[0]].max() <= 1e-9


def test_one_pair_form_equals_the_batched_call(step):
    case, m, v, c = step
    for b, K in ((0, 257), (2, 257), (2, 1), (0, 3)):
        a, x = case.pair(b)
        one = ops.fundamental_step(d(a), d(x), d(case.idx[b, :K]), C.THR2)
        assert one[0].shape == (K, 3, 3, 3) and one[1].shape == (K, 3) and one[2].shape == (K, 3)
        assert np.array_equal(one[0].cpu().numpy(), m[b, :K]) and np.array_equal(one[1].cpu().numpy(), v[b, :K])
        assert np.array_equal(one[2].cpu().numpy(), c[b, :K])


def test_empty_problems_and_refusals():
    case = C.step_case()
    e2 = torch.empty(0, 2, dtype=torch.float64, device=DEV)
    m, v, c = ops.fundamental_step(d(case.x0), d(case.x1), torch.empty(0, 7, dtype=torch.int32, device=DEV), C.THR2)
    assert m.shape == (0, 3, 3, 3) and v.shape == (0, 3) and c.shape == (0, 3)
    m, v, c = ops.fundamental_step(e2, e2, d(case.idx[0, :5]), C.THR2)                  # no points: nothing is valid
    assert not v.any() and not m.any() and not c.any()
    with pytest.raises(GimHipError):
        ops.fundamental_step(d(case.x0), d(case.x1), d(case.idx[0].astype(np.int64)), C.THR2)
    with pytest.raises(GimHipError):
        ops.fundamental_step(d(case.x0), d(case.x1), d(case.idx[0, :, :4]), C.THR2)
    with pytest.raises(GimHipError):
        ops.fundamental_step(d(case.x0), d(case.x1[:10]), d(case.idx[0]), C.THR2)
    with pytest.raises(GimHipError):
        ops.fundamental_step(d(case.x0), d(case.x1), d(case.idx), C.THR2, offsets=d(np.array([0, 1000, 900, 1065], dtype=np.int32)))
    with pytest.raises(GimHipError):
        ops.fundamental_step(torch.from_numpy(case.x0.copy()), d(case.x1), d(case.idx[0]), C.THR2)


def test_find_fundamental_mat_on_the_device():
    """the decidable scene of the CPU test: the mask is the truth and equals ops.ransac_mask of the returned F"""
    Ft, p0, p1, truth = C.ransac_scene()
    F, mask = pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=0, device=DEV, solve="device")
    assert mask.dtype == bool and np.array_equal(mask, truth)
    dist = float(C.sin_dist(F, Ft))
    print(f"sin-distance of the RANSAC model to the truth {dist:.3e}")
    assert dist < 1e-8
    assert np.array_equal(ops.ransac_mask(d(F), d(p0), d(p1), 1.0).cpu().numpy(), mask)
    F6, m6 = pose.find_fundamental_mat(p0[:6], p1[:6], device=DEV, solve="device")
    assert F6 is None and m6.shape == (6,) and not m6.any()


def test_batch_equals_the_single_calls():
    pairs = C.batch_pairs()
    got = pose.find_fundamental_mat_batch(pairs, 1.0, 0.999999, 10000, seed=0, device=DEV)
    assert len(got) == 5 and got[1][0] is None and got[1][1].shape == (6,) and not got[1][1].any()
    assert got[2][0] is not None and got[2][1].all() and got[2][1].shape == (7,)
    for (p0, p1), (F, mask) in zip(pairs, got):
        F1, m1 = pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=0, device=DEV, solve="device")
        assert (F is None) == (F1 is None) and (F is None or np.array_equal(F, F1)) and np.array_equal(mask, m1)
    assert np.array_equal(got[0][1], C.ransac_scene()[3])
    ver = pose.verify_pairs(pairs, threshold=1.0, device=DEV, batch=2)                  # chunks of 2, 2, 1: the same results
    for (F, mask), (F2, m2) in zip(got, ver):
        assert (F is None) == (F2 is None) and (F is None or np.array_equal(F, F2)) and np.array_equal(mask, m2)
    assert pose.find_fundamental_mat_batch([], device=DEV) == []


def test_demo_ransac_solve_device():
    """match_pair of the demo on its images with the seeded init of gim_dkm (a dense matcher samples its matches, so a seeded init has
    enough of them for the geometry filter; 400 here): `ransac_solve="device"` names its backend and returns a mask over the matches
    with at least the seven points of the winning sample; the default call is what it was (same matches, the host backend's name,
    the model and mask of pose.find_fundamental_mat's default path)"""
    from gim_amd import demo
    a1, a2 = (os.path.join(ROOT, "tests", "golden", "demo", n) for n in ("a1.png", "a2.png"))
    torch.manual_seed(0)
    model, detector = demo.build("gim_dkm", None, None)
    torch.manual_seed(7)
    base = demo.match_pair("gim_dkm", model, detector, a1, a2, num=400)
    torch.manual_seed(7)
    dev = demo.match_pair("gim_dkm", model, detector, a1, a2, num=400, ransac_solve="device")
    n = len(base["mconf"])
    print(f"{n} matches; default backend {base.get('ransac_backend')}, inliers {int(base['inliers'].sum()) if 'inliers' in base else None}; "
          f"device inliers {int(dev['inliers'].sum()) if 'inliers' in dev else None}")
    assert n >= 8 and torch.equal(base["mkpts0_f"], dev["mkpts0_f"]) and torch.equal(base["mkpts1_f"], dev["mkpts1_f"])
    assert dev["ransac_backend"] == "device" and base["ransac_backend"] == pose.backend() != "device"
    assert dev["inliers"].shape == (n,) and dev["inliers"].dtype == bool and dev["inliers"].sum() >= 7 and dev["F"].shape == (3, 3)
    if base["ransac_backend"] == "numpy":
        p0, p1 = base["mkpts0_f"].float().cpu().numpy(), base["mkpts1_f"].float().cpu().numpy()
        F, mask = pose.find_fundamental_mat(p0, p1, threshold=1.0, prob=0.999999, max_iters=10000, device=DEV)
        assert np.array_equal(base["F"], F) and np.array_equal(base["inliers"], mask)
    geom = demo.compute_geom({k: dev[k] for k in ("mkpts0_f", "mkpts1_f")}, device=DEV, ransac_solve="device")
    assert np.array_equal(geom["Fundamental"], dev["F"])
