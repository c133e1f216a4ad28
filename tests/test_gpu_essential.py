"""GPU tests of the fused essential-matrix RANSAC step (gim_amd/csrc/essential.hip, ops.essential_step,
pose.find_essential_mat(solve="device"), pose.find_essential_mat_batch(solve="device"), the zeb estimators' `solve=`) against the
host: pose.five_point_ge for validity and models (the same arithmetic apart from FMA contraction), the fp64 numpy Sampson oracle of
tests/fundamental_cases.py and the merged scorer ops.ransac_score for counts.  Inputs: tests/essential_cases.py, whose caps
tests/test_essential_cpu.py checks with the host code alone.

Bars.  Validity: equal to the host's flags on every sample outside the band (tests/essential_cases.py: a factor 10 around each
threshold of the solver, a root gap or a discriminant below 1e-6 relative).  Models: sign-aligned Frobenius distance to the host
model of the same slot at most 1e-8 (a perturbation of pose.five_point's inputs by <= 2 ulp moves its models by up to 3.7e-9: 1e-9
would be inside the solver's own conditioning), unit norm to 1e-14, and the residual bars of the CPU test (8 x pose.five_point's own
maximum on the same samples, floored at 1e-15).  Counts: EXACTLY the oracle's on the device's own models, after checking that no
error lies within 1e-9 relative of thr2, and exactly ops.ransac_score's."""
import numpy as np
import pytest
import torch

import essential_cases as C
from gim_amd import ops, pose, zeb
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def step():
    """one launch over the three pairs of the step case, shared by the tests below -> (case, models, valid, counts) as numpy"""
    case = C.step_case()
    m, v, c = ops.essential_step(d(case.x0), d(case.x1), d(case.idx), C.THR2, offsets=d(case.offsets))
    assert m.shape == (3, 257, 10, 3, 3) and v.shape == (3, 257, 10) and c.shape == (3, 257, 10)
    assert m.dtype == torch.float64 and v.dtype == torch.bool and c.dtype == torch.int32
    return case, m.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy()


def test_step_validity_against_the_host(step):
    case, m, v, c = step
    assert not v[1].any() and not m[1].any() and not c[1].any()                       # the empty pair: every index is outside it
    for b in (0, 2):
        keep = ~case.band[b]
        assert np.array_equal(v[b][keep], case.valid[b][keep]), np.flatnonzero((v[b] != case.valid[b]).any(1) & keep)
        for row in C.PLANTED:
            assert not v[b, row].any() and not m[b, row].any() and not c[b, row].any(), (b, row)
        assert not m[b][~v[b]].any() and not c[b][~v[b]].any()                         # an invalid slot: zero matrix, count 0
        assert np.isfinite(m[b]).all()


def test_step_models_against_the_host(step):
    """every valid device model against the host model of the same slot, and the residual bars of the CPU test on the device's
    models.  First GPU run (MI355X), 2 098 models: distance to the host model at most 1.607e-10; epipolar residual five_point
    5.169e-16, device 1.388e-16; cubic residual five_point 1.057e-10, device 2.319e-10."""
    case, m, v, c = step
    worst_d, worst = 0.0, {"svd": [0.0, 0.0], "dev": [0.0, 0.0]}
    n = 0
    for b in (0, 2):
        a, x = case.pair(b)
        both = v[b] & case.valid[b] & ~case.band[b][:, None]
        worst_d = max(worst_d, C.dist(m[b], case.models[b])[both].max())
        nrm = np.linalg.norm(m[b].reshape(-1, 9), axis=-1)[v[b].reshape(-1)]
        assert np.abs(nrm - 1.0).max() <= 1e-14
        keep = both.any(1)
        idx = case.idx[b][keep]
        Es, vs = pose.five_point(a[idx], x[idx])
        for name, E, ok in (("svd", Es, vs), ("dev", m[b][keep], both[keep])):
            r, cub = C.residuals(E, a[idx], x[idx])
            worst[name][0], worst[name][1] = max(worst[name][0], r[ok].max()), max(worst[name][1], cub[ok].max())
        n += int(both.sum())
    print(f"{n} models: distance to the host {worst_d:.3e}; epipolar residual svd {worst['svd'][0]:.3e} device {worst['dev'][0]:.3e}; "
          f"cubic residual svd {worst['svd'][1]:.3e} device {worst['dev'][1]:.3e}")
    assert n > 1200 and worst_d <= 1e-8
    assert worst["dev"][0] <= max(8.0 * worst["svd"][0], 1e-15) and worst["dev"][1] <= max(8.0 * worst["svd"][1], 1e-15)


def test_step_counts_against_the_oracle_and_the_merged_scorer(step):
    case, m, v, c = step
    for b in (0, 2):
        a, x = case.pair(b)
        e = C.sampson(m[b][v[b]], a, x)
        assert int((np.abs(e - C.THR2) <= 1e-9 * C.THR2).sum()) == 0                   # the condition for exact equality
        want = (e <= C.THR2).sum(1)
        assert np.array_equal(c[b][v[b]], want) and want.max() > 15
    score = ops.ransac_score(d(m.reshape(3, 257 * 10, 3, 3)), d(case.x0), d(case.x1), C.THR2, valid=d(v.reshape(3, 257 * 10)),
                             offsets=d(case.offsets))
    assert np.array_equal(score.cpu().numpy().reshape(3, 257, 10), c)


def test_tiny_case():
    x0, x1, idx, Et, E, valid, info, band = C.tiny_case()
    m, v, c = ops.essential_step(d(x0), d(x1), d(idx), C.THR2)
    m, v, c = m.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy()
    assert m.shape == (1, 10, 3, 3) and np.array_equal(v, valid) and v.any()
    assert (C.sampson(m[0][v[0]], x0, x1) <= 1e-12).all() and (c[0][v[0]] == 5).all() and not c[0][~v[0]].any()
    assert C.dist(m[0][v[0]], Et).min() < 1e-9 and C.dist(m[0], E[0])[v[0]].max() <= 1e-8


def test_one_pair_form_equals_the_batched_call(step):
    case, m, v, c = step
    for b, K in ((0, 257), (2, 257), (2, 1), (0, 3)):
        a, x = case.pair(b)
        one = ops.essential_step(d(a), d(x), d(case.idx[b, :K]), C.THR2)
        assert one[0].shape == (K, 10, 3, 3) and one[1].shape == (K, 10) and one[2].shape == (K, 10)
        assert np.array_equal(one[0].cpu().numpy(), m[b, :K]) and np.array_equal(one[1].cpu().numpy(), v[b, :K])
        assert np.array_equal(one[2].cpu().numpy(), c[b, :K])


def test_empty_problems_and_refusals():
    case = C.step_case()
    e2 = torch.empty(0, 2, dtype=torch.float64, device=DEV)
    m, v, c = ops.essential_step(d(case.x0), d(case.x1), torch.empty(0, 5, dtype=torch.int32, device=DEV), C.THR2)
    assert m.shape == (0, 10, 3, 3) and v.shape == (0, 10) and c.shape == (0, 10)
    m, v, c = ops.essential_step(e2, e2, d(case.idx[0, :5]), C.THR2)                    # no points: nothing is valid
    assert not v.any() and not m.any() and not c.any()
    with pytest.raises(GimHipError):
        ops.essential_step(d(case.x0), d(case.x1), d(case.idx[0].astype(np.int64)), C.THR2)
    with pytest.raises(GimHipError):
        ops.essential_step(d(case.x0), d(case.x1), d(case.idx[0, :, :4]), C.THR2)
    with pytest.raises(GimHipError):
        ops.essential_step(d(case.x0), d(case.x1[:10]), d(case.idx[0]), C.THR2)
    with pytest.raises(GimHipError):
        ops.essential_step(d(case.x0), d(case.x1), d(case.idx), C.THR2, offsets=d(np.array([0, 1000, 900, 1065], dtype=np.int32)))
    with pytest.raises(GimHipError):
        ops.essential_step(torch.from_numpy(case.x0.copy()), d(case.x1), d(case.idx[0]), C.THR2)


def test_find_essential_mat_on_the_device(monkeypatch):
    """the decidable scene of the CPU test: the mask is the truth and equals ops.ransac_mask of the returned E; the pose through
    zeb.estimate_pose is the scene's"""
    Et, x0, x1, truth = C.ransac_scene()
    E, mask = pose.find_essential_mat(x0, x1, C.THR, seed=0, device=DEV, solve="device")
    assert mask.dtype == bool and np.array_equal(mask, truth)
    dist = float(C.dist(E, Et))
    print(f"distance of the RANSAC model to the truth {dist:.3e}")
    assert dist < 1e-8
    assert np.array_equal(ops.ransac_mask(d(E), d(x0), d(x1), C.THR2).cpu().numpy(), mask)
    E4, m4 = pose.find_essential_mat(x0[:4], x1[:4], C.THR, device=DEV, solve="device")
    assert E4 is None and m4.shape == (4,) and not m4.any()
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    R, t, inl = zeb.estimate_pose(C.to_pixels(x0), C.to_pixels(x1), C.K_PIX, C.K_PIX, device=DEV, solve="device")
    tn = C.T_TRUE / np.linalg.norm(C.T_TRUE)
    assert np.abs(R - C.R_TRUE).max() < 1e-6 and np.abs(t - tn).max() < 1e-6 and np.array_equal(inl, truth)


def test_batch_equals_the_single_calls(monkeypatch):
    pairs = C.batch_pairs()
    got = pose.find_essential_mat_batch(pairs, C.THR, seed=0, device=DEV, solve="device")
    assert len(got) == 5 and got[1][0] is None and got[1][1].shape == (4,) and not got[1][1].any()
    assert got[2][0] is not None and got[2][1].all() and got[2][1].shape == (5,)
    for (x0, x1), (E, mask) in zip(pairs, got):
        E1, m1 = pose.find_essential_mat(x0, x1, C.THR, seed=0, device=DEV, solve="device")
        assert (E is None) == (E1 is None) and (E is None or np.array_equal(E, E1)) and np.array_equal(mask, m1)
    assert np.array_equal(got[0][1], C.ransac_scene()[3])
    assert pose.find_essential_mat_batch([], C.THR, device=DEV, solve="device") == []
    # the zeb hooks: the batch estimator returns what the single estimator returns per pair
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    pix = [(C.to_pixels(a), C.to_pixels(b), C.K_PIX, C.K_PIX) for a, b in pairs]
    one = zeb.device_estimator(DEV, solve="device")
    many = zeb.device_batch_estimator(DEV, solve="device")(pix)
    assert len(many) == 5 and many[1] is None and zeb.device_batch_estimator(DEV, solve="device")([]) == []
    for p, got_b in zip(pix, many):
        ref = one(*p)
        assert (ref is None) == (got_b is None)
        if ref is not None:
            assert np.array_equal(ref[0], got_b[0]) and np.array_equal(ref[1], got_b[1]) and np.array_equal(ref[2], got_b[2])
