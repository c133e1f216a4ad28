"""GPU tests of the fused homography RANSAC step (gim_amd/csrc/homography.hip, ops.homography_step / ops.homography_mask and
pose.find_homography(device=)) against the host: pose.homography_4pt for validity, numpy.linalg.solve for the solver's residual, the
transfer_error oracle of tests/homography_oracle.py for counts and masks.  Inputs: tests/homography_cases.py, whose caps
tests/test_homography_cpu.py checks with the host code alone.

Bars.  Solver: the backward error of the device's model in the eight normalised equations, |A h - b|_inf / (|[A b]|_inf |(h, 1)|_inf),
at most 8 x the largest such error of numpy.linalg.solve (LAPACK's partial-pivoting elimination: the same algorithm) over the test's
samples; the factor covers the other summation order, FMA contraction and the de-normalisation the stored model went through.
Validity: equal to the host's flags on every sample outside a factor 10 of a threshold.  Counts and masks: EXACTLY the oracle's on the
device's own models, after checking that no error lies within 1e-9 relative of thr2.
Readings of the first GPU run: see `test_solver_residual`."""
import numpy as np
import pytest
import torch

import homography_cases as C
import homography_oracle as O
from gim_amd import ops, pose
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_models_counts(models, valid, counts, src, dst, host_valid, band):
    """validity against the host, counts against the oracle on the device's models; returns the device's flags"""
    assert models.dtype == np.float64 and valid.dtype == bool and counts.dtype == np.int32
    keep = ~band
    assert np.array_equal(valid[keep], host_valid[keep]), np.flatnonzero(valid[keep] != host_valid[keep])
    assert not models[~valid].any() and not counts[~valid].any()
    if valid.any():
        assert (models[valid][:, 2, 2] == 1.0).all()
        e = O.transfer_error(models[valid], src, dst)
        assert int((np.abs(e - C.THR2) <= 1e-9 * C.THR2).sum()) == 0          # the condition for exact equality
        assert np.array_equal(counts[valid], (e <= C.THR2).sum(1))
    return valid


@pytest.mark.parametrize("P", C.PS)
@pytest.mark.parametrize("K", C.KS)
def test_step_one_pair(K, P):
    src, dst, idx, _, host_valid, band, _ = C.single_case(P)
    m, v, c = ops.homography_step(d(src), d(dst), d(idx[:K]), C.THR2)
    assert m.shape == (K, 3, 3) and v.shape == (K,) and c.shape == (K,)
    _check_models_counts(m.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy(), src, dst, host_valid[:K], band[:K])


def test_solver_residual():
    """First GPU run (MI355X), 693 samples: numpy.linalg.solve's largest residual 9.516e-17, the device's 3.594e-16 (ratio 3.78;
    the device's figure includes the de-normalisation its stored model went through, numpy's solution is measured directly)."""
    worst_np, worst_dev, n = 0.0, 0.0, 0
    for P in C.PS:
        src, dst, idx, _, host_valid, band, info = C.single_case(P)
        m, v, _ = ops.homography_step(d(src), d(dst), d(idx), C.THR2)
        m, v = m.cpu().numpy(), v.cpu().numpy()
        use = v & host_valid & ~band
        A, b = C.normalised_systems(info)
        A, b = A[use], b[use]
        sub = {k: info[k][use] for k in ("ss", "sd", "cs", "cd")}
        r_np = C.residual(A, b, np.linalg.solve(A, b[..., None])[..., 0])
        r_dev = C.residual(A, b, C.renormalise(m[use], sub))
        worst_np, worst_dev, n = max(worst_np, r_np.max()), max(worst_dev, r_dev.max()), n + int(use.sum())
    print(f"solver residual over {n} samples: numpy {worst_np:.3e}, device {worst_dev:.3e}, ratio {worst_dev / worst_np:.2f}")
    assert n > 500 and worst_dev <= 8.0 * worst_np, (worst_dev, worst_np)


def test_step_ragged_pairs_with_an_empty_one():
    case = C.step_case()
    for K in C.KS:
        idx = np.ascontiguousarray(case.idx[:, :K])
        m, v, c = ops.homography_step(d(case.src), d(case.dst), d(idx), C.THR2, offsets=d(case.offsets))
        assert m.shape == (3, K, 3, 3) and v.shape == (3, K) and c.shape == (3, K)
        m, v, c = m.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy()
        assert not v[1].any() and not m[1].any() and not c[1].any()                   # the empty pair: every index is outside it
        for b in (0, 2):
            s, t = case.pair(b)
            _check_models_counts(m[b], v[b], c[b], s, t, case.valid[b][:K], case.band[b][:K])
            one = ops.homography_step(d(s), d(t), d(idx[b]), C.THR2)                    # the pair alone: the same bits
            assert np.array_equal(one[0].cpu().numpy(), m[b]) and np.array_equal(one[2].cpu().numpy(), c[b])
    # indices outside a pair are refused per sample, never turned into an address
    bad = case.idx[:, :3].copy()
    bad[2, 0, 1], bad[2, 1, 0], bad[0, 2, 3] = 65, -1, 1000
    m, v, c = ops.homography_step(d(case.src), d(case.dst), d(bad), C.THR2, offsets=d(case.offsets))
    v = v.cpu().numpy()
    assert not v[2, 0] and not v[2, 1] and not v[0, 2] and not m[2, 0].any().item() and int(c[0, 2]) == 0


def test_mask_equals_the_oracle():
    case = C.step_case()
    best = np.zeros((3, 3, 3))
    for b in (0, 2):
        s, t = case.pair(b)
        k = int(np.argmax(np.where(case.valid[b], (O.transfer_error(case.models[b], s, t) <= C.THR2).sum(1), -1)))
        best[b] = case.models[b][k]
    e = np.concatenate([O.transfer_error(best[b], *case.pair(b)) for b in range(3)])
    assert int((np.abs(e - C.THR2) <= 1e-9 * C.THR2).sum()) == 0
    got = ops.homography_mask(d(best), d(case.src), d(case.dst), C.THR2, offsets=d(case.offsets))
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), e <= C.THR2) and 100 < int(got.sum()) < 1065
    for P in C.PS:
        one = ops.homography_mask(d(best[0]), d(case.src[:P]), d(case.dst[:P]), C.THR2)
        assert np.array_equal(one.cpu().numpy(), e[:P] <= C.THR2)
    zero = ops.homography_mask(d(np.zeros((3, 3))), d(case.src), d(case.dst), C.THR2)    # w == 0 everywhere: no inlier
    assert not zero.any()


def test_empty_problems_and_refusals():
    case = C.step_case()
    e2 = torch.empty(0, 2, dtype=torch.float64, device=DEV)
    m, v, c = ops.homography_step(d(case.src), d(case.dst), torch.empty(0, 4, dtype=torch.int32, device=DEV), C.THR2)
    assert m.shape == (0, 3, 3) and v.shape == (0,) and c.shape == (0,)
    m, v, c = ops.homography_step(e2, e2, d(case.idx[0, :5]), C.THR2)                     # no points: nothing is valid
    assert not v.any() and not m.any() and not c.any()
    assert ops.homography_mask(d(np.eye(3)), e2, e2, C.THR2).shape == (0,)
    with pytest.raises(GimHipError):
        ops.homography_step(d(case.src), d(case.dst), d(case.idx[0].astype(np.int64)), C.THR2)
    with pytest.raises(GimHipError):
        ops.homography_step(d(case.src), d(case.dst[:10]), d(case.idx[0]), C.THR2)
    with pytest.raises(GimHipError):
        ops.homography_step(d(case.src), d(case.dst), d(case.idx), C.THR2, offsets=d(np.array([0, 1000, 900, 1065], dtype=np.int32)))
    with pytest.raises(GimHipError):
        ops.homography_mask(d(np.eye(3, dtype=np.float32)), d(case.src), d(case.dst), C.THR2)
    with pytest.raises(GimHipError):
        ops.homography_step(torch.from_numpy(case.src.copy()), d(case.dst), d(case.idx[0]), C.THR2)


def test_find_homography_on_the_device():
    """the decidable scene of the CPU test: the mask is the truth and the corners land within 1e-6 px (the device's trajectory need
    not be the host's: the solvers round differently)"""
    Ht, src, dst, truth = C.ransac_scene()
    H, mask = pose.find_homography(src, dst, 1.0, 0.999999, 10000, seed=0, device=DEV)
    assert mask.dtype == bool and np.array_equal(mask, truth)
    err = O.corner_error(H, Ht)
    print(f"corner error {err:.3e} px")
    assert H[2, 2] == 1.0 and err <= 1e-6
    H3, m3 = pose.find_homography(src[:3], dst[:3], device=DEV)
    assert H3 is None and not m3.any()
    i4 = np.flatnonzero(truth)[[0, 50, 100, 150]]
    H4, m4 = pose.find_homography(src[i4], dst[i4], device=DEV)
    assert H4 is not None and m4.all()
