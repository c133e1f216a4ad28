"""GPU tests of the RANSAC hypothesis scorer (gim_amd/csrc/ransac_score.hip, ops.ransac_score / ops.ransac_mask, pose.DeviceScorer and
the `device=` paths of gim_amd/pose.py and gim_amd/zeb.py) against the host: pose.sampson_error / pose_math._count_inliers in fp64.

Parity bar: counts and masks are EXACTLY the host's.  The device may contract a * b + c into an FMA where numpy rounds twice, so an
error could land on the other side of thr2 only when it is within rounding of it: the module checks on the host that NO
(model, point) error of its inputs lies within relative 1e-9 of thr2 (the cap on such pairs is zero; the seeds below were chosen on
the CPU so that this holds -- another seed is the remedy if an input change breaks it, never a looser comparison)."""
import numpy as np
import pytest
import torch

from gim_amd import ops, pose, pose_math, zeb
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR2 = (0.5 / 500) ** 2
KS, PS = (1, 63, 65, 2500), (5, 7, 64, 65, 257, 2000)


def _rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _scene(rng, n, ang=0.25):
    """tests/test_pose_cpu.py's two-view scene"""
    R = _rot(rng.normal(size=3), ang)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 9, (n, 1))], 1)
    Y = X @ R.T + t
    return R, t, X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]


def _noisy_pair(seed, n, noise, outlier_share=0.5):
    """normalised matches with gross outliers, in random order (a prefix of the points holds both kinds)"""
    rng = np.random.default_rng(seed)
    _, _, x0, x1 = _scene(rng, n)
    x0 = x0 + rng.normal(size=x0.shape) * noise
    x1 = x1 + rng.normal(size=x1.shape) * noise
    no = int(outlier_share * n)
    x1[:no] = rng.uniform(-0.5, 0.5, (no, 2))
    perm = rng.permutation(n)
    return np.ascontiguousarray(x0[perm]), np.ascontiguousarray(x1[perm])


class _Case:
    """2 000 matches (50 % outliers, 1e-3 noise), the 2 500 five-point candidates of 250 samples of them, and every (model, point)
    error from the host -- computed once for the module, never modified"""

    def __init__(self, seed=101):
        self.x0, self.x1 = _noisy_pair(seed, 2000, 1e-3)
        rng = np.random.default_rng(seed + 1)
        idx = np.stack([rng.choice(2000, 5, replace=False) for _ in range(250)])
        E, valid = pose.five_point(self.x0[idx], self.x1[idx])
        self.models, self.valid = np.ascontiguousarray(E.reshape(-1, 3, 3)), valid.reshape(-1)
        self.err = pose.sampson_error(self.models, self.x0, self.x1)                  # [2500, 2000]
        self.d_x0, self.d_x1 = torch.from_numpy(self.x0).to(DEV), torch.from_numpy(self.x1).to(DEV)
        self.d_models, self.d_valid = torch.from_numpy(self.models).to(DEV), torch.from_numpy(self.valid).to(DEV)
        for a in (self.x0, self.x1, self.models, self.valid, self.err):
            a.setflags(write=False)

    def oracle(self, K, P):
        return np.where(self.valid[:K], (self.err[:K, :P] <= THR2).sum(1), 0)


@pytest.fixture(scope="module")
def case():
    return _Case()


def test_no_error_of_the_inputs_is_within_rounding_of_the_threshold(case):
    """the condition under which exact equality is the right bar (module docstring): zero pairs inside the margin"""
    assert case.models.shape == (2500, 3, 3) and 1000 < case.valid.sum() < 2500
    assert int((np.abs(case.err - THR2) <= 1e-9 * THR2).sum()) == 0
    best = case.oracle(2500, 2000).max()
    assert 200 < best < 1100, best                         # the candidates hold a usable model: the counts are not all trivial


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("K", KS)
def test_counts_equal_the_host(case, K, P):
    got = ops.ransac_score(case.d_models[:K], case.d_x0[:P], case.d_x1[:P], THR2, valid=case.d_valid[:K])
    assert got.dtype == torch.int32 and got.shape == (K,)
    want = case.oracle(K, P)
    assert np.array_equal(got.cpu().numpy(), want), (K, P, int((got.cpu().numpy() != want).sum()))
    if K == 2500 and P == 2000:
        assert np.array_equal(want, pose_math._count_inliers(case.models, case.valid, case.x0, case.x1, THR2))
        # without `valid` the rejected candidates (zero matrices) count every point
        allv = ops.ransac_score(case.d_models, case.d_x0, case.d_x1, THR2).cpu().numpy()
        assert np.array_equal(allv, (case.err <= THR2).sum(1)) and (allv[~case.valid] == 2000).all()


def test_invalid_nan_and_zero_models(case):
    K, P = 65, 257
    models, valid = case.models[:K].copy(), np.ones(K, dtype=bool)
    valid[[0, 5, 64]] = False
    models[1, 1, 2] = np.nan
    models[63, 0, 0] = np.nan
    models[2] = 0.0
    models[62] = 0.0
    got = ops.ransac_score(torch.from_numpy(models).to(DEV), case.d_x0[:P], case.d_x1[:P], THR2, valid=torch.from_numpy(valid).to(DEV)).cpu().numpy()
    want = pose_math._count_inliers(models, valid, case.x0[:P], case.x1[:P], THR2)
    assert np.array_equal(got, want)
    assert (got[[0, 5, 64]] == 0).all() and (got[[1, 63]] == 0).all() and (got[[2, 62]] == P).all()
    # counts is fully written: a second call into the same allocation pattern with everything invalid gives zeros
    none = ops.ransac_score(torch.from_numpy(models).to(DEV), case.d_x0[:P], case.d_x1[:P], THR2, valid=torch.zeros(K, dtype=torch.bool, device=DEV))
    assert int(none.abs().sum()) == 0


def test_ragged_batch(case):
    K, sizes = 65, (257, 0, 4)
    starts = (0, 300, 700)
    models = np.ascontiguousarray(np.stack([case.models[0:65], case.models[100:165], case.models[200:265]]))
    valid = np.ascontiguousarray(np.stack([case.valid[0:65], case.valid[100:165], case.valid[200:265]]))
    x0 = np.concatenate([case.x0[s:s + n] for s, n in zip(starts, sizes)])
    x1 = np.concatenate([case.x1[s:s + n] for s, n in zip(starts, sizes)])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    d = lambda a: torch.from_numpy(np.array(a)).to(DEV)   # noqa: E731  (a copy: the shared arrays are read-only)
    got = ops.ransac_score(d(models), d(x0), d(x1), THR2, valid=d(valid), offsets=d(off))
    assert got.shape == (3, K) and got.dtype == torch.int32
    for b, (s, n) in enumerate(zip(starts, sizes)):
        want = pose_math._count_inliers(models[b], valid[b], case.x0[s:s + n], case.x1[s:s + n], THR2)
        assert np.array_equal(got[b].cpu().numpy(), want), b
        one = ops.ransac_score(d(models[b]), d(case.x0[s:s + n]), d(case.x1[s:s + n]), THR2, valid=d(valid[b]))
        assert np.array_equal(one.cpu().numpy(), want), b
    assert int(got[1].abs().sum()) == 0
    # one model per pair -> the concatenated mask
    best = np.stack([models[b][int(got[b].argmax())] for b in range(3)])
    mask = ops.ransac_mask(d(best), d(x0), d(x1), THR2, offsets=d(off)).cpu().numpy()
    want = np.concatenate([pose.sampson_error(best[b], case.x0[s:s + n], case.x1[s:s + n]) <= THR2 for b, (s, n) in enumerate(zip(starts, sizes))])
    assert mask.dtype == bool and np.array_equal(mask, want)
    with pytest.raises(GimHipError):
        ops.ransac_score(d(models), d(x0), d(x1), THR2, offsets=d(np.array([0, 257, 257, 260], dtype=np.int32)))   # does not end at Ptot = 261
    with pytest.raises(GimHipError):
        ops.ransac_score(d(models), d(x0), d(x1), THR2, offsets=d(np.array([0, 257, 200, 261], dtype=np.int32)))   # not monotone


@pytest.mark.parametrize("P", (5, 257, 2000))
def test_mask_equals_the_host(case, P):
    best = case.models[int(case.oracle(2500, 2000).argmax())]
    got = ops.ransac_mask(torch.from_numpy(best.copy()).to(DEV), case.d_x0[:P], case.d_x1[:P], THR2)
    assert got.dtype == torch.bool and got.shape == (P,)
    assert np.array_equal(got.cpu().numpy(), pose.sampson_error(best, case.x0[:P], case.x1[:P]) <= THR2)


def test_empty_problems_return_cleanly(case):
    e2 = torch.empty(0, 2, dtype=torch.float64, device=DEV)
    assert ops.ransac_score(case.d_models[:0], case.d_x0[:64], case.d_x1[:64], THR2).shape == (0,)                      # K == 0
    got = ops.ransac_score(torch.empty(0, 7, 3, 3, dtype=torch.float64, device=DEV), e2, e2, THR2, offsets=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert got.shape == (0, 7)                                                                                         # B == 0
    assert ops.ransac_score(case.d_models[:9], e2, e2, THR2).tolist() == [0] * 9                                        # no points
    assert ops.ransac_mask(case.d_models[0], e2, e2, THR2).shape == (0,)
    assert ops.ransac_mask(torch.empty(0, 3, 3, dtype=torch.float64, device=DEV), e2, e2, THR2, offsets=torch.zeros(1, dtype=torch.int32, device=DEV)).shape == (0,)
    # the C entry points themselves
    assert ops.lib.gim_ransac_score(None, None, None, None, None, 0, 7, THR2, None, None) == 0
    assert ops.lib.gim_ransac_score(None, None, None, None, None, 2, 0, THR2, None, None) == 0
    assert ops.lib.gim_ransac_mask(None, None, None, None, 0, THR2, None, None) == 0


def test_host_tensors_and_wrong_types_are_refused_before_any_launch(case, monkeypatch):
    def no_launch(*a):
        raise AssertionError("launched")
    m, x0, x1 = torch.from_numpy(case.models[:8].copy()), torch.from_numpy(case.x0[:16].copy()), torch.from_numpy(case.x1[:16].copy())

    class Lib:
        gim_ransac_score = gim_ransac_mask = staticmethod(no_launch)
    monkeypatch.setattr(ops, "lib", Lib)
    with pytest.raises(GimHipError):
        ops.ransac_score(m, x0, x1, THR2)
    with pytest.raises(GimHipError):
        ops.ransac_score(m.to(DEV), x0, x1.to(DEV), THR2)
    with pytest.raises(GimHipError):
        ops.ransac_mask(m[0], x0, x1, THR2)
    with pytest.raises(GimHipError):
        ops.ransac_score(m.to(DEV).float(), x0.to(DEV), x1.to(DEV), THR2)                     # fp32 models
    with pytest.raises(GimHipError):
        ops.ransac_score(m.to(DEV), x0.to(DEV).float(), x1.to(DEV).float(), THR2)             # fp32 points
    with pytest.raises(GimHipError):
        ops.ransac_score(m.to(DEV), x0.to(DEV).t().contiguous().t(), x1.to(DEV), THR2)        # not contiguous
    with pytest.raises(GimHipError):
        ops.ransac_score(m.to(DEV), x0.to(DEV), x1.to(DEV)[:8], THR2)                         # point counts differ
    with pytest.raises(GimHipError):
        ops.ransac_score(m.to(DEV), x0.to(DEV), x1.to(DEV), THR2, valid=torch.ones(7, dtype=torch.bool, device=DEV))


# ---- the RANSAC loops with the scorer on the device -----------------------------------------------------------------------------------
def test_find_essential_mat_on_the_device_equals_the_host():
    x0, x1 = _noisy_pair(7, 500, 2e-4)
    E, mask = pose.find_essential_mat(x0, x1, 1e-3, prob=0.99999, seed=3)
    Ed, maskd = pose.find_essential_mat(x0, x1, 1e-3, prob=0.99999, seed=3, device=DEV)
    assert E is not None and 200 < mask.sum() <= 300
    assert np.array_equal(E, Ed) and E.tobytes() == Ed.tobytes()
    assert maskd.dtype == bool and np.array_equal(mask, maskd)
    En, maskn = pose.find_essential_mat(x0[:4], x1[:4], 1e-3, seed=3, device=DEV)
    assert En is None and maskn.shape == (4,) and not maskn.any()


def test_find_fundamental_mat_on_the_device_equals_the_host():
    x0, x1 = _noisy_pair(8, 300, 4e-4, outlier_share=0.3)
    p0, p1 = x0 * 500.0 + [320.0, 240.0], x1 * 480.0 + [300.0, 250.0]
    F, mask = pose.find_fundamental_mat(p0, p1, threshold=1.0, prob=0.999999, max_iters=10000, seed=3)
    Fd, maskd = pose.find_fundamental_mat(p0, p1, threshold=1.0, prob=0.999999, max_iters=10000, seed=3, device=DEV)
    assert F is not None and mask.sum() > 150
    assert F.tobytes() == Fd.tobytes() and np.array_equal(mask, maskd)


def test_find_essential_mat_batch_equals_the_host():
    pairs = [_noisy_pair(11, 400, 2e-4), _noisy_pair(12, 150, 0.0, outlier_share=0.0), tuple(a[:4] for a in _noisy_pair(13, 10, 0.0))]
    got = pose.find_essential_mat_batch(pairs, 1e-3, prob=0.99999, max_iters=1000, seed=3, device=DEV)
    assert len(got) == 3
    for (a, b), (E, mask) in zip(pairs, got):
        Eh, maskh = pose.find_essential_mat(a, b, 1e-3, prob=0.99999, max_iters=1000, seed=3)
        assert (E is None) == (Eh is None) and np.array_equal(mask, maskh) and mask.dtype == bool
        assert E is None or E.tobytes() == Eh.tobytes()
    assert got[0][0] is not None and got[1][1].all() and got[2][0] is None


def test_evaluate_batch_with_the_batched_estimator_gives_the_host_rows(monkeypatch):
    """the synthetic matches of tests/test_pose_cpu.py's end-to-end case, three pairs in one batch"""
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    rng = np.random.default_rng(11)
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    Ts, k0s, k1s, bids = [], [], [], []
    for p in range(3):
        R, t, x0, x1 = _scene(rng, 200, ang=0.15)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        k0 = x0 * 500.0 + [320.0, 240.0]
        k1 = x1 * 500.0 + [320.0, 240.0]
        k1[:40] = rng.uniform(0, 480, (40, 2))
        Ts.append(T), k0s.append(k0), k1s.append(k1), bids.append(np.full(200, p))
    batch = {"scene_id": ["s"] * 3, "pair_names": (["%04d" % p for p in range(3)], ["%04d" % (p + 1) for p in range(3)]),
             "T_0to1": torch.tensor(np.stack(Ts)), "K0": torch.tensor(np.stack([K] * 3)), "K1": torch.tensor(np.stack([K] * 3)),
             "covisible0": [0.5] * 3, "covisible1": [0.5] * 3,
             "mkpts0_f": torch.tensor(np.concatenate(k0s)).to(DEV), "mkpts1_f": torch.tensor(np.concatenate(k1s)).to(DEV),
             "m_bids": torch.tensor(np.concatenate(bids)).to(DEV)}
    host = zeb.evaluate_batch(batch)
    assert len(host) == 3 and all(float(r.split()[3]) < 1.0 for r in host)
    assert zeb.evaluate_batch(batch, estimate_batch=zeb.device_batch_estimator(DEV)) == host
    assert zeb.evaluate_batch(batch, estimate=zeb.device_estimator(DEV)) == host
