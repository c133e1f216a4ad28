"""GPU tests of RANSAC sampling and step reduction on the device (gim_amd/csrc/ransac_sample.hip, gim_amd/csrc/ransac_records.hip,
ops.ransac_sample, ops.ransac_records, `sampler="device"` through pose, zeb and the demo) against the host: pose.device_samples and
pose.step_records EXACTLY (integer arithmetic: there is no tolerance), and end to end sampler="device" against sampler="philox" on the
same device -- the same samples, the same step kernels on the same inputs, so the model bytes and the masks are equal.  Inputs:
tests/ransac_sampler_cases.py."""
import numpy as np
import pytest
import torch

import essential_cases as EC
import ransac_sampler_cases as C
from gim_amd import demo, ops, pose, zeb
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15          # both halves of the key are in use


def d(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cases are frozen


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 5, 7])
def test_sampler_equals_the_host_restatement(m):
    K = 257
    offsets = np.cumsum([0, m, 0, 2000]).astype(np.int32)
    first, count = np.array([0, 2 ** 32 - 100, 7], dtype=np.int64), np.array([257, 0, 100], dtype=np.int32)
    idx = ops.ransac_sample(d(offsets), d(first), d(count), K, m, SEED)
    assert idx.shape == (3, K, m) and idx.dtype == torch.int32 and idx.device == torch.device(DEV)
    want = np.full((3, K, m), -1, dtype=np.int32)
    want[0] = pose.device_samples(SEED, 0, 257, m, m)
    want[2, :100] = pose.device_samples(SEED, 7, 100, 2000, m)
    assert torch.equal(idx.cpu(), torch.from_numpy(want))
    got = idx.cpu().numpy()
    assert (got[1] == -1).all() and (got[2, 100:] == -1).all()                                  # the padding
    assert ((got[0] >= 0) & (got[0] < m)).all() and ((got[2, :100] >= 0) & (got[2, :100] < 2000)).all()
    # ordinals that cross 2^32, a pair short of one sample, the largest point count, sequences in place of tensors
    offsets = np.cumsum([0, 2000, m - 1, m + 1]).astype(np.int32)
    idx = ops.ransac_sample(d(offsets), [2 ** 32 - 100, 0, 5], [257, 257, 256], K, m, SEED).cpu().numpy()
    assert np.array_equal(idx[0], pose.device_samples(SEED, 2 ** 32 - 100, 257, 2000, m)) and (idx[1] == -1).all()
    assert np.array_equal(idx[2, :256], pose.device_samples(SEED, 5, 256, m + 1, m)) and (idx[2, 256] == -1).all()
    big = ops.ransac_sample(2 ** 31 - 1, d(np.array([3], dtype=np.int64)), d(np.array([64], dtype=np.int32)), 64, m, 1)
    assert big.shape == (64, m) and np.array_equal(big.cpu().numpy(), pose.device_samples(1, 3, 64, 2 ** 31 - 1, m))
    # the launch shape does not matter: K = 1 and K = 600 give the same leading samples
    one = ops.ransac_sample(2000, [0], [1], 1, m, SEED).cpu().numpy()
    many = ops.ransac_sample(2000, [0], [600], 600, m, SEED).cpu().numpy()
    assert np.array_equal(one[0], many[0]) and np.array_equal(many, pose.device_samples(SEED, 0, 600, 2000, m))
    assert ops.ransac_sample(2000, [0], [0], 0, m, SEED).shape == (0, m)


@pytest.mark.parametrize("k", [1, 3, 10])
def test_records_equal_the_host_restatement(k):
    counts, nb, floor = C.count_case(k)
    rec = ops.ransac_records(d(counts), d(nb), d(floor))
    assert rec.shape == (6, 1 + 3 * C.K) and rec.dtype == torch.int32
    ref = pose.step_records(counts, nb, floor)
    C.check_records(rec.cpu().numpy(), ref)
    assert ref[1, 0] > 32 and ref[4, 0] > 0 and nb[4] < C.K
    # one pair alone gives what it gives inside the batch; K = 1; sequences in place of tensors
    for b in (1, 2):
        C.check_records(ops.ransac_records(d(counts[b:b + 1]), [int(nb[b])], [int(floor[b])]).cpu().numpy(), ref[b:b + 1])
    tiny = ops.ransac_records(d(counts[0:1, 5:6]), [1], [0]).cpu().numpy()
    C.check_records(tiny, pose.step_records(counts[0:1, 5:6], [1], [0]))
    assert tiny[0, 0] == 1 and tiny[0, 2] == 0                                                   # every slot ties: the lowest


def test_argument_errors_raise_before_a_launch():
    counts, nb, floor = C.count_case(3)
    with pytest.raises(GimHipError):
        ops.ransac_sample(2000, [0], [4], 4, 6, 0)
    with pytest.raises(GimHipError):
        ops.ransac_sample(2000, [0], [4], 4, 5, -1)
    with pytest.raises(GimHipError):
        ops.ransac_sample(2000, [0], [4], 4, 5, 1 << 64)
    with pytest.raises(GimHipError):
        ops.ransac_sample(d(np.array([0, 9], dtype=np.int32)), d(np.array([0], dtype=np.int32)), [4], 4, 5, 0)     # first: int64
    with pytest.raises(GimHipError):
        ops.ransac_sample(d(np.array([0, 9], dtype=np.int32)), [0, 0], [4], 4, 5, 0)                                 # B = 1
    with pytest.raises(GimHipError):
        ops.ransac_sample(torch.tensor([0, 9], dtype=torch.int32), [0], [4], 4, 5, 0)                                # host memory
    with pytest.raises(GimHipError):
        ops.ransac_records(d(counts[..., :2]), d(nb), d(floor))                                                      # k = 2
    with pytest.raises(GimHipError):
        ops.ransac_records(d(counts).long(), d(nb), d(floor))
    with pytest.raises(GimHipError):
        ops.ransac_records(d(counts), d(nb[:3]), d(floor))
    with pytest.raises(GimHipError):
        ops.ransac_records(torch.from_numpy(counts.copy()), d(nb), d(floor))
    _, x0, x1, _ = EC.ransac_scene()
    for call in (lambda: pose.find_essential_mat(x0, x1, EC.THR, device=DEV, sampler="device"),                       # solve="host"
                 lambda: pose.find_fundamental_mat(x0, x1, device=DEV, solve="device", sampler="device", seed=-1),
                 lambda: pose.find_homography(x0, x1, device=DEV, sampler="device", seed=1 << 64),
                 lambda: pose.find_essential_mat_batch([(x0, x1)], EC.THR, device=DEV, sampler="device"),
                 lambda: zeb.device_batch_estimator(DEV, sampler="device")):
        with pytest.raises(ValueError):
            call()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    (Ma, ma), (Mb, mb) = a, b
    assert (Ma is None) == (Mb is None)
    assert Ma is None or Ma.tobytes() == Mb.tobytes()
    assert ma.dtype == bool and mb.dtype == bool and np.array_equal(ma, mb)


def _single(kind, a, b, sampler, seed=5):
    if kind == "F":
        return pose.find_fundamental_mat(a, b, 1.0, 0.999999, 10000, seed=seed, device=DEV, solve="device", sampler=sampler)
    if kind == "E":
        return pose.find_essential_mat(a, b, EC.THR, seed=seed, device=DEV, solve="device", sampler=sampler)
    return pose.find_homography(a, b, 1.0, 0.999999, 10000, seed=seed, device=DEV, sampler=sampler)


@pytest.mark.parametrize("kind", ["F", "E", "H"])
def test_device_sampler_equals_philox(kind):
    scenes = C.scenes(kind)
    singles = {}
    for name, (a, b) in scenes.items():
        singles[name] = _single(kind, a, b, "device")
        _same(singles[name], _single(kind, a, b, "philox"))
    # sanity alone (the comparison above is the test): about 1 000 of 2 000 and 380 of 400 matches are planted inliers
    assert singles["half outliers"][0] is not None and 500 < singles["half outliers"][1].sum() < 1300
    assert singles["mostly inliers"][1].sum() > 250
    assert singles["fewer than a sample"][0] is None and singles["empty"][0] is None and singles["empty"][1].shape == (0,)
    if kind == "H":
        return                                               # the homography has no batch entry point
    batch = {"F": pose.find_fundamental_mat_batch, "E": pose.find_essential_mat_batch}[kind]
    args = dict(F=(1.0, 0.999999, 10000), E=(EC.THR, 0.999, 1000))[kind]
    names = ["mostly inliers", "empty", "half outliers", "fewer than a sample", "all outliers"]
    pairs = [scenes[n] for n in names]
    got = batch(pairs, *args, seed=5, device=DEV, solve="device", sampler="device")
    ref = batch(pairs, *args, seed=5, device=DEV, solve="device", sampler="philox")
    assert len(got) == 5
    for n, g, r in zip(names, got, ref):
        _same(g, r)
        _same(g, singles[n])
    assert batch([], *args, device=DEV, solve="device", sampler="device") == []


def test_no_launch_without_a_sample(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("launched")

    for name in ("ransac_sample", "ransac_records", "fundamental_step", "essential_step", "homography_step", "ransac_mask", "homography_mask"):
        monkeypatch.setattr(ops, name, boom)
    a, b = C.scenes("F")["fewer than a sample"]
    assert pose.find_fundamental_mat(a, b, device=DEV, solve="device", sampler="device")[0] is None
    assert pose.find_essential_mat(a[:4], b[:4], EC.THR, device=DEV, solve="device", sampler="device")[0] is None
    assert pose.find_homography(a[:3], b[:3], device=DEV, sampler="device")[0] is None
    got = pose.verify_pairs([(a, b), (a[:0], b[:0])], device=DEV, sampler="device")
    assert [g[0] for g in got] == [None, None] and [g[1].shape for g in got] == [(6,), (0,)]


def test_public_surface(monkeypatch):
    """verify_pairs, zeb.estimate_pose, both zeb estimators and demo.compute_geom with the device sampler: what the philox sampler
    gives through the same entry point"""
    f, e = C.scenes("F"), C.scenes("E")
    pairs = [f["mostly inliers"], f["fewer than a sample"], f["all outliers"]]
    got = pose.verify_pairs(pairs, device=DEV, seed=2, batch=2, sampler="device")
    ref = pose.verify_pairs(pairs, device=DEV, seed=2, batch=2, sampler="philox")
    for g, r in zip(got, ref):
        _same(g, r)
    assert got[0][1].sum() > 250 and got[1][0] is None
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    pix = [(EC.to_pixels(a), EC.to_pixels(b), EC.K_PIX, EC.K_PIX) for a, b in (e["mostly inliers"], e["fewer than a sample"], e["half outliers"])]
    one = zeb.device_estimator(DEV, solve="device", sampler="device")
    many = zeb.device_batch_estimator(DEV, solve="device", sampler="device")(pix)
    for p, got_b in zip(pix, many):
        ref = zeb.estimate_pose(*p, device=DEV, solve="device", sampler="philox")
        for other in (one(*p), got_b):
            assert (ref is None) == (other is None)
            if ref is not None:
                assert all(np.array_equal(x, y) for x, y in zip(ref, other))
    assert many[1] is None and many[0] is not None and many[0][2].sum() > 250
    a, b = f["mostly inliers"]
    out = {"mkpts0_f": torch.from_numpy(a).to(DEV), "mkpts1_f": torch.from_numpy(b).to(DEV)}
    geom = demo.compute_geom(out, device=DEV, ransac_solve="device", ransac_sampler="device")
    ref = demo.compute_geom(out, device=DEV, ransac_solve="device", ransac_sampler="philox")
    for key in ("Fundamental", "Homography"):
        assert geom[key] is not None and geom[key].tobytes() == ref[key].tobytes(), key
