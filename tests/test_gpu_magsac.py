"""GPU tests of MAGSAC++ scoring (gim_amd/csrc/ransac_score.hip, gim_amd/csrc/ransac_records.hip: ops.magsac_score, ops.ransac_records64,
`score="magsac"` through pose, the video labeller and the demo) against the host: counts and records EXACTLY, qualities within one
quantisation unit per point of pose.magsac_quality (the device's erf / erfc / exp and its fused multiply-adds against numpy's;
2^-33 of gain is 1.2e-10, the two differ by about 1e-15), batches against single calls bit for bit, and end to end
sampler="device" against sampler="philox" on the same device -- the same samples, kernels and inputs, so model bytes and masks
are equal.  Inputs: tests/magsac_cases.py, tests/ransac_sampler_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import label_link_cases as LC
import magsac_cases as MC
import ransac_sampler_cases as C
from gim_amd import _lib, demo, ops, pose, video_labels
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def d(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cases are frozen


# ---- the score kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("P,K", [(0, 256), (1, 1), (63, 255), (64, 256), (65, 257), (257, 255), (2000, 1), (2000, 257)])
def test_score_equals_the_host_restatement(kind, P, K):
    models, valid, a, b = MC.score_case(kind, P, K)
    for max_thr2 in (None, MC.MAX_THR2):
        q, c = ops.magsac_score(kind, d(models), d(a), d(b), MC.THR2, max_thr2, valid=d(valid))
        assert q.shape == (K,) and q.dtype == torch.int64 and c.shape == (K,) and c.dtype == torch.int32
        rq, rc = pose.magsac_quality(kind, models, valid, a, b, MC.THR2, MC.THR2 if max_thr2 is None else max_thr2)
        q, c = q.cpu().numpy(), c.cpu().numpy()
        assert np.array_equal(c, rc)
        dq = np.abs(q - rq).max()
        print(f"kind {kind} P {P} K {K} max_thr2 {max_thr2}: largest |dQ| {dq} units over {P} points, largest quality {rq.max()}")
        assert dq <= P
        assert (q[~valid] == 0).all() and (c[~valid] == 0).all()
        if K > 4:
            assert q[2] == 0 and c[2] == 0 and q[3] == 0 and c[3] == 0              # a NaN entry, an infinite entry
        if P >= 64 and K > 1:
            assert q[0] > 10 * 2 ** 32 and c[0] > 10 and q[1] >= 2 ** 32             # the truth scores; point 0 has r2 == 0 under model 1
    # without the flags every finite model is scored
    q2, c2 = ops.magsac_score(kind, d(models), d(a), d(b), MC.THR2)
    rq, rc = pose.magsac_quality(kind, models, None, a, b, MC.THR2, MC.THR2)
    assert np.array_equal(c2.cpu().numpy(), rc) and np.abs(q2.cpu().numpy() - rq).max() <= P


@pytest.mark.parametrize("kind", [0, 1])
def test_guard_words_and_a_repeated_launch(kind):
    """the entry point itself on padded buffers: nothing outside quality[B*K] and counts[B*K] is written, and the same launch
    repeated gives the same bytes (integer atomics: any order, one sum)"""
    models, valid, a, b = MC.score_case(kind, 257, 257)
    K, G = 257, 16
    dm, dv, da, db = d(models), d(valid.view(np.uint8)), d(a), d(b)
    off = d(np.array([0, 257], dtype=np.int32))
    runs = []
    for _ in range(2):
        q = torch.full((K + 2 * G,), -0x0123456789ABCDEF, dtype=torch.int64, device=DEV)
        c = torch.full((K + 2 * G,), -0x01234567, dtype=torch.int32, device=DEV)
        rc = _lib.lib.gim_magsac_score(kind, dm.data_ptr(), dv.data_ptr(), da.data_ptr(), db.data_ptr(), off.data_ptr(), 1, K, MC.THR2,
                                       MC.THR2, q[G:].data_ptr(), c[G:].data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _lib.lib.gim_last_error()
        torch.cuda.synchronize()
        q, c = q.cpu().numpy(), c.cpu().numpy()
        assert (q[:G] == -0x0123456789ABCDEF).all() and (q[G + K:] == -0x0123456789ABCDEF).all()
        assert (c[:G] == -0x01234567).all() and (c[G + K:] == -0x01234567).all()
        runs.append((q, c))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    ref = ops.magsac_score(kind, dm, da, db, MC.THR2, valid=dv)
    assert np.array_equal(runs[0][0][G:G + K], ref[0].cpu().numpy()) and np.array_equal(runs[0][1][G:G + K], ref[1].cpu().numpy())


@pytest.mark.parametrize("kind", [0, 1])
def test_ragged_batch_equals_its_single_calls(kind):
    """six pairs, one empty and one of a single point, K = 257 models each: bit for bit the single calls (another launch shape,
    another point split, another place in the batch)"""
    sizes = [257, 0, 1, 2000, 65, 63]
    cases = [MC.score_case(kind, P, 257) for P in sizes]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    models, valid = np.stack([m for m, _, _, _ in cases]), np.stack([v for _, v, _, _ in cases])
    a, b = np.concatenate([x for _, _, x, _ in cases]), np.concatenate([x for _, _, _, x in cases])
    q, c = ops.magsac_score(kind, d(models), d(a), d(b), MC.THR2, MC.MAX_THR2, valid=d(valid), offsets=d(offsets))
    assert q.shape == (6, 257) and c.shape == (6, 257)
    again = ops.magsac_score(kind, d(models), d(a), d(b), MC.THR2, MC.MAX_THR2, valid=d(valid), offsets=d(offsets))
    assert torch.equal(q, again[0]) and torch.equal(c, again[1])
    for i, (m, v, x, y) in enumerate(cases):
        q1, c1 = ops.magsac_score(kind, d(m), d(x), d(y), MC.THR2, MC.MAX_THR2, valid=d(v))
        assert torch.equal(q[i], q1) and torch.equal(c[i], c1), i
    assert (q[1] == 0).all() and (c[1] == 0).all() and q[3].max() > 2 ** 36
    # a pair alone at another place of another batch
    q2, _ = ops.magsac_score(kind, d(models[[3, 0]]), d(np.concatenate([cases[3][2], cases[0][2]])), d(np.concatenate([cases[3][3], cases[0][3]])),
                             MC.THR2, MC.MAX_THR2, valid=d(valid[[3, 0]]), offsets=d(np.array([0, 2000, 2257], dtype=np.int32)))
    assert torch.equal(q2[0], q[3]) and torch.equal(q2[1], q[0])


@pytest.mark.parametrize("k", [1, 3, 10])
def test_records64_equal_the_host_restatement(k):
    q, counts, nb, floor_q, min_count = MC.records_case(k)
    rec = ops.ransac_records64(d(q), d(counts), d(nb), d(floor_q), min_count)
    assert rec.shape == (6, 1 + 4 * MC.K_REC) and rec.dtype == torch.int64
    ref = pose.step_records64(q, counts, nb, floor_q, min_count)
    MC.check_records64(rec.cpu().numpy(), ref)
    assert ref[1, 0] >= 40 and ref[2, 0] == 9 and ref[3, 0] == 0 and ref[4, 0] > 0 and ref[5, 0] == 0
    for b in (1, 2):       # one pair alone gives what it gives inside the batch; sequences in place of tensors
        MC.check_records64(ops.ransac_records64(d(q[b:b + 1]), d(counts[b:b + 1]), [int(nb[b])], [int(floor_q[b])], min_count).cpu().numpy(),
                           ref[b:b + 1])
    # the existing reduction still gives its triples
    c3, nb3, floor3 = C.count_case(k)
    C.check_records(ops.ransac_records(d(c3), d(nb3), d(floor3)).cpu().numpy(), pose.step_records(c3, nb3, floor3))


def test_argument_errors_raise_before_a_launch():
    models, valid, a, b = MC.score_case(1, 64, 256)
    q, counts, nb, floor_q, mc = MC.records_case(3)
    for call in (lambda: ops.magsac_score(2, d(models), d(a), d(b), 1.0),
                 lambda: ops.magsac_score(1, d(models), d(a), d(b), 1.0, 0.0),
                 lambda: ops.magsac_score(1, d(models), d(a), d(b), 1.0, float("inf")),
                 lambda: ops.magsac_score(1, d(models).float(), d(a), d(b), 1.0),
                 lambda: ops.magsac_score(1, d(models), d(a), d(b), 1.0, valid=d(valid[:5])),
                 lambda: ops.magsac_score(1, torch.from_numpy(models.copy()), d(a), d(b), 1.0),
                 lambda: ops.ransac_records64(d(q).int(), d(counts), d(nb), d(floor_q), mc),
                 lambda: ops.ransac_records64(d(q), d(counts[:, :5]), d(nb), d(floor_q), mc),
                 lambda: ops.ransac_records64(d(q), d(counts), d(nb), d(floor_q.astype(np.int32)), mc)):
        with pytest.raises(GimHipError):
            call()
    a, b = C.scenes("F")["mostly inliers"]
    for call in (lambda: pose.find_fundamental_mat(a, b, device=DEV, solve="device", sampler="host", score="magsac"),
                 lambda: pose.find_homography(a, b, device=DEV, score="magsac"),
                 lambda: pose.verify_pairs([(a, b)], device=DEV, sampler="device", score="magsac", max_threshold=-1.0),
                 lambda: pose.find_fundamental_mat_batch([(a, b)], device=DEV, sampler="device", score="sigma")):
        with pytest.raises(ValueError):
            call()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _same(x, y):
    (Ma, ma), (Mb, mb) = x, y
    assert (Ma is None) == (Mb is None)
    assert Ma is None or Ma.tobytes() == Mb.tobytes()
    assert ma.dtype == bool and mb.dtype == bool and np.array_equal(ma, mb)


def _single(kind, a, b, sampler, seed=5, **kw):
    if kind == "F":
        return pose.find_fundamental_mat(a, b, 1.0, 0.999999, 10000, seed=seed, device=DEV, solve="device", sampler=sampler, score="magsac", **kw)
    return pose.find_homography(a, b, 1.0, 0.999999, 10000, seed=seed, device=DEV, sampler=sampler, score="magsac", **kw)


@pytest.mark.parametrize("kind", ["F", "H"])
def test_device_sampler_equals_philox(kind):
    scenes = C.scenes(kind)
    singles = {}
    for name, (a, b) in scenes.items():
        singles[name] = _single(kind, a, b, "device")
        _same(singles[name], _single(kind, a, b, "philox"))
    assert singles["half outliers"][0] is not None and 500 < singles["half outliers"][1].sum() < 1300
    assert singles["mostly inliers"][1].sum() > 250
    assert singles["fewer than a sample"][0] is None and singles["empty"][0] is None and singles["empty"][1].shape == (0,)
    # a wider band is another walk, and the same on both samplers
    a, b = scenes["mostly inliers"]
    _same(_single(kind, a, b, "device", max_threshold=1.5), _single(kind, a, b, "philox", max_threshold=1.5))
    if kind == "H":
        _same(_single(kind, a, b, "device", refit="device"), _single(kind, a, b, "philox", refit="device"))
        return                                               # the homography has no batch entry point
    _same(_single(kind, a, b, "device", refine=2), _single(kind, a, b, "philox", refine=2))
    names = ["mostly inliers", "empty", "half outliers", "fewer than a sample", "all outliers"]
    pairs = [scenes[n] for n in names]
    got = pose.find_fundamental_mat_batch(pairs, 1.0, 0.999999, 10000, seed=5, device=DEV, sampler="device", score="magsac")
    ref = pose.find_fundamental_mat_batch(pairs, 1.0, 0.999999, 10000, seed=5, device=DEV, sampler="philox", score="magsac")
    assert len(got) == 5
    for n, g, r in zip(names, got, ref):
        _same(g, r)
        _same(g, singles[n])
    got = pose.verify_pairs(pairs, device=DEV, seed=5, batch=2, sampler="device", score="magsac", refine=2)
    ref = pose.verify_pairs(pairs, device=DEV, seed=5, batch=2, sampler="philox", score="magsac", refine=2)
    for n, g, r in zip(names, got, ref):
        _same(g, r)
    _same(got[0], _single(kind, *scenes["mostly inliers"], "device", refine=2))
    assert pose.find_fundamental_mat_batch([], device=DEV, sampler="device", score="magsac") == []


def test_no_launch_without_a_sample(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("launched")

    for name in ("ransac_sample", "ransac_records64", "magsac_score", "fundamental_step", "homography_step", "ransac_mask", "homography_mask"):
        monkeypatch.setattr(ops, name, boom)
    a, b = C.scenes("F")["fewer than a sample"]
    assert pose.find_fundamental_mat(a, b, device=DEV, solve="device", sampler="device", score="magsac")[0] is None
    assert pose.find_homography(a[:3], b[:3], device=DEV, sampler="device", score="magsac")[0] is None
    got = pose.verify_pairs([(a, b), (a[:0], b[:0])], device=DEV, sampler="device", score="magsac")
    assert [g[0] for g in got] == [None, None] and [g[1].shape for g in got] == [(6,), (0,)]


def test_the_default_score_is_the_count_walk():
    """score="count" spelled out is the call without it, byte for byte, on the device paths"""
    a, b = C.scenes("F")["mostly inliers"]
    for kw in (dict(solve="device", sampler="device"), dict(solve="device", sampler="philox"), dict(solve="device"), dict()):
        _same(pose.find_fundamental_mat(a, b, seed=3, device=DEV, **kw), pose.find_fundamental_mat(a, b, seed=3, device=DEV, score="count", **kw))
    a, b = C.scenes("H")["mostly inliers"]
    for kw in (dict(sampler="device"), dict()):
        _same(pose.find_homography(a, b, seed=3, device=DEV, **kw), pose.find_homography(a, b, seed=3, device=DEV, score="count", **kw))
    for kw in (dict(sampler="philox"), dict(sampler="device", refit="device"), dict(refit="device")):
        _same(pose.find_homography(a, b, seed=3, device=DEV, **kw), pose.find_homography(a, b, seed=3, device=DEV, score="count", **kw))


@pytest.mark.parametrize("sampler", ["host", "philox", "device"])
def test_the_default_score_of_the_batch_calls(sampler):
    """find_fundamental_mat_batch and verify_pairs on a ragged pair list (an empty pair, one short of a sample, 120 to 2 000
    matches), with and without refine: score="count" spelled out is the call without it, byte for byte"""
    scenes = C.scenes("F")
    pairs = [scenes[n] for n in ("mostly inliers", "empty", "half outliers", "fewer than a sample", "all outliers")]
    for refine in (0, 2):
        kw = dict(seed=3, device=DEV, sampler=sampler, refine=refine)
        plain = pose.find_fundamental_mat_batch(pairs, **kw)
        named = pose.find_fundamental_mat_batch(pairs, score="count", max_threshold=None, **kw)
        assert len(plain) == len(named) == 5 and plain[0][0] is not None and plain[2][0] is not None and plain[1][0] is None
        for x, y in zip(plain, named):
            _same(x, y)
        plain = pose.verify_pairs(pairs, batch=2, **kw)
        named = pose.verify_pairs(pairs, batch=2, score="count", **kw)
        assert len(plain) == len(named) == 5 and plain[0][1].sum() > 250 and plain[3][0] is None
        for x, y in zip(plain, named):
            _same(x, y)


def test_the_default_score_of_the_callers(tmp_path):
    """label_pair, label_pair_list on a device bank, and both calls of the demo's geometry on the device: score="count" /
    ransac_score="count" spelled out is the call without it, byte for byte"""
    k0, k1, _ = LC.pair_scene()
    for kw in (dict(threshold=0.5, max_iters=10000, seed=0), dict(threshold=0.5, max_iters=10000, seed=1, refine=2, affine=LC.AFFINE, vratio=LC.VRATIO)):
        plain = video_labels.label_pair((d(k0), d(k1)), device=DEV, **kw)
        named = video_labels.label_pair((d(k0), d(k1)), device=DEV, score="count", **kw)
        assert len(plain) >= 200 and plain.cpu().numpy().tobytes() == named.cpu().numpy().tobytes()
    frames, segs = MC.video()
    bank = video_labels.FrameBank(len(frames), DEV)
    for i in range(len(frames)):
        bank.put(i, frames[i], seg=segs[i])
    ids = [(0, 2), (1, 3), (2, 5)]
    dirs = {}
    for tag, kw in (("plain", {}), ("count", dict(score="count")), ("magsac", dict(score="magsac"))):
        dirs[tag] = str(tmp_path / tag)
        r = video_labels.label_pair_list(MC.stub_match, bank, ids, "GIM_DKM", dirs[tag], vratio=1.0, exclude=[3], max_iters=500, seed=2, **kw)
        assert r["written"] == ids, (tag, r)
    import os
    assert len(os.listdir(dirs["plain"])) == 5
    for name in sorted(os.listdir(dirs["plain"])):
        assert open(os.path.join(dirs["plain"], name), "rb").read() == open(os.path.join(dirs["count"], name), "rb").read(), name
    for i0, i1 in ids:
        assert 70 <= len(np.load(os.path.join(dirs["magsac"], str(np.array([i0, i1])) + ".npy"))) <= 90      # 80 planted of 100
    a, b = C.scenes("F")["mostly inliers"]
    out = {"mkpts0_f": torch.from_numpy(a).to(DEV), "mkpts1_f": torch.from_numpy(b).to(DEV)}
    for kw in (dict(), dict(ransac_solve="device"), dict(ransac_solve="device", ransac_sampler="philox", ransac_refine=2),
               dict(ransac_solve="device", ransac_sampler="device", homography_refit="device")):
        g0, g1 = demo.compute_geom(out, device=DEV, **kw), demo.compute_geom(out, device=DEV, ransac_score="count", **kw)
        for key in ("Fundamental", "Homography"):
            assert g0[key] is not None and g0[key].tobytes() == g1[key].tobytes(), (kw, key)


# ---- callers -------------------------------------------------------------------------------------------------------------------------
def test_label_pair_with_the_magsac_score():
    """the two-view scene of tests/test_gpu_label_link.py (210 exact matches, 90 outliers, 50 watermarks): the label of
    score="magsac" is label_pack over the mask of the same find_fundamental_mat call, no watermark row survives, and it keeps the
    planted matches as the count run and the host restatement (solve="ge", sampler="philox") do"""
    k0, k1, static = LC.pair_scene()
    kw = dict(threshold=0.5, confidence=0.999999, max_iters=10000, seed=0)
    got = video_labels.label_pair((d(k0), d(k1)), device=DEV, score="magsac", **kw).cpu().numpy()
    base = video_labels.label_pair((d(k0), d(k1)), device=DEV, **kw).cpu().numpy()
    host = video_labels.label_pair_host((k0, k1), score="magsac", **kw)
    print(f"label_pair: {len(got)} rows with score='magsac', {len(base)} with the count, {len(host)} on the host; 210 planted matches")
    moved = video_labels.label_pack_np(k0, k1, moved_thr=1.0)
    Fm, mask = pose.find_fundamental_mat(moved[:, :2].astype(np.float64), moved[:, 2:].astype(np.float64), threshold=0.5, prob=0.999999,
                                         max_iters=10000, seed=0, device=DEV, solve="device", sampler="device", score="magsac")
    assert Fm is not None and got.dtype == np.float32
    assert got.tobytes() == video_labels.label_pack_np(moved[:, :2], moved[:, 2:], keep=mask).tobytes()
    assert not ((np.abs(got[:, :2] - got[:, 2:]) < 1).all(1)).any()
    for rows in (got, base, host):
        assert 200 <= len(rows) <= 230                          # test_gpu_label_link.py's band around the 210 planted matches
    with pytest.raises(ValueError):
        video_labels.label_pair((d(k0), d(k1)), device=DEV, score="usac")


def test_demo_geometry_with_the_magsac_score():
    a, b = C.scenes("F")["mostly inliers"]
    out = {"mkpts0_f": torch.from_numpy(a).to(DEV), "mkpts1_f": torch.from_numpy(b).to(DEV)}
    geom = demo.compute_geom(out, device=DEV, ransac_solve="device", ransac_sampler="device", ransac_score="magsac")
    ref = demo.compute_geom(out, device=DEV, ransac_solve="device", ransac_sampler="philox", ransac_score="magsac")
    for key in ("Fundamental", "Homography"):
        assert geom[key] is not None and geom[key].tobytes() == ref[key].tobytes(), key
    with pytest.raises(ValueError):
        demo.compute_geom(out, device=DEV, ransac_score="magsac")                 # the host sampler
    with pytest.raises(SystemExit):
        demo.main(["--ransac-score", "magsac"])                                     # refused by the parser, before a model is built
    with pytest.raises(SystemExit):
        demo.main(["--ransac-score", "magsac", "--ransac-sampler", "host"])
