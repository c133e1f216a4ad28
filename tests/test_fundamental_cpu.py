"""The seven-point half of the fundamental-matrix RANSAC step without a GPU: pose.seven_point_ge (the numpy restatement of
csrc/fundamental_solve.h) on exact synthetic geometry and against the SVD solver pose.seven_point, its validity rules, the host RANSAC
over it, the unchanged default paths, the new export against the header, the kernel's resources, and -- from the host code alone --
that the seeded inputs of tests/test_gpu_fundamental.py keep their caps (tests/fundamental_cases.py builds those inputs for both)."""
import ctypes
import os
import re

import numpy as np
import pytest

import fundamental_cases as C
from gim_amd import pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}


def _clean_samples(seed=31, n=400, P=500):
    """n samples of an exact scene -> (x0s, x1s [n, 7, 2], F truth)"""
    rng = np.random.default_rng(seed)
    x0, x1, F = C.two_views(rng, P)
    idx = np.stack([rng.choice(P, 7, replace=False) for _ in range(n)])
    return x0[idx], x1[idx], F


# ---- the minimal solver ----------------------------------------------------------------------------------------------------------
def test_exact_geometry_is_recovered():
    """400 samples of exact matches of a known F: the solver is valid on every one and one of its <= 3 models is the truth to a
    sin-distance below 1e-8 (exact data in fp64: readings near 1e-12 and below)"""
    x0s, x1s, Ft = _clean_samples()
    F, v, info = pose.seven_point_ge(x0s, x1s, detail=True)
    assert F.shape == (400, 3, 3, 3) and v.shape == (400, 3) and v.dtype == bool
    assert v.any(1).all() and set(v.sum(1).tolist()) <= {1, 3}
    d = np.where(v, C.sin_dist(F, Ft), np.inf).min(1)
    print(f"sin-distance to the truth: max {d.max():.3e}, median {np.median(d):.3e}")
    assert d.max() < 1e-8
    nrm = np.linalg.norm(F.reshape(400, 3, 9), axis=-1)
    assert np.abs(nrm[v] - 1.0).max() <= 1e-14 and not F[~v].any()
    a = info["roots"]
    three = v.all(1)
    assert three.any() and (np.diff(a[three], axis=1) >= 0).all()                      # the slots are ordered by their root


def test_residuals_and_root_counts_against_the_svd_solver():
    """Every sample of the GPU tests' step case outside the band (both non-empty pairs, 50 % outliers: general 7-tuples, not only
    consistent ones): the number of real roots equals pose.seven_point's, and the elimination's residuals stay within 8 x the SVD
    solver's own maximum on the same samples, floored at 1e-15 -- the homography precedent.
    Measured here (numpy, fp64), 499 samples, max over all valid models: epipolar residual on the seven unit-norm rows, seven_point
    8.066e-17, seven_point_ge 6.505e-19; |det F| of the unit-norm model, seven_point 1.841e-19, seven_point_ge 1.415e-18 (7.7 x the
    SVD solver's, and under the 1e-15 floor)."""
    case = C.step_case()
    worst = {"svd": [0.0, 0.0], "ge": [0.0, 0.0]}
    n = 0
    for b in (0, 2):
        a, c = case.pair(b)
        keep = ~case.band[b] & case.info[b]["ok_scale"] & ((case.idx[b] >= 0) & (case.idx[b] < len(a))).all(1)
        keep &= np.array([len(set(r)) == 7 for r in case.idx[b].tolist()])
        keep[[C.ROW_PLANAR, C.ROW_COLLINEAR, C.ROW_COINCIDE]] = False                  # the SVD solver has no rank rule
        keep &= case.info[b]["ok_cubic"]                                               # nor one for a pencil that is singular throughout
        idx = case.idx[b][keep]
        Fs, vs = pose.seven_point(a[idx], c[idx])
        Fg, vg = case.models[b][keep], case.valid[b][keep]
        assert np.array_equal(vs.sum(1), vg.sum(1)), np.flatnonzero(vs.sum(1) != vg.sum(1))
        for name, F, v in (("svd", Fs, vs), ("ge", Fg, vg)):
            r, det = C.residuals(F, a[idx], c[idx])
            worst[name][0] = max(worst[name][0], r[v].max())
            worst[name][1] = max(worst[name][1], det[v].max())
        n += int(keep.sum())
    print(f"{n} samples: residual svd {worst['svd'][0]:.3e} ge {worst['ge'][0]:.3e}; |det| svd {worst['svd'][1]:.3e} ge {worst['ge'][1]:.3e}")
    assert n > 450
    assert worst["ge"][0] <= max(8.0 * worst["svd"][0], 1e-15) and worst["ge"][1] <= max(8.0 * worst["svd"][1], 1e-15)


def test_validity_rules():
    case = C.step_case()
    for b in (0, 2):
        v, info = case.valid[b], case.info[b]
        for row in (C.ROW_REPEAT, C.ROW_PAST, C.ROW_NEG, C.ROW_PLANAR, C.ROW_COLLINEAR, C.ROW_COINCIDE):
            assert not v[row].any() and not case.models[b][row].any() and not case.band[b][row], (b, row)
        # each for its stated reason: the planar and the collinear sample lose rank, the coincident one has no scale
        assert info["ok_scale"][C.ROW_PLANAR] and not info["ok_rank"][C.ROW_PLANAR] and info["pivot_ratio"][C.ROW_PLANAR] < 1e-14
        assert info["ok_scale"][C.ROW_COLLINEAR] and not info["ok_rank"][C.ROW_COLLINEAR] and info["pivot_ratio"][C.ROW_COLLINEAR] < 1e-14
        assert not info["ok_scale"][C.ROW_COINCIDE]
    assert (~case.info[2]["ok_cubic"]).sum() >= 1          # pair 2 draws three of its coincident points in some sample: the cubic rule
    # a repeated point given to the solver itself is two equal rows: rank 6
    x0s, x1s, _ = _clean_samples(n=1)
    rep = (x0s[:, [0, 1, 2, 3, 4, 5, 0]], x1s[:, [0, 1, 2, 3, 4, 5, 0]])
    F, v, info = pose.seven_point_ge(*rep, detail=True)
    assert not v.any() and not F.any() and not info["ok_rank"][0]
    # NaN, infinity and all-zero input: invalid, never an exception or a non-finite model
    for bad in (np.nan, np.inf):
        y = x0s.copy()
        y[0, 3, 1] = bad
        F, v = pose.seven_point_ge(y, x1s)
        assert not v.any() and not F.any()
    assert not pose.seven_point_ge(np.zeros((1, 7, 2)), np.zeros((1, 7, 2)))[1].any()
    # three matches that share their point on side 1: F^T x1 = 0 for every F of the null space, the cubic vanishes identically
    y = x1s.copy()
    y[0, 1] = y[0, 2] = y[0, 0]
    F, v, info = pose.seven_point_ge(x0s, y, detail=True)
    assert info["ok_rank"][0] and not info["ok_cubic"][0] and info["cubic_scale"][0] < 1e-14 and not v.any() and not F.any()
    # a general sample is far from every rule
    _, v, info = pose.seven_point_ge(x0s, x1s, detail=True)
    assert v.any() and info["pivot_ratio"][0] > 1e-6 and info["cubic_scale"][0] > 1e-6 and info["lead_ratio"][0] > 1e-6


def test_gpu_inputs_keep_their_caps():
    """tests/test_gpu_fundamental.py leaves out samples in the band (at most 2 % per pair), needs both answers outside it, needs
    every (model, point) Sampson error at least 1e-9 relative away from thr2, and non-trivial counts"""
    case = C.step_case()
    assert case.idx.shape == (3, 257, 7) and case.offsets.tolist() == [0, 1000, 1000, 1065]
    for b in (0, 2):
        band, v = case.band[b], case.valid[b]
        assert band.mean() <= 0.02, (b, band.mean())
        any_v = v.any(1)
        assert any_v[~band].sum() >= 200 and (~any_v[~band]).sum() >= 6, (b, any_v.mean())
        assert (v.sum(1)[~band] == 1).any() and (v.sum(1)[~band] == 3).any()               # both branches of the cubic
        a, c = case.pair(b)
        e = C.sampson(case.models[b][v], a, c)
        assert int((np.abs(e - C.THR2) <= 1e-9 * C.THR2).sum()) == 0
        cnt = (e <= C.THR2).sum(1)
        assert (cnt >= 7).all() and cnt.max() > 15, (b, cnt.min(), cnt.max())
    assert not case.valid[1].any()
    x0, x1, idx, F, v, info, band = C.tiny_case()
    assert x0.shape == (7, 2) and idx.shape == (1, 7) and v.any() and not band.any()
    assert (C.sampson(F[0][v[0]], x0, x1) <= 1e-12).all()
    pairs = C.batch_pairs()
    assert [len(a) for a, _ in pairs] == [300, 6, 7, 65, 1000]


# ---- RANSAC on the host ----------------------------------------------------------------------------------------------------------
def test_find_fundamental_mat_ge_on_a_decidable_scene():
    """300 matches, 180 exact inliers, every outlier at least 5 px from its epipolar line: the mask is the truth, exactly"""
    Ft, p0, p1, truth = C.ransac_scene()
    assert truth.sum() == 180 and (np.sqrt(C.sampson(Ft, p0[~truth], p1[~truth])) >= 5.0).all()
    F, mask = pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=0, solve="ge")
    assert mask.dtype == bool and np.array_equal(mask, truth)
    d = float(C.sin_dist(F, Ft))
    print(f"sin-distance of the RANSAC model to the truth {d:.3e}")
    assert d < 1e-8
    F6, m6 = pose.find_fundamental_mat(p0[:6], p1[:6], solve="ge")
    assert F6 is None and m6.shape == (6,) and not m6.any()
    i7 = np.flatnonzero(truth)[:7]
    F7, m7 = pose.find_fundamental_mat(p0[i7], p1[i7], solve="ge")
    assert F7 is not None and m7.all() and m7.shape == (7,)


def test_default_paths_are_unchanged():
    _, p0, p1, _ = C.ransac_scene()
    a = pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=3)
    b = pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=3, solve="host")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].sum() >= 180
    with pytest.raises(ValueError):
        pose.find_fundamental_mat(p0, p1, solve="device")
    with pytest.raises(ValueError):
        pose.find_fundamental_mat(p0, p1, solve="magsac")
    with pytest.raises(ValueError):
        pose.find_fundamental_mat_batch([(p0, p1)], device=None)
    from gim_amd import demo
    with pytest.raises(ValueError):
        demo.match_pair("gim_loftr", None, None, "a.png", "b.png", ransac_solve="cv2")


# ---- the library ------------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


def test_export_follows_the_header_within_revision_115():
    from gim_amd import _lib
    step = _lib.lib.gim_fundamental_step
    res, args = _header_prototype("gim_fundamental_step")
    assert (res, args) == _lib.PROTOTYPES["gim_fundamental_step"] and len(args) == 11
    assert step.restype is res and list(step.argtypes) == args
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    # empty problems return before anything is touched; malformed ones are refused before a launch
    assert step(None, None, None, 0, None, 7, 1.0, None, None, None, None) == 0
    assert step(None, None, None, 2, None, 0, 1.0, None, None, None, None) == 0
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = lambda k: ctypes.c_void_p(p.value + k)   # noqa: E731
    assert step(p, None, p, 1, p, 4, 1.0, p, p, p, None) != 0 and b"NULL" in _lib.lib.gim_last_error()
    assert step(p, p, p, 1, p, 4, 1.0, p, None, p, None) != 0 and b"NULL" in _lib.lib.gim_last_error()
    assert step(p, off(8), p, 1, p, 4, 1.0, p, p, p, None) != 0 and b"16-byte" in _lib.lib.gim_last_error()
    assert step(p, p, p, 1, p, 4, 1.0, off(4), p, p, None) != 0 and b"misaligned" in _lib.lib.gim_last_error()
    assert step(p, p, off(2), 1, p, 4, 1.0, p, p, p, None) != 0 and b"misaligned" in _lib.lib.gim_last_error()
    assert step(p, p, p, 1, off(2), 4, 1.0, p, p, p, None) != 0 and b"misaligned" in _lib.lib.gim_last_error()
    assert step(p, p, p, 1, p, 4, 1.0, p, p, off(2), None) != 0 and b"misaligned" in _lib.lib.gim_last_error()
    assert step(p, p, p, 65536, p, 4, 1.0, p, p, p, None) != 0 and b"65535" in _lib.lib.gim_last_error()
    assert step(p, p, p, -1, p, 4, 1.0, p, p, p, None) != 0
    assert step(p, p, p, 40000, p, 2000, 1.0, p, p, p, None) != 0 and b"samples" in _lib.lib.gim_last_error()   # 27 B K > INT32_MAX


def test_kernel_targets_gfx950_without_scratch():
    """fundamental_step_kernel: 102 VGPRs, no scratch, no spilled register on the build that wrote this test (the pivoting indexes LDS
    at run time, nothing else is indexed at run time); the bar is no scratch and no spills"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    hit = [(n, v) for n, v in kr._kernels().items() if "fundamental_step_kernel(" in n]
    assert hit, "fundamental_step_kernel not found in the library"
    for n, (regs, scratch, spills) in hit:
        print(f"{n[:40]}: {regs} VGPRs, {scratch} B scratch, {spills} spills")
        assert scratch == 0 and spills == 0, (n, regs, scratch, spills)
