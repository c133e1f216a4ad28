"""The five-point half of the essential-matrix RANSAC step without a GPU: pose.five_point_ge (the numpy restatement of
csrc/essential_solve.h) on exact synthetic geometry and against the SVD / LAPACK solver pose.five_point, its validity rules, the host
RANSAC over it, the unchanged default paths, the new export against the header, the kernel's resources, and -- from the host code
alone -- that the seeded inputs of tests/test_gpu_essential.py keep their caps (tests/essential_cases.py builds those inputs for
both)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import essential_cases as C
from gim_amd import pose, zeb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}


def _general_samples(b):
    """the samples of pair b of the step case that reach the solver and lie outside the band -> (keep [K] bool, x0s, x1s [n, 5, 2])"""
    case = C.step_case()
    a, c = case.pair(b)
    idx = case.idx[b]
    keep = ~case.band[b] & ((idx >= 0) & (idx < len(a))).all(1) & np.array([len(set(r)) == 5 for r in idx.tolist()])
    keep &= case.info[b]["ok_input"] & case.info[b]["ok_rank"] & case.info[b]["ok_pivot"]     # five_point has no such rules
    return keep, a[idx[keep]], c[idx[keep]]


# ---- the minimal solver ----------------------------------------------------------------------------------------------------------
def test_exact_geometry_is_recovered():
    """The scenes and samples of tests/test_pose_cpu.py::test_five_point_contains_the_true_essential_matrix (three random poses, 64
    samples of exact matches each) and its measure (largest |entry| of the difference, up to sign): the true E is among the
    candidates of every sample to 1e-9.  Measured here (numpy, fp64): five_point_ge 1.855e-11, five_point 1.143e-11."""
    import test_pose_cpu as T
    rng = np.random.default_rng(1)
    worst = [0.0, 0.0]
    for _ in range(3):
        R, t, x0, x1 = T._scene(rng, 300)
        idx = np.stack([rng.choice(300, 5, replace=False) for _ in range(64)])
        Et = T._essential(R, t)
        E, v, info = pose.five_point_ge(x0[idx], x1[idx], detail=True)
        assert E.shape == (64, 10, 3, 3) and v.shape == (64, 10) and v.dtype == bool
        assert v.any(1).all() and set(v.sum(1).tolist()) <= {2, 4, 6, 8, 10}
        d = np.where(v, T._dist_up_to_sign(E, Et), np.inf).min(1)
        Es, vs = pose.five_point(x0[idx], x1[idx])
        worst = [max(worst[0], d.max()), max(worst[1], np.where(vs, T._dist_up_to_sign(Es, Et), np.inf).min(1).max())]
        assert d.max() < 1e-9
        nrm = np.linalg.norm(E.reshape(64, 10, 9), axis=-1)
        assert np.abs(nrm[v] - 1.0).max() <= 1e-14 and not E[~v].any()
        lam = info["roots"]
        assert (np.diff(np.where(np.isnan(lam), 1e300, lam), axis=1) >= 0).all()           # the slots are ordered by their root
        assert np.array_equal(v, ~np.isnan(lam)) and info["qr_ok"].all() and info["qr_its"].max() < 30
    print(f"largest |entry| distance to the truth: five_point_ge {worst[0]:.3e}, five_point {worst[1]:.3e}")


def test_solutions_and_residuals_against_the_svd_solver():
    """Every sample of the GPU tests' step case outside the band (both non-empty pairs, 50 % outliers: general 5-tuples, not only
    consistent ones): the number of real solutions equals pose.five_point's, the two sets match (sign-aligned Frobenius distance,
    printed), and the elimination's residuals stay within 8 x five_point's own maximum on the same samples, floored at 1e-15.
    Measured here (numpy, fp64), 492 samples: largest set distance 1.770e-10 (median 5.656e-14); epipolar residual max |p1^T E p0|
    five_point 5.169e-16, five_point_ge 1.544e-16; cubic residual max |2 E E^T E - tr(E E^T) E| five_point 1.057e-10, five_point_ge
    2.274e-10 (2.2 x).  The set distance is a reading, not a precision bar; the 1e-6 on it only says that the two solvers found the same
    solutions: outside the band two roots of a sample are at least 1e-6 (relative) apart, so a model nearer than that to a model
    of the other solver is that solver's model of the same root."""
    case = C.step_case()
    worst = {"svd": [0.0, 0.0], "ge": [0.0, 0.0]}
    n, far = 0, []
    for b in (0, 2):
        keep, x0s, x1s = _general_samples(b)
        Es, vs = pose.five_point(x0s, x1s)
        Eg, vg = case.models[b][keep], case.valid[b][keep]
        assert np.array_equal(vs.sum(1), vg.sum(1)), np.flatnonzero(vs.sum(1) != vg.sum(1))
        far += [C.set_dist(Eg[s], vg[s], Es[s], vs[s]) for s in range(len(Eg))]
        for name, E, v in (("svd", Es, vs), ("ge", Eg, vg)):
            r, c = C.residuals(E, x0s, x1s)
            worst[name][0] = max(worst[name][0], r[v].max())
            worst[name][1] = max(worst[name][1], c[v].max())
        n += int(keep.sum())
    print(f"{n} samples: largest set distance {max(far):.3e} (median {np.median(far):.3e}); epipolar residual svd {worst['svd'][0]:.3e} "
          f"ge {worst['ge'][0]:.3e}; cubic residual svd {worst['svd'][1]:.3e} ge {worst['ge'][1]:.3e}")
    assert n > 400
    assert max(far) < 1e-6                                       # the same solutions, not merely equally many
    assert worst["ge"][0] <= max(8.0 * worst["svd"][0], 1e-15) and worst["ge"][1] <= max(8.0 * worst["svd"][1], 1e-15)


def test_validity_rules():
    case = C.step_case()
    for b in (0, 2):
        v, info = case.valid[b], case.info[b]
        for row in C.PLANTED:
            assert not v[row].any() and not case.models[b][row].any() and not case.band[b][row], (b, row)
        # each for its stated reason
        assert info["ok_input"][C.ROW_COINCIDE] and not info["ok_rank"][C.ROW_COINCIDE] and info["rank_ratio"][C.ROW_COINCIDE] < 1e-14
        assert info["ok_input"][C.ROW_RANK4] and not info["ok_rank"][C.ROW_RANK4] and info["rank_ratio"][C.ROW_RANK4] < 1e-14
        assert not info["ok_input"][C.ROW_NONFINITE]
    x0, x1, _ = C.two_views(np.random.default_rng(31), 5)
    x0s, x1s = x0[None], x1[None]
    # NaN, infinity and all-zero input: invalid, never an exception or a non-finite model
    for bad in (np.nan, np.inf, -np.inf):
        for side in (0, 1):
            y = [x0s.copy(), x1s.copy()]
            y[side][0, 3, 1] = bad
            E, v = pose.five_point_ge(*y)
            assert not v.any() and not E.any()
    assert not pose.five_point_ge(np.zeros((1, 5, 2)), np.zeros((1, 5, 2)))[1].any()
    # a general sample is far from every threshold
    _, v, info = pose.five_point_ge(x0s, x1s, detail=True)
    assert v.any() and info["rank_ratio"][0] > 1e-6 and info["pivot_ratio"][0] > 1e-8 and info["w_ratio"][0] > 1e-10
    assert info["gap_rel"][0] > 1e-4 and info["disc_rel"][0] > 1e-4 and info["qr_ok"][0] and not C.in_band(info)[0]
    # the constants mirror the header's
    src = open(os.path.join(ROOT, "gim_amd", "csrc", "essential_solve.h")).read()
    for name in ("RANK_EPS", "PIVOT_EPS", "W_EPS", "QR_EPS", "QR_ITS"):
        m = re.search(r"constexpr (?:double|int) GIM_E5_%s = ([^;]+);" % name, src)
        assert m and float(m.group(1)) == float(getattr(pose, "E5_" + name)), name


def test_gpu_inputs_keep_their_caps():
    """tests/test_gpu_essential.py leaves out samples in the band (at most 2 % per pair), needs enough answers of every kind outside
    it, needs every (model, point) Sampson error at least 1e-9 relative away from thr2, and non-trivial counts"""
    case = C.step_case()
    assert case.idx.shape == (3, 257, 5) and case.offsets.tolist() == [0, 1000, 1000, 1065]
    for b in (0, 2):
        band, v = case.band[b], case.valid[b]
        assert band.mean() <= 0.02, (b, band.mean())
        any_v = v.any(1)
        assert any_v[~band].sum() >= 200, (b, any_v.mean())
        nsol = v.sum(1)[~band]
        assert (nsol == 2).any() and (nsol == 4).any() and (nsol == 6).any(), np.bincount(nsol)
        a, c = case.pair(b)
        e = C.sampson(case.models[b][v], a, c)
        assert int((np.abs(e - C.THR2) <= 1e-9 * C.THR2).sum()) == 0
        cnt = (e <= C.THR2).sum(1)
        assert cnt.max() > 15, (b, cnt.min(), cnt.max())
    assert not case.valid[1].any()
    x0, x1, idx, Et, E, v, info, band = C.tiny_case()
    assert x0.shape == (5, 2) and idx.shape == (1, 5) and v.any() and not band.any()
    assert (C.sampson(E[0][v[0]], x0, x1) <= 1e-12).all() and C.dist(E[0][v[0]], Et).min() < 1e-9
    assert [len(a) for a, _ in C.batch_pairs()] == [300, 4, 5, 65, 1000]


# ---- RANSAC on the host ----------------------------------------------------------------------------------------------------------
def test_find_essential_mat_ge_on_a_decidable_scene(monkeypatch):
    """300 matches, 180 exact inliers, every outlier at least 10 x the threshold from its epipolar line: the mask is the truth,
    exactly, and the pose recovered through zeb.estimate_pose is the scene's"""
    Et, x0, x1, truth = C.ransac_scene()
    assert truth.sum() == 180 and (np.sqrt(C.sampson(Et, x0[~truth], x1[~truth])) >= 10.0 * C.THR).all()
    E, mask = pose.find_essential_mat(x0, x1, C.THR, seed=0, solve="ge")
    assert mask.dtype == bool and np.array_equal(mask, truth)
    d = float(C.dist(E, Et))
    print(f"distance of the RANSAC model to the truth {d:.3e}")
    assert d < 1e-8
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    R, t, inl = zeb.estimate_pose(C.to_pixels(x0), C.to_pixels(x1), C.K_PIX, C.K_PIX, solve="ge")
    tn = C.T_TRUE / np.linalg.norm(C.T_TRUE)
    print(f"|R - R*| {np.abs(R - C.R_TRUE).max():.3e}, |t - t*| {np.abs(t - tn).max():.3e}")
    assert np.abs(R - C.R_TRUE).max() < 1e-6 and np.abs(t - tn).max() < 1e-6 and np.array_equal(inl, truth)
    E4, m4 = pose.find_essential_mat(x0[:4], x1[:4], C.THR, solve="ge")
    assert E4 is None and m4.shape == (4,) and not m4.any()
    i5 = np.flatnonzero(truth)[:5]
    E5, m5 = pose.find_essential_mat(x0[i5], x1[i5], C.THR, solve="ge")
    assert E5 is not None and m5.all() and m5.shape == (5,)


def test_default_paths_are_unchanged():
    _, x0, x1, truth = C.ransac_scene()
    a = pose.find_essential_mat(x0, x1, C.THR, seed=3)
    b = pose.find_essential_mat(x0, x1, C.THR, seed=3, solve="host")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[1], truth)
    c = pose.find_essential_mat_batch([(x0, x1)], C.THR, seed=3)
    assert np.array_equal(a[0], c[0][0]) and np.array_equal(a[1], c[0][1])
    with pytest.raises(ValueError):
        pose.find_essential_mat(x0, x1, C.THR, solve="device")
    with pytest.raises(ValueError):
        pose.find_essential_mat(x0, x1, C.THR, solve="magsac")
    with pytest.raises(ValueError):
        pose.find_essential_mat(x0, x1, C.THR, device="cuda:0", solve="ge")
    with pytest.raises(ValueError):
        pose.find_essential_mat_batch([(x0, x1)], C.THR, solve="device")
    with pytest.raises(ValueError):
        pose.find_essential_mat_batch([(x0, x1)], C.THR, solve="ge")
    with pytest.raises(ValueError):
        pose.find_fundamental_mat_batch([(x0, x1)], device=None)


# ---- the library ------------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


def test_export_follows_the_header_within_revision_115():
    from gim_amd import _lib
    step = _lib.lib.gim_essential_step
    res, args = _header_prototype("gim_essential_step")
    assert (res, args) == _lib.PROTOTYPES["gim_essential_step"] and len(args) == 11
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
    assert step(p, p, p, 40000, p, 600, 1.0, p, p, p, None) != 0 and b"samples" in _lib.lib.gim_last_error()   # 90 B K > INT32_MAX


def test_kernel_targets_gfx950_without_scratch():
    """essential_step_kernel: 220 VGPRs, 11 904 bytes of LDS, no scratch, no spilled register on the build that wrote this test
    (everything indexed at run time lives in LDS); the bar is no scratch and no spills"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    hit = [(n, v) for n, v in kr._kernels().items() if "essential_step_kernel(" in n]
    assert hit, "essential_step_kernel not found in the library"
    for n, (regs, scratch, spills) in hit:
        print(f"{n[:40]}: {regs} VGPRs, {scratch} B scratch, {spills} spills")
        assert scratch == 0 and spills == 0, (n, regs, scratch, spills)


def test_host_check_compiles(tmp_path):
    """tools/e5_host_check.cpp is plain C++ over the solver's header: it compiles with the host compiler (the sanitizer run is a
    development step, recorded in profiles/essential.txt; here only the syntax is checked, which takes no linking)"""
    from gim_amd.build import _hipcc
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or _hipcc()   # hipcc compiles plain C++ too
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "gim_amd", "csrc"),
                        os.path.join(ROOT, "tools", "e5_host_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
