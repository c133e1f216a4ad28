"""recoverPose on the device, without a GPU: pose.recover_pose_ge (the numpy restatement of csrc/recover_pose_solve.h) against the host
pose.recover_pose (LAPACK) on seeded scenes and at its edges, the unchanged default paths against vectors recorded from the parent
commit, the `recover=` argument rules, the new export against the header, the kernel's resources, and tools/rp_host_check.cpp (the
header on the CPU) against recover_pose_ge.  tests/recover_pose_cases.py builds the inputs for this file and the GPU tests."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import host_check
import recover_pose_cases as C
from gim_amd import pose, zeb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "recover_pose_parent.npz")
_CTYPE = {"int": ctypes.c_int, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}


def _against_host(E, x0, x1, dthr=1e9, mask=None):
    """recover_pose_ge against recover_pose on one problem: the undecidable points are left out (capped), the sorted counts agree,
    and where the maximum is unique the winner's (R, t) and mask agree -> (|dR|, |dt|, host's |R^T R - I|, ge's)"""
    dec = C.decidable(E, x0, x1, dthr)
    assert (~dec).mean() <= C.UNDECIDABLE_CAP if len(dec) else True
    n, R, t, good, counts, best = pose.recover_pose_ge(E, x0, x1, dthr, mask=mask, detail=True)
    hn, hR, ht, hgood = pose.recover_pose(E, x0, x1, dthr, mask=mask)
    assert n == counts[best] == int(good.sum()) and good.dtype == bool and good.shape == (len(x0),)
    # the host's four counts, in the device's candidate order (LAPACK may exchange R1 / R2 and negate t)
    cands, q3, z0, z1 = C.host_detail(E, x0, x1)
    perm = C.match_candidates(pose.decompose_essential_ge(E), cands)
    m_in = np.ones(len(x0), dtype=bool) if mask is None else np.asarray(mask) > 0
    hgoods = m_in & (z0 > 0) & (z0 < dthr) & (z1 > 0) & (z1 < dthr)                  # [4, P], host order
    if dec.all():
        assert [int(hgoods[perm[j]].sum()) for j in range(4)] == counts.tolist()
        assert sorted(hgoods.sum(1).tolist()) == sorted(counts.tolist())
    assert np.array_equal(hgoods[perm[best]][dec], good[dec])
    unique = (np.sort(counts)[-1] > np.sort(counts)[-2]) and dec.all()
    dR = dt = 0.0
    if unique:
        assert hn == n
        dR, dt = float(np.abs(R - hR).max()), float(np.abs(t - ht).max())
        assert np.array_equal(hgood[dec], good[dec])
    orth = lambda M: float(np.abs(M.T @ M - np.eye(3)).max())   # noqa: E731
    return dR, dt, orth(hR), orth(R)


def test_ge_against_the_host_on_the_scenes():
    """Five scenes of P = 2 000 (50 % outliers, 5e-4 noise): 0 of the 40 000 (point, candidate) pairs are undecidable; the four
    counts, the winner and the mask equal the host's.  R and t against LAPACK's, measured here (numpy, fp64): |dR| 7.008e-16,
    |dt| 2.220e-16; the bar is 8 x the larger, 5.606e-15 (C.RT_BAR).  Orthogonality max |R^T R - I|: host 1.110e-15, recover_pose_ge
    8.882e-16; the bar is 8 x the host's own figure on the same scenes."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for E, x0, x1, _, _ in C.scenes():
        assert C.decidable(E, x0, x1).all()
        worst = [max(a, b) for a, b in zip(worst, _against_host(E, x0, x1))]
    print(f"|dR| {worst[0]:.3e} |dt| {worst[1]:.3e}; |R^T R - I| host {worst[2]:.3e} ge {worst[3]:.3e}")
    assert worst[0] <= C.RT_BAR and worst[1] <= C.RT_BAR
    assert worst[3] <= 8.0 * worst[2]


def test_the_truth_is_recovered():
    for E, x0, x1, R, t in C.scenes()[:2]:
        n, Rg, tg, good = pose.recover_pose_ge(E, x0, x1)
        assert n > 900 and np.abs(Rg - R).max() < 1e-12 and np.abs(tg - t).max() < 1e-12
        assert abs(np.linalg.det(Rg) - 1.0) < 1e-14


@pytest.mark.parametrize("P", [0, 1, 5, 257])
def test_small_point_counts(P):
    E, x0, x1, _, _ = C.scene(120 + P, P)
    _against_host(E, x0, x1)
    n, R, t, good, counts, best = pose.recover_pose_ge(E, x0, x1, detail=True)
    assert good.shape == (P,) and counts.shape == (4,)
    if P == 0:
        c = pose.decompose_essential_ge(E)
        assert n == 0 and best == 0 and not counts.any() and np.array_equal(R, c[0][0]) and np.array_equal(t, c[0][1])


def test_masks_threshold_and_points_behind():
    E, x0, x1, _, _ = C.scene(101, 2000)
    P = len(x0)
    n, R, t, good, counts, best = pose.recover_pose_ge(E, x0, x1, mask=np.zeros(P, dtype=bool), detail=True)
    assert n == 0 and not counts.any() and best == 0 and not good.any()
    holes = C.mask_with_holes(P)
    _against_host(E, x0, x1, mask=holes)
    full = pose.recover_pose_ge(E, x0, x1, detail=True)
    part = pose.recover_pose_ge(E, x0, x1, mask=holes, detail=True)
    assert np.array_equal(part[3], full[3] & holes) and 0 < part[0] < full[0]
    # distance_thresh = 5: the upper bound bites
    _against_host(E, x0, x1, dthr=5.0)
    near = pose.recover_pose_ge(E, x0, x1, 5.0, detail=True)
    assert 0 < near[0] < full[0] and not (near[3] & ~full[3]).any()
    # every point behind a camera under every candidate
    Eb, b0, b1 = C.behind_scene()
    _against_host(Eb, b0, b1)
    n, _, _, good, counts, best = pose.recover_pose_ge(Eb, b0, b1, detail=True)
    assert n == 0 and not counts.any() and best == 0 and not good.any()
    assert pose.recover_pose(Eb, b0, b1)[0] == 0


def test_invalid_and_rescaled_E():
    E, x0, x1, _, _ = C.scene(102, 300)
    for bad in (np.zeros((3, 3)), np.where(np.eye(3) > 0, np.nan, E), np.where(np.eye(3) > 0, np.inf, E)):
        n, R, t, good, counts, best = pose.recover_pose_ge(bad, x0, x1, detail=True)
        assert n == 0 and best == -1 and not counts.any() and not R.any() and not t.any() and not good.any() and good.shape == (300,)
    ref = pose.recover_pose_ge(E, x0, x1, detail=True)
    for scale in (-1.0, 1e-6, -1e-6):
        got = pose.recover_pose_ge(scale * E, x0, x1, detail=True)
        assert sorted(got[4].tolist()) == sorted(ref[4].tolist()) and got[0] == ref[0]         # the same pose set
        assert C.same_pose(got[1], got[2], ref[1], ref[2]) and np.array_equal(got[3], ref[3])
    # a rank-one E still gives four proper candidates
    for R, t in pose.decompose_essential_ge(np.outer([1.0, 2.0, 3.0], [0.0, 1.0, 0.0])):
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14 and abs(np.linalg.norm(t) - 1.0) < 1e-14


def test_the_constants_mirror_the_header():
    src = open(os.path.join(ROOT, "gim_amd", "csrc", "recover_pose_solve.h")).read()
    for name in ("SWEEPS3", "SWEEPS4", "W_TINY"):
        m = re.search(r"constexpr (?:double|int) GIM_RP_%s = ([^;]+);" % name, src)
        assert m and float(m.group(1)) == float(getattr(pose, "RP_" + name)), name


# ---- defaults and argument rules -----------------------------------------------------------------------------------------------------
def test_default_paths_reproduce_the_parent_commit(monkeypatch):
    """tests/golden/recover_pose_parent.npz was recorded with the parent commit's gim_amd: pose.recover_pose on C.scene(101, 300)
    (no mask, C.mask_with_holes, distance_thresh 5) and zeb.estimate_pose(kpts0, kpts1, K0, K1) on C.ransac_pairs() with the numpy
    backend.  Without `device=` / `recover=` both reproduce it bit for bit."""
    g = np.load(GOLDEN)
    E, x0, x1, _, _ = C.scene(101, 300)
    for name, kw in (("plain", {}), ("holes", {"mask": C.mask_with_holes(300)}), ("thr5", {"distance_thresh": 5.0})):
        for got in (pose.recover_pose(E, x0, x1, **kw), pose.recover_pose(E, x0, x1, device=None, **kw)):
            assert got[0] == int(g[f"rp_{name}_n"]) and np.array_equal(got[1], g[f"rp_{name}_R"])
            assert np.array_equal(got[2], g[f"rp_{name}_t"]) and np.array_equal(got[3], g[f"rp_{name}_mask"])
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    some = 0
    for i, (a, b, k0, k1) in enumerate(C.ransac_pairs()):
        for got in (zeb.estimate_pose(a, b, k0, k1), zeb.estimate_pose(a, b, k0, k1, recover="host")):
            assert (got is None) == bool(g[f"ep_{i}_none"])
            if got is not None:
                some += 1
                assert all(np.array_equal(x, g[f"ep_{i}_{k}"]) for x, k in zip(got, ("R", "t", "inl")))
    assert some >= 4
    # find_essential_mat keeps its two return values
    out = pose.find_essential_mat(*[(p - C.K_PIX[[0, 1], [2, 2]]) / 800.0 for p in C.ransac_pairs()[1][:2]], 1e-3)
    assert len(out) == 2 and out[0].shape == (3, 3) and out[1].dtype == bool


def test_invalid_recover_combinations(monkeypatch):
    monkeypatch.setenv("GIM_POSE_BACKEND", "numpy")
    a, b, k0, k1 = C.ransac_pairs()[1]

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    from gim_amd import ops
    monkeypatch.setattr(ops, "lib", NoLaunch())
    with pytest.raises(ValueError):
        zeb.estimate_pose(a, b, k0, k1, recover="device")                       # no device
    with pytest.raises(ValueError):
        zeb.estimate_pose(a, b, k0, k1, recover="gpu", device="cuda:0")
    with pytest.raises(ValueError):
        zeb.estimate_pose(a, b, k0, k1, solve="ge", recover="device")           # ge runs without a device
    with pytest.raises(ValueError):
        zeb.device_estimator(None, recover="device")
    with pytest.raises(ValueError):
        zeb.device_batch_estimator(None, recover="device")
    with pytest.raises(ValueError):
        zeb.device_batch_estimator("cuda:0", recover="both")
    with pytest.raises(ValueError):
        pose.find_essential_pose(a, b, 1e-3)                                    # needs a device
    with pytest.raises(ValueError):
        pose.find_essential_pose_batch([(a, b)], 1e-3)
    monkeypatch.setenv("GIM_POSE_BACKEND", "cv2")                               # the cv2 backend recovers the pose itself
    monkeypatch.setattr(pose, "backend", lambda: "cv2")
    with pytest.raises(ValueError):
        zeb.estimate_pose(a, b, k0, k1, device="cuda:0", recover="device")
    with pytest.raises(ValueError):
        zeb.device_batch_estimator("cuda:0", recover="device")


# ---- the library ------------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


def test_export_follows_the_header_within_revision_115():
    from gim_amd import _lib
    fn = _lib.lib.gim_recover_pose
    res, args = _header_prototype("gim_recover_pose")
    assert (res, args) == _lib.PROTOTYPES["gim_recover_pose"] and len(args) == 13
    assert fn.restype is res and list(fn.argtypes) == args
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    # an empty batch returns before anything is touched; malformed calls are refused before a launch
    assert fn(None, None, None, None, 0, None, 1e9, None, None, None, None, None, None) == 0
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = lambda k: ctypes.c_void_p(p.value + k)   # noqa: E731
    assert fn(p, p, p, p, 1, None, 1e9, p, p, p, None, p, None) != 0 and b"NULL" in _lib.lib.gim_last_error()
    assert fn(p, None, p, p, 1, None, 1e9, p, p, p, p, p, None) != 0 and b"NULL" in _lib.lib.gim_last_error()
    assert fn(p, p, p, p, 1, None, 1e9, p, p, p, p, None, None) != 0 and b"NULL" in _lib.lib.gim_last_error()
    assert fn(p, off(8), p, p, 1, None, 1e9, p, p, p, p, p, None) != 0 and b"16-byte" in _lib.lib.gim_last_error()
    assert fn(off(4), p, p, p, 1, None, 1e9, p, p, p, p, p, None) != 0 and b"misaligned" in _lib.lib.gim_last_error()
    assert fn(p, p, p, off(2), 1, None, 1e9, p, p, p, p, p, None) != 0 and b"misaligned" in _lib.lib.gim_last_error()
    assert fn(p, p, p, p, 1, None, 1e9, p, off(4), p, p, p, None) != 0 and b"misaligned" in _lib.lib.gim_last_error()
    assert fn(p, p, p, p, 1, None, 1e9, p, p, p, off(2), p, None) != 0 and b"misaligned" in _lib.lib.gim_last_error()
    assert fn(p, p, p, p, 65536, None, 1e9, p, p, p, p, p, None) != 0 and b"65535" in _lib.lib.gim_last_error()
    assert fn(p, p, p, p, -1, None, 1e9, p, p, p, p, p, None) != 0


def test_kernel_targets_gfx950_without_scratch():
    """recover_pose_kernel: 112 VGPRs, 456 bytes of LDS, no scratch, no spilled register on the build that wrote this test (the
    3 x 3 and 4 x 4 matrices are indexed at compile time only); the bar is no scratch and no spills"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    hit = [(n, v) for n, v in kr._kernels().items() if "recover_pose_kernel(" in n]
    assert hit, "recover_pose_kernel not found in the library"
    for n, (regs, scratch, spills) in hit:
        print(f"{n[:40]}: {regs} VGPRs, {scratch} B scratch, {spills} spills")
        assert scratch == 0 and spills == 0, (n, regs, scratch, spills)


def _problem_text(E, x0, x1, dthr, mask):
    f = lambda v: "nan" if np.isnan(v) else repr(float(v))   # noqa: E731
    lines = [f"{len(x0)} {int(mask is not None)} {f(dthr)}", " ".join(f(v) for v in np.asarray(E).ravel())]
    for k in range(len(x0)):
        lines.append(" ".join(f(v) for v in (*x0[k], *x1[k])) + ("" if mask is None else f" {int(mask[k])}"))
    return "\n".join(lines) + "\n"


def test_host_check_agrees_with_the_numpy_oracle(tmp_path):
    """tools/rp_host_check.cpp is plain C++ over the kernel's header; built with the host compiler, its self-check passes and its
    results on problems written here equal recover_pose_ge's: counts, winner and mask exactly on these scenes, R and t within
    C.RT_BAR (the two differ at most by how the compiler rounds a*b+c).  The sanitizer run is a development step, recorded in
    profiles/recover_pose.txt."""
    r = host_check.run("rp_host_check", tmp_path)
    assert r.stdout.strip().endswith("OK"), r.stdout
    E, x0, x1, _, _ = C.scene(101, 2000)
    Es, s0, s1, _, _ = C.scene(125, 5)
    Eb, b0, b1 = C.behind_scene()
    problems = [(E, x0, x1, 1e9, None), (E, x0, x1, 5.0, C.mask_with_holes(2000)), (Es, s0, s1, 1e9, None), (Es, s0[:0], s1[:0], 1e9, None),
                (np.zeros((3, 3)), s0, s1, 1e9, None), (np.where(np.eye(3) > 0, np.nan, Es), s0, s1, 1e9, None), (-1e-6 * E, x0, x1, 1e9, None),
                (Eb, b0, b1, 1e9, None)]
    path = tmp_path / "problems.txt"
    path.write_text("".join(_problem_text(*p) for p in problems))
    r = subprocess.run([str(tmp_path / "rp_host_check"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.strip().split("\n")
    assert len(out) == 3 * len(problems)
    for i, (E_, a, b, dthr, m) in enumerate(problems):
        n, R, t, good, counts, best = pose.recover_pose_ge(E_, a, b, dthr, mask=m, detail=True)
        head = [int(v) for v in out[3 * i].split()]
        Rt = np.array([float(v) for v in out[3 * i + 1].split()])
        got = np.array([c == "1" for c in out[3 * i + 2]], dtype=bool) if len(a) else np.zeros(0, dtype=bool)
        assert head == [i, best, *counts.tolist()], (i, head, best, counts)
        assert np.array_equal(got, good)
        assert C.same_pose(Rt[:9].reshape(3, 3), Rt[9:], R, t), (i, np.abs(Rt[:9].reshape(3, 3) - R).max())
