"""The homography half of gim_amd/pose.py and the demo's compute_geom / warp_pair, without a GPU: the four-point solver and its validity
rules on exact synthetic data, find_homography on a decidable scene, the new exports against the header, find_fundamental_mat
unchanged against vectors recorded from the parent commit (tests/golden/homography_parent.npz), and -- from the host code and the
oracles alone -- that the seeded inputs of tests/test_gpu_homography.py and tests/test_gpu_warp.py keep their caps on undecidable
samples and pixels (tests/homography_cases.py builds those inputs for both)."""
import ctypes
import os
import re

import numpy as np
import pytest

import homography_cases as C
import homography_oracle as O
from gim_amd import pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}


def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


def test_exports_follow_the_header_within_revision_115():
    from gim_amd import _lib
    for name, nargs in (("gim_homography_step", 11), ("gim_homography_mask", 8), ("gim_warp_perspective", 11)):
        fn = getattr(_lib.lib, name)
        res, args = _header_prototype(name)
        assert (res, args) == _lib.PROTOTYPES[name] and len(args) == nargs, (name, args, _lib.PROTOTYPES[name])
        assert fn.restype is res and list(fn.argtypes) == args
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    step, mask, warp = _lib.lib.gim_homography_step, _lib.lib.gim_homography_mask, _lib.lib.gim_warp_perspective
    # empty problems return before anything is touched; malformed ones are refused before a launch
    assert step(None, None, None, 0, None, 7, 1.0, None, None, None, None) == 0
    assert step(None, None, None, 2, None, 0, 1.0, None, None, None, None) == 0
    assert mask(None, None, None, None, 0, 1.0, None, None) == 0
    assert warp(None, 0, 0, 3, 4, 4, None, None, 4, 4, None) == 0 and warp(None, 1, 2, 3, 4, 4, None, None, 0, 4, None) == 0
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert step(p, None, p, 1, p, 4, 1.0, p, p, p, None) != 0 and b"NULL" in _lib.lib.gim_last_error()
    assert step(p, ctypes.c_void_p(p.value + 8), p, 1, p, 4, 1.0, p, p, p, None) != 0 and b"16-byte" in _lib.lib.gim_last_error()
    assert mask(p, p, p, None, 1, 1.0, p, None) != 0
    assert warp(p, 2, 1, 3, 4, 4, p, p, 4, 4, None) != 0 and warp(p, 0, 1, 5, 4, 4, p, p, 4, 4, None) != 0 and warp(p, 0, 1, 3, 4, 4, None, p, 4, 4, None) != 0


def test_kernels_target_gfx950_without_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr._kernels()
    for key in ("homography_step_kernel(", "homography_mask_kernel(", "warp_perspective_kernel<unsigned char>(", "warp_perspective_kernel<float>("):
        hit = [(n, v) for n, v in ks.items() if key in n]
        assert hit, f"{key[:-1]} not found in the library"
        for n, (regs, scratch, spills) in hit:
            assert scratch == 0 and spills == 0 and regs <= 128, (n, regs, scratch, spills)


# ---- the minimal solver ----------------------------------------------------------------------------------------------------------
def test_four_point_solver_recovers_a_known_homography():
    """200 seeded samples, one point per quadrant of the 640 x 480 frame (so the normalised 8 x 8 systems are well conditioned: the
    test checks cond <= 1e4), exact partners under a general projective H.  Bar: 1e-8 px, for the four sample points and for the
    frame corners against the truth -- exact data, fp64, condition <= 1e4 leave errors near 1e-11."""
    rng = np.random.default_rng(41)
    H = O.general_h(rng)
    src = C.quadrant_samples(rng, 200)
    dst = np.stack([O.proj(H, s) for s in src])
    Hs, valid, info = pose.homography_4pt(src, dst, detail=True)
    assert Hs.shape == (200, 1, 3, 3) and valid.shape == (200, 1) and valid.all()
    A, _ = C.normalised_systems(info)
    assert np.linalg.cond(A).max() <= 1e4
    fit = max(np.sqrt(O.transfer_error(Hs[i, 0], src[i], dst[i])).max() for i in range(200))
    corner = max(O.corner_error(Hs[i, 0], H) for i in range(200))
    scale = np.abs(Hs[:, 0] / Hs[:, 0, 2:, 2:] - H / H[2, 2]).max()
    print(f"fit {fit:.3e} px, corners {corner:.3e} px, |H - truth| {scale:.3e}")
    assert (Hs[:, 0, 2, 2] == 1.0).all() and fit <= 1e-8 and corner <= 1e-8


def test_validity_rules():
    rng = np.random.default_rng(42)
    H = O.general_h(rng)
    pts = C.quadrant_samples(rng, 1)[0]
    good = (pts[None], O.proj(H, pts)[None])
    assert pose.homography_4pt(*good)[1].all()
    # a repeated index
    idx = np.array([[0, 1, 2, 1]])
    Hr, vr = pose.homography_4pt(pts[idx], O.proj(H, pts)[idx])
    assert not vr.any() and not Hr.any()
    # three collinear points on one side (the other side in general position)
    col = pts.copy()
    col[2] = 0.25 * col[0] + 0.75 * col[1]
    assert not pose.homography_4pt(col[None], good[1])[1].any() and not pose.homography_4pt(good[1], col[None])[1].any()
    # an orientation flip: the square and the bow tie over the same corners (the triple (1, 2, 3) turns the other way, (0, 1, 2) does not)
    sq = np.array([[100.0, 100.0], [300.0, 100.0], [300.0, 300.0], [100.0, 300.0]])
    Hf, vf, info = pose.homography_4pt(sq[None], sq[[0, 1, 3, 2]][None], detail=True)
    assert not vf.any() and not info["orient_ok"].any() and info["min_area"][0] > 0.1
    # all four triples turned (a mirror image) pass, as HomographyEstimatorCallback::checkSubset decides it
    mir = sq * [-1.0, 1.0] + [640.0, 0.0]
    Hm, vm = pose.homography_4pt(sq[None], mir[None])
    assert vm.all() and np.sqrt(O.transfer_error(Hm[0, 0], sq, mir)).max() <= 1e-8
    # four coincident points, and a NaN
    assert not pose.homography_4pt(np.repeat(pts[:1], 4, 0)[None], good[1])[1].any()
    bad = pts.copy()
    bad[3, 1] = np.nan
    assert not pose.homography_4pt(bad[None], good[1])[1].any()


def test_transfer_error_matches_the_oracle_and_rejects_w_zero():
    rng = np.random.default_rng(43)
    H = np.stack([O.general_h(rng) for _ in range(5)])
    src, dst = rng.uniform(0, 480, (50, 2)), rng.uniform(0, 480, (50, 2))
    e, want = pose.transfer_error(H, src, dst), O.transfer_error(H, src, dst)
    assert e.shape == (5, 50) and np.abs(e - want).max() <= 1e-9 * want.max()
    Hw = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -2.0]])              # w = x - 2: zero at x = 2
    assert np.isinf(pose.transfer_error(Hw, np.array([[2.0, 1.0]]), np.array([[0.0, 0.0]]))).all()
    assert np.isinf(pose.transfer_error(np.zeros((3, 3)), src, dst)).all()


def test_dlt_refit():
    rng = np.random.default_rng(44)
    H = O.general_h(rng)
    src = rng.uniform([0, 0], [640, 480], (50, 2))
    Hd = pose.homography_dlt(src, O.proj(H, src))
    assert Hd[2, 2] == 1.0 and O.corner_error(Hd, H) <= 1e-8
    assert pose.homography_dlt(src[:3], src[:3]) is None and pose.homography_dlt(np.repeat(src[:1], 5, 0), src[:5]) is None


# ---- find_homography on the host -------------------------------------------------------------------------------------------------
def test_find_homography_on_a_decidable_scene():
    """300 matches, 60 % exact inliers, every outlier at least 5 px from its true transfer: the mask is the truth, exactly, and the
    corners land within 1e-6 px"""
    Ht, src, dst, truth = C.ransac_scene()
    assert truth.sum() == 180 and (np.sqrt(O.transfer_error(Ht, src[~truth], dst[~truth])) >= 5.0).all()
    H, mask = pose.find_homography(src, dst, 1.0, 0.999999, 10000, seed=0)
    assert mask.dtype == bool and np.array_equal(mask, truth)
    err = O.corner_error(H, Ht)
    print(f"corner error {err:.3e} px")
    assert H[2, 2] == 1.0 and err <= 1e-6
    # P = 3: nothing; P = 4 exact: all four
    H3, m3 = pose.find_homography(src[:3], dst[:3])
    assert H3 is None and m3.shape == (3,) and not m3.any()
    i4 = np.flatnonzero(truth)[[0, 50, 100, 150]]
    H4, m4 = pose.find_homography(src[i4], dst[i4])
    assert H4 is not None and m4.all() and m4.shape == (4,)


def test_solve_idx_hook_walks_the_same_trajectory():
    """the hook of _ransac_steps, fed by the host solver: same model and mask as the plain call"""
    Ht, src, dst, truth = C.ransac_scene()
    calls = []

    def hook(idx):
        calls.append(idx.shape)
        return pose.homography_4pt(src[idx], dst[idx])

    a = pose._ransac(src, dst, pose.homography_4pt, 4, 1.0, 0.999999, 10000, np.random.default_rng(0), error=pose.transfer_error)
    b = pose._ransac(src, dst, None, 4, 1.0, 0.999999, 10000, np.random.default_rng(0), error=pose.transfer_error, solve_idx=hook)
    assert calls and calls[0] == (250, 4) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_find_fundamental_mat_is_the_parent_commits():
    g = np.load(os.path.join(ROOT, "tests", "golden", "homography_parent.npz"))
    F, mask = pose.find_fundamental_mat(g["p0"], g["p1"], threshold=1.0, prob=0.999999, max_iters=10000, seed=int(g["seed"]))
    assert np.array_equal(F, g["F"]) and np.array_equal(mask, g["mask"]) and mask.sum() > 150


# ---- the GPU tests' inputs, judged by the host code alone ------------------------------------------------------------------------
def test_gpu_solver_inputs_keep_their_caps():
    """tests/test_gpu_homography.py leaves out samples within a factor 10 of a validity threshold (at most 2 %) and needs every
    (model, point) error at least 1e-9 relative away from thr2"""
    case = C.step_case()
    assert case.idx.shape == (3, 257, 4) and case.offsets.tolist() == [0, 1000, 1000, 1065]
    for b in (0, 2):
        band = case.band[b]
        assert band.mean() <= 0.02, (b, band.mean())
        v = case.valid[b]
        assert 0.3 < v[~band].mean() < 1.0 and (~v[~band]).sum() >= 5, (b, v.mean())     # both answers occur
        s, d = case.pair(b)
        e = O.transfer_error(case.models[b][v], s, d)
        assert int((np.abs(e - C.THR2) <= 1e-9 * C.THR2).sum()) == 0
        assert ((e <= C.THR2).sum(1) >= 4).all() and (e <= C.THR2).sum(1).max() > 15      # non-trivial counts
    assert not case.valid[1].any()                                                          # the empty pair


@pytest.mark.parametrize("name", sorted(C.WARP_H))
def test_gpu_warp_inputs_keep_their_caps(name):
    """at most 1 % of a case's pixels may have an oracle value within 1e-3 of a half-integer (where rint could go either way): every
    (source, destination, channel count) of tests/test_gpu_warp.py, the first image under H and the second under its other H"""
    other = "rot_persp" if name != "rot_persp" else "half_pixel"
    for src_hw in C.WARP_SRC:
        for dst_hw in C.WARP_DST:
            for channels in (1, 3):
                img = C.noise_image(src_hw, channels, np.uint8)
                for b, nm in ((0, name), (1, other)):
                    want = O.warp_oracle(img[b], C.WARP_H[nm](src_hw, dst_hw), dst_hw)
                    near = np.abs(want - np.floor(want) - 0.5) <= 1e-3
                    assert near.mean() <= 0.01, (nm, src_hw, dst_hw, channels, near.mean())
                    if nm == "outside":
                        assert not want.any()
                    elif dst_hw != (1, 1):
                        assert want.any()


def test_warp_oracle_on_hand_values():
    img = np.arange(12, dtype=np.float64).reshape(1, 3, 4)
    assert np.array_equal(O.warp_oracle(img, np.eye(3), (3, 4)), img)
    shift = np.array([[1.0, 0, 0.5], [0, 1.0, 0], [0, 0, 1.0]])              # dst x = src x + 0.5: dst(x) = (src(x - 1) + src(x)) / 2
    got = O.warp_oracle(img, shift, (3, 4))
    assert np.array_equal(got[0, 1], [2.0, 4.5, 5.5, 6.5])                    # the left neighbour of x = 0 is outside: half of src(0)


# ---- the demo ---------------------------------------------------------------------------------------------------------------------
def test_compute_geom_and_warp_pair_on_the_demo_images():
    import torch
    from gim_amd import demo
    gd = os.path.join(ROOT, "tests", "golden", "demo")
    img0, img1 = demo.read_image(os.path.join(gd, "a1.png")), demo.read_image(os.path.join(gd, "a2.png"))
    (h0, w0), (h1, w1) = img0.shape[:2], img1.shape[:2]
    rng = np.random.default_rng(45)
    H10 = np.array([[0.95, 0.05, 12.0], [-0.04, 1.02, -7.0], [2e-5, -1e-5, 1.0]])      # image 1 -> image 0
    p1 = rng.uniform([0, 0], [w1, h1], (60, 2))
    p0 = O.proj(H10, p1)
    out = {"mkpts0_f": torch.from_numpy(p0).float(), "mkpts1_f": torch.from_numpy(p1).float(), "F": np.eye(3)}
    geom = demo.compute_geom(out, device=None)
    assert set(geom) == {"Fundamental", "Homography"} and np.array_equal(geom["Fundamental"], np.eye(3))
    assert O.corner_error(geom["Homography"], H10) < 0.05                               # fp32 matches: ~1e-4 px of input rounding
    assert demo.compute_geom({"mkpts0_f": out["mkpts0_f"][:7], "mkpts1_f": out["mkpts1_f"][:7]}) == {}
    del out["F"]
    F = demo.compute_geom({k: v[:20] for k, v in out.items()})["Fundamental"]            # no F in the dict: the seven-point RANSAC runs
    assert F is None or F.shape == (3, 3)
    calls = []

    def oracle_warp(image, H, out_hw):
        calls.append((tuple(image.shape), image.dtype, out_hw))
        sub = O.warp_oracle(image.numpy()[:, ::8, ::8], np.diag([0.125, 0.125, 1.0]) @ H @ np.diag([8.0, 8.0, 1.0]), (out_hw[0] // 8, out_hw[1] // 8))
        full = np.zeros((3, *out_hw), dtype=np.uint8)                                    # a coarse picture is enough for the plumbing
        full[:, :sub.shape[1] * 8:8, :sub.shape[2] * 8:8] = np.rint(sub)
        return torch.from_numpy(full)

    pair = demo.warp_pair(img0, img1, geom["Homography"], warp=oracle_warp)
    assert calls == [((3, h1, w1), torch.uint8, (h0, w0))]
    assert pair.shape == (h0, 2 * w0, 3) and pair.dtype == np.uint8
    assert np.array_equal(pair[:, :w0], img0) and pair[:, w0:].any()
    # the float tensors of `preprocess` are taken as well
    t0 = torch.from_numpy(img0.transpose(2, 0, 1).copy()).float()[None] / 255.0
    assert np.array_equal(demo.warp_pair(t0, img1, geom["Homography"], warp=oracle_warp)[:, :w0], img0)
