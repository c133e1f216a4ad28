"""Frame preparation on the host: gim_amd/frame_prep.py (frame_prep_np, the CPU oracle of gim_frame_prep) against an fp64 coverage
oracle written here from the contract, the mask chain against the reference's three literal steps, the grey formula on every colour,
prepare_pair / label_pair_list on a synthetic video with a host bank, the export against the header, the kernel's code object, and
tools/frame_prep_host_check.cpp (csrc/frame_prep_math.h on the CPU) against the restatement.  tests/frame_prep_cases.py builds the
inputs."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_prep_cases as C  # noqa: E402
import host_check  # noqa: E402

from gim_amd import frame_prep as fp  # noqa: E402
from gim_amd import video_labels as VL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gim_hip.h")
CASES = C.cases()
IDS = [c["name"] for c in CASES]
BAND = 1e-3          # fp64 values this close to a half may round either way in fp32
CAP = 0.01           # at most this share of a case's values may lie in the band


# ---- 1, 2: the area resize ---------------------------------------------------------------------------------------------------------
def coverage_matrix(n, m):
    """[m, n] fp64: the share of destination cell d = [d s, min((d + 1) s, n)) that source cell [k, k + 1) covers, from the contract"""
    s = n / m
    a = np.arange(m, dtype=np.float64) * s
    b = np.minimum((np.arange(m, dtype=np.float64) + 1.0) * s, float(n))
    k = np.arange(n, dtype=np.float64)
    ov = np.clip(np.minimum(b[:, None], k[None] + 1.0) - np.maximum(a[:, None], k[None]), 0.0, None)
    return ov / (b - a)[:, None]


def oracle64(case):
    x0, y0, x1, y1 = case["box"]
    wn, hn = case["size"]
    src = case["frame"][y0:y1, x0:x1].astype(np.float64)
    Wx, Wy = coverage_matrix(x1 - x0, wn), coverage_matrix(y1 - y0, hn)
    return np.einsum("yk,kxc->yxc", Wy, np.einsum("dk,ykc->ydc", Wx, src))


def band_of(v):
    return np.abs(v - np.floor(v) - 0.5) <= BAND


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_resize_against_the_fp64_coverage_oracle(case):
    v = oracle64(case)
    assert np.allclose(coverage_matrix(case["box"][2] - case["box"][0], case["size"][0]).sum(1), 1.0, atol=1e-12)
    band = band_of(v)
    got = fp.frame_prep_np(case["frame"], None, [], case["box"], case["size"], fp.OUT_U8)["u8"]
    print(f"{case['name']}: {int(band.sum())} of {band.size} values within {BAND} of a half")
    assert band.sum() <= CAP * band.size, f"{int(band.sum())} of {band.size} values in the band: a wrong input, choose another seed"
    want = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    assert np.array_equal(got[~band], want[~band])
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


@pytest.mark.parametrize("case", [c for c in CASES if c["integer"]], ids=[c["name"] for c in CASES if c["integer"]])
def test_integer_factors_are_the_rounded_mean(case):
    x0, y0, x1, y1 = case["box"]
    fx, fy = case["integer"]
    wn, hn = case["size"]
    assert (x1 - x0, y1 - y0) == (wn * fx, hn * fy)
    src = case["frame"][y0:y1, x0:x1].astype(np.int64)
    sums = src.reshape(hn, fy, wn, fx, 3).sum((1, 3))
    mean = sums / float(fx * fy)                                  # exact in fp64: sums < 2^16, a power-of-two or small divisor
    got = fp.frame_prep_np(case["frame"], None, [], case["box"], case["size"], fp.OUT_U8)["u8"]
    band = band_of(mean)
    assert band.sum() <= CAP * band.size
    assert np.array_equal(got[~band], np.rint(mean).astype(np.uint8)[~band])
    if (fx, fy) == (1, 1):
        assert np.array_equal(got, case["frame"][y0:y1, x0:x1])


def test_weights_of_one_axis():
    for n, m in ((37, 16), (32, 16), (11, 16), (1, 8), (128, 8), (1920, 720), (1080, 405), (613, 1600)):
        k0, cnt, w = fp.area_weights(n, m)
        assert w.dtype == np.float32 and k0.min() >= 0 and (k0 + cnt).max() <= n and cnt.max() <= fp.MAX_FACTOR + 1
        assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() < 1e-6
        if n <= m:
            assert cnt.max() <= 2                                  # zooming: at most two source pixels per axis
    with pytest.raises(ValueError):
        fp.area_weights(129, 8)


# ---- 3: the mask chain ---------------------------------------------------------------------------------------------------------------
def nearest(img, w, h):
    """INTER_NEAREST with integer floors: dst[i, j] = src[min(i * hs // h, hs - 1), min(j * ws // w, ws - 1)]"""
    hs, ws = img.shape[:2]
    iy = np.minimum(np.arange(h) * hs // h, hs - 1)
    ix = np.minimum(np.arange(w) * ws // w, ws - 1)
    return img[iy[:, None], ix[None]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mask_chain_is_the_three_literal_steps(case):
    H, W = case["frame"].shape[:2]
    x0, y0, x1, y1 = case["box"]
    wn, hn = case["size"]
    seg = nearest(case["seg"], W, H)                               # :342-346 resize to the frame
    seg = nearest(seg[y0:y1, x0:x1], wn, hn)                       # :350-351 crop, resize to the output
    want = np.ones((hn, wn), dtype=bool)
    for cls in case["exclude"]:                                    # :359-365
        want &= seg != cls
    got = fp.frame_prep_np(case["frame"], case["seg"], case["exclude"], case["box"], case["size"], case["flags"])
    assert np.array_equal(got["mask"], want.astype(np.uint8)) and got["kept"] == int(want.sum())
    if case["flags"] & fp.OUT_MASK8:
        assert np.array_equal(got["mask8"], got["mask"][::8, ::8]) and got["mask8"].shape == (hn // 8, wn // 8)
    if case["name"] == "all-excluded":
        assert got["kept"] == 0
    if case["name"] == "none-excluded":
        assert got["kept"] == wn * hn
    with pytest.raises(ValueError):
        fp.frame_prep_np(case["frame"], case["seg"], case["exclude"], case["box"], (wn + 1, hn), fp.OUT_MASK8)


# ---- 4: grey and the fp32 outputs ------------------------------------------------------------------------------------------------------
def test_grey_on_every_colour():
    g, b = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], -1).astype(np.uint8)
        want = (np.uint32(r) * 4899 + g * 9617 + b * 1868 + 8192) // 16384
        assert np.array_equal(fp.gray_u8(rgb), want.astype(np.uint8))
    assert fp.gray_u8(np.array([[255, 255, 255]], dtype=np.uint8))[0] == 255


def test_fp32_outputs_are_the_bytes_over_255():
    frame = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16)] * 3, -1)
    frame[..., 1] = frame[..., 1][::-1]
    seg = (np.arange(256).reshape(16, 16) % 3).astype(np.uint8)
    for masked in (0, fp.MASKED):
        o = fp.frame_prep_np(frame, seg, [1], None, (16, 16), fp.ALL_FLAGS & ~fp.MASKED | masked)
        m = o["mask"] if masked else np.ones_like(o["mask"])
        assert np.array_equal(o["u8"], frame)
        for c in range(3):
            want = np.array([np.float32(int(v)) / np.float32(255.0) for v in (frame[..., c] * m).reshape(-1)], dtype=np.float32).reshape(16, 16)
            assert o["rgb"].dtype == np.float32 and o["rgb"][c].tobytes() == want.tobytes()
            nrm = np.array([(np.float32(int(v)) / np.float32(255.0) - fp.MEAN[c]) / fp.STD[c] for v in frame[..., c].reshape(-1)], dtype=np.float32)
            assert o["norm"][c].tobytes() == nrm.reshape(16, 16).tobytes()
        grey = fp.gray_u8(frame) * m
        want = np.array([np.float32(int(v)) / np.float32(255.0) for v in grey.reshape(-1)], dtype=np.float32).reshape(1, 16, 16)
        assert o["gray"].shape == (1, 16, 16) and o["gray"].tobytes() == want.tobytes()


# ---- 5: prepare_pair and label_pair_list on the host -----------------------------------------------------------------------------------
def test_pair_boxes_are_the_reference_expressions():
    rng = np.random.default_rng(5)
    H, W = 1080, 1920
    for _ in range(20):
        lo = rng.uniform(0, 600, 4)
        pts = (lo + rng.uniform(0, 1, (50, 4)) * rng.uniform(40, 1300 if _ % 2 else 470, 4)).astype(np.float32)
        pts[:, 0::2] = np.clip(pts[:, 0::2], 0, W - 0.5)
        pts[:, 1::2] = np.clip(pts[:, 1::2], 0, H - 0.5)
        pt0, pt1 = pts[:, :2], pts[:, 2:]
        got = VL.pair_boxes(pts, (H, W), (900, 1600))
        for pt, (box, wh, new) in zip((pt0, pt1), got):
            xA0, xA1 = math.floor(pt[:, 0].min()), math.ceil(pt[:, 0].max())      # :296-299
            yA0, yA1 = math.floor(pt[:, 1].min()), math.ceil(pt[:, 1].max())
            hA, wA = yA1 - yA0, xA1 - xA0                                          # :300-301
            scale = min(900 / hA, 1600 / wA)                                       # :586-591
            wn, hn = int(round(wA * scale)), int(round(hA * scale))
            wn, hn = max(wn // 8, 1) * 8, max(hn // 8, 1) * 8                      # :594-600
            assert box == (xA0, yA0, xA1, yA1) and wh == (wA, hA) and new == (wn, hn)
    with pytest.raises(ValueError):
        VL.pair_boxes(np.zeros((0, 4)), (H, W), (900, 1600))
    with pytest.raises(ValueError):
        VL.pair_boxes(np.array([[5.0, 5.0, 5.0, 5.0]]), (H, W), (900, 1600))      # an empty box


def _video(n=12, H=48, W=64):
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    segs = rng.integers(0, 4, (n, 24, 32), dtype=np.uint8)
    segs[5] = 3                                                    # frame 5: every pixel of an excluded class
    return frames, segs


def _stub_match(calls):
    """a matcher that sees the inputs' sizes only: 60 points of a random scene in two views (an exact epipolar geometry), scaled to the
    sizes of the two inputs; match.mode says per call what it returns: "ok", "none" (None: too few descriptors) or "static" (matches
    that did not move: the watermark test drops them all)"""
    def match(inputs):
        h0, w0 = inputs["image0"].shape[-2:]
        h1, w1 = inputs["image1"].shape[-2:]
        calls.append((tuple(inputs["image0"].shape), tuple(inputs["image1"].shape), str(inputs["image0"].dtype)))
        rng = np.random.default_rng(len(calls))
        X = np.stack([rng.uniform(-1, 1, 60), rng.uniform(-0.7, 0.7, 60), rng.uniform(2.5, 6, 60)], 1)
        c, s_ = np.cos(0.08), np.sin(0.08)
        R, t = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]]), np.array([0.4, 0.05, 0.02])
        Y = X @ R.T + t
        u0, u1 = X[:, :2] / X[:, 2:] * 0.6 + 0.5, Y[:, :2] / Y[:, 2:] * 0.6 + 0.5
        k0 = (u0 * [w0, h0]).astype(np.float32)
        k1 = (u1 * [w1, h1]).astype(np.float32)
        mode = match.mode.pop(0)
        if mode == "none":
            return None
        if mode == "static":
            return {"mkpts0_f": k0, "mkpts1_f": k0 + np.float32(0.25)}
        return {"mkpts0_f": k0, "mkpts1_f": k1}
    return match


def test_label_pair_list_on_a_host_bank(tmp_path):
    frames, segs = _video()
    bank = VL.FrameBank(12)
    for i in range(12):
        assert bank.put(i, frames[i], seg=segs[i]) == bank.slots([i])[0]
    ids = [(i, i + 2) for i in range(0, 10, 2)] + [(5, 7)]
    calls = []
    match = _stub_match(calls)
    match.mode = ["ok", "none", "static", "ok", "ok"]             # (0,2) ok, (2,4) None, (4,6) static, (6,8), (8,10) ok; (5,7) is not matched
    first = str(tmp_path / "first")
    r = VL.label_pair_list(match, bank, ids, "GIM_DKM", first, vratio=1.0, exclude=[3], max_iters=500)
    assert r["written"] == [(0, 2), (6, 8), (8, 10)]
    assert r["skipped"] == {(2, 4): "no match", (4, 6): "no inliers", (5, 7): "kept == 0"}
    assert len(calls) == 5 and calls[0] == ((1, 3, 48, 64), (1, 3, 48, 64), "torch.float32")
    assert sorted(os.listdir(first)) == sorted(["nums.npy", "idxs.npy"] + [str(np.array(p)) + ".npy" for p in r["written"]])
    nums, idxs = np.load(os.path.join(first, "nums.npy")), np.load(os.path.join(first, "idxs.npy"))
    assert idxs.tolist() == [[0, 2], [6, 8], [8, 10]] and len(nums) == 3
    store = VL.LabelStore.from_dirs({2: [first]})
    assert store.pairs(2) == [(0, 2), (6, 8), (8, 10)]
    for n, p in zip(nums, idxs):
        lab = store.dump(2, p)
        assert lab.dtype == np.float32 and lab.shape == (n, 4) and n >= 30
    # a second run writes nothing: every file exists; vratio scales a label (:552)
    match.mode = ["ok"]
    again = VL.label_pair_list(match, bank, ids[:1], "GIM_DKM", first, vratio=1.0, exclude=[3], max_iters=500)
    assert again["written"] == [] and again["skipped"] == {(0, 2): "exists"} and match.mode == ["ok"]
    calls.clear()
    VL.label_pair_list(match, bank, ids[:1], "GIM_DKM", str(tmp_path / "half"), vratio=0.5, exclude=[3], max_iters=500)
    assert np.array_equal(np.load(os.path.join(str(tmp_path / "half"), "[0 2].npy")), store.dump(2, (0, 2)) * np.float32(0.5))

    # the second pass consumes the first pass's files: crops to the labels' extents, the affine back to frame pixels
    second = str(tmp_path / "second")
    calls.clear()
    match.mode = ["ok"] * 3
    r2 = VL.label_pair_list(match, bank, ids, "GIM_DKM", second, vratio=1.0, exclude=[3], resize_cache=first, resize_hw=(48, 64),
                            max_iters=500)
    assert r2["written"] == [(0, 2), (6, 8), (8, 10)]
    assert r2["skipped"] == {(2, 4): "no cached label", (4, 6): "no cached label", (5, 7): "no cached label"}
    for (idx0, idx1), call in zip(r2["written"], calls):
        cached = np.load(os.path.join(first, str(np.array([idx0, idx1])) + ".npy"))
        (b0, wh0, n0), (b1, wh1, n1) = VL.pair_boxes(cached, (48, 64), (48, 64))
        assert call[0] == (1, 3, n0[1], n0[0]) and call[1] == (1, 3, n1[1], n1[0])
        lab = np.load(os.path.join(second, str(np.array([idx0, idx1])) + ".npy"))
        assert lab[:, 0].min() >= b0[0] and lab[:, 0].max() <= b0[2] and lab[:, 1].min() >= b0[1] and lab[:, 1].max() <= b0[3]
        assert lab[:, 2].min() >= b1[0] and lab[:, 2].max() <= b1[2] and lab[:, 3].min() >= b1[1] and lab[:, 3].max() <= b1[3]
    assert VL.LabelStore.from_dirs({2: [first, second]}).dump(2, (6, 8)).shape[0] == nums[1] + np.load(os.path.join(second, "nums.npy"))[1]


def test_prepare_pair_on_a_host_bank():
    frames, segs = _video()
    bank = VL.FrameBank(3)
    for i in (0, 1, 2):
        bank.put(i, frames[i], seg=segs[i])
    pts = np.array([[3.25, 4.5, 10.75, 2.25], [40.5, 33.125, 60.0, 44.875], [20.0, 20.0, 30.0, 30.0]], dtype=np.float32)
    (b0, (w0, h0), n0), (b1, (w1, h1), n1) = VL.pair_boxes(pts, (48, 64), (48, 64))
    for method in VL.METHODS:
        inputs, affine, kept = VL.prepare_pair(bank, 0, 2, method, [3], resize=(pts, (48, 64)))
        # :549: mkpts * [wA / wA_new, hA / hA_new] + [xA0, yA0]
        assert affine == (w0 / n0[0], h0 / n0[1], b0[0], b0[1], w1 / n1[0], h1 / n1[1], b1[0], b1[1])
        want0 = fp.frame_prep_np(frames[0], segs[0], [3], b0, n0, fp.ALL_FLAGS)
        want1 = fp.frame_prep_np(frames[2], segs[2], [3], b1, n1, fp.ALL_FLAGS)
        assert kept.tolist() == [want0["kept"], want1["kept"]]
        if method == "GIM_DKM":
            assert inputs["image0"].shape == (1, 3, n0[1], n0[0]) and np.array_equal(inputs["image1"][0].numpy(), want1["rgb"])
        elif method == "GIM_LOFTR":
            plain = fp.frame_prep_np(frames[0], segs[0], [3], b0, n0, fp.OUT_RGB | fp.OUT_GRAY)
            assert np.array_equal(inputs["image0"][0].numpy(), plain["gray"]) and np.array_equal(inputs["color0"][0].numpy(), plain["rgb"])
            assert np.array_equal(inputs["mask1"][0].numpy(), want1["mask8"]) and inputs["mask0"].shape == (1, n0[1] // 8, n0[0] // 8)
        elif method == "GIM_GLUE":
            assert np.array_equal(inputs["gray0"][0].numpy(), want0["gray"]) and inputs["size1"].tolist() == [[n1[0], n1[1]]]
        else:
            assert np.array_equal(inputs["rgb0"], want0["u8"]) and np.array_equal(inputs["mask1"], want1["mask"])
    inputs, affine, kept = VL.prepare_pair(bank, 1, 2, "GIM_GLUE", [3])
    assert affine is None and inputs["gray0"].shape == (1, 1, 48, 64)
    # an evicted frame raises
    bank.put(3, frames[3], seg=segs[3])
    with pytest.raises(VL.GimHipError):
        VL.prepare_pair(bank, 0, 3, "GIM_DKM", [3])
    with pytest.raises(ValueError):
        VL.prepare_pair(bank, 1, 2, "MAGIC", [3])


def test_sift_adapter_needs_opencv():
    try:
        import cv2  # noqa: F401
        cv2.SIFT_create
    except Exception:  # noqa: BLE001
        with pytest.raises(VL.GimHipError):
            VL.sift_match()


# ---- 6: the library ----------------------------------------------------------------------------------------------------------------------
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "gim_stream_t": ctypes.c_void_p}


def _header_prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*(\w+)\s+%s\s*\((.*?)\)\s*;" % name, src, re.S | re.M)
    assert m, f"{name} is not declared in include/gim_hip.h"
    args = [ctypes.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in m.group(2).split(",")]
    return _CTYPE[m.group(1)], args


def _call(fn, frames, S, H, W, seg, jobs, work, elems, outs, kept=None, jobs_dev=None, work_dev=None, excl=None):
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None   # noqa: E731
    return fn(frames, S, H, W, seg, 8, 8, excl if excl is not None else frames, vp(jobs), jobs_dev if jobs_dev is not None else frames,
              len(jobs), vp(work), work_dev if work_dev is not None else frames, len(work), vp(elems), *outs, kept, None)


def test_exports_follow_the_header_within_revision_115():
    from gim_amd import _lib
    for name, n in (("gim_frame_prep", 23), ("gim_frame_prep_tile", 6)):
        res, args = _header_prototype(name)
        fn = getattr(_lib.lib, name)
        assert (res, args) == _lib.PROTOTYPES[name] and len(args) == n
        assert fn.restype is res and list(fn.argtypes) == args
    assert _lib.ABI_VERSION == 115 and _lib.lib.gim_version() == 115
    # the tile rule of the library is the host's
    tile, err = _lib.lib.gim_frame_prep_tile, _lib.lib.gim_last_error
    tw, th = ctypes.c_int(), ctypes.c_int()
    for wc, hc, wn, hn in ((1920, 1080, 720, 405), (37, 29, 16, 8), (1600, 1600, 100, 100), (1, 1, 8, 8), (613, 344, 1600, 896), (160, 40, 10, 24)):
        assert tile(wc, hc, wn, hn, ctypes.byref(tw), ctypes.byref(th)) == 0 and (tw.value, th.value) == fp.choose_tile(wc, hc, wn, hn)
        assert fp.tile_bytes(tw.value, th.value, wc, wn, hc, hn) <= fp.LDS_BYTES
    assert tile(129, 8, 8, 8, ctypes.byref(tw), ctypes.byref(th)) != 0 and b"more than 16" in err()
    # an empty batch returns before anything is touched; malformed calls are refused before a launch
    fn = _lib.lib.gim_frame_prep
    assert fn(*([None, 0, 0, 0, None, 0, 0] + [None] * 3 + [0, None, None, 0] + [None] * 9)) == 0
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    H, W = 40, 160
    good = fp.plan((H, W), [(0, (3, 4, 40, 33), (16, 8), fp.OUT_U8)])
    elems = np.array([10 ** 6] * 6, dtype=np.int64)
    outs = [p] * 6

    def refused(word, jobs=good.jobs, work=good.work, elems=elems, outs=outs, **kw):
        rc = _call(fn, p, 1, H, W, p, jobs, work, elems, outs, **kw)
        assert rc != 0 and word in err(), (rc, err())

    def job(**kw):
        j = good.jobs.copy()
        names = ["slot", "x0", "y0", "x1", "y1", "wn", "hn", "flags", "o0", "o1", "o2", "o3", "o4", "o5", "tw", "th"]
        for k, v in kw.items():
            j[0, names.index(k)] = v
        return j

    refused(b"slot", jobs=job(slot=1))
    refused(b"box", jobs=job(x1=W + 1))
    refused(b"box", jobs=job(x0=40))
    refused(b"output", jobs=job(wn=0))
    for box, size in C.REFUSED:                                    # a factor above 16, on either axis
        refused(b"more than 16", jobs=job(x0=box[0], y0=box[1], x1=box[2], y1=box[3], wn=size[0], hn=size[1]))
        with pytest.raises(ValueError):
            fp.plan((H, W), [(0, box, size, fp.OUT_U8)])
    refused(b"flags", jobs=job(flags=128))
    refused(b"mask8", jobs=job(flags=fp.OUT_MASK8, wn=12))
    refused(b"tile", jobs=job(tw=65))
    refused(b"tile", jobs=job(x0=0, x1=160, wn=10, hn=24, y0=3, y1=36))   # the largest tile does not fit a factor of 16
    refused(b"leaves its buffer", elems=np.array([16 * 8 * 3 - 1] * 6, dtype=np.int64))
    refused(b"leaves its buffer", jobs=job(o0=-1))
    refused(b"is NULL", outs=[None] * 6)
    refused(b"work item", work=np.array([[1, 0, 0, 0]], dtype=np.int32))
    refused(b"work item", work=np.array([[0, 16, 0, 0]], dtype=np.int32))
    refused(b"work item", work=np.array([[0, 0, 3, 0]], dtype=np.int32))
    refused(b"aligned", jobs_dev=ctypes.c_void_p(p.value + 4))
    refused(b"aligned", work_dev=ctypes.c_void_p(p.value + 8))
    refused(b"aligned", excl=ctypes.c_void_p(p.value + 1))
    rc = _call(fn, None, 1, H, W, p, good.jobs, good.work, elems, outs)
    assert rc != 0 and b"NULL" in err()
    rc = fn(p, 1, H, W, None, 0, 0, p, good.jobs.ctypes.data_as(ctypes.c_void_p), p, 1, good.work.ctypes.data_as(ctypes.c_void_p), p, 1,
            elems.ctypes.data_as(ctypes.c_void_p), *outs, p, None)
    assert rc != 0 and b"class maps" in err()                      # kept without class maps


def test_kernel_targets_gfx950_without_scratch():
    """frame_prep_kernel: no scratch and no spilled vector register; 46 KiB of LDS (three workgroups per CU) is the plan"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources_cpu.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    hit = [(n, v) for n, v in kr._kernels().items() if "frame_prep_kernel" in n]
    assert len(hit) == 1, "frame_prep_kernel not found in the library"
    for n, (regs, scratch, spills) in hit:
        print(f"{n[:48]}: {regs} VGPRs, {scratch} B scratch, {spills} spills")
        assert scratch == 0 and spills == 0 and regs <= 128, (n, regs, scratch, spills)


# ---- 7: the header on the CPU ----------------------------------------------------------------------------------------------------------
def _lcg_bytes(seed, n):
    out, x = np.empty(n, dtype=np.uint8), seed
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = x >> 24
    return out


def test_host_check_agrees_with_the_numpy_oracle(tmp_path):
    """tools/frame_prep_host_check.cpp is plain C++ over the kernel's header; built with the host compiler (no sanitizer here: that
    run is a development step, recorded in the README), every byte it prints is frame_prep_np's"""
    r = host_check.run("frame_prep_host_check", tmp_path, "-ffp-contract=off")
    assert r.stdout.strip().endswith("OK"), r.stdout[-2000:]
    lines = r.stdout.strip().split("\n")
    assert (len(lines) - 1) % 7 == 0 and len(lines) >= 50
    for i in range(0, len(lines) - 1, 7):
        head = lines[i].split()
        assert head[0] == "case"
        n, H, W, Hs, Ws, x0, y0, x1, y1, wn, hn, flags, tw, th, kept = (int(v) for v in head[1:])
        raw = _lcg_bytes(1000 + n, H * W * 3 + Hs * Ws)
        frame, seg = raw[:H * W * 3].reshape(H, W, 3), (raw[H * W * 3:] % 7).reshape(Hs, Ws)
        flags_np = fp.ALL_FLAGS & ~fp.MASKED | (flags & fp.MASKED)
        if wn % 8 or hn % 8:
            flags_np &= ~fp.OUT_MASK8
        want = fp.frame_prep_np(frame, seg, [2, 5], (x0, y0, x1, y1), (wn, hn), flags_np)
        assert kept == want["kept"] and (tw, th) == fp.choose_tile(x1 - x0, y1 - y0, wn, hn)
        for k, name in enumerate(fp.OUTPUTS):
            tag, _, hexed = lines[i + 1 + k].partition(" ")
            assert tag == name
            if name in want:
                assert bytes.fromhex(hexed) == want[name].tobytes(), (n, name)
