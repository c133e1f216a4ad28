"""GPU tests of the perspective warp (gim_amd/csrc/warp.hip through ops.warp_perspective) against the numpy fp64 oracle of
tests/homography_oracle.py (the operator's own stated formula, not cv2's fixed-point bytes), and of `python -m gim_amd.demo --out`.

fp32 bar: |device - oracle| <= 8 * 2^-24 * max|src| -- weights rounded once, four fp32 products and three additions, a factor two on
top; the border-blended bilinear form is continuous, so a coordinate that rounds across an integer moves the value by no more.
uint8 bar: equal to rint(oracle) except where the oracle's value lies within 1e-3 of a half-integer; at most 1 % of a case's pixels
may be left out for that (tests/test_homography_cpu.py checks the cap on the oracle alone).  The identity on a same-size destination
returns the source exactly, both dtypes."""
import os

import numpy as np
import pytest
import torch

import homography_cases as C
import homography_oracle as O
from gim_amd import ops
from gim_amd._lib import GimHipError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(got, img, H, dst_hw, name):
    """got [C, hd, wd] from the device against the oracle on img [C, hs, ws]"""
    want = O.warp_oracle(img, H, dst_hw)
    assert got.shape == want.shape, (got.shape, want.shape)
    if img.dtype == np.uint8:
        near = np.abs(want - np.floor(want) - 0.5) <= 1e-3
        assert near.mean() <= 0.01
        bad = (got.astype(np.int64) != np.rint(want).astype(np.int64)) & ~near
        assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4])
    else:
        err, bound = np.abs(got.astype(np.float64) - want).max(), 8 * 2.0 ** -24 * float(np.abs(img).max())
        assert err <= bound, (name, err, bound)
    if name == "outside":
        assert not got.any()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", sorted(C.WARP_H))
def test_warp_against_the_oracle(name, channels, dtype):
    for src_hw in C.WARP_SRC:
        img = C.noise_image(src_hw, channels, dtype)
        d_img = torch.from_numpy(img.copy()).to(DEV)
        for dst_hw in C.WARP_DST:
            H = C.WARP_H[name](src_hw, dst_hw)
            one = ops.warp_perspective(d_img[0], H, dst_hw)                     # [C, H, W], H as an array
            assert one.dtype == d_img.dtype and one.shape == (channels, *dst_hw)
            _compare(one.cpu().numpy(), img[0], H, dst_hw, name)
            # B = 2 with another H for the second image, H as a tensor
            H2 = np.stack([H, C.WARP_H["rot_persp" if name != "rot_persp" else "half_pixel"](src_hw, dst_hw)])
            two = ops.warp_perspective(d_img, torch.from_numpy(H2), dst_hw).cpu().numpy()
            assert np.array_equal(two[0], one.cpu().numpy())
            _compare(two[1], img[1], H2[1], dst_hw, "second")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_identity_returns_the_source(dtype):
    for src_hw in C.WARP_SRC:
        img = C.noise_image(src_hw, 3, dtype)
        got = ops.warp_perspective(torch.from_numpy(img.copy()).to(DEV), np.eye(3), src_hw)
        assert np.array_equal(got.cpu().numpy(), img)
        scaled = ops.warp_perspective(torch.from_numpy(img.copy()).to(DEV), -3.0 * np.eye(3), src_hw)      # H is homogeneous
        assert np.array_equal(scaled.cpu().numpy(), img)


def test_singular_and_malformed_arguments_raise_before_any_launch(monkeypatch):
    img = torch.from_numpy(C.noise_image((5, 7), 3, np.uint8).copy()).to(DEV)

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")

    monkeypatch.setattr(ops, "lib", NoLaunch())
    for H in (np.zeros((3, 3)), np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 0]]),
              np.array([[1.0, 0, np.nan], [0, 1, 0], [0, 0, 1]]), np.array([[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]])):
        with pytest.raises(GimHipError):
            ops.warp_perspective(img, H, (4, 4))
    with pytest.raises(GimHipError):
        ops.warp_perspective(img, np.stack([np.eye(3), np.zeros((3, 3))]), (4, 4))      # one of two is singular
    with pytest.raises(GimHipError):
        ops.warp_perspective(img, np.eye(4), (4, 4))
    with pytest.raises(GimHipError):
        ops.warp_perspective(img.to(torch.int32), np.eye(3), (4, 4))
    with pytest.raises(GimHipError):
        ops.warp_perspective(torch.zeros(1, 5, 4, 4, device=DEV), np.eye(3), (4, 4))    # five channels
    with pytest.raises(GimHipError):
        ops.warp_perspective(img.permute(0, 1, 3, 2), np.eye(3), (4, 4))                # not contiguous
    assert ops.warp_perspective(img, np.eye(3), (0, 4)).shape == (2, 3, 0, 4)           # an empty destination: no launch


def test_demo_writes_the_warp_png(tmp_path):
    """`--out` on the seeded init of gim_loftr: a PNG of [H0, 2 W0] pixels when a homography was found, nothing with fewer than 8
    matches or no model; without `--out` nothing new (the returned dict has no `geom`)"""
    from PIL import Image

    from gim_amd import demo
    a1, a2 = (os.path.join(ROOT, "tests", "golden", "demo", n) for n in ("a1.png", "a2.png"))
    out = demo.main(["--model", "gim_loftr", "--image0", a1, "--image1", a2, "--out", str(tmp_path)])
    files = sorted(os.listdir(tmp_path))
    n = len(out["mconf"])
    if n < 8:
        assert out["geom"] == {} and files == []
    elif out["geom"]["Homography"] is None:
        assert files == []
    else:
        assert files == ["a1_a2_gim_loftr_warp.png"]
        h0, w0 = out["hw0_i"]
        im = Image.open(os.path.join(tmp_path, files[0]))
        assert im.size == (2 * w0, h0) and im.mode == "RGB"
        left = np.asarray(im)[:, :w0]
        assert np.array_equal(left, (out["color0"][0].float() * 255.0).round().clamp(0, 255).byte().permute(1, 2, 0).cpu().numpy())


def test_warp_pair_on_the_device():
    """demo.warp_pair through ops.warp_perspective: crops of the demo images (uint8 arrays, and the float tensors `preprocess`
    makes), left half = image 0 byte for byte, right half = rint of the oracle's warp of image 1"""
    from gim_amd import demo
    a1, a2 = (demo.read_image(os.path.join(ROOT, "tests", "golden", "demo", n)) for n in ("a1.png", "a2.png"))
    img0, img1 = np.ascontiguousarray(a1[100:300, 200:460]), np.ascontiguousarray(a2[50:230, 300:540])
    H = np.array([[1.05, 0.08, -6.0], [-0.06, 0.97, 11.0], [1e-4, -2e-4, 1.0]])
    pair = demo.warp_pair(img0, img1, H, device=DEV)
    assert pair.shape == (200, 520, 3) and pair.dtype == np.uint8 and np.array_equal(pair[:, :260], img0)
    want = O.warp_oracle(img1.transpose(2, 0, 1), H, (200, 260))
    near = np.abs(want - np.floor(want) - 0.5) <= 1e-3
    assert near.mean() <= 0.01 and want.any()
    bad = (pair[:, 260:].transpose(2, 0, 1).astype(np.int64) != np.rint(want).astype(np.int64)) & ~near
    assert not bad.any(), int(bad.sum())
    t0 = torch.from_numpy(img0.transpose(2, 0, 1).copy()).float().div(255.0)[None].to(DEV)
    t1 = torch.from_numpy(img1.transpose(2, 0, 1).copy()).float().div(255.0)[None].to(DEV)
    assert np.array_equal(demo.warp_pair(t0, t1, H, device=DEV), pair)
