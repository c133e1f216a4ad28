"""GPU tests of the semantic segmenter (gim_amd/semseg, csrc/semseg.hip): dilated convolutions on the implicit GEMM, the three PPM /
head kernels against torch on the device, the engine end to end against the CPU restatement (tests/semseg_oracle.py), the fp16 fallback
and the round trip through `python -m gim_amd.semseg` into the hloc plugin's segment-mask reader."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semseg_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _gd(p):
    from gim_amd import _lib
    return {"bf16": _lib.GIM_BF16, "fp16": _lib.GIM_F16, "fp32": _lib.GIM_F32}[p]


# ---- dilated convolutions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("hw", [(9, 13), (21, 17)], ids=str)
def test_dilated_conv_launch(d, prec, hw):
    from gim_amd import ops
    from gim_amd._lib import ACT_RELU
    from gim_amd.packing import pack_conv
    g = torch.Generator().manual_seed(d * 10 + hw[0])
    cin, cout, (H, W) = 72, 64, hw
    x = torch.randn(2, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    res = torch.randn(2, cout, H, W, generator=g)
    bn = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1,
          torch.rand(cout, generator=g) + 0.5, 1e-5)
    pk = pack_conv(w, bn, _gd(prec), DEV, pad=d, dilation=d)
    xt = x.permute(0, 2, 3, 1).contiguous().to(TDT[prec])
    rt = res.permute(0, 2, 3, 1).contiguous().to(TDT[prec])
    y = ops.conv2d(xt.to(DEV), pk, ACT_RELU, res=rt.to(DEV))
    assert y.shape == (2, H, W, cout)
    xr, rr = xt.float().permute(0, 3, 1, 2).to(DEV), rt.float().permute(0, 3, 1, 2).to(DEV)
    ref = F.batch_norm(F.conv2d(xr, w.to(DEV), padding=d, dilation=d), bn[2].to(DEV), bn[3].to(DEV), bn[0].to(DEV), bn[1].to(DEV),
                       False, 0.0, 1e-5)
    ref = F.relu(ref + rr).permute(0, 2, 3, 1)
    tol = {"fp32": 1e-4, "bf16": 3e-2, "fp16": 4e-3}[prec]
    err = (y.float() - ref).abs().max().item() / ref.abs().max().item()
    assert err <= tol, err


# ---- the PPM kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(13, 17), (5, 6), (3, 2), (1, 1), (60, 80)], ids=str)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_ppm_pool(hw, prec):
    from gim_amd import ops
    H, W = hw
    C, ld = 2048, 4096
    g = torch.Generator().manual_seed(H * W)
    buf = torch.rand(2, H, W, ld, generator=g).to(TDT[prec])
    got = ops.ppm_pool(buf.to(DEV), C).cpu()
    x = buf[..., :C].double().permute(0, 3, 1, 2)
    ref = torch.cat([F.adaptive_avg_pool2d(x, s).flatten(2) for s in ops.PPM_SCALES], 2).transpose(1, 2)
    err = ((got.double() - ref).abs().max() / ref.abs().max()).item()
    assert err <= 1e-6, err


@pytest.mark.parametrize("hw", [(13, 17), (5, 6), (2, 3), (135, 240)], ids=str)
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_ppm_upsample_concat(hw, prec):
    from gim_amd import ops
    h, w = hw
    g = torch.Generator().manual_seed(h + w)
    br = torch.randn(2, 50, 512, generator=g)
    cat = torch.full((2, h, w, 4096), 7.0, dtype=TDT[prec], device=DEV)
    ops.ppm_upsample_concat(br.to(DEV), cat, 2048)
    brd = br.to(DEV)
    ref = []
    for s in ops.PPM_SCALES:
        off = ops.PPM_OFFSETS[s]
        src = brd[:, off:off + s * s].transpose(1, 2).reshape(2, 512, s, s)
        ref.append(F.interpolate(src, (h, w), mode="bilinear", align_corners=False))
    ref = torch.cat(ref, 1).permute(0, 2, 3, 1)
    got = cat[..., 2048:].float()
    assert (cat[..., :2048] == 7.0).all()                     # conv5's channels untouched
    if prec == "fp32":
        ulp = torch.finfo(torch.float32).eps * ref.abs().clamp_min(1.0)
        assert ((got - ref).abs() <= 2 * ulp).all(), (got - ref).abs().max().item()
    else:
        assert torch.equal(got, ref.to(torch.float16).float()) or (got - ref).abs().max().item() <= 1e-3 * ref.abs().max().item()


def _h8(n):
    return -(-(-(-(-(-n // 2)) // 2)) // 2)


@pytest.mark.parametrize("size", [(97, 129), (1080, 1920), (1439, 1917)], ids=str)
def test_seg_head_argmax(size):
    from gim_amd import ops
    H, W = size
    h, w = _h8(H), _h8(W)
    g = torch.Generator().manual_seed(H)
    lg = (torch.randn(1, h, w, 152, generator=g) * 4).to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    cls, prob = ops.seg_head_argmax(lg, 150, (H, W), prob=True, flag=flag)
    torch.cuda.synchronize()
    x = F.interpolate(lg[..., :150].permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
    top = x.topk(2, dim=1).values
    margin = top[:, 0] - top[:, 1]
    rprob, rcls = F.softmax(x, dim=1).max(dim=1)
    del x
    diff = cls.long() != rcls
    assert not bool((diff & (margin >= 1e-5)).any()), int((diff & (margin >= 1e-5)).sum())
    assert (prob - rprob).abs().max().item() <= 1e-6
    assert int(flag.item()) == 0
    if size == (1080, 1920):
        for _ in range(3):
            ops.seg_head_argmax(lg, 150, (H, W))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.seg_head_argmax(lg, 150, (H, W))
        e1.record()
        torch.cuda.synchronize()
        print(f"\nseg_head_argmax 1080x1920 (logits {h}x{w}x150): {e0.elapsed_time(e1) / 20 * 1000:.1f} us")
        lg[0, 3, 5, 7] = float("nan")
        ops.seg_head_argmax(lg, 150, (H, W), flag=flag)
        assert int(flag.item()) == 1


# ---- the engine end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sds():
    return O.make_state_dict(0)


def _module(sds, precision):
    from gim_amd.semseg import ModelBuilder, SegmentationModule
    enc = ModelBuilder.build_encoder(arch="resnet50dilated", fc_dim=2048, weights="")
    dec = ModelBuilder.build_decoder(arch="ppm_deepsup", fc_dim=2048, num_class=150, weights="", use_softmax=True)
    enc.load_state_dict(sds[0])
    dec.load_state_dict(sds[1])
    return SegmentationModule(enc, dec, torch.nn.NLLLoss(ignore_index=-1), precision=precision).to(DEV).eval()


_ORACLE = {}


def _oracle(sds, H, W):
    if (H, W) not in _ORACLE:
        img = O.seeded_image(H, W, H + W)
        with torch.no_grad():
            _ORACLE[(H, W)] = (img, O.segment(sds[0], sds[1], img))
    return _ORACLE[(H, W)]


# flip-rate bounds of the 16-bit modes = twice the rate measured on MI355X (97x129 / 480x640, seeded weights of semseg_oracle)
# (measured: bf16 0.47 % / 0.028 %, fp16 0.10 % / 0.007 %; worst flipped pixel's oracle top-2 margin 3.0e-3 / 2.6e-4 of the logit scale)
FLIP_BOUND = {"bf16": 0.0095, "fp16": 0.0021}
MARGIN_FRAC = {"bf16": 0.006, "fp16": 0.0006}    # a flipped pixel's oracle top-2 margin, in units of the logit scale


@pytest.mark.parametrize("size", [(97, 129), (480, 640)], ids=str)
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_end_to_end_against_restatement(sds, size, prec):
    H, W = size
    img, ref = _oracle(sds, H, W)
    m = _module(sds, prec)
    with torch.no_grad():
        lg = m.logits(img.to(DEV)).cpu()
        cls = m.segment(img.to(DEV), (H, W)).cpu()[0]
    scale = ref["logits"].abs().max().item()
    lerr = (lg - ref["logits"]).abs().max().item() / scale
    rcls, margin = ref["cls"][0], ref["margin"][0]
    flips = cls.long() != rcls
    rate = flips.float().mean().item()
    worst = margin[flips].max().item() / scale if bool(flips.any()) else 0.0
    print(f"\n{prec} {H}x{W}: logits err {lerr:.2e} of scale {scale:.1f}; class flips {int(flips.sum())}/{flips.numel()} "
          f"({rate:.5f}), worst flipped margin {worst:.2e} of scale")
    if prec == "fp32":
        assert lerr <= 1e-4
        assert worst < 1e-4
    else:
        assert rate <= FLIP_BOUND[prec], rate
        assert worst <= MARGIN_FRAC[prec], worst


def test_reference_scores_contract(sds):
    """module(feed_dict, segSize=...) returns the reference's softmax scores [B,150,H,W]"""
    img, ref = _oracle(sds, 97, 129)
    m = _module(sds, "fp32")
    with torch.no_grad():
        scores = m({"img_data": img.to(DEV)}, segSize=(97, 129))
    assert scores.shape == (1, 150, 97, 129)
    _, pred = torch.max(scores, dim=1)
    sure = ref["margin"][0] > 1e-4 * ref["logits"].abs().max()
    assert torch.equal(pred.cpu()[0][sure], ref["cls"][0][sure])
    assert (scores.sum(1) - 1).abs().max().item() < 1e-4


def test_fp16_overflow_falls_back_to_fp32(sds):
    enc, dec = dict(sds[0]), dict(sds[1])
    for k in ("layer4.2.bn3.weight", "layer4.2.bn3.bias"):
        enc[k] = enc[k] * 3e4                                   # the last residual store leaves the fp16 range
    big = (enc, dec)
    img = O.seeded_image(97, 129, 5).to(DEV)
    m16, m32 = _module(big, "fp16"), _module(big, "fp32")
    with torch.no_grad():
        ref = m32.segment(img, (97, 129))
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter("always")
            got = m16.segment(img, (97, 129))
    assert any("repeating it in fp32" in str(w.message) for w in wl), [str(w.message) for w in wl]
    assert torch.equal(got, ref)


def test_cli_into_hloc_plugin(tmp_path, sds):
    from PIL import Image
    img_dir, wdir = tmp_path / "images", tmp_path / "weights"
    img_dir.mkdir()
    wdir.mkdir()
    torch.save(sds[0], wdir / "encoder_epoch_20.pth")
    torch.save(sds[1], wdir / "decoder_epoch_20.pth")
    g = torch.Generator().manual_seed(9)
    for name in ("a.png", "b.png"):
        low = torch.rand(3, 15, 20, generator=g)
        im = F.interpolate(low[None], size=(240, 320), mode="bilinear", align_corners=False)[0]
        Image.fromarray((im.permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(img_dir / name)
    seg = tmp_path / "outputs" / "segment"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "gim_amd.semseg", str(img_dir), str(seg), "--weights-dir", str(wdir), "--precision", "fp32"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    maps = {n: np.load(seg / f"{n}.npy") for n in ("a", "b")}
    assert all(v.dtype == np.uint8 and v.shape == (240, 320) for v in maps.values())
    # the same maps through the in-process entry point
    from gim_amd.semseg import segment
    m = _module(sds, "fp32")
    with torch.no_grad():
        direct = segment(np.asarray(Image.open(img_dir / "a.png").convert("RGB")), 1920, DEV, m)
    assert np.array_equal(direct, maps["a"])
    # the plugin reads $GIMRECONSTRUCTION/../segment/<name>.npy and blacks out class-0 pixels (hloc/matchers/dkm.py:63-90)
    import dkm_oracle as DO
    import gim_amd.hloc_matchers as plugins
    from hloc.utils.base_model import dynamic_load
    Model = dynamic_load(plugins, "gim_dkm_hip")
    pm = Model({"max_num_matches": 300}).eval().to(DEV)
    pm.net.load_state_dict(DO.make_state_dict(0))
    seen = {}
    real = pm.adapter.forward

    def spy(d):
        seen.update(d)
        return real(d)

    pm.adapter.forward = spy
    old = os.environ.get("GIMRECONSTRUCTION")
    (tmp_path / "outputs" / "gim_dkm").mkdir()                  # reconstruction.py:58-60: the version directory exists
    os.environ["GIMRECONSTRUCTION"] = str(tmp_path / "outputs" / "gim_dkm")
    try:
        im0, im1 = DO.seeded_pair(240, 320, 3)
        pred = pm({"image0": im0.cuda(), "image1": im1.cuda(), "name0": ["a.png"], "name1": ["b.png"]})
    finally:
        if old is None:
            del os.environ["GIMRECONSTRUCTION"]
        else:
            os.environ["GIMRECONSTRUCTION"] = old
    assert np.array_equal(seen["mask0"], maps["a"]) and np.array_equal(seen["mask1"], maps["b"])
    assert {"keypoints0", "keypoints1", "scores"} <= set(pred)
