"""CPU tests of the semantic segmenter (gim_amd/semseg, tests/semseg_oracle.py): the dilated K-group table against F.conv2d through a
torch emulation of the implicit GEMM's gather, the CPU restatement against the reference's recorded outputs (tests/golden/semseg.npz,
tools/make_golden_semseg.py), the checkpoint surface, and the command line with a stubbed engine.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semseg_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gather_igemm(x_nhwc, pk, stride, pad, Ho, Wo):
    """the mainloop's A operand (igemm_mainloop.h: ktab entry -> c, dx, dy; dy == 255 = K padding; pixel (ho*stride - pad + dy,
    wo*stride - pad + dx) read only when inside the image, else zero), times the packed weights"""
    B, H, W, _ = x_nhwc.shape
    ge = 16 // pk.w.element_size()      # channels per 16-byte K group
    A = torch.zeros(B, Ho, Wo, pk.kpad)
    kt = pk.ktab.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    for grp in range(pk.kpad // ge):
        e = int(kt[grp])
        c, dx, dy = e & 0xFFFF, (e >> 16) & 0xFF, (e >> 24) & 0xFF
        if dy == 255:
            continue
        for ho in range(Ho):
            iy = ho * stride - pad + dy
            if not 0 <= iy < H:
                continue
            for wo in range(Wo):
                ix = wo * stride - pad + dx
                if 0 <= ix < W:
                    A[:, ho, wo, grp * ge:(grp + 1) * ge] = x_nhwc[:, iy, ix, c:c + ge]
    y = A.reshape(-1, pk.kpad) @ pk.w.float().cpu().t()
    if pk.bias is not None:
        y = y + pk.bias.cpu()
    return y.reshape(B, Ho, Wo, pk.npad)[..., :pk.n_store]


@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("dt,cin,cout,hw", [("fp32", 5, 12, (7, 9)), ("bf16", 12, 20, (9, 5)), ("fp16", 3, 8, (5, 11))], ids=str)
def test_dilated_ktab_addressing(d, dt, cin, cout, hw):
    from gim_amd import _lib
    from gim_amd.packing import cstore, pack_conv
    gd = {"fp32": _lib.GIM_F32, "bf16": _lib.GIM_BF16, "fp16": _lib.GIM_F16}[dt]
    g = torch.Generator().manual_seed(d * 100 + cin)
    H, W = hw
    x = torch.randn(2, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    bn = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g), torch.randn(cout, generator=g),
          torch.rand(cout, generator=g) + 0.5, 1e-5)
    pk = pack_conv(w, bn, gd, "cpu", stride=1, pad=d, dilation=d)
    assert pk.dil == d and (pk.halo is None) == (d > 1 or dt == "fp32")
    xn = torch.zeros(2, H, W, pk.cin_pad)
    xn[..., :cin] = x.permute(0, 2, 3, 1)
    if dt != "fp32":
        xn = xn.to(torch.bfloat16 if dt == "bf16" else torch.float16).float()
        x = xn[..., :cin].permute(0, 3, 1, 2)
    got = _gather_igemm(xn, pk, 1, d, H, W)
    ref = F.batch_norm(F.conv2d(x, w, padding=d, dilation=d), bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5).permute(0, 2, 3, 1)
    tol = {"fp32": 1e-5, "bf16": 3e-2, "fp16": 4e-3}[dt]     # 16-bit: the packed weights are rounded
    assert (got[..., :cout] - ref).abs().max() <= tol * ref.abs().max()
    assert (got[..., cout:] == 0).all()
    assert cstore(cin, gd) == pk.cin_pad


@pytest.mark.parametrize("k,stride,pad", [(3, 1, 1), (3, 2, 1), (1, 1, 0), (7, 2, 3)])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_undilated_packs_unchanged(k, stride, pad, dt):
    """dilation=1 (the default every existing caller uses): the table is the (dy, dx, c) walk of before, entry for entry, and the
    3x3 / pad-1 16-bit layers still get their halo pack"""
    from gim_amd import _lib
    from gim_amd.packing import KTILE_BYTES, elem_size, group_elems, pack_conv
    gd = _lib.GIM_BF16 if dt == "bf16" else _lib.GIM_F32
    w = torch.randn(24, 20, k, k, generator=torch.Generator().manual_seed(k))
    a = pack_conv(w, None, gd, "cpu", stride=stride, pad=pad)
    b = pack_conv(w, None, gd, "cpu", stride=stride, pad=pad, dilation=1)
    ge, es = group_elems(gd), elem_size(gd)
    ngrp = (a.kpad * es // KTILE_BYTES + 2) * 8
    want = []
    for grp in range(ngrp):
        tap, c = grp * ge // a.cin_pad, grp * ge % a.cin_pad
        e = (c | ((tap % k) << 16) | ((tap // k) << 24)) if tap < k * k else 0xFF000000
        want.append(e - 2 ** 32 if e >= 2 ** 31 else e)
    assert a.ktab.tolist() == want and torch.equal(a.ktab, b.ktab) and torch.equal(a.w, b.w)
    assert (a.halo is not None) == (dt == "bf16" and k == 3 and stride == 1 and pad == 1) == (b.halo is not None)
    if a.halo is not None:
        assert all(torch.equal(u, v) for u, v in zip(a.halo[:2], b.halo[:2]))


def test_dilation_range_is_checked():
    from gim_amd import _lib
    from gim_amd.packing import pack_conv
    pack_conv(torch.randn(8, 8, 3, 3), None, _lib.GIM_F32, "cpu", pad=127, dilation=127)
    with pytest.raises(AssertionError):
        pack_conv(torch.randn(8, 8, 3, 3), None, _lib.GIM_F32, "cpu", pad=128, dilation=128)


# ---- the restatement against the reference's recorded outputs -----------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "semseg.npz")))


@pytest.fixture(scope="module")
def sds():
    return O.make_state_dict(0)


@pytest.mark.parametrize("size", ["97x129", "37x45"])
def test_restatement_matches_reference(golden, sds, size):
    enc, dec = sds
    img = torch.from_numpy(golden[f"img_{size}"])[None]
    H, W = img.shape[-2:]
    assert torch.equal(img, O.seeded_image(H, W, {"97x129": 11, "37x45": 12}[size]))
    with torch.no_grad():
        r = O.segment(enc, dec, img)
    c5, ref_c5 = r["conv5"][0, ::16].numpy(), golden[f"conv5_{size}"]
    assert np.abs(c5 - ref_c5).max() <= 1e-5 * np.abs(ref_c5).max()
    pooled, ref_p = r["pooled"][0, :, :256].numpy(), golden[f"pooled_{size}"]
    assert pooled.shape == ref_p.shape == (50, 256)
    assert np.abs(pooled - ref_p).max() <= 1e-5 * np.abs(ref_p).max()
    lg, ref_lg = r["logits"][0].numpy(), golden[f"logits_{size}"]
    assert np.abs(lg - ref_lg).max() <= 1e-5 * np.abs(ref_lg).max()
    cls, ref_cls, margin = r["cls"][0].numpy(), golden[f"cls_{size}"], golden[f"margin_{size}"]
    sure = margin > 1e-6
    assert sure.mean() > 0.99
    assert (cls[sure] == ref_cls[sure]).all()
    if size == "37x45":
        assert r["conv5"].shape[-2:] == (5, 6)      # h8 x w8 below the 6 x 6 pyramid: overlapping bins


def test_state_dict_surface(golden, sds):
    from gim_amd.semseg import ModelBuilder
    enc = ModelBuilder.build_encoder(arch="resnet50dilated", fc_dim=2048, weights="")
    dec = ModelBuilder.build_decoder(arch="ppm_deepsup", fc_dim=2048, num_class=150, weights="", use_softmax=True)
    for half, mod, sd in (("enc", enc, sds[0]), ("dec", dec, sds[1])):
        own = mod.state_dict()
        assert len(own) == int(golden[half + "_keys"]) == len(sd)
        assert sum(v.numel() for v in own.values()) == int(golden[half + "_params"])
        assert set(own) == set(sd) and all(own[k].shape == sd[k].shape for k in sd)


def test_checkpoint_two_file_format_loads(tmp_path, sds):
    from gim_amd.semseg import ModelBuilder, SegmentationModule
    enc_sd, dec_sd = sds
    torch.save(enc_sd, tmp_path / "encoder_epoch_20.pth")
    torch.save(dec_sd, tmp_path / "decoder_epoch_20.pth")
    enc = ModelBuilder.build_encoder(arch="resnet50dilated", fc_dim=2048, weights=str(tmp_path / "encoder_epoch_20.pth"))
    dec = ModelBuilder.build_decoder(arch="ppm_deepsup", fc_dim=2048, num_class=150, weights=str(tmp_path / "decoder_epoch_20.pth"),
                                     use_softmax=True)
    for mod, sd in ((enc, enc_sd), (dec, dec_sd)):
        own = mod.state_dict()
        assert all(torch.equal(own[k], sd[k]) for k in sd)
    m = SegmentationModule(enc, dec, torch.nn.NLLLoss(ignore_index=-1))
    assert m.precision == "bf16" and SegmentationModule(enc, dec, None, precision="fp32").precision == "fp32"
    with pytest.raises(NotImplementedError):
        ModelBuilder.build_encoder(arch="resnet18dilated", fc_dim=512, weights="")
    with pytest.raises(NotImplementedError):
        ModelBuilder.build_decoder(arch="upernet", fc_dim=2048, weights="")


def test_dilation_schedule_matches_oracle():
    from gim_amd.semseg import ModelBuilder
    from gim_amd.semseg.model import dilation_schedule, downsample_stride
    enc = ModelBuilder.build_encoder(arch="resnet50dilated", fc_dim=2048, weights="")
    for li, (_, nblk) in enumerate(O.LAYERS, start=1):
        for bi in range(nblk):
            st, d, dst = O.block_geometry(li, bi)
            c2 = getattr(enc, f"layer{li}")[bi].conv2
            assert dilation_schedule(li, bi) == (st, d) and c2.stride == (st, st) and c2.dilation == (d, d) and c2.padding == (d, d)
            if bi == 0:
                assert downsample_stride(li) == dst


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_cli_names_skips_and_writes(tmp_path):
    from PIL import Image
    from gim_amd.semseg import __main__ as cli
    img_dir, out_dir = tmp_path / "images", tmp_path / "segment"
    img_dir.mkdir()
    for i, name in enumerate(("b.png", "a.jpg", "c.png")):
        Image.fromarray(np.full((6 + i, 8, 3), 40 * i, np.uint8)).save(img_dir / name)
    (img_dir / "notes.txt").write_text("not an image")
    out_dir.mkdir()
    np.save(out_dir / "c.npy", np.zeros((1, 1), np.uint8))     # already segmented: skipped
    a = cli.parse_args([str(img_dir), str(out_dir), "--size", "720"])
    assert a.size == 720 and a.weights_dir == "weights" and a.precision is None
    assert cli.parse_args([str(img_dir), str(out_dir)]).size == 1920
    assert cli.map_path("/x", "frame_0001.png") == os.path.join("/x", "frame_0001.npy")
    calls = []

    def stub(rgb, size, device, module):
        calls.append((rgb.shape, size, device, module))
        return np.full(rgb.shape[:2], len(calls), np.uint8)

    assert cli.main([str(img_dir), str(out_dir), "--size", "720"], module="M", segment_fn=stub) == 0
    assert [c[0] for c in calls] == [(7, 8, 3), (6, 8, 3)] and all(c[1:] == (720, "cuda", "M") for c in calls)   # sorted: a.jpg, b.png
    assert np.load(out_dir / "a.npy").tolist() == np.full((7, 8), 1, np.uint8).tolist()
    assert np.load(out_dir / "b.npy").shape == (6, 8) and np.load(out_dir / "c.npy").shape == (1, 1)
    calls.clear()
    cli.main([str(img_dir), str(out_dir)], module="M", segment_fn=stub)
    assert not calls                                            # everything has its map now


def test_segmentation_image_preprocessing():
    from gim_amd.semseg import read_segmentation_image
    rgb = (np.arange(40 * 60 * 3) % 251).astype(np.uint8).reshape(40, 60, 3)
    t = read_segmentation_image(rgb, 100)                       # no resize below the size
    ref = (torch.from_numpy(rgb).float() / 255).permute(2, 0, 1)
    ref = (ref - torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    assert torch.allclose(t, ref, atol=1e-6)
    t = read_segmentation_image(rgb, 30)                        # long side 60 -> 30, the other int(30 * 40 / 60) = 20
    assert t.shape == (3, 20, 30)
    blk = (torch.from_numpy(rgb).float() / 255).permute(2, 0, 1).reshape(3, 20, 2, 30, 2).mean((2, 4))   # integer factor: area mean
    blk = (blk - torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    assert torch.allclose(t, blk, atol=1e-5)
