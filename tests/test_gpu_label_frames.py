"""The video labeller's frame stage on the device: semseg.segment_device against the module fed with frame_prep_np's input,
video_labels.prepare_pair for the three GPU matchers, label_pair_list with a seeded LoFTR in both passes against the same steps done
by hand with frame_prep_np inputs, and the eviction rule of FrameBank."""
import os

import numpy as np
import pytest
import torch

import semseg_oracle as SO
from gim_amd import frame_prep as fp
from gim_amd import semseg
from gim_amd import video_labels as VL
from gim_amd._lib import GimHipError
from tools import synth_loftr as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXCLUDE = [3]


def _frames(n=3, H=96, W=128):
    """frames of one textured canvas seen through a moving window: consecutive frames share most of their content"""
    g = torch.Generator().manual_seed(11)
    canvas = S.textured(1, H + 8 * n, W + 16 * n, g)[0]
    frames = [(canvas[:, 8 * i:8 * i + H, 16 * i:16 * i + W] * 255).round().byte().permute(1, 2, 0).contiguous().numpy() for i in range(n)]
    rng = np.random.default_rng(5)
    segs = [np.kron(rng.integers(0, 4, (6, 8)), np.ones((8, 8), dtype=np.int64)).astype(np.uint8) for _ in range(n)]   # 48 x 64, class 3 excluded
    return frames, segs


def test_segment_device_is_the_module_on_the_contract_input():
    from gim_amd.semseg import ModelBuilder, SegmentationModule
    sds = SO.make_state_dict(0)
    enc = ModelBuilder.build_encoder(arch="resnet50dilated", fc_dim=2048, weights="")
    dec = ModelBuilder.build_decoder(arch="ppm_deepsup", fc_dim=2048, num_class=150, weights="", use_softmax=True)
    enc.load_state_dict(sds[0])
    dec.load_state_dict(sds[1])
    module = SegmentationModule(enc, dec, torch.nn.NLLLoss(ignore_index=-1), precision="fp32").to(DEV).eval()
    frame = np.random.default_rng(9).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    for size, hw in ((64, (42, 64)), (720, (64, 96))):             # resized (96 x 64 -> 64 x 42) and at its own size
        got = semseg.segment_device(torch.from_numpy(frame).to(DEV), size, module)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1,) + hw
        norm = fp.frame_prep_np(frame, None, [], None, (hw[1], hw[0]), fp.OUT_NORM)["norm"]
        with torch.no_grad():
            want = module.segment(torch.from_numpy(norm)[None].to(DEV), hw)
        assert torch.equal(got[0].long(), want[0].long())
    # at its own size the contract input is `segment`'s input, so the class map is `segment`'s
    assert np.array_equal(got[0].cpu().numpy(), semseg.segment(frame, 720, DEV, module))
    # a bank with a module segments on `put`
    bank = VL.FrameBank(2, DEV, module=module, seg_size=64)
    bank.put(7, frame)
    assert torch.equal(bank.seg[bank.slots([7])[0]], semseg.segment_device(torch.from_numpy(frame).to(DEV), 64, module)[0])


def _bank(frames, segs, capacity=3):
    bank = VL.FrameBank(capacity, DEV)
    for i, (f, s) in enumerate(zip(frames, segs)):
        bank.put(i, f, seg=s)
    return bank


def test_prepare_pair_has_the_shapes_the_modules_accept():
    frames, segs = _frames()
    bank = _bank(frames, segs)
    pts = np.array([[10.5, 8.25, 20.0, 12.5], [100.75, 80.5, 120.25, 90.0]], dtype=np.float32)
    (b0, _, n0), (b1, _, n1) = VL.pair_boxes(pts, (96, 128), (96, 128))
    for resize, (s0, s1) in ((None, ((128, 96), (128, 96))), ((pts, (96, 128)), (n0, n1))):
        want = [fp.frame_prep_np(frames[i], segs[i], EXCLUDE, b, s, fp.ALL_FLAGS) for i, b, s in
                ((0, b0 if resize else None, s0), (2, b1 if resize else None, s1))]
        plain = [fp.frame_prep_np(frames[i], segs[i], EXCLUDE, b, s, fp.OUT_RGB | fp.OUT_GRAY) for i, b, s in
                 ((0, b0 if resize else None, s0), (2, b1 if resize else None, s1))]
        for method in ("GIM_DKM", "GIM_LOFTR", "GIM_GLUE"):
            inputs, affine, kept = VL.prepare_pair(bank, 0, 2, method, EXCLUDE, resize)
            assert (affine is None) == (resize is None) and kept.is_cuda and kept.dtype == torch.int32
            assert kept.tolist() == [want[0]["kept"], want[1]["kept"]]
            eq = lambda t, a: t.is_cuda and tuple(t.shape) == (1,) + a.shape and t.cpu().numpy().tobytes() == a.tobytes()   # noqa: E731
            if method == "GIM_DKM":
                assert sorted(inputs) == ["image0", "image1"] and inputs["image0"].dtype == torch.float32
                assert eq(inputs["image0"], want[0]["rgb"]) and eq(inputs["image1"], want[1]["rgb"])
                assert tuple(inputs["image0"].shape) == (1, 3, s0[1], s0[0])
            elif method == "GIM_LOFTR":
                assert eq(inputs["image0"], plain[0]["gray"]) and eq(inputs["color1"], plain[1]["rgb"])
                assert eq(inputs["mask0"], want[0]["mask8"]) and eq(inputs["mask1"], want[1]["mask8"]) and inputs["mask0"].dtype == torch.uint8
                assert tuple(inputs["image1"].shape) == (1, 1, s1[1], s1[0]) and tuple(inputs["mask1"].shape) == (1, s1[1] // 8, s1[0] // 8)
            else:
                assert eq(inputs["gray0"], want[0]["gray"]) and eq(inputs["gray1"], want[1]["gray"])
                assert inputs["size0"].tolist() == [[s0[0], s0[1]]] and inputs["size1"].tolist() == [[s1[0], s1[1]]]


def _by_hand(model, frames, segs, i0, i1, resize, seed):
    jobs, affine = [(i0, None, (128, 96)), (i1, None, (128, 96))], None
    if resize is not None:
        (b0, (w0, h0), n0), (b1, (w1, h1), n1) = VL.pair_boxes(resize, (96, 128), (96, 128))
        jobs = [(i0, b0, n0), (i1, b1, n1)]
        affine = (w0 / n0[0], h0 / n0[1], b0[0], b0[1], w1 / n1[0], h1 / n1[1], b1[0], b1[1])
    a, b = (fp.frame_prep_np(frames[i], segs[i], EXCLUDE, box, size, fp.OUT_RGB | fp.OUT_GRAY | fp.OUT_MASK8) for i, box, size in jobs)
    up = lambda x: torch.from_numpy(x)[None].to(DEV)   # noqa: E731
    data = {"image0": up(a["gray"]), "image1": up(b["gray"]), "color0": up(a["rgb"]), "color1": up(b["rgb"]), "mask0": up(a["mask8"]),
            "mask1": up(b["mask8"])}
    model(data)
    return VL.label_pair(data, device=DEV, affine=affine, vratio=1.0, seed=seed, max_iters=2000)


def test_label_pair_list_with_loftr_in_both_passes(tmp_path):
    frames, segs = _frames()
    bank = _bank(frames, segs)
    model, _ = S.synthetic_model("fp32")
    model = model.to(DEV)
    first, second = str(tmp_path / "first"), str(tmp_path / "second")
    ids = [(0, 1), (1, 2)]
    r = VL.label_pair_list(VL.loftr_match(model), bank, ids, "GIM_LOFTR", first, vratio=1.0, exclude=EXCLUDE, seed=4, max_iters=2000)
    assert r["written"] == ids, r
    for i0, i1 in ids:
        got = np.load(os.path.join(first, str(np.array([i0, i1])) + ".npy"))
        want = _by_hand(model, frames, segs, i0, i1, None, 4)
        print(f"first pass ({i0}, {i1}): {len(got)} rows")
        assert got.dtype == np.float32 and len(got) >= 8 and torch.equal(torch.from_numpy(got), want.cpu())
    r = VL.label_pair_list(VL.loftr_match(model), bank, ids, "GIM_LOFTR", second, vratio=1.0, exclude=EXCLUDE, resize_cache=first,
                           resize_hw=(96, 128), seed=4, max_iters=2000)
    assert len(r["written"]) >= 1, r                               # the crops differ in scale: the seeded network need not match every one
    for i0, i1 in ids:
        cached = np.load(os.path.join(first, str(np.array([i0, i1])) + ".npy"))
        want = _by_hand(model, frames, segs, i0, i1, cached, 4)
        if (i0, i1) not in r["written"]:                           # ... but then the steps done by hand give no label either
            assert r["skipped"][(i0, i1)] == "no inliers" and len(want) == 0
            continue
        got = np.load(os.path.join(second, str(np.array([i0, i1])) + ".npy"))
        print(f"second pass ({i0}, {i1}): {len(got)} rows")
        assert len(got) >= 1 and torch.equal(torch.from_numpy(got), want.cpu())
    store = VL.LabelStore.from_dirs({1: [first, second]})
    assert store.pairs(1) == ids and all(len(store.dump(1, p)) > len(np.load(os.path.join(first, str(np.array(p)) + ".npy")))
                                         for p in r["written"])


def test_an_evicted_frame_raises_before_any_launch(monkeypatch, tmp_path):
    from gim_amd import ops
    frames, segs = _frames()
    bank = _bank(frames[:2], segs[:2], capacity=2)
    bank.put(2, frames[2], seg=segs[2])                            # evicts frame 0, the least recently used
    assert 0 not in bank and 1 in bank and 2 in bank

    def no_launch(*a, **k):
        raise AssertionError("ops.frame_prep must not be called")
    monkeypatch.setattr(ops, "frame_prep", no_launch)
    with pytest.raises(GimHipError, match="not resident"):
        VL.prepare_pair(bank, 0, 1, "GIM_LOFTR", EXCLUDE)
    with pytest.raises(GimHipError, match="not resident"):
        VL.label_pair_list(lambda inputs: None, bank, [(0, 2)], "GIM_DKM", str(tmp_path / "out"), vratio=1.0, exclude=EXCLUDE)
