"""The sparse 1/4-level part of gim_loftr's fine head (gim_amd/loftr/loftr.py: `quarter_sparse`): layer2_outconv + upsample-add and the two
3 x 3 layers of layer2_outconv2 run behind coarse matching on the patch lists A, B, C of gim_fine_tile_lists4, in front of the list-walking
1/2-level lateral that is their only consumer.

forward() with the switch on against forward() with it off, same weights, one process: every output bit-identical -- eager, graph capture,
replay, and a replay over the buffers another pair left behind (the unlisted pixels then hold that pair's values, not zeros).

The textured pair of tests/test_gpu_lateral_sparse.py at 128 x 256 instead of 128 x 192: the 1/4-level map must be whole 8 x 32 patches
(32 x 64 here; 32 x 48 there is not, and the module keeps that size dense -- checked below).  `force_big_tile` sends the small fixture's
launches onto the 256 x 256 tile in BOTH models, as there."""
import pytest
import torch

from tools import synth_loftr as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT = ("b_ids", "i_ids", "j_ids", "m_bids", "gt_mask", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f")
HW = (128, 256)


def _forward(model, c0, c1):
    d = {"image0": c0[:, :1], "image1": c1[:, :1], "color0": c0, "color1": c1}
    model(d)
    torch.cuda.synchronize()
    return {k: d[k].clone() for k in OUT}


def _same(got, ref, what):
    for k in OUT:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (what, k)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_forward_is_bit_identical_with_the_sparse_quarter_level(precision, monkeypatch):
    from gim_amd import ops
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)
    on, sd = S.synthetic_model(precision)
    off, _ = S.synthetic_model(precision, quarter_sparse=False)
    off.load_state_dict({k: v.clone() for k, v in sd.items()})
    on, off = on.to(DEV), off.to(DEV)
    assert on.quarter_sparse and not off.quarter_sparse and on.lateral_sparse and off.lateral_sparse
    bs = 2
    took = []   # launches of the C entry itself: the wrapper's dense path (a refused launch) would be bit-identical too and must not pass for it
    real = ops.lib.gim_conv2d_tiles
    monkeypatch.setattr(ops.lib, "gim_conv2d_tiles", lambda *a: (took.append(1), real(*a))[1])
    c0, c1 = (t.to(DEV) for t in S.textured_pairs(bs, *HW, seed=3, frac=0.5))
    P = on._prepack(torch.device(DEV))
    x = on._to_nhwc([c0, c1], on._img_dt())
    assert on._quarter_sparse_ok(P, [x]) and not off._quarter_sparse_ok(P, [x])
    ref = _forward(off, c0, c1)
    assert not took, "the model with the switch off took the patch-list 3 x 3 launch"
    M = int(ref["b_ids"].numel())
    print(f"{precision}: {M} matches")
    assert M > 50
    for rep in range(3):   # eager, graph capture, replay
        _same(_forward(on, c0, c1), ref, f"forward {rep}")
    assert len(took) >= 4, "forward() did not launch gim_conv2d_tiles (two layers, eager run and graph capture)"
    # a second, different pair replayed over the buffers of the first (mirrored: the matches move to the other side of both frames), a
    # match-poor one, and the first again
    m0, m1 = c0.flip(-1).contiguous(), c1.flip(-1).contiguous()
    ref_m = _forward(off, m0, m1)
    assert ref_m["b_ids"].numel() > 50
    _same(_forward(on, m0, m1), ref_m, "mirrored pair, replay")
    g = torch.Generator().manual_seed(4)
    z0, z1 = torch.rand(bs, 3, *HW, generator=g).to(DEV), torch.rand(bs, 3, *HW, generator=g).to(DEV)
    _same(_forward(on, z0, z1), _forward(off, z0, z1), "noise")
    _same(_forward(on, c0, c1), ref, "first pair again")
    assert len(on._graphs) == 1
    # extract() + match_features() take the dense head and stay the same forward
    feats = on.extract(torch.cat([c0, c1]))
    r = on.match_features(feats, feats, list(range(bs)), list(range(bs, 2 * bs)))
    torch.cuda.synchronize()
    _same({k: r[k] for k in OUT}, ref, "extract + match_features")


def test_dense_quarter_level_is_kept_where_the_list_launches_do_not_apply(monkeypatch):
    """a 1/4-level map that is not whole patches (32 x 48), and any size whose dense launches are not on the 256 x 256 tile (no
    force_big_tile: 16 tiles): forward() keeps the dense launches"""
    from gim_amd import ops
    model, _ = S.synthetic_model("fp16")
    model = model.to(DEV)
    P = model._prepack(torch.device(DEV))
    x = model._to_nhwc([t.to(DEV) for t in S.textured_pairs(1, *HW, seed=3, frac=0.5)], model._img_dt())
    assert model._fine_sparse_ok(P, [x]) and not model._quarter_sparse_ok(P, [x])
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)
    assert model._quarter_sparse_ok(P, [x])
    x192 = model._to_nhwc([t.to(DEV) for t in S.textured_pairs(1, 128, 192, seed=3, frac=0.5)], model._img_dt())
    assert model._lateral_sparse_ok(P, [x192]) and not model._quarter_sparse_ok(P, [x192])
