"""The sparse lateral of gim_loftr's fine head (gim_amd/loftr/loftr.py: `lateral_sparse`): the 1/2-level lateral conv + upsample-add runs
behind coarse matching on the 8 x 32 patches within +-4 pixels of 4 x a matched coarse cell, the two 3 x 3 layers behind it on the +-3 list
as before.

  1. both lists of gim_fine_tile_lists against a few lines of numpy on hand-placed matches, the +-3 one also against gim_fine_tile_list;
  2. forward() with the switch on against forward() with it off, same weights, one process: every output bit-identical, also on a graph
     replay over the buffers another pair left behind.

`force_big_tile` sends the lateral launch of the small fixture (96 patches) onto the upsample-carrying 256 x 256 tile in BOTH models: the
dispatch alone takes that tile from 1024 tiles on, and below it the module keeps the dense lateral (`_lateral_sparse_ok`)."""
import numpy as np
import pytest
import torch

from tools import synth_loftr as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ref_tiles(b, i, j, bs, w0c, w1c, H, W, reach, stride=4):
    """ascending indices of the 8 x 32 patches of [2 bs, H, W] that hold a pixel of [s cy - reach, s cy + reach] x [s cx - reach, s cx + reach],
    clipped to the map, for some match (cy, cx) of its image"""
    ty, tx = H // 8, W // 32
    flags = np.zeros((2 * bs, ty, tx), dtype=bool)
    for bb, ii, jj in zip(b, i, j):
        for side, cell, wc in ((0, ii, w0c), (1, jj, w1c)):
            cy, cx = cell // wc, cell % wc
            y0, y1 = max(stride * cy - reach, 0), min(stride * cy + reach, H - 1)
            x0, x1 = max(stride * cx - reach, 0), min(stride * cx + reach, W - 1)
            flags[side * bs + bb, y0 // 8:y1 // 8 + 1, x0 // 32:x1 // 32 + 1] = True
    return np.flatnonzero(flags.ravel()).astype(np.int32)


def _cell(cy, cx, wc=24):
    return cy * wc + cx


# (pair, cell of image 0, cell of image 1) on 16 x 24 coarse maps / 64 x 96 half-resolution maps = 8 x 3 patches per image.
# cx = 7: columns 25..31 within +-3 stay in patch column 0, column 32 (+4) is patch column 1; cy = 1: rows 1..7 stay in patch row 0, row 8 (+4)
# is patch row 1 -- on side 0 and, mirrored, on side 1; cell (0, 0) and the last cell (15, 23) clip to the map
MATCHES = [(0, _cell(5, 7), _cell(10, 20)), (1, _cell(1, 2), _cell(12, 13)), (1, _cell(10, 20), _cell(5, 7)), (0, _cell(12, 13), _cell(1, 2)),
           (0, _cell(0, 0), _cell(15, 23)), (1, _cell(15, 23), _cell(0, 0)), (1, _cell(1, 7), _cell(3, 15))]


@pytest.mark.parametrize("count", [0, 1, 2, len(MATCHES)])
def test_both_lists_match_the_rule(count):
    from gim_amd import ops
    bs, H, W, w0c, w1c, cap = 2, 64, 96, 24, 24, 16
    ids = torch.full((3, cap), 10 ** 12, dtype=torch.int64)   # rows beyond the count are never read
    ids[:, :len(MATCHES)] = torch.tensor(MATCHES, dtype=torch.int64).T
    ids = ids.to(DEV)
    cnt = torch.tensor([count, 0, 0, 0], dtype=torch.int32, device=DEV)
    t3, n3, t4, n4 = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, w0c, w1c, 4, H, W, depth=2)[:4]
    old_t, old_n = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, w0c, w1c, 4, H, W)[:2]
    torch.cuda.synchronize()
    m = [np.array([r[k] for r in MATCHES[:count]], dtype=np.int64) for k in range(3)]
    ref3, ref4 = _ref_tiles(*m, bs, w0c, w1c, H, W, 3), _ref_tiles(*m, bs, w0c, w1c, H, W, 4)
    g3, g4 = t3[:int(n3.item())].cpu().numpy(), t4[:int(n4.item())].cpu().numpy()
    print(f"count {count}: +-3 {len(g3)} patches (rule {len(ref3)}), +-4 {len(g4)} patches (rule {len(ref4)})")
    assert np.array_equal(g3, ref3) and np.array_equal(g4, ref4)
    assert np.array_equal(old_t[:int(old_n.item())].cpu().numpy(), ref3)      # the existing entry: unchanged
    for g in (g3, g4):
        assert np.all(np.diff(g) > 0)                                        # ascending, no duplicates
    assert set(g3) <= set(g4)
    if count >= 1:   # match 0 (image 0, rows 16..24, columns 24..32): +-4 crosses into patch column 1 of patch row 2, +-3 does not
        assert (0 * 8 + 2) * 3 + 1 in g4 and (0 * 8 + 2) * 3 + 1 not in g3
    if count >= 2:   # match 1 (pair 1, side 0 = image 1): +-4 crosses into patch row 1
        assert (1 * 8 + 1) * 3 + 0 in g4 and (1 * 8 + 1) * 3 + 0 not in g3
    if count == 0:
        assert len(g3) == 0 and len(g4) == 0


OUT = ("b_ids", "i_ids", "j_ids", "m_bids", "gt_mask", "mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f", "expec_f")
HW = (128, 192)


def _forward(model, c0, c1):
    d = {"image0": c0[:, :1], "image1": c1[:, :1], "color0": c0, "color1": c1}
    model(d)
    torch.cuda.synchronize()
    return {k: d[k].clone() for k in OUT}


def _same(got, ref, what):
    for k in OUT:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), (what, k)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_forward_is_bit_identical_with_the_sparse_lateral(precision, monkeypatch):
    from gim_amd import ops
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)
    on, sd = S.synthetic_model(precision)
    off, _ = S.synthetic_model(precision, lateral_sparse=False)
    off.load_state_dict({k: v.clone() for k, v in sd.items()})
    on, off = on.to(DEV), off.to(DEV)
    assert on.lateral_sparse and not off.lateral_sparse and on.fine_sparse and off.fine_sparse
    bs = 2
    took = []   # launches of the C entry itself: the wrapper's dense path (a refused launch) would be bit-identical too and must not pass for it
    real = ops.lib.gim_conv2d_ups_tiles
    monkeypatch.setattr(ops.lib, "gim_conv2d_ups_tiles", lambda *a: (took.append(1), real(*a))[1])
    c0, c1 = (t.to(DEV) for t in S.textured_pairs(bs, *HW, seed=3, frac=0.5))   # the match-rich pair of tests/test_gpu_fine_sparse.py
    ref = _forward(off, c0, c1)
    assert not took, "the model with the switch off took the patch-list lateral"
    M = int(ref["b_ids"].numel())
    print(f"{precision}: {M} matches")
    assert M > 50
    for rep in range(3):   # eager, graph capture, replay
        _same(_forward(on, c0, c1), ref, f"forward {rep}")
    assert len(took) >= 2, "forward() did not launch gim_conv2d_ups_tiles (eager run and graph capture)"
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
    # extract() + match_features() take the dense lateral and stay the same forward
    feats = on.extract(torch.cat([c0, c1]))
    r = on.match_features(feats, feats, list(range(bs)), list(range(bs, 2 * bs)))
    torch.cuda.synchronize()
    _same({k: r[k] for k in OUT}, ref, "extract + match_features")


def test_dense_lateral_is_kept_where_the_list_launch_does_not_apply():
    """without force_big_tile the 96-patch lateral of this size is a two-pass launch in extract(): forward() keeps it dense too"""
    model, _ = S.synthetic_model("fp16")
    model = model.to(DEV)
    P = model._prepack(torch.device(DEV))
    x = model._to_nhwc([t.to(DEV) for t in S.textured_pairs(1, *HW, seed=3, frac=0.5)], model._img_dt())
    assert model._fine_sparse_ok(P, [x]) and not model._lateral_sparse_ok(P, [x])
