"""The quarter-level patch lists of gim_loftr's sparse fine head (gim_fine_tile_lists4, ops.fine_tile_lists(depth=3)) and the chain they feed.

The 1/2-level lateral that walks the +-4 list reads its upsample operand x2_out where Epilogue::ups_accumulate (conv_igemm.hip, lambda
`issue`) stages it: per 32-pixel pass (row Y, first column X0) of a listed patch, source rows y0 = (int)(sy Y), y0 + (y0 < h - 1) and
columns xa .. min(xa + 23, w - 1), xa = (int)(sx X0), fp32.  All of them enter the MFMA, weight 0 or not.  S = their union; list C = the
8 x 32 patches of the 1/4-level map holding a pixel of S, B = of S dilated by 1, A = of S dilated by 2.

  1. A, B, C against a numpy model that stages sources with np.float32 arithmetic as `issue` does; the two half-level lists against the
     rule of tests/test_gpu_lateral_sparse.py (the existing entries' results are unchanged);
  2. the poison chain: every buffer between the trunk and the fine tail pre-filled with NaN, the 1/4-level lateral, the two 3 x 3 layers
     and the 1/2-level lateral on their lists -- every x1_out pixel of a +-4-listed patch finite and bit-identical to the dense chain.  A
     reach that forgot the zero-weight sources (0 x NaN = NaN) fails here."""
import numpy as np
import pytest
import torch

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


def _dilate(m):
    """one pixel in every direction, clipped to the map"""
    p = np.pad(m, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[:, dy:dy + m.shape[1], dx:dx + m.shape[2]]
    return out


def _ref_quarter(t4, bs, H, W):
    """(A, B, C, S) from the +-4 list of half-level patches: the sources `issue` stages, in np.float32 as the kernel has them"""
    h, w = H // 2, W // 2
    sy = np.float32(h - 1) / np.float32(H - 1)
    sx = np.float32(w - 1) / np.float32(W - 1)
    assert sy.dtype == np.float32 and sx.dtype == np.float32
    ty_n, tx_n = H // 8, W // 32
    S = np.zeros((2 * bs, h, w), dtype=bool)
    for p in t4:
        img, r = divmod(int(p), ty_n * tx_n)
        ty, tx = divmod(r, tx_n)
        xa = int(np.float32(sx * np.float32(32 * tx)))
        xe = min(xa + 23, w - 1)
        for Y in range(8 * ty, 8 * ty + 8):
            y0 = int(np.float32(sy * np.float32(Y)))
            y1 = y0 + (1 if y0 < h - 1 else 0)
            S[img, y0, xa:xe + 1] = True
            S[img, y1, xa:xe + 1] = True
    S1 = _dilate(S)
    S2 = _dilate(S1)
    lists = []
    for m in (S2, S1, S):
        pf = m.reshape(2 * bs, h // 8, 8, w // 32, 32).any(axis=(2, 4))
        lists.append(np.flatnonzero(pf.ravel()).astype(np.int32))
    return lists[0], lists[1], lists[2], S


def _match_sets(hc, wc):
    """name -> list of (pair, cell of image 0, cell of image 1) on hc x wc coarse maps, two pairs"""
    cell = lambda cy, cx: cy * wc + cx
    corners = [cell(0, 0), cell(0, wc - 1), cell(hc - 1, 0), cell(hc - 1, wc - 1)]
    # 4 cy + 4 = 8 k for odd cy (the +-4 reach touches the next patch row), 4 cx + 4 = 32 at cx = 7, 4 cx - 4 = 28 at cx = 8 (previous patch
    # column only through -4), cx = 9: 32 .. 40 stays; the mirrored cells on the other side
    straddle = [cell(1, 7), cell(3, 8), cell(5, 9), cell(2, 15), cell(hc - 2, wc - 8), cell(hc - 3, wc - 9), cell(7, 23), cell(9, 24)]
    return {
        "none": [],
        "corners": [(k % 2, c, corners[(k + 1) % 4]) for k, c in enumerate(corners)],
        "straddles": [(k % 2, c, straddle[(k + 3) % len(straddle)]) for k, c in enumerate(straddle)],
        "every cell": [(p, c, c) for p in range(2) for c in range(hc * wc)],
    }


@pytest.mark.parametrize("size", [(64, 128), (240, 320)], ids=["64x128", "240x320"])
@pytest.mark.parametrize("which", ["none", "corners", "straddles", "every cell"])
def test_quarter_lists_match_the_staging_model(size, which):
    from gim_amd import ops
    H, W = size
    bs, hc, wc = 2, H // 4, W // 4
    matches = _match_sets(hc, wc)[which]
    cap = max(len(matches), 1) + 3
    ids = torch.full((3, cap), 10 ** 12, dtype=torch.int64)   # rows beyond the count are never read
    if matches:
        ids[:, :len(matches)] = torch.tensor(matches, dtype=torch.int64).T
    ids = ids.to(DEV)
    cnt = torch.tensor([len(matches), 0, 0, 0], dtype=torch.int32, device=DEV)
    assert ops.fine_tile_lists4_fits(bs, H, W)
    t3, n3, t4, n4, tq, nq = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, wc, wc, 4, H, W, depth=3)
    o3, on3, o4, on4 = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, wc, wc, 4, H, W, depth=2)[:4]
    torch.cuda.synchronize()
    m = [np.array([r[k] for r in matches], dtype=np.int64) for k in range(3)]
    ref3, ref4 = _ref_tiles(*m, bs, wc, wc, H, W, 3), _ref_tiles(*m, bs, wc, wc, H, W, 4)
    g3, g4 = t3[:int(n3.item())].cpu().numpy(), t4[:int(n4.item())].cpu().numpy()
    assert np.array_equal(g3, ref3) and np.array_equal(g4, ref4)
    assert np.array_equal(o3[:int(on3.item())].cpu().numpy(), ref3) and np.array_equal(o4[:int(on4.item())].cpu().numpy(), ref4)   # the existing entry: unchanged
    rA, rB, rC, S = _ref_quarter(ref4, bs, H, W)
    nqh = nq.cpu().numpy()
    gA, gB, gC = (tq[k, :int(nqh[k])].cpu().numpy() for k in range(3))
    total_q = 2 * bs * (H // 16) * (W // 64)
    print(f"{H}x{W} {which}: +-4 {len(g4)} half patches -> A {len(gA)} B {len(gB)} C {len(gC)} of {total_q} quarter patches (model {len(rA)} {len(rB)} {len(rC)})")
    assert np.array_equal(gA, rA) and np.array_equal(gB, rB) and np.array_equal(gC, rC)
    for g in (gA, gB, gC):
        assert np.all(np.diff(g) > 0)                # ascending, no duplicates
    assert set(gC) <= set(gB) <= set(gA)
    if which == "none":
        assert len(gA) == 0
    if which == "every cell":
        assert len(gC) == total_q


def _pk(cout, cin, k, tdt, seed):
    from gim_amd import ops
    from gim_amd.packing import pack_conv
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5
    return pack_conv(w, None, ops.gim_dtype(torch.empty(0, dtype=tdt)), DEV, stride=1, pad=k // 2, bias=torch.randn(cout, generator=g) * 0.1)


def _patches(t):
    B, H, W, C = t.shape
    return t.view(B, H // 8, 8, W // 32, 32, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 8, 32, C)


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_poison_chain(tdt, monkeypatch):
    from gim_amd import ops
    from gim_amd._lib import ACT_LEAKY
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)
    bs, H, W = 1, 64, 128
    h, w, hc, wc = H // 2, W // 2, H // 4, W // 4
    P = {"l2o": _pk(256, 512, 1, tdt, 1), "l2o2a": _pk(256, 256, 3, tdt, 2), "l2o2b": _pk(196, 256, 3, tdt, 3), "l1o": _pk(196, 256, 1, tdt, 4)}
    g = torch.Generator().manual_seed(9)
    x1 = torch.randn(2 * bs, H, W, P["l1o"].cin_pad, generator=g).to(DEV, tdt)
    x2 = torch.randn(2 * bs, h, w, P["l2o"].cin_pad, generator=g).to(DEV, tdt)
    x3_out = torch.randn(2 * bs, h // 2, w // 2, P["l2o"].n_store, generator=g).to(DEV, tdt)
    assert ops.conv_ups_tiles_supported(x2, P["l2o"], x3_out, dense_too=True)
    assert ops.conv_tiles_supported((2 * bs, h, w, 256), P["l2o2a"], dense_too=True) and ops.conv_tiles_supported((2 * bs, h, w, 256), P["l2o2b"], dense_too=True)
    # dense chain (resnet.py:321-327)
    d = ops.conv2d(x2, P["l2o"], ups=x3_out)
    d = ops.conv2d(ops.conv2d(d, P["l2o2a"], ACT_LEAKY), P["l2o2b"])
    dense = ops.conv2d(x1, P["l1o"], ups=d)
    # matches: a corner, a straddling cell, one in the middle; the other side mirrored
    cell = lambda cy, cx: cy * wc + cx
    matches = [(0, cell(0, 0), cell(hc - 1, wc - 1)), (0, cell(1, 7), cell(9, 24)), (0, cell(8, 17), cell(5, 9))]
    ids = torch.tensor(matches, dtype=torch.int64).T.contiguous().to(DEV)
    cnt = torch.tensor([len(matches), 0, 0], dtype=torch.int32, device=DEV)
    t3, n3, t4, n4, tq, nq = ops.fine_tile_lists(ids[0], ids[1], ids[2], cnt, bs, wc, wc, 4, H, W, depth=3)
    nan = lambda *s: torch.full(s, float("nan"), dtype=tdt, device=DEV)
    a_out, b_out, c_out, x1_out = nan(2 * bs, h, w, 256), nan(2 * bs, h, w, 256), nan(2 * bs, h, w, P["l2o2b"].n_store), nan(2 * bs, H, W, P["l1o"].n_store)
    ops.conv2d_ups_tiles(x2, P["l2o"], x3_out, tq[0], nq[0:1], y=a_out)
    ops.conv2d_tiles(a_out, P["l2o2a"], tq[1], nq[1:2], ACT_LEAKY, out=b_out)
    ops.conv2d_tiles(b_out, P["l2o2b"], tq[2], nq[2:3], out=c_out)
    ops.conv2d_ups_tiles(x1, P["l1o"], c_out, t4, n4, y=x1_out)
    torch.cuda.synchronize()
    listed = t4[:int(n4.item())].long()
    total, total_q = 2 * bs * (H // 8) * (W // 32), 2 * bs * (h // 8) * (w // 32)
    nqh = nq.cpu().numpy()
    print(f"{tdt}: +-4 list {listed.numel()} of {total} half patches; A {nqh[0]} B {nqh[1]} C {nqh[2]} of {total_q} quarter patches")
    assert 0 < listed.numel() < total and 0 < nqh[2] <= nqh[1] <= nqh[0] < total_q   # a sparse case: something stays poisoned
    got, ref = _patches(x1_out)[listed], _patches(dense)[listed]
    assert bool(torch.isfinite(got.float()).all()), "a consumed x1_out pixel is not finite: a staged upsample source was never computed"
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), "a consumed x1_out pixel differs from the dense chain"
    assert bool(torch.isnan(_patches(c_out).float()).flatten(1).all(1).any()), "no x2_out patch kept its poison: the case is not sparse"
