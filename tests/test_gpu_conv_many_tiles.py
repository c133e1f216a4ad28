"""The persistent conv kernels where a workgroup walks SEVERAL tiles (conv_igemm.hip, igemm_persistent_body.h: the cross-tile hand-over --
the next tile's first K slab issued in the current tile's last K iteration, the residual prefetch beside it, the epilogue's transposition
through the stage just consumed, `init_acc` of the next column block, `g = gn`; the halo kernel's prefetch of the next patch's halo; the
list kernels with more listed patches than workgroups).  A launch has min(T, RESIDENT) workgroups, RESIDENT = 512 for the 4-wave kernels and
256 for the 8-wave tile, the halo kernel and the list kernels: every shape here has T > RESIDENT, the smallest that put a second and a third
tile on a workgroup.  test_gpu_kernels.py, test_gpu_conv_halo.py, test_gpu_conv3x3_tiles.py and test_gpu_ups_tiles.py stay at one tile per
workgroup.

Per case:
  reference     fp32 F.conv2d on the CPU, operands rounded to the kernel's operand type, BN folded by packing.fold_bn (test_conv2d_bn_act),
                at that test's tolerances `_tol` (an fp32 output of 16-bit operands: fp32's -- exact products, fp32 sums); padded output
                channels are exact zeros
  prefix        the same layer on a prefix of the rows (1024 rows of a flat 1x1 launch, the first image rows of a 3x3 one: one tile per
                workgroup, the regime the other files pin) equals those rows of the many-tile launch bit for bit -- an accumulator does not
                depend on which tile or tile row its pixel sits in as long as both launches run the same tile template, which is asserted
                through gim_conv2d_big_tile for both launches
  repeat        a second launch gives identical bits
  beyond M      the output is a view of a buffer with PAD more rows holding a sentinel (fp32: NaN; 16-bit: 0x7B7B): they stay untouched
  bias          BN shift / bias with a standard deviation of 1, different per channel: a bias of another column block cannot pass

The measured error of every comparison is printed (pytest -s) in front of its assertion."""
import ctypes
import time

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import _gim, _rnd, _tdt, _tol

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7B7B   # a finite 16-bit pattern in both kinds that no computed value of these layers takes (fp16 61 280, bf16 3.3e36)
PAD = 7             # rows behind M that must keep the sentinel


def _close(got, ref, tol, what=""):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    scale = max(1e-6, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    print(f"[close] {what}: {err / scale:.3e} of scale (tol {tol:g})")
    assert err <= tol * scale, f"{what}: max|err|={err:.3e} scale={scale:.3e} rel={err / scale:.3e} tol={tol}"


def _bits(t):
    """integer view: NaN sentinels compare equal to themselves"""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _sentinel_rows(rows, ns, odt):
    if odt == "fp32":
        return torch.full((rows, ns), float("nan"), device=DEV)
    return torch.full((rows, ns), SENTINEL, dtype=torch.int16, device=DEV).view(_tdt(odt))


def _untouched(t):
    return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((_bits(t) == SENTINEL).all())


def _act(name):
    from gim_amd import ops
    return {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}[name]


def _act_ref(name, v):
    return {"none": lambda t: t, "relu": F.relu, "leaky": lambda t: F.leaky_relu(t, 0.01)}[name](v)


def _layer(g, cin, cout, k, norm):
    """(w, bn, bias) of a layer whose folded bias has a standard deviation of about 1, different per channel"""
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    if norm == "bn":
        bn = (0.75 + 0.5 * torch.rand(cout, generator=g), torch.randn(cout, generator=g),
              0.1 * torch.randn(cout, generator=g), 0.5 + torch.rand(cout, generator=g), 1e-5)
        return w, bn, None
    return w, None, torch.randn(cout, generator=g)


def _folded(w, bn, bias):
    from gim_amd.packing import fold_bn
    wf, bf = fold_bn(w, bn)
    return wf, (bf if bias is None else bias)


def _big_tile(pk, geom, x, y, act, res, split16):
    """does the dispatch send this dense launch to the 256 x 256 tile?  (gim_conv2d_big_tile of the launch's own struct, as
    ops.conv_tiles_supported(..., dense_too=True) asks it; 0 for fp32 operands, which reach that tile only as split launches with
    npad % 256 == 0 -- no case here)"""
    from gim_amd import ops
    a = ops._conv_args(pk, geom, x.stride(0), y.stride(0), x=x, y=y, act=act, res=res, split16=split16)
    return bool(ops.lib.gim_conv2d_big_tile(ctypes.byref(a)))


def _launch(pk, x2, geom, odt, act, res2, split16):
    """conv_rows into the first M rows of a sentinel-filled buffer of M + PAD rows -> (buffer, M, on the 256 x 256 tile?)"""
    from gim_amd import ops
    B, _, _, Ho, Wo = geom
    M = B * Ho * Wo
    buf = _sentinel_rows(M + PAD, pk.n_store, odt)
    big = _big_tile(pk, geom, x2, buf[:M], act, res2, split16)
    ops.conv_rows(x2, pk, geom, buf[:M], act, res=res2, split16=split16)
    torch.cuda.synchronize()
    return buf, M, big


# ---- cases 1 - 9: the generic persistent kernels through ops.conv_rows ------------------------------------------------------------------------
# name: (cin, cout, k, norm, act, residual, (B, H, W) -- B = H = 1: a flat launch of W rows, [(operand dtype, output dtype)], force_big_tile,
#        split16, on the 256 x 256 tile?)
H16 = [("bf16", "bf16"), ("fp16", "fp16")]
ALL = [("fp32", "fp32")] + H16
F32OUT = [("bf16", "fp32"), ("fp16", "fp32")]
CASES = {
    # 256 x 64 tile, RESIDENT 512, nkt = 1: the next tile's slab is issued in the only K iteration.  514 tiles: a few workgroups walk two
    "1 256x64 514 tiles": (64, 64, 1, "bn", "relu", False, (1, 1, 362 * 363), ALL + F32OUT, False, False, False),
    # 1029 tiles: up to three per workgroup, the last one has ONE valid row and is some workgroup's third
    "2 256x64 1029 tiles": (64, 64, 1, "bn", "relu", False, (1, 1, 513 * 513), H16, False, False, False),
    # 3x3, nkt = 9 (odd: the LDS stage parity flips from tile to tile): spatial decode of the next tile, image-border taps in a non-first tile
    "3 256x64 3x3": (64, 64, 3, "bn", "relu", False, (1, 362, 363), H16, False, False, False),
    # 128 x 128 tile, npad 384 = 3 N tiles, step 64 is no multiple of 3: consecutive tiles of a workgroup change n0 (init_acc(n0n), column base)
    "4 128x128 n384 528 tiles": (128, 384, 1, "bias", "relu", False, (1, 1, 149 * 151), ALL, False, False, False),
    "4 128x128 n384 1056 tiles": (128, 384, 1, "bias", "relu", False, (1, 1, 45000), ALL, False, False, False),
    # residual: prefetch_res of the current tile beside the next tile's slab; the ragged last tile's residual rows
    "5 128x128 residual": (64, 256, 1, "bn", "relu", True, (1, 1, 33000), H16 + F32OUT, False, False, False),
    # fp32 operands: both copies of the fp32 K loop across tiles
    "6 128x128 fp32 exact": (64, 128, 1, "bn", "none", False, (1, 1, 66049), [("fp32", "fp32")], False, False, False),
    "6 128x128 fp32 split16": (64, 128, 1, "bn", "none", False, (1, 1, 66049), [("fp32", "fp32")], False, True, False),
    # 256 x 256 tile, 8 waves, RESIDENT 256, forced: 259 tiles, the last one row; 196 outputs: the fragment-skipping copy, chosen per tile
    "7 256x256 forced leaky": (256, 256, 1, "bias", "leaky", False, (1, 1, 257 * 257), H16, True, False, True),
    "7 256x256 forced skip": (256, 196, 1, "bias", "none", False, (1, 1, 257 * 257), H16, True, False, True),
    # 256 x 192 tile, 8 waves: the one-N-tile instantiation
    "9 256x192": (144, 144, 1, "bias", "relu", False, (1, 1, 66049), H16, False, False, False),
}
PARAMS = [(name, dts) for name, c in CASES.items() for dts in c[7]]


@pytest.mark.parametrize("name,dts", PARAMS, ids=[f"{n.replace(' ', '_')}-{d[0]}_to_{d[1]}" for n, d in PARAMS])
def test_many_tiles_dense(name, dts, monkeypatch):
    from gim_amd import ops
    from gim_amd.packing import pack_conv
    t0 = time.time()
    cin, cout, k, norm, actname, has_res, (B, H, W), _, force, split16, want_big = CASES[name]
    dt, odt = dts
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", force)
    g = torch.Generator().manual_seed(2000 + list(CASES).index(name))
    w, bn, bias = _layer(g, cin, cout, k, norm)
    pk = pack_conv(w, bn, _gim(dt), DEV, stride=1, pad=k // 2, bias=bias)
    assert pk.cin_pad == cin
    M = B * H * W
    x = torch.randn(M, cin, generator=g)
    res = torch.randn(M, pk.n_store, generator=g) if has_res else None
    xd = x.to(_tdt(dt)).to(DEV)
    resd = res.to(_tdt(odt)).to(DEV) if has_res else None
    act = _act(actname)
    geom = (1, 1, M, 1, M) if k == 1 else (B, H, W, H, W)   # pixel index == row index: the kernel skips the coordinate decode (ops.conv2d)

    buf, _, big = _launch(pk, xd, geom, odt, act, resd, split16)
    y = buf[:M]
    assert big == want_big, "the launch did not run on the tile this case is about"
    assert _untouched(buf[M:]), "rows beyond M were written"

    # ---- reference ----------------------------------------------------------------------------------------------------------------------------
    wf, bf = _folded(w, bn, bias)
    xi = _rnd(x, dt).view(B, H, W, cin).permute(0, 3, 1, 2)
    if split16:   # test_gpu_split16.py: a float64 convolution of the same fp32 values, max 4e-6 and mean 4e-7 of the output scale
        ref = F.conv2d(xi.double(), wf.double(), bf.double(), padding=k // 2)
    else:
        ref = F.conv2d(xi, _rnd(wf, dt), bf, padding=k // 2)
    ref = ref.permute(0, 2, 3, 1).reshape(M, cout)
    if has_res:
        ref = ref + _rnd(res, odt)[:, :cout]
    ref = _act_ref(actname, ref)
    got = y.cpu()
    if split16:
        d = (got[:, :cout].double() - ref).abs()
        scale = ref.abs().max().item()
        print(f"[close] {name} split16: max {d.max().item() / scale:.3e} (tol 4e-06) mean {d.mean().item() / scale:.3e} (tol 4e-07) of scale")
        assert torch.isfinite(got).all()
        assert d.max().item() <= 4e-6 * scale and d.mean().item() <= 4e-7 * scale
    else:
        _close(got[:, :cout], ref, _tol("fp32" if odt == "fp32" else dt), f"{name} {dt}->{odt}")
    if pk.n_store > cout:
        assert (got[:, cout:] == 0).all(), "padded output channels are not exact zeros"

    # ---- a second launch: identical bits ------------------------------------------------------------------------------------------------------
    buf2, _, _ = _launch(pk, xd, geom, odt, act, resd, split16)
    assert torch.equal(_bits(buf2), _bits(buf)), "two launches differ"

    # ---- a prefix of the rows, one tile per workgroup: the same bits --------------------------------------------------------------------------
    if k == 1:
        n = keep = 1024
        pgeom = (1, 1, n, 1, n)
    else:
        n, keep = 9 * W, 8 * W        # the first 9 image rows; the 9th has another bottom neighbour (the padding) than in the full map
        pgeom = (1, 9, W, 9, W)
    pbuf, _, pbig = _launch(pk, xd[:n], pgeom, odt, act, resd[:n] if has_res else None, split16)
    assert pbig == big, "the prefix launch runs another tile template"
    assert _untouched(pbuf[n:])
    same = (_bits(pbuf[:keep]) == _bits(y[:keep])).all(1)
    print(f"[bits] {name} {dt}->{odt}: {int((~same).sum())} of {keep} prefix rows differ from the many-tile launch")
    assert bool(same.all()), "rows depend on how many tiles the launch has"
    print(f"[time] {name} {dt}->{odt}: {time.time() - t0:.2f} s")


def test_big_tile_on_its_own_route():
    """Case 8.  The dispatch takes the 256 x 256 tile on its own from 1024 tiles on: 256 -> 256 1x1, bf16, 512 x 513 = 262 656 rows = 1026 tiles
    on 256 workgroups, four and five tiles each.  Reference, repeat and beyond-M only: a prefix launch would run on another tile.  The
    predicate must say yes here and at 1024 tiles (511 x 513 = 262 143 rows: 1023 full tiles and one of 255 rows), no at 1023 tiles."""
    from gim_amd import ops
    from gim_amd.packing import pack_conv
    t0 = time.time()
    assert not ops.FORCE_BIG_TILE
    g = torch.Generator().manual_seed(2100)
    w, bn, bias = _layer(g, 256, 256, 1, "bias")
    pk = pack_conv(w, bn, _gim("bf16"), DEV, bias=bias)
    M = 512 * 513
    x = torch.randn(M, 256, generator=g)
    xd = x.to(torch.bfloat16).to(DEV)
    act = _act("relu")
    buf, _, big = _launch(pk, xd, (1, 1, M, 1, M), "bf16", act, None, False)
    assert big, "1026 tiles did not go to the 256 x 256 tile"
    for rows, want in ((511 * 513, True), (1023 * 256 + 1, True), (1023 * 256, False), (510 * 513, False)):
        assert _big_tile(pk, (1, 1, rows, 1, rows), xd[:rows], buf[:rows], act, None, False) == want, (rows, want)
    assert _untouched(buf[M:]), "rows beyond M were written"
    ref = F.relu(F.conv2d(_rnd(x, "bf16").view(1, 1, M, 256).permute(0, 3, 1, 2), _rnd(w, "bf16"), bias)).permute(0, 2, 3, 1).reshape(M, 256)
    _close(buf[:M], ref, _tol("bf16"), "8 256x256 own route bf16")
    buf2, _, _ = _launch(pk, xd, (1, 1, M, 1, M), "bf16", act, None, False)
    assert torch.equal(_bits(buf2), _bits(buf)), "two launches differ"
    print(f"[time] 8 256x256 own route: {time.time() - t0:.2f} s")


# ---- case 10: the halo kernel ---------------------------------------------------------------------------------------------------------------
HALO_LAYERS = {"64to128": (64, 128), "128to128": (128, 128), "64to256": (64, 256)}   # one chunk, TN = 2 / two chunks / TN = 4
HALO_TOL = {"bf16": 1e-2, "fp16": 1.5e-3}   # halo against the generic path: test_conv3x3_halo_vs_reference's


def _halo_launch(pk, xd, act):
    from gim_amd import ops
    B, H, W, _ = xd.shape
    M = B * H * W
    buf = _sentinel_rows(M + PAD, pk.n_store, "bf16" if xd.dtype == torch.bfloat16 else "fp16")
    ops.conv3x3_halo(xd, pk, buf[:M].view(B, H, W, pk.n_store), act)
    torch.cuda.synchronize()
    return buf, M


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("layer", list(HALO_LAYERS))
def test_many_tiles_halo(layer, dt):
    """1 x 262 x 250: 33 x 8 = 264 patches on 256 workgroups, ragged in H and W -- the next patch's halo is prefetched during the current
    patch, ragged patches are non-last tiles of their workgroups"""
    from gim_amd import ops
    from gim_amd.packing import pack_conv
    t0 = time.time()
    cin, cout = HALO_LAYERS[layer]
    H, W = 262, 250
    g = torch.Generator().manual_seed(2200 + list(HALO_LAYERS).index(layer))
    w, bn, bias = _layer(g, cin, cout, 3, "bias")
    pk = pack_conv(w, bn, _gim(dt), DEV, stride=1, pad=1, bias=bias)
    assert pk.halo is not None and pk.cin_pad == cin and pk.n_store == cout
    x = torch.randn(1, H, W, cin, generator=g)
    xd = x.to(_tdt(dt)).to(DEV)
    act = _act("relu")
    buf, M = _halo_launch(pk, xd, act)
    assert _untouched(buf[M:]), "rows beyond M were written"
    ref = F.relu(F.conv2d(_rnd(x, dt).permute(0, 3, 1, 2), _rnd(w, dt), bias, padding=1)).permute(0, 2, 3, 1).reshape(M, cout)
    _close(buf[:M], ref, _tol(dt), f"10 halo {layer} {dt}")
    y2 = torch.empty(M, pk.n_store, dtype=_tdt(dt), device=DEV)
    ops.conv_rows(xd.view(-1, cin), pk, (1, H, W, H, W), y2, act)   # the generic path: same products, other K order
    torch.cuda.synchronize()
    _close(buf[:M], y2, HALO_TOL[dt], f"10 halo {layer} {dt} against the generic path")
    buf2, _ = _halo_launch(pk, xd, act)
    assert torch.equal(_bits(buf2), _bits(buf)), "two launches differ"
    # the first 24 image rows (3 x 8 patches, one per workgroup): rows 0 .. 22 see the same taps as in the full map
    pbuf, n = _halo_launch(pk, xd[:, :24].contiguous(), act)
    assert _untouched(pbuf[n:])
    keep = 23 * W
    same = (_bits(pbuf[:keep]) == _bits(buf[:keep])).all(1)
    print(f"[bits] 10 halo {layer} {dt}: {int((~same).sum())} of {keep} prefix rows differ from the many-tile launch")
    assert bool(same.all()), "rows depend on how many patches the launch has"
    print(f"[time] 10 halo {layer} {dt}: {time.time() - t0:.2f} s")


# ---- case 11: the list kernels with more listed patches than workgroups --------------------------------------------------------------------
def _patches(t):
    """[B,H,W,C] -> [B * H/8 * W/32, 8, 32, C] in patch-index order"""
    B, H, W, C = t.shape
    return t.view(B, H // 8, 8, W // 32, 32, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 8, 32, C)


def _check_list(y, dense, listed, what):
    """the assertions of test_gpu_conv3x3_tiles.py::_run: listed patches as the dense launch writes them, every other one keeps the sentinel"""
    yp, dp = _bits(_patches(y)), _bits(_patches(dense))
    on = torch.zeros(yp.shape[0], dtype=torch.bool, device=DEV)
    on[listed] = True
    bad = (yp[on] != dp[on]).flatten(1).any(1)
    print(f"[bits] {what}: {int(on.sum())} of {yp.shape[0]} patches listed, {int(bad.sum())} differ from the dense launch")
    assert not bool(bad.any()), "a listed patch differs from the dense launch"
    assert bool((yp[~on] == SENTINEL).all()), "a patch outside the list was written"
    assert not bool((dp == SENTINEL).all(-1).any()), "the sentinel is a value of the layer"


def _list_args(listed):
    tiles = torch.tensor(listed, dtype=torch.int32, device=DEV)
    return tiles, torch.tensor([len(listed)], dtype=torch.int32, device=DEV)


def _map_sentinel(B, H, W, ns, dt):
    buf = _sentinel_rows(B * H * W + PAD, ns, dt)
    return buf, buf[:B * H * W].view(B, H, W, ns)


LB, LH, LW = 4, 104, 160   # 4 x 13 x 5 = 260 patches
LPER = (LH // 8) * (LW // 32)
# every patch except five spread over the images -- 255 listed, one short of the 256 workgroups -- and except three: 257, the smallest list
# that hands a workgroup a second patch
DROP5 = [7, LPER + 31, 3 * LPER - 1, 3 * LPER, 4 * LPER - 1]
LISTS = {"all but five": [p for p in range(LB * LPER) if p not in DROP5], "all but three": [p for p in range(LB * LPER) if p not in DROP5[1:4]]}

_CACHE = {}


def _list_case(dt):
    """(pk, act, x on the device, reference) of the 64 -> 256 3x3 layer, computed once per dtype and shared (read-only)"""
    if dt not in _CACHE:
        from gim_amd.packing import pack_conv
        g = torch.Generator().manual_seed(2300)
        w, bn, bias = _layer(g, 64, 256, 3, "bias")
        pk = pack_conv(w, bn, _gim(dt), DEV, stride=1, pad=1, bias=bias)
        x = torch.randn(LB, LH, LW, 64, generator=g)
        ref = F.leaky_relu(F.conv2d(_rnd(x, dt).permute(0, 3, 1, 2), _rnd(w, dt), bias, padding=1), 0.01).permute(0, 2, 3, 1)
        _CACHE[dt] = (pk, _act("leaky"), x.to(_tdt(dt)).to(DEV), ref)
    return _CACHE[dt]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_many_listed_tiles_conv3x3(dt, monkeypatch):
    """ops.conv2d_tiles (igemm_conv_tiles_kernel) against the dense launch on the same 256 x 256 tile (forced: 260 tiles stay under the
    dispatch's 1024); the dense launch (260 tiles on 256 workgroups) against the reference"""
    from gim_amd import ops
    t0 = time.time()
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)
    pk, act, xd, ref = _list_case(dt)
    assert ops.conv_tiles_supported(xd, pk, dense_too=True), "the dense launch would not run on the 256 x 256 tile"
    dense = ops.conv2d(xd, pk, act)
    torch.cuda.synchronize()
    _close(dense, ref, _tol(dt), f"11 conv2d_tiles dense {dt}")
    assert torch.equal(_bits(ops.conv2d(xd, pk, act)), _bits(dense)), "two launches differ"
    for which, listed in LISTS.items():
        buf, y = _map_sentinel(LB, LH, LW, pk.n_store, dt)
        out = ops.conv2d_tiles(xd, pk, *_list_args(listed), act, out=y)
        torch.cuda.synchronize()
        assert out.data_ptr() == y.data_ptr()
        _check_list(y, dense, listed, f"11 conv2d_tiles {dt} {which}")
        assert _untouched(buf[LB * LH * LW:]), "rows beyond M were written"
    print(f"[time] 11 conv2d_tiles {dt}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_many_listed_tiles_halo(dt):
    """ops.conv3x3_halo(..., tiles=...) (conv3x3_halo_tiles_kernel) against its dense launch; that one against the reference"""
    from gim_amd import ops
    t0 = time.time()
    pk, act, xd, ref = _list_case(dt)
    dbuf, dense = _map_sentinel(LB, LH, LW, pk.n_store, dt)
    ops.conv3x3_halo(xd, pk, dense, act)
    torch.cuda.synchronize()
    _close(dense, ref, _tol(dt), f"11 halo dense {dt}")
    assert _untouched(dbuf[LB * LH * LW:]), "rows beyond M were written"
    for which, listed in LISTS.items():
        buf, y = _map_sentinel(LB, LH, LW, pk.n_store, dt)
        tiles, n = _list_args(listed)
        ops.conv3x3_halo(xd, pk, y, act, tiles=tiles, n_tiles=n)
        torch.cuda.synchronize()
        _check_list(y, dense, listed, f"11 halo tiles {dt} {which}")
        assert _untouched(buf[LB * LH * LW:]), "rows beyond M were written"
    print(f"[time] 11 halo tiles {dt}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_many_listed_tiles_ups(dt, monkeypatch):
    """ops.conv2d_ups_tiles (igemm_persistent_tiles_kernel) on a 2 x 136 x 256 map, 272 patches, built as in test_gpu_ups_tiles.py (256 -> 196
    lateral conv, the upsample operand 200 wide), every patch except five listed: 267 on 256 workgroups.  The dense launch (forced onto the
    256 x 256 tile, the upsample-add in its epilogue) against conv + F.interpolate in fp32 at test_conv1x1_fused_upsample_add's tolerance."""
    from gim_amd import ops
    from gim_amd.packing import pack_conv
    t0 = time.time()
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)
    B, H, W, cin, cout = 2, 136, 256, 256, 196
    per = (H // 8) * (W // 32)
    g = torch.Generator().manual_seed(2400)
    w, bn, bias = _layer(g, cin, cout, 1, "bias")
    pk = pack_conv(w, bn, _gim(dt), DEV, bias=bias)
    x = torch.randn(B, H, W, cin, generator=g)
    ups = torch.randn(B, H // 2, W // 2, pk.n_store, generator=g)
    ups[..., cout:] = 0
    xd, ud = x.to(_tdt(dt)).to(DEV), ups.to(_tdt(dt)).to(DEV)
    assert ops.conv_ups_tiles_supported(xd, pk, ud, dense_too=True)
    rows = B * H * W
    dbuf, dense = _map_sentinel(B, H, W, pk.n_store, dt)
    fused = ops.conv_rows(xd.view(-1, cin), pk, (1, 1, rows, 1, rows), dense.view(-1, pk.n_store), ups=ud)
    torch.cuda.synchronize()
    assert fused, "the dense launch did not take the upsample-add in its epilogue"
    assert _untouched(dbuf[rows:]), "rows beyond M were written"
    ref = F.conv2d(_rnd(x, dt).permute(0, 3, 1, 2), _rnd(w, dt), bias) \
        + F.interpolate(_rnd(ups[..., :cout], dt).permute(0, 3, 1, 2), scale_factor=2.0, mode="bilinear", align_corners=True)
    _close(dense[..., :cout], ref.permute(0, 2, 3, 1), HALO_TOL[dt], f"11 ups dense {dt}")
    assert (dense[..., cout:] == 0).all(), "padded output channels are not exact zeros"
    listed = [p for p in range(B * per) if p not in (0, per - 1, per, per + 77, 2 * per - 1)]
    buf, y = _map_sentinel(B, H, W, pk.n_store, dt)
    out = ops.conv2d_ups_tiles(xd, pk, ud, *_list_args(listed), y=y)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    _check_list(y, dense, listed, f"11 ups tiles {dt}")
    assert _untouched(buf[rows:]), "rows beyond M were written"
    print(f"[time] 11 ups tiles {dt}: {time.time() - t0:.2f} s")
