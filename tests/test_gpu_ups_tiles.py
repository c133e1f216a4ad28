"""The patch-list form of the FPN's lateral launch (gim_conv2d_ups_tiles, ops.conv2d_ups_tiles): the 1x1 conv + bilinear x2 + add of
gim_conv2d_bn_act with `ups`, on the listed 8 x 32 patches of the output map only.

  1. listed patches are bit-identical to the dense launch, every other pixel keeps the sentinel it held;
  2. a non-square map of the minimum size, where a row / column or tiles_x / tiles_y mix-up cannot hide;
  3. the predicate, and the wrapper's dense path where it refuses.

The dense reference goes through `force_big_tile` (gim_conv_args.use_lds_dma = 3, the tests' way onto the 256 x 256 tile): the dispatch
sends a lateral launch there on its own from 1024 tiles on, the 512 of the shape below stay under that."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7B7B   # a finite 16-bit pattern in both kinds that no computed value of these layers takes (fp16 61 280, bf16 3.3e36)


def _lateral(tdt, cin=256, cout=196, seed=5):
    from gim_amd import ops
    from gim_amd.packing import pack_conv
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    return pack_conv(w, None, ops.gim_dtype(torch.empty(0, dtype=tdt)), DEV)


def _patches(t):
    """[B,H,W,C] -> [B * H/8 * W/32, 8, 32, C] in patch-index order"""
    B, H, W, C = t.shape
    return t.view(B, H // 8, 8, W // 32, 32, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 8, 32, C)


_CACHE = {}


def _case(tdt, B, H, W, ups_ld):
    """(pk, x, ups, dense output) of one shape and dtype, computed once and shared (read-only) by the cases that use it"""
    key = (tdt, B, H, W, ups_ld)
    if key not in _CACHE:
        from gim_amd import ops
        pk = _lateral(tdt)
        g = torch.Generator().manual_seed(11)
        x = torch.randn(B, H, W, pk.cin_pad, generator=g).to(DEV, tdt)
        ups = torch.randn(B, H // 2, W // 2, ups_ld, generator=g).to(DEV, tdt)
        assert ups_ld >= pk.n_store
        dense = torch.empty(B, H, W, pk.n_store, dtype=tdt, device=DEV)
        rows = B * H * W
        fused = ops.conv_rows(x.view(-1, pk.cin_pad), pk, (1, 1, rows, 1, rows), dense.view(-1, pk.n_store), ups=ups)
        torch.cuda.synchronize()
        assert fused, "the dense reference did not take the upsample-add in its epilogue"
        assert torch.isfinite(dense.float()).all() and float(dense.float().abs().max()) > 0.5
        _CACHE[key] = (pk, x, ups, dense)
    return _CACHE[key]


def _run(tdt, B, H, W, ups_ld, listed, count=None, cap=None):
    from gim_amd import ops
    pk, x, ups, dense = _case(tdt, B, H, W, ups_ld)
    total = B * (H // 8) * (W // 32)
    cap = total if cap is None else cap
    tiles = torch.full((cap,), 2 ** 31 - 1, dtype=torch.int32)   # entries behind the count must not be walked
    k = min(len(listed), cap)
    tiles[:k] = torch.tensor(listed[:k], dtype=torch.int32)
    n = torch.tensor([len(listed) if count is None else count], dtype=torch.int32, device=DEV)
    y = torch.full((B, H, W, pk.n_store), SENTINEL, dtype=torch.int16, device=DEV).view(tdt)
    assert ops.conv_ups_tiles_supported(x, pk, ups)
    out = ops.conv2d_ups_tiles(x, pk, ups, tiles.to(DEV), n, y=y)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    on = torch.zeros(total, dtype=torch.bool, device=DEV)
    if k:
        on[listed[:k]] = True
    yp, dp = _patches(y).view(torch.int16), _patches(dense).view(torch.int16)
    bad = (yp[on] != dp[on]).flatten(1).any(1)
    print(f"{tdt} {B}x{H}x{W}: {int(on.sum())} of {total} patches listed, {int(bad.sum())} differ from the dense launch")
    assert not bool(bad.any()), "a listed patch differs from the dense launch"
    assert bool((yp[~on] == SENTINEL).all()), "a patch outside the list was written"
    assert not bool((dp == SENTINEL).all(-1).any()), "the sentinel is a value of the layer"


@pytest.fixture
def big_tile(monkeypatch):
    from gim_amd import ops
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)


B0, H0, W0 = 2, 256, 256            # 512 patches, 32 x 8 per image
PER, TX = (H0 // 8) * (W0 // 32), W0 // 32
LISTS = {
    "empty": [],
    "one": [PER + 5 * TX + 3],
    "corners of the last image": [PER, PER + TX - 1, 2 * PER - TX, 2 * PER - 1],   # source rows 0 / h - 1, source columns 0 / w - 1
    "row ends": [7 * TX, 7 * TX + TX - 1],
    "all": list(range(2 * PER)),
    "random 60 %": sorted(torch.randperm(2 * PER, generator=torch.Generator().manual_seed(3))[:(2 * PER * 6) // 10].tolist()),
}


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("which", list(LISTS))
def test_listed_patches_equal_the_dense_launch(big_tile, tdt, which):
    _run(tdt, B0, H0, W0, 200, LISTS[which])


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_count_beyond_capacity_is_clipped(big_tile, tdt):
    """*n_tiles = 1000 with a 40-entry list: the first 40 are computed, nothing else (as gim_conv3x3_halo_tiles clips it)"""
    _run(tdt, B0, H0, W0, 200, LISTS["random 60 %"], count=1000, cap=40)


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_non_square_map(big_tile, tdt):
    """W = 64 (two patches per row), H = 8 (one patch row) per image, 6 images: patch p is image p / 2, columns 32 (p % 2) .. + 31"""
    _run(tdt, 6, 8, 64, 200, [1, 2, 5, 6, 8, 11])
    _run(tdt, 6, 8, 64, 200, list(range(12)))


def test_predicate_and_dense_path(big_tile):
    from gim_amd import ops
    from gim_amd._lib import ACT_LEAKY
    pk = _lateral(torch.float16)
    ok = lambda B, H, W, **kw: ops.conv_ups_tiles_supported((B, H, W, pk.cin_pad), pk, (B, H // 2, W // 2, pk.n_store), **kw)
    assert ok(2, 16, 64) and ok(1, 8, 32)
    assert not ok(2, 16, 48)          # W % 32 != 0
    assert not ok(2, 12, 64)          # H % 8 != 0
    assert not ok(2, 16, 64, act=ACT_LEAKY)
    assert not ok(2, 16, 64, res=True)
    from gim_amd.packing import pack_conv
    from gim_amd._lib import GIM_F32
    g = torch.Generator().manual_seed(1)
    pk32 = pack_conv(torch.randn(196, 256, 1, 1, generator=g) / 16, None, GIM_F32, DEV)
    assert not ops.conv_ups_tiles_supported((2, 16, 64, pk32.cin_pad), pk32, (2, 8, 32, pk32.n_store))
    # the wrapper runs a refused launch dense: the whole map, whatever the list says
    for tdt, p, shape in ((torch.float32, pk32, (2, 16, 64)), (torch.float16, pk, (2, 16, 48))):
        B, H, W = shape
        x = torch.randn(B, H, W, p.cin_pad, generator=g).to(DEV, tdt)
        ups = torch.randn(B, H // 2, W // 2, p.n_store, generator=g).to(DEV, tdt)
        none = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ops.conv2d_ups_tiles(x, p, ups, torch.zeros(8, dtype=torch.int32, device=DEV), none)
        ref = ops.conv2d(x, p, ups=ups)
        torch.cuda.synchronize()
        assert got.shape == ref.shape and torch.equal(got, ref)
