"""The patch-list form of the plain 3 x 3 launch on the 256 x 256 tile (gim_conv2d_tiles, ops.conv2d_tiles): a 3 x 3 / stride 1 / pad 1
convolution on the listed 8 x 32 patches of its output map only.

  1. listed patches are bit-identical to the dense launch on the same tile, every other pixel keeps the sentinel it held;
  2. the count read on the device: 0 writes nothing, a count beyond the capacity is clipped, an entry outside the map is clamped into it;
  3. the predicate, and the wrapper's dense path where it refuses.

The dense reference goes through `force_big_tile` (gim_conv_args.use_lds_dma = 3, the tests' way onto the 256 x 256 tile): the dispatch
sends a launch there on its own from 1024 tiles on, the 8 of the shape below stay under that.  B = 2, H = 16, W = 64: 2 x 2 patches per
image, so a row / column or tiles_x / tiles_y mix-up cannot hide, and every patch has map borders and patch borders among its taps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7B7B   # a finite 16-bit pattern in both kinds that no computed value of these layers takes (fp16 61 280, bf16 3.3e36)
B0, H0, W0 = 2, 16, 64
TOTAL = B0 * (H0 // 8) * (W0 // 32)
LAYERS = {"256->256 leaky": (256, "leaky"), "256->196": (196, "none")}   # the plain instantiation / the fragment-skipping one


def _patches(t):
    """[B,H,W,C] -> [B * H/8 * W/32, 8, 32, C] in patch-index order"""
    B, H, W, C = t.shape
    return t.view(B, H // 8, 8, W // 32, 32, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 8, 32, C)


_CACHE = {}


def _case(tdt, layer):
    """(pk, act, x, dense output) of one layer and dtype, computed once and shared (read-only) by the cases that use it"""
    key = (tdt, layer)
    if key not in _CACHE:
        from gim_amd import ops
        from gim_amd._lib import ACT_LEAKY, ACT_NONE
        from gim_amd.packing import pack_conv
        cout, actname = LAYERS[layer]
        act = ACT_LEAKY if actname == "leaky" else ACT_NONE
        g = torch.Generator().manual_seed(7)
        w = torch.randn(cout, 256, 3, 3, generator=g) / (9 * 256) ** 0.5
        bias = torch.randn(cout, generator=g) * 0.1
        pk = pack_conv(w, None, ops.gim_dtype(torch.empty(0, dtype=tdt)), DEV, stride=1, pad=1, bias=bias)
        x = torch.randn(B0, H0, W0, pk.cin_pad, generator=g).to(DEV, tdt)
        assert ops.conv_tiles_supported(x, pk, dense_too=True), "the dense reference would not run on the 256 x 256 tile"
        dense = ops.conv2d(x, pk, act)
        torch.cuda.synchronize()
        assert torch.isfinite(dense.float()).all() and float(dense.float().abs().max()) > 0.5
        assert bool((dense.float() < 0).any())   # the activation slot has something to do
        _CACHE[key] = (pk, act, x, dense)
    return _CACHE[key]


def _run(tdt, layer, listed, expect, count=None, cap=None):
    """run the list launch over `listed` (count / capacity as given) into a sentinel-filled map; `expect`: the patches that must come out
    as the dense launch writes them -- every other one must still hold the sentinel"""
    from gim_amd import ops
    pk, act, x, dense = _case(tdt, layer)
    cap = max(len(listed), 1) if cap is None else cap
    tiles = torch.full((cap,), 2 ** 31 - 1, dtype=torch.int32)   # entries behind the count must not be walked
    k = min(len(listed), cap)
    tiles[:k] = torch.tensor(listed[:k], dtype=torch.int32)
    n = torch.tensor([len(listed) if count is None else count], dtype=torch.int32, device=DEV)
    y = torch.full((B0, H0, W0, pk.n_store), SENTINEL, dtype=torch.int16, device=DEV).view(tdt)
    out = ops.conv2d_tiles(x, pk, tiles.to(DEV), n, act, out=y)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    on = torch.zeros(TOTAL, dtype=torch.bool, device=DEV)
    if expect:
        on[list(expect)] = True
    yp, dp = _patches(y).view(torch.int16), _patches(dense).view(torch.int16)
    bad = (yp[on] != dp[on]).flatten(1).any(1)
    print(f"{tdt} {layer}: {int(on.sum())} of {TOTAL} patches expected, {int(bad.sum())} differ from the dense launch")
    assert not bool(bad.any()), "a listed patch differs from the dense launch"
    assert bool((yp[~on] == SENTINEL).all()), "a patch outside the list was written"
    assert not bool((dp == SENTINEL).all(-1).any()), "the sentinel is a value of the layer"


@pytest.fixture
def big_tile(monkeypatch):
    from gim_amd import ops
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", True)


LISTS = {
    "all": list(range(TOTAL)),
    "corner and two touching": [0, 5, 7],       # image 0's first patch; image 1's right column, top and bottom (they share a patch border)
    "last of image 0, first of image 1": [3, 4],   # neighbours in memory, not in any map: the taps must not cross the image border
}


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("which", list(LISTS))
def test_listed_patches_equal_the_dense_launch(big_tile, tdt, layer, which):
    _run(tdt, layer, LISTS[which], LISTS[which])


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer", list(LAYERS))
def test_count_and_entries_are_clipped(big_tile, tdt, layer):
    _run(tdt, layer, [1, 2, 6], [], count=0)                                 # a count of 0 writes nothing
    _run(tdt, layer, [1, 2, 6], [], count=-3)
    _run(tdt, layer, list(range(TOTAL)), [0, 1, 2], count=1000, cap=3)       # *n_tiles beyond the capacity: the first `cap` entries
    _run(tdt, layer, [2, 100], [2, TOTAL - 1])                               # an entry outside the map is clamped into it ...
    _run(tdt, layer, [-5, 6], [0, 6])                                        # ... from either side


def test_predicate_and_dense_path(big_tile):
    from gim_amd import ops
    from gim_amd._lib import ACT_LEAKY, GIM_F32
    from gim_amd.packing import pack_conv
    pk, act, x, dense = _case(torch.float16, "256->256 leaky")
    ok = lambda B, H, W, **kw: ops.conv_tiles_supported((B, H, W, pk.cin_pad), pk, **kw)
    assert ok(2, 16, 64) and ok(1, 8, 32) and ok(2, 16, 64, dense_too=True)
    assert not ok(2, 16, 48)          # W % 32 != 0
    assert not ok(2, 12, 64)          # H % 8 != 0
    assert ok(1024, 64, 128) and not ok(1025, 64, 128)      # 32 768 patches at the most
    g = torch.Generator().manual_seed(1)
    pk1 = pack_conv(torch.randn(256, 256, 1, 1, generator=g) / 16, None, pk.dtype, DEV)
    assert not ops.conv_tiles_supported((2, 16, 64, pk1.cin_pad), pk1)               # not a 3 x 3
    pk128 = pack_conv(torch.randn(128, 256, 3, 3, generator=g) / 48, None, pk.dtype, DEV, stride=1, pad=1)
    assert not ops.conv_tiles_supported((2, 16, 64, pk128.cin_pad), pk128)           # npad % 256 != 0
    pk32 = pack_conv(torch.randn(256, 256, 3, 3, generator=g) / 48, None, GIM_F32, DEV, stride=1, pad=1)
    assert not ops.conv_tiles_supported((2, 16, 64, pk32.cin_pad), pk32)             # fp32 operands
    # the wrapper runs a refused launch dense: the whole map, whatever the list says
    x48 = torch.randn(2, 16, 48, pk.cin_pad, generator=g).to(DEV, torch.float16)
    none = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.conv2d_tiles(x48, pk, torch.zeros(8, dtype=torch.int32, device=DEV), none, ACT_LEAKY)
    ref = ops.conv2d(x48, pk, ACT_LEAKY)
    torch.cuda.synchronize()
    assert got.shape == ref.shape and torch.equal(got, ref)


def test_dense_launch_of_a_small_map_is_not_the_same_tile(monkeypatch):
    """without force_big_tile the 8-tile dense launch runs on another tile: `dense_too` says so, and the module keeps such a layer dense"""
    from gim_amd import ops
    monkeypatch.setattr(ops, "FORCE_BIG_TILE", False)
    pk = _case(torch.float16, "256->256 leaky")[0]
    assert ops.conv_tiles_supported((2, 16, 64, pk.cin_pad), pk) and not ops.conv_tiles_supported((2, 16, 64, pk.cin_pad), pk, dense_too=True)
    assert ops.conv_tiles_supported((16, 120, 160, pk.cin_pad), pk, dense_too=True)   # the benchmark's 1/4-level maps: 1 200 tiles
