"""GPU tests of the dense matchers' feature bank: gim_dense_gather_pairs / gim_dense_emit_pairs (csrc/dense_bank.hip) against torch
indexing and the torch composition of the per-pair tail, `DenseMatcher.extract` / `match_features` (gim_amd/dense.py) against
`match_batch` on the stacked images -- bit for bit -- and the bookkeeping of gim_amd.dense_bank.DenseFeatureBank."""
import os

import numpy as np
import pytest
import torch

import dkm_oracle as DO
import roma_oracle as RO

pytestmark = pytest.mark.gpu
DTS = ["bf16", "fp16", "fp32"]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the gather
def _gather_case():
    dev = _dev()
    g = torch.Generator().manual_seed(1)
    slots, B = 5, 3
    slabs = [torch.randint(0, 256, (slots, nb), generator=g, dtype=torch.uint8).to(dev) for nb in (16, 4112, 1000016)]
    s0, s1 = [4, 1, 4], [0, 4, 2]          # slot 4 is named twice on one side and once on the other
    return dev, slots, B, slabs, s0, s1


@pytest.mark.parametrize("swapped", [False, True], ids=["query", "support"])
def test_gather_equals_torch_indexing(swapped):
    """three levels of 16 B (one piece), 4 112 B (a ragged tail) and 1 000 016 B (many workgroups, each more than one pass) per slot"""
    from gim_amd import ops
    dev, slots, B, slabs, s0, s1 = _gather_case()
    order = s1 + s0 if swapped else s0 + s1
    idx = torch.tensor(order, dtype=torch.int32, device=dev)
    dst = [torch.full((2 * B, t.shape[1]), 0xA5, dtype=torch.uint8, device=dev) for t in slabs]
    ops.dense_gather_pairs(list(zip(slabs, dst)), idx, slots)
    for t, d in zip(slabs, dst):
        assert torch.equal(d, t[idx.long()])


def test_gather_skips_out_of_range_slots():
    from gim_amd import ops
    dev, slots, B, slabs, s0, s1 = _gather_case()
    idx = torch.tensor([4, -1, 0, slots, 2, 1], dtype=torch.int32, device=dev)
    dst = [torch.full((2 * B, t.shape[1]), 0xA5, dtype=torch.uint8, device=dev) for t in slabs]
    ops.dense_gather_pairs(list(zip(slabs, dst)), idx, slots)
    for t, d in zip(slabs, dst):
        for e, s in enumerate(idx.tolist()):
            if 0 <= s < slots:
                assert torch.equal(d[e], t[s])
            else:
                assert bool((d[e] == 0xA5).all()), (e, s)            # the pre-filled pattern is intact


def test_gather_refuses_bad_arguments():
    import ctypes
    from gim_amd import _lib
    dev = _dev()
    slab = torch.zeros(4, 64, dtype=torch.uint8, device=dev)
    dst = torch.zeros(2, 64, dtype=torch.uint8, device=dev)
    idx = torch.zeros(2, dtype=torch.int32, device=dev)

    def call(slab_ptr, dst_ptr, nbytes, levels):
        a = _lib.DenseGatherArgs()
        a.slab[0], a.dst[0], a.slot_bytes[0], a.n_levels = slab_ptr, dst_ptr, nbytes, levels
        return _lib.lib.gim_dense_gather_pairs(ctypes.byref(a), ctypes.c_void_p(idx.data_ptr()), 2, 4, None)

    assert call(slab.data_ptr(), dst.data_ptr(), 64, 1) == 0
    assert call(slab.data_ptr(), dst.data_ptr(), 40, 1) != 0             # bytes per slot: not a multiple of 16
    assert b"multiple of 16" in _lib.lib.gim_last_error()
    assert call(slab.data_ptr() + 4, dst.data_ptr(), 32, 1) != 0         # a misaligned slab
    assert call(slab.data_ptr(), dst.data_ptr() + 8, 32, 1) != 0
    assert call(slab.data_ptr(), dst.data_ptr(), 64, 0) != 0 and call(slab.data_ptr(), dst.data_ptr(), 64, 9) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the emit
def _torch_tail(sparse, mconf, row, rescale):
    """HlocDenseMatcher.forward's tail + match_dense_pair_list's rescale for one pair, with the package's own pieces"""
    from gim_amd.adapters import _unpad_and_mask
    wp0, hp0, wp1, hp1, pl0, pt0, pl1, pt1, ow0, oh0, ow1, oh1, sx0, sy0, sx1, sy1 = row
    m = mconf > 0
    mconf, sparse = mconf[m], sparse[m].contiguous()
    k0, k1, mask = _unpad_and_mask(sparse, (hp0, wp0), (hp1, wp1), (int(ow0), int(oh0), int(pl0), 0, int(pt0), 0),
                                   (int(ow1), int(oh1), int(pl1), 0, int(pt1), 0))
    k0, k1, sc = k0[mask], k1[mask], mconf[mask]
    out0, out1 = k1, k0                                                     # names switched back
    if rescale:
        out0 = (out0 + 0.5) * out0.new_tensor((sx0, sy0)) - 0.5
        out1 = (out1 + 0.5) * out1.new_tensor((sx1, sy1)) - 0.5
    return out0, out1, sc


@pytest.mark.parametrize("rescale", [True, False], ids=["rescaled", "plain"])
def test_emit_equals_the_torch_composition(rescale):
    from gim_amd import ops
    dev = _dev()
    B, num = 3, 1000
    g = torch.Generator().manual_seed(7)
    sparse = torch.rand(B, num, 4, generator=g) * 2.1 - 1.05
    mconf = torch.rand(B, num, generator=g)
    mconf[:, ::7] = 0.0
    mconf[:, 3::11] = -mconf[:, 3::11]
    # (wp0, hp0, wp1, hp1, pl0, pt0, pl1, pt1, ow0, oh0, ow1, oh1, sx0, sy0, sx1, sy1): pads differ per side, scales are not 1
    rows = [(896.0, 672.0, 640.0, 480.0, 14.0, 0.0, 0.0, 21.0, 827.0, 672.0, 640.0, 438.0, 1.5, 1.25, 0.75, 2.0),
            (512.0, 384.0, 896.0, 672.0, 0.0, 7.0, 40.0, 0.0, 512.0, 370.0, 816.0, 672.0, 1.0, 1.0, 3.0, 0.5),
            (896.0, 672.0, 896.0, 672.0, 5.0, 3.0, 9.0, 11.0, 886.0, 666.0, 878.0, 650.0, 2.0, 2.0, 2.0, 2.0)]
    # coordinates exactly ON the strict bounds after the un-padding (every step exact in fp32: 896 * (x + 1) / 2 - 14):
    # x = -1 + 1/32 -> pixel 0 (rejected: the test is > 0); x = 0.875 -> 826 = ow0 - 1 (kept: the test is <=)
    sparse[0, 1] = torch.tensor([-0.96875, 0.0, 0.0, 0.0])
    sparse[0, 2] = torch.tensor([0.875, 0.0, 0.0, 0.0])
    mconf[0, 1:3] = 0.5
    edge, _ = ops.dense_to_pixels(sparse[0, 1:3].to(dev), (672.0, 896.0), (480.0, 640.0))
    assert (edge[:, 0] - 14.0).tolist() == [0.0, 826.0]
    mconf[1] = -mconf[1].abs()                                              # pair 1: every row rejected
    sparse[2] = sparse[2] * 0.5                                             # pair 2: every row in bounds ...
    mconf[2] = mconf[2].abs() + 0.01                                        # ... and none rejected
    sp, mc = sparse.to(dev), mconf.to(dev)
    k0, k1, sc, count = ops.dense_emit_pairs(sp, mc, ops.dense_pair_geometry(rows, dev), rescale=rescale)
    counts = count.tolist()
    for b in range(B):
        r0, r1, rs = _torch_tail(sp[b], mc[b], rows[b], rescale)
        print(f"pair {b}: {counts[b]} of {num} rows kept (torch composition: {rs.shape[0]})")
        assert counts[b] == rs.shape[0]
        assert torch.equal(k0[b, :counts[b]], r0) and torch.equal(k1[b, :counts[b]], r1) and torch.equal(sc[b, :counts[b]], rs)
    assert counts[1] == 0 and counts[2] == num and 0 < counts[0] < num
    kept0 = _torch_tail(sp[0, 1:3], mc[0, 1:3], rows[0], False)[1]          # of the two edge rows only the one at ow0 - 1 stays
    assert kept0.shape[0] == 1 and kept0[0, 0].item() == 826.0


# ------------------------------------------------------------------------------------------------ 3. match_features == match_batch
def _images3():
    a, b = DO.seeded_pair(160, 224, 3)
    c, _ = DO.seeded_pair(160, 224, 5, shift=(4, 14))
    return a, b, c


_ROMA = {}


def _engine(engine, precision, upsample):
    if engine == "dkm":
        from gim_amd.dkm import DKMv3
        m = DKMv3(None, 128, 160, upsample_preds=upsample, precision=precision)
        m.upsample_res = (192, 256)
        m.load_state_dict(DO.make_state_dict(0))
        return m.eval()
    from gim_amd.roma import RoMa
    if "sd" not in _ROMA:
        _ROMA["sd"], _ROMA["dino"] = RO.make_state_dicts(0)
    if precision not in _ROMA:           # one module per precision: packing the ViT takes a while; resolutions are plain attributes
        m = RoMa([112, 140], precision=precision, dinov2_weights=_ROMA["dino"])
        m.load_state_dict(_ROMA["sd"])
        _ROMA[precision] = m.eval()
    m = _ROMA[precision]
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "roma_match.npz"))
    m.h_resized, m.w_resized, m.upsample_preds = 112, 140, upsample
    m.upsample_res = tuple(int(v) for v in g["up"])
    return m


@pytest.mark.parametrize("upsample", [True, False], ids=["upsample", "low-only"])
@pytest.mark.parametrize("precision", DTS)
@pytest.mark.parametrize("engine", ["dkm", "roma"])
def test_match_features_equals_match_batch(engine, precision, upsample):
    """pairs (A,B), (B,A), (A,C) from a bank of three images, one call: a repeated image and a swapped pair in one batch"""
    from gim_amd.dense_bank import DenseFeatureBank
    dev = _dev()
    m = _engine(engine, precision, upsample)
    A, B, C = (t.to(dev) for t in _images3())
    bank = DenseFeatureBank(m, 3)
    for key, im in (("A", A), ("B", B), ("C", C)):
        bank.put(key, im)
    warp, cert = m.match_features(bank, bank.slots(["A", "B", "A"]), bank.slots(["B", "A", "C"]))
    ref_w, ref_c = m.match_batch(torch.cat((A, B, A)), torch.cat((B, A, C)))
    print(f"{engine} {precision} upsample={upsample}: bank {bank.bytes_per_image} bytes per image; max |warp diff| "
          f"{(warp - ref_w).abs().max().item():.3e}, max |certainty diff| {(cert - ref_c).abs().max().item():.3e}")
    assert warp.shape == ref_w.shape and cert.shape == ref_c.shape
    assert torch.equal(warp, ref_w) and torch.equal(cert, ref_c)


# ------------------------------------------------------------------------------------------------ 4. the bank
def test_bank_behaviour():
    from gim_amd._lib import GimHipError
    from gim_amd.dense_bank import DenseFeatureBank
    dev = _dev()
    m = _engine("dkm", "bf16", True)
    A, B, C = (t.to(dev) for t in _images3())
    bank = DenseFeatureBank(m, 2)
    s = bank.put("A", A)
    first = {k: t[s].clone() for k, t in bank.slabs.items()}
    assert bank.put("A", A) == s                                            # a resident key keeps its slot
    assert all(torch.equal(first[k], t[s]) for k, t in bank.slabs.items())  # extraction is idempotent
    assert bank.bytes_per_image == sum(t[0].numel() * t.element_size() for t in bank.slabs.values()) > 0
    bank.put("B", B)
    bank.slots(["A"])                                                       # A is the most recently used
    bank.put("C", C)                                                        # evicts B
    assert "A" in bank and "C" in bank and "B" not in bank and bank.stats.evictions == 1
    with pytest.raises(GimHipError, match="not resident"):
        bank.slots(["A", "B"])
    with pytest.raises(GimHipError, match="outside"):
        m.match_features(bank, [0], [2])
    with pytest.raises(GimHipError, match="pairs per call"):
        m.match_features(bank, [0] * 9, [1] * 9)
    m.load_state_dict(DO.make_state_dict(0))                                # new weights: the resident state is stale
    assert "A" not in bank
    with pytest.raises(GimHipError, match="not resident"):
        bank.slots(["A"])
    assert bank.stats.invalidations == 1 and len(bank) == 0
    with pytest.raises(GimHipError, match="empty"):
        m.match_features(bank, [0], [1])
    m.precision = "fp16"                                                    # so is a precision change
    bank.put("A", A)
    m.precision = "bf16"
    assert "A" not in bank
