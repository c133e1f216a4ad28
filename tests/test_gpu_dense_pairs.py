"""GPU tests of the dense matchers' pair-list path above the engine: `adapters.HlocDenseMatcher.bank_put` / `match_pairs` against
`forward` called pair by pair, and `dense_sfm.match_dense_pair_list(bank=...)` against the per-pair loop -- same seed, equal bits."""
import numpy as np
import pytest
import torch

import dkm_oracle as DO

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


_NET = {}


def _net():
    if "m" not in _NET:
        from gim_amd.dkm import DKMv3
        m = DKMv3(None, 128, 160, upsample_preds=True, precision="bf16")
        m.upsample_res = (192, 256)
        m.load_state_dict(DO.make_state_dict(0))
        _NET["m"] = m.eval()
    return _NET["m"]


def _images(dev):
    """four unpadded images of two sizes, 150 x 224 and 160 x 224: both are padded to 179 x 224 (the model's 4:5 aspect ratio; `forward`
    matches images of one padded size), by different amounts"""
    a, b = DO.seeded_pair(160, 224, 3)
    c, d = DO.seeded_pair(160, 224, 5, shift=(4, 14))
    return {"a.jpg": a[..., :150, :].contiguous().to(dev), "b.jpg": b.contiguous().to(dev),
            "c.jpg": c[..., :150, :].contiguous().to(dev), "d.jpg": d.contiguous().to(dev)}


def _masks(images):
    """class-id maps with a band of class 0 (blacked out by the plugin)"""
    out = {}
    for i, (name, im) in enumerate(images.items()):
        m = np.ones(im.shape[-2:], dtype=np.int64) * (3 + i)
        m[10 * i:10 * i + 25, :40] = 0
        out[name] = m
    return out


@pytest.mark.parametrize("batch_pairs", [1, 2])
@pytest.mark.parametrize("masked,topk", [(False, None), (True, None), (False, 100)], ids=["plain", "masked", "top-100"])
def test_match_pairs_equals_forward_pair_by_pair(masked, topk, batch_pairs):
    from gim_amd.adapters import HlocDenseMatcher
    from gim_amd.dense_bank import DenseFeatureBank
    dev = _dev()
    images = _images(dev)
    masks = _masks(images) if masked else {}
    adapter = HlocDenseMatcher(_net(), 128, 160, max_num_matches=topk, num_samples=512)
    pairs = [("a.jpg", "b.jpg"), ("b.jpg", "a.jpg"), ("a.jpg", "c.jpg")]
    torch.manual_seed(11)
    ref = []
    for n0, n1 in pairs:
        d = {"image0": images[n0], "image1": images[n1]}
        if masked:
            d["mask0"], d["mask1"] = masks[n0], masks[n1]
        ref.append(adapter(d))
    bank = DenseFeatureBank(adapter.net, 3)
    for n in ("a.jpg", "b.jpg", "c.jpg"):
        adapter.bank_put(bank, n, images[n], masks.get(n))
    torch.manual_seed(11)
    got = adapter.match_pairs(bank, pairs, batch_pairs=batch_pairs)
    assert len(got) == len(ref)
    for p, (g, r) in enumerate(zip(got, ref)):
        print(f"pair {p}: {r['scores'].shape[0]} matches by forward, {g['scores'].shape[0]} by match_pairs")
        assert r["scores"].shape[0] > 0
        for k in ("keypoints0", "keypoints1", "scores", "batch_indexes"):
            assert torch.equal(g[k], r[k]), (p, k)


def test_pair_list_with_a_bank_equals_the_loop():
    """4 images, all 6 pairs, non-unit scales: the keypoints of finalize and every assign() output are those of the per-pair loop"""
    from gim_amd.adapters import HlocDenseMatcher
    from gim_amd.dense_bank import DenseFeatureBank
    from gim_amd.dense_sfm import DenseMatchAggregator, match_dense_pair_list
    dev = _dev()
    images = _images(dev)
    names = list(images)
    pairs = [(names[i], names[j]) for i in range(4) for j in range(i + 1, 4)]
    scales = {"a.jpg": (2.0, 2.0), "b.jpg": (1.5, 1.25), "c.jpg": None, "d.jpg": (1.0, 3.0)}
    adapter = HlocDenseMatcher(_net(), 128, 160, num_samples=512)

    def run(**kw):
        agg = DenseMatchAggregator(device=dev)
        torch.manual_seed(5)
        match_dense_pair_list(adapter, images, pairs, agg, scales, **kw)
        kp = agg.finalize(64)
        return agg, kp, list(agg.assign())

    agg0, kp0, as0 = run()
    agg1, kp1, as1 = run(bank=DenseFeatureBank(adapter.net, 4), batch_pairs=2)
    assert agg0.offsets == agg1.offsets and agg0.offsets[-1] > 0 and agg0.pairs == agg1.pairs
    for a, b in zip(agg0._pool, agg1._pool):
        assert torch.equal(a[:agg0.offsets[-1]], b[:agg0.offsets[-1]])                 # add_pair got the same rows in the same order
    for n in names:
        assert np.array_equal(kp0[n][0], kp1[n][0]) and np.array_equal(kp0[n][1], kp1[n][1]) and len(kp0[n][0]) > 0
    assert len(as0) == len(as1) == len(pairs)
    for (m0, s0), (m1, s1) in zip(as0, as1):
        assert np.array_equal(m0, m1) and np.array_equal(s0, s1)
    # a bank too small for a batch is refused, a small one that fits each batch evicts and re-extracts
    from gim_amd._lib import GimHipError
    with pytest.raises(GimHipError, match="slots"):
        run(bank=DenseFeatureBank(adapter.net, 2), batch_pairs=2)
    agg2, kp2, _ = run(bank=DenseFeatureBank(adapter.net, 2), batch_pairs=1)
    assert agg2.offsets == agg0.offsets and all(np.array_equal(kp0[n][0], kp2[n][0]) for n in names)
