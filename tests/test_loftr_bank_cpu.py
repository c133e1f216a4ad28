"""Bookkeeping of gim_amd.loftr.bank (no GPU, no slabs): slot assignment, LRU order, pinning of the batch in flight, capacity errors,
statistics, invalidation; image keys from a collated ZEB batch and from explicit `image_keys*`."""
import pytest
import torch

from gim_amd.loftr.bank import FeatureBank, SlotTable, image_keys

G = (3, 480, 640)   # a shape group


def test_lru_order_and_eviction():
    t = SlotTable(3)
    slots, missing = t.assign(["a", "b", "c"])
    assert sorted(slots) == [0, 1, 2] and [k for k, _ in missing] == ["a", "b", "c"]
    assert t.keys() == ["a", "b", "c"]
    t.assign(["a"])                      # a becomes the most recent
    assert t.keys() == ["b", "c", "a"]
    slot_b = t.slot_of("b")
    slots, missing = t.assign(["d"])     # b is the least recently used: its slot is re-used
    assert missing == [("d", slot_b)] and "b" not in t and t.keys() == ["c", "a", "d"]
    assert t.stats.evictions == 1
    slots, missing = t.assign(["c", "e"])   # c is resident and in the batch: a goes, not c
    assert [k for k, _ in missing] == ["e"] and "a" not in t and "c" in t
    assert len(t) == 3 and len(set(t.slot_of(k) for k in t.keys())) == 3


def test_duplicates_inside_a_batch_take_one_slot():
    t = SlotTable(4)
    keys = ["x", "y", "x", "x", "z", "y"]
    slots, missing = t.assign(keys)
    assert [k for k, _ in missing] == ["x", "y", "z"]
    assert slots[0] == slots[2] == slots[3] and slots[1] == slots[5] and len(set(slots)) == 3
    assert t.stats.misses == 3 and t.stats.hits == 0
    slots2, missing2 = t.assign(["y", "y"])
    assert not missing2 and slots2 == [slots[1]] * 2 and t.stats.hits == 1


def test_pinned_slots_survive_eviction_pressure():
    t = SlotTable(3)
    t.assign(["a", "b", "c"])
    # the batch names the two OLDEST residents and one new image: the only evictable image is c, the most recently used one
    slots, missing = t.assign(["n", "a", "b"])
    assert [k for k, _ in missing] == ["n"] and "c" not in t and "a" in t and "b" in t
    assert len(set(slots)) == 3
    # a full turnover: every resident of the previous batch may go, none of the new batch evicts another of it
    slots, missing = t.assign(["p", "q", "r"])
    assert len(set(slots)) == 3 and len(missing) == 3 and t.keys() == ["p", "q", "r"]


def test_over_capacity_batch_is_refused_and_changes_nothing():
    t = SlotTable(2)
    t.assign(["a", "b"])
    before = (t.keys(), t.stats.as_dict())
    with pytest.raises(ValueError, match="distinct images"):
        t.assign(["a", "c", "d"])
    assert (t.keys(), t.stats.as_dict()) == before
    t.assign(["a", "a", "b", "b"])   # four names, two images: fits
    with pytest.raises(ValueError):
        SlotTable(0)


def test_stats_counts():
    b = FeatureBank(3)
    b.assign(G, ["a", "b"])
    b.assign(G, ["b", "c"])
    b.assign(G, ["d", "a"])      # a is in the batch, so d evicts b, the least recently used of the others
    s = b.stats.as_dict()
    assert s["misses"] == 4 and s["hits"] == 2 and s["evictions"] == 1 and s["invalidations"] == 0
    assert len(b) == 3 and (G, "d") in b and (G, "b") not in b
    # another image shape has its own slots
    b.assign((3, 96, 128), ["a", "z"])
    assert b.stats.misses == 6 and len(b) == 5 and b.stats.evictions == 1


def test_invalidation_empties_the_bank():
    b = FeatureBank(2)
    assert not b.check_tag(("fp16", True, 1))     # first tag: nothing to drop
    assert b.stats.invalidations == 0
    b.assign(G, ["a", "b"])
    assert b.check_tag(("fp16", True, 1)) and len(b) == 2
    assert not b.check_tag(("bf16", True, 2))     # the module moved on (range fallback)
    assert len(b) == 0 and (G, "a") not in b and b.stats.invalidations == 1 and b.tag == ("bf16", True, 2)
    _, missing = b.assign(G, ["a"])
    assert [k for k, _ in missing] == ["a"]
    b.invalidate()
    assert len(b) == 0 and b.nbytes == 0


def _zeb_item(scene, n0, n1):
    return {"image0": torch.zeros(1, 8, 8), "color0": torch.zeros(3, 8, 8), "image1": torch.zeros(1, 8, 8), "color1": torch.zeros(3, 8, 8),
            "scale0": torch.ones(2), "scale1": torch.ones(2), "dataset_name": "GL3D", "scene_id": scene, "pair_id": "0-0",
            "pair_names": (n0, n1), "covisible0": 0.5, "covisible1": 0.5}


def test_keys_from_a_collated_zeb_batch():
    from gim_amd.zeb_data import collate
    batch = collate([_zeb_item("s0", "a", "b"), _zeb_item("s0", "a", "c"), _zeb_item("s1", "a", "b")])
    k0, k1 = image_keys(batch)
    assert k0 == [("s0", "a"), ("s0", "a"), ("s1", "a")] and k1 == [("s0", "b"), ("s0", "c"), ("s1", "b")]
    t = SlotTable(8)
    slots, missing = t.assign(k0 + k1)
    assert len(missing) == 5 and slots[0] == slots[1] != slots[2]     # the same name in another scene is another image
    k0, k1 = image_keys(_zeb_item("s0", "a", "b"))                     # one un-collated pair
    assert k0 == [("s0", "a")] and k1 == [("s0", "b")]


def test_explicit_image_keys_win():
    from gim_amd.zeb_data import collate
    batch = collate([_zeb_item("s0", "a", "b"), _zeb_item("s0", "a", "c")])
    batch["image_keys0"], batch["image_keys1"] = [7, 7], ["p", ("q", 1)]
    assert image_keys(batch) == ([7, 7], ["p", ("q", 1)])
    with pytest.raises(KeyError):
        image_keys({"color0": None})
    with pytest.raises(ValueError):
        image_keys({"image_keys0": [1, 2], "image_keys1": [1]})
