"""gim_amd/bank.py without a GPU: the contract of `SlotBank` stated once and run against the three banks built on it (the launches
stubbed: only the bookkeeping is under test), `pair_batches`, and `sparse_pair_list` with a fake bank and a fake batched matcher."""
import numpy as np
import pytest
import torch

from gim_amd._lib import GimHipError
from gim_amd.bank import SlotBank, pair_batches, sparse_pair_list

CAPACITY = 4


class _FakeModel:
    """what DenseFeatureBank needs of a DenseMatcher"""

    def feature_tag(self):
        return ("m", 0)


def _keypoint_bank():
    from gim_amd.lightglue import KeypointBank
    bank = KeypointBank(CAPACITY, 1, device="cpu")
    return bank, bank.reserve                          # put_many is reserve + a launch on device tensors: there is no CPU path


def _descriptor_bank():
    from gim_amd.nn_match import DescriptorBank
    bank = DescriptorBank(CAPACITY, 8, D=16, device="cpu")
    return bank, lambda keys: [bank.put(k, torch.zeros(3, 2), torch.zeros(3, 16)) for k in keys]


def _dense_bank():
    from gim_amd.dense import DenseFeatures
    from gim_amd.dense_bank import DenseFeatureBank
    model = _FakeModel()
    bank = DenseFeatureBank(model, CAPACITY)
    return bank, lambda keys: bank.put_features(keys, DenseFeatures({"lo1": torch.zeros(len(keys), 4, 4, 8, dtype=torch.bfloat16)},
                                                                    model.feature_tag()))


@pytest.fixture(params=[_keypoint_bank, _descriptor_bank, _dense_bank], ids=["keypoint", "descriptor", "dense"])
def bank_insert(request, monkeypatch):
    from gim_amd import ops
    monkeypatch.setattr(ops, "nn_bank_put", lambda *a, **k: None)      # no device here
    monkeypatch.setattr(ops, "slot_copy", lambda *a, **k: None)
    return request.param()


# the look-ups of the sequence below, per distinct key of a call: what every bank must have counted at its end
WANT_STATS = {"misses": 3 + 1 + 1,          # a b c, d, e
              "hits": 2 + 1 + 2 * 4,        # c a c; a overwritten; e d c a twice, CAPACITY names per table call
              "evictions": 1,               # b for e
              "invalidations": 0}


def test_slot_bank_contract(bank_insert):
    bank, insert = bank_insert
    assert isinstance(bank, SlotBank) and bank.capacity == CAPACITY and len(bank) == 0

    def state():
        return bank.table.keys(), [bank.table.slot_of(k) for k in bank.table.keys()], bank.stats.as_dict()

    # insert, then look up
    sa, sb, sc = insert(["a", "b", "c"])
    assert sorted((sa, sb, sc)) == [0, 1, 2] and len(bank) == 3 and "a" in bank and "d" not in bank
    assert bank.slots(["c", "a", "c"]) == [sc, sa, sc]                   # duplicates share a slot; b is now the least recently used
    # LRU eviction
    assert insert(["d"]) == [3] and bank.stats.evictions == 0
    assert insert(["e"]) == [sb] and "b" not in bank and bank.stats.evictions == 1
    # overwrite
    assert insert(["a"]) == [sa] and bank.stats.evictions == 1 and len(bank) == CAPACITY
    # not resident: evicted, never seen
    before = state()
    with pytest.raises(GimHipError, match="'b' is not resident") as e:
        bank.slots(["a", "b"])
    assert "more" not in str(e.value) and str(e.value).startswith(bank.what)
    with pytest.raises(GimHipError, match=r"'never' is not resident.*; 1 more"):
        bank.slots(["e", "never", "b", "never"])
    assert state() == before
    # more names than slots, all resident
    assert bank.slots(["e", "d", "c", "a"] * 2) == [sb, 3, sc, sa] * 2
    # refused insertions
    before = state()
    with pytest.raises(ValueError, match="distinct"):
        bank.reserve(["x", "x"])
    with pytest.raises(GimHipError, match="5 distinct images"):
        bank.reserve(list("vwxyz"))
    assert state() == before
    # host slot indices
    assert bank.check_slots([CAPACITY - 1, 0]) == [CAPACITY - 1, 0] and bank.check_slots(np.array([1], dtype=np.int64)) == [1]
    for bad in (-1, CAPACITY):
        with pytest.raises(GimHipError, match=f"slot {bad} is outside"):
            bank.check_slots([0, bad])
    assert bank.stats.as_dict() == WANT_STATS


def test_a_bank_needs_a_slot():
    with pytest.raises(ValueError):
        SlotBank(0, "bank")
    assert SlotBank.resolve_device("cpu") == torch.device("cpu")


def test_pair_batches():
    pairs = [(i, i + 1) for i in range(6)]
    assert pair_batches([], 3) == []
    assert pair_batches(pairs, 3) == [pairs[:3], pairs[3:]]               # an exact multiple
    assert pair_batches(pairs + [(9, 0)], 3) == [pairs[:3], pairs[3:], [(9, 0)]]   # and one over it
    assert pair_batches(iter(pairs), 8) == [pairs]
    with pytest.raises(ValueError):
        pair_batches(pairs, 0)


# ------------------------------------------------------------------------------------------------ sparse_pair_list
class _FakeH5(dict):
    """the slice of h5py's group protocol the writers use"""

    def create_group(self, name):
        self[name] = _FakeH5()
        return self[name]

    def create_dataset(self, name, data):
        self[name] = np.asarray(data)


class _FakeBank:
    def __init__(self, keys):
        self.slot = {k: i for i, k in enumerate(keys)}
        self.calls = []

    def slots(self, keys):
        self.calls.append(list(keys))
        gone = [k for k in keys if k not in self.slot]
        if gone:
            raise GimHipError(f"fake bank: image {gone[0]!r} is not resident")
        return [self.slot[k] for k in keys]


def _fake_matcher(batches):
    def match_batch(s0, s1):
        """pair (i, j): matches0 = [i, j, -1] int16, matching_scores0 = [i / 8, j / 8, 0] fp16 -- rows of one array per batch"""
        batches.append((list(s0), list(s1)))
        m = np.array([[a, b, -1] for a, b in zip(s0, s1)], dtype=np.int16)
        return zip(m, (m.clip(0) / 8).astype(np.float16))
    return match_batch


def test_sparse_pair_list_batches_in_order_and_writes_what_it_returns():
    from gim_amd.hloc_formats import pair_key
    keys = ["a", "b", "c", "d"]
    pairs = [("a", "b"), ("c", "a"), ("b", "d"), ("d", "d"), ("b", "a")]
    bank, batches, fd = _FakeBank(keys), [], _FakeH5()
    out = sparse_pair_list(bank, pairs, 2, _fake_matcher(batches), writer=fd, names={k: k + ".jpg" for k in keys})
    assert [(k0, k1) for k0, k1, _, _ in out] == pairs                   # the order of `pairs`
    assert bank.calls == [["a", "c"], ["b", "a"], ["b", "d"], ["d", "d"], ["b"], ["a"]]   # once per side per batch
    assert batches == [([0, 2], [1, 0]), ([1, 3], [3, 3]), ([1], [0])]    # once per batch, a short last one
    assert len(fd) == len(pairs)
    for k0, k1, m, s in out:
        assert m.dtype == np.int16 and s.dtype == np.float16 and m.tolist() == [bank.slot[k0], bank.slot[k1], -1]
        grp = fd[pair_key(k0 + ".jpg", k1 + ".jpg")]
        assert sorted(grp) == ["matches0", "matching_scores0"]
        assert grp["matches0"].dtype == np.int16 and np.array_equal(grp["matches0"], m)
        assert grp["matching_scores0"].dtype == np.float16 and np.array_equal(grp["matching_scores0"], s)
    # no writer, no names: the same list, groups would be named str(key)
    again = sparse_pair_list(_FakeBank(keys), pairs, 8, _fake_matcher([]))
    assert all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) for a, b in zip(out, again)) and len(again) == 5
    assert sparse_pair_list(None, [], 8, None) == []
    with pytest.raises(ValueError):
        sparse_pair_list(bank, pairs, 0, _fake_matcher([]))


def test_sparse_pair_list_refuses_a_batch_before_it_is_matched():
    bank, batches = _FakeBank(["a", "b"]), []
    with pytest.raises(GimHipError, match="'z' is not resident"):
        sparse_pair_list(bank, [("a", "b"), ("b", "a"), ("a", "z"), ("b", "b")], 2, _fake_matcher(batches))
    assert batches == [([0, 1], [1, 0])]                                 # the first batch ran, the one that names z did not
