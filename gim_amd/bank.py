"""The bookkeeping every "encode each image once, match a pair list by slot" path shares; plain Python, torch is imported only where a
function needs it.

  BankStats / SlotTable   caller-supplied hashable image key -> slot over a fixed number of slots, LRU eviction, the slots of the batch in
                          flight pinned, hit / miss / eviction counts.
  SlotBank                the base of the banks with ONE table (gim_amd/lightglue/bank.py KeypointBank, gim_amd/nn_match.py DescriptorBank,
                          gim_amd/dense_bank.py DenseFeatureBank): `reserve` for an insertion, `slots` for a look-up that refuses what is
                          not resident, `check_slots` for host slot indices.  The slabs and the device work are the subclasses'.
                          (LoFTR's FeatureBank, gim_amd/loftr/bank.py, keeps one table per image shape and is no SlotBank.)
  pair_batches            a pair list cut into batches
  sparse_pair_list        the pair-list driver of the sparse matchers: slots per batch, one batched match, hloc's datasets per pair
"""
import collections

from ._lib import GimHipError
from .hloc_formats import write_sparse_matches


class BankStats:
    """hits / misses count image LOOK-UPS per distinct image of a batch (an image named twice in one batch is one look-up);
    evictions count images dropped to make room; invalidations count whole-bank resets (the module's tag changed)"""

    def __init__(self):
        self.hits = self.misses = self.evictions = self.invalidations = 0

    def as_dict(self):
        return {"hits": self.hits, "misses": self.misses, "evictions": self.evictions, "invalidations": self.invalidations}

    def __repr__(self):
        return f"BankStats({self.as_dict()})"


class SlotTable:
    """key -> slot over a fixed number of slots, least recently used key evicted first, pinned slots never."""

    def __init__(self, slots, stats=None):
        if slots < 1:
            raise ValueError("a slot table needs at least one slot")
        self.slots = int(slots)
        self.stats = stats if stats is not None else BankStats()
        self._lru = collections.OrderedDict()   # key -> slot, least recently used first
        self._free = list(range(self.slots - 1, -1, -1))
        self._pinned = set()

    def __len__(self):
        return len(self._lru)

    def __contains__(self, key):
        return key in self._lru

    def keys(self):
        """keys, least recently used first"""
        return list(self._lru)

    def slot_of(self, key):
        return self._lru.get(key)

    def unpin(self):
        self._pinned.clear()

    def assign(self, keys):
        """Slots for the images of ONE batch.  `keys`: the batch's image keys, duplicates allowed.  Returns (slots, missing): slots[i] is the
        slot of keys[i] (equal keys share one slot); missing = [(key, slot)] of the distinct keys that were not resident, in first-use
        order -- the caller fills those slots before it reads any.  Every slot of the batch stays pinned until the next assign() /
        unpin(): making room for one image of the batch never evicts another.  ValueError when the batch needs more distinct images than
        there are slots (nothing is changed then)."""
        distinct = list(dict.fromkeys(keys))
        if len(distinct) > self.slots:
            raise ValueError(f"the batch names {len(distinct)} distinct images, the bank has {self.slots} slots per image shape")
        self.unpin()
        missing = []
        for k in distinct:   # residents first: pinned before anything is evicted
            if k in self._lru:
                self._lru.move_to_end(k)
                self._pinned.add(self._lru[k])
                self.stats.hits += 1
        for k in distinct:
            if k in self._lru:
                continue
            self.stats.misses += 1
            if self._free:
                slot = self._free.pop()
            else:
                victim = next(kk for kk, s in self._lru.items() if s not in self._pinned)   # exists: distinct <= slots
                slot = self._lru.pop(victim)
                self.stats.evictions += 1
            self._lru[k] = slot
            self._pinned.add(slot)
            missing.append((k, slot))
        return [self._lru[k] for k in keys], missing

    def clear(self):
        self._lru.clear()
        self._free = list(range(self.slots - 1, -1, -1))
        self._pinned.clear()


class SlotBank:
    """`capacity_images` slots behind one `SlotTable`.  `what` names the bank in every message ("keypoint bank", ...)."""

    GONE = "never inserted, or evicted from the {} slots"   # why an image may not be resident; {}: the capacity

    def __init__(self, capacity_images, what):
        if capacity_images < 1:
            raise ValueError(f"a {what} needs at least one slot")
        self.what = what
        self.capacity = int(capacity_images)
        self.table = SlotTable(self.capacity)

    @staticmethod
    def resolve_device(device):
        """torch.device(device), a bare "cuda" made the current device"""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    @property
    def stats(self):
        return self.table.stats

    def __len__(self):
        return len(self.table)

    def __contains__(self, key):
        return key in self.table

    def _before_lookup(self):
        """called by `slots` before it looks anything up (the dense bank drops what another module state extracted)"""

    def reserve(self, keys):
        """slots for the images about to be inserted (distinct keys; a resident key keeps its slot and is overwritten), the least
        recently used images evicted to make room.  Refused -- and nothing changed -- for equal keys or more images than slots."""
        keys = list(keys)
        if len(set(keys)) != len(keys):
            raise ValueError(f"{self.what}: the images of one insertion must have distinct keys")
        try:
            slots, _ = self.table.assign(keys)
        except ValueError as e:
            raise GimHipError(f"{self.what}: {e}") from e
        self.table.unpin()
        return slots

    def slots(self, keys):
        """slots of resident images, one per key (duplicates allowed); marks them most recently used.  An image that was never
        inserted, or has been evicted since, raises: a pair must not read whatever lives in its old slot now."""
        self._before_lookup()
        keys = list(keys)
        gone = [k for k in dict.fromkeys(keys) if k not in self.table]
        if gone:
            raise GimHipError(f"{self.what}: image {gone[0]!r} is not resident ({self.GONE.format(self.capacity)})"
                              + (f"; {len(gone) - 1} more" if len(gone) > 1 else ""))
        out = []
        for i in range(0, len(keys), self.capacity):   # SlotTable.assign takes at most `capacity` distinct keys at a time
            out += self.table.assign(keys[i:i + self.capacity])[0]
        self.table.unpin()
        return out

    def check_slots(self, idx):
        """a host sequence of slot indices, range-checked"""
        idx = [int(i) for i in idx]
        bad = [i for i in idx if not 0 <= i < self.capacity]
        if bad:
            raise GimHipError(f"{self.what}: slot {bad[0]} is outside [0, {self.capacity})")
        return idx


def pair_batches(pairs, batch_pairs):
    """the pair list cut into consecutive batches of `batch_pairs` (the last one may be shorter; an empty list gives no batch)"""
    if batch_pairs < 1:
        raise ValueError("batch_pairs must be >= 1")
    pairs = list(pairs)
    return [pairs[i:i + batch_pairs] for i in range(0, len(pairs), batch_pairs)]


def sparse_pair_list(bank, pairs, batch_pairs, match_batch, writer=None, names=None, counts0=None):
    """pairs: a sequence of (key0, key1) of images resident in `bank`, matched as given, in the order given, `batch_pairs` per call of
    `match_batch(slots0, slots1)`, which returns one (matches0 int16, matching_scores0 fp16) pair of numpy arrays per pair of the batch
    (views of ONE host copy per array).  Returns [(key0, key1, matches0, matching_scores0)]; with `writer` (h5py's group protocol) every
    pair is also written through hloc_formats.write_sparse_matches (group name from names[key] if `names` is given, else str(key)).
    counts0(slots0) -> the keypoint counts of the batch's first images, for a matcher whose rows are padded to the bank's capacity: each
    pair's arrays are cut to image 0's own count, the length hloc's datasets have."""
    name = (lambda k: names[k]) if names is not None else str
    out = []
    for batch in pair_batches(pairs, batch_pairs):
        s0, s1 = bank.slots([p[0] for p in batch]), bank.slots([p[1] for p in batch])
        n0 = counts0(s0) if counts0 is not None else [None] * len(batch)
        for (k0, k1), (m, s), n in zip(batch, match_batch(s0, s1), n0):
            m, s = m[:n], s[:n]
            if writer is not None:
                write_sparse_matches(writer, name(k0), name(k1), m, s)
            out.append((k0, k1, m, s))
    return out
