"""Feature bank of the dense matchers: every image of an exhaustive hloc pairing is resized, encoded (at both resolutions) and projected
ONCE, however many pairs name it -- the dense counterpart of gim_amd/loftr/bank.py and gim_amd/lightglue/bank.py (gim_amd/bank.py
`SlotBank` does the bookkeeping here too).

  DenseFeatureBank   `capacity_images` slots of the per-image state `DenseMatcher.extract` returns (gim_amd/dense.py: pyramid levels of
                     both resolutions, the coarse projections, the black-pixel mask), one slab [slots, ...] per tensor kind, allocated when
                     the first image arrives; caller-supplied hashable image key -> slot with LRU eviction.  `put` extracts and stores
                     images, `slots(keys)` names resident images for `DenseMatcher.match_features`, which gathers a pair batch out of the
                     slabs with gim_dense_gather_pairs (csrc/dense_bank.hip).

The state of a slot belongs to ONE module in ONE state (`DenseMatcher.feature_tag()`: weights, device, precision, resolutions): `check`,
called by `put`, `slots` and `match_features`, empties the bank when the module has moved on (load_state_dict, a device move, a
precision change).  A pair that names an image which is no longer resident -- never inserted, evicted, or dropped by such a reset -- raises
GimHipError before anything is launched.

Memory per image: `bytes_per_image` (the README has the figures of the two evaluation sizes).
"""
import torch

from . import ops
from ._lib import GimHipError
from .bank import SlotBank


class DenseFeatureBank(SlotBank):
    GONE = "never inserted, evicted from the {} slots, or dropped when the module changed"

    def __init__(self, model, capacity_images):
        super().__init__(capacity_images, "dense feature bank")
        self.model = model
        self.tag = None
        self.slabs = None       # {kind: [capacity, ...]} in the order extract returns the kinds
        self.device = None
        self.meta = {}          # key -> whatever the caller stored with the image (adapters.HlocDenseMatcher: its padding geometry)

    def __contains__(self, key):
        return self.tag == self.model.feature_tag() and key in self.table

    @property
    def bytes_per_image(self):
        """bytes of one slot over all slabs; None before the first image"""
        if self.slabs is None:
            return None
        return sum(t[0].numel() * t.element_size() for t in self.slabs.values())

    @property
    def nbytes(self):
        return 0 if self.slabs is None else self.bytes_per_image * self.capacity

    def invalidate(self):
        """forget every image and free the slabs"""
        if len(self.table) or self.slabs is not None:
            self.table.stats.invalidations += 1
        self.table.clear()
        self.meta.clear()
        self.slabs = None

    def check(self, model=None):
        """True when the resident state is that of the owning module as it is now; otherwise the bank is emptied and re-tagged"""
        if model is not None and model is not self.model:
            raise GimHipError("this DenseFeatureBank belongs to another module")
        tag = self.model.feature_tag()
        if self.tag == tag:
            return True
        self.invalidate()
        self.tag = tag
        return False

    def _before_lookup(self):
        self.check()

    # ---- device work --------------------------------------------------------------------------------------------------------------
    def put(self, key, image):
        """one image [1,3,H,W] or [3,H,W], padded and masked as `match()` gets it: extracted and stored under `key` (a resident key is
        overwritten in its slot, else the least recently used image makes room).  Returns the slot."""
        if image.dim() == 3:
            image = image[None]
        return self.put_features([key], self.model.extract(image))[0]

    def put_features(self, keys, feats, meta=None):
        """stores what `model.extract` returned for len(keys) images (distinct keys; meta: one caller-side record per image, kept in
        `self.meta[key]`).  Returns their slots."""
        keys = list(keys)
        if len(set(keys)) != len(keys) or len(keys) != len(feats):
            raise GimHipError(f"dense feature bank: {len(keys)} keys (distinct ones are needed) for the state of {len(feats)} images")
        self.check()
        if feats.tag != self.tag:
            raise GimHipError("dense feature bank: the state was extracted before the module changed (weights, device, precision or resolution)")
        first = next(iter(feats.tensors.values()))
        if self.slabs is None:
            for kind, t in feats.tensors.items():
                if (t[0].numel() * t.element_size()) % 16:
                    raise GimHipError(f"dense feature bank: {kind} has {t[0].numel() * t.element_size()} bytes per image, not a multiple of 16")
            self.device = first.device
            self.slabs = {kind: torch.empty(self.capacity, *t.shape[1:], dtype=t.dtype, device=t.device) for kind, t in feats.tensors.items()}
        elif any(tuple(self.slabs[k].shape[1:]) != tuple(t.shape[1:]) or self.slabs[k].dtype != t.dtype for k, t in feats.tensors.items()):
            raise GimHipError("dense feature bank: the images of one bank must have one padded size")   # cannot happen: the model resizes
        slots = self.reserve(keys)
        for kind, t in feats.tensors.items():
            ops.slot_copy(t.contiguous(), self.slabs[kind], dst_idx=slots)
        for k in [k for k in self.meta if k not in self.table]:    # evicted images
            del self.meta[k]
        for i, k in enumerate(keys):
            self.meta[k] = meta[i] if meta is not None else None
        return slots
