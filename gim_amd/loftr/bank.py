"""Feature cache for pair lists: every image of a ZEB pair file, an exhaustive hloc pairing or a video window runs the LoFTR backbone
ONCE, however many pairs name it.

  FeatureBank        slabs of backbone maps ([slots, H/8, W/8, 256] and [slots, H/2, W/2, 128], one pair of slabs per image shape and
                     dtype) plus the bookkeeping: caller-supplied hashable image key -> slot, LRU eviction, slots of the batch in flight
                     pinned, hit / miss / eviction counts.  The bookkeeping (`SlotTable`, gim_amd/bank.py) is plain Python; torch is
                     touched only when a slab is allocated.
  CachedPairMatcher  a callable with the contract of `model(batch)` (gim_amd.zeb.run_scene(matcher=...), gim_amd.runner): finds the
                     batch's images that are not in the bank, extracts them in one `LoFTR.extract` call, scatters the maps into their
                     slots (gim_slot_copy) and matches the batch from the bank (`LoFTR.match_features` with slot indices).

Memory: at 640x480 an image's maps are 60*80*256 + 240*320*128 = 11 059 200 elements -- 22.1 MB in the 16-bit modes, 44.2 MB in fp32;
`capacity_images` slots of that per image shape are allocated when the first image of the shape arrives.
"""
from ..bank import BankStats, SlotTable


class FeatureBank:
    """`capacity_images` slots per (image shape, dtype) group; see the module docstring.  `tag`: the LoFTR.feature_tag() the resident
    maps were extracted under -- `check_tag` empties the bank when the module has moved on."""

    def __init__(self, capacity_images):
        if capacity_images < 1:
            raise ValueError("capacity_images must be >= 1")
        self.capacity = int(capacity_images)
        self.stats = BankStats()
        self.tag = None
        self._tables = {}   # group -> SlotTable
        self._slabs = {}    # group -> LoFTRFeatures over the two slabs

    def table(self, group):
        t = self._tables.get(group)
        if t is None:
            t = self._tables[group] = SlotTable(self.capacity, self.stats)
        return t

    def assign(self, group, keys):
        return self.table(group).assign(keys)

    def __len__(self):
        return sum(len(t) for t in self._tables.values())

    def __contains__(self, group_key):
        group, key = group_key
        return group in self._tables and key in self._tables[group]

    def invalidate(self):
        """forget every image and free the slabs (the module's weights / precision changed)"""
        if self._tables or self._slabs:
            self.stats.invalidations += 1
        self._tables.clear()
        self._slabs.clear()

    def check_tag(self, tag):
        """True when the bank was valid for `tag`; otherwise it is emptied and re-tagged"""
        if self.tag == tag:
            return True
        self.invalidate()
        self.tag = tag
        return False

    def slabs(self, group, like):
        """the group's slabs as a LoFTRFeatures handle of `capacity` images, allocated on first use with the geometry / dtype of `like`
        (a handle LoFTR.extract returned for images of that group)"""
        h = self._slabs.get(group)
        if h is None:
            import torch
            from .loftr import LoFTRFeatures
            new = lambda t: torch.empty(self.capacity, *t.shape[1:], dtype=t.dtype, device=t.device)   # noqa: E731
            h = self._slabs[group] = LoFTRFeatures(new(like.coarse), new(like.fine), like.hw_i, like.tag)
        return h

    @property
    def nbytes(self):
        return sum(h.nbytes for h in self._slabs.values())


def image_keys(batch):
    """(keys of side 0, keys of side 1) of a batch: batch['image_keys0'] / ['image_keys1'] when present (any hashables, one per pair),
    else (scene_id, pair name) from the ZEB loaders' fields (gim_amd.zeb_data.collate: scene_id = [id per pair], pair_names =
    ([name0 per pair], [name1 per pair]))."""
    if "image_keys0" in batch or "image_keys1" in batch:
        k0, k1 = list(batch["image_keys0"]), list(batch["image_keys1"])
    elif "scene_id" in batch and "pair_names" in batch:
        sid, (n0, n1) = batch["scene_id"], batch["pair_names"]
        if isinstance(sid, str):   # an un-collated single pair
            sid, n0, n1 = [sid], [n0], [n1]
        k0, k1 = [(s, n) for s, n in zip(sid, n0)], [(s, n) for s, n in zip(sid, n1)]
    else:
        raise KeyError("CachedPairMatcher needs batch['image_keys0'] / ['image_keys1'] or the ZEB fields scene_id + pair_names to tell images apart")
    if len(k0) != len(k1):
        raise ValueError(f"{len(k0)} image keys on side 0, {len(k1)} on side 1")
    return k0, k1


class CachedPairMatcher:
    """matcher(batch) == model(batch) for a gim_amd.loftr.LoFTR `model`, with the backbone maps of up to `capacity_images` images per
    image shape kept on the device.  The batch carries color0 / color1 (and image0 / image1, scale*, mask*) as for the module; tensors
    are moved to the module's device.  The images of a key must not change while the key is resident."""

    def __init__(self, model, capacity_images):
        self.model = model
        self.bank = FeatureBank(capacity_images)

    @property
    def stats(self):
        return self.bank.stats

    def _device(self):
        return next(self.model.parameters()).device

    def __call__(self, batch):
        from .loftr import StaleFeaturesError
        dev = self._device()
        for k, v in batch.items():
            if hasattr(v, "is_cuda") and v.device != dev:
                batch[k] = v.to(dev)
        for attempt in range(3):   # a range fallback of the module (fp16 -> bf16, split -> exact products) empties the bank: once more
            self.bank.check_tag(self.model.feature_tag())
            try:
                self._run(batch)
                return None
            except StaleFeaturesError:
                if attempt == 2:
                    raise

    def _fill(self, group, colors, keys_sides):
        """slots of one shape group's keys; the images not resident are extracted (one call) and scattered into their slots.
        colors: [color tensor per side], keys_sides: [keys per side].  Returns (slab handle, [slots per side])."""
        from .. import ops
        from .loftr import StaleFeaturesError
        flat = [k for ks in keys_sides for k in ks]
        slots, missing = self.bank.assign(group, flat)
        if missing:
            want = {k: j for j, (k, _) in enumerate(missing)}
            c = colors[0]
            imgs = c.new_empty((len(missing),) + tuple(c.shape[1:]), dtype=c.dtype)
            for color, ks in zip(colors, keys_sides):
                first = {}
                for b, k in enumerate(ks):
                    if k in want:
                        first.setdefault(k, b)
                if first:
                    ops.slot_copy(color, imgs, src_idx=list(first.values()), dst_idx=[want.pop(k) for k in first])
            feats = self.model.extract(imgs)
            if feats.tag != self.bank.tag:   # the extraction itself moved the module (range guard): what the bank holds is stale
                self.bank.table(group).clear()
                raise StaleFeaturesError("the module changed its mode during extraction")
            slab = self.bank.slabs(group, feats)
            dst = [s for _, s in missing]
            ops.slot_copy(feats.coarse, slab.coarse, dst_idx=dst)
            ops.slot_copy(feats.fine, slab.fine, dst_idx=dst)
        slab = self.bank._slabs[group]
        out, off = [], 0
        for ks in keys_sides:
            out.append(slots[off:off + len(ks)])
            off += len(ks)
        return slab, out

    def _run(self, batch):
        import torch
        k0, k1 = image_keys(batch)
        color0, color1 = batch["color0"], batch["color1"]
        if color0.shape[0] != len(k0) or color1.shape[0] != len(k1):
            raise ValueError("one image key per pair and side is needed")
        color0 = color0.contiguous() if color0.dtype == torch.float32 else color0.float().contiguous()
        color1 = color1.contiguous() if color1.dtype == torch.float32 else color1.float().contiguous()
        g0, g1 = tuple(color0.shape[1:]), tuple(color1.shape[1:])
        if g0 == g1:
            slab, (s0, s1) = self._fill(g0, [color0, color1], [k0, k1])
            h0 = h1 = slab
        else:
            h0, (s0,) = self._fill(g0, [color0], [k0])
            h1, (s1,) = self._fill(g1, [color1], [k1])
        self.model.match_features(h0, h1, s0, s1, data=batch)
