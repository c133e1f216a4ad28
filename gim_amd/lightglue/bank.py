"""Keypoint bank for pair lists: every image of an exhaustive hloc pairing runs SuperPoint ONCE and is uploaded ONCE, however many pairs
name it -- the sparse counterpart of gim_amd/loftr/bank.py (gim_amd/bank.py `SlotBank` does the bookkeeping of both kinds of bank).

  KeypointBank   `capacity_images` slots of up to `num_keypoints` keypoints on the device (csrc/lg_bank.hip for the layout):
                     kpts [S, K, 2] fp32, desc [S, K, 256] fp32 | fp16 (`storage`), enc [S, K, 64] fp32
                 `num_keypoints` is the CAPACITY of a slot: an image may hold any 0 <= n <= K keypoints.  `counts` keeps n per slot on
                 the host, `n` is the same table on the device (int32 [S]) for the ragged kernels; rows [n, K) of a slot are zero after
                 the insertion and are never read into a result (gim_lg_gather_pairs_ragged masks by count).
                 plus caller-supplied hashable image key -> slot with LRU eviction.  `put` inserts images (gim_lg_bank_put: descriptor
                 rounding, keypoints and the positional encoding in one launch), `slots(keys)` names resident images for
                 `LightGlue.match_pairs`.

The encoding of a slot is LightGlue's cos | sin table of the image's keypoints: a function of the image and of the matcher's `posenc.Wr`
only.  It therefore belongs to ONE LightGlue module in ONE packing epoch (`LightGlue._pack_epoch`: load_state_dict / _apply move it):
`ensure_encodings`, called by `match_pairs`, rebuilds the table of every resident image from the kept fp32 keypoints and sizes when
another module, or the same one after a repack, shows up.  Images inserted before any module is known get theirs at that point.

Memory: K = 2048 costs 2048 * (8 + 256 * 2 + 256) B = 1.6 MB per image with fp16 descriptors (hloc's feature files are fp16 already),
2.6 MB with fp32.
"""
import weakref

import torch

from .. import ops
from .._lib import GimHipError
from ..bank import SlotBank, SlotTable  # noqa: F401  (SlotTable: named from here by earlier callers)

_STORAGE = {"fp16": torch.float16, "fp32": torch.float32}


class KeypointBank(SlotBank):
    def __init__(self, capacity_images, num_keypoints, storage="fp16", device="cuda"):
        if storage not in _STORAGE:
            raise ValueError(f"storage must be 'fp16' or 'fp32', got {storage!r}")
        if num_keypoints < 1:
            raise ValueError("a keypoint bank needs at least one keypoint per image")
        super().__init__(capacity_images, "keypoint bank")
        self.num_keypoints, self.storage = int(num_keypoints), storage
        self.device = self.resolve_device(device)
        S, K = self.capacity, self.num_keypoints
        self.kpts = torch.empty(S, K, 2, dtype=torch.float32, device=self.device)
        self.desc = torch.empty(S, K, 256, dtype=_STORAGE[storage], device=self.device)
        self.enc = torch.empty(S, K, 64, dtype=torch.float32, device=self.device)
        self.size_wh = torch.ones(S, 2, dtype=torch.float32, device=self.device)   # (w, h) per slot, as gim_lg_posenc takes it
        self.counts = [0] * S                                                      # keypoints per slot (host) ...
        self.n = torch.zeros(S, dtype=torch.int32, device=self.device)             # ... and on the device
        self._owner, self._epoch, self._wr = None, None, None    # the LightGlue module / packing epoch / Wr the encodings belong to
        self._stale = set()                                      # resident slots whose encoding is not of that module

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.kpts, self.desc, self.enc))

    def slot_tensor(self, idx):
        """int32 device tensor of slot indices from a tensor or a sequence of ints (range-checked where that needs no read-back; the
        kernel never uses an out-of-range index as an address)"""
        if torch.is_tensor(idx):
            if idx.dtype != torch.int32 or idx.device != self.device:
                raise GimHipError(f"slot indices must be int32 on {self.device}, got {idx.dtype} on {idx.device}")
            return idx.reshape(-1).contiguous()
        return torch.tensor(self.check_slots(idx), dtype=torch.int32, device=self.device)

    # ---- device work --------------------------------------------------------------------------------------------------------------
    def slot_counts(self, slots):
        """keypoints of the images in `slots` (host ints)"""
        return [self.counts[s] for s in slots]

    def _admit(self, keys, counts):
        """the host half of an insertion: an image above the capacity is refused before anything changes (no slot taken, no launch),
        then the slots are reserved and the counts recorded"""
        keys, counts = list(keys), [int(c) for c in counts]
        for k, c in zip(keys, counts):
            if not 0 <= c <= self.num_keypoints:
                raise GimHipError(f"image {k!r} has {c} keypoints, a slot of this keypoint bank holds {self.num_keypoints}: build the "
                                  "bank with a larger num_keypoints or cap the detector")
        slots = self.reserve(keys)
        for s_, c in zip(slots, counts):
            self.counts[s_] = c
        return slots

    def put(self, key, keypoints, descriptors, image_size):
        """one image: keypoints [n, 2], descriptors [n, 256] for any 0 <= n <= num_keypoints, image_size [2] -- what `LightGlue.forward`
        takes as keypoints0, descriptors0 and image_size0 (hloc's (w, h); the matcher flips whichever it gets, lightglue.py:414-415)
        without the batch axis"""
        sz = torch.as_tensor(image_size)
        return self.put_many([key], [keypoints.reshape(-1, 2)], [descriptors.reshape(-1, 256)], sz.reshape(1, 2))[0]

    def put_many(self, keys, keypoints, descriptors, image_size):
        """n images in one launch: keypoints [n, k, 2], descriptors [n, k, 256] (one count k <= num_keypoints for all of them), or two
        lists of n tensors [k_i, 2] / [k_i, 256] with a count per image; image_size [n, 2].  Returns their slots."""
        keys = list(keys)
        n, K = len(keys), self.num_keypoints
        kps = list(keypoints) if not torch.is_tensor(keypoints) else list(keypoints.unbind(0)) if keypoints.dim() == 3 else None
        des = list(descriptors) if not torch.is_tensor(descriptors) else list(descriptors.unbind(0)) if descriptors.dim() == 3 else None
        ok = kps is not None and des is not None and len(kps) == n and len(des) == n and tuple(image_size.shape) == (n, 2)
        ok = ok and all(k.dim() == 2 and k.shape[1] == 2 and d.dim() == 2 and d.shape == (k.shape[0], 256) for k, d in zip(kps, des))
        if not ok:
            raise GimHipError(f"keypoint bank of up to {K} keypoints per image: got keypoints "
                              f"{tuple(keypoints.shape) if torch.is_tensor(keypoints) else [tuple(k.shape) for k in keypoints]}, descriptors "
                              f"{tuple(descriptors.shape) if torch.is_tensor(descriptors) else [tuple(d.shape) for d in descriptors]}, "
                              f"image_size {tuple(image_size.shape)} for {n} images (per image: keypoints [k, 2], descriptors [k, 256])")
        counts = [int(k.shape[0]) for k in kps]
        if not all(k.is_cuda and d.is_cuda for k, d in zip(kps, des)):
            raise GimHipError("the keypoint bank needs its keypoints and descriptors as device (cuda/HIP) tensors: there is no CPU fallback")
        slots = self._admit(keys, counts)
        dev = self.device
        if torch.is_tensor(keypoints) and torch.is_tensor(descriptors) and counts[0] == K:
            kp = keypoints.to(dev).float().contiguous()
            de = descriptors.to(dev).float().contiguous()
        else:   # rows [k_i, K) of a slot are written as zeros: whatever an evicted image left there is gone
            kp = torch.zeros(n, K, 2, dtype=torch.float32, device=dev)
            de = torch.zeros(n, K, 256, dtype=torch.float32, device=dev)
            for i, (k, d) in enumerate(zip(kps, des)):
                kp[i, :counts[i]] = k
                de[i, :counts[i]] = d
        sz = image_size[:, [1, 0]].to(device=dev, dtype=torch.float32).contiguous()   # the flip and cast of LightGlue.forward
        st = torch.tensor(slots, dtype=torch.int32, device=dev)
        self.size_wh[st.long()] = sz
        self.n[st.long()] = torch.tensor(counts, dtype=torch.int32, device=dev)
        ops.lg_bank_put(kp, de, sz, self._wr, st, self.kpts, self.desc, self.enc)
        if self._wr is None:
            self._stale.update(slots)
        else:
            self._stale.difference_update(slots)
        return slots

    def bind(self, model):
        """make `model` (a gim_amd.lightglue.LightGlue) the owner of the encodings: later insertions compute theirs in the same launch"""
        self.ensure_encodings(model, model._packed_for(self.device)[2])

    def ensure_encodings(self, model, wr):
        """the encodings of every resident image are those of `model` in its current packing epoch (`wr`: its packed posenc.Wr)"""
        owner = self._owner() if self._owner is not None else None
        if owner is not model or self._epoch != model._pack_epoch:
            self._owner, self._epoch, self._wr = weakref.ref(model), model._pack_epoch, wr
            self._stale = {self.table.slot_of(k) for k in self.table.keys()}
        if self._stale:
            slots = sorted(self._stale)
            st = torch.tensor(slots, dtype=torch.int32, device=self.device)
            ops.lg_bank_put(self.kpts[st.long()].contiguous(), None, self.size_wh[st.long()].contiguous(), self._wr, st, None, self.desc,
                            self.enc)
            self._stale.clear()
