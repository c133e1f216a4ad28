"""Keypoint bank for pair lists: every image of an exhaustive hloc pairing runs SuperPoint ONCE and is uploaded ONCE, however many pairs
name it -- the sparse counterpart of gim_amd/loftr/bank.py (gim_amd/bank.py `SlotBank` does the bookkeeping of both kinds of bank).

  KeypointBank   `capacity_images` slots of `num_keypoints` keypoints on the device (csrc/lg_bank.hip for the layout):
                     kpts [S, K, 2] fp32, desc [S, K, 256] fp32 | fp16 (`storage`), enc [S, K, 64] fp32
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
    def put(self, key, keypoints, descriptors, image_size):
        """one image: keypoints [K, 2], descriptors [K, 256], image_size [2] -- what `LightGlue.forward` takes as keypoints0,
        descriptors0 and image_size0 (hloc's (w, h); the matcher flips whichever it gets, lightglue.py:414-415) without the batch axis"""
        sz = torch.as_tensor(image_size)
        return self.put_many([key], keypoints.reshape(1, *keypoints.shape[-2:]), descriptors.reshape(1, *descriptors.shape[-2:]),
                             sz.reshape(1, 2))[0]

    def put_many(self, keys, keypoints, descriptors, image_size):
        """n images in one launch: keypoints [n, K, 2], descriptors [n, K, 256], image_size [n, 2].  Returns their slots."""
        keys = list(keys)
        n, K = len(keys), self.num_keypoints
        if tuple(keypoints.shape) != (n, K, 2) or tuple(descriptors.shape) != (n, K, 256) or tuple(image_size.shape) != (n, 2):
            raise GimHipError(f"keypoint bank of {K} keypoints per image: got keypoints {tuple(keypoints.shape)}, descriptors "
                              f"{tuple(descriptors.shape)}, image_size {tuple(image_size.shape)} for {n} images (ragged counts are not built: "
                              "run the detector with force_num_keypoints)")
        if not keypoints.is_cuda or not descriptors.is_cuda:
            raise GimHipError("the keypoint bank needs device (cuda/HIP) tensors: there is no CPU fallback")
        slots = self.reserve(keys)
        dev = self.device
        kp = keypoints.to(dev).float().contiguous()
        de = descriptors.to(dev).float().contiguous()
        sz = image_size[:, [1, 0]].to(device=dev, dtype=torch.float32).contiguous()   # the flip and cast of LightGlue.forward
        st = torch.tensor(slots, dtype=torch.int32, device=dev)
        self.size_wh[st.long()] = sz
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
