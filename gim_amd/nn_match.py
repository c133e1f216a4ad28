"""`root_sift`, the fifth entry of the reference's model zoo (test.py:61) and the baseline row of the ZEB table: SIFT keypoints on
the host (OpenCV, as in the reference), RootSIFT normalisation + mutual nearest neighbour + Lowe's ratio test on the device in one
fused sweep (gim_amd/csrc/nn_match.hip) that never stores the n0 x n1 similarity matrix.

Restates (reference file:line):
  * `RootSiftMatcher.inference`           trainer/lightning.py:195-241 `root_sift_inference` (= video_preprocessor.py:357-404)
  * `RootSiftMatcher.match_descriptors`   :214-241 of it: everything behind cv2's detectAndCompute

    m = RootSiftMatcher()
    m(batch)                        # ZEB batch dict (color0, color1, image0, image1, scale0, scale1): adds mkpts0_f, mkpts1_f, m_bids, mconf
    zeb.run_scene(m, batches, out)  # the baseline's dump

The matching has no CPU fallback.  The detector is OpenCV's and is imported when `inference` first needs it: where cv2 does not
import, `inference` raises GimHipError before anything touches the device and `match_descriptors` still works on descriptors from
elsewhere.

Pair lists (an exhaustive SfM pairing, the video labeller's neighbouring frames): the descriptors of every image are normalised ONCE into
a `DescriptorBank` and stay on the device; the pairs are matched by slot index, many per launch sequence (gim_nn_match_pairs), with one
host read per batch.  Every pair gets the bits the single-pair call gives it.

    bank = DescriptorBank(capacity_images=32, max_rows=4800)
    bank.put(name, kpts, desc)                                        # once per image
    m.match_pairs(bank, bank.slots(keys0), bank.slots(keys1))         # the batched dict; m_bids = index of the pair
    match_descriptor_pair_list(bank, pairs, batch_pairs=32, writer=h5)  # hloc's matches0 int16 / matching_scores0 fp16 per pair
"""
import numpy as np
import torch

from . import ops
from ._lib import GimHipError
from .bank import SlotBank, sparse_pair_list

NO_DETECTOR = ("root_sift needs OpenCV's SIFT detector (cv2.SIFT_create) to find keypoints, and cv2 does not import here: {}. "
               "Install opencv-python, or call RootSiftMatcher.match_descriptors with descriptors of your own.")


def _cv2():
    try:
        import cv2
        cv2.SIFT_create  # noqa: B018  (opencv < 4.4 without contrib has no SIFT)
    except Exception as e:  # noqa: BLE001
        raise GimHipError(NO_DETECTOR.format(f"{type(e).__name__}: {e}")) from e
    return cv2


class DescriptorBank(SlotBank):
    """`capacity_images` slots of at most `max_rows` descriptors of width D on the device (csrc/nn_match.hip for the layout):
        desc [S, R, D] fp32 (RootSIFT-normalised at insertion when `rootsift`), kpts [S, R, 2] fp32, n [S] int32
    plus caller-supplied hashable image key -> slot with LRU eviction (gim_amd/bank.py `SlotBank`, as the keypoint bank of
    gim_lightglue).  `counts` is the host mirror of n: sizing a batch never reads the device."""

    def __init__(self, capacity_images, max_rows, D=128, rootsift=True, device="cuda"):
        if max_rows < 1:
            raise ValueError("a descriptor bank needs at least one row per image")
        super().__init__(capacity_images, "descriptor bank")
        if D % 16 or not 16 <= D <= 256:
            raise GimHipError(f"descriptor bank: D={D} is not a multiple of 16 in [16, 256]")
        self.max_rows, self.D, self.rootsift = int(max_rows), int(D), bool(rootsift)
        self.device = self.resolve_device(device)
        S, R = self.capacity, self.max_rows
        self.desc = torch.empty(S, R, self.D, dtype=torch.float32, device=self.device)
        self.kpts = torch.zeros(S, R, 2, dtype=torch.float32, device=self.device)
        self.n = torch.zeros(S, dtype=torch.int32, device=self.device)
        self.counts = np.zeros(S, dtype=np.int32)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.desc, self.kpts, self.n))

    # ---- device work --------------------------------------------------------------------------------------------------------------
    def put(self, key, kpts, desc):
        """one image: kpts [n, 2] pixels, desc [n, D] raw descriptors (device tensors; n == 0: an image without keypoints).  A
        resident key keeps its slot and is overwritten; otherwise the least recently used image makes room.  Returns the slot."""
        if desc.dim() != 2 or desc.shape[1] != self.D:
            raise GimHipError(f"descriptor bank of width {self.D}: got descriptors {tuple(desc.shape)} for image {key!r}")
        n = desc.shape[0]
        if n > self.max_rows:
            raise GimHipError(f"descriptor bank: image {key!r} has {n} descriptors, a slot holds max_rows={self.max_rows}")
        if tuple(kpts.shape) != (n, 2):
            raise GimHipError(f"descriptor bank: keypoints {tuple(kpts.shape)} for {n} descriptors of image {key!r}")
        slot = self.reserve([key])[0]
        ops.nn_bank_put(desc.to(self.device).float(), slot, self.desc, self.n, rootsift=self.rootsift)
        if n:
            self.kpts[slot, :n] = kpts.to(self.device).float()
        self.counts[slot] = n
        return slot


def _pair_scale(scale, P, bids, dev):
    """scale [2] | [1, 2] (every pair) or [P, 2] / a sequence of P of them (per pair) -> the factor of every matched row"""
    if not torch.is_tensor(scale):
        scale = torch.stack([torch.as_tensor(x, dtype=torch.float32).reshape(2) for x in scale]) if len(scale) == P and P and \
            not isinstance(scale[0], (int, float)) else torch.as_tensor(scale, dtype=torch.float32)
    scale = scale.to(device=dev, dtype=torch.float32).reshape(-1, 2)
    if scale.shape[0] == 1:
        return scale
    if scale.shape[0] != P:
        raise GimHipError(f"match_pairs: {scale.shape[0]} scales for {P} pairs")
    return scale[bids]


class RootSiftMatcher:
    """`root_sift_inference` on the HIP engine.  ratio: Lowe's threshold (0.8 at both reference call sites)."""

    def __init__(self, ratio=0.8, device="cuda"):
        self.ratio, self.device = ratio, device

    def __call__(self, data):
        return self.inference(data)

    def eval(self):
        return self

    def to(self, device):
        self.device = device
        return self

    @torch.no_grad()
    def match_descriptors(self, kpts0, desc0, kpts1, desc1, scale0=None, scale1=None):
        """kpts [n,2] pixels, desc [n,D] raw (un-normalised, non-negative) descriptors, device tensors; scale [2] or [1,2] as the ZEB
        loaders give it.  -> {mkpts0_f [M,2], mkpts1_f [M,2], m_bids [M] int64 zeros, mconf [M]}: lightning.py:214-241, rows in
        ascending desc0 order like `kpts0[valid]`.  The gather runs on the device; the one host read is the match count."""
        desc0, desc1 = desc0.float(), desc1.float()
        count = torch.zeros(1, dtype=torch.int32, device=desc0.device)
        match0, score0 = ops.nn_match(desc0, desc1, rootsift=True, ratio=self.ratio, count=count)
        M = int(count[0])                                                   # the read-back, as coarse_match reads its match count
        rows = torch.nonzero_static(match0 >= 0, size=M)[:, 0]              # the size is known: no second synchronisation
        cols = match0[rows].long()
        mk0, mk1 = kpts0.float()[rows], kpts1.float()[cols]
        if scale0 is not None:
            mk0 = mk0 * torch.as_tensor(scale0, dtype=mk0.dtype, device=mk0.device).reshape(-1, 2)
        if scale1 is not None:
            mk1 = mk1 * torch.as_tensor(scale1, dtype=mk1.dtype, device=mk1.device).reshape(-1, 2)
        return {"mkpts0_f": mk0, "mkpts1_f": mk1, "m_bids": torch.zeros(rows.shape[0], dtype=torch.int64, device=desc0.device),
                "mconf": score0[rows]}

    @torch.no_grad()
    def match_pairs(self, bank, slots0, slots1, scale0=None, scale1=None):
        """P pairs (slots0[p], slots1[p]) of a `DescriptorBank` in one launch sequence -> the matchers' batched dict {mkpts0_f [M,2],
        mkpts1_f [M,2], m_bids [M] int64 = index of the pair, mconf [M]}, rows ordered by pair, then by ascending desc0 row; restricted
        to m_bids == p it is what `match_descriptors` returns for that pair.  scale: [2] | [1,2] for all pairs or [P,2] per pair.
        The one host read is the P match counts."""
        s0, s1 = bank.check_slots(slots0), bank.check_slots(slots1)
        dev = bank.device
        r = ops.nn_match_pairs(bank.desc, bank.n, bank.counts, s0, s1, ratio=self.ratio)
        P = len(s0)
        counts = r.count.cpu()                                              # the read-back of the batch
        M = int(counts.sum())
        rows = torch.nonzero_static(r.match0 >= 0, size=M)[:, 0]            # ragged row of every match, ascending: pair, then row
        bids = torch.repeat_interleave(torch.arange(P, device=dev), counts.to(dev, torch.int64), output_size=M)
        tab = torch.from_numpy(np.stack([np.asarray(s0, dtype=np.int64), np.asarray(s1, dtype=np.int64),
                                         r.row_off[:P].astype(np.int64)]).reshape(3, P)).to(dev)
        mk0 = bank.kpts[tab[0][bids], rows - tab[2][bids]]
        mk1 = bank.kpts[tab[1][bids], r.match0[rows].long()]
        if scale0 is not None:
            mk0 = mk0 * _pair_scale(scale0, P, bids, dev)
        if scale1 is not None:
            mk1 = mk1 * _pair_scale(scale1, P, bids, dev)
        return {"mkpts0_f": mk0, "mkpts1_f": mk1, "m_bids": bids, "mconf": r.score0[rows]}

    def detect(self, color):
        """lightning.py:197-212 for one image [1,3,H,W] in [0,1] -> (kpts [n,2] float64, desc [n,128] float32) numpy, on the host"""
        cv2 = _cv2()
        image = color.squeeze().permute(1, 2, 0).cpu().numpy() * 255
        image = cv2.cvtColor(image.astype(np.uint8), cv2.COLOR_RGB2BGR)
        H, W = image.shape[:2]
        sift = cv2.SIFT_create(nfeatures=H * W // 64, contrastThreshold=1e-5)
        kpts, desc = sift.detectAndCompute(image, None)
        kpts = np.array([[kp.pt[0], kp.pt[1]] for kp in kpts]).reshape(-1, 2)
        desc = np.zeros((0, 128), dtype=np.float32) if desc is None else desc
        return kpts, desc

    @torch.no_grad()
    def inference(self, data):
        """lightning.py:195-241 on a ZEB batch dict of ONE pair; mutates it like the other matchers."""
        _cv2()                                                              # fail before any device work
        k0, d0 = self.detect(data["color0"])
        k1, d1 = self.detect(data["color1"])
        dev = data["color0"].device if data["color0"].is_cuda else torch.device(self.device)
        k0, d0, k1, d1 = (torch.from_numpy(np.ascontiguousarray(x)).to(dev).float() for x in (k0, d0, k1, d1))
        out = self.match_descriptors(k0, d0, k1, d1, data.get("scale0"), data.get("scale1"))
        data.update({"hw0_i": data["image0"].shape[2:], "hw1_i": data["image1"].shape[2:], **out})
        return data


@torch.no_grad()
def match_descriptor_pair_list(bank, pairs, batch_pairs=32, ratio=0.8, writer=None, names=None):
    """pairs: a sequence of (key0, key1) of images resident in `bank`, matched as given, in the order given, `batch_pairs` per launch
    sequence (gim_amd.lightglue.match_pair_list for the sparse learned matcher).  Returns [(key0, key1, matches0 int16 [n0],
    matching_scores0 fp16 [n0])] as numpy arrays -- hloc's datasets, which leave the device in that format, one copy per batch; with
    `writer` (h5py's group protocol) every pair is also written through hloc_formats.write_sparse_matches (group name from names[key] if
    `names` is given, else str(key))."""
    def match_batch(s0, s1):
        r = ops.nn_match_pairs(bank.desc, bank.n, bank.counts, s0, s1, ratio=ratio, hloc=True)
        m, s = r.matches0_i16.cpu().numpy(), r.matching_scores0_f16.cpu().numpy()
        return [(m[lo:hi], s[lo:hi]) for lo, hi in zip(r.row_off[:-1].tolist(), r.row_off[1:].tolist())]
    return sparse_pair_list(bank, pairs, batch_pairs, match_batch, writer, names)
