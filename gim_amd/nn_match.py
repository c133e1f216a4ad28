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
elsewhere.  One pair per launch; batching several pairs per launch is the obvious follow-up if the video labeller wants it.
"""
import numpy as np
import torch

from . import ops
from ._lib import GimHipError

NO_DETECTOR = ("root_sift needs OpenCV's SIFT detector (cv2.SIFT_create) to find keypoints, and cv2 does not import here: {}. "
               "Install opencv-python, or call RootSiftMatcher.match_descriptors with descriptors of your own.")


def _cv2():
    try:
        import cv2
        cv2.SIFT_create  # noqa: B018  (opencv < 4.4 without contrib has no SIFT)
    except Exception as e:  # noqa: BLE001
        raise GimHipError(NO_DETECTOR.format(f"{type(e).__name__}: {e}")) from e
    return cv2


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
