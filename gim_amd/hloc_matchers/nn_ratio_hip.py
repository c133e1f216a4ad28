"""hloc matcher plugin `nn_ratio_hip`: mutual nearest neighbour + Lowe's ratio test on local descriptors (the job of hloc's
`nearest_neighbor` matcher with `do_mutual_check` and `ratio_threshold`) on the fused HIP sweep of gim_amd/csrc/nn_match.hip.

    model({'descriptors0': [1, D, N0], 'descriptors1': [1, D, N1]}) -> {'matches0': [1, N0] int64 (-1 = no match),
                                                                         'matching_scores0': [1, N0] fp32}
which is what hloc/match_features.py:150-160 stores (`gim_amd.hloc_formats.write_sparse_matches`).  The descriptors are used as they
come (SuperPoint's are unit-norm, D = 256); the conf key `root_sift` is an extension of this plugin (hloc's matcher has none): `True` applies the RootSIFT normalisation of trainer/lightning.py:215 to raw SIFT
descriptors first.  The score of a match is its similarity `(1 + sim) / 2`, as hloc's matcher reports it; unmatched rows score 0.
`do_mutual_check` is always on: the kernel decides mutuality in the same sweep, so `False` is refused.  There is no CPU fallback.

    model.match_pairs_from_features(features, pairs, matches)
the fast path for a pair list (as gim_lightglue_hip's): every image named by `pairs` is read from `features` ONCE into a
gim_amd.nn_match.DescriptorBank (normalised there once when `root_sift`), the pairs are matched `batch_pairs` at a time by slot index
and written to `matches` in hloc's layout -- the datasets the per-pair loop writes.  `features`: name -> group with a `descriptors`
dataset, [D, N] as hloc stores it or [N, D] (told apart by the `keypoints` dataset's N where the group has one, else read as [D, N]);
`matches`: anything with h5py's group protocol.  `pairs` is matched as given.
"""
import numpy as np
import torch

from .. import ops
from ..nn_match import DescriptorBank, match_descriptor_pair_list
from .base import BaseModel


class NnRatioHip(BaseModel):
    default_conf = {
        "ratio_threshold": 0.8,     # None or <= 0: no ratio test
        "do_mutual_check": True,
        "root_sift": False,         # extension: RootSIFT-normalise raw SIFT descriptors first
        "batch_pairs": 32,          # pairs per launch sequence of match_pairs_from_features
    }
    required_inputs = ["descriptors0", "descriptors1"]

    def _init(self, conf):
        if not conf["do_mutual_check"]:
            raise NotImplementedError("nn_ratio_hip: do_mutual_check=False is not implemented (the kernel tests mutuality in its one sweep)")
        self.ratio = float(conf["ratio_threshold"] or 0.0)

    @torch.no_grad()
    def _forward(self, data):
        d0, d1 = data["descriptors0"], data["descriptors1"]
        assert d0.dim() == 3 and d0.shape[0] == 1 and d1.shape[0] == 1, "nn_ratio_hip matches one pair per call: descriptors [1, D, N]"
        match0, score0 = ops.nn_match(d0[0].t().float().contiguous(), d1[0].t().float().contiguous(), rootsift=self.conf["root_sift"],
                                      ratio=self.ratio)
        hit = match0 >= 0
        scores = torch.where(hit, (score0 + 1) / 2, torch.zeros_like(score0))
        return {"matches0": match0.long()[None], "matching_scores0": scores[None]}

    @staticmethod
    def _rows(group):
        """(keypoints [N, 2] or None, descriptors [N, D]) of one feature group"""
        desc = np.asarray(group["descriptors"])
        if desc.ndim != 2:
            raise ValueError(f"nn_ratio_hip: descriptors of shape {desc.shape}; [D, N] or [N, D] expected")
        kpts = np.asarray(group["keypoints"]) if "keypoints" in group else None
        rows_first = kpts is not None and desc.shape[0] == kpts.shape[0] and desc.shape[1] != kpts.shape[0]
        return kpts, desc if rows_first else desc.T

    @torch.no_grad()
    def match_pairs_from_features(self, features, pairs, matches, device=None):
        pairs = [(a, b) for a, b in pairs]
        names = list(dict.fromkeys(n for p in pairs for n in p))
        if not names:
            return []
        dev = torch.device(device) if device is not None else torch.device("cuda")
        images = {n: self._rows(features[n]) for n in names}                # every image is read once
        D = images[names[0]][1].shape[1]
        bank = DescriptorBank(len(names), max(1, max(d.shape[0] for _, d in images.values())), D=D, rootsift=self.conf["root_sift"],
                              device=dev)
        for n in names:
            kpts, desc = images[n]
            kpts = np.zeros((desc.shape[0], 2), dtype=np.float32) if kpts is None else kpts[:, :2]
            bank.put(n, torch.from_numpy(np.ascontiguousarray(kpts, dtype=np.float32)).to(dev),
                     torch.from_numpy(np.ascontiguousarray(desc, dtype=np.float32)).to(dev))
        self.bank = bank                                                    # kept for its stats
        return match_descriptor_pair_list(bank, pairs, batch_pairs=int(self.conf["batch_pairs"]), ratio=self.ratio, writer=matches)
