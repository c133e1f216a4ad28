"""hloc matcher plugin `nn_ratio_hip`: mutual nearest neighbour + Lowe's ratio test on local descriptors (the job of hloc's
`nearest_neighbor` matcher with `do_mutual_check` and `ratio_threshold`) on the fused HIP sweep of gim_amd/csrc/nn_match.hip.

    model({'descriptors0': [1, D, N0], 'descriptors1': [1, D, N1]}) -> {'matches0': [1, N0] int64 (-1 = no match),
                                                                         'matching_scores0': [1, N0] fp32}
which is what hloc/match_features.py:150-160 stores (`gim_amd.hloc_formats.write_sparse_matches`).  The descriptors are used as they
come (SuperPoint's are unit-norm, D = 256); the conf key `root_sift` is an extension of this plugin (hloc's matcher has none): `True` applies the RootSIFT normalisation of trainer/lightning.py:215 to raw SIFT
descriptors first.  The score of a match is its similarity `(1 + sim) / 2`, as hloc's matcher reports it; unmatched rows score 0.
`do_mutual_check` is always on: the kernel decides mutuality in the same sweep, so `False` is refused.  There is no CPU fallback.
"""
import torch

from .. import ops
from .base import BaseModel


class NnRatioHip(BaseModel):
    default_conf = {
        "ratio_threshold": 0.8,     # None or <= 0: no ratio test
        "do_mutual_check": True,
        "root_sift": False,         # extension: RootSIFT-normalise raw SIFT descriptors first
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
