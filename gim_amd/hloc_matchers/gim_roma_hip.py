"""hloc dense-matcher plugin `gim_roma_hip`: the surface of `gim_dkm_hip` (the reference's `hloc/matchers/dkm.py` contract: image0 /
image1 swapped, segment-mask blackout, padding, 8192 samples, top-k) over `gim_amd.roma.RoMa` -- the reference has no hloc plugin for
gim_roma; the conf and the data contract are the dkm plugin's, the padding target is RoMa's square 672 x 672 (demo.py:420-462).

    model({'image0', 'image1', 'name0', 'name1'}) -> {'keypoints0', 'keypoints1', 'scores', 'batch_indexes'}

`weights`: a gim_roma checkpoint under `weights/` (`state_dict` unwrapped, `model.` stripped); `dinov2_weights`: the DINOv2 ViT-L/14
state dict file the reference downloads in its constructor (roma.py:596-604).  The pair-list path (`bank_put`, `match_pairs`,
`match_and_assign_from_images(bank_images=...)`) is inherited unchanged.  No CPU fallback.
"""
import os
from os.path import join

import torch

from ..adapters import HlocDenseMatcher
from ..roma import RoMa
from .gim_dkm_hip import GimDkmHip


class GimRomaHip(GimDkmHip):
    default_conf = {
        "weights": None,            # file name under weights/ (reference: 'gim_roma_100h.ckpt'); None = keep the module's init
        "dinov2_weights": None,     # file with the ViT-L/14 state dict (names of dino.py's vit_large)
        "max_num_matches": None,
        "precision": None,          # 'fp16' (default of the engine), 'bf16' or 'fp32'
    }
    required_inputs = ["image0", "image1"]

    def _init(self, conf):
        self.h, self.w = 672, 672
        kw = {"precision": conf["precision"]} if conf.get("precision") else {}
        model = RoMa([self.h, self.w], **kw)
        if conf.get("dinov2_weights"):
            model.load_dinov2(torch.load(conf["dinov2_weights"], map_location="cpu"))
        if conf.get("weights"):
            path = conf["weights"] if os.path.isabs(conf["weights"]) else join("weights", conf["weights"])
            state_dict = torch.load(path, map_location="cpu")
            if "state_dict" in state_dict.keys():
                state_dict = state_dict["state_dict"]
            model.load_state_dict({(k.replace("model.", "", 1) if k.startswith("model.") else k): v for k, v in state_dict.items()})
        self.net = model
        self.adapter = HlocDenseMatcher(model, self.h, self.w, conf["max_num_matches"], 8192)
