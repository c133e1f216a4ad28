"""hloc extractor plugin `gim_superpoint_hip`: the detector half of reconstruction.py's `--version gim_lightglue` (SuperPoint with 2048
forced keypoints, nms_radius 3, detection_threshold 0; reconstruction.py:95-109, hloc/extract_features.py:29-40, 272-299) on the HIP
engine.

    model({'image': [1, 1|3, H, W]}) -> {'keypoints': [1, K, 2], 'descriptors': [1, K, 256], 'keypoint_scores': [1, K]}
the three datasets hloc stores per image next to `image_size` (extract_features.py:275-299).

H and W must be multiples of 8 (the engine's SuperPoint has no partial 8x8 cell): another size raises a GimHipError naming it, before
any device work.  hloc's `resize_max` preprocessing gives arbitrary sizes -- resize or crop to a multiple of 8 in the loader
(INTEGRATION.md); arbitrary sizes are a separate piece of work.

conf: `max_keypoints`, `nms_radius`, `weights` (file under weights/, the reference's 'gim_lightglue_100h.ckpt': the `superpoint.` half
is loaded, reconstruction.py:102-109; None keeps the module's init), `precision`.  No CPU fallback.
"""
import os
from os.path import join

import torch

from .._lib import GimHipError
from ..hloc_matchers.base import BaseModel
from ..lightglue import SuperPoint


class GimSuperPointHip(BaseModel):
    default_conf = {
        "max_keypoints": 2048,
        "nms_radius": 3,
        "weights": None,
        "precision": None,
    }
    required_inputs = ["image"]

    def _init(self, conf):
        kw = {"precision": conf["precision"]} if conf.get("precision") else {}
        net = SuperPoint({"max_num_keypoints": int(conf["max_keypoints"]), "force_num_keypoints": True, "detection_threshold": 0.0,
                          "nms_radius": int(conf["nms_radius"]), "trainable": False, **kw})
        if conf.get("weights"):
            path = conf["weights"] if os.path.isabs(conf["weights"]) else join("weights", conf["weights"])
            sd = torch.load(path, map_location="cpu")
            sd = sd["state_dict"] if "state_dict" in sd else sd
            net.load_state_dict({k.replace("superpoint.", "", 1): v for k, v in sd.items() if k.startswith("superpoint.")} or
                                {k: v for k, v in sd.items() if not k.startswith("model.")})
        self.net = net.eval()

    @torch.no_grad()
    def _forward(self, data):
        image = data["image"]
        H, W = image.shape[-2:]
        if H % 8 or W % 8:
            raise GimHipError(f"gim_superpoint_hip: image size {W}x{H} (w x h) is not a multiple of 8 in both directions; resize or crop the "
                              "image in the loader (arbitrary sizes are not built)")
        out = self.net({"image": image})
        return {k: out[k] for k in ("keypoints", "descriptors", "keypoint_scores")}
