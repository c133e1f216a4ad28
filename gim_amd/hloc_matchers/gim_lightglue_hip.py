"""hloc matcher plugin `gim_lightglue_hip`: the matcher half of reconstruction.py's `--version gim_lightglue` (LightGlue with
`filter_threshold=0.1` over SuperPoint features, hloc/match_features.py:24-35, 124-160, 244-255) on the HIP engine.

Two ways in:

  model(data)   hloc's own loop, unchanged: the batch-1 dict of `FeaturePairsDataset` (match_features.py:124-147) -- keypoints0/1
                [1, K, 2], descriptors0/1 [1, K, 256], image_size0/1 [1, 2], all floats that were fp16 in the feature file, and the
                image0/1 placeholders nobody reads -- -> {'matches0' [1, K] int64, 'matching_scores0' [1, K] fp32, ...}, which hloc's
                writer stores as int16 / fp16 (:150-160).  One pair per ~200 launches: correct, and bound by launch overhead.

  model.match_pairs_from_features(features, pairs, matches)
                the fast path for a pair list: every image named by `pairs` is read from `features` ONCE into a
                gim_amd.lightglue.KeypointBank, the pairs are matched `batch_pairs` at a time by slot index
                (gim_amd.lightglue.match_pair_list) and written to `matches` in hloc's layout.  `features`: name -> group with
                `keypoints`, `descriptors`, `image_size` datasets (an open h5py.File of extract_features.py, or a dict of dicts of
                arrays); `matches`: anything with h5py's group protocol.  `pairs` is matched as given: apply hloc's
                find_unique_new_pairs first if (j, i) is to be dropped where (i, j) is listed.  The images may hold different numbers
                of keypoints (a detection threshold, force_num_keypoints=False, small images, another 256-d extractor): a slot of
                the bank holds the largest count named, or `max_keypoints` if that is set -- an image above it is refused before
                anything is launched -- and every pair's datasets have the length of image 0's keypoints, as hloc's have.

conf: `weights` (file under weights/, the reference's 'gim_lightglue_100h.ckpt': the `model.` half is loaded, reconstruction.py:116-123;
None keeps the module's init), `filter_threshold`, `precision`, `batch_pairs`, `storage` ('fp16' = the feature file's own precision, or
'fp32'), `max_keypoints` (None, or the capacity of a bank slot).  No CPU fallback.
"""
import os
from os.path import join

import numpy as np
import torch

from .._lib import GimHipError
from ..lightglue import KeypointBank, LightGlue, match_pair_list
from .base import BaseModel


def _rows256(desc):
    """descriptors as [..., K, 256]: the gim detector stores [K, 256], hloc's own SuperPoint wrapper [256, K]"""
    if desc.shape[-1] != 256 and desc.shape[-2] == 256:
        desc = desc.transpose(-1, -2)
    return desc


class GimLightGlueHip(BaseModel):
    default_conf = {
        "weights": None,
        "filter_threshold": 0.1,
        "precision": None,
        "batch_pairs": 8,
        "storage": "fp16",
        "max_keypoints": None,
    }
    required_inputs = ["keypoints0", "keypoints1", "descriptors0", "descriptors1", "image_size0", "image_size1"]

    def _init(self, conf):
        kw = {"precision": conf["precision"]} if conf.get("precision") else {}
        net = LightGlue({"filter_threshold": conf["filter_threshold"], "flash": False, "checkpointed": True, **kw})
        if conf.get("weights"):
            path = conf["weights"] if os.path.isabs(conf["weights"]) else join("weights", conf["weights"])
            sd = torch.load(path, map_location="cpu")
            sd = sd["state_dict"] if "state_dict" in sd else sd
            net.load_state_dict({k.replace("model.", "", 1): v for k, v in sd.items() if k.startswith("model.")} or
                                {k: v for k, v in sd.items() if not k.startswith("superpoint.")})
        self.net = net

    @torch.no_grad()
    def _forward(self, data):
        d = {k: data[k] for k in ("keypoints0", "keypoints1", "image_size0", "image_size1")}
        d["descriptors0"], d["descriptors1"] = _rows256(data["descriptors0"]), _rows256(data["descriptors1"])
        return self.net(d)

    @torch.no_grad()
    def match_pairs_from_features(self, features, pairs, matches, device=None):
        pairs = [(a, b) for a, b in pairs]
        names = list(dict.fromkeys(n for p in pairs for n in p))
        if not names:
            return []
        dev = torch.device(device) if device is not None else next(self.net.parameters()).device
        counts = {n: int(np.shape(features[n]["keypoints"])[0]) for n in names}
        cap = self.conf.get("max_keypoints")
        cap = max(max(counts.values()), 1) if cap is None else int(cap)
        over = [n for n in names if counts[n] > cap]
        if over:
            raise GimHipError(f"image {over[0]!r} has {counts[over[0]]} keypoints, max_keypoints is {cap}"
                              + (f"; {len(over) - 1} more" if len(over) > 1 else ""))
        bank = KeypointBank(len(names), cap, storage=self.conf["storage"], device=dev)
        bank.bind(self.net)
        for n in names:
            g = features[n]
            kp = torch.from_numpy(np.asarray(g["keypoints"])).float().reshape(-1, 2)
            de = _rows256(torch.from_numpy(np.asarray(g["descriptors"])).float()).reshape(-1, 256)
            bank.put(n, kp.to(dev), de.to(dev), torch.from_numpy(np.asarray(g["image_size"])).float())
        return match_pair_list(self.net, bank, pairs, batch_pairs=int(self.conf["batch_pairs"]), writer=matches)
