"""`demo.py --model {gim_dkm, gim_roma, gim_loftr, gim_lightglue}` of the reference, on the HIP engine, plus `root_sift`, the fifth
entry of its model zoo (test.py:61; trainer/lightning.py:195-241).

    python -m gim_amd.demo --model gim_lightglue [--weights weights/gim_lightglue_100h.ckpt] \
           [--image0 assets/demo/a1.png --image1 assets/demo/a2.png] [--precision bf16|fp32] [--resize-max N]

Mirrors the reference entry point step by step (reference file:line):
  * `read_image`         demo.py:123-137  (PIL instead of OpenCV: RGB order, ITU-R 601 grey)
  * `preprocess`         demo.py:140-178  (optional area down-scale to `resize_max`, /255, size made divisible by 8 with the
                                            bilinear tensor resize torchvision's `F.resize` performs, scale = original / new)
  * `build`              demo.py:324-400  (constructor arguments per model, checkpoint unwrapping and the per-model key-prefix
                                            rules; without a checkpoint the seeded init of the modules is kept -- plumbing runs)
  * `match_pair`         demo.py:405-511  (dense: pad / match / sample 5000 / pixels / un-pad / in-bounds mask; gim_loftr: the
                                            module's dict; gim_lightglue: detector x2 + matcher + per-pair gather)
  * robust fitting       demo.py:514-517  cv2.findFundamentalMat(USAC_MAGSAC, 1.0 px, 0.999999, 10000) stays on the host (north_star);
                                            without OpenCV: seven-point RANSAC of gim_amd/pose.py with the same parameters
  * `compute_geom`       demo.py:180-227  the fundamental matrix of the step above and cv2.findHomography(mkpts1, mkpts0, ...) as
                                            pose.find_homography (four-point solve and scoring fused on the device)
  * `warp_pair`          demo.py:230-266  wrap_images(..., "Homography"): image 0 beside cv2.warpPerspective(image 1, H, size of image
                                            0) as ops.warp_perspective; `--out DIR` writes DIR/<name0>_<name1>_<model>_warp.png
Out of scope: the matplotlib figure and its titles (the PNG is the two images side by side, nothing drawn on them),
cv2.stereoRectifyUncalibrated (`H1`, `H2`, the "Fundamental" flavour of wrap_images) and the match-line drawing (`_match.png`).
Returns / prints `{mkpts0_f, mkpts1_f, mconf, m_bids}` in pixels of the ORIGINAL images (kpts * scale, demo.py:499-500 and
the `scale0/scale1` the other models get through their own adapters).
"""
import argparse
import os
from os.path import join

import numpy as np
import torch
import torch.nn.functional as F

MODELS = ("gim_dkm", "gim_roma", "gim_loftr", "gim_lightglue", "root_sift")
CKPT = {"gim_dkm": "gim_dkm_100h.ckpt", "gim_roma": "gim_roma_100h.ckpt", "gim_loftr": "gim_loftr_50h.ckpt",
        "gim_lightglue": "gim_lightglue_100h.ckpt"}   # demo.py:328-347


def read_image(path, grayscale=False):
    """demo.py:123-137 -> uint8 [H,W,3] RGB or [H,W] grey"""
    from PIL import Image
    im = Image.open(path)
    return np.asarray(im.convert("L" if grayscale else "RGB"))


def preprocess(image, grayscale=False, resize_max=None, dfactor=8, antialias=False):
    """demo.py:140-178 -> (float tensor [C,H',W'] in [0,1], scale (x, y) = original size / new size).
    Numerics vs the reference when a resize actually happens: (1) the divisible-by-8 resize is torchvision's `F.resize` on a
    TENSOR = bilinear, align_corners=False; the reference pins torchvision 0.13.1 (environment.yaml), whose tensor path does
    NOT antialias (`antialias=None`), hence the default here -- pass `antialias=True` to reproduce a torchvision >= 0.17
    installation, where it became the default; (2) the `resize_max` downscale is cv2 INTER_AREA in the reference: `mode='area'`
    (adaptive average pooling) equals it for integer factors only, non-integer factors differ in the fractional cell weights;
    (3) `read_image` decodes with PIL instead of OpenCV (identical for PNG, +-1 grey level for JPEG)."""
    image = image.astype(np.float32, copy=False)
    size = image.shape[:2][::-1]
    t = torch.from_numpy(image[None] if grayscale else image.transpose(2, 0, 1)).float()
    if resize_max:
        s = resize_max / max(size)
        if s < 1.0:   # resize_image(..., 'cv2_area'): area averaging (= INTER_AREA for integer factors)
            size_new = tuple(int(round(x * s)) for x in size)
            t = F.interpolate(t[None], size=size_new[::-1], mode="area")[0]
    t = t / 255.0
    size_new = tuple(int(x // dfactor * dfactor) for x in t.shape[-2:])
    t = F.interpolate(t[None], size=size_new, mode="bilinear", align_corners=False, antialias=antialias)[0]   # F.resize on a tensor
    scale = np.array(size) / np.array(size_new)[::-1]
    return t, scale


def _load_ckpt(path):
    sd = torch.load(path, map_location="cpu")
    return sd["state_dict"] if "state_dict" in sd.keys() else sd


def build(model_name, weights=None, precision=None, device="cuda", dinov2_weights=None):
    """demo.py:324-400 -> (model, detector or None) on `device`, eval mode"""
    kw = {"precision": precision} if precision else {}
    detector = None
    if model_name == "gim_dkm":
        from .dkm import DKMv3
        model = DKMv3(weights=None, h=672, w=896, **kw)
        if weights:
            sd = _load_ckpt(weights)
            for k in list(sd.keys()):   # demo.py:357-362: strip `model.`, drop the ResNet's unused fc head (under either name)
                v = sd.pop(k)
                nk = k.replace("model.", "", 1) if k.startswith("model.") else k
                if "encoder.net.fc" not in nk:
                    sd[nk] = v
            model.load_state_dict(sd)
    elif model_name == "gim_roma":
        from .roma import RoMa, random_dinov2_weights
        sd = _load_ckpt(weights) if weights else None
        # the reference downloads dinov2_vitl14_pretrain.pth inside the constructor (roma.py:591-595) and hides the ViT from
        # state_dict() (roma.py:612), so the gim checkpoint does not carry it: pass the same file here (no network access in
        # this engine).  Without any checkpoint a seeded synthetic ViT-L/14 stands in (plumbing runs).
        if dinov2_weights is not None:
            dsd = torch.load(dinov2_weights, map_location="cpu") if isinstance(dinov2_weights, str) else dinov2_weights
        elif sd is None:
            dsd = random_dinov2_weights("cpu")
        else:
            raise ValueError("gim_roma with a checkpoint also needs --dinov2-weights dinov2_vitl14_pretrain.pth "
                             "(the reference fetches it from the hub inside RoMa(), roma.py:591-595)")
        model = RoMa(img_size=[672], dinov2_weights=dsd, **kw)
        if sd is not None:
            for k in list(sd.keys()):
                if k.startswith("model."):
                    sd[k.replace("model.", "", 1)] = sd.pop(k)
            model.load_state_dict(sd)
    elif model_name == "gim_loftr":
        from .loftr import LoFTR, get_cfg_defaults, lower_config
        cfg = lower_config(get_cfg_defaults())["loftr"]
        if precision:
            cfg["precision"] = precision
        model = LoFTR(cfg)
        if weights:
            model.load_state_dict(_load_ckpt(weights))
    elif model_name == "gim_lightglue":
        from .lightglue import LightGlue, SuperPoint
        detector = SuperPoint({"max_num_keypoints": 2048, "force_num_keypoints": True, "detection_threshold": 0.0,
                               "nms_radius": 3, "trainable": False, **kw})
        model = LightGlue({"filter_threshold": 0.1, "flash": False, "checkpointed": True, **kw})
        if weights:
            sd = _load_ckpt(weights)
            for k in list(sd.keys()):
                if k.startswith("model."):
                    sd.pop(k)
                elif k.startswith("superpoint."):
                    sd[k.replace("superpoint.", "", 1)] = sd.pop(k)
            detector.load_state_dict(sd)
            sd = _load_ckpt(weights)
            for k in list(sd.keys()):
                if k.startswith("superpoint."):
                    sd.pop(k)
                elif k.startswith("model."):
                    sd[k.replace("model.", "", 1)] = sd.pop(k)
            model.load_state_dict(sd)
    elif model_name == "root_sift":      # no weights: OpenCV's SIFT on the host, the fused matcher on the device
        from .nn_match import RootSiftMatcher, _cv2
        _cv2()                           # without the detector: the documented error, before anything touches the device
        return RootSiftMatcher(device=device), None
    else:
        raise ValueError(f"--model must be one of {MODELS}, got {model_name!r}")
    if detector is not None:
        detector = detector.eval().to(device)
    return model.eval().to(device), detector


@torch.no_grad()
def match_pair(model_name, model, detector, path0, path1, device="cuda", resize_max=None, num=5000, ransac_solve="host",
               ransac_sampler="host", ransac_refine=0, ransac_score="count"):
    """demo.py:405-511 -> dict(mkpts0_f, mkpts1_f, mconf, m_bids, hw0_i, hw1_i); coordinates in pixels of the pre-processed images
    for the dense matchers and gim_loftr (as the reference leaves them), of the original images for gim_lightglue (:499-500).
    ransac_solve="device": the seven-point solve of the geometry filter runs on the matches' device too, fused with the scoring
    (pose.find_fundamental_mat(solve="device"); `ransac_backend` is then "device"); "host" is the path described below.
    ransac_sampler: the `sampler` of pose.find_fundamental_mat on the numpy and device backends -- "host" (default_rng, the default),
    "philox" (the counter-based draw, made on the host) or "device" (drawn and reduced on the GPU; needs ransac_solve="device").
    OpenCV draws its own samples.
    ransac_refine: the `refine` of pose.find_fundamental_mat on the numpy and device backends -- 0 (the default) or up to 8 rounds
    of eight-point refit on the inliers, the step OpenCV's USAC ends with.
    ransac_score: the `score` of pose.find_fundamental_mat on the numpy and device backends -- "count" (the default) or "magsac"
    (the MAGSAC++ loss that the reference's USAC_MAGSAC names; needs ransac_sampler "philox" or "device")."""
    if ransac_solve not in ("host", "device"):
        raise ValueError(f"ransac_solve={ransac_solve!r}: host or device")
    if ransac_sampler not in ("host", "philox", "device") or (ransac_sampler == "device" and ransac_solve != "device"):
        raise ValueError(f"ransac_sampler={ransac_sampler!r}: host, philox or device, the last with ransac_solve='device'")
    if ransac_score not in ("count", "magsac") or (ransac_score == "magsac" and ransac_sampler == "host"):
        raise ValueError(f"ransac_score={ransac_score!r}: count or magsac, the last with ransac_sampler='philox' or 'device'")
    image0, scale0 = preprocess(read_image(path0), resize_max=resize_max)
    image1, scale1 = preprocess(read_image(path1), resize_max=resize_max)
    image0, image1 = image0.to(device)[None], image1.to(device)[None]
    data = dict(color0=image0, color1=image1, image0=image0, image1=image1)
    if model_name in ("gim_dkm", "gim_roma"):
        from .adapters import dense_demo_inference
        h, w = (672, 896) if model_name == "gim_dkm" else (672, 672)   # demo.py:421-424 (named width, height there)
        kpts0, kpts1, b_ids, mconf = dense_demo_inference(model, image0, image1, h, w, num)
    elif model_name == "gim_loftr":
        model(data)
        kpts0, kpts1, b_ids, mconf = data["mkpts0_f"], data["mkpts1_f"], data["m_bids"], data["mconf"]
    elif model_name == "root_sift":      # pixels of the original images (kpts * scale, lightning.py:228-229)
        data.update(scale0=torch.tensor(scale0, dtype=torch.float32, device=device)[None],
                    scale1=torch.tensor(scale1, dtype=torch.float32, device=device)[None])
        model(data)
        kpts0, kpts1, b_ids, mconf = data["mkpts0_f"], data["mkpts1_f"], data["m_bids"], data["mconf"]
    else:
        from .lightglue import gim_lightglue_inference
        gray0 = preprocess(read_image(path0, grayscale=True), grayscale=True, resize_max=resize_max)[0].to(device)[None]
        gray1 = preprocess(read_image(path1, grayscale=True), grayscale=True, resize_max=resize_max)[0].to(device)[None]
        d = dict(image0=gray0, image1=gray1, color0=image0, color1=image1,
                 scale0=torch.tensor(scale0, dtype=torch.float32, device=device)[None],
                 scale1=torch.tensor(scale1, dtype=torch.float32, device=device)[None],
                 image_size0=torch.tensor(gray0.shape[-2:][::-1], device=device)[None],
                 image_size1=torch.tensor(gray1.shape[-2:][::-1], device=device)[None])
        gim_lightglue_inference(detector, model, d)
        kpts0, kpts1, b_ids, mconf = d["mkpts0_f"], d["mkpts1_f"], d["m_bids"], d["mconf"]
    out = {"mkpts0_f": kpts0, "mkpts1_f": kpts1, "m_bids": b_ids, "mconf": mconf,
           "hw0_i": image0.shape[2:], "hw1_i": image1.shape[2:], "scale0": scale0, "scale1": scale1,
           "color0": image0, "color1": image1}
    # robust fitting on the host (demo.py:514-517): OpenCV's USAC_MAGSAC when cv2 imports, else seven-point RANSAC with the same
    # threshold / confidence / iteration bound (gim_amd/pose.py: plain counting, or its own MAGSAC++ scoring under
    # ransac_score="magsac"; `backend` says which one produced the mask)
    if len(kpts0) >= 8:
        from . import pose
        p0, p1 = kpts0.float().cpu().numpy(), kpts1.float().cpu().numpy()
        out["ransac_backend"] = "device" if ransac_solve == "device" else pose.backend()
        if out["ransac_backend"] == "device":
            # solved and scored on the matches' device, one launch per RANSAC step (pose.DeviceFundamental)
            out["F"], out["inliers"] = pose.find_fundamental_mat(p0, p1, threshold=1.0, prob=0.999999, max_iters=10000,
                                                                 device=kpts0.device if kpts0.is_cuda else None, solve="device",
                                                                 sampler=ransac_sampler, refine=ransac_refine, score=ransac_score)
        elif out["ransac_backend"] == "cv2":
            import cv2
            out["F"], mask = cv2.findFundamentalMat(p0, p1, cv2.USAC_MAGSAC, ransacReprojThreshold=1.0, confidence=0.999999, maxIters=10000)
            out["inliers"] = mask.ravel() > 0 if mask is not None else np.zeros(len(p0), dtype=bool)
        else:
            # the seven-point candidates are scored on the model's device (pose.DeviceScorer), the solver stays on the host
            out["F"], mask = pose.find_fundamental_mat(p0, p1, threshold=1.0, prob=0.999999, max_iters=10000,
                                                       device=kpts0.device if kpts0.is_cuda else None, sampler=ransac_sampler,
                                                       refine=ransac_refine, score=ransac_score)
            out["inliers"] = mask
    return out


def compute_geom(out, device=None, ransac_solve="host", ransac_sampler="host", ransac_refine=0, homography_refit="host",
                 ransac_score="count"):
    """demo.py:180-227 on the dict of `match_pair` -> {"Fundamental": F [3,3] | None, "Homography": H [3,3] | None}, or {} for
    fewer than 8 matches (the reference's 2 x DEFAULT_MIN_NUM_MATCHES).  "Fundamental" is the model the robust-fitting step of
    `match_pair` found (`out["F"]`: pose.find_fundamental_mat's on the numpy backend, cv2's when cv2 filtered; computed here with
    pose.find_fundamental_mat when the dict has none).  "Homography" maps image 1 onto image 0, the reference's argument order and
    parameters: pose.find_homography(mkpts1, mkpts0, 1.0, 0.999999, 10000, device=device) -- on `device` the four-point solve and the
    scoring are one launch per RANSAC step, device=None is the host path.  ransac_solve: the `solve` of pose.find_fundamental_mat
    when the fundamental matrix is computed here ("device" needs `device`).  ransac_sampler: the `sampler` of both calls ("device"
    needs `device`, and ransac_solve="device" when the fundamental matrix is computed here).  ransac_refine: the `refine` of
    pose.find_fundamental_mat when the fundamental matrix is computed here.  homography_refit: the `refit` of pose.find_homography
    -- "host" (the default: `homography_dlt`) or "device" (one gim_model_refit launch; needs `device`), which `main` asks for
    whenever the RANSAC already runs on the device, i.e. on a GPU with --ransac-sampler device.  ransac_score: the `score` of both
    calls ("magsac" needs ransac_sampler "philox" or "device")."""
    from . import pose
    p0 = np.asarray(out["mkpts0_f"].detach().float().cpu().numpy() if torch.is_tensor(out["mkpts0_f"]) else out["mkpts0_f"], dtype=np.float64)
    p1 = np.asarray(out["mkpts1_f"].detach().float().cpu().numpy() if torch.is_tensor(out["mkpts1_f"]) else out["mkpts1_f"], dtype=np.float64)
    if len(p0) < 8:
        return {}
    F = out["F"] if "F" in out else pose.find_fundamental_mat(p0, p1, threshold=1.0, prob=0.999999, max_iters=10000, device=device,
                                                                   solve=ransac_solve, sampler=ransac_sampler, refine=ransac_refine,
                                                                   score=ransac_score)[0]
    H, _ = pose.find_homography(p1, p0, 1.0, 0.999999, 10000, device=device, sampler=ransac_sampler,
                                refit=homography_refit, score=ransac_score)
    return {"Fundamental": None if F is None else np.asarray(F, dtype=np.float64), "Homography": H}


def _as_u8_chw(image, device):
    """uint8 [H,W,3] / [H,W] array (`read_image`) or float tensor [3,H,W] / [1,3,H,W] in [0,1] (`preprocess`) -> uint8 [C,H,W] tensor"""
    if torch.is_tensor(image):
        t = image[0] if image.dim() == 4 else image
        if t.dtype != torch.uint8:
            t = (t.float() * 255.0).round().clamp(0, 255).to(torch.uint8)
    else:
        a = np.asarray(image)
        t = torch.from_numpy(np.ascontiguousarray(a[None] if a.ndim == 2 else a.transpose(2, 0, 1)))
    return t.contiguous().to(device) if device is not None else t.contiguous()


def warp_pair(image0, image1, H, device="cuda", warp=None):
    """wrap_images(image0, image1, geom, "Homography") of demo.py:230-266 without the figure -> uint8 [H0, W0 + W0, 3]: image 0
    beside cv2.warpPerspective(image 1, H, size of image 0), which is ops.warp_perspective on `device` (exact bilinear weights, zero
    border; include/gim_hip.h states the difference from cv2's fixed-point weights).  Images: uint8 arrays of `read_image` or float
    tensors of `preprocess`.  warp: another implementation of ops.warp_perspective(image uint8 [C,H,W], H, out_hw) -- a test's oracle
    on a box without a GPU; there is no silent host path."""
    from . import ops
    i0 = _as_u8_chw(image0, None)
    i1 = _as_u8_chw(image1, device if warp is None else None)
    w1 = (ops.warp_perspective if warp is None else warp)(i1, H, tuple(i0.shape[-2:]))
    w1 = torch.as_tensor(w1).cpu()
    pair = torch.cat([i0.cpu().expand(w1.shape[0], -1, -1) if i0.shape[0] == 1 else i0.cpu(), w1], dim=2)
    pair = pair.expand(3, -1, -1) if pair.shape[0] == 1 else pair
    return np.ascontiguousarray(pair.permute(1, 2, 0).numpy())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", choices=MODELS, default="gim_dkm")
    ap.add_argument("--weights", default=None, help="checkpoint path (default: weights/<the reference's file name> if it exists)")
    ap.add_argument("--image0", default=join("assets", "demo", "a1.png"))
    ap.add_argument("--image1", default=join("assets", "demo", "a2.png"))
    ap.add_argument("--precision", choices=["bf16", "fp32"], default=None)
    ap.add_argument("--resize-max", type=int, default=None)
    ap.add_argument("--dinov2-weights", default=None, help="gim_roma: the DINOv2 ViT-L/14 file the reference downloads")
    ap.add_argument("--out", default=None, help="directory for <name0>_<name1>_<model>_warp.png (image 0 beside image 1 warped by the homography)")
    ap.add_argument("--ransac-solve", choices=["host", "device"], default="host",
                    help="device: the seven-point solve of the geometry filter on the GPU, fused with the scoring (default: the host's solver)")
    ap.add_argument("--ransac-sampler", choices=["host", "philox", "device"], default="host",
                    help="who draws the RANSAC samples: numpy's default_rng (default), the counter-based draw on the host, or the same "
                         "draw on the GPU with every step reduced there (device: needs --ransac-solve device)")
    ap.add_argument("--ransac-refine", type=int, choices=range(0, 9), default=0, metavar="R",
                    help="rounds of eight-point refit on the inliers after the fundamental-matrix RANSAC, 0 to 8 (default 0: none)")
    ap.add_argument("--ransac-score", choices=["count", "magsac"], default="count",
                    help="how the RANSAC ranks its hypotheses: the inlier count (default) or the MAGSAC++ loss the reference's USAC_MAGSAC "
                         "names (magsac: needs --ransac-sampler philox or device)")
    args = ap.parse_args(argv)
    if args.ransac_sampler == "device" and args.ransac_solve != "device":
        ap.error("--ransac-sampler device needs --ransac-solve device")
    if args.ransac_score == "magsac" and args.ransac_sampler == "host":
        ap.error("--ransac-score magsac needs --ransac-sampler philox or device")
    weights = args.weights
    if weights is None and args.model in CKPT and os.path.exists(join("weights", CKPT[args.model])):
        weights = join("weights", CKPT[args.model])
    if weights is None and args.model in CKPT:
        print(f"gim_amd.demo: no checkpoint ({join('weights', CKPT[args.model])} not found): running on the modules' seeded init")
    model, detector = build(args.model, weights, args.precision, dinov2_weights=args.dinov2_weights)
    out = match_pair(args.model, model, detector, args.image0, args.image1, resize_max=args.resize_max, ransac_solve=args.ransac_solve,
                     ransac_sampler=args.ransac_sampler, ransac_refine=args.ransac_refine, ransac_score=args.ransac_score)
    n = len(out["mconf"])
    print(f"{args.model}: {n} matches" + (f", {int(out['inliers'].sum())} inliers ({out['ransac_backend']} RANSAC)" if "inliers" in out else " (fewer than 8: no RANSAC)"))
    for k in range(min(n, 5)):
        a, b = out["mkpts0_f"][k].tolist(), out["mkpts1_f"][k].tolist()
        print(f"  ({a[0]:8.2f}, {a[1]:8.2f}) <-> ({b[0]:8.2f}, {b[1]:8.2f})  conf {float(out['mconf'][k]):.4f}")
    if args.out is not None:     # demo.py:537-540
        kp = out["mkpts0_f"]
        out["geom"] = compute_geom(out, device=kp.device if kp.is_cuda else None, ransac_solve=args.ransac_solve,
                                   ransac_sampler=args.ransac_sampler, ransac_refine=args.ransac_refine,
                                   homography_refit="device" if kp.is_cuda and args.ransac_sampler == "device" else "host",
                                   ransac_score=args.ransac_score)
        if out["geom"].get("Homography") is None:
            print("  no homography (fewer than 8 matches, or no sample with 4 inliers): no _warp.png")
        else:
            from PIL import Image
            os.makedirs(args.out, exist_ok=True)
            name0, name1 = (os.path.splitext(os.path.basename(p))[0] for p in (args.image0, args.image1))
            path = join(args.out, f"{name0}_{name1}_{args.model}_warp.png")
            Image.fromarray(warp_pair(out["color0"], out["color1"], out["geom"]["Homography"], device=out["color1"].device)).save(path)
            print(f"  wrote {path}")
    return out


if __name__ == "__main__":
    main()
