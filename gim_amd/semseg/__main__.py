"""python -m gim_amd.semseg IMAGES OUT_DIR [--size 1920] [--weights-dir weights] [--precision bf16|fp16|fp32]

reconstruction.py:26-53 (`segmentation`) as a command: for every image in IMAGES (sorted) without OUT_DIR/<name minus its 4-character
extension>.npy yet, the uint8 ADE20K-150 class map of the image resized to a long side of at most --size (1920: reconstruction.py;
720: the video labeller).  Weights: <weights-dir>/encoder_epoch_20.pth and decoder_epoch_20.pth, the reference's two-file format."""
import argparse
import os
import sys

import numpy as np

IMAGE_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gim_amd.semseg", description=__doc__.split("\n\n")[1])
    ap.add_argument("images", help="directory of images")
    ap.add_argument("out_dir", help="directory of <name>.npy class maps (created)")
    ap.add_argument("--size", type=int, default=1920, help="long side of the segmented image (1920: SfM, 720: video labeller)")
    ap.add_argument("--weights-dir", default="weights", help="holds encoder_epoch_20.pth and decoder_epoch_20.pth")
    ap.add_argument("--precision", default=None, choices=("bf16", "fp16", "fp32"))
    ap.add_argument("--device", default="cuda")
    return ap.parse_args(argv)


def map_path(out_dir, name):
    """reconstruction.py:47: '{}.npy'.format(img[:-4])"""
    return os.path.join(out_dir, "{}.npy".format(name[:-4]))


def pending(images, out_dir):
    """(name, output path) of every image in `images` whose map does not exist yet, sorted by name"""
    todo = []
    for name in sorted(os.listdir(images)):
        if not name.lower().endswith(IMAGE_EXT):
            continue
        p = map_path(out_dir, name)
        if not os.path.exists(p):
            todo.append((name, p))
    return todo


def build_module(weights_dir, precision=None, device="cuda"):
    from .model import ModelBuilder, SegmentationModule
    paths = [os.path.join(weights_dir, f) for f in ("encoder_epoch_20.pth", "decoder_epoch_20.pth")]
    for p in paths:
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} not found (the reference's ADE20K checkpoints; --weights-dir)")
    enc = ModelBuilder.build_encoder(arch="resnet50dilated", fc_dim=2048, weights=paths[0])
    dec = ModelBuilder.build_decoder(arch="ppm_deepsup", fc_dim=2048, num_class=150, weights=paths[1], use_softmax=True)
    return SegmentationModule(enc, dec, None, precision=precision).to(device).eval()


def read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def main(argv=None, module=None, segment_fn=None):
    """module / segment_fn: a prepared SegmentationModule / a stand-in for gim_amd.semseg.segment (tests)"""
    a = parse_args(argv)
    os.makedirs(a.out_dir, exist_ok=True)
    todo = pending(a.images, a.out_dir)
    if not todo:
        return 0
    if segment_fn is None:
        from . import segment as segment_fn
    if module is None:
        module = build_module(a.weights_dir, a.precision, a.device)
    import torch
    with torch.no_grad():
        for name, p in todo:
            mask = segment_fn(read_rgb(os.path.join(a.images, name)), a.size, a.device, module)
            np.save(p, mask)
            print(f"{name} -> {p} {mask.shape}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
