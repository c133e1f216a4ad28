"""ms per image and algorithmic TFLOP/s of gim_semseg's segment() (the fast path: uint8 map, no full-resolution scores) at the
reference's sizes: 1920 x 1080 and 1920 x 1440 (reconstruction.py, --size 1920) and 720 x 540 (the video labeller, --size 720), in each
precision.  Seeded weights (tests/semseg_oracle.py): the timing does not depend on the values, as long as no 16-bit run trips the
range check (the script reports it when one does).  Algorithmic flops = 2 * MACs of every convolution (real channels, no padding).

    python tools/bench_semseg.py [--precisions bf16,fp16,fp32] [--iters 10] [--sizes 1080x1920,1440x1920,540x720]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def conv_flops(H, W):
    """algorithmic flops of the convolutions of one H x W image (ResnetDilated + PPMDeepsup inference)"""
    from gim_amd.semseg.model import LAYERS, dilation_schedule, downsample_stride
    f = 0
    h, w = -(-H // 2), -(-W // 2)
    f += 2 * h * w * 64 * 3 * 9 + 2 * h * w * 64 * 64 * 9 + 2 * h * w * 128 * 64 * 9
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    inpl = 128
    for li, (planes, nblk) in enumerate(LAYERS, start=1):
        for bi in range(nblk):
            st, _ = dilation_schedule(li, bi)
            f += 2 * h * w * planes * inpl
            if bi == 0 and downsample_stride(li) == 2:
                h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            else:
                h2, w2 = h, w
            f += 2 * h2 * w2 * planes * planes * 9 + 2 * h2 * w2 * planes * 4 * planes
            if bi == 0:
                f += 2 * h2 * w2 * planes * 4 * inpl
            h, w, inpl = h2, w2, planes * 4
    f += 2 * 50 * 512 * 2048 + 2 * h * w * 512 * 4096 * 9 + 2 * h * w * 150 * 512
    return f, (h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16,fp16,fp32")
    ap.add_argument("--sizes", default="1080x1920,1440x1920,540x720")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import semseg_oracle as O
    from gim_amd.semseg import ModelBuilder, SegmentationModule
    enc_sd, dec_sd = O.make_state_dict(0)
    enc = ModelBuilder.build_encoder(arch="resnet50dilated", fc_dim=2048, weights="")
    dec = ModelBuilder.build_decoder(arch="ppm_deepsup", fc_dim=2048, num_class=150, weights="", use_softmax=True)
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    for prec in a.precisions.split(","):
        m = SegmentationModule(enc, dec, None, precision=prec).to("cuda:0").eval()
        for sz in a.sizes.split(","):
            H, W = (int(v) for v in sz.split("x"))
            img = O.seeded_image(H, W, 1).to("cuda:0")
            with torch.no_grad(), warnings.catch_warnings(record=True) as wl:
                warnings.simplefilter("always")
                for _ in range(2):
                    m.segment(img, (H, W))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    cls = m.segment(img, (H, W))       # includes the one-word read-back of the range check
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / a.iters
            fl, hw8 = conv_flops(H, W)
            print(json.dumps({"precision": prec, "size": [H, W], "h8w8": list(hw8), "ms_per_image": round(dt * 1e3, 3),
                              "tflop": round(fl / 1e12, 3), "tflops_per_s": round(fl / dt / 1e12, 1), "classes": int(cls.unique().numel()),
                              "fell_back_to_fp32": any("repeating" in str(w.message) for w in wl)}), flush=True)


if __name__ == "__main__":
    main()
