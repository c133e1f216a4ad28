"""Records tests/golden/semseg.npz from the reference segmenter (CPU only; needs the reference checkout, default /root/reference or
$1): networks/mit_semseg's ResnetDilated(resnet50(pretrained=False), dilate_scale=8) and PPMDeepsup(use_softmax=True) loaded STRICTLY
with tests/semseg_oracle.make_state_dict(0), run through SegmentationModule(feed_dict, segSize=...) at two odd sizes (97 x 129, and
37 x 45 where h8 x w8 = 5 x 6 < 6 x 6: overlapping PPM bins).  The reference's build_encoder is never called with empty weights (it
would download ImageNet weights).

    python tools/make_golden_semseg.py [REFERENCE_ROOT]
"""
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import semseg_oracle as O  # noqa: E402

SIZES = ((97, 129, 11), (37, 45, 12))       # (H, W, image seed)
CH_SUB = 16                                  # conv5 channels kept: every 16th
POOL_CH = slice(0, 256)                      # pooled vectors: channels 0..255
PRIVATE = re.compile(r"\._(tmp_running_mean|tmp_running_var|running_iter)$")


def main(ref_root):
    sys.path.insert(0, ref_root)
    from networks.mit_semseg.models import models as M, resnet as R
    enc_sd, dec_sd = O.make_state_dict(0)
    enc = M.ResnetDilated(R.resnet50(pretrained=False), dilate_scale=8)
    dec = M.PPMDeepsup(num_class=150, fc_dim=2048, use_softmax=True)
    rec = {}
    for nm, mod_, sd in (("enc", enc, enc_sd), ("dec", dec, dec_sd)):
        # strict on the checkpoint surface: every key of the seeded dict is consumed and every parameter / running statistic is
        # set; the only keys left are the synchronised BatchNorm's private bookkeeping buffers, which checkpoints do not carry
        r = mod_.load_state_dict(sd, strict=False)
        assert not r.unexpected_keys, r.unexpected_keys
        assert all(PRIVATE.search(k) for k in r.missing_keys), [k for k in r.missing_keys if not PRIVATE.search(k)]
        pub = {k: v for k, v in mod_.state_dict().items() if not PRIVATE.search(k)}
        assert set(pub) == set(sd) and all(tuple(pub[k].shape) == tuple(sd[k].shape) for k in sd)
        rec[nm + "_keys"] = len(pub)
        rec[nm + "_params"] = sum(v.numel() for v in pub.values())
    mod = M.SegmentationModule(enc, dec, torch.nn.NLLLoss(ignore_index=-1)).eval()
    cap = {}
    dec.conv_last.register_forward_hook(lambda m, i, o: cap.__setitem__("logits", o))
    for i in range(4):
        dec.ppm[i][0].register_forward_hook(lambda m, inp, o, i=i: cap.__setitem__(f"pool{i}", o))
    with torch.no_grad():
        for H, W, seed in SIZES:
            img = O.seeded_image(H, W, seed)
            conv5 = enc(img, return_feature_maps=True)[-1]
            scores = mod({"img_data": img}, segSize=(H, W))
            top = scores.topk(2, dim=1).values
            pooled = torch.cat([cap[f"pool{i}"].flatten(2) for i in range(4)], 2).transpose(1, 2)
            t = f"{H}x{W}"
            rec[f"img_{t}"] = img[0].numpy()
            rec[f"conv5_{t}"] = conv5[0, ::CH_SUB].numpy()
            rec[f"pooled_{t}"] = pooled[0, :, POOL_CH].numpy()
            rec[f"logits_{t}"] = cap["logits"][0].numpy()
            rec[f"cls_{t}"] = scores.argmax(1)[0].numpy().astype(np.uint8)
            rec[f"margin_{t}"] = (top[0, 0] - top[0, 1]).numpy()
            print(t, "conv5", tuple(conv5.shape), "classes", len(np.unique(rec[f"cls_{t}"])), "logit range",
                  float(cap["logits"].min()), float(cap["logits"].max()))
    out = os.path.join(ROOT, "tests", "golden", "semseg.npz")
    np.savez_compressed(out, **{k: np.asarray(v) for k, v in rec.items()})
    print(out, os.path.getsize(out), "bytes", {k: rec[k] for k in ("enc_keys", "dec_keys", "enc_params", "dec_params")})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
