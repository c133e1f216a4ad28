"""What encoding every image once is worth to the dense matchers: the per-pair `HlocDenseMatcher.forward` loop against `match_pairs` from a
DenseFeatureBank over the exhaustive pairs of `--images` synthetic images (8 -> 28 pairs), seeded weights.

    python tools/bench_dense_pairs.py --engine dkm      # gim_dkm 672x896 -> 1152x1536
    python tools/bench_dense_pairs.py --engine roma     # gim_roma 560^2 -> 1120^2
    python tools/bench_dense_pairs.py --engine dkm --part trace   # a few bank batches, for `rocprofv3 --kernel-trace --stats -- python ...`
                                                                  # (dense_gather_kernel / dense_emit_kernel per launch; a run of its own)

Both sides run in ONE process and alternate: repeat r times side (a), then side (b) at batch_pairs 1, 2 and 4 -- the 8 extractions are part
of every (b) figure.  A figure is a host clock around the whole pair list that ends in a device synchronise; the median of `--repeats`
repeats is printed with [min .. max], and differences inside that spread mean nothing.  One JSON line per figure; `--out FILE` appends them
(profiles/dense_pairs.txt).  No data files."""
import argparse
import json
import os
import statistics
import sys
import time


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", required=True, choices=["dkm", "roma"])
    ap.add_argument("--part", default="ab", choices=["ab", "trace"])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--num-samples", type=int, default=8192)
    ap.add_argument("--out", default=None)
    return ap.parse_args(argv)


def main():
    args = parse_args()
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    import torch
    from gim_amd.adapters import HlocDenseMatcher
    from gim_amd.dense_bank import DenseFeatureBank
    assert torch.cuda.is_available(), "bench_dense_pairs.py needs a HIP device (the product path has no CPU mode)"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if args.engine == "dkm":
        from gim_amd.dkm import DKMv3
        h, w = 672, 896
        net = DKMv3(None, h, w, upsample_preds=True).eval()              # random init, upsample_res 1152 x 1536
        case = "gim_dkm 672x896 -> 1152x1536"
    else:
        from gim_amd.roma import RoMa, random_dinov2_weights
        h, w = 560, 560
        net = RoMa([h, w], dinov2_weights=random_dinov2_weights(dev)).eval()
        net.upsample_res = (1120, 1120)
        case = "gim_roma 560x560 -> 1120x1120"
    adapter = HlocDenseMatcher(net, h, w, num_samples=args.num_samples)
    g = torch.Generator().manual_seed(1234)
    base = torch.rand(3, h + 64, w + 64, generator=g)
    base = torch.nn.functional.avg_pool2d(base[None], 5, 1, 2)[0] * 0.8 + 0.1   # smooth texture, no black pixels
    images = {}
    for i in range(args.images):       # crops of one texture: every pair overlaps; already at the model's aspect ratio (no padding)
        dy, dx = (int(v) for v in torch.randint(0, 65, (2,), generator=g))
        images[f"im{i:02d}"] = base[None, :, dy:dy + h, dx:dx + w].contiguous().to(dev)
    names = list(images)
    pairs = [(names[i], names[j]) for i in range(len(names)) for j in range(i + 1, len(names))]

    def emit(rec):
        line = json.dumps({"case": case, "pairs": len(pairs), "images": len(names), "precision": net.precision, **rec})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def side_a():
        for n0, n1 in pairs:
            adapter({"image0": images[n0], "image1": images[n1]})

    def side_b(bp):
        bank = DenseFeatureBank(net, len(names))
        for n in names:
            adapter.bank_put(bank, n, images[n])
        adapter.match_pairs(bank, pairs, batch_pairs=bp)
        return bank

    if args.part == "trace":
        side_b(2)
        torch.cuda.synchronize()
        return
    sides = [("a: forward() per pair", side_a)] + [(f"b: match_pairs, batch_pairs {bp}, extractions included", lambda bp=bp: side_b(bp))
                                                   for bp in (1, 2, 4) if bp <= net.max_batch]
    bank = side_b(1)                   # warm-up of both sides: packing, allocator, first launches
    emit({"bank_bytes_per_image": bank.bytes_per_image})
    del bank
    adapter({"image0": images[names[0]], "image1": images[names[1]]})
    torch.cuda.synchronize()
    times = {nm: [] for nm, _ in sides}
    for _ in range(args.repeats):
        for nm, fn in sides:           # the sides alternate within every repeat
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[nm].append((time.perf_counter() - t0) * 1e3 / len(pairs))
    ref = statistics.median(times[sides[0][0]])
    for nm, _ in sides:
        t = times[nm]
        emit({"side": nm, "ms_per_pair_median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3),
              "speedup_vs_a": round(ref / statistics.median(t), 3)})


if __name__ == "__main__":
    main()
