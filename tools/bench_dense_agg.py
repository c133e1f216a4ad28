"""Dense SfM bookkeeping: the dense matches of the exhaustive pairs of 32 synthetic images (496 pairs, 8 192 matches each, coordinates of
1 536 x 1 152 images) turned into hloc's keypoints and keypoint-indexed matches two ways, from the same device tensors:

  (a) host loop      gim_amd.hloc_formats as the reference's match_dense.py does it: per pair the matches copied to the host,
                     ImageKeypoints.add on both sides; per image finalize(8192); per pair nearest_ids (a KDTree per side) and
                     matches0_from_ids
  (b) aggregator     gim_amd.dense_sfm.DenseMatchAggregator: add_pair (store + vote on the device), finalize(8192) (one read-back),
                     assign(batch_pairs) (one read-back per batch)

    python tools/bench_dense_agg.py [--images 32] [--matches 8192] [--size 1536x1152] [--repeats 5] [--batch-pairs 32]
                                    [--out profiles/dense_agg.txt]
    rocprofv3 --kernel-trace --stats -- python tools/bench_dense_agg.py --repeats 1 --device-only      # each kernel's time alone

Both sides run in one process and alternate.  A figure is a host clock around one pass over the whole list that ends in a device
synchronise, repeated `--repeats` times after one untimed pass: median, and min / max as the spread -- differences inside the spread mean
nothing.  Before the timing the two sides are compared: keypoint cells per image and the share of equal matches0 entries (they differ
where fp32 sums in arrival order and exact sums pick another bin or another of the 8192 best cells; tests/test_gpu_dense_agg.py pins
this on small scenarios).  One JSON line per figure."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--matches", type=int, default=8192)
    ap.add_argument("--size", default="1536x1152")
    ap.add_argument("--max-kps", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-pairs", type=int, default=32)
    ap.add_argument("--device-only", action="store_true", help="skip the host loop (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    import numpy as np
    import torch
    from gim_amd import hloc_formats as H
    from gim_amd.dense_sfm import DenseMatchAggregator
    assert torch.cuda.is_available(), "bench_dense_agg.py needs a HIP device (the product path has no CPU mode)"
    dev = torch.device("cuda", 0)
    W, Hh = (int(x) for x in args.size.split("x"))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    # every image sees the same 20 000 scene points (jittered by up to a pixel per pair, as a dense matcher's samples are): cells are
    # hit from many pairs, as in a real scene
    g = torch.Generator().manual_seed(0)
    scene = [torch.rand(20000, 2, generator=g) * torch.tensor([W - 1.0, Hh - 1.0]) for _ in range(args.images)]
    names = [f"im{i:02d}.jpg" for i in range(args.images)]
    pairs = list(itertools.combinations(range(args.images), 2))
    data = []
    for i, j in pairs:
        pick = torch.randint(0, 20000, (args.matches,), generator=g)
        hi = torch.tensor([W - 1.0, Hh - 1.0])
        k0 = torch.minimum((scene[i][pick] + torch.rand(args.matches, 2, generator=g) - 0.5).clamp_min_(0), hi)
        k1 = torch.minimum((scene[j][pick] + torch.rand(args.matches, 2, generator=g) - 0.5).clamp_min_(0), hi)
        data.append((k0.to(dev), k1.to(dev), (0.05 + 0.95 * torch.rand(args.matches, generator=g)).to(dev)))

    def host_loop():
        imgs = {n: H.ImageKeypoints() for n in names}
        stored = []
        for (i, j), (k0, k1, sc) in zip(pairs, data):
            k0, k1, sc = k0.cpu().numpy(), k1.cpu().numpy(), sc.cpu().numpy()
            stored.append((k0, k1, sc))
            imgs[names[i]].add(k0, sc, 2, 8)
            imgs[names[j]].add(k1, sc, 2, 8)
        final = {n: imgs[n].finalize(args.max_kps) for n in names}
        out = []
        for (i, j), (k0, k1, sc) in zip(pairs, stored):
            out.append(H.matches0_from_ids(H.nearest_ids(k0, final[names[i]][0], 2), H.nearest_ids(k1, final[names[j]][0], 2), sc))
        return final, out

    def aggregator():
        agg = DenseMatchAggregator(max_error=2, cell_size=8, device=dev, capacity_matches=len(pairs) * args.matches)
        for n in names:
            agg.add_image(n, W, Hh)
        for (i, j), (k0, k1, sc) in zip(pairs, data):
            agg.add_pair(names[i], names[j], k0, k1, sc)
        final = agg.finalize(args.max_kps)
        out = list(agg.assign(args.batch_pairs))
        torch.cuda.synchronize()
        return final, out, agg

    emit({"what": "bench_dense_agg", "device": torch.cuda.get_device_name(0), "images": args.images, "pairs": len(pairs),
          "matches_per_pair": args.matches, "size": args.size, "max_kps": args.max_kps, "batch_pairs": args.batch_pairs, "repeats": args.repeats})
    sides = {"(b) aggregator": aggregator}
    fb, mb, agg = aggregator()
    if not args.device_only:
        sides = {"(a) hloc_formats host loop": host_loop, **sides}
        fa, ma = host_loop()
        same_kp = sum(len({tuple(k) for k in fa[n][0].tolist()} & {tuple(k) for k in fb[n][0].tolist()}) for n in names)
        emit({"what": "agreement", "keypoints (a)": sum(len(fa[n][0]) for n in names), "keypoints (b)": sum(len(fb[n][0]) for n in names),
              "keypoint positions in both": same_kp, "matches0 entries (a)": int(sum((m >= 0).sum() for m, _ in ma)),
              "matches0 entries (b)": int(sum((m >= 0).sum() for m, _ in mb)), "dropped (b)": int(np.sum(agg.dropped()))})
    del agg
    ms = {k: [] for k in sides}
    for _ in range(args.repeats):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in ms.items():
        emit({"what": name, "ms_per_list_median": round(statistics.median(v), 2), "ms_min": round(min(v), 2), "ms_max": round(max(v), 2),
              "ms_per_pair_median": round(statistics.median(v) / len(pairs), 3)})
    if len(sides) == 2:
        a, b = ms["(a) hloc_formats host loop"], ms["(b) aggregator"]
        emit({"what": "(a) time / (b) time", "median": round(statistics.median(a) / statistics.median(b), 2), "worst_case": round(min(a) / max(b), 2)})


if __name__ == "__main__":
    main()
