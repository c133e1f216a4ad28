"""root_sift over a pair list: the exhaustive pairs of 32 synthetic images (496 pairs) matched three ways on the same device, D = 128 at
n = 1000 / 2048 / 4800 descriptors per image and D = 256 at n = 2048 (SuperPoint's width through the hloc plugin nn_ratio_hip):

  (a) per pair, as before    a loop of RootSiftMatcher.match_descriptors: both descriptor sets normalised per pair, three tensors and a
                             workspace allocated per pair, the match count read back per pair
  (b) bare ops.nn_match      the same launches without the read-back and the gather: one synchronisation at the end of the list
  (c) pair list              match_descriptor_pair_list over a DescriptorBank at batch_pairs 8 and 32, the 32 `put`s (normalisation once
                             per image) inside the timing, hloc's int16 / fp16 datasets read back once per batch

    python tools/bench_nn_match_pairs.py [--cases 128:1000,128:2048,128:4800,256:2048] [--images 32] [--repeats 5] [--out profiles/nn_match_pairs.txt]

All sides run in one process and alternate.  A figure is a host clock around one pass over the whole list that ends in a device
synchronise, repeated `--repeats` times after one untimed pass: median, and min / max as the spread -- differences inside the spread mean
nothing.  Before the timing the matches of (c) are compared with those of (b) for every pair (they are bit-equal by construction;
tests/test_gpu_nn_match_pairs.py).  One JSON line per figure."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128:1000,128:2048,128:4800,256:2048", help="D:n per case")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    import torch
    from gim_amd import ops
    from gim_amd.nn_match import DescriptorBank, RootSiftMatcher, match_descriptor_pair_list
    assert torch.cuda.is_available(), "bench_nn_match_pairs.py needs a HIP device (the product path has no CPU mode)"
    dev = torch.device("cuda", 0)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def images(n, D, count, seed):
        """`count` views of one scene: every image holds noisy copies of a random 60 % of the scene's descriptors plus rows of its own"""
        g = torch.Generator().manual_seed(seed)

        def sift_like(m):
            d = torch.empty(m, D).exponential_(1 / 25.0, generator=g)
            d[torch.rand(m, D, generator=g) < 0.45] = 0
            return d.round().clamp_(0, 255)
        scene, m = sift_like(n), int(0.6 * n)
        out = []
        for _ in range(count):
            src = scene[torch.randperm(n, generator=g)[:m]]
            seen = (src + (torch.rand(m, D, generator=g) * 6 - 3).round() * (src > 0)).clamp_(0, 255)
            d = torch.cat([seen, sift_like(n - m)])[torch.randperm(n, generator=g)]
            out.append(((torch.rand(n, 2, generator=g) * 640).to(dev), (d + 1e-3).to(dev)))      # no zero-sum row
        return out

    emit({"what": "bench_nn_match_pairs", "device": torch.cuda.get_device_name(0), "images": args.images,
          "pairs": args.images * (args.images - 1) // 2, "repeats": args.repeats})
    matcher = RootSiftMatcher(ratio=0.8)
    for case in args.cases.split(","):
        D, n = (int(x) for x in case.split(":"))
        imgs = images(n, D, args.images, seed=n + D)
        pairs = list(itertools.combinations(range(args.images), 2))

        def per_pair():
            return [matcher.match_descriptors(*imgs[i], *imgs[j])["mconf"].shape[0] for i, j in pairs]

        def bare():
            out = [ops.nn_match(imgs[i][1], imgs[j][1], rootsift=True, ratio=0.8) for i, j in pairs]
            torch.cuda.synchronize()
            return out

        def pair_list(batch):
            bank = DescriptorBank(args.images, n, D=D, rootsift=True, device=dev)
            for k, (kp, d) in enumerate(imgs):
                bank.put(k, kp, d)
            out = match_descriptor_pair_list(bank, pairs, batch_pairs=batch, ratio=0.8)
            torch.cuda.synchronize()
            return out

        sides = {"(a) match_descriptors per pair": per_pair, "(b) bare ops.nn_match, one sync": bare,
                 "(c) pair list, batch_pairs 8": lambda: pair_list(8), "(c) pair list, batch_pairs 32": lambda: pair_list(32)}
        # agreement first (also the untimed pass of every side)
        counts, ref, got = per_pair(), bare(), pair_list(32)
        pair_list(8)
        same = all(torch.equal(m.cpu().short(), torch.from_numpy(g[2])) for (m, _), g in zip(ref, got))
        emit({"what": "agreement", "D": D, "n": n, "pairs": len(pairs), "pair list == single pair on every row": bool(same),
              "matches per pair (mean)": round(sum(counts) / len(counts), 1)})
        del ref, got
        ms = {k: [] for k in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        for name, v in ms.items():
            emit({"what": name, "D": D, "n": n, "ms_per_list_median": round(statistics.median(v), 2), "ms_min": round(min(v), 2),
                  "ms_max": round(max(v), 2), "us_per_pair_median": round(statistics.median(v) / len(pairs) * 1e3, 1)})
        a = statistics.median(ms["(a) match_descriptors per pair"])
        for name in list(sides)[1:]:
            emit({"what": f"(a) time / {name} time", "D": D, "n": n, "median": round(a / statistics.median(ms[name]), 3),
                  "worst_case": round(min(ms["(a) match_descriptors per pair"]) / max(ms[name]), 3)})
        del imgs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
