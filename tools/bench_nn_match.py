"""ops.nn_match (the fused mutual-NN + ratio sweep of csrc/nn_match.hip) against the same arithmetic done the reference's way with stock
torch ops on the same device (what trainer/lightning.py:215-230 computes: the materialised n0 x n1 similarity matrix, its row and column
maxima, the mutual mask, the two best values per row), at the keypoint counts
root_sift produces: n0 = n1 = 4800 (640 x 480 / 64) and 32400 (the video labeller's nfeatures), D = 128.

    python tools/bench_nn_match.py [--sizes 4800,32400] [--steps 10] [--repeats 5] [--out profiles/<name>_nn_match.txt]

Both sides run in one process, alternating, on the same seeded SIFT-like descriptors (integers 0..255, desc1 = noisy permuted subset
of desc0 plus unrelated rows).  A figure is a host clock around `--steps` calls that ends in a device synchronise, repeated `--repeats`
times: median, and min / max as the spread -- differences inside the spread mean nothing.  Peak device memory is
torch.cuda.max_memory_allocated over one call of a side, minus what was allocated before it (the descriptors).  The outputs of the
two sides are compared (rows that differ are near-ties: the sides sum in different orders).  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4800,32400")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    import torch
    from gim_amd import ops
    assert torch.cuda.is_available(), "bench_nn_match.py needs a HIP device (the product path has no CPU mode)"
    dev = torch.device("cuda", 0)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def descriptors(n, D, seed):
        g = torch.Generator().manual_seed(seed)

        def sift_like(m):
            d = torch.empty(m, D).exponential_(1 / 25.0, generator=g)
            d[torch.rand(m, D, generator=g) < 0.45] = 0
            return d.round().clamp_(0, 255)
        d0 = sift_like(n)
        m = int(0.6 * n)
        src = torch.randperm(n, generator=g)[:m]
        planted = (d0[src] + (torch.rand(m, D, generator=g) * 6 - 3).round() * (d0[src] > 0)).clamp_(0, 255)
        d1 = torch.cat([planted, sift_like(n - m)])[torch.randperm(n, generator=g)]
        return (d0 + 1e-3).to(dev), (d1 + 1e-3).to(dev)      # no zero-sum row

    def torch_side(desc0, desc1, thr=0.8):
        """the baseline's arithmetic restated with stock torch ops, similarity matrix materialised: a row matches the column of its largest
        similarity when it is also the largest of that column and the distance ratio of its two best columns is below thr"""
        a = torch.sqrt(desc0 / desc0.sum(1)[:, None])
        b = torch.sqrt(desc1 / desc1.sum(1)[:, None])
        sim = torch.mm(a, b.t())                                  # [n0, n1] fp32
        row_best, col_best = sim.amax(1), sim.amax(0)
        mutual = sim.eq(row_best[:, None]).logical_and_(sim.eq(col_best[None, :]))
        hit, col = mutual.max(1)                                  # first mutual column of the row, if any
        two = sim.topk(2, dim=1).values
        near, far = (2.0 - 2.0 * two).sqrt().unbind(1)            # distances of unit vectors to the best and second best column
        hit = hit & (near / far < thr)
        return col.masked_fill(~hit, -1), row_best

    def hip_side(desc0, desc1):
        return ops.nn_match(desc0, desc1, rootsift=True, ratio=0.8)

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    emit({"what": "bench_nn_match", "device": torch.cuda.get_device_name(0), "dim": args.dim, "steps": args.steps, "repeats": args.repeats})
    for n in [int(x) for x in args.sizes.split(",")]:
        d0, d1 = descriptors(n, args.dim, seed=n)
        sides = {"torch (materialised matrix)": lambda: torch_side(d0, d1), "gim_nn_match": lambda: hip_side(d0, d1)}
        for fn in sides.values():      # warm-up of both
            fn()
            fn()
        mt, st = sides["torch (materialised matrix)"]()
        mh, sh = sides["gim_nn_match"]()
        emit({"what": "agreement", "n": n, "matches_torch": int((mt >= 0).sum()), "matches_hip": int((mh >= 0).sum()),
              "rows_that_differ": int((mt != mh.long()).sum()), "max_score_diff": float((st - sh).abs().max())})
        ms = {k: [] for k in sides}
        for _ in range(args.repeats):  # the two sides alternate: same box, same minute
            for k, fn in sides.items():
                ms[k].append(timed(fn, args.steps))
        for k, fn in sides.items():
            emit({"what": k, "n0": n, "n1": n, "D": args.dim, "ms_median": round(statistics.median(ms[k]), 4), "ms_min": round(min(ms[k]), 4),
                  "ms_max": round(max(ms[k]), 4), "peak_MB_beyond_inputs": round(peak(fn) / 1e6, 2),
                  "TFLOPs_median": round(2.0 * n * n * args.dim / statistics.median(ms[k]) / 1e9, 2)})
        a, b = statistics.median(ms["torch (materialised matrix)"]), statistics.median(ms["gim_nn_match"])
        emit({"what": "torch time / gim_nn_match time", "n": n, "median": round(a / b, 3),
              "worst_case": round(min(ms["torch (materialised matrix)"]) / max(ms["gim_nn_match"]), 3)})


if __name__ == "__main__":
    main()
