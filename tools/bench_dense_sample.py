"""What sampling a batch of pairs in one launch sequence is worth to the dense matchers: the loop of `DenseMatcher.sample()` (one n_pos
read-back, two sorts, about 30 launches per pair) against `DenseMatcher.sample_batch` (gim_balanced_sample_pairs: no read-back, 20 launches
per batch) on the warp / certainty maps of a seeded gim_dkm at 672x896 -> 1152x1536 (n = 1152 * 3072 rows per pair).

    python tools/bench_dense_sample.py                   # num = 5000 and 8192, B = 1, 2, 4
    python tools/bench_dense_sample.py --part trace      # a few sample_batch calls at B = 4, num = 8192, for
                                                         # `rocprofv3 --kernel-trace --stats -- python ...` (a run of its own)

Both sides run in ONE process and alternate within every repeat.  A figure is a host clock around `--calls` calls that ends in a device
synchronise (side (a) synchronises once per pair by itself), per pair; the median of `--repeats` repeats is printed with [min .. max], and
differences inside that spread mean nothing.  One JSON line per figure; `--out FILE` appends them (profiles/dense_sample.txt).  No data
files."""
import argparse
import json
import os
import statistics
import sys
import time


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=["ab", "trace"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    return ap.parse_args(argv)


def main():
    args = parse_args()
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    import torch
    from gim_amd.dkm import DKMv3
    assert torch.cuda.is_available(), "bench_dense_sample.py needs a HIP device (the product path has no CPU mode)"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    h, w = 672, 896
    net = DKMv3(None, h, w, upsample_preds=True).eval()                  # random init, upsample_res 1152 x 1536
    g = torch.Generator().manual_seed(1234)
    base = torch.rand(3, h + 64, w + 64, generator=g)
    base = torch.nn.functional.avg_pool2d(base[None], 5, 1, 2)[0] * 0.8 + 0.1   # smooth texture, no black pixels
    crops = []
    for _ in range(8):                 # crops of one texture: every pair overlaps
        dy, dx = (int(v) for v in torch.randint(0, 65, (2,), generator=g))
        crops.append(base[None, :, dy:dy + h, dx:dx + w])
    BMAX = 4
    warp, cert = net.match_batch(torch.cat(crops[:BMAX]).to(dev), torch.cat(crops[BMAX:2 * BMAX]).to(dev))
    warp, cert = warp.contiguous(), cert.contiguous()
    n = cert[0].numel()
    case = {"case": f"gim_dkm 672x896 -> 1152x1536 maps, n = {n}", "n_pos": [(c > 0).sum().item() for c in cert],
            "above_thresh": [(c > net.sample_thresh).sum().item() for c in cert]}

    def emit(rec):
        line = json.dumps({**case, **rec})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def side_a(B, num):
        for b in range(B):
            net.sample(warp[b], cert[b], num)

    def side_b(B, num):
        net.sample_batch(warp[:B], cert[:B], num)

    if args.part == "trace":
        for _ in range(3):
            side_b(4, 8192)
        torch.cuda.synchronize()
        return
    for num in (5000, 8192):
        for B in (1, 2, 4):
            sides = [("a: sample() per pair", side_a), ("b: sample_batch", side_b)]
            torch.manual_seed(1)
            ref = [net.sample(warp[b], cert[b], num) for b in range(B)]
            torch.manual_seed(1)
            sp, mc, cnt = net.sample_batch(warp[:B], cert[:B], num)      # warm-up of both sides, and the two agree
            same = all(int(cnt[b]) == r[0].shape[0] and torch.equal(sp[b, :r[0].shape[0]], r[0]) and torch.equal(mc[b, :r[1].shape[0]], r[1])
                       for b, r in enumerate(ref))
            times = {nm: [] for nm, _ in sides}
            for _ in range(args.repeats):
                for nm, fn in sides:   # the sides alternate within every repeat
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn(B, num)
                    torch.cuda.synchronize()
                    times[nm].append((time.perf_counter() - t0) * 1e3 / (args.calls * B))
            base_ms = statistics.median(times[sides[0][0]])
            for nm, _ in sides:
                t = times[nm]
                emit({"num": num, "B": B, "side": nm, "ms_per_pair_median": round(statistics.median(t), 4), "min": round(min(t), 4),
                      "max": round(max(t), 4), "speedup_vs_a": round(base_ms / statistics.median(t), 3), "rows_equal": same})


if __name__ == "__main__":
    main()
