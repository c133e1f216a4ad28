"""What extracting LoFTR features once is worth: forward() against extract() + match_features() / CachedPairMatcher at 640x480, batch 8.

    python tools/bench_loftr_reuse.py --part a [--root OTHER_TREE]   # forward() ms per step (also runs on a tree without the feature)
    python tools/bench_loftr_reuse.py --part b                      # match_features() ms per step, features resident; gather launches apart
    python tools/bench_loftr_reuse.py --part c                      # exhaustive pairs of 32 images (496 pairs, 62 batches): cached vs forward()
    python tools/bench_loftr_reuse.py --part trace                  # a few cached steps, for `rocprofv3 --kernel-trace --stats -- python ...`

Timing: every shape is warmed up (eager call, graph capture, replays) first; a figure is a host clock around `--steps` calls that ends in a
device synchronise, repeated `--repeats` times -- the spread of those repeats is printed next to the median, and differences inside it mean
nothing.  The gather launches are timed with device events around each launch.  One JSON line per figure; `--out FILE` appends them.
Seeded weights (tools/synth_loftr.synthetic_model) and seeded, mutually overlapping images: no data files."""
import argparse
import json
import os
import statistics
import sys
import time

H, W = 480, 640


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["a", "b", "c", "trace"])
    ap.add_argument("--root", default=None, help="import gim_amd / tools from this tree instead of the one this file is in (part a)")
    ap.add_argument("--precisions", default="fp16,bf16")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    return ap.parse_args(argv)


def main():
    args = parse_args()
    root = os.path.abspath(args.root or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path.insert(0, root)
    import torch
    from tools import synth_loftr as S
    assert torch.cuda.is_available(), "bench_loftr_reuse.py needs a HIP device (the product path has no CPU mode)"
    dev = torch.device("cuda", 0)
    nb = args.batch

    def emit(rec):
        rec = {"part": args.part, "label": args.label or os.path.basename(root), **rec}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def images(n, seed=1234):
        """n crops of ONE texture at offsets of whole coarse cells plus pixel noise: every pair overlaps by most of the frame"""
        g = torch.Generator().manual_seed(seed)
        pad = 96
        base = S.textured(1, H + pad, W + pad, g)[0]
        offs = [(8 * int(a), 8 * int(b)) for a, b in zip(torch.randint(0, pad // 8 + 1, (n,), generator=g), torch.randint(0, pad // 8 + 1, (n,), generator=g))]
        out = torch.stack([base[:, dy:dy + H, dx:dx + W] for dy, dx in offs])
        return (out + 0.02 * torch.randn(out.shape, generator=g)).clamp(0, 1).contiguous()

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def repeats(fn, steps, n):
        ms = [timed(fn, steps) for _ in range(n)]
        return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "repeats": n, "steps": steps}

    def fwd_batch(a, b):
        return {"image0": a[:, :1], "image1": b[:, :1], "color0": a, "color1": b}

    for precision in args.precisions.split(","):
        model, _ = S.synthetic_model(precision, seed=0)
        model = model.to(dev)
        if args.part == "a":
            c0h, c1h = S.textured_pairs(nb, H, W, seed=1234, frac=0.45)   # bench.py's workload
            c0, c1 = c0h.to(dev), c1h.to(dev)
            step = lambda: model(fwd_batch(c0, c1))   # noqa: E731
            for _ in range(4):
                step()
            d = fwd_batch(c0, c1)
            model(d)
            emit({"what": "forward() per step", "precision": precision, "batch": nb, "matches": int(d["b_ids"].numel()), **repeats(step, args.steps, args.repeats)})
            continue

        from gim_amd import ops
        from gim_amd.loftr import CachedPairMatcher
        if args.part in ("b", "trace"):
            c0h, c1h = S.textured_pairs(nb, H, W, seed=1234, frac=0.45)
            c0, c1 = c0h.to(dev), c1h.to(dev)
            feats = model.extract(torch.cat([c0, c1]))
            i0, i1 = list(range(nb)), list(range(nb, 2 * nb))
            fstep = lambda: model(fwd_batch(c0, c1))   # noqa: E731
            mstep = lambda: model.match_features(feats, feats, i0, i1)   # noqa: E731
            if args.part == "trace":   # no forward() here: beside the one extraction, every kernel of the trace belongs to a cached step
                for _ in range(args.steps):
                    mstep()
                torch.cuda.synchronize()
                emit({"what": "match_features() steps traced (the first eager, the rest replays of one graph)", "precision": precision, "steps": args.steps})
                continue
            for _ in range(4):
                fstep()
                r = mstep()
            # the two sides alternate inside one process: same box, same minute
            rf, rm = [], []
            for _ in range(args.repeats):
                rf.append(timed(fstep, args.steps))
                rm.append(timed(mstep, args.steps))
            med = statistics.median
            emit({"what": "forward() per step (same process)", "precision": precision, "batch": nb, "ms_median": round(med(rf), 4), "ms_min": round(min(rf), 4),
                  "ms_max": round(max(rf), 4), "repeats": args.repeats, "steps": args.steps})
            emit({"what": "match_features() per step, features resident", "precision": precision, "batch": nb, "matches": int(r["b_ids"].numel()),
                  "ms_median": round(med(rm), 4), "ms_min": round(min(rm), 4), "ms_max": round(max(rm), 4), "repeats": args.repeats, "steps": args.steps})
            ii = ops.slot_index(i0 + i1, len(feats), dev)
            gather_ms = {}
            for name, slab in (("coarse rows", feats.coarse), ("fine maps", feats.fine)):
                dst = torch.empty_like(slab)
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
                for _ in range(5):
                    ops.slot_copy(slab, dst, src_idx=ii)
                for e0, e1 in ev:
                    e0.record()
                    ops.slot_copy(slab, dst, src_idx=ii)
                    e1.record()
                torch.cuda.synchronize()
                t = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)
                moved = 2 * dst.numel() * dst.element_size()   # read + written
                gather_ms[name] = t
                emit({"what": f"gather launch: {name}", "precision": precision, "ms_median": round(t, 4), "bytes_read_plus_written": moved,
                      "TB_per_s": round(moved / t / 1e9, 3)})
            emit({"what": "gather share of match_features()", "precision": precision, "gather_ms": round(sum(gather_ms.values()), 4),
                  "share": round(sum(gather_ms.values()) / med(rm), 4)})
            continue

        # part c: the exhaustive pair list of `--images` images, in batches of nb pairs
        imgs = images(args.images).to(dev)
        pairs = [(i, j) for i in range(args.images) for j in range(i + 1, args.images)]
        batches = [pairs[k:k + nb] for k in range(0, len(pairs) - len(pairs) % nb, nb)]
        cols = [(imgs[[p[0] for p in b]].contiguous(), imgs[[p[1] for p in b]].contiguous()) for b in batches]   # the same inputs for both sides
        keys = [([p[0] for p in b], [p[1] for p in b]) for b in batches]
        npairs = len(batches) * nb

        def run_forward():
            n = 0
            for a, b in cols:
                d = fwd_batch(a, b)
                model(d)
                n += d["b_ids"].numel()
            return n

        stats = {}

        def run_cached():
            cm = CachedPairMatcher(model, capacity_images=args.images)   # a new bank: extraction is inside the timed region
            n = 0
            for (a, b), (k0, k1) in zip(cols, keys):
                d = fwd_batch(a, b)
                d["image_keys0"], d["image_keys1"] = k0, k1
                cm(d)
                n += d["b_ids"].numel()
            stats.update(cm.stats.as_dict(), bank_MB=round(cm.bank.nbytes / 1e6, 1))
            return n

        nf, nc = run_forward(), run_cached()   # warm-up of both: every shape (extractions of 1..9 images included) seen, graphs captured
        run_forward(), run_cached()
        tf, tc = [], []
        for _ in range(args.repeats):
            tf.append(timed(run_forward, 1))
            tc.append(timed(run_cached, 1))
        med = statistics.median
        emit({"what": "forward() over the pair list", "precision": precision, "images": args.images, "pairs": npairs, "batches": len(batches), "matches": nf,
              "s_median": round(med(tf) / 1e3, 4), "s_min": round(min(tf) / 1e3, 4), "s_max": round(max(tf) / 1e3, 4),
              "pairs_per_s": round(npairs / (med(tf) / 1e3), 1), "pairs_per_s_worst": round(npairs / (max(tf) / 1e3), 1), "pairs_per_s_best": round(npairs / (min(tf) / 1e3), 1)})
        emit({"what": "CachedPairMatcher over the pair list (extraction included)", "precision": precision, "images": args.images, "pairs": npairs,
              "batches": len(batches), "matches": nc, "bank": stats,
              "s_median": round(med(tc) / 1e3, 4), "s_min": round(min(tc) / 1e3, 4), "s_max": round(max(tc) / 1e3, 4),
              "pairs_per_s": round(npairs / (med(tc) / 1e3), 1), "pairs_per_s_worst": round(npairs / (max(tc) / 1e3), 1), "pairs_per_s_best": round(npairs / (min(tc) / 1e3), 1)})
        emit({"what": "speed-up of the cached list", "precision": precision, "median": round(med(tf) / med(tc), 3), "worst_case": round(min(tf) / max(tc), 3)})


if __name__ == "__main__":
    main()
