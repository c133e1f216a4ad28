"""RANSAC ranked by the inlier count (`score="count"`, the default) against the MAGSAC++ quality (`score="magsac"`,
csrc/ransac_score.hip + gim_ransac_records64), both with sampler="device" on the same inputs: 2 000 matches of a two-view scene in
pixels, 50 % gross outliers, 0.3 px noise.

    python tools/bench_magsac.py [--matches 2000] [--steps 3] [--repeats 5] [--out profiles/magsac.txt]
    python tools/bench_magsac.py --default-only   # the default calls alone (no score= keyword), through calls every earlier revision has
    python tools/bench_magsac.py --kernel-only    # a few gim_magsac_score launches and nothing else, for rocprofv3 --kernel-trace --stats

The protocol of tools/bench_ransac_sampler.py: the sides alternate in one process; a figure is a host clock around `--steps` calls
(every call ends in a read-back, i.e. synchronised), repeated `--repeats` times after one untimed pass: median, and min / max as
the spread.  Rows: pose.find_fundamental_mat(solve="device"), pose.find_homography(device=), pose.verify_pairs over 32 pairs (per
pair), and -- the default calls of the parent revision -- the same three with sampler="host" and no score.  There is no speed bar:
the quality is work the count does not do.  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    os.environ["GIM_POSE_BACKEND"] = "numpy"
    import numpy as np
    import torch
    from gim_amd import ops, pose
    assert torch.cuda.is_available(), "bench_magsac.py needs a HIP device (the device paths have no CPU mode)"
    dev = torch.device("cuda", 0)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def timed(fn, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / steps

    P = args.matches
    Kc = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])

    def scene(seed, planar=False):
        rng = np.random.default_rng(seed)
        X = np.concatenate([rng.uniform(-2.0, 2.0, (P, 2)), rng.uniform(4.0, 8.0, (P, 1))], 1)
        if planar:                                   # a plane: the two views are related by a homography
            X[:, 2] = 5.0 + 0.1 * X[:, 0] - 0.2 * X[:, 1]
        c, s = np.cos(0.2), np.sin(0.2)
        R, t = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]), np.array([0.5, 0.1, 0.05])
        a, b = X @ Kc.T, (X @ R.T + t) @ Kc.T
        p0, p1 = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:] + rng.normal(size=(P, 2)) * 0.3
        p1[:P // 2] = rng.uniform([0, 0], [640, 480], (P // 2, 2))
        return np.ascontiguousarray(p0), np.ascontiguousarray(p1)

    p0, p1 = scene(1)
    h0, h1 = scene(2, planar=True)
    pairs = [scene(100 + b) for b in range(32)]

    if args.kernel_only:
        up = lambda x: torch.from_numpy(x).to(dev)   # noqa: E731
        idx = up(pose.device_samples(1, 0, 250, P, 7))
        models, valid, _ = ops.fundamental_step(up(p0), up(p1), idx, 1.0)
        for _ in range(20):
            ops.magsac_score(1, models.view(-1, 3, 3), up(p0), up(p1), 1.0, valid=valid.view(-1))
        torch.cuda.synchronize()
        return
    emit({"what": "bench_magsac", "device": torch.cuda.get_device_name(0), "matches": P, "steps": args.steps, "repeats": args.repeats,
          "host_threads": torch.get_num_threads(), "default_only": args.default_only})

    def rows(tag, **kw):
        return {f"find_fundamental_mat(solve='device'), {tag}": (lambda: pose.find_fundamental_mat(p0, p1, device=dev, solve="device", **kw), 1),
                f"find_homography(device=), {tag}": (lambda: pose.find_homography(h0, h1, device=dev, **kw), 1),
                f"verify_pairs, 32 pairs, per pair, {tag}": (lambda: pose.verify_pairs(pairs, device=dev, **kw), 32)}

    sides = rows("default (sampler=host, no score)")
    if not args.default_only:
        sides.update(rows("sampler=device score=count", sampler="device"))
        sides.update(rows("sampler=device score=magsac", sampler="device", score="magsac"))
    inl = {}
    for name, (fn, per) in sides.items():
        out = fn()
        inl[name] = int(sum(o[1].sum() for o in out)) if isinstance(out, list) else int(out[-1].sum())
    ms = {k_: [] for k_ in sides}
    for _ in range(args.repeats):
        for name, (fn, per) in sides.items():
            ms[name].append(timed(fn, args.steps) / per)
    for name, (fn, per) in sides.items():
        emit({"what": name, "P": P, "ms_median": round(statistics.median(ms[name]), 4), "ms_min": round(min(ms[name]), 4),
              "ms_max": round(max(ms[name]), 4), "inliers": inl[name]})
    if not args.default_only:
        for name in rows("sampler=device score=count"):
            other = name.replace("score=count", "score=magsac")
            emit({"what": "magsac / count: " + name.split(", sampler")[0], "median": round(statistics.median(ms[other]) / statistics.median(ms[name]), 2)})


if __name__ == "__main__":
    main()
