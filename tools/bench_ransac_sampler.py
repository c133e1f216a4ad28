"""RANSAC with the samples drawn on the host (`sampler="host"`, numpy's default_rng: the default) against `sampler="device"`
(csrc/ransac_sample.hip + csrc/ransac_records.hip: samples drawn and every step reduced on the GPU), the solve on the device on both
sides, on synthetic matches: 2 000 matches of a two-view scene in pixels, 50 % gross outliers, 0.1 px noise.

    python tools/bench_ransac_sampler.py [--matches 2000] [--steps 3] [--repeats 5] [--out profiles/ransac_sampler.txt]
    python tools/bench_ransac_sampler.py --default-only   # the sampler="host" rows alone, through calls every earlier revision has
    python tools/bench_ransac_sampler.py --kernel-only    # a few sampler="device" runs and nothing else, for rocprofv3 --kernel-trace --stats

The protocol of tools/bench_essential.py: the sides alternate in one process on the same inputs; a figure is a host clock around
`--steps` calls (every call ends in a read-back, i.e. synchronised), repeated `--repeats` times after one untimed pass: median, and
min / max as the spread.  Rows: pose.find_fundamental_mat(solve="device"), pose.find_homography(device=), zeb.estimate_pose(device=,
solve="device") and pose.verify_pairs over 32 pairs (per pair).  The two samplers do not walk the same trajectory, so the step counts
are reported and a per-step time with them.  Bytes per step are counted from the shapes: host sampler -- idx up, models + flags +
counts down; device sampler -- 16 B bytes up, n_rec and 32 record triples per pair down (72 more for a newly best model).  One JSON
line per figure."""
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
    from gim_amd import ops, pose, zeb
    assert torch.cuda.is_available(), "bench_ransac_sampler.py needs a HIP device (the device paths have no CPU mode)"
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
        p0, p1 = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:] + rng.normal(size=(P, 2)) * 0.1
        p1[:P // 2] = rng.uniform([0, 0], [640, 480], (P // 2, 2))
        return np.ascontiguousarray(p0), np.ascontiguousarray(p1)

    p0, p1 = scene(1)
    h0, h1 = scene(2, planar=True)
    pairs = [scene(100 + b) for b in range(32)]

    def rows(sampler):
        s = {} if sampler == "host" else {"sampler": sampler}
        return {f"find_fundamental_mat(solve='device'), sampler={sampler}": (lambda: pose.find_fundamental_mat(p0, p1, device=dev, solve="device", **s), 1, 7, 3),
                f"find_homography(device=), sampler={sampler}": (lambda: pose.find_homography(h0, h1, device=dev, **s), 1, 4, 1),
                f"estimate_pose(device=, solve='device'), sampler={sampler}": (lambda: zeb.estimate_pose(p0, p1, Kc, Kc, device=dev, solve="device", **s), 1, 5, 10),
                f"verify_pairs, 32 pairs, per pair, sampler={sampler}": (lambda: pose.verify_pairs(pairs, device=dev, **s), 32, 7, 3)}

    if args.kernel_only:
        for fn, _, _, _ in rows("device").values():
            fn()
        return
    emit({"what": "bench_ransac_sampler", "device": torch.cuda.get_device_name(0), "matches": P, "steps": args.steps, "repeats": args.repeats,
          "host_threads": torch.get_num_threads(), "default_only": args.default_only})

    # step counts: every step of either sampler goes through exactly one of the three step wrappers
    steps = {"n": 0}
    real = {n: getattr(ops, n) for n in ("fundamental_step", "essential_step", "homography_step")}

    def counting(name):
        def f(*a, **k):
            steps["n"] += 1
            return real[name](*a, **k)
        return f

    sides = rows("host")
    if not args.default_only:
        sides.update(rows("device"))
    nsteps, inl = {}, {}
    for name, (fn, per, m, k) in sides.items():
        for n in real:
            setattr(ops, n, counting(n))
        steps["n"] = 0
        out = fn()
        nsteps[name] = steps["n"]
        for n in real:
            setattr(ops, n, real[n])
        inl[name] = int(sum(o[1].sum() for o in out)) if isinstance(out, list) else int(out[-1].sum())   # (.., mask) or a list of them
    ms = {k_: [] for k_ in sides}
    for _ in range(args.repeats):
        for name, (fn, per, m, k) in sides.items():
            ms[name].append(timed(fn, args.steps) / per)
    for name, (fn, per, m, k) in sides.items():
        med = statistics.median(ms[name])
        B = per
        up, down = (16 * B, 4 * 97 * B) if "sampler=device" in name else (250 * m * 4 * B, 250 * k * (72 + 1 + 4) * B)
        emit({"what": name, "P": P, "ms_median": round(med, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
              "launch_sequences": nsteps[name], "ms_per_step": round(med * per / max(nsteps[name], 1), 4), "inliers": inl[name],
              "bytes_up_per_step": up, "bytes_down_per_step": down})
    if not args.default_only:
        for name in rows("host"):
            other = name.replace("sampler=host", "sampler=device")
            emit({"what": "host / device: " + name.split(", sampler")[0], "median": round(statistics.median(ms[name]) / statistics.median(ms[other]), 2),
                  "worst_case": round(min(ms[name]) / max(ms[other]), 2)})


if __name__ == "__main__":
    main()
