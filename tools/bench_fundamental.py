"""pose.find_fundamental_mat with the seven-point solve on the host against `solve="device"` (csrc/fundamental.hip: seven-point solve
and scoring fused, one launch per RANSAC step), on synthetic matches: 2 000 matches of a two-view scene, 50 % gross outliers, 0.5 px
noise.

    python tools/bench_fundamental.py [--matches 2000] [--steps 3] [--repeats 5] [--out profiles/fundamental.txt]

Three sides in one process, alternating, on the same inputs:
  (a) host solve + host score: pose.seven_point (SVD, determinants, eigvals) and pose.sampson_error in numpy;
  (b) host solve + device score: today's `device=` path (pose.DeviceScorer: 750 models uploaded, counts read back);
  (c) device step: sample indices uploaded, models / flags / counts of ONE gim_fundamental_step read back.
Measured: one step of 250 samples; the whole find_fundamental_mat call (threshold 1 px, prob 0.999999, max_iters 10000, the demo's
parameters); and find_fundamental_mat_batch over 8 and 32 such pairs, per pair.  The sides need not walk the same trajectory (the
device solver rounds differently), so the whole-call figures include whatever difference in step count that brings; the step counts
are reported.  A figure is a host clock around `--steps` calls (the device sides end in a read-back, i.e. synchronised), repeated
`--repeats` times: median, and min / max as the spread.  One JSON line per figure."""
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
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    import numpy as np
    import torch
    from gim_amd import pose, pose_math
    assert torch.cuda.is_available(), "bench_fundamental.py needs a HIP device (the device paths have no CPU mode)"
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

    def compare(sides, extra, per=1):
        for fn in sides.values():
            fn()
        ms = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, fn in sides.items():
                ms[k].append(timed(fn, args.steps) / per)
        for k in sides:
            emit({"what": k, **extra, "ms_median": round(statistics.median(ms[k]), 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4)})
        return ms

    P = args.matches

    def scene(seed):
        rng = np.random.default_rng(seed)
        X = np.concatenate([rng.uniform(-2.0, 2.0, (P, 2)), rng.uniform(4.0, 8.0, (P, 1))], 1)
        K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])
        c, s = np.cos(0.2), np.sin(0.2)
        R, t = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]), np.array([0.5, 0.1, 0.05])
        a, b = X @ K.T, (X @ R.T + t) @ K.T
        p0, p1 = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:] + rng.normal(size=(P, 2)) * 0.5
        p1[:P // 2] = rng.uniform([0, 0], [640, 480], (P // 2, 2))
        return np.ascontiguousarray(p0), np.ascontiguousarray(p1)

    p0, p1 = scene(1)
    emit({"what": "bench_fundamental", "device": torch.cuda.get_device_name(0), "matches": P, "steps": args.steps, "repeats": args.repeats,
          "host_threads": torch.get_num_threads()})

    # ---- one step of 250 samples ------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(2)
    idx = np.argsort(rng.random((250, P)), axis=1)[:, :7]
    scorer = pose.DeviceScorer(p0, p1, 1.0, dev)
    fused = pose.DeviceFundamental(p0, p1, 1.0, dev)

    def host_solve():
        F, v = pose.seven_point(p0[idx], p1[idx])
        return F.reshape(-1, 3, 3), v.reshape(-1)

    compare({"one step (a) host solve + host score (250 samples)": lambda: pose_math._count_inliers(*host_solve(), p0, p1, 1.0),
             "one step (b) host solve + device score: upload 750 models + gim_ransac_score + read-back": lambda: scorer.counts(*host_solve()),
             "one step (c) device: upload idx + gim_fundamental_step + read-back": lambda: fused.solve(idx),
             "one step, the host solve alone (pose.seven_point, 250 samples)": host_solve}, {"P": P, "K": 250})

    # ---- the whole call ---------------------------------------------------------------------------------------------------------------
    calls = {"n": 0}
    real_solve = pose.DeviceFundamental.solve

    def counting_solve(self, i):
        calls["n"] += 1
        return real_solve(self, i)

    pose.DeviceFundamental.solve = counting_solve
    Fd, md = pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=0, device=dev, solve="device")
    pose.DeviceFundamental.solve = real_solve
    Fh, mh = pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=0)
    emit({"what": "agreement (a) / (c)", "host_inliers": int(mh.sum()), "device_inliers": int(md.sum()), "masks_differ_at": int((mh != md).sum()),
          "device_steps": calls["n"]})
    ms = compare({"whole call (a) find_fundamental_mat (host)": lambda: pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=0),
                  "whole call (b) find_fundamental_mat(device=)": lambda: pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=0, device=dev),
                  "whole call (c) find_fundamental_mat(device=, solve='device')":
                  lambda: pose.find_fundamental_mat(p0, p1, 1.0, 0.999999, 10000, seed=0, device=dev, solve="device")}, {"P": P})
    ka, kb, kc = list(ms)
    emit({"what": "(b) / (c): today's device path / device step", "median": round(statistics.median(ms[kb]) / statistics.median(ms[kc]), 2),
          "worst_case": round(min(ms[kb]) / max(ms[kc]), 2)})

    # ---- pair lists -------------------------------------------------------------------------------------------------------------------
    for B in (8, 32):
        pairs = [scene(100 + b) for b in range(B)]
        compare({f"batch of {B} pairs, find_fundamental_mat_batch, per pair": lambda: pose.find_fundamental_mat_batch(pairs, 1.0, 0.999999, 10000, 0, dev),
                 f"the same {B} pairs one by one, solve='device', per pair":
                 lambda: [pose.find_fundamental_mat(a, b, 1.0, 0.999999, 10000, seed=0, device=dev, solve="device") for a, b in pairs]},
                {"P": P, "B": B}, per=B)


if __name__ == "__main__":
    main()
