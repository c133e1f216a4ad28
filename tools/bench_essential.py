"""pose.find_essential_mat / zeb.estimate_pose with the five-point solve on the host against `solve="device"` (csrc/essential.hip:
five-point solve and scoring fused, one launch per RANSAC step), on synthetic matches: 2 000 matches of a two-view scene in pixels,
50 % gross outliers, 0.1 px noise, the ZEB parameters (threshold 0.5 px, confidence 0.99999).

    python tools/bench_essential.py [--matches 2000] [--steps 3] [--repeats 5] [--out profiles/essential.txt]
    python tools/bench_essential.py --kernel-only      # a few device steps and nothing else, for a rocprofv3 --kernel-trace --stats run

Three sides in one process, alternating, on the same inputs:
  (a) host solve + host score: pose.five_point (SVD, a linear solve, LAPACK's eig) and pose.sampson_error in numpy;
  (b) host solve + device score: today's `device=` path (pose.DeviceScorer: 2 500 models uploaded, counts read back);
  (c) device step: sample indices uploaded, models / flags / counts of ONE gim_essential_step read back.
Measured: one step of 250 samples; the whole zeb.estimate_pose call (find_essential_mat + recover_pose); and 8 such pairs through
zeb.device_batch_estimator, per pair.  The sides need not walk the same trajectory (the device solver rounds differently), so the
whole-call figures include whatever difference in step count that brings; the step counts are reported.  A figure is a host clock
around `--steps` calls (the device sides end in a read-back, i.e. synchronised), repeated `--repeats` times: median, and min / max
as the spread.  One JSON line per figure."""
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
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    os.environ["GIM_POSE_BACKEND"] = "numpy"
    import numpy as np
    import torch
    from gim_amd import pose, pose_math, zeb
    assert torch.cuda.is_available(), "bench_essential.py needs a HIP device (the device paths have no CPU mode)"
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
    Kc = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])

    def scene(seed):
        rng = np.random.default_rng(seed)
        X = np.concatenate([rng.uniform(-2.0, 2.0, (P, 2)), rng.uniform(4.0, 8.0, (P, 1))], 1)
        c, s = np.cos(0.2), np.sin(0.2)
        R, t = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]), np.array([0.5, 0.1, 0.05])
        a, b = X @ Kc.T, (X @ R.T + t) @ Kc.T
        p0, p1 = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:] + rng.normal(size=(P, 2)) * 0.1
        p1[:P // 2] = rng.uniform([0, 0], [640, 480], (P // 2, 2))
        return np.ascontiguousarray(p0), np.ascontiguousarray(p1)

    p0, p1 = scene(1)
    x0, x1, thr = zeb._normalise(p0, p1, Kc, Kc, 0.5)
    x0, x1 = np.ascontiguousarray(x0), np.ascontiguousarray(x1)
    thr2 = float(thr) ** 2
    rng = np.random.default_rng(2)
    idx = np.argsort(rng.random((250, P)), axis=1)[:, :5]
    fused = pose.DeviceEssential(x0, x1, thr2, dev)
    if args.kernel_only:
        for _ in range(20):
            fused.solve(idx)
        return
    emit({"what": "bench_essential", "device": torch.cuda.get_device_name(0), "matches": P, "steps": args.steps, "repeats": args.repeats,
          "host_threads": torch.get_num_threads()})

    # ---- one step of 250 samples ------------------------------------------------------------------------------------------------------
    scorer = pose.DeviceScorer(x0, x1, thr2, dev)

    def host_solve():
        E, v = pose.five_point(x0[idx], x1[idx])
        return E.reshape(-1, 3, 3), v.reshape(-1)

    compare({"one step (a) host solve + host score (250 samples)": lambda: pose_math._count_inliers(*host_solve(), x0, x1, thr2),
             "one step (b) host solve + device score: upload 2500 models + gim_ransac_score + read-back": lambda: scorer.counts(*host_solve()),
             "one step (c) device: upload idx + gim_essential_step + read-back": lambda: fused.solve(idx),
             "one step, the host solve alone (pose.five_point, 250 samples)": host_solve}, {"P": P, "K": 250})

    # ---- the whole call ---------------------------------------------------------------------------------------------------------------
    calls = {"n": 0}
    real_solve = pose.DeviceEssential.solve

    def counting_solve(self, i):
        calls["n"] += 1
        return real_solve(self, i)

    pose.DeviceEssential.solve = counting_solve
    rd = zeb.estimate_pose(p0, p1, Kc, Kc, device=dev, solve="device")
    pose.DeviceEssential.solve = real_solve
    rh = zeb.estimate_pose(p0, p1, Kc, Kc)
    emit({"what": "agreement (a) / (c)", "host_inliers": int(rh[2].sum()), "device_inliers": int(rd[2].sum()),
          "masks_differ_at": int((rh[2] != rd[2]).sum()), "R_differs_by": float(np.abs(rh[0] - rd[0]).max()), "device_steps": calls["n"]})
    ms = compare({"whole call (a) estimate_pose (host)": lambda: zeb.estimate_pose(p0, p1, Kc, Kc),
                  "whole call (b) estimate_pose(device=)": lambda: zeb.estimate_pose(p0, p1, Kc, Kc, device=dev),
                  "whole call (c) estimate_pose(device=, solve='device')": lambda: zeb.estimate_pose(p0, p1, Kc, Kc, device=dev, solve="device")},
                 {"P": P})
    ka, kb, kc = list(ms)
    emit({"what": "(b) / (c): today's device path / device step", "median": round(statistics.median(ms[kb]) / statistics.median(ms[kc]), 2),
          "worst_case": round(min(ms[kb]) / max(ms[kc]), 2)})

    # ---- 8 pairs through the batch estimator ------------------------------------------------------------------------------------------
    B = 8
    pairs = [(*scene(100 + b), Kc, Kc) for b in range(B)]
    host_b, dev_b = zeb.device_batch_estimator(dev), zeb.device_batch_estimator(dev, solve="device")
    compare({f"batch of {B} pairs (a) estimate_pose one by one on the host, per pair": lambda: [zeb.estimate_pose(*p) for p in pairs],
             f"batch of {B} pairs (b) device_batch_estimator(device), per pair": lambda: host_b(pairs),
             f"batch of {B} pairs (c) device_batch_estimator(device, solve='device'), per pair": lambda: dev_b(pairs)},
            {"P": P, "B": B}, per=B)


if __name__ == "__main__":
    main()
