"""The pose half of the ZEB loop with its RANSAC candidates scored on the device (csrc/ransac_score.hip through pose.DeviceScorer) against
the host path of gim_amd/pose.py (numpy), on synthetic two-view matches: 2 000 matches, 50 % gross outliers, 1e-3 noise.

    python tools/bench_pose.py [--matches 2000] [--models 2500] [--pairs 8] [--steps 3] [--repeats 5] [--out profiles/<name>_pose_score.txt]

Two comparisons, both sides in one process, alternating, on the same inputs:
  (a) one scoring step: K = 2 500 five-point candidates x P = 2 000 points.  Host: pose_math._count_inliers.  Device: DeviceScorer.counts,
      i.e. the upload of the step's models, the launch and the read-back of the counts; the kernel alone (device events around
      gim_ransac_score, models already resident) is reported next to it.
  (b) zeb.estimate_pose per pair, host against `device=`, and `--pairs` such pairs through zeb.device_batch_estimator (lockstep RANSAC,
      one scoring launch per step for all pairs) against the same pairs one by one on the host; the batch figure is per pair.
A figure is a host clock around `--steps` calls (the device side ends in a read-back, i.e. synchronised), repeated `--repeats` times:
median, and min / max as the spread.  The results of the two sides are compared and must be equal.  One JSON line per figure.
The numpy backend is forced (GIM_POSE_BACKEND=numpy): with OpenCV installed estimate_pose would not run pose.py at all."""
import argparse
import json
import os
import statistics
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--models", type=int, default=2500)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    os.environ["GIM_POSE_BACKEND"] = "numpy"
    import numpy as np
    import torch
    from gim_amd import ops, pose, pose_math, zeb
    assert torch.cuda.is_available(), "bench_pose.py needs a HIP device (the device scorer has no CPU mode)"
    dev = torch.device("cuda", 0)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    K0 = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])

    def pixel_pair(seed, n):
        """pixel matches of a known two-view geometry: half of them gross outliers, 0.5 px (1e-3 normalised) noise on the rest"""
        rng = np.random.default_rng(seed)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        S = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(0.25) * S + (1 - np.cos(0.25)) * S @ S
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        X = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 9, (n, 1))], 1)
        Y = X @ R.T + t
        k0 = X[:, :2] / X[:, 2:] * 500.0 + [320.0, 240.0] + rng.normal(size=(n, 2)) * 0.5
        k1 = Y[:, :2] / Y[:, 2:] * 500.0 + [320.0, 240.0] + rng.normal(size=(n, 2)) * 0.5
        k1[:n // 2] = rng.uniform(0, 480, (n // 2, 2))
        return k0, k1

    def timed(fn, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / steps

    def compare(name, sides, extra, steps=None, per=1):
        """sides: {label: fn}, host first; alternating repeats -> one line per side (ms of a call / per) and the ratio host / device"""
        for fn in sides.values():
            fn()
        ms = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, fn in sides.items():
                ms[k].append(timed(fn, steps or args.steps) / per)
        for k in sides:
            emit({"what": k, **extra, "ms_median": round(statistics.median(ms[k]), 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4)})
        host, device = list(sides)
        emit({"what": f"{name}: host time / device time", "median": round(statistics.median(ms[host]) / statistics.median(ms[device]), 2),
              "worst_case": round(min(ms[host]) / max(ms[device]), 2)})

    emit({"what": "bench_pose", "device": torch.cuda.get_device_name(0), "matches": args.matches, "models": args.models, "pairs": args.pairs,
          "steps": args.steps, "repeats": args.repeats, "host_threads": torch.get_num_threads()})

    # ---- (a) one scoring step ------------------------------------------------------------------------------------------------------
    P, K = args.matches, args.models
    k0, k1 = pixel_pair(1, P)
    x0, x1 = (k0 - K0[:2, 2]) / 500.0, (k1 - K0[:2, 2]) / 500.0
    thr2 = (0.5 / 500.0) ** 2
    rng = np.random.default_rng(2)
    idx = np.stack([rng.choice(P, 5, replace=False) for _ in range((K + 9) // 10)])
    E, valid = pose.five_point(x0[idx], x1[idx])
    Ms, valid = np.ascontiguousarray(E.reshape(-1, 3, 3)[:K]), np.ascontiguousarray(valid.reshape(-1)[:K])
    scorer = pose.DeviceScorer(x0, x1, thr2, dev)
    want, got = pose_math._count_inliers(Ms, valid, x0, x1, thr2), scorer.counts(Ms, valid)
    emit({"what": "agreement (a)", "K": K, "P": P, "models_whose_count_differs": int((want != got).sum()), "best_count": int(want.max())})
    assert (want == got).all()
    compare("(a) scoring step", {"pose_math._count_inliers (host)": lambda: pose_math._count_inliers(Ms, valid, x0, x1, thr2),
                                 "DeviceScorer.counts (upload + kernel + read-back)": lambda: scorer.counts(Ms, valid)}, {"K": K, "P": P})
    d_m, d_v = torch.from_numpy(Ms).to(dev), torch.from_numpy(valid).to(dev).view(torch.uint8)
    d_off = torch.tensor([0, P], dtype=torch.int32, device=dev)
    d_c = torch.empty(K, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    st = torch.cuda.current_stream().cuda_stream

    def kernel_ms(n=50):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ops.check(ops.lib.gim_ransac_score(p(d_m), p(d_v), p(scorer.x0), p(scorer.x1), p(d_off), 1, K, thr2, p(d_c), st), "gim_ransac_score")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    kernel_ms()
    km = [kernel_ms() for _ in range(args.repeats)]
    assert (d_c.cpu().numpy() == want).all()
    emit({"what": "gim_ransac_score alone (zeroing of the counts + kernel, device events)", "K": K, "P": P, "ms_median": round(statistics.median(km), 4),
          "ms_min": round(min(km), 4), "ms_max": round(max(km), 4), "Gevals_per_s_median": round(K * P / statistics.median(km) / 1e6, 1)})

    # ---- (b) estimate_pose ---------------------------------------------------------------------------------------------------------
    pairs = [pixel_pair(10 + i, P) for i in range(args.pairs)]
    ka, kb = pairs[0]
    same = lambda a, b: (a is None) == (b is None) and (a is None or all(np.array_equal(u, v) for u, v in zip(a, b)))   # noqa: E731
    rh, rd = zeb.estimate_pose(ka, kb, K0, K0, 0.5, 0.99999), zeb.estimate_pose(ka, kb, K0, K0, 0.5, 0.99999, device=dev)
    emit({"what": "agreement (b) one pair", "equal": bool(same(rh, rd)), "inliers": int(rh[2].sum()) if rh else 0})
    assert same(rh, rd)
    compare("(b) estimate_pose, one pair", {"estimate_pose (host)": lambda: zeb.estimate_pose(ka, kb, K0, K0, 0.5, 0.99999),
                                            "estimate_pose(device=)": lambda: zeb.estimate_pose(ka, kb, K0, K0, 0.5, 0.99999, device=dev)}, {"P": P})
    batch = zeb.device_batch_estimator(dev)
    quads = [(a, b, K0, K0) for a, b in pairs]
    bh, bd = [zeb.estimate_pose(*q, 0.5, 0.99999) for q in quads], batch(quads)
    emit({"what": "agreement (b) batch", "pairs": len(quads), "equal": bool(all(same(u, v) for u, v in zip(bh, bd)))})
    assert all(same(u, v) for u, v in zip(bh, bd))
    n = max(1, len(quads))
    compare(f"(b) estimate_pose, {n} pairs, per pair", {"estimate_pose (host), per pair": lambda: [zeb.estimate_pose(*q, 0.5, 0.99999) for q in quads],
                                                        "device_batch_estimator, per pair": lambda: batch(quads)}, {"P": P, "pairs": n}, steps=1, per=n)


if __name__ == "__main__":
    main()
