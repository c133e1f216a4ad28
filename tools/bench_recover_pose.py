"""pose.recover_pose on the host (four batched LAPACK SVDs of [P,4,4]) against gim_recover_pose (csrc/recover_pose.hip: decomposition,
triangulation, cheirality counts and the winner in one launch), alone and inside zeb.estimate_pose, on synthetic matches: 2 000
matches of a two-view scene in pixels, 50 % gross outliers, 0.1 px noise, the ZEB parameters (threshold 0.5 px, confidence 0.99999) --
the scene of tools/bench_essential.py.

    python tools/bench_recover_pose.py [--matches 2000] [--steps 3] [--repeats 5] [--out profiles/recover_pose.txt]
    python tools/bench_recover_pose.py --kernel-only     # twenty launches and nothing else, for a rocprofv3 --kernel-trace --stats run
    python tools/bench_recover_pose.py --default-only    # the default paths alone (runs on any commit: nothing new is named)

Sides in one process, alternating, on the same inputs:
  recover alone   pose.recover_pose (host) / pose.recover_pose(device=): E, points and mask uploaded, results read back /
                  ops.recover_pose on points that are on the device already, best and R, t read back;
  whole call      zeb.estimate_pose(device=, solve="device", sampler="device") with recover="host" / recover="device";
  8 pairs         zeb.device_batch_estimator(device, solve="device", sampler="device"), recover="host" / "device", per pair.
A figure is a host clock around `--steps` calls (every side ends in a read-back, i.e. synchronised), repeated `--repeats` times:
median, and min / max as the spread.  One JSON line per figure."""
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
    ap.add_argument("--default-only", action="store_true")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    os.environ["GIM_POSE_BACKEND"] = "numpy"
    import numpy as np
    import torch
    from gim_amd import ops, pose, zeb
    assert torch.cuda.is_available(), "bench_recover_pose.py needs a HIP device (the device paths have no CPU mode)"
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
    B = 8
    pairs = [(*scene(100 + b), Kc, Kc) for b in range(B)]
    kw = dict(device=dev, solve="device", sampler="device")
    E, mask = pose.find_essential_mat(x0, x1, thr, prob=0.99999, **kw)
    emit({"what": "bench_recover_pose", "device": torch.cuda.get_device_name(0), "matches": P, "steps": args.steps, "repeats": args.repeats,
          "host_threads": torch.get_num_threads(), "ransac_inliers": int(mask.sum())})
    if args.default_only:
        host_b = zeb.device_batch_estimator(dev, solve="device", sampler="device")
        compare({"recover alone: pose.recover_pose on the host": lambda: pose.recover_pose(E, x0, x1, 1e9, mask=mask),
                 "whole call: estimate_pose(device=, solve='device', sampler='device'), default recover": lambda: zeb.estimate_pose(p0, p1, Kc, Kc, **kw)},
                {"P": P})
        compare({f"batch of {B} pairs: device_batch_estimator(solve='device', sampler='device'), default recover, per pair": lambda: host_b(pairs)},
                {"P": P, "B": B}, per=B)
        return
    d_E, d_x0, d_x1, d_mask = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (E, x0, x1, mask))
    if args.kernel_only:
        for _ in range(20):
            ops.recover_pose(d_E, d_x0, d_x1, mask=d_mask)[1].item()
        return

    # ---- recover alone ----------------------------------------------------------------------------------------------------------------
    def resident():
        n_good, best, R, t, _ = ops.recover_pose(d_E, d_x0, d_x1, mask=d_mask)
        return torch.cat([R.reshape(-1), t]).cpu(), n_good.cpu(), best.cpu()

    h, g = pose.recover_pose(E, x0, x1, 1e9, mask=mask), pose.recover_pose(E, x0, x1, 1e9, mask=mask, device=dev)
    emit({"what": "agreement host / device", "host_n": int(h[0]), "device_n": int(g[0]), "masks_differ_at": int((h[3] != g[3]).sum()),
          "R_differs_by": float(np.abs(h[1] - g[1]).max()), "t_differs_by": float(np.abs(h[2] - g[2]).max())})
    compare({"recover alone: pose.recover_pose on the host": lambda: pose.recover_pose(E, x0, x1, 1e9, mask=mask),
             "recover alone: pose.recover_pose(device=), E + points + mask uploaded, results read back": lambda: pose.recover_pose(E, x0, x1, 1e9, mask=mask, device=dev),
             "recover alone: ops.recover_pose on resident points, R, t, counts read back": resident}, {"P": P})

    # ---- the whole call ---------------------------------------------------------------------------------------------------------------
    rh, rd = zeb.estimate_pose(p0, p1, Kc, Kc, **kw), zeb.estimate_pose(p0, p1, Kc, Kc, recover="device", **kw)
    emit({"what": "agreement recover='host' / 'device'", "masks_differ_at": int((rh[2] != rd[2]).sum()),
          "R_differs_by": float(np.abs(rh[0] - rd[0]).max()), "t_differs_by": float(np.abs(rh[1] - rd[1]).max())})
    compare({"whole call: estimate_pose(device=, solve='device', sampler='device'), recover='host'": lambda: zeb.estimate_pose(p0, p1, Kc, Kc, **kw),
             "whole call: estimate_pose(device=, solve='device', sampler='device'), recover='device'": lambda: zeb.estimate_pose(p0, p1, Kc, Kc, recover="device", **kw)},
            {"P": P})

    # ---- 8 pairs through the batch estimator ------------------------------------------------------------------------------------------
    host_b, dev_b = zeb.device_batch_estimator(dev, solve="device", sampler="device"), zeb.device_batch_estimator(dev, solve="device", sampler="device", recover="device")
    compare({f"batch of {B} pairs: device_batch_estimator(solve='device', sampler='device'), recover='host', per pair": lambda: host_b(pairs),
             f"batch of {B} pairs: device_batch_estimator(solve='device', sampler='device'), recover='device', per pair": lambda: dev_b(pairs)},
            {"P": P, "B": B}, per=B)


if __name__ == "__main__":
    main()
