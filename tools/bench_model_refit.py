"""The least-squares refit on the host (pose.homography_dlt: LAPACK's SVD of a 2n x 9 system, then a second mask) against
gim_model_refit (csrc/model_refit.hip: normalisation, the 9 x 9 normal matrix, its smallest eigenvector, the fresh mask and the
accept rule in one launch), alone and inside the entry points, on synthetic matches: 2 000 matches in pixels of a 640 x 480 pair,
50 % gross outliers, 0.3 px noise, threshold 1 px -- a planar scene for the homography, a general one for the fundamental matrix.

    python tools/bench_model_refit.py [--matches 2000] [--steps 3] [--repeats 5] [--out profiles/model_refit.txt]
    python tools/bench_model_refit.py --kernel-only      # twenty launches per kind and batch size and nothing else, for a
                                                         # rocprofv3 --kernel-trace --stats run of its own
    python tools/bench_model_refit.py --default-only     # the default paths alone (runs on any commit: nothing new is named)

Sides in one process, alternating, on the same inputs:
  find_homography       pose.find_homography(device=, sampler="device") with refit="host" / refit="device";
  the refit alone       pose.homography_dlt on the inliers + DeviceHomography.mask / DeviceHomography.refit on resident points;
  find_fundamental_mat  pose.find_fundamental_mat(device=, solve="device", sampler="device") with refine=0 / refine=3;
  verify_pairs          32 pairs of 2 000 matches, refine=0 / refine=2, per pair.
A figure is a host clock around `--steps` calls (every side ends in a read-back, i.e. synchronised), repeated `--repeats` times:
median, and min / max as the spread.  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time


def scene(np, kind, n, seed):
    """n matches (a, b) in pixels: b ~ H a on a plane (kind 0) or a general two-view scene (kind 1); half of b uniform, 0.3 px noise"""
    rng = np.random.default_rng(seed)
    K = np.array([[520.0, 0.0, 320.0], [0.0, 520.0, 240.0], [0.0, 0.0, 1.0]])
    th = np.deg2rad(10.0)
    R = np.array([[np.cos(th), 0.0, np.sin(th)], [0.0, 1.0, 0.0], [-np.sin(th), 0.0, np.cos(th)]])
    t = np.array([0.4, -0.1, 0.15])
    a = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    rays = np.concatenate([a, np.ones((n, 1))], 1) @ np.linalg.inv(K).T
    depth = 5.0 / (rays @ np.array([0.1, -0.2, 1.0])) if kind == 0 else rng.uniform(3.0, 9.0, n)
    X = (rays * depth[:, None]) @ R.T + t
    b = (X @ K.T)[:, :2] / (X @ K.T)[:, 2:]
    bad = rng.permutation(n)[:n // 2]
    b[bad] = np.stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))], 1)
    good = np.ones(n, dtype=bool)
    good[bad] = False
    return a + 0.3 * rng.normal(size=a.shape) * good[:, None], b + 0.3 * rng.normal(size=b.shape) * good[:, None]


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
    import numpy as np
    import torch
    from gim_amd import ops, pose
    assert torch.cuda.is_available(), "bench_model_refit.py needs a HIP device (the device paths have no CPU mode)"
    dev = torch.device("cuda", 0)
    n = args.matches
    ha, hb = scene(np, 0, n, 1)
    fa, fb = scene(np, 1, n, 2)

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

    def compare(sides, extra=None, per=1):
        for fn in sides.values():
            fn()
        ms = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, fn in sides.items():
                ms[k].append(timed(fn, args.steps) / per)
        for k, v in ms.items():
            emit({"what": k, **(extra or {}), "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)})

    if args.kernel_only:
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
        for kind, (a, b) in enumerate(((ha, hb), (fa, fb))):
            M = pose.find_homography(a, b, device=dev, sampler="device")[0] if kind == 0 else \
                pose.find_fundamental_mat(a, b, device=dev, solve="device", sampler="device")[0]
            for B in (1, 32):
                A, Bp, Ms = up(np.tile(a, (B, 1))), up(np.tile(b, (B, 1))), up(np.tile(M, (B, 1, 1)))
                off = up(np.arange(B + 1, dtype=np.int32) * n)
                for _ in range(20):
                    ops.model_refit(kind, A, Bp, Ms, 1.0, offsets=off, rounds=1)
                torch.cuda.synchronize()
        return
    emit({"what": "bench_model_refit", "device": torch.cuda.get_device_name(0), "matches": n, "steps": args.steps, "repeats": args.repeats,
          "host_threads": torch.get_num_threads()})
    kw_h = dict(device=dev, sampler="device")
    kw_f = dict(device=dev, solve="device", sampler="device")
    pairs = [scene(np, 1, n, 100 + i) for i in range(32)]
    if args.default_only:
        compare({"find_homography(device=, sampler='device'), default refit": lambda: pose.find_homography(ha, hb, **kw_h)}, {"P": n})
        compare({"find_fundamental_mat(solve='device', sampler='device'), default refine": lambda: pose.find_fundamental_mat(fa, fb, **kw_f)}, {"P": n})
        compare({"verify_pairs, 32 pairs, default refine, per pair": lambda: pose.verify_pairs(pairs, device=dev, sampler="device")}, {"P": n, "B": 32}, per=32)
        return
    Hh, mh = pose.find_homography(ha, hb, refit="host", **kw_h)
    Hd, md = pose.find_homography(ha, hb, refit="device", **kw_h)
    emit({"what": "agreement refit='host' / 'device'", "host_n": int(mh.sum()), "device_n": int(md.sum()), "masks_differ_at": int((mh != md).sum()),
          "H_differs_by_rel": float(np.abs(Hh - Hd).max() / np.abs(Hh).max())})
    compare({"find_homography(device=, sampler='device'), refit='host'": lambda: pose.find_homography(ha, hb, refit="host", **kw_h),
             "find_homography(device=, sampler='device'), refit='device'": lambda: pose.find_homography(ha, hb, refit="device", **kw_h)}, {"P": n})
    # the refit alone, from the RANSAC's model and mask, on a step object that holds the points
    step = pose.DeviceHomography(ha, hb, 1.0, dev)
    H0 = pose._ransac_on_device([(ha, hb)], pose.DeviceHomography, 1.0, 0.999999, 10000, 0, dev)[0][0][0]
    m0 = np.asarray(step.mask(H0), dtype=bool)

    def host_refit():
        H2 = pose.homography_dlt(ha[m0], hb[m0])
        return H2, np.asarray(step.mask(H2), dtype=bool)

    compare({"refit alone: pose.homography_dlt on the inliers + the second mask (gim_homography_mask)": host_refit,
             "refit alone: gim_model_refit on resident points, H, mask and counts read back": lambda: step.refit(H0, 1)}, {"P": n, "inliers": int(m0.sum())})
    F0, f0 = pose.find_fundamental_mat(fa, fb, refine=0, **kw_f)
    F3, f3 = pose.find_fundamental_mat(fa, fb, refine=3, **kw_f)
    emit({"what": "find_fundamental_mat refine=0 / refine=3", "inliers_0": int(f0.sum()), "inliers_3": int(f3.sum())})
    compare({"find_fundamental_mat(solve='device', sampler='device'), refine=0": lambda: pose.find_fundamental_mat(fa, fb, refine=0, **kw_f),
             "find_fundamental_mat(solve='device', sampler='device'), refine=3": lambda: pose.find_fundamental_mat(fa, fb, refine=3, **kw_f)}, {"P": n})
    compare({"verify_pairs, 32 pairs, refine=0, per pair": lambda: pose.verify_pairs(pairs, device=dev, sampler="device", refine=0),
             "verify_pairs, 32 pairs, refine=2, per pair": lambda: pose.verify_pairs(pairs, device=dev, sampler="device", refine=2)}, {"P": n, "B": 32}, per=32)


if __name__ == "__main__":
    main()
