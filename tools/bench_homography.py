"""pose.find_homography on the host against `device=` (csrc/homography.hip: four-point solve and scoring fused, one launch per RANSAC
step), and ops.warp_perspective (csrc/warp.hip), on synthetic matches: 2 000 matches of a known homography, 50 % gross outliers,
0.5 px noise.

    python tools/bench_homography.py [--matches 2000] [--steps 3] [--repeats 5] [--out profiles/homography.txt]

Three sides in one process, alternating, on the same inputs:
  (a) find_homography on the host (numpy: homography_4pt + transfer_error);
  (b) find_homography(device=): the same indices drawn on the host and uploaded, models / flags / counts read back per step;
      one step alone (250 samples: upload, launch, read-back) is reported next to it;
  (c) ops.warp_perspective of a 640 x 480 x 3 image onto a 640 x 480 destination, uint8 and fp32 (device events; the kernel only).
A figure is a host clock around `--steps` calls (the device sides end in a read-back, i.e. synchronised), repeated `--repeats` times:
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
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
    import numpy as np
    import torch
    from gim_amd import ops, pose, pose_math
    assert torch.cuda.is_available(), "bench_homography.py needs a HIP device (the device paths have no CPU mode)"
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

    def compare(sides, extra):
        for fn in sides.values():
            fn()
        ms = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, fn in sides.items():
                ms[k].append(timed(fn, args.steps))
        for k in sides:
            emit({"what": k, **extra, "ms_median": round(statistics.median(ms[k]), 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4)})
        return ms

    P = args.matches
    rng = np.random.default_rng(1)
    a = 0.2
    H = np.array([[np.cos(a) * 1.1, -np.sin(a), 25.0], [np.sin(a), np.cos(a) * 0.95, -18.0], [2e-4, -1e-4, 1.0]])
    src = rng.uniform([0, 0], [640, 480], (P, 2))
    q = np.concatenate([src, np.ones((P, 1))], 1) @ H.T
    dst = q[:, :2] / q[:, 2:] + rng.normal(size=(P, 2)) * 0.5
    dst[:P // 2] = rng.uniform([0, 0], [640, 480], (P // 2, 2))
    emit({"what": "bench_homography", "device": torch.cuda.get_device_name(0), "matches": P, "steps": args.steps, "repeats": args.repeats,
          "host_threads": torch.get_num_threads()})

    Hh, mh = pose.find_homography(src, dst, 1.0, 0.999999, 10000, seed=0)
    Hd, md = pose.find_homography(src, dst, 1.0, 0.999999, 10000, seed=0, device=dev)
    emit({"what": "agreement (a) / (b)", "host_inliers": int(mh.sum()), "device_inliers": int(md.sum()), "masks_differ_at": int((mh != md).sum()),
          "max_abs_model_difference": float(np.abs(Hh - Hd).max())})
    ms = compare({"(a) find_homography (host)": lambda: pose.find_homography(src, dst, 1.0, 0.999999, 10000, seed=0),
                  "(b) find_homography(device=)": lambda: pose.find_homography(src, dst, 1.0, 0.999999, 10000, seed=0, device=dev)}, {"P": P})
    ka, kb = list(ms)
    emit({"what": "(a) / (b): host time / device time", "median": round(statistics.median(ms[ka]) / statistics.median(ms[kb]), 2),
          "worst_case": round(min(ms[ka]) / max(ms[kb]), 2)})
    idx = np.argsort(rng.random((250, P)), axis=1)[:, :4]
    dh = pose.DeviceHomography(src, dst, 1.0, dev)
    compare({"one step, host: homography_4pt + transfer_error counts (250 samples)":
             lambda: pose_math._count_inliers(*[x.reshape(-1, *x.shape[2:]) for x in pose.homography_4pt(src[idx], dst[idx])], src, dst, 1.0, error=pose.transfer_error),
             "one step, device: upload idx + gim_homography_step + read-back (250 samples)": lambda: dh.solve(idx)}, {"P": P, "K": 250})

    # ---- (c) the warp ---------------------------------------------------------------------------------------------------------------
    for dtype in (torch.uint8, torch.float32):
        img = (torch.rand(1, 3, 480, 640, device=dev) * 255).to(dtype)
        ops.warp_perspective(img, H, (480, 640))

        def kernel_ms(n=50):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            out = None
            e0.record()
            for _ in range(n):
                out = ops.warp_perspective(img, H, (480, 640))
            e1.record()
            torch.cuda.synchronize()
            assert out is not None
            return e0.elapsed_time(e1) / n
        kernel_ms()
        km = [kernel_ms() for _ in range(args.repeats)]
        px = 480 * 640
        emit({"what": f"(c) ops.warp_perspective 640x480x3 {str(dtype).split('.')[-1]} (H check + upload + kernel per call, device events)",
              "ms_median": round(statistics.median(km), 4), "ms_min": round(min(km), 4), "ms_max": round(max(km), 4),
              "Mpixels_per_s_median": round(px / statistics.median(km) / 1e3, 1)})


if __name__ == "__main__":
    main()
