"""Frame preparation of the video labeller, host against device, in one process (profiles/frame_prep.txt):

    python tools/bench_frame_prep.py [--out profiles/frame_prep.txt]

Two jobs on a seeded 1920 x 1080 frame: long side 720 with the segmenter's `norm` output, and 1600 x 896 with `rgb` + `mask` (a 960 x
540 class map, three excluded classes).
(a) the host restatement frame_prep.frame_prep_np -- and cv2.resize(INTER_AREA) with the same conversions where cv2 imports -- plus the
    upload of its result;
(b) ops.frame_prep on the frame already on the device, and once more with the upload of the uint8 frame (6.2 MB, paid once per frame
    however many jobs read it) counted in.
The sides alternate; a sample is the mean of `reps` calls between two host clock reads with a device synchronise before each;
reported: the median of 5 samples [min .. max].  The device result is compared with the host's, bit for bit, before anything is
timed.  The kernel alone: `rocprofv3 --kernel-trace --stats -- python tools/bench_frame_prep.py --kernel-only`, a run of its own.
Needs a GPU: there is no fall-back."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from gim_amd import frame_prep as fp   # noqa: E402
from gim_amd import ops   # noqa: E402

W, H = 1920, 1080
EXCLUDE = [2, 12, 20]
JOBS = (("long side 720, norm", (720, 405), fp.OUT_NORM), ("1600 x 896, rgb + mask", (1600, 896), fp.OUT_RGB | fp.OUT_MASK | fp.MASKED))


def sample(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--kernel-only", action="store_true", help="20 launches per job and nothing else, for a profiler run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_prep needs a GPU")
    dev = torch.device(args.device)
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    seg = np.kron(rng.integers(0, 30, (54, 96)), np.ones((10, 10), dtype=np.int64)).astype(np.uint8)
    frame_d, seg_d = torch.from_numpy(frame)[None].to(dev), torch.from_numpy(seg)[None].to(dev)
    excl_d = torch.from_numpy(fp.exclude_table(EXCLUDE)).to(dev)
    try:
        import cv2
    except ImportError:
        cv2 = None
    if args.kernel_only:
        for _, size, flags in JOBS:
            for _ in range(20):
                ops.frame_prep(frame_d, seg_d, excl_d, [(0, None, size, flags)])
        torch.cuda.synchronize()
        return
    lines = [f"frame preparation, {W} x {H} uint8 frame, host restatement against ops.frame_prep on {torch.cuda.get_device_name(dev)}",
             "ms per call, median of 5 samples [min .. max]; the sides alternate in one process",
             "cv2: " + ("cv2.resize(INTER_AREA) + the same conversions + upload" if cv2 else "not measured (cv2 does not import here)"), ""]
    fmt = lambda t: f"{statistics.median(t):9.3f} [{min(t):8.3f} .. {max(t):8.3f}]"   # noqa: E731
    for name, size, flags in JOBS:
        names = [n for k, n in enumerate(fp.OUTPUTS) if flags & (1 << k)]

        def host():
            o = fp.frame_prep_np(frame, seg, EXCLUDE, None, size, flags)
            return [torch.from_numpy(o[n]).to(dev) for n in names]

        def host_cv2():
            u8 = cv2.resize(frame, size, interpolation=cv2.INTER_AREA)
            if flags & fp.OUT_NORM:
                return [torch.from_numpy(np.ascontiguousarray(((u8.astype(np.float32) / 255 - fp.MEAN) / fp.STD).transpose(2, 0, 1))).to(dev)]
            m = cv2.resize(cv2.resize(seg, (W, H), interpolation=cv2.INTER_NEAREST), size, interpolation=cv2.INTER_NEAREST)
            m = (fp.exclude_table(EXCLUDE)[m] == 0).astype(np.uint8)
            return [torch.from_numpy(m).to(dev), torch.from_numpy(np.ascontiguousarray((u8 * m[..., None]).transpose(2, 0, 1))).to(dev) / 255]

        def device():
            return ops.frame_prep(frame_d, seg_d, excl_d, [(0, None, size, flags)])

        def device_upload():
            return ops.frame_prep(torch.from_numpy(frame)[None].to(dev), seg_d, excl_d, [(0, None, size, flags)])

        want, got = fp.frame_prep_np(frame, seg, EXCLUDE, None, size, flags), device()
        for n in names:
            assert got.get(0, n).cpu().numpy().tobytes() == want[n].tobytes(), (name, n)
        assert int(got.kept[0]) == want["kept"]
        sides = [("host frame_prep_np + upload", host, 1)] + ([("host cv2 + upload", host_cv2, 5)] if cv2 else []) + \
                [("ops.frame_prep, frame resident", device, 50), ("ops.frame_prep + frame upload", device_upload, 20)]
        for _, fn, _ in sides:
            fn()
        times = {label: [] for label, _, _ in sides}
        for _ in range(5):
            for label, fn, reps in sides:
                times[label].append(sample(fn, reps))
        lines.append(f"{name}: outputs {', '.join(names)}; bit-equal to frame_prep_np")
        for label, _, _ in sides:
            lines.append(f"    {label:<34}{fmt(times[label])}")
        lines.append("")
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
