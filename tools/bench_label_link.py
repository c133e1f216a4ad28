"""`link` and `propagate` of the video labeller, host against device, in one process (profiles/label_link.txt):

    python tools/bench_label_link.py [--out profiles/label_link.txt]

(a) the dict / set formulation on the host -- tests/label_link_oracle.py: a dict per side from rounded pixel key to the last row, the
    shared keys as a set, the sorted unique (i, j) columns; its keys are Python floats, which hash faster than the numpy scalars the
    reference's dict(zip(array, ...)) holds, so this host side is no slower than the reference's;
(b) video_labels.link(device=) on labels that already are on the device, including the read of its 4-byte count
at N = M in {5 000, 32 400, 8 x 32 400} rows on a 1920 x 1080 key range with about 30 % shared keys, and a 9-hop propagate both ways
(10 frames of a synthetic video, 32 000 rows per frame pair).  The two sides alternate; a sample is the mean of `reps` calls between
two host clock reads with a device synchronise before each; reported: the median of 5 samples [min .. max].  The device result is
compared with the host's, bit for bit, before anything is timed.  Needs a GPU: there is no fall-back."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import label_link_oracle as O   # noqa: E402
from gim_amd import video_labels as V   # noqa: E402

W, H = 1920, 1080


def labels(rng, n, shared=0.3):
    lab0 = rng.uniform(0.0, [W - 1, H - 1, W - 1, H - 1], (n, 4)).astype(np.float32)
    lab1 = rng.uniform(0.0, [W - 1, H - 1, W - 1, H - 1], (n, 4)).astype(np.float32)
    k = int(shared * n)
    lab1[rng.permutation(n)[:k], :2] = lab0[rng.permutation(n)[:k], 2:]
    return lab0, lab1


def video(rng, frames=10, tracks=40000, seen=0.8):
    cells = rng.permutation((W - frames) * H)[:tracks]
    base = np.stack([cells % (W - frames), cells // (W - frames)], 1).astype(np.float32)
    out = {1: {}}
    for f in range(frames - 1):
        rows = rng.permutation(tracks)[:int(seen * tracks)]
        out[1][(f, f + 1)] = [np.concatenate([base[rows] + np.float32([f, 0]), base[rows] + np.float32([f + 1, 0])], 1)]
    return out


def sample(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def compare(host, dev, reps_host, reps_dev, rounds=5):
    host(), dev()                                                # warm-up of both
    th, td = [], []
    for _ in range(rounds):
        th.append(sample(host, reps_host))
        td.append(sample(dev, reps_dev))
    fmt = lambda t: f"{statistics.median(t):10.3f} [{min(t):9.3f} .. {max(t):9.3f}]"   # noqa: E731
    return fmt(th), fmt(td), statistics.median(th) / statistics.median(td)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_link needs a GPU")
    dev = torch.device(args.device)
    rng = np.random.default_rng(0)
    lines = [f"link / propagate, host dict-and-set formulation against video_labels.link(device=) on {torch.cuda.get_device_name(dev)}",
             f"key range {W} x {H}; ms per call, median of 5 samples [min .. max]; the two sides alternate in one process", "",
             f"{'case':<28}{'joined':>8}  {'host (a), ms':<36}{'device (b), ms':<36}{'host / device':>14}"]
    for n, reps_host, reps_dev in ((5000, 20, 200), (32400, 3, 100), (8 * 32400, 1, 30)):
        lab0, lab1 = labels(rng, n)
        d0, d1 = torch.from_numpy(lab0).to(dev), torch.from_numpy(lab1).to(dev)
        want = O.link(lab0, lab1, W, 1)
        got = V.link(d0, d1, W, H, 1, device=dev)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), n
        th, td, ratio = compare(lambda: O.link(lab0, lab1, W, 1), lambda: V.link(d0, d1, W, H, 1, device=dev), reps_host, reps_dev)
        lines.append(f"{'link N = M = %d' % n:<28}{len(want):>8}  {th:<36}{td:<36}{ratio:>13.1f}x")
    vid = video(rng)
    walk = O.Walk(vid, W, 64)
    store = V.LabelStore()
    for pair, sources in vid[1].items():
        store.put(1, pair, sources[0])
    run_host = lambda: walk.propagate(0, 9, [1])   # noqa: E731
    run_dev = lambda: V.propagate(store, 0, 9, [1], width=W, height=H, min_final_matches=64, device=dev)   # noqa: E731
    want, got = run_host(), run_dev()                            # the first device run uploads the labels; they stay there
    assert got[1:] == want[1:] == (0, 9) and np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    th, td, ratio = compare(run_host, run_dev, 1, 20)
    lines.append(f"{'propagate, 9 hops x 32000':<28}{len(want[0]):>8}  {th:<36}{td:<36}{ratio:>13.1f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
