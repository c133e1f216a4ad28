"""gim_lightglue over an exhaustive pair list (the matcher half of reconstruction.py --version gim_lightglue), three ways, one GPU:

  (a) loop    hloc's loop shape (match_features.py:244-255): batch 1, both images' features uploaded per pair, LightGlue.forward(),
              matches0 / matching_scores0 brought back as int16 / fp16
  (b) stacked forward() at batch `--batch` on tensors stacked on the device beforehand (the features are NOT re-uploaded: the best
              forward() can do), results brought back the same way
  (c) bank    KeypointBank + match_pair_list at batch `--batch`, the `--images` bank insertions (upload included) inside the timing

    python tools/bench_lightglue_pairs.py [--images 32] [--kpts 2048] [--batch 8] [--repeats 5] [--precision bf16] [--storage fp16]

All three run in one process, the sides alternating (the order rotates from repeat to repeat); reported: the median of the repeats with
[min .. max], per pair.  The gather and the emit launch are timed on their own with HIP events.  Synthetic features (fp16-origin floats,
as hloc's feature files hold them), seeded random weights.  Prints a table and one JSON line."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _features(n, K, seed=0):
    """n images' features on the host: views of one scene (shared points, permuted, with jitter and descriptor noise)"""
    g = torch.Generator().manual_seed(seed)
    base_xy = torch.rand(K, 2, generator=g)
    base_d = torch.nn.functional.normalize(torch.randn(K, 256, generator=g), dim=-1)
    size = torch.tensor([640.0, 480.0])
    out = []
    for _ in range(n):
        perm = torch.randperm(K, generator=g)
        kp = (base_xy[perm] * (size - 1) + 0.5 * torch.randn(K, 2, generator=g)).clamp_(min=0)
        de = torch.nn.functional.normalize(base_d[perm] + 0.05 * torch.randn(K, 256, generator=g), dim=-1)
        out.append((kp.half().float().pin_memory(), de.half().float().pin_memory(), size.clone()))
    return out


def _events_us(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median_us": statistics.median(t), "min_us": t[0], "max_us": t[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--storage", default="fp16")
    a = ap.parse_args()
    from gim_amd import ops
    from gim_amd.lightglue import KeypointBank, LightGlue, match_pair_list
    from gim_amd.lightglue.pairs import pair_batches
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lg = LightGlue({"filter_threshold": 0.1, "flash": False, "checkpointed": True, "precision": a.precision}).eval()
    feats = _features(a.images, a.kpts)
    pairs = list(itertools.combinations(range(a.images), 2))
    batches = pair_batches(pairs, a.batch)

    def side_loop():
        n = 0
        for i, j in pairs:
            d = {}
            for s, im in (("0", feats[i]), ("1", feats[j])):
                d["keypoints" + s] = im[0][None].to(dev, non_blocking=True)
                d["descriptors" + s] = im[1][None].to(dev, non_blocking=True)
                d["image_size" + s] = im[2][None].to(dev, non_blocking=True)
            pred = lg(d)
            m = pred["matches0"][0].cpu().short().numpy()                 # match_features.py:156-160
            pred["matching_scores0"][0].cpu().half().numpy()
            n += int((m > -1).sum())
        return n

    stacked = []   # (b): built once, outside the timing
    for batch in batches:
        d = {}
        for s in (0, 1):
            d[f"keypoints{s}"] = torch.stack([feats[p[s]][0] for p in batch]).to(dev)
            d[f"descriptors{s}"] = torch.stack([feats[p[s]][1] for p in batch]).to(dev)
            d[f"image_size{s}"] = torch.stack([feats[p[s]][2] for p in batch]).to(dev)
        stacked.append(d)

    def side_stacked():
        n = 0
        for d in stacked:
            pred = lg(d)
            m = pred["matches0"].short().cpu().numpy()
            pred["matching_scores0"].half().cpu().numpy()
            n += int((m > -1).sum())
        return n

    def side_bank():
        bank = KeypointBank(a.images, a.kpts, storage=a.storage, device=dev)
        bank.bind(lg)
        for i, (kp, de, sz) in enumerate(feats):
            bank.put(i, kp.to(dev, non_blocking=True), de.to(dev, non_blocking=True), sz)
        out = match_pair_list(lg, bank, pairs, batch_pairs=a.batch)
        return sum(int((m > -1).sum()) for _, _, m, _ in out)

    sides = [("loop", side_loop), ("stacked", side_stacked), ("bank", side_bank)]
    matches = {}
    for name, fn in sides:   # warm-up: weight packing, kernel loading, allocator
        matches[name] = fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in sides}
    for rep in range(a.repeats):
        for k in range(len(sides)):
            name, fn = sides[(rep + k) % len(sides)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / len(pairs) * 1e3)

    # the two new launches alone, at the batch size of (c)
    bank = KeypointBank(a.images, a.kpts, storage=a.storage, device=dev)
    bank.bind(lg)
    for i, (kp, de, sz) in enumerate(feats):
        bank.put(i, kp.to(dev), de.to(dev), sz)
    B, K = min(a.batch, len(pairs)), a.kpts
    s0 = bank.slot_tensor(bank.slots([p[0] for p in pairs[:B]]))
    s1 = bank.slot_tensor(bank.slots([p[1] for p in pairs[:B]]))
    alias = a.precision == "fp32"
    CAT = torch.empty(2 * B * K, 512, dtype={"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[a.precision], device=dev)
    X32 = CAT[:, :256] if alias else torch.empty(2 * B * K, 256, device=dev)
    enc = torch.empty(2 * B * K, 64, device=dev)
    gather = _events_us(lambda: ops.lg_gather_pairs(bank.desc, bank.enc, s0, s1, X32, None if alias else CAT, enc))
    r = ops.AssignResult()
    r.matches0 = torch.randint(-1, K, (B, K), device=dev)
    r.mscores0 = torch.rand(B, K, device=dev)
    emit = _events_us(lambda: ops.lg_emit_hloc(r))
    kp1, de1, sz1 = feats[0]
    kpd, ded = kp1.to(dev), de1.to(dev)
    put = _events_us(lambda: bank.put(0, kpd, ded, sz1))

    def stat(v):
        return {"median_ms_per_pair": statistics.median(v), "min": min(v), "max": max(v), "pairs_per_s": 1e3 / statistics.median(v)}

    res = {name: stat(v) for name, v in times.items()}
    print(f"{len(pairs)} pairs of {a.images} images, K = {a.kpts}, precision {a.precision}, bank storage {a.storage}, "
          f"batch {a.batch}, median of {a.repeats} [min .. max]")
    print("| side | ms / pair | pairs / s | vs (a) |")
    print("|---|---|---|---|")
    label = {"loop": "(a) batch-1 loop, features uploaded per pair, forward()", "stacked": f"(b) forward() at batch {a.batch}, pre-stacked on the device",
             "bank": f"(c) match_pair_list at batch {a.batch}, {a.images} bank insertions included"}
    for name, _ in sides:
        s = res[name]
        print(f"| {label[name]} | {s['median_ms_per_pair']:.3f} [{s['min']:.3f} .. {s['max']:.3f}] | {s['pairs_per_s']:.1f} | "
              f"{res['loop']['median_ms_per_pair'] / s['median_ms_per_pair']:.2f} x |")
    for nm, e in (("gim_lg_gather_pairs", gather), ("gim_lg_emit_hloc", emit), ("KeypointBank.put (one image, incl. host side)", put)):
        print(f"{nm}: {e['median_us']:.1f} us [{e['min_us']:.1f} .. {e['max_us']:.1f}]" + (f" at B = {B}" if "gim" in nm else ""))
    print(json.dumps({"metric": "gim_lightglue exhaustive pair list", "images": a.images, "pairs": len(pairs), "keypoints": a.kpts,
                      "precision": a.precision, "storage": a.storage, "batch": a.batch, "repeats": a.repeats, "sides": res,
                      "matches": matches, "gather": gather, "emit": emit, "put": put, "data": "synthetic"}))


if __name__ == "__main__":
    main()
