"""gim_loftr throughput bench on MI355X (driver contract: see DESIGN.md section 6).

    python bench.py                       # 1 GPU, BASELINE config 2: gim_loftr 640x480, batch 8 pairs, 16-bit operands (IEEE fp16 since round 6; --precision bf16 | fp32)
    python bench.py --gpus 8              # spawns 8 ranks itself (re-exec under torch.distributed.run, 127.0.0.1)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W        # what the driver does
    python bench.py --full                # the same headline, then every extra measurement below (minutes)
    python bench.py --dump-outputs DIR    # + what the last timed step returned, as DIR/<name>.npy (see dump_outputs)

A plain run sets up, warms up, times the K steps, dumps the outputs if asked and prints the line: `value` / `ms_per_step`
and the workload fields.  Every block described below from `roofline` on is taken with --full only (null otherwise).

A "step" = one LoFTR.forward (HIP path through the C ABI) over one batch of 8 synthetic 640x480 pairs that are
already resident in HBM, including the match-count read-back the reference's contract has
(coarse_matching.py:193).  The workload is MATCH-RICH: seeded "trained-like" weights (BatchNorm statistics
calibrated, residual branches damped) on textured image pairs of which ~45 % of the frame corresponds
(tools/synth_loftr.py), so ~1500 coarse matches per pair -- the mean of the reference's own gim_loftr dumps
 -- flow through fine gather / fine transformer / fine matching inside the timed region.  Nothing is
injected into the forward: the matches come out of the images.
Pairs shard embarrassingly across ranks (weak scaling: 8 pairs per rank per step); the only collective is one
RCCL all-gather(v) of the packed matches at the end of the run.  Rank 0 prints ONE JSON line.

`roofline`  = all gim_conv2d_bn_act launches (the implicit-GEMM MFMA kernels, still the dominant kernel: 60 % of the
              step's FLOPs since the round-3 fusions) timed live with HIP events on the launch stream in extra
              instrumented steps; inside it `fused_kernels` (the four fused kernel families, timed the same way),
              `coarse_gemm` (the coarse matching call priced as its similarity GEMM) and `whole_step` (the whole path
              priced with SURVEY 8d's algorithmic work);
`parity_mode`, `bf16_mode` = the fp32 parity mode and the other 16-bit flavour timed on the same batch, each with its
              own `parity` block;
`cpu_baseline` = the CPU oracle (a port of the reference's forward, pinned to it by golden vectors) on this
              host's cores, 1 pair, 1 warm-up + 3 timed forwards; the same oracle run yields
`parity`    = index flip rate / max coordinate and confidence deviation of the benchmarked 16-bit engine against
              the fp32 oracle on that pair;
`h2d_inclusive` = the same step with both image batches starting in pinned host memory (double-buffered copy stream).
Round 5: the headline mode is bf16, what BASELINE config 2 literally names (`fp16_mode` -- a quarter of the index flips, 2-3 % slower -- is the
extra block; rounds 3-4 headlined fp16); `engine_precision` / `fp16_overflowed` say what the module really ran as; `parity.flips_all_marginal`
and `parity.worst_flip` price every index flip by the oracle's own margin; the packed match rows are copied to (pinned) host memory inside
the timed loop; `roofline.traffic_source` names the committed per-round PMC pass `roofline.traffic` comes from.
Round 4: `n_ranks_seen` / `rank_devices` (what the process group and every rank's device really were), `config.stem_operands`
(the first convolution runs on hi + lo operand pairs by default) and `parity.plain_stem` (the same batch with plainly rounded
stem operands, round 3's arithmetic).  GIM_BENCH_DRY_MODEL=1 walks main() on CPU ranks with a stand-in model (tests only).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# host-side runner (pure torch, no HIP library needed to import it).  Module level on purpose: round 3 imported these inside
# main() BELOW their first use on the world > 1 branch and every rank of a multi-GPU job died with UnboundLocalError.
from gim_amd.runner import HostPairFeeder, all_gather_matches, bind_rank_to_cores, pack_matches  # noqa: E402

H, W = 480, 640
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "fp32": 157.3}  # dense, MI355X_MICROARCH.md
SEC_TRAFFIC_JSON = next((p for p in (os.path.join(ROOT, "profiles", f"r0{r}_traffic_secondary.json") for r in (6,)) if os.path.exists(p)), "")
TRAFFIC_JSON = next((p for p in (os.path.join(ROOT, "profiles", f"r0{r}_traffic.json") for r in (6, 5, "4s2", 4, 3, 2)) if os.path.exists(p)), "")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="pairs per rank per step")
    ap.add_argument("--precision", default="fp16", choices=["bf16", "fp16", "fp32"],
                    help="gim_loftr's mode.  fp16 (default since round 6 = the module's own default: the 16-bit kernels on IEEE-fp16 operands behind the "
                         "range guard; 0.15-0.3 %% index flips against the fp32 oracle, max |d mconf| 0.02); bf16 (the dtype BASELINE config 2 names, round 5's "
                         "headline: the same kernels on bf16 operands, 4-5 %% faster -- the fp16 MFMA draws more power --, 0.7-1.3 %% flips, max |d mconf| 0.2: "
                         "reported as `bf16_mode`); fp32: the parity mode (exact indices)")
    ap.add_argument("--coarse-sim", default=None, choices=["fp32", "bf16", "fp16"], help="override LoFTR config['coarse_sim']")
    ap.add_argument("--frac", type=float, default=0.45, help="corresponding fraction of the frame (match count knob)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also take every extra measurement of the line: roofline, h2d_inclusive, parity_mode / bf16_mode / "
                         "fp16_mode, fine_idle, secondary_workloads, cpu_baseline + parity (a plain run reports them as null)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last timed step to DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-pairs", type=int, default=1)
    ap.add_argument("--selftest-launch", action="store_true",
                    help="CPU-only check of the multi-rank launch / timing / gather protocol (gloo, no model)")
    return ap.parse_args(argv)


DUMP_INPUT_KEYS = ("image0", "image1", "color0", "color1", "mask0", "mask1")
DUMP_WHOLE_MAX = 16 << 20     # bytes: a larger output is stored as a fixed, seeded sample of DUMP_SAMPLE entries
DUMP_SAMPLE = 1 << 20
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, data, rows, prefix=""):
    """--dump-outputs: what a caller of the timed path received in the last timed step, as <out_dir>/<prefix><name>.npy --
    every tensor LoFTR.forward put into `data` (floating outputs as float32, integer / bool ones as float64: exact) and the
    packed [pair, x0, y0, x1, y1, conf] rows of the step (`matches_packed`).  data['conf_matrix'] is materialised on demand
    (737 MB at the benchmark's size): it is stored as `conf_matrix_sample` at the flat indices `conf_matrix_sample_index`,
    drawn once from a fixed seed.  Called right after the timed steps, before anything else runs on the model."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    outs = {}
    for k, v in data.items():
        if k in DUMP_INPUT_KEYS:
            continue
        if not torch.is_tensor(v) and callable(getattr(v, "get", None)):   # LazyConfMatrix
            v = v.get()
        if torch.is_tensor(v):
            outs[k] = v
    outs["matches_packed"] = rows
    total = 0
    for k, v in outs.items():
        v = v.detach()
        v = v.float() if (v.is_floating_point() and v.dtype != torch.float64) else v.double()
        if v.numel() * v.element_size() > DUMP_WHOLE_MAX:
            g = torch.Generator().manual_seed(0)
            idx = torch.randint(0, v.numel(), (DUMP_SAMPLE,), generator=g).sort().values
            arrays = {k + "_sample": v.reshape(-1)[idx.to(v.device)], k + "_sample_index": idx.double()}
        else:
            arrays = {k: v}
        for name, a in arrays.items():
            a = a.cpu().numpy()
            total += a.nbytes
            np.save(os.path.join(out_dir, prefix + name + ".npy"), a)
    assert total <= DUMP_MAX_BYTES, f"--dump-outputs wrote {total} bytes, more than {DUMP_MAX_BYTES}"
    return total


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(args, argv):
    """`python bench.py --gpus N` without a launcher: re-exec as N ranks (test.py:188-218 runs pl.Trainer(gpus=N,
    strategy=DDP); here one process per GPU under torch.distributed.run, rendezvous on 127.0.0.1)."""
    if not args.selftest_launch and os.environ.get("GIM_BENCH_DRY_MODEL") != "1":
        have = torch.cuda.device_count()
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} HIP device(s) visible")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, min(8, (os.cpu_count() or 8) // max(1, args.gpus)))))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + argv
    return subprocess.call(cmd, env=env)


def selftest_worker(args, rank, world):
    """gloo/CPU ranks walking the exact launch -> barrier -> timed loop -> gather -> max-over-ranks -> one-line
    protocol of the real bench with a stand-in step (no GPU, no model)."""
    from gim_amd.runner import all_gather_matches, pack_matches
    dist.init_process_group("gloo", rank=rank, world_size=world)
    assert dist.get_world_size() == world == args.gpus, (dist.get_world_size(), world, args.gpus)
    nb = args.batch

    def step(s):
        g = torch.Generator().manual_seed(1000 * rank + s)
        m = 3 + rank
        return {"mkpts0_f": torch.rand(m, 2, generator=g), "mkpts1_f": torch.rand(m, 2, generator=g),
                "mconf": torch.rand(m, generator=g), "m_bids": torch.zeros(m, dtype=torch.int64)}

    who = [None] * world
    dist.all_gather_object(who, (rank, int(os.environ.get("LOCAL_RANK", "-1")), os.getpid()))
    dist.barrier()
    t0 = time.perf_counter()
    rows = [pack_matches(step(s), [(s * world + rank) * nb] * 1) for s in range(args.steps)]
    allrows = all_gather_matches(torch.cat(rows))
    dist.barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"selftest": True, "n_gpus": world, "steps": args.steps, "matches": int(allrows.shape[0]),
                          "expected_matches": args.steps * sum(3 + r for r in range(world)),
                          "ranks": [w[0] for w in who], "local_ranks": [w[1] for w in who],
                          "distinct_processes": len({w[2] for w in who}) == world, "ms_per_step": round(1e3 * float(t) / args.steps, 3)}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch(args, argv))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if args.selftest_launch:
        return selftest_worker(args, rank, world)
    # GIM_BENCH_DRY_MODEL=1 (tests/test_bench_launch_cpu.py): THIS function, line for line, on CPU ranks over gloo with a stand-in
    # model -- process group, core binding, timed loop, match packing, the all-gather, the max-over-ranks reduction and the JSON
    # line are the real ones.  Never set outside that test: the product path has no CPU mode.
    dry = os.environ.get("GIM_BENCH_DRY_MODEL") == "1"
    backend = os.environ.get("GIM_BENCH_BACKEND", "gloo" if dry else "nccl")
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if dry:
        dev = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench.py needs a HIP device (no CPU fallback in the product path)"
        assert torch.cuda.device_count() > local_rank, f"rank {rank}: LOCAL_RANK {local_rank} has no HIP device"
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group(backend, rank=rank, world_size=world, **({} if dry else {"device_id": dev}))
        assert dist.get_world_size() == world
        bind_rank_to_cores(local_rank, world)   # N ranks share one host: own core slice + thread cap per rank

    nb = args.batch
    over = {"coarse_sim": args.coarse_sim} if args.coarse_sim else {}
    if dry:
        ops = S = parity_vs_oracle = flip_margins = None
        sd_cpu = None

        class _DryModel:   # emits 3 + rank matches per pair; nothing else of the engine is exercised
            use_graph, coarse_sim, stem_fp16, stem_split = False, "dry", False, False

            def _split(self):
                return False

            def __call__(self, d):
                g = torch.Generator().manual_seed(7 + rank)
                m = (3 + rank) * nb
                d.update({"mkpts0_f": torch.rand(m, 2, generator=g), "mkpts1_f": torch.rand(m, 2, generator=g),
                          "mconf": torch.rand(m, generator=g), "m_bids": torch.arange(m) % nb, "b_ids": torch.arange(m) % nb})

        model = _DryModel()
        c0h = c1h = c0 = c1 = torch.zeros(nb, 3, 8, 8)
    else:
        from gim_amd import ops
        from tools import synth_loftr as S
        from tools.parity import flip_margins, parity_vs_oracle

        # seeded "trained-like" weights of the gim_loftr architecture (no checkpoint ships with the reference)
        model, sd_cpu = S.synthetic_model(args.precision, seed=0, **over)
        model = model.to(dev)
        c0h, c1h = S.textured_pairs(nb, H, W, seed=1234 + rank, frac=args.frac)
        c0, c1 = c0h.to(dev), c1h.to(dev)

    def step(a=None, b=None):
        a = c0 if a is None else a
        b = c1 if b is None else b
        d = {"image0": a[:, :1], "image1": b[:, :1], "color0": a, "color1": b}
        model(d)
        return d

    def dev_sync():
        if not dry:
            torch.cuda.synchronize()

    def sync_all():
        dev_sync()
        if world > 1:
            dist.barrier()
            dev_sync()

    # which device every rank really sits on, as the process group saw it (the driver's SCALE record can check RCCL saw N ranks)
    rank_devices = [f"{dev.type}:{torch.cuda.current_device()}" if not dry else f"cpu:pid{os.getpid()}"]
    if world > 1:
        got = [None] * world
        dist.all_gather_object(got, rank_devices[0])
        rank_devices = got
    n_ranks_seen = dist.get_world_size() if world > 1 else 1

    for w_ in range(max(2, args.warmup)):  # the COMPLETE step, incl. match packing; the 2nd call captures the HIP graph
        pack_matches(step(), 0)
    all_gather_matches(torch.zeros(1, 6, device=dev))
    # the outputs are read back inside the timed region -- the packed [pair, x0, y0, x1, y1, conf] rows (~270 KB per step) travel to
    # pinned host memory asynchronously behind the step that produced them; sync_all() below waits for the last copy.  The pinned slots
    # (capacity = every coarse cell of every pair a match) are allocated HERE, outside the timed region: hipHostMalloc is not part of a step
    host_cap = nb * (H // 8) * (W // 8)
    host_ring = None if dry else torch.empty(args.steps, host_cap, 6, dtype=torch.float32, pin_memory=True)
    sync_all()
    t0 = time.perf_counter()
    rows = []
    rows_host = []
    tstep = []
    for s in range(args.steps):
        d = step()
        rows.append(pack_matches(d, (s * world + rank) * nb))   # consecutive pair ids of this batch, packed on the device
        if not dry:
            rows_host.append(host_ring[s, :rows[-1].shape[0]])
            rows_host[-1].copy_(rows[-1], non_blocking=True)
        tstep.append(time.perf_counter())
    allrows = all_gather_matches(torch.cat(rows))  # the one collective: matches, for reporting
    n_matches = int(allrows.shape[0])
    sync_all()
    dt = time.perf_counter() - t0
    readback_bytes = sum(r.numel() * 4 for r in rows_host)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    d_last = d
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, d_last, rows[-1], "" if rank == 0 else f"rank{rank}_")
    # the extra measurements below run with --full only (a plain run reports them as null), all but the roofline in single-GPU jobs only
    full = args.full and rank == 0 and not dry
    solo = full and world == 1

    # ---- live roofline of the dominant kernel (instrumented steps outside the timed region) --------
    roof = None
    if full:
        graph_was, model.use_graph = model.use_graph, False  # events need eager launches
        # ... and one stream: the timed configuration runs the coarse transformer as pair chains on parallel streams (loftr.py: tf_chains),
        # where the event pairs of concurrent launches overlap; the per-kernel table below is taken with ONE chain (12 token launches per
        # step instead of 32 shorter ones) -- the implicit-GEMM launches (`achieved`) are the same launches either way
        # Since round 6 layer 3 runs as two image chains too (loftr.py: l3_chains): an as-run pass first (its per-launch durations are what
        # rocprofv3 sees for the same command: `as_run` below), then the single-stream pass every figure of the block is taken from
        # (layer 3 as ONE launch per convolution, every launch alone on the chip -- the definition of rounds 1-5).
        chains_was, model.tf_chains = getattr(model, "tf_chains", 1), 1
        l3_was = getattr(model, "l3_chains", 1)
        as_run = None
        if l3_was > 1:
            step()
            ops.PROFILE, ops.PROFILE_FUSED = [], []
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            prof_c, ops.PROFILE = ops.PROFILE, None
            ops.PROFILE_FUSED = None
            ms_c, fl_c = sum(e0.elapsed_time(e1) for e0, e1, _, _ in prof_c), sum(f for _, _, f, _ in prof_c)
            as_run = {"l3_chains": l3_was, "launches_per_step": len(prof_c) // 2, "avg_launch_us": round(1e3 * ms_c / len(prof_c), 2),
                      "achieved": round(fl_c / (ms_c * 1e-3) / 1e12, 2), "frac": round(fl_c / (ms_c * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[args.precision], 4),
                      "note": "the same launches as the timed steps issue them: layer 3's convolutions as two half-batch launches on parallel streams, "
                              "each sharing the chip with the other chain's kernels -- its event pairs overlap, so the sum of durations exceeds the "
                              "time the launches occupy (the step is 0.23 ms SHORTER this way: DESIGN.md section 4); this is the average a "
                              "rocprofv3 --kernel-trace of the bench command sees (profiles/r06_kernel_stats.txt)"}
            model.l3_chains = 1   # (read per eager forward; the captured graph of the timed steps keeps its two chains)
        step()
        ops.PROFILE, ops.PROFILE_FUSED = [], []
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        prof, ops.PROFILE = ops.PROFILE, None
        fprof, ops.PROFILE_FUSED = ops.PROFILE_FUSED, None
        model.use_graph, model.tf_chains = graph_was, chains_was
        if l3_was > 1:
            model.l3_chains = l3_was
        fam = {}
        for e0, e1, f, name in fprof:
            ms, fl, n = fam.get(name, (0.0, 0.0, 0))
            fam[name] = (ms + e0.elapsed_time(e1), fl + f, n + 1)
        fused = {k: {"launches_per_step": v[2] // 2, "ms_per_step": round(v[0] / 2, 3), "tflops": round(v[1] / (v[0] * 1e-3) / 1e12, 1)}
                 for k, v in fam.items()}
        # the coarse matching call (dual-softmax statistics over the [4800 x 4800] similarity GEMM of every pair + selection):
        # its statistics kernel is the step's second-largest; priced as the GEMM it computes against the dense MFMA peak
        cg = fused.pop("coarse_match", None)
        coarse_gemm = None
        if cg:
            v = fam["coarse_match"]
            coarse_gemm = {"us": round(1e3 * v[0] / v[2], 1), "tflops": cg["tflops"],
                           "frac": round(cg["tflops"] / MFMA_PEAK_TFLOPS[args.precision], 4),
                           "what": "whole gim_coarse_match call (init + statistics + combine + selection + emit kernels; the "
                                   "statistics kernel is ~80 % of it: profiles/r04_cm_stats.txt)"}
        tot_ms = sum(e0.elapsed_time(e1) for e0, e1, _, _ in prof)
        tot_fl = sum(f for _, _, f, _ in prof)
        nlaunch = len(prof)
        achieved = tot_fl / (tot_ms * 1e-3) / 1e12
        peak = MFMA_PEAK_TFLOPS[args.precision]
        by = {}
        for e0, e1, f, lab in prof:
            ms, fl = by.get(lab, (0.0, 0.0))
            by[lab] = (ms + e0.elapsed_time(e1), fl + f)
        top = sorted(by.items(), key=lambda kv: -kv[1][0])[:8]
        # HBM bytes per launch from the TCC counters (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE), collected in
        # separate rocprofv3 --pmc passes of the same workload by tools/pmc_traffic.sh and committed under profiles/
        traffic = traffic_source = None
        if args.precision in ("bf16", "fp16") and nb == 8 and os.path.exists(TRAFFIC_JSON):   # same kernels, same bytes in both 16-bit flavours
            tj = json.load(open(TRAFFIC_JSON))
            # per launch of THIS pass: the PMC passes count the as-run launches (layer 3 as two chains: 25 per forward), `achieved` the 18
            # single-stream ones -- the same bytes per forward either way
            traffic = round(tj["traffic_bytes_per_launch"] * tj["igemm_launches"] / 3 / (nlaunch // 2)) if tj.get("igemm_launches") else round(tj["traffic_bytes_per_launch"])
            traffic_source = (os.path.relpath(TRAFFIC_JSON, ROOT) + ": separate rocprofv3 --pmc passes (TCC FETCH_SIZE x2 gfx950 correction, WRITE_SIZE) of this "
                              "workload by tools/pmc_traffic.sh, committed per round -- NOT collected in this run")
        roof = {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": traffic_source,
                "kernel": "gim_conv2d_bn_act kernels (igemm_persistent_kernel + conv3x3_halo_kernel)", "launches_per_step": nlaunch // 2,
                "avg_launch_us": round(1e3 * tot_ms / nlaunch, 2),
                "gflop_per_launch": round(tot_fl / nlaunch / 1e9, 3),
                "kernel_ms_per_step": round(tot_ms / 2, 3),
                "as_run": as_run,
                "coarse_gemm": coarse_gemm,
                "fused_kernels": fused,   # the hand-fused kernels that took work OUT of the implicit-GEMM kernel (same live HIP-event timing)
                "top_layers_ms_tflops": [[k, round(v[0] / 2, 3), round(v[1] / (v[0] * 1e-3) / 1e12, 1)] for k, v in top]}
        if os.environ.get("GIM_BENCH_ALL_LAYERS"):   # every conv / linear shape: [label, launches per step, ms per step, TFLOP/s]
            cnt = {}
            for _, _, _, lab in prof:
                cnt[lab] = cnt.get(lab, 0) + 1
            roof["all_layers"] = [[k, cnt[k] // 2, round(v[0] / 2, 3), round(v[1] / (v[0] * 1e-3) / 1e12, 1)]
                                  for k, v in sorted(by.items(), key=lambda kv: -kv[1][0])]

    # ---- the same step with the images starting in (pinned) host memory: PCIe-inclusive rate -------------
    # double-buffered staging on a copy stream (gim_amd.runner.HostPairFeeder): the transfer of step s + 1 overlaps step s
    h2d = None
    if solo:
        p0, p1 = c0h.pin_memory(), c1h.pin_memory()
        feeder = HostPairFeeder(dev)

        def h2d_run(n):
            feeder.put([p0, p1])
            for i in range(n):
                a, b = feeder.get()
                if i + 1 < n:
                    feeder.put([p0, p1])
                step(a, b)
                feeder.done()
            torch.cuda.synchronize()

        h2d_run(3)
        n_h, th = 10, None
        for _ in range(3):        # best of three runs of ten steps: a single host hiccup inside ten steps was 40 % of the figure
            t0 = time.perf_counter()
            h2d_run(n_h)
            t0 = (time.perf_counter() - t0) / n_h
            th = t0 if th is None else min(th, t0)
        for _ in range(2):
            step(p0.to(dev, non_blocking=True), p1.to(dev, non_blocking=True))
        torch.cuda.synchronize()
        ts = None
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(5):
                step(p0.to(dev, non_blocking=True), p1.to(dev, non_blocking=True))
            torch.cuda.synchronize()
            t0 = (time.perf_counter() - t0) / 5
            ts = t0 if ts is None else min(ts, t0)
        h2d = {"pairs_per_s": round(nb / th, 2), "ms_per_step": round(1e3 * th, 3),
               "serial_copy_ms_per_step": round(1e3 * ts, 3),
               "note": f"{2 * c0h.numel() * 4 / 1e6:.0f} MB of fp32 NCHW images per step from pinned host memory, double-buffered on a "
                       "copy stream so that the transfer of step s+1 overlaps the kernels of step s (incl. the first, exposed copy); best of "
                       "three runs of ten steps; "
                       "serial_copy = the same copies issued on the compute stream (round 2's figure)"}

    # ---- the other precision modes on the same workload and batch, timed the same way -----------------------------------------
    #   parity_mode: precision='fp32' (fp32 storage; products as fp16 hi / lo pairs since round 6, exact fp32 MFMA products as `exact_products`) -- the mode whose
    #                match indices equal the oracle's
    #   bf16_mode / fp16_mode: the OTHER 16-bit flavour of the same kernels (same MFMA rate, same bytes): bf16 has fp32's exponent
    #                range and 8 significand bits per stored activation, fp16 has 11 (a quarter of bf16's index flips)
    alt_modes = {}
    if solo and args.precision in ("bf16", "fp16") and not os.environ.get("GIM_BENCH_SKIP_PARITY_MODE"):
        other = {"fp16": ("bf16_mode", "bf16", "the same kernels in their bf16 flavour (v_mfma_f32_32x32x16_bf16; the first convolution "
                                               "still reads fp16 operands): same instruction counts and bytes, fp32's exponent range, "
                                               "8 instead of 11 significand bits per stored activation"),
                 "bf16": ("fp16_mode", "fp16", "the same kernels in their IEEE fp16 flavour (v_mfma_f32_32x32x16_f16, v_cvt_pk_f16_f32): same "
                                               "instruction counts and bytes, |activation| < 65504")}[args.precision]
        for name, prec, n_alt, note in (
                ("parity_mode", "fp32", 5, "every GEMM on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32)"),   # (note replaced below when the mode runs split products)
                (other[0], other[1], args.steps, other[2])):
            model.set_precision(prec)
            for _ in range(3):
                da = step()
            torch.cuda.synchronize()
            ta = time.perf_counter()
            for _ in range(n_alt):
                da = step()
            torch.cuda.synchronize()
            ta = (time.perf_counter() - ta) / n_alt
            alt_modes[name] = ({"precision": prec, "pairs_per_s": round(nb / ta, 2), "ms_per_step": round(1e3 * ta, 3), "steps": n_alt,
                                "matches_per_pair": round(da["b_ids"].numel() / nb, 1), "note": "same workload and batch; " + note},
                               {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in da.items() if k != "conf_matrix"})
            if prec == "fp32" and getattr(model, "fp32_split", False):
                # the cross-check: the same mode with every product on v_mfma_f32_32x32x2_f32 (exact fp32 products) instead of fp16 hi / lo pairs
                model.fp32_split = False
                for _ in range(2):
                    dx = step()
                torch.cuda.synchronize()
                tx = time.perf_counter()
                for _ in range(3):
                    dx = step()
                torch.cuda.synchronize()
                tx = (time.perf_counter() - tx) / 3
                model.fp32_split = True
                alt_modes[name][0]["note"] = ("same workload and batch; fp32 storage, the fp32 operands of every GEMM split in registers into IEEE-fp16 hi / lo pairs and "
                                              "multiplied as hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation (gim_conv_args.split16, round 6: "
                                              "2^-22 per product, tests/test_gpu_split16.py); `exact_products` = the same mode on v_mfma_f32_32x32x2_f32")
                alt_modes[name + ".exact_products"] = ({"pairs_per_s": round(nb / tx, 2), "ms_per_step": round(1e3 * tx, 3), "steps": 3},
                                                       {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in dx.items() if k != "conf_matrix"})
        model.set_precision(args.precision, args.coarse_sim)
        torch.cuda.empty_cache()

    # ---- the fine level idle (random-init weights, uniform-noise images: what round 1 reported) ----------
    idle = None
    if solo:
        from gim_amd.loftr import LoFTR, get_cfg_defaults, lower_config
        torch.manual_seed(0)
        cfg = lower_config(get_cfg_defaults())["loftr"]
        cfg["precision"] = args.precision
        cfg.update(over)
        m0 = LoFTR(cfg).eval().to(dev)
        g = torch.Generator().manual_seed(1234)
        u0, u1 = torch.rand(nb, 3, H, W, generator=g).to(dev), torch.rand(nb, 3, H, W, generator=g).to(dev)

        def idle_step():
            dd = {"image0": u0[:, :1], "image1": u1[:, :1], "color0": u0, "color1": u1}
            m0(dd)
            return dd

        for _ in range(3):
            dd = idle_step()
        torch.cuda.synchronize()
        ti = time.perf_counter()
        for _ in range(10):
            dd = idle_step()
        torch.cuda.synchronize()
        ti = (time.perf_counter() - ti) / 10
        idle = {"pairs_per_s": round(nb / ti, 2), "ms_per_step": round(1e3 * ti, 3),
                "matches_per_pair": round(dd["b_ids"].numel() / nb, 2),
                "note": "random-init weights + uniform-noise images: ~1 match per pair, fine level idle (round-1 headline)"}
        del m0, u0, u1
        torch.cuda.empty_cache()

    # HBM bytes per call of the secondary engines: per-round PMC passes (tools/pmc_secondary.sh), committed under profiles/ -- NOT collected in this run
    sec_tr = json.load(open(SEC_TRAFFIC_JSON))["engines"] if SEC_TRAFFIC_JSON else {}
    sec_traffic_src = (f" ({os.path.relpath(SEC_TRAFFIC_JSON, ROOT)}: separate rocprofv3 --pmc passes, FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, bf16 mode)" if SEC_TRAFFIC_JSON
                       else " (no PMC pass on file)")

    def sec_traffic(key):
        return sec_tr.get(key, {}).get("hbm_bytes_per_call")

    # ---- secondary workload (reported, not the metric): gim_lightglue at the same resolution / batch ---------
    sec_prec = "fp32" if args.precision == "fp32" else "bf16"   # the secondary engines have a bf16 and an fp32 mode
    lightglue = None
    if solo and not os.environ.get("GIM_BENCH_SKIP_LIGHTGLUE"):
        from gim_amd.lightglue import LightGlue, SuperPoint, gim_lightglue_inference
        torch.manual_seed(0)  # random-init weights of the reference architecture (no checkpoint in the container)
        det = SuperPoint({"max_num_keypoints": 2048, "force_num_keypoints": True, "detection_threshold": 0.0,
                          "nms_radius": 3, "trainable": False, "precision": sec_prec}).eval()
        lgm = LightGlue({"filter_threshold": 0.1, "flash": False, "checkpointed": True, "precision": sec_prec}).eval()
        gg = torch.Generator().manual_seed(1)
        g0 = torch.nn.functional.interpolate(torch.rand(nb, 1, H // 4, W // 4, generator=gg), size=(H, W), mode="bilinear")
        g0 = (0.7 * g0 + 0.3 * torch.rand(nb, 1, H, W, generator=gg)).contiguous().to(dev)  # textured synthetic images
        g1 = torch.roll(g0, shifts=(16, 24), dims=(2, 3)).contiguous()
        rs = torch.tensor([[H, W]] * nb, device=dev)
        one = torch.ones(nb, 2, device=dev)

        def lg_step():
            dd = {"image0": g0, "image1": g1, "resize0": rs, "resize1": rs, "scale0": one, "scale1": one}
            gim_lightglue_inference(det, lgm, dd)
            return dd["mconf"].shape[0]

        for _ in range(2):
            lg_step()
        torch.cuda.synchronize()
        tl = time.perf_counter()
        for _ in range(10):
            lg_step()
        torch.cuda.synchronize()
        tl = (time.perf_counter() - tl) / 10
        lightglue = {"workload": f"gim_lightglue {W}x{H}, batch {nb} pairs, SuperPoint (2048 keypoints) x2 + LightGlue "
                                 "(9 layers) + adapter, random-init weights", "pairs_per_s": round(nb / tl, 2),
                     "ms_per_step": round(1e3 * tl, 3), "dtype": sec_prec,
                     "achieved_tflops": round(nb / tl * 334e9 / 1e12, 1),
                     "note": "algorithmic 334 GFLOP/pair (SURVEY 8d)"}
        lg_ach = nb / tl * 334e9 / 1e12
        lightglue["roofline"] = {"bound": "mfma", "achieved": round(lg_ach, 1), "peak": MFMA_PEAK_TFLOPS[sec_prec], "unit": "TFLOP/s",
                                 "frac": round(lg_ach / MFMA_PEAK_TFLOPS[sec_prec], 4), "traffic": sec_traffic("lightglue"),
                                 "what": "334 GFLOP per pair (SURVEY 8d) x pairs per step / step time, whole pipeline (SuperPoint x 2, LightGlue, adapter, two read-backs); "
                                         "traffic = HBM bytes per batch-8 step" + sec_traffic_src}
        del det, lgm

    # ---- secondary workloads: the two dense matchers at the reference's own configurations (one pair per call) ----
    dense = {}
    if solo and not os.environ.get("GIM_BENCH_SKIP_DENSE"):
        gg = torch.Generator().manual_seed(1)
        base = torch.nn.functional.interpolate(torch.rand(1, 3, 60, 80, generator=gg), size=(480, 640), mode="bicubic").clamp(0.05, 1)
        im0 = base.to(dev)
        im1 = torch.roll(base, shifts=(12, 20), dims=(2, 3)).to(dev)

        def dense_bench(name, build, note, batch=1, tflop_per_pair=None, parity_note=None, traffic_key=None, prec16="bf16"):
            p16 = sec_prec if sec_prec == "fp32" else prec16   # the engine's default 16-bit mode (gim_dkm: bf16, gim_roma: fp16 since round 6)
            try:
                def make(prec):
                    torch.manual_seed(0)
                    mm = build(prec).eval()
                    with torch.no_grad():   # random init; refiner outputs scaled down so the flow stays in range (what trained weights do)
                        for s_ in ("16", "8", "4", "2", "1"):
                            mm.decoder.conv_refiner[s_].out_conv.weight.mul_(0.05)
                            mm.decoder.conv_refiner[s_].out_conv.bias.mul_(0.05)
                    return mm

                m = make(p16)
                for _ in range(2):
                    warp, cert = m.match(im0, im1)
                    m.sample(warp, cert, 5000)
                torch.cuda.synchronize()
                n_it = 5
                td = time.perf_counter()
                for _ in range(n_it):
                    warp, cert = m.match(im0, im1)
                torch.cuda.synchronize()
                t_match = (time.perf_counter() - td) / n_it
                td = time.perf_counter()
                for _ in range(n_it):
                    m.sample(warp, cert, 5000)
                torch.cuda.synchronize()
                t_sample = (time.perf_counter() - td) / n_it
                dense[name] = {"workload": note, "pairs_per_s": round(1.0 / (t_match + t_sample), 2),
                               "match_ms": round(1e3 * t_match, 2), "sample_ms": round(1e3 * t_sample, 2), "dtype": p16}
                if tflop_per_pair:   # SURVEY 8d's algorithmic work of one match() (low-resolution + upsampling pass) against the dense 16-bit MFMA peak
                    ach = tflop_per_pair / t_match
                    dense[name]["roofline"] = {"bound": "mfma", "achieved": round(ach, 1), "peak": MFMA_PEAK_TFLOPS[p16], "unit": "TFLOP/s",
                                               "frac": round(ach / MFMA_PEAK_TFLOPS[p16], 4), "traffic": sec_traffic(traffic_key),
                                               "what": f"{tflop_per_pair} TFLOP per match() (SURVEY 8d, BASELINE.md section 2) / match_ms; traffic = HBM bytes per match()" + sec_traffic_src}
                if parity_note:
                    dense[name]["parity_note"] = parity_note
                if batch > 1:   # BASELINE's batched configuration: `batch` independent pairs in one engine pass (match_batch)
                    b0, b1 = im0.expand(batch, -1, -1, -1).contiguous(), im1.expand(batch, -1, -1, -1).contiguous()
                    for _ in range(2):
                        wb, cb = m.match_batch(b0, b1)
                    torch.cuda.synchronize()
                    td = time.perf_counter()
                    for _ in range(3):
                        wb, cb = m.match_batch(b0, b1)
                    torch.cuda.synchronize()
                    t_b = (time.perf_counter() - td) / 3
                    dense[name].update({f"batch{batch}_match_ms_per_pair": round(1e3 * t_b / batch, 2),
                                        f"batch{batch}_pairs_per_s": round(batch / (t_b + batch * t_sample), 2)})
                    del wb, cb
                if p16 != "fp32":   # the same engine in its OTHER 16-bit flavour (fp16: 11 instead of 8 significand bits per stored activation)
                    o16 = "fp16" if p16 == "bf16" else "bf16"
                    w16, c16 = warp.float().clone(), cert.float().clone()
                    del m
                    torch.cuda.empty_cache()
                    m = make(o16)
                    for _ in range(3):   # (the first calls of a new module build its per-shape tables on the host)
                        wf, cf = m.match(im0, im1)
                    torch.cuda.synchronize()
                    td = time.perf_counter()
                    for _ in range(n_it):
                        wf, cf = m.match(im0, im1)
                    torch.cuda.synchronize()
                    dense[name][o16 + "_mode"] = {"match_ms": round(1e3 * (time.perf_counter() - td) / n_it, 2), "finite": bool(torch.isfinite(wf).all() and torch.isfinite(cf).all()),
                                                "mean_abs_dwarp_vs_timed_mode": round(float((wf.float() - w16).abs().mean()), 5),
                                                "note": "same random-init weights and pair; tests/test_gpu_dkm.py / test_gpu_roma.py::test_match_fp16_is_closer_than_bf16 hold its distance "
                                                        "from the fp32 oracle against the bf16 mode's"}
                    del wf, cf, w16, c16
                del m
                torch.cuda.empty_cache()
            except Exception as e:  # a secondary line must never cost the headline measurement
                dense[name] = {"error": f"{type(e).__name__}: {e}"[:300]}

        def build_dkm(prec):
            from gim_amd.dkm import DKMv3
            m = DKMv3(None, 672, 896, upsample_preds=True, precision=prec)
            m.upsample_res = (1152, 1536)
            return m

        def build_roma(size):
            def f(prec):
                from gim_amd.roma import RoMa, random_dinov2_weights
                return RoMa([size], precision=prec, dinov2_weights=random_dinov2_weights(dev))
            return f

        dense_bench("gim_dkm", build_dkm, "gim_dkm match() + sample(5000), 672x896 -> upsampling pass 1152x1536, one pair per call, "
                    "random-init weights (trainer/lightning.py:29-37 configuration)", batch=4, tflop_per_pair=5.27, traffic_key="dkm",
                    parity_note="fp32 mode at 672x896 (tests/test_gpu_dense_fullsize.py, profiles/r03_dense_parity.txt): warp max 2.9e-4 / mean 2.5e-5 of scale "
                                "from the reference's PINNED fp32 arithmetic -- the distance that arithmetic's own fp32 GP inverse keeps from its formula "
                                "(condition number ~2e4) -- and max 3.0e-6 from the same oracle with only the GP step in fp64; the timed bf16 mode: mean |d warp| "
                                "~0.009 (tests/test_gpu_dkm.py)")
        dense_bench("gim_roma", build_roma(672), "gim_roma match() + sample(5000), 672x672 -> upsampling pass 1344x1344, one pair per call, "
                    "random-init weights incl. a synthetic DINOv2 ViT-L/14 (RoMa(img_size=[672]), trainer/lightning.py:38-41)", tflop_per_pair=14.44, traffic_key="roma672", prec16="fp16",
                    parity_note="fp32 mode at 672x672: 99.75 % of the warp values within 2e-3 of the reference's pinned fp32 arithmetic (the rest: anchor arg-max "
                                "decisions its own GP noise flips), max 3.6e-7 from the oracle with the GP step in fp64 (profiles/r03_dense_parity.txt)")
        dense_bench("gim_roma_560", build_roma(560), "gim_roma match() + sample(5000), 560x560 -> upsampling pass 1344x1344 (BASELINE config 4: RoMa(img_size=[560]); "
                    "roma.py:658 fixes upsample_res = 1344 x 1344 whatever img_size), one pair per call per GPU, random-init weights", tflop_per_pair=10.03, traffic_key="roma560", prec16="fp16",
                    parity_note="fp32 mode at 560x560 and through the 1344x1344 upsampling pass (tests/test_gpu_dense_fullsize.py::test_roma_560_*): every value within 2e-5 of scale of the "
                                "oracle with the GP step in fp64; the timed mode is the engine's default 16-bit mode")

    # ---- CPU baseline: the oracle on this host's cores, bounded sample; parity of the benchmarked engine ----
    cpu = None
    parity = None
    if solo and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import loftr_oracle as O
        # torch's CPU kernels oversubscribe badly on a 256-thread host (119.9 s per pair with all hardware threads): use at
        # most 64 threads unless told otherwise; `cores` reports what was actually used
        ncore = min(os.cpu_count() or 1, int(os.environ.get("GIM_CPU_THREADS", "64")))
        torch.set_num_threads(ncore)
        n = args.cpu_pairs
        cc0, cc1 = c0h[:n], c1h[:n]

        def cpu_forward():
            with torch.no_grad():
                return O.loftr_forward(sd_cpu, {"image0": cc0[:, :1], "image1": cc1[:, :1], "color0": cc0, "color1": cc1})

        n_timed = int(os.environ.get("GIM_CPU_REPEATS", "3"))
        cpu_forward()  # warm-up
        tcs = []
        for _ in range(n_timed):
            tc = time.perf_counter()
            ref = cpu_forward()
            tcs.append(time.perf_counter() - tc)
        tc = sum(tcs) / len(tcs)
        cpu = {"value": round(n / tc, 5), "unit": "pairs/s", "cores": ncore, "kind": "port",
               "port_of": "networks/loftr/loftr.py:43-91 LoFTR.forward -- oracle/loftr_oracle.py, pinned to the reference's own outputs "
                          "(0.0 ... 4e-7 apart on every stage, tests/golden); /root/reference does not exist on the GPU box",
               "sample": f"{n} pair(s) 640x480 fp32 (pair 0 of the benchmarked batch), oracle/loftr_oracle.py on torch CPU with "
                         f"{ncore} threads, 1 warm-up + {n_timed} timed forwards, {tc:.2f} s each "
                         f"(min {min(tcs):.2f}, max {max(tcs):.2f})"}
        if n == 1:
            parity = parity_vs_oracle(d_last, ref, 0)
            # every index flip priced by the ORACLE's own margin: distance of its confidence from thr = 0.2 and from the runner-up of its row /
            # column (a flip is "marginal" when the oracle's decision itself hangs on < 0.05 of confidence: 16-bit storage moves mconf by ~0.01)
            fm = flip_margins(d_last, ref, 0, 0)
            parity["flips"] = len(fm)
            parity["flips_all_marginal"] = all(min(f[4], abs(f[5])) < 0.05 for f in fm)
            if fm:
                worst = max(fm, key=lambda f: min(f[4], abs(f[5])))
                parity["worst_flip"] = {"i": worst[0], "j": worst[1], "in_oracle": bool(worst[2]), "oracle_conf": round(worst[3], 5),
                                        "margin_to_thr": round(worst[4], 5), "gap_to_runner_up": round(worst[5], 5)}
            parity["note"] = (f"pair 0 of the timed batch: {args.precision} engine (coarse_sim={model.coarse_sim}) vs the fp32 CPU "
                              "oracle; flip_rate = |engine matches XOR oracle matches| / |oracle matches|")
            if args.precision in ("bf16", "fp16"):   # the same batch with the other similarity setting: is the operand rounding visible?
                was = model.coarse_sim
                model.coarse_sim = "fp32" if was == args.precision else args.precision
                alt = parity_vs_oracle(step(), ref, 0)
                parity["other_coarse_sim"] = {"coarse_sim": model.coarse_sim, "flip_rate": alt["flip_rate"],
                                              "mean_abs_dmconf": alt.get("mean_abs_dmconf"), "mean_abs_dmkpts1_px": alt.get("mean_abs_dmkpts1_px")}
                model.coarse_sim = was
                # what the split-operand first convolution buys (or would buy): the same batch with the other setting of the stem
                # (fp16 mode: split by default, `plain_stem` = round 3's mode; bf16 mode: plain by default since round 5, `split_stem`)
                was_split, split_now = model.stem_split, model._split()
                model.stem_split = not split_now
                model._invalidate()
                alt = parity_vs_oracle(step(), ref, 0)
                parity["plain_stem" if split_now else "split_stem"] = {k: alt.get(k) for k in ("flip_rate", "mean_abs_dmconf", "max_abs_dmconf", "mean_abs_dmkpts1_px")}
                model.stem_split = was_split
                model._invalidate()
            for nm, (rec, d_alt) in alt_modes.items():
                rec["parity"] = parity_vs_oracle(d_alt, ref, 0)
    if "parity_mode.exact_products" in alt_modes:
        alt_modes["parity_mode"][0]["exact_products"] = alt_modes.pop("parity_mode.exact_products")[0]

    if rank == 0 and os.environ.get("GIM_BENCH_DEBUG"):
        print("per-step ms:", [round(1e3 * (b - a), 2) for a, b in zip([t0] + tstep[:-1], tstep)], file=sys.stderr)
    if rank == 0:
        pairs = world * nb * args.steps
        if roof is not None:
            # the whole path priced the same way: SURVEY 8d's algorithmic work (0.7135 TFLOP per pair + 33.6 MFLOP per match) over the timed steps
            wf = (0.7135e12 * pairs + 33.6e6 * n_matches) / world
            roof["whole_step"] = {"tflops": round(wf / dt / 1e12, 1), "frac": round(wf / dt / 1e12 / MFMA_PEAK_TFLOPS[args.precision], 4),
                                  "what": "all kernels of a rank's steps: (0.7135 TFLOP x pairs + 33.6 MFLOP x matches) / time, against the same peak"}
        out = {
            "metric": "image-pairs/sec at 640x480", "value": round(pairs / dt, 2), "unit": "pairs/s",
            "n_gpus": world, "n_ranks_seen": n_ranks_seen, "rank_devices": rank_devices, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak", "full": bool(args.full),
            "vs_baseline": None, "dtype": getattr(model, "precision", args.precision), "data": "synthetic",
            # what the module really ran as: a tripped fp16 range guard switches it to bf16 for good (gim_amd/loftr/loftr.py::_range_guard)
            "engine_precision": getattr(model, "precision", args.precision), "fp16_overflowed": bool(getattr(model, "fp16_overflowed", False)),
            "config": {"workload": f"gim_loftr {W}x{H}, batch {nb} pairs per GPU per step, seeded trained-like weights "
                                   f"(calibrated BatchNorm statistics), textured image pairs with {args.frac:.2f} of the frame "
                                   "in correspondence (device resident), fine level loaded, outputs incl. match count read back",
                       "pairs_per_step": world * nb, "matches_per_pair": round(n_matches / max(1, pairs), 1),
                       "coarse_sim": model.coarse_sim, "stem_operands": ("fp16" if (args.precision == "bf16" and model.stem_fp16) else args.precision) +
                                        (" hi+lo pairs (split-operand first convolution)" if model._split() else ""),
                       "parallelism": f"pairs sharded over {world} GPU(s), no collective per step",
                       "hip_graph": bool(model.use_graph), "transformer_pair_chains": int(getattr(model, "tf_chains", 1)),
                       "transformer_rows": {k: bool(getattr(model, k, False)) for k in ("q_local", "kv_fused", "kv_init")},
                       "readback": f"match count every step (host sync) + the packed match rows, {readback_bytes // max(1, args.steps)} B per step, to pinned host "
                                   "memory inside the timed region",
                       "baseline_dtype_note": "BASELINE config 2 names bf16 (round 5's headline, `bf16_mode` here: 4-5 % faster, but 1 % index flips with max |d mconf| 0.2 "
                                              "against the fp32 oracle -- VERDICT r5: parity first).  Round 6 headlines the 16-bit mode that keeps the parity bar "
                                              "(IEEE fp16 operands, 11 instead of 8 significand bits per stored activation, fp32 accumulation, range guard with a bf16 "
                                              "fallback): same kernels, same bytes, same instruction counts"},
            "roofline": roof, "cpu_baseline": cpu, "parity": parity, "parity_mode": alt_modes.get("parity_mode", (None,))[0],
            "fp16_mode": alt_modes.get("fp16_mode", (None,))[0], "bf16_mode": alt_modes.get("bf16_mode", (None,))[0], "h2d_inclusive": h2d, "fine_idle": idle,
            "secondary_workloads": {"gim_lightglue": lightglue, **dense},
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()      # rank 0 is still measuring / printing: leave the group together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
