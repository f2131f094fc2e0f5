#!/usr/bin/env python
"""bench.py — BASELINE.json's metric on MI355X: 15-channel grasp candidates generated +
scored per second (grasp-image generation + LeNet), N GPUs of one node.

Default (--mode replay), the headline: a step = one pass of the hot path (image generation + LeNet
scoring) over the candidate batch of one synthetic cloud; candidates, neighbourhoods and weights are
already resident in HBM when the timed region starts.  Workload = BASELINE.json configs[1]: a single
30k-point synthetic cloud, its first 5000 valid candidates, 15 channels.  With N > 1 every rank owns
its own cloud (cloud_id = rank): no data-path collective, weak scaling; torch.distributed (RCCL) is
used for the barrier and the max-over-ranks time only.  The same line also carries, measured after the
timed region: `detect_end_to_end` (one gpd_hip_detect call, host buffers in and out) and
`batch_end_to_end` (gpd_hip_detect_batch over a few clouds per rank: upload + search + filter + images +
LeNet + records back, two clouds in flight) — the product path, whole job over all ranks.

--config {2,2o,3a,3b,4} selects the other single-GPU BASELINE configs (3a/3b: 3 / 12 channels on the same
cloud, 4: 300k-point clutter cloud, 50000 candidates; 2o: configs[1]'s cloud with sensor-like, off-lattice coordinates).

--mode batch: BASELINE configs[4] end to end — `--clouds` synthetic 30k-point clouds (default 256), cloud i ->
rank i mod N, every cloud uploaded, searched, imaged, scored and its candidates returned to the host
(gpd_hip_detect_batch); a step = one pass over the rank's clouds; value = candidates of all ranks / time.

Prints ONE JSON line (rank 0).  Extra objects: "roofline" (dominant kernel), "kernels"
(both stages), "cpu_baseline" (the CPU oracle on a bounded sample, all host cores — and, where oracle/_ref is in the
tree, the reference's own sources timed on a few samples of the same list, one core, in a child process).

A plain run sets up, warms up, times the steps and prints the line (value, ms_per_step, the per-kernel HIP-event times of the
timed steps and the roofline made of them).  --full adds everything that takes runs of its own: in replay mode the search stage
timed alone, `detect_end_to_end`, the batch legs, the score-accuracy leg, `preprocess` and `cpu_baseline` (and --live-pmc).

--dump-outputs DIR: after the timed steps, what the timed path returned in its last step, as DIR/<name>.npy (rank 0; float32 /
float64, at most 64 MB: a fixed seeded sample of the rows beyond that).  Replay mode: scores.npy (the candidate list's scores, in
list order).  Batch mode: the scored hand records of the last pass, field by field, and per-cloud counts.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
F32_PEAK_TFLOPS = 157.3      # f32 vector == f32-input MFMA peak
BF16_PEAK_TFLOPS = 2500.0    # dense bf16 MFMA (MI355X_MICROARCH.md: ~2.5 PF dense; 16x16x32 measured 2075, 32x32x16 2382)
I8_PEAK_TOPS = 5000.0        # dense int8 MFMA (= the fp8 rate; 16x16x64 measured 3944, 32x32x32 4404)
LDS_PEAK_GBS = 256 * 128 * 2.4  # 256 CUs x 128 B/clk (ds_read_b32 rate; 256 B/clk for b64/b128) x 2.4 GHz (MI355X_MICROARCH.md §LDS)
LENET_MFLOP = {15: 83.04, 12: 73.63, 3: 45.41, 1: 39.14}  # SURVEY.md §8d (+ the 1-channel strategy)
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "r06_traffic.json")  # profiles/collect_r06c.sh (source-stamped: stale figures are dropped)
SQ_FILE = os.path.join(ROOT, "profiles", "r06_pmc_sq.json")          # profiles/collect_r06a.sh
KERNEL_SOURCES = ("gpd_amd/csrc/lenet.hip", "gpd_amd/csrc/lenet_fast.hip", "gpd_amd/csrc/images.hip", "gpd_amd/csrc/search.hip")
DTYPE = ("f64 geometry / u8 images / LeNet f32-equivalent by exact operand splitting: conv1 int8 digit planes of 32-bit fixed-point "
         "weights (i32 accumulate, exact), conv2 + ip1 three bf16 pieces per operand (six exact products per term, f32 accumulate), ip2 f32")


def lenet_mfma_work(C):
    """What the split path's three matrix kernels EXECUTE per image (padding included) and what that is algorithmically
    (gpd_amd/csrc/lenet_fast.hip): conv1 196 tiles x 35 v_mfma_i32_16x16x64_i8 (20 filters x 4 digits = 80 rows, 7 k-steps of 4 taps x
    16 channels for 25 taps x C channels); conv2 36 tiles x 3 column tiles x 96 v_mfma_f32_16x16x32_bf16 (48 filters, 500 -> 512 k, six piece
    products) + 24 units x 48 for filters 48 and 49 (round 6: rows = (filter, kernel column), k = 5 kernel rows x 24 channel slots ->
    128; until then a fourth column tile, 14 of its 16 columns zero); ip1 512 units x 7296 k x six piece products."""
    # conv1: 7 k-steps of 4 taps x 16 channel bytes; since round 6 the narrow images (C <= 4: four-byte pixels) take 3 k-steps of
    # 4 row groups x (4 taps x 4 channel bytes): 15 instead of 35 MFMAs per tile
    c1_mfmas = 15 if C <= 4 else (25 if C == 12 else 35)  # (12 channels: twelve-byte pixels, a kernel row of 5 taps per k-step: 5 k-steps)
    return {
        "conv1_i8_kernel": dict(pipe="i8", executed=196 * c1_mfmas * 32768.0, algorithmic_split=2.0 * 20 * 25 * C * 56 * 56 * 4,
                                algorithmic=2.0 * 20 * 25 * C * 56 * 56),
        "conv2_bf16_kernel": dict(pipe="bf16", executed=(3 * 36 * 96 + 24 * 48) * 16384.0, algorithmic_split=2.0 * 50 * 500 * 24 * 24 * 6,
                                  algorithmic=2.0 * 50 * 500 * 24 * 24),
        "fc1_bf16_kernel": dict(pipe="bf16", executed=2.0 * 512 * 7296 * 6, algorithmic_split=2.0 * 500 * 7200 * 6, algorithmic=2.0 * 500 * 7200),
    }

def lenet_kernel_entry(k_s, fl, n_cand, wk):
    """One LeNet kernel's entry of `kernels`: k_s = seconds per launch (HIP events), fl = SURVEY 8d's f32 FLOPs per image,
    wk = the kernel's entry of lenet_mfma_work (None: no matrix instructions, ip2)."""
    e = {"ms": k_s * 1e3, "algorithmic_flops": fl * n_cand,
         "achieved_TFLOPs": fl * n_cand / k_s / 1e12 if k_s > 0 else None,
         "frac_f32": fl * n_cand / k_s / 1e12 / F32_PEAK_TFLOPS if k_s > 0 else None}
    if wk is not None and k_s > 0:
        peak = I8_PEAK_TOPS if wk["pipe"] == "i8" else BF16_PEAK_TFLOPS
        e.update({"pipe": wk["pipe"], "executed_ops": wk["executed"] * n_cand, "executed_Tops": wk["executed"] * n_cand / k_s / 1e12,
                  "frac_pipe": wk["executed"] * n_cand / k_s / 1e12 / peak,
                  "useful_share_of_executed": wk["algorithmic_split"] / wk["executed"]})
    return e


def lenet_roofline(dom, kd, wk, traffic_bytes):
    """The `roofline` object for the dominant LeNet kernel `dom`: kd = its entry of `kernels` (ms, executed_*, algorithmic_flops,
    achieved_TFLOPs, frac_f32), wk = its entry of lenet_mfma_work, traffic_bytes = HBM bytes per launch from a counter pass or None."""
    peak = I8_PEAK_TOPS if wk["pipe"] == "i8" else BF16_PEAK_TFLOPS
    return {"kernel": dom, "bound": "mfma", "achieved": kd["executed_Tops"], "peak": peak,
            "unit": "TOP/s" if wk["pipe"] == "i8" else "TFLOP/s", "frac": kd["executed_Tops"] / peak,
            "pipe": wk["pipe"], "traffic": traffic_bytes,
            "ops_per_launch": kd["executed_ops"], "launch_ms": kd["ms"],
            "algorithmic_flops_per_launch": kd["algorithmic_flops"],
            "f32_equivalent": {"achieved_TFLOPs": kd["achieved_TFLOPs"], "frac_of_f32_peak": kd["frac_f32"],
                               "frac_of_pipe_peak": kd["achieved_TFLOPs"] / peak,
                               "ceiling_frac_of_pipe_peak": wk["algorithmic"] / wk["executed"],
                               "note": "SURVEY 8d's f32 FLOPs of the layer / the same time, against the 157.3 TFLOP/s f32-input MFMA "
                                       "peak (the pipe of rounds 1-4: conv2 there ran at 0.77 of it) and against the peak of the pipe "
                                       "it runs on now; ceiling = algorithmic / executed operations: what frac_of_pipe_peak would be "
                                       "with the pipe 100 % busy (an exact f32 product costs 4 int8 / 6 bf16 instructions' worth)"},
            "useful_share_of_executed": wk["algorithmic_split"] / wk["executed"],
            "note": "achieved = executed MFMA operations per launch (tiles x instructions x ops per instruction, lenet_mfma_work) / "
                    "HIP-event time of the kernel; useful_share_of_executed = algorithmic FLOPs x the split factor (4 digit planes / 6 "
                    "piece products) over the executed ones (the rest is tile padding: 50 -> 64 filters, 25 -> 28 tap slots, ...)"}


def lenet_stage_roofline(C, n_images, stage_s):
    """The `roofline` object of a line that has only the LeNet STAGE time (--mode batch: HIP events around the stage of every
    cloud, summed): the stage runs on two matrix pipes, so its roofline is the time the executed MFMA operations of its three
    matrix kernels would take with each kernel's pipe at its dense peak (conv1 on int8, conv2 / ip1 on bf16); frac = that
    time / the measured stage time.  (Until round 6 the batch line priced the stage's f32-equivalent FLOPs against the
    157.3 TFLOP/s f32 peak: above 1 since the split kernels, and meaningless.)"""
    if not stage_s or stage_s <= 0:
        return {"kernel": "LeNet stage of the batch (conv1+conv2+ip1+ip2), rank 0", "bound": "mfma", "achieved": None, "peak": None,
                "unit": "TOP/s", "frac": None, "traffic": None}
    work = lenet_mfma_work(C)
    ops = sum(v["executed"] for v in work.values()) * n_images
    t_peak = sum(v["executed"] * n_images / ((I8_PEAK_TOPS if v["pipe"] == "i8" else BF16_PEAK_TFLOPS) * 1e12) for v in work.values())
    return {"kernel": "LeNet stage of the batch (conv1_i8 + conv2_bf16 + fc1_bf16 + ip2, which adds ip1's K quarters), rank 0", "bound": "mfma",
            "achieved": ops / stage_s / 1e12, "peak": ops / t_peak / 1e12, "unit": "TOP/s", "frac": t_peak / stage_s, "traffic": None,
            "executed_ops": ops, "stage_ms": stage_s * 1e3,
            "f32_equivalent_TFLOPs": LENET_MFLOP[C] * 1e6 * n_images / stage_s / 1e12,
            "note": "achieved = executed MFMA operations of the stage's three matrix kernels (lenet_mfma_work: padding included) / the "
                    "stage's HIP-event time summed over the clouds; peak = the same operations / the time they take with each kernel's "
                    "pipe at its dense peak (5 POP/s int8, 2.5 PFLOP/s bf16) — a blended peak, so frac = t_at_peak / t_measured; the "
                    "stage time is measured with the other lane's kernels running beside it"}


CONFIGS = {  # BASELINE.json configs[1..3]
    "2": dict(points=30000, candidates=5000, channels=15, clutter=False),
    "3a": dict(points=30000, candidates=5000, channels=3, clutter=False),
    "3b": dict(points=30000, candidates=5000, channels=12, clutter=False),
    "4": dict(points=300000, candidates=50000, channels=15, clutter=True),
    # configs[1]'s scene with sensor-like coordinates (synth.off_lattice: every point moved by a seeded sub-voxel offset) — the side
    # line on which the reference's unpinned third-party behaviours (FLANN's order among equal distances, ulp-level eigen-solver
    # differences) do not decide outputs; pinned against the reference's own sources by ref_pin_offlattice_*.npz
    "2o": dict(points=30000, candidates=5000, channels=15, clutter=False, off_lattice=True),
}


def source_hashes():
    out = {}
    for rel in KERNEL_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            out[rel] = hashlib.sha1(f.read()).hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="default 20 (replay) / 3 passes over the rank's clouds (batch)")
    ap.add_argument("--warmup", type=int, default=None, help="default 3 (replay) / 1 (batch)")
    ap.add_argument("--mode", choices=("replay", "batch"), default="replay")
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="BASELINE config preset (default: 2)")
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--candidates", type=int, default=None)
    ap.add_argument("--channels", type=int, default=None)
    ap.add_argument("--clutter", action="store_true")
    ap.add_argument("--clouds", type=int, default=256, help="--mode batch: clouds of the whole job (cloud i -> rank i mod N)")
    ap.add_argument("--batch-samples", type=int, default=2564, help="samples per cloud of the batch legs")
    ap.add_argument("--batch-clouds", type=int, default=None,
                    help="replay mode: clouds per rank and pass of the batch_end_to_end leg (default 24 on one GPU, 32 on several; 0 disables)")
    ap.add_argument("--batch-passes", type=int, default=8, help="replay mode: timed passes of the batch_end_to_end leg (after one full untimed pass)")
    ap.add_argument("--cpu-samples", type=int, default=1500, help="samples of the CPU-baseline leg (0 disables)")
    ap.add_argument("--devices", default=None,
                    help="comma list: the HIP device of local rank r is devices[r %% len] (default: r).  `--devices 0,0` runs two ranks on ONE "
                         "GPU — the N > 1 code path on a one-GPU box (tests); it needs --dist-backend gloo (RCCL refuses two ranks on a device)")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl", help="torch.distributed backend of the barrier / reductions")
    ap.add_argument("--live-pmc", dest="live_pmc", action="store_true", default=None,
                    help="measure roofline.traffic / pmc_traffic here (two rocprofv3 --pmc child runs of this file after the timed region, "
                         "~20 s) instead of reading profiles/r06_traffic.json; default: on for the default line on one GPU, unless this "
                         "process is itself being profiled")
    ap.add_argument("--no-live-pmc", dest="live_pmc", action="store_false")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements beside the headline (replay mode: search alone, detect_end_to_end, batch legs, score "
                         "accuracy, preprocess, cpu_baseline); a plain run times the steps and prints the line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last step to DIR/<name>.npy (rank 0, at most 64 MB)")
    args = ap.parse_args()
    if args.live_pmc and not args.full:
        ap.error("--live-pmc runs child benchmarks of its own: it needs --full")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: one process per GPU under torch.distributed.run (RCCL / gloo rendezvous on
        # 127.0.0.1), same arguments; rank 0 of the children prints the ONE line
        sys.exit(_self_launch(args.gpus))
    if args.live_pmc is None:
        # Off by default since round 5: the two TCC counter passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE around a child run)
        # took the GPU node down twice in a row on 2026-09-25 (the pool's known weakness: PMC collection can crash nodes) — a
        # bench line must not be able to do that.  --live-pmc switches them on; without them `traffic` comes from the committed,
        # source-stamped profile when there is one, else it is null.
        args.live_pmc = False
    if args.batch_clouds is None:
        args.batch_clouds = 24 if args.gpus == 1 else 32
    if args.steps is None:
        args.steps = 20 if args.mode == "replay" else 3
    if args.warmup is None:
        args.warmup = 3 if args.mode == "replay" else 1
    preset = CONFIGS[args.config or "2"]
    points = args.points if args.points is not None else preset["points"]
    candidates = args.candidates if args.candidates is not None else preset["candidates"]
    C = args.channels if args.channels is not None else preset["channels"]
    clutter = args.clutter or preset["clutter"]

    # stdout carries exactly ONE line (the JSON of rank 0): everything else that libraries print to
    # fd 1 (RCCL's start-up banner, HIP warnings) goes to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE = %d (run `python bench.py --gpus %d`, or torch.distributed.run with "
                 "--nproc-per-node %d)" % (args.gpus, world, args.gpus, args.gpus))
    if os.environ.get("GPD_BENCH_DRYRUN"):
        # the launch / rendezvous / reduction plumbing without a GPU (tests/test_bench_helpers.py, gloo): everything up to the
        # point where a context would be created
        import torch.distributed as dist
        dist.init_process_group("gloo")
        dist.barrier()
        t = torch.tensor([1.0 + rank, 10.0 * (rank + 1)], dtype=torch.float64)
        tmax, tsum = t.clone(), t.clone()
        dist.all_reduce(tmax[0:1], op=dist.ReduceOp.MAX)
        dist.all_reduce(tsum[1:2], op=dist.ReduceOp.SUM)
        if rank == 0:
            os.write(json_fd, (json.dumps({"dryrun": True, "n_gpus": args.gpus, "world": world, "max": float(tmax[0]), "sum": float(tsum[1]),
                                           "batch_clouds": args.batch_clouds}) + "\n").encode())
        dist.barrier()
        dist.destroy_process_group()
        return
    dist = None
    device = local_rank
    if args.devices:
        devs = [int(x) for x in args.devices.split(",")]
        device = devs[local_rank % len(devs)]
    red_dev = "cuda" if args.dist_backend == "nccl" else "cpu"  # where the reduction tensors live
    if world > 1 or os.environ.get("GPD_BENCH_FORCE_DIST"):  # the env switch exercises the RCCL path on one GPU
        import torch.distributed as dist
        torch.cuda.set_device(device)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group("gloo")

    from gpd_amd import api, synth
    from gpd_amd import dist as gdist
    real = None
    gold = os.path.join(ROOT, "tests", "golden", "lenet%d_params.npz" % C)
    if os.path.exists(gold):
        real = dict(np.load(gold))
    # the headline is timed on the trained-magnitude weight set (the synthetic ip1 / 128: |score| < 20, the range in which
    # BASELINE's "within 1e-4" can be decided — same FLOPs, same kernels)
    w = synth.lenet_weights(C, real=real, trained_magnitude=True)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    def reduce(elapsed, units):
        if dist is None:
            return float(elapsed), float(units)
        t = torch.tensor([elapsed, float(units)], dtype=torch.float64, device=red_dev)
        tmax = t.clone()
        dist.all_reduce(tmax[0:1], op=dist.ReduceOp.MAX)
        dist.all_reduce(t[1:2], op=dist.ReduceOp.SUM)
        return float(tmax[0]), float(t[1])

    def minmax(x):
        if dist is None:
            return float(x), float(x)
        lo = torch.tensor([float(x)], dtype=torch.float64, device=red_dev)
        hi = lo.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        return float(lo[0]), float(hi[0])

    # N > 1: this process feeds ONE GPU — keep its host thread on that GPU's socket (gpd_hip_bind_host_thread; SURVEY 8e: eight
    # feeding processes on a two-socket host).  Not at N = 1: the cpu_baseline leg of the same process wants every host core.
    numa = None
    if world > 1:
        node, ncpu = api.bind_host_thread(device)
        numa = {"node": node, "cpus": ncpu} if node >= 0 else {"node": None, "note": "the host exposes no NUMA topology for this device"}
    ctx = api.Context(api.default_params(C), device=device)
    ctx.set_lenet_weights(w)                       # weights copied once per device at init
    last_pass = []  # (hands, n_sets, n_candidates, stage_ms) per cloud of batch_leg's last timed pass

    def batch_leg(cloud_ids, passes, warm):
        """gpd_hip_detect_batch over the listed clouds (seed 1234 + id): `warm` untimed FULL passes (every lane buffer at its
        final size, clocks up), then `passes` timed ones, barrier-bracketed as a whole and timed one by one (a pass = one call;
        its results are on the host when it returns).  The whole-job figure is all candidates / the bracketed time; the
        per-pass spread says whether that figure can be trusted (a single 75 ms pass after a 3-cloud warm-up gave
        565 k/s on one box and 1.0 M/s on three others)."""
        clouds = [synth.make_cloud(1234 + cid, 30000) for cid in cloud_ids]
        samples = [synth.sample_indices(cl, args.batch_samples) for cl in clouds]
        prepared = ctx.batch(clouds, samples, 0)  # job array + output buffers, built once (as a host that streams clouds would)
        for _ in range(max(warm, 1)):
            ctx.run_batch(prepared)
        barrier()
        t0 = time.perf_counter()
        n_cand = 0
        stage = np.zeros(3)
        pass_s, pass_cand, pass_allocs, pass_host, pass_rows = [], [], [], [], []
        for _ in range(passes):
            tp = time.perf_counter()
            nc_pass = 0
            per_cloud = []
            last_pass[:] = ctx.run_batch(prepared)  # views into the batch's buffers: the last pass's results until the next run
            for hands, ns, nc, ms in last_pass:
                nc_pass += nc
                stage += ms
                per_cloud.append([round(float(x), 2) for x in ms])
            pass_s.append(time.perf_counter() - tp)
            pass_cand.append(nc_pass)
            n_cand += nc_pass
            tl = ctx.last_batch_timeline
            pass_allocs.append(sum(a for _, a in tl))
            pass_host.append(_host_split([h for h, _ in tl]))
            pass_rows.append([[round(x, 2) for x in h] + [ms_c] for (h, _), ms_c in zip(tl, per_cloud)])
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if dist is not None:
            dist.barrier()
        el, tot = reduce(elapsed, n_cand)
        _, ncl = reduce(elapsed, len(clouds) * passes)
        mine = len(clouds) * passes / elapsed  # this rank's own rate: a host-side limiter shows as a spread
        rmin, rmax = minmax(mine)
        rates = sorted(c / t for c, t in zip(pass_cand, pass_s))
        slow = int(np.argmax(pass_s))
        return dict(clouds=int(ncl), clouds_per_rank=len(clouds) * passes, candidates=int(tot), wall_s=el, clouds_per_s=ncl / el,
                    cand_per_s=tot / el, rank_clouds_per_s={"min": rmin, "max": rmax},
                    passes={"n": passes, "warmup_passes": max(warm, 1), "clouds_per_pass": len(clouds),
                            "wall_ms_rank0": [t * 1e3 for t in pass_s],
                            "cand_per_s_rank0": {"min": rates[0], "median": rates[len(rates) // 2], "max": rates[-1]},
                            "buffer_growths_in_timed_passes": int(sum(pass_allocs)),
                            "host_ms_slowest_pass": pass_host[slow], "host_ms_fastest_pass": pass_host[int(np.argmin(pass_s))],
                            # a pass more than 5 % above the median: its clouds one by one, so that the stall can be placed
                            # ([begin done, plan arrived, middle enqueued, results arrived, records copied] ms since entry,
                            #  then the cloud's [search, images, LeNet] kernel ms)
                            "outlier_pass_clouds": pass_rows[slow] if pass_s[slow] > 1.05 * sorted(pass_s)[len(pass_s) // 2] else None,
                            "note": "one pass = one gpd_hip_detect_batch call over the rank's clouds (pipeline filled and drained per call); "
                                    "host_ms: the calling thread's time enqueuing / copying vs blocked on the device (gpd_detect_job.host_ms)"},
                    kernel_ms_rank0={"search": float(stage[0]), "images": float(stage[1]), "lenet": float(stage[2]),
                                     "note": "summed per cloud over the timed passes; two clouds are in flight, so the sum exceeds the wall time"})

    if args.mode == "batch":
        mine = gdist.clouds_of_rank(args.clouds, rank, world)
        assert mine, "more ranks than clouds"
        leg = batch_leg(mine, args.steps, args.warmup)
        if rank == 0:
            net_s = leg["kernel_ms_rank0"]["lenet"] / 1e3
            n0 = leg["candidates"] / world
            out = {
                "metric": "15-ch grasp candidates generated+scored/sec, end to end over a batch of clouds (configs[4])",
                "value": leg["cand_per_s"], "unit": "candidates/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": leg["wall_s"] / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
                "vs_baseline": None, "dtype": DTYPE, "data": "synthetic",
                "config": {"workload": "%d synthetic 30k-point clouds x %d samples (~%d candidates each), 15-channel, cloud i -> rank i mod %d; "
                                       "per cloud: host buffers in, upload, grid, search, filter, images, LeNet, scored candidates out"
                           % (args.clouds, args.batch_samples, leg["candidates"] // max(1, leg["clouds"]), world),
                           "clouds": args.clouds, "samples_per_cloud": args.batch_samples, "channels": C,
                           "sharding": "independent clouds, no collective"},
                "batch_end_to_end": leg, "host_binding_rank0": numa,
                "roofline": lenet_stage_roofline(C, n0, net_s),
            }
            if args.dump_outputs:
                _dump_outputs(args.dump_outputs, _batch_outputs(last_pass))
            sys.stdout.flush()
            os.write(json_fd, (json.dumps(out) + "\n").encode())
        ctx.close()
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    # --- replay mode.  Workload: one cloud per rank (seed 1234 + rank), first `candidates` valid hands
    cloud = synth.make_cloud(1234 + rank, points, clutter=clutter)
    if preset.get("off_lattice"):
        cloud = synth.off_lattice(cloud)
    ctx.upload_cloud(cloud["xyz"], cloud["normals"], cloud["cam_source"], cloud["view_points"])
    n_samples = min(int(candidates / 2.0) + 64, int(cloud["is_object"].sum()))
    si = synth.sample_indices(cloud, n_samples)
    hands = ctx.search(si)  # first call: allocations
    search_ms, search_wall = 1e30, 1e30
    for _ in range(3 if args.full else 0):  # the stage kernels by HIP events / the unfused call incl. the download of every hand record
        t0 = time.perf_counter()
        hands = ctx.search(si)
        search_wall = min(search_wall, time.perf_counter() - t0)
        search_ms = min(search_ms, float(ctx.stage_ms()[0]))
    # host workspace/aperture filter through the product path is part of detect(); here the
    # candidate list is cut to exactly `candidates` hands in (set, slot) order
    hands_f = hands.copy()
    _filter_workspace(hands_f, ctx.params)
    flat = hands_f.reshape(-1)
    vidx = np.flatnonzero(flat["valid"])
    if len(vidx) > candidates:
        flat["valid"][vidx[candidates:]] = 0

    # end-to-end latency of the fused entry point (search + filter + images + LeNet, host buffers in / out)
    if args.full:
        ctx.detect(si)
        walls, kms = [], []
        for _ in range(5):  # median of five calls
            t0 = time.perf_counter()
            _, n_detect = ctx.detect(si)
            walls.append(time.perf_counter() - t0)
            kms.append([float(x) for x in ctx.stage_ms()])
        mid = int(np.argsort(walls)[len(walls) // 2])
        detect_wall, detect_kernel_ms = walls[mid], kms[mid]

    _, cand = ctx.images(hands_f, download=False)   # the benchmark's candidate list, first pass
    n_cand = len(cand)
    ni = ctx.images_stats()

    fallbacks = ctx.fallbacks()  # of the benchmark's candidate list: which slow paths its search / image stage took
    for _ in range(args.warmup):
        ctx.replay(3)
    ctx.replay_times()
    ctx.conv1_stats(reset=True)  # conv1 counts the (chunk, channel) pairs it executes: from here on, the timed launches only
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ctx.replay(3)
    img_ms, net_ms, launches, timed_scores = ctx.replay_times(n_scores=n_cand)  # the scores of the last timed step come back with the times
    kernel_ms = ctx.replay_kernel_ms()              # conv1, conv2, ip1, ip2 (which adds ip1's four K quarters first) summed over the timed steps
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    elapsed, total_cand = reduce(elapsed, n_cand)
    assert launches == args.steps
    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, {"scores": timed_scores})
    pairs_done, pairs_seen = ctx.conv1_stats(reset=True)
    live_frac = pairs_done / pairs_seen if pairs_seen else None
    # (the batch leg runs BEFORE any leg that uses the host's cores: the oracle's OpenMP team and torch's intra-op threads keep
    #  spinning for a while after their last parallel region, and a spinning team beside the HIP runtime's threads showed up as
    #  one 30 ms stall in one of eight batch passes — r04_cold.sh on two boxes; 48 passes without those legs: none)
    batch = None
    if args.full and args.batch_clouds > 0 and C == 15 and not clutter:
        batch = batch_leg([rank + world * k for k in range(args.batch_clouds)], args.batch_passes, 1)
    batch_raw = None
    if args.full and args.batch_clouds > 0 and C == 15 and not clutter and args.config is None and args.gpus == 1:
        batch_raw = _raw_batch_leg(ctx, api, synth, max(args.batch_clouds // 2, 2), max(args.batch_passes // 2, 3), args.batch_samples)
    trained = None
    if args.full and rank == 0 and args.gpus == 1 and C == 15 and args.cpu_samples > 0:
        if batch is not None:  # the batch left its last cloud resident: the benchmark's cloud and its search state once more
            ctx.upload_cloud(cloud["xyz"], cloud["normals"], cloud["cam_source"], cloud["view_points"])
            ctx.search(si)
        trained = _score_accuracy_leg(ctx, hands_f, C, w, timed_scores, synth.lenet_weights(C, real=real))

    if rank == 0:
        value = total_cand * args.steps / elapsed
        img_s = img_ms / 1e3 / args.steps
        net_s = net_ms / 1e3 / args.steps
        # B_img = sum_sets 24*N_i + sum_cand (3600*C + 184)
        b_img = 24.0 * ni["sum_set_ni"] + n_cand * (3600.0 * C + 184.0)
        b_stream = 24.0 * ni["sum_cand_ni"] + n_cand * (3600.0 * C + 184.0)  # what the kernel actually streams
        img_gbs = b_img / img_s / 1e9
        net_tflops = LENET_MFLOP[C] * 1e6 * n_cand / net_s / 1e12
        kernels = {
            "grasp_image_kernel": {"ms": img_s * 1e3, "algorithmic_bytes": b_img, "streamed_bytes": b_stream,
                                   "achieved_GBps": img_gbs, "frac_hbm": img_gbs / HBM_PEAK_GBS,
                                   "cand_per_s": n_cand / img_s},
            "lenet_forward": {"ms": net_s * 1e3, "algorithmic_flops": LENET_MFLOP[C] * 1e6 * n_cand,
                              "achieved_TFLOPs": net_tflops, "frac_f32": net_tflops / F32_PEAK_TFLOPS,
                              "img_per_s": n_cand / net_s},
        }
        # per-kernel LeNet durations (HIP events between the kernels on the context's stream)
        work = lenet_mfma_work(C)
        kflops = {k: v["algorithmic"] for k, v in work.items()}
        kflops["fc2_score_kernel"] = 2.0 * 2 * 500
        for (name, fl), ms_sum in zip(kflops.items(), kernel_ms):
            kernels[name] = lenet_kernel_entry(ms_sum / 1e3 / args.steps, fl, n_cand, work.get(name))
        traffic = _pmc_traffic(n_cand, C, live=args.live_pmc and args.gpus == 1)
        sq = _pmc_sq()
        if sq:
            # the image kernels are latency / LDS bound, not HBM bound: their LDS roofline is the share of
            # the chip's LDS-array cycles that moved data (peak 256 B/clk/CU, MI355X_MICROARCH.md §LDS)
            kernels["grasp_image_kernel"]["lds_roofline"] = sq
        dom = max(work, key=lambda k: kernels[k]["ms"])
        if kernels[dom]["ms"] >= img_s * 1e3 / 3.0:
            # the dominant single kernel of the step.  Since round 5 the LeNet runs on the int8 / bf16 matrix pipes with exactly
            # split operands: `achieved` = the MFMA operations the kernel EXECUTES per launch (instruction count x operations per
            # instruction: padding included, nothing skipped) / its HIP-event time, against the dense peak of ITS pipe — a
            # utilisation, the number to hold against MfmaUtil.  The f32-equivalent rate (SURVEY 8d's algorithmic FLOPs / the same
            # time) rides along, against the 157.3 TFLOP/s f32 peak the previous rounds' f32-input MFMA kernels were priced on.
            roofline = lenet_roofline(dom, kernels[dom], work[dom], traffic.get(dom.replace("_kernel", ""), traffic.get("lenet")))
        else:
            roofline = {"kernel": "image stage (shadow_set + shadow_image + grasp_image kernels)", "bound": "hbm", "achieved": img_gbs, "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": img_gbs / HBM_PEAK_GBS, "traffic": traffic.get("image")}
        if args.full:
            # the stage before the timed one, per call of gpd_hip_search (B_search = sum_samples [12 k_f + 24 N_h + 12] + S n_orient 184)
            sum_kf, sum_nh = _neighbour_counts(cloud, si, ctx.params)
            b_search = 12.0 * sum_kf + 24.0 * sum_nh + 12.0 * n_samples + float(hands.size) * 184.0
            kernels["search"] = {"ms": search_ms, "samples": int(n_samples), "algorithmic_bytes": b_search,
                                 "achieved_GBps": b_search / (search_ms / 1e3) / 1e9, "frac_hbm": b_search / (search_ms / 1e3) / 1e9 / HBM_PEAK_GBS,
                                 "pmc_traffic_bytes": traffic.get("search"),
                                 "note": "neighbourhood + height_list + hand_eval + plan (+ centre on a side stream); not part of `value`"}
        out = {
            "metric": "15-ch grasp candidates scored/sec (imagegen+LeNet) at 1/2/4/8 MI355X" if C == 15 else "%d-ch grasp candidates scored/sec (imagegen+LeNet)" % C,
            "value": value, "unit": "candidates/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": DTYPE, "data": "synthetic",
            "config": {"workload": "single %dk-point synthetic %scloud per GPU (seed 1234+rank%s), first %d valid candidates, %d-channel LeNet"
                       % (points // 1000, "clutter " if clutter else "", ", coordinates moved off the 3 mm lattice by a seeded sub-voxel offset" if preset.get("off_lattice") else "",
                          n_cand, C), "points": points, "candidates_per_gpu": n_cand,
                       "samples": int(n_samples), "channels": C, "sharding": "one cloud per GPU, no collective"},
            "roofline": roofline, "kernels": kernels, "pmc_traffic": traffic,
            "fallbacks": fallbacks,
        }
        if args.full:
            out["search"] = {"samples": int(n_samples), "hand_sets": int(hands.shape[0]), "kernel_ms": search_ms,
                             "wall_ms_incl_download": search_wall * 1e3}
            out["detect_end_to_end"] = {"candidates": int(n_detect), "wall_ms": detect_wall * 1e3,
                                        "kernel_ms": {"search": detect_kernel_ms[0], "images": detect_kernel_ms[1], "lenet": detect_kernel_ms[2]},
                                        "kernel_sum_over_wall": sum(detect_kernel_ms) / (detect_wall * 1e3),
                                        "cand_per_s": n_detect / detect_wall,
                                        "note": "gpd_hip_detect: all candidates of the sample set, host buffers in, scored hands out; "
                                                "filter / compaction / score scatter on the device"}
        if numa is not None:
            out["host_binding_rank0"] = numa
        if trained is not None:
            out["scores_timed_list"] = trained
        if batch is not None:
            batch["note"] = ("gpd_hip_detect_batch, %d clouds per rank and pass x %d samples, %d timed passes after one full untimed pass, two clouds "
                             "in flight per context: upload + grid + search + filter + images + LeNet + scored candidates back to the host"
                             % (args.batch_clouds, args.batch_samples, args.batch_passes))
            out["batch_end_to_end"] = batch
        if batch_raw is not None:
            out["batch_raw_end_to_end"] = batch_raw
        raw = None
        if args.full and args.config is None and C == 15 and not clutter:  # the widened row before the path, on the default line only
            raw, out["preprocess"] = _preprocess_leg(ctx)
        if args.full and args.cpu_samples > 0 and args.gpus == 1:  # the CPU leg runs on rank 0 at N=1 only
            out["cpu_baseline"] = _cpu_baseline(cloud, w, C, si, n_cand, args.cpu_samples)
            if raw is not None:
                out["cpu_baseline"]["preprocess_ms"] = _cpu_preprocess_ms(raw)
                out["cpu_baseline"]["normals_ms"] = _cpu_normals_ms()
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    ctx.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def _raw_batch_leg(ctx, api, synth, n_clouds, passes, n_samples):
    """gpd_hip_detect_batch on RAW scans (gpd_detect_job.raw): 120k-point synthetic scans (the cloud of the `preprocess` leg, one
    seed per cloud: points on the 3 mm lattice, which the reference's voxeliser keeps nearly all of) through workspace cut +
    voxeliser (0.003) + normals (0.03) + search at 2564 sample coordinates + images + LeNet, scored candidates back on the host;
    one untimed pass, then `passes` timed ones.  Not part of `value`."""
    scans, samples = [], []
    for k in range(n_clouds):
        cl = synth.make_cloud(3000 + k, PRE_POINTS)
        scans.append(dict(xyz=cl["xyz"], cam_source=cl["cam_source"], view_points=cl["view_points"]))
        samples.append(cl["xyz"][synth.sample_indices(cl, n_samples)].astype(np.float64))
    jobs, keep = ctx.raw_batch(scans, samples, np.array(PRE_WORKSPACE), PRE_VOXEL, 0.03)
    L = api.lib()
    ctx._check(L.gpd_hip_detect_batch(ctx._h, jobs, len(jobs)))
    times, cands = [], []
    for _ in range(passes):
        t0 = time.perf_counter()
        ctx._check(L.gpd_hip_detect_batch(ctx._h, jobs, len(jobs)))
        times.append(time.perf_counter() - t0)
        cands.append(sum(j.num_candidates for j in jobs))
    order = sorted(times)
    return {"clouds_per_pass": n_clouds, "raw_points_per_cloud": int(len(scans[0]["xyz"])), "points_after_preprocessing": [int(j.num_points_processed) for j in jobs][:4],
            "samples_per_cloud": n_samples, "passes": passes, "wall_ms_per_pass": [t * 1e3 for t in times],
            "ms_per_cloud": {"min": order[0] * 1e3 / n_clouds, "median": order[len(order) // 2] * 1e3 / n_clouds, "max": order[-1] * 1e3 / n_clouds},
            "cand_per_s_median": cands[0] / order[len(order) // 2], "buffer_growths_in_timed_passes": int(sum(j.allocs for j in jobs)),
            "kernel_ms_last_cloud": {"search": float(jobs[-1].stage_ms[0]), "images": float(jobs[-1].stage_ms[1]), "lenet": float(jobs[-1].stage_ms[2])},
            "note": "CandidatesGenerator::preprocessPointCloud inside the batch entry: the voxelised cloud never leaves the device, the voxeliser's "
                    "sequential chain of cloud i + 1 runs on the calling host thread beside cloud i's image / LeNet kernels"}


DUMP_MAX_BYTES = 64 * 1000 * 1000  # --dump-outputs: all files together
NPY_HEADER_BYTES = 256               # room kept per file for its .npy header
HAND_DUMP_FIELDS = ("score", "sample", "frame", "position", "top", "bottom", "center", "grasp_width", "finger_placement_index",
                    "set_index", "slot", "half_antipodal", "full_antipodal")


def _dump_outputs(path, arrays):
    """--dump-outputs: each array as path/<name>.npy (float32 stays float32, everything else float64)."""
    out = {k: np.ascontiguousarray(v, np.float32 if np.asarray(v).dtype == np.float32 else np.float64) for k, v in arrays.items()}
    assert sum(v.nbytes + NPY_HEADER_BYTES for v in out.values()) <= DUMP_MAX_BYTES, "outputs beyond the dump limit"
    os.makedirs(path, exist_ok=True)
    for k, v in out.items():
        np.save(os.path.join(path, k + ".npy"), v)


def _batch_outputs(last_pass):
    """The scored hand records of batch_leg's last timed pass, all clouds in order, one array per field (hand_<field>), and the
    per-cloud counts.  Beyond DUMP_MAX_BYTES a fixed seeded sample of the records is kept, its row numbers in hand_rows."""
    hands = np.concatenate([np.asarray(h) for h, _, _, _ in last_pass])
    out = {"num_sets": np.array([ns for _, ns, _, _ in last_pass], np.float64),
           "num_candidates": np.array([nc for _, _, nc, _ in last_pass], np.float64),
           "num_hands": np.array([len(h) for h, _, _, _ in last_pass], np.float64)}
    row_bytes = sum((4 if f == "score" else 8) * int(np.prod(hands.dtype[f].shape)) for f in HAND_DUMP_FIELDS)
    files = len(out) + len(HAND_DUMP_FIELDS) + 1
    budget = (DUMP_MAX_BYTES - files * NPY_HEADER_BYTES - sum(v.nbytes for v in out.values())) // (row_bytes + 8)
    if len(hands) > budget:
        rows = np.sort(np.random.RandomState(0).choice(len(hands), budget, replace=False))
        hands = hands[rows]
        out["hand_rows"] = rows.astype(np.float64)
    for f in HAND_DUMP_FIELDS:
        out["hand_" + f] = hands[f].astype(np.float32 if f == "score" else np.float64)
    return out


def _host_split(tl):
    """gpd_detect_job.host_ms of one gpd_hip_detect_batch call -> where its host thread spent the call: enqueuing / copying
    (`work`) or blocked on the device (`wait`: the plan summary of cloud i, the results of cloud i - 1).  The entry orders its
    steps begin(i + 1), middle(i), end(i - 1); the stamps are [0] begin done, [1] plan arrived, [2] middle enqueued, [3] results
    arrived, [4] records copied."""
    n = len(tl)
    seq = [(tl[0][0], "work")] if n else []
    for i in range(n):
        if i + 1 < n:
            seq.append((tl[i + 1][0], "work"))
        seq.append((tl[i][1], "wait"))
        seq.append((tl[i][2], "work"))
        if i >= 1:
            seq.append((tl[i - 1][3], "wait"))
            seq.append((tl[i - 1][4], "work"))
    if n:
        seq.append((tl[n - 1][3], "wait"))
        seq.append((tl[n - 1][4], "work"))
    out = {"work": 0.0, "wait": 0.0}
    prev = 0.0
    longest = {"work": 0.0, "wait": 0.0}
    for t, kind in seq:
        d = max(0.0, t - prev)
        out[kind] += d
        longest[kind] = max(longest[kind], d)
        prev = max(prev, t)
    return {"enqueue_and_copy": out["work"], "blocked_on_device": out["wait"], "longest_enqueue_step": longest["work"],
            "longest_wait": longest["wait"], "total": prev}


def _filter_workspace(hands, p):
    """GraspDetector::filterGraspsWorkspace (grasp_detector.cpp:334-398) in numpy, Q6 typo kept."""
    h = hands.reshape(-1)
    F = h["frame"].reshape(-1, 3, 3)
    app, binm = F[:, :, 0], F[:, :, 1]
    half = 0.5 * p.hand_outer_diameter
    lb = h["position"] + half * binm
    rb = h["position"] - half * binm
    lt = lb + p.hand_depth * app
    apr = h["position"] - 0.05 * app
    pts = np.stack([lb, rb, lt, lt, apr], 0)
    mn, mx = pts.min(0), pts.max(0)
    ws = np.array(list(p.workspace_grasps))
    ok = (h["grasp_width"] >= p.min_aperture) & (h["grasp_width"] <= p.max_aperture)
    for r in range(3):
        ok &= (mn[:, r] >= ws[2 * r]) & (mx[:, r] <= ws[2 * r + 1])
    h["valid"] = (h["valid"].astype(bool) & ok).astype(np.uint8)


def _neighbour_counts(cloud, si, p):
    """sum over the samples of k_f (frame radius) and N_h (hand radius) — the sizes SURVEY 8d's B_search is made of
    (bookkeeping for the byte count, by scipy's k-d tree)."""
    from scipy.spatial import cKDTree
    tree = cKDTree(cloud["xyz"].astype(np.float64))
    q = cloud["xyz"][si].astype(np.float64)
    r_hand = max(p.hand_outer_diameter - p.finger_width, p.hand_depth, p.hand_height / 2.0)  # hand_search.cpp:10-22
    kf = tree.query_ball_point(q, p.nn_radius_frames, return_length=True)
    nh = tree.query_ball_point(q, r_hand, return_length=True)
    return float(kf.sum()), float(nh.sum())


def _self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-run under torch.distributed.run, one rank per GPU."""
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def _lenet_f64(images, w):
    """The LeNet in float64 (torch CPU): an order-free yardstick for the float32 scores."""
    import torch
    import torch.nn.functional as Fn
    C = images.shape[3]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    c1w, c1b, c2w, c2b = d(w["c1w"].reshape(20, C, 5, 5)), d(w["c1b"]), d(w["c2w"].reshape(50, 20, 5, 5)), d(w["c2b"])
    f1w, f1b, f2w, f2b = d(w["f1w"].reshape(7200, 500).T.copy()), d(w["f1b"]), d(w["f2w"].reshape(500, 2).T.copy()), d(w["f2b"])
    out = np.zeros(len(images), np.float64)
    with torch.no_grad():
        for i0 in range(0, len(images), 500):  # 500 images at a time: 0.6 GB of float64 activations, whatever the list's length
            x = d(images[i0:i0 + 500].transpose(0, 3, 1, 2).astype(np.float64))
            h = Fn.max_pool2d(Fn.conv2d(x, c1w, c1b), 2)
            h = Fn.max_pool2d(Fn.conv2d(h, c2w, c2b), 2)
            flat = h.permute(0, 2, 3, 1).reshape(len(h), 7200)  # pixel-major, channel-minor (eigen_classifier.cpp:103-107)
            y = torch.relu(Fn.linear(flat, f1w, f1b))
            z = Fn.linear(y, f2w, f2b)
            out[i0:i0 + 500] = (z[:, 1] - z[:, 0]).numpy()
    return out


ACCURACY_LEG_MAX = 5000  # candidates the score-accuracy leg looks at (the whole timed list of every configuration but configs[3])


def _score_accuracy_leg(ctx, hands_f, C, w, timed_scores, w_survey=None):
    """BASELINE's "scores within 1e-4 of the Eigen path" on ALL candidates of the timed list, with the weights the headline is
    timed on (trained-net magnitudes, |score| < 20): the scores the timed region produced (default mode: int8 / bf16 matrix pipes
    on exactly split operands) against the oracle's k-ascending f32 fma chains — the definition the reference's plain-float path
    shares up to summation order (tests/test_ref_pin.py asserts |chain - reference plain float| on the pins) — and both against
    float64 (torch, CPU); then the library's f32-chain mode, which must reproduce the oracle bit for bit."""
    import oracle
    from gpd_amd import api
    # at most the first 5000 candidates of the list (config 4's 50 000 images would be 2.7 GB of pixels on the host and a minute of
    # CPU LeNet: the leg must stay small beside the measurement — round 5 lost three GPU boxes to the unbounded version of this leg)
    sub = hands_f.copy()
    flat = sub.reshape(-1)
    keep = np.flatnonzero(flat["valid"])
    if len(keep) > ACCURACY_LEG_MAX:
        flat["valid"][keep[ACCURACY_LEG_MAX:]] = 0
        timed_scores = timed_scores[:ACCURACY_LEG_MAX]
    imgs, _ = ctx.images(sub, download=True)
    assert len(imgs) == len(timed_scores)
    orc = oracle.lenet(imgs, w)
    f64 = _lenet_f64(imgs, w)
    ctx.set_lenet_mode(api.LENET_F32_CHAIN)
    chain = ctx.score(imgs)
    ctx.set_lenet_mode(api.LENET_SPLIT)
    again = ctx.score(imgs)
    # ... and the same images under SURVEY 8d's own weight set (ip1 ~ N(0, 0.005^2): |score| ~ 1000, one f32 ulp = 6e-5, where only a
    # RELATIVE bound can be stated for any f32 summation order, Eigen's included — VERDICT r5 weak #2)
    survey = None
    if w_survey is not None:
        ctx.set_lenet_weights(w_survey)
        s_split = ctx.score(imgs)
        ctx.set_lenet_mode(api.LENET_F32_CHAIN)
        s_chain = ctx.score(imgs)
        ctx.set_lenet_mode(api.LENET_SPLIT)
        ctx.set_lenet_weights(w)  # the timed set back
        f64s = _lenet_f64(imgs, w_survey)
        orcs = oracle.lenet(imgs, w_survey)
        scale = float(np.abs(f64s).max())
        survey = {"weights": "SURVEY 8d's synthetic set: ip1 ~ N(0, 0.005^2), unscaled", "max_abs_score": scale,
                  "max_rel_split_minus_float64": float(np.abs(s_split - f64s).max() / scale),
                  "max_rel_oracle_chain_minus_float64": float(np.abs(orcs - f64s).max() / scale),
                  "max_rel_split_minus_oracle_chain": float(np.abs(s_split - orcs).max() / scale),
                  "max_abs_split_minus_float64": float(np.abs(s_split - f64s).max()),
                  "one_f32_ulp_at_max_score": float(np.spacing(np.float32(scale))),
                  "f32_chain_mode_bit_identical_to_oracle": bool(np.array_equal(s_chain, orcs)),
                  "note": "relative to max |score|: an absolute 1e-4 is below two f32 ulps of the scores themselves here; "
                          "tests/test_ref_pin.py holds both modes against the reference's own plain-float scores on the pins"}
    return {"images": int(len(imgs)), "weights": "trained magnitude (synthetic ip1 / 128): the set the headline is timed on",
            "survey_8d_weights": survey,
            "max_abs_score": float(np.abs(f64).max()),
            "max_abs_hip_minus_oracle_chain": float(np.abs(timed_scores - orc).max()),
            "max_abs_hip_minus_float64": float(np.abs(timed_scores - f64).max()),
            "max_abs_oracle_chain_minus_float64": float(np.abs(orc - f64).max()),
            "f32_chain_mode_bit_identical_to_oracle": bool(np.array_equal(chain, orc)),
            "timed_scores_reproduced_by_gpd_hip_score": bool(np.array_equal(again, timed_scores)),
            "within_1e-4": bool(np.abs(timed_scores - orc).max() <= 1e-4 and np.abs(timed_scores - f64).max() <= 1e-4),
            "note": "hip = the scores of the last timed step (gpd_hip_replay), all candidates of the timed list"}


def _fc1_tile(n):
    """lenet_fast.hip fc1f_pick_nt: ip1's image-tile height (in 32s) for n images."""
    r = 1
    while True:
        nt = -(-n // (32 * r * 32))
        if nt <= 5:
            return max(nt, 1)
        r += 1


def _live_pmc_kernels():
    """--live-pmc: the two PMC passes of profiles/collect_r06c.sh run from inside this process, on this box — `rocprofv3 --pmc
    FETCH_SIZE` and `--pmc WRITE_SIZE` (counters only, their own runs) around a short child run of this file — and reduced as
    profiles/summarize.py --traffic does (KiB per launch; reads x2 per the gfx950 FETCH_SIZE note of MI355X_MICROARCH.md).
    Returns the per-kernel dict of profiles/r06_traffic.json, or None when rocprofv3 is missing / a pass fails."""
    import glob
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    tmp = tempfile.mkdtemp(prefix="gpd_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    res = {}
    try:
        for counter, key in (("FETCH_SIZE", "fetch_KiB_raw"), ("WRITE_SIZE", "write_KiB")):
            d = os.path.join(tmp, counter)
            cmd = [exe, "--pmc", counter, "-d", d, "-o", "bench", "--", sys.executable, os.path.abspath(__file__), "--steps", "3", "--warmup", "1",
                   "--cpu-samples", "0", "--batch-clouds", "0", "--no-live-pmc", "--full"]
            p = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                p.wait(timeout=120)
            except subprocess.TimeoutExpired:
                import signal
                os.killpg(p.pid, signal.SIGKILL)  # its own session: exactly the processes started here
                p.wait()
                return None
            dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
            if p.returncode != 0 or not dbs:
                return None
            c = sqlite3.connect(dbs[0])
            cols = [r[1] for r in c.execute("pragma table_info(counters_collection)")]
            nm = "kernel_name" if "kernel_name" in cols else "name"
            for name, avg in c.execute("select %s, avg(value) from counters_collection where counter_name = ? group by %s" % (nm, nm), (counter,)):
                res.setdefault(str(name), {})[key] = avg
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for v in res.values():
        v["read_bytes_corrected"] = 2.0 * v.get("fetch_KiB_raw", 0.0) * 1024.0
        v["write_bytes"] = v.get("write_KiB", 0.0) * 1024.0
        v["hbm_bytes_per_launch"] = v["read_bytes_corrected"] + v["write_bytes"]
    return res or None


def _pmc_traffic(n_images, channels=15, live=False):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/r06_traffic.json, produced by
    profiles/collect_r06c.sh on the default workload).  The file carries the SHA-1 of the kernel sources it was measured
    on: when a kernel file has changed since, the numbers are stale and dropped.  live (--live-pmc): measured here and now
    instead (_live_pmc_kernels), the file's figures next to them."""
    if channels != 15 or n_images != 5000:
        return {"note": "the PMC passes were collected on the default workload (15 channels, 5000 candidates) only"}
    filed = None
    if os.path.exists(TRAFFIC_FILE):
        filed = json.load(open(TRAFFIC_FILE))
        filed = filed["kernels"] if filed.get("source_hashes") == source_hashes() else None
    if live:
        try:
            d = _live_pmc_kernels()
        except Exception as e:  # a measurement aid must not take the bench line down with it
            sys.stderr.write("bench.py: live PMC passes failed (%s): the committed profile is reported\n" % e)
            d = None
        if d is not None:
            out = _traffic_totals(d, n_images, "live: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes run by this process on this box (a "
                                  "3-step child run each; reads x2 per the gfx950 note)")
            if filed is not None:
                out["committed_file"] = {k: v for k, v in _traffic_totals(filed, n_images, "").items() if k != "source"}
            return out
    if not os.path.exists(TRAFFIC_FILE):
        return {"note": "no PMC traffic file"}
    if filed is None:
        return {"note": "%s was measured on other kernel sources: stale, not reported" % os.path.relpath(TRAFFIC_FILE, ROOT)}
    return _traffic_totals(filed, n_images, "profiles/r06_traffic.json (separate --pmc FETCH_SIZE / WRITE_SIZE passes of the default workload; "
                           "reads x2 per the gfx950 note; same kernel sources as this run, by SHA-1)")


def _traffic_totals(d, n_images, source):
    out = {"source": source}
    fc1 = "fc1_bf16_kernel<%d>" % _fc1_tile(n_images)

    def total(names):
        vals = [v["hbm_bytes_per_launch"] for k, v in d.items() if any(s in k for s in names)]
        return float(sum(vals)) if vals else None

    out["image"] = total(("grasp_image_kernel<false>", "shadow_image_kernel<6144", "shadow_set_kernel"))
    out["lenet"] = total(("conv1_i8", "conv2_bf16", fc1, "fc1_combine", "fc2_score"))
    out["conv1_i8"] = total(("conv1_i8",))
    out["conv2_bf16"] = total(("conv2_bf16",))
    out["fc1_bf16"] = total((fc1, "fc1_combine"))
    out["search"] = total(("neighbourhood_kernel<false>", "hand_eval_kernel", "plan_kernel", "centre_kernel"))
    return {k: v for k, v in out.items() if v is not None}


def _pmc_sq():
    """LDS-array utilisation of the image kernels from the committed SQ-counter pass (profiles/pmc_sq.sh ->
    profiles/r06_pmc_sq.json), dropped like the traffic numbers when the kernel sources have changed since."""
    if not os.path.exists(SQ_FILE):
        return None
    d = json.load(open(SQ_FILE))
    if d.get("source_hashes") != source_hashes():
        return None
    out = {"source": "profiles/r06_pmc_sq.json: SQ_LDS_IDX_ACTIVE / (GRBM_GUI_ACTIVE / 8 x 256 CUs); bank-conflict cycles as a share of it",
           "peak": "256 B/clk/CU = %.1f TB/s at 2.4 GHz" % (LDS_PEAK_GBS * 2 / 1e3)}
    for k, v in d["kernels"].items():
        for name in ("shadow_image_kernel<6144", "grasp_image_kernel<false>", "shadow_set_kernel"):
            if name in k:
                out[name] = {"frac": v["lds_util"], "conflict_share": v["lds_conflict"], "wait_any": v["wait_any"]}
    return out


PRE_POINTS, PRE_VOXEL, PRE_NORMALS_POINTS = 120000, 0.003, 30000
PRE_WORKSPACE = (-1.0, 1.0, -1.0, 1.0, -1.0, 1.0)  # cfg/eigen_params.cfg


def _preprocess_leg(ctx):
    """SURVEY §8f rank 2 (gpd_hip_preprocess_cloud): workspace cut + the reference's std::set voxeliser on a raw
    120k-point synthetic scan; not part of `value`."""
    import time
    import numpy as np
    from gpd_amd import synth
    raw = synth.make_cloud(4321, PRE_POINTS)
    xyz, cam = raw["xyz"], raw["cam_source"]
    ws = np.array(PRE_WORKSPACE)
    ctx.preprocess_cloud(xyz, cam, ws, PRE_VOXEL)
    t0 = time.perf_counter()
    v, _, _, ms = ctx.preprocess_cloud(xyz, cam, ws, PRE_VOXEL)
    wall = time.perf_counter() - t0
    # SURVEY §8f rank 1 on the same scan, voxelised to the grid the reference uses: Cloud::calculateNormals (radius 0.03)
    grid = synth.make_cloud(4321, PRE_NORMALS_POINTS)
    ctx.upload_cloud(grid["xyz"], np.zeros_like(grid["xyz"]), grid["cam_source"], grid["view_points"])
    ctx.estimate_normals(0.03)
    t0 = time.perf_counter()
    ctx.estimate_normals(0.03)
    n_wall = time.perf_counter() - t0
    return raw, {"points": int(len(xyz)), "kept": int(len(v)), "voxel_size": PRE_VOXEL, "kernel_ms": float(ms), "wall_ms_incl_pcie": wall * 1e3,
                 "normals": {"points": PRE_NORMALS_POINTS, "radius": 0.03, "wall_ms_incl_download": n_wall * 1e3},
                 "note": "Cloud::filterWorkspace + Cloud::voxelizeCloud: cut, voxel keys and the gather of the kept voxels on the device; the "
                         "voxeliser's keep / drop decisions are a strictly sequential chain and run as a table-driven spine walk on ONE host "
                         "core between two small copies (kernel_ms = first to last device operation, the walk included; "
                         "the same walk on one wavefront took 20 ms in rounds 1-2).  cpu_baseline.preprocess_ms is the reference's std::set on one core.  normals: gpd_hip_estimate_normals on a "
                         "30k-point cloud of the benchmark's density"}


def _cpu_preprocess_ms(raw):
    import time
    import oracle
    oracle.voxelize(raw["xyz"][:1000], PRE_VOXEL)
    t0 = time.perf_counter()
    oracle.voxelize(raw["xyz"], PRE_VOXEL)  # every point of the synthetic scan lies inside the workspace
    return (time.perf_counter() - t0) * 1e3


def _cpu_normals_ms():
    import time
    import oracle
    from gpd_amd import synth
    grid = synth.make_cloud(4321, PRE_NORMALS_POINTS)
    t0 = time.perf_counter()
    oracle.estimate_normals(grid["xyz"], grid["cam_source"], grid["view_points"], 0.03)  # OpenMP over the points, all host cores
    return (time.perf_counter() - t0) * 1e3


REF_LIVE_SAMPLES = 24  # samples of the in-run timing of the reference's own sources (~90 ms per candidate on one core: ~6 s)


def _reference_sources_live(cloud, w, C, si_bench):
    """oracle/_ref/libgpd_ref.so — the reference's OWN translation units (unmodified, through the test-only Eigen / PCL / OpenCV
    interface subsets, one thread: its OpenMP loops are racy) — timed HERE, on this host, on the first
    REF_LIVE_SAMPLES samples of the benchmark's own list: ImageGenerator::createImages + Classifier::classifyImages per candidate,
    as `value` counts.  None when the library is not in the tree (it is built where /root/reference exists and travels with the
    snapshot, like the product's own .so files).  Runs in a child process with a time limit: whatever happens inside the
    reference's code cannot take the line with it."""
    import subprocess
    import tempfile
    from oracle import ref
    if not ref.available():
        return None
    with tempfile.TemporaryDirectory(prefix="gpd_reflive_") as tmp:
        path = os.path.join(tmp, "in.npz")
        np.savez(path, C=np.array(C), si=np.ascontiguousarray(si_bench[:REF_LIVE_SAMPLES], np.int32), xyz=cloud["xyz"], normals=cloud["normals"],
                 cam_source=cloud["cam_source"], view_points=cloud["view_points"], **{"w_" + k: np.asarray(v) for k, v in w.items()})
        code = "import sys; sys.path.insert(0, %r); import bench; bench._reference_sources_child(%r)" % (ROOT, path)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, cwd=ROOT)
    for line in r.stdout.splitlines():
        if line.startswith("@@REF "):
            return json.loads(line[6:])
    raise RuntimeError("child rc %s: %s" % (r.returncode, r.stderr[-300:]))


def _reference_sources_child(path):
    """the child of _reference_sources_live: prints one '@@REF {json}' line"""
    import time
    import oracle
    from oracle import ref
    d = np.load(path)
    C = int(d["C"])
    w = {k[2:]: d[k] for k in d.files if k.startswith("w_")}
    p = oracle.default_params(C)
    si = d["si"]
    det = ref.Detector(p, weights=w)
    rc = ref.Cloud(d["xyz"], d["normals"], d["cam_source"], d["view_points"])
    try:
        rc.set_sample_indices(si)
        t0 = time.perf_counter()
        det.generate(rc, len(si))
        t_search = time.perf_counter() - t0
        valid = det.filter_workspace()
        n_valid = int(valid.sum())
        if n_valid == 0:
            print("@@REF null")
            return
        t0 = time.perf_counter()
        img, _ = det.images(rc, n_valid + 16)
        t_img = time.perf_counter() - t0
        t0 = time.perf_counter()
        det.classify(img)
        t_cls = time.perf_counter() - t0
    finally:
        det.close()
        rc.close()
    out = {"kind": "reference", "value": n_valid / (t_img + t_cls), "unit": "candidates/s", "cores": 1,
           "sample": "measured in this run on this host: the first %d samples of the benchmark's list -> %d candidates; the reference's "
                     "ImageGenerator::createImages %.2f s + Classifier::classifyImages %.2f s (generateGraspCandidates %.2f s not counted, "
                     "as in `value`); its own translation units through the test-only Eigen / PCL / OpenCV subsets (plain loops: the "
                     "reference on the real libraries is faster per core), one thread" % (len(si), n_valid, t_img, t_cls, t_search),
           "ms_per_candidate": {"images": t_img / n_valid * 1e3, "classify": t_cls / n_valid * 1e3}}
    sys.stdout.flush()
    print("@@REF " + json.dumps(out))
    sys.stdout.flush()


def _cpu_baseline(cloud, w, C, si_bench, n_cand_bench, n_samples):
    """The OpenMP oracle on the benchmark's OWN candidate list — the same cloud, the same samples, the first n_cand_bench valid
    hands — when `--cpu-samples` allows it (the default does: ~2 s on a 128-core host), else on the first n_samples samples."""
    import oracle
    from gpd_amd import synth
    p = oracle.default_params(C)
    same_list = n_samples >= 1500 and len(si_bench) <= 4000
    si = si_bench if same_list else synth.sample_indices(cloud, n_samples)
    cores = oracle.num_threads()
    oracle.detect(p, cloud["xyz"], cloud["normals"], cloud["cam_source"], cloud["view_points"], si[:16], w)  # warm-up
    _, n_cand, times = oracle.detect(p, cloud["xyz"], cloud["normals"], cloud["cam_source"], cloud["view_points"], si, w,
                                     max_cand=n_cand_bench if same_list else 0)
    n_samples = len(si)
    t = float(times[1] + times[2])
    ref_file = os.path.join(ROOT, "profiles", "r04_ref_cpu_baseline.json")
    ref_own = json.load(open(ref_file)) if os.path.exists(ref_file) else None
    ref_block = ref_own and dict(ref_own, note="NOT measured in this run: the reference's own translation units (through the test-only "
                                 "Eigen / PCL / OpenCV subsets, one thread) were not here (oracle/_ref is built where /root/reference exists and "
                                 "travels with the tree); timed in the build container on this workload's list by profiles/ref_cpu_baseline.py "
                                 "and committed as profiles/r04_ref_cpu_baseline.json")
    try:
        live = _reference_sources_live(cloud, w, C, si_bench)
    except Exception as e:  # the checker's checker must not cost the line
        live = None
        if ref_block is not None:
            ref_block["live_attempt_failed"] = repr(e)[:200]
    if live is not None:
        ref_block = dict(live, committed_full_list=ref_own and {k: ref_own[k] for k in ("value", "sample", "host") if k in ref_own})
    return {"value": n_cand / t, "unit": "candidates/s", "cores": cores, "kind": "port",
            "reference_sources": ref_block,
            "sample": "%d samples -> %s%d candidates of the same cloud%s; images %.2fs + LeNet %.2fs (search %.2fs not counted); "
                      "OpenMP CPU restatement (oracle/), not the reference binary"
                      % (n_samples, "the first " if same_list else "", n_cand, " = the list `value` is measured on" if same_list else "", times[1], times[2], times[0])}


if __name__ == "__main__":
    main()
