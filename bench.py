#!/usr/bin/env python3
"""bench.py - SDF query-points/sec at vox_res=128 (BASELINE.json metric) on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1 either way: under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` the
    ranks read RANK / LOCAL_RANK / WORLD_SIZE from the environment; started plainly with WORLD_SIZE unset,
    bench.py starts those N workers itself as a CHILD process - decided before anything touches the GPU - and
    relays rank 0's JSON line and the return code)

A "step" is one pass of the hot path over one batch of synthetic input with inputs
resident in HBM: for a batch of n_gpus images (one per rank's worth of work, "weak"
scaling) the per-image prologue + the fused decoder over every rank's share of each
image's (128+1)^3 grid (equal point ranges in memory order, rounded to kernel tiles), then -
for N > 1 - one RCCL all_gather that rebuilds the full occupancy grids on every rank
(zeroshape_amd/parallel.py).  For N > 1 every rank runs every image's prologue (0.5 ms at any batch up to 8, no
collective), the per-image f16x3-vs-fp32 output check of image i runs on rank i mod N only and the 8-byte verdicts are
all-gathered (parallel.prepare_sharded).  N = 1: one image, one full
129^3 grid, no collective.  value = grid points evaluated by all ranks / max-over-ranks
time.  Weights: seeded random (no checkpoint ships with the reference); latent_depth:
seeded N(0,1).

--precision selects the decoder arithmetic: "f16x3" (default; split-fp16 on the 16-bit matrix pipe,
csrc/sdf_decoder_split.hip: operands carried as two fp16 halves, ~2^-21 relative; max |logit
difference| to the exact-fp32 kernel ~3e-6 with no occupancy flip on the 129^3 grid - BASELINE.json's
contract is 1e-4 and its own config names bf16) or "f32" (exact-fp32 MFMA, csrc/sdf_decoder.hip).

A plain run sets up, warms up, times the K steps, writes the last step's outputs (--dump-outputs DIR: the occupancy
grids the step returned, DIR/occupancy.npy in float32 - the whole [batch, G, G, G] tensor up to 64 MiB, else a fixed
seeded sample of its points; the inputs are seeded, so two builds compare output for output) and prints the line:
metric / value / unit / higher_is_better / dtype / ms_per_step, the timed steps' own roofline and the calibration.
Everything else below takes runs of its own and comes only with --full (exact_f32, image_check, logit_scale_sweep,
roofline.power, cpu_baseline and the legs; --no-cpu-baseline / --no-extras / --skip-legs trim a --full run).

Extra objects on the JSON line:
  roofline     - the fused decoder kernel against the dense MFMA peak of its dtype (fp16/bf16 2,500 /
                 fp32 157.3 TFLOP/s, MI355X_MICROARCH.md): ALGORITHMIC 5.00 MFLOP/point (SURVEY.md
                 section 8d) x points per launch / mean launch duration from HIP events on the launch
                 stream.  For f16x3 every algorithmic product costs three fp16 MFMAs; the executed
                 matrix rate is reported beside it (`executed`).
  exact_f32    - (f16x3 runs, N = 1) the SAME timed contract (warmup + steps of prologue + launch + sigmoid between
                 barriers, launch event-timed inside each step) through the exact-fp32 kernel - the reference's own
                 arithmetic: ms_per_step, value, its roofline object - and the largest |logit| difference and the
                 occupancy flips between the two arithmetics on the full grid.
  virtual_ranks_8 / _4 / _2 - (N = 1) what ONE rank of `--gpus 8 / 4 / 2` does per step (batch N, its point range of every image),
                 timed for every rank in turn on this GPU; `bound` = the compute-side weak-scaling bound (tools/bench_legs.py).
  cpu_baseline - the oracle (torch-CPU fp32 restatement of the reference, "port") timed on
                 this host's cores on a bounded sample of x-slices of the same grid.
  calibration  - Implicit.prepare's once-per-weight-version verdict on the requested arithmetic: max |f16x3 - f32| logit
                 over 4096 probe points and the arithmetic it selected (2.5e-5 keeps f16x3, else the fp32 kernels run).
  chamfer / pose_search / chamfer_l1 / encoder / encoder_att / vox256 / inference / iso_surface / train_step / trained_weights
               - (N = 1, outside the timed region; tools/bench_legs.py) the rest of the BASELINE metric: the
                 Chamfer NN kernel on [24,10k]x[24,10k] with its fp32-VALU roofline fraction, bit equality
                 to the oracle and the oracle timed on the host (CPU leg ii); the 6912-rotation pose search
                 exhaustive and pruned; Chamfer-L1 against the oracle pipeline and across the two decoder
                 arithmetics; encoder forward B = 1 / 28 with the CPU restatement at B = 1 (CPU leg iii);
                 one training step at per-GPU batch 4; the two decoder arithmetics on weights trained for 304
                 iterations (full-grid difference + calibration verdict).  --no-extras skips them.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VOX_RES = 128
RANGE = (-1.5, 1.5)
FLOP_PER_POINT = 5.00e6          # SURVEY.md section 8d (algorithmic, fp32 reference)
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, exact f32
PEAK_F16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_{f16,bf16}, dense
# matrix work the kernels really execute per point (197 -> 224 latent padding included):
EXEC_FLOP_PER_POINT = {"f32": 39424 * 4096 / 32.0,        # 39,424 MFMAs of 32x32x2 per 32 points
                       "f16x3": 14784 * 32768 / 32.0}    # 14,784 MFMAs of 32x32x16 per 32 points
# HBM-side bytes per 129^3 launch come from a rocprofv3 PMC pass (FETCH_SIZE x2 per the gfx950
# correction + WRITE_SIZE, profiles/README.md) recorded in profiles/decoder_traffic.json together with
# the sha1 of the kernel source it was measured on: reported only while that source is unchanged,
# null (with the stale profile named) otherwise - never a constant that outlives the kernel.
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "decoder_traffic.json")
KERNEL_SOURCE = {"f32": "zeroshape_amd/csrc/sdf_decoder.hip", "f16x3": "zeroshape_amd/csrc/sdf_decoder_split.hip"}


def measured_traffic(precision):
    import hashlib
    try:
        rec = json.load(open(TRAFFIC_FILE))[precision]
        sha = hashlib.sha1(open(os.path.join(ROOT, KERNEL_SOURCE[precision]), "rb").read()).hexdigest()
    except (OSError, KeyError, ValueError):
        return None, None
    if rec.get("source_sha1") != sha:
        return None, "%s (stale: kernel source changed since)" % rec.get("profile")
    return rec["bytes_per_launch"], rec.get("profile")


def power_under_load(launch, seconds=1.6):
    """Socket power and engine clock (rocm-smi) while `launch` runs back to back: the split-fp16 decoder sits at the
    board's power limit, which is what caps its roofline fraction - reported next to it.  None where
    rocm-smi is missing."""
    import re
    import shutil
    import subprocess
    import threading

    import torch
    if shutil.which("rocm-smi") is None:
        return None
    samples, stop = [], threading.Event()

    def sampler():
        while not stop.is_set():
            try:
                out = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--csv"], capture_output=True, text=True,
                                     timeout=5).stdout.strip().split("\n")
                head, row = out[-2].split(","), out[-1].split(",")
                rec = dict(zip(head, row))
                pw = [float(v) for k, v in rec.items() if "Power" in k and re.match(r"^[0-9.]+$", v)]
                ck = [float(re.sub(r"[^0-9.]", "", v)) for k, v in rec.items() if k.startswith("sclk clock speed")]
                if pw and ck:
                    samples.append((pw[0], ck[0]))
            except Exception:
                pass
            stop.wait(0.15)

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    th = threading.Thread(target=sampler)
    th.start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(8):
            launch()
        torch.cuda.synchronize()
    stop.set()
    th.join()
    samples = samples[1:] if len(samples) > 2 else samples        # the first reading may predate the load
    if not samples:
        return None
    return {"socket_w": round(sum(p for p, _ in samples) / len(samples), 1), "sclk_mhz": round(sum(c for _, c in samples) / len(samples)),
            "samples": len(samples), "board_limit_w": 1400, "peak_sclk_mhz": 2400,
            "how": "rocm-smi every 0.15 s over %.1f s of back-to-back decoder launches" % seconds}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, occ):
    """--dump-outputs: what the last timed step returned - the occupancy grids [batch, G, G, G] - as DIR/occupancy.npy in
    float32: the whole tensor when it fits in 64 MiB, else a fixed seeded sample of its points in memory order."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    flat = occ.detach().reshape(-1)
    if flat.numel() * 4 > DUMP_LIMIT_BYTES:
        idx = np.unique(np.random.default_rng(0).integers(0, flat.numel(), DUMP_LIMIT_BYTES // 8))
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    out = flat.float().cpu().numpy()
    if out.size == occ.numel():
        out = out.reshape(tuple(occ.shape))
    np.save(os.path.join(path, "occupancy.npy"), out)


def self_launch(n_gpus, argv):
    """`python bench.py --gpus N` with WORLD_SIZE unset: run the N ranks under torch.distributed.run as a child
    process (never an exec: this process must not have initialised HIP, and it has not - torch is not even imported
    yet), pass its output through and return its exit code."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC only on this pool (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.run(cmd, env=env)
    return proc.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vox-res", type=int, default=VOX_RES)
    ap.add_argument("--precision", choices=("f16x3", "f32"), default="f16x3")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's occupancy grids to DIR/occupancy.npy (float32, at most 64 MiB)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: the exact-fp32 contract, the image-check A/B, power, "
                         "the CPU baseline and the legs of tools/bench_legs.py (a plain run times the steps only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU oracle baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full without the image-check A/B, the power reading and the Chamfer / pose-search / evaluation / "
                         "encoder / training legs (tools/bench_legs.py)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--skip-legs", default="",
                    help="comma-separated extra legs to leave out (names of the line's objects, plus 'chamfer_l1_vox128' for the "
                         "CPU-oracle pipeline at vox 128 inside chamfer_l1); the test suite skips the legs its own tests cover")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))

    import numpy as np
    import torch
    import torch.distributed as dist

    from zeroshape_amd import parallel, synthetic as syn
    from zeroshape_amd.model.shape.implicit import Implicit
    from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started inside a WORLD_SIZE=%d job" % (args.gpus, world))
    if os.environ.get("ZS_BENCH_RENDEZVOUS_ONLY"):
        # launch-path check for boxes without a GPU (tests/test_bench_launch.py): the ranks meet over gloo, agree on
        # the world size, rank 0 prints one JSON line - nothing below runs
        total = torch.ones(1)
        if world > 1:
            dist.init_process_group("gloo")
            dist.all_reduce(total)
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"rendezvous_only": True, "n_gpus": int(total.item()), "steps": args.steps}), flush=True)
        return
    # ZS_DEVICE_OVERRIDE / ZS_DIST_BACKEND exist only to rehearse the multi-rank code path on a
    # single-GPU box (all ranks on one device, gloo instead of RCCL); never set by the driver
    dev_index = int(os.environ.get("ZS_DEVICE_OVERRIDE", local_rank))
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        backend = os.environ.get("ZS_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    N = args.vox_res
    G = N + 1
    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(0, pos_embed=pe).items()}
    net = Implicit(syn.NUM_PATCHES, latent_dim=256, n_channels=256, n_blocks_attn=2, n_layers_mlp=8,
                   num_heads=8, skip_in=[2, 4, 6], pos_perlayer=False)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    net.precision = args.precision
    batch = world                                  # weak scaling: one image of work per rank
    latent = torch.from_numpy(syn.seeded_latent(0, batch)).to(dev)
    axis = torch.linspace(RANGE[0], RANGE[1], G, device=dev)
    net.packed(dev)                                # pack weights once, outside the timed region
    # the once-per-weight-version calibration of the default arithmetic (Implicit.prepare: 4096 probe points through
    # both kernels, one host read) happens here, outside the timed region, like the packing; its verdict decides
    # which kernel the timed steps run and is reported on the line
    st0 = net.prepare(latent)
    # the timed steps return occupancies (apply_sigmoid=True): the arithmetic they run is the state's verdict in THAT space
    precision_run = "f16x3" if st0.precision == "f16x3" and st0.occ_ok else "f32"
    calibration = net.last_calibration
    stream = torch.cuda.current_stream(dev)       # the stream the C ABI launches on

    def step(events=None, precision=None):
        # per-image prologue (all images, every rank; None: the configured arithmetic); N > 1: the per-image output check of
        # image i on rank i % N, verdicts all-gathered (parallel.prepare_sharded)
        st = net.prepare(latent, precision) if world == 1 else parallel.prepare_sharded(net, latent, precision=precision)

        def query(b, e):
            # the decoder launch of this step between two HIP events on its own stream (roofline.launch_ms_*: measured INSIDE the
            # timed steps, so launch time <= step time by construction)
            if events is None:
                return net.query_grid_range(latent, axis, b, e, apply_sigmoid=True, state=st)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = net.query_grid_range(latent, axis, b, e, apply_sigmoid=True, state=st)
            e1.record(stream)
            events.append((e0, e1))
            return out
        return parallel.sharded_level_grid_points(query, G)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        occ = step()
    barrier()
    step_events = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        occ = step(step_events)
    barrier()
    dt = time.perf_counter() - t0
    kern_ms = sorted(a_.elapsed_time(b_) for a_, b_ in step_events)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert occ.shape == (batch, G, G, G)
    points_per_step = batch * G ** 3
    value = points_per_step * args.steps / dt
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, occ)

    # what prepare()'s per-image output check (on by default since round 4; Implicit._launch_image_check) costs the step:
    # the same timed loop without it (round 3's behaviour)
    image_check = None
    if args.full and world == 1 and precision_run == "f16x3" and getattr(net, "image_check", False) and not args.no_extras:
        net.image_check = False
        for _ in range(max(1, args.warmup)):
            step()
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        dt0 = time.perf_counter() - t1
        net.image_check = True
        image_check = {"on": True, "ms_per_step_without": round(dt0 / args.steps * 1e3, 3),
                       "value_without": round(points_per_step * args.steps / dt0, 1),
                       "what": "per-image f16x3-vs-fp32 probe of every prepare() on side streams beside the grid launch"}

    # ---- roofline of the dominant kernel: HIP events around decoder launches only -------
    b, e, _ = parallel.point_bounds(G ** 3, world, rank)
    pts_launch = batch * (e - b)

    def roofline_of(precision, kern_ms):
        mean = sum(kern_ms) / len(kern_ms)
        peak = PEAK_F16_MFMA_TFLOPS if precision == "f16x3" else PEAK_F32_MFMA_TFLOPS
        achieved = pts_launch * FLOP_PER_POINT / (mean * 1e-3) / 1e12
        executed = pts_launch * EXEC_FLOP_PER_POINT[precision] / (mean * 1e-3) / 1e12
        traffic, src = measured_traffic(precision) if (N == 128 and world == 1) else (None, None)
        return {"bound": "mfma",
                "kernel": "sdf_decode_split_kernel<GRID>" if precision == "f16x3" else "sdf_decode_kernel<GRID>",
                "achieved": round(achieved, 3), "peak": peak, "unit": "TFLOP/s",
                "frac": round(achieved / peak, 4),
                "executed": round(executed, 3), "executed_frac": round(executed / peak, 4),
                "traffic": traffic, "traffic_unit": "bytes/launch", "traffic_source": src,
                "points_per_launch": pts_launch, "launch_ms_mean": round(mean, 4),
                "launch_ms_min": round(kern_ms[0], 4), "algorithmic_flop_per_point": FLOP_PER_POINT}

    roofline = roofline_of(precision_run, kern_ms)          # the launches of the timed steps themselves
    roofline["launch_ms_source"] = "HIP events around the decoder launch inside each of the %d timed steps" % args.steps
    if args.full and world == 1 and not args.no_extras:
        st = net.prepare(latent)
        roofline["power"] = power_under_load(
            lambda: net.query_grid_range(latent, axis, b, e, apply_sigmoid=True, state=st))

    exact_f32 = None
    logit_sweep = None
    if args.full and precision_run == "f16x3" and world == 1:
        # the SAME timed contract in the reference's own arithmetic (options/shape.yaml:96 amp false; implicit.py:251-288 is
        # fp32): `warmup` untimed + `steps` timed steps of prologue + exact-fp32 launch + sigmoid between the same barriers, the
        # launch event-timed inside each step - the like-for-like-precision number, driver-checkable (ms_per_step x steps)
        for _ in range(args.warmup):
            step(precision="f32")
        barrier()
        ev32 = []
        t32 = time.perf_counter()
        for _ in range(args.steps):
            step(ev32, precision="f32")
        barrier()
        dt32 = time.perf_counter() - t32
        ms32 = sorted(a_.elapsed_time(b_) for a_, b_ in ev32)
        r32 = roofline_of("f32", ms32)
        r32["launch_ms_source"] = "HIP events around the decoder launch inside each of the %d timed fp32 steps" % args.steps
        st32 = net.prepare(latent, "f32")
        lg = net.query_grid(latent, axis, apply_sigmoid=False, state=net.prepare(latent))
        lg32 = net.query_grid(latent, axis, apply_sigmoid=False, state=st32)
        flips = (lg > 0) != (lg32 > 0)
        exact_f32 = {"value": round(points_per_step * args.steps / dt32, 1), "unit": "points/s",
                     "ms_per_step": round(dt32 / args.steps * 1e3, 3), "steps": args.steps, "warmup": args.warmup,
                     "dtype": "f32", "roofline": r32,
                     "launch_ms_mean": r32["launch_ms_mean"], "roofline_frac": r32["frac"],
                     "roofline_peak": r32["peak"],
                     "max_abs_logit_diff": float((lg - lg32).abs().max()),
                     "occupancy_flips": int(flips.sum()), "points": int(lg.numel()),
                     "max_abs_logit_at_flip": float(lg32[flips].abs().max()) if int(flips.sum()) else 0.0}
        del lg, lg32
        if not args.no_extras and "logit_scale_sweep" not in args.skip_legs.split(","):
            from tools import bench_legs as legs
            try:
                logit_sweep = legs.logit_sweep_leg(dev, sd)
            except Exception as ex:                     # a leg must never take the headline line down
                logit_sweep = {"error": "%s: %s" % (type(ex).__name__, ex)}

    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import decoder_ref
        grid = decoder_ref.dense_grid(RANGE[0], RANGE[1], N)
        lat_c = latent[:1].cpu()
        sl = [int(i) for i in np.linspace(0, N, 33).round()]        # evenly spaced x-slices
        # torch's intra-op pool does not scale to every core of a big host on these small
        # ops: pick the fastest thread count on one slice each, then time the sample with it
        ncpu = os.cpu_count() or 1
        best = None
        for th in sorted(set(min(t, ncpu) for t in (8, 16, 32, 64))):
            torch.set_num_threads(th)
            decoder_ref.level_grid(sd, lat_c, grid, slices=[sl[0]])  # warm-up, untimed
            t1 = time.perf_counter()
            decoder_ref.level_grid(sd, lat_c, grid, slices=[sl[1]])
            el = time.perf_counter() - t1
            if best is None or el < best[1]:
                best = (th, el)
        torch.set_num_threads(best[0])
        cores = best[0]
        done, t1 = 0, time.perf_counter()
        for i in sl:
            decoder_ref.level_grid(sd, lat_c, grid, slices=[i])
            done += 1
            if time.perf_counter() - t1 > args.cpu_seconds and done >= 2:
                break
        cdt = time.perf_counter() - t1
        cpu_baseline = {"value": round(done * G * G / cdt, 1), "unit": "points/s", "cores": cores,
                        "kind": "port",
                        "sample": "%d evenly spaced x-slices of the %d^3 grid (%d points), oracle/"
                                  "decoder_ref.level_grid, torch-CPU fp32, %.1f s; %d of the host's %d cores: the fastest of "
                                  "8/16/32/64 torch intra-op threads on one slice (these small per-slice ops stop "
                                  "scaling beyond that)" % (done, G, done * G * G, cdt, cores, ncpu)}
        # the same restatement over the FULL grids of configs 0 / 2 (vox_res 32 and 64)
        if N == VOX_RES:
            full = {}
            for n_small in (32, 64):
                g_small = decoder_ref.dense_grid(RANGE[0], RANGE[1], n_small)
                t1 = time.perf_counter()
                decoder_ref.level_grid(sd, lat_c, g_small)
                el = time.perf_counter() - t1
                full["vox%d" % n_small] = {"points": (n_small + 1) ** 3, "seconds": round(el, 2),
                                           "value": round((n_small + 1) ** 3 / el, 1), "unit": "points/s"}
            cpu_baseline["full_grids"] = full

    extras = {}
    if args.full and rank == 0 and world == 1 and not args.no_extras and N == VOX_RES:
        from tools import bench_legs as legs
        cpu = not args.no_cpu_baseline
        skip = set(args.skip_legs.split(","))
        for name, fn in (("chamfer", lambda: legs.chamfer_leg(dev, cpu)), ("pose_search", lambda: legs.pose_search_leg(dev)),
                         ("chamfer_l1", lambda: legs.eval_leg(dev, net, sd, vox128="chamfer_l1_vox128" not in skip)),
                         ("encoder", lambda: legs.encoder_leg(dev, cpu)),
                         ("encoder_att", lambda: legs.encoder_att_leg(dev)), ("vox256", lambda: legs.vox256_leg(dev, net)),
                         ("virtual_ranks_8", lambda: legs.virtual_ranks_leg(dev, net)),
                         ("virtual_ranks_4", lambda: legs.virtual_ranks_leg(dev, net, world=4)),
                         ("virtual_ranks_2", lambda: legs.virtual_ranks_leg(dev, net, world=2)),
                         ("inference", lambda: legs.inference_leg(dev)), ("iso_surface", lambda: legs.surface_leg(dev)),
                         ("train_step", lambda: legs.in_subprocess("train", "train_step")),
                         ("trained_weights", lambda: legs.in_subprocess("trained", "trained_weights"))):
            if name in skip:
                continue
            try:
                extras[name] = fn()
            except Exception as e:                      # a leg must never take the headline line down
                extras[name] = {"error": "%s: %s" % (type(e).__name__, e)}

    if rank == 0:
        line = {
            "metric": "sdf_query_points_per_sec_vox%d" % N, "value": round(value, 1),
            "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": precision_run, "data": "synthetic",
            "config": {"workload": "compute_level_grid vox_res=%d: (%d+1)^3 = %d points/image, "
                                   "range [-1.5,1.5], prologue + fused decoder (%s) + sigmoid; batch = "
                                   "n_gpus images, each sharded into equal point ranges, RCCL all_gather for n_gpus>1"
                                   % (N, N, G ** 3, precision_run),
                       "global_batch_images": batch, "points_per_step": points_per_step,
                       "weights": "seeded random (zeroshape_amd/synthetic.py)"},
            "roofline": roofline, "cpu_baseline": cpu_baseline,
            # Implicit.prepare's verdict on these weights: max |f16x3 - f32| logit over the probe points, and the
            # arithmetic it selected (requested: --precision)
            "calibration": dict({k: (v.detach().cpu().tolist() if hasattr(v, "detach") else v) for k, v in (calibration or {}).items()},
                                requested=args.precision),
        }
        if exact_f32 is not None:
            line["exact_f32"] = exact_f32
        if image_check is not None:
            line["image_check"] = image_check
        if logit_sweep is not None:
            line["logit_scale_sweep"] = logit_sweep
        line.update(extras)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
