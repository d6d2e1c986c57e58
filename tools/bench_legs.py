#!/usr/bin/env python3
"""The rest of the BASELINE metric beside bench.py's timed region (N = 1, rank 0, outside the timed
steps): Chamfer NN kernel, 6912-rotation pose search, Chamfer-L1 of a whole evaluation sample
against the oracle pipeline and across the two decoder arithmetics, encoder forward (B = 1 / 28),
one training step (B = 4), and SURVEY.md section 8d's CPU legs (ii) Chamfer and (iii) encoder B = 1.
Every function returns one JSON-able dict and bounds its own run time; bench.py prints them as
extra objects of its line.  Stand-alone:  python tools/bench_legs.py [chamfer pose eval encoder train]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_VALU_TFLOPS = 157.3        # MI355X_MICROARCH.md
FLOP_PER_PAIR = 8                   # 3 sub, 1 mul, 2 fma, 1 cmp, 1 select
GFLOP_DPT, GFLOP_RES, GFLOP_INTR = 2 * 41.3, 2 * 5.0, 2 * 1.0     # per 224^2 image, DESIGN.md 10.3


def _events(fn, reps, stream=None):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record(stream)
    for i in range(reps):
        fn()
        ev[i + 1].record(stream)
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    # (median, minimum): one host stall inside ten 2.7 ms replays (a round-5 line: ms 4.70 next to ms_min 2.61) is not the leg's time
    return 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2]), ms[0]


def chamfer_leg(dev, cpu=True):
    """[24,10k] x [24,10k]: the brute-force scan kernel (roofline-graded: fp32 VALU, 8 flop per
    pair), the grid-accelerated exact kernel, bit equality against the oracle, and the oracle itself timed
    on this host's cores (CPU leg ii: plain C + OpenMP port of chamfer3D.cu:12-134)."""
    from zeroshape_amd import synthetic as syn
    from zeroshape_amd.external.chamfer3D.dist_chamfer_3D import chamfer_3DDist
    B, n, m = 24, 10000, 10000
    a_h, b_h = syn.seeded_cloud(1, B, n), syn.seeded_cloud(2, B, m)
    a, b = torch.from_numpy(a_h).to(dev), torch.from_numpy(b_h).to(dev)
    ch = chamfer_3DDist()
    ms_brute, min_brute = _events(lambda: ch(a, b, "brute"), 10)
    ms_grid, _ = _events(lambda: ch(a, b, "grid"), 10)
    ms_auto, _ = _events(lambda: ch(a, b), 10)
    pairs = 2.0 * B * n * m
    from zeroshape_amd import chamfer_3D as plugin
    auto_is_grid = max(n, m) >= plugin.GRID_MIN_POINTS
    # zs_chamfer_forward's scan: candidates as scalar operands of packed fp32 instructions
    brute_kernel = "nn_both_sgpr_kernel<2>"
    out = {"shape": [B, n, m], "ms": round(ms_brute, 4), "ms_min": round(min_brute, 4),
           "tpairs_per_s": round(pairs / (ms_brute * 1e-3) / 1e12, 3),
           "roofline": {"bound": "valu_f32", "achieved": round(pairs * FLOP_PER_PAIR / (ms_brute * 1e-3) / 1e12, 2),
                        "peak": PEAK_F32_VALU_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(pairs * FLOP_PER_PAIR / (ms_brute * 1e-3) / 1e12 / PEAK_F32_VALU_TFLOPS, 4),
                        "kernel": brute_kernel, "flop_per_pair": FLOP_PER_PAIR},
           "grid_accelerated_ms": round(ms_grid, 4),
           # the kernel chamfer_distance(..., method="auto") - the default of every caller - launches at this size:
           # the exact grid walk evaluates ~10^2 of the 10^4 candidates per query, so its rate is quoted against the
           # ALGORITHMIC pairs of the call (what the reference's kernel evaluates) and may exceed the VALU roofline
           # of the all-pairs form; the walk itself is latency / divergence bound, not on any roofline
           "auto": {"kernel": "nn_grid_kernel (csrc/chamfer_grid.hip)" if auto_is_grid else brute_kernel,
                    "ms": round(ms_auto, 4),
                    "all_pairs_equivalent_tpairs_per_s": round(pairs / (ms_auto * 1e-3) / 1e12, 3),
                    # all-pairs-EQUIVALENT rate: the grid kernel skips most pairs, so this is how fast an all-pairs scan would have to
                    # run to match it - not a utilisation of the VALU
                    "all_pairs_equivalent_frac_of_valu_peak": round(pairs * FLOP_PER_PAIR / (ms_auto * 1e-3) / 1e12 / PEAK_F32_VALU_TFLOPS, 4),
                    "all_pairs_equivalent_note": "pairs the brute-force scan would evaluate / time; the grid kernel evaluates a fraction of them",
                    "speedup_over_brute": round(ms_brute / ms_auto, 2)}}
    if cpu:
        from oracle import chamfer_ref
        t0 = time.perf_counter()
        w = chamfer_ref.chamfer_forward(a_h, b_h)
        dt = time.perf_counter() - t0
        d1, d2, i1, i2 = ch(a, b, "brute")
        g1, g2, j1, j2 = ch(a, b, "grid")
        out["bit_equal_to_oracle"] = bool(
            np.array_equal(d1.cpu().numpy(), w[0]) and np.array_equal(d2.cpu().numpy(), w[1]) and
            np.array_equal(i1.cpu().numpy(), w[2]) and np.array_equal(i2.cpu().numpy(), w[3]) and
            torch.equal(d1, g1) and torch.equal(i1, j1) and torch.equal(d2, g2) and torch.equal(i2, j2))
        out["cpu_baseline"] = {"value": round(pairs / dt / 1e12, 5), "unit": "Tpairs/s", "seconds": round(dt, 2),
                               "cores": os.cpu_count(), "kind": "port",
                               "sample": "one [24,10000]x[24,10000] call, oracle/chamfer_ref.c (C + OpenMP, all cores)"}
    return out


def pose_search_leg(dev):
    """brute_force_search (utils/eval_3D.py:140-170) over the 6912-rotation sphere, 10k x 10k points: the
    exhaustive scan, and the lower-bound pruned scan for an alignable and for an unrelated ground truth."""
    from zeroshape_amd import synthetic as syn
    from zeroshape_amd.utils import eval_3D as E
    n = 10000
    pred = torch.from_numpy(syn.ellipsoid_cloud(0, n)).to(dev)
    R = E._rotation_sphere(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    gt = ((R[1234] @ pred.T).T.contiguous().cpu() + 1e-3 * torch.randn(n, 3, generator=g)).to(dev)
    far = torch.from_numpy(syn.seeded_cloud(9, 1, n)[0]).to(dev)

    def run(gt_, prune, nn=None):
        E.brute_force_search(pred, gt_, device=dev, prune=prune, nn=nn)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = E.brute_force_search(pred, gt_, device=dev, prune=prune, return_index=True, nn=nn)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, o
    ms_ex, o_ex = run(gt, False)
    s_ex = E.brute_force_search.last_scanned
    ms_pr, o_pr = run(gt, True)
    n_pr, s_pr = E.brute_force_search.last_evaluated, E.brute_force_search.last_scanned
    ms_far, o_far = run(far, True)
    n_far, s_far = E.brute_force_search.last_evaluated, E.brute_force_search.last_scanned
    pairs = 6912 * 2.0 * n * n
    # the search that cannot drop a rotation (unrelated ground truth: all 6912 are scanned in full).  Since round 3 the
    # scan is box-culled: ALGORITHMIC pairs (what the reference's all-pairs kernels evaluate, 2 n m per rotation) per
    # second, the fraction of them the kernel really evaluates (from the counting build, profiles/r03_pose_pairs.json:
    # tools/pose_pairs.py) and the executed rate against the fp32 VALU peak; the alignable searches also drop most
    # rotations after 5-35 % of their queries (staged drop, exact)
    evaluated = None
    try:
        evaluated = json.load(open(os.path.join(ROOT, "profiles", "r03_pose_pairs.json")))["str/unalignable"]["fraction"]
    except (OSError, KeyError, ValueError):
        pass
    ms_brute, _ = run(far, False, "brute")
    executed = pairs * (s_far / 6912.0) * (evaluated or 1.0)
    return {"rotations": 6912, "points": [n, n], "nn": "cull (box-culled scan on STR-sorted clouds)",
            "exhaustive_ms": round(ms_ex, 2), "exhaustive_rotations_scanned_in_full": s_ex,
            "pruned_ms": round(ms_pr, 2), "pruned_rotations_evaluated": n_pr, "pruned_rotations_scanned_in_full": s_pr,
            "pruned_equals_exhaustive": bool(o_ex[5] == o_pr[5] and o_ex[6] == o_pr[6] and torch.equal(o_ex[3], o_pr[3])),
            "best_index": int(o_ex[5]), "best_cd": float(o_ex[6]),
            "unalignable_gt_pruned_ms": round(ms_far, 2), "unalignable_gt_rotations_evaluated": n_far,
            "unalignable_gt_rotations_scanned_in_full": s_far,
            "full_scan_algorithmic_tpairs_per_s": round(pairs * (s_far / 6912.0) / (ms_far * 1e-3) / 1e12, 3),
            "full_scan_pairs_evaluated_fraction": evaluated,
            "full_scan_pairs_evaluated_source": "profiles/r03_pose_pairs.json (counting build of csrc/pose_search.hip)",
            "full_scan_executed_tpairs_per_s": round(executed / (ms_far * 1e-3) / 1e12, 3),
            "full_scan_executed_frac_of_fp32_valu_peak": round(executed * FLOP_PER_PAIR / (ms_far * 1e-3) / 1e12 / PEAK_F32_VALU_TFLOPS, 4),
            # round 2's LDS-staged all-pairs kernel on the same sorted clouds (bit-identical record): the roofline-graded form
            "all_pairs_kernel_unalignable_ms": round(ms_brute, 2),
            "all_pairs_kernel_tpairs_per_s": round(pairs / (ms_brute * 1e-3) / 1e12, 3),
            "all_pairs_kernel_frac_of_fp32_valu_peak": round(pairs * FLOP_PER_PAIR / (ms_brute * 1e-3) / 1e12 / PEAK_F32_VALU_TFLOPS, 4)}


def eval_leg(dev, net, sd, vox128=True):
    """Chamfer-L1 (utils/eval_3D.py:136-137) of whole evaluation samples: (a) the HIP pipeline (decoder ->
    marching cubes -> sampling -> normalise -> Chamfer) against the same pipeline built from the oracle's
    pieces on the CPU at vox_res 16 and 64 (tests/test_gpu_eval_pipeline.py, which also runs one sample at vox 128); (b) the split-fp16 against the
    exact-fp32 decoder on the 129^3 grid of the headline workload."""
    from oracle import decoder_ref as R, geometry_ref as G, mc_ref as M
    from zeroshape_amd import synthetic as syn
    from zeroshape_amd.utils import eval_3D as E
    from zeroshape_amd.utils.options import EasyDict as edict

    def opt_of(N, P):
        return edict(dict(device=str(dev), H=224, W=224, arch=dict(win_size=16), data=dict(dataset_test="synthetic"),
                          eval=dict(vox_res=N, range=[-1.5, 1.5], num_points=P, icp=False, brute_force=False,
                                    f_thresholds=[0.005, 0.01, 0.02, 0.05, 0.1, 0.2])))

    def var_of(latent, gt):
        B = latent.shape[0]
        return edict(dict(idx=list(range(B)), latent_depth=latent.to(dev), latent_semantic=None,
                          rgb_input_map=torch.zeros(B, 3, 224, 224, device=dev),
                          pose_gt=torch.eye(3, 4)[None].repeat(B, 1, 1).to(dev), dpc=dict(points=gt.clone().to(dev))))
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2))
    gt = torch.from_numpy(syn.seeded_cloud(5, 2, 1500, -1, 1))
    worst, tri_count = {}, {}
    # the CPU oracle's decoder stops scaling at ~32 torch threads (bench.py's cpu_baseline); a big host's default is every core
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    for N, P, B in ((16, 2000, 2), (64, 4000, 2)) + (((128, 10000, 1),) if vox128 else ()):      # vox 64 = BASELINE config 2, vox 128 = the size the metric is quoted at
        var = var_of(latent[:B], gt[:B])
        E.eval_metrics(opt_of(N, P), var, net)
        occ = R.level_grid(sd, latent[:B], R.dense_grid(-1.5, 1.5, N, B))
        w = 0.0
        for b in range(B):
            tris = M.marching_cubes(occ[b].numpy(), 0.5, np.float32(3.0 / (N + 1)), -1.5)
            pts, _ = M.sample_surface(tris, P, seed=b)
            d1, d2, _, _ = G.chamfer_distance(G.normalize_pc(torch.from_numpy(pts)[None]), G.normalize_pc(gt[b][None]))
            w = max(w, abs(float(d1.mean()) - float(var.cd_acc[b])), abs(float(d2.mean()) - float(var.cd_comp[b])))
            tri_count[N] = len(tris)
        worst[N] = w
    res = {}
    prev = net.precision
    try:
        for prec in ("f32", "f16x3"):
            net.precision = prec
            v = var_of(latent[:1], torch.from_numpy(syn.seeded_cloud(6, 1, 10000, -0.6, 0.6)))
            E.eval_metrics(opt_of(128, 10000), v, net)
            res[prec] = v
    finally:
        net.precision = prev
    a, b = res["f32"], res["f16x3"]
    return {"chamfer_l1_vs_oracle_pipeline_vox16": float(worst[16]), "chamfer_l1_vs_oracle_pipeline_vox64": float(worst[64]),
            "chamfer_l1_vs_oracle_pipeline_vox128": float(worst[128]) if vox128 else None,
            "oracle_triangles_vox64": int(tri_count[64]), "oracle_triangles_vox128": int(tri_count[128]) if vox128 else None,
            "contract": 1e-4,
            "chamfer_l1_f16x3_vs_f32_vox128": float(max((a.cd_acc - b.cd_acc).abs().max(), (a.cd_comp - b.cd_comp).abs().max())),
            "chamfer_l1_vox128": float((a.cd_acc + a.cd_comp) / 2)}


def logit_sweep_leg(dev, sd, targets=(None, 30.0, 60.0, 100.0), N=64):
    """the f16x3 verdict at the logit scales of a confident checkpoint.  The seeded network with its last
    three MLP layers scaled (synthetic.confident_state_dict) until max |logit| over the probe points is ~30 / 60 / 100: what Implicit.prepare
    measures (raw-logit rule, occupancy rule), which arithmetic each kind of call then runs, and the whole vox-64 grid of
    both kinds against the exact-fp32 kernel."""
    from zeroshape_amd import synthetic as syn
    from zeroshape_amd.model.shape.implicit import Implicit
    latent = torch.from_numpy(syn.seeded_latent(0, 1)).to(dev)
    axis = torch.linspace(-1.5, 1.5, N + 1, device=dev)
    rows, gain = [], 1.0
    for target in targets:
        for _ in range(4):                   # the scale is not exactly linear in the gain: iterate towards the target
            net = Implicit(syn.NUM_PATCHES, latent_dim=256, n_channels=256, n_blocks_attn=2, n_layers_mlp=8,
                           num_heads=8, skip_in=[2, 4, 6], pos_perlayer=False)
            net.load_state_dict(syn.confident_state_dict(sd, gain), strict=True)
            net = net.to(dev).eval()
            st = net.prepare(latent)
            cal = net.last_calibration
            if cal is None:
                raise RuntimeError("gain %.1f left the host envelope (program.W_MAX)" % gain)
            if target is None or 0.8 * target < cal["max_abs_logit"] < 1.25 * target:
                break
            gain *= target / cal["max_abs_logit"]
        st32 = net.prepare(latent, "f32")
        occ, occ32 = (net.query_grid(latent, axis, apply_sigmoid=True, state=s_) for s_ in (st, st32))
        lg, lg32 = (net.query_grid(latent, axis, apply_sigmoid=False, state=s_) for s_ in (st, st32))
        flips = ((occ > 0.5) != (occ32 > 0.5)) & (lg32.abs() >= net.FLIP_BAND)
        rows.append({"gain": round(gain, 2), "max_abs_logit": round(cal["max_abs_logit"], 3),
                     "probe_max_abs_dlogit": cal["max_abs_diff"], "probe_max_abs_docc": cal["max_abs_occ_diff"],
                     "probe_flips_outside_band": cal["flips_outside_band"],
                     "selected_raw_logits": cal["selected"], "selected_occupancy": cal["selected_occ"],
                     "grid_max_abs_docc": float((occ - occ32).abs().max()), "grid_flips_outside_band": int(flips.sum()),
                     "grid_max_abs_dlogit_as_returned": float((lg - lg32).abs().max()),
                     "state_precision": st.precision})
    return {"what": "last three MLP layers x gain^(1/3) (synthetic.confident_state_dict); vox %d grid vs the exact-fp32 kernel; rules: raw logits |d| <= %.1e, occupancy |d| <= %.1e and "
                    "no flip outside |logit| < %.0e" % (N, Implicit.CALIBRATION_TOL, Implicit.CALIBRATION_TOL_OCC, Implicit.FLIP_BAND),
            "rows": rows}


def surface_leg(dev, iters=10):
    """convert_to_explicit's device path (utils/eval_3D.py:233-263): marching cubes + 10k area-weighted samples of a
    level grid resident in HBM, vox_res 128 and 256 (BASELINE configs 3 / 5).  The two grid passes (count, emit)
    read G^3 * 4 B each; `grid_gb_per_s` prices them against the whole call, `count_gb_per_s` the first pass alone
    (HIP events around zs_mc_count's launches)."""
    from zeroshape_amd import _lib
    from zeroshape_amd.utils import eval_3D as E
    out = {}
    lib = _lib.load()
    for N in (128, 256):
        G = N + 1
        ax = torch.linspace(-1.5, 1.5, G, device=dev)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        vol = torch.sigmoid(-20.0 * (torch.sqrt(x * x + 1.3 * y * y + 0.8 * z * z) - 0.9)).contiguous()   # an ellipsoid
        tris, pts = E.extract_surface(vol, 0.5, -1.5, 1.5, num_points=10000)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            tris, pts = E.extract_surface(vol, 0.5, -1.5, 1.5, num_points=10000)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / iters * 1e3
        tab, cnt, stride = E._mc_tables(dev)
        scratch = torch.empty(lib.zs_mc_scratch_bytes(G) // 4 + 1, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int32, device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(iters):
            _lib.check(lib.zs_mc_count(_lib.ptr(vol), G, 0.5, _lib.ptr(cnt), _lib.ptr(scratch), _lib.ptr(total),
                                       _lib.current_stream_ptr(dev)), "zs_mc_count")
        ev[1].record()
        torch.cuda.synchronize()
        count_ms = ev[0].elapsed_time(ev[1]) / iters
        gbytes = G ** 3 * 4 / 1e9
        out["vox%d" % N] = {"ms": round(ms, 3), "triangles": int(tris.shape[0]), "grid_mb": round(gbytes * 1e3, 1),
                            "grid_gb_per_s": round(2 * gbytes / (ms * 1e-3), 1),
                            "count_pass_ms": round(count_ms, 4), "count_gb_per_s": round(gbytes / (count_ms * 1e-3), 1)}
    out["hbm_peak_gb_per_s"] = 8000.0
    return out


def _graph(dev, encoder="resnet"):
    from zeroshape_amd.model.compute_graph.graph_shape import Graph
    from zeroshape_amd.utils.options import EasyDict as edict
    opt = edict(dict(H=224, W=224, device=str(dev), pretrain=dict(depth=None),
                     arch=dict(num_heads=8, latent_dim=256, win_size=16,
                               depth=dict(encoder=encoder, n_blocks=12, dsp=2, pretrained=None),
                               rgb=dict(encoder=None, n_blocks=12),
                               impl=dict(n_channels=256, att_blocks=2, mlp_ratio=4., posenc_perlayer=False,
                                         mlp_layers=8, posenc_3D=0, skip_in=[2, 4, 6]))))
    torch.manual_seed(0)
    g = Graph(opt)
    with torch.no_grad():
        torch.nn.init.normal_(g.intr_proj.weight, std=0.01)
    return opt, g.to(dev).eval()


def _profiled_kernels_per_forward(path, forwards=11):
    """Kernel launches per forward from a tools/prof_encoder.sh per-(kernel, grid) table: every row except the model build's
    (weight uploads = __amd_rocclr_copyBuffer, one presplit per layer, torch's fills)."""
    import re
    try:
        n = 0
        for line in open(path):
            m = re.match(r"(.*?)\s+grid\s+\d+\s+\d+\s+\d+\s+calls\s+(\d+)", line)
            if m and not any(t in m.group(1) for t in ("copyBuffer", "presplit_weight", "FillFunctor", "fillBuffer")):
                n += int(m.group(2))
        return round(n / forwards, 1) if n else None
    except OSError:
        return None


def encoder_leg(dev, cpu=True):
    """Encoder half of Graph.forward (graph_shape.py:117-150: DPT-hybrid depth + intrinsics head + seen-surface
    geometry + ResNet-50 coordinate encoder), replayed as one hipGraph, batch 1 and options/shape.yaml's 28;
    CPU leg iii: the oracle's functional restatement (oracle/encoder_ref.graph_forward, torch-CPU fp32), B = 1."""
    from zeroshape_amd import synthetic as syn
    from zeroshape_amd.utils.options import EasyDict as edict
    opt, g = _graph(dev)
    gflop = GFLOP_DPT + GFLOP_RES + GFLOP_INTR
    out = {"gflop_per_image": gflop, "peak": 2500.0, "unit": "TFLOP/s (algorithmic; split-fp16 on the 16-bit matrix pipe)"}
    from zeroshape_amd import _lib
    for B in (1, 28):
        rgb, mask = [torch.from_numpy(x).to(dev) for x in syn.seeded_rgb_scene(0, B)]
        var = edict(dict(idx=list(range(B)), rgb_input_map=rgb, mask_input_map=mask))
        g.enable_hip_graph(False)
        g.forward(opt, var, training=False, get_loss=False)              # packs the weights
        c0 = _lib.CALLS[0]
        g.forward(opt, var, training=False, get_loss=False)
        calls = _lib.CALLS[0] - c0                                       # C-ABI calls (= launches, a few calls launch two) per forward
        g.enable_hip_graph(True)
        ms, mn = _events(lambda: g.forward(opt, var, training=False, get_loss=False), 20 if B == 1 else 7)
        out["b%d" % B] = {"ms": round(ms, 3), "ms_min": round(mn, 3), "tflops": round(gflop * B / ms, 1),
                          "frac_of_peak": round(gflop * B / ms / 2500.0, 4), "abi_calls_per_forward": calls}
    g.enable_hip_graph(False)
    for B in (1, 28):                          # kernels per forward from the committed kernel trace of the same forward (eager)
        k = _profiled_kernels_per_forward(os.path.join(ROOT, "profiles", "r06_encoder_b%d_by_grid.txt" % B))
        if k is not None and "b%d" % B in out:
            out["b%d" % B]["kernels_per_forward"] = k
            out["b%d" % B]["kernels_per_forward_source"] = "profiles/r06_encoder_b%d_by_grid.txt (rocprofv3 kernel trace, 11 forwards)" % B
    if cpu:
        from oracle import encoder_ref
        sd = {k: v.detach().cpu() for k, v in g.state_dict().items()}
        rgb, mask = [torch.from_numpy(x) for x in syn.seeded_rgb_scene(0, 1)]
        ncpu = os.cpu_count() or 1
        best = None
        with torch.no_grad():
            for th in sorted(set(min(t, ncpu) for t in (16, 32, 64))):
                torch.set_num_threads(th)
                encoder_ref.graph_forward(sd, rgb, mask)
                t0 = time.perf_counter()
                encoder_ref.graph_forward(sd, rgb, mask)
                dt = time.perf_counter() - t0
                if best is None or dt < best[1]:
                    best = (th, dt)
        out["cpu_baseline"] = {"value": round(best[1] * 1e3, 1), "unit": "ms per image", "cores": best[0], "kind": "port",
                               "sample": "one 224x224 image, oracle/encoder_ref.graph_forward (torch-CPU fp32), best of 16/32/64 threads"}
    del g
    torch.cuda.empty_cache()
    return out


def encoder_att_leg(dev):
    """The transformer coordinate encoder (arch.depth.encoder = 'att': CoordEmb + CoordEncAtt, /root/reference/model/shape/
    seen_coord_enc.py:49-78,119-139; `north_star`: "window/global attention ... as CDNA4 kernels"): the encoder half of
    Graph.forward with it, B = 1 / 28 as one replayed hipGraph, and its two stages alone - the window stage (Linear(3, C),
    token gather, one ViT block over 196 B sequences of 65 tokens) and the 12 global blocks over B sequences of 197 tokens -
    each captured and replayed, with the split-fp16 matrix work they execute against the 2,500 TFLOP/s 16-bit peak."""
    from zeroshape_amd import synthetic as syn
    from zeroshape_amd.nn import blocks, ops
    from zeroshape_amd.nn.capture import CapturedCall
    from zeroshape_amd.utils.options import EasyDict as edict
    opt, g = _graph(dev, encoder="att")
    enc = g.coord_encoder
    C, heads, win = enc.cls_token.shape[-1], enc.num_heads, enc.win_size
    out = {"embed_dim": C, "heads": heads, "win_size": win, "peak": 2500.0,
           "unit": "TFLOP/s (algorithmic fp32 products; split-fp16 executes 3 MFMAs per product)"}
    for B in (1, 28):
        rgb, mask = [torch.from_numpy(x).to(dev) for x in syn.seeded_rgb_scene(0, B)]
        var = edict(dict(idx=list(range(B)), rgb_input_map=rgb, mask_input_map=mask))
        g.enable_hip_graph(True)
        ms, mn = _events(lambda: g.forward(opt, var, training=False, get_loss=False), 10 if B == 1 else 5)
        g.enable_hip_graph(False)
        # the two stages alone, on the coordinate map the forward produced
        H = W = 224 // opt.arch.depth.dsp
        coord = torch.randn(B, H, W, 3, device=dev) * 0.3
        maskb = (torch.rand(B, H, W, device=dev) > 0.3)
        pk = enc.packed(dev)
        n = (H // win) * (W // win)

        def window_stage(c, m):
            emb = ops.conv2d(ops.pad_channels(c, 4), pk["embed"])
            tok = ops.window_tokens(emb, m > 0.5, pk["invalid"], pk["wcls"], pk["wpos"], win)
            tok = blocks.run_vit_block(tok, pk["wblock"], heads)
            return tok[:, 0].reshape(B, n, C).contiguous()

        def global_stage(feat):
            if pk["zero_pos"] is None or pk["zero_pos"].shape[0] != n + 1:
                pk["zero_pos"] = torch.zeros(n + 1, C, device=dev)
            x = ops.assemble_tokens(feat, pk["cls"], pk["zero_pos"])
            st = None
            for blk in pk["blocks"]:
                x, st = blocks.run_vit_block(x, blk, heads, stats=st, want_stats=True)
            return ops.layer_norm(x, pk["nw"], pk["nb"], 1e-6)
        maskf = maskb.float()
        feat = window_stage(coord, maskf)
        cw = CapturedCall(window_stage, [coord, maskf])
        cg = CapturedCall(global_stage, [feat])
        w_ms, _ = _events(lambda: cw(coord, maskf), 10)
        g_ms, _ = _events(lambda: cg(feat), 10)
        tw, Lw = B * n, win * win + 1                       # window sequences, tokens each
        w_flop = 2.0 * tw * Lw * (4 * C * C + 2 * 2 * C * C) + 4.0 * tw * Lw * Lw * C + 2.0 * B * H * W * 4 * C
        g_flop = 12 * (2.0 * B * (n + 1) * (4 * C * C + 2 * 4 * C * C) + 4.0 * B * (n + 1) ** 2 * C)
        out["b%d" % B] = {"ms": round(ms, 3), "ms_min": round(mn, 3),
                          "window_stage": {"ms": round(w_ms, 4), "sequences": tw, "tokens": Lw, "gflop": round(w_flop / 1e9, 3),
                                           "tflops": round(w_flop / w_ms / 1e9, 2), "frac_of_peak": round(w_flop / w_ms / 1e9 / 2500.0, 5)},
                          "global_blocks": {"ms": round(g_ms, 4), "sequences": B, "tokens": n + 1, "gflop": round(g_flop / 1e9, 3),
                                            "tflops": round(g_flop / g_ms / 1e9, 2), "frac_of_peak": round(g_flop / g_ms / 1e9 / 2500.0, 5)}}
    del g
    torch.cuda.empty_cache()
    return out


def vox256_leg(dev, net):
    """BASELINE config 5 on ONE GPU (evaluate.py OmniObject3D, vox_res 256): the 257^3 grid of one image through the fused
    decoder - ms and points/s - and the eight point ranges of the 8-GPU sharding (zeroshape_amd/parallel.point_bounds) each
    timed alone on this GPU: the per-rank spread the all-gather would wait for.  (The RCCL gather itself has not run on
    hardware: DESIGN.md section 7.)"""
    from zeroshape_amd import parallel, synthetic as syn
    N = 256
    G = N + 1
    latent = torch.from_numpy(syn.seeded_latent(2, 1)).to(dev)
    axis = torch.linspace(-1.5, 1.5, G, device=dev)
    st = net.prepare(latent)
    ms, mn = _events(lambda: net.query_grid(latent, axis, apply_sigmoid=True, state=st), 3)
    per = []
    for r in range(8):
        b, e, _ = parallel.point_bounds(G ** 3, 8, r)
        t, _ = _events(lambda: net.query_grid_range(latent, axis, b, e, state=st), 3)
        per.append(t)
    return {"points": G ** 3, "ms": round(ms, 2), "ms_min": round(mn, 2), "points_per_s": round(G ** 3 / (ms * 1e-3), 0),
            "precision": st.precision,
            "virtual_ranks_8": {"ms_per_rank": [round(t, 2) for t in per], "max_over_min": round(max(per) / min(per), 3),
                                "sum_over_whole": round(sum(per) / ms, 3)}}


def virtual_ranks_leg(dev, net, world=8, N=128, steps=6, distributed_prepare=None):
    """EXACTLY what one rank of `bench.py --gpus <world>` does in a step, timed on ONE GPU for every rank r in turn
    (the 8-GPU step had never been timed, not even virtually): a batch of `world` images, the step's
    prepare() (per-image prologues + the per-image f16x3-vs-fp32 probe checks) and ONE decoder launch over rank r's
    `parallel.point_bounds` range of EVERY image (`world` different 10 MB programs in flight, tiles image-major).  The N = 1
    step (one image, the whole grid) is timed the same way in the same process: `bound` = ms(N = 1) / max_r ms(rank r) is the
    compute-side weak-scaling bound - what `--gpus 8` could reach at best if the all_gather were free.
    distributed_prepare: None / True = bench.py's step for N > 1 (`parallel.prepare_sharded`: every rank runs every prologue,
    the per-image check of image i runs on rank i % world only; the 8-byte all_gather of the verdicts is stood in for by
    `parallel.solo_gather`); False = every rank also checks every image (round 5's step)."""
    from zeroshape_amd import parallel, synthetic as syn
    G = N + 1
    axis = torch.linspace(-1.5, 1.5, G, device=dev)
    stream = torch.cuda.current_stream(dev)
    if distributed_prepare is None:
        distributed_prepare = True

    def timed(latent, b, e, rank=None):
        """-> (ms per step: perf_counter between synchronisations, mean launch ms: HIP events around the decoder launch)"""
        W = latent.shape[0]

        def step(ev=None):
            if rank is not None and distributed_prepare:
                st = parallel.prepare_sharded(net, latent, rank=rank, world_size=W, gather=parallel.solo_gather(rank, W))
            else:
                st = net.prepare(latent)
            if ev is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
            out = net.query_grid_range(latent, axis, b, e, apply_sigmoid=True, state=st)
            if ev is not None:
                e1.record(stream)
                ev.append((e0, e1))
            return out
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        ev = []
        t0 = time.perf_counter()
        for _ in range(steps):
            step(ev)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        return ms, sum(a.elapsed_time(b_) for a, b_ in ev) / len(ev)

    one_ms, one_launch = timed(torch.from_numpy(syn.seeded_latent(0, 1)).to(dev), 0, G ** 3)
    latent = torch.from_numpy(syn.seeded_latent(0, world)).to(dev)
    rows = []
    for r in range(world):
        b, e, _ = parallel.point_bounds(G ** 3, world, r)
        ms, launch = timed(latent, b, e, rank=r)
        rows.append((ms, launch, world * (e - b)))
    worst = max(ms for ms, _, _ in rows)
    return {"world": world, "vox_res": N, "steps": steps, "distributed_prepare": bool(distributed_prepare),
            "n1_step_ms": round(one_ms, 3), "n1_launch_ms": round(one_launch, 3),
            "step_ms_per_rank": [round(ms, 3) for ms, _, _ in rows],
            "launch_ms_per_rank": [round(l, 3) for _, l, _ in rows],
            "prepare_and_check_ms_per_rank": [round(ms - l, 3) for ms, l, _ in rows],
            "points_per_rank": [p for _, _, p in rows],
            "bound": round(one_ms / worst, 4),
            "what": "one GPU plays every rank of `bench.py --gpus %d` in turn: batch %d, the step's prepare (incl. per-image checks) + one "
                    "launch over the rank's point range of every image; bound = n1_step_ms / max(step_ms_per_rank); the RCCL "
                    "all_gather of the results (8.6 MB per image) is NOT in it" % (world, world)}


def inference_leg(dev):
    """BASELINE config 2 ("shape_engine inference, synthetic 224x224 RGB + mask, vox_res=64", one image): image ->
    latent (Graph.forward as one hipGraph) -> 65^3 occupancy grid (prologue + fused decoder), and the evaluation
    setting of config 3 (vox_res 128) for comparison; milliseconds per image, HIP events."""
    from zeroshape_amd import synthetic as syn
    from zeroshape_amd.utils import eval_3D as E
    from zeroshape_amd.utils.options import EasyDict as edict
    opt, g = _graph(dev)
    g.enable_hip_graph(True)
    rgb, mask = [torch.from_numpy(x).to(dev) for x in syn.seeded_rgb_scene(0, 1)]
    var = edict(dict(idx=[0], rgb_input_map=rgb, mask_input_map=mask))
    out = {}
    for N in (64, 128):
        o = edict(dict(opt, eval=dict(vox_res=N, range=[-1.5, 1.5])))
        o.device = str(dev)

        def run():
            v = g.forward(opt, var, training=False, get_loss=False)
            v = v[0] if isinstance(v, tuple) else v
            pts = E.get_dense_3D_grid(o, v, N)
            return E.compute_level_grid(o, g.impl_network, v.latent_depth, None, pts, None)[0]
        for _ in range(3):                     # the side-stream check's scratch and the allocator's pools settle in a few calls
            run()
        ms, mn = _events(run, 10)
        out["vox%d" % N] = {"ms": round(ms, 3), "ms_min": round(mn, 3), "points": (N + 1) ** 3}
        if N == 64:         # the same without prepare()'s per-image output check (round 3's behaviour): what that guarantee costs
            g.impl_network.image_check = False
            ms, mn = _events(run, 10)
            g.impl_network.image_check = True
            out["vox64_without_image_check"] = {"ms": round(ms, 3), "ms_min": round(mn, 3)}
    g.enable_hip_graph(False)
    del g
    torch.cuda.empty_cache()
    return out


def train_leg(dev, steps=8, warmup=3):
    """Runner.train_iteration (model/shape_engine.py:248-297) on BASELINE config 4's per-GPU batch: 4 images,
    4096 SDF samples each, forward + backward + fused AdamW: fp32 with eager launches, fp32 as the captured step
    (optim.hip_graph), and optim.amp (split-fp16 forward / data-gradient GEMMs under the loss scaler) captured."""
    from zeroshape_amd.data.synthetic import Dataset
    from zeroshape_amd.nn import autograd as A
    from zeroshape_amd.utils import options, util
    from zeroshape_amd.utils.options import EasyDict as edict
    from zeroshape_amd.model.shape_engine import Runner

    counts = {}

    def run(amp):
        cmd = options.parse_arguments(["--yaml=%s/options/shape.yaml" % ROOT, "--output_root=/tmp/zs_bench_train",
                                       "--batch_size=4", "--pretrain.depth=", "--arch.depth.pretrained=",
                                       "--training.n_sdf_points=4096",
                                       # random weights, no calibrated depth head: at the recipe's learning rate the
                                       # untrained head collapses within ~20 steps; the step's work
                                       # does not depend on the rate
                                       "--optim.lr=1.e-7", "--optim.lr_ft=1.e-7"] + (["--optim.amp"] if amp else []))
        opt = options.set(cmd)
        opt.world_size = 1
        opt.output_path = None                      # no checkpoints from a benchmark
        r = Runner(opt)
        r.load_train_dataset(opt, dataset=Dataset(opt, split="train", n_items=4, n_points=100, seed=0))
        r.build_networks(opt)
        r.setup_optimizer(opt)
        r.graph.train()
        var0 = util.move_to_device(edict(next(iter(r.train_loader))), opt.device)

        def step():
            r.train_iteration(opt, edict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in var0.items()}))

        def timed(n_warm):
            for _ in range(n_warm):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3
        ms_eager = None if amp else timed(warmup)
        if not amp:                                 # C-ABI calls of one eager step (each is one to a few kernel launches)
            counts["abi_calls"] = _count_abi_calls(step)
            counts["grad_bytes"] = sum(p.numel() * 4 for p in r.graph.parameters() if p.requires_grad)
        opt.optim.hip_graph = True                  # forward + loss + backward replayed as one captured hipGraph
        ms = timed(warmup + 3)                      # two more eager steps, the capture, then replays
        assert getattr(r, "_captured", None) is not None
        assert all(bool(torch.isfinite(p).all()) for p in r.graph.parameters()), "non-finite parameters after the timed steps"
        del r
        torch.cuda.empty_cache()
        return ms_eager, ms
    try:
        ms_eager, ms = run(False)
        _, ms_amp = run(True)
    finally:
        A.set_forward_precision("f32")
        A.set_backward_precision("f32")
    # what ONE rank of the data-parallel step does besides (BASELINE config 4 at 4 images per GPU): the captured step with a
    # GradReducer that really packs and issues its buckets - an RCCL group of one rank, GradReducer(always=True) - as one graph
    # per backward segment.  ms / ms_with_reducer = the compute-side weak-scaling bound of the captured step.
    with_reducer = None
    try:
        import torch.distributed as dist
        from tools import train_segments
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29543")
        dist.init_process_group("nccl", rank=0, world_size=1)
        try:
            rec = train_segments.run(True, steps)
        finally:
            dist.destroy_process_group()
        with_reducer = {"ms": rec["ms_per_step"], "graphs": rec["graphs"], "buckets": rec["buckets"],
                        "buckets_issued_after_each_replay": rec["buckets_issued_after_each_replay"],
                        "gradient_mb_per_segment": rec["gradient_mb_per_segment"],
                        "compute_side_bound": round(ms / rec["ms_per_step"], 4),
                        "what": "captured step, one hipGraph per backward segment, 1-rank RCCL reducer: packs + collective calls "
                                "without a wire; the ring all-reduce itself is unmeasured"}
    except Exception as ex:                               # never take the leg down
        with_reducer = {"error": "%s: %s" % (type(ex).__name__, ex)}
    tflop = 3 * 4 * (GFLOP_DPT + GFLOP_RES + GFLOP_INTR + 4096 * 5.0e-3) / 1e3      # forward + 2x backward
    return {"per_gpu_batch": 4, "sdf_points": 4096, "ms": round(ms, 2), "mode": "fp32, optim.hip_graph (captured step)",
            "ms_eager": round(ms_eager, 2), "ms_amp": round(ms_amp, 2), "images_per_s": round(4 / ms * 1e3, 1),
            "tflops": round(tflop / (ms * 1e-3), 1), "frac_of_f32_mfma_peak": round(tflop / (ms * 1e-3) / 157.3, 4),
            # one eager step's calls into libzeroshape_hip.so (a call is one to a few launches; a kernel trace counts
            # ~2,000 launches per step, profiles/r02_train_b4_final_*) and what a data-parallel step all-reduces
            "abi_calls_per_step": counts.get("abi_calls"), "allreduce_bytes_per_step": counts.get("grad_bytes"),
            "with_reducer_1rank": with_reducer,
            "allreduce": "fp32 gradients in 64 MB buckets under the backward pass (parallel.GradReducer); never run on > 1 GPU"}


def _count_abi_calls(fn):
    """Number of C-ABI calls fn() makes (the library handle is swapped for a counting proxy meanwhile)."""
    from zeroshape_amd import _lib
    real = _lib.load()
    n = [0]

    class Proxy(object):
        def __getattr__(self, name):
            f = getattr(real, name)
            if not callable(f):
                return f

            def call(*a):
                n[0] += 1
                return f(*a)
            return call
    _lib._lib = Proxy()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return n[0]


def trained_leg(dev, iterations=304):
    """The default decoder arithmetic on TRAINED weights: the reference's recipe trained
    for ~300 iterations on the analytic data (tests/test_gpu_trained_weights.py does the same), then the full 129^3 grid
    of a test image through the split-fp16 and the exact-fp32 kernels, and Implicit.prepare's calibration verdict."""
    from zeroshape_amd.data.synthetic import Dataset
    from zeroshape_amd.model.shape_engine import Runner
    from zeroshape_amd.utils import options, util
    from zeroshape_amd.utils.options import EasyDict as edict
    epochs = (iterations + 7) // 8
    cmd = options.parse_arguments(["--yaml=%s/options/shape.yaml" % ROOT, "--output_root=/tmp/zs_bench_trained", "--batch_size=4",
                                   "--max_epoch=%d" % epochs, "--pretrain.depth=", "--arch.depth.pretrained=",
                                   "--eval.vox_res=32", "--eval.num_points=2000", "--eval.batch_size=4",
                                   "--training.n_sdf_points=2048", "--optim.lr=3.e-4", "--optim.lr_ft=1.e-4", "--freq.eval=1000"])
    opt = options.set(cmd)
    opt.world_size = 1
    opt.output_path = None
    torch.manual_seed(0)
    r = Runner(opt)
    r.load_dataset(opt, dataset=Dataset(opt, split="train", n_items=4, n_points=4000),
                   train_dataset=Dataset(opt, split="train", n_items=32, n_points=4000))
    r.build_networks(opt)
    r.setup_optimizer(opt)
    r.graph.train()
    t0 = time.perf_counter()
    first, last = [], []
    for ep in range(epochs):
        for batch in r.train_loader:
            loss = r.train_iteration(opt, util.move_to_device(edict(batch), opt.device)).all.detach()
            (first if ep == 0 else last if ep == epochs - 1 else []).append(loss)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    r.graph.eval()
    var = util.move_to_device(edict(next(iter(r.test_loader))), opt.device)
    with torch.no_grad():
        var = r.graph.forward(opt, var, training=False, get_loss=False)
    net, latent = r.graph.impl_network, var.latent_depth[:1].detach().clone()
    axis = torch.linspace(-1.5, 1.5, 129, device=dev)
    st = net.prepare(latent)
    cal = {k: (v.detach().cpu().tolist() if hasattr(v, "detach") else v) for k, v in net.last_calibration.items()}
    exact = net.query_grid(latent, axis, apply_sigmoid=False, state=net.prepare(latent, "f32"))
    net.envelope_guard = False
    try:
        raw = net.query_grid(latent, axis, apply_sigmoid=False, state=net.prepare(latent, "f16x3", calibrate=False))
    finally:
        net.envelope_guard = True
    err = (raw - exact).abs()
    flips = (raw > 0) != (exact > 0)
    # VERDICT r04 item 2 on the only TRAINED weights there are: the last layer scaled until the logit scale is that of a
    # converged checkpoint (30 / 60 / 100) - the raw-logit error grows with the scale and leaves its rule, the occupancies
    # (what compute_level_grid returns) do not move: the grids keep the split arithmetic
    sweep = []
    w, b = net.impl_mlp.layers[8].weight, net.impl_mlp.layers[8].bias
    w0, b0, base = w.detach().clone(), b.detach().clone(), float(exact.abs().max())
    try:
        for target in (30.0, 60.0, 100.0):
            with torch.no_grad():
                w.copy_(w0 * (target / base))
                b.copy_(b0 * (target / base))
            st_s = net.prepare(latent)
            c = net.last_calibration
            st32 = net.prepare(latent, "f32")
            occ, occ32 = (net.query_grid(latent, axis, apply_sigmoid=True, state=s_) for s_ in (st_s, st32))
            lg32 = net.query_grid(latent, axis, apply_sigmoid=False, state=st32)
            fl = ((occ > 0.5) != (occ32 > 0.5)) & (lg32.abs() >= net.FLIP_BAND)
            sweep.append({"max_abs_logit": round(float(lg32.abs().max()), 2), "probe_max_abs_dlogit": c["max_abs_diff"],
                          "probe_max_abs_docc": c["max_abs_occ_diff"], "probe_flips_outside_band": c["flips_outside_band"],
                          "selected_raw_logits": c["selected"], "selected_occupancy": c["selected_occ"],
                          "grid_max_abs_docc": float((occ - occ32).abs().max()), "grid_flips_outside_band": int(fl.sum()),
                          "grid_tiles_sent_to_fp32": int(net.last_tile_flags.sum()) if net.last_tile_flags is not None and
                          st_s.precision == "f16x3" and st_s.occ_ok else None,
                          "occupancy_grids_run": "f16x3" if st_s.precision == "f16x3" and st_s.occ_ok else "f32"})
    finally:
        with torch.no_grad():
            w.copy_(w0)
            b.copy_(b0)
    return {"iterations": r.it, "train_seconds": round(train_s, 1), "logit_scale_sweep": sweep,
            "loss_first_epoch": round(float(torch.stack(first).mean()), 4), "loss_last_epoch": round(float(torch.stack(last).mean()), 4),
            "max_abs_logit": round(float(exact.abs().max()), 2), "occupied_fraction": round(float((exact > 0).float().mean()), 4),
            "f16x3_vs_f32_full_grid_max_abs": float(err.max()), "f16x3_vs_f32_full_grid_mean_abs": float(err.mean()),
            "occupancy_flips": int(flips.sum()), "points": int(raw.numel()), "contract": 1e-4,
            "calibration": cal, "selected_by_prepare": st.precision}


def in_subprocess(leg, key, timeout=600):
    """Run `python tools/bench_legs.py <leg>` and return its JSON entry: the training leg captures hipGraphs of
    ~1500 launches - a fault inside the HIP runtime there must not take bench.py's headline line down with it."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), leg], capture_output=True, text=True, timeout=timeout)
    for ln in reversed(r.stdout.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)[key]
    raise RuntimeError("leg %s: exit code %d: %s" % (leg, r.returncode, r.stderr.strip()[-300:]))


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    want = sys.argv[1:] or ["chamfer", "pose", "encoder", "train"]
    if "chamfer" in want:
        print(json.dumps({"chamfer": chamfer_leg(dev)}), flush=True)
    if "pose" in want:
        print(json.dumps({"pose_search": pose_search_leg(dev)}), flush=True)
    if "encoder" in want:
        print(json.dumps({"encoder": encoder_leg(dev)}), flush=True)
    if "surface" in want:
        print(json.dumps({"iso_surface": surface_leg(dev)}), flush=True)
    if "inference" in want:
        print(json.dumps({"inference": inference_leg(dev)}), flush=True)
    if "encoder_att" in want:
        print(json.dumps({"encoder_att": encoder_att_leg(dev)}), flush=True)
    if "train" in want:
        print(json.dumps({"train_step": train_leg(dev)}), flush=True)
    if "trained" in want:
        print(json.dumps({"trained_weights": trained_leg(dev)}), flush=True)
