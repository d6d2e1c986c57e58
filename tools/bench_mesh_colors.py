#!/usr/bin/env python3
"""Timing of the vertex colours (csrc/mesh_colors.hip) on the vox-128 sphere mesh of tools/bench_mesh_weld.py (about 34k
vertices, 69k faces) with a synthetic 224 x 224 photo and mask and intrinsics of the size intr_param2mtx produces
(f = 1.3875 W, the principal point at the centre); the sphere of radius 1 sits 3.5 in front of the camera:

  mesh_vertex_colors   HIP events, median of --reps calls after a warm-up, on a mesh that already carries its weld (each call:
                       zs_mesh_colors_seen, the 4-byte read-back of the seen count, zs_mesh_colors_compact,
                       zs_chamfer_forward_ws, zs_mesh_colors_fill, and the allocation of workspace and outputs), and with the
                       weld (normals included) inside the timed region
  turntable            180 frames of 200 x 200 with the vertex colours (zs_render_frames_colored, the corner gather included)
                       next to the same frames with the one base colour (zs_render_frames), in the same process
  the host checker     eval_3D.mesh_vertex_colors_host on the welded host copy, wall time, once: the only other route there
                       is; the device results are compared with it first (equal, not close)

No time target is set; the claims are these comparisons.  Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_colors.py [--reps 20]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests.test_oracle_mc import _sphere
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import util_vis as V


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    dev = torch.device("cuda:0")

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
        return round(0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2]), 4), round(ms[0], 4)

    H = W = 224
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    image = np.stack([j / (W - 1.0), i / (H - 1.0), 0.5 + 0.5 * np.sin(i / 9.0) * np.cos(j / 7.0)]).astype(np.float32)
    mask = ((i - 111.5) ** 2 + (j - 111.5) ** 2 <= 90.0 ** 2).astype(np.float32)
    intr = np.array([[1.3875 * W, 0, W / 2], [0, 1.3875 * H, H / 2], [0, 0, 1]], np.float32)
    mean, scale = np.array([0.0, 0.0, 3.5], np.float32), np.array([1.0], np.float32)
    depth_tol = E.COLOR_DEPTH_TOL_CELLS * 3.0 / 128
    dev_args = [torch.from_numpy(a).to(dev) for a in (image, mask, intr, mean, scale)]

    tris, _ = E.extract_surface(torch.from_numpy(_sphere(129, 1.0, c=(0, 0, 0))[0]).to(dev), 0.5, -1.5, 1.5)
    host = E.SimpleMesh(tris.cpu().numpy())
    t0 = time.perf_counter()
    want = E.mesh_vertex_colors_host(host.vertices, host.faces, host.vertex_normals, image, mask, intr, mean, scale, depth_tol)
    host_s = time.perf_counter() - t0
    mesh = E.mesh_vertex_colors(E.SimpleMesh(tris), *dev_args, depth_tol)
    assert np.array_equal(mesh.vertex_colors, want["colors"]) and np.array_equal(mesh.vertex_seen, want["seen"].astype(bool))
    assert np.array_equal(mesh.device_color_source.cpu().numpy(), want["source"])

    def with_weld():
        E.mesh_vertex_colors(E.SimpleMesh(tris), *dev_args, depth_tol)

    out = {"metric": "mesh_vertex_colors", "reps": reps, "triangles": len(host.faces), "vertices": len(host.vertices),
           "image": [H, W], "supersample": 2, "seen_vertices": int(want["seen"].sum()),
           "seen_area_fraction": round(mesh.seen_area_fraction, 6), "host_checker_s": round(host_s, 3)}
    out["colors_ms"], out["colors_ms_min"] = events(lambda: E.mesh_vertex_colors(mesh, *dev_args, depth_tol))
    out["colors_with_weld_ms"], out["colors_with_weld_ms_min"] = events(with_weld)
    positions, rotations = V.get_positions_and_rotations(n_frames=180)
    out["turntable_plain_ms"], out["turntable_plain_ms_min"] = events(
        lambda: V.render_mesh_frames(tris, positions, rotations, (200, 200), pose_normalize=True))
    out["turntable_colored_ms"], out["turntable_colored_ms_min"] = events(
        lambda: V.render_mesh_frames(tris, positions, rotations, (200, 200), pose_normalize=True, corner_colors=V.corner_colors(mesh)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
