#!/usr/bin/env python3
"""Timing of the vertex adjacency and the smoothing passes (csrc/mesh_smooth.hip) on the vox-128 sphere mesh of
tools/bench_mesh_weld.py and on the `noise45` soup of the tests (271,874 triangles):

  mesh_adjacency       HIP events, median of --reps calls after a warm-up, on a mesh that already carries its weld (each call:
                       the launches of zs_mesh_adjacency, the 8-byte read-back of nnz and the status word, the copy of the
                       neighbour list to its size, and the allocation of scratch and outputs)
  smooth_mesh          the same way at 10 passes (Taubin's pair, boundary pinned) on a mesh that carries its weld and its
                       adjacency: zs_mesh_smooth (10 launches), zs_mesh_gather_faces, the 4-byte read-back of the status
                       word; and at 1 pass, so that (10 passes - 1 pass) / 9 is what one more pass costs
  weld_mesh            for scale, the weld both are built on (normals included), in the same process
  the host checkers    eval_3D.mesh_adjacency_host and eval_3D.smooth_vertices_host (10 passes) on the welded host copy, wall
                       time on the same host (median of 3); the device results are compared with them first

Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_smooth.py [--reps 20]
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

    def wall(fn, n=3):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return round(sorted(ts)[len(ts) // 2], 4)

    volumes = {"sphere_vox128": _sphere(129, 1.0, c=(0, 0, 0))[0],
               "noise45": np.random.RandomState(45).uniform(0, 1, (45, 45, 45)).astype(np.float32)}
    out = {"metric": "mesh_smooth", "reps": reps, "passes": 10}
    for name, vol in volumes.items():
        tris, _ = E.extract_surface(torch.from_numpy(vol).to(dev), 0.5, -1.5, 1.5)
        host = E.SimpleMesh(tris.cpu().numpy())
        want = host.adjacency
        mesh = E.SimpleMesh(tris)
        got = mesh.adjacency
        assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.neighbors, want.neighbors)
        assert np.array_equal(got.boundary, want.boundary)
        smooth = E.smooth_mesh(mesh)
        assert np.array_equal(smooth.triangles.view(np.uint32), E.smooth_mesh(host).triangles.view(np.uint32))
        row = {"triangles": len(host.triangles), "vertices": len(host.vertices), "edges": got.n_edges,
               "max_degree": int(got.degree.max()), "boundary_vertices": int(got.boundary.sum()),
               "host_adjacency_s": wall(lambda: E.mesh_adjacency_host(host.faces, len(host.vertices))),
               "host_smooth10_s": wall(lambda: E.smooth_vertices_host(host.vertices, want.offsets, want.neighbors, want.boundary))}
        row["weld_normals_ms"], row["weld_normals_ms_min"] = events(lambda: E.weld_mesh(tris, normals=True))
        row["adjacency_ms"], row["adjacency_ms_min"] = events(lambda: E.mesh_adjacency(mesh))
        row["smooth10_ms"], row["smooth10_ms_min"] = events(lambda: E.smooth_mesh(mesh))
        row["smooth1_ms"], row["smooth1_ms_min"] = events(lambda: E.smooth_mesh(mesh, iterations=1))
        row["per_pass_us"] = round((row["smooth10_ms"] - row["smooth1_ms"]) / 9.0 * 1000.0, 2)
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
