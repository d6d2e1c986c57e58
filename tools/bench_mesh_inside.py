#!/usr/bin/env python3
"""Timing of the point-in-mesh kernels (csrc/mesh_inside.hip) on the vox-128 sphere mesh of tools/bench_mesh_weld.py and on the
`noise45` soup of the tests (271,874 triangles, open at the border of its grid):

  mesh_winding         HIP events, median of --reps calls after a warm-up, on a mesh that already carries its weld (each call:
                       the column build, the query kernel and the allocation of scratch and outputs; nothing is read back), for
                       100,000 points near the surface - sample_surface points moved by seeded normal noise of half a
                       marching-cubes cell
  mesh_occupancy_grid  the same way, on the 129^3 lattice of the box (-1.5 + i 3 / 129): the queries are made in the kernel
  mesh_volume_iou      the same way, between the mesh simplified at 2 marching-cubes cells and the original on that lattice
                       (two grid calls, one zs_occupancy_counts call, one read-back), both carrying their welds
  the host checker     eval_3D.mesh_winding_host on the same box's host: every (point, face) box in numpy, so only
                       --host-queries of the points are timed (wall time, one run) and the figure for the whole set is that
                       time SCALED by the ratio of the counts - labelled as scaled; the device results on that subset are
                       compared with it first
  pair fraction        the (query, face) pairs read over queries x faces

Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_inside.py [--reps 20] [--host-queries 1000]
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

CELLS = 2.0
SAMPLES = 100000
LATTICE = 129


def main():
    def arg(name, default):
        return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

    reps, host_queries = arg("--reps", 20), arg("--host-queries", 1000)
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

    volumes = {"sphere_vox128": _sphere(129, 1.0, c=(0, 0, 0))[0],
               "noise45": np.random.RandomState(45).uniform(0, 1, (45, 45, 45)).astype(np.float32)}
    lattice = (LATTICE, float(np.float32(3.0 / LATTICE)), -1.5)
    out = {"metric": "mesh_inside", "reps": reps, "cells": CELLS, "host_queries": host_queries, "lattice": LATTICE}
    for name, vol in volumes.items():
        G = vol.shape[0]
        edge = 3.0 / G
        tris, _ = E.extract_surface(torch.from_numpy(vol).to(dev), 0.5, -1.5, 1.5)
        mesh = E.SimpleMesh(tris)
        light = E.simplify_mesh(mesh, CELLS * edge, (-1.5 - 0.5 * edge,) * 3)
        light._device_weld = E.weld_mesh(light.device_triangles, normals=True)
        vertices, faces = (t.cpu().numpy() for t in mesh._device_weld[:2])
        F = int(faces.shape[0])
        row = {"triangles": F, "vertices": int(vertices.shape[0]), "simplified_triangles": int(light.device_triangles.shape[0])}
        noise = torch.randn(SAMPLES, 3, generator=torch.Generator().manual_seed(G)).to(dev) * (0.5 * edge)
        q = (E.sample_surface(tris, SAMPLES, 0) + noise).contiguous()
        done = E.mesh_winding(mesh, q)
        counts = done.check()
        pick = np.unique(np.linspace(0, SAMPLES - 1, host_queries).astype(np.int64))
        sub = q[torch.from_numpy(pick).to(dev)].cpu().numpy()
        t0 = time.perf_counter()
        want = E.mesh_winding_host(sub, vertices, faces)
        host_s = time.perf_counter() - t0
        assert np.array_equal(done.up.cpu().numpy()[pick], want[0]) and np.array_equal(done.down.cpu().numpy()[pick], want[1])
        ms, ms_min = events(lambda: E.mesh_winding(mesh, q))
        row["surface_near_points"] = {
            "queries": SAMPLES, "ms": ms, "ms_min": ms_min, "pairs": counts["pairs"],
            "pair_fraction": round(counts["pairs"] / (float(SAMPLES) * F), 6),
            "inside": int((done.up != 0).sum()), "ambiguous": int((done.up != done.down).sum()),
            "host_s_measured": round(host_s, 3), "host_queries": int(len(pick)),
            "host_s_scaled_to_all_queries": round(host_s * SAMPLES / len(pick), 1)}
        inside, words = E.mesh_occupancy_grid(mesh, *lattice)
        words = E._winding_counts(words.tolist()[:5]), int(words[5])
        ms, ms_min = events(lambda: E.mesh_occupancy_grid(mesh, *lattice))
        row["occupancy_grid"] = {"queries": LATTICE ** 3, "ms": ms, "ms_min": ms_min, "pairs": words[0]["pairs"],
                                 "pair_fraction": round(words[0]["pairs"] / (float(LATTICE) ** 3 * F), 6),
                                 "inside": int((inside != 0).sum()), "ambiguous": words[1]}
        if G == LATTICE:                                             # the mesh's own lattice: is it the occupancy of its grid?
            row["occupancy_grid"]["equals_the_level_grid"] = bool(torch.equal(inside != 0, torch.from_numpy(vol >= 0.5).to(dev)))
        record = E.mesh_volume_iou(light, mesh, *lattice)
        row["volume_iou"] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in record._asdict().items()}
        row["volume_iou_ms"], row["volume_iou_ms_min"] = events(lambda: E.mesh_volume_iou(light, mesh, *lattice))
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
