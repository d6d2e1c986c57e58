#!/usr/bin/env python3
"""Timing of the exact point-to-mesh distance (csrc/mesh_distance.hip) on the vox-128 sphere mesh of tools/bench_mesh_weld.py
and on the `noise45` soup of the tests (271,874 triangles):

  mesh_distance        HIP events, median of --reps calls after a warm-up, on a mesh that already carries its weld (each call:
                       the grid build, the query kernel and the allocation of scratch and outputs; nothing is read back), for
                       two query sets - the vertices of the mesh simplified at 2 marching-cubes cells against the original
                       surface, and 100,000 sample_surface points of the original (on the surface: distance about 0)
  mesh_deviation       the same way, between the original and the simplified mesh (two mesh_distance calls, two
                       zs_mesh_distance_stats calls, one read-back), both carrying their welds
  the host checker     eval_3D.closest_point_on_mesh_host on the same box's host: a brute force, so only --host-queries of the
                       queries are timed (wall time, one run) and the figure for the whole set is that time SCALED by the ratio
                       of the counts - labelled as scaled; the device results on that subset are compared with it first
  pair fraction        the evaluated (query, face) pairs over queries x faces

Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_distance.py [--reps 20] [--host-queries 64]
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


def main():
    def arg(name, default):
        return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

    reps, host_queries = arg("--reps", 20), arg("--host-queries", 64)
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
    out = {"metric": "mesh_distance", "reps": reps, "cells": CELLS, "host_queries": host_queries}
    for name, vol in volumes.items():
        G = vol.shape[0]
        edge = 3.0 / G
        tris, _ = E.extract_surface(torch.from_numpy(vol).to(dev), 0.5, -1.5, 1.5)
        mesh = E.SimpleMesh(tris)
        light = E.simplify_mesh(mesh, CELLS * edge, (-1.5 - 0.5 * edge,) * 3)
        light._device_weld = E.weld_mesh(light.device_triangles, normals=True)
        vertices, faces = (t.cpu().numpy() for t in mesh._device_weld[:2])
        row = {"triangles": int(faces.shape[0]), "vertices": int(vertices.shape[0]), "simplified_triangles": int(light.device_triangles.shape[0])}
        sets = {"simplified_vertices": light._device_weld[0], "surface_samples": E.sample_surface(tris, SAMPLES, 0)}
        for label, q in sets.items():
            done = E.mesh_distance(mesh, q, closest=True)
            counts = done.check()
            pick = np.unique(np.linspace(0, q.shape[0] - 1, host_queries).astype(np.int64))
            sub = q[torch.from_numpy(pick).to(dev)].cpu().numpy()
            t0 = time.perf_counter()
            want = E.closest_point_on_mesh_host(sub, vertices, faces)
            host_s = time.perf_counter() - t0
            assert np.array_equal(done.sqdist.cpu().numpy()[pick].view(np.uint64), want[0].view(np.uint64))
            assert np.array_equal(done.face.cpu().numpy()[pick], want[1])
            assert np.array_equal(done.closest.cpu().numpy()[pick].view(np.uint64), want[2].view(np.uint64))
            ms, ms_min = events(lambda: E.mesh_distance(mesh, q))
            row[label] = {"queries": int(q.shape[0]), "ms": ms, "ms_min": ms_min, "pairs": counts["pairs"],
                          "pair_fraction": round(counts["pairs"] / (float(q.shape[0]) * faces.shape[0]), 6),
                          "max_distance_cells": round(float(done.sqdist.max().sqrt()) / edge, 4),
                          "host_s_measured": round(host_s, 3), "host_queries": int(len(pick)),
                          "host_s_scaled_to_all_queries": round(host_s * q.shape[0] / len(pick), 1)}
        record = E.mesh_deviation(light, mesh, cell_edge=edge)
        row["deviation"] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in record._asdict().items()}
        row["deviation"]["forward_max_cells"] = round(record.forward_max / edge, 4)
        row["deviation"]["backward_max_cells"] = round(record.backward_max / edge, 4)
        row["deviation_ms"], row["deviation_ms_min"] = events(lambda: E.mesh_deviation(light, mesh, cell_edge=edge))
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
