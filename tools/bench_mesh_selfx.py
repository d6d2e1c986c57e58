#!/usr/bin/env python3
"""Timing of the face-against-face kernels (csrc/mesh_selfx.hip) on the vox-128 sphere mesh of tools/bench_mesh_weld.py and on
the `noise45` soup of the tests (271,874 triangles, open at the border of its grid), each raw and after simplify_mesh at two
marching-cubes cells (as the pipelines call it: quadric placement, the cluster planes half a cell below the range):

  mesh_self_intersections   HIP events, median of --reps calls after a warm-up, on a mesh that already carries its weld (each
                            call: the grid build, the counting kernel and the allocation of scratch and outputs; no pair list,
                            nothing is read back)
  the counts                crossing pairs, faces crossed, coincident pairs, skipped faces
  the share examined        the ordered candidate pairs the kernel read (every pair from both sides) over F (F - 1), which is
                            the same number as unordered pairs over all F (F - 1) / 2
  the host checker          eval_3D.mesh_self_intersections_host on the same box's host over --host-rows evenly strided rows
                            against all faces (wall time, one run); the figure for all rows is that time SCALED by the ratio
                            of the counts - labelled as scaled, not measured; the device's per-face counts on those rows are
                            compared with it first, integer for integer

Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_selfx.py [--reps 20] [--host-rows 2000]
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
    def arg(name, default):
        return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

    reps, host_rows = arg("--reps", 20), arg("--host-rows", 2000)
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
    out = {"metric": "mesh_self_intersections", "reps": reps, "host_rows": host_rows}
    for name, vol in volumes.items():
        tris, _ = E.extract_surface(torch.from_numpy(vol).to(dev), 0.5, -1.5, 1.5)
        edge = 3.0 / vol.shape[0]
        raw = E.SimpleMesh(tris)
        meshes = {"raw": raw, "simplified_2_cells": E.simplify_mesh(raw, 2 * edge, origin=(-1.5 - 0.5 * edge,) * 3)}
        for tag, mesh in meshes.items():
            vertices, faces = (t.cpu().numpy() for t in E._device_weld_of(mesh))
            F = int(faces.shape[0])
            done = E.mesh_self_intersections(mesh)
            words = done.check()
            rows = np.unique(np.linspace(0, F - 1, min(host_rows, F)).astype(np.int64))
            t0 = time.perf_counter()
            want, _, _ = E.mesh_self_intersections_host(vertices, faces, rows=rows)
            host_s = time.perf_counter() - t0
            assert np.array_equal(done.face_counts.cpu().numpy()[rows], want)
            ms, ms_min = events(lambda: E.mesh_self_intersections(mesh))
            out["%s_%s" % (name, tag)] = {
                "triangles": F, "vertices": int(vertices.shape[0]), "ms": ms, "ms_min": ms_min,
                "crossing_pairs": words["n_pairs"], "faces_crossed": words["n_faces_crossed"],
                "coincident_pairs": words["n_coincident"], "skipped_faces": words["skipped_faces"],
                "ordered_pairs_examined": words["examined"], "share_examined": round(words["examined"] / (float(F) * (F - 1)), 8),
                "host_s_measured": round(host_s, 3), "host_rows": int(len(rows)),
                "host_s_scaled_to_all_rows": round(host_s * F / len(rows), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
