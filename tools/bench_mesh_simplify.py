#!/usr/bin/env python3
"""Timing of the mesh simplification (csrc/mesh_simplify.hip) on the vox-128 sphere mesh of tools/bench_mesh_weld.py and on
the `noise45` soup of the tests (271,874 triangles), at a cluster edge of 2 marching-cubes cells on the pipelines' grid
(planes half a cell below the range):

  simplify_mesh        HIP events, median of --reps calls after a warm-up, on a mesh that already carries its weld, with the
                       quadric placement and with the mean (each call: the launches of zs_mesh_simplify, the one read-back of
                       the counts, the status word and the origin, the copy of the kept faces to their size, and the
                       allocation of scratch and outputs)
  weld_mesh            for scale, the weld it is built on (normals included), in the same process
  the host checker     eval_3D.simplify_mesh_host on the welded host copy, wall time on the same host (median of 3); the device
                       results are compared with it first
  what came out        faces, vertices and `.obj` bytes (the text util_vis.dump_meshes writes: `v` and `f` lines) before and
                       after, the volume ratio and the watertightness of the result, the counts

Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_simplify.py [--reps 20]
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


def obj_bytes(mesh):
    """The size of the text util_vis.dump_meshes writes for the mesh: a comment line, `v %.6f %.6f %.6f` per vertex, `f %d %d %d`
    per face."""
    v, f = mesh.vertices, mesh.faces + 1
    return (len("# zeroshape_amd mesh: %d vertices, %d faces\n" % (len(v), len(f))) +
            len(("v %.6f %.6f %.6f\n" * len(v)) % tuple(v.astype(np.float64).ravel().tolist())) +
            len(("f %d %d %d\n" * len(f)) % tuple(f.ravel().tolist())))


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
    out = {"metric": "mesh_simplify", "reps": reps, "cells": CELLS}
    for name, vol in volumes.items():
        G = vol.shape[0]
        edge = 3.0 / G
        cell, origin = CELLS * edge, (-1.5 - 0.5 * edge,) * 3
        tris, _ = E.extract_surface(torch.from_numpy(vol).to(dev), 0.5, -1.5, 1.5)
        host = E.SimpleMesh(tris.cpu().numpy())
        mesh = E.SimpleMesh(tris)
        row = {"triangles": len(host.triangles), "vertices": len(host.vertices), "obj_bytes": obj_bytes(host),
               "cell": round(cell, 6)}
        for position in ("quadric", "mean"):
            got = E.simplify_mesh(mesh, cell, origin, position)
            want = E.simplify_mesh(host, cell, origin, position)
            assert got.simplification == want.simplification
            assert np.array_equal(got.triangles.view(np.uint32), want.triangles.view(np.uint32))
            s = got.simplification
            row[position] = {"triangles": s.kept_faces, "vertices": len(got.vertices), "obj_bytes": obj_bytes(got),
                             "clusters": s.clusters, "degenerate": s.degenerate_faces, "duplicate": s.duplicate_faces,
                             "fallbacks": s.fallbacks, "volume_ratio": round(got.volume / host.volume, 5),
                             "is_watertight": got.is_watertight,
                             "host_s": wall(lambda: E.simplify_mesh_host(host.vertices, host.faces, origin, cell, position))}
            row[position]["ms"], row[position]["ms_min"] = events(lambda: E.simplify_mesh(mesh, cell, origin, position))
        row["weld_normals_ms"], row["weld_normals_ms_min"] = events(lambda: E.weld_mesh(tris, normals=True))
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
