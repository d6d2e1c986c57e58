#!/usr/bin/env python3
"""Timing of the mesh weld (csrc/mesh_weld.hip) on the marching-cubes meshes of a sphere at vox 128 and vox 256 (129^3 and
257^3 grids, radius 1 in the +-1.5 cube):

  weld_mesh with and without normals   HIP events, median of --reps calls after a warm-up (each call: the launches of
                                       zs_mesh_weld, the 4-byte read-back of the vertex count, zs_mesh_weld_vertices, and the
                                       allocation of scratch and outputs)
  the host weld                        SimpleMesh's np.unique weld of the same soup, in the same process (median of 3), and
                                       the numpy normals; the device results are compared with them bit for bit first
  convert_to_explicit + dump_meshes    wall time for one grid already on the device, split into its two calls (second of two
                                       runs): what a user who asks for a mesh file waits for

On a commit without weld_mesh (the parent of the one that added it) the device rows are left out and the rest is measured
the same way.  Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_weld.py [--reps 20]
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests.test_oracle_mc import _sphere
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.options import EasyDict as edict


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    dev = torch.device("cuda:0")
    has_weld = hasattr(E, "weld_mesh")

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
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return round(sorted(ts)[len(ts) // 2], 4)

    out = {"metric": "mesh_weld", "reps": reps, "device_weld": has_weld}
    for vox in (128, 256):
        G = vox + 1
        vol = torch.from_numpy(_sphere(G, 1.0, c=(0, 0, 0))[0]).to(dev)
        tris, _ = E.extract_surface(vol, 0.5, -1.5, 1.5)
        soup = tris.cpu().numpy()
        host = E.SimpleMesh(soup)
        row = {"triangles": len(soup), "vertices": len(host.vertices)}
        row["host_weld_s"] = wall(lambda: E.SimpleMesh(soup).vertices)
        if has_weld:
            v, f, n = E.weld_mesh(tris, normals=True)
            assert np.array_equal(v.cpu().numpy().view(np.uint32), host.vertices.view(np.uint32))
            assert np.array_equal(f.cpu().numpy(), host.faces)
            row["normals_max_abs_err"] = float(np.abs(n.cpu().numpy().astype(np.float64) - host.vertex_normals).max())
            row["host_normals_s"] = wall(lambda: E.vertex_normals_host(soup, host.faces, len(host.vertices)))
            row["weld_ms"], row["weld_ms_min"] = events(lambda: E.weld_mesh(tris))
            row["weld_normals_ms"], row["weld_normals_ms_min"] = events(lambda: E.weld_mesh(tris, normals=True))
        with tempfile.TemporaryDirectory() as d:
            opt = edict(dict(device="cuda:0", output_path=d, eval=dict(range=[-1.5, 1.5], num_points=10000)))
            for _ in range(2):                                                   # the second run is the one reported
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                meshes = E.convert_to_explicit(opt, [vol], isoval=0.5)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                V.dump_meshes(opt, ["0"], "mesh", meshes, folder="dump")
                t2 = time.perf_counter()
            row["convert_to_explicit_s"], row["dump_meshes_s"] = round(t1 - t0, 4), round(t2 - t1, 4)
            row["obj_bytes"] = os.path.getsize(os.path.join(d, "dump", "0_mesh.obj"))
            if has_weld:
                t0 = time.perf_counter()
                V.dump_meshes(opt, ["0"], "mesh_n", E.convert_to_explicit(opt, [vol], isoval=0.5), folder="dump", normals=True)
                row["convert_and_dump_with_normals_s"] = round(time.perf_counter() - t0, 4)
        out["vox%d" % vox] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
