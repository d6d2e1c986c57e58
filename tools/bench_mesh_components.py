#!/usr/bin/env python3
"""Timing of the mesh components (csrc/mesh_components.hip) on the vox-128 sphere mesh of tools/bench_mesh_weld.py (one closed
component) and on the `noise45` soup of the tests (271,874 triangles, 921 components, one of them with most of the faces):

  mesh_components      HIP events, median of --reps calls after a warm-up, on a mesh that already carries its weld (each call:
                       the launches of zs_mesh_components, the 8-byte read-back of the count and the status word,
                       zs_mesh_component_stats, and the allocation of scratch and outputs)
  filter_components    the same way, on a mesh that already carries its components (min_component_area = 0.05 and
                       drop_cavities: zs_mesh_components_select, the 4-byte read-back of the kept count, zs_mesh_filter_faces)
  weld_mesh            for scale, the weld the components are built on (normals included)
  the host checker     eval_3D.mesh_components_host on the welded host copy, wall time in the same process (median of 3): the
                       only route there was; the device results are compared with it first

Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_components.py [--reps 20]
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
    out = {"metric": "mesh_components", "reps": reps}
    for name, vol in volumes.items():
        tris, _ = E.extract_surface(torch.from_numpy(vol).to(dev), 0.5, -1.5, 1.5)
        soup = tris.cpu().numpy()
        host = E.SimpleMesh(soup)
        want = E.mesh_components_host(host.vertices, host.faces, soup)
        mesh = E.SimpleMesh(tris)
        got = mesh.components
        assert np.array_equal(got.vertex_labels, want.vertex_labels) and np.array_equal(got.counts, want.counts)
        kept = E.filter_components(mesh, 0.05, True)
        assert np.array_equal(kept.triangles, E.filter_components(host, 0.05, True).triangles)
        row = {"triangles": len(soup), "vertices": len(host.vertices), "components": got.n_components,
               "kept_triangles": len(kept.triangles),
               "area_max_rel_err": float(np.max(np.abs(got.area - want.area) / want.area)),
               "host_components_s": wall(lambda: E.mesh_components_host(host.vertices, host.faces, soup)),
               "host_filter_s": wall(lambda: E.filter_components(host, 0.05, True))}
        row["weld_normals_ms"], row["weld_normals_ms_min"] = events(lambda: E.weld_mesh(tris, normals=True))
        row["components_ms"], row["components_ms_min"] = events(lambda: E.mesh_components(mesh))
        row["filter_ms"], row["filter_ms_min"] = events(lambda: E.filter_components(mesh, 0.05, True))
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
