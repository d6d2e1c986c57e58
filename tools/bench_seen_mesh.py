#!/usr/bin/env python3
"""Timing of the seen-surface mesh (csrc/seen_mesh.hip) at the size the depth demo and dump_results run it: 224 x 224 point
maps, batch 1 and batch 28, on the stepped test surface of tests/seen_mesh_ref.py with 15 % holes (about 42.6k vertices and
45k faces per image).  HIP events around zs_seen_mesh (count, two scan launches, vertices, faces) into preallocated buffers
after a warm-up call, and the wall time of dump_seen_surface for the batch of 28 - kernel, copy back and the 56 .obj / .mtl
files.  Prints one JSON line (secondary to bench.py).

    python tools/bench_seen_mesh.py [--reps 20]
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests.seen_mesh_ref import stepped_surface
from zeroshape_amd import _lib
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.options import EasyDict as edict


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    H = W = 224
    dev = torch.device("cuda:0")
    lib = _lib.load()
    maps = torch.from_numpy(np.stack([stepped_surface(H, W, seed)[0] for seed in range(28)])).to(dev)

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
        return 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2]), ms[0]

    out = {"metric": "seen_mesh_ms", "H": H, "W": W, "reps": reps}
    for B in (1, 28):
        xyz = maps[:B].contiguous()
        vert_id = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        vert_pixel = torch.empty(B, H * W, dtype=torch.int32, device=dev)
        verts = torch.empty(B, H * W, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(B, 2 * (H - 1) * (W - 1), 3, dtype=torch.int32, device=dev)
        counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.zs_seen_mesh_workspace_bytes(B, H, W) // 8, dtype=torch.int64, device=dev)
        stream = _lib.current_stream_ptr(dev)

        def call():
            _lib.check(lib.zs_seen_mesh(_lib.ptr(xyz), None, B, H, W, 0.005, _lib.ptr(vert_id), _lib.ptr(vert_pixel),
                                        _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(counts), _lib.ptr(ws), stream), "zs_seen_mesh")

        ms, ms_min = events(call)
        n = counts.cpu().numpy()
        out["b%d" % B] = {"ms": round(ms, 4), "ms_min": round(ms_min, 4), "vertices": int(n[:, 0].sum()),
                          "faces": int(n[:, 1].sum())}
    with tempfile.TemporaryDirectory() as d:
        opt = edict(output_path=d)
        idx = list(range(28))
        V.dump_seen_surface(opt, idx, "seen_surface_fixed", "image_input", maps, folder="dump")        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        V.dump_seen_surface(opt, idx, "seen_surface_fixed", "image_input", maps, folder="dump")
        wall = time.perf_counter() - t0
        n_bytes = sum(os.path.getsize(os.path.join(d, "dump", f)) for f in os.listdir(os.path.join(d, "dump")))
    out["dump_seen_surface_b28"] = {"wall_s": round(wall, 4), "wall_s_per_image": round(wall / 28, 4), "files": 56,
                                    "bytes_written": n_bytes}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
