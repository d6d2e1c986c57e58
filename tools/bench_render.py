#!/usr/bin/env python3
"""Timing of the mesh turntable (csrc/render.hip) at the size dump_meshes_viz runs it: 180 frames of 200 x 200 of the
vox-128 mesh of the synthetic checkpoint (129^3 grid -> marching cubes, about 69k triangles), pose-normalised on the fly.
HIP events around zs_render_frames (z-buffer clear + scatter + resolve) after a warm-up; prints one JSON line (secondary to
bench.py).  The scatter / resolve split comes from a kernel trace of this script:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_render.py --reps 5
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from zeroshape_amd import _lib
from zeroshape_amd import synthetic as syn
from zeroshape_amd.model.shape.implicit import Implicit
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    n_frames, H, W = 180, 200, 200
    dev = torch.device("cuda:0")
    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(0, pos_embed=pe).items()}
    net = Implicit(196, latent_dim=256, n_channels=256, n_blocks_attn=2, n_layers_mlp=8, num_heads=8,
                   skip_in=[2, 4, 6], pos_perlayer=False)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    latent = torch.from_numpy(syn.seeded_latent(0, 1)).to(dev)
    occ = net.query_grid(latent, torch.linspace(-1.5, 1.5, 129, device=dev), apply_sigmoid=True)
    tris, _ = E.extract_surface(occ[0], 0.5, -1.5, 1.5)
    lib = _lib.load()
    stats = V.mesh_stats(tris)
    xform = V.pretransform_params(stats)
    cams = torch.from_numpy(V.camera_rows(*V.get_positions_and_rotations(n_frames=n_frames))).to(dev)
    rgb = torch.empty(n_frames, H, W, 3, dtype=torch.uint8, device=dev)
    tri = torch.empty(n_frames, H, W, dtype=torch.int32, device=dev)
    zbuf = torch.empty(lib.zs_render_zbuffer_bytes(n_frames, H, W) // 8, dtype=torch.int64, device=dev)

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

    ms, ms_min = events(lambda: V.render_into(tris, xform, cams, H, W, rgb, None, None, zbuf))
    V.render_into(tris, xform, cams, H, W, rgb, None, tri, zbuf)
    covered = float((tri >= 0).float().mean())
    empty_ms, _ = events(lambda: V.render_into(tris[:0], xform, cams, H, W, rgb, None, None, zbuf))
    stats_ms, _ = events(lambda: V.mesh_stats(tris))
    print(json.dumps({"metric": "mesh_turntable_ms", "frames": n_frames, "H": H, "W": W, "triangles": int(tris.shape[0]),
                      "ms": round(ms, 3), "ms_min": round(ms_min, 3), "ms_per_frame": round(ms / n_frames, 4),
                      "covered_pixel_fraction": round(covered, 4),
                      "ms_without_triangles": round(empty_ms, 3),        # z-buffer clear + resolve of empty frames
                      "mesh_stats_ms_with_copy": round(stats_ms, 3), "signed_volume": float(stats[6]),
                      "reps": reps}))


if __name__ == "__main__":
    main()
