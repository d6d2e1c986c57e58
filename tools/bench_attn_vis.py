#!/usr/bin/env python3
"""Timing of the attention heat-map frames (compute_level_grid(vis_attn=True)) at the size demo.py --viz runs them: vox 128
(129^3 grid, 17 x 17 = 289 drawn columns), batch 1, the synthetic checkpoint.  HIP events around Implicit.query_grid_attention
(column points + exact decoder with the raw dump + z-mean reduce, csrc/sdf_decoder.hip) and around the composer
(csrc/attn_vis.hip) after a warm-up; wall time and peak device memory of the whole call on the new path and, in the same
process, on the slice loop (an untagged copy of the grid takes it).  Prints one JSON line (secondary to bench.py).  The
decode / reduce split comes from a kernel trace of this script:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_attn_vis.py --reps 3 --no-loop
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from zeroshape_amd import synthetic as syn
from zeroshape_amd.model.shape.implicit import Implicit
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils.options import EasyDict as edict
from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    vox = int(sys.argv[sys.argv.index("--vox") + 1]) if "--vox" in sys.argv else 128
    dev = torch.device("cuda:0")
    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(0, pos_embed=pe).items()}
    net = Implicit(196, latent_dim=256, n_channels=256, n_blocks_attn=2, n_layers_mlp=8, num_heads=8,
                   skip_in=[2, 4, 6], pos_perlayer=False)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    latent = torch.from_numpy(syn.seeded_latent(0, 1)).to(dev)
    opt = edict(dict(device="cuda", H=224, W=224, eval=dict(vox_res=vox, range=[-1.5, 1.5]), arch=dict(win_size=16)))
    grid = E.get_dense_3D_grid(opt, edict(dict(idx=[0])))
    G = vox + 1
    axis = grid._zs_grid.axis
    images = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(dev)
    columns, frame_col = E.attention_frame_columns(G)
    state = net.prepare(latent)

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

    def whole(points, n):
        """(median wall ms, min wall ms, peak bytes above the start) of n calls of compute_level_grid(vis_attn=True)."""
        E.compute_level_grid(opt, net, latent, None, points, images, vis_attn=True)       # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            E.compute_level_grid(opt, net, latent, None, points, images, vis_attn=True)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        ms.sort()
        return 0.5 * (ms[(n - 1) // 2] + ms[n // 2]), ms[0], torch.cuda.max_memory_allocated() - before

    zm_ms, zm_min = events(lambda: net.query_grid_attention(latent, axis, columns, state=state))
    zmean = net.query_grid_attention(latent, axis, columns, state=state)
    fr_ms, fr_min = events(lambda: E.attention_frames(opt, zmean, frame_col, images))
    imgs, cols, chunks = net.grid_attention_chunks(1, len(columns), G)
    zt = -(-G // 32)
    decoded = len(columns) * zt * 32
    new_ms, new_min, new_peak = whole(grid, reps)
    out = {"metric": "attn_vis_ms", "vox": vox, "batch": 1, "columns": int(len(columns)), "frames": int(len(frame_col)),
           "decoded_points": decoded, "grid_points": G ** 3, "chunks": chunks, "columns_per_chunk": cols,
           "query_grid_attention_ms": round(zm_ms, 3), "query_grid_attention_ms_min": round(zm_min, 3),
           "raw_tile_bytes": decoded * 15488, "attention_frames_ms": round(fr_ms, 3),
           "attention_frames_ms_min": round(fr_min, 3), "frame_bytes": int(len(frame_col)) * 224 * 224 * 3 * 4,
           "level_grid_vis_ms": round(new_ms, 2), "level_grid_vis_ms_min": round(new_min, 2),
           "level_grid_vis_peak_bytes": int(new_peak), "reps": reps}
    if "--no-loop" not in sys.argv:
        loop_reps = max(1, min(reps, 2))                 # seconds per call
        loop_ms, loop_min, loop_peak = whole(grid.clone(), loop_reps)      # the clone drops the tag: the slice loop
        out.update({"slice_loop_ms": round(loop_ms, 2), "slice_loop_ms_min": round(loop_min, 2),
                    "slice_loop_peak_bytes": int(loop_peak), "slice_loop_reps": loop_reps,
                    "speedup": round(loop_ms / new_ms, 2), "peak_ratio": round(loop_peak / max(new_peak, 1), 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
