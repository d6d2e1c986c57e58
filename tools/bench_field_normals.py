#!/usr/bin/env python3
"""Timing of eval_3D.field_normals (weld + zs_mesh_to_field_points + Implicit.field_gradient + zs_field_normals_finish) on the
vox-128 sphere mesh of tools/bench_mesh_weld.py (68,648 triangles, 34,326 vertices) with the seeded decoder of
options/shape.yaml's configuration and the seeded latent: HIP events, a warm-up, then the median of --reps calls (each call
welds again: the mesh's cached weld is dropped first, as for a mesh fresh from convert_to_explicit).  The sphere is only a
vertex set of the right size - the seeded field has another surface - so the line says nothing about the normals themselves
(tests/test_gpu_points_grad.py does).  Prints one JSON line (secondary to bench.py; no gate on the time).

    python tools/bench_field_normals.py [--reps 20] [--chunk 65536]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tests.test_oracle_mc import _sphere
from zeroshape_amd import synthetic as syn
from zeroshape_amd.model.shape.implicit import Implicit
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils.options import EasyDict as edict


def main():
    def arg(name, default):
        return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

    reps, chunk, vox = arg("--reps", 20), arg("--chunk", 65536), 128
    dev = torch.device("cuda:0")
    net = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                   n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS, posenc_3D=0,
                   mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    sd = syn.seeded_state_dict(seed=0, pos_embed=net.pos_embed.detach().numpy())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.to(dev).eval()
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=1)).to(dev)
    opt = edict(dict(device="cuda:0", eval=dict(vox_res=vox, range=[-1.5, 1.5])))
    vol = torch.from_numpy(_sphere(vox + 1, 1.0, c=(0, 0, 0))[0]).to(dev)
    mesh = E.convert_to_explicit(opt, [vol], isoval=0.5)[0]

    def call():
        mesh._device_weld = None
        E.field_normals(opt, net, latent, None, [mesh], chunk=chunk)

    call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        call()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    print(json.dumps({"metric": "field_normals", "vox": vox, "triangles": int(mesh.device_triangles.shape[0]),
                      "vertices": int(mesh.device_field_normals.shape[0]), "chunk": chunk, "reps": reps,
                      "fallbacks": int(mesh.field_normal_fallbacks.item()),
                      "ms_median": round(0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2]), 3), "ms_min": round(ms[0], 3),
                      "peak_memory_mib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)}))


if __name__ == "__main__":
    main()
