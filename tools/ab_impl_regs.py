#!/usr/bin/env python3
"""Two builds of the library in ONE process on ONE box: the split decoder with impl_mlp's second activation array in
registers (the tree's library) against the slab form (a side build, e.g. the parent's source or -DZS_SPLIT_IMPL_SLAB):

    python tools/build_variant_lib.py parent sdf_decoder_split.hip <parent rev>
    python tools/ab_impl_regs.py tools/_timing/parent.so [--launches 96] [--block 4] > profiles/impl_regs_ab.txt

Both libraries are loaded side by side and the binding's handle is switched between launches, block by block (blocks of
`--block` launches, event-timed on the launch stream; the order of the builds rotates from round to round), in the style of
tools/ab_ln_regs.py - on a prepared state, launch only.  Three shapes: the 129^3 grid of the benchmark, and the two
short launches that decide the inference legs: the 65^3 grid and a 4,096-point list (one tile deep).
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zeroshape_amd import _lib                                 # noqa: E402
from zeroshape_amd import synthetic as syn                     # noqa: E402
from zeroshape_amd.model.shape.implicit import Implicit        # noqa: E402
from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed   # noqa: E402

BUILDS = ("slab", "regs")


def typed(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.zs_abi_version() == _lib.ABI_VERSION
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", help="the slab-form library")
    ap.add_argument("--launches", type=int, default=96, help="per build and shape")
    ap.add_argument("--block", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    libs = {"regs": _lib.load(), "slab": typed(os.path.abspath(a.other))}

    def use(build):
        _lib._lib = libs[build]

    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(0, pos_embed=pe).items()}
    net = Implicit(syn.NUM_PATCHES, latent_dim=256, n_channels=256, n_blocks_attn=2, n_layers_mlp=8, num_heads=8,
                   skip_in=[2, 4, 6], pos_perlayer=False)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    net.image_check = False
    latent = torch.from_numpy(syn.seeded_latent(0, 1)).to(dev)
    stream = torch.cuda.current_stream(dev)
    st = net.prepare(latent)
    assert st.precision == "f16x3"
    axes = {G: torch.linspace(-1.5, 1.5, G, device=dev) for G in (129, 65)}
    pts = torch.from_numpy(syn.seeded_cloud(11, 1, 4096, -1.5, 1.5)).to(dev)
    shapes = (("grid 129^3", lambda: net.query_grid_range(latent, axes[129], 0, 129 ** 3, apply_sigmoid=True, state=st)),
              ("grid 65^3", lambda: net.query_grid_range(latent, axes[65], 0, 65 ** 3, apply_sigmoid=True, state=st)),
              ("4,096 points", lambda: net.query_points(st, pts)))
    print("# impl_mlp in registers (regs: %s) vs the slab form (slab: %s), one process, alternating blocks of %d launches, "
          "%d launches per build and shape" % (os.path.relpath(_lib.LIB_PATH, ROOT), a.other, a.block, a.launches))
    print("%-13s %-5s %9s %9s %9s %9s" % ("shape", "build", "mean ms", "median", "min", "max"))
    for name, launch in shapes:
        def one(build):
            use(build)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = launch()
            e1.record(stream)
            return e0, e1, out
        outs = {}
        for build in BUILDS:
            for _ in range(3):
                outs[build] = one(build)[2].clone()
        torch.cuda.synchronize()
        evs = []
        for blk in range(a.launches // a.block):
            for build in BUILDS[blk % 2:] + BUILDS[:blk % 2]:
                for _ in range(a.block):
                    evs.append((build,) + one(build)[:2])
        torch.cuda.synchronize()
        times = {build: [] for build in BUILDS}
        for build, e0, e1 in evs:
            times[build].append(e0.elapsed_time(e1))
        med, mean = {}, {}
        for build in BUILDS:
            t = sorted(times[build])
            med[build], mean[build] = t[len(t) // 2], sum(t) / len(t)
            print("%-13s %-5s %9.4f %9.4f %9.4f %9.4f" % (name, build, mean[build], med[build], t[0], t[-1]))
        print("# %s: regs / slab (median) %.4f  (mean) %.4f;  outputs bit-equal: %s" %
              (name, med["regs"] / med["slab"], mean["regs"] / mean["slab"], bool(torch.equal(outs["regs"], outs["slab"]))))
    use("regs")


if __name__ == "__main__":
    main()
