#!/usr/bin/env python3
"""Block 0's two arms in ONE process on ONE box: from its compact stream (default), from its q/k/v GEMMs
(ZS_SPLIT_BLOCK0_GEMM=1; also what a launch of more than 175 images runs).

The variable is read per launch, so the arms alternate block by block (blocks of `--block` launches, event-timed on the
launch stream; the order of the arms rotates from round to round), in the style of tools/ab_tile_order.py: the whole 129^3
grid through zs_sdf_query_grid_range_split on a prepared state (launch only: table / stream kernels + decode kernel + the
empty fp32 re-evaluation).

    python tools/ab_block0_tables.py [--launches 40] [--block 4] > profiles/block0_two_arms_ab.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zeroshape_amd import synthetic as syn                     # noqa: E402
from zeroshape_amd.model.shape.implicit import Implicit        # noqa: E402
from zeroshape_amd.utils.pos_embed import get_2d_sincos_pos_embed   # noqa: E402


ARMS = ("gemm", "stream")


def set_arm(arm):
    os.environ.pop("ZS_SPLIT_BLOCK0_GEMM", None)
    if arm == "gemm":
        os.environ["ZS_SPLIT_BLOCK0_GEMM"] = "1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--vox-res", type=int, default=128)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pe = get_2d_sincos_pos_embed(256, 14, cls_token=True).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(0, pos_embed=pe).items()}
    net = Implicit(syn.NUM_PATCHES, latent_dim=256, n_channels=256, n_blocks_attn=2, n_layers_mlp=8, num_heads=8,
                   skip_in=[2, 4, 6], pos_perlayer=False)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    net.image_check = False
    latent = torch.from_numpy(syn.seeded_latent(0, 1)).to(dev)
    stream = torch.cuda.current_stream(dev)
    G = a.vox_res + 1
    axis = torch.linspace(-1.5, 1.5, G, device=dev)
    st = net.prepare(latent)
    assert st.precision == "f16x3"

    def one(arm):
        set_arm(arm)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = net.query_grid_range(latent, axis, 0, G ** 3, apply_sigmoid=True, state=st)
        e1.record(stream)
        return e0, e1, out
    outs = {}
    for arm in ARMS:
        for _ in range(3):
            outs[arm] = one(arm)[2].clone()
    torch.cuda.synchronize()
    evs = []
    for blk in range(a.launches // a.block):
        for arm in ARMS[blk % 2:] + ARMS[:blk % 2]:
            for _ in range(a.block):
                evs.append((arm,) + one(arm)[:2])
    torch.cuda.synchronize()
    set_arm("stream")
    times = {arm: [] for arm in ARMS}
    for arm, e0, e1 in evs:
        times[arm].append(e0.elapsed_time(e1))
    print("# block 0: GEMMs (ZS_SPLIT_BLOCK0_GEMM=1) vs compact stream (default), one process, alternating blocks of %d "
          "launches, %d launches per arm, vox %d" % (a.block, len(times["stream"]), a.vox_res))
    print("# max |occupancy(stream) - occupancy(gemm)| over the grid: %.3g" % float((outs["stream"] - outs["gemm"]).abs().max()))
    print("%-6s %9s %9s %9s %9s" % ("arm", "mean ms", "median", "min", "max"))
    med, mean = {}, {}
    for arm in ARMS:
        t = sorted(times[arm])
        med[arm], mean[arm] = t[len(t) // 2], sum(t) / len(t)
        print("%-6s %9.3f %9.3f %9.3f %9.3f" % (arm, mean[arm], med[arm], t[0], t[-1]))
    print("# stream / gemm (median): %.4f   (mean): %.4f" % (med["stream"] / med["gemm"], mean["stream"] / mean["gemm"]))


if __name__ == "__main__":
    main()
