#!/usr/bin/env python3
"""Timing of the ray casting kernels (csrc/mesh_rays.hip) on the vox-128 sphere mesh of tools/bench_mesh_weld.py and on the
`noise45` soup of the tests (271,874 triangles, open at the border of its grid):

  mesh_depth_map       HIP events, median of --reps calls after a warm-up, on a mesh that already carries its weld (each call:
                       the grid build, the query kernel and the allocation of scratch and outputs; nothing is read back): the
                       224 x 224 depth map of a ZeroShape-like camera (f = 1.3875 W, the mesh normalised by scale 0.6 and
                       placed 2.2 in front of the camera); the rays are made in the kernel
  mesh_ray_cast        the same way, for 100,000 seeded random rays through the box: from a point of [-1.6, 1.6]^3 towards
                       another one, with the weights
  mesh_reprojection    the same way, against a mask and a depth made from the mesh's own depth map (one depth-map call, one
                       zs_occupancy_counts call, one zs_mesh_distance_stats call, one read-back)
  the host checker     eval_3D.mesh_rays_host on the same box's host: every (ray, face) pair in numpy, so only --host-rays of
                       the random rays are timed (wall time, one run) and the figure for the whole set is that time SCALED by
                       the ratio of the counts - labelled as scaled; the device results on that subset are compared with it
                       first, bit for bit
  pair fraction        the (ray, face) pairs read over rays x faces

Prints one JSON line (secondary to bench.py).

    python tools/bench_mesh_rays.py [--reps 20] [--host-rays 200]
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

RAYS = 100000
SIZE = 224


def main():
    def arg(name, default):
        return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

    reps, host_rays = arg("--reps", 20), arg("--host-rays", 200)
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
    f = 1.3875
    K = torch.tensor([[f * SIZE, 0, SIZE / 2], [0, f * SIZE, SIZE / 2], [0, 0, 1]], dtype=torch.float32, device=dev)
    mean, scale = torch.tensor([0.0, 0.0, 2.2], device=dev), torch.tensor([0.6], device=dev)
    out = {"metric": "mesh_rays", "reps": reps, "host_rays": host_rays, "image": SIZE}
    for name, vol in volumes.items():
        tris, _ = E.extract_surface(torch.from_numpy(vol).to(dev), 0.5, -1.5, 1.5)
        mesh = E.SimpleMesh(tris)
        vertices, faces = (t.cpu().numpy() for t in E._device_weld_of(mesh))
        F = int(faces.shape[0])
        row = {"triangles": F, "vertices": int(vertices.shape[0])}
        # the depth map
        image = E.mesh_depth_map(mesh, K, mean, scale, SIZE, SIZE)
        words = image.check()
        ms, ms_min = events(lambda: E.mesh_depth_map(mesh, K, mean, scale, SIZE, SIZE))
        row["depth_map"] = {"rays": SIZE * SIZE, "ms": ms, "ms_min": ms_min, "pairs": words["pairs"],
                            "pair_fraction": round(words["pairs"] / (float(SIZE * SIZE) * F), 6), "hit_pixels": words["hit_pixels"],
                            "back_faces": int((image.side == -1).sum())}
        # random rays through the box
        gen = torch.Generator().manual_seed(F)
        ends = (torch.rand(2, RAYS, 3, generator=gen) * 3.2 - 1.6).to(dev)
        o, d = ends[0].contiguous(), (ends[1] - ends[0]).contiguous()
        done = E.mesh_ray_cast(mesh, o, d, bary=True)
        counts = done.check()
        pick = np.unique(np.linspace(0, RAYS - 1, host_rays).astype(np.int64))
        sel = torch.from_numpy(pick).to(dev)
        t0 = time.perf_counter()
        want = E.mesh_rays_host(o[sel].cpu().numpy(), d[sel].cpu().numpy(), vertices, faces, bary=True)
        host_s = time.perf_counter() - t0
        assert np.array_equal(done.t[sel].cpu().numpy().view(np.uint64), want[0].view(np.uint64))
        assert np.array_equal(done.face[sel].cpu().numpy(), want[1]) and np.array_equal(done.side[sel].cpu().numpy(), want[2])
        assert np.array_equal(done.bary[sel].cpu().numpy().view(np.uint64), want[3].view(np.uint64))
        ms, ms_min = events(lambda: E.mesh_ray_cast(mesh, o, d, bary=True))
        row["random_rays"] = {
            "rays": RAYS, "ms": ms, "ms_min": ms_min, "pairs": counts["pairs"],
            "pair_fraction": round(counts["pairs"] / (float(RAYS) * F), 6), "hits": int((done.face >= 0).sum()),
            "back_faces": int((done.side == -1).sum()), "host_s_measured": round(host_s, 3), "host_rays": int(len(pick)),
            "host_s_scaled_to_all_rays": round(host_s * RAYS / len(pick), 1)}
        # the reprojection against the mesh's own image, shifted by one pixel and pushed back by 0.01
        hit = image.face >= 0
        mask = torch.roll(hit, 1, dims=1).to(torch.float32)
        depth = torch.where(hit, image.depth + 0.01, torch.full_like(image.depth, 2.0))
        record = E.mesh_reprojection(mesh, mask, depth, K, mean, scale, depth_tol=0.05, cell_edge=3.0 / vol.shape[0])
        row["reprojection"] = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in record._asdict().items()}
        row["reprojection_ms"], row["reprojection_ms_min"] = events(
            lambda: E.mesh_reprojection(mesh, mask, depth, K, mean, scale, depth_tol=0.05))
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
