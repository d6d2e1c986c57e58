#!/usr/bin/env python3
"""Golden of the REAL reference's `Implicit` differentiated in its query points (build container only; needs /root/reference).

    python tests/golden/make_points_grad_golden.py

The reference's module is a torch module, so `torch.autograd.grad(logit.sum(), points_3D)` on it is the analytic normal field
of the predicted surface.  Three configurations (tests/points_grad_cases.py: options/shape.yaml's, posenc_3D=4, prediction head
+ semantic codes + 3 blocks), seeded weights, latents and clouds (zeroshape_amd/synthetic.py), B = 2, M = 333, on the CPU.  Per
configuration <name>:
  <name>.logit32 / .logit64     logits [2,333] of the module as it is / of module.double() on double inputs
  <name>.g_sum32 / .g_sum64     d(sum logit) / d points [2,333,3]
  <name>.g_cot32 / .g_cot64     d(sum c * logit) / d points for the seeded cotangent c of points_grad_cases.inputs
  <name>.e_ref / .e_ref_cot     max|g32 - g64| / max|g64| of the two: the reference's own fp32 error, the unit of the tests' bound
  <name>.angle_deg              the largest angle between the fp32 and fp64 unit normals -g/|g| of g_sum
Arrays only; stubs as in make_golden.py.  It also prints how many vertices of the vox-16 mesh of the yaml configuration's first
image (oracle/mc_ref.py on the reference's own 17^3 grid, vertices mapped to their field positions) the angle check's
|g64| >= 1e-3 x median rule leaves out for the reference alone."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from tests import points_grad_cases as C                   # noqa: E402


def gradients(net, lat, sem, pts, cot, dtype):
    lat_t = torch.from_numpy(lat).to(dtype)
    sem_t = torch.from_numpy(sem).to(dtype) if sem is not None else None
    p = torch.from_numpy(pts).to(dtype).requires_grad_(True)
    logit, _ = net(lat_t, sem_t, p)
    g_sum, = torch.autograd.grad(logit.sum(), p, retain_graph=True)
    g_cot, = torch.autograd.grad((logit * torch.from_numpy(cot).to(dtype)).sum(), p)
    return logit.detach().numpy(), g_sum.numpy(), g_cot.numpy()


def main():
    import copy
    import make_golden as mg
    assert os.path.isdir(mg.REF)
    mg._install_stubs()
    sys.path.insert(0, mg.REF)
    from model.shape.implicit import Implicit            # noqa: E402  (reference)
    from oracle import mc_ref
    from zeroshape_amd.utils import eval_3D as E

    torch.manual_seed(0)
    torch.set_num_threads(8)
    out, nets = {}, {}
    for name in C.CASES:
        net = Implicit(**C.CASES[name]["ctor"]).eval()
        sd = C.state_dict(name, net.state_dict()["pos_embed"].numpy().copy())
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        for p in net.parameters():
            p.requires_grad_(False)
        nets[name] = (net, copy.deepcopy(net).double())
        lat, sem, pts, cot = C.inputs(name)
        l32, s32, c32 = gradients(nets[name][0], lat, sem, pts, cot, torch.float32)
        l64, s64, c64 = gradients(nets[name][1], lat, sem, pts, cot, torch.float64)
        angle, left_out = C.normal_angles(s32, s64)
        assert left_out == 0.0
        gn = np.linalg.norm(s64.reshape(-1, 3), axis=1)
        out.update({name + ".logit32": l32, name + ".logit64": l64, name + ".g_sum32": s32, name + ".g_sum64": s64,
                    name + ".g_cot32": c32, name + ".g_cot64": c64, name + ".e_ref": np.array([C.rel_error(s32, s64)]),
                    name + ".e_ref_cot": np.array([C.rel_error(c32, c64)]), name + ".angle_deg": np.array([angle])})
        print("%-8s e_ref %.2e  e_ref_cot %.2e  largest angle %.4f deg  min|g| %.3f  median|g| %.3f  logits [%.2f, %.2f]"
              % (name, out[name + ".e_ref"][0], out[name + ".e_ref_cot"][0], angle, gn.min(), np.median(gn), l64.min(), l64.max()))

    # the vox-16 vertex set of the yaml configuration's first image: does the reference alone lose vertices to the rule?
    net32, net64 = nets["yaml"]
    lat = C.inputs("yaml")[0][:1]
    G, lo, hi = 17, -1.5, 1.5
    axis = torch.linspace(lo, hi, G)
    grid = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(1, -1, 3)
    with torch.no_grad():
        occ = torch.sigmoid(net32(torch.from_numpy(lat), None, grid)[0]).reshape(G, G, G).numpy()
    tris = mc_ref.marching_cubes(occ, 0.5, np.float32((hi - lo) / G), np.float32(lo))
    verts = E.SimpleMesh(tris).vertices
    pts = E.mesh_to_field_points_host(verts, lo, G)[None]
    ones = np.ones(pts.shape[:2], np.float32)
    _, g32, _ = gradients(net32, lat, None, pts, ones, torch.float32)
    _, g64, _ = gradients(net64, lat, None, pts, ones, torch.float64)
    angle, left_out = C.normal_angles(g32, g64)
    print("vox-16 mesh of the yaml configuration: %d vertices, the reference alone leaves out %d of them (fp32 against fp64: "
          "largest angle %.4f deg)" % (len(verts), int(round(left_out * len(verts))), angle))
    assert left_out == 0.0, "the reference's own fp64 gradient nearly vanishes at a vox-16 vertex"

    path = os.path.join(HERE, "points_grad_golden.npz")
    np.savez_compressed(path, **out)
    print("points_grad_golden.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
