#!/usr/bin/env python3
"""Golden of the REAL reference's seen-surface mesh writer (build container only; needs /root/reference).

    python tests/golden/make_seen_mesh_golden.py

The reference's own `create_seen_surface` (utils/util_vis.py:137-170) on CPU tensors: for every case the input point map
`<case>_xyz` (fp32 [H,W,3]) and the bytes of the `.obj` and `.mtl` it wrote, `<case>_obj` / `<case>_mtl` (uint8).  The
inputs are the stepped surface of tests/seen_mesh_ref.py - every edge the rule tests is far from the threshold, so no
decision depends on how a length is rounded - and the conditions that construction promises are asserted here before
anything is stored (tests/test_seen_mesh_host_logic.py repeats them on the stored inputs).  utils/util_vis.py imports
render-only modules that are absent here; each gets an empty process-local stub as in make_render_golden.py."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_render_golden import REF, _install_stubs        # noqa: E402
from tests import seen_mesh_ref as R                       # noqa: E402


def cases():
    out = {}
    for name, (H, W, seed) in zip(R.STEPPED_CASES, [(9, 13, 11), (40, 70, 12), (1, 17, 13), (17, 1, 14)]):
        out[name], _ = R.stepped_surface(H, W, seed)
        R.assert_stepped_margins(out[name])
    out["invalid5x6"] = np.full((5, 6, 3), -1.0, np.float32)
    y, x = np.mgrid[0:12, 0:12]
    out["flat12x12"] = np.stack([(x - 6) * 0.0025, (y - 6) * 0.0025, np.ones((12, 12))], -1).astype(np.float32)
    m = R.margins(out["flat12x12"])
    assert m["emitted"] == m["candidates"] == 2 * 11 * 11 and m["edge_margin"] >= 0.05
    assert list(out) == R.GOLDEN_CASES
    return out


def main():
    assert os.path.isdir(REF)
    _install_stubs()
    sys.path.insert(0, REF)
    from utils import util_vis as ref_vis                 # noqa: E402  (reference)
    out = {}
    for name, xyz in cases().items():
        with tempfile.TemporaryDirectory() as d:
            ref_vis.create_seen_surface(R.GOLDEN_SAMPLE_ID, R.GOLDEN_IMG, torch.from_numpy(xyz), d, R.GOLDEN_OBJ_NAME,
                                        connect_thres=R.THRES)
            stem = os.path.join(d, "{}_{}".format(R.GOLDEN_SAMPLE_ID, R.GOLDEN_OBJ_NAME))
            out[name + "_xyz"] = xyz
            for ext in ("obj", "mtl"):
                with open(stem + "." + ext, "rb") as f:
                    out[name + "_" + ext] = np.frombuffer(f.read(), np.uint8)
    path = os.path.join(HERE, "seen_mesh_golden.npz")
    np.savez_compressed(path, **out)
    print("seen_mesh_golden.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
