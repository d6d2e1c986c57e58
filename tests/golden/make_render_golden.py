#!/usr/bin/env python3
"""Golden of the REAL reference's turntable camera path (build container only; needs /root/reference).

    python tests/golden/make_render_golden.py

The reference's own `get_positions_and_rotations` (utils/util_vis.py:320-346) for n_frames = 180 and 12 - positions [F,3] and
the 4x4 matrices of its `look_at` [F,4,4], float64 - and `look_at` (utils/util_vis.py:295-308) for three hand-picked camera
positions.  Arrays only.  utils/util_vis.py imports render-only modules that are absent here (cv2, trimesh, pyrender,
imageio, torchvision, and matplotlib where it is missing): each gets an empty process-local stub; none of them is reached by
the two functions called."""
import importlib
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

LOOK_AT_CASES = np.array([
    # camera position,     target,            up
    [[1.5, 0.0, 0.0],     [0.0, 0.0, 0.0],   [0.0, 1.0, 0.0]],
    [[-0.7, 1.1, 2.3],    [0.2, -0.1, 0.4],  [0.0, 1.0, 0.0]],
    [[0.3, -2.0, -0.9],   [0.0, 0.5, 0.0],   [0.1, 0.2, 1.0]],
], np.float64)


def _install_stubs():
    for name in ["cv2", "trimesh", "pyrender", "imageio", "torchvision", "torchvision.transforms",
                 "torchvision.transforms.functional", "matplotlib", "matplotlib.pyplot"]:
        if name in sys.modules:
            continue
        try:
            importlib.import_module(name)
        except Exception:
            mod = types.ModuleType(name)
            sys.modules[name] = mod
            if "." in name:
                parent, child = name.rsplit(".", 1)
                setattr(sys.modules[parent], child, mod)


def main():
    assert os.path.isdir(REF)
    _install_stubs()
    sys.path.insert(0, REF)
    from utils import util_vis as ref_vis                 # noqa: E402  (reference)
    out = {}
    for n in (180, 12):
        pos, rot = ref_vis.get_positions_and_rotations(n_frames=n)
        out["positions_%d" % n] = np.asarray(pos, np.float64)
        out["rotations_%d" % n] = np.asarray(rot, np.float64)
        assert out["positions_%d" % n].shape == (n, 3) and out["rotations_%d" % n].shape == (n, 4, 4)
    out["look_at_args"] = LOOK_AT_CASES
    out["look_at"] = np.stack([ref_vis.look_at(c[0], c[1], c[2]) for c in LOOK_AT_CASES])
    path = os.path.join(HERE, "render_golden.npz")
    np.savez_compressed(path, **out)
    print("render_golden.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
