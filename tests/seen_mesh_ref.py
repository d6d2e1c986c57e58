"""Test helper: the seen-surface mesh rules of include/zeroshape_hip.h (zs_seen_mesh; create_seen_surface of the
reference, utils/util_vis.py:137-170) restated with vectorised numpy in fp32, the stepped test surface whose threshold
decisions do not depend on rounding, and the margins that make it so.  Not product code."""
import numpy as np

# how the golden's files were named (tests/golden/make_seen_mesh_golden.py)
GOLDEN_SAMPLE_ID, GOLDEN_OBJ_NAME, GOLDEN_IMG = "7", "seen_surface_fixed", "7_image_input.png"
GOLDEN_CASES = ["s9x13", "s40x70", "s1x17", "s17x1", "invalid5x6", "flat12x12"]
STEPPED_CASES = ["s9x13", "s40x70", "s1x17", "s17x1"]
THRES = 0.005


def stepped_surface(H, W, seed, holes=0.15, write_holes=True):
    """z = 1 + 0.0005 * randint(0, 3) + 0.02 * (((x // 5) + (y // 4)) % 3 == 1), lateral pixel spacing 0.0025 * z, and
    ``holes`` of the pixels invalid -> (xyz fp32 [H,W,3] with -1 written into the invalid pixels when ``write_holes``,
    valid bool [H,W])."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    z = 1.0 + 0.0005 * rng.randint(0, 3, size=(H, W)) + 0.02 * (((x // 5) + (y // 4)) % 3 == 1)
    xyz = np.stack([(x - W / 2.0) * 0.0025 * z, (y - H / 2.0) * 0.0025 * z, z], -1).astype(np.float32)
    valid = rng.rand(H, W) >= holes
    if write_holes:
        xyz[~valid] = -1.0
    return xyz, valid


def _length(p, q):
    d = p - q                                                  # fp32
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def _cells(xyz, mask, thres):
    """valid [H,W] and, per cell [H-1,W-1]: corners-valid and the two edge tests of the upper and of the lower triangle."""
    xyz = np.asarray(xyz, np.float32)
    with np.errstate(invalid="ignore"):
        valid = xyz[..., 2] > 0
        if mask is not None:
            valid = valid & (np.asarray(mask, np.float32).reshape(valid.shape) > 0.5)
        thr = np.float32(thres)
        p00, p01, p10, p11 = xyz[:-1, :-1], xyz[:-1, 1:], xyz[1:, :-1], xyz[1:, 1:]
        v00, v01, v10, v11 = valid[:-1, :-1], valid[:-1, 1:], valid[1:, :-1], valid[1:, 1:]
        up = (v00 & v01 & v10, _length(p00, p01) < thr, _length(p00, p10) < thr)
        lo = (v01 & v11 & v10, _length(p01, p11) < thr, _length(p01, p10) < thr)
    return valid, up, lo


def seen_mesh(xyz, mask=None, thres=THRES):
    """One image [H,W,3] -> (verts fp32 [n,3], pixels int32 [n], faces int32 [m,3], vert_id int32 [H,W])."""
    xyz = np.asarray(xyz, np.float32)
    H, W = xyz.shape[:2]
    valid, up, lo = _cells(xyz, mask, thres)
    pixels = np.flatnonzero(valid.ravel()).astype(np.int32)
    vert_id = np.zeros(H * W, np.int32)
    vert_id[pixels] = np.arange(1, len(pixels) + 1, dtype=np.int32)
    vert_id = vert_id.reshape(H, W)
    i00, i01, i10, i11 = vert_id[:-1, :-1], vert_id[:-1, 1:], vert_id[1:, :-1], vert_id[1:, 1:]
    # per cell two candidate rows, upper then lower, cells in raster order
    rows = np.stack([np.stack([i00, i01, i10], -1), np.stack([i01, i11, i10], -1)], 2).reshape(-1, 3)
    keep = np.stack([up[0] & up[1] & up[2], lo[0] & lo[1] & lo[2]], 2).reshape(-1)
    return xyz.reshape(-1, 3)[pixels], pixels, rows[keep].astype(np.int32), vert_id


def margins(xyz, thres=THRES):
    """What the stepped construction promises, measured in float64 on the stored fp32 input: dict with
    ``edge_margin`` (smallest | |e| - thres | / thres over every edge of every cell whose endpoints are vertices),
    ``z_ok`` (every z <= -0.5 or >= 0.1), ``candidates``, ``emitted``, and the three rejection counts."""
    p = np.asarray(xyz, np.float64)
    assert np.isfinite(p).all()
    z = p[..., 2]
    valid = z > 0
    out = dict(z_ok=bool(((z <= -0.5) | (z >= 0.1)).all()), edge_margin=np.inf, candidates=0, emitted=0,
               rejected_corner=0, rejected_first=0, rejected_second=0)
    if min(p.shape[:2]) < 2:
        return out
    p00, p01, p10, p11 = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    v00, v01, v10, v11 = valid[:-1, :-1], valid[:-1, 1:], valid[1:, :-1], valid[1:, 1:]
    norm = lambda a, b: np.sqrt(((a - b) ** 2).sum(-1))       # noqa: E731
    for corners, (a1, b1, ok1), (a2, b2, ok2) in (
            (v00 & v01 & v10, (p00, p01, v00 & v01), (p00, p10, v00 & v10)),
            (v01 & v11 & v10, (p01, p11, v01 & v11), (p01, p10, v01 & v10))):
        e1, e2 = norm(a1, b1), norm(a2, b2)
        for e, ok in ((e1, ok1), (e2, ok2)):
            if ok.any():
                out["edge_margin"] = min(out["edge_margin"], float((np.abs(e[ok] - thres) / thres).min()))
        first, second = e1 < thres, e2 < thres
        out["candidates"] += corners.size
        out["emitted"] += int((corners & first & second).sum())
        out["rejected_corner"] += int((~corners).sum())
        out["rejected_first"] += int((corners & ~first).sum())
        out["rejected_second"] += int((corners & first & ~second).sum())
    return out


def assert_stepped_margins(xyz, thres=THRES):
    """The conditions the golden generator and the tests rely on, for one stepped random image."""
    m = margins(xyz, thres)
    assert m["z_ok"], m
    if m["candidates"]:
        assert m["edge_margin"] >= 0.05, m
        assert m["emitted"] >= 0.25 * m["candidates"], m
        assert m["candidates"] - m["emitted"] >= 0.25 * m["candidates"], m
        assert m["rejected_corner"] > 0 and m["rejected_first"] > 0 and m["rejected_second"] > 0, m
    return m
