"""Host side of the mesh turntable (zeroshape_amd/utils/util_vis.py): the camera path and look_at against the reference's
own (tests/golden/render_golden.npz), the pose normalisation zs_render_frames applies on the fly against a numpy restatement
of the reference's sequence, and the argument checks of the new entry points (no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest

from zeroshape_amd.utils import util_vis as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "render_golden.npz"))


@pytest.mark.parametrize("n", [180, 12])
def test_camera_path_equals_the_reference(golden, n):
    pos, rot = V.get_positions_and_rotations(n_frames=n)
    pos, rot = np.asarray(pos), np.asarray(rot)
    assert pos.dtype == np.float64 and pos.shape == (n, 3) and rot.shape == (n, 4, 4)
    assert np.abs(pos - golden["positions_%d" % n]).max() <= 1e-12
    assert np.abs(rot - golden["rotations_%d" % n]).max() <= 1e-12


def test_look_at_equals_the_reference(golden):
    for args, want in zip(golden["look_at_args"], golden["look_at"]):
        got = V.look_at(args[0], args[1], args[2])
        assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12
        R = got[:3, :3]                                  # camera-to-world: right, up, backward as columns
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


def test_camera_rows_are_position_and_upper_3x3(golden):
    rows = V.camera_rows(golden["positions_12"], golden["rotations_12"])
    assert rows.dtype == np.float32 and rows.shape == (12, 12)
    np.testing.assert_array_equal(rows[:, :3], golden["positions_12"].astype(np.float32))
    np.testing.assert_array_equal(rows[:, 3:].reshape(12, 3, 3), golden["rotations_12"][:, :3, :3].astype(np.float32))


def _rotation(angle, axis):
    """4x4 rotation about a coordinate axis, as trimesh.transformations.rotation_matrix builds it (cos / sin of the angle)."""
    c, s = np.cos(angle), np.sin(angle)
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    M = np.eye(4)
    M[a, a], M[a, b], M[b, a], M[b, b] = c, -s, s, c
    return M


def _signed_volume(tris):
    return float(np.einsum("ni,ni->", tris[:, 0], np.cross(tris[:, 1], tris[:, 2])) / 6.0)


def _reference_sequence(vertices, faces):
    """dump_meshes_viz + scale_to_unit_cube (utils/util_vis.py:112-127, 310-318) restated in numpy on an indexed mesh:
    rotate 180 degrees about z, then about y; fix_inversion (reverse every face when the volume is negative); subtract the
    bounding box's centroid; multiply by 2 / max extent, then by 0.5."""
    v = np.asarray(vertices, np.float64)
    for axis in (2, 1):
        M = _rotation(np.radians(180), axis)
        v = (np.c_[v, np.ones(len(v))] @ M.T)[:, :3]
    f = np.asarray(faces)
    if _signed_volume(v[f]) < 0:
        f = np.fliplr(f)
    lo, hi = v.min(0), v.max(0)
    v = v - (lo + hi) / 2
    v *= 2 / np.max(hi - lo)
    v *= 0.5
    return v[f]


def _apply(params, tris):
    p = params.astype(np.float64)
    out = (tris * p[0:3] - p[3:6]) * p[6]
    return out[:, [0, 2, 1]] if p[7] < 0 else out


def _stats(tris):
    flat = tris.reshape(-1, 3)
    return np.concatenate([flat.min(0), flat.max(0), [_signed_volume(tris)]])


@pytest.mark.parametrize("inverted", [True, False])
def test_pretransform_params_reproduce_the_reference_sequence(inverted):
    # an off-centre tetrahedron with extents (0.9, 2.1, 1.4); `faces` point outwards, reversed they give a negative volume
    vertices = np.array([[2.0, -1.0, 0.5], [2.9, -0.6, 0.7], [2.2, 1.1, 0.9], [2.4, -0.2, 1.9]])
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    if _signed_volume(vertices[faces]) < 0:
        faces = np.fliplr(faces)
    if inverted:
        faces = np.fliplr(faces)
    tris = vertices[faces]
    stats = _stats(tris)
    assert (stats[6] < 0) == inverted
    params = V.pretransform_params(stats)
    assert params.dtype == np.float32 and params.shape == (8,)
    np.testing.assert_array_equal(params[:3], [1, -1, -1])
    assert params[7] == (-1 if inverted else 1)
    assert abs(params[6] - 1 / 2.1) < 1e-7
    got = _apply(params, tris)
    want = _reference_sequence(vertices, faces)
    if inverted:            # a reversed face (v2, v1, v0) and an exchanged one (v0, v2, v1) are the same oriented triangle
        want = np.roll(want, 1, axis=1)
    assert np.abs(got - want).max() < 1e-6                 # the parameters are fp32
    assert _signed_volume(got) > 0
    flat = got.reshape(-1, 3)
    assert np.abs(flat.min(0) + flat.max(0)).max() < 1e-6 and abs(np.max(flat.max(0) - flat.min(0)) - 1) < 1e-6


def test_pretransform_params_refuse_a_mesh_without_extent():
    with pytest.raises(ValueError):
        V.pretransform_params(np.zeros(7))


@pytest.fixture(scope="module")
def lib():
    from zeroshape_amd import build, _lib
    build.build()
    return _lib.load()


def test_sizes_and_argument_errors_without_touching_the_gpu(lib):
    assert lib.zs_render_zbuffer_bytes(180, 200, 200) == 180 * 200 * 200 * 8
    assert lib.zs_render_zbuffer_bytes(1, 0, 5) == 0 and lib.zs_render_zbuffer_bytes(70000, 8, 8) == 0
    assert lib.zs_mesh_stats_scratch_bytes(0) == 0 and lib.zs_mesh_stats_scratch_bytes(1) == 32
    assert lib.zs_mesh_stats_scratch_bytes(257) == 64 and lib.zs_mesh_stats_scratch_bytes(10 ** 7) == 256 * 32
    xf = (ctypes.c_float * 8)(*V.IDENTITY_XFORM)
    base = (ctypes.c_float * 3)(*V.BASE_RGB)
    args = lambda n, F, H, W: (None, n, xf, None, F, H, W, float(V.YFOV), float(V.ZNEAR), base, None, None, None, None, None)  # noqa: E731
    assert lib.zs_render_frames(*args(-1, 1, 8, 8)) == 0 and b"bad size" in lib.zs_last_error()
    assert lib.zs_render_frames(*args(0, 1, 0, 8)) == 0 and b"bad size" in lib.zs_last_error()
    assert lib.zs_render_frames(*args(0, 1, 8, 8)) == 0 and b"null" in lib.zs_last_error()
    assert lib.zs_render_frames(*args(0, 0, 8, 8)) == 1                       # no frames: nothing to do
    assert lib.zs_render_frames(None, 0, xf, None, 1, 8, 8, 4.0, 0.05, base, None, None, None, None, None) == 0
    assert b"bad camera" in lib.zs_last_error()
    assert lib.zs_mesh_stats(None, -1, None, None, None) == 0 and b"negative" in lib.zs_last_error()
    assert lib.zs_mesh_stats(None, 3, None, None, None) == 0 and b"null" in lib.zs_last_error()
