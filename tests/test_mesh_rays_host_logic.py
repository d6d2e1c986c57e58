"""CPU: eval_3D.mesh_rays_host - the definition of mesh_ray_cast and the checker of csrc/mesh_rays.hip - on hand-built cubes
with known hits, against two independent oracles on marching-cubes meshes of closed grids (rays along lattice lines meet the
surface between the last empty and the first occupied lattice point; a +z ray from a point inside hits a back face), on
invalid faces, invalid rays, empty inputs, soups against welds; camera_rays_host against get_pixel_grid and K^-1;
mesh_reprojection_host, mesh_report, the option and the pipelines' entry on host meshes."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import mc_ref
from tests.test_mesh_components_host_logic import host_case, volume_of
from tests.test_mesh_inside_host_logic import cube, together
from zeroshape_amd.utils import camera
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import options
from zeroshape_amd.utils.options import EasyDict as edict

# (grid, zero-padded by one voxel): below the iso value on the border, so the marching-cubes mesh is closed.  three_valued is
# left out on purpose: its values equal to the iso value put lattice points on the surface, where the brackets do not hold.
LATTICE_GRIDS = [("sphere17", False, 867, 170), ("scene25", False, 1875, 507), ("sphere17_clipped", True, 1083, 153),
                 ("noise9", True, 363, 243), ("noise15", True, 867, 675)]
WINDING_GRIDS = [("sphere17", False), ("scene25", False), ("noise9", True), ("noise15", True)]
INF = np.inf


def cast(mesh, origins, directions, **kw):
    t, face, side, bary, counts = E.mesh_rays_host(np.asarray(origins, np.float32).reshape(-1, 3),
                                                   np.asarray(directions, np.float32).reshape(-1, 3), *mesh, **kw)
    assert t.dtype == np.float64 and face.dtype == np.int32 and side.dtype == np.int8
    assert counts.dtype == np.int32 and counts.shape == (5,)
    return t, face, side, bary, counts


def first(mesh, o, d, **kw):
    t, face, side, _, _ = cast(mesh, [o], [d], **kw)
    return float(t[0]), int(face[0]), int(side[0])


@functools.lru_cache(maxsize=None)
def closed_case(name, padded):
    """(the level grid, G, the host mesh of its marching cubes, the lattice coordinates of one axis) - computed once."""
    vol = volume_of(name)
    if padded:
        vol = np.pad(vol, 1)
    G = vol.shape[0]
    soup = mc_ref.marching_cubes(vol, 0.5, np.float32(3.0 / G), np.float32(-1.5)).astype(np.float32)
    axis = E._lattice_host(G, np.float32(3.0 / G), np.float32(-1.5)).reshape(G, G, G, 3)[:, 0, 0, 0]
    return vol, G, E.SimpleMesh(soup), axis


def lattice_line_rays(vol, axis):
    """The rays from the first lattice point of every lattice line along each axis -> (origins, directions, lo, hi): the
    bracket of t for a line with an occupied point (hi = -1 for a line without one)."""
    G = vol.shape[0]
    origins, directions, lo, hi = [], [], [], []
    for a in range(3):
        lines = np.moveaxis(vol, a, 2).reshape(G * G, G) > 0.5
        others = [k for k in range(3) if k != a]
        i, j = np.divmod(np.arange(G * G), G)
        o = np.zeros((G * G, 3), np.float32)
        o[:, a], o[:, others[0]], o[:, others[1]] = axis[0], axis[i], axis[j]
        d = np.zeros((G * G, 3), np.float32)
        d[:, a] = 1.0
        star = np.where(lines.any(axis=1), lines.argmax(axis=1), 0)
        x = axis.astype(np.float64)
        origins.append(o)
        directions.append(d)
        lo.append(np.where(star > 0, x[np.maximum(star - 1, 0)] - x[0], 0.0))
        hi.append(np.where(lines.any(axis=1), x[star] - x[0], -1.0))
    return np.concatenate(origins), np.concatenate(directions), np.concatenate(lo), np.concatenate(hi)


def test_the_outward_cube_from_outside_and_from_the_centre():
    mesh = cube()
    assert E.SimpleMesh(mesh[0][mesh[1]]).volume == 8.0
    # the -x quad is the faces 0 (z >= y) and 1; its normal points to -x: a ray along +x meets it against the normal
    assert first(mesh, (-3, 0.25, 0.5), (1, 0, 0)) == (2.0, 0, 1)
    assert first(mesh, (-3, 0.5, 0.25), (1, 0, 0)) == (2.0, 1, 1)
    assert first(mesh, (-3, 0.25, 0.5), (2, 0, 0)) == (1.0, 0, 1)                  # t counts in units of |d|
    assert first(mesh, (0.1, 0.2, 0), (0, 0, 1))[::2] == (1.0, -1) and first(mesh, (0.1, 0.2, 0), (0, 0, 1))[1] in (10, 11)
    assert first(mesh, (0.1, 0.2, 0), (0, 0, -4))[::2] == (0.25, -1) and first(mesh, (0.1, 0.2, 0), (0, 0, -4))[1] in (8, 9)
    assert first(mesh, (0.5, 5, 0.25), (0, -1, 0))[::2] == (4.0, 1) and first(mesh, (0.5, 5, 0.25), (0, -1, 0))[1] in (6, 7)
    assert first(mesh, (-3, 0.25, 0.5), (-1, 0, 0)) == (INF, -1, 0) and first(mesh, (-3, 2, 0.5), (1, 0, 0)) == (INF, -1, 0)
    t, face, side, bary, counts = cast(mesh, [(-3, 0.25, 0.5), (3, 3, 3)], [(1, 0, 0), (1, 0, 0)], bary=True)
    assert counts.tolist() == [0, 0, 0, 24, 0] and np.isnan(bary[1]).all()
    v, f = mesh
    assert np.array_equal(bary[0] @ v[f[face[0]]].astype(np.float64), [-1.0, 0.25, 0.5]) and abs(bary[0].sum() - 1.0) < 1e-15
    rng = np.random.RandomState(0)
    o = rng.uniform(-3, 3, (400, 3)).astype(np.float32)
    d = rng.normal(size=(400, 3)).astype(np.float32)
    t, face, side, _, _ = cast(mesh, o, d)
    inside = np.all(np.abs(o) < 1, axis=1)
    assert (side[inside] == -1).all() and inside.any() and (side[~inside] >= 0).all() and (side == 1).any() and (side == 0).any()
    p = o.astype(np.float64) + t[:, None] * d.astype(np.float64)
    hit = face >= 0
    assert np.allclose(np.abs(p[hit]).max(axis=1), 1.0, atol=1e-12) and np.all(t[hit] >= 0)


def test_reversed_and_nested_cubes():
    assert first(cube(reverse=True), (-3, 0.25, 0.5), (1, 0, 0)) == (2.0, 0, -1)
    assert first(cube(reverse=True), (0, 0.25, 0.5), (1, 0, 0))[::2] == (1.0, 1)
    nested = together(cube(), cube(-0.5, 0.5, reverse=True))
    t, face, side = first(nested, (0, 0.1, 0.2), (1, 0, 0))          # from the cavity: the inner shell's normals point inwards
    assert (t, side) == (0.5, 1) and face >= 12
    t, face, side = first(nested, (0.75, 0.1, 0.2), (1, 0, 0))       # from between the two: the outer shell from behind
    assert (t, side) == (0.25, -1) and face < 12
    t, face, side = first(nested, (0.75, 0.1, 0.2), (-1, 0, 0))      # ... and the inner shell from behind
    assert (t, side) == (0.25, -1) and face >= 12
    assert first(nested, (-3, 0.1, 0.2), (1, 0, 0)) == (2.0, 0, 1) and first(nested, (-3, 0.2, 0.1), (1, 0, 0)) == (2.0, 1, 1)


def test_edges_corners_and_faces_in_the_plane_of_the_ray():
    mesh = cube()
    v, f = mesh

    def alone(o, d):
        return [first((v, f[k:k + 1]), o, d) for k in range(len(f))]

    rays = [((-3, 0.5, 0.5), (1, 0, 0)),          # through the diagonal that the faces 0 and 1 share
            ((-3, -1, 0.25), (1, 0, 0)),          # through the cube's edge between -x and -y, then inside the plane of -y
            ((-3, -1, -1), (1, 0, 0)),            # through a corner and along an edge
            ((-2, -2, -2), (1, 1, 1)),            # through a corner, along the diagonal
            ((-3, 0.25, 1), (1, 0, 0))]           # in the plane of the top
    for o, d in rays:
        t, face, side = first(mesh, o, d)
        each = alone(o, d)
        hits = [k for k, (tk, fk, sk) in enumerate(each) if fk == 0]
        assert hits and t == min(each[k][0] for k in hits)
        assert face == min(k for k in hits if each[k][0] == t)       # the lowest index among equal t
    assert first(mesh, *rays[0]) == (2.0, 0, 1) and first(mesh, *rays[1]) == (2.0, 0, 1) and first(mesh, *rays[2])[:2] == (2.0, 0)
    assert first(mesh, *rays[3])[0] == 1.0
    assert sum(fk == 0 for _, fk, _ in alone(*rays[0])) >= 2         # both faces at the diagonal are hit: no leak
    # a ray in the plane of a face does not hit that face: the top alone, the -y quad alone
    assert first((v, f[10:12]), (-3, 0.25, 1), (1, 0, 0)) == (INF, -1, 0)
    assert first((v, f[4:6]), (-3, -1, 0.25), (1, 0, 0)) == (INF, -1, 0)
    assert first((v, f[4:6]), (-3, -1, 0.25), (1, 0.5, 0))[0] == INF   # leaves the plane at once: the ray starts outside the quad
    assert first(mesh, (-3, 0.25, 1), (1, 0, 0)) == (2.0, 0, 1)      # the -x face's own top edge is hit


def test_both_ends_of_the_range_are_inclusive():
    mesh = cube()
    o, d = (-3, 0.25, 0.5), (1, 0, 0)
    up, down = float(np.nextafter(2.0, 3.0)), float(np.nextafter(2.0, 1.0))
    assert first(mesh, o, d, t_min=2.0) == (2.0, 0, 1) and first(mesh, o, d, t_max=2.0) == (2.0, 0, 1)
    assert first(mesh, o, d, t_min=2.0, t_max=2.0) == (2.0, 0, 1)
    assert first(mesh, o, d, t_min=up)[::2] == (4.0, -1)             # just beyond: the far side, from behind
    assert first(mesh, o, d, t_max=down) == (INF, -1, 0)
    assert first(mesh, o, d, t_min=up, t_max=down) == (INF, -1, 0) and first(mesh, o, d, t_min=np.nan) == (INF, -1, 0)
    assert first(mesh, (0, 0.25, 0.5), d, t_min=-INF)[::2] == (-1.0, 1)            # behind the origin when asked for
    assert first(mesh, (0, 0.25, 0.5), d)[::2] == (1.0, -1)


def test_duplicated_degenerate_and_invalid_faces_and_invalid_rays():
    v, f = cube()
    assert first((v, np.concatenate([f[3:], f[:3]])), (-3, 0.25, 0.5), (1, 0, 0)) == (2.0, 9, 1)
    assert first((v, np.concatenate([f[3:], f[:3], f[:1]])), (-3, 0.25, 0.5), (1, 0, 0)) == (2.0, 9, 1)      # the copy comes later
    assert first((v, np.concatenate([f[:1], f])), (-3, 0.25, 0.5), (1, 0, 0)) == (2.0, 0, 1)
    # faces without area - a point, a segment through the ray - are never hit
    flat = np.array([[0, 0, 0], [0, 3, 3], [0, 1, 1]])
    assert first((v, flat), (-3, -1, 0), (1, 0, 0)) == (INF, -1, 0) and first((v, flat), (-1, -1, -3), (0, 0, 1)) == (INF, -1, 0)
    verts = np.concatenate([v, [[np.nan, 0, 0], [0, np.inf, 0], [5, 5, 5]]]).astype(np.float32)
    faces = np.concatenate([f[:4], [[0, 1, 8], [9, 2, 3], [0, 1, 11], [-1, 2, 3], [0, 1, 2 ** 31 - 1]], f[4:], [[10, 10, 10]]])
    o = np.array([(-3, 0.25, 0.5), (np.nan, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, np.inf, 0)], np.float32)
    d = np.array([(1, 0, 0), (1, 0, 0), (0, 0, 0), (0, np.nan, 1), (0, -np.inf, 0), (1, 0, 0)], np.float32)
    t, face, side, bary, counts = cast((verts, faces), o, d, bary=True)
    assert t[0] == 2.0 and np.isnan(t[1:]).all() and face.tolist() == [0, -1, -1, -1, -1, -1] and side.tolist() == [1, 0, 0, 0, 0, 0]
    assert counts.tolist() == [5, 5, 1 | 2 | 4, 13, 0] and np.isnan(bary[1:]).all()
    assert cast((v, f), o, d)[4].tolist() == [0, 5, 4, 12, 0]
    assert first((verts, faces), (0, 5, 0), (0, -1, 0))[1] in (11, 12)              # indices count the skipped faces too
    done = E.mesh_ray_cast(E.SimpleMesh(v[f]), o, d, bary=True)
    assert isinstance(done, E.MeshRays) and done.check() == dict(skipped_faces=0, nonfinite_queries=5, status=4, pairs=12)
    assert np.array_equal(done.points()[0], [-1.0, 0.25, 0.5]) and np.isnan(done.points()[1:]).all()
    with pytest.raises(ValueError, match="bary=True"):
        E.SimpleMesh(v[f]).ray_cast(o, d).points()
    from zeroshape_amd import _lib
    with pytest.raises(_lib.ZeroShapeHipError, match="face index"):
        E.MeshRays(t, face, side, bary, counts).check()
    with pytest.raises(ValueError, match="origins and"):
        E.mesh_rays_host(o, d[:3], v, f)


def test_empty_mesh_and_no_rays():
    v, f = cube()
    o, d = np.array([(0, 0, 0), (np.nan, 0, 0)], np.float32), np.array([(0, 0, 1), (0, 0, 1)], np.float32)
    for verts, faces in ((v, np.zeros((0, 3), np.int64)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))):
        t, face, side, bary, counts = cast((verts, faces), o, d, bary=True)
        assert t[0] == INF and np.isnan(t[1]) and face.tolist() == [-1, -1] and side.tolist() == [0, 0] and np.isnan(bary).all()
        assert counts.tolist() == [0, 1, 4, 0, 0]
    t, face, side, bary, counts = cast((v, f), np.zeros((0, 3)), np.zeros((0, 3)), bary=True)
    assert t.shape == (0,) and face.shape == (0,) and side.shape == (0,) and bary.shape == (0, 3) and counts.tolist() == [0] * 5
    nothing = E.SimpleMesh(np.zeros((0, 3, 3), np.float32))
    assert nothing.ray_cast(o, d).t[0] == INF
    image = E.mesh_depth_map(nothing, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.float32(1.0), 2, 3)
    assert image.depth.shape == (2, 3) and np.all(image.depth == INF) and image.check()["hit_pixels"] == 0
    assert E.mesh_depth_map(E.SimpleMesh(v[f]), np.eye(3), np.zeros(3), 1.0, 0, 5).depth.shape == (0, 5)


def test_soup_weld_and_shuffled_faces_give_the_same_t():
    soup, mesh, _ = host_case("scene25")
    rng = np.random.RandomState(3)
    o = np.concatenate([rng.uniform(-1.6, 1.6, (150, 3)), mesh.vertices[::40]]).astype(np.float32)
    d = rng.normal(size=o.shape).astype(np.float32)
    want = E.mesh_rays_host(o, d, mesh.vertices, mesh.faces)
    assert (want[1] >= 0).any() and (want[1] < 0).any() and (want[2] == 1).any() and (want[2] == -1).any()
    as_soup = E.mesh_rays_host(o, d, soup.reshape(-1, 3), np.arange(3 * len(soup)).reshape(-1, 3))
    assert np.array_equal(as_soup[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(as_soup[1], want[1])
    # the order of the faces decides ties only: the random rays (the first 150: none starts on the surface) have none
    order = rng.permutation(len(mesh.faces))
    shuffled = E.mesh_rays_host(o[:150], d[:150], mesh.vertices, mesh.faces[order])
    assert np.array_equal(shuffled[0].view(np.uint64), want[0][:150].view(np.uint64))
    assert np.array_equal(np.where(shuffled[1] >= 0, order[np.maximum(shuffled[1], 0)], -1), want[1][:150])
    assert np.array_equal(shuffled[2], want[2][:150])


@pytest.mark.parametrize("name,padded,n_lines,n_hits", LATTICE_GRIDS)
def test_lattice_line_rays_meet_the_surface_between_two_lattice_points(name, padded, n_lines, n_hits):
    """Independent oracle 1: a ray along a lattice line of a grid that is empty on its border runs along cell edges and
    through mesh vertices; it hits iff the line has an occupied point, between the last empty point and the first occupied
    one (widened by 1e-9 cell edges for the float64 rounding).  side is not asserted: a ray through a vertex may report a
    back-facing neighbour at the same t."""
    vol, G, mesh, axis = closed_case(name, padded)
    o, d, lo, hi = lattice_line_rays(vol, axis)
    t, face, _, _, counts = E.mesh_rays_host(o, d, mesh.vertices, mesh.faces)
    expect = hi >= 0
    assert len(o) == n_lines and expect.sum() == n_hits and counts[:3].tolist() == [0, 0, 0]
    assert np.array_equal(face >= 0, expect)                         # no false hit, no miss
    slack = 1e-9 * 3.0 / G
    assert np.all(t[expect] >= lo[expect] - slack) and np.all(t[expect] <= hi[expect] + slack)


@pytest.mark.parametrize("name,padded", WINDING_GRIDS)
def test_plus_z_rays_agree_with_the_winding_numbers(name, padded):
    """Independent oracle 2: from a point inside a closed mesh the +z ray hits a back face; from a point outside it misses or
    hits a front face."""
    _, G, mesh, _ = closed_case(name, padded)
    rng = np.random.RandomState(len(name))
    q = rng.uniform(-1.6, 1.6, (3000, 3)).astype(np.float32)
    up, down, _ = E.mesh_winding_host(q, mesh.vertices, mesh.faces)
    assert np.array_equal(up, down) and (up != 0).any()             # no point is ambiguous
    d = np.zeros_like(q)
    d[:, 2] = 1.0
    t, face, side, _, _ = E.mesh_rays_host(q, d, mesh.vertices, mesh.faces)
    assert np.all(face[up != 0] >= 0) and ((up == 0) & (face >= 0)).any()
    ties = sides_agree_up_to_ties(mesh, q, d, t, face, side, np.where(up != 0, -1, 1), 1e-9 * 3.0 / G)
    assert ties < 30                                                 # (1 % of the points: a flap is a rare thing)


def sides_agree_up_to_ties(mesh, o, d, t, face, side, want, slack):
    """Every hit has the side ``want``, or - where two sheets of the surface coincide (marching cubes makes flaps without
    thickness where a level equals the iso value on a lattice plane: a front and a back face at the same place, whose t
    differ by float64 rounding alone) - the mesh without the reported face is hit within ``slack`` of the same t from the
    wanted side.  -> the number of such ties."""
    odd = np.flatnonzero((face >= 0) & (side != want))
    for i in odd:
        rest = np.delete(mesh.faces, face[i], axis=0)
        t2, face2, side2, _, _ = E.mesh_rays_host(o[i:i + 1], d[i:i + 1], mesh.vertices, rest)
        assert face2[0] >= 0 and abs(t2[0] - t[i]) <= slack and side2[0] == want[i], (i, t[i], t2[0], side[i], side2[0])
    return len(odd)


def test_camera_rays_against_the_pixel_grid_and_the_inverse():
    H, W = 5, 7
    grid = camera.get_pixel_grid(edict(dict(device="cpu")), H, W).numpy().astype(np.float64)          # rows (x, y, 1), x fastest
    f = 1.3875
    for K in (np.array([[f * W, 0, W / 2], [0, f * H, H / 2], [0, 0, 1]], np.float32),
              np.array([[9.5, 0.25, 3.0], [-0.125, 8.0, 2.5], [0.01, 0.02, 1.5]], np.float32)):
        mean, scale = np.float32([0.25, -0.5, 3.0]), np.float32(1.75)
        o, d = E.camera_rays_host(K, mean, scale, H, W)
        assert o.dtype == np.float32 and d.dtype == np.float32 and o.shape == (H * W, 3) and d.shape == (H * W, 3)
        D = grid @ np.linalg.inv(K.astype(np.float64)).T
        D = D / D[:, 2:]
        # float32 rounding of the result (2^-24 relative) and a float64 inverse (1e-12)
        assert np.allclose(d.astype(np.float64) * np.float64(scale), D, rtol=2.0 ** -23, atol=1e-12)
        assert np.array_equal(o, np.broadcast_to((-mean.astype(np.float64) / np.float64(scale)).astype(np.float32), o.shape))
        assert np.array_equal(d[:, 2], np.full(H * W, np.float32(1.0 / np.float64(scale))))
        # the camera point o + t d, scaled back, has depth t: scale (o + t d) + mean = t D
        X = (o.astype(np.float64) + 2.5 * d.astype(np.float64)) * np.float64(scale) + mean.astype(np.float64)
        assert np.allclose(X, 2.5 * D, rtol=0, atol=1e-5)
    behind = np.array([[10, 0, 3], [0, 10, 2], [0, 0, -1]], np.float32)
    assert np.isnan(E.camera_rays_host(behind, mean, scale, H, W)[1]).all()
    assert np.isnan(E.camera_rays_host(np.zeros((3, 3), np.float32), mean, scale, H, W)[1]).all()
    assert E.camera_rays_host(K, mean, scale, 0, 4)[0].shape == (0, 3)


def _cube_scene():
    """The cube [-1, 1]^3 normalised by mean (0, 0, 5) and scale 2, seen by a 16 x 16 camera with f = 8: its front face lies
    at Z = 3 and covers the pixels with |j - 8| <= 5, |i - 8| <= 5 - 121 pixels, every depth exactly 3."""
    v, f = cube()
    K = np.array([[8, 0, 8], [0, 8, 8], [0, 0, 1]], np.float32)
    mask = np.zeros((16, 16), np.float32)
    mask[3:14, 2:10] = 1.0
    depth = np.full((16, 16), 3.0, np.float32)
    depth[5, 5], depth[6, 6], depth[7, 7], depth[8, 8], depth[9, 9] = 3.5, np.nan, -1.0, 3.25, 3.125
    return E.SimpleMesh(v[f]), mask, depth, K, np.float32([0, 0, 5]), np.float32(2.0)


def test_reprojection_on_a_host_mesh():
    mesh, mask, depth, K, mean, scale = _cube_scene()
    image = E.mesh_depth_map(mesh, K, mean, scale, 16, 16)
    assert image.depth.dtype == np.float32 and image.face.dtype == np.int32 and image.side.dtype == np.int8
    covered = np.zeros((16, 16), bool)
    covered[3:14, 3:14] = True
    assert np.array_equal(image.face >= 0, covered) and np.all(image.depth[covered] == 3.0) and np.all(image.depth[~covered] == INF)
    assert np.all(image.side[covered] == 1) and image.check()["hit_pixels"] == 121 and image.check()["pairs"] == 12 * 256
    record = E.mesh_reprojection(mesh, mask, depth, K, mean, scale, depth_tol=0.1, cell_edge=0.125)
    assert isinstance(record, E.MeshReprojection)
    assert (record.mask_pixels, record.mesh_pixels, record.both, record.either) == (88, 121, 77, 132)
    assert record.silhouette_iou == 77 / 132.0 and record.depth_pixels == 75 and record.back_faces == 0
    assert (record.depth_max, record.depth_max_pixel) == (0.5, (5, 5))
    assert record.depth_mean == 0.875 / 75 and record.depth_rms == np.sqrt(0.328125 / 75)
    assert (record.depth_max_mesh, record.depth_mean_mesh, record.depth_max_cells) == (0.25, 0.875 / 75 / 2, 2.0)
    assert record.agreeing == 73 and (record.depth_tol, record.scale, record.cell_edge) == (0.1, 2.0, 0.125)
    assert record == E.mesh_reprojection_host(mesh.vertices, mesh.faces, mask, depth, K, mean, scale, 0.1, cell_edge=0.125)
    # the round trip: the mesh's own image scores itself perfectly
    own = E.mesh_reprojection(mesh, covered.astype(np.float32), np.where(covered, image.depth, 0.0), K, mean, scale, 0.0)
    assert own.silhouette_iou == 1.0 and own.depth_max == 0.0 and own.agreeing == own.mesh_pixels == own.depth_pixels == 121
    assert own.depth_max_cells is None and own.cell_edge is None
    # from inside: every hit is a back face; nothing in view: NaN and None
    inside = E.mesh_reprojection(mesh, mask, depth, K, np.float32([0, 0, 0]), scale, 0.1)
    assert inside.back_faces == inside.mesh_pixels == 256
    away = E.mesh_reprojection(mesh, mask, depth, K, np.float32([0, 0, -9]), scale, 0.1)
    assert away.mesh_pixels == 0 and away.silhouette_iou == 0.0 and np.isnan(away.depth_max) and away.depth_max_pixel is None
    nothing = E.mesh_reprojection(mesh, np.zeros_like(mask), depth, K, np.float32([0, 0, -9]), scale, 0.1)
    assert np.isnan(nothing.silhouette_iou) and nothing.depth_pixels == 0
    assert "PIXEL-SAMPLED" in E.MeshReprojection.__doc__
    mesh.reprojection = record
    report = E.mesh_report(mesh)
    assert report["reprojection"]["depth_max_pixel"] == [5, 5] and report["reprojection"]["silhouette_iou"] == 77 / 132.0
    assert "reprojection" not in E.mesh_report(E.SimpleMesh(mesh.triangles.copy()))
    json.dumps(report["reprojection"])


def test_the_option_is_parsed_and_command_line_only(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["--yaml=%s/options/shape.yaml" % root, "--output_root=%s" % tmp_path]
    opt = options.set(options.parse_arguments(base + ["--eval.mesh_reprojection=true"]), safe_check=True, need_gpu=False)
    assert opt.eval.mesh_reprojection is True and E.reprojection_option(opt) is True      # no smoothing, no simplification needed
    plain = options.set(options.parse_arguments(base), need_gpu=False)
    assert "mesh_reprojection" not in plain.eval and "eval.mesh_reprojection" in options.COMMAND_LINE_ONLY
    assert E.reprojection_option(plain) is False
    assert E.reprojection_option(edict(dict(eval=dict(mesh_reprojection=False)))) is False
    for yaml in os.listdir(os.path.join(root, "options")):
        with open(os.path.join(root, "options", yaml)) as fh:
            assert "mesh_reprojection" not in fh.read()
    for script in ("demo.py", "evaluate.py"):
        with open(os.path.join(root, script)) as fh:
            assert "--eval.mesh_reprojection=true" in fh.read()


def test_the_pipelines_entry_on_host_meshes(monkeypatch):
    """eval_3D.reprojection with camera.seen_surface replaced by a host stand-in (the real one needs a GPU): every mesh of the
    batch gets the record of its own sample, with the colour pass's depth tolerance and the marching-cubes cell edge."""
    mesh, mask, depth, K, mean, scale = _cube_scene()
    other = E.SimpleMesh(mesh.triangles * np.float32(0.5))
    means, scales = torch.tensor([[0, 0, 5], [0, 0, 4]], dtype=torch.float32), torch.tensor([2.0, 1.0])
    seen = []

    def seen_surface(opt, depth_map, intr, mask_map):
        seen.append((depth_map.shape, intr.shape, mask_map.shape))
        return None, None, None, means, scales

    monkeypatch.setattr(camera, "seen_surface", seen_surface)
    opt = edict(dict(device="cpu", eval=dict(range=[-1.5, 1.5], vox_res=24, mesh_reprojection=True)))
    var = edict(dict(mask_input_map=torch.from_numpy(np.stack([mask, mask]))[:, None],
                     depth_pred=torch.from_numpy(np.stack([depth, depth]))[:, None],
                     intr=torch.from_numpy(np.stack([K, K])), mesh_pred=[mesh, other]))
    assert E.reprojection(opt, var) is var.mesh_pred and seen == [((2, 1, 16, 16), (2, 3, 3), (2, 1, 16, 16))]
    tol = E.default_color_depth_tol(opt)
    assert mesh.reprojection == E.mesh_reprojection_host(mesh.vertices, mesh.faces, mask, depth, K, mean, scale, tol, cell_edge=0.125)
    assert other.reprojection == E.mesh_reprojection_host(other.vertices, other.faces, mask, depth, K, means[1].numpy(), 1.0, tol,
                                                          cell_edge=0.125)
    assert mesh.reprojection.mesh_pixels == 121 and mesh.depth_map.depth.shape == (16, 16)
    assert E.mesh_report(other)["reprojection"]["mesh_pixels"] == other.reprojection.mesh_pixels > 0
    # a predicted camera takes precedence, a tolerance can be given
    var.intr_pred = torch.from_numpy(np.stack([K, K])) * torch.tensor([[[2.0], [2.0], [1.0]]])
    E.reprojection(opt, var, meshes=[mesh], depth_tol=0.25)
    assert mesh.reprojection.depth_tol == 0.25 and mesh.reprojection.mesh_pixels == 100      # the columns 6 .. 15, the rows too
