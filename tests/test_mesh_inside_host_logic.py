"""CPU: eval_3D.mesh_winding_host - the definition of mesh_winding and the checker of csrc/mesh_inside.hip - on hand-built cubes
with known crossing numbers, against the occupancy of the grid on marching-cubes meshes of closed grids (the independent
oracle: the winding number at every lattice point equals that point's occupancy), on invalid faces, points that are not
finite, empty inputs, soups against welds, flat meshes; mesh_signed_distance, mesh_volume_iou and mesh_report on host meshes;
the option and the pipelines."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import mc_ref
from tests.test_mesh_components_host_logic import host_case, volume_of
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import options
from zeroshape_amd.utils.options import EasyDict as edict

# (grid, zero-padded by one voxel): marching-cubes meshes that are closed because the grid is below the iso value on its border
CLOSED_GRIDS = [("sphere17", False), ("scene25", False), ("sphere17_clipped", True), ("noise9", True), ("three_valued", True)]


def cube(lo=-1.0, hi=1.0, reverse=False):
    """(vertices [8,3], faces [12,3]) of the cube [lo, hi]^3, outward (positive volume) unless ``reverse``; vertex 4 xi + 2 yi + zi.
    The last two faces are the top (+z)."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]        # -x +x -y +y -z +z
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    return v, (f[:, ::-1].copy() if reverse else f)


def together(*meshes):
    verts, faces, at = [], [], 0
    for v, f in meshes:
        verts.append(v)
        faces.append(f + at)
        at += len(v)
    return np.concatenate(verts), np.concatenate(faces)


def winding(points, mesh):
    up, down, counts = E.mesh_winding_host(np.asarray(points, np.float32).reshape(-1, 3), *mesh)
    assert up.dtype == np.int32 and down.dtype == np.int32 and counts.dtype == np.int32 and counts.shape == (5,)
    return list(zip(up.tolist(), down.tolist()))


@functools.lru_cache(maxsize=None)
def closed_case(name, padded):
    """(the level grid, G, the host mesh of its marching cubes, the lattice points) - computed once, changed by nobody."""
    vol = volume_of(name)
    if padded:
        vol = np.pad(vol, 1)
    G = vol.shape[0]
    soup = mc_ref.marching_cubes(vol, 0.5, np.float32(3.0 / G), np.float32(-1.5)).astype(np.float32)
    return vol, G, E.SimpleMesh(soup), E._lattice_host(G, np.float32(3.0 / G), np.float32(-1.5))


def test_the_outward_cube():
    mesh = cube()
    assert E.SimpleMesh(mesh[0][mesh[1]]).volume == 8.0
    inside = [(0, 0, 0), (0.3, 0.3, 0.3), (-1, 0, 0), (0, -1, 0)]   # the centre; on the top face's diagonal; on two side faces
    assert winding(inside, mesh) == [(1, 1)] * 4
    assert winding([(1, 0, 0), (0, 1, 0), (1, 1, 1)], mesh) == [(0, 0)] * 3       # the shift moves them out
    assert winding([(-1, -1, -1)], mesh) == [(1, 0)]
    assert winding([(0, 0, 1)], mesh) == [(0, 1)]                                  # on the top face: ambiguous
    assert winding([(0, 0, -1)], mesh) == [(1, 0)]                                 # on the bottom face: ambiguous
    assert winding([(0, 0, 5), (0, 0, -5), (3, 0, 0), (0.5, -7, 0.5)], mesh) == [(0, 0)] * 4
    rng = np.random.RandomState(0)
    q = rng.uniform(-2, 2, (500, 3)).astype(np.float32)
    want = np.all(np.abs(q) < 1, axis=1).astype(np.int32)
    up, down, _ = E.mesh_winding_host(q, *mesh)
    assert np.array_equal(up, want) and np.array_equal(down, want)


def test_reversed_nested_overlapping_and_open_cubes():
    assert winding([(0, 0, 0)], cube(reverse=True)) == [(-1, -1)]
    nested = together(cube(), cube(-0.5, 0.5, reverse=True))
    assert winding([(0, 0, 0), (0.1, -0.2, 0.3)], nested) == [(0, 0)] * 2         # in the cavity
    assert winding([(0.75, 0.1, 0.2), (0.1, 0.2, -0.8), (0.1, 0.2, 0.8)], nested) == [(1, 1)] * 3      # between the two
    two = together(cube(), cube(0.0, 2.0))
    assert winding([(0.5, 0.4, 0.3)], two) == [(2, 2)] and winding([(-0.5, 0.4, 0.3), (1.5, 1.4, 1.3)], two) == [(1, 1)] * 2
    v, f = cube()
    assert winding([(0, 0, 0)], (v, f[:10])) == [(0, 1)]                           # without its two top faces: ambiguous


@pytest.mark.parametrize("name,padded", CLOSED_GRIDS)
def test_winding_equals_occupancy_on_closed_marching_cubes_meshes(name, padded):
    vol, G, mesh, lattice = closed_case(name, padded)
    up, down, counts = E.mesh_winding_host(lattice, mesh.vertices, mesh.faces)
    assert counts[:3].tolist() == [0, 0, 0]
    keep = np.ones(G ** 3, bool) if name != "three_valued" else (vol != 0.5).reshape(-1)       # those points lie on the surface
    assert keep.sum() == G ** 3 - (254 if name == "three_valued" else 0)
    occupied = (vol >= 0.5).reshape(-1)
    assert np.array_equal((up != 0)[keep], occupied[keep]) and np.array_equal(up[keep], down[keep])
    assert occupied.any() and set(np.unique(up[keep]).tolist()) <= {0, 1}
    if name == "three_valued":
        odd = (up != down) | ((up != 0) != occupied)
        assert odd.any() and not odd[keep].any()                    # every exception is at a point whose level is the iso value
    # the same through mesh_occupancy_grid and SimpleMesh.contains
    inside, counts6 = E.mesh_occupancy_grid(mesh, G, np.float32(3.0 / G), -1.5)
    assert inside.dtype == np.int8 and inside.shape == (G, G, G) and np.array_equal(inside.reshape(-1) != 0, up != 0)
    assert counts6.shape == (6,) and counts6[5] == (up != down).sum() and np.array_equal(counts6[:5], counts)
    assert np.array_equal(mesh.contains(lattice[::7]), (up != 0)[::7])


def test_open_meshes_give_ambiguous_points_not_wrong_answers():
    _, mesh, _ = host_case("noise9")                                # not padded: open at the border of the grid, top and bottom too
    assert not mesh.is_watertight
    lattice = E._lattice_host(9, np.float32(3.0 / 9), np.float32(-1.5))
    up, down, _ = E.mesh_winding_host(lattice, mesh.vertices, mesh.faces)
    assert (up != down).any() and (up == down).any()


def test_invalid_faces_and_points_that_are_not_finite():
    v, f = cube()
    verts = np.concatenate([v, [[np.nan, 0, 0], [0, np.inf, 0], [5, 5, 5]]]).astype(np.float32)
    faces = np.concatenate([f[:4], [[0, 1, 8], [9, 2, 3], [0, 1, 11], [-1, 2, 3], [0, 1, 2 ** 31 - 1]], f[4:], [[10, 10, 10]]])
    q = np.array([(0, 0, 0), (np.nan, 0, 0), (0.2, 0.1, 0), (0, np.inf, 0), (0, 0, -np.inf), (3, 3, 3)], np.float32)
    up, down, counts = E.mesh_winding_host(q, verts, faces)
    assert up.tolist() == [1, 0, 1, 0, 0, 0] and down.tolist() == [1, 0, 1, 0, 0, 0]
    assert counts.tolist() == [5, 3, 1 | 2 | 4, 13 * 3, 0]
    assert E.mesh_winding_host(q[[0, 2]], verts, faces[:6])[2].tolist() == [2, 0, 1, 8, 0]
    assert E.mesh_winding_host(q[[0, 2]], verts, np.concatenate([f, [[0, 1, 11]]]))[2].tolist() == [1, 0, 2, 24, 0]
    assert E.mesh_winding_host(q, v, f)[2].tolist() == [0, 3, 4, 36, 0]
    done = E.mesh_winding(E.SimpleMesh(v[f]), q)
    assert isinstance(done, E.MeshWinding) and done.check() == dict(skipped_faces=0, nonfinite_queries=3, status=4, pairs=36)
    from zeroshape_amd import _lib
    with pytest.raises(_lib.ZeroShapeHipError, match="face index"):
        E.MeshWinding(up, down, counts).check()


def test_empty_mesh_and_no_points():
    v, f = cube()
    q = np.array([(0, 0, 0), (np.nan, 0, 0)], np.float32)
    for verts, faces in ((v, np.zeros((0, 3), np.int64)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))):
        up, down, counts = E.mesh_winding_host(q, verts, faces)
        assert up.tolist() == [0, 0] and down.tolist() == [0, 0] and counts.tolist() == [0, 1, 4, 0, 0]
    up, down, counts = E.mesh_winding_host(np.zeros((0, 3), np.float32), v, f)
    assert up.shape == (0,) and down.shape == (0,) and counts.tolist() == [0] * 5
    nothing = E.SimpleMesh(np.zeros((0, 3, 3), np.float32))
    assert not nothing.contains(q).any() and E.mesh_occupancy_grid(nothing, 3, 1.0, -1.0)[0].sum() == 0
    assert E.mesh_occupancy_grid(E.SimpleMesh(v[f]), 0, 1.0, 0.0)[0].shape == (0, 0, 0)


def test_soup_weld_and_duplicated_vertices_give_the_same_numbers():
    soup, mesh, _ = host_case("scene25")
    rng = np.random.RandomState(3)
    q = np.concatenate([rng.uniform(-1.6, 1.6, (300, 3)), mesh.vertices[::9], soup.mean(axis=1)[::11],
                        E._lattice_host(25, np.float32(3.0 / 25), np.float32(-1.5))[::13]]).astype(np.float32)
    want = E.mesh_winding_host(q, mesh.vertices, mesh.faces)
    assert (want[0] != 0).any() and (want[0] != want[1]).any()      # vertices and centroids lie on the surface
    as_soup = E.mesh_winding_host(q, soup.reshape(-1, 3), np.arange(3 * len(soup)).reshape(-1, 3))
    # a weld whose first hundred vertices exist twice, every second face using the copies
    verts = np.concatenate([mesh.vertices, mesh.vertices[:100]])
    faces = mesh.faces.copy()
    faces[::2] = np.where(faces[::2] < 100, faces[::2] + len(mesh.vertices), faces[::2])
    doubled = E.mesh_winding_host(q, verts, faces)
    shuffled = E.mesh_winding_host(q, mesh.vertices, mesh.faces[rng.permutation(len(mesh.faces))][:, [1, 2, 0]])
    for other in (as_soup, doubled, shuffled):
        assert np.array_equal(other[0], want[0]) and np.array_equal(other[1], want[1])


def _sheet(n=6, step=0.25):
    g = np.arange(n)
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * np.float32(step)
    quad = np.array([[i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1] for i in range(n - 1) for j in range(n - 1)])
    return grid, np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]])


def test_a_vertical_plane_has_winding_zero_everywhere():
    """All faces project to segments: no face contains any point, also for points in the plane."""
    grid, faces = _sheet()
    rng = np.random.RandomState(4)
    q = rng.uniform(-1, 2, (300, 3)).astype(np.float32)
    for axis in (0, 1):
        verts = np.insert(grid, axis, np.float32(0.5), axis=1)
        inplane = np.concatenate([q, verts, verts[faces].mean(axis=1)]).astype(np.float32)
        inplane[:100, axis] = 0.5
        up, down, _ = E.mesh_winding_host(inplane, verts, faces)
        assert not up.any() and not down.any()


def test_a_horizontal_sheet():
    grid, faces = _sheet()                                           # [0, 1.25]^2 at z = 0.5, counter-clockwise from above
    verts = np.insert(grid, 2, np.float32(0.5), axis=1)
    q = [(0.6, 0.6, 0.0), (0.6, 0.6, 1.0), (0.6, 0.6, 0.5), (0.5, 0.5, 0.0), (0.25, 0.6, 1.0), (2.0, 0.6, 0.0), (0.0, 0.0, 0.0),
         (1.25, 1.25, 0.0), (0.6, 1.25, 0.0), (0.6, 0.0, 0.0)]
    assert winding(q, (verts, faces)) == [(1, 0), (0, -1), (0, 0), (1, 0), (0, -1), (0, 0), (1, 0), (0, 0), (0, 0), (1, 0)]
    assert winding(q[:2], (verts, faces[:, ::-1])) == [(-1, 0), (0, 1)]


def test_signed_distance_on_the_cube():
    v, f = cube()
    mesh = E.SimpleMesh(v[f])
    q = np.array([(0, 0, 0), (0.5, 0, 0), (2, 0, 0), (0, 0, -3), (0.25, 0.5, 0.75), (np.nan, 0, 0), (1.5, 1.5, 1.5)], np.float32)
    signed = mesh.signed_distance_to(q)
    assert signed.dtype == np.float64 and signed[:5].tolist() == [-1.0, -0.5, 1.0, 2.0, -0.25] and np.isnan(signed[5])
    plain = E.mesh_distance(mesh, q, closest=True)
    assert np.array_equal(np.abs(signed).view(np.uint64), np.sqrt(plain.sqdist).view(np.uint64))
    signed2, closest = E.mesh_signed_distance(mesh, q, closest=True)
    assert np.array_equal(signed2.view(np.uint64), signed.view(np.uint64))
    assert np.array_equal(closest.view(np.uint64), plain.closest.view(np.uint64))
    # on a marching-cubes mesh: the magnitude is mesh_distance's, the sign the occupancy's
    vol, G, sphere, lattice = closed_case("sphere17", False)
    signed = E.mesh_signed_distance(sphere, lattice[::5])
    assert np.array_equal(signed < 0, (vol >= 0.5).reshape(-1)[::5])
    assert np.array_equal(np.abs(signed).view(np.uint64), np.sqrt(E.mesh_distance(sphere, lattice[::5]).sqdist).view(np.uint64))
    nothing = E.mesh_signed_distance(E.SimpleMesh(np.zeros((0, 3, 3), np.float32)), q)
    assert np.isnan(nothing[5]) and np.all(nothing[[0, 1, 2, 3, 4, 6]] == np.inf)


def test_volume_iou_on_host_meshes():
    big, small, far = (E.SimpleMesh(v[f]) for v, f in (cube(), cube(-0.5, 0.5), cube(2.0, 3.0)))
    # 16 points per axis at -1.875 + 0.25 i: no point on a face of either cube; 8 per axis inside the big one, 4 inside the small
    lattice = (16, 0.25, -1.875)
    same = E.mesh_volume_iou(big, E.SimpleMesh(big.triangles.copy()), *lattice)
    assert same == E.MeshVolumeIoU(512, 512, 512, 512, 1.0, 0, 0, 0.25 ** 3)
    nested = E.mesh_volume_iou(small, big, *lattice)
    assert nested == E.MeshVolumeIoU(64, 512, 64, 512, 64 / 512.0, 0, 0, 0.25 ** 3)
    assert nested.inside * nested.cell_volume == 1.0 and nested.inside_reference * nested.cell_volume == 8.0
    apart = E.mesh_volume_iou(small, far, 24, 0.25, -1.875)
    assert (apart.inside, apart.inside_reference, apart.both, apart.either, apart.iou) == (64, 64, 0, 128, 0.0)
    nothing = E.SimpleMesh(np.zeros((0, 3, 3), np.float32))
    empty = E.mesh_volume_iou(nothing, E.SimpleMesh(np.zeros((0, 3, 3), np.float32)), *lattice)
    assert empty[:4] == (0, 0, 0, 0) and np.isnan(empty.iou) and empty.ambiguous == 0
    # a lattice through the faces: the points on the top face are ambiguous and counted
    onface = E.mesh_volume_iou(big, small, 5, 0.5, -1.0)
    assert onface.ambiguous > 0 and onface.ambiguous_reference > 0
    with pytest.raises(ValueError, match="both"):
        E.mesh_volume_iou(big, edict(dict(device_triangles=torch.zeros(0))), *lattice)
    assert "LATTICE-SAMPLED" in E.mesh_volume_iou.__doc__ and "LATTICE-SAMPLED" in E.MeshVolumeIoU.__doc__
    # the processed scene: smoothing shrinks it a little
    _, scene, _ = host_case("scene25")
    record = E.mesh_volume_iou(E.smooth_mesh(scene, 5), scene, 25, np.float32(3.0 / 25), -1.5)
    assert 0.5 < record.iou < 1.0 and record.both <= min(record.inside, record.inside_reference) <= record.either
    assert record.inside_reference == (volume_of("scene25") >= 0.5).sum() and record.ambiguous_reference == 0
    light = E.smooth_mesh(scene, 5)
    light.volume_iou = record
    report = E.mesh_report(light)
    assert report["volume_iou"] == record._asdict() and "volume_iou" not in E.mesh_report(scene)
    json.dumps(report["volume_iou"])


def test_the_option_is_parsed_and_command_line_only(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["--yaml=%s/options/shape.yaml" % root, "--output_root=%s" % tmp_path]
    opt = options.set(options.parse_arguments(base + ["--eval.simplify_cells=2.0", "--eval.mesh_iou=true"]),
                      safe_check=True, need_gpu=False)
    assert opt.eval.mesh_iou is True
    G = int(opt.eval.vox_res) + 1
    lo, hi = opt.eval.range
    assert E._iou_option(opt, E._smooth_options(opt), E._simplify_options(opt)) == (G, float(np.float32((hi - lo) / G)), float(lo))
    assert E._iou_option(opt, None, E._simplify_options(opt), G=25)[0] == 25
    plain = options.set(options.parse_arguments(base), need_gpu=False)
    assert "mesh_iou" not in plain.eval and "eval.mesh_iou" in options.COMMAND_LINE_ONLY
    assert E._iou_option(plain, None, None) is None
    alone = options.set(options.parse_arguments(base + ["--eval.mesh_iou=true"]), safe_check=True, need_gpu=False)
    with pytest.raises(ValueError, match="mesh_iou needs"):
        E._iou_option(alone, E._smooth_options(alone), E._simplify_options(alone))
    off = edict(dict(eval=dict(range=[-1.5, 1.5], vox_res=25, mesh_iou=False)))
    assert E._iou_option(off, None, None) is None
    for yaml in os.listdir(os.path.join(root, "options")):
        with open(os.path.join(root, "options", yaml)) as fh:
            assert "mesh_iou" not in fh.read()


def test_the_pipelines_on_host_meshes(monkeypatch, tmp_path):
    """_surface_clouds and convert_to_explicit with marching cubes and the sampler replaced by host stand-ins (the real ones need
    a GPU): with eval.mesh_iou the delivered mesh carries the record against the mesh as it stood after the component filter,
    on the marching-cubes lattice of the level grid; without it nothing is attached and the calls are the parent's."""
    soup, mesh, _ = host_case("scene25")
    calls = []

    def extract(vol, isoval, range_min, range_max, num_points=0, seed=0):
        calls.append(("extract", num_points, seed))
        return soup, (torch.zeros(num_points, 3) if num_points else None)

    def sample(tris, num_points, seed=0):
        calls.append(("sample", num_points, seed))
        return torch.zeros(num_points, 3)

    monkeypatch.setattr(E, "extract_surface", extract)
    monkeypatch.setattr(E, "sample_surface", sample)
    vol = torch.zeros(25, 25, 25)

    def opt(**extra):
        return edict(dict(device="cpu", output_path=str(tmp_path), eval=dict(range=[-1.5, 1.5], vox_res=25, num_points=100, **extra)))

    edge = 3.0 / 25
    lattice = (25, float(np.float32(edge)), -1.5)
    grid = (2 * edge, (-1.5 - 0.5 * edge,) * 3)
    filtered = E.filter_components(mesh, 0.1, False)
    want_chain = E.mesh_volume_iou(E.simplify_mesh(E.smooth_mesh(filtered, 2), *grid), filtered, *lattice)
    want_simple = E.mesh_volume_iou(E.simplify_mesh(mesh, *grid), mesh, *lattice)
    assert 0.5 < want_simple.iou < 1.0 and want_chain.inside_reference < want_simple.inside_reference    # the floater is gone
    for run in (lambda o: E.convert_to_explicit(o, [vol], 0.5, to_pointcloud=True, seed=3), lambda o: E._surface_clouds(o, vol[None], seed=3)):
        got = run(opt(simplify_cells=2, mesh_iou=True))[0][0]
        assert got.volume_iou == want_simple and not hasattr(got, "deviation")
        assert E.mesh_report(got)["volume_iou"]["iou"] == want_simple.iou
        got = run(opt(simplify_cells=2, min_component_area=0.1, smooth_iterations=2, mesh_iou=True, mesh_deviation=True))[0][0]
        assert got.volume_iou == want_chain and got.deviation is not None
        for extra in (dict(), dict(mesh_iou=False)):
            del calls[:]
            plain = run(opt(simplify_cells=2, **extra))[0][0]
            assert calls == [("extract", 0, 0), ("sample", 100, 3)] and not hasattr(plain, "volume_iou")
            assert "volume_iou" not in E.mesh_report(plain)
        del calls[:]
        plain = run(opt())[0][0]
        assert calls == [("extract", 100, 3)] and not hasattr(plain, "volume_iou")
        for extra in (dict(), dict(min_component_area=0.1)):
            with pytest.raises(ValueError, match="mesh_iou needs"):
                run(opt(mesh_iou=True, **extra))
    # the helper's new keyword has a default: its callers of before are served
    assert not hasattr(E._cleaned_and_smoothed(mesh, None, (2, 0.5, -0.53, True)), "volume_iou")
