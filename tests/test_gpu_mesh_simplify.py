"""GPU: the simplification kernels (csrc/mesh_simplify.hip) against their checker eval_3D.simplify_mesh_host - equal, not
close: the uint32 views of the soups and the counts - on marching-cubes soups at 2 and 3 cells with both placements, on strips
around the workgroup size and the scan tile, on a fan whose hub cluster has more incidences than a workgroup, on one cluster,
on a cluster per vertex, on hand-written soups; the raw entry point's status words and argument checks; determinism;
residency; the opt-in through convert_to_explicit and _surface_clouds."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_mesh_components_host_logic import KNOWN, volume_of
from tests.test_mesh_simplify_host_logic import check_hand_case, grid_of, hand_cases
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu

PARITY_CASES = ["sphere17", "sphere17_clipped", "scene25", "noise9", "noise23", "three_valued"]
POSITIONS = ("quadric", "mean")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(soup on the GPU, the numpy-welded host mesh of its host copy) - computed once, read by all."""
    tris, _ = E.extract_surface(torch.from_numpy(volume_of(name)).cuda(), 0.5, -1.5, 1.5)
    return tris, E.SimpleMesh(tris.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _want(name, cells, position):
    """The checker's mesh for a marching-cubes case - computed once, read by all."""
    cell, origin = grid_of(name, cells)
    return E.simplify_mesh(_case(name)[1], cell, origin, position)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_equal(out, want):
    """A device result against the host path's: the same bits in the same order, the same record."""
    assert out.device_triangles is not None and out.device_triangles.is_cuda and out.device_triangles.dtype == torch.float32
    assert out.device_triangles.is_contiguous() and out.device_triangles.shape == want.triangles.shape
    assert out.simplification == want.simplification, (out.simplification, want.simplification)
    assert np.array_equal(_bits(out.triangles), _bits(want.triangles))


def _both(soup, cell, origin=None, position="quadric"):
    """simplify_mesh on the device and on the host from one host soup -> the device mesh, compared."""
    soup = np.ascontiguousarray(soup, np.float32)
    out = E.simplify_mesh(E.SimpleMesh(torch.from_numpy(soup).cuda()), cell, origin, position)
    _assert_equal(out, E.simplify_mesh(E.SimpleMesh(soup), cell, origin, position))
    return out


@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("cells", [2, 3])
@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity(name, cells, position):
    tris, _ = _case(name)
    cell, origin = grid_of(name, cells)
    out = E.simplify_mesh(E.SimpleMesh(tris), cell, origin, position)
    _assert_equal(out, _want(name, cells, position))
    assert 0 < out.simplification.kept_faces < tris.shape[0]


def test_the_parity_cases_reach_the_duplicates_and_the_fallback():
    records = [_want(name, cells, position).simplification for name in PARITY_CASES for cells in (2, 3) for position in POSITIONS]
    assert any(s.duplicate_faces > 0 for s in records) and any(s.fallbacks > 0 for s in records)
    assert any(s.degenerate_faces > 0 for s in records)
    # and the device reports the same for one case that has both
    s = _want("noise23", 2, "quadric").simplification
    assert s.duplicate_faces > 0 and s.fallbacks > 0
    got = E.simplify_mesh(E.SimpleMesh(_case("noise23")[0]), *grid_of("noise23", 2)).simplification
    assert (got.duplicate_faces, got.fallbacks) == (s.duplicate_faces, s.fallbacks)


def test_parity_noise45():
    tris, ref = _case("noise45")
    cell, origin = grid_of("noise45", 2)
    _assert_equal(E.simplify_mesh(E.SimpleMesh(tris), cell, origin), E.simplify_mesh(ref, cell, origin))


def test_the_default_origin():
    tris, ref = _case("scene25")
    out = E.simplify_mesh(E.SimpleMesh(tris), 0.25)
    _assert_equal(out, E.simplify_mesh(ref, 0.25))
    assert out.simplification.origin == tuple(float(v) for v in ref.vertices.min(axis=0))


def _strip(n_vertices):
    """A triangle strip over n_vertices vertices (n_vertices - 2 faces), consistently wound, with a wavy third coordinate."""
    i = np.arange(n_vertices)
    verts = np.stack([(i // 2).astype(np.float32), (i % 2).astype(np.float32), np.sin(i * 0.37).astype(np.float32)], axis=1)
    j = np.arange(n_vertices - 2)
    faces = np.stack([np.where(j % 2 == 0, j, j + 1), np.where(j % 2 == 0, j + 1, j), j + 2], axis=1)
    return verts[faces]


@pytest.mark.parametrize("n_vertices", [255, 256, 257, 258, 2047, 2048, 2049, 2050, 2051])
def test_strips_around_the_workgroup_and_the_scan_tile(n_vertices):
    """Vertex counts - and, two below them, face counts - at the workgroup size and the scan tile and one to either side."""
    soup = _strip(n_vertices)
    for position in POSITIONS:
        out = _both(soup, 2.5, (-0.3, -0.3, -1.7), position)                     # clusters of up to six vertices
        assert 0 < out.simplification.kept_faces < n_vertices - 2 and out.simplification.clusters < n_vertices / 3
    # a cell per vertex: n_vertices clusters, the scan's total, and the input back
    alone = _both(soup, 0.4, (-0.3, -0.3, -1.7))
    assert alone.simplification.clusters == n_vertices and alone.simplification.kept_faces == n_vertices - 2
    assert np.array_equal(_bits(alone.triangles), _bits(soup))


def _fan(n=300):
    a = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([0.3 * np.cos(a), 0.3 * np.sin(a), 0.1 * np.cos(7 * a)], axis=1).astype(np.float32)
    hub = np.array([0.05, -0.02, 0.05], np.float32)
    return np.stack([np.broadcast_to(hub, (n, 3)), ring, np.roll(ring, -1, axis=0)], axis=1)


def test_a_hub_cluster_with_more_incidences_than_a_workgroup():
    soup = _fan(300)
    ref = E.SimpleMesh(soup)
    done = E.simplify_mesh_host(ref.vertices, ref.faces, (-0.5, -0.5, -0.5), 0.4)
    hub = done.cluster_of[int(np.flatnonzero((ref.vertices == soup[0, 0]).all(axis=1))[0])]
    incidences = np.bincount(done.cluster_of[ref.faces.reshape(-1)])
    assert incidences[hub] > 300 and np.bincount(done.cluster_of)[hub] > 1          # walked, not copied
    for position in POSITIONS:
        out = _both(soup, 0.4, (-0.5, -0.5, -0.5), position)
        assert 0 < out.simplification.kept_faces < 300


def test_one_cluster_and_a_cluster_per_vertex():
    tris, ref = _case("scene25")
    for position in POSITIONS:
        out = E.simplify_mesh(E.SimpleMesh(tris), 100.0, (-2.0, -2.0, -2.0), position)
        _assert_equal(out, E.simplify_mesh(ref, 100.0, (-2.0, -2.0, -2.0), position))
        s = out.simplification
        assert (s.kept_faces, s.clusters, s.degenerate_faces, s.duplicate_faces) == (0, 1, 2308, 0)
        assert out.device_triangles.shape == (0, 3, 3)
        cell, origin = grid_of("scene25", 0.001)
        same = E.simplify_mesh(E.SimpleMesh(tris), cell, origin, position)
        _assert_equal(same, E.simplify_mesh(ref, cell, origin, position))
        s = same.simplification
        assert (s.kept_faces, s.clusters, s.degenerate_faces, s.duplicate_faces, s.fallbacks) == (2308, 1160, 0, 0, 0)
        assert torch.equal(same.device_triangles.view(torch.int32), tris.view(torch.int32))       # the input's bits, its order


def run_device(vertices, faces, origin, cell, position):
    out = _both(vertices[faces], cell, origin, position)
    s = out.simplification
    return out.triangles, dict(kept=s.kept_faces, clusters=s.clusters, degenerate=s.degenerate_faces, duplicate=s.duplicate_faces,
                               fallbacks=s.fallbacks)


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_written_soups_on_the_device(name):
    check_hand_case(name, run_device)


def test_an_empty_mesh():
    out = E.simplify_mesh(E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda")), 0.5)
    assert out.device_triangles.is_cuda and out.device_triangles.shape == (0, 3, 3) and out.vertices.shape == (0, 3)
    s = out.simplification
    assert (s.input_faces, s.kept_faces, s.clusters, s.degenerate_faces, s.duplicate_faces) == (0, 0, 0, 0, 0)


def test_negative_coordinates_and_a_vertex_on_a_cell_plane():
    tris, ref = _case("sphere17")
    shifted = (tris - 7.25).contiguous()                                           # every coordinate negative
    ref_shifted = E.SimpleMesh(shifted.cpu().numpy())
    for origin in ((-9.5, -9.25, -9.125), None):
        out = E.simplify_mesh(E.SimpleMesh(shifted), 0.3, origin)
        _assert_equal(out, E.simplify_mesh(ref_shifted, 0.3, origin))
        assert 0 < out.simplification.kept_faces < 676
    # vertices exactly on cell planes: quarters on a grid of halves through -1 (a vertex on a plane belongs to the cell above)
    q = np.float32(0.25)
    verts = np.array([[-2, -2, -2], [2, -2, -2], [-2, 2, -2], [-2, -2, 2], [-1, -2, -2], [-3, -2, -2], [0, 0, -2], [1, 1, 1]],
                     np.float32) * q
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [4, 6, 7], [5, 6, 7], [0, 4, 6], [5, 1, 7]])
    done = E.simplify_mesh_host(verts, faces, (-1.0, -1.0, -1.0), 0.5)
    # x = -0.5 lies on a plane: with -0.25 in the cell above it, not with -0.75 in the cell below
    assert done.cluster_of[0] == done.cluster_of[4] != done.cluster_of[5] and done.counts["clusters"] == 7
    _both(verts[faces], 0.5, (-1.0, -1.0, -1.0))
    _both(verts[faces], 0.75, (-1.0, -1.0, -1.0), "mean")
    # and the marching-cubes lattice itself on the planes: origin at the range's minimum, whole cells
    edge = 3.0 / 17
    out = E.simplify_mesh(E.SimpleMesh(tris), 2 * edge, (-1.5, -1.5, -1.5))
    _assert_equal(out, E.simplify_mesh(ref, 2 * edge, (-1.5, -1.5, -1.5)))


def test_two_runs_give_the_same_bytes():
    tris, _ = _case("noise23")
    cell, origin = grid_of("noise23", 2)
    for position in POSITIONS:
        a, b = (E.simplify_mesh(E.SimpleMesh(tris), cell, origin, position) for _ in range(2))
        assert torch.equal(a.device_triangles.view(torch.int32), b.device_triangles.view(torch.int32))
        assert a.simplification == b.simplification


def test_the_result_is_resident_and_carries_nothing():
    tris, _ = _case("scene25")
    mesh = E.SimpleMesh(tris)
    mesh.adjacency, mesh.components                                                # the input carries a weld and more
    cell, origin = grid_of("scene25", 2)
    out = E.simplify_mesh(mesh, cell, origin)
    assert out.device_triangles.is_cuda and out._triangles is None and out._indexed is None and out._normals is None
    assert out._device_weld is None and out._components is None and out._adjacency is None
    assert out.device_vertex_colors is None and out.device_field_normals is None
    assert out.device_triangles.data_ptr() != tris.data_ptr() and out.device_triangles.shape == (444, 3, 3)
    assert mesh._device_weld is not None and mesh.device_triangles.data_ptr() == tris.data_ptr()
    fresh = E.SimpleMesh(tris)
    E.simplify_mesh(fresh, cell, origin)
    assert fresh._device_weld is not None                                          # the weld it made is kept
    with pytest.raises(ValueError, match="cell"):
        E.simplify_mesh(mesh, 0.0)
    with pytest.raises(ValueError, match="position"):
        E.simplify_mesh(mesh, 0.5, position="median")
    assert E.mesh_report(out)["simplification"]["kept_faces"] == 444 and "simplification" not in E.mesh_report(mesh)


def _raw(vertices, faces, origin, cell, mode=1):
    """zs_mesh_simplify on buffers of the right sizes -> (return code, out_counts, the filled part of out_tris)."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    v = torch.tensor(np.asarray(vertices, np.float32), device="cuda").reshape(-1, 3).contiguous()
    f = torch.tensor(np.asarray(faces, np.int32), device="cuda").reshape(-1, 3).contiguous()
    o = torch.tensor(origin, dtype=torch.float64, device="cuda")
    n, n_verts = f.shape[0], v.shape[0]
    room = torch.full((n, 3, 3), -9.0, dtype=torch.float32, device="cuda")
    counts = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.zs_mesh_simplify_scratch_bytes(n, n_verts) // 8 + 1, dtype=torch.int64, device="cuda")
    rc = lib.zs_mesh_simplify(_lib.ptr(v), _lib.ptr(f), n, n_verts, _lib.ptr(o), float(cell), mode, _lib.ptr(room), _lib.ptr(counts),
                              _lib.ptr(scratch), _lib.current_stream_ptr(v.device))
    torch.cuda.synchronize()
    return rc, counts.tolist(), room.cpu().numpy()


def test_status_words():
    """A vertex that is not finite, a grid finer than 2^21 cells and a face index outside the vertices: the call returns, the
    status word says which, every count stays consistent and nothing is written past the kept faces."""
    _, ref = _case("sphere17")
    verts, faces = ref.vertices, ref.faces.astype(np.int32)
    n = len(faces)
    cell, origin = grid_of("sphere17", 2)
    rc, counts, room = _raw(verts, faces, origin, cell)
    want = E.simplify_mesh_host(verts, faces, origin, cell)
    assert rc == 1 and counts == [136, 70, 540, 0, 0, 0] and np.array_equal(_bits(room[:136]), _bits(want.triangles))
    assert np.all(room[136:] == -9.0)
    for bad in (np.nan, np.inf, -np.inf):
        broken = verts.copy()
        broken[7, 1] = bad
        rc, counts, room = _raw(broken, faces, origin, cell)
        assert rc == 1 and counts[4] == 1 and counts[0] + counts[2] + counts[3] == n and np.all(room[counts[0]:] == -9.0)
    rc, counts, room = _raw(verts, faces, origin, 1e-7)                                            # about 3e7 cells per axis
    assert rc == 1 and counts[4] == 1 and counts[0] + counts[2] + counts[3] == n
    rc, counts, room = _raw(verts, faces, (0.0, 0.0, 0.0), cell)                                   # vertices below the origin
    assert rc == 1 and counts[4] == 1
    outside = faces.copy()
    outside[3, 2], outside[9, 0] = len(verts), -1
    for mode in (1, 0):
        rc, counts, room = _raw(verts, outside, origin, cell, mode)
        assert rc == 1 and counts[4] == 2 and counts[0] + counts[2] + counts[3] == n and np.all(room[counts[0]:] == -9.0)
        assert np.all(np.isfinite(room[:counts[0]]))
    broken = verts.copy()
    broken[7, 1] = np.nan
    assert _raw(broken, outside, origin, cell)[1][4] == 3
    # through simplify_mesh: the host path's ValueError
    from zeroshape_amd import _lib
    bad_soup = torch.from_numpy(ref.triangles.copy()).cuda()
    bad_soup[5, 1, 2] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        E.simplify_mesh(E.SimpleMesh(bad_soup), cell, origin)
    with pytest.raises(ValueError, match="outside"):
        E.simplify_mesh(E.SimpleMesh(_case("sphere17")[0]), 1e-7)
    mesh = E.SimpleMesh(torch.zeros(n, 3, 3, device="cuda"))
    mesh._device_weld = (torch.from_numpy(verts).cuda(), torch.from_numpy(outside).cuda(), None)
    with pytest.raises(_lib.ZeroShapeHipError, match="status 2"):
        E.simplify_mesh(mesh, cell, origin)


def test_argument_checks_of_the_raw_entry_point():
    """0 and a message that names the entry point, before anything is launched (a host buffer stands in for every non-null
    pointer: nothing may read it); zero sizes return 1."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p, odd = ctypes.c_void_p(base + (-base) % 8), ctypes.c_void_p(base + (-base) % 8 + 4)

    def fails(rc, what):
        msg = lib.zs_last_error()
        assert rc == 0 and msg.startswith(b"zs_mesh_simplify: ") and what.encode() in msg, (what, rc, msg)

    def call(n=1, v=3, cell=0.5, mode=1, ptr=p, scratch=p, **null):
        args = dict(vertices=ptr, faces=ptr, origin=ptr, out_tris=ptr, out_counts=ptr)
        args.update(null)
        return lib.zs_mesh_simplify(args["vertices"], args["faces"], n, v, args["origin"], cell, mode, args["out_tris"],
                                    args["out_counts"], scratch, None)

    fails(call(n=-1), "negative size")
    fails(call(v=-3), "negative size")
    fails(call(n=2 ** 28 + 1), "too large")
    fails(call(n=2 ** 22, v=2 ** 21 + 1), "too large")
    fails(call(n=1, v=4), "bad vertex count")
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        fails(call(cell=bad), "cell must be")
    for bad in (-1, 2):
        fails(call(mode=bad), "mode must be")
    for name in ("vertices", "faces", "origin", "out_tris", "out_counts"):
        fails(call(**{name: None}), "null pointer")
    fails(call(scratch=None), "null pointer")
    fails(call(scratch=odd), "8-byte aligned")
    assert call(n=0, v=0, ptr=None, scratch=None) == 1
    size = lib.zs_mesh_simplify_scratch_bytes
    assert size(0, 0) == 0 and size(-1, 3) == 0 and size(1, 4) == 0 and size(2 ** 28 + 1, 3) == 0 and size(2 ** 22, 2 ** 21 + 1) == 0
    assert size(1, 3) > 0 and size(1, 3) % 256 == 0 and size(2 ** 22, 2 ** 21) > size(1, 3)


def _opt(tmp_path, **extra):
    return edict(dict(device="cuda", output_path=str(tmp_path), eval=dict(range=[-1.5, 1.5], vox_res=25, num_points=2000, **extra)))


def test_through_the_pipelines(tmp_path):
    vol = torch.from_numpy(volume_of("scene25")).cuda()
    tris, ref = _case("scene25")
    want = _want("scene25", 2, "quadric")                                          # the host path, the pipelines' grid
    meshes, clouds = E.convert_to_explicit(_opt(tmp_path, simplify_cells=2), [vol], 0.5, to_pointcloud=True, seed=3)
    _assert_equal(meshes[0], want)
    again = E.sample_surface(meshes[0].device_triangles, 2000, 3).cpu().numpy()
    assert clouds.dtype == np.float64 and clouds.shape == (1, 2000, 3) and np.array_equal(clouds[0], again.astype(np.float64))
    _assert_equal(E.convert_to_explicit(_opt(tmp_path, simplify_cells=2.0), [vol], 0.5)[0], want)
    meshes2, cloud2 = E._surface_clouds(_opt(tmp_path, simplify_cells=2), vol[None], seed=3)
    _assert_equal(meshes2[0], want)
    assert cloud2.is_cuda and np.array_equal(cloud2[0].cpu().numpy(), again)
    mean = E.convert_to_explicit(_opt(tmp_path, simplify_cells=3, simplify_position="mean"), [vol], 0.5)[0]
    _assert_equal(mean, _want("scene25", 3, "mean"))
    # after the component filter and the smoothing
    cell, origin = grid_of("scene25", 2)
    chain = E.simplify_mesh(E.smooth_mesh(E.filter_components(ref, 0.1, False), 2), cell, origin)
    for got, _ in (E.convert_to_explicit(_opt(tmp_path, simplify_cells=2, min_component_area=0.1, smooth_iterations=2), [vol], 0.5,
                                         to_pointcloud=True, seed=3),
                   E._surface_clouds(_opt(tmp_path, simplify_cells=2, min_component_area=0.1, smooth_iterations=2), vol[None], seed=3)):
        _assert_equal(got[0], chain)
        assert got[0].simplification.input_faces == 288 + 1928
    # without the option: today's calls, bit for bit
    direct_tris, direct_pts = E.extract_surface(vol, 0.5, -1.5, 1.5, 2000, 3)
    plain_m, plain_c = E.convert_to_explicit(_opt(tmp_path), [vol], 0.5, to_pointcloud=True, seed=3)
    assert plain_m[0]._device_weld is None and not hasattr(plain_m[0], "simplification")
    assert torch.equal(plain_m[0].device_triangles.view(torch.int32), direct_tris.view(torch.int32))
    assert np.array_equal(plain_c[0], direct_pts.cpu().numpy().astype(np.float64))
    plain2_m, plain2_c = E._surface_clouds(_opt(tmp_path), vol[None], seed=3)
    assert torch.equal(plain2_m[0].device_triangles.view(torch.int32), direct_tris.view(torch.int32))
    assert torch.equal(plain2_c[0].view(torch.int32), direct_pts.view(torch.int32))
    with pytest.raises(ValueError, match="simplify_cells"):
        E.convert_to_explicit(_opt(tmp_path, simplify_position="mean"), [vol], 0.5)
