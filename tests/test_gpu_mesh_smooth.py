"""GPU: the adjacency and smoothing kernels (csrc/mesh_smooth.hip) against their checkers eval_3D.mesh_adjacency_host and
eval_3D.smooth_vertices_host - equal, not close: the CSR, the flags and the uint32 views of the smoothed soups - on
marching-cubes soups, on strips around the workgroup size and the scan tile, on a fan whose hub has a row longer than a
workgroup and on hand-written soups; the raw entry points' argument checks and status words; determinism; the opt-in through
convert_to_explicit and _surface_clouds."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_mesh_components_host_logic import KNOWN, volume_of
from tests.test_mesh_smooth_host_logic import check_hand_mesh, hand_meshes
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu

CASES = list(KNOWN)
#           iterations, lamb, mu, pin_boundary
TAUBIN = (10, 0.5, -0.53, True)
LAPLACE_FREE = (3, 0.5, None, False)
ONE_PINNED = (1, 0.5, -0.53, True)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(soup on the GPU, the numpy-welded host mesh of its host copy) - computed once, read by all."""
    tris, _ = E.extract_surface(torch.from_numpy(volume_of(name)).cuda(), 0.5, -1.5, 1.5)
    return tris, E.SimpleMesh(tris.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_adjacency_equal(got, want):
    for t, dtype in ((got.device_offsets, torch.int32), (got.device_neighbors, torch.int32), (got.device_boundary, torch.uint8)):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()
    assert got.offsets.dtype == np.int32 and got.neighbors.dtype == np.int32 and got.boundary.dtype == np.uint8
    assert got.offsets.shape == want.offsets.shape and np.array_equal(got.offsets, want.offsets)
    assert got.neighbors.shape == want.neighbors.shape and np.array_equal(got.neighbors, want.neighbors)
    assert got.boundary.shape == want.boundary.shape and np.array_equal(got.boundary, want.boundary)
    assert got.n_edges == want.n_edges and np.array_equal(got.degree, want.degree)


def _assert_smooth_equal(tris, ref, args):
    """smooth_mesh on the device against smooth_mesh on the host mesh: the same bits, on the device, in face order."""
    out = E.smooth_mesh(E.SimpleMesh(tris), *args)
    want = E.smooth_mesh(ref, *args)
    assert out.device_triangles is not None and out.device_triangles.is_cuda and out.device_triangles.dtype == torch.float32
    assert out._triangles is None and out._device_weld is None and out._components is None and out._adjacency is None
    assert out.device_triangles.shape == tris.shape
    assert np.array_equal(_bits(out.triangles), _bits(want.triangles))
    return out


@pytest.mark.parametrize("name", CASES)
def test_adjacency_parity(name):
    tris, ref = _case(name)
    mesh = E.SimpleMesh(tris)
    got = mesh.adjacency
    _assert_adjacency_equal(got, ref.adjacency)
    assert got.n_edges == KNOWN[name][4]
    assert mesh.adjacency is got and mesh._device_weld is not None                   # cached; the weld is kept
    rows = mesh.vertex_neighbors
    assert len(rows) == len(ref.vertices) and np.array_equal(np.concatenate(rows), ref.adjacency.neighbors)


@pytest.mark.parametrize("args", [TAUBIN, LAPLACE_FREE, ONE_PINNED], ids=["taubin10", "laplace3_free", "one_pinned"])
@pytest.mark.parametrize("name", ["sphere17", "sphere17_clipped", "scene25", "noise9", "noise23", "three_valued"])
def test_smoothing_parity(name, args):
    tris, ref = _case(name)
    out = _assert_smooth_equal(tris, ref, args)
    assert not np.array_equal(_bits(out.triangles), _bits(ref.triangles))            # something moved


def test_smoothing_parity_noise45():
    tris, ref = _case("noise45")
    _assert_smooth_equal(tris, ref, (2, 0.5, -0.53, True))


def _strip(n_vertices):
    """A triangle strip over n_vertices vertices (n_vertices - 2 faces), consistently wound, with a wavy third coordinate so
    that smoothing moves something."""
    i = np.arange(n_vertices)
    verts = np.stack([(i // 2).astype(np.float32), (i % 2).astype(np.float32), np.sin(i * 0.37).astype(np.float32)], axis=1)
    j = np.arange(n_vertices - 2)
    faces = np.stack([np.where(j % 2 == 0, j, j + 1), np.where(j % 2 == 0, j + 1, j), j + 2], axis=1)
    return verts[faces]


@pytest.mark.parametrize("n_vertices", [255, 256, 257, 2047, 2048, 2049, 4097])
def test_strips_around_the_workgroup_and_the_scan_tile(n_vertices):
    soup = _strip(n_vertices)
    tris, ref = torch.from_numpy(soup).cuda(), E.SimpleMesh(soup)
    assert len(ref.vertices) == n_vertices
    mesh = E.SimpleMesh(tris)
    _assert_adjacency_equal(mesh.adjacency, ref.adjacency)
    assert mesh.adjacency.boundary.all() and mesh.adjacency.n_edges == 2 * n_vertices - 3
    free = _assert_smooth_equal(tris, ref, (4, 0.5, -0.53, False))
    assert not np.array_equal(_bits(free.triangles), _bits(soup))
    pinned = _assert_smooth_equal(tris, ref, (4, 0.5, -0.53, True))
    assert np.array_equal(_bits(pinned.triangles), _bits(soup))


def _fan(n=300):
    a = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(a), np.sin(a), 0.1 * np.cos(7 * a)], axis=1).astype(np.float32)
    hub = np.array([0.05, -0.02, 0.5], np.float32)
    return np.stack([np.broadcast_to(hub, (n, 3)), ring, np.roll(ring, -1, axis=0)], axis=1)


def test_a_hub_with_a_row_longer_than_a_workgroup():
    soup = _fan(300)
    tris, ref = torch.from_numpy(soup).cuda(), E.SimpleMesh(soup)
    mesh = E.SimpleMesh(tris)
    _assert_adjacency_equal(mesh.adjacency, ref.adjacency)
    adj = ref.adjacency
    hub = int(np.argmax(adj.degree))
    assert adj.degree[hub] == 300 and len(ref.vertices) == 301 and adj.n_edges == 600
    assert adj.boundary[hub] == 0 and int(adj.boundary.sum()) == 300
    pinned = _assert_smooth_equal(tris, ref, (1, 0.5, None, True))
    # only the hub moves, to the checker's value
    moved = E.smooth_vertices_host(ref.vertices, adj.offsets, adj.neighbors, adj.boundary, 1, 0.5, None, True)
    assert np.array_equal(_bits(np.delete(moved, hub, axis=0)), _bits(np.delete(ref.vertices, hub, axis=0)))
    assert not np.array_equal(moved[hub], ref.vertices[hub])
    assert np.array_equal(_bits(pinned.triangles), _bits(moved[ref.faces]))
    _assert_smooth_equal(tris, ref, (1, 0.5, None, False))
    _assert_smooth_equal(tris, ref, (5, 0.5, -0.53, False))


@pytest.mark.parametrize("name", sorted(hand_meshes()))
def test_hand_written_meshes_on_the_device(name):
    mesh = check_hand_mesh(name, lambda soup: E.SimpleMesh(torch.from_numpy(soup).cuda()))
    assert mesh.adjacency.device_offsets is not None and mesh.adjacency.device_offsets.is_cuda
    _assert_adjacency_equal(mesh.adjacency, E.SimpleMesh(hand_meshes()[name]).adjacency)


def test_an_empty_mesh():
    mesh = E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda"))
    adj = mesh.adjacency
    assert adj.device_offsets.tolist() == [0] and adj.device_neighbors.shape == (0,) and adj.device_boundary.shape == (0,)
    assert adj.n_edges == 0 and mesh.vertex_neighbors == []
    out = E.smooth_mesh(mesh, 3)
    assert out.device_triangles.is_cuda and out.device_triangles.shape == (0, 3, 3) and out.vertices.shape == (0, 3)


def test_zero_iterations_and_argument_checks():
    tris, ref = _case("sphere17_clipped")
    out = E.smooth_mesh(E.SimpleMesh(tris), 0)
    assert out.device_triangles is not tris and torch.equal(out.device_triangles.view(torch.int32), tris.view(torch.int32))
    mesh = E.SimpleMesh(tris)
    for bad in (dict(iterations=-1), dict(iterations=2.5), dict(lamb=0.0), dict(lamb=1.5), dict(mu=0.0), dict(mu=-1.5)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            E.smooth_mesh(mesh, **bad)
    assert mesh._adjacency is None                                                   # checked before anything is computed


def test_two_runs_give_the_same_bytes():
    tris, _ = _case("noise23")
    a, b = E.mesh_adjacency(E.SimpleMesh(tris)), E.mesh_adjacency(E.SimpleMesh(tris))
    for key in ("device_offsets", "device_neighbors", "device_boundary"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    x, y = E.smooth_mesh(E.SimpleMesh(tris)), E.smooth_mesh(E.SimpleMesh(tris))
    assert torch.equal(x.device_triangles.view(torch.int32), y.device_triangles.view(torch.int32))


def test_argument_checks_of_the_raw_entry_points():
    """0 and a message that names the entry point, before anything is launched (a host buffer stands in for every non-null
    pointer: nothing may read it); zero sizes return 1."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p, odd = ctypes.c_void_p(base + (-base) % 8), ctypes.c_void_p(base + (-base) % 8 + 4)
    q = ctypes.c_void_p(p.value + 64)

    def fails(name, rc, what):
        msg = lib.zs_last_error()
        assert rc == 0 and msg.startswith(name.encode() + b": ") and what.encode() in msg, (name, what, rc, msg)

    adj = lambda n, v, ptr=p, scratch=p: lib.zs_mesh_adjacency(ptr, n, v, ptr, ptr, ptr, ptr, scratch, None)
    fails("zs_mesh_adjacency", adj(-1, 3), "negative size")
    fails("zs_mesh_adjacency", adj(1, -3), "negative size")
    fails("zs_mesh_adjacency", adj(1, 4), "bad vertex count")
    fails("zs_mesh_adjacency", adj(2 ** 28 + 1, 3), "too large")
    fails("zs_mesh_adjacency", adj(1, 3, None), "null pointer")
    fails("zs_mesh_adjacency", adj(1, 3, p, None), "null pointer")
    fails("zs_mesh_adjacency", adj(1, 3, p, odd), "8-byte aligned")
    assert adj(0, 0, None, None) == 1
    assert lib.zs_mesh_adjacency_scratch_bytes(0, 0) == 0 and lib.zs_mesh_adjacency_scratch_bytes(-1, 3) == 0
    assert lib.zs_mesh_adjacency_scratch_bytes(1, 4) == 0 and lib.zs_mesh_adjacency_scratch_bytes(2 ** 28 + 1, 3) == 0
    assert lib.zs_mesh_adjacency_scratch_bytes(1, 3) % 256 == 0 and lib.zs_mesh_adjacency_scratch_bytes(1, 3) > 0

    def smooth(v, passes=2, lamb=0.5, mu=-0.53, alternate=1, ptr=p, out=q, scratch=p):
        return lib.zs_mesh_smooth(ptr, v, ptr, ptr, None, passes, lamb, mu, alternate, out, ptr, scratch, None)

    fails("zs_mesh_smooth", smooth(-1), "negative size")
    fails("zs_mesh_smooth", smooth(3, passes=-1), "negative size")
    fails("zs_mesh_smooth", smooth(3 * 2 ** 28 + 1), "too large")
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        fails("zs_mesh_smooth", smooth(3, lamb=bad), "lambda")
    for bad in (0.0, 0.5, -1.0001, float("nan")):
        fails("zs_mesh_smooth", smooth(3, mu=bad), "mu must")
    fails("zs_mesh_smooth", smooth(3, ptr=None), "null pointer")
    fails("zs_mesh_smooth", smooth(3, out=None), "null pointer")
    fails("zs_mesh_smooth", smooth(3, scratch=None), "null pointer")
    fails("zs_mesh_smooth", smooth(3, scratch=odd), "8-byte aligned")
    fails("zs_mesh_smooth", smooth(3, out=p), "must not be the input")
    assert smooth(0, ptr=None, out=None, scratch=None) == 1
    assert lib.zs_mesh_smooth_scratch_bytes(0) == 0 and lib.zs_mesh_smooth_scratch_bytes(-1) == 0
    assert lib.zs_mesh_smooth_scratch_bytes(3 * 2 ** 28 + 1) == 0 and lib.zs_mesh_smooth_scratch_bytes(3) == 512

    gather = lambda n, v, ptr=p: lib.zs_mesh_gather_faces(ptr, ptr, n, v, ptr, None)
    fails("zs_mesh_gather_faces", gather(-1, 3), "negative size")
    fails("zs_mesh_gather_faces", gather(1, -3), "negative size")
    fails("zs_mesh_gather_faces", gather(2 ** 28 + 1, 3), "too large")
    fails("zs_mesh_gather_faces", gather(1, 3, None), "null pointer")
    assert gather(0, 0, None) == 1 and gather(0, 5, None) == 1


def test_a_face_index_outside_the_vertices():
    """Status 2, and ZeroShapeHipError through mesh_adjacency; the other faces' edges are still there, the rejected face
    contributes none."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    faces = torch.tensor([[0, 1, 2], [2, 1, 4], [1, 3, 2]], dtype=torch.int32, device="cuda")         # 4 == n_verts
    n, n_verts = 3, 4
    offsets = torch.empty(n_verts + 1, dtype=torch.int32, device="cuda")
    neighbors = torch.full((6 * n,), -7, dtype=torch.int32, device="cuda")
    boundary = torch.empty(n_verts, dtype=torch.uint8, device="cuda")
    out = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.zs_mesh_adjacency_scratch_bytes(n, n_verts) // 8 + 1, dtype=torch.int64, device="cuda")
    _lib.check(lib.zs_mesh_adjacency(_lib.ptr(faces), n, n_verts, _lib.ptr(offsets), _lib.ptr(neighbors), _lib.ptr(boundary),
                                     _lib.ptr(out), _lib.ptr(scratch), _lib.current_stream_ptr(faces.device)), "zs_mesh_adjacency")
    want = E.mesh_adjacency_host(faces[[0, 2]].cpu().numpy(), n_verts)
    assert out.tolist() == [len(want.neighbors), 2]
    assert offsets.tolist() == want.offsets.tolist() and boundary.tolist() == want.boundary.tolist()
    assert neighbors.tolist() == want.neighbors.tolist() + [-7] * (6 * n - len(want.neighbors))       # nothing past nnz
    mesh = E.SimpleMesh(torch.zeros(3, 3, 3, device="cuda"))
    mesh._device_weld = (torch.zeros(n_verts, 3, device="cuda"), faces, None)
    with pytest.raises(_lib.ZeroShapeHipError, match="status 2"):
        E.mesh_adjacency(mesh)


def test_rows_that_cannot_be_followed_set_the_status():
    """zs_mesh_smooth on a hand-made CSR: a neighbour index outside the vertices (status 2) and rows that run backwards or
    past offsets[V] (status 1) are not followed - those vertices are copied, the others move."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    x = torch.tensor([[0, 0, 0], [2, 4, 6], [1, 1, 1]], dtype=torch.float32, device=dev)

    def run(offsets, neighbors, passes=1):
        off = torch.tensor(offsets, dtype=torch.int32, device=dev)
        nb = torch.tensor(neighbors, dtype=torch.int32, device=dev)
        out, status = torch.full_like(x, -9.0), torch.full((1,), -1, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.zs_mesh_smooth_scratch_bytes(3) // 8, dtype=torch.int64, device=dev)
        _lib.check(lib.zs_mesh_smooth(_lib.ptr(x), 3, _lib.ptr(off), _lib.ptr(nb), None, passes, 0.5, 0.0, 0, _lib.ptr(out),
                                      _lib.ptr(status), _lib.ptr(scratch), _lib.current_stream_ptr(dev)), "zs_mesh_smooth")
        return out.tolist(), int(status.item())

    assert run([0, 1, 2, 2], [1, 0]) == ([[1, 2, 3], [1, 2, 3], [1, 1, 1]], 0)
    assert run([0, 1, 2, 2], [1, 3]) == ([[1, 2, 3], [2, 4, 6], [1, 1, 1]], 2)
    assert run([0, 1, 2, 2], [1, -1]) == ([[1, 2, 3], [2, 4, 6], [1, 1, 1]], 2)
    assert run([0, 2, 1, 1], [1, 0]) == ([[0, 0, 0], [2, 4, 6], [1, 1, 1]], 1)           # row 0 runs past offsets[V], row 1 backwards
    assert run([0, 1, 2, 2], [1, 0], passes=0) == (x.tolist(), 0)
    assert run([0, 1, 2, 2], [1, 0], passes=2) == ([[1, 2, 3], [1, 2, 3], [1, 1, 1]], 0)   # the two swap their means: (1, 2, 3) stays


def _opt(tmp_path, **extra):
    return edict(dict(device="cuda", output_path=str(tmp_path), eval=dict(range=[-1.5, 1.5], num_points=2000, **extra)))


def test_through_the_pipelines(tmp_path):
    vol = torch.from_numpy(volume_of("scene25")).cuda()
    tris, ref = _case("scene25")
    want = E.smooth_mesh(E.SimpleMesh(tris), 4)
    meshes, clouds = E.convert_to_explicit(_opt(tmp_path, smooth_iterations=4), [vol], 0.5, to_pointcloud=True, seed=3)
    assert meshes[0].device_triangles.is_cuda and torch.equal(meshes[0].device_triangles.view(torch.int32),
                                                              want.device_triangles.view(torch.int32))
    again = E.sample_surface(want.device_triangles, 2000, 3).cpu().numpy()
    assert clouds.dtype == np.float64 and clouds.shape == (1, 2000, 3) and np.array_equal(clouds[0], again.astype(np.float64))
    only_mesh = E.convert_to_explicit(_opt(tmp_path, smooth_iterations=4), [vol], 0.5)
    assert torch.equal(only_mesh[0].device_triangles.view(torch.int32), want.device_triangles.view(torch.int32))
    meshes2, cloud2 = E._surface_clouds(_opt(tmp_path, smooth_iterations=4), vol[None], seed=3)
    assert torch.equal(meshes2[0].device_triangles.view(torch.int32), want.device_triangles.view(torch.int32))
    assert cloud2.is_cuda and np.array_equal(cloud2[0].cpu().numpy(), again)
    # the other options reach smooth_mesh
    lap = E.convert_to_explicit(_opt(tmp_path, smooth_iterations=3, smooth_lambda=0.4, smooth_mu="none",
                                     smooth_free_boundary=True), [vol], 0.5)[0]
    assert torch.equal(lap.device_triangles.view(torch.int32),
                       E.smooth_mesh(E.SimpleMesh(tris), 3, 0.4, None, False).device_triangles.view(torch.int32))
    # with the component filter: filtering comes first
    solid = E.filter_components(E.SimpleMesh(tris), 0.1, False)
    assert solid.device_triangles.shape[0] == 288 + 1928                                  # the floater is gone
    want_f = E.smooth_mesh(solid, 4)
    for got, pts in (E.convert_to_explicit(_opt(tmp_path, smooth_iterations=4, min_component_area=0.1), [vol], 0.5,
                                           to_pointcloud=True, seed=3),
                     E._surface_clouds(_opt(tmp_path, smooth_iterations=4, min_component_area=0.1), vol[None], seed=3)):
        assert torch.equal(got[0].device_triangles.view(torch.int32), want_f.device_triangles.view(torch.int32))
        pts = pts[0].cpu().numpy() if isinstance(pts, torch.Tensor) else pts[0]
        assert np.array_equal(pts, E.sample_surface(want_f.device_triangles, 2000, 3).cpu().numpy().astype(pts.dtype))
    # without the options: today's calls, bit for bit
    direct_tris, direct_pts = E.extract_surface(vol, 0.5, -1.5, 1.5, 2000, 3)
    plain_m, plain_c = E.convert_to_explicit(_opt(tmp_path), [vol], 0.5, to_pointcloud=True, seed=3)
    assert plain_m[0]._adjacency is None and plain_m[0]._device_weld is None               # nothing welded when not asked for
    assert torch.equal(plain_m[0].device_triangles.view(torch.int32), direct_tris.view(torch.int32))
    assert np.array_equal(plain_c[0], direct_pts.cpu().numpy().astype(np.float64))
    plain2_m, plain2_c = E._surface_clouds(_opt(tmp_path), vol[None], seed=3)
    assert torch.equal(plain2_m[0].device_triangles.view(torch.int32), direct_tris.view(torch.int32))
    assert torch.equal(plain2_c[0].view(torch.int32), direct_pts.view(torch.int32))
    assert not torch.equal(direct_tris, want.device_triangles)
