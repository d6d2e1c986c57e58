"""GPU: the point-to-mesh distance kernels (csrc/mesh_distance.hip) against their checker eval_3D.closest_point_on_mesh_host -
equal, not close: the uint64 views of the squared distances and the closest points, and the face indices - on marching-cubes
meshes with near, on-surface and far queries, on query and face counts around the workgroup size and the scan tile, on a flat
mesh, one cell, one huge face, degenerate and duplicated faces; the raw entry point's counts and argument checks; that the grid
prunes; zs_mesh_distance_stats against mesh_distance_stats_host; mesh_deviation against the host record; determinism; residency;
the opt-in through convert_to_explicit, _surface_clouds and demo.py.

The checker is a brute force in numpy (about 6 M pairs a second): where faces x queries would exceed PAIRS the queries are an
evenly strided subset, and for a mesh's own vertices the device answers all of them against the rule (distance 0, the lowest
face around the vertex, the vertex itself)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.test_mesh_components_host_logic import volume_of
from tests.test_mesh_simplify_host_logic import grid_of
from tests.test_oracle_mc import _sphere
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_CASES = ["sphere17", "sphere17_clipped", "scene25", "noise9", "noise23", "three_valued"]
PAIRS = 8 << 20


@functools.lru_cache(maxsize=None)
def _case(name):
    """(soup on the GPU, the numpy-welded host mesh of its host copy) - computed once, read by all."""
    tris, _ = E.extract_surface(torch.from_numpy(volume_of(name)).cuda(), 0.5, -1.5, 1.5)
    return tris, E.SimpleMesh(tris.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _sphere65():
    tris, _ = E.extract_surface(torch.from_numpy(_sphere(65, 1.0)[0]).cuda(), 0.5, -1.5, 1.5)
    return tris, E.SimpleMesh(tris.cpu().numpy())


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _strided(n, faces):
    keep = max(1, min(n, PAIRS // max(faces, 1)))
    return np.unique(np.linspace(0, n - 1, keep).astype(np.int64)) if n else np.zeros(0, np.int64)


def _raw(vertices, faces, queries, closest=True, fill=True):
    """zs_mesh_distance on buffers of the right sizes -> (return code, out_counts, sqdist, face, closest)."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    v = torch.tensor(np.asarray(vertices, np.float32), device="cuda").reshape(-1, 3).contiguous()
    f = torch.tensor(np.asarray(faces, np.int32), device="cuda").reshape(-1, 3).contiguous()
    q = torch.tensor(np.asarray(queries, np.float32), device="cuda").reshape(-1, 3).contiguous()
    n, n_verts, m = f.shape[0], v.shape[0], q.shape[0]
    sq = torch.full((m,), -9.0, dtype=torch.float64, device="cuda")
    face = torch.full((m,), -9, dtype=torch.int32, device="cuda")
    point = torch.full((m, 3), -9.0, dtype=torch.float64, device="cuda") if closest else None
    counts = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.zs_mesh_distance_scratch_bytes(n, m)
    assert nbytes > 0 and nbytes % 256 == 0
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    rc = lib.zs_mesh_distance(_lib.ptr(v), _lib.ptr(f), n, n_verts, _lib.ptr(q), m, _lib.ptr(sq), _lib.ptr(face), _lib.ptr(point),
                              _lib.ptr(counts), _lib.ptr(scratch), _lib.current_stream_ptr(v.device))
    torch.cuda.synchronize()
    return rc, counts.tolist(), sq.cpu().numpy(), face.cpu().numpy(), None if point is None else point.cpu().numpy()


def _pairs(counts):
    return (counts[3] & 0xffffffff) | ((counts[4] & 0xffffffff) << 32)


def _assert_raw_parity(vertices, faces, queries):
    """The raw entry point against the checker on one indexed mesh -> (counts, sqdist, face)."""
    rc, counts, sq, face, point = _raw(vertices, faces, queries)
    want = E.closest_point_on_mesh_host(queries, vertices, faces)
    assert rc == 1 and counts[0] == want[3]
    assert np.array_equal(face, want[1]), np.flatnonzero(face != want[1])[:8]
    assert np.array_equal(bits(sq), bits(want[0])) and np.array_equal(bits(point), bits(want[2]))
    return counts, sq, face


def _assert_mesh_parity(tris, host, queries):
    """mesh_distance on a GPU mesh against the checker on the numpy weld of the same soup; ``queries`` a host array."""
    mesh = E.SimpleMesh(tris)
    q = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).cuda()
    done = mesh.distance_to(q, closest=True)
    assert done.sqdist.is_cuda and done.sqdist.dtype == torch.float64 and done.face.dtype == torch.int32
    assert done.closest.is_cuda and done.closest.dtype == torch.float64 and done.closest.shape == (len(queries), 3)
    want = E.closest_point_on_mesh_host(queries, host.vertices, host.faces)
    assert np.array_equal(done.face.cpu().numpy(), want[1])
    assert np.array_equal(bits(done.sqdist.cpu().numpy()), bits(want[0])) and np.array_equal(bits(done.closest.cpu().numpy()), bits(want[2]))
    counts = done.check()
    assert counts["skipped_faces"] == 0 and counts["status"] == 0 and 0 < counts["pairs"] <= len(queries) * len(host.faces)
    return done, counts


@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity_on_a_mesh_s_own_vertices(name):
    """Distance 0 and a tie on every shared vertex: all vertices against the rule, a strided subset against the checker."""
    tris, host = _case(name)
    V, F = len(host.vertices), len(host.faces)
    done = E.mesh_distance(E.SimpleMesh(tris), torch.from_numpy(host.vertices).cuda(), closest=True)
    lowest = np.full(V, F)
    np.minimum.at(lowest, host.faces.reshape(-1), np.repeat(np.arange(F), 3))
    assert torch.all(done.sqdist == 0.0) and np.array_equal(done.face.cpu().numpy(), lowest)
    assert np.array_equal(bits(done.closest.cpu().numpy()), bits(host.vertices.astype(np.float64)))
    _assert_mesh_parity(tris, host, host.vertices[_strided(V, F)])


@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity_on_the_points_of_the_simplified_mesh(name):
    tris, host = _case(name)
    light = E.simplify_mesh(host, *grid_of(name, 2)).vertices
    _, counts = _assert_mesh_parity(tris, host, light[_strided(len(light), len(host.faces))])


@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity_on_far_queries(name):
    """1,000 seeded points in twice the bounding box: the search leaves the grid on every side."""
    tris, host = _case(name)
    lo, hi = host.vertices.min(axis=0).astype(np.float64), host.vertices.max(axis=0).astype(np.float64)
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q = (centre + np.random.RandomState(len(name)).uniform(-2, 2, (1000, 3)) * half).astype(np.float32)
    for a in range(3):
        assert (q[:, a] < lo[a]).any() and (q[:, a] > hi[a]).any()
    _assert_mesh_parity(tris, host, q)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_query_counts(m):
    tris, host = _case("scene25")
    q = np.random.RandomState(m).uniform(-1.6, 1.6, (m, 3)).astype(np.float32)
    q[::3] = host.vertices[(np.arange(len(q[::3])) * 7) % len(host.vertices)]       # some on the surface
    _assert_mesh_parity(tris, host, q)


def _strip(n_vertices):
    """A triangle strip over n_vertices vertices (n_vertices - 2 faces), consistently wound, with a wavy third coordinate."""
    i = np.arange(n_vertices)
    verts = np.stack([(i // 2).astype(np.float32), (i % 2).astype(np.float32), np.sin(i * 0.37).astype(np.float32)], axis=1)
    j = np.arange(n_vertices - 2)
    faces = np.stack([np.where(j % 2 == 0, j, j + 1), np.where(j % 2 == 0, j + 1, j), j + 2], axis=1)
    return verts, faces


@pytest.mark.parametrize("n_faces", [1, 2, 255, 256, 257, 2047, 2048, 2049])
def test_face_counts_around_the_workgroup_and_the_scan_tile(n_faces):
    verts, faces = _strip(n_faces + 2)
    rng = np.random.RandomState(n_faces)
    q = np.concatenate([rng.uniform(-2, 3, (300, 3)) * [n_faces / 4.0 + 1, 1, 1], verts[:: max(1, len(verts) // 200)],
                        0.5 * (verts[:-1] + verts[1:])[:: max(1, len(verts) // 100)]]).astype(np.float32)
    counts, sq, face = _assert_raw_parity(verts, faces, q)
    assert counts[:3] == [0, 0, 0] and np.all((face >= 0) & (face < n_faces)) and 0 < _pairs(counts) <= n_faces * len(q)


def test_a_flat_mesh():
    """One axis without extent (one slab), then two."""
    g = np.arange(24)
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * np.float32(0.25)
    quad = np.array([[i * 24 + j, (i + 1) * 24 + j, (i + 1) * 24 + j + 1, i * 24 + j + 1] for i in range(23) for j in range(23)])
    faces = np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]])
    rng = np.random.RandomState(4)
    q = rng.uniform(-2, 8, (400, 3)).astype(np.float32)
    q[:100, 2] = 1.5                                                               # in the plane
    for axis in range(3):
        verts = np.insert(grid, axis, np.float32(1.5), axis=1)
        counts, sq, face = _assert_raw_parity(verts, faces, np.roll(q, axis + 1, axis=1))
        assert 0 < _pairs(counts) < len(faces) * len(q)                            # the slab still prunes
    line = np.stack([np.arange(40) * 0.1, np.full(40, 2.0), np.full(40, -1.0)], axis=1).astype(np.float32)
    _assert_raw_parity(line, np.stack([np.arange(38), np.arange(38) + 1, np.arange(38) + 2], axis=1), q)


def test_all_faces_in_one_cell():
    """Fewer than sixteen faces make one cell; and many faces whose boxes share one centre fall into one cell of many."""
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    q = np.random.RandomState(5).uniform(-1, 2, (300, 3)).astype(np.float32)
    counts, _, _ = _assert_raw_parity(tet, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], q)
    assert _pairs(counts) == 4 * 300
    # 400 triangles around one centre: every box is centred at the origin
    rng = np.random.RandomState(6)
    a = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    b = a * rng.uniform(-1, 1, (400, 3)).astype(np.float32)                        # inside the box of a and -a
    verts = np.stack([a, b, -a], axis=1).reshape(-1, 3)
    faces = np.arange(1200).reshape(400, 3)
    boxes = verts[faces]
    assert np.all(boxes.min(axis=1) + boxes.max(axis=1) == 0)
    counts, _, _ = _assert_raw_parity(verts, faces, q)
    assert 0 < _pairs(counts) <= 400 * 300


def test_one_face_that_spans_the_box_among_2000_small_ones():
    """The largest half-extent is half the box: it governs the bound, which prunes little or nothing; the answer is still the
    checker's."""
    rng = np.random.RandomState(7)
    centres = rng.uniform(-1, 1, (2000, 1, 3))
    small = (centres + rng.uniform(-0.02, 0.02, (2000, 3, 3))).astype(np.float32)
    huge = np.array([[[-1.2, -1.2, -1.2], [1.2, 1.2, -1.1], [-1.1, 1.2, 1.2]]], np.float32)
    q = rng.uniform(-1.5, 1.5, (600, 3)).astype(np.float32)
    without, _, _ = _assert_raw_parity(small.reshape(-1, 3), np.arange(6000).reshape(-1, 3), q)
    for soup in (np.concatenate([small[:1000], huge, small[1000:]]), np.concatenate([huge, small])):
        verts = soup.reshape(-1, 3)
        faces = np.arange(len(verts)).reshape(-1, 3)
        counts, sq, face = _assert_raw_parity(verts, faces, q)
        big = int(np.flatnonzero((soup == huge[0]).all(axis=(1, 2)))[0])
        assert (face == big).any() and (face != big).any()
        print("pairs evaluated: %d with the huge face, %d without, of %d" % (_pairs(counts), _pairs(without), 2001 * 600))
        assert _pairs(without) < _pairs(counts) <= 2001 * 600


def test_degenerate_and_duplicated_faces_on_the_device():
    _, host = _case("sphere17")
    verts = np.concatenate([host.vertices, [[3, 3, 3], [3, 3, 3], [2, 2, 2]]]).astype(np.float32)
    V = len(host.vertices)
    extra = [[0, 0, 5], [7, 9, 9], [V, V, V], [V, V + 1, V], [V, V + 2, V + 1], [3, 3, 3]] + host.faces[:40].tolist() + host.faces[10:20, [1, 2, 0]].tolist()
    faces = np.concatenate([host.faces[:300], extra, host.faces[300:], host.faces[:5]])
    rng = np.random.RandomState(8)
    q = np.concatenate([rng.uniform(-2, 4, (400, 3)), verts[::3], [[2.5, 2.5, 2.5], [3, 3, 3], [4, 4, 4]]]).astype(np.float32)
    counts, sq, face = _assert_raw_parity(verts, faces, q)
    assert counts[:3] == [0, 0, 0] and np.all(np.isfinite(sq))
    assert face[-2] == 300 + 2 and sq[-2] == 0.0 and face[-3] == 300 + 4 and face[-1] == 300 + 2
    # only degenerate faces
    _assert_raw_parity(verts, np.array(extra[:6]), q)


def test_skipped_faces_and_queries_that_are_not_finite():
    _, host = _case("scene25")
    verts, faces = host.vertices.copy(), host.faces.copy()
    verts[7, 1], verts[11, 0], verts[500, 2] = np.nan, np.inf, -np.inf
    faces[3, 2], faces[9, 0], faces[2000, 1] = len(verts), -1, 2 ** 31 - 1
    bad = np.isin(faces, [7, 11, 500]).any(axis=1)
    bad[[3, 9, 2000]] = True
    q = np.random.RandomState(9).uniform(-1.6, 1.6, (500, 3)).astype(np.float32)
    q[5, 0], q[9, 2], q[20, 1], q[499] = np.nan, np.inf, -np.inf, np.nan
    rows = [5, 9, 20, 499]
    rc, counts, sq, face, point = _raw(verts, faces, q)
    assert rc == 1 and counts[:3] == [int(bad.sum()), 4, 1 | 2 | 4]
    assert np.all(np.isnan(sq[rows])) and np.all(face[rows] == -1) and np.all(np.isnan(point[rows]))
    rest = np.setdiff1d(np.arange(500), rows)
    keep = np.flatnonzero(~bad)
    want = E.closest_point_on_mesh_host(q[rest], np.nan_to_num(verts, posinf=0.0, neginf=0.0), faces[keep])
    assert np.array_equal(face[rest], keep[want[1]]) and np.array_equal(bits(sq[rest]), bits(want[0]))
    assert np.array_equal(bits(point[rest]), bits(want[2])) and 0 < _pairs(counts) <= len(keep) * len(rest)
    # one kind at a time: the status bits
    only = host.faces.copy()
    only[3, 2] = len(verts)
    assert _raw(host.vertices, only, q[rest])[1][:3] == [1, 0, 2]
    assert _raw(verts, host.faces, q[rest])[1][:3] == [int(np.isin(host.faces, [7, 11, 500]).any(axis=1).sum()), 0, 1]
    # no valid face at all, no vertices, no faces: +inf and -1, without closest too
    for v, f in ((verts[:3] * np.nan, [[0, 1, 2]]), (np.zeros((0, 3)), [[0, 1, 2]]), (verts, np.zeros((0, 3)))):
        rc, counts, sq, face, point = _raw(v, f, q, closest=False)
        assert rc == 1 and counts == [len(f), 4, (4 | (2 if len(v) == 0 else 1)) if len(f) else 4, 0, 0] and point is None
        assert np.all(sq[rest] == np.inf) and np.all(np.isnan(sq[rows])) and np.all(face == -1)
    # through mesh_distance: the face-index bit raises where the counts are read
    from zeroshape_amd import _lib
    mesh = E.SimpleMesh(torch.zeros(len(only), 3, 3, device="cuda"))
    mesh._device_weld = (torch.from_numpy(host.vertices).cuda(), torch.from_numpy(only.astype(np.int32)).cuda(), None)
    done = E.mesh_distance(mesh, torch.from_numpy(q).cuda())
    with pytest.raises(_lib.ZeroShapeHipError, match="status 6"):
        done.check()
    with pytest.raises(_lib.ZeroShapeHipError, match="face index"):
        E.mesh_deviation(mesh, E.SimpleMesh(_case("scene25")[0]))
    with pytest.raises(ValueError, match="CUDA"):
        E.mesh_distance(mesh, q)
    with pytest.raises(ValueError, match="CUDA"):
        E.mesh_distance(mesh, torch.from_numpy(q))


def test_argument_checks_of_the_raw_entry_points():
    """0 and a message that names the entry point, before anything is launched (a host buffer stands in for every non-null
    pointer: nothing may read it); zero queries return 1."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p, odd = ctypes.c_void_p(base + (-base) % 8), ctypes.c_void_p(base + (-base) % 8 + 4)

    def fails(rc, what, who=b"zs_mesh_distance: "):
        msg = lib.zs_last_error()
        assert rc == 0 and msg.startswith(who) and what.encode() in msg, (what, rc, msg)

    def call(n=1, v=3, m=1, ptr=p, scratch=p, **null):
        args = dict(vertices=ptr, faces=ptr, queries=ptr, out_sqdist=ptr, out_face=ptr, out_closest=ptr, out_counts=ptr)
        args.update(null)
        return lib.zs_mesh_distance(args["vertices"], args["faces"], n, v, args["queries"], m, args["out_sqdist"], args["out_face"],
                                    args["out_closest"], args["out_counts"], scratch, None)

    fails(call(n=-1), "negative size")
    fails(call(v=-3), "negative size")
    fails(call(m=-1), "negative size")
    fails(call(n=2 ** 24 + 1), "too large")
    fails(call(m=2 ** 28 + 1), "too large")
    for name in ("vertices", "faces", "queries", "out_sqdist", "out_face", "out_counts"):
        fails(call(**{name: None}), "null pointer")
    fails(call(scratch=None), "null pointer")
    fails(call(scratch=odd), "8-byte aligned")
    fails(call(scratch=odd, out_closest=None), "8-byte aligned")                  # out_closest may be null: the next check speaks
    assert call(m=0, ptr=None, scratch=None) == 1 and call(n=0, v=0, m=0, ptr=None, scratch=None) == 1
    size = lib.zs_mesh_distance_scratch_bytes
    assert size(-1, 1) == 0 and size(1, -1) == 0 and size(2 ** 24 + 1, 1) == 0 and size(1, 2 ** 28 + 1) == 0
    for n, m in ((0, 0), (0, 5), (1, 1), (17, 3), (2 ** 24, 2 ** 28)):
        assert size(n, m) > 0 and size(n, m) % 256 == 0
    assert size(2 ** 24, 1) > size(2 ** 20, 1) > size(1, 1)
    stats = lib.zs_mesh_distance_stats
    fails(stats(p, -1, p, p, None), "negative size", b"zs_mesh_distance_stats: ")
    for args in ((None, 1, p, p), (p, 1, None, p), (p, 1, p, None)):
        fails(stats(*args, None), "null pointer", b"zs_mesh_distance_stats: ")
    assert stats(None, 0, None, None, None) == 1


def test_pruning_is_real():
    """The 65^3 sphere (about 17k faces) against all its vertices: fewer than a tenth of faces x queries are evaluated (two
    faces per cell and a stop after ring 1 suggest about 2 %); 512 seeded queries against the checker."""
    tris, host = _sphere65()
    F, V = len(host.faces), len(host.vertices)
    assert 15000 < F < 20000
    done = E.mesh_distance(E.SimpleMesh(tris), torch.from_numpy(host.vertices).cuda())
    counts = done.check()
    fraction = counts["pairs"] / float(F * V)
    print("65^3 sphere: %d faces x %d vertices, %d pairs evaluated: %.3f %%" % (F, V, counts["pairs"], 100 * fraction))
    assert 0 < fraction < 0.1
    assert torch.all(done.sqdist == 0.0)
    q = np.random.RandomState(65).uniform(-1.2, 1.2, (512, 3)).astype(np.float32)
    _, counts = _assert_mesh_parity(tris, host, q)
    print("512 queries in the box: %.3f %%" % (100.0 * counts["pairs"] / (512.0 * F)))


def _stats_device(x):
    from zeroshape_amd import _lib
    lib = _lib.load()
    d2 = torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda()
    out = torch.full((4,), -9.0, dtype=torch.float64, device="cuda")
    at = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    _lib.check(lib.zs_mesh_distance_stats(_lib.ptr(d2), len(x), _lib.ptr(out), _lib.ptr(at), _lib.current_stream_ptr(d2.device)),
               "zs_mesh_distance_stats")
    return out.cpu().numpy(), int(at.item())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 34326])
def test_stats_against_the_host(n):
    rng = np.random.RandomState(n)
    d2 = rng.uniform(0, 2, n) ** 2 * 10.0 ** rng.randint(-6, 3, n)
    if n > 1:
        d2[n // 2] = d2[n - 1] = d2.max()                                          # the maximum three times: the lowest index
    for holes in (False, True):
        x = d2.copy()
        if holes and n > 3:
            x[1], x[n - 2], x[n // 3] = np.nan, np.inf, np.nan
            x[::97] = np.inf
        got, at = _stats_device(x)
        want, want_at = E.mesh_distance_stats_host(x)
        assert np.array_equal(bits(got), bits(want)) and at == want_at, (got, want, at, want_at)
        assert got[3] == np.isfinite(x).sum()
    got, at = _stats_device(np.full(300, np.nan))
    assert np.all(np.isnan(got[:3])) and got[3] == 0 and at == -1


@functools.lru_cache(maxsize=None)
def _processed(device):
    """scene25 smoothed 5 passes and simplified at 2 cells, with its source, on the device or the host."""
    tris, host = _case("scene25")
    source = E.SimpleMesh(tris) if device else host
    return E.simplify_mesh(E.smooth_mesh(source, 5), *grid_of("scene25", 2)), source


def test_mesh_deviation_equals_the_host_record():
    got = E.mesh_deviation(*_processed(True), cell_edge=0.12)
    want = E.mesh_deviation(*_processed(False), cell_edge=0.12)
    assert isinstance(got, E.MeshDeviation) and got._fields == want._fields
    for name in got._fields:
        a, b = getattr(got, name), getattr(want, name)
        assert type(a) is type(b) and (np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64) if isinstance(a, float) else a == b), name
    assert 0 < got.forward_mean <= got.forward_rms <= got.forward_max
    assert 0 < got.backward_max and (got.forward_vertices, got.backward_vertices) == (len(_processed(False)[0].vertices), 1160)


def test_two_runs_give_the_same_bytes():
    tris, host = _case("noise23")
    q = torch.from_numpy(np.random.RandomState(2).uniform(-1.7, 1.7, (5000, 3)).astype(np.float32)).cuda()
    a, b = (E.mesh_distance(E.SimpleMesh(tris), q, closest=True) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype != torch.int32 else x, y.view(torch.int32) if y.dtype != torch.int32 else y)
    light, source = _processed(True)
    assert E.mesh_deviation(light, source) == E.mesh_deviation(light, source)


def test_the_results_are_resident_and_the_mesh_keeps_its_weld():
    tris, host = _case("scene25")
    mesh = E.SimpleMesh(tris)
    before = set(vars(mesh))
    q = torch.from_numpy(host.vertices[:100] + np.float32(0.01)).cuda()
    done = mesh.distance_to(q)
    assert isinstance(done, E.MeshDistance) and done.closest is None
    assert done.sqdist.is_cuda and done.face.is_cuda and done.counts.is_cuda and done.counts.dtype == torch.int32
    assert mesh._device_weld is not None and set(vars(mesh)) == before             # the weld it made is kept; nothing else
    assert mesh._triangles is None and mesh._indexed is None and mesh._components is None and mesh._adjacency is None
    weld = mesh._device_weld
    mesh.distance_to(q, closest=True)
    assert mesh._device_weld is weld
    empty = mesh.distance_to(torch.zeros(0, 3, device="cuda"), closest=True)
    assert empty.sqdist.shape == (0,) and empty.closest.shape == (0, 3) and empty.check()["pairs"] == 0
    nothing = E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda")).distance_to(q)
    assert torch.all(nothing.sqdist == float("inf")) and torch.all(nothing.face == -1)
    light, source = _processed(True)
    fresh = E.SimpleMesh(light.device_triangles)
    record = E.mesh_deviation(fresh, source)
    assert fresh._device_weld is not None and not hasattr(fresh, "deviation") and record.cell_edge is None
    with pytest.raises(ValueError, match="both"):
        E.mesh_deviation(fresh, host)


def _opt(tmp_path, **extra):
    return edict(dict(device="cuda", output_path=str(tmp_path), eval=dict(range=[-1.5, 1.5], vox_res=25, num_points=2000, **extra)))


def test_through_the_pipelines(tmp_path):
    vol = torch.from_numpy(volume_of("scene25")).cuda()
    tris, host = _case("scene25")
    edge = 3.0 / 25
    for extra in (dict(simplify_cells=2), dict(smooth_iterations=5), dict(simplify_cells=2, min_component_area=0.1, smooth_iterations=2)):
        filtered = E.filter_components(E.SimpleMesh(tris), extra["min_component_area"], False) if "min_component_area" in extra else E.SimpleMesh(tris)
        plain_m, plain_c = E.convert_to_explicit(_opt(tmp_path, **extra), [vol], 0.5, to_pointcloud=True, seed=3)
        want = E.mesh_deviation(plain_m[0], filtered, cell_edge=edge)              # the filtered mesh and the delivered mesh
        assert not hasattr(plain_m[0], "deviation")
        for meshes, clouds in (E.convert_to_explicit(_opt(tmp_path, mesh_deviation=True, **extra), [vol], 0.5, to_pointcloud=True, seed=3),
                               E._surface_clouds(_opt(tmp_path, mesh_deviation=True, **extra), vol[None], seed=3)):
            assert meshes[0].deviation == want and meshes[0].deviation.cell_edge == edge
            # the flag changes neither the triangles nor the clouds
            assert torch.equal(meshes[0].device_triangles.view(torch.int32), plain_m[0].device_triangles.view(torch.int32))
            cloud = clouds[0].cpu().numpy().astype(np.float64) if isinstance(clouds, torch.Tensor) else clouds[0]
            assert np.array_equal(cloud, plain_c[0])
        report = E.mesh_report(meshes[0])["deviation"]
        assert report["forward_max_cells"] == want.forward_max / edge and report["forward_index"] == want.forward_index
    assert 0 < want.forward_max and want.backward_vertices < 1160                  # against the filtered mesh, not the extracted one
    # without the flag and without any step: today's calls, bit for bit
    direct_tris, direct_pts = E.extract_surface(vol, 0.5, -1.5, 1.5, 2000, 3)
    for extra in (dict(), dict(mesh_deviation=False)):
        m, c = E.convert_to_explicit(_opt(tmp_path, **extra), [vol], 0.5, to_pointcloud=True, seed=3)
        assert m[0]._device_weld is None and not hasattr(m[0], "deviation")
        assert torch.equal(m[0].device_triangles.view(torch.int32), direct_tris.view(torch.int32))
        assert np.array_equal(c[0], direct_pts.cpu().numpy().astype(np.float64))
        m2, c2 = E._surface_clouds(_opt(tmp_path, **extra), vol[None], seed=3)
        assert torch.equal(m2[0].device_triangles.view(torch.int32), direct_tris.view(torch.int32))
        assert torch.equal(c2[0].view(torch.int32), direct_pts.view(torch.int32))
    with pytest.raises(ValueError, match="mesh_deviation needs"):
        E.convert_to_explicit(_opt(tmp_path, mesh_deviation=True), [vol], 0.5)
    with pytest.raises(ValueError, match="mesh_deviation needs"):
        E._surface_clouds(_opt(tmp_path, mesh_deviation=True, min_component_area=0.1), vol[None])


def test_demo_script_writes_the_deviation(tmp_path, encoder_sd, seeded_sd):
    import subprocess
    import sys
    from PIL import Image
    from zeroshape_amd.data.synthetic import Dataset
    from zeroshape_amd.utils import options
    opt = options.set(options.parse_arguments(["--yaml=%s/options/shape.yaml" % ROOT, "--output_root=%s" % tmp_path]),
                      need_gpu=False)
    item = Dataset(opt, n_items=1)[0]
    os.makedirs(tmp_path / "data" / "images")
    os.makedirs(tmp_path / "data" / "masks")
    rgb = (item["rgb_input_map"].numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
    Image.fromarray(rgb).save(tmp_path / "data" / "images" / "blob.png")
    Image.fromarray((item["mask_input_map"][0].numpy() * 255).astype(np.uint8)).save(tmp_path / "data" / "masks" / "blob.png")
    full = dict(encoder_sd)
    full.update({"impl_network." + k: v for k, v in seeded_sd.items()})
    # the seeded decoder's 0.5 level set is empty on this image: the last bias is moved so that the level lies inside the
    # logits' range (as the colour tests' demo run does, for the reasons given there)
    full["impl_network.impl_mlp.layers.8.bias"] = full["impl_network.impl_mlp.layers.8.bias"] + 0.26
    torch.save(dict(epoch=0, iter=0, best_val=1.0, best_ep=0, graph=full), tmp_path / "shape.ckpt")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0", ZS_SYNTHETIC_ITEMS="4", ZS_SYNTHETIC_STANDIN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--yaml=options/shape.yaml", "--task=shape",
                        "--datadir=%s/data" % tmp_path, "--eval.vox_res=32", "--ckpt=%s/shape.ckpt" % tmp_path,
                        "--output_root=%s" % tmp_path, "--eval.simplify_cells=2.0", "--eval.mesh_deviation=true",
                        "--eval.mesh_report=true"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    report = json.load(open(tmp_path / "data" / "preds" / "blob_mesh_report.json"))
    record = report["deviation"]
    print("demo.py: deviation", record)
    assert 0.0 < record["forward_max_cells"] < 1.5 * np.sqrt(3)
    assert record["forward_max_cells"] == record["forward_max"] / record["cell_edge"] and record["cell_edge"] > 0
    assert record["forward_vertices"] > 0 and record["backward_vertices"] > record["forward_vertices"] and "simplification" in report
