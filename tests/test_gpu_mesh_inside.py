"""GPU: the point-in-mesh kernels (csrc/mesh_inside.hip) against their checker eval_3D.mesh_winding_host and, without the
checker, against the occupancy of the grid a marching-cubes mesh was made from.  Every comparison is integer equality: the
crossing numbers of both rays and the counts - on marching-cubes meshes with lattice, on-surface, random and far queries, on
query and face counts around the workgroup size and the scan tile, on flat meshes, one column, one huge face, degenerate,
duplicated and invalid faces; the grid entry against the point entry; zs_occupancy_counts against numpy; the raw entry points'
argument checks; determinism; residency; mesh_signed_distance and mesh_volume_iou against the host; the opt-in through
convert_to_explicit, _surface_clouds and demo.py.

The checker tests every (point, face) box in numpy (about 10^8 pairs a second): where faces x queries would exceed PAIRS the
queries are an evenly strided subset."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.test_mesh_components_host_logic import volume_of
from tests.test_mesh_simplify_host_logic import grid_of
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_CASES = ["sphere17", "sphere17_clipped", "scene25", "noise9", "noise23", "three_valued"]
# (grid, zero-padded by one voxel): below the iso value on the border, so the marching-cubes mesh is closed
CLOSED_GRIDS = [("sphere17", False), ("scene25", False), ("sphere17_clipped", True), ("noise9", True), ("noise15", True),
                ("noise23", True), ("three_valued", True)]
PAIRS = 1 << 27


@functools.lru_cache(maxsize=None)
def _case(name, padded=False):
    """(the level grid, the soup on the GPU, the numpy-welded host mesh of its host copy) - computed once, read by all."""
    vol = volume_of(name)
    if padded:
        vol = np.pad(vol, 1)
    tris, _ = E.extract_surface(torch.from_numpy(vol).cuda(), 0.5, -1.5, 1.5)
    return vol, tris, E.SimpleMesh(tris.cpu().numpy())


def _strided(n, faces):
    keep = max(1, min(n, PAIRS // max(faces, 1)))
    return np.unique(np.linspace(0, n - 1, keep).astype(np.int64)) if n else np.zeros(0, np.int64)


def _buffers(vertices, faces):
    v = torch.tensor(np.asarray(vertices, np.float32), device="cuda").reshape(-1, 3).contiguous()
    f = torch.tensor(np.asarray(faces, np.int32), device="cuda").reshape(-1, 3).contiguous()
    return v, f


def _raw(vertices, faces, queries, with_down=True):
    """zs_mesh_winding on buffers of the right sizes -> (return code, out_counts, up, down)."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    v, f = _buffers(vertices, faces)
    q = torch.tensor(np.asarray(queries, np.float32), device="cuda").reshape(-1, 3).contiguous()
    n, n_verts, m = f.shape[0], v.shape[0], q.shape[0]
    up = torch.full((m,), -9, dtype=torch.int32, device="cuda")
    down = torch.full((m,), -9, dtype=torch.int32, device="cuda") if with_down else None
    counts = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.zs_mesh_winding_scratch_bytes(n, m)
    assert nbytes > 0 and nbytes % 256 == 0
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    rc = lib.zs_mesh_winding(_lib.ptr(v), _lib.ptr(f), n, n_verts, _lib.ptr(q), m, _lib.ptr(up), _lib.ptr(down), _lib.ptr(counts),
                             _lib.ptr(scratch), _lib.current_stream_ptr(v.device))
    torch.cuda.synchronize()
    return rc, counts.tolist(), up.cpu().numpy(), None if down is None else down.cpu().numpy()


def _raw_grid(vertices, faces, G, scale, offset):
    """zs_mesh_winding_grid -> (return code, out_counts [6], inside [G^3] int8)."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    v, f = _buffers(vertices, faces)
    n, n_verts = f.shape[0], v.shape[0]
    inside = torch.full((G ** 3,), -9, dtype=torch.int8, device="cuda")
    counts = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.zs_mesh_winding_scratch_bytes(n, G ** 3)
    assert nbytes > 0 and nbytes % 256 == 0
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    rc = lib.zs_mesh_winding_grid(_lib.ptr(v), _lib.ptr(f), n, n_verts, G, float(np.float32(scale)), float(np.float32(offset)),
                                  _lib.ptr(inside), _lib.ptr(counts), _lib.ptr(scratch), _lib.current_stream_ptr(v.device))
    torch.cuda.synchronize()
    return rc, counts.tolist(), inside.cpu().numpy()


def _pairs(counts):
    return (counts[3] & 0xffffffff) | ((counts[4] & 0xffffffff) << 32)


def _assert_raw_parity(vertices, faces, queries):
    """The raw entry point against the checker on one indexed mesh -> (counts, up, down)."""
    queries = np.asarray(queries, np.float32).reshape(-1, 3)
    rc, counts, up, down = _raw(vertices, faces, queries)
    want_up, want_down, want_counts = E.mesh_winding_host(queries, vertices, faces)
    assert rc == 1 and counts[:3] == want_counts[:3].tolist()
    assert np.array_equal(up, want_up), np.flatnonzero(up != want_up)[:8]
    assert np.array_equal(down, want_down), np.flatnonzero(down != want_down)[:8]
    assert _pairs(counts) <= _pairs(want_counts.tolist())            # the columns read no pair twice
    return counts, up, down


def _lattice(G):
    return E._lattice_host(G, np.float32(3.0 / G), np.float32(-1.5))


@pytest.mark.parametrize("name", PARITY_CASES)
def test_against_the_checker(name):
    """Lattice points (rays along lattice lines, through vertices and along edges), vertices and face centroids (on the
    surface), random points in and around the box (queries outside it on every side) - through mesh_winding on a GPU mesh."""
    vol, tris, host = _case(name)
    rng = np.random.RandomState(len(name))
    lo, hi = host.vertices.min(axis=0).astype(np.float64), host.vertices.max(axis=0).astype(np.float64)
    around = (0.5 * (lo + hi) + rng.uniform(-1.5, 1.5, (2000, 3)) * 0.5 * (hi - lo)).astype(np.float32)
    for a in range(3):
        assert (around[:, a] < lo[a]).any() and (around[:, a] > hi[a]).any()
    q = np.concatenate([_lattice(vol.shape[0]), host.vertices, host.triangles.mean(axis=1), around]).astype(np.float32)
    q = q[_strided(len(q), len(host.faces))]
    done = E.mesh_winding(E.SimpleMesh(tris), torch.from_numpy(q).cuda())
    assert done.up.is_cuda and done.up.dtype == torch.int32 and done.down.dtype == torch.int32 and done.up.shape == (len(q),)
    want_up, want_down, _ = E.mesh_winding_host(q, host.vertices, host.faces)
    assert np.array_equal(done.up.cpu().numpy(), want_up) and np.array_equal(done.down.cpu().numpy(), want_down)
    assert (want_up != 0).any() and (want_up != want_down).any()
    counts = done.check()
    assert counts["skipped_faces"] == 0 and counts["status"] == 0 and 0 < counts["pairs"] < len(q) * len(host.faces)


@pytest.mark.parametrize("name,padded", CLOSED_GRIDS)
def test_the_grid_entry_against_occupancy(name, padded):
    """Without the checker: on the closed marching-cubes mesh of a grid the winding number at every lattice point is that
    point's occupancy, and no point is ambiguous."""
    vol, tris, host = _case(name, padded)
    G = vol.shape[0]
    inside, counts = E.mesh_occupancy_grid(E.SimpleMesh(tris), G, np.float32(3.0 / G), -1.5)
    assert inside.is_cuda and inside.dtype == torch.int8 and inside.shape == (G, G, G) and counts.shape == (6,)
    inside, counts = inside.cpu().numpy(), counts.tolist()
    assert set(np.unique(inside).tolist()) <= {0, 1} and counts[:3] == [0, 0, 0] and 0 < _pairs(counts) < G ** 3 * len(host.faces)
    occupied = vol >= 0.5
    if name == "three_valued":
        keep = vol != 0.5                                            # the points whose level is the iso value lie on the surface
        assert np.array_equal(inside[keep] != 0, occupied[keep]) and keep.sum() == G ** 3 - 254
    else:
        assert np.array_equal(inside != 0, occupied) and counts[5] == 0
    assert occupied.any()


@pytest.mark.parametrize("name,padded,G,scale,offset", [
    ("scene25", False, 25, 3.0 / 25, -1.5), ("scene25", False, 33, 0.11, -1.9), ("noise9", False, 9, 3.0 / 9, -1.5),
    ("three_valued", True, 11, 3.0 / 11, -1.5), ("sphere17", False, 20, 0.05, -0.3)])
def test_the_grid_entry_equals_the_point_entry(name, padded, G, scale, offset):
    """The same lattice made in the kernel and uploaded; a lattice larger than and shifted against the mesh, one inside it."""
    _, _, host = _case(name, padded)
    rc, counts, inside = _raw_grid(host.vertices, host.faces, G, scale, offset)
    q = E._lattice_host(G, np.float32(scale), np.float32(offset))
    rc2, counts2, up, down = _raw(host.vertices, host.faces, q)
    assert rc == 1 and rc2 == 1 and np.array_equal(inside, (up != 0).astype(np.int8))
    assert counts[:5] == counts2 and counts[5] == (up != down).sum()
    if name == "noise9":
        assert counts[5] > 0                                         # open at the border


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 255, 256, 257, 2049])
def test_query_counts(m):
    _, tris, host = _case("scene25")
    q = np.random.RandomState(m).uniform(-1.6, 1.6, (m, 3)).astype(np.float32)
    q[::3] = host.vertices[(np.arange(len(q[::3])) * 7) % len(host.vertices)]       # some on the surface
    if m == 0:
        rc, counts, up, down = _raw(host.vertices, host.faces, q)
        assert rc == 1 and counts == [-1] * 5 and up.shape == (0,)   # touches nothing
        return
    _assert_raw_parity(host.vertices, host.faces, q)


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
    q = np.concatenate([rng.uniform(-0.5, 1.5, (600, 3)) * [n_faces / 2.0 + 1, 1, 1], verts[:: max(1, len(verts) // 200)],
                        0.5 * (verts[:-1] + verts[1:])[:: max(1, len(verts) // 100)]]).astype(np.float32)
    counts, up, down = _assert_raw_parity(verts, faces, q)
    assert counts[:3] == [0, 0, 0] and (up.any() or down.any()) and 0 < _pairs(counts) <= n_faces * len(q)


@pytest.mark.parametrize("G", [1, 2, 33])
def test_grid_sizes(G):
    _, _, host = _case("sphere17")
    scale, offset = (0.0, 0.1) if G == 1 else (1.3, -0.2) if G == 2 else (2.4 / (G - 1), -1.2)
    rc, counts, inside = _raw_grid(host.vertices, host.faces, G, scale, offset)
    up, down, want = E.mesh_winding_host(E._lattice_host(G, np.float32(scale), np.float32(offset)), host.vertices, host.faces)
    assert rc == 1 and np.array_equal(inside, (up != 0).astype(np.int8)) and counts[:3] == [0, 0, 0] and counts[5] == (up != down).sum()
    assert inside.any() and (G == 1 or not inside.all())


def test_a_single_column():
    """Fewer than eight faces make one column: every pair is read."""
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    q = np.random.RandomState(5).uniform(-0.5, 1.2, (300, 3)).astype(np.float32)
    counts, up, down = _assert_raw_parity(tet, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], q)
    assert _pairs(counts) == 4 * 300 and (up == 1).any() and np.array_equal(up, down)
    # 400 triangles whose boxes share one centre fall into one column of many
    rng = np.random.RandomState(6)
    a = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    b = a * rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    verts = np.stack([a, b, -a], axis=1).reshape(-1, 3)
    _assert_raw_parity(verts, np.arange(1200).reshape(400, 3), q)


def _sheet(n=24, step=0.25):
    g = np.arange(n)
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * np.float32(step)
    quad = np.array([[i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1] for i in range(n - 1) for j in range(n - 1)])
    return grid, np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]])


def test_an_axis_without_extent():
    """The vertical plane (x = const, then y = const: one column along that axis; all faces project to segments, the winding
    is 0 everywhere, also in the plane) and the horizontal sheet (no extent in z, which the columns do not see)."""
    grid, faces = _sheet()
    rng = np.random.RandomState(4)
    q = rng.uniform(-2, 8, (600, 3)).astype(np.float32)
    for axis in range(3):
        verts = np.insert(grid, axis, np.float32(1.5), axis=1)
        here = np.concatenate([q, verts[::5], verts[faces].mean(axis=1)[::7]]).astype(np.float32)
        here[:150, axis] = 1.5                                       # in the plane
        counts, up, down = _assert_raw_parity(verts, faces, here)
        assert 0 < _pairs(counts) < len(faces) * len(here)           # the columns still prune
        assert (not up.any() and not down.any()) if axis < 2 else (up.any() and down.any() and not np.array_equal(up, down))
    line = np.stack([np.arange(40) * 0.1, np.full(40, 2.0), np.full(40, -1.0)], axis=1).astype(np.float32)
    _, up, down = _assert_raw_parity(line, np.stack([np.arange(38), np.arange(38) + 1, np.arange(38) + 2], axis=1), q)
    assert not up.any() and not down.any()


def test_one_face_that_spans_the_box_among_2000_small_ones():
    """The reaches of the huge face are half the grid each way: a query reads the columns within half the box of its own -
    all of them from the middle of the box, a quarter from a corner - slow, still the checker's numbers; without the huge
    face the columns prune."""
    rng = np.random.RandomState(7)
    centres = rng.uniform(-1, 1, (2000, 1, 3))
    small = (centres + rng.uniform(-0.02, 0.02, (2000, 3, 3))).astype(np.float32)
    huge = np.array([[[-1.2, -1.2, -1.2], [1.2, -1.2, -1.1], [0.1, 1.2, 1.2]]], np.float32)
    q = np.concatenate([rng.uniform(-1.5, 1.5, (600, 3)), small.mean(axis=1)[::10] - [0, 0, 0.5]]).astype(np.float32)
    middle = (rng.uniform(-1, 1, (300, 3)) * [0.15, 0.15, 1.5]).astype(np.float32)          # within 0.15 of the box's centre in x, y
    without, up0, _ = _assert_raw_parity(small.reshape(-1, 3), np.arange(6000).reshape(-1, 3), q)
    assert _pairs(without) < 0.02 * 2000 * len(q)
    middle_without = _pairs(_raw(small.reshape(-1, 3), np.arange(6000).reshape(-1, 3), middle)[1])
    for soup in (np.concatenate([small[:1000], huge, small[1000:]]), np.concatenate([huge, small])):
        verts = soup.reshape(-1, 3)
        faces = np.arange(len(verts)).reshape(-1, 3)
        counts, up, down = _assert_raw_parity(verts, faces, q)
        assert (up != up0).any() and up0.any()                       # the huge face is crossed, and so are small ones
        middle_with, _, _ = _assert_raw_parity(verts, faces, middle)
        print("pairs read from the middle: %d with the huge face, %d without, of %d; from everywhere: %d and %d of %d" % (
            _pairs(middle_with), middle_without, 2001 * len(middle), _pairs(counts), _pairs(without), 2001 * len(q)))
        assert _pairs(middle_with) >= 0.99 * 2001 * len(middle) and middle_without < 0.02 * 2000 * len(middle)
        assert _pairs(counts) > 0.25 * 2001 * np.all(np.abs(q[:, :2]) <= 1.2, axis=1).sum() * 0.9


def test_degenerate_and_duplicated_faces_on_the_device():
    _, _, host = _case("sphere17")
    verts = np.concatenate([host.vertices, [[3, 3, 3], [3, 3, 3], [2, 2, 2]]]).astype(np.float32)
    V = len(host.vertices)
    extra = [[0, 0, 5], [7, 9, 9], [V, V, V], [V, V + 1, V], [V, V + 2, V + 1], [3, 3, 3]] + host.faces[:40].tolist() + host.faces[10:20, [1, 2, 0]].tolist()
    faces = np.concatenate([host.faces[:300], extra, host.faces[300:], host.faces[:5]])
    rng = np.random.RandomState(8)
    q = np.concatenate([rng.uniform(-1, 1, (600, 3)), verts[::3], [[2.5, 2.5, 2.5], [3, 3, 3], [4, 4, 4]]]).astype(np.float32)
    counts, up, down = _assert_raw_parity(verts, faces, q)
    assert counts[:3] == [0, 0, 0] and up.any()
    _, up, down = _assert_raw_parity(verts, np.array(extra[:6]), q)  # only degenerate faces
    assert not up.any() and not down.any()


def test_skipped_faces_queries_that_are_not_finite_and_a_null_out_down():
    _, _, host = _case("scene25")
    verts, faces = host.vertices.copy(), host.faces.copy()
    verts[7, 1], verts[11, 0], verts[500, 2] = np.nan, np.inf, -np.inf
    faces[3, 2], faces[9, 0], faces[2000, 1] = len(verts), -1, 2 ** 31 - 1
    bad = np.isin(faces, [7, 11, 500]).any(axis=1)
    bad[[3, 9, 2000]] = True
    q = np.random.RandomState(9).uniform(-1.6, 1.6, (500, 3)).astype(np.float32)
    q[5, 0], q[9, 2], q[20, 1], q[499] = np.nan, np.inf, -np.inf, np.nan
    rows = [5, 9, 20, 499]
    counts, up, down = _assert_raw_parity(verts, faces, q)
    assert counts[:3] == [int(bad.sum()), 4, 1 | 2 | 4] and not up[rows].any() and not down[rows].any() and up.any()
    # the valid faces alone give the same numbers: a skipped face is not read through
    rest = np.setdiff1d(np.arange(500), rows)
    want = E.mesh_winding_host(q[rest], np.nan_to_num(verts, posinf=0.0, neginf=0.0), faces[~bad])
    assert np.array_equal(up[rest], want[0]) and np.array_equal(down[rest], want[1])
    # one kind at a time: the status bits
    only = host.faces.copy()
    only[3, 2] = len(verts)
    assert _raw(host.vertices, only, q[rest])[1][:3] == [1, 0, 2]
    assert _raw(verts, host.faces, q[rest])[1][:3] == [int(np.isin(host.faces, [7, 11, 500]).any(axis=1).sum()), 0, 1]
    # without out_down
    rc, counts1, up1, none = _raw(verts, faces, q, with_down=False)
    assert rc == 1 and none is None and np.array_equal(up1, up) and counts1 == counts
    # no valid face at all, no vertices, no faces
    for v, f in ((verts[:3] * np.nan, [[0, 1, 2]]), (np.zeros((0, 3)), [[0, 1, 2]]), (verts, np.zeros((0, 3)))):
        rc, counts, up, down = _raw(v, f, q)
        assert rc == 1 and counts == [len(f), 4, (4 | (2 if len(v) == 0 else 1)) if len(f) else 4, 0, 0]
        assert not up.any() and not down.any()
        rc, counts, inside = _raw_grid(v, f, 5, 0.5, -1.0)
        assert rc == 1 and counts == [len(f), 0, ((2 if len(v) == 0 else 1)) if len(f) else 0, 0, 0, 0] and not inside.any()
    # a lattice that is not finite
    rc, counts, inside = _raw_grid(host.vertices, host.faces, 3, np.inf, 0.0)
    assert rc == 1 and counts[1] == 27 and counts[2] == 4 and not inside.any()
    # through mesh_winding: the face-index bit raises where the counts are read
    from zeroshape_amd import _lib
    mesh = E.SimpleMesh(torch.zeros(len(only), 3, 3, device="cuda"))
    mesh._device_weld = (torch.from_numpy(host.vertices).cuda(), torch.from_numpy(only.astype(np.int32)).cuda(), None)
    done = E.mesh_winding(mesh, torch.from_numpy(q).cuda())
    with pytest.raises(_lib.ZeroShapeHipError, match="status 6"):
        done.check()
    with pytest.raises(_lib.ZeroShapeHipError, match="face index"):
        E.mesh_volume_iou(mesh, E.SimpleMesh(_case("scene25")[1]), 9, 3.0 / 9, -1.5)
    for points in (q, torch.from_numpy(q)):
        with pytest.raises(ValueError, match="CUDA"):
            E.mesh_winding(mesh, points)
        with pytest.raises(ValueError, match="CUDA"):
            mesh.contains(points)


def test_argument_checks_of_the_raw_entry_points():
    """0 and a message that names the entry point, before anything is launched (a host buffer stands in for every non-null
    pointer: nothing may read it); zero queries return 1."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p, odd = ctypes.c_void_p(base + (-base) % 8), ctypes.c_void_p(base + (-base) % 8 + 4)

    def fails(rc, what, who):
        msg = lib.zs_last_error()
        assert rc == 0 and msg.startswith(who) and what.encode() in msg, (what, rc, msg)

    def call(n=1, v=3, m=1, ptr=p, scratch=p, **null):
        args = dict(vertices=ptr, faces=ptr, queries=ptr, out_up=ptr, out_down=ptr, out_counts=ptr)
        args.update(null)
        return lib.zs_mesh_winding(args["vertices"], args["faces"], n, v, args["queries"], m, args["out_up"], args["out_down"],
                                   args["out_counts"], scratch, None)

    who = b"zs_mesh_winding: "
    fails(call(n=-1), "negative size", who)
    fails(call(v=-3), "negative size", who)
    fails(call(m=-1), "negative size", who)
    fails(call(n=2 ** 24 + 1), "too large", who)
    fails(call(m=2 ** 28 + 1), "too large", who)
    for name in ("vertices", "faces", "queries", "out_up", "out_counts"):
        fails(call(**{name: None}), "null pointer", who)
    fails(call(scratch=None), "null pointer", who)
    fails(call(scratch=odd), "8-byte aligned", who)
    fails(call(scratch=odd, out_down=None), "8-byte aligned", who)   # out_down may be null: the next check speaks
    assert call(m=0, ptr=None, scratch=None) == 1 and call(n=0, v=0, m=0, ptr=None, scratch=None) == 1

    def grid(n=1, v=3, G=2, ptr=p, scratch=p, **null):
        args = dict(vertices=ptr, faces=ptr, out_inside=ptr, out_counts=ptr)
        args.update(null)
        return lib.zs_mesh_winding_grid(args["vertices"], args["faces"], n, v, G, 1.0, 0.0, args["out_inside"], args["out_counts"],
                                        scratch, None)

    who = b"zs_mesh_winding_grid: "
    fails(grid(n=-1), "negative size", who)
    fails(grid(v=-1), "negative size", who)
    fails(grid(G=-1), "negative size", who)
    fails(grid(n=2 ** 24 + 1), "too large", who)
    fails(grid(G=646), "too large", who)
    for name in ("vertices", "faces", "out_inside", "out_counts"):
        fails(grid(**{name: None}), "null pointer", who)
    fails(grid(scratch=None), "null pointer", who)
    fails(grid(scratch=odd), "8-byte aligned", who)
    assert grid(G=0, ptr=None, scratch=None) == 1
    size = lib.zs_mesh_winding_scratch_bytes
    assert size(-1, 1) == 0 and size(1, -1) == 0 and size(2 ** 24 + 1, 1) == 0 and size(1, 2 ** 28 + 1) == 0
    for n, m in ((0, 0), (0, 5), (1, 1), (17, 3), (2 ** 24, 2 ** 28), (100, 645 ** 3)):
        assert size(n, m) > 0 and size(n, m) % 256 == 0
    assert size(2 ** 24, 1) > size(2 ** 20, 1) > size(1, 1) and size(100, 646 ** 3) == 0
    who = b"zs_occupancy_counts: "
    occ = lib.zs_occupancy_counts
    fails(occ(p, p, -1, p, None), "negative size", who)
    fails(occ(p, p, 2 ** 40 + 1, p, None), "too large", who)
    for args in ((None, p, 1, p), (p, None, 1, p), (p, p, 1, None), (None, None, 0, None)):
        fails(occ(*args, None), "null pointer", who)
    fails(occ(p, p, 1, odd, None), "8-byte aligned", who)


@pytest.mark.parametrize("n", [0, 1, 63, 257, 100003, 129 ** 3])
def test_occupancy_counts(n):
    from zeroshape_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(n)
    a, b = (rng.randint(-1, 2, n) * (rng.uniform(0, 1, n) < 0.6)).astype(np.int8), rng.choice([0, 1, 1, -128, 127], n).astype(np.int8)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.zs_occupancy_counts(_lib.ptr(da), _lib.ptr(db), n, _lib.ptr(out), _lib.current_stream_ptr(out.device)),
               "zs_occupancy_counts")
    x, y = a != 0, b != 0
    assert out.tolist() == [int(x.sum()), int(y.sum()), int((x & y).sum()), int((x | y).sum())]


def test_pruning_is_real():
    """The padded noise23 mesh (about 40k faces) on its own lattice: a small fraction of faces x points is read."""
    vol, tris, host = _case("noise23", True)
    G, F = vol.shape[0], len(host.faces)
    inside, counts = E.mesh_occupancy_grid(E.SimpleMesh(tris), G, np.float32(3.0 / G), -1.5)
    fraction = _pairs(counts.tolist()) / float(F * G ** 3)
    print("noise23 padded: %d faces x %d points, %.4f %% of the pairs read" % (F, G ** 3, 100 * fraction))
    assert 0 < fraction < 0.01


def test_two_runs_give_the_same_bytes():
    _, tris, host = _case("noise23")
    q = torch.from_numpy(np.random.RandomState(2).uniform(-1.7, 1.7, (5000, 3)).astype(np.float32)).cuda()
    a, b = (E.mesh_winding(E.SimpleMesh(tris), q) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    a, b = (E.mesh_occupancy_grid(E.SimpleMesh(tris), 33, 0.1, -1.6) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_signed_distance_and_contains_on_the_device():
    vol, tris, host = _case("scene25")
    q = np.concatenate([_lattice(25)[::9], np.random.RandomState(3).uniform(-1.6, 1.6, (500, 3)), [[np.nan, 0, 0]]]).astype(np.float32)
    mesh = E.SimpleMesh(tris)
    dq = torch.from_numpy(q).cuda()
    signed, closest = mesh.signed_distance_to(dq, closest=True)
    assert signed.is_cuda and signed.dtype == torch.float64 and closest.is_cuda and closest.shape == (len(q), 3)
    want, want_closest = E.mesh_signed_distance(host, q, closest=True)
    assert np.array_equal(signed.cpu().numpy()[:-1].view(np.uint64), want[:-1].view(np.uint64))
    assert np.array_equal(closest.cpu().numpy()[:-1].view(np.uint64), want_closest[:-1].view(np.uint64))
    assert np.isnan(want[-1]) and bool(torch.isnan(signed[-1])) and np.all(np.isfinite(want[:-1]))     # the point that is not finite
    assert (want < 0).any() and (want > 0).any()
    got = mesh.contains(dq)
    assert got.is_cuda and got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), host.contains(q))
    assert np.array_equal(got.cpu().numpy()[:len(_lattice(25)[::9])], (vol >= 0.5).reshape(-1)[::9])
    nothing = E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda"))
    assert torch.all(nothing.signed_distance_to(dq[:-1]) == float("inf")) and not nothing.contains(dq).any()


@functools.lru_cache(maxsize=None)
def _processed(device, how):
    """scene25 smoothed 5 passes or simplified at 2 cells, with its source, on the device or the host."""
    _, tris, host = _case("scene25")
    source = E.SimpleMesh(tris) if device else host
    return (E.smooth_mesh(source, 5) if how == "smoothed" else E.simplify_mesh(source, *grid_of("scene25", 2))), source


@pytest.mark.parametrize("how", ["smoothed", "simplified"])
def test_mesh_volume_iou_equals_the_host_record(how):
    lattice = (25, np.float32(3.0 / 25), -1.5)
    got = E.mesh_volume_iou(*_processed(True, how), *lattice)
    want = E.mesh_volume_iou(*_processed(False, how), *lattice)
    assert isinstance(got, E.MeshVolumeIoU) and got._fields == want._fields
    for name in got._fields:
        a, b = getattr(got, name), getattr(want, name)
        assert type(a) is type(b) and a == b, name
    assert 0.5 < got.iou < 1.0 and got.inside_reference == (volume_of("scene25") >= 0.5).sum() and got.ambiguous_reference == 0
    assert got.both <= min(got.inside, got.inside_reference) <= got.either
    with pytest.raises(ValueError, match="both"):
        E.mesh_volume_iou(_processed(True, how)[0], _processed(False, how)[1], *lattice)


def test_the_results_are_resident_and_the_mesh_keeps_its_weld():
    _, tris, host = _case("scene25")
    mesh = E.SimpleMesh(tris)
    before = set(vars(mesh))
    q = torch.from_numpy(host.vertices[:100] + np.float32(0.01)).cuda()
    done = E.mesh_winding(mesh, q)
    assert isinstance(done, E.MeshWinding) and done.up.is_cuda and done.down.is_cuda and done.counts.is_cuda
    assert done.counts.dtype == torch.int32 and done.counts.shape == (5,)
    assert mesh._device_weld is not None and set(vars(mesh)) == before             # the weld it made is kept; nothing else
    assert mesh._triangles is None and mesh._indexed is None and mesh._components is None and mesh._adjacency is None
    weld = mesh._device_weld
    mesh.contains(q)
    mesh.signed_distance_to(q)
    inside, counts = E.mesh_occupancy_grid(mesh, 9, 3.0 / 9, -1.5)
    assert mesh._device_weld is weld and inside.is_cuda and counts.is_cuda
    assert mesh._triangles is None and mesh._indexed is None
    empty = E.mesh_winding(mesh, torch.zeros(0, 3, device="cuda"))
    assert empty.up.shape == (0,) and empty.down.shape == (0,) and empty.check()["pairs"] == 0
    assert E.mesh_occupancy_grid(mesh, 0, 1.0, 0.0)[0].shape == (0, 0, 0)
    fresh, source = E.SimpleMesh(_processed(True, "simplified")[0].device_triangles), E.SimpleMesh(tris)
    record = E.mesh_volume_iou(fresh, source, 25, np.float32(3.0 / 25), -1.5)
    assert fresh._device_weld is not None and source._device_weld is not None and not hasattr(fresh, "volume_iou")
    assert fresh._triangles is None and source._triangles is None and record.either > 0


def _opt(tmp_path, **extra):
    return edict(dict(device="cuda", output_path=str(tmp_path), eval=dict(range=[-1.5, 1.5], vox_res=25, num_points=2000, **extra)))


def test_through_the_pipelines(tmp_path):
    vol = torch.from_numpy(volume_of("scene25")).cuda()
    _, tris, host = _case("scene25")
    lattice = (25, float(np.float32(3.0 / 25)), -1.5)
    for extra in (dict(simplify_cells=2), dict(smooth_iterations=5), dict(simplify_cells=2, min_component_area=0.1, smooth_iterations=2)):
        filtered = E.filter_components(E.SimpleMesh(tris), extra["min_component_area"], False) if "min_component_area" in extra else E.SimpleMesh(tris)
        plain_m, plain_c = E.convert_to_explicit(_opt(tmp_path, **extra), [vol], 0.5, to_pointcloud=True, seed=3)
        want = E.mesh_volume_iou(plain_m[0], filtered, *lattice)                   # the filtered mesh and the delivered mesh
        assert not hasattr(plain_m[0], "volume_iou")
        for meshes, clouds in (E.convert_to_explicit(_opt(tmp_path, mesh_iou=True, **extra), [vol], 0.5, to_pointcloud=True, seed=3),
                               E._surface_clouds(_opt(tmp_path, mesh_iou=True, **extra), vol[None], seed=3)):
            assert meshes[0].volume_iou == want and not hasattr(meshes[0], "deviation")
            # the flag changes neither the triangles nor the clouds
            assert torch.equal(meshes[0].device_triangles.view(torch.int32), plain_m[0].device_triangles.view(torch.int32))
            cloud = clouds[0].cpu().numpy().astype(np.float64) if isinstance(clouds, torch.Tensor) else clouds[0]
            assert np.array_equal(cloud, plain_c[0])
        assert E.mesh_report(meshes[0])["volume_iou"] == want._asdict()
    assert 0.5 < want.iou < 1.0 and want.inside_reference < (volume_of("scene25") >= 0.5).sum()       # against the filtered mesh
    # without the flag and without any step: the parent's calls, bit for bit
    direct_tris, direct_pts = E.extract_surface(vol, 0.5, -1.5, 1.5, 2000, 3)
    for extra in (dict(), dict(mesh_iou=False)):
        m, c = E.convert_to_explicit(_opt(tmp_path, **extra), [vol], 0.5, to_pointcloud=True, seed=3)
        assert m[0]._device_weld is None and not hasattr(m[0], "volume_iou")
        assert torch.equal(m[0].device_triangles.view(torch.int32), direct_tris.view(torch.int32))
        assert np.array_equal(c[0], direct_pts.cpu().numpy().astype(np.float64))
        m2, c2 = E._surface_clouds(_opt(tmp_path, **extra), vol[None], seed=3)
        assert torch.equal(m2[0].device_triangles.view(torch.int32), direct_tris.view(torch.int32))
        assert torch.equal(c2[0].view(torch.int32), direct_pts.view(torch.int32))
    with pytest.raises(ValueError, match="mesh_iou needs"):
        E.convert_to_explicit(_opt(tmp_path, mesh_iou=True), [vol], 0.5)
    with pytest.raises(ValueError, match="mesh_iou needs"):
        E._surface_clouds(_opt(tmp_path, mesh_iou=True, min_component_area=0.1), vol[None])


def test_demo_script_writes_the_volume_iou(tmp_path, encoder_sd, seeded_sd):
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
    # logits' range (as the distance tests' demo run does)
    full["impl_network.impl_mlp.layers.8.bias"] = full["impl_network.impl_mlp.layers.8.bias"] + 0.26
    torch.save(dict(epoch=0, iter=0, best_val=1.0, best_ep=0, graph=full), tmp_path / "shape.ckpt")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0", ZS_SYNTHETIC_ITEMS="4", ZS_SYNTHETIC_STANDIN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--yaml=options/shape.yaml", "--task=shape",
                        "--datadir=%s/data" % tmp_path, "--eval.vox_res=32", "--ckpt=%s/shape.ckpt" % tmp_path,
                        "--output_root=%s" % tmp_path, "--eval.simplify_cells=2.0", "--eval.mesh_iou=true",
                        "--eval.mesh_report=true"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    report = json.load(open(tmp_path / "data" / "preds" / "blob_mesh_report.json"))
    record = report["volume_iou"]
    print("demo.py: volume_iou", record)
    assert set(record) == set(E.MeshVolumeIoU._fields) and "deviation" not in report and "simplification" in report
    assert 0 < record["both"] <= min(record["inside"], record["inside_reference"]) <= record["either"] <= 33 ** 3
    assert record["iou"] == record["both"] / record["either"] and record["cell_volume"] > 0
