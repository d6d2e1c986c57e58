"""GPU: the ray casting kernels (csrc/mesh_rays.hip) against their checker eval_3D.mesh_rays_host and, without the checker,
against the two independent oracles of tests/test_mesh_rays_host_logic.py and a round trip through the depth map.  Every
comparison with the checker is equality of bits (t, the weights) and of integers (face, side, the first three counts), with
the pairs read never above the brute force's: on marching-cubes meshes with lattice-line, random, axis-parallel, vertex and
centroid rays, on ray and face counts around the workgroup size and the scan tile, a single cell, a flat sheet, one huge face,
rays beyond the grid, finite ranges, skipped faces and invalid rays; the image entry against the point entry; the raw entry
points' argument checks; determinism; residency; mesh_reprojection against the host; the opt-in through Runner and demo.py.

The checker runs at 1-2 10^7 (ray, face) pairs a second: where faces x rays would exceed PAIRS the rays are an evenly strided
subset."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_mesh_inside import _sheet, _strip
from tests.test_mesh_components_host_logic import volume_of
from tests.test_mesh_rays_host_logic import LATTICE_GRIDS, WINDING_GRIDS, lattice_line_rays, sides_agree_up_to_ties
from zeroshape_amd.utils import camera
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_CASES = ["sphere17", "sphere17_clipped", "scene25", "noise9", "noise23", "three_valued"]
PAIRS = 1 << 25
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _case(name, padded=False):
    """(the level grid, the soup on the GPU, the numpy-welded host mesh of its host copy) - computed once, read by all."""
    vol = volume_of(name)
    if padded:
        vol = np.pad(vol, 1)
    tris, _ = E.extract_surface(torch.from_numpy(vol).cuda(), 0.5, -1.5, 1.5)
    return vol, tris, E.SimpleMesh(tris.cpu().numpy())


def _axis(G):
    return E._lattice_host(G, np.float32(3.0 / G), np.float32(-1.5)).reshape(G, G, G, 3)[:, 0, 0, 0]


def _strided(n, faces):
    keep = max(1, min(n, PAIRS // max(faces, 1)))
    return np.unique(np.linspace(0, n - 1, keep).astype(np.int64)) if n else np.zeros(0, np.int64)


def _pairs(counts):
    return (counts[3] & 0xffffffff) | ((counts[4] & 0xffffffff) << 32)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _raw(vertices, faces, origins, directions, t_min=0.0, t_max=INF, bary=True):
    """zs_mesh_rays on buffers of the right sizes -> (return code, out_counts, t, face, side, bary)."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    v = torch.tensor(np.asarray(vertices, np.float32), device="cuda").reshape(-1, 3).contiguous()
    f = torch.tensor(np.asarray(faces, np.int32), device="cuda").reshape(-1, 3).contiguous()
    o = torch.tensor(np.asarray(origins, np.float32), device="cuda").reshape(-1, 3).contiguous()
    d = torch.tensor(np.asarray(directions, np.float32), device="cuda").reshape(-1, 3).contiguous()
    n, n_verts, m = f.shape[0], v.shape[0], o.shape[0]
    t = torch.full((m,), -9.0, dtype=torch.float64, device="cuda")
    face = torch.full((m,), -9, dtype=torch.int32, device="cuda")
    side = torch.full((m,), -9, dtype=torch.int8, device="cuda")
    w = torch.full((m, 3), -9.0, dtype=torch.float64, device="cuda") if bary else None
    counts = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.zs_mesh_rays_scratch_bytes(n, m)
    assert nbytes % 256 == 0 and (nbytes > 0) == (m > 0)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    rc = lib.zs_mesh_rays(_lib.ptr(v), _lib.ptr(f), n, n_verts, _lib.ptr(o), _lib.ptr(d), m, float(t_min), float(t_max), _lib.ptr(t),
                          _lib.ptr(face), _lib.ptr(side), _lib.ptr(w), _lib.ptr(counts), _lib.ptr(scratch),
                          _lib.current_stream_ptr(v.device))
    torch.cuda.synchronize()
    return rc, counts.tolist(), t.cpu().numpy(), face.cpu().numpy(), side.cpu().numpy(), None if w is None else w.cpu().numpy()


def _raw_image(vertices, faces, intr, mean, scale, H, W, t_min=0.0, t_max=INF):
    """zs_mesh_rays_image -> (return code, out_counts [6], depth, face, side)."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    v = torch.tensor(np.asarray(vertices, np.float32), device="cuda").reshape(-1, 3).contiguous()
    f = torch.tensor(np.asarray(faces, np.int32), device="cuda").reshape(-1, 3).contiguous()
    K, mu, s = (torch.tensor(np.asarray(x, np.float32).reshape(-1), device="cuda") for x in (intr, mean, scale))
    n, n_verts = f.shape[0], v.shape[0]
    depth = torch.full((H, W), -9.0, dtype=torch.float32, device="cuda")
    face = torch.full((H, W), -9, dtype=torch.int32, device="cuda")
    side = torch.full((H, W), -9, dtype=torch.int8, device="cuda")
    counts = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.zs_mesh_rays_scratch_bytes(n, H * W)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    rc = lib.zs_mesh_rays_image(_lib.ptr(v), _lib.ptr(f), n, n_verts, _lib.ptr(K), _lib.ptr(mu), _lib.ptr(s), H, W, float(t_min),
                                float(t_max), _lib.ptr(depth), _lib.ptr(face), _lib.ptr(side), _lib.ptr(counts), _lib.ptr(scratch),
                                _lib.current_stream_ptr(v.device))
    torch.cuda.synchronize()
    return rc, counts.tolist(), depth.cpu().numpy(), face.cpu().numpy(), side.cpu().numpy()


def _assert_equal(got, want):
    """(t, face, side, bary) of the device against the checker's: bits and integers."""
    t, face, side, w = got
    assert np.array_equal(_bits(t), _bits(want[0])), np.flatnonzero(_bits(t) != _bits(want[0]))[:8]
    assert np.array_equal(face, want[1]), np.flatnonzero(face != want[1])[:8]
    assert np.array_equal(side, want[2]), np.flatnonzero(side != want[2])[:8]
    if w is not None:
        assert np.array_equal(_bits(w), _bits(want[3]))


def _assert_raw_parity(vertices, faces, origins, directions, **kw):
    """The raw entry point against the checker on one indexed mesh -> (counts, t, face, side)."""
    o, d = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(directions, np.float32).reshape(-1, 3)
    rc, counts, t, face, side, w = _raw(vertices, faces, o, d, **kw)
    want = E.mesh_rays_host(o, d, vertices, faces, bary=True, **{k: v for k, v in kw.items() if k != "bary"})
    assert rc == 1 and counts[:3] == want[4][:3].tolist()
    _assert_equal((t, face, side, w), want)
    assert _pairs(counts) <= _pairs(want[4].tolist())                # no pair is read twice
    return counts, t, face, side


def _directions(rng, n):
    """Random directions; every fourth is parallel to an axis (components of +0 and -0), every fourth of the rest to a plane."""
    d = rng.normal(size=(n, 3)).astype(np.float32)
    axis = rng.randint(0, 3, n)
    for k in range(0, n, 4):
        keep = d[k, axis[k]]
        d[k] = [0.0, -0.0, 0.0]
        d[k, axis[k]] = keep
    for k in range(1, n, 8):
        d[k, axis[k]] = 0.0
    return d


def _mixed_rays(vol, host, seed):
    rng = np.random.RandomState(seed)
    lo, hi = host.vertices.min(axis=0).astype(np.float64), host.vertices.max(axis=0).astype(np.float64)
    around = (0.5 * (lo + hi) + rng.uniform(-1.5, 1.5, (1500, 3)) * 0.5 * (hi - lo)).astype(np.float32)
    for a in range(3):
        assert (around[:, a] < lo[a]).any() and (around[:, a] > hi[a]).any()
    line_o, line_d, _, _ = lattice_line_rays(vol, _axis(vol.shape[0]))
    surface = np.concatenate([host.vertices[::3], host.triangles.mean(axis=1)[::5]]).astype(np.float32)
    o = np.concatenate([line_o, around, surface])
    d = np.concatenate([line_d, _directions(rng, len(around)), _directions(rng, len(surface))])
    keep = _strided(len(o), len(host.faces))
    return o[keep], d[keep]


@pytest.mark.parametrize("name", PARITY_CASES)
def test_against_the_checker(name):
    """Lattice-line rays (along cell edges, through vertices), rays from random points in and around the box (outside it on
    every side) in random and axis-parallel directions, rays from vertices and face centroids - through mesh_ray_cast."""
    vol, tris, host = _case(name)
    o, d = _mixed_rays(vol, host, len(name))
    mesh = E.SimpleMesh(tris)
    done = mesh.ray_cast(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), bary=True)
    assert done.t.is_cuda and done.t.dtype == torch.float64 and done.face.dtype == torch.int32 and done.side.dtype == torch.int8
    assert done.t.shape == (len(o),) and done.bary.shape == (len(o), 3) and done.bary.dtype == torch.float64
    want = E.mesh_rays_host(o, d, host.vertices, host.faces, bary=True)
    _assert_equal([x.cpu().numpy() for x in done[:4]], want)
    assert (want[1] >= 0).any() and (want[1] < 0).any() and (want[2] == 1).any() and (want[2] == -1).any()
    counts = done.check()
    assert counts["skipped_faces"] == 0 and counts["status"] == 0 and 0 < counts["pairs"] < len(o) * len(host.faces)
    # the hit points from the weights lie where the rays are: |p - (o + t d)| within float64 rounding of the coordinates
    hit = want[1] >= 0
    p = done.points().cpu().numpy()
    with np.errstate(invalid="ignore"):
        along = o.astype(np.float64) + want[0][:, None] * d.astype(np.float64)
    assert np.isnan(p[~hit]).all() and np.abs(p[hit] - along[hit]).max() < 1e-9


@pytest.mark.parametrize("name,padded,n_lines,n_hits", LATTICE_GRIDS)
def test_lattice_line_rays_on_the_device(name, padded, n_lines, n_hits):
    """Independent oracle 1, without the checker: the ray along a lattice line hits iff the line has an occupied point,
    between the last empty and the first occupied lattice point."""
    vol, tris, host = _case(name, padded)
    G = vol.shape[0]
    o, d, lo, hi = lattice_line_rays(vol, _axis(G))
    done = E.mesh_ray_cast(E.SimpleMesh(tris), torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    t, face = done.t.cpu().numpy(), done.face.cpu().numpy()
    expect = hi >= 0
    assert len(o) == n_lines and expect.sum() == n_hits and np.array_equal(face >= 0, expect)
    slack = 1e-9 * 3.0 / G
    assert np.all(t[expect] >= lo[expect] - slack) and np.all(t[expect] <= hi[expect] + slack)


@pytest.mark.parametrize("name,padded", WINDING_GRIDS)
def test_plus_z_rays_agree_with_the_winding_numbers_on_the_device(name, padded):
    """Independent oracle 2, without the checker: against zs_mesh_winding."""
    vol, tris, host = _case(name, padded)
    mesh = E.SimpleMesh(tris)
    q = np.random.RandomState(len(name)).uniform(-1.6, 1.6, (3000, 3)).astype(np.float32)
    d = np.zeros_like(q)
    d[:, 2] = 1.0
    winding = E.mesh_winding(mesh, torch.from_numpy(q).cuda())
    up = winding.up.cpu().numpy()
    assert torch.equal(winding.up, winding.down) and (up != 0).any()
    done = E.mesh_ray_cast(mesh, torch.from_numpy(q).cuda(), torch.from_numpy(d).cuda())
    t, face, side = (x.cpu().numpy() for x in done[:3])
    assert np.all(face[up != 0] >= 0) and ((up == 0) & (face >= 0)).any()
    assert sides_agree_up_to_ties(host, q, d, t, face, side, np.where(up != 0, -1, 1), 1e-9 * 3.0 / vol.shape[0]) < 30


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 255, 256, 257])
def test_ray_counts(m):
    _, tris, host = _case("scene25")
    rng = np.random.RandomState(m)
    o = rng.uniform(-1.6, 1.6, (m, 3)).astype(np.float32)
    o[::3] = host.vertices[(np.arange(len(o[::3])) * 7) % len(host.vertices)]       # some start on the surface
    d = _directions(rng, m)
    if m == 0:
        rc, counts, t, face, side, w = _raw(host.vertices, host.faces, o, d)
        assert rc == 1 and counts == [-1] * 5 and t.shape == (0,)   # touches nothing
        return
    _assert_raw_parity(host.vertices, host.faces, o, d)


@pytest.mark.parametrize("n_faces", [1, 2, 255, 256, 257, 2047, 2048, 2049])
def test_face_counts_around_the_workgroup_and_the_scan_tile(n_faces):
    verts, faces = _strip(n_faces + 2)
    rng = np.random.RandomState(n_faces)
    o = np.concatenate([rng.uniform(-0.5, 1.5, (400, 3)) * [n_faces / 2.0 + 1, 1, 2] - [0, 0, 1], verts[:: max(1, len(verts) // 100)],
                        0.5 * (verts[:-1] + verts[1:])[:: max(1, len(verts) // 100)]]).astype(np.float32)
    d = _directions(rng, len(o))
    d[:200] = [0.0, 0.0, 1.0]
    d[:200:2] = [0.0, 0.0, -1.0]
    counts, t, face, side = _assert_raw_parity(verts, faces, o, d)
    assert counts[:3] == [0, 0, 0] and (face >= 0).any() and 0 < _pairs(counts) <= n_faces * len(o)


def test_a_single_cell():
    """Fewer than sixteen faces make one cell: a ray reads every face or, where t excludes the cell, none."""
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    rng = np.random.RandomState(5)
    o = rng.uniform(-0.5, 1.2, (300, 3)).astype(np.float32)
    d = _directions(rng, 300)
    counts, t, face, side = _assert_raw_parity(tet, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], o, d)
    assert _pairs(counts) % 4 == 0 and 0 < _pairs(counts) <= 4 * 300 and (side == 1).any() and (side == -1).any()
    # 400 triangles whose boxes share one centre fall into one cell of many
    rng = np.random.RandomState(6)
    a = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    b = a * rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    verts = np.stack([a, b, -a], axis=1).reshape(-1, 3)
    _assert_raw_parity(verts, np.arange(1200).reshape(400, 3), o * 2, d)


def test_an_axis_without_extent():
    """A flat sheet in each of the three planes: rays across it, rays inside its plane (which hit nothing: det = 0), rays
    from its own vertices and centroids."""
    grid, faces = _sheet()
    rng = np.random.RandomState(4)
    for axis in range(3):
        verts = np.insert(grid, axis, np.float32(1.5), axis=1)
        o = np.concatenate([rng.uniform(-2, 8, (450, 3)), verts[::5], verts[faces].mean(axis=1)[::7]]).astype(np.float32)
        d = _directions(rng, len(o))
        o[:150, axis] = 1.5                                          # in the plane ...
        d[:150, axis] = 0.0                                          # ... and staying there
        across = np.zeros(3, np.float32)
        across[axis] = 1.0
        d[150:300] = across * np.where(o[150:300, axis] < 1.5, 1, -1)[:, None]      # straight at the sheet
        counts, t, face, side = _assert_raw_parity(verts, faces, o, d)
        assert not (face[:150] >= 0).any() and (face[150:300] >= 0).any() and (face[150:300] < 0).any()
        assert 0 < _pairs(counts) < len(faces) * len(o)             # the cells still prune
    line = np.stack([np.arange(40) * 0.1, np.full(40, 2.0), np.full(40, -1.0)], axis=1).astype(np.float32)
    _, t, face, side = _assert_raw_parity(line, np.stack([np.arange(38), np.arange(38) + 1, np.arange(38) + 2], axis=1),
                                          rng.uniform(-2, 4, (200, 3)), _directions(rng, 200))
    assert not (face >= 0).any()


def test_one_face_that_spans_the_box_among_2000_small_ones():
    """The reaches of the huge face are half the grid each way: slow, still the checker's bits; without it the cells prune."""
    rng = np.random.RandomState(7)
    centres = rng.uniform(-1, 1, (2000, 1, 3))
    small = (centres + rng.uniform(-0.02, 0.02, (2000, 3, 3))).astype(np.float32)
    huge = np.array([[[-1.2, -1.2, -1.2], [1.2, -1.2, -1.1], [0.1, 1.2, 1.2]]], np.float32)
    o = rng.uniform(-1.5, 1.5, (600, 3)).astype(np.float32)
    d = _directions(rng, 600)
    without, t0, face0, _ = _assert_raw_parity(small.reshape(-1, 3), np.arange(6000).reshape(-1, 3), o, d)
    assert _pairs(without) < 0.05 * 2000 * len(o)
    for soup in (np.concatenate([small[:1000], huge, small[1000:]]), np.concatenate([huge, small])):
        verts = soup.reshape(-1, 3)
        counts, t, face, side = _assert_raw_parity(verts, np.arange(len(verts)).reshape(-1, 3), o, d)
        assert (t != t0).any() and (face0 >= 0).any()                # the huge face is hit, and so are small ones
        print("pairs read: %d with the huge face, %d without, of %d" % (_pairs(counts), _pairs(without), 2001 * len(o)))


def test_rays_that_start_beyond_the_grid():
    _, _, host = _case("scene25")
    rng = np.random.RandomState(11)
    n = 240
    o = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    d = (rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    side_of = np.arange(n) % 6
    for k in range(6):
        rows = side_of == k
        o[rows, k // 2] = 4.0 if k % 2 else -4.0
        d[rows, k // 2] = 1.0 if k % 2 else -1.0                     # beyond the box along the major axis, pointing away
    counts, t, face, side = _assert_raw_parity(host.vertices, host.faces, o, d)
    assert not (face >= 0).any() and np.all(t == INF) and _pairs(counts) == 0      # excluded by t alone: nothing is read
    counts, t, face, side = _assert_raw_parity(host.vertices, host.faces, o, -d)   # ... and pointing at it
    assert (face >= 0).any() and _pairs(counts) > 0
    o2 = o.copy()
    o2[:, [1, 2, 0]] = o                                             # beyond the box beside the ray's major axis
    counts, t, face, side = _assert_raw_parity(host.vertices, host.faces, o2, d)
    far, straight = o.copy(), np.zeros_like(d)
    for k in range(6):
        rows = side_of == k
        far[rows, k // 2] *= 1e6                                     # from far away, straight at the box
        straight[rows, k // 2] = -d[rows, k // 2]
    counts, t, face, side = _assert_raw_parity(host.vertices, host.faces, far, straight)
    assert (face >= 0).any() and np.all(t[face >= 0] > 3.9e6)


def test_finite_ranges_with_equality():
    _, _, host = _case("sphere17")
    rng = np.random.RandomState(12)
    o = rng.uniform(-1.6, 1.6, (300, 3)).astype(np.float32)
    d = _directions(rng, 300)
    _, t, face, side = _assert_raw_parity(host.vertices, host.faces, o, d)
    k = int(np.flatnonzero(face >= 0)[0])
    first = float(t[k])
    for kw in (dict(t_min=first), dict(t_max=first), dict(t_min=first, t_max=first)):              # both ends are inclusive
        _, t1, face1, _ = _assert_raw_parity(host.vertices, host.faces, o, d, **kw)
        assert t1[k] == first and face1[k] == face[k]
    _, t1, face1, _ = _assert_raw_parity(host.vertices, host.faces, o, d, t_min=float(np.nextafter(first, INF)))
    assert t1[k] > first
    _, t1, face1, _ = _assert_raw_parity(host.vertices, host.faces, o, d, t_max=float(np.nextafter(first, -INF)))
    assert face1[k] == -1 and t1[k] == INF
    for kw in (dict(t_min=0.3, t_max=0.9), dict(t_min=-INF), dict(t_min=-2.0, t_max=-0.1), dict(t_min=1.0, t_max=0.5),
               dict(t_min=float("nan")), dict(t_max=float("nan")), dict(t_min=-INF, t_max=-INF)):
        _assert_raw_parity(host.vertices, host.faces, o, d, **kw)


def test_skipped_faces_invalid_rays_and_a_null_out_bary():
    _, _, host = _case("scene25")
    verts, faces = host.vertices.copy(), host.faces.copy()
    verts[7, 1], verts[11, 0], verts[500, 2] = np.nan, np.inf, -np.inf
    faces[3, 2], faces[9, 0], faces[2000, 1] = len(verts), -1, 2 ** 31 - 1
    bad = np.isin(faces, [7, 11, 500]).any(axis=1)
    bad[[3, 9, 2000]] = True
    rng = np.random.RandomState(9)
    o = rng.uniform(-1.6, 1.6, (500, 3)).astype(np.float32)
    d = _directions(rng, 500)
    o[5, 0], o[9, 2], d[20, 1], d[499], d[30] = np.nan, np.inf, -np.inf, np.nan, 0.0
    rows = [5, 9, 20, 30, 499]
    counts, t, face, side = _assert_raw_parity(verts, faces, o, d)
    assert counts[:3] == [int(bad.sum()), 5, 1 | 2 | 4] and np.isnan(t[rows]).all() and (face[rows] == -1).all() and not side[rows].any()
    # the valid faces alone give the same hits: a skipped face is not read through
    rest = np.setdiff1d(np.arange(500), rows)
    index = np.flatnonzero(~bad)
    want = E.mesh_rays_host(o[rest], d[rest], np.nan_to_num(verts, posinf=0.0, neginf=0.0), faces[~bad])
    assert np.array_equal(_bits(t[rest]), _bits(want[0])) and np.array_equal(face[rest], np.where(want[1] >= 0, index[want[1]], -1))
    # one kind at a time: the status bits
    only = host.faces.copy()
    only[3, 2] = len(verts)
    assert _raw(host.vertices, only, o[rest], d[rest])[1][:3] == [1, 0, 2]
    assert _raw(verts, host.faces, o[rest], d[rest])[1][:3] == [int(np.isin(host.faces, [7, 11, 500]).any(axis=1).sum()), 0, 1]
    # without out_bary
    rc, counts1, t1, face1, side1, none = _raw(verts, faces, o, d, bary=False)
    assert rc == 1 and none is None and np.array_equal(_bits(t1), _bits(t)) and np.array_equal(face1, face) and counts1 == counts
    # no valid face at all, no vertices, no faces
    for v, f in ((verts[:3] * np.nan, [[0, 1, 2]]), (np.zeros((0, 3)), [[0, 1, 2]]), (verts, np.zeros((0, 3)))):
        rc, counts, t, face, side, w = _raw(v, f, o, d)
        assert rc == 1 and counts == [len(f), 5, (4 | (2 if len(v) == 0 else 1)) if len(f) else 4, 0, 0]
        assert np.all(t[rest] == INF) and (face == -1).all() and not side.any() and np.isnan(w).all()
    # through mesh_ray_cast: the face-index bit raises where the counts are read
    from zeroshape_amd import _lib
    mesh = E.SimpleMesh(torch.zeros(len(only), 3, 3, device="cuda"))
    mesh._device_weld = (torch.from_numpy(host.vertices).cuda(), torch.from_numpy(only.astype(np.int32)).cuda(), None)
    done = E.mesh_ray_cast(mesh, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    with pytest.raises(_lib.ZeroShapeHipError, match="status 6"):
        done.check()
    for rays in ((o, d), (torch.from_numpy(o), torch.from_numpy(d)), (torch.from_numpy(o).cuda(), d)):
        with pytest.raises(ValueError, match="CUDA"):
            E.mesh_ray_cast(mesh, *rays)
    with pytest.raises(ValueError, match="CUDA"):
        E.mesh_depth_map(mesh, np.eye(3), torch.zeros(3).cuda(), torch.ones(1).cuda(), 4, 4)


def test_argument_checks_of_the_raw_entry_points():
    """0 and a message that names the entry point, before anything is launched (a host buffer stands in for every non-null
    pointer: nothing may read it); zero rays return 1."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p, odd = ctypes.c_void_p(base + (-base) % 8), ctypes.c_void_p(base + (-base) % 8 + 4)

    def fails(rc, what, who):
        msg = lib.zs_last_error()
        assert rc == 0 and msg.startswith(who) and what.encode() in msg, (what, rc, msg)

    def call(n=1, v=3, m=1, ptr=p, scratch=p, **null):
        args = dict(vertices=ptr, faces=ptr, origins=ptr, directions=ptr, out_t=ptr, out_face=ptr, out_side=ptr, out_bary=ptr,
                    out_counts=ptr)
        args.update(null)
        return lib.zs_mesh_rays(args["vertices"], args["faces"], n, v, args["origins"], args["directions"], m, 0.0, INF,
                                args["out_t"], args["out_face"], args["out_side"], args["out_bary"], args["out_counts"], scratch, None)

    who = b"zs_mesh_rays: "
    fails(call(n=-1), "negative size", who)
    fails(call(v=-3), "negative size", who)
    fails(call(m=-1), "negative size", who)
    fails(call(n=2 ** 24 + 1), "too large", who)
    fails(call(m=2 ** 28 + 1), "too large", who)
    for name in ("vertices", "faces", "origins", "directions", "out_t", "out_face", "out_side", "out_counts"):
        fails(call(**{name: None}), "null pointer", who)
    fails(call(scratch=None), "null pointer", who)
    fails(call(scratch=odd), "8-byte aligned", who)
    fails(call(scratch=odd, out_bary=None), "8-byte aligned", who)   # out_bary may be null: the next check speaks
    assert call(m=0, ptr=None, scratch=None) == 1 and call(n=0, v=0, m=0, ptr=None, scratch=None) == 1

    def image(n=1, v=3, H=2, W=2, ptr=p, scratch=p, **null):
        args = dict(vertices=ptr, faces=ptr, intr=ptr, mean=ptr, scale=ptr, out_depth=ptr, out_face=ptr, out_side=ptr, out_counts=ptr)
        args.update(null)
        return lib.zs_mesh_rays_image(args["vertices"], args["faces"], n, v, args["intr"], args["mean"], args["scale"], H, W, 0.0, INF,
                                      args["out_depth"], args["out_face"], args["out_side"], args["out_counts"], scratch, None)

    who = b"zs_mesh_rays_image: "
    fails(image(n=-1), "negative size", who)
    fails(image(v=-1), "negative size", who)
    fails(image(H=-1), "negative size", who)
    fails(image(W=-1), "negative size", who)
    fails(image(n=2 ** 24 + 1), "too large", who)
    fails(image(H=16385), "too large", who)
    fails(image(H=16384, W=16385), "too large", who)
    for name in ("vertices", "faces", "intr", "mean", "scale", "out_depth", "out_face", "out_side", "out_counts"):
        fails(image(**{name: None}), "null pointer", who)
    fails(image(scratch=None), "null pointer", who)
    fails(image(scratch=odd), "8-byte aligned", who)
    assert image(H=0, ptr=None, scratch=None) == 1 and image(W=0, ptr=None, scratch=None) == 1
    size = lib.zs_mesh_rays_scratch_bytes
    assert size(-1, 1) == 0 and size(1, -1) == 0 and size(2 ** 24 + 1, 1) == 0 and size(1, 2 ** 28 + 1) == 0
    assert size(0, 0) == 0 and size(17, 0) == 0                      # nothing to cast: empty
    for n, m in ((0, 5), (1, 1), (17, 3), (2 ** 24, 2 ** 28), (100, 224 * 224)):
        assert size(n, m) > 0 and size(n, m) % 256 == 0
    assert size(2 ** 24, 1) > size(2 ** 20, 1) > size(1, 1) and size(1000, 1) == size(1000, 2 ** 28)   # the face count alone


def test_two_runs_give_the_same_bytes():
    vol, tris, host = _case("noise23")
    o, d = _mixed_rays(vol, host, 2)
    do, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    a, b = (E.mesh_ray_cast(E.SimpleMesh(tris), do, dd, bary=True) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
    K, mean, scale = _camera(64, 64)
    a, b = (E.mesh_depth_map(E.SimpleMesh(tris), *(torch.from_numpy(x).cuda() for x in (K, mean, scale)), 64, 64) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_pruning_is_real():
    vol, tris, host = _case("sphere17")
    o, d = _mixed_rays(vol, host, 1)
    done = E.mesh_ray_cast(E.SimpleMesh(tris), torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    pairs, brute = done.check()["pairs"], len(o) * len(host.faces)
    print("sphere17: %d faces x %d rays, %.3f %% of the pairs read" % (len(host.faces), len(o), 100.0 * pairs / brute))
    assert 0 < pairs < brute


def _camera(H, W, z=2.2, scale=0.6):
    """A ZeroShape-like camera (f = 1.3875 W) and a normalisation that puts the [-1.5, 1.5]^3 box in front of it."""
    f = 1.3875
    K = np.array([[f * W, 0, W / 2], [0, f * H, H / 2], [0, 0, 1]], np.float32)
    return K, np.float32([0.05, -0.03, z]), np.float32([scale])


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (5, 3), (64, 64), (224, 224)])
def test_the_image_entry_equals_the_point_entry(H, W):
    """The rays made in the kernel and camera_rays_host's rays uploaded; at 64 x 64 also against the checker and with a camera
    that has skew, rays that are invalid (D_z <= 0) and a finite range."""
    _, _, host = _case("sphere17")
    cameras = [_camera(H, W)]
    if (H, W) == (64, 64):
        # a projective third row: D_z changes its sign along 153.8 j + 30.6 i = 7656, inside the image
        cameras.append((np.array([[90, 3, 30], [-2, 85, 33], [1.8, 0.4, 1]], np.float32), np.float32([0.1, 0, 2.5]), np.float32([0.7])))
    seen = []
    for K, mean, scale in cameras:
        for kw in (dict(), dict(t_min=2.0, t_max=2.4)) if (H, W) == (64, 64) else (dict(),):
            rc, counts, depth, face, side = _raw_image(host.vertices, host.faces, K, mean, scale, H, W, **kw)
            o, d = E.camera_rays_host(K, mean, scale, H, W)
            rc2, counts2, t, face2, side2, _ = _raw(host.vertices, host.faces, o, d, **kw)
            assert rc == 1 and rc2 == 1 and counts[:5] == counts2 and counts[5] == (face2 >= 0).sum()
            with np.errstate(over="ignore"):
                assert np.array_equal(depth.reshape(-1).view(np.uint32), t.astype(np.float32).view(np.uint32))
            assert np.array_equal(face.reshape(-1), face2) and np.array_equal(side.reshape(-1), side2)
            if (H, W) == (64, 64):
                want = E.mesh_rays_host(o, d, host.vertices, host.faces, **kw)
                _assert_equal((t, face2, side2, None), want)
                assert counts[1] == int(np.isnan(d).any(axis=1).sum())
            seen.append(counts)
    if (H, W) == (64, 64):
        assert seen[2][1] > 0 and seen[2][5] > 0 and seen[0][1] == 0 # the second camera looks backwards for some pixels
    if H * W >= 64 * 64:
        assert 0 < seen[0][5] < H * W


def test_the_round_trip_through_the_depth_map():
    """Without the checker: the depth map and its hit mask, fed back, score the mesh perfectly; the hit points, unprojected
    with camera.unproj_depth and normalised, lie on the mesh within the float32 rounding of the ray and the unprojection."""
    _, tris, host = _case("scene25")
    H = W = 64
    K, mean, scale = _camera(H, W)
    dK, dmean, dscale = (torch.from_numpy(x).cuda() for x in (K, mean, scale))
    mesh = E.SimpleMesh(tris)
    image = E.mesh_depth_map(mesh, dK, dmean, dscale, H, W)
    hit = image.face >= 0
    depth = torch.where(hit, image.depth, torch.zeros_like(image.depth))
    record = E.mesh_reprojection(mesh, hit.to(torch.float32), depth, dK, dmean, dscale, depth_tol=0.0)
    assert record.silhouette_iou == 1.0 and record.depth_max == 0.0 and record.depth_rms == 0.0
    assert record.agreeing == record.mesh_pixels == record.depth_pixels == int(hit.sum()) > 100
    assert record.mask_pixels == record.both == record.either == record.mesh_pixels and record.back_faces == 0
    X = camera.unproj_depth(edict(dict(H=H, W=W)), depth[None, None], dK[None])[0]                  # [H*W,3] in the camera frame
    v = (X - dmean[None]) / dscale
    rows = hit.reshape(-1)
    sq = mesh.distance_to(v[rows].contiguous()).sqdist.cpu().numpy()
    o, d = E.camera_rays_host(K, mean, scale, H, W)
    reach = depth.reshape(-1).cpu().numpy().astype(np.float64) * np.linalg.norm(d.astype(np.float64) * np.float64(scale[0]), axis=1)
    bound = 64 * 2.0 ** -24 * np.maximum(reach, np.linalg.norm(mean.astype(np.float64))) / np.float64(scale[0])
    print("round trip: largest distance %.3e, its bound %.3e" % (np.sqrt(sq).max(), bound[rows.cpu().numpy()].min()))
    assert np.all(np.sqrt(sq) <= bound[rows.cpu().numpy()])


@functools.lru_cache(maxsize=None)
def _scene(H=64, W=64):
    """scene25 in the camera, with a mask shifted against its silhouette and a depth that is the mesh's own (the host's depth
    map) moved by up to 0.3 either way, with holes - computed once, changed by nobody."""
    _, tris, host = _case("scene25")
    K, mean, scale = _camera(H, W)
    rng = np.random.RandomState(13)
    ii, jj = np.mgrid[:H, :W]
    mask = (((ii - H / 2) ** 2 + (jj - W / 2 - 3) ** 2) < (0.3 * H) ** 2).astype(np.float32)
    own = E.mesh_depth_map(host, K, mean, scale, H, W).depth
    depth = (np.where(np.isfinite(own), own, 2.0) + 0.3 * rng.uniform(-1, 1, (H, W))).astype(np.float32)
    depth[::7, ::5], depth[3::11, 2::9], depth[5::13, 1::6] = np.nan, -1.0, np.inf
    return tris, host, mask, depth, K, mean, scale


def test_mesh_reprojection_equals_the_host_record():
    tris, host, mask, depth, K, mean, scale = _scene()
    device = [torch.from_numpy(x).cuda() for x in (mask, depth, K, mean, scale)]
    for kw in (dict(depth_tol=0.05, cell_edge=3.0 / 25), dict(depth_tol=0.3)):
        got = E.mesh_reprojection(E.SimpleMesh(tris), *device, **kw)
        want = E.mesh_reprojection(host, mask, depth, K, mean, scale, **kw)
        assert isinstance(got, E.MeshReprojection) and got._fields == want._fields
        for name in got._fields:
            a, b = getattr(got, name), getattr(want, name)
            assert type(a) is type(b) and (a == b or (a != a and b != b)), (name, a, b)
        assert 0 < got.both < got.either and 0 < got.agreeing < got.depth_pixels < got.both and got.depth_max > 0
    image = E.mesh_depth_map(E.SimpleMesh(tris), *device[2:], 64, 64)
    want = E.mesh_depth_map(host, K, mean, scale, 64, 64)
    assert np.array_equal(image.depth.cpu().numpy().view(np.uint32), want.depth.view(np.uint32))
    assert np.array_equal(image.face.cpu().numpy(), want.face) and np.array_equal(image.side.cpu().numpy(), want.side)
    assert image.check()["hit_pixels"] == want.check()["hit_pixels"] and image.counts.tolist()[:3] == want.counts.tolist()[:3]
    with pytest.raises(ValueError, match="CUDA"):
        E.mesh_reprojection(E.SimpleMesh(tris), mask, *device[1:], depth_tol=0.1)


def test_the_results_are_resident_and_the_mesh_keeps_its_weld():
    tris, host, mask, depth, K, mean, scale = _scene()
    mesh = E.SimpleMesh(tris)
    before = set(vars(mesh))
    o = torch.from_numpy(host.vertices[:100] + np.float32(0.01)).cuda()
    done = mesh.ray_cast(o, torch.ones_like(o), bary=True)
    assert isinstance(done, E.MeshRays) and all(x.is_cuda for x in done) and done.mesh is mesh
    assert done.counts.dtype == torch.int32 and done.counts.shape == (5,) and done.points().is_cuda
    assert mesh._device_weld is not None and set(vars(mesh)) == before             # the weld it made is kept; nothing else
    assert mesh._triangles is None and mesh._indexed is None and mesh._components is None and mesh._adjacency is None
    weld = mesh._device_weld
    device = [torch.from_numpy(x).cuda() for x in (mask, depth, K, mean, scale)]
    image = E.mesh_depth_map(mesh, *device[2:], 64, 64)
    assert isinstance(image, E.MeshDepthMap) and all(x.is_cuda for x in image) and image.counts.shape == (6,)
    assert image.depth.dtype == torch.float32 and image.depth.shape == (64, 64) and image.side.dtype == torch.int8
    E.mesh_reprojection(mesh, *device, depth_tol=0.1)
    assert mesh._device_weld is weld and mesh._triangles is None and mesh._indexed is None and set(vars(mesh)) == before
    empty = mesh.ray_cast(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda"), bary=True)
    assert empty.t.shape == (0,) and empty.bary.shape == (0, 3) and empty.check()["pairs"] == 0
    assert E.mesh_depth_map(mesh, *device[2:], 0, 5).depth.shape == (0, 5)
    nothing = E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda"))
    assert torch.all(nothing.ray_cast(o, torch.ones_like(o)).t == INF)
    assert E.mesh_reprojection(nothing, *device, depth_tol=0.1).mesh_pixels == 0


def test_the_opt_in_through_the_runner(tmp_path, encoder_sd, seeded_sd):
    from tests.test_gpu_seen_mesh import shape_opt
    from zeroshape_amd.data.synthetic import Dataset
    from zeroshape_amd.model.shape_engine import Runner
    full = dict(encoder_sd)
    full.update({"impl_network." + k: v for k, v in seeded_sd.items()})
    full["impl_network.impl_mlp.layers.8.bias"] = full["impl_network.impl_mlp.layers.8.bias"] + 0.26     # a level set that exists
    reports = {}
    for flag in (False, True):
        out = tmp_path / ("on" if flag else "off")
        opt = shape_opt(out)
        opt.eval.dump_results = True
        opt.eval.mesh_report = True
        if flag:
            opt.eval.mesh_reprojection = True
        r = Runner(opt)
        r.load_dataset(opt, dataset=Dataset(opt, n_items=2, n_points=1000))
        r.build_networks(opt)
        r.graph.load_state_dict(full, strict=True)
        r.evaluate(opt)
        reports[flag] = [json.load(open(out / "dump_synthetic" / ("%d_mesh_report.json" % i))) for i in (0, 1)]
    for off, on in zip(reports[False], reports[True]):
        assert "reprojection" not in off and set(on["reprojection"]) == set(E.MeshReprojection._fields)
        assert set(on) == set(off) | {"reprojection"} and (on["faces"], on["vertices"]) == (off["faces"], off["vertices"])
        record = on["reprojection"]
        assert record["mask_pixels"] > 0 and record["both"] <= min(record["mask_pixels"], record["mesh_pixels"]) <= record["either"]
        assert record["cell_edge"] == 3.0 / 16


def test_demo_script_writes_the_reprojection(tmp_path, encoder_sd, seeded_sd):
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
                        "--output_root=%s" % tmp_path, "--eval.mesh_reprojection=true", "--eval.mesh_report=true"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    preds = tmp_path / "data" / "preds"
    report = json.load(open(preds / "blob_mesh_report.json"))
    record = report["reprojection"]
    print("demo.py: reprojection", record)
    assert set(record) == set(E.MeshReprojection._fields) and "volume_iou" not in report and "deviation" not in report
    assert 0 < record["both"] <= min(record["mask_pixels"], record["mesh_pixels"]) <= record["either"] <= 224 * 224
    assert record["silhouette_iou"] == record["both"] / record["either"] and record["cell_edge"] == 3.0 / 32
    assert record["agreeing"] <= record["depth_pixels"] <= record["both"]
    png = np.asarray(Image.open(preds / "blob_mesh_depth.png"))
    assert png.shape == (224, 224) and png.dtype == np.uint16 and (png < 65535).sum() > 0
