"""No GPU: the numpy restatement of the vertex normals (eval_3D.vertex_normals_host, the checker of csrc/mesh_weld.hip) on a
marching-cubes sphere, SimpleMesh from an array with its new ``vertex_normals``, the OBJ text of dump_meshes with and without
normals, and the argument checks of zs_mesh_weld / zs_mesh_weld_vertices through the raw library."""
import ctypes

import numpy as np

from oracle import mc_ref as M
from tests.test_oracle_mc import _sphere
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.eval_3D import SimpleMesh, vertex_normals_host
from zeroshape_amd.utils.options import EasyDict as edict

CENTRE = np.array([0.1, -0.05, 0.2])


def _sphere_soup():
    vol, ax = _sphere(17, 0.8)
    step = float(ax[1] - ax[0])
    return M.marching_cubes(vol, 0.5, step, float(ax[0]))         # index -> linspace coordinate: the sphere around CENTRE


def test_normals_of_a_sphere_are_unit_and_point_outwards():
    """Every normal is unit length (or exactly zero), and its dot product with the analytic radial direction (vertex -
    centre) is POSITIVE for every vertex: the tables wind a triangle so that cross(v1 - v0, v2 - v0) points towards
    decreasing values (tests/test_oracle_mc.py: test_tables_are_crack_free_for_every_sign_pattern), which for an occupancy
    grid - above the iso value inside - is out of the object."""
    tris = _sphere_soup()
    m = SimpleMesh(tris)
    n = vertex_normals_host(tris, m.faces, len(m.vertices))
    assert n.dtype == np.float32 and n.shape == m.vertices.shape and len(n) > 100
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    zero = ~n.any(axis=1)
    assert np.all(zero | (np.abs(length - 1.0) < 1e-6))
    assert zero.sum() == 0                                        # (a closed sphere has no vertex without area around it)
    radial = m.vertices.astype(np.float64) - CENTRE
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    dots = (n * radial).sum(axis=1)
    assert np.all(dots > 0), (dots.min(), dots.max())
    assert dots.min() > 0.9                                       # and close to it: the mesh is a sphere


def test_normals_formula_by_hand():
    """Two triangles sharing an edge, areas 0.5 and 1: the shared vertices get the area-weighted mean, a vertex of one
    triangle that triangle's normal; a zero-area triangle adds nothing and its own vertex gets (0, 0, 0); a non-finite sum
    gives (0, 0, 0)."""
    tris = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]],           # normal (0, 0, 1), cross = (0, 0, 1)
                     [[0, 0, 0], [0, 0, 2], [1, 0, 0]],           # cross = (0, 2, 0)
                     [[5, 5, 5], [6, 6, 6], [7, 7, 7]],           # collinear: cross = 0
                     [[9, 0, 0], [9, 3e38, 0], [9, 0, 3e38]]],    # cross = (9e76, 0, 0): beyond fp32, fine in fp64
                    np.float32)
    m = SimpleMesh(tris)
    n = m.vertex_normals
    where = {tuple(v): i for i, v in enumerate(m.vertices.tolist())}
    np.testing.assert_allclose(n[where[(0, 1, 0)]], [0, 0, 1], atol=1e-7)
    np.testing.assert_allclose(n[where[(0, 0, 2)]], [0, 1, 0], atol=1e-7)
    np.testing.assert_allclose(n[where[(0, 0, 0)]], np.array([0, 2, 1]) / np.sqrt(5.0), atol=1e-7)
    np.testing.assert_allclose(n[where[(1, 0, 0)]], np.array([0, 2, 1]) / np.sqrt(5.0), atol=1e-7)
    for v in ((5, 5, 5), (6, 6, 6), (7, 7, 7)):
        assert not n[where[v]].any()
    np.testing.assert_allclose(n[where[(9, 0, 0)]], [1, 0, 0], atol=1e-7)          # 9e76 is finite in fp64: a normal
    nan = tris.copy()
    nan[0, 1, 0] = np.inf
    bad = SimpleMesh(nan)
    k = int(np.flatnonzero(np.isinf(bad.vertices).any(axis=1))[0])
    assert not bad.vertex_normals[k].any() and not np.isnan(bad.vertex_normals).any()


def test_simple_mesh_from_an_array_needs_no_gpu_and_has_vertex_normals():
    tris = _sphere_soup()
    m = SimpleMesh(tris)
    assert m.device_triangles is None
    assert m.triangles.dtype == np.float32 and m.triangles.shape == tris.shape and np.array_equal(m.triangles, tris)
    assert m.vertices.dtype == np.float32 and m.faces.dtype == np.int64
    assert np.array_equal(m.vertices[m.faces].view(np.uint32), (tris + np.float32(0)).view(np.uint32))
    n = m.vertex_normals
    assert n.dtype == np.float32 and n.shape == m.vertices.shape
    assert np.array_equal(n, vertex_normals_host(tris, m.faces, len(m.vertices))) and m.vertex_normals is n
    e = SimpleMesh(np.zeros((0, 3, 3), np.float32))
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3) and e.vertex_normals.shape == (0, 3)
    assert e.vertex_normals.dtype == np.float32
    # a list, and a CPU tensor, are arrays too
    import torch
    assert SimpleMesh(tris.tolist()).vertices.shape == m.vertices.shape
    assert SimpleMesh(torch.from_numpy(tris)).device_triangles is None


def _obj_by_loops(mesh):
    """dump_meshes as it was written before the formatting went in bulk: a write per line."""
    verts, faces = mesh.vertices, mesh.faces + 1
    out = ["# zeroshape_amd mesh: %d vertices, %d faces\n" % (len(verts), len(faces))]
    for v in verts:
        out.append("v %.6f %.6f %.6f\n" % tuple(v))
    for t in faces:
        out.append("f %d %d %d\n" % tuple(t))
    return "".join(out)


def test_dump_meshes_text(tmp_path):
    """Default: byte-identical to the per-line loops.  normals=True: the same header and vertex lines, then one vn line per
    vertex and faces as a//a b//b c//c with the same indices."""
    soup = _sphere_soup()
    awkward = np.array([[[0.0, -0.0, 1e-7], [-1.5, 1234.5678, 0.1], [1e10, -2.5e-7, 0.3333333]]], np.float32)
    meshes = [SimpleMesh(soup), SimpleMesh(np.zeros((0, 3, 3), np.float32)), SimpleMesh(awkward)]
    opt = edict(output_path=str(tmp_path))
    V.dump_meshes(opt, ["a", "b", "c"], "mesh", meshes, folder="dump")
    V.dump_meshes(opt, ["a", "b", "c"], "mesh_n", meshes, folder="dump", normals=True)
    for i, mesh in zip("abc", meshes):
        plain = (tmp_path / "dump" / ("%s_mesh.obj" % i)).read_bytes()
        assert plain == _obj_by_loops(mesh).encode()
        lines = (tmp_path / "dump" / ("%s_mesh_n.obj" % i)).read_text().splitlines()
        nv, nf = len(mesh.vertices), len(mesh.faces)
        assert len(lines) == 1 + 2 * nv + nf
        assert lines[:1 + nv] == plain.decode().splitlines()[:1 + nv]
        vn = lines[1 + nv:1 + 2 * nv]
        assert all(ln.startswith("vn ") for ln in vn)
        assert vn == ["vn %.6f %.6f %.6f" % tuple(x) for x in mesh.vertex_normals]
        assert lines[1 + 2 * nv:] == ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in (mesh.faces + 1)]
        assert sum(ln.startswith("v ") for ln in lines) == nv


def test_weld_arguments_are_checked_before_anything_is_touched():
    """0 + a message that starts with the entry point's name, or 1 for an empty problem, before any pointer is dereferenced
    or anything is launched (a 64-byte host buffer stands in for every non-null pointer)."""
    from zeroshape_amd import _lib, build
    build.build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)

    def weld(n=5, tris=p, faces=p, n_verts=p, scratch=p):
        return lib.zs_mesh_weld(tris, n, faces, n_verts, scratch, None)

    def verts(n=5, tris=p, scratch=p, n_verts=7, vertices=p, normals=p):
        return lib.zs_mesh_weld_vertices(tris, n, scratch, n_verts, vertices, normals, None)

    def fails(name, rc, what):
        assert rc == 0, (name, what)
        msg = lib.zs_last_error()
        assert msg.startswith(name.encode() + b": ") and what.encode() in msg, (name, what, msg)

    fails("zs_mesh_weld", weld(n=-1), "negative")
    fails("zs_mesh_weld", weld(n=2 ** 29 + 1), "too large")
    for name in ("tris", "faces", "n_verts", "scratch"):
        fails("zs_mesh_weld", weld(**{name: None}), "null")
    fails("zs_mesh_weld", weld(scratch=odd), "8-byte aligned")
    assert weld(n=0) == 1 and weld(n=0, tris=None, faces=None, n_verts=None, scratch=None) == 1
    assert buf.raw == b"\0" * 64                                   # n_tris == 0: nothing written, the count included

    fails("zs_mesh_weld_vertices", verts(n=-1), "negative")
    fails("zs_mesh_weld_vertices", verts(n_verts=-1), "negative")
    fails("zs_mesh_weld_vertices", verts(n=2 ** 29 + 1), "too large")
    fails("zs_mesh_weld_vertices", verts(n_verts=16), "bad vertex count")
    for name in ("tris", "scratch", "vertices"):
        fails("zs_mesh_weld_vertices", verts(**{name: None}), "null")
    fails("zs_mesh_weld_vertices", verts(scratch=odd), "8-byte aligned")
    assert verts(n=0) == 1 and verts(n_verts=0) == 1
    assert verts(n=0, tris=None, scratch=None, n_verts=0, vertices=None, normals=None) == 1

    assert lib.zs_mesh_weld_scratch_bytes(0) == 0 and lib.zs_mesh_weld_scratch_bytes(-3) == 0
    assert lib.zs_mesh_weld_scratch_bytes(2 ** 29 + 1) == 0
