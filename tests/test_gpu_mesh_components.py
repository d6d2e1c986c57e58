"""GPU: the mesh-component kernels (csrc/mesh_components.hip) against their checker eval_3D.mesh_components_host - labels, the
count and every integer column equal, the fp64 sums within the bound of two summation orders of identical terms - on
marching-cubes soups, around the scan tile and the workgroup size, on a deep chain in three face orders and on hand-written
soups; the argument checks of the raw entry points; determinism; filter_components on the device against the host filter;
the opt-in through convert_to_explicit; demo.py's report."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from tests.test_mesh_components_host_logic import (CASES, KNOWN, SCENE_KEPT, THRESHOLDS, check_hand_soup, expected_selection,
                                                   hand_soups, volume_of)
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu

INT_COLUMNS = E.COMPONENT_COLUMNS


@functools.lru_cache(maxsize=None)
def _case(name):
    """(soup on the GPU, its host copy, the numpy-welded host mesh, the checker's result) - computed once, read by all."""
    tris, _ = E.extract_surface(torch.from_numpy(volume_of(name)).cuda(), 0.5, -1.5, 1.5)
    soup = tris.cpu().numpy()
    ref = E.SimpleMesh(soup)
    return tris, soup, ref, ref.components


def _assert_on_device(comps):
    for t, dtype in ((comps.device_vertex_labels, torch.int32), (comps.device_face_labels, torch.int32),
                     (comps.device_counts, torch.int32), (comps.device_measures, torch.float64)):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype
    assert comps.device_counts.shape == (comps.n_components, 8) and comps.device_measures.shape == (comps.n_components, 2)


def _assert_equals_checker(got, want, soup, faces, what=""):
    """Integers exactly; area and signed volume of component c within n_c * 2^-52 * sum_c |term| - two summation orders of
    the same n_c fp64 terms differ from the exact sum by at most (n_c - 1) * 2^-53 * sum |term| each (first order)."""
    _assert_on_device(got)
    assert got.n_components == want.n_components
    assert got.vertex_labels.dtype == np.int32 and np.array_equal(got.vertex_labels, want.vertex_labels)
    assert got.face_labels.dtype == np.int32 and np.array_equal(got.face_labels, want.face_labels)
    for k, col in enumerate(INT_COLUMNS):
        assert np.array_equal(got.counts[:, k], want.counts[:, k]), col
    assert np.array_equal(got.closed, want.closed)
    area_t, vol_t = E.mesh_face_terms_host(soup, faces)
    C = want.n_components
    n_c = np.bincount(want.face_labels, minlength=C).astype(np.float64)
    worst = 0.0
    for mine, theirs, terms in ((got.area, want.area, area_t), (got.signed_volume, want.signed_volume, vol_t)):
        assert mine.dtype == np.float64 and mine.shape == theirs.shape
        bound = n_c * 2.0 ** -52 * np.bincount(want.face_labels, weights=np.abs(terms), minlength=C)
        err = np.abs(mine - theirs)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        worst = max(worst, float(ratio.max()) if C else 0.0)
        assert np.all(err <= bound), (what, float(ratio.max()))
    print("%s: %d components, worst |error| / bound = %.3g" % (what, C, worst))


@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_checker(name):
    tris, soup, ref, want = _case(name)
    F, Vn, D, C, Ed, B, N, M = KNOWN[name]                           # the device soup is the oracle's: the same known answers
    assert (len(soup), len(ref.vertices), want.n_components, int(want.edges.sum())) == (F, Vn, C, Ed)
    mesh = E.SimpleMesh(tris)
    got = mesh.components
    _assert_equals_checker(got, want, soup, ref.faces, name)
    assert mesh.components is got and mesh._device_weld is not None                 # cached; the weld is kept
    assert (int(got.degenerate_faces.sum()), int(got.boundary_edges.sum()), int(got.nonmanifold_edges.sum()),
            int(got.misoriented_edges.sum())) == (D, B, N, M)
    assert mesh.is_watertight == ref.is_watertight and mesh.euler_number == ref.euler_number
    # the totals: the components' bounds added up (at most F * 2^-52 * sum |term|; a volume term is at most |v0| / 3 < 0.87
    # of its face's area term inside the +-1.5 cube) plus the rounding of adding C numbers on either side
    tol = (F + 2 * C) * 2.0 ** -52 * ref.area
    assert abs(mesh.area - ref.area) <= tol and abs(mesh.volume - ref.volume) <= tol


@pytest.mark.parametrize("k", [1, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_disjoint_triangles_around_the_tile_sizes(k):
    """k triangles that touch nowhere: as many components as faces; triangle i has the vertices 3 i .. 3 i + 2 of the weld
    (ascending x), so its label is i."""
    soup = np.zeros((k, 3, 3), np.float32)
    soup[:, :, 0] = 3.0 * np.arange(k, dtype=np.float32)[:, None]
    soup[:, 1, 0] += 1.0
    soup[:, 2, 1] = 1.0
    got = E.SimpleMesh(torch.from_numpy(soup).cuda()).components
    _assert_on_device(got)
    assert got.n_components == k and np.array_equal(got.face_labels, np.arange(k))
    assert np.array_equal(got.vertex_labels, np.repeat(np.arange(k), 3))
    assert np.array_equal(got.counts, np.tile(np.array([[1, 3, 0, 3, 3, 0, 0, 1]], np.int32), (k, 1)))
    assert np.array_equal(got.area, np.full(k, 0.5)) and not got.signed_volume.any() and not got.closed.any()


def _strip(n):
    """A triangle strip of n faces over n + 2 vertices, consistently wound."""
    i = np.arange(n + 2)
    verts = np.stack([(i // 2).astype(np.float32), (i % 2).astype(np.float32), np.zeros(n + 2, np.float32)], axis=1)
    j = np.arange(n)
    faces = np.stack([np.where(j % 2 == 0, j, j + 1), np.where(j % 2 == 0, j + 1, j), j + 2], axis=1)
    return verts[faces]


@pytest.mark.parametrize("order", ["forward", "reversed", "permuted"])
def test_deep_chain(order):
    soup = _strip(5000)
    if order == "reversed":
        soup = soup[::-1].copy()
    elif order == "permuted":
        soup = soup[np.random.RandomState(7).permutation(len(soup))]
    ref = E.SimpleMesh(soup)
    got = E.SimpleMesh(torch.from_numpy(soup).cuda()).components
    _assert_equals_checker(got, ref.components, soup, ref.faces, "strip " + order)
    assert got.n_components == 1 and got.counts.tolist() == [[5000, 5002, 0, 10001, 5002, 0, 0, 1]]
    assert not got.vertex_labels.any() and not got.face_labels.any()


@pytest.mark.parametrize("name", sorted(hand_soups()))
def test_hand_written_soups_on_the_device(name):
    soup, expect = hand_soups()[name]
    ref = E.SimpleMesh(soup)
    mesh = E.SimpleMesh(torch.from_numpy(soup).cuda())
    got = mesh.components
    check_hand_soup(got, expect)
    _assert_equals_checker(got, ref.components, soup, ref.faces, name)
    assert got.vertex_labels.shape == (len(ref.vertices),) and got.face_labels.shape == (len(soup),)
    if name == "tets":
        solid = E.filter_components(mesh, drop_cavities=True)
        assert solid.device_triangles is not None and np.array_equal(solid.triangles, soup[:4]) and solid.is_watertight
    if name == "empty":
        assert got.counts.dtype == np.int32 and got.area.dtype == np.float64 and got.vertex_labels.dtype == np.int32
        assert not mesh.is_watertight and mesh.area == 0.0 and mesh.euler_number == 0
        out = E.filter_components(mesh, 0.5, True)
        assert out.device_triangles is not None and out.device_triangles.shape == (0, 3, 3)


def test_argument_checks_of_the_raw_entry_points():
    """0 and a message that names the entry point, before anything is launched (a host buffer stands in for every non-null
    pointer: nothing may read it); zero sizes return 1."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p, odd = ctypes.c_void_p(base + (-base) % 8), ctypes.c_void_p(base + (-base) % 8 + 4)

    def fails(name, rc, what):
        msg = lib.zs_last_error()
        assert rc == 0 and msg.startswith(name.encode() + b": ") and what.encode() in msg, (name, what, rc, msg)

    comp = lambda n, v, ptr=p, scratch=p: lib.zs_mesh_components(ptr, n, v, ptr, ptr, ptr, scratch, None)
    stats = lambda n, v, c, ptr=p, scratch=p: lib.zs_mesh_component_stats(ptr, ptr, ptr, ptr, n, v, c, ptr, ptr, scratch, None)
    select = lambda n, v, c, ptr=p, scratch=p, rel=0.5: lib.zs_mesh_components_select(ptr, ptr, c, rel, 0, None, ptr, n, v, ptr,
                                                                                       ptr, scratch, None)
    filt = lambda n, kept, ptr=p: lib.zs_mesh_filter_faces(ptr, ptr, n, ptr, kept, None)
    fails("zs_mesh_components", comp(-1, 3), "negative size")
    fails("zs_mesh_components", comp(1, -3), "negative size")
    fails("zs_mesh_components", comp(1, 4), "bad vertex count")
    fails("zs_mesh_components", comp(1, 3, None), "null pointer")
    fails("zs_mesh_components", comp(1, 3, p, None), "null pointer")
    fails("zs_mesh_components", comp(1, 3, p, odd), "8-byte aligned")
    assert comp(0, 0, None, None) == 1
    fails("zs_mesh_component_stats", stats(-1, 3, 1), "negative size")
    fails("zs_mesh_component_stats", stats(1, 3, -1), "negative size")
    fails("zs_mesh_component_stats", stats(1, 3, 4), "bad component count")
    fails("zs_mesh_component_stats", stats(1, 3, 1, None), "null pointer")
    fails("zs_mesh_component_stats", stats(1, 3, 1, p, odd), "8-byte aligned")
    assert stats(0, 0, 0, None, None) == 1 and stats(1, 3, 0, None, None) == 1
    fails("zs_mesh_components_select", select(-1, 3, 1), "negative size")
    fails("zs_mesh_components_select", select(1, 3, -1), "negative size")
    fails("zs_mesh_components_select", select(1, 3, 1, rel=1.5), "min_rel_area")
    fails("zs_mesh_components_select", select(1, 3, 1, rel=float("nan")), "min_rel_area")
    fails("zs_mesh_components_select", select(1, 3, 1, None), "null pointer")
    fails("zs_mesh_components_select", select(1, 3, 1, p, odd), "8-byte aligned")
    assert select(0, 0, 0, None, None) == 1
    fails("zs_mesh_filter_faces", filt(-1, 0), "negative size")
    fails("zs_mesh_filter_faces", filt(1, -1), "negative size")
    fails("zs_mesh_filter_faces", filt(1, 2), "bad count")
    fails("zs_mesh_filter_faces", filt(1, 1, None), "null pointer")
    assert filt(0, 0, None) == 1 and filt(5, 0, None) == 1
    assert lib.zs_mesh_components_scratch_bytes(0, 0) == 0 and lib.zs_mesh_components_scratch_bytes(-1, 3) == 0
    assert lib.zs_mesh_components_scratch_bytes(1, 4) == 0 and lib.zs_mesh_components_scratch_bytes(2 ** 29 + 1, 3) == 0
    assert lib.zs_mesh_components_scratch_bytes(1, 3) % 256 == 0 and lib.zs_mesh_components_scratch_bytes(1, 3) > 0


def test_two_runs_give_the_same_bits():
    tris = _case("noise23")[0]
    a, b = E.mesh_components(E.SimpleMesh(tris)), E.mesh_components(E.SimpleMesh(tris))
    for key in ("device_vertex_labels", "device_face_labels", "device_counts"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert torch.equal(a.device_measures.view(torch.int64), b.device_measures.view(torch.int64))


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("drop_cavities", [False, True])
def test_filtering_on_the_device(threshold, drop_cavities):
    tris, soup, ref, want = _case("scene25")
    kept = expected_selection(want, threshold, drop_cavities)
    assert np.flatnonzero(kept).tolist() == SCENE_KEPT[(threshold, drop_cavities)]
    host = E.filter_components(ref, min_component_area=threshold, drop_cavities=drop_cavities)
    out = E.filter_components(E.SimpleMesh(tris), min_component_area=threshold, drop_cavities=drop_cavities)
    assert isinstance(out, E.SimpleMesh) and out.device_triangles is not None and out.device_triangles.is_cuda
    assert out.device_triangles.dtype == torch.float32 and out._triangles is None
    assert np.array_equal(out.triangles.view(np.uint32), host.triangles.view(np.uint32))
    assert np.array_equal(out.triangles.view(np.uint32), soup[kept[want.face_labels]].view(np.uint32))
    assert np.array_equal(out.vertices.view(np.uint32), host.vertices.view(np.uint32)) and np.array_equal(out.faces, host.faces)
    assert out.components.n_components == int(kept.sum()) and out.components.faces.tolist() == want.faces[kept].tolist()


def test_filtering_keep_nothing_and_empty():
    tris, soup, ref, want = _case("scene25")
    mesh = E.SimpleMesh(tris)
    floater = E.filter_components(mesh, keep=[2])
    assert floater.device_triangles.shape == (92, 3, 3) and np.array_equal(floater.triangles, soup[want.face_labels == 2])
    both = E.filter_components(mesh, keep=[2, 0])
    assert np.array_equal(both.triangles, soup[want.face_labels != 1])                  # soup order, not the order of `keep`
    for nothing in (E.filter_components(mesh, keep=[]),
                    E.filter_components(E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda")), 0.1, True)):
        assert nothing.device_triangles.shape == (0, 3, 3) and nothing.device_triangles.is_cuda
        assert nothing.vertices.shape == (0, 3) and nothing.components.n_components == 0
    # a rule that keeps nothing: the cavity alone, then cavities dropped
    cavity = E.filter_components(mesh, keep=[0])
    assert cavity.volume < 0 and len(E.filter_components(cavity, drop_cavities=True).triangles) == 0
    with pytest.raises(ValueError, match="min_component_area"):
        E.filter_components(mesh, min_component_area=1.5)
    with pytest.raises(ValueError, match="keep"):
        E.filter_components(mesh, keep=[3])


def _opt(tmp_path, **extra):
    return edict(dict(device="cuda", output_path=str(tmp_path), eval=dict(range=[-1.5, 1.5], num_points=2000, **extra)))


def test_through_the_pipeline(tmp_path):
    vol = torch.from_numpy(volume_of("scene25")).cuda()
    tris, soup, ref, want = _case("scene25")
    meshes, clouds = E.convert_to_explicit(_opt(tmp_path, min_component_area=0.1, drop_cavities=True), [vol], 0.5,
                                           to_pointcloud=True, seed=3)
    solid = meshes[0]
    assert solid.device_triangles.shape == (1928, 3, 3) and np.array_equal(solid.triangles, soup[want.face_labels == 1])
    again = E.sample_surface(solid.device_triangles, 2000, 3).cpu().numpy()
    assert clouds.dtype == np.float64 and clouds.shape == (1, 2000, 3) and np.array_equal(clouds[0], again.astype(np.float64))
    # the solid alone: a sphere of radius 0.9 * 24/25 in marching cubes' coordinates, one grid step = 3/25
    dist = np.linalg.norm(clouds[0], axis=1)
    print("distance from the origin: %.4f .. %.4f" % (dist.min(), dist.max()))
    assert np.all(np.abs(dist - 0.9 * 24 / 25) <= 3.0 / 25)
    centre = -1.5 + (np.array([1.15, 1.1, -1.1]) + 1.5) * 24 / 25                      # the floater's, in those coordinates
    assert np.linalg.norm(clouds[0] - centre, axis=1).min() > 0.5
    # options absent = today's calls; a threshold below every ratio with cavities kept changes nothing
    plain_m, plain_c = E.convert_to_explicit(_opt(tmp_path), [vol], 0.5, to_pointcloud=True, seed=3)
    same_m, same_c = E.convert_to_explicit(_opt(tmp_path, min_component_area=0.02), [vol], 0.5, to_pointcloud=True, seed=3)
    assert plain_m[0]._components is None                                               # nothing labelled when not asked for
    assert torch.equal(plain_m[0].device_triangles, tris) and torch.equal(same_m[0].device_triangles, tris)
    assert np.array_equal(plain_c, same_c) and np.linalg.norm(plain_c[0] - centre, axis=1).min() < 0.3     # on the floater
    # the evaluation's own route: the same mesh and the same points
    meshes2, cloud2 = E._surface_clouds(_opt(tmp_path, min_component_area=0.1, drop_cavities=True), vol[None], seed=3)
    assert torch.equal(meshes2[0].device_triangles, solid.device_triangles) and cloud2.is_cuda
    assert np.array_equal(cloud2[0].cpu().numpy(), again)
    plain2 = E._surface_clouds(_opt(tmp_path), vol[None], seed=3)[1]
    assert np.array_equal(plain2[0].cpu().numpy().astype(np.float64), plain_c[0])


def test_demo_report_and_filtered_obj(tmp_path):
    """demo.py's pieces on an analytic scene at vox 32 (a 33^3 grid: solid, cavity, floater): the report's totals are the
    object's, and the .obj written for a filtered mesh is the filtered mesh."""
    from tests.test_oracle_mc import _sphere
    G = 33
    scene = np.maximum(np.minimum(_sphere(G, 0.9, (0, 0, 0))[0], 1 - _sphere(G, 0.35, (0.05, 0, 0))[0]),
                       _sphere(G, 0.2, (1.15, 1.1, -1.1))[0]).astype(np.float32)
    vol = torch.from_numpy(scene).cuda()
    opt = _opt(tmp_path, min_component_area=0.1, drop_cavities=True)
    whole = E.convert_to_explicit(_opt(tmp_path), [vol], 0.5)[0]
    mesh = E.convert_to_explicit(opt, [vol], 0.5)[0]
    assert whole.components.n_components == 3 and mesh.components.n_components == 1
    V.dump_meshes(opt, ["a"], "mesh", [mesh], folder="preds")
    V.dump_mesh_reports(opt, ["a"], "mesh_report", [mesh], folder="preds")
    V.dump_mesh_reports(opt, ["w"], "mesh_report", [whole], folder="preds")
    obj = (tmp_path / "preds" / "a_mesh.obj").read_bytes()
    solid = int(np.argmax(whole.components.area))
    assert obj.count(b"\nv ") == len(mesh.vertices) == int(whole.components.vertices[solid])
    assert obj.count(b"\nf ") == len(mesh.faces) == int(whole.components.faces[solid])
    report = json.loads((tmp_path / "preds" / "a_mesh_report.json").read_text())
    assert report["area"] == mesh.area and report["volume"] == mesh.volume and report["euler_number"] == mesh.euler_number == 2
    assert report["is_watertight"] is True and report["components"] == 1 and report["faces"] == len(mesh.faces)
    assert report["vertices"] == len(mesh.vertices) and len(report["component_table"]) == 1
    assert report["component_table"][0]["closed"] is True and report["component_table"][0]["edges"] == 3 * len(mesh.faces) // 2
    full = json.loads((tmp_path / "preds" / "w_mesh_report.json").read_text())
    assert full["components"] == 3 and full["euler_number"] == 6 and full["area"] == whole.area
    assert [row["faces"] for row in full["component_table"]] == whole.components.faces.tolist()
    assert sum(row["signed_volume"] < 0 for row in full["component_table"]) == 1
