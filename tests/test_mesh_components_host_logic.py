"""CPU: eval_3D.mesh_components_host - the definition of the mesh-component quantities and the checker of
csrc/mesh_components.hip - against an independent computation (scipy's connected components, np.unique edge counting,
np.bincount sums) on marching-cubes soups of the oracle with known answers and on hand-written soups; filter_components on
host meshes; the options; SimpleMesh's trimesh-named properties."""
import functools

import numpy as np
import pytest

from oracle import mc_ref
from tests.test_oracle_mc import _sphere
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import options
from zeroshape_amd.utils.options import EasyDict as edict

THRESHOLDS = (0.02, 0.1, 1.0)


def volume_of(name):
    """The level grids of the cases: those of tests/test_oracle_mc.py / tests/test_gpu_mesh_weld.py, and scene25 - a solid with
    a cavity and a floater."""
    if name.startswith("noise"):
        G = int(name[5:])
        return np.random.RandomState(G).uniform(0, 1, (G, G, G)).astype(np.float32)
    if name == "sphere17":
        return _sphere(17, 0.8)[0]
    if name == "sphere17_clipped":
        return _sphere(17, 0.8, (1.2, 0, 0))[0]
    if name == "three_valued":
        return np.random.RandomState(5).choice([0, 0.5, 1], (9, 9, 9)).astype(np.float32)
    assert name == "scene25"
    G = 25
    big = _sphere(G, 0.9, (0, 0, 0))[0]
    hole = _sphere(G, 0.35, (0.05, 0, 0))[0]
    fl = _sphere(G, 0.2, (1.15, 1.1, -1.1))[0]
    return np.maximum(np.minimum(big, 1 - hole), fl).astype(np.float32)


#         F, V, degenerate, components, E, boundary, non-manifold, misoriented
KNOWN = {
    "sphere17": (676, 340, 0, 1, 1014, 0, 0, 0),
    "sphere17_clipped": (492, 261, 0, 1, 752, 28, 0, 0),
    "scene25": (2308, 1160, 0, 3, 3462, 0, 0, 0),
    "noise9": (1655, 1009, 0, 18, 2688, 411, 0, 0),
    "noise23": (34278, 17471, 0, 136, 52799, 2916, 76, 0),
    "noise45": (271874, 133260, 0, 921, 413130, 11566, 464, 0),
    "three_valued": (1156, 594, 141, 4, 1618, 278, 45, 0),
}
CASES = list(KNOWN)


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(the oracle's soup, its numpy-welded SimpleMesh, the checker's result) - computed once, changed by nobody."""
    vol = volume_of(name)
    G = vol.shape[0]
    soup = mc_ref.marching_cubes(vol, 0.5, np.float32(3.0 / G), np.float32(-1.5)).astype(np.float32)
    mesh = E.SimpleMesh(soup)
    return soup, mesh, E.mesh_components_host(mesh.vertices, mesh.faces, soup)


def independent(soup, faces, n_vertices):
    """The same quantities another way: scipy's connected components over the face graph, np.unique over sorted vertex pairs,
    np.linalg / np.cross for the terms."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64)
    rows, cols = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_vertices, n_vertices))
    n, raw = connected_components(graph, directed=False)
    # renumber by smallest vertex index
    smallest = np.full(n, n_vertices, np.int64)
    np.minimum.at(smallest, raw, np.arange(n_vertices))
    rank = np.empty(n, np.int64)
    rank[np.argsort(smallest)] = np.arange(n)
    vlab = rank[raw]
    flab = vlab[f[:, 0]] if len(f) else np.zeros(0, np.int64)
    deg = np.array([len(set(row)) < 3 for row in f.tolist()], bool)
    good = f[~deg]
    half = np.concatenate([good[:, [0, 1]], good[:, [1, 2]], good[:, [2, 0]]])
    und, inv, uses = np.unique(np.sort(half, axis=1), axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    fwd = np.zeros(len(und), np.int64)
    np.add.at(fwd, inv, (half[:, 0] < half[:, 1]).astype(np.int64))
    elab = vlab[und[:, 0]] if len(und) else np.zeros(0, np.int64)
    out = dict(n=n, vlab=vlab, flab=flab)
    out["faces"] = np.bincount(flab, minlength=n)
    out["vertices"] = np.bincount(vlab, minlength=n)
    out["degenerate_faces"] = np.bincount(flab[deg], minlength=n)
    out["edges"] = np.bincount(elab, minlength=n)
    out["boundary_edges"] = np.bincount(elab[uses == 1], minlength=n)
    out["nonmanifold_edges"] = np.bincount(elab[uses > 2], minlength=n)
    out["misoriented_edges"] = np.bincount(elab[(uses == 2) & ((fwd == 0) | (fwd == 2))], minlength=n)
    t = np.asarray(soup, np.float32).astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    vol = np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])) / 6.0
    area[deg], vol[deg] = 0.0, 0.0
    out["area"] = np.bincount(flab, weights=area, minlength=n)
    out["signed_volume"] = np.bincount(flab, weights=vol, minlength=n)
    out["abs_area"], out["abs_volume"] = out["area"], np.bincount(flab, weights=np.abs(vol), minlength=n)
    return out


@pytest.mark.parametrize("name", CASES)
def test_host_checker_against_an_independent_computation(name):
    soup, mesh, got = host_case(name)
    want = independent(soup, mesh.faces, len(mesh.vertices))
    F, V, D, C, Ed, B, N, M = KNOWN[name]
    assert (len(soup), len(mesh.vertices), got.n_components) == (F, V, C)
    assert (int(got.degenerate_faces.sum()), int(got.edges.sum()), int(got.boundary_edges.sum()),
            int(got.nonmanifold_edges.sum()), int(got.misoriented_edges.sum())) == (D, Ed, B, N, M)
    assert got.n_components == want["n"]
    assert got.vertex_labels.dtype == np.int32 and got.face_labels.dtype == np.int32 and got.counts.dtype == np.int32
    assert got.area.dtype == np.float64 and got.signed_volume.dtype == np.float64 and got.closed.dtype == bool
    assert np.array_equal(got.vertex_labels, want["vlab"]) and np.array_equal(got.face_labels, want["flab"])
    for col in ("faces", "vertices", "degenerate_faces", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges"):
        assert np.array_equal(getattr(got, col), want[col]), col
    assert np.array_equal(got.euler, want["vertices"] - want["edges"] + want["faces"] - want["degenerate_faces"])
    assert np.array_equal(got.closed, (want["faces"] > want["degenerate_faces"]) & (want["boundary_edges"] == 0)
                          & (want["nonmanifold_edges"] == 0) & (want["misoriented_edges"] == 0))
    # the same float64 terms up to the rounding of another formula (a few ulp each), added in the same order
    assert np.all(np.abs(got.area - want["area"]) <= 1e-12 * want["abs_area"] + 1e-300)
    assert np.all(np.abs(got.signed_volume - want["signed_volume"]) <= 1e-12 * want["abs_volume"] + 1e-300)
    # labels ascend with the components' smallest vertex
    first = [int(np.flatnonzero(got.vertex_labels == c)[0]) for c in range(min(got.n_components, 20))]
    assert first == sorted(first) and (not first or first[0] == 0)


def test_known_measures():
    _, mesh, sphere = host_case("sphere17")
    assert sphere.closed.tolist() == [True] and abs(sphere.signed_volume[0] - 1.7316) < 5e-5
    assert mesh.is_watertight and mesh.euler_number == 2 and abs(mesh.volume - 1.7316) < 5e-5
    assert abs(mesh.area - sphere.area[0]) == 0.0
    _, clipped, comps = host_case("sphere17_clipped")
    assert not clipped.is_watertight and comps.closed.tolist() == [False]
    _, scene, comps = host_case("scene25")
    assert comps.faces.tolist() == [288, 1928, 92] and comps.closed.tolist() == [True] * 3
    assert np.allclose(comps.area, [1.3619, 9.3276, 0.4081], atol=5e-5)
    assert np.allclose(comps.signed_volume, [-0.1468, 2.6692, 0.0232], atol=5e-5)
    assert scene.is_watertight and scene.euler_number == 6
    assert abs(scene.area - comps.area.sum()) == 0.0 and abs(scene.volume - comps.signed_volume.sum()) == 0.0
    ratio = comps.area / comps.area.max()
    assert np.allclose(ratio, [0.146, 1.0, 0.0438], atol=5e-4)
    # a summation-order difference cannot decide what a threshold keeps: every ratio is far from every threshold (the largest
    # component's own ratio is max / max = 1 in any order, and it is compared with 1.0 * max exactly)
    assert ratio[1] == 1.0
    for th in THRESHOLDS:
        assert np.all(np.abs(np.delete(ratio, 1) - th) >= 1e-6)
    assert scene.components is scene.components                                  # cached


# ---- hand-written soups ----

TET = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
OUTWARD = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]


def _tet(offset, inward=False):
    faces = np.array(OUTWARD)[:, ::-1] if inward else np.array(OUTWARD)
    return (TET + np.float32(offset))[faces]


def hand_soups():
    """name -> (soup [n,3,3] float32, expectations)."""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    out = {}
    # two triangles that share one vertex: one component
    out["bow_tie"] = (np.stack([tri, np.array([[0, 0, 0], [-1, 0, 0], [0, -1, 0]], np.float32)]),
                      dict(n=1, faces=[2], vertices=[5], edges=[6], boundary_edges=[6], misoriented_edges=[0], euler=[1],
                           closed=[False]))
    # two triangles over the edge (0,0,0) -> (1,0,0), both running through it in that direction
    out["misoriented"] = (np.stack([tri, np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0]], np.float32)]),
                          dict(n=1, faces=[2], vertices=[4], edges=[5], boundary_edges=[4], misoriented_edges=[1], closed=[False]))
    out["tets"] = (np.concatenate([_tet(0.0), _tet(5.0, inward=True)]),
                   dict(n=2, faces=[4, 4], vertices=[4, 4], edges=[6, 6], boundary_edges=[0, 0], euler=[2, 2],
                        closed=[True, True], signed_volume=[1.0 / 6, -1.0 / 6]))
    # a face with a repeated vertex beside a proper one
    out["repeated_index"] = (np.stack([tri, np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)]),
                             dict(n=1, faces=[2], vertices=[3], degenerate_faces=[1], edges=[3], boundary_edges=[3], euler=[1],
                                  closed=[False], area=[0.5], signed_volume=[0.0]))
    out["all_degenerate"] = (np.array([[[0, 0, 0], [0, 0, 0], [1, 0, 0]], [[2, 2, 2], [2, 2, 2], [2, 2, 2]]], np.float32),
                             dict(n=2, faces=[1, 1], vertices=[2, 1], degenerate_faces=[1, 1], edges=[0, 0], boundary_edges=[0, 0],
                                  euler=[2, 1], closed=[False, False], area=[0.0, 0.0], signed_volume=[0.0, 0.0]))
    out["empty"] = (np.zeros((0, 3, 3), np.float32), dict(n=0))
    return out


def check_hand_soup(comps, expect):
    assert comps.n_components == expect["n"]
    for key, want in expect.items():
        if key == "n":
            continue
        got = getattr(comps, key)
        if key in ("area", "signed_volume"):
            assert np.allclose(got, want, rtol=1e-12, atol=0), (key, got)
            assert all(g == 0.0 for g, w in zip(got, want) if w == 0.0), (key, got)     # degenerate terms: exactly zero
        else:
            assert got.tolist() == want, (key, got)


@pytest.mark.parametrize("name", sorted(hand_soups()))
def test_hand_written_soups(name):
    soup, expect = hand_soups()[name]
    mesh = E.SimpleMesh(soup)
    comps = mesh.components
    check_hand_soup(comps, expect)
    assert comps.device_counts is None
    assert comps.vertex_labels.shape == (len(mesh.vertices),) and comps.face_labels.shape == (len(soup),)
    if name == "tets":
        only_solid = E.filter_components(mesh, drop_cavities=True)
        assert np.array_equal(only_solid.triangles, soup[:4]) and only_solid.is_watertight and only_solid.volume > 0
        assert len(E.filter_components(mesh).triangles) == 8
    if name in ("empty", "all_degenerate"):
        assert not mesh.is_watertight
    if name == "empty":
        assert mesh.area == 0.0 and mesh.volume == 0.0 and mesh.euler_number == 0
        assert len(E.filter_components(mesh, 0.5, True).triangles) == 0
        assert comps.counts.shape == (0, 8) and comps.area.shape == (0,) and comps.closed.shape == (0,)


# ---- filter_components on host meshes ----

def expected_selection(comps, threshold, drop_cavities):
    kept = comps.area >= threshold * comps.area.max()
    if drop_cavities:
        kept &= ~(comps.closed & (comps.signed_volume < 0))
    return kept


SCENE_KEPT = {(0.02, False): [0, 1, 2], (0.02, True): [1, 2], (0.1, False): [0, 1], (0.1, True): [1],
              (1.0, False): [1], (1.0, True): [1]}


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("drop_cavities", [False, True])
def test_filter_components_on_the_host(threshold, drop_cavities):
    soup, mesh, comps = host_case("scene25")
    kept = expected_selection(comps, threshold, drop_cavities)
    assert np.flatnonzero(kept).tolist() == SCENE_KEPT[(threshold, drop_cavities)]
    out = E.filter_components(mesh, min_component_area=threshold, drop_cavities=drop_cavities)
    assert isinstance(out, E.SimpleMesh) and out.device_triangles is None
    sub = soup[kept[comps.face_labels]]
    assert out.triangles.dtype == np.float32 and np.array_equal(out.triangles.view(np.uint32), sub.view(np.uint32))
    want = E.SimpleMesh(sub)
    assert np.array_equal(out.vertices.view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(out.faces, want.faces)
    assert out.components.n_components == int(kept.sum())
    assert out.components.faces.tolist() == comps.faces[kept].tolist()


def test_filter_components_keep_and_argument_checks():
    soup, mesh, comps = host_case("scene25")
    floater = E.filter_components(mesh, keep=[2])
    assert np.array_equal(floater.triangles, soup[comps.face_labels == 2]) and len(floater.triangles) == 92
    assert len(E.filter_components(mesh, keep=[]).triangles) == 0
    assert len(E.filter_components(mesh).triangles) == len(soup)                 # no rule: everything
    for bad in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="min_component_area"):
            E.filter_components(mesh, min_component_area=bad)
    with pytest.raises(ValueError, match="keep"):
        E.filter_components(mesh, keep=[3])


# ---- options ----

def test_both_options_pass_the_safe_check(tmp_path):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = options.parse_arguments(["--yaml=%s/options/shape.yaml" % root, "--output_root=%s" % tmp_path,
                                   "--eval.min_component_area=0.05", "--eval.drop_cavities"])
    opt = options.set(cmd, safe_check=True, need_gpu=False)
    assert opt.eval.min_component_area == 0.05 and opt.eval.drop_cavities is True
    assert E._component_options(opt) == (0.05, True)
    plain = options.set(options.parse_arguments(["--yaml=%s/options/shape.yaml" % root, "--output_root=%s" % tmp_path]),
                        need_gpu=False)
    assert "min_component_area" not in plain.eval and "drop_cavities" not in plain.eval      # no yaml file carries them
    assert E._component_options(plain) is None
    opt = edict(dict(eval=dict(range=[-1.5, 1.5])))
    over = edict(dict(eval=dict(min_component_area=0.05, drop_cavities=True)))
    assert "eval.min_component_area" in options.COMMAND_LINE_ONLY and "eval.drop_cavities" in options.COMMAND_LINE_ONLY
    out = options.override_options(opt, over, safe_check=True)
    assert out.eval.min_component_area == 0.05 and out.eval.drop_cavities is True
    assert E._component_options(out) == (0.05, True)
    assert E._component_options(edict(dict(eval=dict(range=[-1.5, 1.5])))) is None
    assert E._component_options(edict(dict(eval=dict(drop_cavities=True)))) == (None, True)
    with pytest.raises(KeyError):
        options.override_options(edict(dict(eval=dict())), edict(dict(eval=dict(no_such_option=1))), safe_check=True)
