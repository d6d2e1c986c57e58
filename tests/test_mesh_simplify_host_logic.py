"""CPU: eval_3D.simplify_mesh_host - the definition of simplify_mesh and the checker of csrc/mesh_simplify.hip - on the
marching-cubes soups of the oracle (structure of the output, the counts, the distance bound, the cluster assignment against an
independent computation, the identity at a tiny cell, one cluster at a huge one), on hand-written soups with exact answers,
and on a 65^3 sphere's volume under the two placements; simplify_mesh on host meshes, mesh_report, the options, the
pipelines."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import mc_ref
from tests.test_mesh_components_host_logic import KNOWN, host_case, volume_of
from tests.test_oracle_mc import _sphere
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import options
from zeroshape_amd.utils.options import EasyDict as edict

CASES = list(KNOWN)
POSITIONS = ("quadric", "mean")


def grid_of(name, cells):
    """(cell, origin) the way the pipelines set them: ``cells`` marching-cubes cells, planes half a cell below the range."""
    edge = 3.0 / volume_of(name).shape[0]
    return cells * edge, (-1.5 - 0.5 * edge,) * 3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def simplified(name, cells, position):
    _, mesh, _ = host_case(name)
    cell, origin = grid_of(name, cells)
    return E.simplify_mesh_host(mesh.vertices, mesh.faces, origin, cell, position)


def rotated(ids):
    """Rows of three ids, the smallest first, the cyclic order kept (independent of the checker: np.roll row by row)."""
    return np.array([np.roll(row, -int(np.argmin(row))) for row in np.asarray(ids).reshape(-1, 3)], np.int64).reshape(-1, 3)


@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("cells", [2, 3])
@pytest.mark.parametrize("name", CASES)
def test_structure_counts_and_distance(name, cells, position):
    _, mesh, _ = host_case(name)
    cell, origin = grid_of(name, cells)
    got = simplified(name, cells, position)
    F, V = len(mesh.faces), len(mesh.vertices)
    counts = got.counts
    assert got.triangles.dtype == np.float32 and got.triangles.shape == (counts["kept"], 3, 3)
    assert got.representatives.dtype == np.float32 and got.representatives.shape == (counts["clusters"], 3)
    assert got.cluster_of.shape == (V,) and got.kept.shape == (F,) and int(got.kept.sum()) == counts["kept"]
    # counts
    assert counts["kept"] + counts["degenerate"] + counts["duplicate"] == F
    assert 0 < counts["clusters"] < V and 0 < counts["kept"] < F
    assert len(np.unique(got.triangles.reshape(-1, 3), axis=0)) <= counts["clusters"]
    assert counts["fallbacks"] == int(got.fell_back.sum()) and (position == "quadric" or counts["fallbacks"] == 0)
    # faces: no repeated vertex, no two equal up to rotation; the soup is the representatives through the kept faces
    ids = got.cluster_of[mesh.faces[got.kept]]
    assert np.all((ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2]))
    assert len(np.unique(rotated(ids), axis=0)) == len(ids)
    assert np.array_equal(bits(got.triangles), bits(got.representatives[ids]))
    # every dropped face is degenerate or repeats a kept one that comes before it
    all_ids = got.cluster_of[mesh.faces]
    degenerate = (all_ids[:, 0] == all_ids[:, 1]) | (all_ids[:, 1] == all_ids[:, 2]) | (all_ids[:, 0] == all_ids[:, 2])
    assert int(degenerate.sum()) == counts["degenerate"] and not got.kept[degenerate].any()
    first_of = {}
    for f in np.flatnonzero(~degenerate):
        first_of.setdefault(tuple(np.roll(all_ids[f], -int(np.argmin(all_ids[f])))), f)
    assert np.array_equal(np.flatnonzero(got.kept), sorted(first_of.values()))
    # the distance bound, per axis, up to the float32 rounding of the representative
    moved = np.abs(mesh.vertices.astype(np.float64) - got.representatives[got.cluster_of].astype(np.float64))
    slack = 2.0 * np.finfo(np.float32).eps * np.abs(mesh.vertices).max()
    assert moved.max() <= 1.5 * cell + slack
    if position == "mean":
        assert moved.max() <= 1.0 * cell + slack                                  # both lie in one cell


@pytest.mark.parametrize("cells", [2, 3])
@pytest.mark.parametrize("name", CASES)
def test_cluster_assignment_against_unique_rows(name, cells):
    _, mesh, _ = host_case(name)
    cell, origin = grid_of(name, cells)
    got = simplified(name, cells, "quadric")
    rows = np.floor((mesh.vertices.astype(np.float64) - np.asarray(origin)) / cell).astype(np.int64)
    cells_used, inverse = np.unique(rows, axis=0, return_inverse=True)               # lexicographic: the key's order
    assert len(cells_used) == got.counts["clusters"] and np.array_equal(inverse.reshape(-1), got.cluster_of)
    assert np.array_equal(got.cluster_of, simplified(name, cells, "mean").cluster_of)
    # a cluster of one vertex keeps that vertex's bits, in both placements
    size = np.bincount(got.cluster_of)
    alone = np.flatnonzero(size[got.cluster_of] == 1)
    for position in POSITIONS:
        reps = simplified(name, cells, position).representatives
        assert np.array_equal(bits(reps[got.cluster_of[alone]]), bits(mesh.vertices[alone]))
    # the mean placement against a plain float64 mean (other order of additions: close, not equal)
    mean = np.stack([np.bincount(got.cluster_of, mesh.vertices[:, a].astype(np.float64)) for a in range(3)], axis=1) / size[:, None]
    assert np.abs(simplified(name, cells, "mean").representatives - mean).max() <= 4e-7


@pytest.mark.parametrize("name", ["sphere17", "scene25"])
def test_a_cell_per_vertex_returns_the_input(name):
    soup, mesh, _ = host_case(name)
    cell, origin = grid_of(name, 0.001)
    for position in POSITIONS:
        got = E.simplify_mesh_host(mesh.vertices, mesh.faces, origin, cell, position)
        assert got.counts == dict(kept=len(soup), clusters=len(mesh.vertices), degenerate=0, duplicate=0, fallbacks=0)
        assert got.triangles.shape == soup.shape and np.array_equal(bits(got.triangles), bits(soup))


@pytest.mark.parametrize("name", CASES)
def test_one_cluster_gives_the_empty_mesh(name):
    soup, mesh, _ = host_case(name)
    cell, origin = grid_of(name, 100)
    out = E.simplify_mesh(mesh, cell, origin)
    s = out.simplification
    assert out.triangles.shape == (0, 3, 3) and out.vertices.shape == (0, 3)
    assert (s.kept_faces, s.clusters, s.degenerate_faces, s.duplicate_faces, s.input_faces) == (0, 1, len(soup), 0, len(soup))


# ---- hand-written soups ----

def _grid_patch(nx, ny, point):
    """An nx x ny grid of vertices point(i, j), two triangles per square, consistently wound -> (vertices, faces)."""
    verts = np.array([point(i, j) for i in range(nx) for j in range(ny)], np.float32)
    faces = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            a, b, c, d = i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1
            faces += [[a, b, c], [a, c, d]]
    return verts, np.array(faces, np.int64)


def hand_cases():
    """name -> (vertices [V,3] float32, faces [F,3], origin, cell)."""
    out = {}
    tet = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 2.5]], np.float32)
    tet_faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    out["tetrahedron"] = (tet, tet_faces, (0.0, 0.0, 0.0), 1.0)
    # two tetrahedra, the apex of each in the cell of its first vertex, the second in the cells of the first: each gives the
    # triples (a, c, b) and (b, c, a) - a triangle and its mirror image - and two faces that hold cell a twice
    one = np.array([[0.25, 0.25, 0.25], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 0.75]], np.float32)
    two = one + np.float32(0.125)
    out["two_tetrahedra"] = (np.concatenate([one, two]), np.concatenate([tet_faces, tet_faces + 4]), (0.0, 0.0, 0.0), 1.0)
    # a face, the same face rotated (a duplicate), and its mirror image (kept)
    out["twins"] = (tet[:3], np.array([[0, 1, 2], [1, 2, 0], [0, 2, 1]]), (0.0, 0.0, 0.0), 1.0)
    # a tilted plane at coordinates around 5: 13 x 13 vertices 0.3 apart, cells of 1
    out["plane"] = _grid_patch(13, 13, lambda i, j: (4.1 + 0.3 * i, 3.2 + 0.3 * j, 5.05 + 0.25 * (0.3 * i) - 0.15 * (0.3 * j))) + \
        ((0.0, 0.0, 0.0), 1.0)
    # two sheets through the same 3 x 3 cells, z = 0.3 and z = 0.5 + 0.2 x: they meet at x = -1, outside every cell's box
    lower, faces = _grid_patch(3, 3, lambda i, j: (0.25 + i, 0.25 + j, 0.3))
    upper, _ = _grid_patch(3, 3, lambda i, j: (0.25 + i, 0.25 + j, 0.5 + 0.2 * (0.25 + i)))
    out["crease"] = (np.concatenate([lower, upper]), np.concatenate([faces, faces + 9]), (0.0, 0.0, 0.0), 1.0)
    return out


def check_hand_case(name, run):
    """``run(vertices, faces, origin, cell, position)`` -> (soup [kept,3,3] float32, counts dict): the exact answers."""
    verts, faces, origin, cell = hand_cases()[name]
    soup = verts[faces]
    for position in POSITIONS:
        got, counts = run(verts, faces, origin, cell, position)
        assert counts["kept"] + counts["degenerate"] + counts["duplicate"] == len(faces) and len(got) == counts["kept"]
        if name == "tetrahedron":
            assert counts == dict(kept=4, clusters=4, degenerate=0, duplicate=0, fallbacks=0)
            assert np.array_equal(bits(got), bits(soup))
        elif name == "two_tetrahedra":
            assert counts["kept"] == 2 and counts["clusters"] == 3 and counts["degenerate"] == 4 and counts["duplicate"] == 2
            # faces 0 and 3 of the first tetrahedron: the same three representatives, wound both ways
            assert np.array_equal(bits(got[0]), bits(got[1][[2, 1, 0]])) or np.array_equal(bits(got[0][[0, 2, 1]]), bits(got[1]))
            assert len(np.unique(got.reshape(-1, 3), axis=0)) == 3
            # cells b and c hold two vertices each, 0.125 apart per axis: their mean is exact
            if position == "mean":
                assert np.array_equal(got[0][2], verts[1] + np.float32(0.0625)) and np.array_equal(got[0][1], verts[2] + np.float32(0.0625))
        elif name == "twins":
            assert counts == dict(kept=2, clusters=3, degenerate=0, duplicate=1, fallbacks=0)
            assert np.array_equal(bits(got), bits(soup[[0, 2]]))
        elif name == "plane":
            assert counts["fallbacks"] == 0 and counts["duplicate"] == 0 and 0 < counts["kept"] < len(faces)
            normal = np.array([0.25, -0.15, -1.0])
            p = got.reshape(-1, 3).astype(np.float64)
            off = np.abs((p - np.array([4.1, 3.2, 5.05])) @ normal) / np.linalg.norm(normal)
            # the input's own float32 vertices are off the real-valued plane by up to about an ulp of their coordinates (4 to
            # 8: one binade); a representative - a mean or a minimiser over such vertices, rounded once more - by a few
            assert off.max() <= 4 * np.spacing(np.float32(6.5))
        else:
            assert counts["clusters"] == 9 and counts["kept"] == 8 and counts["duplicate"] == 8 and counts["degenerate"] == 0
            assert counts["fallbacks"] == (9 if position == "quadric" else 0)
    return verts, faces, origin, cell


def run_host(vertices, faces, origin, cell, position):
    done = E.simplify_mesh_host(vertices, faces, origin, cell, position)
    return done.triangles, done.counts


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_written_soups(name):
    verts, faces, origin, cell = check_hand_case(name, run_host)
    if name == "crease":
        quadric = E.simplify_mesh_host(verts, faces, origin, cell, "quadric")
        mean = E.simplify_mesh_host(verts, faces, origin, cell, "mean")
        assert quadric.fell_back.all() and np.array_equal(bits(quadric.representatives), bits(mean.representatives))
        # the fallback was taken because the minimiser lies outside: without the pull to the mean, the two planes' quadric is
        # smallest on their line of intersection x = -1, more than a cell from every cell centre (x = 0.5, 1.5, 2.5)
        rows = np.array([[0.0, 0.0, 1.0, 0.3], [-0.2, 0.0, 1.0, 0.5]])
        on_the_line = np.linalg.lstsq(rows[:, [0, 2]], rows[:, 3], rcond=None)[0]
        assert abs(on_the_line[0] + 1.0) < 1e-12 and abs(on_the_line[1] - 0.3) < 1e-12
        # a gentler tilt, whose line x = 1.25 passes through the middle column's box: those clusters are placed, not averaged
        verts2 = verts.copy()
        verts2[9:, 2] = np.float32(0.3) + np.float32(0.2) * (verts2[9:, 0] - np.float32(1.25))
        placed = E.simplify_mesh_host(verts2, faces, origin, cell, "quadric")
        column = np.floor(verts2[:9, 0]).astype(int)[np.argsort(placed.cluster_of[:9])]        # the cell's x index, by cluster id
        assert not placed.fell_back[column == 1].any() and placed.counts["fallbacks"] < 9
        on_line = placed.representatives[column == 1].astype(np.float64)
        assert np.abs(on_line[:, 0] - 1.25).max() < 0.01 and np.abs(on_line[:, 2] - 0.3).max() < 0.01
    if name == "plane":
        assert E.simplify_mesh_host(verts, faces, origin, cell, "quadric").counts["clusters"] == 4 * 4 * 2 - 12


# ---- volume ----

def test_quadric_placement_keeps_the_volume_better_than_the_mean():
    vol = _sphere(65, 0.8)[0]
    edge = 3.0 / 65
    mesh = E.SimpleMesh(mc_ref.marching_cubes(vol, 0.5, np.float32(edge), np.float32(-1.5)).astype(np.float32))
    start = mesh.volume
    for cells in (2, 4):
        ratio = {p: E.simplify_mesh(mesh, cells * edge, (-1.5 - 0.5 * edge,) * 3, p).volume / start for p in POSITIONS}
        print("65^3 sphere, %d cells: volume ratio quadric %.5f, mean %.5f" % (cells, ratio["quadric"], ratio["mean"]))
        assert abs(ratio["quadric"] - 1.0) < abs(ratio["mean"] - 1.0)


# ---- simplify_mesh on host meshes ----

def test_simplify_mesh_returns_a_new_mesh_with_its_record():
    soup, mesh, _ = host_case("scene25")
    cell, origin = grid_of("scene25", 2)
    out = E.simplify_mesh(mesh, cell, origin)
    want = simplified("scene25", 2, "quadric")
    assert isinstance(out, E.SimpleMesh) and out is not mesh and out.device_triangles is None
    assert out._components is None and out._adjacency is None and out._device_weld is None and out.device_vertex_colors is None
    assert np.array_equal(bits(out.triangles), bits(want.triangles)) and np.array_equal(bits(mesh.triangles), bits(soup))
    s = out.simplification
    assert isinstance(s, E.MeshSimplification) and s.cell == cell and s.origin == tuple(origin) and s.position == "quadric"
    assert (s.input_faces, s.clusters, s.degenerate_faces, s.duplicate_faces, s.kept_faces, s.fallbacks) == (2308, 228, 1864, 0, 444, 0)
    assert len(out.vertices) == 228 and out.is_watertight
    # the default origin: the per-axis minimum
    auto = E.simplify_mesh(mesh, cell, position="mean")
    assert auto.simplification.origin == tuple(float(v) for v in mesh.vertices.min(axis=0)) and auto.simplification.position == "mean"
    lo = mesh.vertices.min(axis=0).astype(np.float64)
    assert np.array_equal(bits(auto.triangles), bits(E.simplify_mesh_host(mesh.vertices, mesh.faces, lo, cell, "mean").triangles))
    # mesh_report carries the record only for such a mesh
    report = E.mesh_report(out)
    assert report["simplification"] == dict(cell=cell, origin=list(origin), position="quadric", input_faces=2308, clusters=228,
                                            degenerate_faces=1864, duplicate_faces=0, kept_faces=444, fallbacks=0)
    assert report["faces"] == 444 and report["is_watertight"] is True
    assert "simplification" not in E.mesh_report(mesh) and not hasattr(mesh, "simplification")
    import json
    json.dumps(report)
    # an empty mesh gives an empty mesh
    empty = E.simplify_mesh(E.SimpleMesh(np.zeros((0, 3, 3), np.float32)), 0.5)
    assert empty.triangles.shape == (0, 3, 3) and empty.simplification.kept_faces == 0 and empty.simplification.clusters == 0


def test_argument_checks():
    _, mesh, _ = host_case("sphere17")
    for bad in (0.0, -1.0, float("nan"), float("inf"), None, "2", True):
        with pytest.raises(ValueError, match="cell"):
            E.simplify_mesh(mesh, bad)
    for bad in ("median", "QUADRIC", None, 1):
        with pytest.raises(ValueError, match="position"):
            E.simplify_mesh(mesh, 0.5, position=bad)
    for bad in ((0.0, 0.0), (0.0, 0.0, float("nan")), "abc", 1.0):
        with pytest.raises(ValueError, match="origin"):
            E.simplify_mesh(mesh, 0.5, origin=bad)
    E.simplify_mesh(mesh, np.float32(0.5), origin=np.array([-2, -2, -2]))
    # a vertex outside the grid, a grid finer than 2^21 cells, a vertex that is not finite
    with pytest.raises(ValueError, match="outside"):
        E.simplify_mesh(mesh, 0.5, origin=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="outside"):
        E.simplify_mesh(mesh, 1e-7)
    broken = mesh.vertices.copy()
    broken[5, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        E.simplify_mesh_host(broken, mesh.faces, (-2.0, -2.0, -2.0), 0.5)
    with pytest.raises(ValueError, match="face index"):
        E.simplify_mesh_host(mesh.vertices, np.array([[0, 1, len(mesh.vertices)]]), (-2.0, -2.0, -2.0), 0.5)


# ---- options and pipelines ----

def test_the_options_are_parsed_and_command_line_only(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["--yaml=%s/options/shape.yaml" % root, "--output_root=%s" % tmp_path]
    opt = options.set(options.parse_arguments(base + ["--eval.simplify_cells=2.0", "--eval.simplify_position=mean"]),
                      safe_check=True, need_gpu=False)
    edge = (float(opt.eval.range[1]) - float(opt.eval.range[0])) / float(opt.eval.vox_res)
    assert E.COLOR_DEPTH_TOL_CELLS * edge == E.default_color_depth_tol(opt)
    assert E._simplify_options(opt) == (2.0 * edge, (float(opt.eval.range[0]) - 0.5 * edge,) * 3, "mean")
    opt = options.set(options.parse_arguments(base + ["--eval.simplify_cells=3"]), safe_check=True, need_gpu=False)
    assert E._simplify_options(opt) == (3.0 * edge, (float(opt.eval.range[0]) - 0.5 * edge,) * 3, "quadric")
    plain = options.set(options.parse_arguments(base), need_gpu=False)
    for key in E.SIMPLIFY_OPTIONS:
        assert key not in plain.eval and "eval." + key in options.COMMAND_LINE_ONLY          # no yaml file carries them
    assert E._simplify_options(plain) is None
    assert E._simplify_options(edict(dict(eval=dict(range=[-1.5, 1.5])))) is None
    for bad in (dict(simplify_position="mean"), dict(simplify_cells=0), dict(simplify_cells=-2.0), dict(simplify_cells="two"),
                dict(simplify_cells=True), dict(simplify_cells=2.0, simplify_position="median")):
        with pytest.raises(ValueError):
            E._simplify_options(edict(dict(eval=dict(range=[-1.5, 1.5], vox_res=25, **bad))))


def test_the_pipelines_on_host_meshes(monkeypatch, tmp_path):
    """_surface_clouds and convert_to_explicit with marching cubes and the sampler replaced by host stand-ins (the real ones need
    a GPU): with eval.simplify_cells the simplified mesh is delivered and sampled, after the filter and the smoothing; without it
    the calls are today's."""
    soup, mesh, _ = host_case("scene25")
    calls = []

    def extract(vol, isoval, range_min, range_max, num_points=0, seed=0):
        calls.append(("extract", num_points, seed))
        return soup, (torch.zeros(num_points, 3) if num_points else None)

    def sample(tris, num_points, seed=0):
        calls.append(("sample", tris, num_points, seed))
        return torch.zeros(num_points, 3)

    monkeypatch.setattr(E, "extract_surface", extract)
    monkeypatch.setattr(E, "sample_surface", sample)
    vol = torch.zeros(25, 25, 25)

    def opt(**extra):
        return edict(dict(device="cpu", output_path=str(tmp_path), eval=dict(range=[-1.5, 1.5], vox_res=25, num_points=100, **extra)))

    edge = 3.0 / 25
    want = E.simplify_mesh(mesh, 2 * edge, (-1.5 - 0.5 * edge,) * 3)
    assert np.array_equal(bits(want.triangles), bits(simplified("scene25", 2, "quadric").triangles))
    for run in (lambda o: E.convert_to_explicit(o, [vol], 0.5, to_pointcloud=True, seed=3), lambda o: E._surface_clouds(o, vol[None], seed=3)):
        del calls[:]
        meshes, clouds = run(opt(simplify_cells=2))
        assert np.array_equal(bits(meshes[0].triangles), bits(want.triangles)) and meshes[0].simplification == want.simplification
        assert [c[0] for c in calls] == ["extract", "sample"] and calls[0][1:] == (0, 0) and calls[1][2:] == (100, 3)
        assert calls[1][1] is meshes[0].device_triangles and clouds.shape == (1, 100, 3)       # sampled: the delivered mesh
        got = run(opt(simplify_cells=3.0, simplify_position="mean"))[0][0]
        assert np.array_equal(bits(got.triangles), bits(simplified("scene25", 3, "mean").triangles))
        assert got.simplification.position == "mean"
        # after the component filter and the smoothing
        got = run(opt(simplify_cells=2, min_component_area=0.1, smooth_iterations=2))[0][0]
        chain = E.simplify_mesh(E.smooth_mesh(E.filter_components(mesh, 0.1, False), 2), 2 * edge, (-1.5 - 0.5 * edge,) * 3)
        assert np.array_equal(bits(got.triangles), bits(chain.triangles)) and got.simplification.input_faces == 288 + 1928
        # without the option: one call of marching cubes with the points, nothing else
        del calls[:]
        plain = run(opt())[0][0]
        assert calls == [("extract", 100, 3)] and not hasattr(plain, "simplification")
        assert np.array_equal(bits(plain.triangles), bits(soup))
        with pytest.raises(ValueError, match="simplify_cells"):
            run(opt(simplify_position="mean"))
    only_mesh = E.convert_to_explicit(opt(simplify_cells=2), [vol], 0.5)
    assert np.array_equal(bits(only_mesh[0].triangles), bits(want.triangles))
