"""CPU: eval_3D.closest_point_on_mesh_host - the definition of mesh_distance and the checker of csrc/mesh_distance.hip - on one
triangle with hand-computed answers in every Voronoi region, against a barycentric lattice on marching-cubes meshes, on
degenerate, tied, skipped and missing faces; mesh_distance_stats_host against hand sums; mesh_deviation on host meshes,
mesh_report, the option, the pipelines."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_mesh_components_host_logic import host_case
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import options
from zeroshape_amd.utils.options import EasyDict as edict

A, B, C = (0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0)
TRIANGLE = (np.array([A, B, C], np.float32), np.array([[0, 1, 2]]))

# query, closest point, squared distance: worked out by hand for the triangle (0,0,0), (4,0,0), (0,4,0)
VORONOI = [
    ((-1, -1, 0), A, 2.0), ((-1, -2, 2), A, 9.0),                                  # the region of vertex a
    ((6, -1, 0), B, 5.0), ((5, 0, 0), B, 1.0),                                     # ... of b
    ((-1, 6, 0), C, 5.0), ((0, 5, 1), C, 2.0),                                     # ... of c
    ((2, -3, 0), (2, 0, 0), 9.0), ((1, -1, 1), (1, 0, 0), 2.0),                    # the region of edge ab
    ((-3, 2, 0), (0, 2, 0), 9.0), ((-1, 3, -1), (0, 3, 0), 2.0),                   # ... of ac
    ((4, 4, 0), (2, 2, 0), 8.0), ((3, 3, 1), (2, 2, 0), 3.0),                      # ... of bc
    ((1, 1, 5), (1, 1, 0), 25.0), ((1, 1, -2), (1, 1, 0), 4.0), ((1, 2, 0), (1, 2, 0), 0.0),        # above, below, inside
    ((2, 0, 0), (2, 0, 0), 0.0), ((0, 2, 0), (0, 2, 0), 0.0), ((2, 2, 0), (2, 2, 0), 0.0),          # on each edge
    ((2, 0, 3), (2, 0, 0), 9.0), ((0, 1, -1), (0, 1, 0), 1.0), ((1, 3, 2), (1, 3, 0), 4.0),        # above and below each edge
    (A, A, 0.0), (B, B, 0.0), (C, C, 0.0),                                         # at each vertex
]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_one_triangle_in_every_voronoi_region():
    q = np.array([v[0] for v in VORONOI], np.float32)
    for verts, faces in (TRIANGLE, (TRIANGLE[0][[1, 2, 0]], TRIANGLE[1]), (TRIANGLE[0][[2, 0, 1]], TRIANGLE[1]),
                         (TRIANGLE[0][[0, 2, 1]], TRIANGLE[1])):                   # every corner in every role, both windings
        sq, face, closest, skipped = E.closest_point_on_mesh_host(q, verts, faces)
        assert sq.dtype == np.float64 and face.dtype == np.int64 and closest.dtype == np.float64 and skipped == 0
        assert np.array_equal(sq, [v[2] for v in VORONOI]) and np.all(face == 0)
        assert np.array_equal(closest, np.array([v[1] for v in VORONOI], np.float64))
    # moved and scaled: the same answers up to rounding
    scale, shift = 0.37, np.array([0.3, -1.1, 2.2])
    sq, _, closest, _ = E.closest_point_on_mesh_host(q * np.float32(scale) + shift.astype(np.float32),
                                                     TRIANGLE[0] * np.float32(scale) + shift.astype(np.float32), TRIANGLE[1])
    assert np.abs(sq - np.array([v[2] for v in VORONOI]) * scale ** 2).max() < 1e-5
    assert np.abs(closest - (np.array([v[1] for v in VORONOI]) * scale + shift)).max() < 1e-5


def lattice_points(vertices, faces, k):
    """The (k + 1)(k + 2) / 2 points a + (i u + j v) / k, i + j <= k, of every face -> [F,L,3] float64."""
    tri = vertices[faces].astype(np.float64)
    ij = np.array([(i, j) for i in range(k + 1) for j in range(k + 1 - i)], np.float64) / k
    return tri[:, None, 0] + ij[None, :, :1] * (tri[:, 1] - tri[:, 0])[:, None] + ij[None, :, 1:] * (tri[:, 2] - tri[:, 0])[:, None]


@pytest.mark.parametrize("name", ["sphere17", "scene25"])
def test_the_checker_against_a_barycentric_lattice(name):
    """An independent bound: the distance is at most that to the nearest of k x k samples of every face, and at least that
    minus the samples' spacing (every point of a face lies in a small triangle of the lattice, within one of its edges - at most
    the longest edge / k - of a lattice point)."""
    _, mesh, _ = host_case(name)
    k = 6
    rng = np.random.RandomState(3)
    q = rng.uniform(-1.6, 1.6, (150, 3)).astype(np.float32)
    sq, face, closest, skipped = E.closest_point_on_mesh_host(q, mesh.vertices, mesh.faces)
    assert skipped == 0 and np.all(np.isfinite(sq)) and np.all((face >= 0) & (face < len(mesh.faces)))
    samples = lattice_points(mesh.vertices, mesh.faces, k).reshape(-1, 3)
    nearest = np.sqrt(((q.astype(np.float64)[:, None] - samples[None]) ** 2).sum(-1).min(axis=1))
    tri = mesh.vertices[mesh.faces].astype(np.float64)
    spacing = np.sqrt(((tri - np.roll(tri, 1, axis=1)) ** 2).sum(-1)).max() / k
    d = np.sqrt(sq)
    assert np.all(d <= nearest + 1e-12) and np.all(d >= nearest - spacing)
    assert (d < nearest - 1e-6).any()                                              # and it does better than the samples
    # the closest point is at that distance and lies on the face that is named (its plane, inside its box)
    assert np.abs(np.sqrt(((q - closest) ** 2).sum(-1)) - d).max() < 1e-12
    a, b, c = (tri[face][:, i] for i in range(3))
    n = np.cross(b - a, c - a)
    off = np.abs(((closest - a) * n).sum(-1)) / np.maximum(np.sqrt((n * n).sum(-1)), 1e-300)
    assert off.max() < 1e-9
    assert np.all(closest >= tri[face].min(axis=1) - 1e-9) and np.all(closest <= tri[face].max(axis=1) + 1e-9)


def segment_distance(q, p0, p1):
    q, p0, p1 = (np.asarray(v, np.float64) for v in (q, p0, p1))
    e = p1 - p0
    s = np.clip(((q - p0) @ e) / max(e @ e, 1e-300), 0.0, 1.0)
    return np.sqrt((((p0 + s[:, None] * e) - q) ** 2).sum(-1))


def test_degenerate_faces_are_segments_and_points():
    verts = np.array([[0, 0, 0], [2, 0, 0], [0.5, 0, 0], [5, 5, 5], [9, 9, 9], [9, 10, 9], [10, 9, 9]], np.float32)
    rng = np.random.RandomState(0)
    q = rng.uniform(-3, 11, (200, 3)).astype(np.float32)
    want = segment_distance(q, verts[0], verts[1])
    for face in ([0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [0, 2, 1], [2, 0, 1], [0, 1, 2]):      # a zero edge; three in a line
        sq, idx, closest, skipped = E.closest_point_on_mesh_host(q, verts, [face])
        assert skipped == 0 and np.all(np.isfinite(sq)) and np.all(np.isfinite(closest)) and np.all(idx == 0)
        assert np.abs(np.sqrt(sq) - want).max() < 1e-12
    point = np.sqrt(((q.astype(np.float64) - 5.0) ** 2).sum(-1))
    sq, idx, closest, _ = E.closest_point_on_mesh_host(q, verts, [[3, 3, 3]])
    assert np.array_equal(sq, point ** 2) or np.abs(np.sqrt(sq) - point).max() < 1e-12
    assert np.all(closest == 5.0)
    # mixed with proper faces: the minimum over all of them
    faces = np.array([[4, 5, 6], [0, 0, 1], [3, 3, 3], [4, 6, 5]])
    sq, idx, closest, _ = E.closest_point_on_mesh_host(q, verts, faces)
    proper = np.sqrt(E.closest_point_on_mesh_host(q, verts, faces[:1])[0])
    assert np.all(np.isfinite(sq)) and np.abs(np.sqrt(sq) - np.minimum(np.minimum(want, point), proper)).max() < 1e-12
    assert set(idx.tolist()) == {0, 1, 2}                                          # never the duplicate


def test_ties_take_the_lower_face_index():
    # two faces that share the edge on the x axis, at right angles: a point on the edge, above it on the bisector, at a shared
    # vertex
    verts = np.array([[0, 0, 0], [2, 0, 0], [1, 2, 0], [1, 0, 2]], np.float32)
    q = np.array([[1, 0, 0], [0.5, 0, 0], [0, 0, 0], [2, 0, 0], [1, -1, -1], [1, 1, 1]], np.float32)
    for faces in ([[0, 1, 2], [1, 0, 3]], [[1, 0, 3], [0, 1, 2]], [[0, 1, 2], [0, 1, 3]]):
        sq, idx, closest, _ = E.closest_point_on_mesh_host(q, verts, faces)
        assert np.all(idx == 0), idx
        assert np.array_equal(sq, [0, 0, 0, 0, 2, 1])                         # (1, 1, 1): one above either face
    # a duplicated face, among others before and after it
    faces = np.array([[1, 0, 3], [0, 1, 2], [0, 1, 2], [1, 2, 0], [0, 1, 2]])
    sq, idx, _, _ = E.closest_point_on_mesh_host(np.array([[1, 1, -0.5], [1, 1.5, -3]], np.float32), verts, faces)
    assert np.array_equal(idx, [1, 1]) and np.array_equal(sq, [0.25, 9.0])
    # the blocks of the brute force do not change who wins
    _, mesh, _ = host_case("sphere17")
    whole = E.closest_point_on_mesh_host(mesh.vertices, mesh.vertices, mesh.faces)
    lowest = np.full(len(mesh.vertices), len(mesh.faces))
    np.minimum.at(lowest, mesh.faces.reshape(-1), np.repeat(np.arange(len(mesh.faces)), 3))
    assert np.all(whole[0] == 0.0) and np.array_equal(whole[1], lowest) and np.array_equal(whole[2], mesh.vertices.astype(np.float64))
    for block in (1 << 10, 7 << 10, 1 << 22):
        other = E.closest_point_on_mesh_host(mesh.vertices, mesh.vertices, mesh.faces, block=block)
        assert np.array_equal(other[1], whole[1]) and np.array_equal(bits(other[2]), bits(whole[2]))


def test_skipped_faces_and_points_that_are_not_finite():
    _, mesh, _ = host_case("sphere17")
    verts, faces = mesh.vertices.copy(), mesh.faces.copy()
    rng = np.random.RandomState(1)
    q = rng.uniform(-1.5, 1.5, (64, 3)).astype(np.float32)
    verts[7, 1], verts[11, 0] = np.nan, np.inf
    faces[3, 2], faces[9, 0] = len(verts), -1
    bad = np.zeros(len(faces), bool)
    bad[[3, 9]] = True
    bad |= np.isin(faces, [7, 11]).any(axis=1)
    sq, idx, closest, skipped = E.closest_point_on_mesh_host(q, verts, faces)
    assert skipped == int(bad.sum()) and skipped > 2 and np.all(np.isfinite(sq)) and not bad[idx].any()
    keep = np.flatnonzero(~bad)
    clean = E.closest_point_on_mesh_host(q, np.nan_to_num(verts, posinf=0.0), faces[keep])
    assert np.array_equal(bits(sq), bits(clean[0])) and np.array_equal(idx, keep[clean[1]]) and np.array_equal(bits(closest), bits(clean[2]))
    # points that are not finite
    q[5, 0], q[9, 2], q[20, 1] = np.nan, np.inf, -np.inf
    sq2, idx2, closest2, _ = E.closest_point_on_mesh_host(q, verts, faces)
    rows = [5, 9, 20]
    assert np.all(np.isnan(sq2[rows])) and np.all(idx2[rows] == -1) and np.all(np.isnan(closest2[rows]))
    rest = np.setdiff1d(np.arange(64), rows)
    assert np.array_equal(bits(sq2[rest]), bits(sq[rest])) and np.array_equal(idx2[rest], idx[rest])
    done = E.mesh_distance(E.SimpleMesh(mesh.triangles), q)
    assert done.check() == dict(skipped_faces=0, nonfinite_queries=3, status=4, pairs=676 * 61) and done.closest is None


def test_an_empty_mesh_and_no_points():
    q = np.array([[0, 0, 0], [1, 2, 3], [np.nan, 0, 0]], np.float32)
    for verts, faces in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)),
                         (np.zeros((3, 3), np.float32), np.array([[0, 1, 3]])),                     # every face skipped
                         (np.full((3, 3), np.nan, np.float32), np.array([[0, 1, 2]]))):
        sq, idx, closest, skipped = E.closest_point_on_mesh_host(q, verts, faces)
        assert np.all(sq[:2] == np.inf) and np.isnan(sq[2]) and np.all(idx == -1) and np.all(np.isnan(closest)) and skipped == len(faces)
    sq, idx, closest, _ = E.closest_point_on_mesh_host(np.zeros((0, 3), np.float32), *TRIANGLE)
    assert sq.shape == (0,) and idx.shape == (0,) and closest.shape == (0, 3)
    done = E.SimpleMesh(np.zeros((0, 3, 3), np.float32)).distance_to(q[:2], closest=True)
    assert np.all(done.sqdist == np.inf) and np.all(done.face == -1) and done.closest.shape == (2, 3)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_stats_against_hand_sums(n):
    rng = np.random.RandomState(n)
    d2 = rng.uniform(0, 4, n) ** 2
    if n > 1:
        d2[n // 2] = d2.max()                                                      # the maximum twice: the lower index
    for holes in (False, True):
        x = d2.copy()
        if holes and n > 3:
            x[1], x[n - 1], x[n // 3] = np.nan, np.inf, np.nan
        ok = np.isfinite(x)
        d = np.sqrt(np.where(ok, x, 0.0))
        # thread t = i mod 256 adds its elements in ascending i; then the partial sums in ascending t - in plain loops
        s, s2 = np.zeros(256), np.zeros(256)
        for i in range(n):
            if ok[i]:
                s[i % 256] = s[i % 256] + d[i]
                s2[i % 256] = s2[i % 256] + x[i]
        total = total2 = 0.0
        for t in range(256):
            total, total2 = total + s[t], total2 + s2[t]
        count = int(ok.sum())
        got, at = E.mesh_distance_stats_host(x)
        want = np.array([d[ok].max(), total / count, np.sqrt(total2 / count), count])
        assert got.dtype == np.float64 and np.array_equal(bits(got), bits(want)), (got, want)
        assert at == int(np.flatnonzero(ok & (d == d[ok].max()))[0])
        assert abs(got[1] - d[ok].mean()) < 1e-12 and abs(got[2] - np.sqrt((d[ok] ** 2).mean())) < 1e-12
    got, at = E.mesh_distance_stats_host(np.array([np.nan, np.inf]))
    assert np.all(np.isnan(got[:3])) and got[3] == 0 and at == -1
    assert E.mesh_distance_stats_host(np.zeros(0))[1] == -1


def _cube(shift=0.0):
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32) + np.array([shift, 0, 0], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v[np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])]


def test_mesh_deviation_on_host_meshes():
    soup, mesh, _ = host_case("sphere17")
    same = E.mesh_deviation(mesh, E.SimpleMesh(soup.copy()))
    assert isinstance(same, E.MeshDeviation) and same.cell_edge is None
    assert (same.forward_max, same.forward_mean, same.forward_rms, same.backward_max, same.backward_mean, same.backward_rms) == (0,) * 6
    assert (same.forward_index, same.backward_index, same.forward_vertices, same.backward_vertices) == (0, 0, 340, 340)
    # a copy shifted along x: nothing lies farther than the shift
    t = 0.125
    moved = E.mesh_deviation(E.SimpleMesh(soup + np.array([t, 0, 0], np.float32)), mesh)
    for side in (moved.forward_max, moved.backward_max):
        assert 0.5 * t < side <= t * (1 + 1e-6)
    assert 0 < moved.forward_mean <= moved.forward_rms <= moved.forward_max
    # a closed convex case: the unit cube and its copy a quarter along x - the far face's corners are exactly t away, both ways
    cube = E.mesh_deviation(E.SimpleMesh(_cube(0.25)), E.SimpleMesh(_cube()))
    assert cube.forward_max == 0.25 and cube.backward_max == 0.25 and (cube.forward_vertices, cube.backward_vertices) == (8, 8)
    assert cube.forward_mean == 0.125 and cube.forward_rms == np.sqrt(0.25 ** 2 / 2)
    a, b = E.SimpleMesh(_cube(0.25)), E.SimpleMesh(_cube())
    assert a.vertices[cube.forward_index][0] == 1.25 and b.vertices[cube.backward_index][0] == 0.0
    # the simplification's own bound: every vertex of the result lies within 1.5 cells per axis of the vertices it replaces,
    # which lie on the original surface
    edge = 3.0 / 17
    light = E.simplify_mesh(mesh, 2 * edge, (-1.5 - 0.5 * edge,) * 3)
    got = E.mesh_deviation(light, mesh, cell_edge=edge)
    assert 0 < got.forward_max <= 1.5 * np.sqrt(3) * edge and got.cell_edge == edge       # (in marching-cubes cells: the stricter reading)
    assert 0 < got.backward_max
    assert (got.forward_vertices, got.backward_vertices) == (len(light.vertices), 340)
    # the fields are the checkers' numbers
    done = E.mesh_distance(mesh, light.vertices)
    stats, at = E.mesh_distance_stats_host(done.sqdist)
    assert (got.forward_max, got.forward_mean, got.forward_rms, got.forward_index) == (stats[0], stats[1], stats[2], at)
    with pytest.raises(ValueError, match="both"):
        E.mesh_deviation(mesh, edict(dict(device_triangles=torch.zeros(0))))


def test_mesh_report_key_sets():
    soup, mesh, _ = host_case("sphere17")
    plain = set(E.mesh_report(mesh))
    assert "deviation" not in plain and not hasattr(mesh, "deviation")
    edge = 3.0 / 17
    light = E.simplify_mesh(mesh, 2 * edge, (-1.5 - 0.5 * edge,) * 3)
    assert set(E.mesh_report(light)) == plain | {"simplification"}
    light.deviation = E.mesh_deviation(light, mesh)
    report = E.mesh_report(light)
    assert set(report) == plain | {"simplification", "deviation"}
    assert set(report["deviation"]) == set(E.MeshDeviation._fields) and report["deviation"]["cell_edge"] is None
    light.deviation = E.mesh_deviation(light, mesh, cell_edge=edge)
    record = E.mesh_report(light)["deviation"]
    cells = {"%s_%s_cells" % (s, w) for s in ("forward", "backward") for w in ("max", "mean", "rms")}
    assert set(record) == set(E.MeshDeviation._fields) | cells
    assert record["forward_max_cells"] == record["forward_max"] / edge and 0 < record["forward_max_cells"] < 2 * 1.5 * np.sqrt(3)
    json.dumps(record)


def test_the_option_is_parsed_and_command_line_only(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["--yaml=%s/options/shape.yaml" % root, "--output_root=%s" % tmp_path]
    opt = options.set(options.parse_arguments(base + ["--eval.simplify_cells=2.0", "--eval.mesh_deviation=true"]),
                      safe_check=True, need_gpu=False)
    edge = (float(opt.eval.range[1]) - float(opt.eval.range[0])) / float(opt.eval.vox_res)
    assert opt.eval.mesh_deviation is True
    assert E._deviation_option(opt, E._smooth_options(opt), E._simplify_options(opt)) == edge
    plain = options.set(options.parse_arguments(base), need_gpu=False)
    assert "mesh_deviation" not in plain.eval and "eval.mesh_deviation" in options.COMMAND_LINE_ONLY
    assert E._deviation_option(plain, None, None) is None
    alone = options.set(options.parse_arguments(base + ["--eval.mesh_deviation=true"]), safe_check=True, need_gpu=False)
    with pytest.raises(ValueError, match="mesh_deviation needs"):
        E._deviation_option(alone, E._smooth_options(alone), E._simplify_options(alone))
    off = edict(dict(eval=dict(range=[-1.5, 1.5], vox_res=25, mesh_deviation=False)))
    assert E._deviation_option(off, None, None) is None
    for yaml in os.listdir(os.path.join(root, "options")):
        with open(os.path.join(root, "options", yaml)) as fh:
            assert "mesh_deviation" not in fh.read()


def test_the_pipelines_on_host_meshes(monkeypatch, tmp_path):
    """_surface_clouds and convert_to_explicit with marching cubes and the sampler replaced by host stand-ins (the real ones need
    a GPU): with eval.mesh_deviation the delivered mesh carries the record against the mesh as it stood after the component
    filter; without it nothing is attached and the calls are today's."""
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
    grid = (2 * edge, (-1.5 - 0.5 * edge,) * 3)
    filtered = E.filter_components(mesh, 0.1, False)
    chain = E.simplify_mesh(E.smooth_mesh(filtered, 2), *grid)
    want_chain = E.mesh_deviation(chain, filtered, cell_edge=edge)
    want_simple = E.mesh_deviation(E.simplify_mesh(mesh, *grid), mesh, cell_edge=edge)
    want_smooth = E.mesh_deviation(E.smooth_mesh(mesh, 5), mesh, cell_edge=edge)
    assert 0 < want_simple.forward_max / edge < 2 * 1.5 * np.sqrt(3) and 0 < want_smooth.forward_max < edge
    for run in (lambda o: E.convert_to_explicit(o, [vol], 0.5, to_pointcloud=True, seed=3), lambda o: E._surface_clouds(o, vol[None], seed=3)):
        got = run(opt(simplify_cells=2, mesh_deviation=True))[0][0]
        assert got.deviation == want_simple and got.simplification.kept_faces == 444
        assert E.mesh_report(got)["deviation"]["forward_max_cells"] == want_simple.forward_max / edge
        assert run(opt(smooth_iterations=5, mesh_deviation=True))[0][0].deviation == want_smooth
        got = run(opt(simplify_cells=2, min_component_area=0.1, smooth_iterations=2, mesh_deviation=True))[0][0]
        assert got.deviation == want_chain and got.deviation.backward_vertices == len(filtered.vertices) < len(mesh.vertices)
        # without the flag (absent or false): today's calls, nothing attached
        for extra in (dict(), dict(mesh_deviation=False)):
            del calls[:]
            plain = run(opt(simplify_cells=2, **extra))[0][0]
            assert calls == [("extract", 0, 0), ("sample", 100, 3)] and not hasattr(plain, "deviation")
            assert "deviation" not in E.mesh_report(plain)
        del calls[:]
        plain = run(opt())[0][0]
        assert calls == [("extract", 100, 3)] and not hasattr(plain, "deviation")
        for extra in (dict(), dict(min_component_area=0.1)):
            with pytest.raises(ValueError, match="mesh_deviation needs"):
                run(opt(mesh_deviation=True, **extra))
    # the helper's new keyword has a default: its callers of before are served
    assert not hasattr(E._cleaned_and_smoothed(mesh, None, (2, 0.5, -0.53, True)), "deviation")
