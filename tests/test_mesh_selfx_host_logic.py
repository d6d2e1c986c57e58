"""CPU: eval_3D.mesh_self_intersections_host - the definition of the face-against-face query and the checker of
csrc/mesh_selfx.hip - against an independent exact computation in integers (the geometric statement: an edge whose ends lie
strictly on opposite sides of the other face's plane and whose crossing point lies in the closed triangle) on random integer
soups, where touching, coplanar, shared-vertex and shared-edge contacts are frequent; hand-written soups with known answers;
the oracle that does not depend on the checker (a raw marching-cubes mesh has no crossing) and the pinned counts of the
processed meshes; the host path of mesh_self_intersections, SimpleMesh's Open3D names, the option and mesh_report."""
import functools
import json
import os

import numpy as np
import pytest

from tests.test_mesh_components_host_logic import host_case
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import options
from zeroshape_amd.utils.options import EasyDict as edict

RAW = ("sphere17", "sphere17_clipped", "scene25", "noise9", "three_valued", "noise23")
GRID = {"sphere17": 17, "sphere17_clipped": 17, "scene25": 25, "noise9": 9, "three_valued": 9, "noise23": 23}


def soup_mesh(soup):
    """The soup as an indexed mesh without a weld: every face has three vertices of its own."""
    tris = np.asarray(soup, np.float32).reshape(-1, 3, 3)
    return tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.int64).reshape(-1, 3)


def check(soup, **kw):
    v, f = soup_mesh(soup)
    return E.mesh_self_intersections_host(v, f, pairs=True, **kw)


def simplified(name, cells, position):
    """simplify_mesh on the host mesh of the case as the pipelines call it: ``cells`` marching-cubes cells, the cluster planes
    half a cell below the range."""
    edge = 3.0 / GRID[name]
    return E.simplify_mesh(host_case(name)[1], cells * edge, origin=(-1.5 - 0.5 * edge,) * 3, position=position)


@functools.lru_cache(maxsize=None)
def two_spheres(aligned):
    """The sphere17 soup and a shifted copy of itself: by (0.7, 0.1, 0.05), or by exactly four lattice steps along x."""
    soup = host_case("sphere17")[0]
    shift = np.float32([np.float32(3.0 / 17 * 4), 0, 0]) if aligned else np.float32([0.7, 0.1, 0.05])
    return np.concatenate([soup, soup + shift]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def smoothed_noise23(mu):
    return E.smooth_mesh(host_case("noise23")[1], 10, 0.5, mu)


def totals(mesh):
    _, _, rec = E.mesh_self_intersections_host(mesh.vertices, mesh.faces)
    return rec["crossing_pairs"], rec["faces_crossed"], rec["coincident_pairs"]


# ---- the independent computation ----

def exact_crossings(tris):
    """int64 [F,3,3] -> (the crossing pairs (i, j), i < j, in lexicographic order; the coincident pairs).  An edge (p, q) of
    one face crosses the other face (a, b, c) with the normal n = (b - a) x (c - a) when the heights n . (p - a) and
    n . (q - a) have strictly opposite signs and the point X where the edge meets the plane lies in the closed triangle:
    n . ((v - u) x (X - u)) >= 0 for its three edges u -> v.  X = p + (hp / w)(q - p) with w = hp - hq is kept as the integer
    vector w X, so every number is an exact integer."""
    t = np.asarray(tris, np.int64)
    F = len(t)
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(F), np.arange(F), indexing="ij"))
    keep = i != j
    i, j = i[keep], j[keep]
    a, b, c = t[j, 0], t[j, 1], t[j, 2]
    n = np.cross(b - a, c - a)
    hit = np.zeros(len(i), bool)
    for k0, k1 in ((0, 1), (1, 2), (2, 0)):
        p, q = t[i, k0], t[i, k1]
        hp, hq = np.einsum("ij,ij->i", n, p - a), np.einsum("ij,ij->i", n, q - a)
        w = hp - hq
        wX = p * w[:, None] + hp[:, None] * (q - p)
        inside = np.ones(len(i), bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= np.einsum("ij,ij->i", n, np.cross(v - u, wX - u * w[:, None])) * np.sign(w) >= 0
        hit |= (hp * hq < 0) & inside
    crossing = set()
    for x, y in zip(i[hit].tolist(), j[hit].tolist()):
        crossing.add((min(x, y), max(x, y)))
    keys = [tuple(sorted(map(tuple, face))) for face in t.tolist()]
    twins = [(x, y) for x in range(F) for y in range(x + 1, F) if keys[x] == keys[y]]
    return sorted(crossing), twins


def integer_soup(seed, n=200):
    rng = np.random.RandomState(seed)
    tris = rng.randint(0, 8, (n, 3, 3)).astype(np.int64)
    tris[:6] = tris[6:12][:, [0, 2, 1]]                              # mirror twins
    tris[12:15] = tris[15:18][:, [1, 2, 0]]                          # the same face from another corner
    tris[18, 1] = tris[18, 0]                                        # zero area: two equal corners
    tris[19] = tris[19, 0] + np.array([[0, 0, 0], [1, 1, 0], [3, 3, 0]])     # zero area: three corners on a line
    return tris


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_checker_against_the_exact_integer_computation(seed):
    tris = integer_soup(seed)
    want_pairs, want_twins = exact_crossings(tris)
    counts, pairs, rec = check(tris)
    assert len(want_pairs) > 100 and len(want_twins) >= 9            # the soup is dense: the contacts are all there
    assert [tuple(p) for p in pairs.tolist()] == want_pairs
    assert rec["crossing_pairs"] == len(want_pairs) and rec["coincident_pairs"] == len(want_twins)
    want_counts = np.bincount(np.asarray(want_pairs).reshape(-1), minlength=len(tris))
    assert np.array_equal(counts, want_counts) and rec["faces_crossed"] == int((want_counts > 0).sum())
    assert rec["skipped_faces"] == 0 and rec["status"] == 0 and rec["brute_force"] == len(tris) * (len(tris) - 1)
    assert 2 * len(want_pairs) <= rec["candidates"] <= rec["brute_force"]

    # a subset of the rows: their counts, their pairs with a higher face
    rows = np.array([7, 0, 150, 19, 18, 199])
    sub_counts, sub_pairs, sub = check(tris, rows=rows)
    assert np.array_equal(sub_counts, counts[rows])
    assert [tuple(p) for p in sub_pairs.tolist()] == [p for p in want_pairs if p[0] in set(rows.tolist())]
    assert sub["crossing_pairs"] == len(sub_pairs) and sub["faces_crossed"] == int((counts[rows] > 0).sum())

    # the corners of every face rotated, and walked the other way round: the same answer
    for turned in (tris[:, [1, 2, 0]], tris[:, [2, 0, 1]], tris[:, [0, 2, 1]]):
        c2, p2, r2 = check(turned)
        assert np.array_equal(c2, counts) and np.array_equal(p2, pairs) and r2 == rec
    # welded: the same faces over shared vertices
    mesh = E.SimpleMesh(tris.astype(np.float32))
    c3, p3, r3 = E.mesh_self_intersections_host(mesh.vertices, mesh.faces, pairs=True)
    assert len(mesh.vertices) < 3 * len(tris) and np.array_equal(c3, counts) and np.array_equal(p3, pairs) and r3 == rec
    # the faces permuted: the counts move with them, the pairs are renamed
    perm = np.random.RandomState(seed + 10).permutation(len(tris))   # new face k is old face perm[k]
    c4, p4, r4 = check(tris[perm])
    assert np.array_equal(c4, counts[perm]) and r4 == rec
    renamed = sorted(tuple(sorted((int(perm[x]), int(perm[y])))) for x, y in p4.tolist())
    assert renamed == want_pairs


# ---- hand-written soups ----

FLOOR = [(0, 0, 0), (2, 0, 0), (0, 2, 0)]


def answer(*faces):
    counts, pairs, rec = check(np.asarray(faces, np.float32))
    assert counts.sum() == 2 * len(pairs) == 2 * rec["crossing_pairs"]
    return [tuple(p) for p in pairs.tolist()], rec["coincident_pairs"], counts.tolist()


def test_a_triangle_pierced_by_another():
    blade = [(0.5, 0.5, -1), (0.5, 0.5, 1), (3, 3, 1)]
    assert answer(FLOOR, blade) == ([(0, 1)], 0, [1, 1])
    # from one side only: the edge of the blade goes through the floor, no edge of the floor reaches the blade
    needle = [(0.5, 0.5, -1), (0.5, 0.5, 1), (0.5, 0.25, 1)]
    assert answer(FLOOR, needle) == ([(0, 1)], 0, [1, 1])
    assert answer(needle, FLOOR) == ([(0, 1)], 0, [1, 1])
    # lifted off the floor: nothing
    assert answer(FLOOR, [(x, y, z + 1.5) for x, y, z in blade]) == ([], 0, [0, 0])


def tetrahedron(corner, size):
    o = np.asarray(corner, np.float64)
    x, y, z = o + [size, 0, 0], o + [0, size, 0], o + [0, 0, size]
    return [[o, y, x], [o, x, z], [o, z, y], [x, y, z]]              # wound outwards


def test_two_interpenetrating_tetrahedra():
    """The corner (1, 1, 1) of the second lies inside the first and its three axis edges leave through the slanted face
    x + y + z = 4: the three faces at that corner each cross the slanted face, and the slanted face's edges cross them."""
    soup = np.asarray(tetrahedron((0, 0, 0), 4) + tetrahedron((1, 1, 1), 4))
    pairs, twins, counts = answer(*soup)
    want, _ = exact_crossings(soup.astype(np.int64))
    assert pairs == want == [(3, 4), (3, 5), (3, 6)] and twins == 0 and counts == [0, 0, 0, 3, 1, 1, 1, 0]
    # one tetrahedron alone: neighbours along edges and at corners, nothing crosses
    assert answer(*soup[:4]) == ([], 0, [0, 0, 0, 0])


def test_touching_is_not_crossing():
    # a corner on a corner and a corner resting in the face - standing on it, and hanging below it
    for tip in ((0, 0, 0), (0.5, 0.5, 0), (0.25, 1.5, 0)):
        tip = np.asarray(tip, np.float64)
        assert answer(FLOOR, [tip, tip + (0.25, 0, 1), tip + (0, 0.25, 1)]) == ([], 0, [0, 0])
        assert answer(FLOOR, [tip + (0.25, 0, -1), tip, tip + (0, 0.25, -1)]) == ([], 0, [0, 0])
    # a corner on an edge of the floor, the face standing along that edge
    assert answer(FLOOR, [(1, 0, 0), (1.25, 0, 1), (0.75, 0, 1)]) == ([], 0, [0, 0])
    # ... but standing ACROSS it, the floor's edge runs through the corner from one side of the face to the other: the
    # triangle is closed, and that is a crossing (the exact computation above says the same)
    assert answer(FLOOR, [(1, 0, 0), (1, 0.25, 1), (1, -0.25, 1)]) == ([(0, 1)], 0, [1, 1])
    # a shared edge: a fold at any angle, flat, and folded back onto the neighbour (coplanar overlap across the edge)
    for apex in ((2, 2, 0), (2, 2, 1), (1, 1, 3), (0.5, 0.5, 0), (0.25, 0.25, 0)):
        assert answer(FLOOR, [(2, 0, 0), apex, (0, 2, 0)]) == ([], 0, [0, 0])
    # an edge lying in the other face's plane, through its inside
    assert answer(FLOOR, [(0.25, 0.5, 0), (0.75, 0.5, 0), (0.5, 0.5, 2)]) == ([], 0, [0, 0])


def test_coplanar_overlap_is_not_crossing_and_twins_are_coincident():
    assert answer(FLOOR, [(0.5, 0.5, 0), (3, 0.5, 0), (0.5, 3, 0)]) == ([], 0, [0, 0])
    assert answer(FLOOR, [(0.25, 0.25, 0), (1, 0.25, 0), (0.25, 1, 0)]) == ([], 0, [0, 0])          # one inside the other
    assert answer(FLOOR, FLOOR) == ([], 1, [0, 0])
    assert answer(FLOOR, FLOOR[::-1]) == ([], 1, [0, 0])                                             # the mirror twin
    assert answer(FLOOR, [FLOOR[1], FLOOR[2], FLOOR[0]], FLOOR[::-1]) == ([], 3, [0, 0, 0])
    # equal as sets of points, not as faces: (a, a, b) and (a, b, b)
    a, b = (0, 0, 0), (1, 2, 3)
    assert answer([a, a, b], [a, b, b]) == ([], 0, [0, 0]) and answer([a, a, b], [b, a, a]) == ([], 1, [0, 0])
    # -0.0 and 0.0 are one value
    assert answer(FLOOR, [(-0.0, 0, -0.0), (2, -0.0, 0), (0, 2, 0)]) == ([], 1, [0, 0])


def test_a_segment_through_a_shared_edge_never_leaks():
    """Two faces share the edge (0,0,0)-(0,4,0); segments run exactly through points of it - the roof's ridge, the flat
    sheet's seam, at the middle, at thirds (not representable: the rounded point lies beside the edge) and through its end."""
    for left, right in (((-2, 0, -1), (2, 0, -1)), ((-2, 0, 0), (2, 0, 0)), ((-2, 1, 3), (2, 0, 0.5))):
        sheet = [[(0, 0, 0), (0, 4, 0), left], [(0, 4, 0), (0, 0, 0), right]]
        for y in (2.0, 1.0, 4.0 / 3.0, 0.1, 3.7):
            for d in ((1, 0, 2), (0.3, 0.2, 1), (-1, 0.5, 1), (0, 0, 1)):
                d = np.asarray(d, np.float64)
                m = np.array([0, y, 0], np.float64)
                blade = [m - d, m + d, m + d + (0, 0.125, 0.125)]
                pairs, _, _ = answer(sheet[0], sheet[1], blade)
                assert (0, 2) in pairs or (1, 2) in pairs, (left, y, d.tolist())
                assert (0, 1) not in pairs


def test_a_face_poking_through_a_neighbour_is_found_through_the_opposite_edge():
    poke = [(0, 0, 0), (1.5, 0.2, 1), (0.2, 1.5, -1)]               # shares the corner (0, 0, 0) with the floor
    assert answer(FLOOR, poke) == ([(0, 1)], 0, [1, 1])
    # on a weld and with the shared vertex duplicated alike
    v = np.float32([(0, 0, 0), (2, 0, 0), (0, 2, 0), (1.5, 0.2, 1), (0.2, 1.5, -1), (0, 0, 0)])
    for faces in ([[0, 1, 2], [0, 3, 4]], [[0, 1, 2], [5, 3, 4]]):
        counts, pairs, _ = E.mesh_self_intersections_host(v, np.asarray(faces), pairs=True)
        assert pairs.tolist() == [[0, 1]] and counts.tolist() == [1, 1]
    # not poking: both other corners above
    assert answer(FLOOR, [(0, 0, 0), (1.5, 0.2, 1), (0.2, 1.5, 1)]) == ([], 0, [0, 0])


def test_a_face_of_zero_area():
    sliver = [(0.5, 0.5, -1), (0.5, 0.5, -1), (0.5, 0.5, 1)]         # two equal corners: a segment through the floor
    assert answer(FLOOR, sliver) == ([(0, 1)], 0, [1, 1])
    line = [(0, 0, 0), (1, 1, 0), (3, 3, 0)]                         # three corners on a line: a plane that nothing crosses
    assert answer(line, [(1, 1, -1), (1, 1, 1), (5, 5, 5)]) == ([], 0, [0, 0])
    assert answer(line, [(2, 2, -1), (2, 2, 1), (2, 7, 1)]) == ([(0, 1)], 0, [1, 1])         # ... but its edges cross others
    assert answer(line, [(2, 1, -1), (2, 1, 1), (2, 7, 1)]) == ([(0, 1)], 0, [1, 1])
    assert answer(line, [(2, 3, -1), (2, 3, 1), (2, 7, 1)]) == ([], 0, [0, 0])
    point = [(0.5, 0.5, 0)] * 3
    assert answer(FLOOR, point, point) == ([], 1, [0, 0, 0])


def test_invalid_faces_are_skipped_and_the_empty_mesh():
    v = np.float32([(0, 0, 0), (2, 0, 0), (0, 2, 0), (0.5, 0.5, -1), (0.5, 0.5, 1), (3, 3, 1), (np.nan, 0, 0), (np.inf, 1, 1)])
    faces = np.array([[0, 1, 2], [3, 4, 8], [3, 4, 5], [3, 4, 6], [-1, 4, 5], [7, 4, 3]])
    counts, pairs, rec = E.mesh_self_intersections_host(v, faces, pairs=True)
    assert counts.tolist() == [1, 0, 1, 0, 0, 0] and pairs.tolist() == [[0, 2]]
    assert rec["skipped_faces"] == 4 and rec["status"] == 3 and rec["brute_force"] == 2
    counts, pairs, rec = E.mesh_self_intersections_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), pairs=True)
    assert counts.shape == (0,) and pairs.shape == (0, 2) and rec["crossing_pairs"] == rec["skipped_faces"] == 0
    assert E.mesh_self_intersections_host(v, faces[:1])[1] is None


# ---- the oracle without the checker, and the pinned counts ----

@pytest.mark.parametrize("name", RAW)
def test_a_raw_marching_cubes_mesh_has_no_crossing(name):
    crossing, faces_crossed, coincident = totals(host_case(name)[1])
    assert (crossing, faces_crossed) == (0, 0)
    assert coincident == {"three_valued": 12, "noise23": 38}.get(name, 0)     # flaps without thickness: twins, not crossings


PINNED = [("three_valued", 2, "quadric", (27, 34, 26)), ("three_valued", 2, "mean", (27, 36, 26)),
          ("noise9", 2, "quadric", (3, 4, 29)), ("noise9", 2, "mean", (0, 0, 29)),
          ("noise9", 3, "quadric", (4, 6, 24)), ("noise9", 3, "mean", (0, 0, 24)),
          ("noise23", 2, "quadric", (336, 441, 701)),
          ("sphere17", 2, "quadric", (0, 0, 0)), ("scene25", 3, "mean", (0, 0, 0))]


@pytest.mark.parametrize("name,cells,position,want", PINNED)
def test_pinned_counts_of_simplified_meshes(name, cells, position, want):
    assert totals(simplified(name, cells, position)) == want


def test_pinned_counts_of_smoothed_meshes_and_of_two_spheres():
    assert totals(smoothed_noise23(-0.53)) == (4, 5, 38)             # ten Taubin passes
    assert totals(smoothed_noise23(None)) == (0, 0, 38)              # ten Laplacian passes
    assert totals(E.SimpleMesh(two_spheres(False))) == (128, 123, 0)
    assert totals(E.SimpleMesh(two_spheres(True))) == (147, 114, 0)  # lattice-aligned: edges through edges and vertices


# ---- the public interface on host meshes ----

def test_host_meshes_go_through_the_checker():
    mesh = E.SimpleMesh(two_spheres(False))
    counts, pairs, rec = E.mesh_self_intersections_host(mesh.vertices, mesh.faces, pairs=True)
    done = E.mesh_self_intersections(mesh)
    assert isinstance(done, E.MeshSelfIntersections) and done.pairs is None and np.array_equal(done.face_counts, counts)
    assert done.counts.dtype == np.int32 and done.counts.shape == (9,)
    assert done.check() == dict(n_pairs=128, n_coincident=0, n_faces_crossed=123, skipped_faces=0, status=0,
                                examined=1352 * 1351, truncated=False)
    assert mesh.self_intersections is mesh.self_intersections and mesh.is_self_intersecting() is True
    assert np.array_equal(mesh.self_intersections.face_counts, counts)
    listed = mesh.get_self_intersecting_triangles()
    assert listed.dtype == np.int64 and np.array_equal(listed, pairs) and listed.shape == (128, 2)
    full = E.mesh_self_intersections(mesh, pairs=True)
    assert np.array_equal(full.pairs, pairs) and full.check()["truncated"] is False
    short = E.mesh_self_intersections(mesh, capacity=100)
    assert np.array_equal(short.pairs, pairs[:100]) and short.check()["truncated"] is True
    long = E.mesh_self_intersections(mesh, pairs=True, capacity=130)
    assert np.array_equal(long.pairs[:128], pairs) and np.all(long.pairs[128:] == -1) and long.check()["truncated"] is False
    assert E.mesh_self_intersections(mesh, capacity=0).pairs.shape == (0, 2)
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="capacity"):
            E.mesh_self_intersections(mesh, capacity=bad)
    clean = host_case("sphere17")[1]
    assert clean.is_self_intersecting() is False and clean.get_self_intersecting_triangles().shape == (0, 2)
    empty = E.SimpleMesh(np.zeros((0, 3, 3), np.float32))
    assert empty.is_self_intersecting() is False and empty.self_intersections.face_counts.shape == (0,)
    assert "coplanar" in E.MeshSelfIntersections.__doc__ and "repaired" in E.MeshSelfIntersections.__doc__


def test_the_option_is_parsed_and_command_line_only(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["--yaml=%s/options/shape.yaml" % root, "--output_root=%s" % tmp_path]
    opt = options.set(options.parse_arguments(base + ["--eval.mesh_self_intersections=true"]), safe_check=True, need_gpu=False)
    assert opt.eval.mesh_self_intersections is True and E.self_intersections_option(opt) is True     # no other switch needed
    plain = options.set(options.parse_arguments(base), need_gpu=False)
    assert "mesh_self_intersections" not in plain.eval and "eval.mesh_self_intersections" in options.COMMAND_LINE_ONLY
    assert E.self_intersections_option(plain) is False
    assert E.self_intersections_option(edict(dict(eval=dict(mesh_self_intersections=False)))) is False
    for yaml in os.listdir(os.path.join(root, "options")):
        with open(os.path.join(root, "options", yaml)) as fh:
            assert "mesh_self_intersections" not in fh.read()
    for script in ("demo.py", "evaluate.py"):
        with open(os.path.join(root, script)) as fh:
            assert "--eval.mesh_self_intersections=true" in fh.read()


def test_the_report_on_host_meshes():
    """The helper of the pipelines on host meshes: the delivered mesh carries its record, with the record of the mesh before
    the processing steps when one ran; without the switch the report has no such key and nothing is computed."""
    edge = 3.0 / 9
    simplifying = (2 * edge, (-1.5 - 0.5 * edge,) * 3, "quadric")
    raw = E.SimpleMesh(host_case("three_valued")[0])
    assert "self_intersections" not in E.mesh_report(raw) and raw._self_intersections is None
    plain = E._cleaned_and_smoothed(raw, None, None, simplifying)
    assert "self_intersections" not in E.mesh_report(plain) and plain._self_intersections is None

    out = E._cleaned_and_smoothed(E.SimpleMesh(host_case("three_valued")[0]), None, None, simplifying, selfx=True)
    report = E.mesh_report(out)
    assert report["self_intersections"] == dict(crossing_pairs=27, faces_crossed=34, coincident_pairs=26, skipped_faces=0,
                                                before=dict(crossing_pairs=0, faces_crossed=0, coincident_pairs=12,
                                                            skipped_faces=0))
    assert np.array_equal(out.triangles, plain.triangles)                        # the switch changes nothing else
    json.dumps(report["self_intersections"])
    # smoothing counts as a step; the component filter alone does not
    smooth = E._cleaned_and_smoothed(E.SimpleMesh(host_case("noise9")[0]), (None, False), (2, 0.5, -0.53, True), selfx=True)
    assert set(E.mesh_report(smooth)["self_intersections"]) == {"crossing_pairs", "faces_crossed", "coincident_pairs",
                                                                 "skipped_faces", "before"}
    filtered = E._cleaned_and_smoothed(E.SimpleMesh(host_case("noise9")[0]), (0.05, False), None, selfx=True)
    assert E.mesh_report(filtered)["self_intersections"] == dict(crossing_pairs=0, faces_crossed=0, coincident_pairs=0,
                                                                  skipped_faces=0)
    alone = E._with_self_intersections(E.SimpleMesh(two_spheres(False)))
    assert E.mesh_report(alone)["self_intersections"] == dict(crossing_pairs=128, faces_crossed=123, coincident_pairs=0,
                                                              skipped_faces=0)
