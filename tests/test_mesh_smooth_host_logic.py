"""CPU: eval_3D.mesh_adjacency_host and eval_3D.smooth_vertices_host - the definitions of the vertex neighbourhood and of the
smoothing passes, and the checkers of csrc/mesh_smooth.hip - against known counts and an independent computation (scipy's
sparse matrices) on the marching-cubes soups of the oracle, on hand-written soups with exact answers, and on sphere17's
volume; smooth_mesh on host meshes; the options."""
import os

import numpy as np
import pytest

from tests.test_mesh_components_host_logic import KNOWN, host_case
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import options
from zeroshape_amd.utils.options import EasyDict as edict

CASES = list(KNOWN)
#                     max degree, boundary vertices
NEIGHBOURHOOD = {"sphere17": (9, 0), "sphere17_clipped": (9, 28), "scene25": (9, 0), "noise9": (13, 411), "noise23": (16, 2916),
                 "noise45": (16, 11566), "three_valued": (19, 255)}


def edge_uses(faces):
    """Independent of the checker: unique sorted vertex pairs of the faces with three distinct indices, and their use counts."""
    f = np.asarray(faces, np.int64)
    good = f[[len(set(row)) == 3 for row in f.tolist()]] if len(f) else f
    half = np.concatenate([good[:, [0, 1]], good[:, [1, 2]], good[:, [2, 0]]])
    return np.unique(np.sort(half, axis=1), axis=0, return_counts=True)


@pytest.mark.parametrize("name", CASES)
def test_adjacency_on_the_marching_cubes_cases(name):
    _, mesh, _ = host_case(name)
    V = len(mesh.vertices)
    adj = E.mesh_adjacency_host(mesh.faces, V)
    assert adj.offsets.dtype == np.int32 and adj.neighbors.dtype == np.int32 and adj.boundary.dtype == np.uint8
    assert adj.degree.dtype == np.int32 and adj.device_offsets is None
    assert adj.offsets.shape == (V + 1,) and adj.boundary.shape == (V,) and adj.neighbors.shape == (adj.offsets[-1],)
    F, Vn, D, C, Ed, B, N, M = KNOWN[name]
    edges, uses = edge_uses(mesh.faces)
    assert adj.n_edges == Ed == len(edges) and int((uses == 1).sum()) == B
    max_degree, boundary_vertices = NEIGHBOURHOOD[name]
    assert int(adj.degree.max()) == max_degree and int(adj.boundary.sum()) == boundary_vertices
    assert int(adj.degree.min()) > 0                                             # no vertex without an edge in any case
    want = np.zeros(V, np.uint8)
    want[edges[uses == 1].reshape(-1)] = 1
    assert np.array_equal(adj.boundary, want)
    if name == "three_valued":
        f = mesh.faces
        assert int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()) == D == 141
    # SimpleMesh's views of it
    assert mesh.adjacency is mesh.adjacency and np.array_equal(mesh.adjacency.neighbors, adj.neighbors)
    rows = mesh.vertex_neighbors
    assert len(rows) == V and [len(r) for r in rows[:50]] == adj.degree[:50].tolist()
    assert all(np.array_equal(rows[v], adj.neighbors[adj.offsets[v]:adj.offsets[v + 1]]) for v in (0, V // 2, V - 1))


def scipy_matrix(faces, n_vertices):
    from scipy.sparse import coo_matrix
    f = np.asarray(faces, np.int64)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    rows = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    cols = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    A = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_vertices, n_vertices)).tocsr()
    A.data[:] = 1.0                                                              # binarised: duplicates were summed
    A.sort_indices()
    return A


@pytest.mark.parametrize("name", CASES)
def test_against_scipy(name):
    _, mesh, _ = host_case(name)
    V = len(mesh.vertices)
    adj = mesh.adjacency
    A = scipy_matrix(mesh.faces, V)
    assert np.array_equal(A.indptr, adj.offsets) and np.array_equal(A.indices, adj.neighbors)
    # one free pass: the same terms in another order
    x = mesh.vertices.astype(np.float64)
    lamb = 0.5
    want = x + lamb * ((A @ x) / adj.degree[:, None] - x)
    x1 = E.smooth_positions_host(x, adj.offsets, adj.neighbors, adj.boundary, 1, lamb, None, False)
    assert x1.dtype == np.float64 and np.all(np.abs(x1 - want) <= 1e-12 * np.abs(x).max())
    got = E.smooth_vertices_host(mesh.vertices, adj.offsets, adj.neighbors, adj.boundary, 1, lamb, None, False)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), x1.astype(np.float32).view(np.uint32))


# ---- known answers ----

TET = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
TET_FACES = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)


def hand_meshes():
    """name -> soup [n,3,3] float32."""
    fan = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return {
        "tetrahedron": TET[TET_FACES],
        "triangle": TRI[None],
        "degenerate": np.array([[[0, 0, 0], [0, 0, 0], [1, 2, 3]]], np.float32),                     # (p, p, q)
        "three_on_an_edge": fan[np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]])],
        "duplicated_face": np.concatenate([TRI[None], TRI[None]]),
        "empty": np.zeros((0, 3, 3), np.float32),
    }


def check_hand_mesh(name, make):
    """``make(soup)`` -> SimpleMesh (host or device): the exact answers of the issue."""
    soup = hand_meshes()[name]
    mesh = make(soup)
    adj = mesh.adjacency
    same = lambda a, b: np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    if name == "tetrahedron":
        assert adj.degree.tolist() == [3] * 4 and adj.n_edges == 6 and not adj.boundary.any()
        assert [r.tolist() for r in mesh.vertex_neighbors] == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
        # the mean of the three others is -x / 3: x' = x (1 - 4 lamb / 3)
        assert same(E.smooth_mesh(mesh, 1, 0.75, None).triangles, np.zeros_like(soup))
        assert same(E.smooth_mesh(mesh, 1, 0.375, None).triangles, soup * np.float32(0.5))
        assert same(E.smooth_mesh(mesh, 2, 0.375, -0.75).triangles, soup)          # x 1/2, then x 2
        assert same(E.smooth_mesh(mesh, 0).triangles, soup)
    elif name == "triangle":
        assert adj.degree.tolist() == [2] * 3 and adj.boundary.tolist() == [1] * 3 and adj.n_edges == 3
        assert same(E.smooth_mesh(mesh, 3).triangles, soup)                        # pinned
        v = mesh.vertices.astype(np.float64)
        want = np.stack([v[i] + 0.5 * ((v[(i + 1) % 3] + v[(i + 2) % 3]) / 2.0 - v[i]) for i in range(3)])
        # (vertex i's neighbours in ascending order: whichever order, two terms add commutatively)
        assert same(E.smooth_mesh(mesh, 1, 0.5, None, pin_boundary=False).triangles, want.astype(np.float32)[mesh.faces])
    elif name == "degenerate":
        assert len(mesh.vertices) == 2 and adj.degree.tolist() == [0, 0] and adj.n_edges == 0 and not adj.boundary.any()
        assert adj.neighbors.shape == (0,) and adj.offsets.tolist() == [0, 0, 0]
        for pin in (True, False):
            assert same(E.smooth_mesh(mesh, 4, pin_boundary=pin).triangles, soup)
    elif name == "three_on_an_edge":
        # the weld's order is by coordinate bits; find the two ends of the shared edge
        v = mesh.vertices
        a = int(np.flatnonzero((v == [0, 0, 0]).all(axis=1))[0])
        b = int(np.flatnonzero((v == [1, 0, 0]).all(axis=1))[0])
        assert adj.n_edges == 7 and adj.degree[a] == 4 and adj.degree[b] == 4
        assert adj.boundary.tolist() == [1] * 5                                    # through the six outer edges, used once each
        edges, uses = edge_uses(mesh.faces)
        assert uses[(edges == sorted((a, b))).all(axis=1)].tolist() == [3] and sorted(uses.tolist()) == [1] * 6 + [3]
    elif name == "duplicated_face":
        assert adj.degree.tolist() == [2] * 3 and adj.n_edges == 3 and not adj.boundary.any()        # every edge used twice
        assert [r.tolist() for r in mesh.vertex_neighbors] == [[1, 2], [0, 2], [0, 1]]
    else:
        assert adj.offsets.tolist() == [0] and adj.neighbors.shape == (0,) and adj.boundary.shape == (0,) and adj.n_edges == 0
        assert adj.offsets.dtype == np.int32 and adj.neighbors.dtype == np.int32 and adj.boundary.dtype == np.uint8
        assert mesh.vertex_neighbors == []
        out = E.smooth_mesh(mesh, 5)
        assert out.triangles.shape == (0, 3, 3) and out.vertices.shape == (0, 3)
    return mesh


@pytest.mark.parametrize("name", sorted(hand_meshes()))
def test_hand_written_meshes(name):
    mesh = check_hand_mesh(name, E.SimpleMesh)
    assert mesh.adjacency.device_offsets is None


def test_an_edge_used_three_times_is_no_boundary_edge():
    """In the fan of hand_meshes() every vertex also has an edge that is used once, so the flags there say nothing about the
    spine.  Here no edge is used once: a face three times over (every edge used three times), and the fan with each face
    doubled (the spine six times, the outer edges twice) - no flag anywhere."""
    adj = E.mesh_adjacency_host(np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2]]), 3)
    assert adj.n_edges == 3 and not adj.boundary.any() and adj.degree.tolist() == [2, 2, 2]
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [1, 0, 2], [1, 0, 3], [1, 0, 4]])
    adj = E.mesh_adjacency_host(faces, 5)
    assert adj.n_edges == 7 and not adj.boundary.any()
    # and one outer face on its own: its two outer edges are used once, the spine four times
    adj = E.mesh_adjacency_host(np.concatenate([faces[[0, 0, 0]], faces[[1]]]), 5)
    assert adj.boundary.tolist() == [1, 1, 0, 1, 0] and adj.degree.tolist() == [3, 3, 2, 2, 0]


def test_smooth_mesh_returns_a_new_mesh():
    soup, mesh, _ = host_case("sphere17")
    out = E.smooth_mesh(mesh)
    assert isinstance(out, E.SimpleMesh) and out is not mesh and out.device_triangles is None
    assert out._components is None and out._adjacency is None and out._device_weld is None and out.device_vertex_colors is None
    assert out.triangles.dtype == np.float32 and out.triangles.shape == soup.shape
    adj = mesh.adjacency
    moved = E.smooth_vertices_host(mesh.vertices, adj.offsets, adj.neighbors, adj.boundary, 10, 0.5, -0.53, True)
    assert np.array_equal(out.triangles.view(np.uint32), moved[mesh.faces].view(np.uint32))            # the input's face order
    assert np.array_equal(mesh.triangles.view(np.uint32), soup.view(np.uint32))                        # the input is untouched
    zero = E.smooth_mesh(mesh, iterations=0)
    assert np.array_equal(zero.triangles.view(np.uint32), soup.view(np.uint32))
    # pinned boundary vertices stay
    _, clipped, _ = host_case("sphere17_clipped")
    adj = clipped.adjacency
    moved = E.smooth_vertices_host(clipped.vertices, adj.offsets, adj.neighbors, adj.boundary, 10, 0.5, -0.53, True)
    pinned = adj.boundary.astype(bool)
    assert np.array_equal(moved[pinned].view(np.uint32), clipped.vertices[pinned].view(np.uint32))
    assert not np.array_equal(moved[~pinned], clipped.vertices[~pinned])
    free = E.smooth_vertices_host(clipped.vertices, adj.offsets, adj.neighbors, adj.boundary, 10, 0.5, -0.53, False)
    assert not np.array_equal(free[pinned], clipped.vertices[pinned])


def test_sphere17_volumes():
    _, mesh, _ = host_case("sphere17")
    start = mesh.volume
    taubin = E.smooth_mesh(mesh).volume
    laplace = E.smooth_mesh(mesh, mu=None).volume
    print("sphere17 volume: %.5f, 10 Taubin passes %.5f, 10 Laplacian passes %.5f" % (start, taubin, laplace))
    assert abs(taubin - start) <= 0.01 * start
    assert laplace < 0.75 * start
    assert abs(start - 1.73158) < 5e-5 and abs(taubin - 1.74224) < 5e-5 and abs(laplace - 1.21714) < 5e-5


def test_argument_checks():
    _, mesh, _ = host_case("sphere17")
    for bad in (-1, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="iterations"):
            E.smooth_mesh(mesh, iterations=bad)
    for bad in (0.0, -0.5, 1.0001, float("nan"), None, "x"):
        with pytest.raises(ValueError, match="lamb"):
            E.smooth_mesh(mesh, lamb=bad)
    for bad in (0.0, 0.5, -1.0001, float("nan"), "none"):
        with pytest.raises(ValueError, match="mu"):
            E.smooth_mesh(mesh, mu=bad)
    E.smooth_mesh(mesh, iterations=np.int64(1), lamb=1.0, mu=-1.0)                # the ends that are inside


# ---- options ----

def test_the_options_pass_the_safe_check(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["--yaml=%s/options/shape.yaml" % root, "--output_root=%s" % tmp_path]
    cmd = options.parse_arguments(base + ["--eval.smooth_iterations=6", "--eval.smooth_lambda=0.4", "--eval.smooth_mu=none",
                                          "--eval.smooth_free_boundary=true"])
    opt = options.set(cmd, safe_check=True, need_gpu=False)
    assert E._smooth_options(opt) == (6, 0.4, None, False)
    opt = options.set(options.parse_arguments(base + ["--eval.smooth_iterations=4"]), safe_check=True, need_gpu=False)
    assert E._smooth_options(opt) == (4, 0.5, -0.53, True)
    opt = options.set(options.parse_arguments(base + ["--eval.smooth_iterations=4", "--eval.smooth_mu=-0.6"]), need_gpu=False)
    assert E._smooth_options(opt) == (4, 0.5, -0.6, True)
    plain = options.set(options.parse_arguments(base), need_gpu=False)
    for key in ("smooth_iterations", "smooth_lambda", "smooth_mu", "smooth_free_boundary"):
        assert key not in plain.eval and "eval." + key in options.COMMAND_LINE_ONLY        # no yaml file carries them
    assert E._smooth_options(plain) is None and E._component_options(plain) is None
    assert E._smooth_options(edict(dict(eval=dict(range=[-1.5, 1.5])))) is None
    for bad in (dict(smooth_iterations=-1), dict(smooth_iterations=2, smooth_lambda=0.0), dict(smooth_iterations=2, smooth_mu=0.5),
                dict(smooth_iterations=2, smooth_mu="maybe"), dict(smooth_lambda=0.4), dict(smooth_free_boundary=True)):
        with pytest.raises(ValueError):
            E._smooth_options(edict(dict(eval=bad)))
