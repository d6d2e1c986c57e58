"""Host checks of the marching-cubes tables and the numpy oracle (no GPU)."""
import numpy as np

from oracle import mc_ref as M
from zeroshape_amd import mc_tables as T


def test_tables_are_consistent():
    assert T.MAX_TRIS == 5 and T.TRI_COUNT[0] == 0 and T.TRI_COUNT[255] == 0
    for c in range(256):
        ins = [(c >> i) & 1 for i in range(8)]
        cross = {e for e, (a, b) in enumerate(T.EDGES) if ins[a] != ins[b]}
        used = set(T.TRI_TABLE[c][T.TRI_TABLE[c] >= 0].tolist())
        assert cross == used                       # every sign change is meshed, nothing else
        assert (T.TRI_TABLE[c] >= 0).sum() == 3 * T.TRI_COUNT[c]


def test_oracle_derives_its_own_tables_and_they_are_the_products():
    """oracle/mc_ref.py no longer imports the product's tables: it derives the 256 cases itself
    (geometric faces, marching squares per face, cross-product orientation) - and arrives at the same tables, entry for
    entry, so every bit-for-bit triangle comparison of the GPU kernel now runs against independently derived cases."""
    src = open(M.__file__.replace(".pyc", ".py")).read()
    assert "import mc_tables" not in src and "from zeroshape_amd" not in src
    np.testing.assert_array_equal(M.TRI_TABLE, T.TRI_TABLE)
    np.testing.assert_array_equal(M.TRI_COUNT, T.TRI_COUNT)
    np.testing.assert_array_equal(M.CORNERS, T.CORNERS)
    assert [tuple(sorted((int(a), int(b)))) for a, b in zip(M._EA, M._EB)] == [tuple(sorted(e)) for e in T.EDGES.tolist()]


def test_tables_are_crack_free_for_every_sign_pattern():
    """The table-independent verifier on the PRODUCT's tables: per case a consistently oriented manifold whose boundary is
    exactly the six faces' contour segments; for all 256 x 3 x 16 neighbour pairs the shared face carries the same
    segments reversed - crack-freeness and winding for every sign pattern, exhaustively (not on a sphere)."""
    assert M.verify_case_tables(T.TRI_TABLE, T.TRI_COUNT) == []
    # the face rule itself (case 1 = only corner 0 has its bit set, i.e. a value BELOW the iso level): the three segments
    # circle corner 0 and the triangle's normal points towards it - towards decreasing values, which for an occupancy grid
    # (occ > 0.5 inside the object) is out of the object
    segs = M.case_segments(1)
    assert sorted(e for s in segs for e in s) == [0, 0, 3, 3, 8, 8]
    tri = T.TRI_TABLE[1][:3]
    p = np.array([M._mid(int(e)) for e in tri])
    normal = np.cross(p[1] - p[0], p[2] - p[0])
    assert np.dot(normal, M.CORNERS[0] - p.mean(0)) > 0


def test_any_single_table_entry_perturbed_is_caught():
    """Every single-entry change of every row (each of the 11 other edge ids, and -1), every swap of two entries of a
    triangle (flipped winding), a dropped or duplicated triangle: verify_case reports it.  (What a row may change without
    being wrong - which diagonal a loop's fan uses, the order of its triangles - is pinned by the table equality above.)"""
    tried = 0
    for case in range(256):
        n = int(T.TRI_COUNT[case])
        base = T.TRI_TABLE[case].astype(np.int64)
        assert M.verify_case(case, base, n) == []
        for pos in range(3 * n):
            for val in list(range(12)) + [-1]:
                if val == base[pos]:
                    continue
                row = base.copy()
                row[pos] = val
                assert M.verify_case(case, row, n), (case, pos, val)
                tried += 1
        for t in range(n):
            row = base.copy()
            row[3 * t], row[3 * t + 1] = base[3 * t + 1], base[3 * t]
            assert M.verify_case(case, row, n), (case, t, "winding")
            row = base.copy()                                            # triangle t removed, the rest moved up
            row[3 * t:3 * n - 3] = base[3 * t + 3:3 * n]
            row[3 * n - 3:3 * n] = -1
            assert M.verify_case(case, row, n - 1), (case, t, "dropped")
            if n < M.MAX_TRIS:
                row = base.copy()
                row[3 * n:3 * n + 3] = base[3 * t:3 * t + 3]
                assert M.verify_case(case, row, n + 1), (case, t, "duplicated")
        if n:
            assert M.verify_case(case, base, n - 1) and M.verify_case(case ^ 1, base, n)
    assert tried > 25000
    # ... and a whole-table change that keeps every row valid by itself but breaks a shared face cannot exist under this
    # check: a row's boundary is pinned to the face rule, and the rule reads the four shared corners only (the neighbour
    # sweep of verify_case_tables confirms it on the table itself)
    bad = T.TRI_TABLE.copy()
    bad[1, :3] = bad[1, [1, 0, 2]]
    errs = M.verify_case_tables(bad, T.TRI_COUNT)
    assert any(e.startswith("case 1:") for e in errs) and any("disagree on their shared face" in e for e in errs)


def _sphere(G, r, c=None):
    ax = np.linspace(-1.5, 1.5, G, dtype=np.float32)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    c = c or (0.1, -0.05, 0.2)
    d = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)
    return (1.0 / (1.0 + np.exp((d - r) * 20.0))).astype(np.float32), ax     # >0.5 inside, like occ


def _noise(G, seed):
    return np.random.RandomState(seed).uniform(0, 1, (G, G, G)).astype(np.float32)       # every case, incl. ambiguous ones


def _three_valued(G, seed):
    """Corner values exactly ON the iso level 0.5 (never below it): vertices on grid corners, zero-area triangles."""
    return np.random.RandomState(seed).choice(np.float32([0.0, 0.5, 1.0]), size=(G, G, G)).astype(np.float32)


def _non_finite(G, seed):
    """Noise with one NaN, one +inf and one -inf, away from each other and from the faces."""
    vol = _noise(G, seed)
    vol[2, 3, 4], vol[G - 3, 2, G - 2], vol[G // 2, G - 3, 1] = np.nan, np.inf, -np.inf
    return vol


def _wide_range(G, seed):
    """Values in [-2, 3]: for an iso level and a world range other than the pipeline's 0.5 and (-1.5, 1.5)."""
    return np.random.RandomState(seed).uniform(-2, 3, (G, G, G)).astype(np.float32)


WIDE_ISO, WIDE_RANGE = 0.3, (-0.7, 2.1)          # 0.3 is not a float32: both sides round it the same way or the cases differ


def _field_f(G, slab=6, share=0.5):
    """A sphere of radius 1.7 in the [-1.5, 1.5] box - it cuts all six faces of the grid - with about `share` of the
    values in the last `slab` k-columns replaced by uniform noise: surface in the first and last cubes of the k-rows (the
    row ends the count pass reads apart from the rest) and in the first and last i / j slabs."""
    vol = _sphere(G, 1.7, c=(0.1, -0.05, 0.2))[0]
    rs = np.random.RandomState(1000 + G)
    shape = (G, G, slab)
    noise = rs.uniform(0, 1, shape).astype(np.float32)
    vol[:, :, G - slab:] = np.where(rs.uniform(0, 1, shape) < share, noise, vol[:, :, G - slab:])
    return vol


def soup_cube_census(tris, G, lo=-1.5, hi=1.5):
    """How many triangles of a soup of marching_cubes(vol, iso, (hi - lo) / G, lo) lie, strictly, in the last cube of a
    k-row and in the first / last slab of cubes along i and j.  A triangle of cube index c along an axis has its
    coordinates in [plane(c), plane(c + 1)]; counted are those inside the slab with a vertex off its inner plane."""
    scale = np.float32((hi - lo) / G)
    plane = lambda c: M._fma32(np.float32(c), scale, np.float32(lo))      # noqa: E731  (monotonic in c, as the vertices are)
    mn, mx = tris.min(axis=1), tris.max(axis=1)                              # [n,3]
    first = lambda a: int(((mx[:, a] <= plane(1)) & (mn[:, a] < plane(1))).sum())              # noqa: E731
    last = lambda a: int(((mn[:, a] >= plane(G - 2)) & (mx[:, a] > plane(G - 2))).sum())       # noqa: E731
    return dict(row_end=last(2), i_first=first(0), i_last=last(0), j_first=first(1), j_last=last(1))


def test_sphere_mesh_is_closed_and_accurate():
    G = 17
    vol, ax = _sphere(G, 0.8)
    # unit-scale world transform (index -> linspace coordinate) to check geometry
    step = float(ax[1] - ax[0])
    tris = M.marching_cubes(vol, 0.5, step, float(ax[0]))
    assert len(tris) > 100
    r = np.linalg.norm(tris.reshape(-1, 3) - np.array([0.1, -0.05, 0.2]), axis=1)
    assert np.abs(r - 0.8).max() < 0.03            # vertices sit on the iso-sphere (linear interp)
    # watertight: every undirected edge is shared by exactly two triangles, with opposite
    # directions (consistent winding) - possible to check exactly because shared vertices are
    # bit-identical
    edges = {}
    for t in tris:
        for a in range(3):
            p, q = tuple(t[a]), tuple(t[(a + 1) % 3])
            edges[(p, q)] = edges.get((p, q), 0) + 1
    assert all(v == 1 for v in edges.values())
    assert all((q, p) in edges for (p, q) in edges)
    # area ~ 4 pi r^2
    assert abs(M.triangle_areas(tris).sum() - 4 * np.pi * 0.64) / (4 * np.pi * 0.64) < 0.03


def test_reference_vertex_scaling_gotcha():
    """vertices are index / S * (max - min) + min with S = G, not G - 1 (utils/eval_3D.py:252-255)."""
    G = 9
    vol, _ = _sphere(G, 0.8, c=(0, 0, 0))
    tris = M.marching_cubes(vol, 0.5, np.float32(3.0 / G), -1.5)
    v = tris.reshape(-1, 3)
    # the sphere is centred in index space at (G-1)/2 -> world centre = (G-1)/2 * 3/G - 1.5 = -1.5/G
    np.testing.assert_allclose(v.mean(0), [-1.5 / G] * 3, atol=0.03)


def test_sampling_is_area_weighted_and_on_surface():
    G = 13
    vol, ax = _sphere(G, 0.9, c=(0, 0, 0))
    step = float(ax[1] - ax[0])
    tris = M.marching_cubes(vol, 0.5, step, float(ax[0]))
    pts, ids = M.sample_surface(tris, 4000, seed=3)
    # on the triangles it claims
    for s in range(0, 4000, 97):
        a, b, c = tris[ids[s]].astype(np.float64)
        n = np.cross(b - a, c - a)
        assert abs(np.dot(pts[s] - a, n)) / (np.linalg.norm(n) + 1e-30) < 1e-5
    r = np.linalg.norm(pts, axis=1)
    assert np.abs(r - 0.9).max() < 0.06
    # octant occupancy ~ uniform
    occ = np.bincount((pts[:, 0] > 0) * 4 + (pts[:, 1] > 0) * 2 + (pts[:, 2] > 0), minlength=8) / 4000.0
    assert np.abs(occ - 0.125).max() < 0.03
    # empty mesh -> zeros
    z, _ = M.sample_surface(np.zeros((0, 3, 3), np.float32), 5, 0)
    assert z.shape == (5, 3) and not z.any()


def test_vectorised_extraction_and_sampling_equal_the_loops_bit_for_bit():
    """oracle/mc_ref.py extracts all cubes (and draws all samples) at once since round 4 so that the pipeline tests run at
    vox 64 / 128; the cube-by-cube and sample-by-sample forms it replaced stay as its check."""
    import numpy as np
    from oracle import mc_ref as M
    rs = np.random.RandomState(0)
    for G in (5, 8, 11):
        ax = np.linspace(-1.5, 1.5, G)
        x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
        vol = (1.0 / (1.0 + np.exp(20 * (np.sqrt(x * x + 1.3 * y * y + 0.8 * z * z) - 0.9))) + 0.05 * rs.randn(G, G, G)).astype(np.float32)
        a = M.marching_cubes(vol, 0.5, np.float32(3.0 / G), -1.5)
        b = M.marching_cubes_loop(vol, 0.5, np.float32(3.0 / G), -1.5)
        assert a.shape == b.shape and len(a) > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        p1, i1 = M.sample_surface(a, 300, seed=G)
        p2, i2 = M.sample_surface_loop(b, 300, seed=G)
        assert np.array_equal(i1, i2) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    assert len(M.marching_cubes(np.zeros((4, 4, 4), np.float32), 0.5, np.float32(1.0), 0.0)) == 0


def test_vectorised_extraction_equals_the_loop_on_level_values_non_finite_values_and_another_level():
    """The inputs tests/test_gpu_mc_full_size.py adds, at G = 6: corner values exactly on the level (zero-area triangles),
    a NaN and both infinities (NaN vertices: compared as NaN, everything else bit for bit), and the iso level 0.3 with the
    world range (-0.7, 2.1)."""
    G = 6
    for vol, iso, (lo, hi) in ((_three_valued(G, G), 0.5, (-1.5, 1.5)), (_non_finite(G, G), 0.5, (-1.5, 1.5)),
                               (_wide_range(G, G), WIDE_ISO, WIDE_RANGE)):
        scale = np.float32((hi - lo) / G)
        with np.errstate(all="ignore"):
            a = M.marching_cubes(vol, iso, scale, lo)
            b = M.marching_cubes_loop(vol, iso, scale, lo)
        assert a.shape == b.shape and len(a) > 50
        nan = np.isnan(a)
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(nan, np.isnan(b))
        assert np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])
        assert nan.any() == (not np.isfinite(vol).all())
    tv = M.marching_cubes(_three_valued(G, G), 0.5, np.float32(3.0 / G), -1.5)
    assert (M.triangle_areas(tv) == 0).sum() > 5


def test_vectorised_sampling_equals_the_loop_past_one_scan_tile_with_zero_area_triangles():
    """300 samples on a soup of more than 2,048 triangles (what the device scans as one tile) that has zero-area ones:
    the same ids and the same bits, and no id on a triangle without area."""
    tris = M.marching_cubes(_three_valued(13, 13), 0.5, np.float32(3.0 / 13), -1.5)
    area = M.triangle_areas(tris)
    assert len(tris) > 2048 and (area == 0).sum() > 100
    for seed in (7, 2 ** 64 - 1):
        p1, i1 = M.sample_surface(tris, 300, seed)
        p2, i2 = M.sample_surface_loop(tris, 300, seed)
        assert np.array_equal(i1, i2) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
        assert (area[i1] > 0).all() and i1.max() >= 2048


def test_full_size_field_has_surface_at_the_row_ends_and_on_every_face():
    """_field_f (the volume of the 129^3 and 253^3 .. 258^3 GPU cases), checked small: triangles in the last cube of the
    k-rows and in the first and last slabs of cubes along i and j; and soup_cube_census counts cubes, not vertices - a
    closed sphere away from the faces has none there."""
    G = 33
    census = soup_cube_census(M.marching_cubes(_field_f(G), 0.5, np.float32(3.0 / G), -1.5), G)
    assert census["row_end"] > 1000 and min(census.values()) > 100, census
    inner = soup_cube_census(M.marching_cubes(_sphere(G, 0.8)[0], 0.5, np.float32(3.0 / G), -1.5), G)
    assert set(inner.values()) == {0}
    # one triangle in each place, by hand: cube (0, 3, G - 2) and cube (G - 2, 0, 5)
    P = lambda *v: M._fma32(np.float32(v), np.float32(3.0 / G), np.float32(-1.5))      # noqa: E731
    t = np.stack([np.stack([P(0.5, 3, G - 2), P(1, 3.5, G - 2), P(1, 3, G - 1.5)]),
                  np.stack([P(G - 2, 0.5, 5), P(G - 1.5, 0, 5), P(G - 2, 0, 5.5)])]).astype(np.float32)
    assert soup_cube_census(t[:1], G) == dict(row_end=1, i_first=1, i_last=0, j_first=0, j_last=0)
    assert soup_cube_census(t[1:], G) == dict(row_end=0, i_first=0, i_last=1, j_first=1, j_last=0)


def test_simple_mesh_is_indexed_like_mcubes():
    """utils/eval_3D.py:250-256: mcubes.marching_cubes returns welded (vertices, triangles); SimpleMesh welds the kernel's soup
    lazily (unique rows: shared vertices are bit-identical) and keeps the triangle set."""
    import numpy as np
    from oracle import mc_ref as M
    from zeroshape_amd.utils.eval_3D import SimpleMesh
    G = 20
    vol = _sphere(G, 0.9, c=(0, 0, 0))[0]
    tris = M.marching_cubes(vol, 0.5, np.float32(3.0 / G), -1.5)
    m = SimpleMesh(tris)
    assert len(m.faces) == len(tris) and len(m.vertices) < 3 * len(tris)
    assert len(np.unique(m.vertices.view(np.uint32), axis=0)) == len(m.vertices)
    assert np.array_equal(m.vertices[m.faces].view(np.uint32), (tris + np.float32(0)).view(np.uint32))
    assert len(m.vertices) - len(m.faces) // 2 == 2          # closed genus-0 surface: V - E + F = 2 with E = 3F/2
    e = SimpleMesh(np.zeros((0, 3, 3), np.float32))
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3)
