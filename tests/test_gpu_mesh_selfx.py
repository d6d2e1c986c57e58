"""GPU: the face-against-face kernels (csrc/mesh_selfx.hip) against their checker eval_3D.mesh_self_intersections_host.
Every comparison is equality of integers - the per-face counts, the pair list row for row, the totals - with the pairs examined
never above the brute force's: on marching-cubes meshes raw, simplified, smoothed and doubled, on face counts around the wave,
the workgroup and the scan tile, a single cell, a flat sheet with a blade through it, one huge face among 2,000 small ones,
skipped faces and the empty mesh; the pair list at every kind of capacity; the raw entry points' argument checks; determinism;
residency; the opt-in through Runner and demo.py.

On noise23 the checker runs over an evenly strided subset of the rows, sized as tests/test_gpu_mesh_rays.py sizes its rays."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_mesh_inside import _sheet
from tests.test_gpu_mesh_rays import _case, _strided
from tests.test_mesh_selfx_host_logic import GRID, two_spheres
from zeroshape_amd.utils import eval_3D as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_CASES = ["sphere17", "sphere17_clipped", "scene25", "noise9", "three_valued", "noise23"]
UNTOUCHED = -7


def _u64(lo, hi):
    return (lo & 0xffffffff) | ((hi & 0xffffffff) << 32)


def _raw(vertices, faces, capacity=0):
    """zs_mesh_self_intersections on buffers of the right sizes -> (return code, out_counts [9], face counts, pair rows)."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    v = torch.tensor(np.asarray(vertices, np.float32), device="cuda").reshape(-1, 3).contiguous()
    f = torch.tensor(np.asarray(faces, np.int32), device="cuda").reshape(-1, 3).contiguous()
    n, n_verts = f.shape[0], v.shape[0]
    face_counts = torch.full((n,), UNTOUCHED, dtype=torch.int32, device="cuda")
    rows = torch.full((capacity, 2), UNTOUCHED, dtype=torch.int32, device="cuda")
    counts = torch.full((9,), -1, dtype=torch.int32, device="cuda")
    nbytes = lib.zs_mesh_self_intersections_scratch_bytes(n, capacity)
    assert nbytes % 256 == 0 and nbytes > 0
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    rc = lib.zs_mesh_self_intersections(_lib.ptr(v), _lib.ptr(f), n, n_verts, _lib.ptr(face_counts),
                                        None if capacity == 0 else _lib.ptr(rows), capacity, _lib.ptr(counts),
                                        _lib.ptr(scratch), _lib.current_stream_ptr(v.device))
    torch.cuda.synchronize()
    return rc, counts.tolist(), face_counts.cpu().numpy(), rows.cpu().numpy()


def _assert_counts(counts, rec, n_valid):
    """The nine words against the checker's record over all rows."""
    assert counts[:2] == [rec["skipped_faces"], rec["status"]]
    assert _u64(*counts[2:4]) == rec["crossing_pairs"] and _u64(*counts[4:6]) == rec["coincident_pairs"]
    assert counts[6] == rec["faces_crossed"]
    assert rec["candidates"] <= _u64(*counts[7:9]) <= rec["brute_force"] == n_valid * max(n_valid - 1, 0)


def _assert_raw_parity(vertices, faces, extra=3):
    """The raw entry point against the checker over all rows, the pair list with room to spare -> (counts, face counts, pairs)."""
    want_counts, want_pairs, rec = E.mesh_self_intersections_host(vertices, faces, pairs=True)
    capacity = len(want_pairs) + extra
    rc, counts, face_counts, rows = _raw(vertices, faces, capacity)
    assert rc == 1
    assert np.array_equal(face_counts, want_counts), np.flatnonzero(face_counts != want_counts)[:8]
    _assert_counts(counts, rec, len(want_counts) - rec["skipped_faces"])
    assert np.array_equal(rows[:len(want_pairs)], want_pairs) and np.all(rows[len(want_pairs):] == UNTOUCHED)
    return counts, face_counts, want_pairs


def _assert_mesh_parity(mesh, strided=False):
    """mesh_self_intersections on a GPU mesh against the checker on its host copy (all rows, or an evenly strided subset:
    then the per-face counts of those rows and the pairs that begin at them) -> the checked totals."""
    done = E.mesh_self_intersections(mesh, pairs=True)
    got = done.check()
    vertices, faces = mesh.vertices, mesh.faces
    rows = _strided(len(faces), len(faces)) if strided else None
    want_counts, want_pairs, rec = E.mesh_self_intersections_host(vertices, faces, rows=rows, pairs=True)
    face_counts, pairs = done.face_counts.cpu().numpy(), done.pairs.cpu().numpy()
    assert pairs.shape == (got["n_pairs"], 2) and not got["truncated"]
    assert np.all(pairs[:, 0] < pairs[:, 1]) and np.array_equal(pairs, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))])
    assert np.array_equal(np.bincount(pairs.reshape(-1), minlength=len(faces)), face_counts)       # the list and the counts agree
    assert got["n_faces_crossed"] == int((face_counts > 0).sum()) and got["skipped_faces"] == rec["skipped_faces"] == 0
    if rows is None:
        assert np.array_equal(face_counts, want_counts) and np.array_equal(pairs, want_pairs)
        assert (got["n_pairs"], got["n_coincident"]) == (rec["crossing_pairs"], rec["coincident_pairs"])
        assert rec["candidates"] <= got["examined"] <= rec["brute_force"]
    else:
        assert 500 < len(rows) < len(faces)
        assert np.array_equal(face_counts[rows], want_counts), rows[np.flatnonzero(face_counts[rows] != want_counts)[:8]]
        assert np.array_equal(pairs[np.isin(pairs[:, 0], rows)], want_pairs)
        assert got["examined"] <= len(faces) * (len(faces) - 1)
    return got


def _simplified(tris, name, cells, position="quadric"):
    edge = 3.0 / GRID[name]
    return E.simplify_mesh(E.SimpleMesh(tris), cells * edge, origin=(-1.5 - 0.5 * edge,) * 3, position=position)


def _random_soup(n, seed, density=40.0, size=0.3):
    """n triangles of about ``size`` across whose centres fill a box at ``density`` per unit volume, with a few twins."""
    rng = np.random.RandomState(seed)
    side = (n / density) ** (1.0 / 3.0)
    soup = (rng.uniform(0, side, (n, 1, 3)) + rng.uniform(-size, size, (n, 3, 3))).astype(np.float32)
    if n >= 8:
        soup[n // 2] = soup[1][::-1]
        soup[n - 1] = soup[2][[1, 2, 0]]
    return soup.reshape(-1, 3), np.arange(3 * n).reshape(n, 3)


# ---- parity with the checker ----

@pytest.mark.parametrize("name", RAW_CASES)
def test_raw_marching_cubes_meshes(name):
    _, tris, _ = _case(name)
    got = _assert_mesh_parity(E.SimpleMesh(tris), strided=name == "noise23")
    assert got["n_pairs"] == 0 and got["n_faces_crossed"] == 0       # the oracle without the checker
    assert got["n_coincident"] == {"three_valued": 12, "noise23": 38}.get(name, 0)


@pytest.mark.parametrize("name,position,want", [("three_valued", "quadric", (27, 34, 26)), ("three_valued", "mean", (27, 36, 26)),
                                                ("noise9", "quadric", (3, 4, 29)), ("noise9", "mean", (0, 0, 29))])
def test_simplified_meshes(name, position, want):
    got = _assert_mesh_parity(_simplified(_case(name)[1], name, 2, position))
    assert (got["n_pairs"], got["n_faces_crossed"], got["n_coincident"]) == want


@pytest.mark.parametrize("aligned,want", [(False, (128, 123)), (True, (147, 114))])
def test_two_spheres(aligned, want):
    got = _assert_mesh_parity(E.SimpleMesh(torch.from_numpy(two_spheres(aligned)).cuda()))
    assert (got["n_pairs"], got["n_faces_crossed"], got["n_coincident"]) == want + (0,)
    # the soup without a weld: every face on vertices of its own
    soup = two_spheres(aligned).reshape(-1, 3)
    counts, _, pairs = _assert_raw_parity(soup, np.arange(len(soup)).reshape(-1, 3))
    assert len(pairs) == want[0]


def test_noise23_after_ten_taubin_passes():
    mesh = E.smooth_mesh(E.SimpleMesh(_case("noise23")[1]), 10, 0.5, -0.53)
    got = _assert_mesh_parity(mesh, strided=True)
    assert (got["n_pairs"], got["n_faces_crossed"], got["n_coincident"]) == (4, 5, 38)


# ---- sizes and shapes ----

@pytest.mark.parametrize("n_faces", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049])
def test_face_counts_around_the_wave_the_workgroup_and_the_scan_tile(n_faces):
    """(the run lengths are scanned over n_faces + 1 elements in tiles of 2,048: 2,048 faces are one step past the tile)"""
    vertices, faces = _random_soup(n_faces, n_faces)
    counts, face_counts, pairs = _assert_raw_parity(vertices, faces)
    assert counts[:2] == [0, 0] and (len(pairs) > 0) == (n_faces >= 63)
    if n_faces >= 8:
        assert _u64(*counts[4:6]) == 2


def test_a_single_cell():
    """Fewer than sixteen faces make one cell: every face reads every other."""
    vertices, faces = _random_soup(12, 3, density=400.0)
    counts, face_counts, pairs = _assert_raw_parity(vertices, faces)
    assert _u64(*counts[7:9]) == 12 * 11 and len(pairs) > 3
    # 400 triangles whose boxes share one centre fall into one cell of many
    rng = np.random.RandomState(6)
    a = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    b = a * rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    counts, face_counts, pairs = _assert_raw_parity(np.stack([a, b, -a], axis=1).reshape(-1, 3), np.arange(1200).reshape(400, 3))
    assert _u64(*counts[7:9]) == 400 * 399 and len(pairs) > 400


def test_an_axis_without_extent():
    """A flat sheet in each of the three planes: coplanar neighbours, no crossing; then the same sheet with a blade through
    it, which crosses the faces along its cut and nothing else."""
    grid, faces = _sheet()
    for axis in range(3):
        flat = np.insert(grid, axis, np.float32(1.5), axis=1)
        counts, face_counts, pairs = _assert_raw_parity(flat, faces)
        assert len(pairs) == 0 and 0 < _u64(*counts[7:9]) < len(faces) * (len(faces) - 1)         # the cells still prune
        blade = np.array([[0.3, 1.1, 0.0], [5.2, 4.3, 0.0], [2.0, 3.0, 0.0]], np.float32)          # (u, v, height)
        blade[:, 2] = [-1.0, -1.0, 2.0]
        blade = np.insert(blade[:, :2], axis, blade[:, 2] + np.float32(1.5), axis=1)
        both = np.concatenate([flat, blade]).astype(np.float32)
        cut = np.concatenate([faces, [[len(flat), len(flat) + 1, len(flat) + 2]]])
        counts, face_counts, pairs = _assert_raw_parity(both, cut)
        assert face_counts[-1] == len(pairs) > 10 and np.all(pairs[:, 1] == len(faces)) and np.all(face_counts[:-1] <= 1)


def test_one_face_that_spans_the_box_among_2000_small_ones():
    """The reaches of the huge face are half the grid each way: every thread reads most of the grid - slow, still the
    checker's integers; its run of the pair list is long, and in order wherever the face stands."""
    rng = np.random.RandomState(7)
    centres = rng.uniform(-1, 1, (2000, 1, 3))
    small = (centres + rng.uniform(-0.12, 0.12, (2000, 3, 3))).astype(np.float32)
    huge = np.array([[[-1.2, -1.2, -1.2], [1.2, -1.2, -1.1], [0.1, 1.2, 1.2]]], np.float32)
    without, _, _ = _assert_raw_parity(small.reshape(-1, 3), np.arange(6000).reshape(-1, 3))
    assert _u64(*without[7:9]) < 0.1 * 2000 * 1999
    for at, soup in ((1000, np.concatenate([small[:1000], huge, small[1000:]])), (0, np.concatenate([huge, small])),
                     (2000, np.concatenate([small, huge]))):
        verts = soup.reshape(-1, 3)
        counts, face_counts, pairs = _assert_raw_parity(verts, np.arange(len(verts)).reshape(-1, 3))
        assert face_counts[at] > 60 and face_counts[at] == int(((pairs[:, 0] == at) | (pairs[:, 1] == at)).sum())
        print("pairs examined: %d with the huge face (it crosses %d), %d without, of %d"
              % (_u64(*counts[7:9]), face_counts[at], _u64(*without[7:9]), 2001 * 2000))


def test_skipped_faces_and_the_empty_mesh():
    vertices, faces = _random_soup(300, 11)
    vertices, faces = vertices.copy(), faces.astype(np.int64).copy()
    faces[5, 1], faces[17, 0], faces[40, 2], faces[299, 0] = -1, len(vertices), 2 ** 31 - 1, -2 ** 31
    vertices[faces[60, 0], 1], vertices[faces[61, 2], 0], vertices[faces[250, 1], 2] = np.nan, np.inf, -np.inf
    counts, face_counts, pairs = _assert_raw_parity(vertices, faces)
    bad = [5, 17, 40, 299, 60, 61, 250]
    assert counts[:2] == [7, 3] and np.all(face_counts[bad] == 0) and not np.isin(pairs, bad).any() and len(pairs) > 20
    # only a corner that is not finite: status 1; no valid face at all
    vertices2, faces2 = _random_soup(40, 12)
    vertices2[0, 0] = np.nan
    counts, _, _ = _assert_raw_parity(vertices2, faces2)
    assert counts[:2] == [1, 1]
    counts, face_counts, _ = _assert_raw_parity(np.full((9, 3), np.nan, np.float32), np.arange(9).reshape(3, 3))
    assert counts == [3, 1, 0, 0, 0, 0, 0, 0, 0] and face_counts.tolist() == [0, 0, 0]
    # n_faces = 0: nine zeros, nothing else is touched
    rc, counts, face_counts, rows = _raw(np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32), capacity=5)
    assert rc == 1 and counts == [0] * 9 and face_counts.shape == (0,) and np.all(rows == UNTOUCHED)
    empty = E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda"))
    done = E.mesh_self_intersections(empty, pairs=True)
    assert done.face_counts.shape == (0,) and done.pairs.shape == (0, 2) and done.check()["n_pairs"] == 0
    assert empty.is_self_intersecting() is False


# ---- the pair list ----

def test_the_pair_list_at_every_capacity():
    host = E.SimpleMesh(two_spheres(False))
    vertices, faces = host.vertices, host.faces
    want_counts, want, rec = E.mesh_self_intersections_host(vertices, faces, pairs=True)
    assert len(want) == 128 and np.array_equal(want, want[np.lexsort((want[:, 1], want[:, 0]))]) and np.all(want[:, 0] < want[:, 1])
    for capacity in (128, 127, 100, 1, 129, 200):
        rc, counts, face_counts, rows = _raw(vertices, faces, capacity)
        assert rc == 1 and _u64(*counts[2:4]) == 128 and np.array_equal(face_counts, want_counts)
        assert np.array_equal(rows[:min(capacity, 128)], want[:capacity]) and np.all(rows[128:] == UNTOUCHED)
    # no list: capacity 0 with a null pointer; the totals are all there
    rc, counts, face_counts, rows = _raw(vertices, faces, 0)
    assert rc == 1 and _u64(*counts[2:4]) == 128 and counts[6] == 123 and np.array_equal(face_counts, want_counts)
    # the faces in another order: the list is still in order (the records of a cell are not)
    perm = np.random.RandomState(3).permutation(len(faces))
    _assert_raw_parity(vertices, faces[perm])
    # through Python: the two calls, a given capacity, truncation
    mesh = E.SimpleMesh(torch.from_numpy(two_spheres(False)).cuda())
    full = E.mesh_self_intersections(mesh, pairs=True)
    assert full.pairs.dtype == torch.int32 and full.pairs.shape == (128, 2) and full.check()["truncated"] is False
    listed = mesh.get_self_intersecting_triangles()
    assert listed.dtype == np.int64 and np.array_equal(listed, full.pairs.cpu().numpy()) and mesh.is_self_intersecting() is True
    short = E.mesh_self_intersections(mesh, capacity=50)
    assert short.check()["truncated"] is True and np.array_equal(short.pairs.cpu().numpy(), listed[:50])
    roomy = E.mesh_self_intersections(mesh, pairs=True, capacity=130)
    assert roomy.check()["truncated"] is False and np.array_equal(roomy.pairs.cpu().numpy()[:128], listed)
    assert torch.all(roomy.pairs[128:] == -1)
    assert E.mesh_self_intersections(mesh, capacity=0).pairs.shape == (0, 2) and E.mesh_self_intersections(mesh).pairs is None
    with pytest.raises(ValueError, match="capacity"):
        E.mesh_self_intersections(mesh, capacity=-1)


# ---- pruning, arguments, determinism, residency ----

SHARE = 0.0063   # measured: 3,656,187 ordered pairs examined over 34,278 x 34,277 / 2 = 0.6224 %


def test_pruning_is_real():
    """Not a performance claim: the grid leaves most pairs unread.  Measured once on noise23: SHARE of the F (F - 1) / 2
    pairs (the kernel counts ordered pairs: each pair from both sides); the bound is twice that."""
    _, tris, host = _case("noise23")
    F = len(host.faces)
    got = E.mesh_self_intersections(E.SimpleMesh(tris)).check()
    share = got["examined"] / (F * (F - 1) / 2.0)
    print("noise23: %d faces, %d ordered pairs examined, %.4f %% of F (F - 1) / 2" % (F, got["examined"], 100.0 * share))
    assert 0 < got["examined"] <= F * (F - 1)
    assert share < 2 * SHARE


def test_argument_checks_of_the_raw_entry_points():
    """0 and a message that names the entry point, before anything is launched (a host buffer stands in for every non-null
    pointer: nothing may read it)."""
    from zeroshape_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p, odd = ctypes.c_void_p(base + (-base) % 8), ctypes.c_void_p(base + (-base) % 8 + 4)

    def fails(rc, what):
        msg = lib.zs_last_error()
        assert rc == 0 and msg.startswith(b"zs_mesh_self_intersections: ") and what.encode() in msg, (what, rc, msg)

    def call(n=1, v=3, capacity=1, ptr=p, scratch=p, **null):
        args = dict(vertices=ptr, faces=ptr, out_face_counts=ptr, out_pairs=ptr, out_counts=ptr)
        args.update(null)
        return lib.zs_mesh_self_intersections(args["vertices"], args["faces"], n, v, args["out_face_counts"], args["out_pairs"],
                                              capacity, args["out_counts"], scratch, None)

    fails(call(n=-1), "negative size")
    fails(call(v=-3), "negative size")
    fails(call(capacity=-1), "negative size")
    fails(call(n=2 ** 24 + 1), "too large")
    fails(call(capacity=2 ** 30 + 1), "too large")
    for name in ("vertices", "faces", "out_face_counts", "out_pairs", "out_counts"):
        fails(call(**{name: None}), "null pointer")
    fails(call(n=0, out_counts=None), "null pointer")
    fails(call(n=0, out_pairs=None), "null pointer")                 # a capacity without a list
    fails(call(scratch=None), "null pointer")
    fails(call(scratch=odd), "8-byte aligned")
    fails(call(scratch=odd, out_pairs=None, capacity=0), "8-byte aligned")       # no list is allowed: the next check speaks
    size = lib.zs_mesh_self_intersections_scratch_bytes
    assert size(-1, 0) == 0 and size(1, -1) == 0 and size(2 ** 24 + 1, 0) == 0 and size(1, 2 ** 30 + 1) == 0
    for n, c in ((0, 0), (1, 1), (17, 3), (2 ** 24, 2 ** 30), (100, 0)):
        assert size(n, c) > 0 and size(n, c) % 256 == 0
    assert size(2 ** 24, 0) > size(2 ** 20, 0) > size(1, 0) and size(1000, 0) == size(1000, 2 ** 30)     # the face count alone


def test_two_runs_give_the_same_bytes():
    _, tris, _ = _case("noise23")
    smooth = E.smooth_mesh(E.SimpleMesh(tris), 10, 0.5, -0.53).device_triangles
    for soup in (smooth, _simplified(tris, "noise23", 2).device_triangles):
        a, b = (E.mesh_self_intersections(E.SimpleMesh(soup), pairs=True) for _ in range(2))
        assert a.check()["n_pairs"] > 0
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_the_results_are_resident_and_the_mesh_keeps_its_weld():
    mesh = E.SimpleMesh(torch.from_numpy(two_spheres(False)).cuda())
    before = set(vars(mesh))
    done = mesh.self_intersections
    assert isinstance(done, E.MeshSelfIntersections) and done.pairs is None and done.face_counts.is_cuda and done.counts.is_cuda
    assert done.face_counts.dtype == torch.int32 and done.counts.dtype == torch.int32 and done.counts.shape == (9,)
    assert mesh._device_weld is not None and set(vars(mesh)) == before             # the weld it made is kept; nothing else
    assert mesh._triangles is None and mesh._indexed is None and mesh._components is None and mesh._adjacency is None
    weld = mesh._device_weld
    assert mesh.self_intersections is done                           # computed once
    with_list = E.mesh_self_intersections(mesh, pairs=True)
    assert with_list.pairs.is_cuda and mesh._device_weld is weld and mesh._triangles is None and mesh._indexed is None
    assert done.check() == dict(with_list.check(), truncated=False)


# ---- the opt-in ----

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
            opt.eval.mesh_self_intersections = True
        r = Runner(opt)
        r.load_dataset(opt, dataset=Dataset(opt, n_items=2, n_points=1000))
        r.build_networks(opt)
        r.graph.load_state_dict(full, strict=True)
        r.evaluate(opt)
        reports[flag] = [json.load(open(out / "dump_synthetic" / ("%d_mesh_report.json" % i))) for i in (0, 1)]
    for off, on in zip(reports[False], reports[True]):
        assert "self_intersections" not in off
        assert set(on) == set(off) | {"self_intersections"} and (on["faces"], on["vertices"]) == (off["faces"], off["vertices"])
        record = on["self_intersections"]
        assert set(record) == {"crossing_pairs", "faces_crossed", "coincident_pairs", "skipped_faces"}       # no step ran
        assert record["crossing_pairs"] == record["faces_crossed"] == record["skipped_faces"] == 0           # marching cubes


def test_demo_script_writes_the_entry(tmp_path, encoder_sd, seeded_sd):
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
                        "--output_root=%s" % tmp_path, "--eval.mesh_self_intersections=true", "--eval.simplify_cells=2",
                        "--eval.mesh_report=true"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    report = json.load(open(tmp_path / "data" / "preds" / "blob_mesh_report.json"))
    record = report["self_intersections"]
    print("demo.py: self_intersections", record)
    four = {"crossing_pairs", "faces_crossed", "coincident_pairs", "skipped_faces"}
    assert set(record) == four | {"before"} and set(record["before"]) == four and "simplification" in report
    assert record["before"]["crossing_pairs"] == record["before"]["faces_crossed"] == 0            # marching cubes' own mesh
    assert record["skipped_faces"] == 0 and record["crossing_pairs"] >= (record["faces_crossed"] + 1) // 2
    assert "reprojection" not in report and "deviation" not in report
