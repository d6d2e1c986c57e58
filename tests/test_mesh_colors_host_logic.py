"""eval_3D.mesh_vertex_colors_host - the float64 numpy definition of the vertex colours and the checker of
csrc/mesh_colors.hip - on scenes with known answers (tests/mesh_colors_cases.py).  No GPU."""
import numpy as np
import pytest

from tests import mesh_colors_cases as C
from zeroshape_amd.utils import eval_3D as E


def run(scene):
    return E.mesh_vertex_colors_host(**scene)


def test_fronto_parallel_square_takes_the_texels_of_its_corners():
    s = C.scene(C.square(*C.FRONT, 2.0))
    out = run(s)
    assert out["seen"].all() and (out["source"] == np.arange(4)).all()
    for u, w in C.corners(C.FRONT):
        k = C.find(s["vertices"], u, w, 2.0)
        assert (out["u"][k], out["w"][k], out["Z"][k]) == (u, w, 2.0)
        assert (out["colors"][k] == C.texel(w, u)).all()
    assert out["seen_area"] == out["total_area"] == 4.0 * 3.0             # mesh units: (8 px * 2 / 8 / 0.5) x (6 px * 2 / 8 / 0.5)


def test_half_integer_pixels_give_the_rounded_four_texel_mean():
    s = C.scene(C.square(4.5, 3.5, 12.5, 9.5, 2.0))
    out = run(s)
    assert out["seen"].all()
    img = s["image"].astype(np.float64)
    for u, w in C.corners((4.5, 3.5, 12.5, 9.5)):
        k = C.find(s["vertices"], u, w, 2.0)
        i, j = int(w), int(u)
        four = 0.25 * ((img[:, i, j] + img[:, i, j + 1]) + (img[:, i + 1, j] + img[:, i + 1, j + 1]))
        assert (out["colors"][k] == np.floor(255.0 * four + 0.5).astype(np.uint8)).all()
        assert abs(int(out["colors"][k][2]) - 128) <= 1                   # two dark and two bright texels


def test_square_behind_is_hidden_and_copies_the_nearest_front_vertices():
    s = C.analytic_scenes()["occluded"]
    out = run(s)
    v = s["vertices"]
    for (u, w), (fu, fw) in zip(C.corners(C.BACK), C.corners(C.FRONT)):
        k, near = C.find(v, u, w, 3.0), C.find(v, fu, fw, 2.0)
        assert out["seen"][near] == 1 and out["seen"][k] == 0
        assert out["source"][k] == near
        assert (out["colors"][k] == C.texel(fw, fu)).all()
    assert out["seen"].sum() == 4
    assert 0.0 < out["seen_area"] < out["total_area"]


def test_exact_distance_tie_goes_to_the_lower_index():
    s = C.analytic_scenes()["tie"]
    out = run(s)
    v = s["vertices"]
    fc = C.corners(C.FRONT)
    pairs = [(fc[0], fc[1]), (fc[1], fc[2]), (fc[2], fc[3]), (fc[3], fc[0])]          # top, right, bottom, left
    for (u, w), (p, q) in zip(C.DIAMOND, pairs):
        k = C.find(v, u, w, 3.0)
        a, b = C.find(v, *p, 2.0), C.find(v, *q, 2.0)
        da, db = [((v[k].astype(np.float64) - v[x]) ** 2).sum() for x in (a, b)]
        assert da == db and out["seen"][k] == 0
        assert out["source"][k] == min(a, b)


@pytest.mark.parametrize("name,fade", [("occluded", 0.0), ("fade_mid", 4.0), ("fade_full", 1.0)])
def test_fade_follows_the_formula(name, fade):
    s = C.analytic_scenes()[name]
    out = run(s)
    v = s["vertices"]
    dist = np.sqrt(0.5 ** 2 + 0.75 ** 2 + 2.0 ** 2)                       # back corner to its front corner, mesh units
    t = min(dist / fade, 1.0) if fade > 0 else 0.0
    assert (t == 0.0, 0.0 < t < 1.0, t == 1.0) == (name == "occluded", name == "fade_mid", name == "fade_full")
    for (u, w), (fu, fw) in zip(C.corners(C.BACK), C.corners(C.FRONT)):
        k = C.find(v, u, w, 3.0)
        want = np.floor((1.0 - t) * C.texel(fw, fu).astype(np.float64) + t * 255.0 * np.float32(C.BASE).astype(np.float64) + 0.5)
        assert (out["colors"][k] == want.astype(np.uint8)).all()


def test_depth_tol_flips_seen_at_the_gap_between_the_squares():
    scenes = C.analytic_scenes()
    below, above = run(scenes["tol_below"]), run(scenes["tol_above"])
    assert below["seen"].sum() == 4 and above["seen"].sum() == 8
    assert (above["source"] == np.arange(8)).all()


@pytest.mark.parametrize("k", range(4))
def test_one_mask_texel_in_the_footprint_hides_the_vertex(k):
    s = C.analytic_scenes()["mask%d" % k]
    out = run(s)
    hidden = C.find(s["vertices"], 4, 3, 2.0)
    assert out["seen"][hidden] == 0 and out["seen"].sum() == 3


def test_outside_the_frame_behind_the_camera_and_facing_away():
    scenes = C.analytic_scenes()
    s = scenes["u_outside"]
    out = run(s)
    assert [int(out["seen"][C.find(s["vertices"], u, w, 2.0)]) for u, w in C.corners((10, 3, 16, 9))] == [1, 0, 0, 1]
    s = scenes["w_outside"]
    out = run(s)
    assert [int(out["seen"][C.find(s["vertices"], u, w, 2.0)]) for u, w in C.corners((4, -1, 12, 5))] == [0, 0, 1, 1]
    out = run(scenes["behind"])
    assert not out["seen"].any() and (out["source"] == -1).all()
    assert (out["Z"] == -2.0).all() and ((out["u"] >= 0) & (out["u"] <= C.W - 1)).all()
    assert (out["colors"] == np.floor(255.0 * np.float32(C.BASE).astype(np.float64) + 0.5).astype(np.uint8)).all()
    assert not run(scenes["flipped"])["seen"].any()
    assert not run(scenes["grazing_below"])["seen"].any()
    assert run(scenes["grazing_above"])["seen"].all()


def test_projection_round_trip_of_an_unprojected_depth_map():
    """Pixels unprojected with the oracle's unproj_depth (oracle/frontend_ref.py) and normalised like the seen surface come
    back at their own pixel indices."""
    import torch
    from oracle import frontend_ref
    h = w = 24
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    depth = (1.5 + 0.3 * np.sin(i / 5.0) * np.cos(j / 7.0)).astype(np.float32)
    intr = np.array([[30.0, 0, 11.5], [0, 28.0, 12.25], [0, 0, 1]], np.float32)
    pts = frontend_ref.unproj_depth(torch.from_numpy(depth)[None, None], torch.from_numpy(intr)[None])[0].numpy()
    mean = pts.mean(axis=0).astype(np.float32)
    scale = np.float32(np.linalg.norm(pts - mean, axis=1).max())
    verts = ((pts - mean) / scale).astype(np.float32)
    out = E.mesh_vertex_colors_host(verts, np.zeros((0, 3), np.int64), np.zeros_like(verts), C.photo(h, w), np.ones((h, w), np.float32),
                                    intr, mean, scale, depth_tol=0.1)
    assert np.abs(out["u"] - j.reshape(-1)).max() < 1e-4 and np.abs(out["w"] - i.reshape(-1)).max() < 1e-4
    assert np.abs(out["Z"] - depth.reshape(-1)).max() < 1e-4


def test_fma32_and_the_nearest_point_rule_agree_with_the_chamfer_oracle():
    from oracle import chamfer_ref
    rng = np.random.default_rng(5)
    q = rng.standard_normal((300, 3)).astype(np.float32)
    c = np.concatenate([rng.standard_normal((200, 3)), q[:50] + 1.0]).astype(np.float32)
    c = np.concatenate([c, c[:40]])                                       # exact duplicates: ties
    dist, idx = E.nearest_point_host(q, c)
    d1, _, i1, _ = chamfer_ref.chamfer_forward(q[None], c[None])
    assert (idx == i1[0]).all() and (dist.view(np.uint32) == d1[0].view(np.uint32)).all()


def test_device_entry_points_reject_host_inputs():
    import torch
    mesh = E.SimpleMesh(C.square(*C.FRONT, 2.0))
    z = torch.zeros(3)
    with pytest.raises(ValueError, match="no CPU path"):
        E.mesh_vertex_colors(mesh, z, z, z, z, z, 0.1)
    with pytest.raises(ValueError, match="vertex colours"):
        mesh.vertex_colors
    with pytest.raises(ValueError):
        mesh.seen_area_fraction
    assert "seen_area_fraction" not in E.mesh_report(mesh)


def test_argument_checks_of_the_library_without_a_gpu():
    import ctypes
    from zeroshape_amd import _lib, build
    build.build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    base = (ctypes.c_float * 3)(0.5, 0.5, 0.8)

    def seen(V=4, F=2, H=8, W=8, ss=2, tol=0.1, cos=0.1, ptr=p):
        return lib.zs_mesh_colors_seen(ptr, ptr, ptr, V, F, ptr, ptr, H, W, ptr, ptr, ptr, ss, tol, cos, ptr, ptr, ptr, ptr, ptr, ptr, None)

    def fails(call, what):
        assert call == 0 and what.encode() in lib.zs_last_error(), lib.zs_last_error()

    fails(seen(V=-1), "negative size")
    fails(seen(V=2 ** 29 + 1), "too large")
    fails(seen(F=2 ** 29 + 1), "too large")
    fails(seen(H=0), "bad image size")
    fails(seen(ss=0), "bad image size")
    fails(seen(H=16384, ss=2), "bad image size")
    fails(seen(tol=-1.0), "bad thresholds")
    fails(seen(ptr=None), "null pointer")
    assert seen(V=0, ptr=None) == 1                                       # an empty mesh: nothing to launch
    assert lib.zs_mesh_colors_workspace_bytes(0, 0, 8, 8, 2) == 0 and lib.zs_mesh_colors_workspace_bytes(2 ** 29 + 1, 1, 8, 8, 2) == 0
    assert lib.zs_mesh_colors_workspace_bytes(4, 2, 8, 8, 2) >= 4 * 4 + 4 * 24 + 16 * 16 * 8
    fails(lib.zs_mesh_colors_compact(p, p, 4, 5, p, p, p, p, p, None), "bad count")
    fails(lib.zs_mesh_colors_compact(None, p, 4, 2, p, p, p, p, p, None), "null pointer")
    assert lib.zs_mesh_colors_compact(None, None, 0, 0, None, None, None, None, None, None) == 1
    fails(lib.zs_mesh_colors_fill(p, p, p, p, 4, 5, 0.0, base, p, p, None), "bad count")
    fails(lib.zs_mesh_colors_fill(p, p, p, p, 4, 2, -1.0, base, p, p, None), "fade")
    fails(lib.zs_mesh_colors_fill(None, p, p, p, 4, 2, 0.0, base, p, p, None), "null pointer")
    assert lib.zs_mesh_colors_fill(None, None, None, None, 4, 4, 0.0, base, None, None, None) == 1
    xf = (ctypes.c_float * 8)(1, 1, 1, 0, 0, 0, 1, 1)
    fails(lib.zs_render_frames_colored(p, 1, xf, p, 1, 8, 8, 1.0, 0.05, None, p, None, None, p, None), "null pointer")
    fails(lib.zs_render_frames_colored(p, -1, xf, p, 1, 8, 8, 1.0, 0.05, p, p, None, None, p, None), "bad size")
    assert lib.zs_render_frames_colored(None, 0, xf, None, 0, 8, 8, 1.0, 0.05, None, None, None, None, None, None) == 1
