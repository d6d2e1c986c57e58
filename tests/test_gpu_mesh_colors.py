"""GPU: vertex colours from the input photo (csrc/mesh_colors.hip) against their definition eval_3D.mesh_vertex_colors_host -
colours, seen flags and sources EQUAL (fp64 basic operations, contraction off: no tolerance), the seen area fraction within
1e-12 relative of the host sum - on the analytic scenes of tests/mesh_colors_cases.py, on two marching-cubes spheres, on
degenerate inputs and on a seen-surface sheet; determinism; the per-corner albedo of the turntable renderer against
zs_render_frames and a float64 restatement; dump_meshes, mesh_report and demo.py."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_colors_cases as C
from tests.test_gpu_render import octahedron, path_frames
from zeroshape_amd.utils import camera
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """The module's cached meshes are released, and what its tests left is collected, when it ends."""
    yield
    import gc
    spheres.cache_clear()
    spheres_want.cache_clear()
    gc.collect()


def cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def gpu_mesh(vertices, faces, normals):
    """A GPU SimpleMesh that carries the given weld (the scenes prescribe their normals)."""
    v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    mesh = E.SimpleMesh(cuda(v[f].reshape(-1, 3, 3), np.float32))
    mesh._device_weld = (cuda(v, np.float32), cuda(f, np.int32), cuda(normals, np.float32))
    return mesh


def run_gpu(mesh, s):
    kw = {k: s[k] for k in ("min_cos", "supersample", "fade", "base_rgb") if k in s}
    return E.mesh_vertex_colors(mesh, cuda(s["image"]), cuda(s["mask"]), cuda(s["intr"]), cuda(s["mean"]),
                                cuda(np.asarray(s["scale"], np.float32).reshape(1)), s["depth_tol"], **kw)


def assert_equals_checker(mesh, want, what=""):
    for t, dtype, shape in ((mesh.device_vertex_colors, torch.uint8, (len(want["seen"]), 3)),
                            (mesh.device_vertex_seen, torch.uint8, (len(want["seen"]),)),
                            (mesh.device_color_source, torch.int32, (len(want["seen"]),)),
                            (mesh.device_seen_area, torch.float64, (2,))):
        assert t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape
    seen, source, colors = mesh.vertex_seen, mesh.device_color_source.cpu().numpy(), mesh.vertex_colors
    area = mesh.device_seen_area.cpu().numpy()
    print("%s: V %d, seen %d, |seen differs| %d, |source differs| %d, |colour differs| %d, areas %r against %r"
          % (what, len(seen), int(seen.sum()), int((seen != want["seen"].astype(bool)).sum()), int((source != want["source"]).sum()),
             int((colors != want["colors"]).any(axis=1).sum()), area.tolist(), (want["seen_area"], want["total_area"])))
    assert np.array_equal(seen, want["seen"].astype(bool))
    assert np.array_equal(source, want["source"])
    assert colors.dtype == np.uint8 and np.array_equal(colors, want["colors"])
    for got, ref in zip(area, (want["seen_area"], want["total_area"])):
        assert abs(got - ref) <= 1e-12 * abs(ref)
    frac = want["seen_area"] / want["total_area"] if want["total_area"] > 0 else 0.0
    assert abs(mesh.seen_area_fraction - frac) <= 1e-12 * frac


# ---- the analytic scenes of the CPU file ----

SCENES = C.analytic_scenes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_analytic_scene_equals_the_checker(name):
    s = SCENES[name]
    mesh = run_gpu(gpu_mesh(s["vertices"], s["faces"], s["normals"]), s)
    assert_equals_checker(mesh, E.mesh_vertex_colors_host(**s), name)


# ---- two marching-cubes spheres ----

@functools.lru_cache(maxsize=None)
def spheres(vox):
    """(soup on the GPU, the numpy-welded host mesh) of the two spheres at this resolution - extracted once."""
    tris, _ = E.extract_surface(cuda(C.two_spheres_volume(vox)), 0.5, *C.SPH_RANGE)
    return tris, E.SimpleMesh(tris.cpu().numpy())


@functools.lru_cache(maxsize=None)
def spheres_want(vox, ss, depth_tol=None):
    _, ref = spheres(vox)
    img, mask = C.sphere_photo_and_mask()
    return E.mesh_vertex_colors_host(ref.vertices, ref.faces, ref.vertex_normals, img, mask, C.SPH_K, C.SPH_MEAN, C.SPH_SCALE,
                                     C.sphere_depth_tol(vox) if depth_tol is None else depth_tol, supersample=ss)


def spheres_gpu(vox, ss, tris=None):
    img, mask = C.sphere_photo_and_mask()
    mesh = E.SimpleMesh(spheres(vox)[0] if tris is None else tris)
    return E.mesh_vertex_colors(mesh, cuda(img), cuda(mask), cuda(C.SPH_K), cuda(C.SPH_MEAN), cuda(np.float32([C.SPH_SCALE])),
                                C.sphere_depth_tol(vox), supersample=ss)


# vox 16 (the per-vertex kernels' 256-thread blocks: V, F, seen and hidden all above 256) at every supersampling; vox 48 once,
# where V, F, seen and hidden all exceed one 2048-element tile of the scan, which no sphere in a 17^3 grid can
@pytest.mark.parametrize("vox,ss,block", [(16, 1, 256), (16, 2, 256), (16, 3, 256), (48, 2, 2048)])
def test_two_spheres_equal_the_checker(vox, ss, block):
    _, ref = spheres(vox)
    want = spheres_want(vox, ss)
    V_, n_seen = len(ref.vertices), int(want["seen"].sum())
    assert ref.components.n_components == 2
    assert min(V_, len(ref.faces), n_seen, V_ - n_seen) > block
    assert n_seen >= 0.1 * V_ and V_ - n_seen >= 0.1 * V_
    assert int(spheres_want(vox, ss, depth_tol=1e30)["seen"].sum()) > n_seen             # the z-buffer decides some vertices
    mesh = spheres_gpu(vox, ss)
    assert np.array_equal(mesh.vertices, ref.vertices) and np.array_equal(mesh.faces, ref.faces)      # the GPU weld is the host's
    assert_equals_checker(mesh, want, "spheres vox %d ss %d" % (vox, ss))


def test_two_calls_give_the_same_bits_and_face_order_does_not_change_seen():
    a, b = spheres_gpu(16, 2), spheres_gpu(16, 2)
    for name in ("device_vertex_colors", "device_vertex_seen", "device_color_source", "device_seen_area"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    _, ref = spheres(16)
    perm = np.random.default_rng(3).permutation(len(ref.faces))
    shuffled = gpu_mesh(ref.vertices, ref.faces[perm], ref.vertex_normals)
    img, mask = C.sphere_photo_and_mask()
    E.mesh_vertex_colors(shuffled, cuda(img), cuda(mask), cuda(C.SPH_K), cuda(C.SPH_MEAN), cuda(np.float32([C.SPH_SCALE])),
                         C.sphere_depth_tol(16), supersample=2)
    assert np.array_equal(shuffled.vertex_seen, a.vertex_seen)
    assert np.array_equal(shuffled.vertex_colors, a.vertex_colors)


# ---- degenerate inputs ----

def test_nothing_seen_gives_the_base_colour_everywhere():
    s = dict(SCENES["occluded"], mask=np.zeros((C.H, C.W), np.float32), base_rgb=(0.25, 0.5, 1.0))
    mesh = run_gpu(gpu_mesh(s["vertices"], s["faces"], s["normals"]), s)
    assert not mesh.vertex_seen.any() and (mesh.device_color_source.cpu().numpy() == -1).all()
    assert (mesh.vertex_colors == np.array([64, 128, 255], np.uint8)).all()        # floor(255 base + 0.5)
    assert mesh.seen_area_fraction == 0.0
    assert_equals_checker(mesh, E.mesh_vertex_colors_host(**s), "nothing seen")


def test_empty_mesh_gives_empty_outputs():
    mesh = E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda"))
    s = SCENES["front"]
    from zeroshape_amd import _lib
    calls = _lib.CALLS[0]
    run_gpu(mesh, s)
    assert _lib.CALLS[0] == calls                                  # no launch
    assert mesh.vertex_colors.shape == (0, 3) and mesh.vertex_colors.dtype == np.uint8 and mesh.vertex_seen.shape == (0,)
    assert tuple(mesh.device_color_source.shape) == (0,) and mesh.seen_area_fraction == 0.0


def test_face_larger_than_the_frame_and_face_across_the_camera_plane():
    front = C.square(*C.FRONT, 2.0)
    huge = C.square(-400, -300, 400, 300, 1.5)                     # covers every z-buffer texel in front of the square
    s = C.scene(np.concatenate([front, huge]))
    mesh = run_gpu(gpu_mesh(s["vertices"], s["faces"], s["normals"]), s)
    want = E.mesh_vertex_colors_host(**s)
    assert not want["seen"].any()                                  # the square is behind it, its own corners outside the frame
    assert_equals_checker(mesh, want, "huge face")
    across = np.array([[C.mesh_point(8, 6, -1.0), C.mesh_point(2, 2, 1.0), C.mesh_point(14, 2, 1.0)]], np.float32)
    s = C.scene(np.concatenate([front, across]), depth_tol=0.01)
    want = E.mesh_vertex_colors_host(**s)
    v = s["vertices"]
    assert want["seen"][[C.find(v, u, w, 2.0) for u, w in C.corners(C.FRONT)]].all()      # skipped whole: it occludes nothing
    assert want["seen"][C.find(v, 8, 6, -1.0)] == 0
    assert_equals_checker(run_gpu(gpu_mesh(s["vertices"], s["faces"], s["normals"]), s), want, "face across Z = 0")


# ---- the seen-surface sheet: every vertex is seen and has its own pixel's colour ----

def test_seen_surface_sheet_is_all_seen_with_its_own_texels():
    """The sheet is made of the pixels one step inside the frame: a vertex unprojected from a pixel of the frame's outermost
    ring projects back to within 1e-6 of the frame's edge, on either side of it, and the rule 0 <= u <= W - 1 is exact."""
    n = 64
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    depth = cuda((1.6 + 0.25 * np.sin(i / 11.0) * np.cos(j / 13.0))[None, None], np.float32)
    intr = cuda(np.array([[[90.0, 0, 31.5], [0, 90.0, 31.5], [0, 0, 1]]], np.float32))
    pts = camera.unproj_depth(edict(H=n, W=n), depth, intr)                               # [1, n*n, 3], camera frame
    inner = torch.zeros(1, 1, n, n, device="cuda")
    inner[:, :, 1:-1, 1:-1] = 1.0
    mask = torch.ones(1, 1, n, n, device="cuda")
    mean, scale = camera.valid_norm_fac(pts, inner)
    (verts, pixels, faces), = V.seen_surface_mesh(pts.view(1, n, n, 3), inner, connect_thres=0.2)
    assert len(verts) == (n - 2) ** 2 and len(faces) == 2 * (n - 3) ** 2
    verts = ((verts - mean[0].cpu().numpy()) / scale.cpu().numpy()).astype(np.float32)     # its own normalisation
    assert len(np.unique(verts, axis=0)) == (n - 2) ** 2
    soup = verts[faces[:, [0, 2, 1]] - 1]                          # (create_seen_surface winds away from the camera)
    mesh = E.SimpleMesh(cuda(soup, np.float32))
    image = C.photo(n, n)
    E.mesh_vertex_colors(mesh, cuda(image), mask[0, 0], intr[0], mean[0], scale, depth_tol=0.05)
    assert mesh.vertex_seen.all() and mesh.seen_area_fraction == 1.0
    assert np.array_equal(mesh.device_color_source.cpu().numpy(), np.arange((n - 2) ** 2))
    where = {tuple(v): p for v, p in zip(verts.tolist(), pixels.tolist())}
    pix = np.array([where[tuple(v)] for v in mesh.vertices.tolist()])
    want = np.stack([C.texel(p // n, p % n) for p in pix])
    assert np.array_equal(mesh.vertex_colors, want)
    ref = E.mesh_vertex_colors_host(mesh.vertices, mesh.faces, mesh.vertex_normals, image, np.ones((n, n), np.float32),
                                    intr[0].cpu().numpy(), mean[0].cpu().numpy(), scale.cpu().numpy(), 0.05)
    assert_equals_checker(mesh, ref, "seen-surface sheet")


# ---- the renderer's per-corner albedo ----

def oracle_render_colored(tris, corner_rgb, xform, cams, H, W):
    """tests/test_gpu_render.py's float64 rasteriser with the albedo interpolated perspective-correctly from the corner colours
    -> the unrounded colour [F,H,W,3] (1 = background), tri [F,H,W]."""
    tris, xform, cams = np.asarray(tris, np.float64).reshape(-1, 3, 3), np.asarray(xform, np.float64), np.asarray(cams, np.float64)
    cols = np.asarray(corner_rgb, np.float64).reshape(-1, 3, 3) / 255.0
    tn = math.tan(float(np.float32(V.YFOV)) * 0.5)
    ta = tn * (W / H)
    znear, half_w, half_h = float(np.float32(V.ZNEAR)), W * 0.5, H * 0.5
    world = (tris * xform[0:3] - xform[3:6]) * xform[6]
    if xform[7] < 0:
        world, cols = world[:, [0, 2, 1]], cols[:, [0, 2, 1]]
    F = len(cams)
    depth, tri, colour = np.full((F, H, W), np.inf), np.full((F, H, W), -1, np.int64), np.ones((F, H, W, 3))
    for f in range(F):
        c = cams[f]
        w = world - c[0:3]
        vc = np.stack([c[3 + a] * w[..., 0] + c[6 + a] * w[..., 1] + c[9 + a] * w[..., 2] for a in range(3)], -1)
        z = -vc[..., 2]
        x, y = (vc[..., 0] / (z * ta) + 1.0) * half_w, (1.0 - vc[..., 1] / (z * tn)) * half_h
        area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
        for t in range(len(tris)):
            if not (z[t] > znear).all() or not abs(area[t]) > 0:
                continue
            X, Y, Z, A = x[t], y[t], z[t], area[t]
            py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
            w0 = ((X[2] - X[1]) * (py - Y[1]) - (Y[2] - Y[1]) * (px - X[1])) / A
            w1 = ((X[0] - X[2]) * (py - Y[2]) - (Y[0] - Y[2]) * (px - X[2])) / A
            w2 = ((X[1] - X[0]) * (py - Y[0]) - (Y[1] - Y[0]) * (px - X[0])) / A
            q = np.stack([w0 / Z[0], w1 / Z[1], w2 / Z[2]], -1)
            d = 1.0 / q.sum(-1)
            win = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (d < depth[f])
            hit = d[..., None] * (q @ vc[t])
            nrm = np.cross(vc[t, 1] - vc[t, 0], vc[t, 2] - vc[t, 0])
            nrm = nrm / np.linalg.norm(nrm)
            shade = 0.3 + 0.7 * np.abs((-hit / np.linalg.norm(hit, axis=-1, keepdims=True)) @ nrm)
            albedo = (q @ cols[t]) / q.sum(-1, keepdims=True)
            depth[f][win], tri[f][win] = d[win], t
            colour[f][win] = (albedo * shade[..., None])[win]
    return colour, tri


def render_both(tris, corner, xform, cams, H, W):
    Fr = cams.shape[0]
    out = []
    for colors in (None, corner):
        rgb = torch.empty(Fr, H, W, 3, dtype=torch.uint8, device="cuda")
        depth = torch.empty(Fr, H, W, dtype=torch.float32, device="cuda")
        tri = torch.empty(Fr, H, W, dtype=torch.int32, device="cuda")
        V.render_into(tris, xform, cams, H, W, rgb, depth, tri, corner_colors=colors)
        out.append((rgb, depth, tri))
    return out


@pytest.mark.parametrize("winding", [1.0, -1.0])
def test_colored_frames_against_the_plain_renderer_and_a_float64_restatement(winding, monkeypatch):
    H, W = 40, 56
    soup = octahedron()
    tris = cuda(soup)
    cams_host = V.camera_rows(*path_frames())
    cams = cuda(cams_host)
    assert cams.shape[0] == 8
    xform = np.array([1, -1, -1, 0.02, -0.01, 0.03, 0.9, winding], np.float32)
    # one colour on every corner: the plain renderer with that colour as its base
    monkeypatch.setattr(V, "BASE_RGB", (0.2, 0.4, 0.6))
    flat = torch.tensor([51, 102, 153], dtype=torch.uint8, device="cuda").expand(len(soup), 3, 3).contiguous()
    (rgb0, depth0, tri0), (rgb1, depth1, tri1) = render_both(tris, flat, xform, cams, H, W)
    assert torch.equal(tri0, tri1) and torch.equal(depth0.view(torch.int32), depth1.view(torch.int32))
    assert (tri0 >= 0).sum() > 500
    print("constant corners: %d of %d bytes differ" % (int((rgb0 != rgb1).sum()), rgb0.numel()))
    assert torch.equal(rgb0, rgb1)
    # random corners
    corner = np.random.default_rng(11).integers(0, 256, (len(soup), 3, 3)).astype(np.uint8)
    (_, depth0, tri0), (rgb1, depth1, tri1) = render_both(tris, cuda(corner), xform, cams, H, W)
    assert torch.equal(tri0, tri1) and torch.equal(depth0.view(torch.int32), depth1.view(torch.int32))
    colour, want_tri = oracle_render_colored(soup, corner, xform, cams_host, H, W)
    assert np.array_equal(tri1.cpu().numpy(), want_tri)
    err = np.abs(rgb1.cpu().numpy().astype(np.float64) - 255.0 * colour)
    print("random corners: max colour difference %.3f grey levels" % err.max())
    assert err.max() <= 1.0 + 1e-9
    assert (rgb1.cpu().numpy()[want_tri < 0] == 255).all()


# ---- dumps ----

def test_dump_meshes_with_colours_and_mesh_report_keys(tmp_path):
    opt = edict(output_path=str(tmp_path))
    plain, colored = E.SimpleMesh(spheres(16)[0]), spheres_gpu(16, 2)
    V.dump_meshes(opt, ["plain"], "mesh", [plain])
    V.dump_meshes(opt, ["before"], "mesh", [colored], colors=False)
    assert open(tmp_path / "dump" / "plain_mesh.obj", "rb").read() == open(tmp_path / "dump" / "before_mesh.obj", "rb").read()
    v, f = colored.vertices, colored.faces + 1                     # the text dump_meshes wrote before it knew of colours
    old = "".join(["# zeroshape_amd mesh: %d vertices, %d faces\n" % (len(v), len(f))] + ["v %.6f %.6f %.6f\n" % tuple(r) for r in v.tolist()]
                  + ["f %d %d %d\n" % tuple(r) for r in f.tolist()])
    assert open(tmp_path / "dump" / "plain_mesh.obj").read() == old
    for normals in (False, True):
        V.dump_meshes(opt, ["c%d" % normals], "mesh", [colored], colors=True, normals=normals)
        rows = open(tmp_path / "dump" / ("c%d_mesh.obj" % normals)).read().split("\n")
        vs = [r.split() for r in rows if r.startswith("v ")]
        assert len(vs) == len(v) and all(len(r) == 7 for r in vs)
        got = np.array([[float(x) for x in r[1:]] for r in vs])
        assert np.abs(got[:, 3:] - colored.vertex_colors / 255.0).max() < 1.0 / 255.0 / 2.0
        assert np.abs(got[:, :3] - v).max() <= 5e-7
        assert sum(r.startswith("vn ") for r in rows) == (len(v) if normals else 0)
        assert sum(r.startswith("f ") for r in rows) == len(f)
    keys = set(E.mesh_report(plain))
    assert keys == {"vertices", "faces", "components", "area", "volume", "euler_number", "is_watertight", "component_table"}
    report = E.mesh_report(colored)
    assert set(report) == keys | {"seen_area_fraction"}
    want = spheres_want(16, 2)
    assert abs(report["seen_area_fraction"] - want["seen_area"] / want["total_area"]) < 1e-12
    with pytest.raises(ValueError, match="vertex colours"):
        V.dump_meshes(opt, ["x"], "mesh", [plain], colors=True)


def test_colored_turntable_of_a_mesh(tmp_path):
    colored = spheres_gpu(16, 2)
    frames = V.visualize_mesh(colored, str(tmp_path / "viz"), resolution=(48, 40), write_frames=False, n_frames=6,
                              pose_normalize=True, colors=True)
    plain = V.visualize_mesh(colored, str(tmp_path / "plain"), resolution=(48, 40), write_frames=False, n_frames=6,
                             pose_normalize=True)
    assert frames.shape == plain.shape == (6, 40, 48, 3)
    assert np.array_equal((frames == 255).all(-1), (plain == 255).all(-1)) and (frames != plain).any()
    assert (tmp_path / "viz.gif").exists()


def off_the_base_line(rgb, tol=24):
    """Pixels [...,3] that are neither white nor a shade of util_vis.BASE_RGB (r = g, b = 1.6 r), with room for a GIF palette."""
    r, g, b = [rgb[..., k].astype(np.float64) for k in range(3)]
    white = (rgb > 255 - tol).all(-1)
    line = (np.abs(r - g) <= tol) & (np.abs(b - V.BASE_RGB[2] / V.BASE_RGB[0] * r) <= tol)
    return ~white & ~line


def test_demo_script_writes_a_coloured_mesh_and_turntable(tmp_path, encoder_sd, seeded_sd):
    import json
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
    # the seeded decoder's logits on this image lie in [-0.48, -0.08]: its 0.5 level set is empty and the demo would write a
    # mesh without vertices.  The last bias is moved so that the level lies inside that range, where the surface is a sheet
    # the input camera looks at (shifts of 0.12 to 0.32 are; from 0.34 on a part of the sheet hangs right in front of the
    # camera, which sits inside the evaluation cube with these random intrinsics, and correctly hides everything else).
    full["impl_network.impl_mlp.layers.8.bias"] = full["impl_network.impl_mlp.layers.8.bias"] + 0.26
    torch.save(dict(epoch=0, iter=0, best_val=1.0, best_ep=0, graph=full), tmp_path / "shape.ckpt")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0", ZS_SYNTHETIC_ITEMS="4", ZS_SYNTHETIC_STANDIN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--yaml=options/shape.yaml", "--task=shape",
                        "--datadir=%s/data" % tmp_path, "--eval.vox_res=32", "--ckpt=%s/shape.ckpt" % tmp_path,
                        "--output_root=%s" % tmp_path, "--eval.vertex_colors=true", "--eval.mesh_report=true", "--viz"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    preds = tmp_path / "data" / "preds"
    rows = open(preds / "blob_mesh.obj").read().split("\n")
    vs = [row.split() for row in rows if row.startswith("v ")]
    assert len(vs) > 0 and all(len(row) == 7 for row in vs)
    assert all(0.0 <= float(x) <= 1.0 for row in vs for x in row[4:])
    report = json.load(open(preds / "blob_mesh_report.json"))
    assert 0.0 <= report["seen_area_fraction"] <= 1.0
    gif = Image.open(preds / "blob_mesh_viz.gif")
    assert gif.n_frames == 180 and gif.size == (200, 200)
    first = np.asarray(gif.convert("RGB"))
    odd = off_the_base_line(first)
    print("first frame: %d pixels off the base colour's shading line, seen area fraction %.3f" % (int(odd.sum()), report["seen_area_fraction"]))
    assert odd.sum() > 0
