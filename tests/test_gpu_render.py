"""GPU: the mesh turntable renderer (csrc/render.hip through zeroshape_amd/utils/util_vis.py) against a float64 numpy
rasteriser written here that implements the same rules - projection, inclusive coverage at pixel centres, perspective-correct
depth, nearest wins / lower index at equal depth, flat shading - and loops over triangles; then the GIF dumps and demo.py --viz.

pyrender's pixels are not a reference here (no GL, no pyrender): parity with them is unpinned."""
import math
import os

import numpy as np
import pytest
import torch

from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_TOL = 1e-4        # ~6x the fp32-vs-fp64 difference of this rasteriser on the octahedron / sphere cases (2.6e-6 / 1.5e-5)
FRAMES = list(range(0, 180, 23))


# ---- the oracle ----

def oracle_render(tris, xform, cams, H, W, base=V.BASE_RGB):
    """tris [n,3,3], xform [8], cams [F,12] (the fp32 values the kernel gets, computed with in float64) ->
    rgb uint8 [F,H,W,3] and the unrounded colour [F,H,W,3], depth [F,H,W] (inf = nothing), tri [F,H,W] (-1 = nothing)."""
    tris, xform, cams = np.asarray(tris, np.float64).reshape(-1, 3, 3), np.asarray(xform, np.float64), np.asarray(cams, np.float64)
    tn = math.tan(float(np.float32(V.YFOV)) * 0.5)
    ta = tn * (W / H)
    znear, half_w, half_h = float(np.float32(V.ZNEAR)), W * 0.5, H * 0.5
    world = (tris * xform[0:3] - xform[3:6]) * xform[6]
    if xform[7] < 0:
        world = world[:, [0, 2, 1]]
    F = len(cams)
    depth = np.full((F, H, W), np.inf)
    tri = np.full((F, H, W), -1, np.int64)
    colour = np.ones((F, H, W, 3))
    base = np.asarray([float(np.float32(b)) for b in base])
    for f in range(F):
        c = cams[f]
        w = world - c[0:3]
        vc = np.stack([c[3 + a] * w[..., 0] + c[6 + a] * w[..., 1] + c[9 + a] * w[..., 2] for a in range(3)], -1)   # R^T (p - pos)
        z = -vc[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            x = (vc[..., 0] / (z * ta) + 1.0) * half_w
            y = (1.0 - vc[..., 1] / (z * tn)) * half_h
            area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
        for t in range(len(tris)):
            if not (z[t] > znear).all() or not abs(area[t]) > 0:
                continue
            X, Y, Z, A = x[t], y[t], z[t], area[t]
            j0, j1 = int(max(math.ceil(X.min() - 0.5), 0)), int(min(math.floor(X.max() - 0.5), W - 1))
            i0, i1 = int(max(math.ceil(Y.min() - 0.5), 0)), int(min(math.floor(Y.max() - 0.5), H - 1))
            if j0 > j1 or i0 > i1:
                continue
            py, px = np.meshgrid(np.arange(i0, i1 + 1) + 0.5, np.arange(j0, j1 + 1) + 0.5, indexing="ij")
            w0 = ((X[2] - X[1]) * (py - Y[1]) - (Y[2] - Y[1]) * (px - X[1])) / A
            w1 = ((X[0] - X[2]) * (py - Y[2]) - (Y[0] - Y[2]) * (px - X[2])) / A
            w2 = ((X[1] - X[0]) * (py - Y[0]) - (Y[1] - Y[0]) * (px - X[0])) / A
            d = 1.0 / (w0 / Z[0] + w1 / Z[1] + w2 / Z[2])
            sub_d, sub_t, sub_c = depth[f, i0:i1 + 1, j0:j1 + 1], tri[f, i0:i1 + 1, j0:j1 + 1], colour[f, i0:i1 + 1, j0:j1 + 1]
            win = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (d < sub_d)      # triangles come in index order: a tie keeps the lower
            if not win.any():
                continue
            # flat shade at the hit: the perspective-correct point on the triangle, the light at the camera (the origin)
            hit = d[..., None] * (w0[..., None] * vc[t, 0] / Z[0] + w1[..., None] * vc[t, 1] / Z[1] + w2[..., None] * vc[t, 2] / Z[2])
            n = np.cross(vc[t, 1] - vc[t, 0], vc[t, 2] - vc[t, 0])
            n = n / np.linalg.norm(n)
            l = -hit / np.linalg.norm(hit, axis=-1, keepdims=True)
            shade = 0.3 + 0.7 * np.abs(l @ n)
            sub_d[win], sub_t[win] = d[win], t
            sub_c[win] = (base * shade[..., None])[win]
    rgb = np.floor(255.0 * colour + 0.5).clip(0, 255).astype(np.uint8)
    return rgb, colour, depth, tri


def gpu_render(tris, positions, rotations, W, H, pose_normalize=False):
    t = torch.from_numpy(np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)).cuda()
    rgb, depth, tri = V.render_mesh_frames(t, positions, rotations, (W, H), return_depth=True, return_tri=True,
                                           pose_normalize=pose_normalize)
    assert rgb.shape == (len(positions), H, W, 3) and rgb.dtype == torch.uint8
    assert depth.shape == tri.shape == (len(positions), H, W) and depth.dtype == torch.float32 and tri.dtype == torch.int32
    return rgb.cpu().numpy(), depth.cpu().numpy(), tri.cpu().numpy()


def numpy_stats(tris):
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    flat = tris.reshape(-1, 3)
    vol = np.einsum("ni,ni->", tris[:, 0], np.cross(tris[:, 1], tris[:, 2])) / 6.0
    return np.concatenate([flat.min(0), flat.max(0), [vol]])


def check_against_oracle(got, want, what):
    """`tri` equal on every pixel; depth within DEPTH_TOL on every covered pixel (no exclusions are taken); colours within one
    grey level of the formula evaluated in float64 at the oracle's hit."""
    rgb, depth, tri = got
    _, colour, want_depth, want_tri = want
    covered = want_tri >= 0
    mism = int((tri != want_tri).sum())
    err = np.abs(depth[covered].astype(np.float64) - want_depth[covered])
    cerr = np.abs(rgb.astype(np.float64) - 255.0 * colour)
    print("%s: %d covered pixels, %d index mismatches, max depth difference %.3g, max colour difference %.3f grey levels"
          % (what, int(covered.sum()), mism, err.max() if err.size else 0.0, cerr.max()))
    assert covered.sum() > 0
    assert mism == 0
    assert np.isinf(depth[~covered]).all() and (depth[~covered] > 0).all()
    assert err.max() <= DEPTH_TOL
    assert (rgb[~covered] == 255).all()
    assert cerr.max() <= 1.0 + 1e-9


def front_camera(z=1.5):
    pos = np.array([0.0, 0.0, z])
    return [pos], [V.look_at(pos, np.zeros(3), np.array([0.0, 1.0, 0.0]))]


def render_and_check(tris, positions, rotations, W, H, what):
    xform = V.IDENTITY_XFORM
    got = gpu_render(tris, positions, rotations, W, H)
    want = oracle_render(np.asarray(tris, np.float32), xform, V.camera_rows(positions, rotations), H, W)
    check_against_oracle(got, want, what)
    return got, want


# ---- case A: tie-break and clipping, 32 x 32, one frame ----

TRI_FRONT = np.array([[-0.52, -0.41, 0.0], [0.63, -0.33, 0.1], [-0.07, 0.58, -0.1]], np.float32)


def test_one_triangle_matches_exactly():
    pos, rot = front_camera()
    got, want = render_and_check(TRI_FRONT[None], pos, rot, 32, 32, "one triangle")
    assert 50 < (want[3] >= 0).sum() < 32 * 32 and (got[2] >= 0).sum() == (want[3] >= 0).sum()
    # no pixel centre within 1e-3 px of an edge: the exact comparison above cannot hinge on rounding
    cams = V.camera_rows(pos, rot).astype(np.float64)[0]
    vc = (TRI_FRONT.astype(np.float64) - cams[:3]) @ cams[3:].reshape(3, 3)
    tn = math.tan(float(np.float32(V.YFOV)) * 0.5)
    xy = np.stack([(vc[:, 0] / (-vc[:, 2] * tn) + 1) * 16, (1 - vc[:, 1] / (-vc[:, 2] * tn)) * 16], -1)
    py, px = np.meshgrid(np.arange(32) + 0.5, np.arange(32) + 0.5, indexing="ij")
    for a, b in ((0, 1), (1, 2), (2, 0)):
        e = xy[b] - xy[a]
        dist = np.abs(e[0] * (py - xy[a, 1]) - e[1] * (px - xy[a, 0])) / np.linalg.norm(e)
        assert dist.min() > 1e-3


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_nearer_triangle_wins_whatever_the_order(order):
    far = TRI_FRONT + np.float32([0.1, 0.05, -0.4])
    pair = np.stack([TRI_FRONT, far])[list(order)]
    got, want = render_and_check(pair, *front_camera(), 32, 32, "two depths %s" % (order,))
    near_index = order.index(0)
    alone = [oracle_render(pair[[k]], V.IDENTITY_XFORM, V.camera_rows(*front_camera()), 32, 32)[3] >= 0 for k in (0, 1)]
    overlap = alone[0] & alone[1]
    assert overlap.sum() > 50 and (got[2][overlap] == near_index).all()
    assert (got[2] == 1 - near_index).any()                       # the far one shows where the near one is not


def test_coplanar_identical_triangles_lower_index_wins():
    got, _ = render_and_check(np.stack([TRI_FRONT, TRI_FRONT, TRI_FRONT]), *front_camera(), 32, 32, "identical triangles")
    assert set(np.unique(got[2])) == {-1, 0}


def test_triangles_behind_the_camera_or_across_the_near_plane_draw_nothing():
    behind = TRI_FRONT + np.float32([0, 0, 2.5])                            # all of it at z > 1.5
    across = np.array([[-0.3, -0.3, 0.0], [0.3, -0.3, 0.0], [0.0, 0.2, 1.48]], np.float32)      # one vertex 0.02 in front
    rgb, depth, tri = gpu_render(np.stack([behind, across]), *front_camera(), 32, 32)
    assert (rgb == 255).all() and np.isinf(depth).all() and (tri == -1).all()
    want = oracle_render(np.stack([behind, across]), V.IDENTITY_XFORM, V.camera_rows(*front_camera()), 32, 32)
    assert (want[3] == -1).all()


def test_huge_triangle_is_clamped_to_the_frame_and_guard_frames_stay_untouched():
    huge = np.array([[-30.0, -20.3, -0.5], [40.0, 26.9, 0.3], [-10.0, 60.0, 0.6]], np.float32)     # one edge runs through the frame
    small = TRI_FRONT + np.float32([0, 0, 0.7])
    tris = np.stack([huge, small])
    pos, rot = front_camera()
    H = W = 32
    cams = torch.from_numpy(V.camera_rows(pos, rot)).cuda()
    rgb = torch.full((3, H, W, 3), 77, dtype=torch.uint8, device="cuda")
    depth = torch.full((3, H, W), -5.0, dtype=torch.float32, device="cuda")
    tri = torch.full((3, H, W), 12345, dtype=torch.int32, device="cuda")
    zbuf = torch.full((3, H * W), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    V.render_into(torch.from_numpy(tris).cuda(), V.IDENTITY_XFORM, cams, H, W, rgb[1:2], depth[1:2], tri[1:2], zbuf[1])
    torch.cuda.synchronize()
    for g in (0, 2):
        assert (rgb[g] == 77).all() and (depth[g] == -5.0).all() and (tri[g] == 12345).all() and (zbuf[g] == 0x5A5A5A5A5A5A5A5A).all()
    got = (rgb[1:2].cpu().numpy(), depth[1:2].cpu().numpy(), tri[1:2].cpu().numpy())
    want = oracle_render(tris, V.IDENTITY_XFORM, V.camera_rows(pos, rot), H, W)
    check_against_oracle(got, want, "huge triangle")
    on_border = np.concatenate([want[3][0, 0], want[3][0, -1], want[3][0, :, 0], want[3][0, :, -1]])
    assert (on_border == 0).any() and (want[3] == -1).any() and (want[3] == 1).any()     # it leaves the frame, and not all of it is covered


def test_no_triangles_gives_white_frames():
    pos, rot = V.get_positions_and_rotations(n_frames=12)
    rgb, depth, tri = gpu_render(np.zeros((0, 3, 3), np.float32), pos, rot, 32, 32)
    assert rgb.shape == (12, 32, 32, 3) and (rgb == 255).all() and np.isinf(depth).all() and (depth > 0).all() and (tri == -1).all()


# ---- cases B, C: closed meshes on the reference's camera path ----

def octahedron():
    a = 0.5
    px, nx, py, ny, pz, nz = [a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, a], [0, 0, -a]
    return np.array([[px, py, pz], [py, nx, pz], [nx, ny, pz], [ny, px, pz], [py, px, nz], [nx, py, nz], [ny, nx, nz],
                     [px, ny, nz]], np.float32)


def latlong_sphere(n_lat=12, n_lon=24, r=0.5):
    """n_lat x n_lon quads split in two: 576 triangles; the two at a pole's quad include one of zero area (the sliver)."""
    th = np.linspace(0, np.pi, n_lat + 1)
    ph = np.linspace(0, 2 * np.pi, n_lon + 1)
    p = lambda i, j: [r * np.sin(th[i]) * np.cos(ph[j]), r * np.cos(th[i]), r * np.sin(th[i]) * np.sin(ph[j])]   # noqa: E731
    tris = []
    for i in range(n_lat):
        for j in range(n_lon):
            tris.append([p(i, j), p(i + 1, j), p(i + 1, j + 1)])
            tris.append([p(i, j), p(i + 1, j + 1), p(i, j + 1)])
    return np.array(tris, np.float32)


def path_frames(frames=FRAMES):
    pos, rot = V.get_positions_and_rotations(n_frames=180)
    return [pos[f] for f in frames], [rot[f] for f in frames]


def test_octahedron_on_the_camera_path():
    tris = octahedron()
    assert tris.shape == (8, 3, 3)
    render_and_check(tris, *path_frames(), 64, 64, "octahedron")


def test_sphere_with_polar_slivers_on_the_camera_path():
    tris = latlong_sphere()
    assert tris.shape == (576, 3, 3)
    render_and_check(tris, *path_frames(), 96, 96, "sphere")


def test_rectangular_odd_frame():
    """W != H (the aspect enters the projection), an odd height.  The width is even on purpose: frame 0 looks along the
    octahedron's plane x = 0, whose edges project onto x_pix = W/2 - with an odd W that is a column of pixel centres, and which
    of the two triangles sharing such an edge is nearer is then decided by the last bit of the depth."""
    render_and_check(octahedron(), *path_frames([0, 46, 100]), 46, 37, "octahedron 46 x 37")


# ---- case D: a marching-cubes mesh, pose-normalised on the fly ----

@pytest.fixture(scope="module")
def mc_mesh():
    from zeroshape_amd.utils.eval_3D import extract_surface
    G = 17
    i, j, k = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    q = ((i - 9.3) / 6.1) ** 2 + ((j - 7.2) / 4.6) ** 2 + ((k - 8.4) / 3.3) ** 2           # off-centre in the grid
    vol = torch.from_numpy(np.sqrt(q).astype(np.float32)).cuda()
    tris, _ = extract_surface(vol, 1.0, -1.5, 1.5)
    assert 300 < tris.shape[0] < 4000
    return tris


@pytest.fixture(scope="module")
def mc_frames(mc_mesh):
    pos, rot = V.get_positions_and_rotations(n_frames=180)
    run = lambda: V.render_mesh_frames(mc_mesh, pos, rot, (200, 200), return_depth=True, return_tri=True, pose_normalize=True)  # noqa: E731
    return run(), run()


def test_mesh_stats_against_numpy(mc_mesh):
    got = V.mesh_stats(mc_mesh)
    want = numpy_stats(mc_mesh.cpu().numpy())
    np.testing.assert_array_equal(got[:6], want[:6].astype(np.float32))
    assert abs(got[6] - want[6]) <= 1e-5 * abs(want[6]) and abs(want[6]) > 0.1
    np.testing.assert_array_equal(V.mesh_stats(mc_mesh), got)                  # fixed-order reduction
    np.testing.assert_array_equal(V.mesh_stats(mc_mesh[:0]), np.zeros(7, np.float32))
    one = V.mesh_stats(mc_mesh[5:6].contiguous())
    np.testing.assert_array_equal(one[:6], numpy_stats(mc_mesh[5:6].cpu().numpy())[:6].astype(np.float32))


@pytest.mark.parametrize("name,n", [("F257", 65535), ("F257", 65536), ("F257", 65537), ("F257", 131073), ("F257", None),
                                    ("F129", None)])
def test_mesh_stats_past_one_triangle_per_thread(name, n):
    """zs_mesh_stats launches at most 256 blocks of 256 threads: up to 65,536 triangles a thread has one (65,535: the last
    thread none), from 65,537 on the threads stride over the soup, and the final kernel reduces all 256 partials.  Slices
    of a production-size marching-cubes soup (open surfaces: their signed terms cancel, hence the second term of the bound)."""
    from tests.test_gpu_mc_full_size import case
    soup = case(name)[2]
    soup = soup if n is None else soup[:n]
    assert soup.is_contiguous() and soup.shape[0] == (n or soup.shape[0]) and soup.shape[0] > (65536 if n is None else 0)
    tris = soup.cpu().numpy()
    got = V.mesh_stats(soup)
    want = numpy_stats(tris)
    t64 = tris.astype(np.float64)
    terms = np.abs(np.einsum("ni,ni->n", t64[:, 0], np.cross(t64[:, 1], t64[:, 2]))).sum() / 6.0
    # one fp32 rounding of the result (2^-24 = 6e-8) + the fp64 accumulation in whatever order (n * 2^-53 = 1.5e-10 of the
    # terms' magnitudes at 1.3 M triangles, with margin)
    bound = 1.2e-7 * abs(want[6]) + 1e-9 * terms
    print("%s[:%s]: %d triangles, volume %.9g (numpy %.9g), |difference| %.3g, bound %.3g"
          % (name, n, len(tris), got[6], want[6], abs(got[6] - want[6]), bound))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got[:6], want[:6].astype(np.float32))
    assert abs(float(got[6]) - want[6]) <= bound
    np.testing.assert_array_equal(V.mesh_stats(soup).view(np.uint32), got.view(np.uint32))         # fixed-order reduction


def test_mc_mesh_turntable_is_deterministic_and_stays_in_view(mc_frames):
    a, b = mc_frames
    for x, y in zip(a, b):
        assert x.shape[:3] == (180, 200, 200) and torch.equal(x, y)
    # (depth: +inf == +inf under torch.equal; compare the bits as well)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    covered = a[2] >= 0
    assert bool(covered.flatten(1).any(1).all())                                  # every frame shows the mesh
    rows, cols = covered.any(2), covered.any(1)                                   # [F,H], [F,W]
    # pose normalisation: the mesh fits the unit cube around the origin, so it never touches the frame's border
    assert not bool(rows[:, 0].any() or rows[:, -1].any() or cols[:, 0].any() or cols[:, -1].any())
    assert bool(((a[0] == 255).all(-1) == ~covered).all())                        # the shaded mesh is never pure white


def test_mc_mesh_frames_match_the_oracle(mc_mesh, mc_frames):
    frames = [0, 60, 120]
    pos, rot = path_frames(frames)
    tris = mc_mesh.cpu().numpy()
    xform = V.pretransform_params(numpy_stats(tris))
    np.testing.assert_array_equal(xform, V.pretransform_params(V.mesh_stats(mc_mesh)))
    want = oracle_render(tris, xform, V.camera_rows(pos, rot), 200, 200)
    got = tuple(x[frames].cpu().numpy() for x in mc_frames[0])
    check_against_oracle(got, want, "marching-cubes mesh, %d triangles" % len(tris))


# ---- cases E, F: the dumps ----

def test_dump_meshes_viz_writes_gif_and_frames(mc_mesh, tmp_path):
    from PIL import Image
    from zeroshape_amd.utils.eval_3D import SimpleMesh
    opt = edict(dict(output_path=str(tmp_path), device="cuda"))
    empty = SimpleMesh(np.zeros((0, 3, 3), np.float32))
    V.dump_meshes_viz(opt, [7], "mesh_viz", [empty])
    assert list(tmp_path.iterdir()) == []                                          # an empty mesh: nothing written, nothing raised
    mesh = SimpleMesh(mc_mesh.cpu().numpy())
    V.dump_meshes_viz(opt, [3, 4], "mesh_viz", [mesh, empty], save_frames=True)
    assert sorted(p.name for p in (tmp_path / "dump").iterdir()) == ["3_mesh_viz", "3_mesh_viz.gif"]
    gif = Image.open(tmp_path / "dump" / "3_mesh_viz.gif")
    assert gif.n_frames == 180 and gif.size == (200, 200) and gif.info["duration"] == 80 and gif.info["loop"] == 0
    jpgs = sorted(p.name for p in (tmp_path / "dump" / "3_mesh_viz").iterdir())
    assert jpgs == ["%04d.jpg" % i for i in range(180)]
    assert Image.open(tmp_path / "dump" / "3_mesh_viz" / "0090.jpg").size == (200, 200)
    V.dump_meshes_viz(opt, [5], "mesh_viz", [mesh], save_frames=False, folder="preds")
    assert [p.name for p in (tmp_path / "preds").iterdir()] == ["5_mesh_viz.gif"]


def test_visualize_mesh_returns_the_frames_it_wrote(mc_mesh, tmp_path):
    from PIL import Image
    frames = V.visualize_mesh(mc_mesh.cpu().numpy(), str(tmp_path / "m"), resolution=(48, 40), write_frames=False, n_frames=12,
                              pose_normalize=True)
    assert frames.dtype == np.uint8 and frames.shape == (12, 40, 48, 3)
    gif = Image.open(tmp_path / "m.gif")
    assert gif.n_frames == 12 and gif.size == (48, 40) and not (tmp_path / "m").exists()
    pos, rot = V.get_positions_and_rotations(n_frames=12)
    want = V.render_mesh_frames(mc_mesh, pos, rot, (48, 40), pose_normalize=True).cpu().numpy()
    np.testing.assert_array_equal(frames, want)


def test_dump_attentions_writes_a_gif_of_the_level_grid_frames(seeded_sd, tmp_path):
    from PIL import Image
    from zeroshape_amd import synthetic as syn
    from zeroshape_amd.model.shape.implicit import Implicit
    from zeroshape_amd.utils import eval_3D as E
    net = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                   n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                   posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    net.load_state_dict(seeded_sd, strict=True)
    net = net.cuda().eval()
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=1)).cuda()
    opt = edict(dict(device="cuda", output_path=str(tmp_path), H=224, W=224, eval=dict(vox_res=16, range=[-1.5, 1.5]),
                     arch=dict(win_size=16)))
    grid = E.get_dense_3D_grid(opt, edict(dict(idx=[0])))
    images = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
    _, frames = E.compute_level_grid(opt, net, latent, None, grid, images, vis_attn=True)
    V.dump_attentions(opt, ["blob"], "attn", frames)
    gif = Image.open(tmp_path / "dump" / "blob_attn.gif")
    assert gif.n_frames == len(frames[0]) > 1 and gif.size == (224, 224) and gif.info["duration"] == 50
    # a tensor of raw maps is stored as it was before
    raw = torch.rand(2, 5, 197)
    V.dump_attentions(opt, [1, 2], "attn", raw)
    np.testing.assert_array_equal(np.load(tmp_path / "dump" / "2_attn.npy"), raw[1].numpy())
    assert sorted(p.name for p in (tmp_path / "dump").iterdir()) == ["1_attn.npy", "2_attn.npy", "blob_attn.gif"]


# ---- case G: demo.py --viz ----

def test_demo_script_with_viz(tmp_path, encoder_sd, seeded_sd):
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
    torch.save(dict(epoch=0, iter=0, best_val=1.0, best_ep=0, graph=full), tmp_path / "shape.ckpt")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0", ZS_SYNTHETIC_ITEMS="4", ZS_SYNTHETIC_STANDIN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--yaml=options/shape.yaml", "--task=shape",
                        "--datadir=%s/data" % tmp_path, "--eval.vox_res=32", "--ckpt=%s/shape.ckpt" % tmp_path,
                        "--output_root=%s" % tmp_path, "--viz"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    preds = tmp_path / "data" / "preds"
    names = {p.name for p in preds.iterdir()}
    base = {"blob_image_input.png", "blob_mask_input.png", "blob_depth_est.png", "blob_mesh.obj", "blob_attn.gif"}
    has_faces = any(ln.startswith("f ") for ln in open(preds / "blob_mesh.obj"))
    assert names == base | ({"blob_mesh_viz.gif"} if has_faces else set())
    attn = Image.open(preds / "blob_attn.gif")
    assert attn.n_frames == len(range(0, 33, 8)) * len(range(0, 33 // 8 * 8 + 1, 8)) and attn.size == (224, 224)
    if has_faces:
        gif = Image.open(preds / "blob_mesh_viz.gif")
        assert gif.n_frames == 180 and gif.size == (200, 200)
