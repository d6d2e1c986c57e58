"""Scenes with known answers for the vertex-colour tests (tests/test_mesh_colors_host_logic.py runs the numpy definition on
them, tests/test_gpu_mesh_colors.py the kernels).  Not a test module.

The photo is H x W = 12 x 16 with texels at multiples of 1/255 that are distinct per pixel: r = j, g = i, b = 255 ((i + j) & 1),
all over 255.  The camera is f = 8, c = (8, 6); the mesh frame is X = v scale + mean with mean = (0.25, -0.5, 1), scale = 0.5: a
point at depth Z that projects to pixel (u, w) sits at X = ((u - 8) Z / 8, (w - 6) Z / 8, Z), and every number the scenes use is
exact in float32."""
import numpy as np

H, W = 12, 16
K = np.array([[8, 0, 8], [0, 8, 6], [0, 0, 1]], np.float32)
MEAN = np.array([0.25, -0.5, 1.0], np.float32)
SCALE = np.float32(0.5)
BASE = (0.5, 0.5, 0.8)


def photo(h=H, w=W):
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (np.stack([j, i, 255 * ((i + j) & 1)]).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def texel(i, j):
    """The uint8 colour of pixel (row i, col j)."""
    return np.array([j, i, 255 * ((i + j) & 1)], np.uint8)


def mesh_point(u, w, Z):
    """The mesh-frame vertex that projects to pixel (u, w) at camera depth Z."""
    X = np.array([(u - 8.0) * Z / 8.0, (w - 6.0) * Z / 8.0, Z], np.float64)
    return ((X - MEAN.astype(np.float64)) / np.float64(SCALE)).astype(np.float32)


def quad(corners, Z, flip=False):
    """Two triangles over four pixel positions (u, w) given clockwise on the screen (x right, y down), at depth Z, wound so that
    the area-weighted normal points at the camera (``flip``: away from it)."""
    a, b, c, d = [mesh_point(u, w, Z) for u, w in corners]
    tris = np.array([[a, c, b], [a, d, c]], np.float32)
    return tris[:, [0, 2, 1]] if flip else tris


def square(u0, w0, u1, w1, Z, flip=False):
    return quad([(u0, w0), (u1, w0), (u1, w1), (u0, w1)], Z, flip)


FRONT = (4, 3, 12, 9)                     # the front square's pixel box, at Z = 2
BACK = (6, 5, 10, 7)                      # the smaller square behind it, inside its silhouette, at Z = 3
DIAMOND = [(8, 5), (10, 6), (8, 7), (6, 6)]      # behind the front square: every corner is equally far from two front corners


def weld(soup):
    """(vertices float32 [V,3], faces int64 [F,3], normals float32 [V,3]) of a soup: SimpleMesh's numpy weld."""
    from zeroshape_amd.utils.eval_3D import SimpleMesh
    m = SimpleMesh(np.asarray(soup, np.float32))
    return m.vertices, m.faces, m.vertex_normals


def scene(soup, normals=None, mask=None, image=None, **kw):
    """The arguments of mesh_vertex_colors_host as a dict."""
    v, f, n = weld(soup)
    image = photo() if image is None else image
    args = dict(vertices=v, faces=f, normals=n if normals is None else np.asarray(normals, np.float32),
                image=image, mask=np.ones(image.shape[1:], np.float32) if mask is None else mask,
                intr=K, mean=MEAN, scale=SCALE, depth_tol=0.1, base_rgb=BASE)
    args.update(kw)
    return args


def find(vertices, u, w, Z):
    """Index of the vertex at pixel (u, w), depth Z."""
    hit = np.flatnonzero((vertices == mesh_point(u, w, Z)).all(axis=1))
    assert len(hit) == 1
    return int(hit[0])


def corners(box):
    u0, w0, u1, w1 = box
    return [(u0, w0), (u1, w0), (u1, w1), (u0, w1)]


def analytic_scenes():
    """name -> scene: every scene of the CPU file, for the GPU file to run against the checker."""
    front, back = square(*FRONT, 2.0), square(*BACK, 3.0)
    out = {"front": scene(front),
           "half": scene(square(4.5, 3.5, 12.5, 9.5, 2.0)),
           "occluded": scene(np.concatenate([front, back])),
           "tie": scene(np.concatenate([front, quad(DIAMOND, 3.0)])),
           "tol_below": scene(np.concatenate([front, back]), depth_tol=2.0 * (1 - 1e-12)),
           "tol_above": scene(np.concatenate([front, back]), depth_tol=2.0 * (1 + 1e-12)),
           "flipped": scene(square(*FRONT, 2.0, flip=True)),
           "u_outside": scene(square(10, 3, 16, 9, 2.0)),
           "w_outside": scene(square(4, -1, 12, 5, 2.0)),
           "behind": behind_scene()}
    for name, fade in (("fade_mid", 4.0), ("fade_full", 1.0)):
        out[name] = scene(np.concatenate([front, back]), fade=fade)
    for k, (i, j) in enumerate([(3, 4), (3, 5), (4, 4), (4, 5)]):
        mask = np.ones((H, W), np.float32)
        mask[i, j] = 0.5
        out["mask%d" % k] = scene(front, mask=mask)
    for name, cos in (("grazing_below", 0.05), ("grazing_above", 0.15)):
        out[name] = grazing_scene(cos)
    return out


def behind_scene():
    """The front square mirrored to Z = -2 with normals that face the camera: only Z > 0 fails."""
    soup = square(*FRONT, -2.0)
    v, _, _ = weld(soup)
    X = v.astype(np.float64) * np.float64(SCALE) + MEAN.astype(np.float64)
    n = -X / np.linalg.norm(X, axis=1, keepdims=True)
    return scene(soup, normals=n.astype(np.float32))


def grazing_scene(cos):
    """The front square with normals at the given cosine to the ray towards the camera (min_cos is 0.1)."""
    soup = square(*FRONT, 2.0)
    v, _, _ = weld(soup)
    X = v.astype(np.float64) * np.float64(SCALE) + MEAN.astype(np.float64)
    d = -X / np.linalg.norm(X, axis=1, keepdims=True)
    side = np.cross(d, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    n = cos * d + np.sqrt(1.0 - cos * cos) * side
    return scene(soup, normals=n.astype(np.float32))


# ---- two marching-cubes spheres, the smaller one behind the larger in the camera: real occlusion, two components ----

SPH_H, SPH_W = 32, 48
SPH_K = np.array([[185, 0, 23.5], [0, 185, 15.5], [0, 0, 1]], np.float32)
SPH_MEAN = np.array([0.0, 0.0, 6.0], np.float32)
SPH_SCALE = np.float32(1.0)
SPH_RANGE = (-0.5, 0.5)


def two_spheres_volume(vox):
    """Occupancy [G,G,G] float32 (G = vox + 1 samples over SPH_RANGE, x slowest), above 0.5 inside a sphere of radius 0.38 at
    (0, 0, -0.11) and a sphere of radius 0.08 at (0.03, 0.02, 0.4) - farther from the camera, mostly inside the first one's
    silhouette."""
    axis = np.linspace(SPH_RANGE[0], SPH_RANGE[1], vox + 1)
    x, y, z = np.meshgrid(axis, axis, axis, indexing="ij")
    d1 = np.sqrt(x * x + y * y + (z + 0.11) ** 2) - 0.38
    d2 = np.sqrt((x - 0.03) ** 2 + (y - 0.02) ** 2 + (z - 0.4) ** 2) - 0.08
    return np.clip(0.5 - 4.0 * np.minimum(d1, d2), 0.0, 1.0).astype(np.float32)


def sphere_photo_and_mask():
    """The 32 x 48 photo and a mask that is 1 inside a disc of 12.5 pixels around the principal point (it cuts the silhouette
    of the larger sphere, so the mask rule decides some vertices)."""
    i, j = np.meshgrid(np.arange(SPH_H), np.arange(SPH_W), indexing="ij")
    mask = ((i - 15.5) ** 2 + (j - 23.5) ** 2 <= 12.5 ** 2).astype(np.float32)
    return photo(SPH_H, SPH_W), mask


def sphere_depth_tol(vox):
    return 1.5 * (SPH_RANGE[1] - SPH_RANGE[0]) / vox
