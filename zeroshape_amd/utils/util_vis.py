"""Result dumps for demo.py and Runner.dump_results.  The reference's utils/util_vis.py renders with pyrender / cv2 /
trimesh, which this image does not have (and pyrender needs OpenGL, which a headless compute node does not have either).
Here: input image and mask as PNG, depth maps as 16-bit PNG, meshes as Wavefront OBJ with welded vertices, attention maps as
.npy or - given the frames of ``compute_level_grid(vis_attn=True)`` - as GIF, the rotating mesh render of ``dump_meshes_viz``
/ ``visualize_mesh`` from the library's own rasteriser (csrc/render.hip: all frames in one call, one copy back to the host),
the textured seen-surface mesh of ``dump_seen_surface`` / ``create_seen_surface`` (csrc/seen_mesh.hip: validity, edge tests
and the order-preserving compaction of a whole batch in one call; the .obj / .mtl text is the reference's byte for byte) and
the coloured point clouds of ``dump_pointclouds_compare`` / ``dump_pointclouds`` as binary PLY.
The turntable's geometry and shading formula are pinned by tests; pyrender's PBR pixels are not reproduced (parity unpinned).
File names follow the reference's `<output_path>/<folder>/<idx>_<name>.<ext>` pattern."""
import os

import numpy as np


def _path(opt, folder, idx, name, ext):
    d = os.path.join(opt.output_path, folder)
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, "{}_{}.{}".format(idx, name, ext))


def _write_gif(path, images, duration):
    """PIL images -> looping GIF at ``duration`` ms a frame, one GIF frame per image, each whole and with its own colour
    table.  ``Image.save(save_all=True)`` folds an image that equals the one before it into that one's duration; the
    turntable's camera path repeats a pose where two of its segments meet, so it would write 177 frames for 180."""
    from PIL import GifImagePlugin, Image
    frames = [im if im.mode == "P" else im.convert("P", palette=Image.Palette.ADAPTIVE) for im in images]
    with open(path, "wb") as fp:
        for block in GifImagePlugin.getheader(frames[0], info=dict(loop=0, duration=duration))[0]:
            fp.write(block)
        for frame in frames:
            for block in GifImagePlugin.getdata(frame, duration=duration, include_color_table=True):
                fp.write(block)
        fp.write(b";")


def dump_images(opt, idx, name, images, masks=None, from_range=(0, 1), folder="dump", **_):
    """images [B,C,H,W] (C = 1 or 3) in `from_range` -> 8-bit PNG (with `masks` as alpha)."""
    from PIL import Image
    lo, hi = from_range
    x = ((images.detach().float().cpu().numpy() - lo) / (hi - lo)).clip(0, 1)
    for b, i in enumerate(idx):
        img = (x[b].transpose(1, 2, 0) * 255 + 0.5).astype(np.uint8)
        if img.shape[2] == 1:
            img = img[:, :, 0]
        im = Image.fromarray(img)
        if masks is not None:
            im.putalpha(Image.fromarray((masks[b, 0].detach().cpu().numpy() * 255).astype(np.uint8)))
        im.save(_path(opt, folder, i, name, "png"))


def dump_depths(opt, idx, name, depths, masks=None, rescale=False, folder="dump", **_):
    """depths [B,1,H,W] -> 16-bit PNG; with `rescale` the masked range is stretched to full scale."""
    from PIL import Image
    d = depths.detach().float().cpu().numpy()[:, 0]
    for b, i in enumerate(idx):
        x = d[b]
        if masks is not None:
            m = masks[b, 0].detach().cpu().numpy() > 0.5
            if rescale and m.any():
                lo, hi = x[m].min(), x[m].max()
                x = (x - lo) / max(hi - lo, 1e-8)
            x = np.where(m, x, 1.0)
        Image.fromarray((x.clip(0, 1) * 65535 + 0.5).astype(np.uint16)).save(_path(opt, folder, i, name, "png"))


def dump_meshes(opt, idx, name, meshes, folder="dump", normals=False, colors=False, **_):
    """meshes: eval_3D.SimpleMesh objects -> OBJ with shared vertices (the indexed form mcubes.marching_cubes returns in
    the reference; the marching-cubes kernel emits bit-identical coordinates for shared vertices): a comment line, one
    ``v %.6f %.6f %.6f`` per vertex, one ``f %d %d %d`` per face.  With ``normals`` also one ``vn %.6f %.6f %.6f`` per vertex
    (mesh.vertex_normals) after the vertices, and the faces as ``f a//a b//b c//c``, so that a viewer shades smoothly.
    ``normals="field"``: the same lines from mesh.field_normals (eval_3D.field_normals: minus the field's normalised gradient).
    With ``colors`` the vertex lines become ``v %.6f %.6f %.6f %.6f %.6f %.6f`` - x y z r g b with r, g, b = mesh.vertex_colors / 255
    (eval_3D.vertex_colors), the de-facto OBJ vertex-colour extension MeshLab, Blender and Open3D read; it combines with ``normals``.
    Formatted in bulk, one % per block and one write per file: the same bytes as a write per line, which took 64 ms for the
    vox-128 mesh."""
    if isinstance(normals, str) and normals != "field":
        raise ValueError("dump_meshes: normals must be False, True or 'field', got %r" % (normals,))
    for i, mesh in zip(idx, meshes):
        if normals == "field":
            vn = mesh.field_normals
        else:
            vn = mesh.vertex_normals if normals else None         # (first: a GPU-built mesh then welds once)
        verts, faces = mesh.vertices, mesh.faces + 1              # the indexed form (eval_3D.SimpleMesh welds the soup)
        text = ["# zeroshape_amd mesh: %d vertices, %d faces\n" % (len(verts), len(faces))]
        if colors:
            rows = np.concatenate([verts.astype(np.float64), mesh.vertex_colors.astype(np.float64) / 255.0], axis=1)
            text.append(("v %.6f %.6f %.6f %.6f %.6f %.6f\n" * len(rows)) % tuple(rows.ravel().tolist()))
        else:
            text.append(("v %.6f %.6f %.6f\n" * len(verts)) % tuple(verts.astype(np.float64).ravel().tolist()))
        if normals:
            text += [("vn %.6f %.6f %.6f\n" * len(vn)) % tuple(vn.astype(np.float64).ravel().tolist()),
                     ("f %d//%d %d//%d %d//%d\n" * len(faces)) % tuple(np.repeat(faces, 2, axis=1).ravel().tolist())]
        else:
            text.append(("f %d %d %d\n" * len(faces)) % tuple(faces.ravel().tolist()))
        with open(_path(opt, folder, i, name, "obj"), "w") as f:
            f.write("".join(text))


def dump_mesh_reports(opt, idx, name, meshes, folder="dump", **_):
    """meshes: eval_3D.SimpleMesh objects -> one JSON file each (eval_3D.mesh_report): the totals under trimesh's names -
    area, volume, euler_number, is_watertight, the vertex, face and component counts - and the per-component table."""
    import json
    from . import eval_3D
    for i, mesh in zip(idx, meshes):
        with open(_path(opt, folder, i, name, "json"), "w") as f:
            json.dump(eval_3D.mesh_report(mesh), f, indent=1)
            f.write("\n")


def dump_attentions(opt, idx, name, attn, folder="dump", **_):
    """Per-sample frame lists (what ``compute_level_grid(vis_attn=True)`` returns: [H,W,3] arrays in [0,1]) -> GIF at 50 ms a
    frame like the reference (utils/util_vis.py:93-97).  A tensor (or a list of tensors) of raw maps -> .npy per sample: the
    reference colour-maps those over the image with cv2, here they are stored as they are."""
    if attn is None:
        return
    for b, i in enumerate(idx):
        a = attn[b]
        if isinstance(a, (list, tuple)):
            from PIL import Image
            frames = [Image.fromarray((np.asarray(f) * 255).astype(np.uint8)).convert("RGB") for f in a]
            if frames:
                _write_gif(_path(opt, folder, i, name, "gif"), frames, 50)
            continue
        np.save(_path(opt, folder, i, name, "npy"), np.asarray(a.detach().cpu() if hasattr(a, "detach") else a))


# ---- mesh turntable (utils/util_vis.py:112-127, 295-405) ----

YFOV = np.pi / 3.0                  # pyrender.PerspectiveCamera(yfov=np.pi / 3.0, aspectRatio=1.0)
ZNEAR = 0.05                        # pyrender's default near plane
BASE_RGB = (0.5, 0.5, 0.8)          # baseColorFactor of the reference's material


def look_at(camera_position, camera_target, up_vector):
    """utils/util_vis.py:295-308: the camera's axes as the columns of the upper 3x3 (right, up, backward - the camera looks
    along -z), and the translation of the inverse in the last row."""
    back = camera_position - camera_target
    back = back / np.linalg.norm(back)
    right = np.cross(up_vector, back)
    right = right / np.linalg.norm(right)
    up = np.cross(back, right)
    return np.array([
        [right[0], up[0], back[0], 0.0],
        [right[1], up[1], back[1], 0.0],
        [right[2], up[2], back[2], 0.0],
        [-np.dot(right, camera_position), -np.dot(up, camera_position), np.dot(back, camera_position), 1.0]])


def get_positions_and_rotations(n_frames=180, r=1.5):
    """utils/util_vis.py:320-346: the four-segment camera path around the origin at radius ``r`` in the horizontal plane - a
    full circle descending from height 1 to -1, half a circle at -1, a full circle climbing back, half a circle at 1."""
    n_full, n_half = n_frames // 3, n_frames // 6
    ring = lambda theta, elev: np.array([r * np.cos(theta), elev, r * np.sin(theta)])      # noqa: E731
    pos = [ring(t, e) for t, e in zip(np.linspace(0.5 * np.pi, 2.5 * np.pi, n_full), np.linspace(1, -1, n_full))]
    pos += [ring(t, -1) for t in np.linspace(2.5 * np.pi, 3.5 * np.pi, n_half)]
    pos += [ring(t, e) for t, e in zip(np.linspace(3.5 * np.pi, 5.5 * np.pi, n_full), np.linspace(-1, 1, n_full))]
    pos += [ring(t, 1) for t in np.linspace(3.5 * np.pi, 4.5 * np.pi, n_half)]
    target, up = np.array([0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    return pos, [look_at(x, target, up) for x in pos]


IDENTITY_XFORM = np.array([1, 1, 1, 0, 0, 0, 1, 1], np.float32)


def pretransform_params(stats):
    """``stats`` = (bounding-box min xyz, max xyz, signed volume) of a triangle soup, what zs_mesh_stats writes -> the eight
    numbers zs_render_frames applies on the fly, (flip xyz, centre xyz, scale, winding): dump_meshes_viz's two 180-degree
    rotations about z and then y, (x, y, z) -> (x, -y, -z); scale_to_unit_cube's centring on the bounding box of the rotated
    mesh and scaling by 1 / its largest extent; trimesh.repair.fix_inversion's v1 <-> v2 exchange when the volume is negative
    (the rotations are proper, they leave its sign alone)."""
    stats = np.asarray(stats, np.float64)
    flip = np.array([1.0, -1.0, -1.0])
    a, b = stats[0:3] * flip, stats[3:6] * flip
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    extent = float(np.max(hi - lo))
    if not extent > 0:
        raise ValueError("mesh has no extent")
    winding = -1.0 if stats[6] < 0 else 1.0
    return np.concatenate([flip, (lo + hi) / 2, [1.0 / extent, winding]]).astype(np.float32)


def camera_rows(positions, rotations):
    """[F][12] fp32 rows for zs_render_frames: position, then the camera-to-world rotation (the upper 3x3 of what look_at
    returns, as visualize_mesh puts it into the pose, utils/util_vis.py:384-386)."""
    pos = np.asarray(positions, np.float64).reshape(-1, 3)
    rot = np.asarray(rotations, np.float64)[:, :3, :3].reshape(-1, 9)
    assert len(pos) == len(rot)
    return np.ascontiguousarray(np.concatenate([pos, rot], axis=1), np.float32)


def mesh_stats(triangles):
    """zs_mesh_stats of a GPU soup [n,3,3] fp32 -> 7 floats on the host (a 28-byte copy)."""
    import torch
    from .. import _lib
    lib = _lib.load()
    n = triangles.shape[0]
    out = torch.empty(7, dtype=torch.float32, device=triangles.device)
    scratch = torch.empty(max(lib.zs_mesh_stats_scratch_bytes(n) // 8, 1), dtype=torch.float64, device=triangles.device)
    with _lib.on(triangles.device):
        _lib.check(lib.zs_mesh_stats(_lib.ptr(triangles), n, _lib.ptr(out), _lib.ptr(scratch),
                                     _lib.current_stream_ptr(triangles.device)), "zs_mesh_stats")
    return out.cpu().numpy()


def render_into(triangles, xform, cams, H, W, rgb, depth=None, tri=None, zbuffer=None, corner_colors=None):
    """zs_render_frames into caller-owned GPU buffers: ``triangles`` [n,3,3] fp32, ``xform`` 8 host floats, ``cams`` [F,12]
    fp32 on the device, ``rgb`` uint8 [F,H,W,3], ``depth`` fp32 / ``tri`` int32 [F,H,W] or None.  With ``corner_colors`` (uint8
    [n,3,3] on the device: r g b of every triangle corner) zs_render_frames_colored: the albedo is interpolated from them
    instead of BASE_RGB."""
    import ctypes
    import torch
    from .. import _lib
    lib = _lib.load()
    dev = triangles.device
    F = cams.shape[0]
    assert triangles.is_cuda and triangles.dtype == torch.float32 and triangles.is_contiguous() and triangles.shape[1:] == (3, 3)
    assert cams.device == dev and cams.dtype == torch.float32 and cams.is_contiguous() and cams.shape == (F, 12)
    assert rgb.device == dev and rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.shape == (F, H, W, 3)
    assert depth is None or (depth.device == dev and depth.dtype == torch.float32 and depth.is_contiguous()
                             and depth.shape == (F, H, W))
    assert tri is None or (tri.device == dev and tri.dtype == torch.int32 and tri.is_contiguous() and tri.shape == (F, H, W))
    if zbuffer is None:
        zbuffer = torch.empty(max(lib.zs_render_zbuffer_bytes(F, H, W) // 8, 1), dtype=torch.int64, device=dev)
    assert zbuffer.device == dev and zbuffer.numel() * zbuffer.element_size() >= lib.zs_render_zbuffer_bytes(F, H, W)
    xf = (ctypes.c_float * 8)(*[float(v) for v in xform])
    base = (ctypes.c_float * 3)(*BASE_RGB)
    with _lib.on(dev):
        if corner_colors is not None:
            assert (corner_colors.device == dev and corner_colors.dtype == torch.uint8 and corner_colors.is_contiguous()
                    and corner_colors.shape == (triangles.shape[0], 3, 3))
            _lib.check(lib.zs_render_frames_colored(_lib.ptr(triangles), triangles.shape[0], xf, _lib.ptr(cams), F, H, W, float(YFOV),
                                                    float(ZNEAR), _lib.ptr(corner_colors), _lib.ptr(rgb), _lib.ptr(depth),
                                                    _lib.ptr(tri), _lib.ptr(zbuffer), _lib.current_stream_ptr(dev)),
                       "zs_render_frames_colored")
            return
        _lib.check(lib.zs_render_frames(_lib.ptr(triangles), triangles.shape[0], xf, _lib.ptr(cams), F, H, W, float(YFOV),
                                        float(ZNEAR), base, _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(tri), _lib.ptr(zbuffer),
                                        _lib.current_stream_ptr(dev)), "zs_render_frames")


def render_mesh_frames(triangles, positions, rotations, resolution, return_depth=False, return_tri=False,
                       pose_normalize=False, corner_colors=None):
    """All frames of a camera path in one call.  ``triangles``: GPU tensor [n,3,3] fp32; ``positions`` / ``rotations``: what
    get_positions_and_rotations returns; ``resolution`` = (width, height) like pyrender.OffscreenRenderer's.  Returns the
    GPU tensor rgb uint8 [F,H,W,3], or the tuple (rgb[, depth fp32 [F,H,W]][, tri int32 [F,H,W]]).  With ``pose_normalize`` the
    mesh is turned, centred and scaled on the fly as dump_meshes_viz does (pretransform_params of its zs_mesh_stats).
    ``corner_colors``: uint8 [n,3,3] on the device (``vertex_colors[faces]``) instead of the one BASE_RGB."""
    import torch
    W, H = int(resolution[0]), int(resolution[1])
    dev = triangles.device
    triangles = triangles.detach().contiguous()
    cams = torch.from_numpy(camera_rows(positions, rotations)).to(dev)
    F = cams.shape[0]
    xform = pretransform_params(mesh_stats(triangles)) if pose_normalize and triangles.shape[0] else IDENTITY_XFORM
    rgb = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    depth = torch.empty(F, H, W, dtype=torch.float32, device=dev) if return_depth else None
    tri = torch.empty(F, H, W, dtype=torch.int32, device=dev) if return_tri else None
    render_into(triangles, xform, cams, H, W, rgb, depth, tri, corner_colors=corner_colors)
    out = (rgb,) + ((depth,) if return_depth else ()) + ((tri,) if return_tri else ())
    return out[0] if len(out) == 1 else out


def _soup(mesh):
    """The triangle soup of ``mesh``: a SimpleMesh's GPU tensor when it was built from one (no host copy, no second upload),
    else its host array; anything else is taken to be the soup itself."""
    soup = getattr(mesh, "device_triangles", None)
    return soup if soup is not None else getattr(mesh, "triangles", mesh)


def corner_colors(mesh):
    """uint8 [n,3,3] on the device: the vertex colours of a coloured GPU SimpleMesh at every corner of its soup (the weld's faces
    are in soup order), for render_mesh_frames."""
    if getattr(mesh, "device_vertex_colors", None) is None:
        raise ValueError("this mesh has no vertex colours: eval_3D.vertex_colors(opt, var) computes them")
    return mesh.device_vertex_colors[mesh._device_weld[1].long()].contiguous()


def visualize_mesh(mesh, output_path, resolution=(200, 200), write_gif=True, write_frames=True, time_per_frame=80,
                   n_frames=180, pose_normalize=False, device="cuda", colors=False):
    """utils/util_vis.py:348-405.  ``mesh``: an eval_3D.SimpleMesh, or a triangle soup [n,3,3] as tensor or array (a host
    soup is uploaded once).  Renders the ``n_frames`` of get_positions_and_rotations in one call, copies them to the host
    once, writes ``<output_path>.gif`` (80 ms a frame, endless loop - the reference ignores ``time_per_frame`` too) and, with
    ``write_frames``, ``<output_path>/0000.jpg ...``.  With ``colors`` (a SimpleMesh that eval_3D.vertex_colors coloured) the
    albedo is the mesh's vertex colours, gathered per triangle corner on the device.  Returns the frames, uint8 [n_frames,H,W,3]."""
    import torch
    from PIL import Image
    soup = _soup(mesh)
    if not isinstance(soup, torch.Tensor):
        soup = torch.from_numpy(np.ascontiguousarray(soup, np.float32)).to(device)
    soup = soup.to(torch.float32).reshape(-1, 3, 3)
    positions, rotations = get_positions_and_rotations(n_frames=n_frames)
    frames = render_mesh_frames(soup, positions, rotations, resolution, pose_normalize=pose_normalize,
                                corner_colors=corner_colors(mesh) if colors else None).cpu().numpy()
    images = [Image.fromarray(f, mode="RGB") for f in frames]
    if write_gif:
        _write_gif("{}.gif".format(output_path), images, 80)
    if write_frames:
        os.makedirs(output_path, exist_ok=True)
        for i, img in enumerate(images):
            img.save(os.path.join(output_path, "{:04d}.jpg".format(i)))
    return frames


def dump_meshes_viz(opt, idx, name, meshes, save_frames=True, folder="dump", colors=False):
    """utils/util_vis.py:112-127: ``<idx>_<name>.gif`` (and ``<idx>_<name>/0000.jpg ...`` with ``save_frames``) of every mesh,
    turned, centred and scaled to the unit cube.  An empty mesh writes nothing and raises nothing (the reference's
    ``try/except`` around scale_to_unit_cube).  ``colors``: the meshes' vertex colours instead of BASE_RGB (visualize_mesh)."""
    for i, mesh in zip(idx, meshes):
        if len(_soup(mesh)) == 0:                    # (a tensor's length is its shape: no copy to the host)
            continue
        fname = _path(opt, folder, i, name, "gif")[:-4]
        visualize_mesh(mesh, fname, write_frames=save_frames, pose_normalize=True, device=getattr(opt, "device", "cuda"),
                       colors=colors)


# ---- seen-surface mesh (utils/util_vis.py:129-170) ----

def seen_mesh_buffers(xyz, mask=None, connect_thres=0.005):
    """zs_seen_mesh on a GPU point map ``xyz`` [B,H,W,3] (``mask``: B*H*W values, a pixel with mask <= 0.5 is no vertex) ->
    the GPU tensors (vert_id int32 [B,H,W], vert_pixel int32 [B,H*W], verts fp32 [B,H*W,3], faces int32
    [B,2(H-1)(W-1),3], counts int32 [B,2]).  Rows of the three compacted buffers beyond ``counts`` are unwritten."""
    import torch
    from .. import _lib
    if not (isinstance(xyz, torch.Tensor) and xyz.is_cuda):
        raise ValueError("seen_surface_mesh: xyz must be a GPU tensor (there is no CPU path)")
    if xyz.dim() != 4 or xyz.shape[3] != 3:
        raise ValueError("seen_surface_mesh: xyz must be [B,H,W,3], got %s" % (tuple(xyz.shape),))
    lib = _lib.load()
    dev = xyz.device
    B, H, W = xyz.shape[:3]
    xyz = xyz.detach().to(torch.float32).contiguous()
    if mask is not None:
        if not mask.is_cuda or mask.numel() != B * H * W:
            raise ValueError("seen_surface_mesh: mask must be a GPU tensor of B*H*W values")
        mask = mask.detach().to(torch.float32).contiguous()
    cells = max(H - 1, 0) * max(W - 1, 0)
    vert_id = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    vert_pixel = torch.empty(B, H * W, dtype=torch.int32, device=dev)
    verts = torch.empty(B, H * W, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(B, 2 * cells, 3, dtype=torch.int32, device=dev)
    counts = torch.zeros(B, 2, dtype=torch.int32, device=dev)
    if B * H * W:
        ws = torch.empty(max(lib.zs_seen_mesh_workspace_bytes(B, H, W) // 8, 1), dtype=torch.int64, device=dev)
        with _lib.on(dev):
            _lib.check(lib.zs_seen_mesh(_lib.ptr(xyz), _lib.ptr(mask), B, H, W, float(connect_thres), _lib.ptr(vert_id),
                                        _lib.ptr(vert_pixel), _lib.ptr(verts), _lib.ptr(faces) if cells else None,
                                        _lib.ptr(counts), _lib.ptr(ws), _lib.current_stream_ptr(dev)), "zs_seen_mesh")
    return vert_id, vert_pixel, verts, faces, counts


def seen_surface_mesh(xyz, mask=None, connect_thres=0.005):
    """The seen-surface meshes of a batch of camera-frame point maps, by the rules of create_seen_surface
    (utils/util_vis.py:137-170): ``xyz`` GPU tensor [B,H,W,3] -> per image (verts float32 [n,3], pixels int32 [n] = raster
    index y*W+x of every vertex, faces int32 [m,3] = 1-based vertex indices) as numpy arrays.  One kernel call for the
    batch; the copy back is the counts first, then only the used prefixes of the three buffers (one copy each)."""
    import torch
    _, vert_pixel, verts, faces, counts = seen_mesh_buffers(xyz, mask, connect_thres)
    n = counts.cpu().numpy()
    B = n.shape[0]
    if B == 0:
        return []

    def used(buf, col):
        return torch.cat([buf[b, :int(n[b, col])] for b in range(B)]).cpu().numpy()

    v, p, f = used(verts, 0), used(vert_pixel, 0), used(faces, 1)
    vo, fo = np.concatenate([[0], np.cumsum(n[:, 0])]), np.concatenate([[0], np.cumsum(n[:, 1])])
    return [(v[vo[b]:vo[b + 1]], p[vo[b]:vo[b + 1]], f[fo[b]:fo[b + 1]]) for b in range(B)]


def write_seen_surface_obj(output_folder, sample_ID, obj_name, img_path, verts, pixels, faces, H, W):
    """The host half of create_seen_surface: ``<output_folder>/<sample_ID>_<obj_name>.mtl`` and ``.obj`` with the
    reference's text byte for byte (utils/util_vis.py:141-170) - per vertex ``v %.4f %.4f %.4f`` and ``vt %.8f %.8f`` with
    u = x / W, v = 1 - y / H in float64 from the pixel index (fp32 uv would change the eighth decimal), then ``usemtl`` and
    one ``f a/a b/b c/c`` per face.  Formatted in bulk: one % per block, one write per file."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    pixels = np.asarray(pixels, np.int64).reshape(-1)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    assert len(verts) == len(pixels)
    stem = "{}/{}_{}".format(output_folder, sample_ID, obj_name)
    with open(stem + ".mtl", "w") as f:
        f.write("newmtl material_0\n"
                "Ka 0.200000 0.200000 0.200000\n"
                "Kd 0.752941 0.752941 0.752941\n"
                "Ks 1.000000 1.000000 1.000000\n"
                "Tr 1.000000\n"
                "illum 2\n"
                "Ns 0.000000\n"
                "map_Ka %s\n"
                "map_Kd %s\n" % (img_path, img_path))
    y, x = pixels // W, pixels % W
    u, v = x.astype(np.float64) / float(W), 1.0 - y.astype(np.float64) / float(H)
    rows = np.concatenate([verts.astype(np.float64), u[:, None], v[:, None]], axis=1)
    text = ["mtllib {}_{}.mtl\n".format(sample_ID, obj_name),
            ("v %.4f %.4f %.4f\nvt %.8f %.8f\n" * len(rows)) % tuple(rows.ravel().tolist()),
            "usemtl material_0\n",
            ("f %d/%d %d/%d %d/%d\n" * len(faces)) % tuple(np.repeat(faces, 2, axis=1).ravel().tolist())]
    with open(stem + ".obj", "w") as f:
        f.write("".join(text))


def create_seen_surface(sample_ID, img_path, XYZ, output_folder, obj_name, connect_thres=0.005):
    """utils/util_vis.py:137-170 for one GPU point map ``XYZ`` [H,W,3]: the mesh from zs_seen_mesh, the files from
    write_seen_surface_obj."""
    H, W = XYZ.shape[:2]
    (verts, pixels, faces), = seen_surface_mesh(XYZ[None], None, connect_thres)
    write_seen_surface_obj(output_folder, sample_ID, obj_name, img_path, verts, pixels, faces, H, W)


def dump_seen_surface(opt, idx, obj_name, img_name, seen_projs, folder='dump', masks=None):
    """utils/util_vis.py:129-134: ``seen_projs`` [B,H,W,3] on the GPU -> ``<idx>_<obj_name>.obj/.mtl`` per sample, textured
    with ``<idx>_<img_name>.png`` of the same folder.  The whole batch goes through one kernel call; ``masks`` (B*H*W
    values, optional) is the kernel's validity mask."""
    out_folder = "{}/{}".format(opt.output_path, folder)
    os.makedirs(out_folder, exist_ok=True)
    H, W = seen_projs.shape[1:3]
    for i, (verts, pixels, faces) in zip(idx, seen_surface_mesh(seen_projs, masks)):
        write_seen_surface_obj(out_folder, i, obj_name, "{}_{}.png".format(i, img_name), verts, pixels, faces, H, W)


# ---- coloured point clouds (utils/util_vis.py:172-197) ----

_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                        ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])


def write_pointcloud_ply(path, points, colors):
    """``points`` [N,3] and ``colors`` [N,3] uint8 -> binary little-endian PLY: ``element vertex N``, ``property float
    x/y/z``, ``property uchar red/green/blue/alpha`` (alpha 255) - the layout trimesh writes for a coloured PointCloud.
    trimesh is not a dependency of this package: byte parity with its exporter (its header comment included) is unpinned."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    assert len(points) == len(colors)
    rec = np.empty(len(points), _PLY_VERTEX)
    rec["x"], rec["y"], rec["z"] = points[:, 0], points[:, 1], points[:, 2]
    rec["red"], rec["green"], rec["blue"], rec["alpha"] = colors[:, 0], colors[:, 1], colors[:, 2], 255
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
              "end_header\n" % len(points))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def dump_pointclouds_compare(opt, idx, name, preds, gts, folder='dump'):
    """utils/util_vis.py:172-184: ``<idx>_<name>.ply`` with the prediction [N1,3] in red (255,0,0) and the ground truth
    [N2,3] in green (0,255,0), prediction rows first (binary PLY of write_pointcloud_ply; parity with trimesh unpinned)."""
    for b, i in enumerate(idx):
        pred, gt = _host(preds[b]).reshape(-1, 3), _host(gts[b]).reshape(-1, 3)
        colors = np.zeros((len(pred) + len(gt), 3), np.uint8)
        colors[:len(pred), 0] = 255
        colors[len(pred):, 1] = 255
        write_pointcloud_ply(_path(opt, folder, i, name, "ply"), np.vstack([pred, gt]), colors)


def dump_pointclouds(opt, idx, name, pcs, colors, folder='dump', colormap='jet'):
    """utils/util_vis.py:186-197: ``<idx>_<name>.ply`` of every cloud [N,3]; ``colors`` [N,3] uint8, or [N,1] in [0,1] mapped
    through the 256-entry jet table of eval_3D._jet_lut (entry floor(255 c); matplotlib is not a dependency, another
    colormap raises).  Binary PLY of write_pointcloud_ply; parity with trimesh unpinned."""
    if colormap != 'jet':
        raise ValueError("dump_pointclouds: only the 'jet' colormap is built in, got %r" % (colormap,))
    from .eval_3D import _jet_lut
    for i, pc, color in zip(idx, pcs, colors):
        color = _host(color)
        if color.ndim == 2 and color.shape[1] == 1:
            color = _jet_lut()[np.uint8(255 * np.clip(color[:, 0].astype(np.float64), 0.0, 1.0))]
        write_pointcloud_ply(_path(opt, folder, i, name, "ply"), _host(pc), color[:, :3])
