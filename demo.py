#!/usr/bin/env python3
"""Single-image demo with the reference's command line (demo.py of ZeroShape):

    python demo.py --yaml=options/shape.yaml --task=shape --datadir=examples --eval.vox_res=128 --ckpt=weights/shape.ckpt
    python demo.py --yaml=options/depth.yaml --task=depth --datadir=examples --ckpt=weights/depth.ckpt
    python demo.py --yaml=options/shape.yaml --task=shape --datadir=examples --ckpt=weights/shape.ckpt --viz

<datadir>/images/*.png|jpg with <datadir>/masks/<same name>.png -> <datadir>/preds/: the cropped
input and mask, and for the shape task the reconstructed mesh (marching cubes at 0.5 of the
(vox_res+1)^3 occupancy grid, as OBJ), for the depth task the depth map and two textured meshes of the
surface the camera sees, <name>_seen_surface_fixed.obj/.mtl from the fixed intrinsics and
<name>_seen_surface_pred.obj/.mtl from the predicted ones (the pair that shows what the intrinsics head
does; written when the graph has one), both textured with <name>_image_input.png.  The predicted depth is
unprojected on the GPU and the meshes - validity, edge tests, vertex and face order of the reference's
create_seen_surface - come from one kernel call each (csrc/seen_mesh.hip).  Same preprocessing as the
reference (demo.py:27-70: mask binarised at 127, square crop 1.2x the mask's bounding box, resize to
image_size, white background, intrinsics f = 1.3875 * W).  Everything after image loading runs on
the GPU through the HIP library.

--viz (opt-in, shape task) adds the two animations the reference's demo leaves: <name>_attn.gif, the
attention of the decoder's points over the input image as the query sweeps the grid (the slice-loop
path with vis_attn=True), and <name>_mesh_viz.gif, 180 frames of the mesh on the reference's camera
path from the library's rasteriser (geometry and shading formula pinned by tests; pyrender's PBR
pixels are not reproduced).  Without --viz the files written are exactly the four above.

--eval.field_normals=true (opt-in, shape task) gives <name>_mesh.obj one `vn` line per vertex - minus the normalised
gradient of the occupancy field at the vertex (eval_3D.field_normals) - and faces of the form a//a.

--eval.min_component_area=0.05 and --eval.drop_cavities=true (opt-in, shape task) clean the mesh on the GPU before it is
written (eval_3D.filter_components): connected components whose area is below that fraction of the largest one's - the
detached blobs of a single-view reconstruction - and closed inner shells of negative volume are dropped.
--eval.mesh_report=true adds <name>_mesh_report.json next to the .obj: area, volume, Euler number, watertightness and the
per-component table (faces, vertices, edges, boundary / non-manifold / misoriented edges, area, signed volume) of the mesh
that was written.

--eval.smooth_iterations=10 (opt-in, shape task) smooths the mesh on the GPU before it is written (eval_3D.smooth_mesh, after
the component filter): Taubin passes over the vertex neighbourhood, which take the terraces out of a sharp field's marching
cubes without the shrinkage of plain Laplacian smoothing.  --eval.smooth_lambda (0.5) and --eval.smooth_mu (-0.53; none =
plain Laplacian passes) are the two factors, --eval.smooth_free_boundary=true lets the vertices of open edges move too.

--eval.simplify_cells=2.0 (opt-in, shape task) makes the mesh lighter on the GPU before it is written (eval_3D.simplify_mesh,
after the component filter and the smoothing, before the colours and any sampling - so every number reported describes the
mesh that is delivered): the vertices inside each cube of that many marching-cubes cells become one vertex, placed where the
quadric error of the faces around them is smallest, and the faces that collapse or repeat are dropped (2 cells: about a fifth
of the faces).  --eval.simplify_position=mean places the vertex at the cluster's mean instead.  Watertightness is not
guaranteed - coarse cells join sheets that pass through one cell; with --eval.mesh_report=true the report says what came out
and gains a `simplification` entry with the counts.

--eval.mesh_deviation=true (opt-in, with --eval.smooth_iterations or --eval.simplify_cells; an error without either) measures
how far the smoothing and the simplification moved the surface (eval_3D.mesh_deviation, exact point-to-triangle distances on
the GPU): the distance of every vertex of the delivered mesh to the surface marching cubes extracted (after the component
filter: dropping floaters is intended) and of every vertex of that surface to the delivered mesh.  With --eval.mesh_report=true
the report gains a `deviation` entry: max, mean, rms and the vertex at the maximum for both directions, in mesh units and in
marching-cubes cells.  It is sampled at the vertices: a lower bound on the Hausdorff distance, not the continuous one.

--eval.mesh_iou=true (opt-in, with --eval.smooth_iterations or --eval.simplify_cells; an error without either) measures how
much volume those steps added or removed (eval_3D.mesh_volume_iou, exact point-in-mesh tests on the GPU): the occupancy of the
delivered mesh and of the surface marching cubes extracted (after the component filter) at the points of the evaluation
grid's own lattice.  With --eval.mesh_report=true the report gains a `volume_iou` entry: the lattice points inside each mesh,
inside both and inside either, their ratio, and how many points were ambiguous (on the surface, or under a hole of an open
mesh).  It is sampled on the lattice: counts of points, not integrals over the solids.

--eval.vertex_colors=true (opt-in, shape task) colours the mesh from the input photo on the GPU (eval_3D.vertex_colors): a
vertex the input camera saw takes the photo's bilinear texel, every other vertex the colour of the nearest seen one.
<name>_mesh.obj then has `v x y z r g b` lines (the vertex-colour extension MeshLab, Blender and Open3D read), with --viz
<name>_mesh_viz.gif is rendered with those colours, and with --eval.mesh_report=true the report gains seen_area_fraction.
--eval.color_fade=<mesh units> fades copied colours towards the plain material colour with the distance from the seen
surface (0, the default: no fade), --eval.color_min_cos (0.1) is the smallest cosine between a vertex normal and the ray to the
camera that still counts as facing it, --eval.color_supersample (2) the z-buffer's resolution over the photo's.  Applied
after the component filter and the field normals.

--eval.mesh_reprojection=true (opt-in, shape task; needs no smoothing or simplification: it scores the prediction itself)
relates the mesh to the photo it was predicted from, without ground truth (eval_3D.reprojection, exact first hits of the input
camera's rays on the GPU): does the silhouette of the mesh cover the input mask, and does its first surface lie where the
predicted depth says the seen surface is?  <name>_mesh_depth.png is the depth map of the mesh in the input camera (written
like <name>_depth_est.png, over the pixels the mesh covers), and with --eval.mesh_report=true the report gains a
`reprojection` entry: the pixel counts and the silhouette IoU, max / mean / rms of |Z_mesh - depth| in camera units, mesh
units and marching-cubes cells with the pixel at the maximum, the pixels that agree within the colour pass's depth tolerance,
and the pixels whose first hit is a back face.  It is sampled at the pixel centres.

--eval.mesh_self_intersections=true (opt-in, shape task; needs no smoothing or simplification: it scores the delivered mesh
itself) finds the faces of the mesh that pass through each other (eval_3D.mesh_self_intersections, an exact face-against-face
test on the GPU; Open3D's is_self_intersecting).  With --eval.mesh_report=true the report gains a `self_intersections` entry:
crossing_pairs, faces_crossed, coincident_pairs (two faces on the same three corners: the one coplanar contact that is
counted, apart from the crossings) and skipped_faces - and, when --eval.smooth_iterations or --eval.simplify_cells ran, the
same four of the mesh before those steps under `before`: what they added.  Nothing is repaired.
"""
import importlib
import os
import shutil
import sys

import numpy as np
import torch
from PIL import Image

import zeroshape_amd.compat as compat

compat.install()
import utils.options as options                                              # noqa: E402
from utils.eval_3D import compute_level_grid, convert_to_explicit, get_dense_3D_grid   # noqa: E402
from utils.util import EasyDict as edict                                     # noqa: E402
from zeroshape_amd.utils import camera, eval_3D, util_vis                    # noqa: E402


def bbox_from_mask(mask, thr):
    on = (mask > thr).astype(np.float32)
    assert on.sum() > 0, "Empty mask!"
    cols, rows = np.flatnonzero(on.sum(axis=-2)), np.flatnonzero(on.sum(axis=-1))
    return cols[0], rows[0], cols[-1], rows[-1]


def preprocess_image(opt, image, bbox):
    """demo.py:38-58: square crop (PIL pads outside the frame with transparent black, like
    torchvision's crop of a PIL image), resize, composite on the background colour."""
    x1, y1, x2, y2 = bbox
    size = max(y2 - y1, x2 - x1) * 1.2
    yc, xc = (y1 + y2) / 2, (x1 + x2) / 2
    top, left, side = int(yc - size / 2), int(xc - size / 2), int(size)
    image = image.crop((left, top, left + side, top + side))
    if image.size[0] != opt.W or image.size[1] != opt.H:
        image = image.resize((opt.W, opt.H))
    arr = torch.from_numpy(np.asarray(image, np.float32) / 255.0).permute(2, 0, 1)
    rgb, mask = arr[:3], arr[3:]
    if opt.data.bgcolor is not None:
        rgb = rgb * mask + opt.data.bgcolor * (1 - mask)
        mask = (mask > 0.5).float()
    return rgb, mask


def get_image(opt, image_name, mask_name):
    image = Image.open(os.path.join(opt.datadir, 'images', image_name)).convert("RGB")
    mask = Image.open(os.path.join(opt.datadir, 'masks', mask_name)).convert("L")
    mask_np = (np.array(mask) > 127).astype(np.float32)                   # demo.py:61-63
    image = Image.merge("RGBA", (*image.split(), mask))
    return preprocess_image(opt, image, bbox_from_mask(mask_np, 0.5))


def prepare_data(opt):
    names = sorted(n for n in os.listdir(os.path.join(opt.datadir, 'images')) if n.endswith(('.png', '.jpg')))
    f = 1.3875
    K = torch.tensor([[f * opt.W, 0, opt.W / 2], [0, f * opt.H, opt.H / 2], [0, 0, 1]]).float()
    data = []
    for i, name in enumerate(names):
        rgb, mask = get_image(opt, name, name[:-4] + '.png')
        data.append(edict(rgb_input_map=rgb.unsqueeze(0).to(opt.device), mask_input_map=mask.unsqueeze(0).to(opt.device),
                          intr=K.unsqueeze(0).to(opt.device), idx=torch.tensor([i + 1]).to(opt.device).long()))
    return data, [n[:-4] for n in names]


@torch.no_grad()
def marching_cubes(opt, var, impl_network, vis_attn=False):
    points_3D = get_dense_3D_grid(opt, var)                                # [B,G,G,G,3] (tagged: fused grid query)
    level_vox, attn_vis = compute_level_grid(opt, impl_network, var.latent_depth, var.latent_semantic, points_3D,
                                             var.rgb_input_map, vis_attn)
    var.eval_vox = level_vox
    if attn_vis:
        var.attn_vis = attn_vis
    var.mesh_pred = convert_to_explicit(opt, list(level_vox), isoval=0.5, to_pointcloud=False)
    return var


def main():
    opt = options.set(opt_cmd=options.parse_arguments(sys.argv[1:]), safe_check=False)
    opt.device = "cuda:0"
    if os.path.basename(opt.yaml).split('.')[0] != opt.task:
        raise ValueError('Detected different tasks between specified and the yaml, please double check!')
    if opt.task == 'shape':
        opt.pretrain.depth = None
    opt.arch.depth.pretrained = None
    graph = importlib.import_module("model.compute_graph.graph_{}".format(opt.task)).Graph(opt).to(opt.device)
    checkpoint = torch.load(opt.ckpt, map_location="cpu")
    print("resuming from epoch {} (iteration {}, best_val {:.4f})".format(checkpoint["epoch"] + 1, checkpoint["iter"],
                                                                          checkpoint["best_val"]))
    graph.load_state_dict(checkpoint["graph"], strict=True)
    graph.eval()
    data_list, name_list = prepare_data(opt)
    save_folder = os.path.join(opt.datadir, 'preds')
    if os.path.isdir(save_folder):
        shutil.rmtree(save_folder)
    os.makedirs(save_folder)
    opt.output_path = opt.datadir
    viz = bool(opt.get("viz", False))
    field_normals = bool(opt.eval.get("field_normals", False))
    mesh_report = bool(opt.eval.get("mesh_report", False))
    colors = eval_3D.color_options(opt)
    reprojection = eval_3D.reprojection_option(opt)
    for var, name in zip(data_list, name_list):
        with torch.no_grad():
            var = graph.forward(opt, var, training=False, get_loss=False)
            util_vis.dump_images(opt, [name], "image_input", var.rgb_input_map, from_range=(0, 1), folder='preds')
            util_vis.dump_images(opt, [name], "mask_input", var.mask_input_map, folder='preds')
            util_vis.dump_depths(opt, [name], "depth_est", var.depth_pred, var.mask_input_map, rescale=True, folder='preds')
            if opt.task == 'shape':
                var = marching_cubes(opt, var, graph.impl_network, vis_attn=viz)
                if field_normals:      # --eval.field_normals=true: <name>_mesh.obj gets `vn` lines, -grad/|grad| of the field
                    eval_3D.field_normals(opt, graph.impl_network, var.latent_depth, var.latent_semantic, var.mesh_pred)
                if colors is not None:  # --eval.vertex_colors=true: `v x y z r g b` lines, a coloured turntable, the seen fraction
                    eval_3D.vertex_colors(opt, var, **colors)
                if reprojection:       # --eval.mesh_reprojection=true: <name>_mesh_depth.png, the report's `reprojection` entry
                    eval_3D.reprojection(opt, var)
                    depth = torch.stack([m.depth_map.depth for m in var.mesh_pred])[:, None]
                    util_vis.dump_depths(opt, [name], "mesh_depth", torch.nan_to_num(depth, nan=0.0, posinf=0.0),
                                         torch.isfinite(depth), rescale=True, folder='preds')
                util_vis.dump_meshes(opt, [name], "mesh", var.mesh_pred, folder='preds',
                                     normals="field" if field_normals else False, colors=colors is not None)
                if mesh_report:        # --eval.mesh_report=true: <name>_mesh_report.json, the totals and components of that mesh
                    util_vis.dump_mesh_reports(opt, [name], "mesh_report", var.mesh_pred, folder='preds')
                if viz:
                    util_vis.dump_attentions(opt, [name], "attn", var.attn_vis, folder='preds')
                    util_vis.dump_meshes_viz(opt, [name], "mesh_viz", var.mesh_pred, save_frames=False, folder='preds',
                                             colors=colors is not None)
            elif opt.task == 'depth':
                # demo.py:205-214 of the reference; the mask goes to the kernel in place of its `* mask + (1 - mask) * -1`
                B, _, H, W = var.depth_pred.shape
                for tag, intr in (("fixed", var.intr), ("pred", var.intr_pred if 'intr_pred' in var else None)):
                    if intr is None:
                        continue
                    seen = camera.unproj_depth(opt, var.depth_pred, intr).view(B, H, W, 3)
                    util_vis.dump_seen_surface(opt, [name], "seen_surface_" + tag, "image_input", seen, folder='preds',
                                               masks=var.mask_input_map)
        print("{}: done".format(name))


if __name__ == "__main__":
    main()
