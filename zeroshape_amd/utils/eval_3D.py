"""Mirror of the reference's utils/eval_3D.py for the hot path: same function names,
argument meaning and return values, running on the hand-written HIP kernels.

  get_dense_3D_grid   utils/eval_3D.py:11-20
  compute_level_grid  utils/eval_3D.py:22-81   (vis_attn branch: z-mean attention of the drawn grid columns + frame
                                               composer on the device, csrc/attn_vis.hip; the slice loop otherwise)
  standardize_pc      utils/eval_3D.py:83-91
  normalize_pc        utils/eval_3D.py:93-102
  brute_force_search  utils/eval_3D.py:140-170
  compute_fscore      utils/eval_3D.py:215-231
  chamfer_distance    utils/eval_3D.py:265-269
  ICP                 utils/eval_3D.py:271-284
  eval_metrics(_default|_BF)  utils/eval_3D.py:104-138,172-213
  convert_to_explicit utils/eval_3D.py:233-263  (GPU marching cubes + sampling)

torch is used here for device memory, streams and orchestration; every numeric step -
the decoder over the dense grid, the nearest-neighbour searches, normalisation, F-score,
ICP, iso-surface extraction - is a HIP kernel behind the C ABI and raises if
libzeroshape_hip.so is missing (no fallback).

``convert_to_explicit`` (utils/eval_3D.py:233-263: PyMCubes + trimesh on the host in the
reference) runs on the GPU here: csrc/marching_cubes.hip.  The meshes it returns keep
their triangles in HBM; the indexed form and the vertex normals come from csrc/mesh_weld.hip (``weld_mesh``) when read.
"""

import collections

import numpy as np
import os

import torch

from ..external.chamfer3D.dist_chamfer_3D import chamfer_3DDist
from .camera import get_rotation_sphere
from .util_vis import BASE_RGB


class _GridInfo(object):
    """Metadata attached to tensors made by get_dense_3D_grid so that
    compute_level_grid can use the fused grid kernel (coordinates generated in the
    kernel from the linspace axis) instead of re-reading the points tensor."""
    __slots__ = ("axis", "G", "version")

    def __init__(self, axis, G, version):
        self.axis, self.G, self.version = axis, G, version   # version: the tensor's in-place counter at tagging


@torch.no_grad()
def get_dense_3D_grid(opt, var, N=None):
    """utils/eval_3D.py:11-20: [B, N+1, N+1, N+1, 3] fp32, x slowest, z fastest."""
    batch_size = len(var.idx)
    N = N or opt.eval.vox_res
    range_min, range_max = opt.eval.range
    grid = torch.linspace(range_min, range_max, N + 1, device=opt.device)
    points_3D = torch.stack(torch.meshgrid(grid, grid, grid, indexing='ij'), dim=-1)
    points_3D = points_3D.repeat(batch_size, 1, 1, 1, 1)
    points_3D._zs_grid = _GridInfo(grid, N + 1, points_3D._version)
    return points_3D


def image_sharding(opt):
    """(rank, world) of the per-image sharding of SURVEY.md section 8e - the grid's point ranges and the pose
    search's rotations split over the ranks of ONE image - or None: on when ``opt.eval.shard_image`` is set (the
    engine resolves its "auto" default: more ranks than test images, model/shape_engine.py) and a process group of more
    than one rank exists."""
    from .. import parallel
    try:
        on = bool(opt.eval.shard_image)
    except (AttributeError, KeyError):
        on = False
    rank, world = parallel.world()
    return (rank, world) if on and world > 1 else None


@torch.no_grad()
def compute_level_grid(opt, impl_network, latent_depth, latent_semantic, points_3D, images,
                       vis_attn=False):
    """utils/eval_3D.py:22-81.  Returns (occ [B,G,G,G] in (0,1), images_vis | None).

    Fast path: ``impl_network`` is the HIP decoder and ``points_3D`` came from
    get_dense_3D_grid -> one fused launch per image batch over the whole grid
    (no per-slice loop, no points tensor read, no attention materialisation).
    With ``vis_attn`` the same occupancies, plus the heat-map frames from the attention of the grid columns
    they draw (query_grid_attention: 1.7 % of the points at vox 128, reduced to the z-mean on the device) and
    one composer launch (attention_frames); one device-to-host copy of all frames.
    Otherwise (also with image sharding and vis_attn): the reference's slice loop through ``impl_network(...)``."""
    latent_depth = latent_depth.to(torch.float32) if latent_depth is not None else None
    latent_semantic = latent_semantic.to(torch.float32) if latent_semantic is not None else None
    batch_size = points_3D.shape[0]
    N = points_3D.shape[1]
    assert N == points_3D.shape[2] == points_3D.shape[3]
    assert points_3D.shape[4] == 3

    info = getattr(points_3D, "_zs_grid", None)
    if info is not None and (info.version != points_3D._version or info.G != N):
        info = None            # modified in place since get_dense_3D_grid made it: read the points
    fast = info is not None and hasattr(impl_network, "query_grid") and getattr(impl_network, "fused", True) \
        and latent_semantic is None
    if fast and vis_attn and image_sharding(opt) is None:
        columns, frame_col = attention_frame_columns(N)
        state = impl_network.prepare(latent_depth)
        occ = impl_network.query_grid(latent_depth, info.axis, apply_sigmoid=True, state=state)
        zmean = impl_network.query_grid_attention(latent_depth, info.axis, columns, state=state)
        frames = attention_frames(opt, zmean, frame_col, images).cpu().numpy()       # the one device-to-host copy
        return occ, [[frames[b, f] for f in range(frames.shape[1])] for b in range(batch_size)]
    if fast and not vis_attn:
        if image_sharding(opt) is not None:
            # every rank holds the same images (and ran the same prologue); rank r evaluates its tile-aligned
            # point range of every image and ONE all_gather_into_tensor rebuilds the grids everywhere
            from .. import parallel
            state = parallel.prepare_sharded(impl_network, latent_depth)      # image i's output check on rank i % world
            occ = parallel.sharded_level_grid_points(
                lambda b, e: impl_network.query_grid_range(latent_depth, info.axis, b, e, apply_sigmoid=True,
                                                           state=state), N)
            return occ, None
        occ = impl_network.query_grid(latent_depth, info.axis, apply_sigmoid=True)
        return occ, None

    pts = points_3D.view(batch_size, N, N * N, 3)
    occ, attn = [], []
    hip_net = hasattr(impl_network, "query_grid")
    for i in range(N):
        if hip_net:   # our decoder: skip the attention dump unless it is going to be drawn
            occ_slice, attn_slice = impl_network(latent_depth, latent_semantic, pts[:, i], need_attn=vis_attn)
        else:
            occ_slice, attn_slice = impl_network(latent_depth, latent_semantic, pts[:, i])
        occ.append(occ_slice)
        if vis_attn:
            attn.append(attn_slice.detach())
    occ = torch.stack(occ, dim=1).view(batch_size, N, N, N)
    occ = torch.sigmoid(occ)
    images_vis = None
    if vis_attn:
        images_vis = _attention_frames(opt, attn, images, batch_size, N)
    return occ, images_vis


def _jet_lut():
    """The 256-entry 'jet' colour table (RGB, uint8) from its closed form - r, g, b = clamp(1.5 - |4x - 3|, |4x - 2|, |4x - 1|)
    at x = i / 255 - the map cv2.COLORMAP_JET tabulates (utils/util_vis.py:285; cv2 is not a dependency of this package,
    and its table may differ from the closed form by one grey level)."""
    x = np.arange(256, dtype=np.float64) / 255.0
    chan = lambda c: np.clip(1.5 - np.abs(4.0 * x - c), 0.0, 1.0)      # noqa: E731
    return np.uint8(np.round(255.0 * np.stack([chan(3.0), chan(2.0), chan(1.0)], -1)))


def show_att_on_image(img, mask):
    """utils/util_vis.py:267-293: the attention map [H, W] in [0, 1] as a jet heat map added onto the image [H, W, 3] in
    [0, 1], rescaled to a maximum of 1.  numpy only (round 5: the product path no longer reaches for the reference's module)."""
    assert np.max(img) <= 1 and np.max(mask) <= 1
    heatmap = np.float32(_jet_lut()[np.uint8(255 * mask)]) / 255
    merged = heatmap + np.float32(img)
    return merged / np.max(merged)


def attention_frame_columns(G):
    """The frames of utils/eval_3D.py:62-79 as host-side index lists: ``columns`` int32 [n_cols, 2] = the distinct grid
    columns (ix, iy) the loop draws, in ascending order, and ``frame_col`` int32 [F] = the column of every frame in the
    loop's order - rows (iy) 0, 8, ..., columns (ix) 0, 8, ..., G // 8 * 8 ascending on rows that are multiples of 16 and
    descending on the others.  A G that is a multiple of 8 makes the loop index column G: IndexError, here too."""
    last = G // 8 * 8
    if last >= G:
        raise IndexError("index %d is out of bounds for dimension 1 with size %d" % (last, G))
    frames = []
    for row in range(0, G, 8):
        cols = range(0, last + 1, 8) if row % 16 == 0 else range(last, -1, -8)
        frames += [(col, row) for col in cols]
    distinct = sorted(set(frames))
    where = {c: i for i, c in enumerate(distinct)}
    return (np.asarray(distinct, np.int32).reshape(-1, 2), np.asarray([where[c] for c in frames], np.int32))


_JET_LUT_DEV = {}


@torch.no_grad()
def attention_frames(opt, zmean, frame_col, images):
    """utils/eval_3D.py:62-79 + show_att_on_image for every frame in ONE launch (zs_attn_frames, csrc/attn_vis.hip):
    ``zmean`` [B, n_cols, 1 + R*R] (Implicit.query_grid_attention), ``frame_col`` [F] indices into n_cols, ``images``
    [B, 3, H, W] in [0, 1] -> GPU tensor [B, F, H, W, 3] fp32.  show_att_on_image's assertion on the image is kept (one
    check per call; the mask is v / max v <= 1 by construction)."""
    from .. import _lib
    lib = _lib.load()
    dev = zmean.device
    H, W = int(opt.H), int(opt.W)
    R = H // opt.arch.win_size
    B, n_cols = zmean.shape[0], zmean.shape[1]
    zmean = _gpu_f32(zmean, "zmean")
    images = _gpu_f32(images, "images")
    if zmean.shape[2] != 1 + R * R:
        raise ValueError("zmean must be [B, n_cols, %d] for %d x %d patches, got %s" % (1 + R * R, R, R, tuple(zmean.shape)))
    if tuple(images.shape) != (B, 3, H, W):
        raise ValueError("images must be [%d, 3, %d, %d], got %s" % (B, H, W, tuple(images.shape)))
    fc = np.ascontiguousarray(np.asarray(frame_col, np.int32).reshape(-1))
    if fc.size and (fc.min() < 0 or fc.max() >= n_cols):
        raise IndexError("frame column outside [0, %d)" % n_cols)
    assert B == 0 or float(images.max()) <= 1
    key = str(dev)
    if key not in _JET_LUT_DEV:
        _JET_LUT_DEV[key] = torch.from_numpy(_jet_lut()).to(dev).contiguous()
    frames = torch.empty(B, fc.size, H, W, 3, dtype=torch.float32, device=dev)
    fc_dev = torch.from_numpy(fc).to(dev)
    with torch.cuda.device(dev):
        rc = lib.zs_attn_frames(_lib.ptr(zmean), B, n_cols, _lib.ptr(fc_dev), fc.size, _lib.ptr(images), H, W,
                                _lib.ptr(_JET_LUT_DEV[key]), R, _lib.ptr(frames), _lib.current_stream_ptr(dev))
    _lib.check(rc, "zs_attn_frames")
    return frames


def _attention_frames(opt, attn, images, batch_size, N):
    """utils/eval_3D.py:47-80: host-side heat-map frames of the slice loop (the fused path: attention_frames)."""
    N_global = 1
    feat_res = opt.H // opt.arch.win_size
    attn = torch.stack(attn, dim=1).view(batch_size, N, N, N, N_global + feat_res ** 2)
    attn = torch.mean(attn, dim=3)
    attn_global = attn[:, :, :, :N_global].sum(dim=-1, keepdim=True)
    attn_local = attn[:, :, :, N_global:].view(batch_size, N, N, feat_res, feat_res)
    attn_vis = attn_global.unsqueeze(-1) + attn_local
    images_vis = []
    for b in range(batch_size):
        frames = []
        for row in range(0, N, 8):
            col_range = range(0, N // 8 * 8 + 1, 8) if row % 16 == 0 else range(N // 8 * 8, -1, -8)
            for col in col_range:
                a = attn_vis[b, col, row]
                a = torch.nn.functional.interpolate(a[None, None], size=(opt.H, opt.W), mode='bilinear',
                                                    align_corners=False)[0, 0].cpu().numpy()
                a /= a.max()
                frames.append(show_att_on_image(images[b].permute(1, 2, 0).cpu().numpy(), a))
        images_vis.append(frames)
    return images_vis


def _gpu_f32(t, what):
    if not t.is_cuda:
        raise ValueError("%s must be a GPU tensor; zeroshape_amd has no CPU path" % what)
    return t.detach().to(torch.float32).contiguous()


@torch.no_grad()
def standardize_pc(pc):
    """utils/eval_3D.py:83-91: zs_standardize_pc."""
    from .. import _lib
    assert len(pc.shape) == 3 and pc.shape[2] == 3
    lib = _lib.load()
    x = _gpu_f32(pc, "pc")
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = lib.zs_standardize_pc(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(out), _lib.current_stream_ptr(x.device))
    _lib.check(rc, "zs_standardize_pc")
    return out


@torch.no_grad()
def normalize_pc(pc):
    """utils/eval_3D.py:93-102 (z extent ignored, like the reference): zs_normalize_pc."""
    from .. import _lib
    assert len(pc.shape) == 3 and pc.shape[2] == 3
    lib = _lib.load()
    x = _gpu_f32(pc, "pc")
    B, n = x.shape[0], x.shape[1]
    out = torch.empty_like(x)
    scratch = torch.empty(16 * max(B, 1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.zs_normalize_pc(_lib.ptr(x), B, n, _lib.ptr(out), _lib.ptr(scratch), _lib.current_stream_ptr(x.device))
    _lib.check(rc, "zs_normalize_pc")
    return out


_THRESHOLDS = {}


def _threshold_tensor(thresholds, device, pad_to=None):
    key = (tuple(float(t) for t in thresholds), str(device), pad_to)
    if key not in _THRESHOLDS:
        vals = list(key[0]) + [0.0] * max(0, (pad_to or 0) - len(key[0]))   # d < 0 never holds: padded entries score 0
        _THRESHOLDS[key] = torch.tensor(vals, dtype=torch.float32, device=device)
    return _THRESHOLDS[key]


@torch.no_grad()
def compute_fscore(dist1, dist2, thresholds=[0.005, 0.01, 0.02, 0.05, 0.1, 0.2]):
    """utils/eval_3D.py:215-231 on un-squared distances [B,n], [B,m] -> [B, len(thresholds)]: zs_fscore."""
    from .. import _lib
    lib = _lib.load()
    d1, d2 = _gpu_f32(dist1, "dist1"), _gpu_f32(dist2, "dist2")
    B = d1.shape[0]
    thr = _threshold_tensor(thresholds, d1.device)
    out = torch.empty(B, len(thresholds), dtype=torch.float32, device=d1.device)
    with torch.cuda.device(d1.device):
        rc = lib.zs_fscore(_lib.ptr(d1), d1.shape[1], _lib.ptr(d2), d2.shape[1], B, _lib.ptr(thr), len(thresholds),
                           _lib.ptr(out), _lib.current_stream_ptr(d1.device))
    _lib.check(rc, "zs_fscore")
    return out


_CHAMFER = chamfer_3DDist()  # stateless; the reference builds a new module per call (:267)


def chamfer_distance(opt, X1, X2, method="auto"):
    """utils/eval_3D.py:265-269: un-squared NN distances both ways + int32 indices.
    ``method`` picks the kernel ("auto" | "grid" | "brute"); outputs are bit-identical."""
    assert X1.shape[2] == 3
    dist_1, dist_2, idx_1, idx_2 = _CHAMFER(X1, X2, method)
    return dist_1.sqrt(), dist_2.sqrt(), idx_1, idx_2


def _bf_lower_bounds(pc_pred, pc_gt_n, rotations):
    """zs_bf_lower_bounds: per-rotation lower bounds of the Chamfer-L1 (csrc/bf_prune.hip)."""
    from .. import _lib
    lib = _lib.load()
    dev = pc_pred.device
    pred = pc_pred.reshape(-1, 3).contiguous()
    gt = pc_gt_n.reshape(-1, 3).contiguous()
    R = rotations.to(dev).float().contiguous()
    gw = lib.zs_bf_grid_bytes() // 4
    grids = torch.empty(2 * gw, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.zs_bf_scratch_bytes() // 4, dtype=torch.int32, device=dev)
    lb = torch.empty(R.shape[0], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.zs_bf_lower_bounds(_lib.ptr(pred), pred.shape[0], _lib.ptr(gt), gt.shape[0], _lib.ptr(R),
                                    R.shape[0], _lib.ptr(grids), _lib.ptr(grids[gw:]), _lib.ptr(scratch),
                                    _lib.ptr(lb), _lib.current_stream_ptr(dev))
    _lib.check(rc, "zs_bf_lower_bounds")
    return lb


_POSE_MODES = {"brute": 0, "pairs": 1, "cull": 2}     # zs_pose_search_batch_sorted: mode


def _spatially_sorted(points):
    """points [n,3] (GPU, fp32) -> the same points in an order whose runs of 64 are compact boxes (sort-tile-recursive,
    zs_str_sort)."""
    from .. import _lib
    lib = _lib.load()
    pts = points.contiguous()
    n = pts.shape[0]
    out = torch.empty_like(pts)
    st = _lib.current_stream_ptr(pts.device)
    with torch.cuda.device(pts.device):
        scratch = torch.empty(max(1, lib.zs_str_scratch_bytes(n) // 4), dtype=torch.float32, device=pts.device)
        rc = lib.zs_str_sort(_lib.ptr(pts), n, _lib.ptr(out), None, _lib.ptr(scratch), st)
    _lib.check(rc, "zs_str_sort")
    return out


_ROTATIONS = {}


def _rotation_sphere(device):
    key = str(torch.device(device))
    if key not in _ROTATIONS:       # 6912 x 3 x 3, built once per device (the reference rebuilds it per call, :148)
        _ROTATIONS[key] = get_rotation_sphere(azim_sample=24, elev_sample=24, roll_sample=12, scales=[1.0],
                                              device=device).float().contiguous()
    return _ROTATIONS[key]


@torch.no_grad()
def brute_force_search(pc_pred, pc_gt, f_thresholds=[0.005, 0.01, 0.02, 0.05, 0.1, 0.2], device="cuda",
                       rotations=None, rot_slice=None, return_index=False, batch_size=256, prune=True, nn=None,
                       first_batch=None, rot_shard=None, group=None, peek=None):
    """utils/eval_3D.py:140-170: best rigid alignment over the 6912-rotation sphere by
    Chamfer-L1, with the reference's first-strict-minimum rule (:161-168).

    Same result as the exhaustive scan, less work: every rotation first gets a rigorous lower
    bound of its Chamfer-L1 (``prune``; csrc/bf_prune.hip); rotations are then evaluated exactly
    in order of increasing bound, ``batch_size`` at a time (the reference: 24 in index order,
    :149), by the fused kernels of csrc/pose_search.hip - rotate, normalize_pc, nearest
    neighbours both ways, sqrt / means / F-score, running (cd, rotation index) minimum, all on
    the device - and a batch whose smallest bound already exceeds the best exact distance returns
    at once.  No rotated clouds, no PyTorch or BLAS launch inside the search; the batches are enqueued without waiting
    for each other, except that after the 2nd and the 4th one (``peek``, default on; ZS_POSE_PEEK=0: never) the host reads the
    running best (one 64-byte copy) and STOPS enqueuing when the next batch's smallest bound already fails the kernels' own
    test - an alignable ground truth finds its winner in the first batch or two, and the 27 batches behind it were 240
    launches that returned at once: 1.1 ms of a 2.8 ms search.  Same record, bit for bit: the bounds ascend and the best only
    falls, so every batch the host skips is one the device would have skipped.  The winner is the lexicographic minimum of
    (cd, rotation index) over the evaluated rotations; pruned ones are strictly worse, so this IS
    the first strict minimum of the full scan.
    ``nn`` picks the nearest-neighbour kernels of the exact evaluations: "cull" (None: the default), "pairs" or "brute";
    anything else raises ValueError.  Both clouds are first put into a spatial order (sort-tile-recursive, zs_str_sort;
    once per search), so that 64 consecutive points fill a compact box - also after the rotation; the statistics of
    normalize_pc and the returned clouds keep the caller's order.  "cull" reads candidates 64 at a time through the
    scalar cache and skips every block whose bounding box is farther from a query than its current nearest neighbour,
    nearest tiles first; "pairs" is the same kernel without the skipping, "brute" an LDS-staged scan of every pair of the
    same sorted clouds - the two references the tests prove "cull" against.  The records are bit-identical
    (tests/test_gpu_chamfer.py): every query ends with the same minimum and the sums keep their fixed order.
    ``rot_slice=(start, stop)`` restricts the scan to a contiguous index range; ``return_index`` appends the
    winning global rotation index and its cd (one host read of the 64-byte record).
    ``rot_shard=(rank, world)`` is the multi-GPU form (every rank of ``group`` calls with the
    same clouds): every rank bounds and sorts the whole sphere (1 ms, identical on all of them), rank r takes
    positions r, r + W, ... of that order - equal shares of promising and hopeless rotations - and after its first
    batch the ranks exchange their best distance (ONE 4-byte all-reduce MIN on the stream, no host read) so every
    later batch is pruned against the GLOBAL best; at the end the 64-byte records are all-gathered and the
    lexicographic (cd, index) minimum taken on the device - the same record, bit for bit, as the single-rank scan
    (a rotation's record does not depend on the batch it was evaluated in)."""
    from .. import _lib
    nn = "cull" if nn is None else nn
    if nn not in _POSE_MODES:
        raise ValueError("nn must be 'cull', 'pairs' or 'brute', got %r" % (nn,))
    lib = _lib.load()
    if len(f_thresholds) > 6:
        raise ValueError("the fused pose search carries six F-score thresholds (options/shape.yaml:54)")
    dev = torch.device(device)
    pred = pc_pred.to(dev).float().contiguous()
    pc_gt = normalize_pc(pc_gt.to(dev).unsqueeze(0).float().contiguous())
    rotations = _rotation_sphere(dev) if rotations is None else rotations.to(dev).float().contiguous()
    start, stop = (0, len(rotations)) if rot_slice is None else rot_slice
    if stop <= start:
        raise ValueError("empty rotation range")
    batch_size = min(int(batch_size), lib.zs_pose_max_batch())      # (256: the kernels address a batch by thread)
    first_batch = min(batch_size, 32) if first_batch is None else max(1, min(int(first_batch), batch_size))
    K = stop - start
    n, m = pred.shape[0], pc_gt.shape[1]
    order = lb_sorted = None
    if prune and (K > batch_size or rot_shard is not None):
        lb = _bf_lower_bounds(pred, pc_gt[0], rotations[start:stop])
        lb_sorted, order = torch.sort(lb, stable=True)
        order = order.to(torch.int32)
    if rot_shard is not None:
        srank, sworld = rot_shard
        if order is None:
            order = torch.arange(K, dtype=torch.int32, device=dev)
        # The shares only partition the sphere - and the shared running best only prunes validly - if every rank holds
        # bit-identical clouds (per-rank random weights, or a dataset that samples points per process, would
        # silently return a wrong winner).  One 16-byte MIN/MAX all-reduce of a checksum per call; a mismatch raises.
        _check_identical_inputs(pred, pc_gt, order, group)
        order = order[srank::sworld].contiguous()
        lb_sorted = lb_sorted[srank::sworld].contiguous() if lb_sorted is not None else None
        K = int(order.numel())
    thr = _threshold_tensor(f_thresholds, dev, pad_to=6)
    best = torch.empty(lib.zs_pose_best_bytes() // 4, dtype=torch.float32, device=dev)
    pred_s, gt_s = _spatially_sorted(pred), _spatially_sorted(pc_gt[0])
    gt_pack = torch.empty(lib.zs_pose_pack_bytes(m) // 4, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.zs_pose_sorted_scratch_bytes(n, m, max(1, min(batch_size, K))) // 4, dtype=torch.float32,
                          device=dev)
    st = _lib.current_stream_ptr(dev)
    rot_base = rotations.data_ptr() + 36 * start

    def launch(rot_ptr, order_ptr, count, offset, lb_ptr):
        return lib.zs_pose_search_batch_sorted(_lib.ptr(pred), _lib.ptr(pred_s), n, _lib.ptr(gt_s), _lib.ptr(gt_pack), m,
                                               rot_ptr, order_ptr, count, offset, lb_ptr, _lib.ptr(thr), _lib.ptr(best),
                                               _lib.ptr(scratch), _POSE_MODES[nn], st)

    with torch.cuda.device(dev):
        _lib.check(lib.zs_pose_best_init(_lib.ptr(best), st), "zs_pose_best_init")
        _lib.check(lib.zs_pose_pack(_lib.ptr(gt_s), m, _lib.ptr(gt_pack), st), "zs_pose_pack")
        # a small first batch: its winner lets the staged drop (csrc/pose_search.hip) thin out every later batch
        starts, pos = [], 0
        while pos < K:
            starts.append((pos, min(first_batch if pos == 0 else batch_size, K - pos)))
            pos += starts[-1][1]
        # kept (argument and ZS_POSE_PEEK): the only way to run the plain host loop, which enqueues every batch and never
        # reads the record mid-search - what a caller that must not synchronise wants, and the A/B of the peek itself
        peek = (os.environ.get("ZS_POSE_PEEK", "1") != "0") if peek is None else bool(peek)
        lb_host = None
        for bi, (pos, count) in enumerate(starts):
            if peek and lb_sorted is not None and bi in (2, 4) and not torch.cuda.is_current_stream_capturing():
                # the kernels' batch_pruned() (csrc/pose_search.hip:75-77) on the host, in the same fp32 arithmetic
                if lb_host is None:
                    lb_host = lb_sorted.cpu().numpy()
                rec = best.cpu().numpy()
                bound = min(np.float32(rec[0]), np.float32(rec[12]))
                if np.float32(np.float32(lb_host[pos]) * np.float32(1.0 - 1e-3)) - np.float32(1e-6) > bound:
                    break
            if order is not None:      # rotation b of the batch = rotations[start + order[pos + b]]
                rc = launch(rot_base, order.data_ptr() + 4 * pos, count, start,
                            lb_sorted.data_ptr() + 4 * pos if lb_sorted is not None else None)
            else:                      # index order
                rc = launch(rot_base + 36 * pos, None, count, start + pos, None)
            _lib.check(rc, "zs_pose_search_batch_sorted")
            if rot_shard is not None and bi == 0:
                _share_running_best(best, group)
        if rot_shard is not None:
            if K == 0:                 # more ranks than rotations: this rank reports the neutral record
                _share_running_best(best, group)
            best = _reduce_best_records(best, group)
        ibest = best.view(torch.int32)
        best_pred = torch.empty(n, 3, dtype=torch.float32, device=dev)
        rc = lib.zs_pose_apply(_lib.ptr(pred), n, _lib.ptr(rotations), ibest.data_ptr() + 4, _lib.ptr(best_pred),
                               _lib.ptr(scratch), st)
        _lib.check(rc, "zs_pose_apply")
    out = (best[2].clone(), best[3].clone(), best[4:4 + len(f_thresholds)].clone(), best_pred, pc_gt)
    brute_force_search.last_evaluated = brute_force_search.last_scanned = None
    if return_index:
        rec = best.cpu()
        irec = rec.view(torch.int32)
        brute_force_search.last_evaluated = int(irec[10])        # diagnostics: rotations the lower bounds let through
        brute_force_search.last_scanned = int(irec[11])          # ... of which scanned in full (not killed by the probe)
        out = out + (int(irec[1]), float(rec[0]))
    return out


def _check_identical_inputs(pred, gt, order, group=None):
    """Raise unless every rank of `group` passed the same prediction / ground-truth clouds and derived the same rotation order
    (bit patterns summed as int64: order-independent per tensor, but any differing element changes it)."""
    import torch.distributed as dist
    sums = torch.stack([pred.contiguous().view(torch.int32).to(torch.int64).sum(),
                        gt.contiguous().view(torch.int32).to(torch.int64).sum(),
                        (order.to(torch.int64) * torch.arange(1, order.numel() + 1, device=order.device)).sum()])
    lo, hi = sums.clone(), sums.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
    if not bool((lo == hi).all()):
        raise RuntimeError("brute_force_search(rot_shard=...): the ranks hold different prediction / ground-truth clouds "
                           "(checksums %s vs %s); sharding the rotation sphere needs identical inputs on every rank "
                           "(same weights, same sample)" % (lo.tolist(), hi.tolist()))


def _share_running_best(best, group=None):
    """best[12] <- min over the ranks of best[0] (csrc/pose_search.hip: prune_bound).  Stream-ordered, no host read."""
    import torch.distributed as dist
    bound = best[0:1].clone()
    dist.all_reduce(bound, op=dist.ReduceOp.MIN, group=group)
    best[12:13].copy_(bound)


def _reduce_best_records(best, group=None):
    """The ranks' 64-byte records all-gathered; returns the record of the lexicographic (cd, rotation index) minimum
    - the first strict minimum of the sequential scan (utils/eval_3D.py:161-168) - with the evaluated / scanned
    counters summed over the ranks.  Device-side throughout."""
    from .. import parallel
    return parallel.reduce_best_records(best, group)


def _surface_clouds(opt, level_vox, seed=0):
    """level grids [B,G,G,G] (GPU tensor) -> (meshes, dpc_pred [B,num_points,3] fp32 on the
    device): convert_to_explicit without the device->host->device round trip of the
    reference (utils/eval_3D.py:115-118,181-184)."""
    meshes, clouds = [], []
    range_min, range_max = opt.eval.range
    cleaning, smoothing, simplifying = _component_options(opt), _smooth_options(opt), _simplify_options(opt)
    deviation_cell = _deviation_option(opt, smoothing, simplifying)
    iou_lattice = _iou_option(opt, smoothing, simplifying, G=level_vox.shape[1])
    selfx = self_intersections_option(opt)
    for i in range(level_vox.shape[0]):
        if cleaning is None and smoothing is None and simplifying is None:
            tris, pts = extract_surface(level_vox[i], 0.5, range_min, range_max, opt.eval.num_points, seed + i)
            mesh = SimpleMesh(tris)                      # stays in HBM until a dump reads it
            if selfx:                      # eval.mesh_self_intersections: the report's entry
                _with_self_intersections(mesh)
        else:                              # eval.min_component_area / eval.drop_cavities, eval.smooth_*, eval.simplify_cells:
            tris, _ = extract_surface(level_vox[i], 0.5, range_min, range_max)          # sample the mesh that is delivered
            mesh = _cleaned_and_smoothed(SimpleMesh(tris), cleaning, smoothing, simplifying, deviation_cell, iou_lattice, selfx)
            pts = sample_surface(mesh.device_triangles, opt.eval.num_points, seed + i)
        meshes.append(mesh)
        clouds.append(pts)
    return meshes, torch.stack(clouds, dim=0)


def _component_options(opt):
    """(min_component_area, drop_cavities) when either opt-in is set (``--eval.min_component_area=0.05``,
    ``--eval.drop_cavities=true``: no yaml file carries them), else None: the pipelines then make today's calls."""
    min_area = opt.eval.get("min_component_area", None)
    drop = bool(opt.eval.get("drop_cavities", False))
    if min_area is None and not drop:
        return None
    return (None if min_area is None else float(min_area)), drop


SMOOTH_OPTIONS = ("smooth_iterations", "smooth_lambda", "smooth_mu", "smooth_free_boundary")


def _smooth_options(opt):
    """(iterations, lamb, mu, pin_boundary) for smooth_mesh when ``--eval.smooth_iterations=N`` is set (opt-in, command line
    only: no yaml file carries it), else None: the pipelines then make today's calls.  ``--eval.smooth_lambda`` and
    ``--eval.smooth_mu`` replace smooth_mesh's defaults (``--eval.smooth_mu=none``: plain Laplacian passes) and
    ``--eval.smooth_free_boundary=true`` lets the vertices of open edges move; any of them without the pass count is an
    error, not ignored."""
    iterations = opt.eval.get("smooth_iterations", None)
    if iterations is None:
        extra = [k for k in SMOOTH_OPTIONS[1:] if k in opt.eval]
        if extra:
            raise ValueError("eval.%s needs eval.smooth_iterations" % extra[0])
        return None
    mu = opt.eval.get("smooth_mu", -0.53)
    if isinstance(mu, str):
        if mu.strip().lower() != "none":
            raise ValueError("eval.smooth_mu must be a number in [-1, 0) or none, got %r" % (mu,))
        mu = None
    args = (iterations, opt.eval.get("smooth_lambda", 0.5), mu, not bool(opt.eval.get("smooth_free_boundary", False)))
    _check_smooth_arguments(*args[:3])
    return args


SIMPLIFY_OPTIONS = ("simplify_cells", "simplify_position")


def _mc_cell_edge(opt):
    """A cell of the evaluation grid in mesh units, as default_color_depth_tol counts it."""
    range_min, range_max = opt.eval.range
    return (float(range_max) - float(range_min)) / float(opt.eval.vox_res)


def _simplify_options(opt):
    """(cell, origin, position) for simplify_mesh when ``--eval.simplify_cells=2.0`` is set (opt-in, command line only: no yaml
    file carries it), else None: the pipelines then make today's calls.  The value is the cluster edge in marching-cubes cells
    (_mc_cell_edge: the unit of default_color_depth_tol); the cluster planes sit half such a cell below ``eval.range``'s
    minimum, so that with an integer setting the lattice coordinates of the marching-cubes vertices do not lie on them.
    ``--eval.simplify_position=mean`` takes the cluster means instead of the quadric minimisers; without the cell count it is
    an error, not ignored."""
    cells = opt.eval.get("simplify_cells", None)
    if cells is None:
        if "simplify_position" in opt.eval:
            raise ValueError("eval.simplify_position needs eval.simplify_cells")
        return None
    if isinstance(cells, bool) or not isinstance(cells, (int, float, np.integer, np.floating)) or not (0.0 < float(cells) < np.inf):
        raise ValueError("eval.simplify_cells must be a finite number > 0, got %r" % (cells,))
    position = opt.eval.get("simplify_position", "quadric")
    edge = _mc_cell_edge(opt)
    cell = float(cells) * edge
    _check_simplify_arguments(cell, position)
    return cell, (float(opt.eval.range[0]) - 0.5 * edge,) * 3, position


def _deviation_option(opt, smoothing, simplifying):
    """The marching-cubes cell edge when ``--eval.mesh_deviation=true`` is set (opt-in, command line only: no yaml file carries
    it), else None: the pipelines then make today's calls.  The record compares the delivered mesh with the mesh it was made
    from, so without ``eval.smooth_iterations`` and ``eval.simplify_cells`` there is nothing to compare: an error, not ignored."""
    if not bool(opt.eval.get("mesh_deviation", False)):
        return None
    if smoothing is None and simplifying is None:
        raise ValueError("eval.mesh_deviation needs eval.smooth_iterations or eval.simplify_cells")
    return _mc_cell_edge(opt)


def _iou_option(opt, smoothing, simplifying, G=None):
    """The marching-cubes lattice (G, scale, offset) of the evaluation grid when ``--eval.mesh_iou=true`` is set (opt-in, command
    line only: no yaml file carries it), else None: the pipelines then make today's calls.  ``G`` samples per axis - the level
    grid's own size where the caller has one, else ``eval.vox_res`` + 1 as get_dense_3D_grid makes it - at
    scale = (range_max - range_min) / G as extract_surface computes it and offset = range_min.  The record compares the
    delivered mesh with the mesh it was made from, so without ``eval.smooth_iterations`` and ``eval.simplify_cells`` there is
    nothing to compare: an error, not ignored."""
    if not bool(opt.eval.get("mesh_iou", False)):
        return None
    if smoothing is None and simplifying is None:
        raise ValueError("eval.mesh_iou needs eval.smooth_iterations or eval.simplify_cells")
    range_min, range_max = opt.eval.range
    G = int(opt.eval.vox_res) + 1 if G is None else int(G)
    return G, float(np.float32((range_max - range_min) / G)), float(range_min)


def _cleaned_and_smoothed(mesh, cleaning, smoothing, simplifying=None, deviation_cell=None, iou_lattice=None, selfx=False):
    """The opt-in steps between marching cubes and sampling, in their order: filter_components, then smooth_mesh, then
    simplify_mesh - last, so that the colours, the sampled points and with them the metrics describe the mesh that is
    delivered.  With ``deviation_cell`` (_deviation_option) the delivered mesh gets ``deviation``: mesh_deviation against the
    mesh as it stood after filter_components - dropping floaters is intended and is not deviation.  With ``iou_lattice``
    (_iou_option) it gets ``volume_iou``: mesh_volume_iou against the same mesh on that lattice.  With ``selfx``
    (self_intersections_option) it gets its ``self_intersections`` and, when a smoothing or simplification step ran,
    ``self_intersections_before``: the record of that same mesh (_with_self_intersections)."""
    if cleaning is not None:
        mesh = filter_components(mesh, *cleaning)
    reference = mesh
    if smoothing is not None:
        mesh = smooth_mesh(mesh, *smoothing)
    if simplifying is not None:
        mesh = simplify_mesh(mesh, *simplifying)
    if deviation_cell is not None:
        mesh.deviation = mesh_deviation(mesh, reference, cell_edge=deviation_cell)
    if iou_lattice is not None:
        mesh.volume_iou = mesh_volume_iou(mesh, reference, *iou_lattice)
    if selfx:
        _with_self_intersections(mesh, reference)
    return mesh


def _gt_to_view_frame(opt, var):
    """utils/eval_3D.py:120-123 / :186-190: the ground truth rotated into the view frame (R_gt p, no translation; x and y
    negated for pix3d).  One launch of zs_transform_points (round 6: the reference's `R @ p^T` was a rocBLAS batched GEMM on
    this path) - the pix3d sign flip rides on the rotation's first two rows, which negates exactly."""
    from . import camera
    pose = var.pose_gt.detach().to(torch.float32)
    B = pose.shape[0]
    T = torch.zeros(B, 3, 4, dtype=torch.float32, device=pose.device)
    T[:, :, :3] = pose[..., :3]
    if opt.data.dataset_test == 'pix3d':
        T[:, :2] = -T[:, :2]
    zero, one = torch.zeros(B, 3, device=pose.device), torch.ones(B, device=pose.device)
    var.dpc.points = camera.transform_points(var.dpc.points, T, zero, one)


@torch.no_grad()
def eval_metrics_default(opt, var, impl_network, vis_only=False):
    """utils/eval_3D.py:104-138."""
    points_3D = get_dense_3D_grid(opt, var)
    batch_size = points_3D.shape[0]
    level_vox, attn_vis = compute_level_grid(opt, impl_network, var.latent_depth, var.latent_semantic,
                                             points_3D, var.rgb_input_map, vis_only)
    if attn_vis:
        var.attn_vis = attn_vis
    var.eval_vox = points_3D.view(batch_size, -1, 3)
    var.mesh_pred, var.dpc_pred = _surface_clouds(opt, level_vox)
    _gt_to_view_frame(opt, var)
    var.dpc_pred = normalize_pc(var.dpc_pred)
    var.dpc.points = normalize_pc(var.dpc.points)
    if vis_only:
        return
    if opt.eval.icp:
        var.dpc_pred = ICP(opt, var.dpc_pred, var.dpc.points)
    dist_acc, dist_comp, _, _ = chamfer_distance(opt, X1=var.dpc_pred, X2=var.dpc.points)
    var.f_score = compute_fscore(dist_acc, dist_comp, opt.eval.f_thresholds)
    assert dist_acc.shape[1] == opt.eval.num_points
    var.cd_acc = dist_acc.mean(dim=1)
    var.cd_comp = dist_comp.mean(dim=1)
    return dist_acc.mean(), dist_comp.mean()


def eval_metrics_BF(opt, var, impl_network, vis_only=False):
    """utils/eval_3D.py:172-207."""
    points_3D = get_dense_3D_grid(opt, var)
    batch_size = points_3D.shape[0]
    level_vox, attn_vis = compute_level_grid(opt, impl_network, var.latent_depth, var.latent_semantic,
                                             points_3D, var.rgb_input_map, vis_only)
    if attn_vis:
        var.attn_vis = attn_vis
    var.eval_vox = points_3D.view(batch_size, -1, 3)
    var.mesh_pred, var.dpc_pred = _surface_clouds(opt, level_vox)
    _gt_to_view_frame(opt, var)
    if vis_only:
        return
    cd_acc, cd_comp, f_score = [], [], []
    shard = image_sharding(opt)
    for i in range(batch_size):
        best_acc, best_comp, best_fscore, best_pred, best_gt = \
            brute_force_search(var.dpc_pred[i], var.dpc.points[i], opt.eval.f_thresholds, opt.device, rot_shard=shard)
        var.dpc_pred[i] = best_pred.clone()
        var.dpc.points[i] = best_gt.clone()
        cd_acc.append(best_acc)
        cd_comp.append(best_comp)
        f_score.append(best_fscore)
    var.cd_acc = torch.stack(cd_acc, dim=0)
    var.cd_comp = torch.stack(cd_comp, dim=0)
    var.f_score = torch.stack(f_score, dim=0)
    return var.cd_acc.mean(), var.cd_comp.mean()


def eval_metrics(opt, var, impl_network, vis_only=False):
    """utils/eval_3D.py:209-213."""
    if opt.eval.brute_force:
        return eval_metrics_BF(opt, var, impl_network, vis_only)
    return eval_metrics_default(opt, var, impl_network, vis_only)


@torch.no_grad()
def ICP(opt, X1, X2, num_iter=50):
    """utils/eval_3D.py:271-284: every iteration is the Chamfer call + zs_icp_step (centroids, 3x3 cross-covariance, its SVD
    by Jacobi rotations, the reference's sign rule and the rigid update on the device: no ATen / LAPACK call, no host
    read in the loop)."""
    from .. import _lib
    assert len(X1) == len(X2)
    lib = _lib.load()
    x1, x2 = _gpu_f32(X1, "X1"), _gpu_f32(X2, "X2")
    B, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    scratch = torch.empty(max(1, lib.zs_icp_scratch_bytes(B) // 4), dtype=torch.float32, device=x1.device)
    nxt = torch.empty_like(x1)
    if x1.data_ptr() == X1.data_ptr():
        x1 = x1.clone()                         # the caller's tensor is not updated in place (the reference rebinds X1)
    for it in range(num_iter):
        _, _, idx, _ = chamfer_distance(opt, x1, x2)
        with torch.cuda.device(x1.device):
            rc = lib.zs_icp_step(_lib.ptr(x1), n, _lib.ptr(x2), m, _lib.ptr(idx), B, _lib.ptr(nxt), _lib.ptr(scratch),
                                 _lib.current_stream_ptr(x1.device))
        _lib.check(rc, "zs_icp_step")
        x1, nxt = nxt, x1
    return x1


class SimpleMesh(object):
    """Stand-in for the ``trimesh.Trimesh`` objects the reference stores in ``var.mesh_pred`` (dumps and the demo's .obj):
    ``triangles`` [n,3,3] = the iso-surface kernel's triangle soup (what sampling reads); ``vertices`` [v,3] / ``faces`` [n,3] =
    the INDEXED form ``mcubes.marching_cubes`` returns (utils/eval_3D.py:250-256), welded lazily on first access: a vertex on
    a grid edge is computed from the same two corner values by every cube sharing the edge, so equal vertices are equal bit
    for bit and welding = unique rows of the soup (``vertices[faces]`` reproduces ``triangles`` exactly).
    ``vertex_normals`` [v,3] float32 (trimesh's name): the area-weighted formula of vertex_normals_host; parity with
    trimesh's own weighting is unpinned (trimesh is not a dependency of this package).
    ``components`` (a MeshComponents: labels, per-component counts, area and signed volume) and, from it, trimesh's ``area``,
    ``volume``, ``euler_number`` and ``is_watertight``; filter_components(mesh, ...) is the stand-in for ``mesh.split()`` + a
    choice among the parts.
    ``adjacency`` (a MeshAdjacency: the vertex neighbourhood as a CSR, boundary flags) and trimesh's ``vertex_neighbors``;
    smooth_mesh(mesh, ...) is the stand-in for ``trimesh.smoothing.filter_taubin`` / ``filter_laplacian``.
    ``self_intersections`` (a MeshSelfIntersections: per face the number of other faces it crosses, the totals) and Open3D's
    ``is_self_intersecting()`` / ``get_self_intersecting_triangles()``.

    Built from a GPU tensor the mesh stays in HBM: ``device_triangles`` is that tensor (the turntable renders from it),
    the weld and the normals come from weld_mesh (csrc/mesh_weld.hip) on first access, and ``triangles`` / ``vertices`` /
    ``faces`` / ``vertex_normals`` are host copies made when somebody reads them - float32, float32, int64, float32, the same
    values either way.  Built from an array nothing needs a GPU (``device_triangles`` is None): the numpy weld below, which is
    also the kernels' checker."""

    def __init__(self, triangles):
        self.device_triangles = self._triangles = self._indexed = self._normals = None
        # set by field_normals(): the weld it made (vertices, faces, normals on the device: _weld copies it instead of welding
        # again), the field's normals [V,3] fp32 on the device, and the device count [1] int32 of vertices that fell back
        self._device_weld = self.device_field_normals = self.field_normal_fallbacks = self._field_normals = None
        self._components = None                          # mesh_components(self), cached by the ``components`` property
        self._adjacency = None                           # mesh_adjacency(self), cached by the ``adjacency`` property
        self._self_intersections = None                  # mesh_self_intersections(self), cached by ``self_intersections``
        # set by mesh_vertex_colors(): colours uint8 [V,3], seen flags uint8 [V], colour sources int32 [V] and (seen area, total
        # area) fp64 [2] on the device, and the host copies the properties below make when read
        self.device_vertex_colors = self.device_vertex_seen = self.device_color_source = self.device_seen_area = None
        self._vertex_colors = self._vertex_seen = self._seen_area = None
        if isinstance(triangles, torch.Tensor) and triangles.is_cuda:
            self.device_triangles = triangles.detach().to(torch.float32).reshape(-1, 3, 3).contiguous()
        else:
            self._triangles = np.asarray(triangles, np.float32).reshape(-1, 3, 3)

    @property
    def triangles(self):
        if self._triangles is None:
            self._triangles = self.device_triangles.cpu().numpy()
        return self._triangles

    def _weld(self, normals=False):
        if self.device_triangles is not None:
            if self._indexed is None or (normals and self._normals is None):
                welded = self._device_weld or weld_mesh(self.device_triangles, normals=normals)
                out = [t.cpu().numpy() for t in welded]
                self._indexed = (out[0], out[1].astype(np.int64))
                if len(out) > 2:
                    self._normals = out[2]
            return self._indexed
        if self._indexed is None:
            soup = np.ascontiguousarray(self.triangles.reshape(-1, 3))
            if len(soup) == 0:
                self._indexed = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
            else:
                keys = (soup + np.float32(0.0)).view(np.uint32)          # -0.0 and 0.0 are one vertex
                _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
                self._indexed = (soup[first], inverse.reshape(-1, 3).astype(np.int64))
        if normals and self._normals is None:
            self._normals = vertex_normals_host(self.triangles, self._indexed[1], len(self._indexed[0]))
        return self._indexed

    @property
    def vertices(self):
        return self._weld()[0]

    @property
    def faces(self):
        return self._weld()[1]

    @property
    def vertex_normals(self):
        self._weld(normals=True)
        return self._normals

    @property
    def components(self):
        """mesh_components(self), computed once: the connected components with their counts and measures (on the device for
        a GPU mesh until a column is read)."""
        if self._components is None:
            self._components = mesh_components(self)
        return self._components

    @property
    def adjacency(self):
        """mesh_adjacency(self), computed once: the vertex neighbourhood as a CSR with the boundary flags (a MeshAdjacency, on
        the device for a GPU mesh until an array is read); smooth_mesh(mesh, ...) runs over it."""
        if self._adjacency is None:
            self._adjacency = mesh_adjacency(self)
        return self._adjacency

    @property
    def self_intersections(self):
        """mesh_self_intersections(self), computed once: for every face the number of other faces it crosses, and the counts
        (a MeshSelfIntersections, on the device for a GPU mesh until ``check()`` reads the counts)."""
        if self._self_intersections is None:
            self._self_intersections = mesh_self_intersections(self)
        return self._self_intersections

    def is_self_intersecting(self):
        """Open3D's name: whether two faces of this mesh cross (mesh_self_intersections_host's rule: touching, coplanar
        overlap, coincident faces and the contact of neighbours do not count)."""
        return self.self_intersections.check()["n_pairs"] > 0

    def get_self_intersecting_triangles(self):
        """Open3D's name: [n,2] int64 on the host, the crossing pairs of faces (i, j), i < j, in lexicographic order
        (mesh_self_intersections(self, pairs=True): for a GPU mesh two calls with a read of the total in between)."""
        found = mesh_self_intersections(self, pairs=True).pairs
        if isinstance(found, torch.Tensor):
            found = found.cpu().numpy()
        return np.asarray(found, np.int64).reshape(-1, 2)

    def distance_to(self, points, closest=False):
        """mesh_distance(self, points, closest): the exact distance from ``points`` [M,3] to this surface - the nearest face and
        the squared distance to it (a MeshDistance; CUDA tensors for a GPU mesh, whose points must be a CUDA tensor)."""
        return mesh_distance(self, points, closest=closest)

    def contains(self, points):
        """trimesh's name: mesh_contains(self, points) - whether each of ``points`` [M,3] lies inside this mesh ([M] bool; a
        CUDA tensor for a GPU mesh, whose points must be a CUDA tensor)."""
        return mesh_contains(self, points)

    def signed_distance_to(self, points, closest=False):
        """mesh_signed_distance(self, points, closest): the exact distance from ``points`` [M,3] to this surface, negative
        inside ([M] float64; with ``closest`` also the nearest point of the surface)."""
        return mesh_signed_distance(self, points, closest=closest)

    def ray_cast(self, origins, directions, t_min=0.0, t_max=float("inf"), bary=False):
        """trimesh's ``ray.intersects_first``: mesh_ray_cast(self, origins, directions, ...) - where the rays o + t d first
        meet this surface (a MeshRays: t, face, side, weights; CUDA tensors for a GPU mesh, whose rays must be CUDA tensors)."""
        return mesh_ray_cast(self, origins, directions, t_min=t_min, t_max=t_max, bary=bary)

    @property
    def vertex_neighbors(self):
        """trimesh's name: a list of V int arrays, the indices of the vertices that share an edge with each vertex, ascending
        (``adjacency`` split into its rows on the host)."""
        adj = self.adjacency
        return np.split(adj.neighbors, adj.offsets[1:-1]) if len(adj.offsets) > 1 else []

    @property
    def area(self):
        """trimesh's name: the surface area, the sum over the components (float)."""
        return float(self.components.area.sum())

    @property
    def volume(self):
        """trimesh's name: the signed volume, the sum over the components - positive for a solid wound like marching cubes'
        meshes, a closed cavity counts negative (float)."""
        return float(self.components.signed_volume.sum())

    @property
    def euler_number(self):
        """trimesh's name: V - E + F over the whole mesh, degenerate faces (two equal indices) left out of E and F (int)."""
        return int(self.components.euler.sum())

    @property
    def is_watertight(self):
        """trimesh's name: at least one component, and every component closed - every edge used by exactly two faces that
        run through it in opposite directions."""
        closed = self.components.closed
        return bool(len(closed) > 0 and closed.all())

    @property
    def field_normals(self):
        """[v,3] float32, the rows of ``vertices``: minus the occupancy field's normalised gradient at each vertex, computed
        by field_normals() (on the device until read here)."""
        if self.device_field_normals is None:
            raise ValueError("this mesh has no field normals: eval_3D.field_normals(opt, impl_network, latents, meshes) "
                             "computes them")
        if self._field_normals is None:
            self._field_normals = self.device_field_normals.cpu().numpy()
        return self._field_normals


    def _colored(self, what):
        if self.device_vertex_colors is None:
            raise ValueError("this mesh has no %s: eval_3D.vertex_colors(opt, var) or eval_3D.mesh_vertex_colors(mesh, ...) "
                             "computes them" % what)

    @property
    def vertex_colors(self):
        """[v,3] uint8, the rows of ``vertices``: the input photo where the input camera saw the vertex, the colour of the
        nearest seen vertex elsewhere, computed by mesh_vertex_colors() (on the device until read here)."""
        self._colored("vertex colours")
        if self._vertex_colors is None:
            self._vertex_colors = self.device_vertex_colors.cpu().numpy()
        return self._vertex_colors

    @property
    def vertex_seen(self):
        """[v] bool: whether the input camera saw the vertex (mesh_vertex_colors_host's rule)."""
        self._colored("seen flags")
        if self._vertex_seen is None:
            self._vertex_seen = self.device_vertex_seen.cpu().numpy().astype(bool)
        return self._vertex_seen

    @property
    def seen_area_fraction(self):
        """The area of the faces whose three vertices the input camera saw over the mesh's area (float; 0.0 for a mesh
        without area)."""
        self._colored("seen area")
        if self._seen_area is None:
            self._seen_area = self.device_seen_area.cpu().numpy()
        seen, total = self._seen_area
        return float(seen / total) if total > 0.0 else 0.0


def mesh_to_field_points_host(vertices, range_min, G):
    """zs_mesh_to_field_points restated in numpy, operation for operation: marching cubes puts grid index u at
    v = min + u (max - min) / G (G samples per axis), the grid linspace(min, max, G) has sample u at min + u (max - min) / (G - 1),
    so the field that made vertex v was evaluated at p = min + (v - min) G / (G - 1) - float64, rounded to float32 (the minimum
    as the float32 the kernel receives)."""
    lo = np.float64(np.float32(range_min))
    v = np.asarray(vertices, np.float32).astype(np.float64)
    return (lo + (v - lo) * np.float64(G) / np.float64(G - 1)).astype(np.float32)


def field_normals(opt, impl_network, latent_depth, latent_semantic, meshes, chunk=65536):
    """Vertex normals from the field itself: for mesh b of the batch (SimpleMesh objects of convert_to_explicit on
    ``opt.eval.vox_res`` / ``opt.eval.range``) weld (weld_mesh), map the vertices to where the field that made them was
    evaluated (zs_mesh_to_field_points), take the gradient of the logit there with image b's latent
    (``impl_network.field_gradient``, ``chunk`` points at a time) and finish (zs_field_normals_finish): n = -g / |g| - occupancy
    rises inwards, so minus the gradient points out - with the weld's area-weighted normal wherever |g| is zero or not finite.
    Stored as ``mesh.field_normals`` ([V,3] float32, on the device until read; [0,3] for an empty mesh);
    ``mesh.field_normal_fallbacks`` is the device count [1] int32 of vertices that fell back.  GPU meshes only: a mesh built
    from a host array raises ValueError.  -> meshes."""
    from .. import _lib
    lib = _lib.load()
    range_min = float(opt.eval.range[0])
    G = int(opt.eval.vox_res) + 1
    if len(meshes) > latent_depth.shape[0]:
        raise ValueError("field_normals: %d meshes for %d latents" % (len(meshes), latent_depth.shape[0]))
    for b, mesh in enumerate(meshes):
        if getattr(mesh, "device_triangles", None) is None:
            raise ValueError("field_normals: mesh %d was built from a host array; there is no CPU path" % b)
    for b, mesh in enumerate(meshes):
        if mesh._device_weld is None:
            mesh._device_weld = weld_mesh(mesh.device_triangles, normals=True)
        vertices, _, fallback = mesh._device_weld
        V, dev = vertices.shape[0], vertices.device
        normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        if V:
            points = torch.empty_like(vertices)
            with _lib.on(dev):
                _lib.check(lib.zs_mesh_to_field_points(_lib.ptr(vertices), V, range_min, G, _lib.ptr(points),
                                                       _lib.current_stream_ptr(dev)), "zs_mesh_to_field_points")
            sem = None if latent_semantic is None else latent_semantic[b:b + 1]
            _, grad = impl_network.field_gradient(latent_depth[b:b + 1], sem, points.unsqueeze(0), chunk=chunk)
            grad = grad.reshape(V, 3)
            with _lib.on(dev):
                _lib.check(lib.zs_field_normals_finish(_lib.ptr(grad), _lib.ptr(fallback), V, _lib.ptr(normals), _lib.ptr(count),
                                                       _lib.current_stream_ptr(dev)), "zs_field_normals_finish")
        mesh.device_field_normals, mesh.field_normal_fallbacks, mesh._field_normals = normals, count, None
    return meshes


def vertex_normals_host(triangles, faces, n_vertices):
    """The normals of zs_mesh_weld_vertices restated in numpy, operation for operation: per vertex the sum of
    cross(v1 - v0, v2 - v0) over its corners' triangles in ascending soup order (``np.add.at`` adds in index order; a triangle
    that holds the vertex twice counts twice) in float64, normalised in float64, rounded to float32; a zero or non-finite sum
    gives (0, 0, 0).  ``triangles`` [n,3,3] float32, ``faces`` [n,3] -> [n_vertices,3] float32."""
    t = np.asarray(triangles, np.float32).reshape(-1, 3, 3).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a, b = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        face_n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                           a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                           a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        total = np.zeros((int(n_vertices), 3), np.float64)
        np.add.at(total, np.asarray(faces, np.int64).reshape(-1), np.repeat(face_n, 3, axis=0))
        length = np.sqrt(total[:, 0] * total[:, 0] + total[:, 1] * total[:, 1] + total[:, 2] * total[:, 2])
        ok = (length > 0.0) & (length < np.inf)
        return np.where(ok[:, None], total / np.where(ok, length, 1.0)[:, None], 0.0).astype(np.float32)


@torch.no_grad()
def weld_mesh(tris, normals=False):
    """A triangle soup [n,3,3] on the GPU -> (vertices [V,3] fp32, faces [n,3] int32[, normals [V,3] fp32]), GPU tensors on
    the soup's device, enqueued on the current stream: zs_mesh_weld + zs_mesh_weld_vertices (csrc/mesh_weld.hip).  The
    semantics of SimpleMesh's numpy weld, bit for bit - np.unique's row order of the (x + 0, y + 0, z + 0) bit patterns, the
    first occurrence's own bits as the stored vertex - and the normals of vertex_normals_host.  One 4-byte device-to-host
    copy: the vertex count, which sizes the outputs."""
    from .. import _lib
    lib = _lib.load()
    if not (isinstance(tris, torch.Tensor) and tris.is_cuda):
        raise ValueError("weld_mesh: tris must be a GPU tensor (SimpleMesh welds an array on the host)")
    soup = tris.detach().to(torch.float32).reshape(-1, 3, 3).contiguous()
    n, dev = soup.shape[0], soup.device
    faces = torch.empty(n, 3, dtype=torch.int32, device=dev)
    n_verts = 0
    if n:
        scratch = torch.empty(lib.zs_mesh_weld_scratch_bytes(n) // 8, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        stream = _lib.current_stream_ptr(dev)
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_weld(_lib.ptr(soup), n, _lib.ptr(faces), _lib.ptr(count), _lib.ptr(scratch), stream),
                       "zs_mesh_weld")
            n_verts = int(count.item())                      # 4-byte D2H: sizes the outputs
    vertices = torch.empty(n_verts, 3, dtype=torch.float32, device=dev)
    vnormals = torch.empty(n_verts, 3, dtype=torch.float32, device=dev) if normals else None
    if n:
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_weld_vertices(_lib.ptr(soup), n, _lib.ptr(scratch), n_verts, _lib.ptr(vertices),
                                                 _lib.ptr(vnormals), stream), "zs_mesh_weld_vertices")
    return (vertices, faces, vnormals) if normals else (vertices, faces)


COMPONENT_COLUMNS = ("faces", "vertices", "degenerate_faces", "edges", "boundary_edges", "nonmanifold_edges",
                     "misoriented_edges", "euler")


class MeshComponents(object):
    """The connected components of a mesh (mesh_components / mesh_components_host), numbered in ascending order of their
    smallest vertex index:

      n_components                      int
      vertex_labels [V], face_labels [F] int32 (a face has the label of its first vertex)
      counts [C,8] int32                the columns of COMPONENT_COLUMNS, also readable by name: ``faces``, ``vertices``,
                                        ``degenerate_faces``, ``edges``, ``boundary_edges``, ``nonmanifold_edges``,
                                        ``misoriented_edges``, ``euler``
      area, signed_volume [C] float64
      closed [C] bool                   at least one non-degenerate face and no boundary, non-manifold or misoriented edge

    From a GPU mesh the ``device_*`` tensors (vertex_labels, face_labels, counts, measures [C,2] fp64 = area, signed volume)
    hold the results and the arrays above are host copies made when first read; from a host mesh they are None."""

    def __init__(self, n_components, vertex_labels, face_labels, counts, measures):
        self.n_components = int(n_components)
        self.device_vertex_labels = self.device_face_labels = self.device_counts = self.device_measures = None
        self._host = {}
        given = dict(vertex_labels=vertex_labels, face_labels=face_labels, counts=counts, measures=measures)
        if isinstance(counts, torch.Tensor):
            for key, value in given.items():
                setattr(self, "device_" + key, value)
        else:
            self._host = given

    def _read(self, key):
        if key not in self._host:
            self._host[key] = getattr(self, "device_" + key).cpu().numpy()
        return self._host[key]

    vertex_labels = property(lambda self: self._read("vertex_labels"))
    face_labels = property(lambda self: self._read("face_labels"))
    counts = property(lambda self: self._read("counts"))
    area = property(lambda self: self._read("measures")[:, 0])
    signed_volume = property(lambda self: self._read("measures")[:, 1])

    @property
    def closed(self):
        c = self.counts
        return (c[:, 0] - c[:, 2] > 0) & (c[:, 4] == 0) & (c[:, 5] == 0) & (c[:, 6] == 0)

    def table(self):
        """The per-component table as a list of dicts of Python numbers (what demo.py's mesh report stores)."""
        closed = self.closed
        return [dict([(name, int(self.counts[c, k])) for k, name in enumerate(COMPONENT_COLUMNS)]
                     + [("closed", bool(closed[c])), ("area", float(self.area[c])), ("signed_volume", float(self.signed_volume[c]))])
                for c in range(self.n_components)]


for _k, _name in enumerate(COMPONENT_COLUMNS):
    setattr(MeshComponents, _name, property(lambda self, _k=_k: self.counts[:, _k]))


def mesh_face_terms_host(triangles, faces):
    """The per-face terms of mesh_components_host's sums, float64 [F] each: area |cross(v1 - v0, v2 - v0)| / 2 and signed
    volume dot(v0, cross(v1, v2)) / 6 from the float32 corners, operation by operation as cs_terms_kernel computes them; a
    face with two equal indices gives exactly 0 for both."""
    t = np.asarray(triangles, np.float32).reshape(-1, 3, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    with np.errstate(over="ignore", invalid="ignore"):
        x0, y0, z0 = t[:, 0, 0], t[:, 0, 1], t[:, 0, 2]
        x1, y1, z1 = t[:, 1, 0], t[:, 1, 1], t[:, 1, 2]
        x2, y2, z2 = t[:, 2, 0], t[:, 2, 1], t[:, 2, 2]
        ax, ay, az, bx, by, bz = x1 - x0, y1 - y0, z1 - z0, x2 - x0, y2 - y0, z2 - z0
        nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        area = 0.5 * np.sqrt(nx * nx + ny * ny + nz * nz)
        cx, cy, cz = y1 * z2 - z1 * y2, z1 * x2 - x1 * z2, x1 * y2 - y1 * x2
        volume = (x0 * cx + y0 * cy + z0 * cz) / 6.0
    return np.where(degenerate, 0.0, area), np.where(degenerate, 0.0, volume)


def mesh_components_host(vertices, faces, triangles):
    """The definition of the mesh-component quantities and the checker of csrc/mesh_components.hip, in numpy.
    ``vertices`` [V,3] (only V is used), ``faces`` [F,3] the weld's indices, ``triangles`` [F,3,3] float32 the soup the weld
    was made from -> MeshComponents.

    Components: two vertices are connected when some face holds both.  Sharing a welded vertex is enough, an edge is not
    required: trimesh's ``split`` goes by edge adjacency and separates two bodies that touch in a point - this deliberately
    does not.  Components are numbered in ascending order of their smallest vertex index; a face has the label of its first
    vertex.  A face is degenerate when two of its three indices are equal (by index, not by area): it belongs to its
    component, is counted in ``degenerate_faces``, has no edges and is left out of the face term of the Euler number; its
    area and volume terms are exactly zero.  ``edges`` = unique undirected vertex pairs of the other faces; ``boundary_edges``
    are used by exactly one face, ``nonmanifold_edges`` by more than two, ``misoriented_edges`` by exactly two whose
    half-edges run the same way; an edge belongs to the component of its vertices.  euler = vertices - edges + (faces -
    degenerate_faces).  area = sum of |cross(v1 - v0, v2 - v0)| / 2, signed_volume = sum of dot(v0, cross(v1, v2)) / 6 over the
    component's faces in ascending face order, from the float32 corners converted to float64, every operation as written
    below (the kernels do the same operations; only the order of the additions differs).  With the winding of this package's
    marching cubes a solid body has a positive volume and a closed cavity a negative one."""
    V = len(vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    assert np.asarray(triangles).size == 9 * F and (F == 0 or (f.min() >= 0 and f.max() < V))
    # union-find by rounds: hook every face's roots under the smallest of them, then jump every pointer to its root
    root = np.arange(V, dtype=np.int64)
    live = f
    while len(live):
        r = root[live]
        low = r.min(axis=1)
        differ = (r != low[:, None]).any(axis=1)               # faces whose vertices are not under one root yet
        live, r, low = live[differ], r[differ], low[differ]
        if not len(live):
            break
        np.minimum.at(root, r.reshape(-1), np.repeat(low, 3))
        while True:
            jumped = root[root]
            if np.array_equal(jumped, root):
                break
            root = jumped
    roots = np.flatnonzero(root == np.arange(V))                     # ascending: the smallest vertex of each component
    C = len(roots)
    vertex_labels = np.searchsorted(roots, root).astype(np.int32)
    face_labels = vertex_labels[f[:, 0]].astype(np.int32) if F else np.zeros(0, np.int32)
    counts = np.zeros((C, len(COMPONENT_COLUMNS)), np.int32)
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    counts[:, 0] = np.bincount(face_labels, minlength=C)
    counts[:, 1] = np.bincount(vertex_labels, minlength=C)
    counts[:, 2] = np.bincount(face_labels[degenerate], minlength=C)
    g = f[~degenerate]
    a, b = g.reshape(-1), g[:, [1, 2, 0]].reshape(-1)                # the half-edges a -> b
    key = (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
    edge, inverse, uses = np.unique(key, return_inverse=True, return_counts=True)
    forward = np.bincount(inverse.reshape(-1), weights=(a < b), minlength=len(edge)).astype(np.int64)
    edge_label = vertex_labels[(edge >> np.uint64(32)).astype(np.int64)]
    counts[:, 3] = np.bincount(edge_label, minlength=C)
    counts[:, 4] = np.bincount(edge_label[uses == 1], minlength=C)
    counts[:, 5] = np.bincount(edge_label[uses > 2], minlength=C)
    counts[:, 6] = np.bincount(edge_label[(uses == 2) & (forward != 1)], minlength=C)
    counts[:, 7] = counts[:, 1] - counts[:, 3] + (counts[:, 0] - counts[:, 2])
    area, volume = mesh_face_terms_host(triangles, f)
    measures = np.zeros((C, 2), np.float64)
    measures[:, 0] = np.bincount(face_labels, weights=area, minlength=C)      # (bincount adds in face order)
    measures[:, 1] = np.bincount(face_labels, weights=volume, minlength=C)
    return MeshComponents(C, vertex_labels, face_labels, counts, measures)


def _components_device(tris, faces, n_verts):
    """zs_mesh_components + zs_mesh_component_stats on a welded GPU mesh -> MeshComponents of device tensors.  One 8-byte
    device-to-host copy: the component count, which sizes the tables, with the kernels' status word beside it."""
    from .. import _lib
    lib = _lib.load()
    n, dev = tris.shape[0], tris.device
    vertex_labels = torch.empty(n_verts, dtype=torch.int32, device=dev)
    face_labels = torch.empty(n, dtype=torch.int32, device=dev)
    n_comps = 0
    if n and n_verts:
        scratch = torch.empty(lib.zs_mesh_components_scratch_bytes(n, n_verts) // 8 + 1, dtype=torch.int64, device=dev)
        out = torch.zeros(2, dtype=torch.int32, device=dev)
        stream = _lib.current_stream_ptr(dev)
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_components(_lib.ptr(faces), n, n_verts, _lib.ptr(vertex_labels), _lib.ptr(face_labels),
                                              _lib.ptr(out), _lib.ptr(scratch), stream), "zs_mesh_components")
            n_comps, status = out.tolist()                   # 8-byte D2H: sizes the tables
        if status:
            raise _lib.ZeroShapeHipError("zs_mesh_components: status %d (%s)" % (
                status, "a face index outside the vertices" if status & 2 else "a linking loop ran into its bound"))
    counts = torch.empty(n_comps, len(COMPONENT_COLUMNS), dtype=torch.int32, device=dev)
    measures = torch.empty(n_comps, 2, dtype=torch.float64, device=dev)
    if n_comps:
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_component_stats(_lib.ptr(tris), _lib.ptr(faces), _lib.ptr(vertex_labels), _lib.ptr(face_labels),
                                                   n, n_verts, n_comps, _lib.ptr(counts), _lib.ptr(measures), _lib.ptr(scratch),
                                                   stream), "zs_mesh_component_stats")
    return MeshComponents(n_comps, vertex_labels, face_labels, counts, measures)


@torch.no_grad()
def mesh_components(mesh):
    """The connected components of a SimpleMesh with their counts and measures -> MeshComponents (the semantics:
    mesh_components_host).  A GPU mesh is labelled and measured on the device (csrc/mesh_components.hip) from the weld it
    carries (``_device_weld``, which field_normals leaves too) or, if it has none yet, from one weld_mesh call whose result it
    then keeps; a mesh built from a host array goes through the host checker.  ``mesh.components`` caches the result."""
    if getattr(mesh, "device_triangles", None) is not None:
        if mesh._device_weld is None:
            mesh._device_weld = weld_mesh(mesh.device_triangles, normals=True)
        vertices, faces = mesh._device_weld[0], mesh._device_weld[1]
        return _components_device(mesh.device_triangles, faces, vertices.shape[0])
    return mesh_components_host(mesh.vertices, mesh.faces, mesh.triangles)


def _check_filter_arguments(min_component_area, keep, n_components):
    if min_component_area is not None and not (0.0 < float(min_component_area) <= 1.0):
        raise ValueError("filter_components: min_component_area must lie in (0, 1], got %r" % (min_component_area,))
    if keep is None:
        return None
    flags = np.zeros(n_components, np.uint8)
    ids = np.asarray(list(keep), np.int64).reshape(-1)
    if len(ids) and (ids.min() < 0 or ids.max() >= n_components):
        raise ValueError("filter_components: keep names a component outside 0..%d" % (n_components - 1))
    flags[ids] = 1
    return flags


def select_components_host(components, min_component_area=None, drop_cavities=False, keep=None):
    """The rule of filter_components in numpy -> bool [C]: the checker of zs_mesh_components_select."""
    flags = _check_filter_arguments(min_component_area, keep, components.n_components)
    if flags is not None:
        return flags.astype(bool)
    kept = np.ones(components.n_components, bool)
    if min_component_area is not None and components.n_components:
        kept &= components.area >= np.float64(min_component_area) * components.area.max()
    if drop_cavities:
        kept &= ~(components.closed & (components.signed_volume < 0.0))
    return kept


@torch.no_grad()
def filter_components(mesh, min_component_area=None, drop_cavities=False, keep=None):
    """A new SimpleMesh of the components of ``mesh`` that pass - its soup is the kept faces in soup order, on the GPU for a
    GPU mesh (rule and compaction run on the device: zs_mesh_components_select, one 4-byte read-back of the kept count,
    zs_mesh_filter_faces), in numpy for a host mesh.  Component c is kept iff
    ``area[c] >= min_component_area * max(area)`` (``min_component_area`` in (0, 1]; at 1.0 only the largest component and
    exact ties stay; None: no area rule) and, with ``drop_cavities``, it is not a closed component of negative signed
    volume; or, with ``keep`` (component labels) given, iff c is in ``keep``.  An empty mesh, or a rule that keeps nothing,
    gives an empty mesh."""
    comps = mesh.components
    flags = _check_filter_arguments(min_component_area, keep, comps.n_components)
    if getattr(mesh, "device_triangles", None) is None:
        kept = select_components_host(comps, min_component_area, drop_cavities, keep)
        return SimpleMesh(mesh.triangles[kept[comps.face_labels]] if len(mesh.triangles) else mesh.triangles.copy())
    from .. import _lib
    lib = _lib.load()
    tris = mesh.device_triangles
    n, dev = tris.shape[0], tris.device
    n_verts = comps.device_vertex_labels.shape[0]
    n_kept = 0
    if n and n_verts:
        scratch = torch.empty(lib.zs_mesh_components_scratch_bytes(n, n_verts) // 8 + 1, dtype=torch.int64, device=dev)
        keep_pos = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        explicit = None if flags is None else torch.from_numpy(flags).to(dev)
        stream = _lib.current_stream_ptr(dev)
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_components_select(
                _lib.ptr(comps.device_counts), _lib.ptr(comps.device_measures), comps.n_components,
                0.0 if min_component_area is None else float(min_component_area), int(bool(drop_cavities)), _lib.ptr(explicit),
                _lib.ptr(comps.device_face_labels), n, n_verts, _lib.ptr(keep_pos), _lib.ptr(count), _lib.ptr(scratch), stream),
                "zs_mesh_components_select")
            n_kept = int(count.item())                       # 4-byte D2H: sizes the output
    out = torch.empty(n_kept, 3, 3, dtype=torch.float32, device=dev)
    if n_kept:
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_filter_faces(_lib.ptr(tris), _lib.ptr(keep_pos), n, _lib.ptr(out), n_kept, stream),
                       "zs_mesh_filter_faces")
    return SimpleMesh(out)


# ---- vertex neighbourhood and smoothing (csrc/mesh_smooth.hip) ----

class MeshAdjacency(object):
    """The vertex neighbourhood of an indexed mesh (mesh_adjacency / mesh_adjacency_host) as a CSR:

      offsets [V + 1] int32, neighbors [nnz] int32   row v = neighbors[offsets[v]:offsets[v + 1]]: the distinct other endpoints of
                                                     v's edges, ascending (a face with two equal indices has no edges)
      boundary [V] uint8                             1 iff some edge at the vertex is used by exactly one non-degenerate face
      degree [V] int32                               offsets[1:] - offsets[:-1]
      n_edges                                        int, nnz / 2: the unique undirected edges

    From a GPU mesh the ``device_*`` tensors (offsets, neighbors, boundary) hold the results and the arrays above are host
    copies made when first read; from a host mesh they are None."""

    def __init__(self, offsets, neighbors, boundary):
        self.device_offsets = self.device_neighbors = self.device_boundary = None
        self._host = {}
        given = dict(offsets=offsets, neighbors=neighbors, boundary=boundary)
        if isinstance(offsets, torch.Tensor):
            for key, value in given.items():
                setattr(self, "device_" + key, value)
        else:
            self._host = given
        self.n_edges = int(neighbors.shape[0]) // 2

    def _read(self, key):
        if key not in self._host:
            self._host[key] = getattr(self, "device_" + key).cpu().numpy()
        return self._host[key]

    offsets = property(lambda self: self._read("offsets"))
    neighbors = property(lambda self: self._read("neighbors"))
    boundary = property(lambda self: self._read("boundary"))
    degree = property(lambda self: np.diff(self.offsets).astype(np.int32))


def mesh_adjacency_host(faces, n_vertices):
    """The definition of MeshAdjacency and the checker of zs_mesh_adjacency, in numpy.  ``faces`` [F,3] the weld's indices over
    ``n_vertices`` vertices.  A face with two equal indices (the components' rule for a degenerate face) contributes no
    edges, every other face its three undirected edges; a duplicated edge is listed once; an edge is a boundary edge when
    exactly one such face uses it (three or more uses: not a boundary edge)."""
    V = int(n_vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    assert len(f) == 0 or (f.min() >= 0 and f.max() < V)
    g = f[~((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))]
    a, b = g.reshape(-1), g[:, [1, 2, 0]].reshape(-1)                # every use of an edge, entered in both of its rows
    key = np.concatenate([(a << 32) | b, (b << 32) | a])
    entry, uses = np.unique(key, return_counts=True)                 # row after row, each row ascending
    source = entry >> 32
    boundary = np.zeros(V, np.uint8)
    boundary[source[uses == 1]] = 1
    offsets = np.searchsorted(source, np.arange(V + 1)).astype(np.int32)
    return MeshAdjacency(offsets, (entry & 0xffffffff).astype(np.int32), boundary)


def _check_smooth_arguments(iterations, lamb, mu):
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError("smooth_mesh: iterations must be an integer >= 0, got %r" % (iterations,))
    if isinstance(lamb, bool) or not isinstance(lamb, (int, float, np.integer, np.floating)) or not (0.0 < float(lamb) <= 1.0):
        raise ValueError("smooth_mesh: lamb must lie in (0, 1], got %r" % (lamb,))
    if mu is not None and (isinstance(mu, bool) or not isinstance(mu, (int, float, np.integer, np.floating))
                           or not (-1.0 <= float(mu) < 0.0)):
        raise ValueError("smooth_mesh: mu must be None (every pass uses lamb) or lie in [-1, 0), got %r" % (mu,))


def smooth_vertices_host(vertices, offsets, neighbors, boundary, iterations=10, lamb=0.5, mu=-0.53, pin_boundary=True):
    """The definition of smooth_mesh's passes and the checker of zs_mesh_smooth, in numpy: ``vertices`` [V,3] float32 are widened
    once to float64 and stay float64 between passes; pass t (from 0) uses f = ``lamb``, or f = ``mu`` when ``mu`` is given and t
    is odd (trimesh's counting: 10 iterations are 5 lambda|mu pairs).  A vertex moves iff its degree is positive and it is not
    pinned (``pin_boundary`` and its boundary flag set): s = 0, then s = s + x[neighbour] along its row in row order, m = s /
    degree, x' = x + f * (m - x), every operation as written - the sum goes slot by slot (slot k of every row that has one), so
    the float64 additions happen in the kernel's order.  The other vertices are copied.  After the last pass the positions are
    rounded to float32 -> [V,3] float32; ``iterations`` = 0 returns the input's bits."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    x = smooth_positions_host(v32.astype(np.float64), offsets, neighbors, boundary, iterations, lamb, mu, pin_boundary)
    return x.astype(np.float32)


def smooth_positions_host(x, offsets, neighbors, boundary, iterations, lamb, mu, pin_boundary):
    """The passes of smooth_vertices_host on float64 positions [V,3] -> float64 [V,3], before the rounding to float32."""
    _check_smooth_arguments(iterations, lamb, mu)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    if iterations == 0 or len(x) == 0:
        return x.copy()
    offsets, neighbors = np.asarray(offsets, np.int64), np.asarray(neighbors, np.int64)
    V = len(x)
    assert offsets.shape == (V + 1,) and offsets[0] == 0 and np.all(np.diff(offsets) >= 0) and offsets[-1] == len(neighbors)
    assert len(neighbors) == 0 or (neighbors.min() >= 0 and neighbors.max() < V)
    degree = np.diff(offsets)
    moving = degree > 0
    if pin_boundary:
        moving &= np.asarray(boundary).reshape(-1) == 0
    rows = np.flatnonzero(moving)
    begin, count = offsets[rows], degree[rows]
    by_slot = []                                                     # slot k: (positions among ``rows``, the neighbours there)
    for k in range(int(count.max()) if len(rows) else 0):
        has = np.flatnonzero(count > k)
        by_slot.append((has, neighbors[begin[has] + k]))
    d = count.astype(np.float64)[:, None]
    for t in range(int(iterations)):
        f = np.float64(mu if (mu is not None and t % 2 == 1) else lamb)
        s = np.zeros((len(rows), 3), np.float64)
        for has, nb in by_slot:
            s[has] = s[has] + x[nb]
        m = s / d
        new = x.copy()
        new[rows] = x[rows] + f * (m - x[rows])
        x = new
    return x


def _adjacency_device(faces, n_verts):
    """zs_mesh_adjacency on a welded GPU mesh -> MeshAdjacency of device tensors.  One 8-byte device-to-host copy: nnz, which
    sizes ``neighbors``, with the kernels' status word beside it."""
    from .. import _lib
    lib = _lib.load()
    n, dev = faces.shape[0], faces.device
    offsets = torch.zeros(n_verts + 1, dtype=torch.int32, device=dev)
    boundary = torch.zeros(n_verts, dtype=torch.uint8, device=dev)
    neighbors = torch.empty(0, dtype=torch.int32, device=dev)
    if n and n_verts:
        nbytes = lib.zs_mesh_adjacency_scratch_bytes(n, n_verts)
        if nbytes == 0:
            raise _lib.ZeroShapeHipError("mesh_adjacency: %d faces over %d vertices exceed the kernels' limits" % (n, n_verts))
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
        room = torch.empty(6 * n, dtype=torch.int32, device=dev)
        out = torch.zeros(2, dtype=torch.int32, device=dev)
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_adjacency(_lib.ptr(faces), n, n_verts, _lib.ptr(offsets), _lib.ptr(room), _lib.ptr(boundary),
                                             _lib.ptr(out), _lib.ptr(scratch), _lib.current_stream_ptr(dev)), "zs_mesh_adjacency")
            nnz, status = out.tolist()                       # 8-byte D2H: sizes the neighbour list
        if status:
            raise _lib.ZeroShapeHipError("zs_mesh_adjacency: status %d (a face index outside the vertices)" % status)
        neighbors = room[:nnz].clone()
    return MeshAdjacency(offsets, neighbors, boundary)


@torch.no_grad()
def mesh_adjacency(mesh):
    """The vertex neighbourhood of a SimpleMesh -> MeshAdjacency (the semantics: mesh_adjacency_host).  A GPU mesh is processed
    on the device (csrc/mesh_smooth.hip) from the weld it carries or, if it has none yet, from one weld_mesh call whose result
    it then keeps, as mesh_components does; a mesh built from a host array goes through the host checker.
    ``mesh.adjacency`` caches the result."""
    if getattr(mesh, "device_triangles", None) is not None:
        if mesh._device_weld is None:
            mesh._device_weld = weld_mesh(mesh.device_triangles, normals=True)
        vertices, faces = mesh._device_weld[0], mesh._device_weld[1]
        return _adjacency_device(faces, vertices.shape[0])
    return mesh_adjacency_host(mesh.faces, len(mesh.vertices))


@torch.no_grad()
def smooth_mesh(mesh, iterations=10, lamb=0.5, mu=-0.53, pin_boundary=True):
    """A new SimpleMesh whose vertices are those of ``mesh`` after ``iterations`` smoothing passes over its vertex
    neighbourhood (the semantics: smooth_vertices_host) and whose soup is those vertices gathered through the faces, in the
    input's face order - trimesh's ``smoothing.filter_taubin`` / ``filter_laplacian`` with uniform weights.  Pass t uses
    ``lamb`` (0 < lamb <= 1), or ``mu`` (-1 <= mu < 0) when t is odd: 10 iterations are 5 shrink|inflate pairs, which keep the
    volume that plain Laplacian smoothing (``mu=None``: every pass uses ``lamb``) loses.  The defaults are Taubin's published
    pair - a design choice, not a measurement.  With ``pin_boundary`` the vertices of open edges stay where they are.  A GPU
    mesh stays in HBM (zs_mesh_smooth + zs_mesh_gather_faces on the weld and the adjacency it carries; one 4-byte read-back, the
    status word); a host mesh is computed in numpy.  The new mesh carries nothing from the old one - no weld, components or
    colours: smooth first, then colour.  An empty mesh gives an empty mesh."""
    _check_smooth_arguments(iterations, lamb, mu)
    adj = mesh.adjacency
    if getattr(mesh, "device_triangles", None) is None:
        moved = smooth_vertices_host(mesh.vertices, adj.offsets, adj.neighbors, adj.boundary, iterations, lamb, mu, pin_boundary)
        return SimpleMesh(moved[mesh.faces] if len(mesh.faces) else mesh.triangles.copy())
    from .. import _lib
    lib = _lib.load()
    vertices, faces = mesh._device_weld[0], mesh._device_weld[1]
    n, n_verts, dev = faces.shape[0], vertices.shape[0], vertices.device
    out = torch.empty(n, 3, 3, dtype=torch.float32, device=dev)
    if n and n_verts:
        moved = torch.empty_like(vertices)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.zs_mesh_smooth_scratch_bytes(n_verts) // 8 + 1, dtype=torch.int64, device=dev)
        stream = _lib.current_stream_ptr(dev)
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_smooth(_lib.ptr(vertices), n_verts, _lib.ptr(adj.device_offsets), _lib.ptr(adj.device_neighbors),
                                          _lib.ptr(adj.device_boundary) if pin_boundary else None, int(iterations), float(lamb),
                                          0.0 if mu is None else float(mu), int(mu is not None), _lib.ptr(moved), _lib.ptr(status),
                                          _lib.ptr(scratch), stream), "zs_mesh_smooth")
            _lib.check(lib.zs_mesh_gather_faces(_lib.ptr(moved), _lib.ptr(faces), n, n_verts, _lib.ptr(out), stream),
                       "zs_mesh_gather_faces")
            bad = int(status.item())                         # 4-byte D2H, after everything is enqueued
        if bad:
            raise _lib.ZeroShapeHipError("zs_mesh_smooth: status %d (%s)" % (
                bad, "a neighbour index outside the vertices" if bad & 2 else "a row of the adjacency runs backwards"))
    return SimpleMesh(out)


# ---- simplification: vertex clustering with quadric-error placement (csrc/mesh_simplify.hip) ----

# The weight of the pull towards the cluster mean relative to the mean eigenvalue of the cluster's quadric: a design choice, not
# a measurement (MSIMP_RHO of csrc/mesh_simplify.hip is the same number).  It keeps the system solvable where the quadric
# alone is singular (a flat or straight-creased neighbourhood) and is too small to move a well-determined minimiser visibly.
SIMPLIFY_RHO = 1e-3
SIMPLIFY_POSITIONS = ("mean", "quadric")                 # zs_mesh_simplify: mode
SIMPLIFY_CELL_BITS = 21                                  # cells per axis: [0, 2^21)
SIMPLIFY_MAX_VERTICES = 1 << 21                          # three cluster ids share one 63-bit key

MeshSimplification = collections.namedtuple(
    "MeshSimplification", "cell origin position input_faces clusters degenerate_faces duplicate_faces kept_faces fallbacks")
MeshSimplification.__doc__ = """What simplify_mesh did, on the mesh it returns (``mesh.simplification``): ``cell`` (float), ``origin``
(3 floats), ``position`` ("quadric" or "mean"), and the counts - ``input_faces`` = ``kept_faces`` + ``degenerate_faces`` (two
corners in one cluster) + ``duplicate_faces`` (a kept face already has these three clusters in this rotation), ``clusters`` (the
occupied cells), ``fallbacks`` (clusters of two or more vertices where quadric placement was asked for and the mean was
taken)."""

SimplifiedHost = collections.namedtuple("SimplifiedHost", "triangles cluster_of representatives kept fell_back counts")


def _sums_in_order(values, starts, counts, short=64):
    """Per segment i of the rows of ``values`` [N,k] float64 (rows starts[i] .. starts[i] + counts[i]): s = 0, then s = s + row,
    row after row - the additions of one thread that walks the segment.  Segments of up to ``short`` rows go slot by slot (slot k
    of every segment that has one), the longer ones one at a time through np.add.accumulate, which adds in index order; both are
    that sequence of float64 additions -> [S,k]."""
    sums = np.zeros((len(starts), values.shape[1]), np.float64)
    if len(starts) == 0:
        return sums
    small = counts <= short
    for k in range(int(counts[small].max()) if small.any() else 0):
        has = np.flatnonzero(small & (counts > k))
        sums[has] = sums[has] + values[starts[has] + k]
    zero = np.zeros((1, values.shape[1]), np.float64)
    for i in np.flatnonzero(~small):
        sums[i] = np.add.accumulate(np.concatenate([zero, values[starts[i]:starts[i] + counts[i]]]), axis=0)[-1]
    return sums


def _check_simplify_arguments(cell, position):
    if isinstance(cell, bool) or not isinstance(cell, (int, float, np.integer, np.floating)) or not (0.0 < float(cell) < np.inf):
        raise ValueError("simplify_mesh: cell must be a finite number > 0, got %r" % (cell,))
    if position not in SIMPLIFY_POSITIONS:
        raise ValueError("simplify_mesh: position must be 'quadric' or 'mean', got %r" % (position,))


def _simplify_origin(origin):
    try:
        o = np.asarray(origin, np.float64).reshape(-1)
    except (TypeError, ValueError):
        o = np.zeros(0)
    if o.shape != (3,) or not np.all(np.isfinite(o)):
        raise ValueError("simplify_mesh: origin must be None or three finite numbers, got %r" % (origin,))
    return o


def simplify_mesh_host(vertices, faces, origin, cell, position="quadric"):
    """The definition of simplify_mesh and the checker of zs_mesh_simplify, in numpy: uniform-grid vertex clustering
    (Rossignac-Borrel) with quadric-error placement (Lindstrom; Open3D's ``simplify_vertex_clustering``) of an indexed mesh -
    ``vertices`` [V,3] float32, ``faces`` [F,3] - on the grid of edge ``cell`` (float64) whose planes pass through ``origin``
    (3 float64).  Every formula is elementwise float64 in the order written; every sum goes through _sums_in_order.

      cells       c = floor((float64(v) - origin) / cell) per axis, each in [0, 2^21): ValueError for a coordinate that is not
                  finite or a c outside.  Vertices with equal c are one cluster; ids ascend with cx << 42 | cy << 21 | cz, and
                  inside a cluster the members are taken in ascending vertex index (a stable sort).
      mean        in coordinates local to the cell centre origin + (c + 0.5) * cell: s = 0, s = s + (float64(v) - centre) over
                  the members, m = s / count.
      quadrics    (``position`` = "quadric") every (face, corner) adds, to the cluster of that corner's vertex, its face's plane
                  quadric in THAT cluster's local coordinates: p, q, r = the three vertices minus the centre, n = (q - p) x (r - p),
                  |n| = sqrt((n0 n0 + n1 n1) + n2 n2), d = -((n0 p0 + n1 p1) + n2 p2); A += (n_i n_j) / |n|, b += (n_i d) / |n| -
                  the weighting is n n^T / |n|: the unit normal's quadric times twice the face's area.  (The constant term
                  d d / |n|, the tenth entry, does not enter the minimiser and is not kept.)  A face whose |n| is zero or not
                  finite adds nothing.  Per cluster the terms are added in ascending 3 * face + corner.
      placement   minimise x^T A x + 2 b^T x + w |x - m|^2 with w = SIMPLIFY_RHO * trace(A) / 3: (A + w I) x = w m - b solved by
                  Cramer's rule through the six cofactors of the symmetric matrix.  The mean m is taken instead (a
                  ``fallback``) when the trace is not positive, x is not finite or some |x| component exceeds ``cell``;
                  ``position`` = "mean" always takes m.  representative = float32(centre + x); a cluster of one vertex keeps that
                  vertex's bits.
      faces       corners -> cluster ids.  A face with two equal ids is dropped (``degenerate``).  The others are compared
                  after rotating the smallest id to the front, which keeps the orientation: of faces with the same rotated triple
                  the first in input order is kept, the others are dropped (``duplicate``).  A face and its mirror image
                  (opposite orientation) are both kept, as Open3D keeps them.  The kept faces come out in input face order
                  with the input's corner order, each corner its cluster's representative.

    Two guarantees follow: every input vertex lies within 1.5 * ``cell`` of its cluster's representative per axis, up to the
    float32 rounding (half a cell to the centre, at most one from there), and when no two vertices share a cell and no input
    face has two equal indices the output is the input's soup, bit for bit, in the input's order.  Manifoldness and
    watertightness are NOT guaranteed: two sheets that pass through one cell are joined there.
    -> SimplifiedHost(triangles [kept,3,3] float32, cluster_of [V] int64, representatives [clusters,3] float32, kept [F] bool,
    fell_back [clusters] bool, counts dict(kept, clusters, degenerate, duplicate, fallbacks))."""
    _check_simplify_arguments(cell, position)
    o, h = _simplify_origin(origin), np.float64(cell)
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(v32), len(f)
    if V > SIMPLIFY_MAX_VERTICES:
        raise ValueError("simplify_mesh: %d vertices exceed the limit of 2^21" % V)
    if F and (f.min() < 0 or f.max() >= V):
        raise ValueError("simplify_mesh: a face index lies outside the vertices")
    if V == 0 or F == 0:
        return SimplifiedHost(np.zeros((0, 3, 3), np.float32), np.zeros(V, np.int64), np.zeros((0, 3), np.float32),
                              np.zeros(F, bool), np.zeros(0, bool), dict(kept=0, clusters=0, degenerate=0, duplicate=0, fallbacks=0))
    x = v32.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        t = np.floor((x - o) / h)
        if not (np.all(np.isfinite(x)) and np.all((t >= 0.0) & (t < float(1 << SIMPLIFY_CELL_BITS)))):
            raise ValueError("simplify_mesh: a vertex is not finite or lies outside the 2^21 cells per axis of this grid")
    c = t.astype(np.int64)
    key = (c[:, 0] << (2 * SIMPLIFY_CELL_BITS)) | (c[:, 1] << SIMPLIFY_CELL_BITS) | c[:, 2]
    order = np.argsort(key, kind="stable")                           # cluster after cluster, members in ascending vertex index
    skey = key[order]
    head = np.concatenate([[True], skey[1:] != skey[:-1]])
    cid_sorted = np.cumsum(head) - 1
    cluster_of = np.empty(V, np.int64)
    cluster_of[order] = cid_sorted
    starts = np.flatnonzero(head)
    C = len(starts)
    counts = np.diff(np.concatenate([starts, [V]]))
    centre = o + (c[order[starts]].astype(np.float64) + 0.5) * h     # [C,3]
    mean = _sums_in_order(x[order] - centre[cid_sorted], starts, counts) / counts.astype(np.float64)[:, None]
    local = mean
    fell_back = np.zeros(C, bool)
    if position == "quadric":
        corner_cluster = cluster_of[f.reshape(-1)]
        iorder = np.argsort(corner_cluster, kind="stable")           # key cluster << bits | (3 face + corner), ascending
        icluster = corner_cluster[iorder]
        face = f[iorder // 3]
        ce = centre[icluster]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            p, q, r = x[face[:, 0]] - ce, x[face[:, 1]] - ce, x[face[:, 2]] - ce
            u, w = q - p, r - p
            n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
            n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
            n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
            length = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
            d = -((n0 * p[:, 0] + n1 * p[:, 1]) + n2 * p[:, 2])
            has_normal = (length > 0.0) & (length < np.inf)
            terms = np.stack([(n0 * n0) / length, (n0 * n1) / length, (n0 * n2) / length, (n1 * n1) / length, (n1 * n2) / length,
                              (n2 * n2) / length, (n0 * d) / length, (n1 * d) / length, (n2 * d) / length], axis=1)
            terms = np.where(has_normal[:, None], terms, 0.0)        # (s + 0.0 == s: a sum that starts at +0.0 is never -0.0)
            istarts = np.searchsorted(icluster, np.arange(C))
            icounts = np.bincount(corner_cluster, minlength=C)
            a00, a01, a02, a11, a12, a22, b0, b1, b2 = _sums_in_order(terms, istarts, icounts).T
            trace = (a00 + a11) + a22
            wt = (SIMPLIFY_RHO * trace) / 3.0
            M00, M11, M22, M01, M02, M12 = a00 + wt, a11 + wt, a22 + wt, a01, a02, a12
            m0, m1, m2 = mean.T
            r0, r1, r2 = wt * m0 - b0, wt * m1 - b1, wt * m2 - b2
            C00, C01, C02 = M11 * M22 - M12 * M12, M02 * M12 - M01 * M22, M01 * M12 - M02 * M11
            C11, C12, C22 = M00 * M22 - M02 * M02, M01 * M02 - M00 * M12, M00 * M11 - M01 * M01
            det = (M00 * C00 + M01 * C01) + M02 * C02
            y = np.stack([((C00 * r0 + C01 * r1) + C02 * r2) / det, ((C01 * r0 + C11 * r1) + C12 * r2) / det,
                          ((C02 * r0 + C12 * r1) + C22 * r2) / det], axis=1)
            ok = (trace > 0.0) & np.all(np.abs(y) <= h, axis=1)      # (False for NaN)
        local = np.where(ok[:, None], y, mean)
        fell_back = ~ok & (counts > 1)
    rep = (centre + local).astype(np.float32)
    single = counts == 1
    rep[single] = v32[order[starts[single]]]
    # faces
    g = cluster_of[f]
    a, b, cc = g[:, 0], g[:, 1], g[:, 2]
    degenerate = (a == b) | (b == cc) | (a == cc)
    first = np.where((a < b) & (a < cc), 0, np.where(b < cc, 1, 2))
    rows = np.arange(F)
    triple = (g[rows, first] << (2 * SIMPLIFY_CELL_BITS)) | (g[rows, (first + 1) % 3] << SIMPLIFY_CELL_BITS) | g[rows, (first + 2) % 3]
    good = np.flatnonzero(~degenerate)
    forder = good[np.argsort(triple[good], kind="stable")]           # equal triples in input face order
    ft = triple[forder]
    fhead = np.concatenate([[True], ft[1:] != ft[:-1]]) if len(ft) else np.zeros(0, bool)
    kept = np.zeros(F, bool)
    kept[forder[fhead]] = True
    out_counts = dict(kept=int(kept.sum()), clusters=int(C), degenerate=int(degenerate.sum()),
                      duplicate=int(len(good) - fhead.sum()), fallbacks=int(fell_back.sum()))
    return SimplifiedHost(rep[g[kept]], cluster_of, rep, kept, fell_back, out_counts)


def _simplified(triangles, cell, origin, position, n_faces, counts):
    mesh = SimpleMesh(triangles)
    mesh.simplification = MeshSimplification(float(cell), tuple(float(v) for v in origin), position, int(n_faces), counts["clusters"],
                                             counts["degenerate"], counts["duplicate"], counts["kept"], counts["fallbacks"])
    return mesh


@torch.no_grad()
def simplify_mesh(mesh, cell, origin=None, position="quadric"):
    """A new, lighter SimpleMesh: the vertices of ``mesh`` that share a cell of the uniform grid of edge ``cell`` through
    ``origin`` become one vertex - placed where the quadric error of the faces around them is smallest (``position`` =
    "quadric": keeps edges, corners and the volume better) or at their mean ("mean") - and the faces that collapse or repeat
    are dropped: the semantics are simplify_mesh_host's, the stand-in for Open3D's ``simplify_vertex_clustering`` /
    trimesh-side decimation.  ``origin`` None is the per-axis minimum of the vertices (exact in float32 on either path).  A face
    and its opposite-orientation twin are both kept, as Open3D keeps them.  Every input vertex lies within 1.5 ``cell`` per axis
    of the vertex that replaces it; a mesh whose vertices all have a cell of their own comes back bit for bit.  Manifoldness
    and watertightness are not guaranteed - coarse cells join sheets that pass through one cell: ``mesh_report`` of the result
    says what came out.  A GPU mesh stays in HBM (zs_mesh_simplify on the weld it carries or, if it has none yet, on one
    weld_mesh call whose result it then keeps; one small read-back at the end: the counts, the status word and the origin); a
    host mesh is computed in numpy.  The new mesh carries nothing from the old one - no weld, components, adjacency, normals or
    colours: simplify first, then colour - and one extra attribute, ``simplification`` (a MeshSimplification).  ValueError for
    a ``cell`` that is not finite and positive, an unknown ``position``, a vertex that is not finite or a grid finer than 2^21
    cells per axis over the mesh.  An empty mesh gives an empty mesh."""
    _check_simplify_arguments(cell, position)
    given = None if origin is None else _simplify_origin(origin)
    zero = dict(kept=0, clusters=0, degenerate=0, duplicate=0, fallbacks=0)
    if getattr(mesh, "device_triangles", None) is None:
        vertices, faces = mesh.vertices, mesh.faces
        if len(faces) == 0:
            return _simplified(np.zeros((0, 3, 3), np.float32), cell, np.zeros(3) if given is None else given, position, 0, zero)
        o = vertices.min(axis=0).astype(np.float64) if given is None else given
        done = simplify_mesh_host(vertices, faces, o, cell, position)
        return _simplified(done.triangles, cell, o, position, len(faces), done.counts)
    from .. import _lib
    lib = _lib.load()
    if mesh._device_weld is None:
        mesh._device_weld = weld_mesh(mesh.device_triangles, normals=True)
    vertices, faces = mesh._device_weld[0], mesh._device_weld[1]
    n, n_verts, dev = faces.shape[0], vertices.shape[0], vertices.device
    if n == 0 or n_verts == 0:
        return _simplified(torch.empty(0, 3, 3, dtype=torch.float32, device=dev), cell, np.zeros(3) if given is None else given,
                           position, n, zero)
    nbytes = lib.zs_mesh_simplify_scratch_bytes(n, n_verts)
    if nbytes == 0:
        raise _lib.ZeroShapeHipError("simplify_mesh: %d faces over %d vertices exceed the kernels' limits" % (n, n_verts))
    if given is None:
        o = vertices.amin(dim=0).to(torch.float64)                   # stays on the device: the kernels read it there
    else:
        o = torch.tensor(given, dtype=torch.float64, device=dev)
    room = torch.empty(n, 3, 3, dtype=torch.float32, device=dev)
    counts = torch.zeros(6, dtype=torch.int32, device=dev)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    with _lib.on(dev):
        _lib.check(lib.zs_mesh_simplify(_lib.ptr(vertices), _lib.ptr(faces), n, n_verts, _lib.ptr(o), float(cell),
                                        SIMPLIFY_POSITIONS.index(position), _lib.ptr(room), _lib.ptr(counts), _lib.ptr(scratch),
                                        _lib.current_stream_ptr(dev)), "zs_mesh_simplify")
        tail = torch.cat([o, counts.to(torch.float64)]).tolist()     # the one D2H, after everything is enqueued: 72 bytes
    kept, clusters, degenerate, duplicate, status, fallbacks = (int(v) for v in tail[3:])
    if status & 2:
        raise _lib.ZeroShapeHipError("zs_mesh_simplify: status %d (a face index outside the vertices)" % status)
    if status:
        raise ValueError("simplify_mesh: a vertex is not finite or lies outside the 2^21 cells per axis of this grid "
                         "(zs_mesh_simplify: status %d)" % status)
    return _simplified(room[:kept].clone(), cell, tail[:3], position, n,
                       dict(kept=kept, clusters=clusters, degenerate=degenerate, duplicate=duplicate, fallbacks=fallbacks))


# ---- exact point-to-mesh distance (csrc/mesh_distance.hip) ----

MESH_DISTANCE_STATUS_VERTEX, MESH_DISTANCE_STATUS_INDEX, MESH_DISTANCE_STATUS_QUERY = 1, 2, 4   # zs_mesh_distance: status bits


class MeshDistance(collections.namedtuple("MeshDistance", "sqdist face closest counts")):
    """What mesh_distance returns: ``sqdist`` [M] float64 (the squared distance of every point to the mesh), ``face`` [M] (the
    face that attains it, the lowest index among equals; -1 where there is none), ``closest`` [M,3] float64 (the closest point
    of that face; None unless asked for) and ``counts`` [5] int32 - the faces that were skipped, the points that are not finite,
    the status word and the number of (point, face) pairs that were evaluated as two 32-bit halves.  CUDA tensors for a GPU
    mesh (int32 faces, nothing has been read back), numpy arrays for a host mesh (int64 faces)."""
    __slots__ = ()

    def check(self):
        """Reads ``counts`` (for a GPU mesh the one device-to-host copy, 20 bytes) -> dict(skipped_faces, nonfinite_queries,
        status, pairs).  ZeroShapeHipError when the status word says that a face index lay outside the vertices - a weld
        never makes one."""
        words = [int(v) for v in (self.counts.tolist() if self.counts is not None else [0] * 5)]
        return _distance_counts(words)


def _distance_counts(words):
    skipped, bad, status, lo, hi = words
    if status & MESH_DISTANCE_STATUS_INDEX:
        from .. import _lib
        raise _lib.ZeroShapeHipError("zs_mesh_distance: status %d (a face index outside the vertices)" % status)
    return dict(skipped_faces=skipped, nonfinite_queries=bad, status=status, pairs=(lo & 0xffffffff) | ((hi & 0xffffffff) << 32))


def _valid_faces(vertices, faces):
    """-> (valid [F] bool, status): a face is valid when its three indices lie inside the vertices and its corners are finite."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = np.all((f >= 0) & (f < len(v32)), axis=1)
    finite = np.zeros(len(f), bool)
    finite[inside] = np.all(np.isfinite(v32[f[inside]]), axis=(1, 2))
    status = (MESH_DISTANCE_STATUS_INDEX if not inside.all() else 0) | (MESH_DISTANCE_STATUS_VERTEX if (inside & ~finite).any() else 0)
    return inside & finite, status


def _sub3(x, y):
    return x[0] - y[0], x[1] - y[1], x[2] - y[2]


def _dot3(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _cross3(x, y):
    return x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]


def _closest_on_faces(q, a, b, c, with_point=False):
    """The points q against the faces (a, b, c), each a triple of float64 component arrays that broadcast against each other
    (q [Q,1] and corners [1,F]: every pair; or all [Q]: row by row) -> d2, or (d2, the closest point as a triple): the formula of
    closest_point_on_mesh_host, operation for operation."""
    def segment(p0, p1, w):
        e = _sub3(p1, p0)
        t, l = _dot3(w, e), _dot3(e, e)
        inner = (t > 0.0) & (t < l)
        end = (t > 0.0) & ~inner
        s = t / l                                                    # (used only where 0 < t < l)
        point = tuple(np.where(inner, p0[k] + s * e[k], np.where(end, p1[k], p0[k])) for k in range(3))
        d = _sub3(q, point)
        return _dot3(d, d), point

    w = _sub3(q, a)
    best, point = segment(a, b, w)
    for p0, p1, w0 in ((a, c, w), (b, c, _sub3(q, b))):
        d2, other = segment(p0, p1, w0)
        closer = d2 < best
        best = np.where(closer, d2, best)
        if with_point:
            point = tuple(np.where(closer, other[k], point[k]) for k in range(3))
    u, v = _sub3(b, a), _sub3(c, a)
    n = _cross3(u, v)
    nn = _dot3(n, n)
    g, h = _dot3(_cross3(u, w), n), _dot3(_cross3(w, v), n)
    inside = (nn > 0.0) & (h >= 0.0) & (g >= 0.0) & (h + g <= nn)
    beta, gamma = h / nn, g / nn                                     # (used only where nn > 0)
    other = tuple((a[k] + beta * u[k]) + gamma * v[k] for k in range(3))
    d = _sub3(q, other)
    d2 = _dot3(d, d)
    closer = inside & (d2 < best)
    best = np.where(closer, d2, best)
    if with_point:
        return best, tuple(np.where(closer, other[k], point[k]) for k in range(3))
    return best


def closest_point_on_mesh_host(points, vertices, faces, block=1 << 18):
    """The definition of mesh_distance and the checker of zs_mesh_distance, in numpy: for every point q of ``points`` [M,3]
    float32 the lexicographic minimum over the valid faces f of (d2(q, f), f) on the indexed mesh ``vertices`` [V,3] float32,
    ``faces`` [F,3] - a brute force over all faces, ``block`` (point, face) pairs at a time.  A face is valid when its three
    indices lie inside the vertices and its corners are finite; the others are skipped and counted.  Everything is elementwise
    float64 in the order written, from the float32 corners a, b, c and the float32 point:

      segment(p0, p1)    e = p1 - p0, w = q - p0, t = (wx ex + wy ey) + wz ez, l = (ex ex + ey ey) + ez ez;  t <= 0: p0;  else
                         t >= l: p1 (the vertex's own bits);  else p0 + (t / l) e.  The denominator l is used only where
                         0 < t < l: an edge of length zero has t = 0 and gives p0.
      interior(a, b, c)  u = b - a, v = c - a, w = q - a, n = u x v, nn = (nx nx + ny ny) + nz nz, g = (u x w) . n,
                         h = (w x v) . n (dots added left to right, cross products as a_y b_z - a_z b_y and its rotations);
                         inside when nn > 0, h >= 0, g >= 0 and h + g <= nn; then the point is (a + (h / nn) u) + (g / nn) v.
                         The denominator nn is used only where nn > 0: a face of zero area has no interior candidate.
      d2                 d = q - point, d2 = (dx dx + dy dy) + dz dz.
      the face           segment(a, b), segment(a, c), segment(b, c), interior, in this order; a later candidate replaces an
                         earlier one only with a strictly smaller d2.

    The closest point of a triangle is the foot of the perpendicular where that falls inside and a point of the boundary
    otherwise, so the smallest candidate is the exact distance in each of the seven Voronoi regions.  A face with a
    zero-length edge is a segment, a face with three equal corners a point: no NaN arises from finite inputs.  A point at a
    vertex is at d2 = 0 exactly from every face around it: the lowest face index wins, as for a point on a shared edge or a
    duplicated face.  A point that is not finite gets (NaN, -1, NaN); without a valid face every other point gets
    (+inf, -1, NaN).  -> (sqdist [M] float64, face [M] int64, closest [M,3] float64, skipped_faces int)."""
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid, _ = _valid_faces(v32, f)
    index = np.flatnonzero(valid)
    corners = v32[f[index]].astype(np.float64)                       # [Fv,3,3]
    M = len(p32)
    sqdist, face, closest = np.full(M, np.inf), np.full(M, -1, np.int64), np.full((M, 3), np.nan)
    finite = np.all(np.isfinite(p32), axis=1)
    sqdist[~finite] = np.nan
    rows = np.flatnonzero(finite)
    chunk = 1024
    step = max(1, int(block) // chunk)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r0 in range(0, len(rows), chunk):
            sel = rows[r0:r0 + chunk]
            q64 = p32[sel].astype(np.float64)
            q = tuple(q64[:, k, None] for k in range(3))
            best, best_f = np.full(len(sel), np.inf), np.full(len(sel), -1, np.int64)
            lane = np.arange(len(sel))
            for f0 in range(0, len(index), step):
                tri = corners[f0:f0 + step]
                a, b, c = (tuple(tri[None, :, i, k] for k in range(3)) for i in range(3))
                d2 = _closest_on_faces(q, a, b, c)
                j = np.argmin(d2, axis=1)                            # the first of equal minima: the lowest face index
                d2 = d2[lane, j]
                closer = d2 < best                                   # strictly: an earlier block holds the lower indices
                best = np.where(closer, d2, best)
                best_f = np.where(closer, index[f0 + j], best_f)
            best_p = np.full((len(sel), 3), np.nan)
            if len(index):                                           # the closest point: the same formula on the winning face alone
                tri = v32[f[best_f]].astype(np.float64)
                a, b, c = (tuple(tri[:, i, k] for k in range(3)) for i in range(3))
                _, point = _closest_on_faces(tuple(q64[:, k] for k in range(3)), a, b, c, with_point=True)
                best_p = np.stack(point, axis=1)
            sqdist[sel], face[sel], closest[sel] = best, best_f, best_p
    return sqdist, face, closest, int(len(f) - len(index))


def mesh_distance_stats_host(sqdist):
    """The checker of zs_mesh_distance_stats: over d = sqrt(d2) of the entries of ``sqdist`` that are finite (the others are
    left out) -> (float64 [4]: the largest d, the mean d, the rms d = sqrt(sum d2 / n), n; the lowest index with the largest d).
    The sums are the kernel's sequence of float64 additions: element i goes to thread i mod 256, a thread adds its elements in
    ascending i, then the 256 partial sums are added in ascending thread - np.add.accumulate, which adds in index order, down
    the columns of a zero-padded [-1, 256] view and then along the row of partial sums.  Without a finite entry: NaN, NaN, NaN,
    0 and -1."""
    d2 = np.asarray(sqdist, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (d2 >= 0.0) & (d2 < np.inf)
        n = int(ok.sum())
        if n == 0:
            return np.array([np.nan, np.nan, np.nan, 0.0]), -1
        d = np.sqrt(np.where(ok, d2, 0.0))

        def total(x):
            padded = np.concatenate([np.where(ok, x, 0.0), np.zeros((-len(x)) % 256)]).reshape(-1, 256)
            return np.add.accumulate(np.add.accumulate(padded, axis=0)[-1])[-1]

        at = int(np.argmax(np.where(ok, d, -1.0)))                   # the first of equal maxima
        return np.array([d[at], total(d) / float(n), np.sqrt(total(d2) / float(n)), float(n)]), at


@torch.no_grad()
def mesh_distance(mesh, points, closest=False):
    """The exact distance from ``points`` [M,3] to the surface of ``mesh`` (a SimpleMesh): for every point the nearest face,
    the squared distance to it and, with ``closest``, the nearest point of it -> a MeshDistance.  The semantics are
    closest_point_on_mesh_host's: float64 arithmetic on the float32 vertices and points, the lowest face index among equal
    distances, a face of zero area a segment or a point, faces with a corner that is not finite skipped, (NaN, -1) for a point
    that is not finite and (+inf, -1) against an empty mesh.
    A GPU mesh is searched on the device (zs_mesh_distance: a uniform grid over the faces, walked ring by ring under a bound
    that only skips what is provably farther - the brute force's bits) on the weld it carries or, if it has none yet, on one
    weld_mesh call whose result it then keeps; ``points`` must then be a CUDA float32 tensor (ValueError otherwise), the results
    are CUDA tensors and nothing is read back: ``MeshDistance.check()`` reads the counts and raises ZeroShapeHipError for a
    status word that reports a face index outside the vertices.  A host mesh goes through the numpy checker."""
    if getattr(mesh, "device_triangles", None) is None:
        if isinstance(points, torch.Tensor):
            points = points.detach().cpu().numpy()
        p32 = np.asarray(points, np.float32).reshape(-1, 3)
        vertices, faces = mesh.vertices, mesh.faces
        sq, face, point, skipped = closest_point_on_mesh_host(p32, vertices, faces)
        valid, status = _valid_faces(vertices, faces)
        bad = int((~np.all(np.isfinite(p32), axis=1)).sum())
        pairs = int(valid.sum()) * (len(p32) - bad)
        counts = np.array([skipped, bad, status | (MESH_DISTANCE_STATUS_QUERY if bad else 0), pairs & 0xffffffff, pairs >> 32],
                          np.int64).astype(np.uint32).view(np.int32)
        return MeshDistance(sq, face, point if closest else None, counts)
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        raise ValueError("mesh_distance: a GPU mesh needs its points as a CUDA tensor")
    from .. import _lib
    lib = _lib.load()
    if mesh._device_weld is None:
        mesh._device_weld = weld_mesh(mesh.device_triangles, normals=True)
    vertices, faces = mesh._device_weld[0], mesh._device_weld[1]
    dev = vertices.device
    pts = points.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    n, n_verts, m = faces.shape[0], vertices.shape[0], pts.shape[0]
    sq = torch.empty(m, dtype=torch.float64, device=dev)
    face = torch.empty(m, dtype=torch.int32, device=dev)
    point = torch.empty(m, 3, dtype=torch.float64, device=dev) if closest else None
    counts = torch.zeros(5, dtype=torch.int32, device=dev)
    if m == 0:
        return MeshDistance(sq, face, point, counts)
    nbytes = lib.zs_mesh_distance_scratch_bytes(n, m)
    if nbytes == 0:
        raise _lib.ZeroShapeHipError("mesh_distance: %d faces and %d points exceed the kernels' limits" % (n, m))
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    with _lib.on(dev):
        _lib.check(lib.zs_mesh_distance(_lib.ptr(vertices), _lib.ptr(faces), n, n_verts, _lib.ptr(pts), m, _lib.ptr(sq),
                                        _lib.ptr(face), _lib.ptr(point), _lib.ptr(counts), _lib.ptr(scratch),
                                        _lib.current_stream_ptr(dev)), "zs_mesh_distance")
    return MeshDistance(sq, face, point, counts)


MeshDeviation = collections.namedtuple(
    "MeshDeviation", "forward_max forward_mean forward_rms forward_index forward_vertices "
                     "backward_max backward_mean backward_rms backward_index backward_vertices cell_edge")
MeshDeviation.__doc__ = """What mesh_deviation measured between a mesh and the reference it was made from, in mesh units.  ``forward``:
the distances of the vertices of the mesh to the surface of the reference - the largest, the mean, the root mean square, the
index of the vertex (a row of ``mesh.vertices``) where the largest is attained (the lowest among equals) and the number of
vertices.  ``backward``: the same for the vertices of the reference against the surface of the mesh (the index is a row of
``reference.vertices``).  ``cell_edge``: None, or the edge of a marching-cubes cell in mesh units when the pipelines made the
record - mesh_report then also gives the distances in cells.  The record is VERTEX-SAMPLED: each maximum is a lower bound on
the one-sided Hausdorff distance of the two surfaces (the largest distance may be attained inside a face), not the continuous
Hausdorff distance; the distances themselves are exact."""


def _deviation_record(forward, forward_at, backward, backward_at, cell_edge):
    return MeshDeviation(float(forward[0]), float(forward[1]), float(forward[2]), int(forward_at), int(forward[3]),
                         float(backward[0]), float(backward[1]), float(backward[2]), int(backward_at), int(backward[3]),
                         None if cell_edge is None else float(cell_edge))


@torch.no_grad()
def mesh_deviation(mesh, reference, cell_edge=None):
    """How far the surface of ``mesh`` lies from the surface of ``reference`` (two SimpleMesh, both on the GPU or both on the
    host; typically a smoothed or simplified mesh and the mesh it was made from) -> a MeshDeviation: max, mean and rms of the
    exact distances of the vertices of ``mesh`` to the surface of ``reference`` (forward) and of the vertices of ``reference``
    to the surface of ``mesh`` (backward), with the vertex at each maximum.  Vertex-sampled: a bound from the vertices, not the
    continuous Hausdorff distance (see MeshDeviation).  On the GPU: two mesh_distance calls and two zs_mesh_distance_stats
    calls on the welds the meshes carry (made and kept where missing), then ONE small read-back - the two records and the
    two status words; on the host closest_point_on_mesh_host and mesh_distance_stats_host, the kernels' checkers, which give
    the same numbers bit for bit.  A side without vertices, or against an empty mesh, gives NaN, NaN, NaN, -1 and 0."""
    on_device = getattr(mesh, "device_triangles", None) is not None
    if on_device != (getattr(reference, "device_triangles", None) is not None):
        raise ValueError("mesh_deviation: both meshes must live on the GPU or both on the host")
    if not on_device:
        sides = []
        for source, target in ((mesh, reference), (reference, mesh)):
            done = mesh_distance(target, source.vertices)
            done.check()
            sides.extend(mesh_distance_stats_host(done.sqdist))
        return _deviation_record(*sides, cell_edge=cell_edge)
    from .. import _lib
    lib = _lib.load()
    for m in (mesh, reference):
        if m._device_weld is None:
            m._device_weld = weld_mesh(m.device_triangles, normals=True)
    dev = mesh.device_triangles.device
    tail = []
    for source, target in ((mesh, reference), (reference, mesh)):
        done = mesh_distance(target, source._device_weld[0])
        out = torch.tensor([float("nan")] * 3 + [0.0], dtype=torch.float64, device=dev)
        at = torch.full((1,), -1, dtype=torch.int32, device=dev)
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_distance_stats(_lib.ptr(done.sqdist), done.sqdist.shape[0], _lib.ptr(out), _lib.ptr(at),
                                                  _lib.current_stream_ptr(dev)), "zs_mesh_distance_stats")
        tail += [out, at.to(torch.float64), done.counts.to(torch.float64)]
    f, f_at, f_counts, b, b_at, b_counts = (t.tolist() for t in torch.cat(tail).split([4, 1, 5, 4, 1, 5]))      # the one D2H
    for words in (f_counts, b_counts):
        _distance_counts([int(v) for v in words])
    return _deviation_record(f, f_at[0], b, b_at[0], cell_edge)


# ---- on which side of a mesh a point lies (csrc/mesh_inside.hip) ----


class MeshWinding(collections.namedtuple("MeshWinding", "up down counts")):
    """What mesh_winding returns: ``up`` [M] int32 and ``down`` [M] int32, the signed crossing numbers of the +z and the -z ray
    from every point (for a closed mesh wound like marching cubes' both are the winding number: 1 in a solid, 0 outside and in
    a cavity, 2 where two solids overlap, -1 in a solid wound the other way; ``up != down`` marks a point as AMBIGUOUS - the
    mesh is open along the point's column, or the point lies on the surface), and ``counts`` [5] int32 as MeshDistance's: the
    faces that were skipped, the points that are not finite, the status word and the number of (point, face) pairs that were
    read as two 32-bit halves.  CUDA tensors for a GPU mesh (nothing has been read back), numpy arrays for a host mesh."""
    __slots__ = ()

    def check(self):
        """Reads ``counts`` (for a GPU mesh the one device-to-host copy, 20 bytes) -> dict(skipped_faces, nonfinite_queries,
        status, pairs).  ZeroShapeHipError when the status word says that a face index lay outside the vertices - a weld
        never makes one."""
        return _winding_counts([int(v) for v in self.counts.tolist()])


def _winding_counts(words, who="zs_mesh_winding"):
    skipped, bad, status, lo, hi = words[:5]
    if status & MESH_DISTANCE_STATUS_INDEX:
        from .. import _lib
        raise _lib.ZeroShapeHipError("%s: status %d (a face index outside the vertices)" % (who, status))
    return dict(skipped_faces=skipped, nonfinite_queries=bad, status=status, pairs=(lo & 0xffffffff) | ((hi & 0xffffffff) << 32))


def _edge_side_host(u, v, qx, qy):
    """The sign (float64 -1, 0, 1) of the side of (qx, qy) against the directed edge u -> v (triples of float64 arrays), ties
    broken by the symbolic shift: mesh_winding_host's step 2, operation for operation."""
    forward = (u[0] < v[0]) | ((u[0] == v[0]) & ((u[1] < v[1]) | ((u[1] == v[1]) & (u[2] <= v[2]))))     # walks lo -> hi
    lx, ly = np.where(forward, u[0], v[0]), np.where(forward, u[1], v[1])
    hx, hy = np.where(forward, v[0], u[0]), np.where(forward, v[1], u[1])
    ex, ey = hx - lx, hy - ly
    s = ex * (qy - ly) - ey * (qx - lx)
    s = np.sign(np.where(s == 0.0, np.where(ey != 0.0, -np.sign(ey), np.sign(ex)), s))
    return np.where(forward, s, -s)


def mesh_winding_host(points, vertices, faces, block=1 << 22):
    """The definition of mesh_winding and the checker of zs_mesh_winding, in numpy: for every point q of ``points`` [M,3]
    float32 the signed crossing numbers of the +z ray (up) and of the -z ray (down) over the valid faces of the indexed mesh
    ``vertices`` [V,3] float32, ``faces`` [F,3] - every point against every face, ``block`` (point, face) pairs at a time.  A
    face is valid when its three indices lie inside the vertices and its corners are finite; the others are skipped and
    counted.  A point that is not finite gets (0, 0) and is counted.  Everything is elementwise float64 in the order written,
    from the float32 corners a, b, c and the float32 point:

      box        the face is a candidate only if min(ax, bx, cx) <= qx <= max(ax, bx, cx) and the same in y (the float32
                 values themselves).  It excludes no face that lies over q; as a part of the definition it makes pruning by
                 boxes exact by construction.
      side       of each directed edge u -> v (a -> b, b -> c, c -> a): (lo, hi) = the endpoints ordered lexicographically by
                 their (x, y, z) values - not indices: a soup, a weld of it and duplicated vertices give a shared edge the same
                 number;  s = (hx - lx) (qy - ly) - (hy - ly) (qx - lx);  where s == 0: s = -sign(hy - ly) if hy != ly, else
                 sign(hx - lx) (0 when the edge projects to a point);  negated when the face walks the edge hi -> lo.  The tie
                 rule is a symbolic shift of q by (eps, eps^2) in x, y: a ray never meets a projected edge or vertex, and a
                 face that projects to a segment never contains q.
      facing     up-facing over q when the three sides are > 0, down-facing when they are < 0; otherwise it does not count.
      height     A = a - q, B = b - q, C = c - q, det = (Ax (By Cz - Bz Cy) + Ay (Bz Cx - Bx Cz)) + Az (Bx Cy - By Cx);
                 det == 0 counts for neither ray.
      counts     up = #(up-facing, det > 0) - #(down-facing, det < 0);  down = #(down-facing, det > 0) - #(up-facing, det < 0).

    For a closed mesh wound like marching cubes' (positive ``volume``) both equal the winding number; a point is inside when
    up != 0, and up != down marks it ambiguous (see MeshWinding).  Nothing here repairs open meshes.
    -> (up [M] int32, down [M] int32, counts [5] int32: skipped faces, points that are not finite, the status word of
    mesh_distance, and valid faces x finite points - the pairs of a scan over all faces - as two 32-bit halves)."""
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid, status = _valid_faces(v32, f)
    corners32 = v32[f[valid]]                                        # [Fv,3,3]
    corners = corners32.astype(np.float64)
    lo32, hi32 = corners32[:, :, :2].min(axis=1), corners32[:, :, :2].max(axis=1)
    M = len(p32)
    up, down = np.zeros(M, np.int32), np.zeros(M, np.int32)
    finite = np.all(np.isfinite(p32), axis=1)
    rows = np.flatnonzero(finite)
    chunk = max(1, int(block) // max(len(corners), 1))
    with np.errstate(over="ignore", invalid="ignore"):
        for r0 in range(0, len(rows) if len(corners) else 0, chunk):
            sel = rows[r0:r0 + chunk]
            qx32, qy32 = p32[sel, 0, None], p32[sel, 1, None]
            box = (lo32[None, :, 0] <= qx32) & (qx32 <= hi32[None, :, 0]) & (lo32[None, :, 1] <= qy32) & (qy32 <= hi32[None, :, 1])
            qi, fi = np.nonzero(box)                                 # the candidates, pair by pair from here on
            q = p32[sel[qi]].astype(np.float64)
            a, b, c = (tuple(corners[fi, k, j] for j in range(3)) for k in range(3))
            sides = [_edge_side_host(u, v, q[:, 0], q[:, 1]) for u, v in ((a, b), (b, c), (c, a))]
            faces_up = (sides[0] > 0) & (sides[1] > 0) & (sides[2] > 0)
            faces_down = (sides[0] < 0) & (sides[1] < 0) & (sides[2] < 0)
            A, B, C = (tuple(x[j] - q[:, j] for j in range(3)) for x in (a, b, c))
            det = (A[0] * (B[1] * C[2] - B[2] * C[1]) + A[1] * (B[2] * C[0] - B[0] * C[2])) + A[2] * (B[0] * C[1] - B[1] * C[0])
            above, below = det > 0.0, det < 0.0
            for out, plus, minus in ((up, faces_up & above, faces_down & below), (down, faces_down & above, faces_up & below)):
                term = plus.astype(np.int64) - minus.astype(np.int64)
                out[sel] = np.bincount(qi, weights=term, minlength=len(sel)).astype(np.int32)
    bad = int(M - len(rows))
    pairs = int(valid.sum()) * len(rows)
    counts = np.array([len(f) - int(valid.sum()), bad, status | (MESH_DISTANCE_STATUS_QUERY if bad else 0), pairs & 0xffffffff,
                       pairs >> 32], np.int64).astype(np.uint32).view(np.int32)
    return up, down, counts


def _device_weld_of(mesh):
    if mesh._device_weld is None:
        mesh._device_weld = weld_mesh(mesh.device_triangles, normals=True)
    return mesh._device_weld[0], mesh._device_weld[1]


def _winding_scratch(lib, n_faces, n_queries, dev, who):
    from .. import _lib
    nbytes = lib.zs_mesh_winding_scratch_bytes(n_faces, n_queries)
    if nbytes == 0:
        raise _lib.ZeroShapeHipError("%s: %d faces and %d points exceed the kernels' limits" % (who, n_faces, n_queries))
    return torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)


@torch.no_grad()
def mesh_winding(mesh, points):
    """On which side of the surface of ``mesh`` (a SimpleMesh) the ``points`` [M,3] lie: the signed crossing numbers of the
    +z and the -z ray from every point -> a MeshWinding.  The semantics are mesh_winding_host's: float64 arithmetic on the
    float32 vertices and points, a symbolic shift of the point where a ray would meet an edge or a vertex, faces with a corner
    that is not finite skipped, (0, 0) for a point that is not finite.  Exact, and meaningful for meshes that are open, folded
    or overlapping: an open mesh gives ambiguous points (``up != down``) instead of a wrong answer.
    A GPU mesh is searched on the device (zs_mesh_winding: a uniform grid of columns over x, y that skips only faces whose box
    does not contain the point - the brute force's integers) on the weld it carries or, if it has none yet, on one weld_mesh
    call whose result it then keeps; ``points`` must then be a CUDA float32 tensor (ValueError otherwise), the results are
    CUDA tensors and nothing is read back: ``MeshWinding.check()`` reads the counts.  A host mesh goes through the numpy
    checker."""
    if getattr(mesh, "device_triangles", None) is None:
        if isinstance(points, torch.Tensor):
            points = points.detach().cpu().numpy()
        return MeshWinding(*mesh_winding_host(points, mesh.vertices, mesh.faces))
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        raise ValueError("mesh_winding: a GPU mesh needs its points as a CUDA tensor")
    from .. import _lib
    lib = _lib.load()
    vertices, faces = _device_weld_of(mesh)
    dev = vertices.device
    pts = points.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    n, n_verts, m = faces.shape[0], vertices.shape[0], pts.shape[0]
    up = torch.empty(m, dtype=torch.int32, device=dev)
    down = torch.empty(m, dtype=torch.int32, device=dev)
    counts = torch.zeros(5, dtype=torch.int32, device=dev)
    if m == 0:
        return MeshWinding(up, down, counts)
    scratch = _winding_scratch(lib, n, m, dev, "mesh_winding")
    with _lib.on(dev):
        _lib.check(lib.zs_mesh_winding(_lib.ptr(vertices), _lib.ptr(faces), n, n_verts, _lib.ptr(pts), m, _lib.ptr(up),
                                       _lib.ptr(down), _lib.ptr(counts), _lib.ptr(scratch), _lib.current_stream_ptr(dev)),
                   "zs_mesh_winding")
    return MeshWinding(up, down, counts)


def mesh_contains(mesh, points):
    """trimesh's ``contains``: whether each of ``points`` [M,3] lies inside ``mesh`` - mesh_winding(mesh, points).up != 0 ->
    [M] bool, a CUDA tensor for a GPU mesh (nothing is read back), a numpy array for a host mesh.  A point on the surface or
    under a hole gets the answer of its +z ray; mesh_winding tells which points those are."""
    return mesh_winding(mesh, points).up != 0


def mesh_signed_distance(mesh, points, closest=False):
    """The signed distance from ``points`` [M,3] to the surface of ``mesh``: sqrt(sqdist) of mesh_distance, negative where
    mesh_winding's ``up`` != 0 (inside: the usual sign of a signed distance field) -> [M] float64, or with ``closest`` the pair
    (signed distance, the nearest point of the surface [M,3] float64).  A point that is not finite keeps NaN and every point
    against an empty mesh keeps +inf.  CUDA tensors for a GPU mesh - two searches, the sign applied on the device, nothing
    read back - and numpy arrays for a host mesh."""
    done = mesh_distance(mesh, points, closest=closest)
    inside = mesh_winding(mesh, points).up != 0
    if isinstance(done.sqdist, torch.Tensor):
        d = torch.sqrt(done.sqdist)
        signed = torch.where(inside, -d, d)
    else:
        with np.errstate(invalid="ignore"):
            d = np.sqrt(done.sqdist)
        signed = np.where(inside, -d, d)
    return (signed, done.closest) if closest else signed


def _lattice_host(G, scale, offset):
    """The G^3 lattice points of zs_mesh_winding_grid, x slowest: fmaf(i, scale, offset) per axis in float32."""
    axis = _fma32(np.arange(G, dtype=np.float32), np.full(G, scale, np.float32), np.full(G, offset, np.float32))
    return np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)


@torch.no_grad()
def mesh_occupancy_grid(mesh, G, scale, offset):
    """The inverse of marching cubes: the occupancy of ``mesh`` on the G^3 lattice whose point (ix, iy, iz) lies at
    fmaf(i, scale, offset) per axis in float32 - the formula marching cubes uses for its vertices, so with
    scale = (range_max - range_min) / G and offset = range_min a mesh is tested on the lattice it was made on.
    -> (inside [G,G,G] int8, x slowest: mesh_winding's ``up`` != 0 at every lattice point; counts [6] int32: MeshWinding's
    five words and the number of ambiguous points).  A GPU mesh makes the lattice in the kernel (zs_mesh_winding_grid) on the
    weld it carries or makes and keeps; the results are CUDA tensors and nothing is read back.  A host mesh goes through the
    numpy checker."""
    G = int(G)
    if G < 0:
        raise ValueError("mesh_occupancy_grid: G must not be negative, got %d" % G)
    scale, offset = float(np.float32(scale)), float(np.float32(offset))
    if getattr(mesh, "device_triangles", None) is None:
        up, down, counts = mesh_winding_host(_lattice_host(G, scale, offset), mesh.vertices, mesh.faces)
        return (up != 0).astype(np.int8).reshape(G, G, G), np.append(counts, np.int32((up != down).sum()))
    from .. import _lib
    lib = _lib.load()
    vertices, faces = _device_weld_of(mesh)
    dev = vertices.device
    inside = torch.empty(G, G, G, dtype=torch.int8, device=dev)
    counts = torch.zeros(6, dtype=torch.int32, device=dev)
    if G == 0:
        return inside, counts
    if G > 645:
        raise _lib.ZeroShapeHipError("mesh_occupancy_grid: G = %d exceeds the kernels' limit (G^3 <= 2^28)" % G)
    n, n_verts = faces.shape[0], vertices.shape[0]
    scratch = _winding_scratch(lib, n, G ** 3, dev, "mesh_occupancy_grid")
    with _lib.on(dev):
        _lib.check(lib.zs_mesh_winding_grid(_lib.ptr(vertices), _lib.ptr(faces), n, n_verts, G, scale, offset, _lib.ptr(inside),
                                            _lib.ptr(counts), _lib.ptr(scratch), _lib.current_stream_ptr(dev)),
                   "zs_mesh_winding_grid")
    return inside, counts


MeshVolumeIoU = collections.namedtuple(
    "MeshVolumeIoU", "inside inside_reference both either iou ambiguous ambiguous_reference cell_volume")
MeshVolumeIoU.__doc__ = """What mesh_volume_iou counted on a lattice: the lattice points inside the mesh (``inside``), inside the reference
(``inside_reference``), inside both and inside either; ``iou`` = both / either (NaN when either is 0); the lattice points
whose two rays disagreed (``ambiguous`` for the mesh, ``ambiguous_reference`` for the reference: points on the surface, or
under a hole of an open mesh - counted, not repaired); and ``cell_volume`` = scale^3, so that a count times it approximates a
volume in mesh units.  The record is LATTICE-SAMPLED: counts of lattice points, not integrals over the solids."""


@torch.no_grad()
def mesh_volume_iou(mesh, reference, G, scale, offset):
    """The volume intersection-over-union of ``mesh`` and ``reference`` (two SimpleMesh, both on the GPU or both on the host;
    typically a smoothed or simplified mesh and the mesh it was made from), LATTICE-SAMPLED: the occupancies of both meshes on
    the G^3 lattice of mesh_occupancy_grid are counted, not the solids integrated -> a MeshVolumeIoU.  Unlike the signed sum
    behind ``mesh.volume`` the occupancy is meaningful for meshes that are open, folded or overlapping; the record says how
    many lattice points were ambiguous.  On the GPU: two zs_mesh_winding_grid calls and one zs_occupancy_counts call on the
    welds the meshes carry (made and kept where missing), then ONE small read-back - the four counts and the two count
    records; on the host the numpy checker, which gives the same integers."""
    on_device = getattr(mesh, "device_triangles", None) is not None
    if on_device != (getattr(reference, "device_triangles", None) is not None):
        raise ValueError("mesh_volume_iou: both meshes must live on the GPU or both on the host")
    a, counts_a = mesh_occupancy_grid(mesh, G, scale, offset)
    b, counts_b = mesh_occupancy_grid(reference, G, scale, offset)
    if not on_device:
        x, y = a != 0, b != 0
        totals = [int(x.sum()), int(y.sum()), int((x & y).sum()), int((x | y).sum())]
        words_a, words_b = counts_a.tolist(), counts_b.tolist()
    else:
        from .. import _lib
        lib = _lib.load()
        dev = a.device
        out = torch.zeros(4, dtype=torch.int64, device=dev)
        with _lib.on(dev):
            _lib.check(lib.zs_occupancy_counts(_lib.ptr(a), _lib.ptr(b), a.numel(), _lib.ptr(out), _lib.current_stream_ptr(dev)),
                       "zs_occupancy_counts")
        tail = torch.cat([out, counts_a.to(torch.int64), counts_b.to(torch.int64)]).tolist()               # the one D2H
        totals, words_a, words_b = tail[:4], tail[4:10], tail[10:]
    for words in (words_a, words_b):
        _winding_counts([int(v) for v in words], "zs_mesh_winding_grid")
    inside, inside_reference, both, either = (int(v) for v in totals)
    return MeshVolumeIoU(inside, inside_reference, both, either, both / float(either) if either else float("nan"),
                         int(words_a[5]), int(words_b[5]), float(np.float32(scale)) ** 3)


# ---- where a ray first meets a mesh (csrc/mesh_rays.hip) ----


class MeshRays(collections.namedtuple("MeshRays", "t face side bary counts")):
    """What mesh_ray_cast returns: ``t`` [N] float64 (the ray parameter of the first hit: the point is o + t d; +inf for a
    miss, NaN for an invalid ray), ``face`` [N] int32 (the face that is hit, the lowest index among equal t; -1 without a
    hit), ``side`` [N] int8 (+1: the ray meets the face against its normal (b - a) x (c - a), from outside on a marching-cubes
    mesh; -1: from behind; 0 without a hit), ``bary`` [N,3] float64 (the weights of the face's corners a, b, c at the hit, NaN
    without one; None unless asked for) and ``counts`` [5] int32 as MeshDistance's - the faces that were skipped, the rays that
    are invalid, the status word and the number of (ray, face) pairs that were read as two 32-bit halves.  CUDA tensors for a
    GPU mesh (nothing has been read back), numpy arrays for a host mesh.  ``mesh`` is the mesh that was cast against."""
    mesh = None

    def check(self):
        """Reads ``counts`` (for a GPU mesh the one device-to-host copy, 20 bytes) -> dict(skipped_faces, nonfinite_queries,
        status, pairs).  ZeroShapeHipError when the status word says that a face index lay outside the vertices - a weld
        never makes one."""
        return _winding_counts([int(v) for v in self.counts.tolist()], "zs_mesh_rays")

    def points(self):
        """The hit points [N,3] float64 from the weights, (wa a + wb b) + wc c per component on the mesh's welded corners
        (NaN rows without a hit) - on the device for a GPU mesh, nothing is read back.  Needs ``bary``."""
        if self.bary is None:
            raise ValueError("MeshRays.points needs the weights: cast with bary=True")
        if isinstance(self.t, torch.Tensor):
            vertices, faces = _device_weld_of(self.mesh)
            hit = self.face >= 0
            corners = vertices.to(torch.float64)[faces.long()[self.face.clamp(min=0).long()]] if faces.shape[0] else \
                torch.zeros(self.face.shape[0], 3, 3, dtype=torch.float64, device=self.face.device)
            w = self.bary
            p = (w[:, 0, None] * corners[:, 0] + w[:, 1, None] * corners[:, 1]) + w[:, 2, None] * corners[:, 2]
            return torch.where(hit[:, None], p, torch.full_like(p, float("nan")))
        vertices, faces = self.mesh.vertices, self.mesh.faces
        hit = self.face >= 0
        corners = vertices.astype(np.float64)[faces[np.maximum(self.face, 0)]] if len(faces) else np.zeros((len(self.face), 3, 3))
        w = self.bary
        with np.errstate(invalid="ignore"):
            p = (w[:, 0, None] * corners[:, 0] + w[:, 1, None] * corners[:, 1]) + w[:, 2, None] * corners[:, 2]
        return np.where(hit[:, None], p, np.nan)


def _ray_frames(o32, d32):
    """-> (ok [N] bool, K [N,3] int: the axes kx, ky, kz of every ray, S [N,3] float64: Sx, Sy, Sz) - mesh_rays_host's
    'per ray' step.  Invalid rays get the frame of +z."""
    ok = np.all(np.isfinite(o32), axis=1) & np.all(np.isfinite(d32), axis=1) & np.any(d32 != 0.0, axis=1)
    d = np.where(ok[:, None], d32, np.float32([0.0, 0.0, 1.0])).astype(np.float64)
    kz = np.argmax(np.abs(d), axis=1)                                # the first of the largest
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    rows = np.arange(len(d))
    dz = d[rows, kz]
    kx, ky = np.where(dz < 0.0, ky, kx), np.where(dz < 0.0, kx, ky)
    with np.errstate(over="ignore"):
        S = np.stack([d[rows, kx] / dz, d[rows, ky] / dz, 1.0 / dz], axis=1)
    return ok, np.stack([kx, ky, kz], axis=1), S


def mesh_rays_host(origins, directions, vertices, faces, t_min=0.0, t_max=np.inf, bary=False, block=1 << 19):
    """The definition of mesh_ray_cast and the checker of zs_mesh_rays, in numpy: for every ray (o, d) of ``origins`` and
    ``directions`` [N,3] float32 the first face it meets on the indexed mesh ``vertices`` [V,3] float32, ``faces`` [F,3] - every
    ray against every valid face, ``block`` (ray, face) pairs at a time.  A face is valid when its three indices lie inside the
    vertices and its corners are finite; the others are skipped and counted.  A ray is invalid when a component of o or d is
    not finite or d = 0: it gets (NaN, -1, 0) and is counted.  The test is the watertight one of Woop, Benthin and Wald (2013);
    everything is elementwise float64 in the order written, from the float32 corners a, b, c and the float32 ray:

      per ray    kz = the first axis with the largest |d|, kx = (kz + 1) mod 3, ky = (kx + 1) mod 3; kx and ky are swapped when
                 d[kz] < 0;  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
      per face   A = a - o;  Ax = A[kx] - (Sx A[kz]), Ay = A[ky] - (Sy A[kz]), Az = Sz A[kz];  the same for B = b - o and
                 C = c - o;  U = (Cx By) - (Cy Bx), V = (Ax Cy) - (Ay Cx), W = (Bx Ay) - (By Ax);  det = (U + V) + W;
                 t = (((U Az) + (V Bz)) + (W Cz)) / det.
      hit        iff (U >= 0 and V >= 0 and W >= 0) or (U <= 0 and V <= 0 and W <= 0), det != 0, t_min <= t <= t_max (edges
                 and both ends of the range inclusive) and |t| < inf.  The last is a guard: |A| < 2^129 and |Sx|, |Sy| <= 1
                 keep U, V, W below 2^262 and |Sz| <= 2^149 keeps the numerator below 2^542, but a det that cancels to its
                 last bits can make the quotient overflow for inputs that span the whole float32 range; such a face is not
                 hit, so that +inf stays the mark of a miss.  An intermediate that overflows on the way (inf - inf = NaN)
                 fails the comparisons and is not hit either.
      result     the smallest t wins, among equal t the lowest face index.  side = +1 where det > 0, -1 where det < 0: with
                 d = +z the frame is (x, y, z) and det = -((b - a) x (c - a))_z, so det > 0 means that the ray runs AGAINST
                 the normal - from outside on a mesh wound like marching cubes'; the swap keeps that reading for d[kz] < 0.
                 The weights of (a, b, c) are U / det, V / det, W / det.

    Watertight: the sheared corner (Ax, Ay) depends on the corner and the ray only, so the two faces at a shared edge compute
    edge functions that are exact negatives of each other: a ray through a shared edge or a vertex hits at least one of the
    faces around it.  A ray in the plane of a face, or a face without area, has det = 0 and is not hit.
    -> (t [N] float64: +inf for a miss, NaN for an invalid ray; face [N] int32: -1; side [N] int8: 0; bary [N,3] float64 with
    NaN rows, or None without ``bary``; counts [5] int32: skipped faces, invalid rays, the status word of mesh_distance, and
    valid faces x valid rays - the pairs of a scan over all faces - as two 32-bit halves)."""
    o32 = np.asarray(origins, np.float32).reshape(-1, 3)
    d32 = np.asarray(directions, np.float32).reshape(-1, 3)
    if len(o32) != len(d32):
        raise ValueError("mesh_rays_host: %d origins and %d directions" % (len(o32), len(d32)))
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t_min, t_max = np.float64(t_min), np.float64(t_max)
    valid, status = _valid_faces(v32, f)
    index = np.flatnonzero(valid)
    corners = v32[f[index]].astype(np.float64)                       # [Fv,3,3]
    N = len(o32)
    ok, K, S = _ray_frames(o32, d32)
    t_out = np.where(ok, np.inf, np.nan)
    face_out, side_out = np.full(N, -1, np.int32), np.zeros(N, np.int8)
    bary_out = np.full((N, 3), np.nan) if bary else None
    rows = np.flatnonzero(ok)
    chunk = max(1, int(block) // max(len(corners), 1))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r0 in range(0, len(rows) if len(corners) else 0, chunk):
            sel = rows[r0:r0 + chunk]
            k, s = K[sel], S[sel]
            o = np.take_along_axis(o32[sel].astype(np.float64), k, axis=1)              # [r,3]: o[kx], o[ky], o[kz]
            P = corners[:, :, k].transpose(2, 0, 1, 3) - o[:, None, None, :]            # [r,Fv,corner,(kx ky kz)]: A, B, C
            X = P[..., 0] - s[:, 0, None, None] * P[..., 2]
            Y = P[..., 1] - s[:, 1, None, None] * P[..., 2]
            Z = s[:, 2, None, None] * P[..., 2]
            Ax, Bx, Cx = X[..., 0], X[..., 1], X[..., 2]
            Ay, By, Cy = Y[..., 0], Y[..., 1], Y[..., 2]
            U = Cx * By - Cy * Bx
            V = Ax * Cy - Ay * Cx
            W = Bx * Ay - By * Ax
            det = (U + V) + W
            t = ((U * Z[..., 0] + V * Z[..., 1]) + W * Z[..., 2]) / det
            hit = (((U >= 0.0) & (V >= 0.0) & (W >= 0.0)) | ((U <= 0.0) & (V <= 0.0) & (W <= 0.0))) & (det != 0.0) \
                & (t >= t_min) & (t <= t_max) & (np.abs(t) < np.inf)
            t = np.where(hit, t, np.inf)
            j = np.argmin(t, axis=1)                                 # the first of equal minima: the lowest face index
            lane = np.arange(len(sel))
            got = hit[lane, j]
            t_out[sel] = t[lane, j]
            face_out[sel] = np.where(got, index[j], -1)
            side_out[sel] = np.where(got, np.where(det[lane, j] > 0.0, 1, -1), 0)
            if bary:
                w = np.stack([U[lane, j], V[lane, j], W[lane, j]], axis=1) / det[lane, j, None]
                bary_out[sel] = np.where(got[:, None], w, np.nan)
    bad = int(N - len(rows))
    pairs = int(valid.sum()) * len(rows)
    counts = np.array([len(f) - int(valid.sum()), bad, status | (MESH_DISTANCE_STATUS_QUERY if bad else 0), pairs & 0xffffffff,
                       pairs >> 32], np.int64).astype(np.uint32).view(np.int32)
    return t_out, face_out, side_out, bary_out, counts


def camera_rays_host(intr, mean, scale, H, W):
    """The rays of zs_mesh_rays_image, in numpy: one ray per pixel of an H x W pinhole camera with the intrinsics ``intr``
    [3,3] float32, in the frame of a mesh that was normalised by (``mean`` [3], ``scale``) float32 - v = (X - mean) / scale for a
    camera point X.  Pixel (row i, col j) is at (j, i, 1), camera.get_pixel_grid's and mesh_vertex_colors_host's convention.
    Float64 in the order written, from the float32 values K = intr:

      c00 = K11 K22 - K12 K21,  c01 = K02 K21 - K01 K22,  c02 = K01 K12 - K02 K11
      c10 = K12 K20 - K10 K22,  c11 = K00 K22 - K02 K20,  c12 = K02 K10 - K00 K12
      c20 = K10 K21 - K11 K20,  c21 = K01 K20 - K00 K21,  c22 = K00 K11 - K01 K10      (the adjugate)
      det = (K00 c00 + K01 c10) + K02 c20
      D_r = ((c_r0 j + c_r1 i) + c_r2) / det  for r = x, y, z:  D = K^-1 (j, i, 1)
      o = -mean / scale;  d = ((Dx / Dz) / scale, (Dy / Dz) / scale, 1 / scale)

    both rounded to float32.  A pixel whose Dz is not > 0 and finite gets d = NaN - an invalid ray.  With D / Dz the third
    component of the camera point o + t d is t itself: the ray parameter is the camera depth Z, up to the rounding of o and d.
    -> (origins [H*W,3] float32, directions [H*W,3] float32), pixel (i, j) in row i W + j."""
    K = np.asarray(intr, np.float32).reshape(3, 3).astype(np.float64)
    mu = np.asarray(mean, np.float32).reshape(3).astype(np.float64)
    s = np.float64(np.asarray(scale, np.float32).reshape(-1)[0])
    H, W = int(H), int(W)
    n = H * W
    pj = (np.arange(n) % max(W, 1)).astype(np.float64)
    pi = (np.arange(n) // max(W, 1)).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = [[K[1, 1] * K[2, 2] - K[1, 2] * K[2, 1], K[0, 2] * K[2, 1] - K[0, 1] * K[2, 2], K[0, 1] * K[1, 2] - K[0, 2] * K[1, 1]],
             [K[1, 2] * K[2, 0] - K[1, 0] * K[2, 2], K[0, 0] * K[2, 2] - K[0, 2] * K[2, 0], K[0, 2] * K[1, 0] - K[0, 0] * K[1, 2]],
             [K[1, 0] * K[2, 1] - K[1, 1] * K[2, 0], K[0, 1] * K[2, 0] - K[0, 0] * K[2, 1], K[0, 0] * K[1, 1] - K[0, 1] * K[1, 0]]]
        det = (K[0, 0] * c[0][0] + K[0, 1] * c[1][0]) + K[0, 2] * c[2][0]
        D = [((c[r][0] * pj + c[r][1] * pi) + c[r][2]) / det for r in range(3)]
        forward = (D[2] > 0.0) & (D[2] < np.inf)
        d = np.stack([(D[0] / D[2]) / s, (D[1] / D[2]) / s, np.full(n, 1.0 / s)], axis=1)
        d = np.where(forward[:, None], d, np.nan).astype(np.float32)
        o = np.broadcast_to((-mu / s).astype(np.float32), (n, 3)).copy()
    return o, d


def _rays_scratch(lib, n_faces, n_rays, dev, who):
    from .. import _lib
    nbytes = lib.zs_mesh_rays_scratch_bytes(n_faces, n_rays)
    if nbytes == 0:
        raise _lib.ZeroShapeHipError("%s: %d faces and %d rays exceed the kernels' limits" % (who, n_faces, n_rays))
    return torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)


@torch.no_grad()
def mesh_ray_cast(mesh, origins, directions, t_min=0.0, t_max=float("inf"), bary=False):
    """trimesh's ``ray.intersects_first`` / ``intersects_location``: where the rays o + t d (``origins``, ``directions`` [N,3],
    t_min <= t <= t_max) first meet the surface of ``mesh`` (a SimpleMesh) -> a MeshRays: the parameter, the face, the side
    the ray came from and, with ``bary``, the weights of the face's corners (``MeshRays.points()`` makes the hit points of
    them).  The semantics are mesh_rays_host's: the watertight test in float64 on the float32 vertices and rays, edges and
    both ends of the range inclusive, the lowest face index among equal t, faces with a corner that is not finite skipped,
    (NaN, -1, 0) for a ray that is not finite or has no direction.  Directions need not be normalised: t counts in units of |d|.
    A GPU mesh is searched on the device (zs_mesh_rays: a uniform grid over the faces, walked slab by slab along the ray under
    bounds that only skip what the test cannot hit - the brute force's bits) on the weld it carries or, if it has none yet, on
    one weld_mesh call whose result it then keeps; the rays must then be CUDA float32 tensors (ValueError otherwise), the
    results are CUDA tensors and nothing is read back: ``MeshRays.check()`` reads the counts.  A host mesh goes through the
    numpy checker."""
    if getattr(mesh, "device_triangles", None) is None:
        o, d = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (origins, directions))
        out = MeshRays(*mesh_rays_host(o, d, mesh.vertices, mesh.faces, t_min, t_max, bary))
        out.mesh = mesh
        return out
    for x in (origins, directions):
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise ValueError("mesh_ray_cast: a GPU mesh needs its rays as CUDA tensors")
    from .. import _lib
    lib = _lib.load()
    vertices, faces = _device_weld_of(mesh)
    dev = vertices.device
    o = origins.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    d = directions.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    if o.shape[0] != d.shape[0]:
        raise ValueError("mesh_ray_cast: %d origins and %d directions" % (o.shape[0], d.shape[0]))
    n, n_verts, m = faces.shape[0], vertices.shape[0], o.shape[0]
    t = torch.empty(m, dtype=torch.float64, device=dev)
    face = torch.empty(m, dtype=torch.int32, device=dev)
    side = torch.empty(m, dtype=torch.int8, device=dev)
    weights = torch.empty(m, 3, dtype=torch.float64, device=dev) if bary else None
    counts = torch.zeros(5, dtype=torch.int32, device=dev)
    if m:
        scratch = _rays_scratch(lib, n, m, dev, "mesh_ray_cast")
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_rays(_lib.ptr(vertices), _lib.ptr(faces), n, n_verts, _lib.ptr(o), _lib.ptr(d), m, float(t_min),
                                        float(t_max), _lib.ptr(t), _lib.ptr(face), _lib.ptr(side), _lib.ptr(weights),
                                        _lib.ptr(counts), _lib.ptr(scratch), _lib.current_stream_ptr(dev)), "zs_mesh_rays")
    out = MeshRays(t, face, side, weights, counts)
    out.mesh = mesh
    return out


class MeshDepthMap(collections.namedtuple("MeshDepthMap", "depth face side counts")):
    """What mesh_depth_map returns: ``depth`` [H,W] float32 (the camera depth Z of the first surface along the pixel's ray:
    (float)t of mesh_rays_host on camera_rays_host's rays; +inf where the ray misses, NaN for an invalid pixel), ``face``
    [H,W] int32 and ``side`` [H,W] int8 as MeshRays', and ``counts`` [6] int32: MeshRays' five words and the number of pixels
    that hit.  CUDA tensors for a GPU mesh (nothing has been read back), numpy arrays for a host mesh."""
    __slots__ = ()

    def check(self):
        """Reads ``counts`` -> dict(skipped_faces, nonfinite_queries, status, pairs, hit_pixels); ZeroShapeHipError as
        MeshRays.check()."""
        words = [int(v) for v in self.counts.tolist()]
        return dict(_winding_counts(words, "zs_mesh_rays_image"), hit_pixels=words[5])


def _camera_host(intr, mean, scale):
    return tuple(np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float32) for x in (intr, mean, scale))


@torch.no_grad()
def mesh_depth_map(mesh, intr, mean, scale, H, W, t_min=0.0, t_max=float("inf")):
    """The image of ``mesh`` in a pinhole camera: for every pixel of an H x W image the depth of the first surface, the face and
    the side -> a MeshDepthMap.  ``intr`` [3,3], ``mean`` [3] and ``scale`` (one value) are the camera and the normalisation
    of the mesh frame - one sample of var.intr_pred and of camera.seen_surface's (mean, scale); the rays and their semantics
    are camera_rays_host's and mesh_rays_host's.  A GPU mesh makes the rays in the kernel (zs_mesh_rays_image) on the weld it
    carries or makes and keeps; the camera must then be CUDA tensors (ValueError otherwise), the results are CUDA tensors and
    nothing is read back.  A host mesh goes through the numpy checkers."""
    H, W = int(H), int(W)
    if H < 0 or W < 0:
        raise ValueError("mesh_depth_map: H and W must not be negative, got %d x %d" % (H, W))
    if getattr(mesh, "device_triangles", None) is None:
        o, d = camera_rays_host(*_camera_host(intr, mean, scale), H, W)
        t, face, side, _, counts = mesh_rays_host(o, d, mesh.vertices, mesh.faces, t_min, t_max)
        with np.errstate(over="ignore"):
            depth = t.astype(np.float32)
        return MeshDepthMap(depth.reshape(H, W), face.reshape(H, W), side.reshape(H, W), np.append(counts, np.int32((face >= 0).sum())))
    tensors = dict(intr=intr, mean=mean, scale=scale)
    for name, x in tensors.items():
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise ValueError("mesh_depth_map: a GPU mesh needs %s as a CUDA tensor" % name)
    intr, mean, scale = [_gpu_f32(tensors[k], k) for k in ("intr", "mean", "scale")]
    if intr.numel() != 9 or mean.numel() != 3 or scale.numel() != 1:
        raise ValueError("mesh_depth_map: intr must hold 9 values, mean 3 and scale 1")
    from .. import _lib
    lib = _lib.load()
    vertices, faces = _device_weld_of(mesh)
    dev = vertices.device
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    face = torch.empty(H, W, dtype=torch.int32, device=dev)
    side = torch.empty(H, W, dtype=torch.int8, device=dev)
    counts = torch.zeros(6, dtype=torch.int32, device=dev)
    if H * W:
        n, n_verts = faces.shape[0], vertices.shape[0]
        scratch = _rays_scratch(lib, n, H * W, dev, "mesh_depth_map")
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_rays_image(_lib.ptr(vertices), _lib.ptr(faces), n, n_verts, _lib.ptr(intr), _lib.ptr(mean),
                                              _lib.ptr(scale), H, W, float(t_min), float(t_max), _lib.ptr(depth), _lib.ptr(face),
                                              _lib.ptr(side), _lib.ptr(counts), _lib.ptr(scratch), _lib.current_stream_ptr(dev)),
                       "zs_mesh_rays_image")
    return MeshDepthMap(depth, face, side, counts)


MeshReprojection = collections.namedtuple(
    "MeshReprojection", "mask_pixels mesh_pixels both either silhouette_iou depth_pixels depth_max depth_mean depth_rms "
                        "depth_max_pixel depth_max_mesh depth_mean_mesh depth_rms_mesh depth_max_cells depth_mean_cells "
                        "depth_rms_cells agreeing back_faces depth_tol scale cell_edge")
MeshReprojection.__doc__ = """What mesh_reprojection measured between a mesh and the photo it was predicted from, in the input camera.  With R
the pixels whose ray hits the mesh and M the pixels of the mask (> 0.5): ``mask_pixels`` = |M|, ``mesh_pixels`` = |R|, ``both``,
``either`` and ``silhouette_iou`` = both / either (NaN when either is 0).  Over the ``depth_pixels`` pixels of M and R whose
predicted depth is finite and positive: ``depth_max``, ``depth_mean`` and ``depth_rms`` of |Z_mesh - depth| in camera units (NaN
without such a pixel), ``depth_max_pixel`` the (row, col) where the largest is attained (the first in row order; None
without one), the same three in mesh units (``*_mesh``: / scale) and, when ``cell_edge`` is known, in marching-cubes cells
(``*_cells``, else None).  ``agreeing``: the pixels among them with |Z_mesh - depth| <= depth_tol scale (``depth_tol`` in mesh
units).  ``back_faces``: the pixels of R whose first hit has side -1 - the camera is inside the mesh, or the mesh is open
towards it.  ``scale``: the normalisation's.  The record is PIXEL-SAMPLED: one ray through each pixel's centre."""


def _reprojection_record(counts4, stats, at, agreeing, back_faces, depth_tol, scale, cell_edge, W):
    mask_pixels, mesh_pixels, both, either = (int(v) for v in counts4)
    n = int(stats[3])
    mx, mean, rms = (float(v) for v in stats[:3])
    scale = float(scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        in_mesh = [float(np.float64(v) / np.float64(scale)) for v in (mx, mean, rms)]
        in_cells = [None] * 3 if cell_edge is None else [float(np.float64(v) / np.float64(cell_edge)) for v in in_mesh]
    pixel = None if int(at) < 0 else (int(at) // int(W), int(at) % int(W))
    return MeshReprojection(mask_pixels, mesh_pixels, both, either, both / float(either) if either else float("nan"), n, mx, mean,
                            rms, pixel, in_mesh[0], in_mesh[1], in_mesh[2], in_cells[0], in_cells[1], in_cells[2], int(agreeing),
                            int(back_faces), float(depth_tol), scale, None if cell_edge is None else float(cell_edge))


def mesh_reprojection_host(vertices, faces, mask, depth, intr, mean, scale, depth_tol, cell_edge=None):
    """The definition of mesh_reprojection and its checker, in numpy on mesh_rays_host: ``mask`` and ``depth`` hold H x W
    float32 values (``mask`` gives H and W), the camera is camera_rays_host's.  Z_mesh = float32(t) of the pixel's ray (what
    mesh_depth_map stores), R = the pixels that hit, M = mask > 0.5, the depth pixels = M and R and depth finite and > 0;
    e = |float64(Z_mesh) - float64(depth)|; max, mean and rms = mesh_distance_stats_host of e e (the kernel's summation
    order); agreeing = #(e <= float64(depth_tol) float64(scale)); back_faces = #(side = -1).  -> a MeshReprojection."""
    msk = np.asarray(mask, np.float32)
    msk = msk.reshape(msk.shape[-2:])
    H, W = msk.shape
    dep = np.asarray(depth, np.float32).reshape(H, W)
    K, mu, s = (np.asarray(x, np.float32) for x in (intr, mean, scale))
    o, d = camera_rays_host(K, mu, s, H, W)
    t, face, side, _, _ = mesh_rays_host(o, d, vertices, faces)
    with np.errstate(over="ignore", invalid="ignore"):
        z = t.astype(np.float32).reshape(H, W)
        R, M = (face >= 0).reshape(H, W), msk > np.float32(0.5)
        use = M & R & np.isfinite(dep) & (dep > 0.0)
        e = np.abs(z.astype(np.float64) - dep.astype(np.float64))
        sq = np.where(use, e * e, np.nan).reshape(-1)
        stats, at = mesh_distance_stats_host(sq)
        tol = np.float64(depth_tol) * np.float64(s.reshape(-1)[0])
        agreeing = int((use & (e <= tol)).sum())
    return _reprojection_record([M.sum(), R.sum(), (M & R).sum(), (M | R).sum()], stats, at, agreeing, int((side == -1).sum()),
                                depth_tol, s.reshape(-1)[0], cell_edge, W)


@torch.no_grad()
def mesh_reprojection(mesh, mask, depth, intr, mean, scale, depth_tol, cell_edge=None, depth_map=None):
    """A ground-truth-free score of a predicted mesh: its image in the input camera against the input mask and the predicted
    depth -> a MeshReprojection (the semantics: mesh_reprojection_host).  ``mask`` and ``depth`` hold H x W values (one sample
    of var.mask_input_map and var.depth_pred), ``intr``, ``mean``, ``scale`` as for mesh_depth_map, ``depth_tol`` in mesh units,
    ``cell_edge`` the edge of a marching-cubes cell in mesh units when the distances are wanted in cells too.  On the GPU:
    mesh_depth_map (or ``depth_map``, a MeshDepthMap of the same camera made before), zs_occupancy_counts on the two
    silhouettes, zs_mesh_distance_stats on the squared differences, then ONE small read-back; a host mesh goes through the
    numpy checker, which gives the same numbers bit for bit."""
    if getattr(mesh, "device_triangles", None) is None:
        args = [x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (mask, depth, intr, mean, scale)]
        return mesh_reprojection_host(mesh.vertices, mesh.faces, *args, depth_tol=depth_tol, cell_edge=cell_edge)
    tensors = dict(mask=mask, depth=depth, intr=intr, mean=mean, scale=scale)
    for name, x in tensors.items():
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise ValueError("mesh_reprojection: a GPU mesh needs %s as a CUDA tensor" % name)
    mask, depth, scale = _gpu_f32(mask, "mask"), _gpu_f32(depth, "depth"), _gpu_f32(scale, "scale")
    if mask.dim() < 2 or depth.numel() != mask.numel():
        raise ValueError("mesh_reprojection: mask must be [..,H,W] and depth must hold as many values")
    H, W = int(mask.shape[-2]), int(mask.shape[-1])
    if mask.numel() != H * W:
        raise ValueError("mesh_reprojection: one sample at a time, got a mask of shape %s" % (tuple(mask.shape),))
    from .. import _lib
    lib = _lib.load()
    image = mesh_depth_map(mesh, intr, mean, scale, H, W) if depth_map is None else depth_map
    dev = image.depth.device
    mask, depth = mask.reshape(H, W).to(dev), depth.reshape(H, W).to(dev)
    R, M = image.face >= 0, mask > 0.5
    use = M & R & torch.isfinite(depth) & (depth > 0.0)
    e = (image.depth.to(torch.float64) - depth.to(torch.float64)).abs()
    sq = torch.where(use, e * e, torch.full_like(e, float("nan"))).reshape(-1).contiguous()
    tol = float(depth_tol) * scale.reshape(-1)[0].to(device=dev, dtype=torch.float64)
    a, b = R.to(torch.int8).contiguous(), M.to(torch.int8).contiguous()
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    stats = torch.tensor([float("nan")] * 3 + [0.0], dtype=torch.float64, device=dev)
    at = torch.full((1,), -1, dtype=torch.int32, device=dev)
    with _lib.on(dev):
        _lib.check(lib.zs_occupancy_counts(_lib.ptr(b), _lib.ptr(a), H * W, _lib.ptr(totals), _lib.current_stream_ptr(dev)),
                   "zs_occupancy_counts")
        _lib.check(lib.zs_mesh_distance_stats(_lib.ptr(sq), H * W, _lib.ptr(stats), _lib.ptr(at), _lib.current_stream_ptr(dev)),
                   "zs_mesh_distance_stats")
    more = torch.stack([(use & (e <= tol)).sum(), (image.side == -1).sum()]).to(torch.float64)
    tail = torch.cat([totals.to(torch.float64), stats, at.to(torch.float64), more, scale.reshape(-1)[:1].to(dev, torch.float64),
                      image.counts.to(torch.float64)]).tolist()                                      # the one D2H
    _winding_counts([int(v) for v in tail[12:17]], "zs_mesh_rays_image")
    return _reprojection_record(tail[:4], tail[4:8], tail[8], tail[9], tail[10], depth_tol, tail[11], cell_edge, W)


def reprojection(opt, var, meshes=None, depth_tol=None):
    """mesh_reprojection for every mesh of the batch (``meshes``, default ``var.mesh_pred``) with sample b of
    ``var.mask_input_map``, ``var.depth_pred`` and ``var.intr_pred`` (``var.intr`` when there is no prediction); (mean, scale)
    come from camera.seen_surface on ``var.depth_pred``, as in vertex_colors.  ``depth_tol`` defaults to
    default_color_depth_tol(opt); the record knows the marching-cubes cell edge.  Sets ``mesh.reprojection`` (the record) and
    ``mesh.depth_map`` (the MeshDepthMap it was made from, on the device).  -> meshes."""
    from . import camera
    meshes = var.mesh_pred if meshes is None else meshes
    intr = var.intr_pred if getattr(var, "intr_pred", None) is not None else var.intr
    _, _, _, mean, scale = camera.seen_surface(opt, var.depth_pred, intr, var.mask_input_map)
    depth_tol = default_color_depth_tol(opt) if depth_tol is None else depth_tol
    for b, mesh in enumerate(meshes):
        mask, depth = var.mask_input_map[b], var.depth_pred[b]
        mesh.depth_map = mesh_depth_map(mesh, intr[b], mean[b], scale[b:b + 1], int(mask.shape[-2]), int(mask.shape[-1]))
        mesh.reprojection = mesh_reprojection(mesh, mask, depth, intr[b], mean[b], scale[b:b + 1], depth_tol,
                                              cell_edge=_mc_cell_edge(opt), depth_map=mesh.depth_map)
    return meshes


def reprojection_option(opt):
    """Whether ``--eval.mesh_reprojection=true`` is set (opt-in, command line only: no yaml file carries it).  It scores the
    prediction itself, so it needs no smoothing or simplification."""
    return bool(opt.eval.get("mesh_reprojection", False))


# ---- which faces pass through each other (csrc/mesh_selfx.hip) ----


class MeshSelfIntersections(collections.namedtuple("MeshSelfIntersections", "face_counts pairs counts")):
    """What mesh_self_intersections returns: ``face_counts`` [F] (for every face the number of other faces it crosses),
    ``pairs`` [n,2] (the crossing pairs (i, j), i < j, in lexicographic order - the first ``capacity`` of them when a capacity
    was given, rows beyond the total left at -1; None unless asked for) and ``counts`` [9] int32: the faces that were skipped,
    the status word, the crossing pairs as two 32-bit halves, the coincident pairs as two halves, the faces with a count > 0
    and the ordered candidate pairs that were examined as two halves.  CUDA int32 tensors for a GPU mesh (nothing has been
    read back), numpy arrays for a host mesh (int64 counts and pairs).  Coincident pairs - two faces on the same three
    corner positions, either orientation - are the one coplanar contact that is counted, apart from the crossings; touching,
    coplanar overlap and the contact of faces that share a vertex or an edge are neither.  Nothing is repaired."""
    __slots__ = ()

    def check(self):
        """Reads ``counts`` (for a GPU mesh the one device-to-host copy, 36 bytes) -> dict(n_pairs, n_coincident,
        n_faces_crossed, skipped_faces, status, examined, truncated: whether ``pairs`` holds fewer rows than there are
        pairs).  ZeroShapeHipError when the status word says that a face index lay outside the vertices - a weld never makes
        one."""
        w = [int(v) & 0xffffffff for v in self.counts.tolist()]
        if w[1] & MESH_DISTANCE_STATUS_INDEX:
            from .. import _lib
            raise _lib.ZeroShapeHipError("zs_mesh_self_intersections: status %d (a face index outside the vertices)" % w[1])
        n_pairs = w[2] | (w[3] << 32)
        return dict(n_pairs=n_pairs, n_coincident=w[4] | (w[5] << 32), n_faces_crossed=w[6], skipped_faces=w[0], status=w[1],
                    examined=w[7] | (w[8] << 32), truncated=self.pairs is not None and int(self.pairs.shape[0]) < n_pairs)


def _lex_before(u, v):
    """u before v in the lexicographic order of the values (triples of component arrays)."""
    return (u[0] < v[0]) | ((u[0] == v[0]) & ((u[1] < v[1]) | ((u[1] == v[1]) & (u[2] < v[2]))))


def _choose3(first, u, v):
    return tuple(np.where(first, u[k], v[k]) for k in range(3))


def _det3(D, L, H):
    return (D[0] * (L[1] * H[2] - L[2] * H[1]) + D[1] * (L[2] * H[0] - L[0] * H[2])) + D[2] * (L[0] * H[1] - L[1] * H[0])


def _edges_cross_host(S, T):
    """Whether an edge of the faces S crosses the faces T, row by row: S and T are triples of corners, each a triple of
    float64 component arrays [N] - mesh_self_intersections_host's segment rule, operation for operation."""
    a, b, c = T
    side = [_det3(_sub3(a, x), _sub3(b, x), _sub3(c, x)) for x in S]
    out = np.zeros(len(a[0]), bool)
    for k0, k1 in ((0, 1), (1, 2), (2, 0)):
        ss, st = side[k0], side[k1]
        at = np.flatnonzero(((ss > 0.0) & (st < 0.0)) | ((ss < 0.0) & (st > 0.0)))
        if len(at) == 0:
            continue
        s, t = tuple(x[at] for x in S[k0]), tuple(x[at] for x in S[k1])
        fa, fb, fc = (tuple(x[at] for x in corner) for corner in T)
        swap = _lex_before(t, s)
        p, q = _choose3(swap, t, s), _choose3(swap, s, t)
        D = _sub3(q, p)
        e = []
        for u, v in ((fa, fb), (fb, fc), (fc, fa)):
            down = _lex_before(v, u)                                 # the face walks the edge hi -> lo
            lo, hi = _choose3(down, v, u), _choose3(down, u, v)
            value = _det3(D, _sub3(lo, p), _sub3(hi, p))
            e.append(np.where(down, -value, value))
        out[at] |= (((e[0] >= 0.0) & (e[1] >= 0.0) & (e[2] >= 0.0)) | ((e[0] <= 0.0) & (e[1] <= 0.0) & (e[2] <= 0.0))) & \
            ~((e[0] == 0.0) & (e[1] == 0.0) & (e[2] == 0.0))
    return out


def mesh_self_intersections_host(vertices, faces, rows=None, pairs=False):
    """The definition of mesh_self_intersections and the checker of zs_mesh_self_intersections, in numpy: every face of
    ``rows`` (default: all) against every face of the indexed mesh ``vertices`` [V,3] float32, ``faces`` [F,3].  A face is
    valid when its three indices lie inside the vertices and its corners are finite; the others are skipped, counted, and
    cross nothing.  Everything is elementwise float64 in the order written, from the float32 corners of two valid faces
    i != j:

      candidates   only if the float32 boxes overlap on every axis, ends included: min_i <= max_j and min_j <= max_i.  The
                   box test is part of the definition (as in mesh_winding_host), so pruning by boxes is exact by construction.
      det(D, L, H) = (Dx (Ly Hz - Lz Hy) + Dy (Lz Hx - Lx Hz)) + Dz (Lx Hy - Ly Hx), mesh_winding_host's grouping.
      a segment crosses the face (a, b, c): (p, q) = its ends ordered lexicographically by their (x, y, z) values;
                   sp = det(a - p, b - p, c - p) and sq = det(a - q, b - q, c - q) strictly of opposite signs; D = q - p; for
                   each directed edge u -> v of a -> b, b -> c, c -> a: (lo, hi) = u, v ordered by value,
                   e = det(D, lo - p, hi - p), negated when the face walks hi -> lo; the three e all >= 0 or all <= 0, and
                   not all three 0.
      S, T cross   iff an edge of S crosses T or an edge of T crosses S (symmetric).
      coincident   iff the three corner positions of S are those of T in some order, by value: either orientation, so a
                   mirror twin is one coincident pair (the unordered triples are compared: the degenerate faces (a, a, b)
                   and (a, b, b) are not coincident).

    What follows: an end that equals a corner of the face makes a zero row, so its det is exactly 0 - faces that share a
    vertex or an edge are never reported for that contact, on a soup, on any weld and with duplicated vertices alike, with no
    special case; a face that pokes through a neighbour it shares one vertex with is still found, through the opposite edge.
    Touching is not crossing (a vertex lying in another face has det 0), coplanar overlap and a coplanar fold across a shared
    edge are not crossing (every det 0): coincident pairs are the one coplanar case that is counted, separately.  A face of
    zero area has a plane that nothing crosses, but its edges can cross others.  An edge function depends on the segment and
    the ordered edge alone, so the two faces at an edge compute exact negatives: a segment through a shared edge crosses at
    least one of them.
    -> (face_counts [R] int64: for every row the number of other faces it crosses; pairs [n,2] int64, the crossing (i, j)
    with i in ``rows`` and j > i in lexicographic order - all crossing pairs for the default rows - or None; a dict:
    crossing_pairs and coincident_pairs (both over i in ``rows``, j > i), faces_crossed (rows with a count > 0),
    skipped_faces and status (the whole mesh), candidates (the (i, j), i in ``rows``, j != i, whose boxes overlap) and
    brute_force (the ordered pairs of a row with another valid face))."""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid, status = _valid_faces(v32, f)
    F = len(f)
    rows = np.arange(F, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).reshape(-1)
    corners = np.zeros((F, 3, 3), np.float32)
    corners[valid] = v32[f[valid]]
    mn, mx = corners.min(axis=1), corners.max(axis=1)
    index = np.flatnonzero(valid)
    face_counts = np.zeros(len(rows), np.int64)
    found, n_coincident, n_candidates = [], 0, 0
    # only to be quick: the valid faces and the rows in the order of their box minimum along x.  The rows of a chunk then
    # see the faces whose minimum lies in [smallest minimum of the chunk - widest box, largest maximum of the chunk]: a face
    # outside begins beyond every row's end or ends before every row's beginning.  The box test below decides.
    index = index[np.argsort(mn[index, 0], kind="stable")]
    start_x = mn[index, 0].astype(np.float64)
    widest = float((mx[index, 0].astype(np.float64) - start_x).max()) * (1.0 + 2.0 ** -40) if len(index) else 0.0   # (rounding)
    order = np.flatnonzero(valid[rows])
    order = order[np.argsort(mn[rows[order], 0], kind="stable")]                         # positions in rows
    chunk = 512
    with np.errstate(over="ignore", invalid="ignore"):
        for r0 in range(0, len(order), chunk):
            where = order[r0:r0 + chunk]
            r = rows[where]
            j0 = np.searchsorted(start_x, float(mn[r, 0].min()) - widest, side="left")
            j1 = np.searchsorted(start_x, float(mx[r, 0].max()), side="right")
            window = index[j0:j1]
            near = (mn[r, None, 0] <= mx[None, window, 0]) & (mn[None, window, 0] <= mx[r, None, 0])
            ri, jj = np.nonzero(near)
            i, j = r[ri], window[jj]
            keep = i != j
            for k in (1, 2):
                keep &= (mn[i, k] <= mx[j, k]) & (mn[j, k] <= mx[i, k])
            ri, i, j = ri[keep], i[keep], j[keep]
            n_candidates += len(i)
            S64, T64 = corners[i].astype(np.float64), corners[j].astype(np.float64)
            S = tuple(tuple(S64[:, c, k] for k in range(3)) for c in range(3))
            T = tuple(tuple(T64[:, c, k] for k in range(3)) for c in range(3))
            crossing = _edges_cross_host(S, T) | _edges_cross_host(T, S)
            m = np.all(S64[:, :, None, :] == T64[:, None, :, :], axis=3)                 # [N, corner of S, corner of T]
            twins = np.zeros(len(i), bool)
            for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
                twins |= m[:, 0, perm[0]] & m[:, 1, perm[1]] & m[:, 2, perm[2]]
            n_coincident += int((twins & (j > i)).sum())
            face_counts += np.bincount(where[ri[crossing]], minlength=len(rows))
            above = crossing & (j > i)
            found.append(np.stack([i[above], j[above]], axis=1))
    found = np.concatenate(found) if found else np.zeros((0, 2), np.int64)
    found = found[np.lexsort((found[:, 1], found[:, 0]))]
    n_rows_valid = int(valid[rows].sum())
    record = dict(crossing_pairs=len(found), coincident_pairs=n_coincident, faces_crossed=int((face_counts > 0).sum()),
                  skipped_faces=int(F - len(index)), status=int(status), candidates=int(n_candidates),
                  brute_force=n_rows_valid * max(len(index) - 1, 0))
    return face_counts, (found if pairs else None), record


def _check_capacity(capacity):
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0):
        raise ValueError("mesh_self_intersections: capacity must be an integer >= 0 or None, got %r" % (capacity,))


@torch.no_grad()
def mesh_self_intersections(mesh, pairs=False, capacity=None):
    """Open3D's ``is_self_intersecting`` / ``get_self_intersecting_triangles``: which faces of ``mesh`` (a SimpleMesh) pass
    through each other -> a MeshSelfIntersections: per face the number of other faces it crosses, with ``pairs`` the
    crossing pairs (i, j), i < j, in lexicographic order, and the counts.  The semantics are mesh_self_intersections_host's:
    float64 arithmetic on the float32 corners, boxes that overlap as part of the definition, strict sides - touching,
    coplanar overlap and the contact of neighbours are not crossings; coincident pairs are counted apart.
    A GPU mesh is searched on the device (zs_mesh_self_intersections: a uniform grid over the faces read through integer
    reaches that skip no candidate - the counts of the test of all pairs) on the weld it carries or, if it has none yet, on
    one weld_mesh call whose result it then keeps; the results are CUDA tensors and nothing is read back:
    ``MeshSelfIntersections.check()`` reads the counts.  With ``capacity`` the pair list has that many rows (the first ones;
    rows beyond the total stay -1; ``check()["truncated"]`` says whether some are missing).  With ``pairs`` and NO capacity
    the call SYNCHRONISES: one counting call, a read of the 8-byte total, then the call that writes exactly that many rows.
    A host mesh goes through the numpy checker."""
    _check_capacity(capacity)
    want_pairs = bool(pairs) or capacity is not None
    if getattr(mesh, "device_triangles", None) is None:
        face_counts, found, rec = mesh_self_intersections_host(mesh.vertices, mesh.faces, pairs=True)
        examined = rec["brute_force"]
        words = [rec["skipped_faces"], rec["status"], rec["crossing_pairs"] & 0xffffffff, rec["crossing_pairs"] >> 32,
                 rec["coincident_pairs"] & 0xffffffff, rec["coincident_pairs"] >> 32, rec["faces_crossed"],
                 examined & 0xffffffff, examined >> 32]
        counts = np.array(words, np.int64).astype(np.uint32).view(np.int32)
        if capacity is not None:
            rows = np.full((int(capacity), 2), -1, np.int64)
            rows[:min(int(capacity), len(found))] = found[:int(capacity)]
            found = rows
        return MeshSelfIntersections(face_counts, found if want_pairs else None, counts)
    from .. import _lib
    lib = _lib.load()
    vertices, faces = _device_weld_of(mesh)
    dev = vertices.device
    n, n_verts = faces.shape[0], vertices.shape[0]
    face_counts = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(9, dtype=torch.int32, device=dev)

    def call(rows, cap):
        nbytes = lib.zs_mesh_self_intersections_scratch_bytes(n, cap)
        if nbytes == 0:
            raise _lib.ZeroShapeHipError("mesh_self_intersections: %d faces and a capacity of %d exceed the kernels' limits" % (n, cap))
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_self_intersections(_lib.ptr(vertices), _lib.ptr(faces), n, n_verts, _lib.ptr(face_counts),
                                                      _lib.ptr(rows), cap, _lib.ptr(counts), _lib.ptr(scratch),
                                                      _lib.current_stream_ptr(dev)), "zs_mesh_self_intersections")

    if not want_pairs:
        call(None, 0)
        return MeshSelfIntersections(face_counts, None, counts)
    if capacity is None:
        call(None, 0)
        lo, hi = (int(v) & 0xffffffff for v in counts[2:4].tolist())                     # the one read in between: 8 bytes
        capacity = lo | (hi << 32)
    rows = torch.full((int(capacity), 2), -1, dtype=torch.int32, device=dev)
    call(rows if capacity > 0 else None, int(capacity))
    return MeshSelfIntersections(face_counts, rows, counts)


def self_intersections_option(opt):
    """Whether ``--eval.mesh_self_intersections=true`` is set (opt-in, command line only: no yaml file carries it).  It
    scores the delivered mesh itself, so it needs no smoothing or simplification."""
    return bool(opt.eval.get("mesh_self_intersections", False))


def _with_self_intersections(mesh, reference=None):
    """``eval.mesh_self_intersections``: the delivered mesh gets its ``self_intersections`` (computed here, kept) and - where a
    smoothing or simplification step made it from ``reference``, the mesh as it stood after filter_components -
    ``self_intersections_before``, the record of that mesh: what the steps added.  -> mesh."""
    if reference is not None and reference is not mesh:
        mesh.self_intersections_before = reference.self_intersections
    mesh.self_intersections                              # (the property computes the record and keeps it)
    return mesh


def _self_intersections_record(done):
    c = done.check()
    return dict(crossing_pairs=c["n_pairs"], faces_crossed=c["n_faces_crossed"], coincident_pairs=c["n_coincident"],
                skipped_faces=c["skipped_faces"])


def mesh_report(mesh):
    """What demo.py's ``--eval.mesh_report=true`` stores as JSON: the totals of a SimpleMesh (trimesh's names) and its
    per-component table; a mesh that mesh_vertex_colors coloured also reports its ``seen_area_fraction``, a mesh that
    simplify_mesh made its ``simplification`` (the cell, the origin, the placement and the counts: with ``is_watertight`` and
    the component table beside it, what the clustering did to the surface), and a mesh that carries a ``deviation`` (a
    MeshDeviation, set by the pipelines under ``eval.mesh_deviation``) that record - with the six distances also in
    marching-cubes cells (``*_cells``) when the record knows the cell edge; a mesh that carries a ``volume_iou`` (a
    MeshVolumeIoU, set by the pipelines under ``eval.mesh_iou``) that record; a mesh that carries a ``reprojection`` (a
    MeshReprojection, set by the pipelines under ``eval.mesh_reprojection``) that record; a mesh whose ``self_intersections``
    the pipelines computed under ``eval.mesh_self_intersections`` the entry ``self_intersections``: crossing_pairs,
    faces_crossed, coincident_pairs (the one coplanar contact that is counted, apart from the crossings) and skipped_faces,
    with the same four of the mesh before smoothing and simplification under ``before`` when such a step ran."""
    comps = mesh.components
    report = dict(vertices=int(comps.vertices.sum()), faces=int(comps.faces.sum()), components=comps.n_components,
                  area=mesh.area, volume=mesh.volume, euler_number=mesh.euler_number, is_watertight=mesh.is_watertight,
                  component_table=comps.table())
    if getattr(mesh, "device_vertex_colors", None) is not None:
        report["seen_area_fraction"] = mesh.seen_area_fraction
    if getattr(mesh, "simplification", None) is not None:
        record = mesh.simplification._asdict()
        record["origin"] = list(record["origin"])
        report["simplification"] = record
    if getattr(mesh, "deviation", None) is not None:
        record = mesh.deviation._asdict()
        if record["cell_edge"] is not None:
            for side in ("forward", "backward"):
                for what in ("max", "mean", "rms"):
                    record["%s_%s_cells" % (side, what)] = record["%s_%s" % (side, what)] / record["cell_edge"]
        report["deviation"] = record
    if getattr(mesh, "volume_iou", None) is not None:
        report["volume_iou"] = mesh.volume_iou._asdict()
    if getattr(mesh, "reprojection", None) is not None:
        record = mesh.reprojection._asdict()
        if record["depth_max_pixel"] is not None:
            record["depth_max_pixel"] = list(record["depth_max_pixel"])
        report["reprojection"] = record
    if getattr(mesh, "_self_intersections", None) is not None:
        record = _self_intersections_record(mesh._self_intersections)
        if getattr(mesh, "self_intersections_before", None) is not None:
            record["before"] = _self_intersections_record(mesh.self_intersections_before)
        report["self_intersections"] = record
    return report


# ---- vertex colours from the input photo (csrc/mesh_colors.hip) ----

# Design choices, not measurements: a vertex counts as facing the camera when the cosine between its normal and the ray to
# the camera exceeds COLOR_MIN_COS (grazing vertices would smear texels along the silhouette), and as unoccluded when it lies
# within COLOR_DEPTH_TOL_CELLS marching-cubes cells (mesh units: cells * (range_max - range_min) / vox_res) behind the nearest
# surface of its z-buffer texel (a face is at most one cell across, so a vertex's own neighbourhood passes).
COLOR_MIN_COS = 0.1
COLOR_DEPTH_TOL_CELLS = 1.5


def default_color_depth_tol(opt):
    """The occlusion tolerance of vertex_colors in mesh units: COLOR_DEPTH_TOL_CELLS cells of the evaluation grid."""
    range_min, range_max = opt.eval.range
    return COLOR_DEPTH_TOL_CELLS * (float(range_max) - float(range_min)) / float(opt.eval.vox_res)


def _round_u8(x):
    """floor(x + 0.5) clamped to [0, 255] as uint8, NaN -> 0: col_round of csrc/mesh_colors.hip."""
    with np.errstate(invalid="ignore"):
        r = np.floor(np.asarray(x, np.float64) + 0.5)
        return np.where(r >= 0.0, np.minimum(r, 255.0), 0.0).astype(np.uint8)


def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd in
    float64 (the rounded sum moved, when inexact and even, to its neighbour on the side of the exact value - found with the
    TwoSum error term), and a round-to-odd value with 53 >= 2 * 24 + 2 bits rounds to float32 like the exact one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        move = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(move, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def nearest_point_host(queries, candidates, block=1 << 22):
    """For every query [n,3] the nearest candidate [m,3] (m > 0) by zs_chamfer_forward_ws's rule, brute force: float32
    (dx, dy, dz) = candidate - query, d = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), the lowest index among equal minima ->
    (squared distance float32 [n], index int32 [n])."""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    c = np.asarray(candidates, np.float32).reshape(-1, 3)
    dist, index = np.zeros(len(q), np.float32), np.zeros(len(q), np.int32)
    rows = max(1, block // max(len(c), 1))
    for lo in range(0, len(q), rows):
        d3 = c[None, :, :] - q[lo:lo + rows, None, :]
        d = _fma32(d3[..., 2], d3[..., 2], _fma32(d3[..., 1], d3[..., 1], d3[..., 0] * d3[..., 0]))
        best = np.argmin(d, axis=1)                               # (the first minimum: the lowest index)
        index[lo:lo + rows] = best
        dist[lo:lo + rows] = d[np.arange(len(best)), best]
    return dist, index


def mesh_vertex_colors_host(vertices, faces, normals, image, mask, intr, mean, scale, depth_tol, min_cos=COLOR_MIN_COS,
                            supersample=2, fade=0.0, base_rgb=BASE_RGB):
    """The definition of mesh_vertex_colors and the checker of csrc/mesh_colors.hip: float64 numpy from the float32 inputs,
    operation for operation (the kernels are built without contraction, so the outputs are equal, not close).
    ``vertices`` [V,3], ``faces`` [F,3], ``normals`` [V,3] (the weld's, area weighted), ``image`` [3,H,W] in [0,1], ``mask``
    [H,W], ``intr`` [3,3], ``mean`` [3], ``scale`` scalar -> dict: colors uint8 [V,3], seen uint8 [V], source int32 [V],
    seen_area / total_area (float), u, w, Z float64 [V].

    A. X = v scale + mean, p = K X, Z = p_z, u = p_x / p_z, w = p_y / p_z; pixel (row i, col j) is at (u, w) = (j, i).
    B. A z-buffer of ss H x ss W in that camera, a plain loop over the faces in index order: raster coordinates (u + 0.5) ss,
       (w + 0.5) ss, pixel centres (j + 0.5, i + 0.5), coverage inclusive on every edge, faces with a Z not > 0 or not finite
       or with zero / NaN / overflowing area skipped whole, depth 1 / (sum w_k / Z_k) rounded to float32, the nearest depth
       wins and at equal depth the lower face index.
    C. Seen iff Z > 0 and finite, 0 <= u <= W - 1, 0 <= w <= H - 1; n . (-X) > min_cos |n| |X| (a zero or non-finite n fails);
       the four mask texels of the bilinear footprint are > 0.5; and the z-buffer texel of (u, w) is empty, or holds a face of
       this vertex, or Z <= depth + depth_tol scale.  Colour: bilinear, floor(255 c + 0.5) clamped.
    D/E. A hidden vertex takes the colour of the nearest seen vertex in mesh space (nearest_point_host), faded towards
       ``base_rgb`` by t = min(sqrt(dist) / fade, 1) (fade 0: t = 0): floor((1 - t) c_nn + t 255 base + 0.5) clamped.  When no
       vertex is seen every vertex gets 255 base and source -1."""
    f64 = np.float64
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(f64)
    img = np.asarray(image, np.float32).astype(f64)
    msk = np.asarray(mask, np.float32).reshape(img.shape[1:])
    K = np.asarray(intr, np.float32).reshape(3, 3).astype(f64)
    mu = np.asarray(mean, np.float32).reshape(3).astype(f64)
    s = f64(np.asarray(scale, np.float32).reshape(-1)[0])
    base = np.asarray(base_rgb, np.float32).reshape(3).astype(f64)
    depth_tol, min_cos, fade, ss = f64(depth_tol), f64(min_cos), f64(fade), int(supersample)
    H, W = img.shape[1:]
    Hz, Wz = H * ss, W * ss
    V = len(v32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        X = v32.astype(f64) * s + mu
        p = [K[r, 0] * X[:, 0] + K[r, 1] * X[:, 1] + K[r, 2] * X[:, 2] for r in range(3)]
        Z, u, w = p[2], p[0] / p[2], p[1] / p[2]
        # B
        zdepth, zface = np.full((Hz, Wz), np.inf, np.float32), np.full((Hz, Wz), -1, np.int64)
        xr, yr = (u + 0.5) * f64(ss), (w + 0.5) * f64(ss)
        for t in range(len(f)):
            idx = f[t]
            z, x, y = Z[idx], xr[idx], yr[idx]
            if not np.all((z > 0.0) & (z <= 1.7e308)):
                continue
            area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
            if not abs(area) > 0.0 or not abs(area) <= 1.0e300:
                continue
            j0, j1 = int(min(max(np.ceil(x.min() - 0.5), 0.0), Wz)), int(max(min(np.floor(x.max() - 0.5), Wz - 1.0), -1.0))
            i0, i1 = int(min(max(np.ceil(y.min() - 0.5), 0.0), Hz)), int(max(min(np.floor(y.max() - 0.5), Hz - 1.0), -1.0))
            if i1 < i0 or j1 < j0:
                continue
            py, px = (np.arange(i0, i1 + 1, dtype=f64) + 0.5)[:, None], (np.arange(j0, j1 + 1, dtype=f64) + 0.5)[None, :]
            w0 = ((x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])) / area
            w1 = ((x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])) / area
            w2 = ((x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])) / area
            d = (1.0 / (w0 / z[0] + w1 / z[1] + w2 / z[2])).astype(np.float32)
            hit = (w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0) & (d > 0.0) & (d <= np.float32(3.0e38))
            sub_d, sub_f = zdepth[i0:i1 + 1, j0:j1 + 1], zface[i0:i1 + 1, j0:j1 + 1]
            hit &= d < sub_d                                      # (ascending faces: a tie keeps the lower index)
            sub_d[hit], sub_f[hit] = d[hit], t
        # C
        ok = (Z > 0.0) & (Z <= 1.7e308) & (u >= 0.0) & (u <= f64(W - 1)) & (w >= 0.0) & (w <= f64(H - 1))
        dvec = -X
        nn = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        dd = np.sqrt(dvec[:, 0] * dvec[:, 0] + dvec[:, 1] * dvec[:, 1] + dvec[:, 2] * dvec[:, 2])
        dot = n[:, 0] * dvec[:, 0] + n[:, 1] * dvec[:, 1] + n[:, 2] * dvec[:, 2]
        ok &= (nn > 0.0) & (nn <= 1.7e308) & (dot > min_cos * nn * dd)
        us, ws = np.where(ok, u, 0.0), np.where(ok, w, 0.0)       # (indices only of vertices still in the running)
        j0 = np.minimum(np.floor(us).astype(np.int64), max(W - 2, 0))
        i0 = np.minimum(np.floor(ws).astype(np.int64), max(H - 2, 0))
        j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
        half = np.float32(0.5)
        ok &= (msk[i0, j0] > half) & (msk[i0, j1] > half) & (msk[i1, j0] > half) & (msk[i1, j1] > half)
        fu, fv = us - j0.astype(f64), ws - i0.astype(f64)
        colors = np.zeros((V, 3), np.uint8)
        for c in range(3):
            t00, t01, t10, t11 = img[c][i0, j0], img[c][i0, j1], img[c][i1, j0], img[c][i1, j1]
            val = (1.0 - fv) * ((1.0 - fu) * t00 + fu * t01) + fv * ((1.0 - fu) * t10 + fu * t11)
            colors[:, c] = _round_u8(255.0 * val)
        jz = np.minimum(np.floor((us + 0.5) * f64(ss)).astype(np.int64), Wz - 1)
        iz = np.minimum(np.floor((ws + 0.5) * f64(ss)).astype(np.int64), Hz - 1)
        win_f, win_d = zface[iz, jz], zdepth[iz, jz].astype(f64)
        own = (f[np.maximum(win_f, 0)] == np.arange(V)[:, None]).any(axis=1) if len(f) else np.zeros(V, bool)
        ok &= (win_f < 0) | own | (Z <= win_d + depth_tol * s)
        colors[~ok] = 0
        # fraction
        tri = v32.astype(f64)[f]
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        nx, ny, nz = (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
        area = 0.5 * np.sqrt(nx * nx + ny * ny + nz * nz)
        seen_area, total_area = float(area[ok[f].all(axis=1)].sum()), float(area.sum())
        # D, E
        source = np.where(ok, np.arange(V), -1).astype(np.int32)
        seen_ids, hidden_ids = np.flatnonzero(ok), np.flatnonzero(~ok)
        if len(hidden_ids):
            if len(seen_ids) == 0:
                colors[:] = _round_u8(255.0 * base)
            else:
                dist, near = nearest_point_host(v32[hidden_ids], v32[seen_ids])
                src = seen_ids[near]
                t = np.minimum(np.sqrt(dist.astype(f64)) / fade, 1.0) if fade > 0.0 else np.zeros(len(src), f64)
                t = np.where(t <= 1.0, t, 1.0)
                colors[hidden_ids] = _round_u8((1.0 - t)[:, None] * colors[src].astype(f64) + t[:, None] * (255.0 * base)[None, :])
                source[hidden_ids] = src
    return dict(colors=colors, seen=ok.astype(np.uint8), source=source, seen_area=seen_area, total_area=total_area, u=u, w=w, Z=Z)


@torch.no_grad()
def mesh_vertex_colors(mesh, image, mask, intr, mean, scale, depth_tol, min_cos=COLOR_MIN_COS, supersample=2, fade=0.0,
                       base_rgb=BASE_RGB):
    """Colours one GPU SimpleMesh from the photo it was predicted from (the semantics: mesh_vertex_colors_host), on the current
    stream: ``image`` [3,H,W] fp32 in [0,1], ``mask`` H*W values, ``intr`` [3,3], ``mean`` [3], ``scale`` one value - GPU tensors,
    one sample of var.rgb_input_map / mask_input_map / intr_pred and of seen_surface's normalisation.  ``depth_tol`` and
    ``fade`` are in mesh units.  Reuses the weld the mesh carries (``_device_weld``) or welds with normals and keeps it.
    zs_mesh_colors_seen, the 4-byte read-back of the seen count, zs_mesh_colors_compact, the library's own nearest-neighbour
    search (zs_chamfer_forward_ws: hidden against seen) and zs_mesh_colors_fill.  Stores ``mesh.device_vertex_colors`` uint8
    [V,3], ``device_vertex_seen`` uint8 [V], ``device_color_source`` int32 [V] (the vertex itself when seen, the vertex it
    copied from when hidden, -1 when nothing is seen) and ``device_seen_area`` fp64 [2] (seen area, total area), all on the
    device until read through ``vertex_colors`` / ``vertex_seen`` / ``seen_area_fraction``.  A host-built mesh or CPU tensors
    raise ValueError: there is no CPU path.  -> mesh."""
    import ctypes
    from .. import _lib
    if getattr(mesh, "device_triangles", None) is None:
        raise ValueError("mesh_vertex_colors: the mesh was built from a host array; there is no CPU path")
    tensors = dict(image=image, mask=mask, intr=intr, mean=mean, scale=scale)
    for name, t in tensors.items():
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError("mesh_vertex_colors: %s must be a GPU tensor; there is no CPU path" % name)
    image, mask, intr, mean, scale = [_gpu_f32(tensors[k], k) for k in ("image", "mask", "intr", "mean", "scale")]
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError("mesh_vertex_colors: image must be [3,H,W], got %s" % (tuple(image.shape),))
    H, W = int(image.shape[1]), int(image.shape[2])
    if mask.numel() != H * W or intr.numel() != 9 or mean.numel() != 3 or scale.numel() != 1:
        raise ValueError("mesh_vertex_colors: mask must hold H*W values, intr 9, mean 3 and scale 1")
    ss = int(supersample)
    if ss < 1:
        raise ValueError("mesh_vertex_colors: supersample must be >= 1, got %r" % (supersample,))
    lib = _lib.load()
    if mesh._device_weld is None:
        mesh._device_weld = weld_mesh(mesh.device_triangles, normals=True)
    vertices, faces, normals = mesh._device_weld
    V, F, dev = vertices.shape[0], faces.shape[0], vertices.device
    colors = torch.zeros(V, 3, dtype=torch.uint8, device=dev)
    seen = torch.zeros(V, dtype=torch.uint8, device=dev)
    source = torch.full((V,), -1, dtype=torch.int32, device=dev)
    area = torch.zeros(2, dtype=torch.float64, device=dev)
    if V:
        nbytes = lib.zs_mesh_colors_workspace_bytes(V, F, H, W, ss)
        if nbytes == 0:
            raise _lib.ZeroShapeHipError("mesh_vertex_colors: V=%d F=%d at %dx%d x%d exceeds one launch" % (V, F, H, W, ss))
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = _lib.current_stream_ptr(dev)
        base = (ctypes.c_float * 3)(*[float(c) for c in base_rgb])
        with _lib.on(dev):
            _lib.check(lib.zs_mesh_colors_seen(
                _lib.ptr(vertices), _lib.ptr(faces), _lib.ptr(normals), V, F, _lib.ptr(image), _lib.ptr(mask), H, W, _lib.ptr(intr),
                _lib.ptr(mean), _lib.ptr(scale), ss, float(depth_tol), float(min_cos), _lib.ptr(colors), _lib.ptr(seen),
                _lib.ptr(source), _lib.ptr(count), _lib.ptr(area), _lib.ptr(ws), stream), "zs_mesh_colors_seen")
            n_seen = int(count.item())                       # 4-byte D2H: sizes the two lists
            n_hidden = V - n_seen
            if n_hidden:
                seen_idx = torch.empty(n_seen, dtype=torch.int32, device=dev)
                seen_xyz = torch.empty(n_seen, 3, dtype=torch.float32, device=dev)
                hidden_idx = torch.empty(n_hidden, dtype=torch.int32, device=dev)
                hidden_xyz = torch.empty(n_hidden, 3, dtype=torch.float32, device=dev)
                _lib.check(lib.zs_mesh_colors_compact(_lib.ptr(vertices), _lib.ptr(seen), V, n_seen, _lib.ptr(ws), _lib.ptr(seen_idx),
                                                      _lib.ptr(seen_xyz), _lib.ptr(hidden_idx), _lib.ptr(hidden_xyz), stream),
                           "zs_mesh_colors_compact")
                near = dist = None
                if n_seen:
                    dist = torch.empty(n_hidden, dtype=torch.float32, device=dev)
                    near = torch.empty(n_hidden, dtype=torch.int32, device=dev)
                    dist2 = torch.empty(n_seen, dtype=torch.float32, device=dev)
                    near2 = torch.empty(n_seen, dtype=torch.int32, device=dev)
                    cbytes = lib.zs_chamfer_workspace_bytes(1, n_hidden, n_seen)
                    cws = torch.empty((cbytes + 15) // 16 * 2, dtype=torch.int64, device=dev)
                    _lib.check(lib.zs_chamfer_forward_ws(_lib.ptr(hidden_xyz), _lib.ptr(seen_xyz), 1, n_hidden, n_seen, _lib.ptr(dist),
                                                         _lib.ptr(dist2), _lib.ptr(near), _lib.ptr(near2), _lib.ptr(cws), cbytes,
                                                         stream), "zs_chamfer_forward_ws")
                _lib.check(lib.zs_mesh_colors_fill(_lib.ptr(hidden_idx), _lib.ptr(seen_idx), _lib.ptr(near), _lib.ptr(dist), V, n_seen,
                                                   float(fade), base, _lib.ptr(colors), _lib.ptr(source), stream),
                           "zs_mesh_colors_fill")
    mesh.device_vertex_colors, mesh.device_vertex_seen, mesh.device_color_source, mesh.device_seen_area = colors, seen, source, area
    mesh._vertex_colors = mesh._vertex_seen = mesh._seen_area = None
    return mesh


def vertex_colors(opt, var, meshes=None, **kw):
    """mesh_vertex_colors for every mesh of the batch (``meshes``, default ``var.mesh_pred``) with sample b of
    ``var.rgb_input_map``, ``var.mask_input_map`` and ``var.intr_pred`` (``var.intr`` when there is no prediction).  (mean, scale)
    come from camera.seen_surface on ``var.depth_pred`` - the kernel Graph.forward normalised the seen surface with, on the same
    inputs, hence the same bits.  ``depth_tol`` defaults to default_color_depth_tol(opt); further keywords go to
    mesh_vertex_colors.  -> meshes."""
    from . import camera
    meshes = var.mesh_pred if meshes is None else meshes
    intr = var.intr_pred if getattr(var, "intr_pred", None) is not None else var.intr
    _, _, _, mean, scale = camera.seen_surface(opt, var.depth_pred, intr, var.mask_input_map)
    kw.setdefault("depth_tol", default_color_depth_tol(opt))
    for b, mesh in enumerate(meshes):
        mesh_vertex_colors(mesh, var.rgb_input_map[b], var.mask_input_map[b], intr[b], mean[b], scale[b:b + 1], **kw)
    return meshes


def color_options(opt):
    """The keywords of vertex_colors when ``--eval.vertex_colors=true`` is set (``--eval.color_fade=<mesh units>``,
    ``--eval.color_min_cos``, ``--eval.color_supersample``: no yaml file carries them), else None."""
    if not bool(opt.eval.get("vertex_colors", False)):
        return None
    return dict(fade=float(opt.eval.get("color_fade", 0.0)), min_cos=float(opt.eval.get("color_min_cos", COLOR_MIN_COS)),
                supersample=int(opt.eval.get("color_supersample", 2)))


_MC_TABLES = {}


def _mc_tables(device):
    key = str(device)
    if key not in _MC_TABLES:
        from .. import mc_tables as T
        stride = 16
        tab = -np.ones((256, stride), np.int8)
        tab[:, :T.TRI_TABLE.shape[1]] = T.TRI_TABLE
        _MC_TABLES[key] = (torch.from_numpy(tab).to(device), torch.from_numpy(T.TRI_COUNT.astype(np.uint8)).to(device),
                           stride)
    return _MC_TABLES[key]


@torch.no_grad()
def extract_surface(level_vox, isoval, range_min, range_max, num_points=0, seed=0):
    """GPU marching cubes (+ optional area-weighted sampling) of ONE level grid [G,G,G] that
    already lives on the device.  Returns (triangles [n,3,3] fp32 GPU tensor,
    points [num_points,3] fp32 GPU tensor | None).  Vertex scaling reproduces the reference's
    ``v / S * (max - min) + min`` with S = G (utils/eval_3D.py:252-255)."""
    from .. import _lib
    lib = _lib.load()
    vol = level_vox.detach().to(torch.float32).contiguous()
    assert vol.dim() == 3 and vol.shape[0] == vol.shape[1] == vol.shape[2] and vol.is_cuda
    G = vol.shape[0]
    dev = vol.device
    tab, cnt, stride = _mc_tables(dev)
    scratch = torch.empty(lib.zs_mc_scratch_bytes(G) // 4 + 1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = _lib.current_stream_ptr(dev)
    with torch.cuda.device(dev):
        _lib.check(lib.zs_mc_count(_lib.ptr(vol), G, float(isoval), _lib.ptr(cnt), _lib.ptr(scratch),
                                   _lib.ptr(total), stream), "zs_mc_count")
        n_tris = int(total.item())                       # 4-byte D2H: sizes the output
        tris = torch.empty(n_tris, 3, 3, dtype=torch.float32, device=dev)
        scale = np.float32((range_max - range_min) / G)
        _lib.check(lib.zs_mc_emit(_lib.ptr(vol), G, float(isoval), _lib.ptr(tab), stride, _lib.ptr(cnt),
                                  _lib.ptr(scratch), float(scale), float(range_min), _lib.ptr(tris), n_tris,
                                  stream), "zs_mc_emit")
        pts = sample_surface(tris, num_points, seed) if num_points else None
    return tris, pts


@torch.no_grad()
def sample_surface(tris, num_points, seed=0):
    """``num_points`` area-weighted points [num_points,3] fp32 on a triangle soup [n,3,3] that lives on the GPU
    (zs_mesh_sample: counter-based random stream seeded by ``seed``; an empty soup gives zeros), enqueued on the current
    stream.  extract_surface samples through this, and so does the pipeline after filter_components."""
    from .. import _lib
    lib = _lib.load()
    if not (isinstance(tris, torch.Tensor) and tris.is_cuda):
        raise ValueError("sample_surface: tris must be a GPU tensor")
    soup = tris.detach().to(torch.float32).reshape(-1, 3, 3).contiguous()
    n_tris, dev = soup.shape[0], soup.device
    pts = torch.empty(int(num_points), 3, dtype=torch.float32, device=dev)
    cum = torch.empty(max(lib.zs_mesh_sample_scratch_doubles(n_tris), 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.zs_mesh_sample(_lib.ptr(soup), n_tris, int(num_points), int(seed) & ((1 << 64) - 1),
                                      _lib.ptr(cum), _lib.ptr(pts), _lib.current_stream_ptr(dev)), "zs_mesh_sample")
    return pts


def convert_to_explicit(opt, level_grids, isoval=0., to_pointcloud=False, seed=0):
    """utils/eval_3D.py:233-263 on the GPU: marching cubes at ``isoval`` + area-weighted surface
    sampling, one level grid at a time (no Python threads, no PyMCubes / trimesh).
    ``level_grids``: list of [G,G,G] arrays or GPU tensors (a numpy grid is uploaded - pass
    the tensor compute_level_grid returned to keep the grid in HBM).  Returns ``meshes``
    (SimpleMesh list) and, with ``to_pointcloud``, ``pointclouds`` float64 [B,num_points,3]
    like the reference (an empty mesh gives zeros, :262).  The random stream is a
    counter-based generator seeded by ``seed`` + the grid index, not numpy's global RNG.
    With ``opt.eval.min_component_area`` / ``opt.eval.drop_cavities`` set (opt-in) every mesh goes through
    filter_components first, with ``opt.eval.smooth_iterations`` set (opt-in, _smooth_options) through smooth_mesh after
    that, with ``opt.eval.simplify_cells`` set (opt-in, _simplify_options) through simplify_mesh last, and the points are
    sampled on what comes out: the metrics describe the mesh that is delivered.  With ``opt.eval.mesh_deviation`` (opt-in,
    _deviation_option) that mesh carries ``deviation``: how far the smoothing and the simplification moved the surface; with
    ``opt.eval.mesh_iou`` (opt-in, _iou_option) it carries ``volume_iou``: how much volume they added or removed, counted on
    the level grid's own marching-cubes lattice; with ``opt.eval.mesh_self_intersections`` (opt-in,
    self_intersections_option) it carries ``self_intersections``: which of its faces pass through each other."""
    device = getattr(opt, "device", "cuda")
    meshes, clouds = [], []
    for i, g in enumerate(level_grids):
        vol = g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g, np.float32))
        vol = vol.to(device)
        assert vol.shape[0] == vol.shape[1] == vol.shape[2]
        range_min, range_max = opt.eval.range
        cleaning, smoothing, simplifying = _component_options(opt), _smooth_options(opt), _simplify_options(opt)
        deviation_cell = _deviation_option(opt, smoothing, simplifying)
        iou_lattice = _iou_option(opt, smoothing, simplifying, G=vol.shape[0])
        selfx = self_intersections_option(opt)
        if cleaning is None and smoothing is None and simplifying is None:
            tris, pts = extract_surface(vol, isoval, range_min, range_max,
                                        opt.eval.num_points if to_pointcloud else 0, seed + i)
            mesh = SimpleMesh(tris)                      # stays in HBM until a dump reads it
            if selfx:
                _with_self_intersections(mesh)
        else:                   # marching cubes, filter_components, smooth_mesh, simplify_mesh, then sampling with the same seed
            tris, _ = extract_surface(vol, isoval, range_min, range_max)
            mesh = _cleaned_and_smoothed(SimpleMesh(tris), cleaning, smoothing, simplifying, deviation_cell, iou_lattice, selfx)
            pts = sample_surface(mesh.device_triangles, opt.eval.num_points, seed + i) if to_pointcloud else None
        meshes.append(mesh)
        if to_pointcloud:
            clouds.append(pts.cpu().numpy().astype(np.float64))
    if to_pointcloud:
        return meshes, np.stack(clouds, axis=0)
    return meshes
