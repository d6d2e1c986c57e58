/* zeroshape_hip.h - C ABI of libzeroshape_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for ZeroShape's dense SDF-query / Chamfer hot path.  Plain
 * pointers and sizes only: every pointer is a DEVICE pointer unless marked
 * [host]; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All entry points are asynchronous w.r.t. the host (they enqueue on `stream`
 * and return) and return 1 on success, 0 on failure - the convention of the
 * reference's native launchers (external/chamfer3D/chamfer3D.cu:145-151).
 * After a 0, zs_last_error() gives a thread-local message.  Nothing here
 * allocates device memory; callers own every buffer.
 *
 * Reference interfaces replaced (paths relative to the upstream ZeroShape tree):
 *   zs_chamfer_forward   <- chamfer_cuda_forward,  external/chamfer3D/chamfer3D.cu:136-154
 *                           (bound as chamfer_3D.forward, chamfer_cuda.cpp:19-21,31)
 *   zs_chamfer_backward  <- chamfer_cuda_backward, external/chamfer3D/chamfer3D.cu:176-195
 *                           (bound as chamfer_3D.backward, chamfer_cuda.cpp:24-28,32)
 *   zs_sdf_*             <- Implicit.forward, model/shape/implicit.py:251-288, as it is
 *                           driven by compute_level_grid, utils/eval_3D.py:22-45, and
 *                           get_dense_3D_grid, utils/eval_3D.py:11-20
 *   zs_bf_lower_bounds   <- pruning for brute_force_search, utils/eval_3D.py:140-170
 *   zs_pose_search_batch_sorted <- one batch of brute_force_search, utils/eval_3D.py:149-168
 *   zs_normalize_pc      <- normalize_pc, utils/eval_3D.py:93-102
 *   zs_standardize_pc, zs_icp_step <- standardize_pc, ICP, utils/eval_3D.py:83-91, 271-284
 *   zs_fscore            <- compute_fscore, utils/eval_3D.py:215-231
 *   zs_mc_*, zs_mesh_*   <- convert_to_explicit, utils/eval_3D.py:233-263 (PyMCubes
 *                           marching_cubes + trimesh.sample on the host)
 *   zs_mesh_weld, zs_mesh_weld_vertices <- the (vertices, triangles) mcubes.marching_cubes
 *                           returns and trimesh's vertex_normals, utils/eval_3D.py:250-256
 *   zs_mesh_stats, zs_render_frames <- dump_meshes_viz, scale_to_unit_cube, visualize_mesh,
 *                           utils/util_vis.py:112-127, 310-405 (trimesh + pyrender on OpenGL)
 *   zs_seen_mesh_workspace_bytes, zs_seen_mesh <- create_seen_surface, utils/util_vis.py:137-170
 *                           (a Python loop over every pixel with a host sync per test)
 *   zs_seen_surface, zs_unproj_depth, zs_valid_norm_fac, zs_masked_resample,
 *   zs_intr_param2mtx    <- the seen-surface geometry of Graph.forward,
 *                           model/compute_graph/graph_shape.py:89-113,131-144, with
 *                           utils/camera.py:52-108 and utils/util.py:323-345
 *   zs_depth_metrics     <- DepthMetric.compute_metrics, utils/eval_depth.py:46-116
 *   zs_conv2d_nhwc, zs_group_norm_nhwc, zs_layer_norm, zs_attention, zs_max_pool_nhwc,
 *   zs_global_mean_nhwc, zs_upsample2x_nhwc, zs_assemble_tokens, zs_readout_concat,
 *   zs_nchw_to_nhwc, zs_nhwc_to_nchw
 *                        <- the layers of the image encoders: DPTDepthModel
 *                           (model/depth/dpt_depth.py:68-122, blocks.py, vit.py), CoordEncRes
 *                           (model/shape/seen_coord_enc.py:141-194), the intrinsics head
 *                           (model/compute_graph/graph_shape.py:18-28,125-129)
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 */
#ifndef ZEROSHAPE_HIP_H
#define ZEROSHAPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZS_ABI_VERSION 46

/* ABI version of the loaded library (== ZS_ABI_VERSION it was built with). */
int zs_abi_version(void);

/* Thread-local description of the last failure ("" if none). [host] */
const char *zs_last_error(void);

/* ------------------------------------------------------------------------- *
 * Chamfer-3D nearest neighbour (external/chamfer3D/chamfer3D.cu)
 * ------------------------------------------------------------------------- */

/* For every point of xyz1[b][n][3] the SQUARED distance to, and index of, its
 * nearest point in xyz2[b][m][3], and vice versa.  fp32, contiguous.
 *   dist1[b][n], idx1[b][n]  : nearest in xyz2 for each xyz1 point
 *   dist2[b][m], idx2[b][m]  : nearest in xyz1 for each xyz2 point
 * d = fma(dz,dz, fma(dy,dy, dx*dx)) with (dx,dy,dz) = other - self (bit-exact with
 * the reference kernel under nvcc's default FMA contraction); ties resolve to the
 * LOWEST index (chamfer3D.cu:36,126).  If the other cloud is empty the outputs of
 * that direction are left untouched (the reference kernel writes nothing either;
 * its caller pre-zeroes them, dist_chamfer_3D.py:29-38).
 * Non-finite points (zs_chamfer_forward and zs_chamfer_forward_ws alike, bit for bit): every
 * query starts from the record (+inf, index 0) and a candidate replaces it only on a strict
 * d < best, in index order.  So a candidate whose distance is NaN never wins; a query with a
 * NaN coordinate gets (+inf, 0); a distance of +inf never replaces the initial (+inf, 0).
 * This is NOT the reference's behaviour: its kernel takes the first candidate of every
 * 512-candidate tile unconditionally, so its answer depends on where a NaN sits, and the test
 * oracle (oracle/chamfer_ref.c) takes candidate 0 unconditionally - a NaN in candidate 0 or in
 * the query makes its distance NaN.  On NaN-free input all of them agree. */
int zs_chamfer_forward(const float *xyz1, const float *xyz2, int b, int n, int m,
                       float *dist1, float *dist2, int *idx1, int *idx2, void *stream);

/* Same contract and bit-identical results, but spatially accelerated: the candidate clouds
 * are binned into uniform grids in `workspace` (zs_chamfer_workspace_bytes(b, n, m) bytes,
 * 16-byte aligned, contents scratch) and each query only evaluates the candidates whose
 * cells can still beat its running minimum.  Worth it from a few thousand points per cloud. */
size_t zs_chamfer_workspace_bytes(int b, int n, int m);
int zs_chamfer_forward_ws(const float *xyz1, const float *xyz2, int b, int n, int m,
                          float *dist1, float *dist2, int *idx1, int *idx2,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Gradient scatter (chamfer3D.cu:155-195): gradxyz1[b][n][3] / gradxyz2[b][m][3] are
 * ACCUMULATED into with fp32 atomics (caller zeroes them, dist_chamfer_3D.py:51-55):
 *   g = 2*graddist1[i][j];  gradxyz1[i][j] += g*(p1 - p2[idx1]);  gradxyz2[i][idx1] -= same
 * and symmetrically for direction 2. */
int zs_chamfer_backward(const float *xyz1, const float *xyz2, int b, int n, int m,
                        float *gradxyz1, float *gradxyz2,
                        const float *graddist1, const float *graddist2,
                        const int *idx1, const int *idx2, void *stream);

/* ------------------------------------------------------------------------- *
 * Implicit occupancy decoder (model/shape/implicit.py), default architecture of
 * options/shape.yaml:19-44: C=256, 8 heads x 32, 2 attention blocks (mlp 4x),
 * 197 latent tokens, 8-layer softplus(beta=100) MLP with skips at 2,4,6.
 *
 * Data flow:
 *   zs_sdf_program_bytes()                  size of one packed "decoder program"
 *   [host] pack the state_dict             zeroshape_amd/program.py -> float32 words
 *   zs_sdf_prologue(program, latent, ...)  per image: hoisted latent path
 *                                          (latent_proj + pos_embed, block-0 latent
 *                                          self-attention + MLP, K/V of both blocks)
 *                                          written into the program's K/V records
 *   zs_sdf_query_points / _grid            per query point: the fused decoder; `workspace`
 *                                          (zs_sdf_workspace_bytes(), 16-byte aligned) may be
 *                                          shared by launches on the same stream
 * ------------------------------------------------------------------------- */

/* Bytes of one per-image decoder program (weights in MFMA operand order + K/V). */
size_t zs_sdf_program_bytes(void);
/* Bytes of the per-image scratch the prologue needs. */
size_t zs_sdf_prologue_scratch_bytes(void);
/* Bytes of the workspace the query kernels need (independent of batch and point count:
 * one 96 KiB slab per resident wave, 96 MiB in all; contents are scratch, the caller need not
 * initialise it: since ABI 33 the library zeroes the split-fp16 kernels' tile counter in its last
 * 4 KiB (dynamic tile order) on the stream in front of every launch - a 4-byte memset
 * node under stream capture).  One workspace per stream that launches concurrently.
 * ZS_SPLIT_STATIC_TILES=1 in the environment (read per launch) selects the static tile deal. */
size_t zs_sdf_workspace_bytes(void);
/* Extra workspace bytes zs_sdf_query_points needs BEHIND the fixed part when `attn` is
 * requested (raw probability tiles: ~14.5 KiB per point). */
size_t zs_sdf_attn_scratch_bytes(int batch, int m);

/* Fill the per-image K/V records of `programs[i]` (i < batch; programs are
 * program_stride_bytes apart, each initialised by copying the packed weights)
 * from latent_depth[batch][197][256] fp32.  `lat_params` is the packed latent-path
 * parameter block (zeroshape_amd/program.py: pack_latent_params). */
int zs_sdf_prologue(void *programs, size_t program_stride_bytes, const float *lat_params,
                    const float *latent_depth, int batch, void *scratch, void *stream);
/* The same with options (ABI 33).  ZS_SDF_POS_PERLAYER: Implicit(pos_perlayer=True) - the reference class's own default,
 * model/shape/implicit.py:269-272 - adds pos_embed to the latent rows in front of EVERY attention block, not only the first:
 * the K/V records of block 1 come from LN1'(x2 + pos_embed).  zs_sdf_prologue == flags 0 (options/shape.yaml:44). */
#define ZS_SDF_POS_PERLAYER 1
int zs_sdf_prologue_ex(void *programs, size_t program_stride_bytes, const float *lat_params,
                       const float *latent_depth, int batch, void *scratch, int flags, void *stream);

/* The comparison behind the choice of arithmetic (zeroshape_amd/model/shape/implicit.py: Implicit.prepare): got / want
 * [batch][m] logits of the same probe points from the split-fp16 and the exact-fp32 kernel -> stats[batch][5] = max |got - want|,
 * mean |got - want|, max |want|, max |sigmoid(got) - sigmoid(want)|, number of sign disagreements at |want| >= flip_band (any
 * non-finite input: the first four NaN); flags (optional) [batch][2] int32 = 1 when the image FAILS the raw-logit rule
 * (max |d| <= tol) / the occupancy rule (max |d occ| <= tol_occ and no such disagreement).  One launch, fixed reduction order. */
int zs_sdf_verdict_stats(const float *got, const float *want, int batch, int m, float flip_band, float tol, float tol_occ,
                         float *stats, int *flags, void *stream);

/* logits[batch][m] = Implicit(latent, None, points[batch][m][3]) (pre-sigmoid).
 * attn (optional, may be NULL): [batch][m][197] = mean over heads and blocks of the
 * point->latent attention probabilities (implicit.py:63,79,277; the self column is
 * excluded after the softmax over 198, so rows sum to < 1).  When given, `workspace` must
 * hold zs_sdf_workspace_bytes() + zs_sdf_attn_scratch_bytes(batch, m) bytes.
 * tile_mask (optional, NULL = every tile; here and in the two grid entry points below):
 * int32[batch * ceil(m / 128)], one entry per 128-point tile of each image in point order; a zero
 * entry leaves that tile's outputs untouched.  It is how the exact-fp32 kernel re-evaluates the
 * tiles the split-fp16 kernel flagged (see below); not combinable with attn. */
int zs_sdf_query_points(const void *programs, size_t program_stride_bytes, int batch,
                        const float *points, int m, float *logits, float *attn,
                        const int *tile_mask, void *workspace, void *stream);

/* Dense-grid query without materialising the points tensor.  Evaluates x-slices
 * [slice_begin, slice_end) of the G^3 grid (G = vox_res+1 samples per axis; coordinate
 * i -> axis[i], `axis` being torch.linspace(range_min, range_max, G) supplied by the
 * caller so values are bit-identical to utils/eval_3D.py:16).  Layout of out:
 * [batch][slice_end-slice_begin][G][G], x slowest / z fastest, like occ in
 * utils/eval_3D.py:45-46.  apply_sigmoid!=0 stores sigmoid(logit) (compute_level_grid's
 * return), else the logit. */
int zs_sdf_query_grid(const void *programs, size_t program_stride_bytes, int batch,
                      const float *axis, int G, int slice_begin, int slice_end,
                      int apply_sigmoid, float *out, const int *tile_mask, void *workspace,
                      void *stream);

/* z-mean attention of grid columns (the heat-map GIF of compute_level_grid(vis_attn=True), utils/eval_3D.py:47-80, which
 * averages the attention map over z and draws only the columns at multiples of 8): for every column (ix, iy) of
 * columns[n_cols][2] (int32, device; 0 <= ix, iy < G)
 *   zmean[batch][n_cols][197] = mean over iz < G of the attn row zs_sdf_query_points gives for (axis[ix], axis[iy], axis[iz])
 * on EXACT fp32 programs, without that [points][197] tensor: per chunk of columns the entry writes the points (the bits
 * zs_sdf_query_grid reads from `axis`), runs the attention variant of the exact kernel on them (logits discarded) and
 * reduces its raw probability tiles straight to the column means - fixed summation order, no atomics, bit-identical
 * from run to run and for every chunking.  A column is padded to whole 32-point wave tiles.
 *   workspace : zs_sdf_workspace_bytes(), as for the other queries
 *   scratch   : scratch_bytes >= zs_sdf_grid_attn_zmean_scratch_bytes(batch, n_cols, G, cap_bytes), 16-byte aligned; the
 *               entry uses scratch_bytes as its cap
 * cap_bytes (0 = 256 MiB) bounds the scratch whatever batch, n_cols and G are: the columns are split into chunks of
 * *cols_per_chunk columns of *imgs_per_chunk images (zs_sdf_grid_attn_zmean_chunk; every image, or - when one column of
 * every image exceeds the cap - one column of as many images as fit), enqueued in stream order on the same scratch.  A cap
 * below one column of one image (ceil(G / 32) wave tiles rounded up to a 128-point tile, ~1.9 MiB each) is an error:
 * _scratch_bytes returns 0, the others 0 with a message.  batch == 0 or n_cols == 0: 1, nothing launched. */
size_t zs_sdf_grid_attn_zmean_scratch_bytes(int batch, int n_cols, int G, size_t cap_bytes);
int zs_sdf_grid_attn_zmean_chunk(int batch, int n_cols, int G, size_t cap_bytes, int *imgs_per_chunk /* [host] */,
                                 int *cols_per_chunk /* [host] */);
int zs_sdf_grid_attn_zmean(const void *programs, size_t program_stride_bytes, int batch,
                           const float *axis, int G, const int *columns, int n_cols, float *zmean,
                           void *workspace, void *scratch, size_t scratch_bytes, void *stream);

/* Heat-map frames of the attention GIF (utils/eval_3D.py:62-79 + show_att_on_image, utils/util_vis.py:267-293) composed on
 * the device, one workgroup per frame:
 *   a[R][R]  = zmean[b][frame_col[f]][0] + zmean[b][frame_col[f]][1 + ..]          (zmean: [batch][n_cols][1 + R*R])
 *   v[H][W]  = bilinear upsample of a, align_corners = false, fp32 (scale = (float)R / H, src = scale (d + 0.5) - 0.5
 *              clamped at 0, i1 = i0 + (i0 < R - 1), v = l0h (l0w a00 + l1w a01) + l1h (l0w a10 + l1w a11))
 *   level    = (uint8)(255 (v / max v));  heat = lut[level] / 255;  merged = heat + image;  frame = merged / max merged
 * images: [batch][3][H][W] fp32 in [0, 1]; lut: [256][3] uint8 (RGB); frames: [batch][n_frames][H][W][3] fp32.  The two
 * maxima are exact in any order, so frames are bit-reproducible.  1 <= R <= 64; frame_col entries outside [0, n_cols) are
 * clamped. */
int zs_attn_frames(const float *zmean, int batch, int n_cols, const int *frame_col, int n_frames,
                   const float *images, int H, int W, const uint8_t *lut, int R, float *frames, void *stream);

/* Split-fp16 ("f16x3") decoder: the same network with every contraction on the 16-bit matrix
 * pipe, both operands split into two fp16 halves (A B ~= Ah Bh + Ah Bl + Al Bh, fp32
 * accumulation; halves rounded to nearest even: <= 2^-22 relative operand error without a sign
 * preference for |x| < 65520, inf / nan beyond): max |logit difference| to the exact-fp32 kernels
 * ~3e-6 on the seeded network, 1.5e-5 on a trained one with logits up to 17 - as far from the fp32
 * CPU oracle as the fp32 kernels are (contract 1e-4); 2.8x their throughput.
 *   zs_sdf_split_programs     fp32 programs (after zs_sdf_prologue) -> split programs of the
 *                             same size and stride rules (split_programs must not alias programs)
 *   zs_sdf_query_points_split / zs_sdf_query_grid_split
 *                             as zs_sdf_query_points (without the attention map) / _grid, on
 *                             split programs; same workspace
 * Envelope guard.  The operand error acts on the attention logits in absolute terms,
 * |dS| <= 2.5 * 2^-21 * d^-1/2 |q| |k|, and operands beyond +-65504 saturate.  tile_flags (optional,
 * NULL = no guard): int32[batch * ceil(m / 128)] ZEROED by the caller; the kernel sets the entry
 * of every 128-point tile in which some point and head reach d^-1/2 |q| max_l |k_l| > 64, or whose
 * program holds an operand that is not finite or outside the fp16 range (those tiles' outputs
 * are NaN).  Passing the same array as tile_mask to the exact-fp32 entry point on the same
 * stream re-evaluates exactly those tiles - no host round trip (Implicit.query_* does this). */
int zs_sdf_split_programs(const void *programs, size_t program_stride_bytes, void *split_programs,
                          size_t split_stride_bytes, int batch, void *stream);
int zs_sdf_query_points_split(const void *split_programs, size_t program_stride_bytes, int batch,
                              const float *points, int m, float *logits, int *tile_flags,
                              void *workspace, void *stream);
int zs_sdf_query_grid_split(const void *split_programs, size_t program_stride_bytes, int batch,
                            const float *axis, int G, int slice_begin, int slice_end,
                            int apply_sigmoid, float *out, int *tile_flags, void *workspace,
                            void *stream);

/* Block 0's point-side q/k/v as a rank-4 table (ABI 41).  Block 0's point row is point_proj(xyz), affine in (x, y, z, 1), so
 * after LN1 all 768 q/k/v rows are rstd * (T (x, y, z, 1)) + c with T [768][4] and c [768] functions of the weights alone.
 * A split launch of up to 175 images writes the tables of its images to the head of `workspace` (16 KiB per image, inside
 * the region of the exact-fp32 kernel's slabs) with one small kernel in front of the decode kernel; the compact streams
 * below are built from them.  The decode kernel itself no longer reads a table (it once evaluated block 0's q/k/v from it
 * and stepped over their K-blocks in the weight stream).
 *   zs_sdf_block0_tables      that kernel alone: tables[batch][4096] floats = [b_proj 256][c 768][T 3,072] of each split
 *                             program, in the kernel's register order (zeroshape_amd/program.py: block0_window) */
int zs_sdf_block0_tables(const void *split_programs, size_t program_stride_bytes, int batch, float *tables, void *stream);

/* Block 0 from a compact stream of its own (ABI 45).  With the table, a head's q, k, v and its 224 point-to-latent logits are
 * rank-5 maps of u = (rstd x, rstd y, rstd z, rstd, 1): one v_mfma_f32_32x32x16_f16 per 32 x 32 tile on packed operands
 * instead of K-blocks of three.  While tables and streams fit the head of `workspace` (175 images per launch) every split
 * launch also writes, behind the tables, 544 KiB per image: block 0's 8 x 34 K-block slots in consumption order (packed
 * operands, and copies of the program's V and proj K-blocks), and the decode kernel streams block 0 from there before it
 * continues in the program at K-block 736 (4,464 slots and 13,352 MFMAs per wave tile instead of 4,928 and 14,784).
 * ZS_SPLIT_BLOCK0_GEMM=1 in the environment (read per launch), or more than 175 images per launch, selects the GEMM path:
 * block 0 runs its q/k/v GEMMs from the program like block 1, and neither tables nor streams are written.  (Launches of
 * 176 to 6,144 images used to evaluate q/k/v from the tables alone; they now take this fallback, which is <= 8e-7 from it.)
 *   zs_sdf_block0_streams     that kernel alone: streams[batch][557,056] bytes from the split programs and their tables
 *                             (zs_sdf_block0_tables; zeroshape_amd/program.py: block0_stream) */
int zs_sdf_block0_streams(const void *split_programs, size_t program_stride_bytes, int batch, const float *tables,
                          void *streams, void *stream);

/* As zs_sdf_query_grid / zs_sdf_query_grid_split, for the points [point_begin, point_end) of
 * the grid in its memory order (x slowest, z fastest): out[batch][point_end - point_begin].
 * This is the unit of the multi-GPU sharding (zeroshape_amd/parallel.py): equal point ranges
 * instead of whole x-slices (129 slices over 8 ranks would leave 17-17-...-10). */
int zs_sdf_query_grid_range(const void *programs, size_t program_stride_bytes, int batch,
                            const float *axis, int G, long long point_begin, long long point_end,
                            int apply_sigmoid, float *out, const int *tile_mask, void *workspace,
                            void *stream);
int zs_sdf_query_grid_range_split(const void *split_programs, size_t program_stride_bytes, int batch,
                                  const float *axis, int G, long long point_begin,
                                  long long point_end, int apply_sigmoid, float *out,
                                  int *tile_flags, void *workspace, void *stream);

/* ------------------------------------------------------------------------- *
 * Brute-force pose search support (brute_force_search, utils/eval_3D.py:140-170).
 * lower_bounds[i] <= Chamfer-L1 of rotation i (normalize_pc(R_i pred) vs gt_normalized),
 * up to rounding: rigorous cell-distance bounds on 32^3 occupancy grids of the two clouds.
 * The host evaluates rotations exactly in order of increasing bound and stops when the
 * smallest remaining bound (with a margin) exceeds the best exact distance - same winner
 * as the exhaustive scan.  pred [n][3] raw, gt_normalized [m][3], rotations [k][3][3];
 * grid_gt / grid_pred: zs_bf_grid_bytes() each, scratch: zs_bf_scratch_bytes().
 * ------------------------------------------------------------------------- */
size_t zs_bf_grid_bytes(void);
size_t zs_bf_scratch_bytes(void);
int zs_bf_lower_bounds(const float *pred, int n, const float *gt_normalized, int m,
                       const float *rotations, int k, float *grid_gt, float *grid_pred,
                       void *scratch, float *lower_bounds, void *stream);

/* ------------------------------------------------------------------------- *
 * Fused pose search (brute_force_search, utils/eval_3D.py:140-170) and its helpers
 * normalize_pc (:93-102) and compute_fscore (:215-231).
 *
 * zs_pose_search_batch_sorted - the one search entry - evaluates `count` (<= zs_pose_max_batch()) rotations exactly:
 * rotate pred[n][3], normalize_pc, nearest neighbours both ways against the normalised ground truth [m][3] with the
 * arithmetic of zs_chamfer_forward, sqrt, means, the six F-score thresholds - and merges the
 * lexicographic (Chamfer-L1, rotation index) minimum into the running record `best`
 * (zs_pose_best_bytes(), device; zs_pose_best_init first): float cd, int32 index, float acc,
 * comp, f[6], int32 rotations evaluated, int32 rotations scanned in full, float external bound (slot 12: +inf,
 * or the best distance other ranks have found - it tightens every pruning decision of later batches and never
 * enters the record; zeroshape_amd/utils/eval_3D.py shares it once per search).  That minimum over all batches is the reference's first
 * strict minimum (:161-168).  Rotation b of the batch is rotations[order ? order[b] : b]
 * ([..][3][3]); its reported index is that number + index_offset.  lower_bound (optional,
 * device): one float, the smallest zs_bf_lower_bounds value in this batch - when it proves the
 * batch cannot beat `best`, the kernels return at once, so all batches can be enqueued without
 * a host synchronisation.  No rotated cloud, distance or index array is materialised; results
 * are bit-reproducible (fixed reduction order) whatever batch a rotation is evaluated in.
 *
 * Both clouds arrive twice: `pred` in the caller's order - the statistics of normalize_pc are summed in it, and it is the
 * order zs_pose_apply sees - and pred_sorted / gt_sorted in the sort-tile-recursive order of zs_str_sort (x slabs, y strips
 * inside a slab, z inside a strip; cuts at whole leaves of 64 points, three stable radix sorts, so the permutation is a
 * pure function of the coordinates; scratch: zs_str_scratch_bytes(n); perm may be NULL), whose leaves of 64 consecutive
 * points have near-cubic boxes, also after a rotation.  zs_pose_pack writes a sorted cloud as a PACK
 * (zs_pose_pack_bytes(points)): [sub-tile of 64][x | y | z][64] coordinates, the exact box of every sub-tile and of every
 * tile of 16 - the form in which a wave reads candidates through the scalar cache.  Three modes, one record:
 *   mode 0  every pair, candidates staged in LDS (reads gt_sorted; gt_pack unused)   - the tests' independent reference
 *   mode 1  every pair on packs (the kernel of mode 2 without the skipping)          - the tests' second reference
 *   mode 2  every (query, 64 candidates) block whose box is farther than the query's current nearest neighbour is
 *           skipped, tiles nearest first                                             - the default of brute_force_search
 * All three give the same minima and the same fixed-order sums - the same record, bit for bit; mode 2 from a fraction of
 * the distance evaluations (utils/eval_3D.py:140-170 evaluates them all).
 * scratch: zs_pose_sorted_scratch_bytes(n, m, count) (one pack of the prediction per rotation of the batch).
 * zs_pose_apply: out[n][3] = normalize_pc(rotations[index[0]] pred) (index: device int32;
 * scratch: 64 bytes).  zs_normalize_pc: out[b][n][3] = normalize_pc(pc[b][n][3]) (scratch: 64 b
 * bytes).  zs_fscore: out[b][n_thresholds] from UN-squared distances dist1[b][n], dist2[b][m].
 *
 * Removed in ABI 46 (DESIGN.md section 4c names them): the unsorted search entry and its scratch size, the three entry
 * points of the uniform-grid arm and the two of the Z-order sort.
 * ------------------------------------------------------------------------- */
int zs_pose_max_batch(void);
size_t zs_pose_best_bytes(void);
int zs_pose_best_init(float *best, void *stream);
size_t zs_str_scratch_bytes(int n);
int zs_str_sort(const float *points, int n, float *sorted, int *perm, void *scratch, void *stream);
size_t zs_pose_pack_bytes(int points);
int zs_pose_pack(const float *sorted_points, int points, float *pack, void *stream);
size_t zs_pose_sorted_scratch_bytes(int n, int m, int count);
int zs_pose_search_batch_sorted(const float *pred, const float *pred_sorted, int n, const float *gt_sorted,
                                const float *gt_pack, int m, const float *rotations, const int *order, int count,
                                int index_offset, const float *lower_bound, const float *thresholds6, float *best,
                                void *scratch, int mode, void *stream);
int zs_pose_apply(const float *pred, int n, const float *rotations, const int *index, float *out,
                  void *scratch, void *stream);
int zs_normalize_pc(const float *pc, int b, int n, float *out, void *scratch, void *stream);
/* standardize_pc (utils/eval_3D.py:83-91): zero mean, RMS distance from the origin 1/2; pc, out [b][n][3].
 * zs_icp_step: one iteration of the reference's ICP (utils/eval_3D.py:276-283) after its Chamfer call: idx1 [b][n] =
 * nearest neighbour of x1's points in x2 (zs_chamfer_forward's idx1) -> centroids, 3x3 cross-covariance (double sums),
 * R = V U^T from its SVD (Jacobi on the device) with the reference's sign rule, x1_out = (x1 - t1) R^T + t2.  x1_out
 * must not alias x1.  scratch: zs_icp_scratch_bytes(b) (R, t1, t2 per batch element stay there). */
int zs_standardize_pc(const float *pc, int b, int n, float *out, void *stream);
size_t zs_icp_scratch_bytes(int b);
int zs_icp_step(const float *x1, int n, const float *x2, int m, const int *idx1, int b, float *x1_out, void *scratch,
                void *stream);
int zs_fscore(const float *dist1, int n, const float *dist2, int m, int b, const float *thresholds,
              int n_thresholds, float *out, void *stream);

/* ------------------------------------------------------------------------- *
 * Iso-surface extraction + surface sampling (replaces convert_to_explicit,
 * utils/eval_3D.py:233-263: PyMCubes marching_cubes + trimesh sample on the host).
 * Case tables come from the caller (zeroshape_amd/mc_tables.py): tri_table int8
 * [256][table_stride] (edge ids, -1 padded), tri_count uint8 [256].
 *
 *   zs_mc_count  : triangle counts per unit of 256 cubes -> exclusive offsets and the list of non-empty
 *                  units in `scratch` (zs_mc_scratch_bytes(G), 8-byte aligned) and the grand total in
 *                  *total (device int); one read of the volume with 16-byte row loads
 *   zs_mc_emit   : tris[n_tris][3][3] fp32 triangle soup in world space
 *                  (index * scale + offset), cube order x-slowest, deterministic; reads the volume
 *                  only in the non-empty units (one wave each, a lane per triangle)
 *   zs_mesh_sample: n_samples area-weighted points (counter-based RNG, `seed`);
 *                  cum_area = scratch of zs_mesh_sample_scratch_doubles(n_tris) doubles (the cumulative
 *                  areas and the tile totals of their scan); an empty mesh yields zeros
 * vol is [G][G][G] fp32 (x slowest), a cube corner is "inside" when value < iso.
 * ------------------------------------------------------------------------- */
size_t zs_mc_scratch_bytes(int G);
size_t zs_mesh_sample_scratch_doubles(int n_tris);
int zs_mc_count(const float *vol, int G, float iso, const uint8_t *tri_count, void *scratch,
                int *total, void *stream);
int zs_mc_emit(const float *vol, int G, float iso, const int8_t *tri_table, int table_stride,
               const uint8_t *tri_count, const void *scratch, float scale, float offset,
               float *tris, int n_tris, void *stream);
int zs_mesh_sample(const float *tris, int n_tris, int n_samples, uint64_t seed, double *cum_area,
                   float *points, void *stream);

/* ------------------------------------------------------------------------- *
 * Welding a triangle soup tris[n_tris][3][3] fp32 into the indexed form mcubes.marching_cubes
 * returns (utils/eval_3D.py:250-256), with the vertex normals trimesh derives for free.  Any
 * soup: corners weld when their coordinates are equal, whatever produced them.
 *   key of a corner : the uint32 bit patterns of (x + 0.0f, y + 0.0f, z + 0.0f): -0.0 and 0.0
 *                     are one vertex
 *   vertex order    : ascending (x, y, z) key, lexicographic, compared as UNSIGNED INTEGERS -
 *                     the row order of np.unique(keys, axis=0), not float order (negative
 *                     coordinates come after positive ones, descending)
 *   vertices [V][3] : the unchanged bits of the FIRST corner in soup order that has the key
 *   faces [n_tris][3]: int32, faces[t][k] = index of the vertex of corner 3 t + k
 *   normals [V][3]  : or NULL.  N = sum of cross(v1 - v0, v2 - v0) over the triangles of the
 *                     vertex's corners in ascending soup order (a triangle that holds the vertex
 *                     twice counts twice), every operation in fp64 as written; N / |N| in fp64,
 *                     rounded to fp32; (0, 0, 0) when |N| is zero, infinite or NaN
 * A stable radix sort of the corners, head flags, one scan, a scatter; a thread per vertex for
 * the vertices and normals.  No atomics: two runs give the same bits.
 *   zs_mesh_weld          writes faces and the vertex count *n_verts (device int); the caller
 *                         reads those 4 bytes, allocates, and calls
 *   zs_mesh_weld_vertices with the SAME tris, n_tris and scratch, untouched in between.
 *                         n_verts above the weld's own count writes only the weld's vertices.
 * scratch: zs_mesh_weld_scratch_bytes(n_tris) bytes, 8-byte aligned (0 for n_tris <= 0 and
 * beyond the limit n_tris <= 2^29).  n_tris == 0 is a mesh of zero vertices: both calls return 1
 * and touch nothing, *n_verts included.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_weld_scratch_bytes(int n_tris);
int zs_mesh_weld(const float *tris, int n_tris, int *faces, int *n_verts, void *scratch, void *stream);
int zs_mesh_weld_vertices(const float *tris, int n_tris, const void *scratch, int n_verts,
                          float *vertices, float *normals, void *stream);

/* ------------------------------------------------------------------------- *
 * Connected components of an indexed mesh, their counts and measures, and the removal of
 * components from the soup (csrc/mesh_components.hip; eval_3D.mesh_components_host restates all
 * of it in numpy and defines it).  faces [n_tris][3] int32 over n_verts vertices is the weld's
 * output, tris [n_tris][3][3] the soup it was made from.
 *   components : two vertices are connected when some face holds both (a shared vertex is
 *                enough, an edge is not needed).  Label = the rank of the component's smallest
 *                vertex index.  vertex_labels [n_verts], face_labels [n_tris] (the label of the
 *                face's first vertex), out[2] (device ints) = the component count and a status
 *                word: 0, or nonzero when a loop ran into its bound (1) or a face index lies
 *                outside [0, n_verts) (2) - the labels are then not to be used.
 *                A lock-free union-find over the faces, a flattening kernel, one scan.
 *   stats      : after the caller has read the count.  counts [n_comps][8] int32 = faces,
 *                vertices, degenerate faces (two equal indices), edges (unique vertex pairs of the
 *                other faces), boundary edges (used once), non-manifold edges (used more than
 *                twice), misoriented edges (used twice, in the same direction), Euler number
 *                V - E + (F - degenerate).  measures [n_comps][2] fp64 = area (sum of
 *                |cross(v1 - v0, v2 - v0)| / 2) and signed volume (sum of v0 . cross(v1, v2) / 6)
 *                from the soup's fp32 corners, every operation in fp64 as written in the checker;
 *                a degenerate face adds exactly 0.  The integers by integer atomics; the sums by a
 *                stable sort of the faces by label and a fixed-shape segmented reduction - no
 *                floating-point atomics, two runs give the same bits.
 *   select     : keep[c] = explicit_keep[c] != 0 when explicit_keep (uint8 [n_comps]) is given;
 *                otherwise area[c] >= min_rel_area * max(area) (fp64; min_rel_area = 0 switches
 *                the area rule off) and, with drop_cavities, not (closed and signed volume < 0),
 *                closed = at least one non-degenerate face and no boundary, non-manifold or
 *                misoriented edge.  keep_pos [n_tris] int32 = the inclusive scan of the faces'
 *                keep flags, *n_kept (device int) = its last element.
 *   filter     : after the caller has read n_kept: out_tris[keep_pos[f] - 1] = tris[f] for the
 *                kept faces - the soup's order is preserved.
 * scratch: zs_mesh_components_scratch_bytes(n_tris, n_verts) bytes, 8-byte aligned, for any of the
 * calls (0 for empty and out-of-range sizes); nothing is carried in it from one call to the next.
 * Limits: n_tris <= 2^29, n_verts <= 3 n_tris, n_comps <= n_verts.  Zero sizes return 1 and touch
 * nothing.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_components_scratch_bytes(int n_tris, int n_verts);
int zs_mesh_components(const int *faces, int n_tris, int n_verts, int *vertex_labels, int *face_labels, int *out,
                       void *scratch, void *stream);
int zs_mesh_component_stats(const float *tris, const int *faces, const int *vertex_labels, const int *face_labels,
                            int n_tris, int n_verts, int n_comps, int *counts, double *measures, void *scratch,
                            void *stream);
int zs_mesh_components_select(const int *counts, const double *measures, int n_comps, double min_rel_area,
                              int drop_cavities, const uint8_t *explicit_keep, const int *face_labels, int n_tris,
                              int n_verts, int *keep_pos, int *n_kept, void *scratch, void *stream);
int zs_mesh_filter_faces(const float *tris, const int *keep_pos, int n_tris, float *out_tris, int n_kept, void *stream);

/* ------------------------------------------------------------------------- *
 * The vertex neighbourhood of an indexed mesh and Laplacian / Taubin smoothing over it
 * (csrc/mesh_smooth.hip; eval_3D.mesh_adjacency_host and eval_3D.smooth_vertices_host restate
 * both in numpy and define them: the kernels equal them bit for bit).  faces [n_tris][3] int32
 * over n_verts vertices is the weld's output.
 *   adjacency : a face with two equal indices contributes no edges, every other face its three
 *               undirected edges.  offsets [n_verts + 1] int32; neighbors int32, allocated by the
 *               caller for 6 n_tris entries, of which the first nnz = offsets[n_verts] are
 *               written: row v = neighbors[offsets[v] .. offsets[v + 1]) holds the distinct other
 *               endpoints of v's edges in ascending order.  boundary [n_verts] uint8 = 1 iff some
 *               edge at the vertex is used by exactly one non-degenerate face (an edge used three
 *               or more times is not a boundary edge).  out[2] (device ints) = nnz and a status
 *               word: 0, or 2 when a face index lies outside [0, n_verts) - such a face
 *               contributes nothing, and no index is used as an address before it is tested.
 *               One radix sort of the 6 n_tris directed entries (64-bit keys), head flags, one
 *               scan, a binary search per vertex.  Integers only and no atomic whose order
 *               matters: two runs give the same bytes.
 *   smooth    : `passes` passes over positions kept in fp64 between passes.  Pass t (from 0) uses
 *               f = lambda, or f = mu when `alternate` is set and t is odd.  A vertex moves iff its
 *               row is not empty and it is not pinned (boundary given and boundary[v] != 0):
 *                 s = 0; for k in row order: s = s + x[neighbors[k]];  m = s / (double)degree;
 *                 x' = x + f * (m - x)
 *               per coordinate, every operation in fp64 as written; the other vertices are copied.
 *               After the last pass the positions are rounded to fp32 into out_vertices (not the
 *               input); passes == 0 copies the input's bits.  *status (device int) = 0, or
 *               nonzero when a row had offsets[v] < 0, offsets[v + 1] < offsets[v] or
 *               offsets[v + 1] > offsets[n_verts] (1) or a neighbour index outside [0, n_verts)
 *               (2): such a row is not followed and its vertex is copied.  A thread per vertex
 *               walks its row - the order of the additions is the contract - and every pass is a
 *               launch of its own.  0 < lambda <= 1; -1 <= mu < 0 when `alternate` is set.
 *               neighbors may be NULL for an adjacency without edges: a row that is not empty
 *               then sets the status (1).
 *   gather    : out_tris[f][k] = vertices[faces[f][k]]: the soup of an indexed mesh in face
 *               order (NaN for an index outside [0, n_verts)).
 * scratch, 8-byte aligned: zs_mesh_adjacency_scratch_bytes(n_tris, n_verts) and
 * zs_mesh_smooth_scratch_bytes(n_verts) bytes (0 for empty and out-of-range sizes; smoothing needs
 * none for passes <= 1).  Limits: those of zs_mesh_components, except n_tris <= 2^28 - the
 * 6 n_tris directed entries are counted in int32; n_verts <= 3 * 2^28 for the smoothing.  Zero
 * sizes return 1 and touch nothing.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_adjacency_scratch_bytes(int n_tris, int n_verts);
int zs_mesh_adjacency(const int *faces, int n_tris, int n_verts, int *offsets, int *neighbors, uint8_t *boundary, int *out,
                      void *scratch, void *stream);
size_t zs_mesh_smooth_scratch_bytes(int n_verts);
int zs_mesh_smooth(const float *vertices, int n_verts, const int *offsets, const int *neighbors, const uint8_t *boundary,
                   int passes, double lambda, double mu, int alternate, float *out_vertices, int *status, void *scratch,
                   void *stream);
int zs_mesh_gather_faces(const float *vertices, const int *faces, int n_tris, int n_verts, float *out_tris, void *stream);

/* ------------------------------------------------------------------------- *
 * Mesh simplification by uniform-grid vertex clustering with quadric-error placement
 * (csrc/mesh_simplify.hip; the semantics are eval_3D.simplify_mesh_host's, bit for bit).
 * vertices [n_verts,3] fp32 and faces [n_tris,3] int32 are the weld's (zs_mesh_weld); origin is
 * a DEVICE pointer to 3 doubles (the caller may have computed it on the device: nothing is read
 * back), cell the cluster edge, mode 1 = quadric placement, 0 = the cluster mean.
 *   cells     : c = floor(((double)v - origin) / cell) per axis, each in [0, 2^21); vertices with
 *               equal (cx, cy, cz) form a cluster; cluster ids ascend with cx << 42 | cy << 21 | cz.
 *   mean      : in coordinates local to the cell centre origin + (c + 0.5) cell: the members'
 *               local positions added in fp64 in ascending vertex index, divided by the count.
 *   quadrics  : every (face, corner) adds, to the cluster of that corner's vertex, the plane
 *               quadric n n^T / |n| of its face (n = (v1 - v0) x (v2 - v0), |n| = twice the area:
 *               area weighting), built in fp64 from the three fp32 vertices in that cluster's local
 *               coordinates; a face whose |n| is zero or not finite adds nothing.  Summed per
 *               cluster in ascending 3 face + corner.
 *   placement : minimise x^T A x + 2 b^T x + w |x - m|^2, w = 1e-3 trace(A) / 3 (the constant is a
 *               design choice): (A + w I) x = w m - b by Cramer's rule.  The mean m instead when
 *               the trace is not positive, x is not finite or some |x| component exceeds cell
 *               (counted in out_counts[5]).  A cluster of one vertex keeps that vertex's bits.
 *               representative = (float)(centre + x).
 *   faces     : corners -> cluster ids; a face with two equal ids is dropped (degenerate); among
 *               faces whose ids are equal up to rotation the first in input order is kept, the
 *               others are dropped (duplicate); a face and its mirror image are both kept.  The
 *               kept faces go to out_tris [n_tris,3,3] (room for every input face) in input face
 *               order with the input's corner order, each corner its cluster's representative.
 * out_counts[6] (device ints): kept, clusters, degenerate, duplicate, status, fallbacks.  status:
 * 0, |1 when a coordinate is not finite or a cell index lies outside [0, 2^21) (such a vertex is
 * put into cell 0), |2 when a face index lies outside [0, n_verts) (such a face is dropped and
 * counted with the degenerate ones; no index is used as an address before it is tested).  The
 * call only enqueues: it returns 1 whatever the status word will say.
 * scratch, 8-byte aligned: zs_mesh_simplify_scratch_bytes(n_tris, n_verts) bytes (0 for empty and
 * out-of-range sizes).  Limits: n_tris <= 2^28, n_verts <= 2^21 (three cluster ids share one 63-bit
 * sort key), n_verts <= 3 n_tris.  Zero sizes return 1 and touch nothing.
 * Every sum is walked by one thread in a fixed order and the counters are integer atomics: two
 * runs give the same bytes.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_simplify_scratch_bytes(int n_tris, int n_verts);
int zs_mesh_simplify(const float *vertices, const int *faces, int n_tris, int n_verts, const double *origin, double cell,
                     int mode, float *out_tris, int *out_counts, void *scratch, void *stream);

/* ------------------------------------------------------------------------- *
 * Exact distance from points to a triangle mesh (csrc/mesh_distance.hip; the semantics are
 * eval_3D.closest_point_on_mesh_host's, bit for bit).  vertices [n_verts,3] fp32 and faces
 * [n_faces,3] int32 are the weld's (zs_mesh_weld), queries [n_queries,3] fp32.
 * For every query the lexicographic minimum over the valid faces of (d2, face index):
 *   out_sqdist [n_queries] fp64, out_face [n_queries] int32, out_closest [n_queries,3] fp64 (may be
 *   NULL): the closest point of that face.  The point is the best of four fp64 candidates, taken in
 *   this order, a later one only when strictly closer: the closest points of the segments (a, b),
 *   (a, c), (b, c) - p0 when t = (q - p0).(p1 - p0) <= 0, p1 when t >= l = |p1 - p0|^2, else
 *   p0 + (t / l)(p1 - p0) - and the foot of the perpendicular (a + (h / nn) u) + (g / nn) v when it
 *   lies inside (nn = |u x v|^2 > 0, h = ((q - a) x v).n >= 0, g = (u x (q - a)).n >= 0, h + g <= nn).
 *   d2 = (dx dx + dy dy) + dz dz.  Nothing is divided by zero: a face of zero area is the union of
 *   its edges (a segment; a point when the corners are equal).  A query at a vertex gives exactly 0.
 *   A face with an index outside [0, n_verts) or a corner that is not finite is skipped (no index is
 *   used as an address before it is tested); a query that is not finite gets NaN, -1, NaN; with no
 *   valid face every finite query gets +inf, -1, NaN.
 * out_counts[5] (device ints): skipped faces, queries that are not finite, status (|1 a corner that
 * is not finite, |2 a face index outside the vertices, |4 a query that is not finite), and the
 * number of evaluated (query, face) pairs as two 32-bit halves, low first.
 * The search is a uniform grid over the faces (each binned once, by the centre of its box; at most
 * 64^3 cells, about two faces per cell) walked ring by ring under a bound that skips a face only
 * when its d2 is provably larger: the result equals the scan over all faces.  The call only
 * enqueues: it returns 1 whatever the status word will say.
 * scratch, 8-byte aligned: zs_mesh_distance_scratch_bytes(n_faces, n_queries) bytes (a multiple of
 * 256; 0 for sizes outside the limits n_faces <= 2^24, n_queries <= 2^28).  n_queries = 0 returns
 * 1 and touches nothing; n_faces = 0 is an empty mesh.
 *
 * zs_mesh_distance_stats: out[4] fp64 = the largest d, the mean d, the rms d and the number n of
 * entries of sqdist [n] that are finite (the others are left out), d = sqrt(d2); *out_index = the
 * lowest index with the largest d (-1 and NaNs when n is 0).  One workgroup of 256 threads: thread
 * t adds its elements i = t, t + 256, ... in ascending i, thread 0 the 256 partial sums in
 * ascending t: a fixed sequence of fp64 additions.  n = 0 returns 1 and touches nothing.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_distance_scratch_bytes(int n_faces, int n_queries);
int zs_mesh_distance(const float *vertices, const int *faces, int n_faces, int n_verts, const float *queries, int n_queries,
                     double *out_sqdist, int *out_face, double *out_closest, int *out_counts, void *scratch, void *stream);
int zs_mesh_distance_stats(const double *sqdist, int n, double *out, int *out_index, void *stream);

/* ------------------------------------------------------------------------- *
 * On which side of a triangle mesh a point lies (csrc/mesh_inside.hip; the semantics are
 * eval_3D.mesh_winding_host's, exactly).  vertices [n_verts,3] fp32 and faces [n_faces,3] int32 are
 * the weld's (zs_mesh_weld), queries [n_queries,3] fp32.
 * For every query the signed crossing numbers of the +z ray (out_up [n_queries] int32) and of the
 * -z ray (out_down [n_queries] int32, may be NULL) over the valid faces.  fp64 as written, from the
 * fp32 corners a, b, c and the fp32 query q:
 *   box     a face is a candidate only if min(ax, bx, cx) <= qx <= max(ax, bx, cx), and so in y.
 *   side    of each directed edge u -> v (a -> b, b -> c, c -> a): (lo, hi) = its endpoints ordered
 *           lexicographically by their (x, y, z) values; s = (hx - lx)(qy - ly) - (hy - ly)(qx - lx);
 *           where s == 0: -sign(hy - ly) if hy != ly, else sign(hx - lx); negated when the face
 *           walks the edge hi -> lo (a symbolic shift of q by (eps, eps^2): no ray meets an edge).
 *   facing  up when the three sides are > 0, down when they are < 0, else the face does not count.
 *   height  A = a - q, B = b - q, C = c - q,
 *           det = (Ax (By Cz - Bz Cy) + Ay (Bz Cx - Bx Cz)) + Az (Bx Cy - By Cx); 0 counts for neither.
 *   up = #(up-facing, det > 0) - #(down-facing, det < 0), down = #(down-facing, det > 0) -
 *   #(up-facing, det < 0).  For a closed mesh wound like marching cubes' both are the winding number.
 *   A face with an index outside [0, n_verts) or a corner that is not finite is skipped (no index is
 *   used as an address before it is tested); a query that is not finite gets 0, 0.
 * out_counts[5] (device ints): as zs_mesh_distance's - skipped faces, queries that are not finite,
 * status (|1 a corner that is not finite, |2 a face index outside the vertices, |4 a query that is
 * not finite), and the number of (query, face) pairs read, as two 32-bit halves, low first.
 * The search is a uniform grid of columns over x, y (each face binned once, by the centre of its
 * box; at most 1024^2 columns, about two faces per column); a query visits the columns that can
 * hold a face whose box contains it, found with integer reaches through one monotone index
 * function: the counts equal the scan over all faces.  The call only enqueues.
 * scratch, 8-byte aligned: zs_mesh_winding_scratch_bytes(n_faces, n_queries) bytes (a multiple of
 * 256; 0 for sizes outside the limits n_faces <= 2^24, n_queries <= 2^28).  n_queries = 0 returns 1
 * and touches nothing; n_faces = 0 is an empty mesh.
 *
 * zs_mesh_winding_grid: the same for the G^3 lattice points (fmaf(ix, scale, offset),
 * fmaf(iy, scale, offset), fmaf(iz, scale, offset)) - marching cubes' own vertex formula - made in
 * the kernel: out_inside [G^3] int8, x slowest, = (up != 0).  out_counts[6]: the five words above and
 * the number of ambiguous points (up != down).  scratch: zs_mesh_winding_scratch_bytes(n_faces, G^3);
 * G <= 645 (G^3 <= 2^28); G = 0 returns 1 and touches nothing.
 *
 * zs_occupancy_counts: out[4] int64 (device, 8-byte aligned) = |A|, |B|, |A and B|, |A or B| of two
 * int8 arrays of n elements (non-zero = inside): integer sums, exact.  n = 0 writes four zeros.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_winding_scratch_bytes(int n_faces, int n_queries);
int zs_mesh_winding(const float *vertices, const int *faces, int n_faces, int n_verts, const float *queries, int n_queries,
                    int *out_up, int *out_down, int *out_counts, void *scratch, void *stream);
int zs_mesh_winding_grid(const float *vertices, const int *faces, int n_faces, int n_verts, int G, float scale, float offset,
                         signed char *out_inside, int *out_counts, void *scratch, void *stream);
int zs_occupancy_counts(const signed char *a, const signed char *b, long long n, long long *out, void *stream);

/* ------------------------------------------------------------------------- *
 * Where a ray first meets a triangle mesh (csrc/mesh_rays.hip; the semantics are
 * eval_3D.mesh_rays_host's, bit for bit).  vertices [n_verts,3] fp32 and faces [n_faces,3] int32 are
 * the weld's (zs_mesh_weld), origins and directions [n_rays,3] fp32, t_min <= t <= t_max the range
 * of the ray parameter (both ends inclusive; -inf and +inf allowed).
 * The watertight test of Woop, Benthin and Wald (2013), fp64 as written from the fp32 values:
 *   ray     kz = the first axis with the largest |d|, kx = (kz + 1) mod 3, ky = (kx + 1) mod 3, kx and
 *           ky swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
 *   face    A = a - o; Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], Az = Sz A[kz]; so for B and C;
 *           U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax; det = (U + V) + W;
 *           t = ((U Az + V Bz) + W Cz) / det.
 *   hit     iff U, V, W are all >= 0 or all <= 0, det != 0, t_min <= t <= t_max and t is finite.
 *   result  the smallest t, the lowest face index among equal t: out_t [n_rays] fp64 (+inf for a
 *           miss), out_face [n_rays] int32 (-1), out_side [n_rays] int8 (+1 when det > 0: the ray
 *           meets the face against its normal (b - a) x (c - a); -1 from behind; 0 for a miss) and
 *           out_bary [n_rays,3] fp64 (may be NULL): U / det, V / det, W / det, the weights of
 *           a, b, c (NaN for a miss).
 *   A face with an index outside [0, n_verts) or a corner that is not finite is skipped (no index is
 *   used as an address before it is tested); a ray with a component that is not finite or with
 *   d = 0 gets (NaN, -1, 0).
 * out_counts[5] (device ints): as zs_mesh_distance's - skipped faces, invalid rays, status (|1 a
 * corner that is not finite, |2 a face index outside the vertices, |4 an invalid ray), and the
 * number of (ray, face) pairs read, as two 32-bit halves, low first.
 * The search is the uniform grid of zs_mesh_distance (each face binned once, by the centre of its
 * box; at most 64^3 cells) walked slab by slab along the ray's major axis with the integer reaches
 * of zs_mesh_winding; it ends when the next slab begins beyond the best t.  The call only enqueues.
 * scratch, 8-byte aligned: zs_mesh_rays_scratch_bytes(n_faces, n_rays) bytes (a multiple of 256; 0
 * for n_rays = 0 and for sizes outside the limits n_faces <= 2^24, n_rays <= 2^28).  n_rays = 0
 * returns 1 and touches nothing; n_faces = 0 is an empty mesh.
 *
 * zs_mesh_rays_image: the same for the H x W rays of a pinhole camera, made in the kernel
 * (eval_3D.camera_rays_host): pixel (row i, col j) is at (j, i, 1), D = K^-1 (j, i, 1) by the
 * adjugate in fp64 from intr [9] fp32 (device), D / D_z, o = -mean / scale and d = D / scale
 * (mean [3], scale [1] fp32, device) rounded to fp32; a pixel whose D_z is not > 0 and finite is an
 * invalid ray.  out_depth [H,W] fp32 = (float)t - the camera depth Z of the first surface -
 * out_face [H,W] int32, out_side [H,W] int8.  out_counts[6]: the five words above and the number of
 * pixels that hit.  scratch: zs_mesh_rays_scratch_bytes(n_faces, H * W); H, W <= 16384 and
 * H * W <= 2^28; H = 0 or W = 0 returns 1 and touches nothing.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_rays_scratch_bytes(int n_faces, int n_rays);
int zs_mesh_rays(const float *vertices, const int *faces, int n_faces, int n_verts, const float *origins, const float *directions,
                 int n_rays, double t_min, double t_max, double *out_t, int *out_face, signed char *out_side, double *out_bary,
                 int *out_counts, void *scratch, void *stream);
int zs_mesh_rays_image(const float *vertices, const int *faces, int n_faces, int n_verts, const float *intr, const float *mean,
                       const float *scale, int H, int W, double t_min, double t_max, float *out_depth, int *out_face,
                       signed char *out_side, int *out_counts, void *scratch, void *stream);

/* ------------------------------------------------------------------------- *
 * Which faces of a triangle mesh pass through each other (csrc/mesh_selfx.hip; the semantics are
 * eval_3D.mesh_self_intersections_host's, in every integer).  vertices [n_verts,3] fp32 and faces
 * [n_faces,3] int32 are the weld's (zs_mesh_weld).  fp64 as written, from the fp32 corners of two
 * valid faces i != j:
 *   box     a candidate pair only if the fp32 boxes overlap on every axis, ends included.
 *   det     det(D, L, H) = (Dx (Ly Hz - Lz Hy) + Dy (Lz Hx - Lx Hz)) + Dz (Lx Hy - Ly Hx).
 *   segment (p, q) = its ends ordered lexicographically by their (x, y, z) values, against the face
 *           (a, b, c): sp = det(a - p, b - p, c - p), sq = det(a - q, b - q, c - q) strictly of
 *           opposite signs; D = q - p; for each directed edge u -> v of a -> b, b -> c, c -> a:
 *           (lo, hi) = u, v ordered by value, e = det(D, lo - p, hi - p), negated when the face walks
 *           hi -> lo; crosses iff the three e are all >= 0 or all <= 0 and not all 0.
 *   cross   iff an edge of one crosses the other, either way round.  Touching, coplanar overlap and
 *           the contact of faces that share a vertex or an edge are not crossings (sp = 0 exactly).
 *   coincident  iff the three corner positions of one are those of the other in some order, by value
 *           (either orientation): the one coplanar case that is counted, separately.
 *   A face with an index outside [0, n_verts) or a corner that is not finite is skipped (no index is
 *   used as an address before it is tested) and crosses nothing.
 * out_face_counts [n_faces] int32: the number of other faces each face crosses (plain stores).
 * out_pairs [capacity,2] int32 (may be NULL with capacity 0): the crossing pairs (i, j), i < j, in
 * lexicographic order - the first `capacity` of them when there are more; rows beyond the total are
 * not touched.
 * out_counts[9] (device ints): skipped faces, status (|1 a corner that is not finite, |2 a face index
 * outside the vertices), crossing pairs (i < j) as two 32-bit halves, low first, coincident pairs
 * likewise, faces with a count > 0, and the ORDERED candidate pairs examined (every record read with
 * j != i, before the box test; each face counts all j != i it crosses, so a pair is tested from both
 * sides) as two halves.
 * The search is the uniform grid of zs_mesh_distance (each face binned once, by the centre of its
 * box; at most 64^3 cells) with the integer reaches of zs_mesh_winding through one monotone index
 * function: the counts equal the test of all pairs.  The call only enqueues.
 * scratch, 8-byte aligned: zs_mesh_self_intersections_scratch_bytes(n_faces, capacity) bytes (a
 * multiple of 256; 0 for sizes outside the limits n_faces <= 2^24, capacity <= 2^30).  n_faces = 0 is
 * an empty mesh: nine zeros.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_self_intersections_scratch_bytes(int n_faces, int capacity);
int zs_mesh_self_intersections(const float *vertices, const int *faces, int n_faces, int n_verts, int *out_face_counts,
                               int *out_pairs, int capacity, int *out_counts, void *scratch, void *stream);

/* ------------------------------------------------------------------------- *
 * Vertex normals from the occupancy field's own gradient (csrc/field_normals.hip; the gradient
 * itself is Implicit.field_gradient's, between the two calls).
 *   to_field_points : marching cubes scales a vertex at grid index u to v = min + u (max - min) / G
 *                     with G samples per axis (utils/eval_3D.py:252-255), but sample u of
 *                     linspace(min, max, G) lies at min + u (max - min) / (G - 1).  points[i] =
 *                     min + (vertices[i] - min) G / (G - 1), where the field that made the vertex
 *                     was evaluated: fp64 as written, rounded to fp32.  n vertices of 3 floats; G >= 2.
 *   finish          : normals[v] = -grad[v] / |grad[v]| (occupancy rises inwards), length and
 *                     division in fp64, rounded to fp32.  Where |grad[v]| is zero, infinite or NaN:
 *                     fallback[v] (or (0, 0, 0) when fallback is NULL), and *n_fallback (device
 *                     int, zeroed by the caller) is incremented.
 * ------------------------------------------------------------------------- */
int zs_mesh_to_field_points(const float *vertices, size_t n, float range_min, int G, float *points, void *stream);
int zs_field_normals_finish(const float *grad, const float *fallback, size_t n, float *normals, int *n_fallback,
                            void *stream);

/* ------------------------------------------------------------------------- *
 * Mesh turntable renderer (replaces dump_meshes_viz / scale_to_unit_cube / visualize_mesh,
 * utils/util_vis.py:112-127, 310-405: trimesh + pyrender on OpenGL).  A z-buffer rasteriser
 * over the triangle soup tris[n_tris][3][3] that zs_mc_emit writes; all frames of a camera
 * path in one call.  pyrender's PBR pixels are not reproduced (parity unpinned: no GL here);
 * the geometry and the shading formula below are what the tests pin.
 * ------------------------------------------------------------------------- */

/* Bounding box and signed volume of the soup: out[7] (device) = min xyz, max xyz,
 * sum(v0 . (v1 x v2)) / 6 (accumulated in fp64).  Per-block partials in `scratch`
 * (zs_mesh_stats_scratch_bytes(n_tris) bytes, 8-byte aligned) are summed by one block in a
 * fixed order: no float atomics, bit-reproducible.  n_tris == 0 writes seven zeros (tris and
 * scratch may then be NULL). */
size_t zs_mesh_stats_scratch_bytes(int n_tris);
int zs_mesh_stats(const float *tris, int n_tris, float *out, void *scratch, void *stream);

/* Renders `frames` views of the soup into rgb[frames][H][W][3] uint8 and, when not NULL,
 * depth[frames][H][W] fp32 (camera-space distance along the view axis, +inf where nothing is
 * hit) and tri[frames][H][W] int32 (index of the visible triangle, -1 where nothing is hit).
 *   xform [host][8]  : flip xyz, centre xyz, scale, winding - every vertex becomes
 *                      (flip * v - centre) * scale on the fly (never written back), and v1 / v2
 *                      of every triangle are exchanged when winding < 0
 *   cams [frames][12]: camera position (3) + camera-to-world rotation (3x3, row-major); the
 *                      camera looks along -z of its own frame, +y is up (pyrender's convention)
 *   yfov, znear      : vertical field of view in radians (aspect = W / H), near plane
 *   base_rgb [host][3]: material colour; c = base * (0.3 + 0.7 |n . l|) per face, n = unit face
 *                      normal, l = unit vector from the hit point to the camera; stored
 *                      floor(255 c + 0.5); the background is white
 *   zbuffer          : zs_render_zbuffer_bytes(frames, H, W) bytes of scratch, 8-byte aligned
 * With zv = -z_c: x_pix = (x_c / (zv tan(yfov/2) aspect) + 1) W/2 and
 * y_pix = (1 - y_c / (zv tan(yfov/2))) H/2; the centre of pixel (row i, col j) is
 * (j + 0.5, i + 0.5); a pixel is covered when its three barycentrics are >= 0 (inclusive on
 * every edge).  Depth is perspective correct; the nearest depth wins and at exactly equal
 * (fp32) depth the smaller triangle index: one 64-bit atomic maximum per covered pixel, so the
 * result does not depend on the order of execution.  Zero-area triangles and triangles with a
 * vertex at zv <= znear are skipped whole.  n_tris == 0 gives white frames (tris may be NULL);
 * frames == 0 does nothing.  Limits: frames <= 65535, H and W <= 16384 (the size function
 * returns 0 beyond them). */
size_t zs_render_zbuffer_bytes(int frames, int H, int W);
int zs_render_frames(const float *tris, int n_tris, const float *xform, const float *cams,
                     int frames, int H, int W, float yfov, float znear, const float *base_rgb,
                     uint8_t *rgb, float *depth, int *tri, void *zbuffer, void *stream);

/* The same frames with a colour per triangle corner instead of one base colour:
 * corner_rgb [n_tris][3][3] uint8 (corner k of triangle t, then r g b; may be NULL when n_tris == 0).
 * Clear and scatter are zs_render_frames': depth and tri are the same bits.  The resolve recomputes
 * the winner's projected corners and w0, w1, w2 at the pixel centre exactly as the scatter did and
 * interpolates the albedo perspective-correctly in fp64, a = (sum w_k / z_k c_k / 255) / (sum w_k / z_k);
 * the pixel is floor(255 a (0.3 + 0.7 |n . l|) + 0.5); the background is white. */
int zs_render_frames_colored(const float *tris, int n_tris, const float *xform, const float *cams,
                             int frames, int H, int W, float yfov, float znear, const uint8_t *corner_rgb,
                             uint8_t *rgb, float *depth, int *tri, void *zbuffer, void *stream);

/* ------------------------------------------------------------------------- *
 * Vertex colours of a predicted mesh from the input photo (csrc/mesh_colors.hip;
 * eval_3D.mesh_vertex_colors_host restates all of it in float64 numpy, operation for operation, and
 * defines it).  The mesh is the weld's: vertices [n_verts][3] fp32, faces [n_tris][3] int32, normals
 * [n_verts][3] fp32 (area weighted).  It lives in the normalised frame of the input camera: vertex v
 * sits at X = v scale + mean in the camera and projects through K (device: K[9] row-major, mean[3],
 * scale[1], fp32).  image [3][H][W] fp32 planar in [0, 1], mask [H][W] fp32; pixel (row i, col j) is
 * at (u, w) = (j, i).  Geometry in fp64 from the fp32 inputs, only + - * / sqrt floor and comparisons.
 *   seen    : p = K X, Z = p_z, u = p_x / p_z, w = p_y / p_z.  A z-buffer of ss H x ss W words in that
 *             camera by the rules of zs_render_frames' scatter (raster coordinates (u + 0.5) ss,
 *             (w + 0.5) ss; a face with a Z not > 0 or not finite is skipped whole).  A vertex is seen iff
 *             Z > 0 and finite, 0 <= u <= W - 1, 0 <= w <= H - 1; n . (-X) > min_cos |n| |X| (a zero or
 *             non-finite n fails); the four mask texels of its bilinear footprint (j0 = min(floor(u),
 *             max(W - 2, 0)), j1 = min(j0 + 1, W - 1), rows likewise) are > 0.5; and the z-buffer word at
 *             (min(floor((w + 0.5) ss), ss H - 1), min(floor((u + 0.5) ss), ss W - 1)) is 0, or names a
 *             face that holds the vertex, or Z <= (double)depth + depth_tol scale.  depth_tol is in
 *             mesh units.  Writes seen [n_verts] uint8, colors [n_verts][3] uint8 (the bilinear
 *             texel, floor(255 c + 0.5) clamped; 0 for a hidden vertex until the fill), source
 *             [n_verts] int32 (the vertex itself, -1 when hidden), *n_seen (device int: the caller reads
 *             these 4 bytes) and fraction[2] fp64 = the area of the faces whose three vertices are
 *             seen, and the total area (fixed-order block reduction, no float atomics).
 *   compact : after the caller has read n_seen, with the SAME workspace untouched in between:
 *             seen_idx [n_seen] / seen_xyz [n_seen][3] and hidden_idx / hidden_xyz [n_verts - n_seen],
 *             the vertex indices and positions in ascending vertex order.  The caller then finds the
 *             nearest seen vertex of every hidden one with zs_chamfer_forward_ws (xyz1 = hidden,
 *             xyz2 = seen, b = 1: squared distance, the lowest index among equal minima).
 *   fill    : hidden vertex k of the list takes the colour of seen_idx[nearest[k]], faded towards
 *             base_rgb [host][3]: t = fade > 0 ? min(sqrt(dist[k]) / fade, 1) : 0, c = (1 - t) c_nn + t 255 base
 *             on the uint8 c_nn, floor(c + 0.5) clamped; source = that seen vertex.  With n_seen == 0
 *             (seen_idx, nearest and dist may be NULL) every vertex gets 255 base and source -1.
 * workspace: zs_mesh_colors_workspace_bytes(n_verts, n_tris, H, W, ss) bytes, 8-byte aligned (0 for an
 * empty mesh and beyond the limits n_verts, n_tris <= 2^29, ss H and ss W <= 16384).  n_verts == 0
 * returns 1 and touches nothing.
 * ------------------------------------------------------------------------- */
size_t zs_mesh_colors_workspace_bytes(int n_verts, int n_tris, int H, int W, int ss);
int zs_mesh_colors_seen(const float *vertices, const int *faces, const float *normals, int n_verts, int n_tris,
                        const float *image, const float *mask, int H, int W, const float *K, const float *mean,
                        const float *scale, int ss, double depth_tol, double min_cos, uint8_t *colors, uint8_t *seen,
                        int *source, int *n_seen, double *fraction, void *workspace, void *stream);
int zs_mesh_colors_compact(const float *vertices, const uint8_t *seen, int n_verts, int n_seen, const void *workspace,
                           int *seen_idx, float *seen_xyz, int *hidden_idx, float *hidden_xyz, void *stream);
int zs_mesh_colors_fill(const int *hidden_idx, const int *seen_idx, const int *nearest, const float *dist, int n_verts,
                        int n_seen, double fade, const float *base_rgb, uint8_t *colors, int *source, void *stream);

/* ------------------------------------------------------------------------- *
 * Seen-surface mesh (replaces create_seen_surface, utils/util_vis.py:137-170): the textured
 * mesh of the surface the camera sees, from a camera-frame point map, in the reference's order.
 *   xyz  [B][H][W][3] : camera-frame points
 *   mask [B][H][W]    : or NULL; a pixel with mask <= 0.5 is invalid
 * A pixel is a vertex iff z > 0 (NaN is not) and its mask allows it; vertices are numbered from
 * 1 in raster order (y outer, x inner) per image.  Cells (y, x), y < H-1, x < W-1, in raster
 * order, the upper triangle first, then the lower:
 *   upper (y,x), (y,x+1), (y+1,x)     : three vertices, |P(y,x) - P(y,x+1)| < thr and
 *                                       |P(y,x) - P(y+1,x)| < thr
 *   lower (y,x+1), (y+1,x+1), (y+1,x) : three vertices, |P(y,x+1) - P(y+1,x+1)| < thr and
 *                                       |P(y,x+1) - P(y+1,x)| < thr
 * with |d| = sqrtf(dx*dx + dy*dy + dz*dz) in fp32 as written; a NaN length rejects.
 *   vert_id    [B][H][W]              : 1-based OBJ index of the pixel's vertex, 0 = none
 *   vert_pixel [B][H*W]               : compacted: raster index y*W + x of vertex k
 *   verts      [B][H*W][3]            : compacted: xyz of vertex k, bits unchanged
 *   faces      [B][2*(H-1)*(W-1)][3]  : compacted: 1-based vertex indices in the order above
 *                                       (may be NULL when H == 1 or W == 1: no cells)
 *   counts     [B][2]                 : (n_verts, n_faces)
 * Rows of the compacted buffers beyond `counts` are left unwritten.  Compaction is by prefix
 * scan, no atomics: the order is the reference's and two runs give the same bits.  workspace:
 * zs_seen_mesh_workspace_bytes(batch, H, W) bytes, 8-byte aligned.  batch, H or W == 0 does
 * nothing; batch * H * W <= 2^30 (the size function returns 0 beyond that). */
size_t zs_seen_mesh_workspace_bytes(int batch, int H, int W);
int zs_seen_mesh(const float *xyz, const float *mask, int batch, int H, int W, float connect_thres,
                 int *vert_id, int *vert_pixel, float *verts, int *faces, int *counts,
                 void *workspace, void *stream);

/* ------------------------------------------------------------------------- *
 * Seen-surface geometry front-end (model/compute_graph/graph_shape.py:131-144).
 * All maps are fp32, row-major, batch outermost.
 *
 *   zs_intr_param2mtx : params [B][3] = (scale_f, delta_cx, delta_cy) -> intr [B][3][3]
 *                       (graph_shape.py:89-113: f = 1.3875 * W * 4^tanh(p0), ...)
 *   zs_unproj_depth   : depth [B][H][W], intr [B][3][3] -> points [B][H*W][3] =
 *                       K^-1 [x,y,1]^T * depth (utils/camera.py:88-108)
 *   zs_valid_norm_fac : points [B][n][3], mask [B][n] bytes (torch.bool) -> mean [B][3] of
 *                       the selected points and max_dist [B] = max |p - mean|
 *                       (utils/camera.py:52-78).  An empty selection gives NaN (the
 *                       reference raises there).
 *   zs_masked_resample: interpolate_coordmap / interpolate_depth (utils/util.py:323-345):
 *                       map [B][C][H][W], mask [B][1][H][W] (valid where > 0.5) ->
 *                       out [B][C][Ho][Wo] = bilinear(map*mask)/(bilinear(mask)+1e-6) where
 *                       bilinear(mask) > 0.5 else `bg`; mask_out [B][1][Ho][Wo] in {0,1}.
 *                       Bilinear = torch interpolate(mode='bilinear', align_corners=False).
 *   zs_seen_surface   : the whole chain in one launch: unproject, masked mean / max radius
 *                       (-> mean [B][3], scale [B]), seen_points [B][H*W][3] =
 *                       (p - mean) / scale with invalid pixels zeroed, and, when coord_dsp
 *                       is not NULL, coord_dsp [B][3][Ho][Wo] + mask_dsp [B][1][Ho][Wo] =
 *                       interpolate_coordmap of the channel-major seen map.
 * ------------------------------------------------------------------------- */
int zs_intr_param2mtx(const float *params, int batch, int H, int W, float *intr, void *stream);
int zs_unproj_depth(const float *depth, const float *intr, int batch, int H, int W, float *points,
                    void *stream);
int zs_valid_norm_fac(const float *points, const uint8_t *mask, int batch, int n, float *mean,
                      float *max_dist, void *stream);
int zs_masked_resample(const float *map, const float *mask, int batch, int channels, int H, int W,
                       int Ho, int Wo, float bg, float *out, float *mask_out, void *stream);
int zs_seen_surface(const float *depth, const float *intr, const float *mask, int batch, int H, int W,
                    int Ho, int Wo, float *seen_points, float *mean, float *scale, float *coord_dsp,
                    float *mask_dsp, void *stream);
/* The same chain cut into 64 pixel chunks per image (three launches: chunk sums -> mean + chunk max radius -> scale +
 * normalise / resample): 80 -> ~12 us at batch 1, where one workgroup per image is a chain of dependent passes through one
 * CU.  The chunk sums are added in chunk order (reproducible; a different association than the one-workgroup form, ~1e-7
 * relative).  workspace: zs_seen_surface_workspace_bytes(batch) bytes; NULL = zs_seen_surface. */
size_t zs_seen_surface_workspace_bytes(int batch);
int zs_seen_surface_ws(const float *depth, const float *intr, const float *mask, int batch, int H, int W,
                       int Ho, int Wo, float *seen_points, float *mean, float *scale, float *coord_dsp,
                       float *mask_dsp, void *workspace, void *stream);

/* ------------------------------------------------------------------------- *
 * Depth metrics with least-squares scale/shift alignment in disparity space
 * (DepthMetric.compute_metrics, utils/eval_depth.py:46-116).  prediction, target,
 * mask: [B][n] fp32 (valid where mask > 0.5); thresholds: [host] n_thresholds <= 8
 * floats; depth_cap <= 0 means "no cap".  metrics [B][n_thresholds + 3] =
 * (d>thr_0 .. d>thr_k, rmse, l1_err, abs_rel); prediction_depth [B][n] (may be NULL) =
 * the aligned depth of every pixel; scale_shift [B][2] (may be NULL).
 * flags: ZS_DEPTH_PRED_IS_DISPARITY = prediction_type 'disparity' (:67-68);
 * ZS_DEPTH_SOLVE_ONLY = compute_scale_and_shift alone (:11-34): prediction and target are
 * used as given and only scale_shift is written.
 * ------------------------------------------------------------------------- */
#define ZS_DEPTH_PRED_IS_DISPARITY 1
#define ZS_DEPTH_SOLVE_ONLY 2
int zs_depth_metrics(const float *prediction, const float *target, const float *mask, int batch, int n,
                     int flags, float depth_cap, const float *thresholds,
                     int n_thresholds, float *metrics, float *prediction_depth, float *scale_shift,
                     void *stream);

/* ------------------------------------------------------------------------- *
 * Encoder layers (inference).  Activations are fp32 channels-last: [B][H][W][C]; a token
 * matrix [n][C] is the B=1, H=1, W=n case.
 *
 * zs_conv2d_nhwc: convolution / linear layer as an implicit GEMM on the fp32 MFMA pipe.
 *   packed_w: zs_conv2d_packed_floats(Cin,Cout,kh,kw) floats laid out [K16/4][CoutPad][4],
 *             value W[cout][tap][cin] at k = tap*Cin + cin (tap = ky*kw + kx), K16 = K rounded
 *             up to 16, CoutPad = Cout rounded up to 128, zero padded.  Cin % 4 == 0.
 *   out[p][c] = act( (sum_k A[p][k] W[k][c]) * scale[c] + shift[c] + res1[p][c] + res2[p][c] )
 *   A = input taps at (oy*stride - pad_t + ky, ox*stride - pad_l + kx); out-of-range taps are 0;
 *   in-range taps are first ReLU'd (flags & ZS_CONV_IN_RELU) and mapped a*in_scale + in_shift.
 *   scale / shift / res1 / res2 may be NULL (1 / 0 / none).  Explicit top/left padding with
 *   bounds-checked bottom/right covers torch's symmetric padding and timm's 'same' padding.
 *   Two tilings, chosen by problem size: 128x128 (LDS double-buffered) when that yields >= 192
 *   workgroups, else 32x64 with K split over the four waves and a fixed-order LDS reduction.
 * zs_group_norm_nhwc: y = GN_groups(x) * gamma + beta (+ residual) (ReLU if relu), per sample.
 * zs_layer_norm: rows of length C.
 * zs_attention: qkv [B][L][3*heads*head_dim] (q | k | v, head-major inside each) ->
 *   out [B][L][heads*head_dim] = softmax(q k^T / sqrt(head_dim)) v.  head_dim 32 or 64.
 * zs_max_pool_nhwc: k x k window, -inf padding.   zs_global_mean_nhwc: [B][HW][C] -> [B][C].
 * zs_upsample2x_nhwc: bilinear, align_corners=True, [B][H][W][C] -> [B][2H][2W][C].
 * zs_nchw_to_nhwc / zs_nhwc_to_nchw: boundary layout conversion (Cpad >= C zero-fills; mask [B][HW],
 *   may be NULL, multiplies every channel of a pixel: CoordEncRes' coord*mask, seen_coord_enc.py:184).
 * zs_assemble_tokens: tokens [B][n+1][C] = [cls | feat [B][n][C]] + pos [n+1][C].
 * zs_readout_concat: out [B][n][2C] = [tokens[b][1+i] | tokens[b][0]]  (vit.py:31-43).
 * zs_window_tokens: CoordEmb's token preparation (seen_coord_enc.py:50-71): emb [B][H][W][C],
 *   mask [B][H][W] bytes (invalid pixels take invalid_token [C]), cls [C], pos [win*win+1][C] ->
 *   out [B*(H/win)*(W/win)][win*win+1][C].
 * ------------------------------------------------------------------------- */
#define ZS_ACT_NONE 0
#define ZS_ACT_RELU 1
#define ZS_ACT_GELU 2
#define ZS_ACT_RELU_CLAMP1 3
#define ZS_ACT_SOFTPLUS 4 /* torch Softplus(beta, threshold=20); zs_act_forward / zs_act_backward only */
#define ZS_CONV_IN_RELU 1
#define ZS_CONV_FORCE_LARGE 2 /* tiling override (tests / tuning): 128x128 tiles */
#define ZS_CONV_FORCE_SMALL 4 /* 32x64 tiles with the K range split over the 4 waves */
#define ZS_CONV_F16X3 16      /* split-fp16 arithmetic on the 16-bit matrix pipe (csrc/zs_split16.h): operands
                               carried as two fp16 halves (~2^-21 relative for 2e-4 <~ |x| <= 65504), three
                               K = 16 MFMAs per eight fp32 ones; inference */
#define ZS_CONV_SPLIT_SMALL 32 /* with a workspace: small-tile layers that would leave most CUs idle split K across
                               * workgroups (partial sums in the workspace, fixed-order reduction kernel) */
/* Bits 64 and 256 are RETIRED (they selected the stream-K kernels, removed in ABI 42: DESIGN.md section 9.1).  Do not reuse
 * them: zs_conv2d_nhwc, zs_conv2d_nhwc_ws and zs_conv2d_nhwc_fused refuse a call that sets either (return 0, zs_last_error). */
#define ZS_CONV_RETIRED_64 64
#define ZS_CONV_RETIRED_256 256
#define ZS_CONV_W_PRESPLIT 128 /* with ZS_CONV_F16X3: packed_w is the output of zs_conv2d_presplit_weight (the weights'
                               * fp16 halves, same size and indexing as the fp32 packing) - no operand split of the
                               * weights at run time */
#define ZS_CONV_IN_DILATE2 8  /* read the input as if zero-stuffed x2 ([B][2H-1][2W-1][Cin] virtual): the
                                 data gradient of a stride-2 convolution as a stride-1 convolution */
#define ZS_CONV_FORCE_TILE256 1024 /* tests / tuning: the 256 x 256 ping-pong kernel (csrc/nn_conv_pp256.h) for every layer it can
                                    * run - pointwise, ZS_CONV_F16X3 | ZS_CONV_W_PRESPLIT, Cin % 32 == 0, Cout % 4 == 0 - whatever
                                    * its size (by default: K >= 768 and at least half a round of tiles, or K >= 2048) */
#define ZS_CONV_OUT_K16 2048  /* pointwise split-fp16 layers of few rows only (the streaming GEMM kernel, csrc/nn_gemm_stream.hip): `out`
                              * is written K16-MAJOR, [Cout / 16][M][16] floats instead of [M][Cout] (Cout % 16 == 0, no residuals, no
                              * statistics) ... */
#define ZS_CONV_IN_K16 4096   /* ... and `in` is read that way ([Cin / 16][M][16]): the 32 rows of a K = 16 step are 2 KiB of consecutive
                              * bytes for the consumer (the ViT MLP's hidden tensor at batch 1: fc2 20 -> 14 us).  A layer the kernel
                              * does not take is refused (returns 0): ask zs_conv2d_k16_ok first. */
#define ZS_CONV_IN_UPSAMPLE2 512 /* zs_conv3x3_tail_nhwc only: `in` is [B][H/2][W/2][Cin] and the layer runs on its x2 bilinear
                                    up-sampling (align_corners, zs_upsample2x_nhwc's formula), which is never written */
size_t zs_conv2d_packed_floats(int Cin, int Cout, int kh, int kw);
/* packed_w (zs_pack_conv_weight / nn/pack.py layout, zs_conv2d_packed_floats() floats) -> split_w, same size: the
 * split-fp16 halves of every weight in the order the ZS_CONV_F16X3 kernels consume them (ZS_CONV_W_PRESPLIT). */
int zs_conv2d_presplit_weight(const float *packed_w, float *split_w, int Cin, int Cout, int kh, int kw, void *stream);
/* The same for n operands in ONE launch (what optim.amp does after every optimiser step, right behind
 * zs_pack_conv_weight_multi): device arrays packed[n], split[n], cout_pad[n] (the operands' padded column counts) and
 * pair_prefix[n + 1] = running sum of pairs_i = K16_i / 16 * 2 * cout_pad_i (pair_prefix[n] == total_pairs). */
int zs_conv2d_presplit_weight_multi(const void *const *packed, void *const *split, const int *cout_pad,
                                    const unsigned long long *pair_prefix, int n, unsigned long long total_pairs,
                                    void *stream);
int zs_conv2d_nhwc(const float *in, const float *packed_w, const float *scale, const float *shift,
                   const float *res1, const float *res2, float *out, int batch, int Hin, int Win, int Cin,
                   int Hout, int Wout, int Cout, int kh, int kw, int stride, int pad_t, int pad_l, int flags,
                   float in_scale, float in_shift, int act, void *stream);
/* As zs_conv2d_nhwc, with a workspace of zs_conv2d_splitk_workspace_bytes() bytes (16-byte aligned, ZEROED ONCE by
 * the caller when allocated - its first 1 MiB are the streaming kernel's tickets, which the kernels leave at zero - and
 * used by one stream at a time; NULL = zs_conv2d_nhwc).  It holds the partial results of a contraction split across
 * workgroups, which a second kernel (or the last workgroup of a tile) sums in range order before the fused epilogue.  One
 * flag asks for such a split: ZS_CONV_SPLIT_SMALL (problems that would launch fewer than 256 small-tile workgroups - 14x14
 * feature maps, 197-token matrices at small batch).  Independently of it a workspace lets these paths split by the layer's
 * shape: small-tile layers with K >= 2048 on <= 64 workgroups; and, with ZS_CONV_F16X3 | ZS_CONV_W_PRESPLIT, 3x3 stride-1
 * layers of 32..191 input-patch workgroups (nn_conv_patch.h), layers of 40..191 tiles with >= 96 k-steps on the LDS-DMA
 * kernel, the last partial round of the 256 x 256 tiles (nn_conv_pp256.h) and pointwise layers of few rows (the streaming
 * kernel).  With a workspace the large-tile kernels also start at 96 instead of 192 tiles.  All of it is deterministic. */
size_t zs_conv2d_splitk_workspace_bytes(void);
int zs_conv2d_nhwc_ws(const float *in, const float *packed_w, const float *scale, const float *shift,
                   const float *res1, const float *res2, float *out, int batch, int Hin, int Win, int Cin,
                   int Hout, int Wout, int Cout, int kh, int kw, int stride, int pad_t, int pad_l, int flags,
                   float in_scale, float in_shift, int act, void *workspace, void *stream);

/* Fused normalisations around a small-tile launch of zs_conv2d_nhwc (batch-1 encoder: one launch per convolution instead
 * of convolution + GroupNorm / LayerNorm; reference: timm ResNetV2's GroupNormAct behind every StdConv2dSame, restated in
 * oracle/standins.py, and timm Block's norm1 / norm2, /root/reference/model/depth/vit.py:118-154).
 *   out_mode 1: besides `out`, the launch writes out_stats [ceil(M / 32)][out_groups][2] = (sum, sum of squares) of the
 *               stored values per 32-row tile and group of Cout / out_groups channels.
 *   out_mode 2: out_stats [M][ceil(Cout / tile columns)][2] = (sum, M2 about the tile-row mean) per row and column tile
 *               (zs_conv2d_fused_cols() columns per tile for this problem).
 *   in_mode 1:  A = relu(GroupNorm_{in_groups}(in) * in_gamma + in_beta), statistics from in_stats [in_tiles][in_groups][2]
 *               (a producer's out_mode 1 over the same tensor); zero padding stays zero.
 *   in_mode 2:  A = (in - mean_row) * rstd_row from in_stats [M][in_tiles <= 32][2] (a producer's out_mode 2); gamma / beta are
 *               expected inside packed_w / shift (W' = gamma * W, shift' = shift + beta W).  Pointwise layers only.
 * Statistics tiles must not straddle samples (batch 1, or Hin * Win a multiple of 32).  Requires ZS_CONV_F16X3 |
 * ZS_CONV_W_PRESPLIT, Cin % 8 == 0, Cin = 32 * 2^k <= 1024 for in_mode 1, Cout % 4 == 0; forces the small-tile kernel. */
typedef struct zs_conv_fuse {
    int in_mode, in_tiles, in_groups;
    int in_gshift;            /* set by the library (log2 of the channels per group) */
    const float *in_stats, *in_gamma, *in_beta;
    float in_eps;
    int out_mode, out_groups;
    float *out_stats;
} zs_conv_fuse;
int zs_conv2d_nhwc_fused(const float *in, const float *packed_w, const float *scale, const float *shift,
                         const float *res1, const float *res2, float *out, int batch, int Hin, int Win,
                         int Cin, int Hout, int Wout, int Cout, int kh, int kw, int stride, int pad_t,
                         int pad_l, int flags, float in_scale, float in_shift, int act, const zs_conv_fuse *fuse,
                         void *workspace, void *stream);
/* columns per tile (32 or 64) the fused small-tile launch uses for a problem of M rows and Cout columns: the consumer of
 * out_mode 2 statistics needs ceil(Cout / this) as its in_tiles */
int zs_conv2d_fused_cols(int M, int Cout);
/* 1 when a pointwise layer of M rows, Cin -> Cout, with `flags` (ZS_CONV_IN_K16 and / or ZS_CONV_OUT_K16) would be accepted:
 * ln_in_tiles > 0 = fuse.in_mode 2 with that many statistics tiles, row_stats_out = fuse.out_mode 2, has_res = a residual. */
int zs_conv2d_k16_ok(int M, int Cin, int Cout, int flags, int ln_in_tiles, int row_stats_out, int has_res);
/* y = [relu]( GroupNorm_32(x) * gamma + beta + r ) in ONE pass over x, from the (sum, sum of squares) tiles a fused launch wrote
 * (out_mode 1; `tiles` per sample).  r = residual [B][HW][C] (may be NULL), or GroupNorm_32(residual) * res_gamma + res_beta when
 * res_stats is given (the projection shortcut of a bottleneck's first block). */
/* y = max_pool_{k, stride, -inf padding}( relu(GroupNorm_32(x) * gamma + beta) ) from a fused launch's group statistics (timm
 * ResNetV2 stem: StdConv -> GroupNormAct -> MaxPool2dSame): one small launch turns the tile sums into `table` [B][C][2]
 * (scale, shift; caller-provided scratch), the pooling launch applies them on load - the normalised map is never written. */
int zs_gn_relu_max_pool_nhwc(const float *x, const float *stats, int tiles, const float *gamma, const float *beta,
                             float *table, float *y, int batch, int Hin, int Win, int C, int Hout, int Wout, int k,
                             int stride, int pad_t, int pad_l, float eps, void *stream);
int zs_group_norm_apply_stats(const float *x, const float *stats, int tiles, const float *gamma, const float *beta,
                              const float *residual, const float *res_stats, int res_tiles, const float *res_gamma,
                              const float *res_beta, float *y, int batch, int HW, int C, float eps, int relu, void *stream);
/* A 3x3 stride-1 pad-1 layer of at most 32 output channels with a fused pointwise TAIL to ONE channel - DPT's depth head,
 * model/depth/dpt_depth.py (reference: DPT output_conv[2..5]: Conv 128 -> 32 3x3, ReLU, Conv 32 -> 1, ReLU):
 *   out[b][y][x] = tail_act( tail_b[0] + sum_c tail_w[c] * act( conv3x3(in)[b][y][x][c] * scale[c] + shift[c] ) )
 * in [B][H][W][Cin] (Cin % 16 == 0), out [B][H][W] floats; packed_w = zs_conv2d_presplit_weight output of the 3x3 layer
 * (split-fp16 arithmetic only: flags must hold ZS_CONV_F16X3 | ZS_CONV_W_PRESPLIT; ZS_CONV_IN_RELU and ZS_CONV_IN_UPSAMPLE2 - H, W
 * even, the OUTPUT size - optional); tail_w [Cout],
 * tail_b [1] (NULL = 0).  The 32-channel intermediate ([B][H][W][32], 180 MB at 224^2 x 28) is never written.  Returns 0 with
 * zs_last_error set for geometries it does not take (the caller then issues the two layers separately). */
int zs_conv3x3_tail_nhwc(const float *in, const float *packed_w, const float *scale, const float *shift, float *out,
                         int batch, int H, int W, int Cin, int Cout, int flags, int act, const float *tail_w,
                         const float *tail_b, int tail_act, void *stream);
int zs_group_norm_nhwc(const float *x, const float *gamma, const float *beta, const float *residual, float *y,
                       int batch, int HW, int C, int groups, float eps, int relu, void *stream);
/* The same with a workspace (zs_group_norm_workspace_bytes; NULL = zs_group_norm_nhwc): tensors of >= 8 MiB take two
 * coalesced launches - per (sample, pixel chunk) group sums, then the normalisation - instead of one workgroup per
 * (sample, group) slice (whose loads use a quarter of every cache line in NHWC).  Deterministic (fixed-order sums). */
size_t zs_group_norm_workspace_bytes(int batch, int HW, int C, int groups);
int zs_group_norm_nhwc_ws(const float *x, const float *gamma, const float *beta, const float *residual, float *y,
                          int batch, int HW, int C, int groups, float eps, int relu, void *workspace, void *stream);
int zs_layer_norm(const float *x, const float *gamma, const float *beta, float *y, int rows, int C, float eps,
                  void *stream);
int zs_attention(const float *qkv, float *out, int batch, int L, int heads, int head_dim, void *stream);
/* zs_attention in split-fp16 arithmetic (three 16-bit MFMAs per product, ~2^-21 relative; csrc/zs_split16.h): the
 * inference encoders' default, like ZS_CONV_F16X3 for the convolutions. */
int zs_attention_split(const float *qkv, float *out, int batch, int L, int heads, int head_dim, void *stream);
int zs_max_pool_nhwc(const float *x, float *y, int batch, int Hin, int Win, int C, int Hout, int Wout, int k,
                     int stride, int pad_t, int pad_l, void *stream);
int zs_global_mean_nhwc(const float *x, float *y, int batch, int HW, int C, void *stream);
int zs_upsample2x_nhwc(const float *x, float *y, int batch, int Hin, int Win, int C, void *stream);
int zs_nchw_to_nhwc(const float *x, const float *mask, float *y, int batch, int C, int HW, int Cpad,
                    void *stream);
int zs_nhwc_to_nchw(const float *x, float *y, int batch, int C, int HW, void *stream);
int zs_assemble_tokens(const float *feat, const float *cls, const float *pos, float *tokens, int batch, int n,
                       int C, void *stream);
int zs_readout_concat(const float *tokens, float *out, int batch, int n, int C, void *stream);
int zs_window_tokens(const float *emb, const uint8_t *mask, const float *invalid_token, const float *cls,
                     const float *pos, float *out, int batch, int H, int W, int C, int win, void *stream);

/* ------------------------------------------------------------------------- *
 * Training (fp32; autograd over these entry points lives in zeroshape_amd/nn/autograd.py).
 * Replaces what the reference gets from torch.autograd + cuDNN/cuBLAS when train.py runs
 * Runner.train_iteration (model/shape_engine.py:248-297): Graph.forward(training=True)
 * (model/compute_graph/graph_shape.py:115-204), Loss.shape_loss (utils/loss.py:18-28),
 * loss.backward(), torch.optim.AdamW.step (model/shape_engine.py:132).
 * Every reduction runs in a fixed order (two-stage partial sums, no atomics).
 *
 * Convolution / linear layer gradients:
 *   zs_pack_conv_weight : torch-layout weight w[Cout][CinTot][kh][kw] (channel sub-range
 *       [cin0, cin0+Cin)) -> the packed operand of zs_conv2d_nhwc.  dgrad = 0: forward operand
 *       (Cin zero-padded to a multiple of 4; zs_conv2d_packed_floats(CinP, Cout, kh, kw) floats).
 *       dgrad = 1: operand of the DATA gradient, a convolution of dY (Cout zero-padded to a
 *       multiple of 4 = its input channels) with flipped taps and Cin outputs
 *       (zs_conv2d_packed_floats(CoutP, Cin, kh, kw) floats): dX = zs_conv2d_nhwc(dY, packed,
 *       stride 1, pad = k-1-pad, ZS_CONV_IN_DILATE2 when the forward stride was 2).
 *   zs_conv2d_wgrad : dw[cout][cin0+c][ky][kx] (=|+=) sum over output pixels of
 *       dy[pixel][cout] * A[pixel][(ky,kx,c)], A = the forward's input taps incl. its input
 *       transform (flags & ZS_CONV_IN_RELU, in_scale, in_shift).  in is [B][Hin][Win][CinP]
 *       (CinP % 4 == 0, channels >= Cin are padding), dy is [B][Hout][Wout][CoutP] with
 *       CoutP = Cout rounded up to 4.  db (may be NULL) receives the bias gradient [Cout] = the column
 *       sums of dy, gathered from the tiles the kernel stages anyway.
 *       workspace: zs_conv2d_wgrad_workspace_bytes(...).
 *   zs_standardize_weight(_bwd) : timm StdConv2d: rows of n = Cin*kh*kw weights,
 *       (w - mean) / sqrt(biased var + eps), and the adjoint for a gradient w.r.t. the result.
 * Pointwise / normalisation:
 *   zs_act_forward / zs_act_backward : GELU(erf), Softplus(beta), ReLU, ReLU+clamp1; backward
 *       takes `ref` = the pre-activation input (GELU, softplus) or the OUTPUT (ReLU variants).
 *   zs_add_scaled_rows : y[b][..] = x[b][..] + scale[b] * branch[b][..] (x may be NULL):
 *       residual with per-sample stochastic depth (timm DropPath, implicit.py:8,83-109).
 *   zs_column_sum : out[c] = scale * sum_rows x[row][c]   (bias gradients, reductions).
 *   zs_layer_norm_bwd : dx, dgamma, dbeta of zs_layer_norm (statistics recomputed from x).
 *   zs_attention_bwd : dqkv [B][L][3*heads*head_dim] of zs_attention; L <= 512.
 * Decoder (model/shape/implicit.py:25-79, ImplFuncAttention):
 *   zs_point_attention : out[b][i] = softmax over (Ll latent keys + the point itself) of
 *       q_i k^T / sqrt(d), times the values; qkv_points [B][M][3*heads*32], qkv_latent
 *       [B][Ll][3*heads*32] (q | k | v, head-major).  Ll <= 256, head_dim 32.
 *   zs_point_attention_bwd : dqkv_points (all of q, k, v), dqkv_latent: k and v columns
 *       written (accumulate_latent = 0, q columns zeroed) or added to (accumulate_latent = 1).
 * Loss / optimiser:
 *   zs_bce_logits(_bwd) : Loss.shape_loss: mean over n of w * BCEWithLogits(logit, sdf < 0),
 *       w = impt_weight where |sdf| < impt_thres else 1; backward scales by *grad_loss (device).
 *   zs_adamw_multi : torch.optim.AdamW (decoupled decay, bias correction, eps outside the
 *       sqrt) over a DEVICE table of tensors in one launch; chunk c = elements
 *       [chunk_start[c], +zs_multi_tensor_chunk_elems()) of tensor chunk_tensor[c].
 *       grad_scale (device scalar, may be NULL) multiplies every gradient (clipping, loss-scale removal);
 *       a grad_scale of 0 or nan skips the whole update (an overflowed gradient under loss scaling).
 *       `step` counts the calls; *skipped_steps (device int, may be NULL) the calls that were skipped that way:
 *       the bias corrections use step - *skipped_steps, as torch's GradScaler never steps on an overflow.
 *   zs_copy_multi  : entry.param[i] = entry.grad[i] * scale (gradient bucketing for all-reduce).
 *   zs_sumsq_multi : *sumsq = sum of entry.grad[i]^2 over the table (partial: n_chunks floats).
 * ------------------------------------------------------------------------- */
typedef struct zs_tensor_entry {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    unsigned long long n;
    float lr, weight_decay;
} zs_tensor_entry;

int zs_pack_conv_weight(const float *w, float *packed, int Cout, int Cin, int cin0, int CinTot, int kh, int kw,
                        int dgrad, void *stream);
/* zs_pack_conv_weight over a DEVICE table of layers in one launch (every operand of a model after
 * an optimiser step): ld = CinTot*kh*kw, taps = kh*kw, K16 / NPad = the padded operand dimensions
 * (K rounded up to 16, N rounded up to 128); chunk c = the chunk_start[c]-th of the
 * zs_pack_entry_chunks(...) chunks of entry chunk_entry[c] (an LDS tile of 64 operand columns x 16 or 64
 * channels x all taps for kernels up to 3x3, zs_pack_chunk_elems() consecutive elements otherwise), every chunk
 * of an entry exactly once.  The operand must have been packed once by zs_pack_conv_weight (its K padding rows
 * are not rewritten). */
typedef struct zs_pack_entry {
    const float *src;
    float *dst;
    int Cout, Cin, cin0, ld, taps, dgrad, K16, NPad;
} zs_pack_entry;
int zs_pack_chunk_elems(void);
int zs_pack_entry_chunks(int Cout, int Cin, int taps, int dgrad, int K16, int NPad);
int zs_pack_conv_weight_multi(const zs_pack_entry *table, const int *chunk_entry, const unsigned long long *chunk_start,
                              int n_chunks, void *stream);
/* The same launch also writing the fp16 halves of the operands (the layout of zs_conv2d_presplit_weight) from the tiles it
 * holds: split_dst[e] = the split buffer of entry e (K16 * NPad floats) or NULL; non-NULL only for entries for which
 * zs_pack_entry_inline_split(Cout, Cin, taps, dgrad) returns 1 (kernels up to 3x3 whose K-side channel count, rounded up
 * to 4, is a multiple of 16).  split_only != 0: the fp32 operand (entry.dst) of those entries is NOT rewritten - for
 * callers whose every consumer reads the halves (optim.amp: one pass over the weights instead of re-pack + split). */
int zs_pack_entry_inline_split(int Cout, int Cin, int taps, int dgrad);
int zs_pack_conv_weight_multi_split(const zs_pack_entry *table, const int *chunk_entry,
                                    const unsigned long long *chunk_start, int n_chunks, float *const *split_dst,
                                    int split_only, void *stream);
size_t zs_conv2d_wgrad_workspace_bytes(int batch, int Hout, int Wout, int Cin, int Cout, int kh, int kw);
int zs_conv2d_wgrad(const float *in, const float *dy, float *dw, float *db, void *workspace, int batch, int Hin, int Win,
                    int CinP, int Hout, int Wout, int Cout, int kh, int kw, int stride, int pad_t, int pad_l,
                    int flags, float in_scale, float in_shift, int Cin, int cin0, int CinTot, int accumulate,
                    void *stream);
/* Data gradient of a convolution with Cin <= 4 input channels (the network stems: as a GEMM it would
 * fill 3 of 128 tile columns), direct gather form: dx [B][H][W][CinP] (padding channels zeroed) =
 * scale * sum over the output pixels that read the input pixel of dy [B][Hout][Wout][Cout] . w
 * (torch layout, channel sub-range [cin0, cin0+Cin) of CinTot).  Cout % 4 == 0. */
int zs_conv2d_dgrad_small_cin(const float *dy, const float *w, float *dx, int batch, int H, int W, int CinP, int Hout,
                              int Wout, int Cout, int kh, int kw, int stride, int pad_t, int pad_l, int Cin, int cin0,
                              int CinTot, float scale, void *stream);
int zs_standardize_weight(const float *w, float *out, int Cout, int n, float eps, void *stream);
/* zs_standardize_weight over a device table of weights in one launch: entry e = rows x n weights (rows = Cout, n = the
 * fan-in) from w to out with its eps; row_prefix[e] = the number of rows of the entries before e (n_entries ints,
 * row_prefix[0] = 0), total_rows = their sum.  Same arithmetic as the single call. */
typedef struct zs_std_entry {
    const float *w;
    float *out;
    int rows, n;
    float eps;
    int pad;
} zs_std_entry;
int zs_standardize_weight_multi(const zs_std_entry *table, const int *row_prefix, int n_entries, int total_rows, void *stream);
int zs_standardize_weight_bwd(const float *w, const float *grad_out, float *dw, int Cout, int n, float eps,
                              void *stream);
int zs_act_forward(const float *x, float *y, size_t n, int act, float beta, void *stream);
int zs_act_backward(const float *dy, const float *ref, float *dx, size_t n, int act, float beta, void *stream);
/* NeRF positional encoding of 3D points - the reference's get_embedder(L, 3) (utils/layers.py:8-53; used by MLPBlocks when
 * posenc_3D = L > 0, model/shape/implicit.py:139-166): out[i][0:3+6L] = [x | sin(x 2^0) | cos(x 2^0) | ... | sin(x 2^(L-1)) |
 * cos(x 2^(L-1))], each group 3 wide (x, y, z), zero padded to `stride` floats per point (stride >= 3 + 6 L). */
int zs_posenc3d(const float *points, size_t n, int L, float *out, int stride, void *stream);
/* Its adjoint: dpoints[i][0:3] from the cotangent denc[i][0:stride] of the encoding, per axis
 * dx = denc[x] + sum_k 2^k (cos(2^k x) denc[sin_k] - sin(2^k x) denc[cos_k]), with 2^k x rounded to fp32 as the forward rounds it
 * and the forward's channel order.  Channels from 3 + 6 L on (the padding) are never read. */
int zs_posenc3d_bwd(const float *points, size_t n, int L, const float *denc, int stride, float *dpoints, void *stream);
int zs_add_scaled_rows(const float *x, const float *branch, const float *scale, float *y, int batch,
                       size_t per_sample, void *stream);
size_t zs_column_sum_workspace_bytes(int rows, int C);
int zs_column_sum(const float *x, float *out, int rows, int C, float scale, void *workspace, void *stream);
size_t zs_layer_norm_bwd_workspace_bytes(int rows, int C);
int zs_layer_norm_bwd(const float *dy, const float *x, const float *gamma, float *dx, float *dgamma, float *dbeta,
                      int rows, int C, float eps, void *workspace, void *stream);
/* The same with dx = (LayerNorm's input gradient) + add [rows][C] (may be NULL): the gradient arriving at x from its other
 * consumer (a residual connection), summed in the same pass instead of by a separate elementwise launch. */
int zs_layer_norm_bwd_add(const float *dy, const float *x, const float *gamma, const float *add, float *dx, float *dgamma,
                          float *dbeta, int rows, int C, float eps, void *workspace, void *stream);
size_t zs_attention_bwd_workspace_bytes(int batch, int L, int heads);
int zs_attention_bwd(const float *qkv, const float *dout, float *dqkv, void *workspace, int batch, int L, int heads,
                     int head_dim, void *stream);
int zs_point_attention(const float *qkv_points, const float *qkv_latent, float *out, int batch, int M, int Ll,
                       int heads, int head_dim, void *stream);
/* The attention map a decoder call returns (implicit.py:60-66,277): attn[b][i][j] (=|+=, `accumulate`) weight * mean over the
 * heads of the softmax probability of point i for latent token j (softmax over the Ll latent keys AND the point itself; the
 * point's own column is dropped afterwards).  One call per attention block with weight = 1 / n_blocks gives the reference's
 * average over blocks.  Same size limits as zs_point_attention. */
int zs_point_attention_probs(const float *qkv_points, const float *qkv_latent, float *attn, int batch, int M, int Ll,
                             int heads, int head_dim, float weight, int accumulate, void *stream);
size_t zs_point_attention_bwd_workspace_bytes(int batch, int M, int Ll, int heads);
int zs_point_attention_bwd(const float *qkv_points, const float *qkv_latent, const float *dout, float *dqkv_points,
                           float *dqkv_latent, int accumulate_latent, void *workspace, int batch, int M, int Ll,
                           int heads, int head_dim, void *stream);
size_t zs_bce_logits_workspace_bytes(size_t n);
int zs_bce_logits(const float *logits, const float *sdf, size_t n, float impt_thres, float impt_weight, float *loss,
                  void *workspace, void *stream);
int zs_bce_logits_bwd(const float *logits, const float *sdf, size_t n, float impt_thres, float impt_weight,
                      const float *grad_loss, float *dlogits, void *stream);
/* The depth task's losses (options/depth.yaml).
 *   zs_midas_loss : MidasLoss.forward (model/depth/midas_loss.py:166-185, shrink_mask False) on
 *       prediction / target / mask [B][1][H][W] (valid where mask > 0.5): scale-and-shift-invariant MAE
 *       (median / mean-absolute-deviation alignment per image) + alpha * gradient matching over
 *       `scales` <= 4 power-of-two strides of the least-squares aligned maps (inverse_depth != 0:
 *       1 / (d + 1e-6) first), image-based reduction.  *loss is a device scalar; workspace
 *       (zs_midas_loss_workspace_bytes(B)) keeps the per-image statistics for the backward.
 *   zs_midas_loss_bwd : d loss / d prediction [B][1][H][W], scaled by *grad_loss (device), through
 *       the median element, the deviations and the 2x2 least-squares solve, like torch.autograd.
 *   zs_intr_loss(_bwd) : Loss.intr_loss (utils/loss.py:36-43): seen_* [n][3], mask [n] over the
 *       whole batch; out2 = (loss, sum of the mask) on the device. */
/* MidasLoss.erode_mask (model/depth/midas_loss.py:153-162; training.depth_loss.mask_shrink):
 * out[b][y][x] = 1 iff every value of the pool x pool block of mask[b] that holds (y, x) equals 1
 * (max_pool2d with stride = kernel, then F.interpolate(mode='nearest') back), else 0.  [B][H][W] fp32. */
int zs_erode_mask(const float *mask, int batch, int H, int W, int pool, float *out, void *stream);
size_t zs_midas_loss_workspace_bytes(int batch);
int zs_midas_loss(const float *prediction, const float *target, const float *mask, int batch, int H, int W, float alpha,
                  int scales, int inverse_depth, float *loss, void *workspace, void *stream);
int zs_midas_loss_bwd(const float *prediction, const float *target, const float *mask, int batch, int H, int W,
                      float alpha, int scales, int inverse_depth, const void *workspace, const float *grad_loss,
                      float *dprediction, void *stream);
int zs_intr_loss(const float *seen_pred, const float *seen_gt, const float *mask, size_t n, float *out2, void *stream);
int zs_intr_loss_bwd(const float *seen_pred, const float *seen_gt, const float *mask, size_t n, const float *out2,
                     const float *grad_loss, float *dseen_pred, void *stream);
int zs_multi_tensor_chunk_elems(void);
int zs_adamw_multi(const zs_tensor_entry *table, const int *chunk_tensor, const unsigned long long *chunk_start,
                   int n_chunks, float beta1, float beta2, float eps, int step, const float *grad_scale,
                   const int *skipped_steps, void *stream);
int zs_copy_multi(const zs_tensor_entry *table, const int *chunk_tensor, const unsigned long long *chunk_start,
                  int n_chunks, float scale, void *stream);
int zs_sumsq_multi(const zs_tensor_entry *table, const int *chunk_tensor, const unsigned long long *chunk_start,
                   int n_chunks, float *partial, float *sumsq, void *stream);

/* Encoder training (BatchNorm / GroupNorm / pooling / resampling / geometry backward).
 *   zs_batch_norm_train : nn.BatchNorm2d in training mode over [rows][C] (rows = B*H*W): batch
 *       mean / biased variance -> y = (x-mean)*rstd*gamma+beta (+residual) (ReLU if relu);
 *       running_mean / running_var (may both be NULL) updated with `momentum` and the unbiased
 *       variance like torch; save_mean / save_rstd [C] feed the backward.
 *   zs_batch_norm_bwd   : y_relu = the forward output when ReLU was fused (masks dy), else NULL;
 *       dresidual (may be NULL) = the masked dy.
 *   zs_group_norm_bwd   : backward of zs_group_norm_nhwc (statistics recomputed from x).
 *   zs_max_pool_bwd_nhwc / zs_global_mean_bwd_nhwc / zs_upsample2x_bwd_nhwc: adjoints of the
 *       forward layers in gather form (no atomics); max-pool routes to the first maximum of a
 *       window in row-major order, as torch does.
 *   zs_nhwc_to_nchw_masked : y[b][c][p] = x[b][p][c] * mask[b][p], c < C <= Cpad.
 *   zs_seen_surface_bwd : backward of zs_seen_surface for Ho = H, Wo = W (the ResNet coordinate
 *       encoder): d_seen_points [B][HW][3] and/or d_coord_dsp [B][3][H][W] (either may be NULL)
 *       -> d_depth [B][HW], d_intr [B][3][3], through the masked mean and the max-radius scale
 *       (utils/camera.py:52-108 as torch.autograd differentiates them).
 *   zs_intr_param2mtx_bwd : d_intr -> d_params [B][3] (graph_shape.py:89-113). */
size_t zs_batch_norm_workspace_bytes(int rows, int C);
int zs_batch_norm_train(const float *x, const float *gamma, const float *beta, const float *residual, float *y,
                        float *running_mean, float *running_var, float *save_mean, float *save_rstd, int rows, int C,
                        float eps, float momentum, int relu, void *workspace, void *stream);
int zs_batch_norm_bwd(const float *x, const float *dy, const float *y_relu, const float *gamma, const float *save_mean,
                      const float *save_rstd, float *dx, float *dresidual, float *dgamma, float *dbeta, int rows, int C,
                      void *workspace, void *stream);
size_t zs_group_norm_bwd_workspace_bytes(int batch, int C);
int zs_group_norm_bwd(const float *x, const float *dy, const float *y_relu, const float *gamma, float *dx,
                      float *dresidual, float *dgamma, float *dbeta, int batch, int HW, int C, int groups, float eps,
                      void *workspace, void *stream);
int zs_max_pool_bwd_nhwc(const float *x, const float *dy, float *dx, int batch, int Hin, int Win, int C, int Hout,
                         int Wout, int k, int stride, int pad_t, int pad_l, void *stream);
int zs_global_mean_bwd_nhwc(const float *dy, float *dx, int batch, int HW, int C, void *stream);
int zs_upsample2x_bwd_nhwc(const float *dy, float *dx, int batch, int Hin, int Win, int C, void *stream);
int zs_nhwc_to_nchw_masked(const float *x, const float *mask, float *y, int batch, int C, int HW, int Cpad,
                           void *stream);
int zs_seen_surface_bwd(const float *depth, const float *intr, const float *mask, const float *mean, const float *scale,
                        const float *d_seen_points, const float *d_coord_dsp, int batch, int H, int W, float *d_depth,
                        float *d_intr, void *stream);
int zs_intr_param2mtx_bwd(const float *params, const float *d_intr, int batch, int H, int W, float *d_params,
                          void *stream);
/* Training of the transformer coordinate encoder (CoordEmb / CoordEncAtt, seen_coord_enc.py:13-139):
 *   zs_window_tokens_bwd : adjoint of zs_window_tokens in gather form - d_out [B*nwy*nwx][win*win+1][C] ->
 *       d_emb [B][H][W][C] (valid pixels), d_inv_rows [B][H][W][C] (the rows that fed invalid_coord_token) and
 *       d_cls_rows [B*nwy*nwx][C]; their column sums (zs_column_sum) are the two token gradients.
 *   zs_coord_dsp2_bwd : adjoint of the 2x down-sampling of the seen-surface coordinate map (interpolate_coordmap,
 *       utils/util.py:336-345, dsp = 2) as the same-size gradient zs_seen_surface_bwd takes: d_dsp [B][3][H/2][W/2],
 *       mask [B][H][W], mask_dsp [B][H/2][W/2] -> d_full [B][3][H][W]. */
int zs_window_tokens_bwd(const float *d_out, const uint8_t *mask, float *d_emb, float *d_inv_rows, float *d_cls_rows,
                         int batch, int H, int W, int C, int win, void *stream);
int zs_coord_dsp2_bwd(const float *d_dsp, const float *mask, const float *mask_dsp, float *d_full, int batch, int H,
                      int W, void *stream);
/* Bilinear resize (align_corners=False) of a channels-last grid [Hi][Wi][C] -> [Ho][Wo][C]
 * (vit.py:103-120 _resize_pos_embed); backward != 0: x is the gradient of the [Ho][Wo][C] output
 * and y receives the gradient of the [Hi][Wi][C] input.  zs_readout_concat_bwd: adjoint of
 * zs_readout_concat (dout [B][n][2C] -> dtokens [B][n+1][C]). */
/* graph_shape.py:163-173: out[b][i] = ((R_b p + t_b) - mean_b) / scale_b with pose [B][3][4] = [R|t]:
 * the ground-truth query points in the normalised frame of the (GT) seen surface. */
int zs_transform_points(const float *points, const float *pose, const float *mean, const float *scale, float *out,
                        int batch, int n, void *stream);
int zs_resize_bilinear_nhwc(const float *x, float *y, int Hi, int Wi, int Ho, int Wo, int C, int backward,
                            void *stream);
int zs_readout_concat_bwd(const float *dout, float *dtokens, int batch, int n, int C, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ZEROSHAPE_HIP_H */
