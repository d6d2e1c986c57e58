// Vertex colours for a predicted mesh from the input photo (gfx950): project the welded mesh into the input camera, decide
// per vertex whether that camera saw it, look the photo up there, and give every vertex the camera did not see the colour of
// the nearest one it did.  The reference's meshes are bare geometry, so there is nothing to compare against: the contract
// is eval_3D.mesh_vertex_colors_host, a float64 numpy restatement that follows these kernels operation for operation
// (tests/test_gpu_mesh_colors.py demands equality, not closeness).
//
// The predicted shape lives in the normalised camera frame of the input view (model/compute_graph/graph_shape.py:131-144:
// seen = (K^-1 [x, y, 1]^T depth - mean) / scale), so a mesh vertex v sits at X = v scale + mean in the camera and projects
// through K.  Pixel (row i, col j) is at (u, w) = (j, i): integer coordinates are texel centres (unproj_depth's convention).
//
// zs_mesh_colors_seen, all on the stream:
//   project   : a thread per vertex.  X = v scale + mean, p = K X (all three rows), Z = p_z, u = p_x / p_z, w = p_y / p_z
//   z-buffer  : ss H x ss W words, a thread per face, the rules of render.hip's scatter: raster coordinates
//               x_r = (u + 0.5) ss, y_r = (w + 0.5) ss, pixel centres (j + 0.5, i + 0.5), coverage inclusive on every edge, a face
//               with a Z that is not > 0 or not finite, or with zero / NaN / overflowing area, skipped whole, depth
//               1 / (sum w_k / Z_k) rounded to fp32, ONE 64-bit atomicMax of (~bits(depth) << 32) | ~face per covered pixel - the
//               result does not depend on the order of execution
//   seen      : a thread per vertex.  Seen iff (1) Z > 0 and finite, 0 <= u <= W - 1, 0 <= w <= H - 1; (2) it faces the camera,
//               n . d > min_cos |n| |d| with d = -X (a zero or non-finite normal fails); (3) the four mask texels of its bilinear
//               footprint are > 0.5; (4) the z-buffer word at (floor(y_r), floor(x_r)) is 0, or names a face that holds this
//               vertex, or Z <= (double)depth + depth_tol scale.  Colour: bilinear in fp64, uint8(clamp(floor(255 c + 0.5)))
//   fraction  : area of the faces whose three vertices are seen, and the total area: per-block partials in a fixed order, one
//               block sums them in a fixed order - no float atomics
//   positions : the inclusive scan of the seen flags (zs_scan.h) and the seen count, the one value the host reads
// zs_mesh_colors_compact: order-preserving lists of the seen and the hidden vertices (index + position), for the library's
//               own nearest-neighbour search (zs_chamfer_forward_ws: xyz1 = hidden, xyz2 = seen)
// zs_mesh_colors_fill: hidden vertex <- colour of its nearest seen vertex, faded towards base with the distance:
//               t = fade > 0 ? min(sqrt(dist) / fade, 1) : 0, c = (1 - t) c_nn + t 255 base, floor(c + 0.5) clamped;
//               with no seen vertex at all every vertex gets 255 base and source -1
//
// The geometry is fp64 from the fp32 inputs and uses only + - * / sqrt floor and comparisons; built with -ffp-contract=off.
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int COL_THREADS = 256;
constexpr int COL_MAX = 1 << 29;               // vertices / faces of one launch
constexpr int COL_MAX_SIDE = 16384;            // ss * H, ss * W
constexpr int FRAC_MAX_BLOCKS = 256;           // partials the final block sums, one per thread

struct ColView {
    int H, W, ss, Hz, Wz;
};

__global__ __launch_bounds__(COL_THREADS) void col_project_kernel(const float *__restrict__ verts, int n_verts,
                                                                  const float *__restrict__ K, const float *__restrict__ mean,
                                                                  const float *__restrict__ scale, double *__restrict__ proj) {
    const long long vl = (long long)blockIdx.x * COL_THREADS + threadIdx.x;
    if (vl >= n_verts) return;
    const double s = (double)scale[0];
    double X[3], p[3];
    for (int a = 0; a < 3; ++a) X[a] = (double)verts[vl * 3 + a] * s + (double)mean[a];
    for (int r = 0; r < 3; ++r) p[r] = (double)K[r * 3 + 0] * X[0] + (double)K[r * 3 + 1] * X[1] + (double)K[r * 3 + 2] * X[2];
    proj[vl * 3 + 0] = p[0] / p[2];
    proj[vl * 3 + 1] = p[1] / p[2];
    proj[vl * 3 + 2] = p[2];
}

__global__ __launch_bounds__(COL_THREADS) void col_zbuffer_kernel(const int *__restrict__ faces, int n_tris, int n_verts,
                                                                  const double *__restrict__ proj, ColView vw,
                                                                  unsigned long long *__restrict__ zbuf) {
    const long long tl = (long long)blockIdx.x * COL_THREADS + threadIdx.x;
    if (tl >= n_tris) return;
    const int t = (int)tl;
    double z[3], x[3], y[3];
    for (int k = 0; k < 3; ++k) {
        const int v = faces[tl * 3 + k];
        if (v < 0 || v >= n_verts) return;                        // not a face of this mesh
        z[k] = proj[(size_t)v * 3 + 2];
        if (!(z[k] > 0.0) || !(z[k] <= 1.7e308)) return;          // at or behind the camera, infinite or NaN: skipped whole
        x[k] = (proj[(size_t)v * 3 + 0] + 0.5) * (double)vw.ss;
        y[k] = (proj[(size_t)v * 3 + 1] + 0.5) * (double)vw.ss;
    }
    const double area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]);
    if (!(fabs(area) > 0.0) || !(fabs(area) <= 1.0e300)) return;      // zero area, NaN or overflow
    const double xlo = fmin(fmin(x[0], x[1]), x[2]), xhi = fmax(fmax(x[0], x[1]), x[2]);
    const double ylo = fmin(fmin(y[0], y[1]), y[2]), yhi = fmax(fmax(y[0], y[1]), y[2]);
    const int j0 = (int)fmin(fmax(ceil(xlo - 0.5), 0.0), (double)vw.Wz), j1 = (int)fmax(fmin(floor(xhi - 0.5), (double)(vw.Wz - 1)), -1.0);
    const int i0 = (int)fmin(fmax(ceil(ylo - 0.5), 0.0), (double)vw.Hz), i1 = (int)fmax(fmin(floor(yhi - 0.5), (double)(vw.Hz - 1)), -1.0);
    const unsigned long long low = (unsigned long long)(~(unsigned)t);
    for (int i = i0; i <= i1; ++i) {
        const double py = (double)i + 0.5;
        for (int j = j0; j <= j1; ++j) {
            const double px = (double)j + 0.5;
            const double w0 = ((x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])) / area;
            const double w1 = ((x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])) / area;
            const double w2 = ((x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])) / area;
            if (!(w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0)) continue;
            const float d = (float)(1.0 / (w0 / z[0] + w1 / z[1] + w2 / z[2]));
            if (!(d > 0.0f) || !(d <= 3.0e38f)) continue;
            // positive floats order like their bit patterns: inverted, the maximum is the nearest
            const unsigned long long key = ((unsigned long long)(~__float_as_uint(d)) << 32) | low;
            atomicMax(zbuf + (size_t)i * vw.Wz + j, key);
        }
    }
}

// floor(x + 0.5) clamped to [0, 255]; NaN gives 0
__device__ __forceinline__ uint8_t col_round(double x) {
    const double r = floor(x + 0.5);
    if (!(r >= 0.0)) return 0;
    return (uint8_t)(r > 255.0 ? 255.0 : r);
}

__global__ __launch_bounds__(COL_THREADS) void col_seen_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                               const float *__restrict__ normals, int n_verts, int n_tris,
                                                               const double *__restrict__ proj, const float *__restrict__ image,
                                                               const float *__restrict__ mask, const float *__restrict__ mean,
                                                               const float *__restrict__ scale, ColView vw, double depth_tol,
                                                               double min_cos, const unsigned long long *__restrict__ zbuf,
                                                               uint8_t *__restrict__ colors, uint8_t *__restrict__ seen,
                                                               int *__restrict__ source, int *__restrict__ pos) {
    const long long vl = (long long)blockIdx.x * COL_THREADS + threadIdx.x;
    if (vl >= n_verts) return;
    const int v = (int)vl;
    const int H = vw.H, W = vw.W;
    const double u = proj[vl * 3 + 0], w = proj[vl * 3 + 1], Z = proj[vl * 3 + 2];
    const double s = (double)scale[0];
    bool ok = Z > 0.0 && Z <= 1.7e308 && u >= 0.0 && u <= (double)(W - 1) && w >= 0.0 && w <= (double)(H - 1);
    if (ok) {                                                     // faces the camera
        double n[3], d[3];
        for (int a = 0; a < 3; ++a) {
            n[a] = (double)normals[vl * 3 + a];
            d[a] = -((double)verts[vl * 3 + a] * s + (double)mean[a]);
        }
        const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), dd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double dot = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
        ok = nn > 0.0 && nn <= 1.7e308 && dot > min_cos * nn * dd;
    }
    uint8_t rgb[3] = {0, 0, 0};
    if (ok) {                                                     // the bilinear footprint lies on the object
        const int j0 = min((int)floor(u), max(W - 2, 0)), i0 = min((int)floor(w), max(H - 2, 0));
        const int j1 = min(j0 + 1, W - 1), i1 = min(i0 + 1, H - 1);
        ok = mask[(size_t)i0 * W + j0] > 0.5f && mask[(size_t)i0 * W + j1] > 0.5f && mask[(size_t)i1 * W + j0] > 0.5f &&
             mask[(size_t)i1 * W + j1] > 0.5f;
        if (ok) {
            const double fu = u - (double)j0, fv = w - (double)i0;
            for (int c = 0; c < 3; ++c) {
                const float *img = image + (size_t)c * H * W;
                const double t00 = (double)img[(size_t)i0 * W + j0], t01 = (double)img[(size_t)i0 * W + j1];
                const double t10 = (double)img[(size_t)i1 * W + j0], t11 = (double)img[(size_t)i1 * W + j1];
                const double val = (1.0 - fv) * ((1.0 - fu) * t00 + fu * t01) + fv * ((1.0 - fu) * t10 + fu * t11);
                rgb[c] = col_round(255.0 * val);
            }
        }
    }
    if (ok) {                                                     // not occluded
        const int jz = min((int)floor((u + 0.5) * (double)vw.ss), vw.Wz - 1), iz = min((int)floor((w + 0.5) * (double)vw.ss), vw.Hz - 1);
        const unsigned long long key = zbuf[(size_t)iz * vw.Wz + jz];
        if (key) {
            const int t = (int)~(unsigned)key;
            const float depth = __uint_as_float(~(unsigned)(key >> 32));
            bool own = false;
            if (t >= 0 && t < n_tris) own = faces[(size_t)t * 3] == v || faces[(size_t)t * 3 + 1] == v || faces[(size_t)t * 3 + 2] == v;
            ok = own || Z <= (double)depth + depth_tol * s;
        }
    }
    seen[vl] = ok ? 1 : 0;
    pos[vl] = ok ? 1 : 0;
    source[vl] = ok ? v : -1;
    for (int c = 0; c < 3; ++c) colors[vl * 3 + c] = ok ? rgb[c] : (uint8_t)0;
}

struct FracPartial {
    double seen, total;
};

__device__ __forceinline__ void frac_reduce(FracPartial &p, FracPartial *lds) {
    const int tid = threadIdx.x;
    lds[tid] = p;
    __syncthreads();
    for (int s = COL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            lds[tid].seen += lds[tid + s].seen;
            lds[tid].total += lds[tid + s].total;
        }
        __syncthreads();
    }
    p = lds[0];
}

inline int frac_blocks(int n) {
    const int b = (n + COL_THREADS - 1) / COL_THREADS;
    return b < FRAC_MAX_BLOCKS ? b : FRAC_MAX_BLOCKS;
}

__global__ __launch_bounds__(COL_THREADS) void col_fraction_partial_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                                           int n_tris, int n_verts, const uint8_t *__restrict__ seen,
                                                                           FracPartial *__restrict__ partials) {
    __shared__ FracPartial lds[COL_THREADS];
    FracPartial p = {0.0, 0.0};
    for (long long t = (long long)blockIdx.x * COL_THREADS + threadIdx.x; t < n_tris; t += (long long)gridDim.x * COL_THREADS) {
        const int a = faces[t * 3], b = faces[t * 3 + 1], c = faces[t * 3 + 2];
        if (a < 0 || a >= n_verts || b < 0 || b >= n_verts || c < 0 || c >= n_verts) continue;
        double e1[3], e2[3];
        for (int k = 0; k < 3; ++k) {
            e1[k] = (double)verts[(size_t)b * 3 + k] - (double)verts[(size_t)a * 3 + k];
            e2[k] = (double)verts[(size_t)c * 3 + k] - (double)verts[(size_t)a * 3 + k];
        }
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const double area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
        p.total += area;
        if (seen[a] && seen[b] && seen[c]) p.seen += area;
    }
    frac_reduce(p, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

__global__ __launch_bounds__(COL_THREADS) void col_fraction_final_kernel(const FracPartial *__restrict__ partials, int blocks,
                                                                         double *__restrict__ fraction) {
    __shared__ FracPartial lds[COL_THREADS];
    FracPartial p = {0.0, 0.0};
    if ((int)threadIdx.x < blocks) p = partials[threadIdx.x];
    frac_reduce(p, lds);
    if (threadIdx.x == 0) {
        fraction[0] = p.seen;
        fraction[1] = p.total;
    }
}

__global__ __launch_bounds__(COL_THREADS) void col_compact_kernel(const float *__restrict__ verts, const uint8_t *__restrict__ seen,
                                                                  const int *__restrict__ pos, int n_verts, int n_seen,
                                                                  int *__restrict__ seen_idx, float *__restrict__ seen_xyz,
                                                                  int *__restrict__ hidden_idx, float *__restrict__ hidden_xyz) {
    const long long vl = (long long)blockIdx.x * COL_THREADS + threadIdx.x;
    if (vl >= n_verts) return;
    const int before = pos[vl];                                   // seen vertices up to and including this one
    int *idx;
    float *xyz;
    long long k, limit;
    if (seen[vl]) {
        idx = seen_idx, xyz = seen_xyz, k = (long long)before - 1, limit = n_seen;
    } else {
        idx = hidden_idx, xyz = hidden_xyz, k = vl - before, limit = (long long)n_verts - n_seen;
    }
    if (k < 0 || k >= limit) return;                              // (a count that is not this mesh's: nothing out of bounds)
    idx[k] = (int)vl;
    for (int a = 0; a < 3; ++a) xyz[k * 3 + a] = verts[vl * 3 + a];
}

__global__ __launch_bounds__(COL_THREADS) void col_fill_kernel(const int *__restrict__ hidden_idx, const int *__restrict__ seen_idx,
                                                               const int *__restrict__ nearest, const float *__restrict__ dist,
                                                               int n_verts, int n_seen, double fade, double b0, double b1, double b2,
                                                               uint8_t *__restrict__ colors, int *__restrict__ source) {
    const long long kl = (long long)blockIdx.x * COL_THREADS + threadIdx.x;
    if (kl >= (long long)n_verts - n_seen) return;
    const int v = hidden_idx[kl];
    if (v < 0 || v >= n_verts) return;
    const double base[3] = {255.0 * b0, 255.0 * b1, 255.0 * b2};
    if (n_seen == 0) {
        for (int c = 0; c < 3; ++c) colors[(size_t)v * 3 + c] = col_round(base[c]);
        source[v] = -1;
        return;
    }
    const int j = nearest[kl];
    if (j < 0 || j >= n_seen) return;
    const int src = seen_idx[j];
    if (src < 0 || src >= n_verts) return;
    double t = 0.0;
    if (fade > 0.0) {
        t = sqrt((double)dist[kl]) / fade;
        if (!(t <= 1.0)) t = 1.0;
    }
    for (int c = 0; c < 3; ++c)
        colors[(size_t)v * 3 + c] = col_round((1.0 - t) * (double)colors[(size_t)src * 3 + c] + t * base[c]);
    source[v] = src;
}

size_t col_align(size_t n) { return (n + 255) & ~(size_t)255; }

struct ColScratch {
    size_t pos, tiles, proj, partials, zbuf, total;
};

ColScratch col_scratch(int n_verts, int Hz, int Wz) {
    ColScratch s;
    s.pos = 0;
    s.tiles = s.pos + col_align((size_t)n_verts * 4);
    s.proj = s.tiles + col_align(((size_t)scan_tiles(n_verts) + 1) * 4);
    s.partials = s.proj + col_align((size_t)n_verts * 3 * sizeof(double));
    s.zbuf = s.partials + col_align((size_t)FRAC_MAX_BLOCKS * sizeof(FracPartial));
    s.total = s.zbuf + col_align((size_t)Hz * Wz * sizeof(unsigned long long));
    return s;
}

bool col_sizes_ok(const char *who, int n_verts, int n_tris) {
    if (n_verts < 0 || n_tris < 0) {
        zs::set_err("%s: negative size (n_verts=%d n_tris=%d)", who, n_verts, n_tris);
        return false;
    }
    if (n_verts > COL_MAX || n_tris > COL_MAX) {
        zs::set_err("%s: too large (n_verts=%d n_tris=%d > 2^29)", who, n_verts, n_tris);
        return false;
    }
    return true;
}

bool col_view_ok(int H, int W, int ss) {
    return H >= 1 && W >= 1 && ss >= 1 && (long long)H * ss <= COL_MAX_SIDE && (long long)W * ss <= COL_MAX_SIDE;
}

dim3 col_grid(long long n) { return dim3((unsigned)((n + COL_THREADS - 1) / COL_THREADS)); }

}  // namespace

extern "C" size_t zs_mesh_colors_workspace_bytes(int n_verts, int n_tris, int H, int W, int ss) {
    if (n_verts <= 0 || n_tris < 0 || n_verts > COL_MAX || n_tris > COL_MAX || !col_view_ok(H, W, ss)) return 0;
    return col_scratch(n_verts, H * ss, W * ss).total;
}

extern "C" int zs_mesh_colors_seen(const float *vertices, const int *faces, const float *normals, int n_verts, int n_tris,
                                   const float *image, const float *mask, int H, int W, const float *K, const float *mean,
                                   const float *scale, int ss, double depth_tol, double min_cos, uint8_t *colors, uint8_t *seen,
                                   int *source, int *n_seen, double *fraction, void *workspace, void *stream) {
    const char *who = "zs_mesh_colors_seen";
    if (!col_sizes_ok(who, n_verts, n_tris)) return 0;
    if (!col_view_ok(H, W, ss)) {
        zs::set_err("%s: bad image size (H=%d W=%d ss=%d; ss H and ss W at most %d)", who, H, W, ss, COL_MAX_SIDE);
        return 0;
    }
    if (!(depth_tol >= 0.0) || !(min_cos >= -1.0 && min_cos <= 1.0)) {
        zs::set_err("%s: bad thresholds (depth_tol=%g min_cos=%g)", who, depth_tol, min_cos);
        return 0;
    }
    if (n_verts == 0) return 1;
    if (!vertices || !normals || !image || !mask || !K || !mean || !scale || !colors || !seen || !source || !n_seen || !fraction ||
        !workspace || (n_tris > 0 && !faces)) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) {
        zs::set_err("%s: workspace must be 8-byte aligned", who);
        return 0;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    ColView vw;
    vw.H = H, vw.W = W, vw.ss = ss, vw.Hz = H * ss, vw.Wz = W * ss;
    const ColScratch s = col_scratch(n_verts, vw.Hz, vw.Wz);
    char *base = static_cast<char *>(workspace);
    int *pos = reinterpret_cast<int *>(base + s.pos), *tile_tot = reinterpret_cast<int *>(base + s.tiles);
    double *proj = reinterpret_cast<double *>(base + s.proj);
    FracPartial *partials = reinterpret_cast<FracPartial *>(base + s.partials);
    unsigned long long *zbuf = reinterpret_cast<unsigned long long *>(base + s.zbuf);
    const dim3 block(COL_THREADS);
    const int tiles = scan_tiles(n_verts);

    if (hipMemsetAsync(zbuf, 0, (size_t)vw.Hz * vw.Wz * sizeof(unsigned long long), st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    hipLaunchKernelGGL(col_project_kernel, col_grid(n_verts), block, 0, st, vertices, n_verts, K, mean, scale, proj);
    if (n_tris > 0)
        hipLaunchKernelGGL(col_zbuffer_kernel, col_grid(n_tris), block, 0, st, faces, n_tris, n_verts, static_cast<const double *>(proj),
                           vw, zbuf);
    hipLaunchKernelGGL(col_seen_kernel, col_grid(n_verts), block, 0, st, vertices, faces, normals, n_verts, n_tris,
                       static_cast<const double *>(proj), image, mask, mean, scale, vw, depth_tol, min_cos,
                       static_cast<const unsigned long long *>(zbuf), colors, seen, source, pos);
    const int blocks = n_tris > 0 ? frac_blocks(n_tris) : 0;
    if (blocks)
        hipLaunchKernelGGL(col_fraction_partial_kernel, dim3(blocks), block, 0, st, vertices, faces, n_tris, n_verts,
                           static_cast<const uint8_t *>(seen), partials);
    hipLaunchKernelGGL(col_fraction_final_kernel, dim3(1), block, 0, st, static_cast<const FracPartial *>(partials), blocks, fraction);
    hipLaunchKernelGGL((scan_tiles_kernel<int, true>), dim3(tiles), dim3(256), 0, st, pos, (long long)n_verts, tile_tot);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(tiles), dim3(256), 0, st, pos, (long long)n_verts,
                       static_cast<const int *>(tile_tot), tiles, n_seen);
    return zs::check_launch(who) ? 1 : 0;
}

extern "C" int zs_mesh_colors_compact(const float *vertices, const uint8_t *seen, int n_verts, int n_seen, const void *workspace,
                                      int *seen_idx, float *seen_xyz, int *hidden_idx, float *hidden_xyz, void *stream) {
    const char *who = "zs_mesh_colors_compact";
    if (!col_sizes_ok(who, n_verts, 0)) return 0;
    if (n_seen < 0 || n_seen > n_verts) {
        zs::set_err("%s: bad count (n_seen=%d of %d vertices)", who, n_seen, n_verts);
        return 0;
    }
    if (n_verts == 0) return 1;
    if (!vertices || !seen || !workspace || (n_seen > 0 && (!seen_idx || !seen_xyz)) ||
        (n_seen < n_verts && (!hidden_idx || !hidden_xyz))) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) {
        zs::set_err("%s: workspace must be 8-byte aligned", who);
        return 0;
    }
    const int *pos = reinterpret_cast<const int *>(static_cast<const char *>(workspace));      // ColScratch.pos == 0
    hipLaunchKernelGGL(col_compact_kernel, col_grid(n_verts), dim3(COL_THREADS), 0, static_cast<hipStream_t>(stream), vertices, seen,
                       pos, n_verts, n_seen, seen_idx, seen_xyz, hidden_idx, hidden_xyz);
    return zs::check_launch(who) ? 1 : 0;
}

extern "C" int zs_mesh_colors_fill(const int *hidden_idx, const int *seen_idx, const int *nearest, const float *dist, int n_verts,
                                   int n_seen, double fade, const float *base_rgb, uint8_t *colors, int *source, void *stream) {
    const char *who = "zs_mesh_colors_fill";
    if (!col_sizes_ok(who, n_verts, 0)) return 0;
    if (n_seen < 0 || n_seen > n_verts) {
        zs::set_err("%s: bad count (n_seen=%d of %d vertices)", who, n_seen, n_verts);
        return 0;
    }
    if (!(fade >= 0.0)) {
        zs::set_err("%s: fade must be >= 0 (0 = no fade), got %g", who, fade);
        return 0;
    }
    if (n_verts == n_seen) return 1;                              // nothing hidden (an empty mesh included)
    if (!hidden_idx || !base_rgb || !colors || !source || (n_seen > 0 && (!seen_idx || !nearest || !dist))) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    hipLaunchKernelGGL(col_fill_kernel, col_grid((long long)n_verts - n_seen), dim3(COL_THREADS), 0, static_cast<hipStream_t>(stream),
                       hidden_idx, seen_idx, nearest, dist, n_verts, n_seen, fade, (double)base_rgb[0], (double)base_rgb[1],
                       (double)base_rgb[2], colors, source);
    return zs::check_launch(who) ? 1 : 0;
}
