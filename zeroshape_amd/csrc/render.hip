// Mesh turntable renderer on the GPU (gfx950): a z-buffer rasteriser over the triangle soup zs_mc_emit writes.
//
// Replaces the reference's dump_meshes_viz / visualize_mesh (utils/util_vis.py:112-127, 310-405), which render 180 frames
// per sample with pyrender on OpenGL - not available on a headless compute node.  pyrender's PBR pixels are NOT reproduced:
// there is no GL, pyrender or trimesh to compare against, so that parity is "unpinned" (DESIGN.md section 5).  What is
// pinned (tests/test_gpu_render.py, a float64 numpy rasteriser) is the geometry - which triangle is visible at which
// pixel and at what depth - and the shading formula below.
//
// Pipeline (all frames of a turntable in one call, the soup never leaves HBM):
//   mesh_stats   : bounding box + signed volume sum(v0 . (v1 x v2)) / 6; per-block partials in a fixed order, then one
//                  block sums the partials in a fixed order - no float atomics, bit-reproducible
//   scatter      : one thread per (frame, triangle): pre-transform, camera transform, projection, then a loop over the
//                  pixel centres of the clamped bounding box with ONE 64-bit atomicMax per covered pixel on
//                  zbuffer[f][i][j] = (~bits(depth) << 32) | ~triangle: the maximum is the nearest depth and, at exactly
//                  equal depth, the smaller index - order-independent, hence deterministic (0 = nothing hit)
//   resolve      : one thread per pixel: decodes the winner, shades it flat, writes rgb (+ depth, + tri)
//
// Pre-transform (applied on the fly, never written back): v' = (flip * v - centre) * scale, and v1 <-> v2 of every
// triangle when winding < 0 - dump_meshes_viz's two 180-degree rotations (x, y, z) -> (x, -y, -z), scale_to_unit_cube and
// trimesh.repair.fix_inversion; zeroshape_amd/utils/util_vis.py derives the eight numbers from mesh_stats.
//
// Camera (pyrender's convention): looks along -z of its own frame, +y up; cams[f] = position (3) + camera-to-world
// rotation (3x3, row-major).  With zv = -z_c:
//   x_pix = (x_c / (zv tan(yfov/2) aspect) + 1) W/2,   y_pix = (1 - y_c / (zv tan(yfov/2))) H/2,   aspect = W/H
// the centre of pixel (row i, col j) is (j + 0.5, i + 0.5); a pixel is covered when all three barycentrics (edge functions
// over the signed area) are >= 0 - inclusive on every edge, so neighbours leave no cracks and the depth test decides shared
// pixels.  Zero-area triangles and triangles with any vertex at zv <= znear are skipped whole.  Depth is perspective
// correct, 1 / (w0/z0 + w1/z1 + w2/z2), rounded to fp32 for the z-buffer word.
//
// Shading (flat): c = base * (0.3 + 0.7 |n . l|), n = unit face normal in camera space, l = unit vector from the hit point to
// the camera (the reference's light rides on the camera pose); stored uint8(floor(255 c + 0.5)); background white.
//
// The geometry runs in fp64: per (frame, triangle) it is ~200 flops - 12 M pairs at 180 frames x 69 k triangles are a few
// GFLOP, far below the cost of the launch's memory traffic - and coverage then agrees with a float64 restatement on every
// pixel.  Built with -ffp-contract=off so that the restatement can follow it operation for operation.
#include "zs_common.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int RENDER_THREADS = 256;
constexpr int STATS_THREADS = 256;
constexpr int STATS_MAX_BLOCKS = 256;      // partials the final block sums, one per thread

struct StatsPartial {                      // 32 bytes
    float mn[3], mx[3];
    double vol6;                           // sum of v0 . (v1 x v2)
};

inline int stats_blocks(int n) {
    const int b = (n + STATS_THREADS - 1) / STATS_THREADS;
    return b < STATS_MAX_BLOCKS ? b : STATS_MAX_BLOCKS;
}

// tree reduction of one partial per thread, fixed order; the result is in p of thread 0
__device__ __forceinline__ void stats_reduce(StatsPartial &p, StatsPartial *lds) {
    const int tid = threadIdx.x;
    lds[tid] = p;
    __syncthreads();
    for (int s = STATS_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            StatsPartial &a = lds[tid];
            const StatsPartial &b = lds[tid + s];
            for (int c = 0; c < 3; ++c) {
                a.mn[c] = fminf(a.mn[c], b.mn[c]);
                a.mx[c] = fmaxf(a.mx[c], b.mx[c]);
            }
            a.vol6 += b.vol6;
        }
        __syncthreads();
    }
    p = lds[0];
}

__device__ __forceinline__ StatsPartial stats_identity() {
    StatsPartial p;
    for (int c = 0; c < 3; ++c) {
        p.mn[c] = INFINITY;
        p.mx[c] = -INFINITY;
    }
    p.vol6 = 0.0;
    return p;
}

__global__ __launch_bounds__(STATS_THREADS) void mesh_stats_partial_kernel(const float *__restrict__ tris, int n,
                                                                            StatsPartial *__restrict__ partials) {
    __shared__ StatsPartial lds[STATS_THREADS];
    StatsPartial p = stats_identity();
    for (long long t = (long long)blockIdx.x * STATS_THREADS + threadIdx.x; t < n; t += (long long)gridDim.x * STATS_THREADS) {
        const float *v = tris + t * 9;
        double d[9];
        for (int k = 0; k < 9; ++k) {
            const float x = v[k];
            p.mn[k % 3] = fminf(p.mn[k % 3], x);
            p.mx[k % 3] = fmaxf(p.mx[k % 3], x);
            d[k] = (double)x;
        }
        const double cx = d[4] * d[8] - d[5] * d[7], cy = d[5] * d[6] - d[3] * d[8], cz = d[3] * d[7] - d[4] * d[6];
        p.vol6 += d[0] * cx + d[1] * cy + d[2] * cz;
    }
    stats_reduce(p, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

__global__ __launch_bounds__(STATS_THREADS) void mesh_stats_final_kernel(const StatsPartial *__restrict__ partials, int blocks,
                                                                          float *__restrict__ out) {
    __shared__ StatsPartial lds[STATS_THREADS];
    StatsPartial p = (int)threadIdx.x < blocks ? partials[threadIdx.x] : stats_identity();
    stats_reduce(p, lds);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; ++c) {
            out[c] = p.mn[c];
            out[3 + c] = p.mx[c];
        }
        out[6] = (float)(p.vol6 / 6.0);
    }
}

struct RenderXform {
    double flip[3], centre[3], scale;
    int swap;                              // exchange v1 and v2 of every triangle
};

struct RenderView {
    double ta, tn;                         // tan(yfov/2) * aspect, tan(yfov/2)
    double half_w, half_h, znear;
    int H, W;
};

// triangle t, pre-transformed, in the frame of the camera `cam` (position, row-major camera-to-world rotation)
__device__ __forceinline__ void camera_triangle(const float *__restrict__ tris, int t, const RenderXform &xf,
                                                const float *__restrict__ cam, double v[3][3]) {
    const float *p = tris + (size_t)t * 9;
    double c[12];
    for (int k = 0; k < 12; ++k) c[k] = (double)cam[k];
    for (int k = 0; k < 3; ++k) {
        const int src = (xf.swap && k) ? 3 - k : k;
        double w[3];
        for (int a = 0; a < 3; ++a) w[a] = ((double)p[src * 3 + a] * xf.flip[a] - xf.centre[a]) * xf.scale - c[a];
        for (int a = 0; a < 3; ++a) v[k][a] = c[3 + a] * w[0] + c[6 + a] * w[1] + c[9 + a] * w[2];    // R^T (p - pos)
    }
}

__global__ __launch_bounds__(RENDER_THREADS) void render_scatter_kernel(const float *__restrict__ tris, int n, RenderXform xf,
                                                                        const float *__restrict__ cams, RenderView vw,
                                                                        unsigned long long *__restrict__ zbuf) {
    const long long tl = (long long)blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (tl >= n) return;
    const int t = (int)tl, f = blockIdx.y;
    double v[3][3];
    camera_triangle(tris, t, xf, cams + (size_t)f * 12, v);
    double z[3], x[3], y[3];
    for (int k = 0; k < 3; ++k) {
        z[k] = -v[k][2];
        if (!(z[k] > vw.znear)) return;                       // at or behind the near plane (or NaN): skipped whole
        x[k] = (v[k][0] / (z[k] * vw.ta) + 1.0) * vw.half_w;
        y[k] = (1.0 - v[k][1] / (z[k] * vw.tn)) * vw.half_h;
    }
    const double area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]);
    if (!(fabs(area) > 0.0) || !(fabs(area) <= 1.0e300)) return;      // zero area, NaN or overflow
    // pixel centres (j + 0.5, i + 0.5) inside the bounding box, clamped to the frame (in fp64: the box may be huge)
    const double xlo = fmin(fmin(x[0], x[1]), x[2]), xhi = fmax(fmax(x[0], x[1]), x[2]);
    const double ylo = fmin(fmin(y[0], y[1]), y[2]), yhi = fmax(fmax(y[0], y[1]), y[2]);
    const int j0 = (int)fmin(fmax(ceil(xlo - 0.5), 0.0), (double)vw.W), j1 = (int)fmax(fmin(floor(xhi - 0.5), (double)(vw.W - 1)), -1.0);
    const int i0 = (int)fmin(fmax(ceil(ylo - 0.5), 0.0), (double)vw.H), i1 = (int)fmax(fmin(floor(yhi - 0.5), (double)(vw.H - 1)), -1.0);
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
            atomicMax(zbuf + ((size_t)f * vw.H + i) * vw.W + j, key);
        }
    }
}

__global__ __launch_bounds__(RENDER_THREADS) void render_resolve_kernel(const float *__restrict__ tris, RenderXform xf,
                                                                        const float *__restrict__ cams, RenderView vw,
                                                                        long long pixels, float br, float bg, float bb,
                                                                        const unsigned long long *__restrict__ zbuf,
                                                                        uint8_t *__restrict__ rgb, float *__restrict__ depth,
                                                                        int *__restrict__ tri) {
    const long long q = (long long)blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (q >= pixels) return;
    const unsigned long long key = zbuf[q];
    uint8_t r = 255, g = 255, b = 255;
    float d = INFINITY;
    int t = -1;
    if (key) {
        t = (int)~(unsigned)key;
        d = __uint_as_float(~(unsigned)(key >> 32));
        const long long hw = (long long)vw.H * vw.W;
        const int f = (int)(q / hw), rem = (int)(q - (long long)f * hw), i = rem / vw.W, j = rem - i * vw.W;
        double v[3][3];
        camera_triangle(tris, t, xf, cams + (size_t)f * 12, v);
        const double e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
        const double e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        // the hit point is depth * (dx, dy, -1) in camera space; the camera sits at the origin
        const double dx = (((double)j + 0.5) / vw.half_w - 1.0) * vw.ta, dy = (1.0 - ((double)i + 0.5) / vw.half_h) * vw.tn;
        const double nn = sqrt(nx * nx + ny * ny + nz * nz), ll = sqrt(dx * dx + dy * dy + 1.0);
        const double ndl = nn > 0.0 ? fabs(nz - nx * dx - ny * dy) / (nn * ll) : 0.0;
        const double shade = 0.3 + 0.7 * ndl;
        r = (uint8_t)fmin(fmax(floor(255.0 * ((double)br * shade) + 0.5), 0.0), 255.0);
        g = (uint8_t)fmin(fmax(floor(255.0 * ((double)bg * shade) + 0.5), 0.0), 255.0);
        b = (uint8_t)fmin(fmax(floor(255.0 * ((double)bb * shade) + 0.5), 0.0), 255.0);
    }
    rgb[q * 3 + 0] = r;
    rgb[q * 3 + 1] = g;
    rgb[q * 3 + 2] = b;
    if (depth) depth[q] = d;
    if (tri) tri[q] = t;
}

// The resolve of zs_render_frames_colored: the same winner, depth, normal and light, but the albedo is interpolated from
// the winner's three corner colours instead of one base colour.  The projected corners and w0, w1, w2 at the pixel centre are
// recomputed exactly as the scatter computed them (the same operations on the same inputs: the same bits), and the albedo is
// perspective correct in fp64: a = (sum w_k / z_k c_k / 255) / (sum w_k / z_k).  A kernel of its own, so that the uncoloured
// frames cannot change.
__global__ __launch_bounds__(RENDER_THREADS) void render_resolve_colored_kernel(const float *__restrict__ tris, RenderXform xf,
                                                                                const float *__restrict__ cams, RenderView vw,
                                                                                long long pixels,
                                                                                const uint8_t *__restrict__ corner_rgb,
                                                                                const unsigned long long *__restrict__ zbuf,
                                                                                uint8_t *__restrict__ rgb, float *__restrict__ depth,
                                                                                int *__restrict__ tri) {
    const long long q = (long long)blockIdx.x * RENDER_THREADS + threadIdx.x;
    if (q >= pixels) return;
    const unsigned long long key = zbuf[q];
    uint8_t out[3] = {255, 255, 255};
    float d = INFINITY;
    int t = -1;
    if (key) {
        t = (int)~(unsigned)key;
        d = __uint_as_float(~(unsigned)(key >> 32));
        const long long hw = (long long)vw.H * vw.W;
        const int f = (int)(q / hw), rem = (int)(q - (long long)f * hw), i = rem / vw.W, j = rem - i * vw.W;
        double v[3][3];
        camera_triangle(tris, t, xf, cams + (size_t)f * 12, v);
        double z[3], x[3], y[3];
        for (int k = 0; k < 3; ++k) {
            z[k] = -v[k][2];
            x[k] = (v[k][0] / (z[k] * vw.ta) + 1.0) * vw.half_w;
            y[k] = (1.0 - v[k][1] / (z[k] * vw.tn)) * vw.half_h;
        }
        const double area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]);
        const double px = (double)j + 0.5, py = (double)i + 0.5;
        const double w0 = ((x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])) / area;
        const double w1 = ((x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])) / area;
        const double w2 = ((x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])) / area;
        const double q0 = w0 / z[0], q1 = w1 / z[1], q2 = w2 / z[2];
        const double den = q0 + q1 + q2;
        const double e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
        const double e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const double dx = (((double)j + 0.5) / vw.half_w - 1.0) * vw.ta, dy = (1.0 - ((double)i + 0.5) / vw.half_h) * vw.tn;
        const double nn = sqrt(nx * nx + ny * ny + nz * nz), ll = sqrt(dx * dx + dy * dy + 1.0);
        const double ndl = nn > 0.0 ? fabs(nz - nx * dx - ny * dy) / (nn * ll) : 0.0;
        const double shade = 0.3 + 0.7 * ndl;
        const uint8_t *c = corner_rgb + (size_t)t * 9;
        // (xf.swap exchanges corners 1 and 2 of the triangle: their colours go with them)
        const int c1 = xf.swap ? 2 : 1, c2 = xf.swap ? 1 : 2;
        for (int ch = 0; ch < 3; ++ch) {
            const double a = (q0 * ((double)c[ch] / 255.0) + q1 * ((double)c[c1 * 3 + ch] / 255.0) + q2 * ((double)c[c2 * 3 + ch] / 255.0)) / den;
            const double p = floor(255.0 * a * shade + 0.5);
            out[ch] = (uint8_t)(p >= 0.0 ? fmin(p, 255.0) : 0.0);
        }
    }
    rgb[q * 3 + 0] = out[0];
    rgb[q * 3 + 1] = out[1];
    rgb[q * 3 + 2] = out[2];
    if (depth) depth[q] = d;
    if (tri) tri[q] = t;
}

constexpr int RENDER_MAX_FRAMES = 65535;   // frames ride on blockIdx.y
constexpr int RENDER_MAX_SIDE = 16384;

bool render_dims_ok(int frames, int H, int W) {
    return frames >= 0 && frames <= RENDER_MAX_FRAMES && H >= 1 && H <= RENDER_MAX_SIDE && W >= 1 && W <= RENDER_MAX_SIDE;
}

}  // namespace

extern "C" size_t zs_mesh_stats_scratch_bytes(int n_tris) {
    return n_tris <= 0 ? 0 : (size_t)stats_blocks(n_tris) * sizeof(StatsPartial);
}

extern "C" int zs_mesh_stats(const float *tris, int n_tris, float *out, void *scratch, void *stream) {
    if (n_tris < 0) {
        zs::set_err("zs_mesh_stats: negative size");
        return 0;
    }
    if (!out) {
        zs::set_err("zs_mesh_stats: null pointer");
        return 0;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_tris == 0) {                     // empty mesh -> zeros
        (void)hipMemsetAsync(out, 0, 7 * sizeof(float), s);
        return zs::check_launch("zs_mesh_stats") ? 1 : 0;
    }
    if (!tris || !scratch) {
        zs::set_err("zs_mesh_stats: null pointer");
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("zs_mesh_stats: scratch must be 8-byte aligned");
        return 0;
    }
    const int blocks = stats_blocks(n_tris);
    StatsPartial *partials = static_cast<StatsPartial *>(scratch);
    hipLaunchKernelGGL(mesh_stats_partial_kernel, dim3(blocks), dim3(STATS_THREADS), 0, s, tris, n_tris, partials);
    hipLaunchKernelGGL(mesh_stats_final_kernel, dim3(1), dim3(STATS_THREADS), 0, s, partials, blocks, out);
    return zs::check_launch("zs_mesh_stats") ? 1 : 0;
}

extern "C" size_t zs_render_zbuffer_bytes(int frames, int H, int W) {
    if (!render_dims_ok(frames, H, W)) return 0;
    return (size_t)frames * H * W * sizeof(unsigned long long);
}

namespace {

// zs_render_frames (corner_rgb == NULL: one base colour) and zs_render_frames_colored (base_rgb == NULL): the same checks, clear
// and scatter; only the resolve kernel differs
int render_frames(const char *who, const float *tris, int n_tris, const float *xform, const float *cams, int frames, int H, int W,
                  float yfov, float znear, const float *base_rgb, const uint8_t *corner_rgb, uint8_t *rgb, float *depth, int *tri,
                  void *zbuffer, void *stream) {
    if (n_tris < 0 || !render_dims_ok(frames, H, W)) {
        zs::set_err("%s: bad size (n_tris=%d frames=%d H=%d W=%d)", who, n_tris, frames, H, W);
        return 0;
    }
    if (!(yfov > 0.0f && yfov < 3.14159f) || !(znear > 0.0f)) {
        zs::set_err("%s: bad camera (yfov=%g znear=%g)", who, (double)yfov, (double)znear);
        return 0;
    }
    const long long pixels = (long long)frames * H * W;
    if (pixels > 0x7fffffffLL * RENDER_THREADS) {
        zs::set_err("%s: %lld pixels exceed one launch", who, pixels);
        return 0;
    }
    if (frames == 0) return 1;
    if (!xform || !cams || (!base_rgb && !corner_rgb) || !rgb || !zbuffer || (n_tris > 0 && !tris)) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(zbuffer) & 7) {
        zs::set_err("%s: zbuffer must be 8-byte aligned", who);
        return 0;
    }
    RenderXform xf;
    for (int a = 0; a < 3; ++a) {
        xf.flip[a] = (double)xform[a];
        xf.centre[a] = (double)xform[3 + a];
    }
    xf.scale = (double)xform[6];
    xf.swap = xform[7] < 0.0f;
    RenderView vw;
    vw.tn = tan((double)yfov * 0.5);
    vw.ta = vw.tn * ((double)W / (double)H);
    vw.half_w = (double)W * 0.5;
    vw.half_h = (double)H * 0.5;
    vw.znear = (double)znear;
    vw.H = H;
    vw.W = W;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long *zbuf = static_cast<unsigned long long *>(zbuffer);
    (void)hipMemsetAsync(zbuf, 0, (size_t)pixels * sizeof(unsigned long long), s);
    if (n_tris > 0)
        hipLaunchKernelGGL(render_scatter_kernel, dim3((unsigned)(((long long)n_tris + RENDER_THREADS - 1) / RENDER_THREADS), (unsigned)frames),
                           dim3(RENDER_THREADS), 0, s, tris, n_tris, xf, cams, vw, zbuf);
    const dim3 pgrid((unsigned)((pixels + RENDER_THREADS - 1) / RENDER_THREADS));
    if (corner_rgb)
        hipLaunchKernelGGL(render_resolve_colored_kernel, pgrid, dim3(RENDER_THREADS), 0, s, tris, xf, cams, vw, pixels, corner_rgb,
                           zbuf, rgb, depth, tri);
    else
        hipLaunchKernelGGL(render_resolve_kernel, pgrid, dim3(RENDER_THREADS), 0, s, tris, xf, cams, vw, pixels, base_rgb[0],
                           base_rgb[1], base_rgb[2], zbuf, rgb, depth, tri);
    return zs::check_launch(who) ? 1 : 0;
}

}  // namespace

extern "C" int zs_render_frames(const float *tris, int n_tris, const float *xform, const float *cams, int frames, int H,
                                int W, float yfov, float znear, const float *base_rgb, uint8_t *rgb, float *depth, int *tri,
                                void *zbuffer, void *stream) {
    return render_frames("zs_render_frames", tris, n_tris, xform, cams, frames, H, W, yfov, znear, base_rgb, nullptr, rgb, depth, tri,
                         zbuffer, stream);
}

extern "C" int zs_render_frames_colored(const float *tris, int n_tris, const float *xform, const float *cams, int frames, int H,
                                        int W, float yfov, float znear, const uint8_t *corner_rgb, uint8_t *rgb, float *depth,
                                        int *tri, void *zbuffer, void *stream) {
    if (!corner_rgb && n_tris > 0 && frames > 0 && render_dims_ok(frames, H, W)) {
        zs::set_err("zs_render_frames_colored: null pointer");
        return 0;
    }
    static const float white[3] = {1.0f, 1.0f, 1.0f};             // (n_tris == 0: white frames, no corner is read)
    return render_frames("zs_render_frames_colored", tris, n_tris, xform, cams, frames, H, W, yfov, znear,
                         corner_rgb ? nullptr : white, corner_rgb, rgb, depth, tri, zbuffer, stream);
}
