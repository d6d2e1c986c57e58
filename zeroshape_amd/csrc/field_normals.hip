// Vertex normals from the occupancy field's own gradient (eval_3D.field_normals): the two launches around
// Implicit.field_gradient.
//
// zs_mesh_to_field_points: marching cubes scales a vertex at grid index u to v = min + u (max - min) / G with G = the
//   number of samples per axis (utils/eval_3D.py:252-255 of the reference), while sample u of the grid linspace(min, max, G)
//   sits at min + u (max - min) / (G - 1).  The field was evaluated THERE, so its gradient is taken at
//   p = min + (v - min) G / (G - 1): fp64 as written, rounded to fp32.
// zs_field_normals_finish: n = -g / |g| (occupancy rises inwards: minus the gradient points out), |g| and the division in
//   fp64, rounded to fp32 like the weld's normals; where |g| is zero, infinite or NaN the vertex takes its fallback normal
//   (the weld's area-weighted one; (0, 0, 0) without a fallback) and *n_fallback counts it (one atomic add per such vertex).
#include "zs_common.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>

namespace {

constexpr int FN_THREADS = 256;

__global__ __launch_bounds__(FN_THREADS) void mesh_to_field_points_kernel(const float *__restrict__ vertices, size_t n3, float range_min,
                                                                          int G, float *__restrict__ points) {
    const size_t i = (size_t)blockIdx.x * FN_THREADS + threadIdx.x;
    if (i >= n3) return;
    const double lo = range_min;
    points[i] = (float)(lo + ((double)vertices[i] - lo) * (double)G / (double)(G - 1));
}

__global__ __launch_bounds__(FN_THREADS) void field_normals_finish_kernel(const float *__restrict__ grad, const float *__restrict__ fallback,
                                                                          size_t n, float *__restrict__ normals,
                                                                          int *__restrict__ n_fallback) {
    const size_t v = (size_t)blockIdx.x * FN_THREADS + threadIdx.x;
    if (v >= n) return;
    const double gx = grad[v * 3], gy = grad[v * 3 + 1], gz = grad[v * 3 + 2];
    const double len = sqrt(gx * gx + gy * gy + gz * gz);
    const bool ok = len > 0.0 && len < (double)INFINITY;          // a zero, infinite or NaN gradient: the fallback
    float out[3];
    if (ok) {
        out[0] = (float)(-gx / len);
        out[1] = (float)(-gy / len);
        out[2] = (float)(-gz / len);
    } else {
        for (int d = 0; d < 3; d++) out[d] = fallback ? fallback[v * 3 + d] : 0.0f;
        atomicAdd(n_fallback, 1);
    }
    for (int d = 0; d < 3; d++) normals[v * 3 + d] = out[d];
}

unsigned blocks(size_t total) { return (unsigned)((total + FN_THREADS - 1) / FN_THREADS); }

}  // namespace

extern "C" int zs_mesh_to_field_points(const float *vertices, size_t n, float range_min, int G, float *points, void *stream) {
    if (G < 2) {
        zs::set_err("zs_mesh_to_field_points: bad grid (G=%d: at least two samples per axis)", G);
        return 0;
    }
    if (n == 0) return 1;
    if (n > ((size_t)1 << 36)) {
        zs::set_err("zs_mesh_to_field_points: too large (n=%zu > 2^36)", n);
        return 0;
    }
    if (!vertices || !points) {
        zs::set_err("zs_mesh_to_field_points: null pointer");
        return 0;
    }
    hipLaunchKernelGGL(mesh_to_field_points_kernel, dim3(blocks(n * 3)), dim3(FN_THREADS), 0, static_cast<hipStream_t>(stream),
                       vertices, n * 3, range_min, G, points);
    return zs::check_launch("zs_mesh_to_field_points") ? 1 : 0;
}

extern "C" int zs_field_normals_finish(const float *grad, const float *fallback, size_t n, float *normals, int *n_fallback,
                                       void *stream) {
    if (n == 0) return 1;
    if (n > ((size_t)1 << 31)) {
        zs::set_err("zs_field_normals_finish: too large (n=%zu > 2^31)", n);
        return 0;
    }
    if (!grad || !normals || !n_fallback) {
        zs::set_err("zs_field_normals_finish: null pointer");
        return 0;
    }
    hipLaunchKernelGGL(field_normals_finish_kernel, dim3(blocks(n)), dim3(FN_THREADS), 0, static_cast<hipStream_t>(stream), grad,
                       fallback, n, normals, n_fallback);
    return zs::check_launch("zs_field_normals_finish") ? 1 : 0;
}
