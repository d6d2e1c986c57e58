// Welding a triangle soup into the indexed form (vertices, faces) on the GPU, with area-weighted vertex normals: the device
// form of SimpleMesh._weld (utils/eval_3D.py), which is `np.unique(keys, axis=0, return_index, return_inverse)` over the
// 3n corners of the soup.  Any soup, not only marching cubes': corners weld when their coordinates are equal, whatever made
// them.
//
// Key of a corner = the uint32 bit patterns of (x + 0.0f, y + 0.0f, z + 0.0f) (-0.0 and 0.0 are one vertex); unique keys in
// lexicographic (x, y, z) order AS UNSIGNED INTEGERS - np.unique's order of the rows, not float order.  A stable sort of
// the corners by that key puts the corners of one vertex into one contiguous run in ascending soup index, so the head of
// a run is the vertex's first occurrence (its un-canonicalised bits are the stored vertex) and a walk along the run visits
// the vertex's triangles in soup order.
//
// zs_mesh_weld:
//   weld_zkey_kernel            key = z bits, value = corner index
//   rocprim::radix_sort_pairs   32 bits, stable (LSD radix)
//   weld_xykey_kernel           key = x bits << 32 | y bits of the corner now at each position
//   rocprim::radix_sort_pairs   64 bits, stable: positions are now in (x, y, z) order, ties in soup order
//   weld_heads_kernel           1 where a position's key differs from the one before it
//   scan_tiles_kernel / scan_offsets_kernel (zs_scan.h)   inclusive: position -> 1 + its vertex index
//   weld_faces_kernel           faces[corner] = vertex index; run_start[vertex] = position of its head; the vertex count
// zs_mesh_weld_vertices (after the caller has read the count and allocated):
//   weld_vertices_kernel        a thread per vertex: the head's coordinates and - optionally - the normal: the sum over
//                               the run, in run order, of cross(v1 - v0, v2 - v0) in fp64, normalised in fp64, rounded to
//                               fp32.  No atomics anywhere: every output is a pure function of the soup.
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int MW_THREADS = 256;
constexpr int MW_MAX_TRIS = 1 << 29;        // 3 n corners stay below 2^31

__device__ __forceinline__ unsigned key_bits(float v) { return __float_as_uint(v + 0.0f); }

__global__ __launch_bounds__(MW_THREADS) void weld_zkey_kernel(const float *__restrict__ soup, int m, unsigned *__restrict__ keys,
                                                               unsigned *__restrict__ vals) {
    const int i = blockIdx.x * MW_THREADS + threadIdx.x;
    if (i >= m) return;
    keys[i] = key_bits(soup[(size_t)i * 3 + 2]);
    vals[i] = (unsigned)i;
}

__global__ __launch_bounds__(MW_THREADS) void weld_xykey_kernel(const float *__restrict__ soup, int m,
                                                                const unsigned *__restrict__ vals,
                                                                unsigned long long *__restrict__ keys) {
    const int j = blockIdx.x * MW_THREADS + threadIdx.x;
    if (j >= m) return;
    const size_t c = vals[j];
    keys[j] = ((unsigned long long)key_bits(soup[c * 3]) << 32) | key_bits(soup[c * 3 + 1]);
}

__global__ __launch_bounds__(MW_THREADS) void weld_heads_kernel(const float *__restrict__ soup, int m,
                                                                const unsigned long long *__restrict__ xy,
                                                                const unsigned *__restrict__ perm, int *__restrict__ heads) {
    const int j = blockIdx.x * MW_THREADS + threadIdx.x;
    if (j >= m) return;
    int head = 1;
    if (j > 0 && xy[j] == xy[j - 1])
        head = key_bits(soup[(size_t)perm[j] * 3 + 2]) != key_bits(soup[(size_t)perm[j - 1] * 3 + 2]);
    heads[j] = head;
}

// ids = the inclusive scan of the head flags: position j belongs to vertex ids[j] - 1
__global__ __launch_bounds__(MW_THREADS) void weld_faces_kernel(int m, const int *__restrict__ ids, const unsigned *__restrict__ perm,
                                                                int *__restrict__ faces, int *__restrict__ run_start,
                                                                int *__restrict__ count, int *__restrict__ n_verts) {
    const int j = blockIdx.x * MW_THREADS + threadIdx.x;
    if (j >= m) return;
    const int id = ids[j] - 1;
    faces[perm[j]] = id;
    if (j == 0 || ids[j - 1] != ids[j]) run_start[id] = j;
    if (j == m - 1) {
        *count = id + 1;
        *n_verts = id + 1;
    }
}

__global__ __launch_bounds__(MW_THREADS) void weld_vertices_kernel(const float *__restrict__ soup, int m,
                                                                   const unsigned *__restrict__ perm,
                                                                   const int *__restrict__ run_start, const int *__restrict__ count,
                                                                   int n_verts, float *__restrict__ vertices,
                                                                   float *__restrict__ normals) {
    const int v = blockIdx.x * MW_THREADS + threadIdx.x;
    const int total = min(n_verts, *count);          // (a caller's count beyond the weld's own reads nothing)
    if (v >= total) return;
    const int begin = run_start[v], end = v + 1 < *count ? run_start[v + 1] : m;
    const size_t head = perm[begin];
    vertices[(size_t)v * 3] = soup[head * 3];
    vertices[(size_t)v * 3 + 1] = soup[head * 3 + 1];
    vertices[(size_t)v * 3 + 2] = soup[head * 3 + 2];
    if (!normals) return;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    for (int k = begin; k < end; k++) {
        const float *t = soup + (size_t)(perm[k] / 3u) * 9;
        const double x0 = t[0], y0 = t[1], z0 = t[2];
        const double ax = (double)t[3] - x0, ay = (double)t[4] - y0, az = (double)t[5] - z0;
        const double bx = (double)t[6] - x0, by = (double)t[7] - y0, bz = (double)t[8] - z0;
        nx += ay * bz - az * by;
        ny += az * bx - ax * bz;
        nz += ax * by - ay * bx;
    }
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    const bool ok = len > 0.0 && len < (double)INFINITY;         // a zero, infinite or NaN sum: no normal
    normals[(size_t)v * 3] = ok ? (float)(nx / len) : 0.0f;
    normals[(size_t)v * 3 + 1] = ok ? (float)(ny / len) : 0.0f;
    normals[(size_t)v * 3 + 2] = ok ? (float)(nz / len) : 0.0f;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

size_t sort32_temp_bytes(int m) {
    size_t bytes = 0;
    unsigned *none = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, none, none, none, none, (size_t)m, 0u, 32u);
    return bytes;
}
size_t sort64_temp_bytes(int m) {
    size_t bytes = 0;
    unsigned long long *k = nullptr;
    unsigned *v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)m, 0u, 64u);
    return bytes;
}

// The scratch of one weld of m corners.  Regions that are never live together share their bytes:
//   a  z keys in | z keys out (sort 1), then the run starts (zs_mesh_weld_vertices reads them)
//   b  (x, y) keys in (sort 2)                 c  (x, y) keys out
//   d  corner indices in (sort 1), then the head flags and their scan
//   e  corner indices after sort 1             f  corner indices after sort 2 = the order (zs_mesh_weld_vertices reads it)
//   g  the scan's tile totals, then the vertex count
//   temp  the sorts' workspace, last
struct WeldScratch {
    size_t a, b, c, d, e, f, g, temp;
};
WeldScratch weld_scratch(int m) {
    const size_t a4 = align256((size_t)m * 4), a8 = align256((size_t)m * 8);
    WeldScratch s;
    s.a = 0;
    s.b = s.a + 2 * a4;
    s.c = s.b + a8;
    s.d = s.c + a8;
    s.e = s.d + a4;
    s.f = s.e + a4;
    s.g = s.f + a4;
    s.temp = s.g + align256(((size_t)scan_tiles(m) + 1) * 4);
    return s;
}
size_t weld_temp_bytes(int m) {
    const size_t t32 = sort32_temp_bytes(m), t64 = sort64_temp_bytes(m);
    return t32 > t64 ? t32 : t64;
}

}  // namespace

extern "C" size_t zs_mesh_weld_scratch_bytes(int n_tris) {
    if (n_tris <= 0 || n_tris > MW_MAX_TRIS) return 0;
    return weld_scratch(3 * n_tris).temp + align256(weld_temp_bytes(3 * n_tris));
}

extern "C" int zs_mesh_weld(const float *tris, int n_tris, int *faces, int *n_verts, void *scratch, void *stream) {
    if (n_tris < 0) {
        zs::set_err("zs_mesh_weld: negative size (n_tris=%d)", n_tris);
        return 0;
    }
    if (n_tris == 0) return 1;
    if (n_tris > MW_MAX_TRIS) {
        zs::set_err("zs_mesh_weld: too large (n_tris=%d > 2^29)", n_tris);
        return 0;
    }
    if (!tris || !faces || !n_verts || !scratch) {
        zs::set_err("zs_mesh_weld: null pointer");
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("zs_mesh_weld: scratch must be 8-byte aligned");
        return 0;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int m = 3 * n_tris;
    const WeldScratch s = weld_scratch(m);
    char *base = static_cast<char *>(scratch);
    const size_t a4 = align256((size_t)m * 4);
    unsigned *zkeys_in = reinterpret_cast<unsigned *>(base + s.a), *zkeys_out = reinterpret_cast<unsigned *>(base + s.a + a4);
    int *run_start = reinterpret_cast<int *>(base + s.a);
    unsigned long long *xy_in = reinterpret_cast<unsigned long long *>(base + s.b);
    unsigned long long *xy_out = reinterpret_cast<unsigned long long *>(base + s.c);
    unsigned *vals_in = reinterpret_cast<unsigned *>(base + s.d);
    int *ids = reinterpret_cast<int *>(base + s.d);
    unsigned *vals_z = reinterpret_cast<unsigned *>(base + s.e), *perm = reinterpret_cast<unsigned *>(base + s.f);
    int *tile_tot = reinterpret_cast<int *>(base + s.g);
    const int tiles = scan_tiles(m);
    int *count = tile_tot + tiles;
    void *temp = base + s.temp;
    const size_t sort_bytes = weld_temp_bytes(m);
    size_t temp_bytes = sort_bytes;
    const dim3 grid((m + MW_THREADS - 1) / MW_THREADS), block(MW_THREADS);

    hipLaunchKernelGGL(weld_zkey_kernel, grid, block, 0, st, tris, m, zkeys_in, vals_in);
    if (rocprim::radix_sort_pairs(temp, temp_bytes, zkeys_in, zkeys_out, vals_in, vals_z, (size_t)m, 0u, 32u, st) != hipSuccess) {
        zs::set_err("zs_mesh_weld: rocprim::radix_sort_pairs failed");
        return 0;
    }
    hipLaunchKernelGGL(weld_xykey_kernel, grid, block, 0, st, tris, m, static_cast<const unsigned *>(vals_z), xy_in);
    temp_bytes = sort_bytes;
    if (rocprim::radix_sort_pairs(temp, temp_bytes, xy_in, xy_out, vals_z, perm, (size_t)m, 0u, 64u, st) != hipSuccess) {
        zs::set_err("zs_mesh_weld: rocprim::radix_sort_pairs failed");
        return 0;
    }
    hipLaunchKernelGGL(weld_heads_kernel, grid, block, 0, st, tris, m, static_cast<const unsigned long long *>(xy_out),
                       static_cast<const unsigned *>(perm), ids);
    hipLaunchKernelGGL((scan_tiles_kernel<int, true>), dim3(tiles), dim3(256), 0, st, ids, (long long)m, tile_tot);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(tiles), dim3(256), 0, st, ids, (long long)m, static_cast<const int *>(tile_tot),
                       tiles, static_cast<int *>(nullptr));
    hipLaunchKernelGGL(weld_faces_kernel, grid, block, 0, st, m, static_cast<const int *>(ids), static_cast<const unsigned *>(perm),
                       faces, run_start, count, n_verts);
    return zs::check_launch("zs_mesh_weld") ? 1 : 0;
}

extern "C" int zs_mesh_weld_vertices(const float *tris, int n_tris, const void *scratch, int n_verts, float *vertices,
                                     float *normals, void *stream) {
    if (n_tris < 0 || n_verts < 0) {
        zs::set_err("zs_mesh_weld_vertices: negative size (n_tris=%d n_verts=%d)", n_tris, n_verts);
        return 0;
    }
    if (n_tris == 0 || n_verts == 0) return 1;
    if (n_tris > MW_MAX_TRIS) {
        zs::set_err("zs_mesh_weld_vertices: too large (n_tris=%d > 2^29)", n_tris);
        return 0;
    }
    if (n_verts > 3 * n_tris) {
        zs::set_err("zs_mesh_weld_vertices: bad vertex count (%d > 3 * %d corners)", n_verts, n_tris);
        return 0;
    }
    if (!tris || !scratch || !vertices) {
        zs::set_err("zs_mesh_weld_vertices: null pointer");
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("zs_mesh_weld_vertices: scratch must be 8-byte aligned");
        return 0;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int m = 3 * n_tris;
    const WeldScratch s = weld_scratch(m);
    const char *base = static_cast<const char *>(scratch);
    const int *run_start = reinterpret_cast<const int *>(base + s.a);
    const unsigned *perm = reinterpret_cast<const unsigned *>(base + s.f);
    const int *count = reinterpret_cast<const int *>(base + s.g) + scan_tiles(m);
    hipLaunchKernelGGL(weld_vertices_kernel, dim3((n_verts + MW_THREADS - 1) / MW_THREADS), dim3(MW_THREADS), 0, st, tris, m, perm,
                       run_start, count, n_verts, vertices, normals);
    return zs::check_launch("zs_mesh_weld_vertices") ? 1 : 0;
}
