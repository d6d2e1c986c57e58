// The vertex neighbourhood of an indexed mesh (the faces of zs_mesh_weld) as a CSR, the boundary flags of its vertices, and
// Laplacian / Taubin smoothing over it: the device form of eval_3D.mesh_adjacency_host and eval_3D.smooth_vertices_host, which
// define the semantics.  The kernels equal them bit for bit.
//
// zs_mesh_adjacency (integers only: every output is a pure function of the faces):
//   adj_keys_kernel             a thread per face edge: the two directed entries a -> b and b -> a as 64-bit keys
//                               source << bits | target, bits = the width of n_verts.  A face with two equal indices, or with
//                               an index outside [0, n_verts) (status word |= 2; the index is tested before it is used for
//                               anything), gets keys past every real one: n_verts << bits
//   rocprim::radix_sort_keys    2 * bits key bits: row after row, each row ascending, every use of an undirected edge one
//                               entry in the rows of both of its endpoints
//   adj_heads_kernel            head = a real key that differs from the one before it.  A head whose successor differs too
//                               is an edge used exactly once: boundary[source] = 1 (every writer writes the same byte)
//   scan_tiles_kernel / scan_offsets_kernel (zs_scan.h)   inclusive over the head flags: head -> 1 + its slot in neighbors
//   adj_emit_kernel             neighbors[slot] = target of every head
//   adj_offsets_kernel          a thread per v in [0, n_verts]: a binary search for the first key >= v << bits; offsets[v] =
//                               the number of heads before it (vertices without edges included); out = nnz, status
// zs_mesh_smooth:
//   smooth_pass_kernel          a thread per vertex, one launch per pass (the dependency between passes is the launch
//                               boundary): s = 0; s = s + x[neighbour] along the row in row order; m = s / degree;
//                               x' = x + f * (m - x), fp64 operations as written (built with -ffp-contract=off).  The order of
//                               the additions is the contract, so a row is never split over lanes.  The first pass reads
//                               the fp32 input (widened on the way in), the last one rounds to fp32 on the way out, the
//                               passes between them alternate between two fp64 buffers in scratch.
// zs_mesh_gather_faces:         out_tris[f][k] = vertices[faces[f][k]]
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_MAX_TRIS = 1 << 28;        // 6 n directed entries stay below 2^31 (offsets and nnz are int32)
enum { STATUS_ROW = 1, STATUS_INDEX = 2 };

typedef unsigned long long u64;

// ---- adjacency ----

__global__ __launch_bounds__(MS_THREADS) void adj_keys_kernel(const int *__restrict__ faces, int m, int n_verts, int bits,
                                                              u64 *__restrict__ keys, int *status) {
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= m) return;
    const int f = i / 3, k = i - 3 * f;
    const int *face = faces + (size_t)f * 3;
    const int f0 = face[0], f1 = face[1], f2 = face[2];
    const bool in_range = (unsigned)f0 < (unsigned)n_verts && (unsigned)f1 < (unsigned)n_verts && (unsigned)f2 < (unsigned)n_verts;
    if (!in_range && k == 0) atomicOr(status, STATUS_INDEX);
    const u64 none = (u64)(unsigned)n_verts << bits;                 // a degenerate or rejected face has no edges
    u64 ab = none, ba = none;
    if (in_range && f0 != f1 && f1 != f2 && f0 != f2) {
        const u64 a = (unsigned)(k == 0 ? f0 : k == 1 ? f1 : f2), b = (unsigned)(k == 0 ? f1 : k == 1 ? f2 : f0);
        ab = (a << bits) | b;
        ba = (b << bits) | a;
    }
    keys[(size_t)i * 2] = ab;
    keys[(size_t)i * 2 + 1] = ba;
}

__global__ __launch_bounds__(MS_THREADS) void adj_heads_kernel(const u64 *__restrict__ keys, int n_keys, int n_verts, int bits,
                                                               int *__restrict__ heads, unsigned char *boundary) {
    const int j = blockIdx.x * MS_THREADS + threadIdx.x;
    if (j >= n_keys) return;
    const u64 key = keys[j];
    const unsigned src = (unsigned)(key >> bits);
    const bool head = src < (unsigned)n_verts && (j == 0 || keys[j - 1] != key);
    heads[j] = head;
    if (head && (j + 1 == n_keys || keys[j + 1] != key)) boundary[src] = 1;
}

__global__ __launch_bounds__(MS_THREADS) void adj_emit_kernel(const u64 *__restrict__ keys, const int *__restrict__ pos, int n_keys,
                                                              int n_verts, int bits, int *__restrict__ neighbors) {
    const int j = blockIdx.x * MS_THREADS + threadIdx.x;
    if (j >= n_keys) return;
    const int p = pos[j], before = j ? pos[j - 1] : 0;
    if (p == before + 1 && p >= 1 && p <= n_keys) neighbors[p - 1] = (int)(unsigned)(keys[j] & ((1ull << bits) - 1));
}

__global__ __launch_bounds__(MS_THREADS) void adj_offsets_kernel(const u64 *__restrict__ keys, const int *__restrict__ pos,
                                                                 int n_keys, int n_verts, int bits, int *__restrict__ offsets,
                                                                 int *__restrict__ out) {
    const int v = blockIdx.x * MS_THREADS + threadIdx.x;
    if (v > n_verts) return;
    const u64 want = (u64)(unsigned)v << bits;
    int lo = 0, hi = n_keys;                                         // the first position whose key is >= want
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    const int before = lo ? pos[lo - 1] : 0;                         // the heads in front of it
    offsets[v] = before;
    if (v == n_verts) out[0] = before;                               // (out[1], the status word, is adj_keys_kernel's)
}

// ---- smoothing ----

template <typename TIn, typename TOut>
__global__ __launch_bounds__(MS_THREADS) void smooth_pass_kernel(const TIn *__restrict__ x, int n_verts,
                                                                 const int *__restrict__ offsets, const int *__restrict__ neighbors,
                                                                 const unsigned char *__restrict__ boundary, double f,
                                                                 TOut *__restrict__ y, int *status) {
    const int v = blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= n_verts) return;
    const double x0 = (double)x[(size_t)v * 3], x1 = (double)x[(size_t)v * 3 + 1], x2 = (double)x[(size_t)v * 3 + 2];
    double y0 = x0, y1 = x1, y2 = x2;
    const int begin = offsets[v], end = offsets[v + 1];
    const bool row_ok = begin >= 0 && end >= begin && end <= (neighbors ? offsets[n_verts] : 0);
    if (!row_ok) atomicOr(status, STATUS_ROW);
    if (row_ok && end > begin && !(boundary && boundary[v])) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        bool ok = true;
        for (int k = begin; k < end; k++) {
            const int n = neighbors[k];
            if ((unsigned)n >= (unsigned)n_verts) {                  // not followed: the vertex stays
                ok = false;
                break;
            }
            s0 = s0 + (double)x[(size_t)n * 3];
            s1 = s1 + (double)x[(size_t)n * 3 + 1];
            s2 = s2 + (double)x[(size_t)n * 3 + 2];
        }
        if (ok) {
            const double d = (double)(end - begin);
            const double m0 = s0 / d, m1 = s1 / d, m2 = s2 / d;
            y0 = x0 + f * (m0 - x0);
            y1 = x1 + f * (m1 - x1);
            y2 = x2 + f * (m2 - x2);
        } else {
            atomicOr(status, STATUS_INDEX);
        }
    }
    y[(size_t)v * 3] = (TOut)y0;
    y[(size_t)v * 3 + 1] = (TOut)y1;
    y[(size_t)v * 3 + 2] = (TOut)y2;
}

// ---- the soup of an indexed mesh ----

__global__ __launch_bounds__(MS_THREADS) void gather_faces_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                  int m, int n_verts, float *__restrict__ out) {
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;             // corner 3 f + k
    if (i >= m) return;
    const int v = faces[i];
    const bool ok = (unsigned)v < (unsigned)n_verts;
    const float *p = vertices + (size_t)(ok ? v : 0) * 3;
    out[(size_t)i * 3] = ok ? p[0] : NAN;
    out[(size_t)i * 3 + 1] = ok ? p[1] : NAN;
    out[(size_t)i * 3 + 2] = ok ? p[2] : NAN;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int key_bits(int n_verts) {                                          // n_verts itself must fit: it marks the keys of no edge
    int bits = 1;
    while (bits < 31 && ((unsigned)n_verts >> bits)) bits++;
    return bits;
}

size_t sort_temp_bytes(int n_keys, int bits) {
    size_t bytes = 0;
    u64 *k = nullptr;
    (void)rocprim::radix_sort_keys(nullptr, bytes, k, k, (size_t)n_keys, 0u, (unsigned)(2 * bits));
    return bytes;
}

// keys in | keys out (64-bit, 6 n) | head flags -> slots (6 n) | tile totals | the sort's workspace
struct AdjScratch {
    size_t keys_in, keys_out, pos, tiles, temp, total;
};
AdjScratch adj_scratch(int n_tris, int n_verts) {
    const size_t n_keys = (size_t)6 * n_tris;
    AdjScratch s;
    s.keys_in = 0;
    s.keys_out = s.keys_in + align256(n_keys * 8);
    s.pos = s.keys_out + align256(n_keys * 8);
    s.tiles = s.pos + align256(n_keys * 4);
    s.temp = s.tiles + align256(((size_t)scan_tiles((long long)n_keys) + 1) * 4);
    s.total = s.temp + align256(sort_temp_bytes((int)n_keys, key_bits(n_verts)));
    return s;
}

bool sizes_ok(const char *who, int n_tris, int n_verts) {
    if (n_tris < 0 || n_verts < 0) {
        zs::set_err("%s: negative size (n_tris=%d n_verts=%d)", who, n_tris, n_verts);
        return false;
    }
    if (n_tris > MS_MAX_TRIS) {
        zs::set_err("%s: too large (n_tris=%d > 2^28)", who, n_tris);
        return false;
    }
    if ((long long)n_verts > 3ll * n_tris) {
        zs::set_err("%s: bad vertex count (%d > 3 * %d corners)", who, n_verts, n_tris);
        return false;
    }
    return true;
}

bool scratch_ok(const char *who, const void *scratch) {
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("%s: scratch must be 8-byte aligned", who);
        return false;
    }
    return true;
}

dim3 grid_for(long long n) { return dim3((unsigned)((n + MS_THREADS - 1) / MS_THREADS)); }

template <typename TIn, typename TOut>
void launch_pass(hipStream_t st, const TIn *x, int n_verts, const int *offsets, const int *neighbors, const unsigned char *boundary,
                 double f, TOut *y, int *status) {
    hipLaunchKernelGGL((smooth_pass_kernel<TIn, TOut>), grid_for(n_verts), dim3(MS_THREADS), 0, st, x, n_verts, offsets, neighbors,
                       boundary, f, y, status);
}

}  // namespace

extern "C" size_t zs_mesh_adjacency_scratch_bytes(int n_tris, int n_verts) {
    if (n_tris <= 0 || n_verts <= 0 || n_tris > MS_MAX_TRIS || (long long)n_verts > 3ll * n_tris) return 0;
    return adj_scratch(n_tris, n_verts).total;
}

extern "C" int zs_mesh_adjacency(const int *faces, int n_tris, int n_verts, int *offsets, int *neighbors, uint8_t *boundary,
                                 int *out, void *scratch, void *stream) {
    const char *who = "zs_mesh_adjacency";
    if (!sizes_ok(who, n_tris, n_verts)) return 0;
    if (n_tris == 0 || n_verts == 0) return 1;
    if (!faces || !offsets || !neighbors || !boundary || !out || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (!scratch_ok(who, scratch)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const AdjScratch s = adj_scratch(n_tris, n_verts);
    char *base = static_cast<char *>(scratch);
    u64 *keys_in = reinterpret_cast<u64 *>(base + s.keys_in), *keys_out = reinterpret_cast<u64 *>(base + s.keys_out);
    int *pos = reinterpret_cast<int *>(base + s.pos), *tile_tot = reinterpret_cast<int *>(base + s.tiles);
    const int m = 3 * n_tris, n_keys = 6 * n_tris, bits = key_bits(n_verts), tiles = scan_tiles(n_keys);
    size_t temp_bytes = s.total - s.temp;
    const dim3 block(MS_THREADS);

    if (hipMemsetAsync(out, 0, 2 * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(boundary, 0, (size_t)n_verts, st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    hipLaunchKernelGGL(adj_keys_kernel, grid_for(m), block, 0, st, faces, m, n_verts, bits, keys_in, out + 1);
    if (rocprim::radix_sort_keys(base + s.temp, temp_bytes, keys_in, keys_out, (size_t)n_keys, 0u, (unsigned)(2 * bits), st) !=
        hipSuccess) {
        zs::set_err("%s: rocprim::radix_sort_keys failed", who);
        return 0;
    }
    const u64 *sorted = keys_out;
    hipLaunchKernelGGL(adj_heads_kernel, grid_for(n_keys), block, 0, st, sorted, n_keys, n_verts, bits, pos, boundary);
    hipLaunchKernelGGL((scan_tiles_kernel<int, true>), dim3(tiles), dim3(256), 0, st, pos, (long long)n_keys, tile_tot);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(tiles), dim3(256), 0, st, pos, (long long)n_keys,
                       static_cast<const int *>(tile_tot), tiles, static_cast<int *>(nullptr));
    hipLaunchKernelGGL(adj_emit_kernel, grid_for(n_keys), block, 0, st, sorted, static_cast<const int *>(pos), n_keys, n_verts, bits,
                       neighbors);
    hipLaunchKernelGGL(adj_offsets_kernel, grid_for((long long)n_verts + 1), block, 0, st, sorted, static_cast<const int *>(pos),
                       n_keys, n_verts, bits, offsets, out);
    return zs::check_launch(who) ? 1 : 0;
}

extern "C" size_t zs_mesh_smooth_scratch_bytes(int n_verts) {
    if (n_verts <= 0 || (long long)n_verts > 3ll * MS_MAX_TRIS) return 0;
    return 2 * align256((size_t)n_verts * 3 * sizeof(double));
}

extern "C" int zs_mesh_smooth(const float *vertices, int n_verts, const int *offsets, const int *neighbors, const uint8_t *boundary,
                              int passes, double lambda, double mu, int alternate, float *out_vertices, int *status, void *scratch,
                              void *stream) {
    const char *who = "zs_mesh_smooth";
    if (n_verts < 0 || passes < 0) {
        zs::set_err("%s: negative size (n_verts=%d passes=%d)", who, n_verts, passes);
        return 0;
    }
    if ((long long)n_verts > 3ll * MS_MAX_TRIS) {
        zs::set_err("%s: too large (n_verts=%d > 3 * 2^28)", who, n_verts);
        return 0;
    }
    if (!(lambda > 0.0 && lambda <= 1.0)) {
        zs::set_err("%s: lambda must lie in (0, 1], got %g", who, lambda);
        return 0;
    }
    if (alternate && !(mu >= -1.0 && mu < 0.0)) {
        zs::set_err("%s: mu must lie in [-1, 0), got %g", who, mu);
        return 0;
    }
    if (n_verts == 0) return 1;
    if (!vertices || !offsets || !out_vertices || !status || (passes > 1 && !scratch)) {    // (neighbors: NULL = no edges)
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (passes > 0 && out_vertices == vertices) {                    // (a pass reads what its neighbours' threads would write)
        zs::set_err("%s: out_vertices must not be the input", who);
        return 0;
    }
    if (!scratch_ok(who, scratch)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    if (passes == 0) {                                               // the input's bits
        if (out_vertices != vertices &&
            hipMemcpyAsync(out_vertices, vertices, (size_t)n_verts * 3 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            zs::set_err("%s: hipMemcpyAsync failed", who);
            return 0;
        }
        return 1;
    }
    double *buf[2] = {static_cast<double *>(scratch),
                      reinterpret_cast<double *>(static_cast<char *>(scratch) + align256((size_t)n_verts * 3 * sizeof(double)))};
    for (int t = 0; t < passes; t++) {
        const double f = alternate && (t & 1) ? mu : lambda;
        const bool first = t == 0, last = t == passes - 1;
        const double *src = buf[(t + 1) & 1];                        // pass t writes buf[t & 1]
        double *dst = buf[t & 1];
        if (first && last) launch_pass(st, vertices, n_verts, offsets, neighbors, boundary, f, out_vertices, status);
        else if (first) launch_pass(st, vertices, n_verts, offsets, neighbors, boundary, f, dst, status);
        else if (last) launch_pass(st, src, n_verts, offsets, neighbors, boundary, f, out_vertices, status);
        else launch_pass(st, src, n_verts, offsets, neighbors, boundary, f, dst, status);
    }
    return zs::check_launch(who) ? 1 : 0;
}

extern "C" int zs_mesh_gather_faces(const float *vertices, const int *faces, int n_tris, int n_verts, float *out_tris, void *stream) {
    const char *who = "zs_mesh_gather_faces";
    if (n_tris < 0 || n_verts < 0) {
        zs::set_err("%s: negative size (n_tris=%d n_verts=%d)", who, n_tris, n_verts);
        return 0;
    }
    if (n_tris > MS_MAX_TRIS) {
        zs::set_err("%s: too large (n_tris=%d > 2^28)", who, n_tris);
        return 0;
    }
    if (n_tris == 0) return 1;
    if (!faces || !out_tris || (n_verts && !vertices)) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    hipLaunchKernelGGL(gather_faces_kernel, grid_for(3ll * n_tris), dim3(MS_THREADS), 0, static_cast<hipStream_t>(stream), vertices,
                       faces, 3 * n_tris, n_verts, out_tris);
    return zs::check_launch(who) ? 1 : 0;
}
