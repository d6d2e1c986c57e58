// Uniform-grid vertex clustering with quadric-error placement (Rossignac-Borrel, Lindstrom; Open3D's
// simplify_vertex_clustering) over an indexed mesh (the vertices and faces of zs_mesh_weld): the device form of
// eval_3D.simplify_mesh_host, which defines the semantics.  The kernels equal it bit for bit.
//
// zs_mesh_simplify:
//   cell_keys_kernel            a thread per vertex: c = floor(((double)v - origin) / cell) per axis, key = cx << 42 | cy << 21 | cz.
//                               A coordinate that is not finite or a c outside [0, 2^21) sets status bit 1 and gives c = 0
//   rocprim::radix_sort_pairs   (key, vertex index), stable: a cluster's members sit in ascending vertex index
//   cluster_heads_kernel, scan  head = a key that differs from the one before it; inclusive scan: cluster id + 1
//   cluster_assign_kernel       cluster_of[vertex], the first sorted position of every cluster
//   cluster_mean_kernel         a thread per cluster walks its members: s = 0; s = s + ((double)v - centre) in ascending vertex
//                               index, centre = origin + ((double)c + 0.5) * cell; m = s / (double)count
//   incidence_keys_kernel       (quadric placement) a thread per (face, corner): key = cluster << bits | (3 face + corner)
//   rocprim::radix_sort_keys    cluster after cluster, each cluster's incidences ascending
//   place_kernel                a thread per cluster: the fp64 plane quadrics n n^T / |n| of its incidences' faces, each built
//                               from the face's three fp32 vertices in the cluster's local coordinates, summed in ascending key
//                               order; (A + w I) x = w m - b by Cramer's rule, w = MSIMP_RHO trace(A) / 3; the mean when the trace
//                               is not positive, x is not finite or some |x| exceeds the cell; a cluster of one vertex keeps that
//                               vertex's bits.  representative = (float)(centre + x)
//   face_keys_kernel            corners -> cluster ids; two equal ids: degenerate, dropped; else the ids rotated smallest first
//                               (the orientation stays) packed into one 63-bit key
//   rocprim::radix_sort_pairs   (key, face index), stable: equal triples in input face order
//   face_heads_kernel           the first face of every triple is kept, the others are duplicates; flags scattered back to
//                               face order, inclusive scan: the output slot + 1
//   emit_kernel                 out_tris[slot][k] = representative[cluster_of[faces[f][k]]]: the input's corner order
// Every sum is walked by one thread in a fixed order (the order of the additions is the contract; built with
// -ffp-contract=off), the counters are integer atomics: two runs give the same bytes.
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_TRIS = 1 << 28;          // 3 n incidences stay below 2^31
constexpr int SP_MAX_VERTS = 1 << 21;         // three cluster ids share one 63-bit key
constexpr int SP_CELL_BITS = 21;
constexpr double SP_CELL_LIMIT = 2097152.0;   // 2^21 cells per axis
// The weight of the pull towards the cluster mean relative to the mean eigenvalue of A: a design choice, not a measurement
// (eval_3D.SIMPLIFY_RHO is the same number).
constexpr double MSIMP_RHO = 1e-3;
enum { STATUS_CELL = 1, STATUS_INDEX = 2 };
enum { OUT_KEPT = 0, OUT_CLUSTERS = 1, OUT_DEGENERATE = 2, OUT_DUPLICATE = 3, OUT_STATUS = 4, OUT_FALLBACKS = 5, OUT_WORDS = 6 };
enum { MODE_MEAN = 0, MODE_QUADRIC = 1 };

typedef unsigned long long u64;

// ---- clusters ----

__global__ __launch_bounds__(SP_THREADS) void cell_keys_kernel(const float *__restrict__ vertices, int n_verts,
                                                               const double *__restrict__ origin, double cell,
                                                               u64 *__restrict__ keys, int *__restrict__ index, int *out) {
    const int v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= n_verts) return;
    u64 c[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double t = floor(((double)vertices[(size_t)v * 3 + a] - origin[a]) / cell);
        ok = ok && t >= 0.0 && t < SP_CELL_LIMIT;                    // (false for NaN)
        c[a] = ok ? (u64)t : 0;
    }
    if (!ok) {
        atomicOr(out + OUT_STATUS, STATUS_CELL);
        c[0] = c[1] = c[2] = 0;
    }
    keys[v] = (c[0] << (2 * SP_CELL_BITS)) | (c[1] << SP_CELL_BITS) | c[2];
    index[v] = v;
}

__global__ __launch_bounds__(SP_THREADS) void cluster_heads_kernel(const u64 *__restrict__ keys, int n_verts, int *__restrict__ pos) {
    const int j = blockIdx.x * SP_THREADS + threadIdx.x;
    if (j >= n_verts) return;
    pos[j] = j == 0 || keys[j - 1] != keys[j];
}

// pos: the inclusive scan of the head flags
__global__ __launch_bounds__(SP_THREADS) void cluster_assign_kernel(const int *__restrict__ index, const int *__restrict__ pos,
                                                                    int n_verts, int *__restrict__ cluster_of,
                                                                    int *__restrict__ start) {
    const int j = blockIdx.x * SP_THREADS + threadIdx.x;
    if (j >= n_verts) return;
    const int id = pos[j] - 1, v = index[j];
    if ((unsigned)id >= (unsigned)n_verts || (unsigned)v >= (unsigned)n_verts) return;       // (cannot happen)
    cluster_of[v] = id;
    if (j == 0 || pos[j - 1] != pos[j]) start[id] = j;
    if (j == n_verts - 1) start[id + 1] = n_verts;
}

__device__ __forceinline__ void cell_centre(u64 key, const double *__restrict__ origin, double cell, double centre[3]) {
    const u64 mask = (1ull << SP_CELL_BITS) - 1;
    const u64 c[3] = {key >> (2 * SP_CELL_BITS), (key >> SP_CELL_BITS) & mask, key & mask};
#pragma unroll
    for (int a = 0; a < 3; a++) centre[a] = origin[a] + ((double)c[a] + 0.5) * cell;
}

__global__ __launch_bounds__(SP_THREADS) void cluster_mean_kernel(const float *__restrict__ vertices, int n_verts,
                                                                  const double *__restrict__ origin, double cell,
                                                                  const u64 *__restrict__ keys, const int *__restrict__ index,
                                                                  const int *__restrict__ pos, const int *__restrict__ start,
                                                                  double *__restrict__ mean) {
    const int id = blockIdx.x * SP_THREADS + threadIdx.x;
    if (id >= n_verts || id >= pos[n_verts - 1]) return;
    const int begin = start[id], end = start[id + 1];
    if (begin < 0 || end <= begin || end > n_verts) return;          // (cannot happen)
    double centre[3];
    cell_centre(keys[begin], origin, cell, centre);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = begin; j < end; j++) {
        const int v = index[j];
        if ((unsigned)v >= (unsigned)n_verts) continue;              // (cannot happen)
        s0 = s0 + ((double)vertices[(size_t)v * 3] - centre[0]);
        s1 = s1 + ((double)vertices[(size_t)v * 3 + 1] - centre[1]);
        s2 = s2 + ((double)vertices[(size_t)v * 3 + 2] - centre[2]);
    }
    const double d = (double)(end - begin);
    mean[(size_t)id * 3] = s0 / d;
    mean[(size_t)id * 3 + 1] = s1 / d;
    mean[(size_t)id * 3 + 2] = s2 / d;
}

// ---- quadrics and placement ----

__global__ __launch_bounds__(SP_THREADS) void incidence_keys_kernel(const int *__restrict__ faces, int m, int n_verts,
                                                                    const int *__restrict__ cluster_of, int bits,
                                                                    u64 *__restrict__ keys, int *out) {
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;             // 3 face + corner
    if (i >= m) return;
    const int v = faces[i];
    u64 key = (u64)(unsigned)n_verts << bits;                        // past every cluster
    if ((unsigned)v < (unsigned)n_verts) key = ((u64)(unsigned)cluster_of[v] << bits) | (u64)(unsigned)i;
    else atomicOr(out + OUT_STATUS, STATUS_INDEX);
    keys[i] = key;
}

__global__ __launch_bounds__(SP_THREADS) void place_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                           int m, int n_verts, const double *__restrict__ origin, double cell,
                                                           int mode, const u64 *__restrict__ vkeys, const int *__restrict__ index,
                                                           const int *__restrict__ pos, const int *__restrict__ start,
                                                           const double *__restrict__ mean, const u64 *__restrict__ ikeys,
                                                           int bits, float *__restrict__ rep, int *out) {
    const int id = blockIdx.x * SP_THREADS + threadIdx.x;
    if (id >= n_verts || id >= pos[n_verts - 1]) return;
    const int begin = start[id], end = start[id + 1];
    if (begin < 0 || end <= begin || end > n_verts) return;          // (cannot happen)
    float *r = rep + (size_t)id * 3;
    if (end - begin == 1) {                                          // one member: its own bits
        const int v = index[begin];
        const bool ok = (unsigned)v < (unsigned)n_verts;
        for (int a = 0; a < 3; a++) r[a] = ok ? vertices[(size_t)v * 3 + a] : NAN;
        return;
    }
    double centre[3];
    cell_centre(vkeys[begin], origin, cell, centre);
    const double m0 = mean[(size_t)id * 3], m1 = mean[(size_t)id * 3 + 1], m2 = mean[(size_t)id * 3 + 2];
    double x0 = m0, x1 = m1, x2 = m2;
    if (mode == MODE_QUADRIC) {
        const u64 want = (u64)(unsigned)id << bits;
        int lo = 0, hi = m;                                          // the first incidence whose key is >= want
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (ikeys[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int j = lo; j < m; j++) {
            const u64 key = ikeys[j];
            if ((key >> bits) != (u64)(unsigned)id) break;
            const int i = (int)(unsigned)(key & ((1ull << bits) - 1));
            if ((unsigned)i >= (unsigned)m) break;                   // (cannot happen)
            const int *face = faces + (size_t)(i / 3) * 3;
            const int f0 = face[0], f1 = face[1], f2 = face[2];
            if ((unsigned)f0 >= (unsigned)n_verts || (unsigned)f1 >= (unsigned)n_verts || (unsigned)f2 >= (unsigned)n_verts)
                continue;                                            // a rejected face adds nothing
            const float *p = vertices + (size_t)f0 * 3, *q = vertices + (size_t)f1 * 3, *s = vertices + (size_t)f2 * 3;
            const double p0 = (double)p[0] - centre[0], p1 = (double)p[1] - centre[1], p2 = (double)p[2] - centre[2];
            const double q0 = (double)q[0] - centre[0], q1 = (double)q[1] - centre[1], q2 = (double)q[2] - centre[2];
            const double s0 = (double)s[0] - centre[0], s1 = (double)s[1] - centre[1], s2 = (double)s[2] - centre[2];
            const double u0 = q0 - p0, u1 = q1 - p1, u2 = q2 - p2, w0 = s0 - p0, w1 = s1 - p1, w2 = s2 - p2;
            const double n0 = u1 * w2 - u2 * w1, n1 = u2 * w0 - u0 * w2, n2 = u0 * w1 - u1 * w0;
            const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            if (!(len > 0.0 && len < INFINITY)) continue;            // a face without a normal adds nothing
            const double d = -((n0 * p0 + n1 * p1) + n2 * p2);
            a00 = a00 + (n0 * n0) / len;
            a01 = a01 + (n0 * n1) / len;
            a02 = a02 + (n0 * n2) / len;
            a11 = a11 + (n1 * n1) / len;
            a12 = a12 + (n1 * n2) / len;
            a22 = a22 + (n2 * n2) / len;
            b0 = b0 + (n0 * d) / len;
            b1 = b1 + (n1 * d) / len;
            b2 = b2 + (n2 * d) / len;
        }
        const double trace = (a00 + a11) + a22;
        bool ok = trace > 0.0;
        if (ok) {
            const double w = (MSIMP_RHO * trace) / 3.0;
            const double M00 = a00 + w, M11 = a11 + w, M22 = a22 + w, M01 = a01, M02 = a02, M12 = a12;
            const double r0 = w * m0 - b0, r1 = w * m1 - b1, r2 = w * m2 - b2;
            const double C00 = M11 * M22 - M12 * M12, C01 = M02 * M12 - M01 * M22, C02 = M01 * M12 - M02 * M11;
            const double C11 = M00 * M22 - M02 * M02, C12 = M01 * M02 - M00 * M12, C22 = M00 * M11 - M01 * M01;
            const double det = (M00 * C00 + M01 * C01) + M02 * C02;
            const double y0 = ((C00 * r0 + C01 * r1) + C02 * r2) / det;
            const double y1 = ((C01 * r0 + C11 * r1) + C12 * r2) / det;
            const double y2 = ((C02 * r0 + C12 * r1) + C22 * r2) / det;
            ok = fabs(y0) <= cell && fabs(y1) <= cell && fabs(y2) <= cell;                   // (false for NaN)
            if (ok) {
                x0 = y0;
                x1 = y1;
                x2 = y2;
            }
        }
        if (!ok) atomicAdd(out + OUT_FALLBACKS, 1);
    }
    r[0] = (float)(centre[0] + x0);
    r[1] = (float)(centre[1] + x1);
    r[2] = (float)(centre[2] + x2);
}

// ---- faces ----

__global__ __launch_bounds__(SP_THREADS) void face_keys_kernel(const int *__restrict__ faces, int n_tris, int n_verts,
                                                               const int *__restrict__ cluster_of, u64 *__restrict__ keys,
                                                               int *__restrict__ index, int *out) {
    const int f = blockIdx.x * SP_THREADS + threadIdx.x;
    if (f >= n_tris) return;
    const int *face = faces + (size_t)f * 3;
    const int f0 = face[0], f1 = face[1], f2 = face[2];
    u64 key = ~0ull;                                                 // a dropped face: past every triple
    if ((unsigned)f0 < (unsigned)n_verts && (unsigned)f1 < (unsigned)n_verts && (unsigned)f2 < (unsigned)n_verts) {
        const u64 a = (unsigned)cluster_of[f0], b = (unsigned)cluster_of[f1], c = (unsigned)cluster_of[f2];
        if (a == b || b == c || a == c) {
            atomicAdd(out + OUT_DEGENERATE, 1);
        } else {                                                     // the smallest id first, the cyclic order kept
            const u64 x = a < b && a < c ? a : b < c ? b : c;
            const u64 y = x == a ? b : x == b ? c : a, z = x == a ? c : x == b ? a : b;
            key = (x << (2 * SP_CELL_BITS)) | (y << SP_CELL_BITS) | z;
        }
    } else {
        atomicOr(out + OUT_STATUS, STATUS_INDEX);
        atomicAdd(out + OUT_DEGENERATE, 1);                          // a rejected face is dropped with the degenerate ones
    }
    keys[f] = key;
    index[f] = f;
}

__global__ __launch_bounds__(SP_THREADS) void face_heads_kernel(const u64 *__restrict__ keys, const int *__restrict__ index,
                                                                int n_tris, int *__restrict__ keep, int *out) {
    const int j = blockIdx.x * SP_THREADS + threadIdx.x;
    if (j >= n_tris) return;
    const int f = index[j];
    if ((unsigned)f >= (unsigned)n_tris) return;                     // (cannot happen)
    const u64 key = keys[j];
    const bool real = key != ~0ull, head = real && (j == 0 || keys[j - 1] != key);
    keep[f] = head;
    if (real && !head) atomicAdd(out + OUT_DUPLICATE, 1);
}

// pos: the inclusive scan of the keep flags, in face order
__global__ __launch_bounds__(SP_THREADS) void emit_kernel(const int *__restrict__ faces, int m, int n_verts,
                                                          const int *__restrict__ cluster_of, const int *__restrict__ pos,
                                                          const float *__restrict__ rep, float *__restrict__ out_tris) {
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;             // 3 face + corner
    if (i >= m) return;
    const int f = i / 3, k = i - 3 * f;
    const int p = pos[f], before = f ? pos[f - 1] : 0;
    if (p != before + 1 || p < 1 || p > m / 3) return;               // not kept
    const int v = faces[i];
    if ((unsigned)v >= (unsigned)n_verts) return;                    // (a kept face has its three indices in range)
    const float *r = rep + (size_t)cluster_of[v] * 3;
    float *o = out_tris + ((size_t)(p - 1) * 3 + k) * 3;
    o[0] = r[0];
    o[1] = r[1];
    o[2] = r[2];
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int width_of(unsigned n) {                                           // n itself must fit: it marks the keys past every real one
    int bits = 1;
    while (bits < 32 && (n >> bits)) bits++;
    return bits;
}

size_t sort_temp_bytes(int n_tris, int n_verts) {
    size_t pairs_v = 0, keys_i = 0, pairs_f = 0;
    u64 *k = nullptr;
    int *v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, pairs_v, k, k, v, v, (size_t)n_verts, 0u, 3u * SP_CELL_BITS);
    (void)rocprim::radix_sort_keys(nullptr, keys_i, k, k, (size_t)3 * n_tris, 0u,
                                   (unsigned)(width_of(3u * (unsigned)n_tris) + width_of((unsigned)n_verts)));
    (void)rocprim::radix_sort_pairs(nullptr, pairs_f, k, k, v, v, (size_t)n_tris, 0u, 64u);
    const size_t a = pairs_v > keys_i ? pairs_v : keys_i;
    return a > pairs_f ? a : pairs_f;
}

// vertex keys in | out | vertex indices in | out | head flags -> cluster ids + 1 | tile totals | cluster_of | cluster starts |
// means (fp64) | representatives | incidence keys in | out | face keys in | out | face indices in | out | keep flags -> slots |
// tile totals | the sorts' workspace
struct SimplifyScratch {
    size_t vkeys_in, vkeys_out, vidx_in, vidx_out, vpos, vtiles, cluster_of, start, mean, rep, ikeys_in, ikeys_out, fkeys_in,
        fkeys_out, fidx_in, fidx_out, fpos, ftiles, temp, total;
};
SimplifyScratch simplify_scratch(int n_tris, int n_verts) {
    const size_t V = (size_t)n_verts, F = (size_t)n_tris;
    SimplifyScratch s;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    };
    s.vkeys_in = take(V * 8);
    s.vkeys_out = take(V * 8);
    s.vidx_in = take(V * 4);
    s.vidx_out = take(V * 4);
    s.vpos = take(V * 4);
    s.vtiles = take(((size_t)scan_tiles((long long)V) + 1) * 4);
    s.cluster_of = take(V * 4);
    s.start = take((V + 1) * 4);
    s.mean = take(V * 3 * 8);
    s.rep = take(V * 3 * 4);
    s.ikeys_in = take(F * 3 * 8);
    s.ikeys_out = take(F * 3 * 8);
    s.fkeys_in = take(F * 8);
    s.fkeys_out = take(F * 8);
    s.fidx_in = take(F * 4);
    s.fidx_out = take(F * 4);
    s.fpos = take(F * 4);
    s.ftiles = take(((size_t)scan_tiles((long long)F) + 1) * 4);
    s.temp = take(sort_temp_bytes(n_tris, n_verts));
    s.total = at;
    return s;
}

bool sizes_in_limits(int n_tris, int n_verts) {
    return n_tris >= 0 && n_verts >= 0 && n_tris <= SP_MAX_TRIS && n_verts <= SP_MAX_VERTS && (long long)n_verts <= 3ll * n_tris;
}

dim3 grid_for(long long n) { return dim3((unsigned)((n + SP_THREADS - 1) / SP_THREADS)); }

}  // namespace

extern "C" size_t zs_mesh_simplify_scratch_bytes(int n_tris, int n_verts) {
    if (n_tris <= 0 || n_verts <= 0 || !sizes_in_limits(n_tris, n_verts)) return 0;
    return simplify_scratch(n_tris, n_verts).total;
}

extern "C" int zs_mesh_simplify(const float *vertices, const int *faces, int n_tris, int n_verts, const double *origin, double cell,
                                int mode, float *out_tris, int *out_counts, void *scratch, void *stream) {
    const char *who = "zs_mesh_simplify";
    if (n_tris < 0 || n_verts < 0) {
        zs::set_err("%s: negative size (n_tris=%d n_verts=%d)", who, n_tris, n_verts);
        return 0;
    }
    if (n_tris > SP_MAX_TRIS || n_verts > SP_MAX_VERTS) {
        zs::set_err("%s: too large (n_tris=%d > 2^28 or n_verts=%d > 2^21)", who, n_tris, n_verts);
        return 0;
    }
    if ((long long)n_verts > 3ll * n_tris) {
        zs::set_err("%s: bad vertex count (%d > 3 * %d corners)", who, n_verts, n_tris);
        return 0;
    }
    if (!(cell > 0.0 && cell < INFINITY)) {
        zs::set_err("%s: cell must be finite and positive, got %g", who, cell);
        return 0;
    }
    if (mode != MODE_MEAN && mode != MODE_QUADRIC) {
        zs::set_err("%s: mode must be 0 (mean) or 1 (quadric), got %d", who, mode);
        return 0;
    }
    if (n_tris == 0 || n_verts == 0) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!vertices || !faces || !origin || !out_tris || !out_counts || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("%s: scratch must be 8-byte aligned", who);
        return 0;
    }
    const SimplifyScratch s = simplify_scratch(n_tris, n_verts);
    char *base = static_cast<char *>(scratch);
    u64 *vkeys_in = reinterpret_cast<u64 *>(base + s.vkeys_in), *vkeys = reinterpret_cast<u64 *>(base + s.vkeys_out);
    int *vidx_in = reinterpret_cast<int *>(base + s.vidx_in), *vidx = reinterpret_cast<int *>(base + s.vidx_out);
    int *vpos = reinterpret_cast<int *>(base + s.vpos), *vtiles = reinterpret_cast<int *>(base + s.vtiles);
    int *cluster_of = reinterpret_cast<int *>(base + s.cluster_of), *start = reinterpret_cast<int *>(base + s.start);
    double *mean = reinterpret_cast<double *>(base + s.mean);
    float *rep = reinterpret_cast<float *>(base + s.rep);
    u64 *ikeys_in = reinterpret_cast<u64 *>(base + s.ikeys_in), *ikeys = reinterpret_cast<u64 *>(base + s.ikeys_out);
    u64 *fkeys_in = reinterpret_cast<u64 *>(base + s.fkeys_in), *fkeys = reinterpret_cast<u64 *>(base + s.fkeys_out);
    int *fidx_in = reinterpret_cast<int *>(base + s.fidx_in), *fidx = reinterpret_cast<int *>(base + s.fidx_out);
    int *fpos = reinterpret_cast<int *>(base + s.fpos), *ftiles = reinterpret_cast<int *>(base + s.ftiles);
    void *temp = base + s.temp;
    size_t temp_bytes = s.total - s.temp;
    const int m = 3 * n_tris, bits = width_of((unsigned)m), cluster_bits = width_of((unsigned)n_verts);
    const int vt = scan_tiles(n_verts), ft = scan_tiles(n_tris);
    const dim3 block(SP_THREADS);

    if (hipMemsetAsync(out_counts, 0, OUT_WORDS * sizeof(int), st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    // clusters
    hipLaunchKernelGGL(cell_keys_kernel, grid_for(n_verts), block, 0, st, vertices, n_verts, origin, cell, vkeys_in, vidx_in,
                       out_counts);
    if (rocprim::radix_sort_pairs(temp, temp_bytes, vkeys_in, vkeys, vidx_in, vidx, (size_t)n_verts, 0u, 3u * SP_CELL_BITS, st) !=
        hipSuccess) {
        zs::set_err("%s: rocprim::radix_sort_pairs failed", who);
        return 0;
    }
    hipLaunchKernelGGL(cluster_heads_kernel, grid_for(n_verts), block, 0, st, static_cast<const u64 *>(vkeys), n_verts, vpos);
    hipLaunchKernelGGL((scan_tiles_kernel<int, true>), dim3(vt), dim3(256), 0, st, vpos, (long long)n_verts, vtiles);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(vt), dim3(256), 0, st, vpos, (long long)n_verts,
                       static_cast<const int *>(vtiles), vt, out_counts + OUT_CLUSTERS);
    hipLaunchKernelGGL(cluster_assign_kernel, grid_for(n_verts), block, 0, st, static_cast<const int *>(vidx),
                       static_cast<const int *>(vpos), n_verts, cluster_of, start);
    hipLaunchKernelGGL(cluster_mean_kernel, grid_for(n_verts), block, 0, st, vertices, n_verts, origin, cell,
                       static_cast<const u64 *>(vkeys), static_cast<const int *>(vidx), static_cast<const int *>(vpos),
                       static_cast<const int *>(start), mean);
    // quadrics and placement
    if (mode == MODE_QUADRIC) {
        hipLaunchKernelGGL(incidence_keys_kernel, grid_for(m), block, 0, st, faces, m, n_verts, static_cast<const int *>(cluster_of),
                           bits, ikeys_in, out_counts);
        temp_bytes = s.total - s.temp;
        if (rocprim::radix_sort_keys(temp, temp_bytes, ikeys_in, ikeys, (size_t)m, 0u, (unsigned)(bits + cluster_bits), st) !=
            hipSuccess) {
            zs::set_err("%s: rocprim::radix_sort_keys failed", who);
            return 0;
        }
    }
    hipLaunchKernelGGL(place_kernel, grid_for(n_verts), block, 0, st, vertices, faces, m, n_verts, origin, cell, mode,
                       static_cast<const u64 *>(vkeys), static_cast<const int *>(vidx), static_cast<const int *>(vpos),
                       static_cast<const int *>(start), static_cast<const double *>(mean), static_cast<const u64 *>(ikeys), bits, rep,
                       out_counts);
    // faces
    hipLaunchKernelGGL(face_keys_kernel, grid_for(n_tris), block, 0, st, faces, n_tris, n_verts,
                       static_cast<const int *>(cluster_of), fkeys_in, fidx_in, out_counts);
    temp_bytes = s.total - s.temp;
    if (rocprim::radix_sort_pairs(temp, temp_bytes, fkeys_in, fkeys, fidx_in, fidx, (size_t)n_tris, 0u, 64u, st) != hipSuccess) {
        zs::set_err("%s: rocprim::radix_sort_pairs failed", who);
        return 0;
    }
    hipLaunchKernelGGL(face_heads_kernel, grid_for(n_tris), block, 0, st, static_cast<const u64 *>(fkeys),
                       static_cast<const int *>(fidx), n_tris, fpos, out_counts);
    hipLaunchKernelGGL((scan_tiles_kernel<int, true>), dim3(ft), dim3(256), 0, st, fpos, (long long)n_tris, ftiles);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(ft), dim3(256), 0, st, fpos, (long long)n_tris,
                       static_cast<const int *>(ftiles), ft, out_counts + OUT_KEPT);
    hipLaunchKernelGGL(emit_kernel, grid_for(m), block, 0, st, faces, m, n_verts, static_cast<const int *>(cluster_of),
                       static_cast<const int *>(fpos), static_cast<const float *>(rep), out_tris);
    return zs::check_launch(who) ? 1 : 0;
}
