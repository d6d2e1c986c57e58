// Connected components of an indexed mesh (the faces of zs_mesh_weld), their exact integer counts and fp64 measures, and the
// order-preserving removal of components from the soup: the device form of eval_3D.mesh_components_host, which defines the
// semantics.  Two vertices are connected when some face holds both; the label of a component is its rank among the
// components' smallest vertex indices.
//
// zs_mesh_components:
//   cc_init_kernel              parent[v] = v, status = 0
//   cc_link_kernel              a thread per face: union(f0, f1), union(f0, f2).  Lock-free union-find in the style of ECL-CC:
//                               the larger root is hooked under the smaller with a compare-and-swap, so a parent only ever
//                               decreases and the final root of a component is its smallest vertex, whatever order the
//                               workgroups run in.  EVERY access to parent[] in this kernel is a relaxed agent-scope atomic
//                               (load, compare-exchange, fetch-min for the path halving): a plain load may be served from
//                               another XCD's stale L2 line and bring an old, larger parent back - "parents only decrease"
//                               would break, and a cycle in the forest never ends.  No thread waits for another; every
//                               find / hook loop is bounded by n_verts + 2 iterations (a chain has at most n_verts links,
//                               and a failed hook means another thread's hook succeeded, of which there are fewer than
//                               n_verts); a thread that gets past the bound, or meets a face index outside [0, n_verts),
//                               sets the status word and leaves.
//   cc_flatten_kernel           a kernel of its own, after the linking has ended: root[v] by walking parent[] (read-only),
//                               is_root[v]
//   scan_tiles_kernel / scan_offsets_kernel (zs_scan.h)   inclusive over is_root: root r is component ids[r] - 1
//   cc_vertex_labels_kernel     vertex_labels[v] = ids[root[v]] - 1; out[0] = the count, out[1] = the status word
//   cc_face_labels_kernel       face_labels[f] = vertex_labels[faces[f][0]]
// zs_mesh_component_stats (after the caller has read the count and allocated the tables):
//   integer columns             integer atomics, one per wave and label (cs_wave_add): exact in any order
//     cs_vertex_count_kernel    vertices
//     cs_edge_keys_kernel       half-edge key = min << 32 | max, value = 1 when the half-edge runs min -> max; the three
//                               half-edges of a degenerate face (two equal indices) get a key past every real one
//     rocprim::radix_sort_pairs 64 bits
//     cs_edge_count_kernel      the head of a run of equal keys looks two positions ahead: used once = boundary, more than
//                               twice = non-manifold, twice with equal directions = misoriented
//   fp64 measures               no floating-point atomics: a stable sort of the face indices by label, then a fixed-shape
//                               segmented reduction - every output is a pure function of the input
//     cs_face_keys_kernel / rocprim::radix_sort_pairs (32 bits, stable): component c owns positions [begin[c], end[c])
//     cs_terms_kernel           a workgroup per 256 sorted positions: the face's area and signed-volume terms in fp64 as
//                               written in mesh_components_host (a degenerate face: exactly 0), a segmented Hillis-Steele
//                               scan in LDS; a component that begins and ends inside the chunk is finished here, the others
//                               leave one partial per chunk
//     cs_finish_kernel          a wave per component: the chunk partials, lane-strided in chunk order, then an xor
//                               butterfly; faces = end - begin; the Euler number
// zs_mesh_components_select:    one workgroup: the largest area, then keep[c] by the rule of eval_3D.filter_components;
//                               per-face flags; the scan of zs_scan.h; the count
// zs_mesh_filter_faces:         out[keep_pos[f] - 1] = tris[f] for the kept faces: soup order is preserved
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_MAX_TRIS = 1 << 29;        // 3 n half-edges stay below 2^31
constexpr int MC_COLS = 8;                  // faces, vertices, degenerate, edges, boundary, non-manifold, misoriented, euler
enum { COL_FACES, COL_VERTS, COL_DEGEN, COL_EDGES, COL_BOUNDARY, COL_NONMANIFOLD, COL_MISORIENTED, COL_EULER };
enum { STATUS_BOUND = 1, STATUS_INDEX = 2 };

// ---- linking ----

__device__ __forceinline__ int parent_load(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v at the time of the last read, or -1 past the bound.  Path halving: parent[v] <- min(parent[v], grandparent).
__device__ int cc_find(int *parent, int v, int bound, int *status) {
    int p = parent_load(parent + v);
    for (int it = 0; p != v; it++) {
        if (it >= bound) {
            atomicOr(status, STATUS_BOUND);
            return -1;
        }
        const int gp = parent_load(parent + p);
        if (gp != p) __hip_atomic_fetch_min(parent + v, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = p;
        p = gp;
    }
    return v;
}

__device__ void cc_union(int *parent, int a, int b, int bound, int *status) {
    for (int it = 0; it < bound; it++) {
        a = cc_find(parent, a, bound, status);
        b = cc_find(parent, b, bound, status);
        if (a < 0 || b < 0 || a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int expected = hi;                      // still a root: hook it under the smaller one
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = hi;                                 // somebody else hooked hi first: find again from there
        b = lo;
    }
    atomicOr(status, STATUS_BOUND);
}

__global__ __launch_bounds__(MC_THREADS) void cc_init_kernel(int *__restrict__ parent, int n_verts, int *__restrict__ status) {
    const int v = blockIdx.x * MC_THREADS + threadIdx.x;
    if (v == 0) *status = 0;
    if (v < n_verts) parent[v] = v;
}

__global__ __launch_bounds__(MC_THREADS) void cc_link_kernel(const int *__restrict__ faces, int n_tris, int n_verts, int *parent,
                                                             int *status) {
    const int f = blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= n_tris) return;
    const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
    if ((unsigned)a >= (unsigned)n_verts || (unsigned)b >= (unsigned)n_verts || (unsigned)c >= (unsigned)n_verts) {
        atomicOr(status, STATUS_INDEX);
        return;
    }
    const int bound = n_verts + 2;
    if (a != b) cc_union(parent, a, b, bound, status);
    if (a != c) cc_union(parent, a, c, bound, status);
}

__global__ __launch_bounds__(MC_THREADS) void cc_flatten_kernel(const int *__restrict__ parent, int n_verts, int *__restrict__ root,
                                                                int *__restrict__ is_root, int *__restrict__ status) {
    const int v = blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= n_verts) return;
    int r = v, p = parent[v];
    for (int it = 0; p != r; it++) {
        if (it >= n_verts + 2 || (unsigned)p >= (unsigned)n_verts) {
            atomicOr(status, STATUS_BOUND);
            break;
        }
        r = p;
        p = parent[r];
    }
    root[v] = r;
    is_root[v] = parent[v] == v;
}

__global__ __launch_bounds__(MC_THREADS) void cc_vertex_labels_kernel(const int *__restrict__ root, const int *__restrict__ ids,
                                                                      int n_verts, const int *__restrict__ status,
                                                                      int *__restrict__ vertex_labels, int *__restrict__ out) {
    const int v = blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= n_verts) return;
    const int r = root[v];
    vertex_labels[v] = ((unsigned)r < (unsigned)n_verts ? ids[r] : 0) - 1;
    if (v == n_verts - 1) {
        out[0] = ids[v];
        out[1] = *status;
    }
}

__global__ __launch_bounds__(MC_THREADS) void cc_face_labels_kernel(const int *__restrict__ faces, int n_tris, int n_verts,
                                                                    const int *__restrict__ vertex_labels,
                                                                    int *__restrict__ face_labels) {
    const int f = blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= n_tris) return;
    const int a = faces[(size_t)f * 3];
    face_labels[f] = (unsigned)a < (unsigned)n_verts ? vertex_labels[a] : -1;
}

// ---- integer columns ----

// counts[label][cols[k]] += the number of lanes of this wave with that label and flags[k]: one atomic per wave, label and
// column.  Every lane of the wave must call it (lanes with nothing to add pass valid = false).
template <int N>
__device__ __forceinline__ void cs_wave_add(int *counts, int n_comps, bool valid, int label, const int (&cols)[N],
                                            const bool (&flags)[N]) {
    const int lane = threadIdx.x & 63;
    bool pending = valid && (unsigned)label < (unsigned)n_comps;
    unsigned long long left = __ballot(pending);
    while (left) {                                                   // (wave-uniform: one round per distinct label, <= 64)
        const int leader = __ffsll((long long)left) - 1;
        const int lab = __shfl(label, leader, 64);
        const bool mine = pending && label == lab;
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int n = __popcll(__ballot(mine && flags[k]));
            if (lane == leader && n) atomicAdd(counts + (size_t)lab * MC_COLS + cols[k], n);
        }
        pending = pending && !mine;
        left = __ballot(pending);
    }
}

__global__ __launch_bounds__(MC_THREADS) void cs_vertex_count_kernel(const int *__restrict__ vertex_labels, int n_verts, int n_comps,
                                                                     int *counts) {
    const int v = blockIdx.x * MC_THREADS + threadIdx.x;
    const bool valid = v < n_verts;
    const int cols[1] = {COL_VERTS};
    const bool flags[1] = {true};
    cs_wave_add<1>(counts, n_comps, valid, valid ? vertex_labels[v] : -1, cols, flags);
}

__device__ __forceinline__ bool face_ok(int a, int b, int c, int n_verts) {
    return (unsigned)a < (unsigned)n_verts && (unsigned)b < (unsigned)n_verts && (unsigned)c < (unsigned)n_verts;
}

__global__ __launch_bounds__(MC_THREADS) void cs_edge_keys_kernel(const int *__restrict__ faces, int m, int n_verts,
                                                                  unsigned long long *__restrict__ keys, unsigned *__restrict__ vals) {
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= m) return;
    const int f = i / 3, k = i - 3 * f;
    const int *face = faces + (size_t)f * 3;
    const int f0 = face[0], f1 = face[1], f2 = face[2];
    const int a = k == 0 ? f0 : k == 1 ? f1 : f2, b = k == 0 ? f1 : k == 1 ? f2 : f0;
    unsigned long long key = ~0ull;                                  // a degenerate face has no edges
    if (face_ok(f0, f1, f2, n_verts) && f0 != f1 && f1 != f2 && f0 != f2)
        key = ((unsigned long long)(unsigned)(a < b ? a : b) << 32) | (unsigned)(a < b ? b : a);
    keys[i] = key;
    vals[i] = a < b;
}

__global__ __launch_bounds__(MC_THREADS) void cs_edge_count_kernel(const unsigned long long *__restrict__ keys,
                                                                   const unsigned *__restrict__ dirs, int m, int n_verts,
                                                                   const int *__restrict__ vertex_labels, int n_comps, int *counts) {
    const int j = blockIdx.x * MC_THREADS + threadIdx.x;
    bool head = false, two = false, more = false, same = false;
    int label = -1;
    if (j < m) {
        const unsigned long long key = keys[j];
        head = key != ~0ull && (j == 0 || keys[j - 1] != key);
        if (head) {
            two = j + 1 < m && keys[j + 1] == key;
            more = two && j + 2 < m && keys[j + 2] == key;
            same = two && !more && dirs[j] == dirs[j + 1];
            const unsigned lo = (unsigned)(key >> 32);
            label = lo < (unsigned)n_verts ? vertex_labels[lo] : -1;
        }
    }
    const int cols[4] = {COL_EDGES, COL_BOUNDARY, COL_NONMANIFOLD, COL_MISORIENTED};
    const bool flags[4] = {true, !two, more, same};
    cs_wave_add<4>(counts, n_comps, head, label, cols, flags);
}

// ---- fp64 measures ----

__global__ __launch_bounds__(MC_THREADS) void cs_face_keys_kernel(const int *__restrict__ face_labels, int n_tris,
                                                                  unsigned *__restrict__ keys, unsigned *__restrict__ vals) {
    const int f = blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= n_tris) return;
    keys[f] = (unsigned)face_labels[f];
    vals[f] = (unsigned)f;
}

// chunk j = sorted positions [256 j, 256 j + 256).  first[j] = the sum of the chunk's first segment (when that segment does
// not both begin after the chunk's first position and end in it), last[j] = the sum of its last one: 2 doubles each.
__global__ __launch_bounds__(MC_THREADS) void cs_terms_kernel(const float *__restrict__ tris, const int *__restrict__ faces,
                                                              const unsigned *__restrict__ labels, const unsigned *__restrict__ order,
                                                              int n_tris, int n_comps, int *counts, int *__restrict__ seg_begin,
                                                              int *__restrict__ seg_end, double *__restrict__ first,
                                                              double *__restrict__ last, double *__restrict__ measures) {
    __shared__ double s_area[MC_THREADS], s_vol[MC_THREADS];
    __shared__ int s_lab[MC_THREADS];
    const int tid = threadIdx.x, p = blockIdx.x * MC_THREADS + tid;
    const bool valid = p < n_tris;
    int lab = -1;
    double area = 0.0, vol = 0.0;
    bool degenerate = false;
    if (valid) {
        lab = (int)labels[p];
        if ((unsigned)lab >= (unsigned)n_comps) lab = -1;            // (a label the caller's count does not cover)
        const size_t f = order[p];
        const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        degenerate = a == b || b == c || a == c;
        if (!degenerate) {
            const float *t = tris + f * 9;
            const double x0 = t[0], y0 = t[1], z0 = t[2], x1 = t[3], y1 = t[4], z1 = t[5], x2 = t[6], y2 = t[7], z2 = t[8];
            const double ax = x1 - x0, ay = y1 - y0, az = z1 - z0, bx = x2 - x0, by = y2 - y0, bz = z2 - z0;
            const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
            const double cx = y1 * z2 - z1 * y2, cy = z1 * x2 - x1 * z2, cz = x1 * y2 - y1 * x2;
            vol = (x0 * cx + y0 * cy + z0 * cz) / 6.0;
        }
    }
    s_lab[tid] = lab;
    s_area[tid] = area;
    s_vol[tid] = vol;
    __syncthreads();
    for (int o = 1; o < MC_THREADS; o <<= 1) {                       // segmented inclusive scan: [max(segment, tid - 2o + 1), tid]
        const bool take = tid >= o && s_lab[tid - o] == lab;
        const double a = take ? s_area[tid - o] : 0.0, v = take ? s_vol[tid - o] : 0.0;
        __syncthreads();
        if (take) {
            s_area[tid] += a;
            s_vol[tid] += v;
        }
        __syncthreads();
    }
    const bool begins = valid && (p == 0 || labels[p - 1] != labels[p]);
    const bool ends = valid && (p == n_tris - 1 || labels[p + 1] != labels[p]);
    const bool chunk_last = valid && (tid == MC_THREADS - 1 || p == n_tris - 1);
    if (lab >= 0) {
        if (begins) seg_begin[lab] = p;
        if (ends) seg_end[lab] = p + 1;
    }
    if (valid && (ends || chunk_last)) {
        const bool of_first = s_lab[0] == lab;                       // sorted: equal to the first label = the first segment
        if (ends && !of_first && lab >= 0) {                         // began after the chunk's first position, ends here: whole
            measures[(size_t)lab * 2] = s_area[tid];
            measures[(size_t)lab * 2 + 1] = s_vol[tid];
        }
        if (of_first) {
            first[(size_t)blockIdx.x * 2] = s_area[tid];
            first[(size_t)blockIdx.x * 2 + 1] = s_vol[tid];
        }
        if (chunk_last) {
            last[(size_t)blockIdx.x * 2] = s_area[tid];
            last[(size_t)blockIdx.x * 2 + 1] = s_vol[tid];
        }
    }
    const int cols[1] = {COL_DEGEN};
    const bool flags[1] = {degenerate};
    cs_wave_add<1>(counts, n_comps, valid, lab, cols, flags);
}

// a wave per component
__global__ __launch_bounds__(MC_THREADS) void cs_finish_kernel(int n_comps, const int *__restrict__ seg_begin,
                                                               const int *__restrict__ seg_end, const double *__restrict__ first,
                                                               const double *__restrict__ last, int *__restrict__ counts,
                                                               double *__restrict__ measures) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * (MC_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= n_comps) return;                                        // (wave-uniform)
    const int s = seg_begin[c], e = seg_end[c];
    int *row = counts + (size_t)c * MC_COLS;
    if (e > s) {
        const int j0 = s / MC_THREADS, j1 = (e - 1) / MC_THREADS;
        // one chunk: cs_terms_kernel wrote the sum itself unless the segment is the chunk's first one
        if (j0 != j1 || s == j0 * MC_THREADS) {
            double area = 0.0, vol = 0.0;
            for (int j = j0 + 1 + lane; j <= j1; j += 64) {          // j0 < j <= j1: the segment is the first of chunk j
                area += first[(size_t)j * 2];
                vol += first[(size_t)j * 2 + 1];
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                area += __shfl_xor(area, o, 64);
                vol += __shfl_xor(vol, o, 64);
            }
            const double *head = j0 == j1 ? first : last;            // (j0 < j1: the segment is the last of chunk j0)
            if (lane == 0) {
                measures[(size_t)c * 2] = head[(size_t)j0 * 2] + area;
                measures[(size_t)c * 2 + 1] = head[(size_t)j0 * 2 + 1] + vol;
            }
        }
    }
    if (lane == 0) {
        row[COL_FACES] = e > s ? e - s : 0;
        row[COL_EULER] = row[COL_VERTS] - row[COL_EDGES] + (row[COL_FACES] - row[COL_DEGEN]);
    }
}

// ---- selection and compaction ----

__device__ __forceinline__ bool comp_closed(const int *row) {
    return row[COL_FACES] - row[COL_DEGEN] > 0 && row[COL_BOUNDARY] == 0 && row[COL_NONMANIFOLD] == 0 && row[COL_MISORIENTED] == 0;
}

__global__ __launch_bounds__(MC_THREADS) void sel_components_kernel(const int *__restrict__ counts, const double *__restrict__ measures,
                                                                    int n_comps, double min_rel_area, int drop_cavities,
                                                                    const unsigned char *__restrict__ explicit_keep,
                                                                    unsigned char *__restrict__ keep) {
    __shared__ double s_max[MC_THREADS];
    double largest = -INFINITY;
    if (!explicit_keep && min_rel_area > 0.0) {
        for (int c = threadIdx.x; c < n_comps; c += MC_THREADS) largest = fmax(largest, measures[(size_t)c * 2]);
        s_max[threadIdx.x] = largest;
        __syncthreads();
        for (int o = MC_THREADS / 2; o >= 1; o >>= 1) {
            if ((int)threadIdx.x < o) s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + o]);
            __syncthreads();
        }
        largest = s_max[0];
    }
    for (int c = threadIdx.x; c < n_comps; c += MC_THREADS) {
        bool k;
        if (explicit_keep) {
            k = explicit_keep[c] != 0;
        } else {
            k = true;
            if (min_rel_area > 0.0) k = measures[(size_t)c * 2] >= min_rel_area * largest;
            if (drop_cavities && comp_closed(counts + (size_t)c * MC_COLS) && measures[(size_t)c * 2 + 1] < 0.0) k = false;
        }
        keep[c] = k;
    }
}

__global__ __launch_bounds__(MC_THREADS) void sel_faces_kernel(const int *__restrict__ face_labels, int n_tris, int n_comps,
                                                               const unsigned char *__restrict__ keep, int *__restrict__ keep_pos) {
    const int f = blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= n_tris) return;
    const int c = face_labels[f];
    keep_pos[f] = (unsigned)c < (unsigned)n_comps && keep[c];
}

__global__ void sel_count_kernel(const int *__restrict__ keep_pos, int n_tris, int *__restrict__ n_kept) {
    *n_kept = keep_pos[n_tris - 1];
}

__global__ __launch_bounds__(MC_THREADS) void filter_faces_kernel(const float *__restrict__ tris, const int *__restrict__ keep_pos,
                                                                  int n_tris, float *__restrict__ out, int n_kept) {
    const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= (long long)n_tris * 9) return;
    const int f = (int)(i / 9), k = (int)(i - (long long)f * 9);
    const int pos = keep_pos[f], before = f ? keep_pos[f - 1] : 0;
    if (pos == before + 1 && pos >= 1 && pos <= n_kept) out[(size_t)(pos - 1) * 9 + k] = tris[i];
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
size_t sort_temp_bytes(int n_tris) {
    const size_t t32 = sort32_temp_bytes(n_tris), t64 = sort64_temp_bytes(3 * n_tris);
    return t32 > t64 ? t32 : t64;
}

int chunks_of(int n_tris) { return (n_tris + MC_THREADS - 1) / MC_THREADS; }

// One scratch for the four calls; none of them needs what another left in it.
//   labelling  parent | root | is_root -> ids | tile totals + the status word
//   stats      keys in | keys out (64-bit, 3 n; the face sort's 32-bit keys and values share them) | values in | values out |
//              segment begin | segment end | first | last | the sorts' workspace
//   selection  keep flags | tile totals
struct CompScratch {
    size_t parent, root, ids, tiles;                                 // labelling
    size_t keys_in, keys_out, vals_in, vals_out, seg_begin, seg_end, first, last, temp;
    size_t keep, sel_tiles;                                          // selection
    size_t total;
};
CompScratch comp_scratch(int n_tris, int n_verts) {
    const size_t m = (size_t)3 * n_tris, v4 = align256((size_t)n_verts * 4);
    CompScratch s;
    s.parent = 0;
    s.root = s.parent + v4;
    s.ids = s.root + v4;
    s.tiles = s.ids + v4;
    const size_t labelling = s.tiles + align256(((size_t)scan_tiles(n_verts) + 1) * 4);
    s.keys_in = 0;
    s.keys_out = s.keys_in + align256(m * 8);
    s.vals_in = s.keys_out + align256(m * 8);
    s.vals_out = s.vals_in + align256(m * 4);
    s.seg_begin = s.vals_out + align256(m * 4);
    s.seg_end = s.seg_begin + v4;
    s.first = s.seg_end + v4;
    s.last = s.first + align256((size_t)chunks_of(n_tris) * 16);
    s.temp = s.last + align256((size_t)chunks_of(n_tris) * 16);
    const size_t stats = s.temp + align256(n_tris > 0 ? sort_temp_bytes(n_tris) : 0);
    s.keep = 0;
    s.sel_tiles = s.keep + align256((size_t)n_verts);
    const size_t selection = s.sel_tiles + align256(((size_t)scan_tiles(n_tris) + 1) * 4);
    s.total = labelling > stats ? labelling : stats;
    if (selection > s.total) s.total = selection;
    return s;
}

bool sizes_ok(const char *who, int n_tris, int n_verts) {
    if (n_tris < 0 || n_verts < 0) {
        zs::set_err("%s: negative size (n_tris=%d n_verts=%d)", who, n_tris, n_verts);
        return false;
    }
    if (n_tris > MC_MAX_TRIS) {
        zs::set_err("%s: too large (n_tris=%d > 2^29)", who, n_tris);
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

dim3 grid_for(long long n) { return dim3((unsigned)((n + MC_THREADS - 1) / MC_THREADS)); }

}  // namespace

extern "C" size_t zs_mesh_components_scratch_bytes(int n_tris, int n_verts) {
    if (n_tris <= 0 || n_verts <= 0 || n_tris > MC_MAX_TRIS || (long long)n_verts > 3ll * n_tris) return 0;
    return comp_scratch(n_tris, n_verts).total;
}

extern "C" int zs_mesh_components(const int *faces, int n_tris, int n_verts, int *vertex_labels, int *face_labels, int *out,
                                  void *scratch, void *stream) {
    const char *who = "zs_mesh_components";
    if (!sizes_ok(who, n_tris, n_verts)) return 0;
    if (n_tris == 0 || n_verts == 0) return 1;
    if (!faces || !vertex_labels || !face_labels || !out || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (!scratch_ok(who, scratch)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CompScratch s = comp_scratch(n_tris, n_verts);
    char *base = static_cast<char *>(scratch);
    int *parent = reinterpret_cast<int *>(base + s.parent), *root = reinterpret_cast<int *>(base + s.root);
    int *ids = reinterpret_cast<int *>(base + s.ids), *tile_tot = reinterpret_cast<int *>(base + s.tiles);
    const int tiles = scan_tiles(n_verts);
    int *status = tile_tot + tiles;
    const dim3 block(MC_THREADS), vgrid = grid_for(n_verts), fgrid = grid_for(n_tris);

    hipLaunchKernelGGL(cc_init_kernel, vgrid, block, 0, st, parent, n_verts, status);
    hipLaunchKernelGGL(cc_link_kernel, fgrid, block, 0, st, faces, n_tris, n_verts, parent, status);
    hipLaunchKernelGGL(cc_flatten_kernel, vgrid, block, 0, st, static_cast<const int *>(parent), n_verts, root, ids, status);
    hipLaunchKernelGGL((scan_tiles_kernel<int, true>), dim3(tiles), dim3(256), 0, st, ids, (long long)n_verts, tile_tot);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(tiles), dim3(256), 0, st, ids, (long long)n_verts,
                       static_cast<const int *>(tile_tot), tiles, static_cast<int *>(nullptr));
    hipLaunchKernelGGL(cc_vertex_labels_kernel, vgrid, block, 0, st, static_cast<const int *>(root), static_cast<const int *>(ids),
                       n_verts, static_cast<const int *>(status), vertex_labels, out);
    hipLaunchKernelGGL(cc_face_labels_kernel, fgrid, block, 0, st, faces, n_tris, n_verts, static_cast<const int *>(vertex_labels),
                       face_labels);
    return zs::check_launch(who) ? 1 : 0;
}

extern "C" int zs_mesh_component_stats(const float *tris, const int *faces, const int *vertex_labels, const int *face_labels,
                                       int n_tris, int n_verts, int n_comps, int *counts, double *measures, void *scratch,
                                       void *stream) {
    const char *who = "zs_mesh_component_stats";
    if (!sizes_ok(who, n_tris, n_verts)) return 0;
    if (n_comps < 0) {
        zs::set_err("%s: negative size (n_comps=%d)", who, n_comps);
        return 0;
    }
    if (n_comps > n_verts) {
        zs::set_err("%s: bad component count (%d > %d vertices)", who, n_comps, n_verts);
        return 0;
    }
    if (n_tris == 0 || n_verts == 0 || n_comps == 0) return 1;
    if (!tris || !faces || !vertex_labels || !face_labels || !counts || !measures || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (!scratch_ok(who, scratch)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CompScratch s = comp_scratch(n_tris, n_verts);
    char *base = static_cast<char *>(scratch);
    const int m = 3 * n_tris, chunks = chunks_of(n_tris);
    unsigned long long *ekeys_in = reinterpret_cast<unsigned long long *>(base + s.keys_in);
    unsigned long long *ekeys_out = reinterpret_cast<unsigned long long *>(base + s.keys_out);
    unsigned *fkeys_in = reinterpret_cast<unsigned *>(base + s.keys_in), *fkeys_out = reinterpret_cast<unsigned *>(base + s.keys_out);
    unsigned *vals_in = reinterpret_cast<unsigned *>(base + s.vals_in), *vals_out = reinterpret_cast<unsigned *>(base + s.vals_out);
    int *seg_begin = reinterpret_cast<int *>(base + s.seg_begin), *seg_end = reinterpret_cast<int *>(base + s.seg_end);
    double *first = reinterpret_cast<double *>(base + s.first), *last = reinterpret_cast<double *>(base + s.last);
    void *temp = base + s.temp;
    const size_t sort_bytes = sort_temp_bytes(n_tris);
    size_t temp_bytes = sort_bytes;
    const dim3 block(MC_THREADS);

    if (hipMemsetAsync(counts, 0, (size_t)n_comps * MC_COLS * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(measures, 0, (size_t)n_comps * 2 * sizeof(double), st) != hipSuccess ||
        hipMemsetAsync(seg_begin, 0, (size_t)n_comps * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(seg_end, 0, (size_t)n_comps * sizeof(int), st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    hipLaunchKernelGGL(cs_vertex_count_kernel, grid_for(n_verts), block, 0, st, vertex_labels, n_verts, n_comps, counts);
    // edges
    hipLaunchKernelGGL(cs_edge_keys_kernel, grid_for(m), block, 0, st, faces, m, n_verts, ekeys_in, vals_in);
    if (rocprim::radix_sort_pairs(temp, temp_bytes, ekeys_in, ekeys_out, vals_in, vals_out, (size_t)m, 0u, 64u, st) != hipSuccess) {
        zs::set_err("%s: rocprim::radix_sort_pairs failed", who);
        return 0;
    }
    hipLaunchKernelGGL(cs_edge_count_kernel, grid_for(m), block, 0, st, static_cast<const unsigned long long *>(ekeys_out),
                       static_cast<const unsigned *>(vals_out), m, n_verts, vertex_labels, n_comps, counts);
    // measures (the edge sort's buffers are free again)
    hipLaunchKernelGGL(cs_face_keys_kernel, grid_for(n_tris), block, 0, st, face_labels, n_tris, fkeys_in, vals_in);
    temp_bytes = sort_bytes;
    if (rocprim::radix_sort_pairs(temp, temp_bytes, fkeys_in, fkeys_out, vals_in, vals_out, (size_t)n_tris, 0u, 32u, st) !=
        hipSuccess) {
        zs::set_err("%s: rocprim::radix_sort_pairs failed", who);
        return 0;
    }
    hipLaunchKernelGGL(cs_terms_kernel, dim3(chunks), block, 0, st, tris, faces, static_cast<const unsigned *>(fkeys_out),
                       static_cast<const unsigned *>(vals_out), n_tris, n_comps, counts, seg_begin, seg_end, first, last, measures);
    hipLaunchKernelGGL(cs_finish_kernel, dim3((n_comps + MC_THREADS / 64 - 1) / (MC_THREADS / 64)), block, 0, st, n_comps,
                       static_cast<const int *>(seg_begin), static_cast<const int *>(seg_end), static_cast<const double *>(first),
                       static_cast<const double *>(last), counts, measures);
    return zs::check_launch(who) ? 1 : 0;
}

extern "C" int zs_mesh_components_select(const int *counts, const double *measures, int n_comps, double min_rel_area,
                                         int drop_cavities, const uint8_t *explicit_keep, const int *face_labels, int n_tris,
                                         int n_verts, int *keep_pos, int *n_kept, void *scratch, void *stream) {
    const char *who = "zs_mesh_components_select";
    if (!sizes_ok(who, n_tris, n_verts)) return 0;
    if (n_comps < 0) {
        zs::set_err("%s: negative size (n_comps=%d)", who, n_comps);
        return 0;
    }
    if (n_comps > n_verts) {
        zs::set_err("%s: bad component count (%d > %d vertices)", who, n_comps, n_verts);
        return 0;
    }
    if (!(min_rel_area >= 0.0 && min_rel_area <= 1.0)) {
        zs::set_err("%s: min_rel_area must lie in [0, 1] (0 = no area rule), got %g", who, min_rel_area);
        return 0;
    }
    if (n_tris == 0 || n_verts == 0) return 1;
    if (!face_labels || !keep_pos || !n_kept || !scratch || (n_comps && (!counts || !measures))) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (!scratch_ok(who, scratch)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CompScratch s = comp_scratch(n_tris, n_verts);
    char *base = static_cast<char *>(scratch);
    unsigned char *keep = reinterpret_cast<unsigned char *>(base + s.keep);
    int *tile_tot = reinterpret_cast<int *>(base + s.sel_tiles);
    const int tiles = scan_tiles(n_tris);
    const dim3 block(MC_THREADS);
    if (n_comps)
        hipLaunchKernelGGL(sel_components_kernel, dim3(1), block, 0, st, counts, measures, n_comps, min_rel_area, drop_cavities,
                           explicit_keep, keep);
    hipLaunchKernelGGL(sel_faces_kernel, grid_for(n_tris), block, 0, st, face_labels, n_tris, n_comps,
                       static_cast<const unsigned char *>(keep), keep_pos);
    hipLaunchKernelGGL((scan_tiles_kernel<int, true>), dim3(tiles), dim3(256), 0, st, keep_pos, (long long)n_tris, tile_tot);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(tiles), dim3(256), 0, st, keep_pos, (long long)n_tris,
                       static_cast<const int *>(tile_tot), tiles, static_cast<int *>(nullptr));
    hipLaunchKernelGGL(sel_count_kernel, dim3(1), dim3(1), 0, st, static_cast<const int *>(keep_pos), n_tris, n_kept);
    return zs::check_launch(who) ? 1 : 0;
}

extern "C" int zs_mesh_filter_faces(const float *tris, const int *keep_pos, int n_tris, float *out_tris, int n_kept, void *stream) {
    const char *who = "zs_mesh_filter_faces";
    if (n_tris < 0 || n_kept < 0) {
        zs::set_err("%s: negative size (n_tris=%d n_kept=%d)", who, n_tris, n_kept);
        return 0;
    }
    if (n_tris > MC_MAX_TRIS) {
        zs::set_err("%s: too large (n_tris=%d > 2^29)", who, n_tris);
        return 0;
    }
    if (n_kept > n_tris) {
        zs::set_err("%s: bad count (n_kept=%d > n_tris=%d)", who, n_kept, n_tris);
        return 0;
    }
    if (n_tris == 0 || n_kept == 0) return 1;
    if (!tris || !keep_pos || !out_tris) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    hipLaunchKernelGGL(filter_faces_kernel, grid_for((long long)n_tris * 9), dim3(MC_THREADS), 0, static_cast<hipStream_t>(stream),
                       tris, keep_pos, n_tris, out_tris, n_kept);
    return zs::check_launch(who) ? 1 : 0;
}
