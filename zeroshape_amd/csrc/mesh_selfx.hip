// Which faces of a triangle mesh pass through each other (for every face the number of other faces it crosses, the crossing
// pairs in order, the totals) over an indexed mesh (the vertices and faces of zs_mesh_weld): the device form of
// eval_3D.mesh_self_intersections_host, which defines the semantics.  The kernels equal it in every integer.
//
// The contract.  A face is valid when its three indices lie inside the vertices and its nine coordinates are finite; the
// others are skipped (counted, never read through) and cross nothing.  Everything below is fp64, operations as written
// (-ffp-contract=off), from the fp32 corners of two valid faces i != j:
//
//   candidates  only if their fp32 boxes overlap on every axis, ends included: min_i <= max_j and min_j <= max_i.  The box
//               test is part of the definition (as in mesh_inside.hip), so pruning by boxes is exact by construction.
//   det(D, L, H) = (Dx (Ly Hz - Lz Hy) + Dy (Lz Hx - Lx Hz)) + Dz (Lx Hy - Ly Hx), the grouping of mesh_inside.hip.
//   side(x)     of a point x against the face (a, b, c): det(a - x, b - x, c - x).
//   a segment crosses the face (a, b, c) when side() of its two ends is strictly of opposite signs and, with (p, q) = its
//               ends ordered lexicographically by their (x, y, z) values and D = q - p, the three edge functions - for every
//               directed edge u -> v of a -> b, b -> c, c -> a: (lo, hi) = u, v ordered by value, e = det(D, lo - p, hi - p),
//               negated when the face walks the edge hi -> lo - are all >= 0 or all <= 0 and not all three 0.
//   S, T cross  iff an edge of S crosses T or an edge of T crosses S: symmetric.
//   coincident  iff the three corner positions of S are those of T in some order, by value (either orientation; the faces
//               (a, a, b) and (a, b, b) are not coincident).
// side(x) depends on the point and the face alone, so the three edges of a face share three values: where the three corners
// of T lie on one closed side of S no edge function of T against S is computed at all - the checker's answer, sooner.
// An end that equals a corner of the face makes a zero row and side = 0 exactly: faces that share a vertex or an edge are
// never reported for that contact.  An edge function depends on the segment and the (ordered) edge alone, so the two faces
// at an edge compute exact negatives: a segment through a shared edge crosses at least one of them.
//
// The search: the uniform grid of mesh_distance.hip (na cells per axis over the box of the valid faces, na the largest with
// 2 na^3 <= n_faces, at most SX_MAX_AXIS; an axis without extent is one slab; a face is binned once, by the centre of its
// box: memory depends on the face count alone) with the integer reaches of mesh_inside.hip: all cell indices come from ONE
// monotone function cell(p), and the build reduces, per axis, the largest distance in CELLS from the cell of a face's centre
// down to the cell of its box minimum (reach_lo) and up to that of its box maximum (reach_hi).
//   face_bounds_kernel .. scatter_kernel   the build of mesh_rays.hip (copies)
//   query_kernel<false>  a thread per valid face i reads, per axis, the cells [cell(min_i) - reach_hi, cell(max_i) + reach_lo].
//                        Nothing is skipped, by integers alone: a candidate j overlaps i on the axis, so there is a value h in
//                        both intervals, and cell(min_j) <= cell(h) <= cell(max_j), cell(min_i) <= cell(h) <= cell(max_i) by
//                        monotonicity; the cell k of j's centre has k - reach_lo <= cell(min_j) and cell(max_j) <= k + reach_hi
//                        (the reaches are maxima over all faces), hence cell(min_i) - reach_hi <= k <= cell(max_i) + reach_lo.
//                        No slack.  It counts ALL j != i that it crosses (out_face_counts, a plain store), those with j > i
//                        (the run lengths of the pair list) and, among j > i, the coincident ones.  Every pair is therefore
//                        tested from both sides - the predicate is symmetric - and "examined" counts ORDERED pairs: every
//                        record read with j != i, before the box test; the brute force reads Fv (Fv - 1).
//   scan_*               zs_scan.h, exclusive, 64-bit, over the F + 1 run lengths: where each face's run begins, the total
//   query_kernel<true>   a thread per face with a run that begins below the capacity walks the same cells again and keeps
//                        the smallest j > i that fit, in ascending order, by insertion into its own rows of out_pairs (the
//                        order of the records inside a cell is that of the scatter's atomics and must not show): rows
//                        (i, j), i < j, in lexicographic order, the first `capacity` of them, nothing beyond the total.
// One face as large as the mesh makes the reaches as large as the grid: every thread reads most of the grid - slow, still exact.
// All counters are integer atomics (per wave: shuffles, then one lane adds 32 bits and the carry): two runs give the same bytes.
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int SX_THREADS = 256;
constexpr int SX_MAX_FACES = 1 << 24;
constexpr int SX_MAX_CAPACITY = 1 << 30;
// design parameters, not measurements: the distance grid's (about two faces per cell, at most 64^3 cells, 48-byte records)
constexpr int SX_MAX_AXIS = 64;
constexpr int SX_RECORD_WORDS = 12;           // ax ay az bx | by bz cx cy | cz face - -
constexpr int SX_META_DOUBLES = 16;           // lo[3] cs[3] inv[3] hi[3] - | reach_lo[3] reach_hi[3] as ints in the last three
constexpr int SX_META_REACH = 13;
constexpr int SX_PART = 6;                    // min[3] max[3]
enum { STATUS_VERTEX = 1, STATUS_INDEX = 2 };
enum { OUT_SKIPPED = 0, OUT_STATUS = 1, OUT_CROSS_LO = 2, OUT_CROSS_HI = 3, OUT_SAME_LO = 4, OUT_SAME_HI = 5, OUT_FACES = 6,
       OUT_EXAMINED_LO = 7, OUT_EXAMINED_HI = 8, OUT_WORDS = 9 };
typedef unsigned long long u64;

int axis_cells(int n_faces) {
    int a = 1;
    while (a < SX_MAX_AXIS && 2ll * (a + 1) * (a + 1) * (a + 1) <= (long long)n_faces) a++;
    return a;
}

// the one index function of the build and the query: monotone (not decreasing) in p
__device__ __forceinline__ int cell_coord(double p, double lo, double inv, int nc) {
    double t = (p - lo) * inv;
    t = fmin(fmax(t, 0.0), (double)(nc - 1));                        // (also maps NaN to 0)
    return (int)t;
}

// the three corners of a valid face; false when an index lies outside the vertices (nothing is read then) or a corner is not finite
__device__ __forceinline__ bool load_face(const float *__restrict__ vertices, const int *__restrict__ faces, int f, int n_verts,
                                          float p[9], int &why) {
    const int *face = faces + (size_t)f * 3;
    const int i0 = face[0], i1 = face[1], i2 = face[2];
    if ((unsigned)i0 >= (unsigned)n_verts || (unsigned)i1 >= (unsigned)n_verts || (unsigned)i2 >= (unsigned)n_verts) {
        why = STATUS_INDEX;
        return false;
    }
    const int idx[3] = {i0, i1, i2};
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            p[3 * k + a] = vertices[(size_t)idx[k] * 3 + a];
            finite = finite && isfinite(p[3 * k + a]);
        }
    why = STATUS_VERTEX;
    return finite;
}

__device__ __forceinline__ void face_box(const float p[9], double mn[3], double mx[3]) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        mn[a] = (double)fminf(p[a], fminf(p[3 + a], p[6 + a]));
        mx[a] = (double)fmaxf(p[a], fmaxf(p[3 + a], p[6 + a]));
    }
}

// min (which < 3) or max over a workgroup; the result in thread 0
__device__ __forceinline__ void block_reduce_part(double v[SX_PART], double (*lds)[SX_THREADS / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SX_PART; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(v[k], o, 64);
            v[k] = k < 3 ? fmin(v[k], other) : fmax(v[k], other);
        }
        if (lane == 0) lds[k][wave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SX_PART; k++) {
            for (int w = 1; w < SX_THREADS / 64; w++) lds[k][0] = k < 3 ? fmin(lds[k][0], lds[k][w]) : fmax(lds[k][0], lds[k][w]);
            v[k] = lds[k][0];
        }
    }
}

__device__ __forceinline__ void empty_part(double v[SX_PART]) {
#pragma unroll
    for (int k = 0; k < SX_PART; k++) v[k] = k < 3 ? INFINITY : -INFINITY;
}

// ---- the grid (mesh_rays.hip's build) ----

__global__ __launch_bounds__(SX_THREADS) void face_bounds_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                 int n_faces, int n_verts, int *__restrict__ cell_of,
                                                                 double *__restrict__ partial, int *out) {
    __shared__ double lds[SX_PART][SX_THREADS / 64];
    const int f = blockIdx.x * SX_THREADS + threadIdx.x;
    double v[SX_PART];
    empty_part(v);
    if (f < n_faces) {
        float p[9];
        int why = 0;
        const bool valid = load_face(vertices, faces, f, n_verts, p, why);
        cell_of[f] = valid ? 0 : -1;
        if (valid) {
            double mn[3], mx[3];
            face_box(p, mn, mx);
#pragma unroll
            for (int a = 0; a < 3; a++) {
                v[a] = mn[a];
                v[3 + a] = mx[a];
            }
        } else {
            atomicAdd(out + OUT_SKIPPED, 1);
            atomicOr(out + OUT_STATUS, why);
        }
    }
    block_reduce_part(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SX_PART; k++) partial[(size_t)blockIdx.x * SX_PART + k] = v[k];
    }
}

// (the reaches, the ints behind the thirteen doubles, were zeroed by the entry point's memset)
__global__ __launch_bounds__(SX_THREADS) void grid_meta_kernel(const double *__restrict__ partial, int n_partial, int na,
                                                               double *__restrict__ meta) {
    __shared__ double lds[SX_PART][SX_THREADS / 64];
    double v[SX_PART];
    empty_part(v);
    for (int i = threadIdx.x; i < n_partial; i += SX_THREADS)
#pragma unroll
        for (int k = 0; k < SX_PART; k++) {
            const double other = partial[(size_t)i * SX_PART + k];
            v[k] = k < 3 ? fmin(v[k], other) : fmax(v[k], other);
        }
    block_reduce_part(v, lds);
    if (threadIdx.x != 0) return;
    const bool any = v[0] <= v[3];                                   // no valid face: one empty cell at the origin
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = any ? v[a] : 0.0, hi = any ? v[3 + a] : 0.0;
        double ext = hi - lo;
        if (!(ext > 0.0)) ext = 0.0;
        double inv = ext > 0.0 ? (double)na / ext : 0.0;
        if (!(inv > 0.0 && inv < INFINITY)) inv = 0.0;               // an extent too small to divide by: one slab
        meta[a] = lo;
        meta[3 + a] = inv > 0.0 ? ext / (double)na : 0.0;
        meta[6 + a] = inv;
        meta[9 + a] = hi;
    }
}

__global__ __launch_bounds__(SX_THREADS) void cell_count_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                int n_faces, int n_verts, double *__restrict__ meta, int na,
                                                                int *__restrict__ cell_of, int *__restrict__ count) {
    const int f = blockIdx.x * SX_THREADS + threadIdx.x;
    int reach[6] = {0, 0, 0, 0, 0, 0};                               // lo x y z, hi x y z
    float p[9];
    int why;
    if (f < n_faces && cell_of[f] >= 0 && load_face(vertices, faces, f, n_verts, p, why)) {
        double mn[3], mx[3];
        face_box(p, mn, mx);
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double lo = meta[a], inv = meta[6 + a];
            const int nc = inv > 0.0 ? na : 1;
            // mn <= 0.5 (mn + mx) <= mx also after rounding, so the three cells are ordered
            c[a] = cell_coord(0.5 * (mn[a] + mx[a]), lo, inv, nc);
            reach[a] = c[a] - cell_coord(mn[a], lo, inv, nc);
            reach[3 + a] = cell_coord(mx[a], lo, inv, nc) - c[a];
        }
        const int cell = (c[2] * na + c[1]) * na + c[0];
        cell_of[f] = cell;
        atomicAdd(count + cell, 1);
    }
    int *out = reinterpret_cast<int *>(meta + SX_META_REACH);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int r = max(reach[k], 0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r = max(r, __shfl_xor(r, o, 64));
        if ((threadIdx.x & 63) == 0 && r > 0) atomicMax(out + k, r);
    }
}

// start: the exclusive scan of the counts
__global__ __launch_bounds__(SX_THREADS) void scatter_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                             int n_faces, int n_verts, int n_cells, const int *__restrict__ cell_of,
                                                             const int *__restrict__ start, int *__restrict__ cursor,
                                                             float4 *__restrict__ records) {
    const int f = blockIdx.x * SX_THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const int c = cell_of[f];
    if (c < 0 || c >= n_cells) return;
    float p[9];
    int why;
    if (!load_face(vertices, faces, f, n_verts, p, why)) return;     // (cannot happen)
    const int pos = start[c] + atomicAdd(cursor + c, 1);
    if (pos < 0 || pos >= n_faces) return;                           // (cannot happen)
    float4 *rec = records + (size_t)pos * 3;
    rec[0] = make_float4(p[0], p[1], p[2], p[3]);
    rec[1] = make_float4(p[4], p[5], p[6], p[7]);
    rec[2] = make_float4(p[8], __int_as_float(f), 0.f, 0.f);
}

// ---- the predicate ----

struct P3 {
    double x, y, z;
};

__device__ __forceinline__ P3 point(float x, float y, float z) {
    P3 r;
    r.x = (double)x;
    r.y = (double)y;
    r.z = (double)z;
    return r;
}

__device__ __forceinline__ P3 minus(const P3 &u, const P3 &v) {
    P3 r;
    r.x = u.x - v.x;
    r.y = u.y - v.y;
    r.z = u.z - v.z;
    return r;
}

// u before v in the lexicographic order of the values
__device__ __forceinline__ bool before(const P3 &u, const P3 &v) {
    return u.x < v.x || (u.x == v.x && (u.y < v.y || (u.y == v.y && u.z < v.z)));
}

__device__ __forceinline__ bool same(const P3 &u, const P3 &v) { return u.x == v.x && u.y == v.y && u.z == v.z; }

__device__ __forceinline__ P3 choose(bool first, const P3 &u, const P3 &v) {
    P3 r;
    r.x = first ? u.x : v.x;
    r.y = first ? u.y : v.y;
    r.z = first ? u.z : v.z;
    return r;
}

__device__ __forceinline__ double det3(const P3 &D, const P3 &L, const P3 &H) {
    return (D.x * (L.y * H.z - L.z * H.y) + D.y * (L.z * H.x - L.x * H.z)) + D.z * (L.x * H.y - L.y * H.x);
}

__device__ __forceinline__ double side_of(const P3 &a, const P3 &b, const P3 &c, const P3 &x) {
    return det3(minus(a, x), minus(b, x), minus(c, x));
}

// the edge function of the directed face edge u -> v for the segment p + t D
__device__ __forceinline__ double edge_function(const P3 &D, const P3 &p, const P3 &u, const P3 &v) {
    const bool down = before(v, u);                                  // the face walks the edge hi -> lo
    const P3 lo = choose(down, v, u), hi = choose(down, u, v);
    const double e = det3(D, minus(lo, p), minus(hi, p));
    return down ? -e : e;
}

// the segment (s, t), whose ends have the sides ss and st against the face (a, b, c)
__device__ __forceinline__ bool segment_crosses(const P3 &s, const P3 &t, double ss, double st, const P3 &a, const P3 &b,
                                                const P3 &c) {
    if (!((ss > 0.0 && st < 0.0) || (ss < 0.0 && st > 0.0))) return false;
    const bool swap = before(t, s);
    const P3 p = choose(swap, t, s), q = choose(swap, s, t);
    const P3 D = minus(q, p);
    const double e0 = edge_function(D, p, a, b), e1 = edge_function(D, p, b, c), e2 = edge_function(D, p, c, a);
    return ((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0)) &&
           !(e0 == 0.0 && e1 == 0.0 && e2 == 0.0);
}

// whether an edge of the face (s0, s1, s2) crosses the face (a, b, c)
__device__ __forceinline__ bool edges_cross(const P3 &s0, const P3 &s1, const P3 &s2, const P3 &a, const P3 &b, const P3 &c) {
    const double d0 = side_of(a, b, c, s0), d1 = side_of(a, b, c, s1), d2 = side_of(a, b, c, s2);
    return segment_crosses(s0, s1, d0, d1, a, b, c) || segment_crosses(s1, s2, d1, d2, a, b, c) ||
           segment_crosses(s2, s0, d2, d0, a, b, c);
}

// whether (s0, s1, s2) is a permutation of (a, b, c), by value
__device__ __forceinline__ bool same_corners(const P3 &s0, const P3 &s1, const P3 &s2, const P3 &a, const P3 &b, const P3 &c) {
    const bool m00 = same(s0, a), m01 = same(s0, b), m02 = same(s0, c);
    const bool m10 = same(s1, a), m11 = same(s1, b), m12 = same(s1, c);
    const bool m20 = same(s2, a), m21 = same(s2, b), m22 = same(s2, c);
    return (m00 && m11 && m22) || (m00 && m12 && m21) || (m01 && m10 && m22) || (m01 && m12 && m20) || (m02 && m10 && m21) ||
           (m02 && m11 && m20);
}

// ---- the query ----

// COUNT (WRITE = false): out_face_counts[i], runs[i] = the number of crossed j > i, the totals.
// WRITE: runs = the exclusive scan of those; the smallest j > i of face i go to the rows [runs[i], min(runs[i + 1], capacity)).
template <bool WRITE>
__global__ __launch_bounds__(SX_THREADS) void query_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                           int n_faces, int n_verts, const int *__restrict__ cell_of,
                                                           const double *__restrict__ meta, int na, const int *__restrict__ start,
                                                           const float4 *__restrict__ records, int *__restrict__ out_face_counts,
                                                           u64 *__restrict__ runs, int *out_pairs, int capacity, int *out) {
    const int i = blockIdx.x * SX_THREADS + threadIdx.x;
    unsigned examined = 0, crossed = 0, crossed_above = 0, coincident = 0;
    float own[9];
    int why;
    bool walk = i < n_faces && cell_of[i] >= 0 && load_face(vertices, faces, i, n_verts, own, why);
    u64 row = 0;
    int room = 0, have = 0;
    if (WRITE && walk) {
        row = runs[i];
        const u64 end = runs[i + 1];
        walk = end > row && row < (u64)capacity;
        if (walk) {
            room = (int)(end - row < (u64)capacity - row ? end - row : (u64)capacity - row);
            for (int k = 0; k < room; k++) out_pairs[2 * (row + k)] = i;
        }
    }
    if (walk) {
        double mn[3], mx[3];
        face_box(own, mn, mx);
        const int *reach = reinterpret_cast<const int *>(meta + SX_META_REACH);
        int c_lo[3], c_hi[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double lo = meta[a], inv = meta[6 + a];
            const int nc = inv > 0.0 ? na : 1;
            c_lo[a] = max(cell_coord(mn[a], lo, inv, nc) - reach[3 + a], 0);
            c_hi[a] = min(cell_coord(mx[a], lo, inv, nc) + reach[a], nc - 1);
        }
        const P3 s0 = point(own[0], own[1], own[2]), s1 = point(own[3], own[4], own[5]), s2 = point(own[6], own[7], own[8]);
        // along x (stride 1) the cells c_lo .. c_hi are adjacent: one run of records
        const int run = c_hi[0] - c_lo[0] + 1;
        for (int cz = c_lo[2]; cz <= c_hi[2]; cz++)
            for (int cy = c_lo[1]; cy <= c_hi[1]; cy++) {
                const int cell = (cz * na + cy) * na + c_lo[0];
                const int e = min(start[cell + run], n_faces);
                for (int p = max(start[cell], 0); p < e; p++) {
                    const float4 r0 = records[(size_t)p * 3], r1 = records[(size_t)p * 3 + 1], r2 = records[(size_t)p * 3 + 2];
                    const int j = __float_as_int(r2.y);
                    if (WRITE ? j <= i : j == i) continue;
                    examined++;
                    const bool apart = (double)fminf(r0.x, fminf(r0.w, r1.z)) > mx[0] || (double)fmaxf(r0.x, fmaxf(r0.w, r1.z)) < mn[0] ||
                                       (double)fminf(r0.y, fminf(r1.x, r1.w)) > mx[1] || (double)fmaxf(r0.y, fmaxf(r1.x, r1.w)) < mn[1] ||
                                       (double)fminf(r0.z, fminf(r1.y, r2.x)) > mx[2] || (double)fmaxf(r0.z, fmaxf(r1.y, r2.x)) < mn[2];
                    if (apart) continue;
                    const P3 a = point(r0.x, r0.y, r0.z), b = point(r0.w, r1.x, r1.y), c = point(r1.z, r1.w, r2.x);
                    if (!WRITE && j > i && same_corners(s0, s1, s2, a, b, c)) coincident++;
                    if (!(edges_cross(s0, s1, s2, a, b, c) || edges_cross(a, b, c, s0, s1, s2))) continue;
                    if (!WRITE) {
                        crossed++;
                        if (j > i) crossed_above++;
                    } else {
                        // keep the `room` smallest in ascending order: the rows of this thread alone
                        int k;
                        if (have == room) {
                            if (room == 0 || j > out_pairs[2 * (row + room - 1) + 1]) continue;
                            k = room - 1;
                        } else {
                            k = have++;
                        }
                        while (k > 0) {
                            const int below = out_pairs[2 * (row + k - 1) + 1];
                            if (below <= j) break;
                            out_pairs[2 * (row + k) + 1] = below;
                            k--;
                        }
                        out_pairs[2 * (row + k) + 1] = j;
                    }
                }
            }
    }
    if (WRITE) return;
    if (i < n_faces) {
        out_face_counts[i] = (int)crossed;
        runs[i] = (u64)crossed_above;
    }
    const int n_crossed = __popcll(__ballot(crossed > 0));
    if ((threadIdx.x & 63) == 0 && n_crossed) atomicAdd(out + OUT_FACES, n_crossed);
    // a thread has less than 2^24 of each, a wave less than 2^30
    unsigned sums[3] = {crossed_above, coincident, examined};
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sums[k] += __shfl_xor(sums[k], o, 64);
        if ((threadIdx.x & 63) == 0 && sums[k]) {
            unsigned *lo = reinterpret_cast<unsigned *>(out + OUT_CROSS_LO + (k == 2 ? 5 : 2 * k));
            const unsigned was = atomicAdd(lo, sums[k]);
            if (was + sums[k] < was) atomicAdd(lo + 1, 1u);
        }
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// meta | the workgroups' boxes | cell of every face | cell counts -> starts (na^3 + 1) | tile totals | cursors | records |
// the run lengths -> the run starts (F + 1, 64-bit) | their tile totals
struct SelfScratch {
    size_t meta, partial, cell_of, start, tiles, cursor, records, runs, run_tiles, total;
    int na, n_cells, n_partial;
};
SelfScratch self_scratch(int n_faces) {
    const size_t F = (size_t)n_faces;
    SelfScratch s;
    s.na = axis_cells(n_faces);
    s.n_cells = s.na * s.na * s.na;
    s.n_partial = (n_faces + SX_THREADS - 1) / SX_THREADS;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    };
    s.meta = take(SX_META_DOUBLES * 8);
    s.partial = take((size_t)s.n_partial * SX_PART * 8);
    s.cell_of = take(F * 4);
    s.start = take(((size_t)s.n_cells + 1) * 4);
    s.tiles = take(((size_t)scan_tiles((long long)s.n_cells + 1) + 1) * 4);
    s.cursor = take((size_t)s.n_cells * 4);
    s.records = take(F * SX_RECORD_WORDS * 4);
    s.runs = take((F + 1) * 8);
    s.run_tiles = take(((size_t)scan_tiles((long long)F + 1) + 1) * 8);
    s.total = at;
    return s;
}

dim3 grid_for(long long n) { return dim3((unsigned)((n + SX_THREADS - 1) / SX_THREADS)); }

}  // namespace

extern "C" size_t zs_mesh_self_intersections_scratch_bytes(int n_faces, int capacity) {
    if (n_faces < 0 || capacity < 0 || n_faces > SX_MAX_FACES || capacity > SX_MAX_CAPACITY) return 0;
    return self_scratch(n_faces).total;
}

extern "C" int zs_mesh_self_intersections(const float *vertices, const int *faces, int n_faces, int n_verts, int *out_face_counts,
                                          int *out_pairs, int capacity, int *out_counts, void *scratch, void *stream) {
    const char *who = "zs_mesh_self_intersections";
    if (n_faces < 0 || n_verts < 0 || capacity < 0) {
        zs::set_err("%s: negative size (n_faces=%d n_verts=%d capacity=%d)", who, n_faces, n_verts, capacity);
        return 0;
    }
    if (n_faces > SX_MAX_FACES || capacity > SX_MAX_CAPACITY) {
        zs::set_err("%s: too large (n_faces=%d > 2^24 or capacity=%d > 2^30)", who, n_faces, capacity);
        return 0;
    }
    if (!out_counts || (capacity > 0 && !out_pairs) ||
        (n_faces > 0 && (!faces || (n_verts > 0 && !vertices) || !out_face_counts || !scratch))) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("%s: scratch must be 8-byte aligned", who);
        return 0;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out_counts, 0, OUT_WORDS * sizeof(int), st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    if (n_faces == 0) return 1;                                      // an empty mesh: all zeros

    const SelfScratch s = self_scratch(n_faces);
    char *base = static_cast<char *>(scratch);
    double *meta = reinterpret_cast<double *>(base + s.meta), *partial = reinterpret_cast<double *>(base + s.partial);
    int *cell_of = reinterpret_cast<int *>(base + s.cell_of), *start = reinterpret_cast<int *>(base + s.start);
    int *tiles = reinterpret_cast<int *>(base + s.tiles), *cursor = reinterpret_cast<int *>(base + s.cursor);
    float4 *records = reinterpret_cast<float4 *>(base + s.records);
    u64 *runs = reinterpret_cast<u64 *>(base + s.runs), *run_tiles = reinterpret_cast<u64 *>(base + s.run_tiles);
    const long long n_scan = (long long)s.n_cells + 1, n_runs = (long long)n_faces + 1;
    const int nt = scan_tiles(n_scan), rt = scan_tiles(n_runs);
    const dim3 block(SX_THREADS);

    // the meta block (its reaches start at zero); the counts, their sentinel, the tile totals and the cursors are adjacent;
    // the sentinel of the run lengths
    if (hipMemsetAsync(base + s.meta, 0, SX_META_DOUBLES * 8, st) != hipSuccess ||
        hipMemsetAsync(base + s.start, 0, s.records - s.start, st) != hipSuccess ||
        hipMemsetAsync(runs + n_faces, 0, sizeof(u64), st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    hipLaunchKernelGGL(face_bounds_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts, cell_of, partial,
                       out_counts);
    hipLaunchKernelGGL(grid_meta_kernel, dim3(1), block, 0, st, static_cast<const double *>(partial), s.n_partial, s.na, meta);
    hipLaunchKernelGGL(cell_count_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts, meta, s.na, cell_of,
                       start);
    hipLaunchKernelGGL((scan_tiles_kernel<int, false>), dim3(nt), dim3(256), 0, st, start, n_scan, tiles);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(nt), dim3(256), 0, st, start, n_scan, static_cast<const int *>(tiles), nt,
                       static_cast<int *>(nullptr));
    hipLaunchKernelGGL(scatter_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts, s.n_cells,
                       static_cast<const int *>(cell_of), static_cast<const int *>(start), cursor, records);
    hipLaunchKernelGGL(query_kernel<false>, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts,
                       static_cast<const int *>(cell_of), static_cast<const double *>(meta), s.na, static_cast<const int *>(start),
                       static_cast<const float4 *>(records), out_face_counts, runs, static_cast<int *>(nullptr), 0, out_counts);
    if (capacity > 0) {
        hipLaunchKernelGGL((scan_tiles_kernel<u64, false>), dim3(rt), dim3(256), 0, st, runs, n_runs, run_tiles);
        hipLaunchKernelGGL(scan_offsets_kernel<u64>, dim3(rt), dim3(256), 0, st, runs, n_runs, static_cast<const u64 *>(run_tiles), rt,
                           static_cast<u64 *>(nullptr));
        hipLaunchKernelGGL(query_kernel<true>, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts,
                           static_cast<const int *>(cell_of), static_cast<const double *>(meta), s.na,
                           static_cast<const int *>(start), static_cast<const float4 *>(records), static_cast<int *>(nullptr), runs,
                           out_pairs, capacity, out_counts);
    }
    return zs::check_launch(who) ? 1 : 0;
}
