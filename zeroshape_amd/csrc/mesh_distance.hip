// Exact distance from points to a triangle mesh (closest face, closest point, squared distance) over an indexed mesh (the
// vertices and faces of zs_mesh_weld): the device form of eval_3D.closest_point_on_mesh_host, which defines the semantics.
// The kernels equal it bit for bit.
//
// The contract.  For a query q the result is the lexicographic minimum over the valid faces f of (d2(q, f), f).  A face is
// valid when its three indices lie inside the vertices and its nine coordinates are finite; the others are skipped (counted,
// never read through).  Everything below is fp64, operations as written (-ffp-contract=off), from the fp32 vertices a, b, c
// of the face and the fp32 query:
//
//   segment(p0, p1):   e = p1 - p0, w = q - p0, t = (wx ex + wy ey) + wz ez, l = (ex ex + ey ey) + ez ez
//                      t <= 0: the point is p0;  else t >= l: the point is p1 (the vertex's own bits);
//                      else the point is p0 + (t / l) e, component by component.
//                      The one denominator, l, is divided by only where 0 < t < l: an edge of length zero has t = 0 and
//                      gives p0, nothing is divided by zero and no NaN can arise from finite inputs.
//   interior(a, b, c): u = b - a, v = c - a, w = q - a, n = u x v (nx = uy vz - uz vy, ny = uz vx - ux vz, nz = ux vy - uy vx),
//                      nn = (nx nx + ny ny) + nz nz, m = u x w, k = w x v, g = (mx nx + my ny) + mz nz, h = (kx nx + ky ny) + kz nz.
//                      The projection lies inside when nn > 0, h >= 0, g >= 0 and h + g <= nn; then the point is
//                      (a + (h / nn) u) + (g / nn) v.  The denominator nn is divided by only where nn > 0: a face of zero area
//                      has no interior candidate and is the union of its edges - a segment, or a point when a = b = c.
//   distance:          d = q - point, d2 = (dx dx + dy dy) + dz dz.
//   the face:          the candidates are taken in the order segment(a, b), segment(a, c), segment(b, c), interior; a later
//                      one replaces an earlier one only with a strictly smaller d2.
// The closest point of a triangle is the foot of the perpendicular when that falls inside and a point of the boundary
// otherwise, so the smallest candidate is the exact distance in every Voronoi region without a region test.  A query at a
// vertex gives d2 = 0 exactly (the segment returns the vertex's bits) for every face around it: the lowest index wins.
//
// The search: a uniform grid of na cells per axis over the bounding box of the valid faces (na: the largest with
// 2 na^3 <= n_faces, at most MD_MAX_AXIS; an axis of zero extent is one slab).  A face is binned once, by the centre
// 0.5 (min + max) of its axis-aligned box, so memory depends on the face count alone; the build also reduces the largest
// half-extent 0.5 (max - min) per axis over all faces.
//   face_bounds_kernel   a thread per face: validity (status, skipped count), box; a workgroup's box and half-extents -> partials
//   grid_meta_kernel     one workgroup reduces the partials: origin, cell sizes, half-extents, slack
//   cell_count_kernel    a thread per valid face: its cell, an integer atomic on the cell's count
//   scan_*               zs_scan.h, exclusive, over the na^3 + 1 counts: the cell starts
//   scatter_kernel       a thread per valid face: its 48-byte record (nine coordinates, the face index; three 16-byte loads)
//                        to start + cursor++.  The order inside a cell is not fixed and does not matter: the minimum is
//                        lexicographic in (d2, face).
//   query_kernel         a thread per query walks the cells ring by ring around its own cell and stops when
//                        bound = min over the sides of the visited block that have cells beyond them of
//                                (distance from q to that side) - (the largest half-extent along that axis), minus slack
//                        is positive and bound^2 (1 - 1e-12) exceeds the running minimum.  A face in an unvisited cell has
//                        its centre beyond one of those sides and reaches back at most the half-extent, so all of it lies
//                        farther than bound; slack = 1e-12 (largest |coordinate| + the three extents) is four orders above
//                        the fp64 rounding of the centres, the cell planes and the closest point, and the factor covers
//                        the rounding of the squares.  A skipped face therefore has a strictly larger d2, and the result
//                        equals the scan over all faces bit for bit.  One face as large as the box makes the half-extent
//                        as large as the grid: no bound is positive, every cell is visited - a full scan, still exact.
// The evaluated (query, face) pairs are counted per thread, reduced per wave with shuffles and added by one lane with vector
// atomics (a 32-bit add and its carry); the counters are integer atomics: two runs give the same bytes.
//
// zs_mesh_distance_stats: one workgroup of 256 threads over d = sqrt(d2), entries that are not finite left out and not
// counted: thread t adds its elements i = t, t + 256, ... in ascending i (s = s + d; s2 = s2 + d2; the largest d, the lowest
// index first), thread 0 adds the 256 partial sums in ascending t: max, mean = s / n, rms = sqrt(s2 / n), n.
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_MAX_FACES = 1 << 24;
constexpr int MD_MAX_QUERIES = 1 << 28;
constexpr int MD_MAX_AXIS = 64;               // at most 64^3 cells (1 MiB of starts): reached at 2 * 64^3 = 524,288 faces
constexpr int MD_RECORD_WORDS = 12;           // ax ay az bx | by bz cx cy | cz face - -
constexpr int MD_META_DOUBLES = 16;           // lo[3] cs[3] inv[3] half[3] slack - - -
constexpr int MD_PART = 9;                    // min[3] max[3] half[3]
constexpr double MD_SLACK = 1e-12, MD_SHRINK = 1.0 - 1e-12;
enum { STATUS_VERTEX = 1, STATUS_INDEX = 2, STATUS_QUERY = 4 };
enum { OUT_SKIPPED = 0, OUT_BAD_QUERIES = 1, OUT_STATUS = 2, OUT_PAIRS_LO = 3, OUT_PAIRS_HI = 4, OUT_WORDS = 5 };

int axis_cells(int n_faces) {
    int a = 1;
    while (a < MD_MAX_AXIS && 2ll * (a + 1) * (a + 1) * (a + 1) <= (long long)n_faces) a++;
    return a;
}

struct GridMeta {
    double lo[3], cs[3], inv[3], half[3], slack;
    int nc[3];
};

__device__ __forceinline__ GridMeta load_meta(const double *__restrict__ meta, int na) {
    GridMeta g;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        g.lo[a] = meta[a];
        g.cs[a] = meta[3 + a];
        g.inv[a] = meta[6 + a];
        g.half[a] = meta[9 + a];
        g.nc[a] = g.inv[a] > 0.0 ? na : 1;                           // an axis without extent is one slab
    }
    g.slack = meta[12];
    return g;
}

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

// min (which < 3), max (which < 6) or max again (the half-extents) over a workgroup; the result in thread 0
__device__ __forceinline__ void block_reduce_part(double v[MD_PART], double (*lds)[MD_THREADS / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MD_PART; k++) {
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
        for (int k = 0; k < MD_PART; k++)
            for (int w = 1; w < MD_THREADS / 64; w++) lds[k][0] = k < 3 ? fmin(lds[k][0], lds[k][w]) : fmax(lds[k][0], lds[k][w]);
#pragma unroll
        for (int k = 0; k < MD_PART; k++) v[k] = lds[k][0];
    }
}

__device__ __forceinline__ void empty_part(double v[MD_PART]) {
#pragma unroll
    for (int k = 0; k < MD_PART; k++) v[k] = k < 3 ? INFINITY : k < 6 ? -INFINITY : 0.0;
}

// ---- the grid ----

__global__ __launch_bounds__(MD_THREADS) void face_bounds_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                 int n_faces, int n_verts, int *__restrict__ cell_of,
                                                                 double *__restrict__ partial, int *out) {
    __shared__ double lds[MD_PART][MD_THREADS / 64];
    const int f = blockIdx.x * MD_THREADS + threadIdx.x;
    double v[MD_PART];
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
                v[6 + a] = 0.5 * (mx[a] - mn[a]);
            }
        } else {
            atomicAdd(out + OUT_SKIPPED, 1);
            atomicOr(out + OUT_STATUS, why);
        }
    }
    block_reduce_part(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < MD_PART; k++) partial[(size_t)blockIdx.x * MD_PART + k] = v[k];
    }
}

__global__ __launch_bounds__(MD_THREADS) void grid_meta_kernel(const double *__restrict__ partial, int n_partial, int na,
                                                               double *__restrict__ meta) {
    __shared__ double lds[MD_PART][MD_THREADS / 64];
    double v[MD_PART];
    empty_part(v);
    for (int i = threadIdx.x; i < n_partial; i += MD_THREADS)
#pragma unroll
        for (int k = 0; k < MD_PART; k++) {
            const double other = partial[(size_t)i * MD_PART + k];
            v[k] = k < 3 ? fmin(v[k], other) : fmax(v[k], other);
        }
    block_reduce_part(v, lds);
    if (threadIdx.x != 0) return;
    const bool any = v[0] <= v[3];                                   // no valid face: one empty cell at the origin
    double maxabs = 0.0, extents = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = any ? v[a] : 0.0, hi = any ? v[3 + a] : 0.0;
        double ext = hi - lo;
        if (!(ext > 0.0)) ext = 0.0;
        meta[a] = lo;
        meta[3 + a] = ext / (double)na;
        meta[6 + a] = ext > 0.0 ? (double)na / ext : 0.0;
        meta[9 + a] = any ? v[6 + a] : 0.0;
        maxabs = fmax(maxabs, fmax(fabs(lo), fabs(hi)));
        extents = extents + ext;
    }
    meta[12] = MD_SLACK * (maxabs + extents);
}

__device__ __forceinline__ int cell_of_box(const GridMeta &g, int na, const double mn[3], const double mx[3]) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) c[a] = cell_coord(0.5 * (mn[a] + mx[a]), g.lo[a], g.inv[a], g.nc[a]);
    return (c[2] * na + c[1]) * na + c[0];
}

__global__ __launch_bounds__(MD_THREADS) void cell_count_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                int n_faces, int n_verts, const double *__restrict__ meta, int na,
                                                                int *__restrict__ cell_of, int *__restrict__ count) {
    const int f = blockIdx.x * MD_THREADS + threadIdx.x;
    if (f >= n_faces || cell_of[f] < 0) return;
    float p[9];
    int why;
    if (!load_face(vertices, faces, f, n_verts, p, why)) return;     // (cannot happen: the face was valid)
    const GridMeta g = load_meta(meta, na);
    double mn[3], mx[3];
    face_box(p, mn, mx);
    const int c = cell_of_box(g, na, mn, mx);
    cell_of[f] = c;
    atomicAdd(count + c, 1);
}

// start: the exclusive scan of the counts
__global__ __launch_bounds__(MD_THREADS) void scatter_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                             int n_faces, int n_verts, int n_cells, const int *__restrict__ cell_of,
                                                             const int *__restrict__ start, int *__restrict__ cursor,
                                                             float4 *__restrict__ records) {
    const int f = blockIdx.x * MD_THREADS + threadIdx.x;
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

// ---- the closest point ----

struct Closest {
    double d2, x, y, z;
};

__device__ __forceinline__ void offer(Closest &best, double qx, double qy, double qz, double cx, double cy, double cz, bool first) {
    const double dx = qx - cx, dy = qy - cy, dz = qz - cz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (first || d2 < best.d2) {
        best.d2 = d2;
        best.x = cx;
        best.y = cy;
        best.z = cz;
    }
}

__device__ __forceinline__ void segment(Closest &best, double qx, double qy, double qz, double p0x, double p0y, double p0z,
                                        double p1x, double p1y, double p1z, bool first) {
    const double ex = p1x - p0x, ey = p1y - p0y, ez = p1z - p0z;
    const double wx = qx - p0x, wy = qy - p0y, wz = qz - p0z;
    const double t = (wx * ex + wy * ey) + wz * ez;
    const double l = (ex * ex + ey * ey) + ez * ez;
    double cx = p0x, cy = p0y, cz = p0z;
    if (t > 0.0) {
        if (t < l) {
            const double s = t / l;
            cx = p0x + s * ex;
            cy = p0y + s * ey;
            cz = p0z + s * ez;
        } else {
            cx = p1x;
            cy = p1y;
            cz = p1z;
        }
    }
    offer(best, qx, qy, qz, cx, cy, cz, first);
}

__device__ __forceinline__ Closest closest_on_face(double qx, double qy, double qz, const float4 r0, const float4 r1, const float4 r2) {
    const double ax = (double)r0.x, ay = (double)r0.y, az = (double)r0.z;
    const double bx = (double)r0.w, by = (double)r1.x, bz = (double)r1.y;
    const double cx = (double)r1.z, cy = (double)r1.w, cz = (double)r2.x;
    Closest best;
    segment(best, qx, qy, qz, ax, ay, az, bx, by, bz, true);
    segment(best, qx, qy, qz, ax, ay, az, cx, cy, cz, false);
    segment(best, qx, qy, qz, bx, by, bz, cx, cy, cz, false);
    const double ux = bx - ax, uy = by - ay, uz = bz - az;
    const double vx = cx - ax, vy = cy - ay, vz = cz - az;
    const double wx = qx - ax, wy = qy - ay, wz = qz - az;
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    const double mx = uy * wz - uz * wy, my = uz * wx - ux * wz, mz = ux * wy - uy * wx;
    const double kx = wy * vz - wz * vy, ky = wz * vx - wx * vz, kz = wx * vy - wy * vx;
    const double g = (mx * nx + my * ny) + mz * nz;
    const double h = (kx * nx + ky * ny) + kz * nz;
    if (nn > 0.0 && h >= 0.0 && g >= 0.0 && h + g <= nn) {
        const double beta = h / nn, gamma = g / nn;
        offer(best, qx, qy, qz, (ax + beta * ux) + gamma * vx, (ay + beta * uy) + gamma * vy, (az + beta * uz) + gamma * vz, false);
    }
    return best;
}

__global__ __launch_bounds__(MD_THREADS) void query_kernel(const float *__restrict__ queries, int n_queries,
                                                           const double *__restrict__ meta, int na,
                                                           const int *__restrict__ start, const float4 *__restrict__ records,
                                                           int n_faces, double *__restrict__ out_sqdist, int *__restrict__ out_face,
                                                           double *__restrict__ out_closest, int *out) {
    const int i = blockIdx.x * MD_THREADS + threadIdx.x;
    unsigned pairs = 0;
    if (i < n_queries) {
        const float fx = queries[(size_t)i * 3], fy = queries[(size_t)i * 3 + 1], fz = queries[(size_t)i * 3 + 2];
        Closest best;
        best.d2 = INFINITY;
        best.x = best.y = best.z = NAN;
        int best_f = -1;
        if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) {
            best.d2 = NAN;
            atomicAdd(out + OUT_BAD_QUERIES, 1);
            atomicOr(out + OUT_STATUS, STATUS_QUERY);
        } else {
            const GridMeta g = load_meta(meta, na);
            const double q[3] = {(double)fx, (double)fy, (double)fz};
            int c0[3];
#pragma unroll
            for (int a = 0; a < 3; a++) c0[a] = cell_coord(q[a], g.lo[a], g.inv[a], g.nc[a]);
            for (int r = 0; r < na; r++) {
                const int zlo = max(c0[2] - r, 0), zhi = min(c0[2] + r, g.nc[2] - 1);
                const int ylo = max(c0[1] - r, 0), yhi = min(c0[1] + r, g.nc[1] - 1);
                const int xlo = max(c0[0] - r, 0), xhi = min(c0[0] + r, g.nc[0] - 1);
                for (int cz = zlo; cz <= zhi; cz++)
                    for (int cy = ylo; cy <= yhi; cy++) {
                        const bool shell_zy = (abs(cz - c0[2]) == r) || (abs(cy - c0[1]) == r);
                        // inside the slab only the two end cells of the x run belong to the shell
                        const int xstep = shell_zy ? 1 : max(xhi - xlo, 1);
                        for (int cx = xlo; cx <= xhi; cx += xstep) {
                            if (!shell_zy && abs(cx - c0[0]) != r) continue;
                            const int c = (cz * na + cy) * na + cx;
                            const int e = min(start[c + 1], n_faces);
                            for (int p = max(start[c], 0); p < e; p++) {
                                const float4 r0 = records[(size_t)p * 3], r1 = records[(size_t)p * 3 + 1], r2 = records[(size_t)p * 3 + 2];
                                const Closest got = closest_on_face(q[0], q[1], q[2], r0, r1, r2);
                                const int f = __float_as_int(r2.y);
                                pairs++;
                                if (got.d2 < best.d2 || (got.d2 == best.d2 && f < best_f)) {
                                    best = got;
                                    best_f = f;
                                }
                            }
                        }
                    }
                // every unvisited face has its centre outside the visited block along at least one axis and reaches back at
                // most the largest half-extent; sides of the block that coincide with the grid have nothing beyond them
                double bound = INFINITY;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    if (c0[a] - r > 0) bound = fmin(bound, (q[a] - (g.lo[a] + (double)(c0[a] - r) * g.cs[a])) - g.half[a]);
                    if (c0[a] + r < g.nc[a] - 1) bound = fmin(bound, ((g.lo[a] + (double)(c0[a] + r + 1) * g.cs[a]) - q[a]) - g.half[a]);
                }
                bound = bound - g.slack;
                if (bound > 0.0 && (bound * bound) * MD_SHRINK > best.d2) break;                // also true for bound = +inf
            }
        }
        out_sqdist[i] = best.d2;
        out_face[i] = best_f;
        if (out_closest) {
            out_closest[(size_t)i * 3] = best.x;
            out_closest[(size_t)i * 3 + 1] = best.y;
            out_closest[(size_t)i * 3 + 2] = best.z;
        }
    }
    // the evaluated pairs: a thread has at most 2^24, a wave at most 2^30
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pairs += __shfl_xor(pairs, o, 64);
    if ((threadIdx.x & 63) == 0 && pairs) {
        unsigned *lo = reinterpret_cast<unsigned *>(out + OUT_PAIRS_LO), *hi = reinterpret_cast<unsigned *>(out + OUT_PAIRS_HI);
        const unsigned before = atomicAdd(lo, pairs);
        if (before + pairs < before) atomicAdd(hi, 1u);
    }
}

// ---- statistics ----

__global__ __launch_bounds__(MD_THREADS) void stats_kernel(const double *__restrict__ sqdist, int n, double *__restrict__ out,
                                                           int *__restrict__ out_index) {
    __shared__ double sum[MD_THREADS], sum2[MD_THREADS], top[MD_THREADS];
    __shared__ int count[MD_THREADS], where[MD_THREADS];
    const int t = threadIdx.x;
    double s = 0.0, s2 = 0.0, big = -1.0;
    int cnt = 0, at = -1;
    for (int i = t; i < n; i += MD_THREADS) {
        const double d2 = sqdist[i];
        if (!(d2 >= 0.0 && d2 < INFINITY)) continue;                 // NaN, +inf (and a negative value, which no distance is)
        const double d = sqrt(d2);
        s = s + d;
        s2 = s2 + d2;
        cnt++;
        if (d > big) {
            big = d;
            at = i;
        }
    }
    sum[t] = s;
    sum2[t] = s2;
    top[t] = big;
    count[t] = cnt;
    where[t] = at;
    __syncthreads();
    if (t != 0) return;
    s = 0.0;
    s2 = 0.0;
    big = -1.0;
    cnt = 0;
    at = -1;
    for (int k = 0; k < MD_THREADS; k++) {
        s = s + sum[k];
        s2 = s2 + sum2[k];
        cnt += count[k];
        if (where[k] >= 0 && (top[k] > big || (top[k] == big && where[k] < at))) {
            big = top[k];
            at = where[k];
        }
    }
    const double nd = (double)cnt;
    out[0] = cnt ? big : NAN;
    out[1] = s / nd;                                                 // (0 / 0 = NaN without a finite entry)
    out[2] = sqrt(s2 / nd);
    out[3] = nd;
    *out_index = at;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// meta | the workgroups' boxes | cell of every face | cell counts -> starts (na^3 + 1) | tile totals | cursors | records
struct DistanceScratch {
    size_t meta, partial, cell_of, start, tiles, cursor, records, total;
    int na, n_cells, n_partial;
};
DistanceScratch distance_scratch(int n_faces) {
    const size_t F = (size_t)n_faces;
    DistanceScratch s;
    s.na = axis_cells(n_faces);
    s.n_cells = s.na * s.na * s.na;
    s.n_partial = (n_faces + MD_THREADS - 1) / MD_THREADS;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    };
    s.meta = take(MD_META_DOUBLES * 8);
    s.partial = take((size_t)s.n_partial * MD_PART * 8);
    s.cell_of = take(F * 4);
    s.start = take(((size_t)s.n_cells + 1) * 4);
    s.tiles = take(((size_t)scan_tiles((long long)s.n_cells + 1) + 1) * 4);
    s.cursor = take((size_t)s.n_cells * 4);
    s.records = take(F * MD_RECORD_WORDS * 4);
    s.total = at;
    return s;
}

dim3 grid_for(long long n) { return dim3((unsigned)((n + MD_THREADS - 1) / MD_THREADS)); }

}  // namespace

extern "C" size_t zs_mesh_distance_scratch_bytes(int n_faces, int n_queries) {
    if (n_faces < 0 || n_queries < 0 || n_faces > MD_MAX_FACES || n_queries > MD_MAX_QUERIES) return 0;
    return distance_scratch(n_faces).total;
}

extern "C" int zs_mesh_distance(const float *vertices, const int *faces, int n_faces, int n_verts, const float *queries,
                                int n_queries, double *out_sqdist, int *out_face, double *out_closest, int *out_counts,
                                void *scratch, void *stream) {
    const char *who = "zs_mesh_distance";
    if (n_faces < 0 || n_verts < 0 || n_queries < 0) {
        zs::set_err("%s: negative size (n_faces=%d n_verts=%d n_queries=%d)", who, n_faces, n_verts, n_queries);
        return 0;
    }
    if (n_faces > MD_MAX_FACES || n_queries > MD_MAX_QUERIES) {
        zs::set_err("%s: too large (n_faces=%d > 2^24 or n_queries=%d > 2^28)", who, n_faces, n_queries);
        return 0;
    }
    if (n_queries == 0) return 1;
    if ((n_faces > 0 && (!faces || (n_verts > 0 && !vertices))) || !queries || !out_sqdist || !out_face || !out_counts || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("%s: scratch must be 8-byte aligned", who);
        return 0;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DistanceScratch s = distance_scratch(n_faces);
    char *base = static_cast<char *>(scratch);
    double *meta = reinterpret_cast<double *>(base + s.meta), *partial = reinterpret_cast<double *>(base + s.partial);
    int *cell_of = reinterpret_cast<int *>(base + s.cell_of), *start = reinterpret_cast<int *>(base + s.start);
    int *tiles = reinterpret_cast<int *>(base + s.tiles), *cursor = reinterpret_cast<int *>(base + s.cursor);
    float4 *records = reinterpret_cast<float4 *>(base + s.records);
    const long long n_scan = (long long)s.n_cells + 1;
    const int nt = scan_tiles(n_scan);
    const dim3 block(MD_THREADS);

    // the counts, their sentinel, the tile totals and the cursors are adjacent: one memset
    if (hipMemsetAsync(out_counts, 0, OUT_WORDS * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(base + s.start, 0, s.records - s.start, st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    if (n_faces > 0)
        hipLaunchKernelGGL(face_bounds_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts, cell_of, partial,
                           out_counts);
    hipLaunchKernelGGL(grid_meta_kernel, dim3(1), block, 0, st, static_cast<const double *>(partial), s.n_partial, s.na, meta);
    if (n_faces > 0)
        hipLaunchKernelGGL(cell_count_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts,
                           static_cast<const double *>(meta), s.na, cell_of, start);
    hipLaunchKernelGGL((scan_tiles_kernel<int, false>), dim3(nt), dim3(256), 0, st, start, n_scan, tiles);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(nt), dim3(256), 0, st, start, n_scan, static_cast<const int *>(tiles), nt,
                       static_cast<int *>(nullptr));
    if (n_faces > 0)
        hipLaunchKernelGGL(scatter_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts, s.n_cells,
                           static_cast<const int *>(cell_of), static_cast<const int *>(start), cursor, records);
    hipLaunchKernelGGL(query_kernel, grid_for(n_queries), block, 0, st, queries, n_queries, static_cast<const double *>(meta), s.na,
                       static_cast<const int *>(start), static_cast<const float4 *>(records), n_faces, out_sqdist, out_face,
                       out_closest, out_counts);
    return zs::check_launch(who) ? 1 : 0;
}

extern "C" int zs_mesh_distance_stats(const double *sqdist, int n, double *out, int *out_index, void *stream) {
    const char *who = "zs_mesh_distance_stats";
    if (n < 0) {
        zs::set_err("%s: negative size (n=%d)", who, n);
        return 0;
    }
    if (n == 0) return 1;
    if (!sqdist || !out || !out_index) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    hipLaunchKernelGGL(stats_kernel, dim3(1), dim3(MD_THREADS), 0, static_cast<hipStream_t>(stream), sqdist, n, out, out_index);
    return zs::check_launch(who) ? 1 : 0;
}
