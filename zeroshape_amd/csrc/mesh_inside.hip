// On which side of a triangle mesh a point lies: the signed crossing numbers of the +z and the -z ray from every query over an
// indexed mesh (the vertices and faces of zs_mesh_weld) - the device form of eval_3D.mesh_winding_host, which defines the
// semantics.  The kernels equal it exactly: every comparison is between integers.
//
// The contract.  A face is valid when its three indices lie inside the vertices and its nine coordinates are finite; the
// others are skipped (counted, never read through).  A query that is not finite gets (0, 0) and is counted.  Everything below
// is fp64, operations as written (-ffp-contract=off), from the fp32 corners a, b, c of a valid face and the fp32 query q:
//
//   box        the face is a candidate only if min(ax, bx, cx) <= qx <= max(ax, bx, cx) and the same in y (the fp32 values
//              themselves).  No face that lies over q is excluded; the test is part of the definition, so pruning by boxes
//              is exact by construction.
//   side(u, v) of the directed edge u -> v (a -> b, b -> c, c -> a): (lo, hi) = the endpoints ordered lexicographically by
//              their (x, y, z) VALUES (not indices: a soup, a weld and duplicated vertices give a shared edge one number),
//              s = (hx - lx) (qy - ly) - (hy - ly) (qx - lx);  where s == 0: s = -sign(hy - ly) if hy != ly, else
//              sign(hx - lx) (0 when the edge projects to a point);  negated when the face walks the edge hi -> lo.
//              The tie rule is a symbolic shift of q by (eps, eps^2) in x, y: the ray never meets a projected edge or
//              vertex, and a face that projects to a segment never contains q.
//   facing     up-facing over q when the three sides are > 0, down-facing when they are < 0; otherwise the face does not count.
//   height     A = a - q, B = b - q, C = c - q,
//              det = (Ax (By Cz - Bz Cy) + Ay (Bz Cx - Bx Cz)) + Az (Bx Cy - By Cx);  det == 0 counts for neither ray.
//   counts     up   = #(up-facing, det > 0) - #(down-facing, det < 0)     the signed crossing number of the +z ray
//              down = #(down-facing, det > 0) - #(up-facing, det < 0)     ... of the -z ray
// For a closed mesh wound like marching cubes' both equal the winding number; up != down marks a point as ambiguous (the mesh
// is open along the point's column, or the point lies on the surface).
//
// The search: a uniform grid of nc x nc columns over the x, y bounding box of the valid faces (nc: the largest with
// 2 nc^2 <= n_faces, at most MI_MAX_AXIS; an axis without extent is one column).  A face is binned once, by the centre
// 0.5 (min + max) of its x, y box, so memory depends on the face count alone.  All column indices come from ONE monotone
// function col(p) = (int)clamp((p - lo) inv, 0, nc - 1).  The build also reduces, per axis, the largest distance in COLUMNS
// from the column of a face's centre down to the column of its box minimum (reach_lo) and up to that of its box maximum
// (reach_hi).  A face that passes the box test has col(min) <= col(q) <= col(max) by monotonicity, so the column of its
// centre lies in [col(q) - reach_hi, col(q) + reach_lo]: a thread per query visits exactly these columns and skips no
// candidate.  The argument is about integers only; there is no slack and no rounding analysis.  One face as large as the mesh
// makes the reach as large as the grid: every query scans every column - slow, still exact.
//   face_bounds_kernel   a thread per face: validity (status, skipped count), x, y box; a workgroup's box -> partials
//   grid_meta_kernel     one workgroup reduces the partials: origin and inverse column size per axis
//   cell_count_kernel    a thread per valid face: its column, an integer atomic on the column's count; the reaches, reduced
//                        per wave, by integer atomic max
//   scan_*               zs_scan.h, exclusive, over the nc^2 + 1 counts: the column starts
//   scatter_kernel       a thread per valid face: its 48-byte record (nine coordinates, the face index; three 16-byte loads)
//                        to start + cursor++.  The order inside a column does not matter: the counts are sums of integers.
//   query_kernel         a thread per query; the grid form makes its query from the lattice index (fmaf(i, scale, offset) per
//                        axis, x slowest), writes up != 0 as one byte and counts the ambiguous points.
// The evaluated (query, face) pairs - every record read - are counted per thread, reduced per wave with shuffles and added by
// one lane with vector atomics (a 32-bit add and its carry).  All counters are integer atomics: two runs give the same bytes.
//
// zs_occupancy_counts: |A|, |B|, |A and B|, |A or B| of two int8 occupancy arrays (non-zero = inside): integer sums per
// thread, per wave by shuffles, one 64-bit vector atomic per wave and count - exact.
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int MI_THREADS = 256;
constexpr int MI_MAX_FACES = 1 << 24;
constexpr int MI_MAX_QUERIES = 1 << 28;
constexpr int MI_MAX_GRID = 645;              // 645^3 < 2^28 <= 646^3
constexpr int MI_MAX_AXIS = 1024;             // at most 1024^2 columns (4 MiB of starts): reached at 2 * 1024^2 = 2,097,152 faces
constexpr int MI_RECORD_WORDS = 12;           // ax ay az bx | by bz cx cy | cz face - -
constexpr int MI_META_DOUBLES = 8;            // lo[2] inv[2] | reach_lo[2] reach_hi[2] as ints in the next two doubles | - -
constexpr int MI_PART = 4;                    // min[2] max[2]
enum { STATUS_VERTEX = 1, STATUS_INDEX = 2, STATUS_QUERY = 4 };
enum { OUT_SKIPPED = 0, OUT_BAD_QUERIES = 1, OUT_STATUS = 2, OUT_PAIRS_LO = 3, OUT_PAIRS_HI = 4, OUT_WORDS = 5, OUT_AMBIGUOUS = 5,
       OUT_GRID_WORDS = 6 };

int axis_columns(int n_faces) {
    int a = 1;
    while (a < MI_MAX_AXIS && 2ll * (a + 1) * (a + 1) <= (long long)n_faces) a++;
    return a;
}

struct ColumnGrid {
    double lo[2], inv[2];
    int nc[2], reach_lo[2], reach_hi[2];
};

__device__ __forceinline__ ColumnGrid load_grid(const double *__restrict__ meta, int na, bool with_reach) {
    ColumnGrid g;
    const int *reach = reinterpret_cast<const int *>(meta + 4);
#pragma unroll
    for (int a = 0; a < 2; a++) {
        g.lo[a] = meta[a];
        g.inv[a] = meta[2 + a];
        g.nc[a] = g.inv[a] > 0.0 ? na : 1;                           // an axis without extent is one column
        g.reach_lo[a] = with_reach ? reach[a] : 0;
        g.reach_hi[a] = with_reach ? reach[2 + a] : 0;
    }
    return g;
}

// the one index function of the build and the queries: monotone (not decreasing) in p
__device__ __forceinline__ int column_coord(double p, double lo, double inv, int nc) {
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

__device__ __forceinline__ void face_box_xy(const float p[9], double mn[2], double mx[2]) {
#pragma unroll
    for (int a = 0; a < 2; a++) {
        mn[a] = (double)fminf(p[a], fminf(p[3 + a], p[6 + a]));
        mx[a] = (double)fmaxf(p[a], fmaxf(p[3 + a], p[6 + a]));
    }
}

// min (which < 2) or max over a workgroup; the result in thread 0
__device__ __forceinline__ void block_reduce_part(double v[MI_PART], double (*lds)[MI_THREADS / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MI_PART; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(v[k], o, 64);
            v[k] = k < 2 ? fmin(v[k], other) : fmax(v[k], other);
        }
        if (lane == 0) lds[k][wave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < MI_PART; k++) {
            for (int w = 1; w < MI_THREADS / 64; w++) lds[k][0] = k < 2 ? fmin(lds[k][0], lds[k][w]) : fmax(lds[k][0], lds[k][w]);
            v[k] = lds[k][0];
        }
    }
}

__device__ __forceinline__ void empty_part(double v[MI_PART]) {
#pragma unroll
    for (int k = 0; k < MI_PART; k++) v[k] = k < 2 ? INFINITY : -INFINITY;
}

// ---- the columns ----

__global__ __launch_bounds__(MI_THREADS) void face_bounds_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                 int n_faces, int n_verts, int *__restrict__ cell_of,
                                                                 double *__restrict__ partial, int *out) {
    __shared__ double lds[MI_PART][MI_THREADS / 64];
    const int f = blockIdx.x * MI_THREADS + threadIdx.x;
    double v[MI_PART];
    empty_part(v);
    if (f < n_faces) {
        float p[9];
        int why = 0;
        const bool valid = load_face(vertices, faces, f, n_verts, p, why);
        cell_of[f] = valid ? 0 : -1;
        if (valid) {
            double mn[2], mx[2];
            face_box_xy(p, mn, mx);
#pragma unroll
            for (int a = 0; a < 2; a++) {
                v[a] = mn[a];
                v[2 + a] = mx[a];
            }
        } else {
            atomicAdd(out + OUT_SKIPPED, 1);
            atomicOr(out + OUT_STATUS, why);
        }
    }
    block_reduce_part(v, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < MI_PART; k++) partial[(size_t)blockIdx.x * MI_PART + k] = v[k];
    }
}

// (the reaches, the ints behind the four doubles, were zeroed by the entry point's memset)
__global__ __launch_bounds__(MI_THREADS) void grid_meta_kernel(const double *__restrict__ partial, int n_partial, int na,
                                                               double *__restrict__ meta) {
    __shared__ double lds[MI_PART][MI_THREADS / 64];
    double v[MI_PART];
    empty_part(v);
    for (int i = threadIdx.x; i < n_partial; i += MI_THREADS)
#pragma unroll
        for (int k = 0; k < MI_PART; k++) {
            const double other = partial[(size_t)i * MI_PART + k];
            v[k] = k < 2 ? fmin(v[k], other) : fmax(v[k], other);
        }
    block_reduce_part(v, lds);
    if (threadIdx.x != 0) return;
    const bool any = v[0] <= v[2];                                   // no valid face: one empty column at the origin
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const double lo = any ? v[a] : 0.0, hi = any ? v[2 + a] : 0.0;
        double ext = hi - lo;
        if (!(ext > 0.0)) ext = 0.0;
        double inv = ext > 0.0 ? (double)na / ext : 0.0;
        if (!(inv > 0.0 && inv < INFINITY)) inv = 0.0;               // an extent too small to divide by: one column
        meta[a] = lo;
        meta[2 + a] = inv;
    }
}

__global__ __launch_bounds__(MI_THREADS) void cell_count_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                int n_faces, int n_verts, double *__restrict__ meta, int na,
                                                                int *__restrict__ cell_of, int *__restrict__ count) {
    const int f = blockIdx.x * MI_THREADS + threadIdx.x;
    int reach[4] = {0, 0, 0, 0};                                     // lo x, lo y, hi x, hi y
    float p[9];
    int why;
    if (f < n_faces && cell_of[f] >= 0 && load_face(vertices, faces, f, n_verts, p, why)) {
        const ColumnGrid g = load_grid(meta, na, false);
        double mn[2], mx[2];
        face_box_xy(p, mn, mx);
        int c[2];
#pragma unroll
        for (int a = 0; a < 2; a++) {
            // mn <= 0.5 (mn + mx) <= mx also after rounding, so the three columns are ordered
            c[a] = column_coord(0.5 * (mn[a] + mx[a]), g.lo[a], g.inv[a], g.nc[a]);
            reach[a] = c[a] - column_coord(mn[a], g.lo[a], g.inv[a], g.nc[a]);
            reach[2 + a] = column_coord(mx[a], g.lo[a], g.inv[a], g.nc[a]) - c[a];
        }
        const int col = c[1] * na + c[0];
        cell_of[f] = col;
        atomicAdd(count + col, 1);
    }
    int *out = reinterpret_cast<int *>(meta + 4);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int r = max(reach[k], 0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r = max(r, __shfl_xor(r, o, 64));
        if ((threadIdx.x & 63) == 0 && r > 0) atomicMax(out + k, r);
    }
}

// start: the exclusive scan of the counts
__global__ __launch_bounds__(MI_THREADS) void scatter_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                             int n_faces, int n_verts, int n_cells, const int *__restrict__ cell_of,
                                                             const int *__restrict__ start, int *__restrict__ cursor,
                                                             float4 *__restrict__ records) {
    const int f = blockIdx.x * MI_THREADS + threadIdx.x;
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

// ---- the crossing numbers ----

// the sign of the side of q against the directed edge u -> v, ties broken by the symbolic shift
__device__ __forceinline__ int edge_side(double ux, double uy, double uz, double vx, double vy, double vz, double qx, double qy) {
    const bool forward = ux < vx || (ux == vx && (uy < vy || (uy == vy && uz <= vz)));      // the face walks the edge lo -> hi
    const double lx = forward ? ux : vx, ly = forward ? uy : vy;
    const double hx = forward ? vx : ux, hy = forward ? vy : uy;
    const double ex = hx - lx, ey = hy - ly;
    const double s = ex * (qy - ly) - ey * (qx - lx);
    int sign = (s > 0.0) - (s < 0.0);
    if (s == 0.0) sign = ey != 0.0 ? -((ey > 0.0) - (ey < 0.0)) : (ex > 0.0) - (ex < 0.0);
    return forward ? sign : -sign;
}

__device__ __forceinline__ void cross_face(float fx, float fy, float fz, const float4 r0, const float4 r1, const float4 r2, int &up,
                                           int &down) {
    // the box, on the fp32 values
    if (!(fminf(r0.x, fminf(r0.w, r1.z)) <= fx && fx <= fmaxf(r0.x, fmaxf(r0.w, r1.z)))) return;
    if (!(fminf(r0.y, fminf(r1.x, r1.w)) <= fy && fy <= fmaxf(r0.y, fmaxf(r1.x, r1.w)))) return;
    const double qx = (double)fx, qy = (double)fy, qz = (double)fz;
    const double ax = (double)r0.x, ay = (double)r0.y, az = (double)r0.z;
    const double bx = (double)r0.w, by = (double)r1.x, bz = (double)r1.y;
    const double cx = (double)r1.z, cy = (double)r1.w, cz = (double)r2.x;
    const int s0 = edge_side(ax, ay, az, bx, by, bz, qx, qy);
    const int s1 = edge_side(bx, by, bz, cx, cy, cz, qx, qy);
    const int s2 = edge_side(cx, cy, cz, ax, ay, az, qx, qy);
    const bool faces_up = s0 > 0 && s1 > 0 && s2 > 0, faces_down = s0 < 0 && s1 < 0 && s2 < 0;
    if (!faces_up && !faces_down) return;
    const double Ax = ax - qx, Ay = ay - qy, Az = az - qz;
    const double Bx = bx - qx, By = by - qy, Bz = bz - qz;
    const double Cx = cx - qx, Cy = cy - qy, Cz = cz - qz;
    const double det = (Ax * (By * Cz - Bz * Cy) + Ay * (Bz * Cx - Bx * Cz)) + Az * (Bx * Cy - By * Cx);
    // (sums of flags, not branches on which counter to touch: the two counters stay in registers)
    const int above = det > 0.0, below = det < 0.0, u = faces_up, d = faces_down;
    up += (u & above) - (d & below);
    down += (d & above) - (u & below);
}

// GRID: the queries are the lattice points (ix, iy, iz) of a G^3 lattice, x slowest, fmaf(i, scale, offset) per axis; the
// result is one byte per point (up != 0) and the count of ambiguous points.  Otherwise: queries [n,3], out_up and out_down.
template <bool GRID>
__global__ __launch_bounds__(MI_THREADS) void query_kernel(const float *__restrict__ queries, int n_queries, int G, float scale,
                                                           float offset, const double *__restrict__ meta, int na,
                                                           const int *__restrict__ start, const float4 *__restrict__ records,
                                                           int n_faces, int *__restrict__ out_up, int *__restrict__ out_down,
                                                           signed char *__restrict__ out_inside, int *out) {
    const int i = blockIdx.x * MI_THREADS + threadIdx.x;
    unsigned pairs = 0;
    bool ambiguous = false;
    if (i < n_queries) {
        float fx, fy, fz;
        if (GRID) {
            const int iz = i % G, iy = (i / G) % G, ix = i / (G * G);
            fx = fmaf((float)ix, scale, offset);
            fy = fmaf((float)iy, scale, offset);
            fz = fmaf((float)iz, scale, offset);
        } else {
            fx = queries[(size_t)i * 3];
            fy = queries[(size_t)i * 3 + 1];
            fz = queries[(size_t)i * 3 + 2];
        }
        int up = 0, down = 0;
        if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) {
            atomicAdd(out + OUT_BAD_QUERIES, 1);
            atomicOr(out + OUT_STATUS, STATUS_QUERY);
        } else {
            const ColumnGrid g = load_grid(meta, na, true);
            const int c0x = column_coord((double)fx, g.lo[0], g.inv[0], g.nc[0]);
            const int c0y = column_coord((double)fy, g.lo[1], g.inv[1], g.nc[1]);
            // a candidate's centre column c has c - reach_lo <= col(q) <= c + reach_hi
            const int xlo = max(c0x - g.reach_hi[0], 0), xhi = min(c0x + g.reach_lo[0], g.nc[0] - 1);
            const int ylo = max(c0y - g.reach_hi[1], 0), yhi = min(c0y + g.reach_lo[1], g.nc[1] - 1);
            for (int cy = ylo; cy <= yhi; cy++) {
                // the columns xlo .. xhi of a row are adjacent: one run of records
                const int e = min(start[cy * na + xhi + 1], n_faces);
                for (int p = max(start[cy * na + xlo], 0); p < e; p++) {
                    const float4 r0 = records[(size_t)p * 3], r1 = records[(size_t)p * 3 + 1], r2 = records[(size_t)p * 3 + 2];
                    pairs++;
                    cross_face(fx, fy, fz, r0, r1, r2, up, down);
                }
            }
        }
        if (GRID) {
            out_inside[i] = (signed char)(up != 0);
            ambiguous = up != down;
        } else {
            out_up[i] = up;
            if (out_down) out_down[i] = down;
        }
    }
    if (GRID) {
        const int n_ambiguous = __popcll(__ballot(ambiguous));
        if ((threadIdx.x & 63) == 0 && n_ambiguous) atomicAdd(out + OUT_AMBIGUOUS, n_ambiguous);
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

// ---- occupancy counts ----

constexpr int OC_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(MI_THREADS) void occupancy_counts_kernel(const signed char *__restrict__ a, const signed char *__restrict__ b,
                                                                      long long n, unsigned long long *out) {
    unsigned na = 0, nb = 0, both = 0, either = 0;                   // a thread sees at most 2^28 / 256 elements
    const long long stride = (long long)gridDim.x * MI_THREADS;
    for (long long i = (long long)blockIdx.x * MI_THREADS + threadIdx.x; i < n; i += stride) {
        const bool x = a[i] != 0, y = b[i] != 0;
        na += x;
        nb += y;
        both += x && y;
        either += x || y;
    }
    unsigned v[4] = {na, nb, both, either};
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(out + k, (unsigned long long)v[k]);
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// meta | the workgroups' boxes | column of every face | column counts -> starts (nc^2 + 1) | tile totals | cursors | records
struct WindingScratch {
    size_t meta, partial, cell_of, start, tiles, cursor, records, total;
    int na, n_cells, n_partial;
};
WindingScratch winding_scratch(int n_faces) {
    const size_t F = (size_t)n_faces;
    WindingScratch s;
    s.na = axis_columns(n_faces);
    s.n_cells = s.na * s.na;
    s.n_partial = (n_faces + MI_THREADS - 1) / MI_THREADS;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    };
    s.meta = take(MI_META_DOUBLES * 8);
    s.partial = take((size_t)s.n_partial * MI_PART * 8);
    s.cell_of = take(F * 4);
    s.start = take(((size_t)s.n_cells + 1) * 4);
    s.tiles = take(((size_t)scan_tiles((long long)s.n_cells + 1) + 1) * 4);
    s.cursor = take((size_t)s.n_cells * 4);
    s.records = take(F * MI_RECORD_WORDS * 4);
    s.total = at;
    return s;
}

dim3 grid_for(long long n) { return dim3((unsigned)((n + MI_THREADS - 1) / MI_THREADS)); }

// the build and the query launch that both entry points share; the arguments were checked
int run_winding(const char *who, const float *vertices, const int *faces, int n_faces, int n_verts, const float *queries,
                int n_queries, int G, float scale, float offset, int *out_up, int *out_down, signed char *out_inside, int *out_counts,
                int n_counts, void *scratch, hipStream_t st) {
    const WindingScratch s = winding_scratch(n_faces);
    char *base = static_cast<char *>(scratch);
    double *meta = reinterpret_cast<double *>(base + s.meta), *partial = reinterpret_cast<double *>(base + s.partial);
    int *cell_of = reinterpret_cast<int *>(base + s.cell_of), *start = reinterpret_cast<int *>(base + s.start);
    int *tiles = reinterpret_cast<int *>(base + s.tiles), *cursor = reinterpret_cast<int *>(base + s.cursor);
    float4 *records = reinterpret_cast<float4 *>(base + s.records);
    const long long n_scan = (long long)s.n_cells + 1;
    const int nt = scan_tiles(n_scan);
    const dim3 block(MI_THREADS);

    // the meta block (its reaches start at zero); the counts, their sentinel, the tile totals and the cursors are adjacent
    if (hipMemsetAsync(out_counts, 0, (size_t)n_counts * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(base + s.meta, 0, MI_META_DOUBLES * 8, st) != hipSuccess ||
        hipMemsetAsync(base + s.start, 0, s.records - s.start, st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    if (n_faces > 0)
        hipLaunchKernelGGL(face_bounds_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts, cell_of, partial,
                           out_counts);
    hipLaunchKernelGGL(grid_meta_kernel, dim3(1), block, 0, st, static_cast<const double *>(partial), s.n_partial, s.na, meta);
    if (n_faces > 0)
        hipLaunchKernelGGL(cell_count_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts, meta, s.na, cell_of,
                           start);
    hipLaunchKernelGGL((scan_tiles_kernel<int, false>), dim3(nt), dim3(256), 0, st, start, n_scan, tiles);
    hipLaunchKernelGGL(scan_offsets_kernel<int>, dim3(nt), dim3(256), 0, st, start, n_scan, static_cast<const int *>(tiles), nt,
                       static_cast<int *>(nullptr));
    if (n_faces > 0)
        hipLaunchKernelGGL(scatter_kernel, grid_for(n_faces), block, 0, st, vertices, faces, n_faces, n_verts, s.n_cells,
                           static_cast<const int *>(cell_of), static_cast<const int *>(start), cursor, records);
    if (out_inside)
        hipLaunchKernelGGL(query_kernel<true>, grid_for(n_queries), block, 0, st, queries, n_queries, G, scale, offset,
                           static_cast<const double *>(meta), s.na, static_cast<const int *>(start),
                           static_cast<const float4 *>(records), n_faces, out_up, out_down, out_inside, out_counts);
    else
        hipLaunchKernelGGL(query_kernel<false>, grid_for(n_queries), block, 0, st, queries, n_queries, G, scale, offset,
                           static_cast<const double *>(meta), s.na, static_cast<const int *>(start),
                           static_cast<const float4 *>(records), n_faces, out_up, out_down, out_inside, out_counts);
    return zs::check_launch(who) ? 1 : 0;
}

}  // namespace

extern "C" size_t zs_mesh_winding_scratch_bytes(int n_faces, int n_queries) {
    if (n_faces < 0 || n_queries < 0 || n_faces > MI_MAX_FACES || n_queries > MI_MAX_QUERIES) return 0;
    return winding_scratch(n_faces).total;
}

extern "C" int zs_mesh_winding(const float *vertices, const int *faces, int n_faces, int n_verts, const float *queries, int n_queries,
                               int *out_up, int *out_down, int *out_counts, void *scratch, void *stream) {
    const char *who = "zs_mesh_winding";
    if (n_faces < 0 || n_verts < 0 || n_queries < 0) {
        zs::set_err("%s: negative size (n_faces=%d n_verts=%d n_queries=%d)", who, n_faces, n_verts, n_queries);
        return 0;
    }
    if (n_faces > MI_MAX_FACES || n_queries > MI_MAX_QUERIES) {
        zs::set_err("%s: too large (n_faces=%d > 2^24 or n_queries=%d > 2^28)", who, n_faces, n_queries);
        return 0;
    }
    if (n_queries == 0) return 1;
    if ((n_faces > 0 && (!faces || (n_verts > 0 && !vertices))) || !queries || !out_up || !out_counts || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("%s: scratch must be 8-byte aligned", who);
        return 0;
    }
    return run_winding(who, vertices, faces, n_faces, n_verts, queries, n_queries, 0, 0.f, 0.f, out_up, out_down, nullptr, out_counts,
                       OUT_WORDS, scratch, static_cast<hipStream_t>(stream));
}

extern "C" int zs_mesh_winding_grid(const float *vertices, const int *faces, int n_faces, int n_verts, int G, float scale, float offset,
                                    signed char *out_inside, int *out_counts, void *scratch, void *stream) {
    const char *who = "zs_mesh_winding_grid";
    if (n_faces < 0 || n_verts < 0 || G < 0) {
        zs::set_err("%s: negative size (n_faces=%d n_verts=%d G=%d)", who, n_faces, n_verts, G);
        return 0;
    }
    if (n_faces > MI_MAX_FACES || G > MI_MAX_GRID) {
        zs::set_err("%s: too large (n_faces=%d > 2^24 or G=%d > %d: G^3 > 2^28)", who, n_faces, G, MI_MAX_GRID);
        return 0;
    }
    if (G == 0) return 1;
    if ((n_faces > 0 && (!faces || (n_verts > 0 && !vertices))) || !out_inside || !out_counts || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("%s: scratch must be 8-byte aligned", who);
        return 0;
    }
    return run_winding(who, vertices, faces, n_faces, n_verts, nullptr, G * G * G, G, scale, offset, nullptr, nullptr, out_inside,
                       out_counts, OUT_GRID_WORDS, scratch, static_cast<hipStream_t>(stream));
}

extern "C" int zs_occupancy_counts(const signed char *a, const signed char *b, long long n, long long *out, void *stream) {
    const char *who = "zs_occupancy_counts";
    if (n < 0) {
        zs::set_err("%s: negative size (n=%lld)", who, n);
        return 0;
    }
    if (n > (1ll << 40)) {
        zs::set_err("%s: too large (n=%lld > 2^40)", who, n);
        return 0;
    }
    if (!out || (n > 0 && (!a || !b))) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(out) & 7) {
        zs::set_err("%s: out must be 8-byte aligned", who);
        return 0;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out, 0, 4 * sizeof(long long), st) != hipSuccess) {
        zs::set_err("%s: hipMemsetAsync failed", who);
        return 0;
    }
    if (n == 0) return 1;
    // (a thread's 32-bit counts: at most 2^40 / (blocks * 256) elements each, blocks = 2048 beyond 2^19 elements: < 2^22)
    const long long want = (n + MI_THREADS - 1) / MI_THREADS;
    const unsigned blocks = (unsigned)(want < OC_MAX_BLOCKS ? want : OC_MAX_BLOCKS);
    hipLaunchKernelGGL(occupancy_counts_kernel, dim3(blocks), dim3(MI_THREADS), 0, st, a, b, n, reinterpret_cast<unsigned long long *>(out));
    return zs::check_launch(who) ? 1 : 0;
}
