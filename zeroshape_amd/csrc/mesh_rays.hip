// Where a ray first meets a triangle mesh (the face, the ray parameter t, the side, the barycentric weights) over an indexed
// mesh (the vertices and faces of zs_mesh_weld): the device form of eval_3D.mesh_rays_host, which defines the semantics.
// The kernels equal it bit for bit.
//
// The contract.  A face is valid when its three indices lie inside the vertices and its nine coordinates are finite; the
// others are skipped (counted, never read through).  A ray (o, d) is invalid when a component is not finite or d = 0; it gets
// (NaN, -1, 0) and is counted.  Everything below is fp64, operations as written (-ffp-contract=off), from the fp32 corners
// a, b, c of a valid face and the fp32 ray - the watertight test of Woop, Benthin and Wald (2013):
//
//   per ray    kz = the first axis with the largest |d|, kx = (kz + 1) mod 3, ky = (kx + 1) mod 3; kx and ky swapped when
//              d[kz] < 0;  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
//   per face   A = a - o;  Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], Az = Sz A[kz];  the same for B and C;
//              U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax;  det = (U + V) + W;
//              t = ((U Az + V Bz) + W Cz) / det.
//   hit        iff (U, V, W) are all >= 0 or all <= 0, det != 0, t_min <= t <= t_max and t is finite (the guard: extreme
//              inputs can overflow the quotient; +inf stays the mark of a miss).
//   result     the lexicographic minimum of (t, face) over the faces that are hit; side = +1 when det > 0 (the ray runs
//              against the normal (b - a) x (c - a)), -1 when det < 0; the weights of (a, b, c) are U / det, V / det, W / det.
//              A miss is (+inf, -1, 0, NaN weights).
// The sheared corner (Ax, Ay) depends on the corner and the ray alone, so the two faces at an edge compute edge functions
// that are exact negatives: a ray through an edge or a vertex hits at least one face around it.
//
// The search: the uniform grid of mesh_distance.hip (na cells per axis over the box of the valid faces, na the largest with
// 2 na^3 <= n_faces, at most MR_MAX_AXIS; an axis without extent is one slab; a face is binned once, by the centre of its
// box: memory depends on the face count alone) with the integer reaches of mesh_inside.hip: all cell indices come from ONE
// monotone function cell(p), and the build reduces, per axis, the largest distance in CELLS from the cell of a face's centre
// down to the cell of its box minimum (reach_lo) and up to that of its box maximum (reach_hi).
//   face_bounds_kernel   a thread per face: validity (status, skipped count), box; a workgroup's box -> partials
//   grid_meta_kernel     one workgroup reduces the partials: origin, cell sizes, the far corner, the scale of the slack
//   cell_count_kernel    a thread per valid face: its cell, an integer atomic on the cell's count; the reaches by atomic max
//   scan_*               zs_scan.h, exclusive, over the na^3 + 1 counts: the cell starts
//   scatter_kernel       a thread per valid face: its 48-byte record to start + cursor++ (the order inside a cell does not
//                        matter: the minimum is lexicographic in (t, face))
//   query_kernel         a thread per ray walks the slabs of its major axis w = kz in ray order.  The faces whose centre lies
//                        in slab c have all their w coordinates in the cells [c - reach_lo, c + reach_hi], that is between two
//                        cell planes (the box of the mesh at the ends), widened by the slack: the ray is there for t in
//                        [ta, tb] (one multiplication by Sz per plane - the only quotient of the walk, and |d[w]| > 0).
//                        A hit's t is a mean of its corners' Az with weights of one sign, so it lies in that interval up to
//                        the rounding that the t slack (1e-12 of the largest |t| over the box) covers.  The walk skips a slab
//                        with tb < t_min and ends when ta > min(t_max, best t): ta does not decrease along the walk, so
//                        every face left out has a strictly larger t.  Inside a slab the ray's extent along the two other
//                        axes over [max(ta, t_min), min(tb, t_max, best t)], widened by the slack, is mapped through cell()
//                        and widened by the reaches as in mesh_inside.hip - a face whose box the ray passes has
//                        cell(min) <= cell(h) <= cell(max) for a point h of both, so its centre's cell lies inside the
//                        rectangle by monotonicity alone.  Each slab is visited once: every cell is read at most once per ray.
//                        slack = MR_SLACK (|largest coordinate| + the three extents + |largest o|): ten orders above the
//                        fp64 rounding of the planes, the ray's points and the sheared corners.  It also covers the one
//                        place where the fp64 test can differ from geometry: an edge function that rounds to zero lets
//                        the test accept a ray that passes a face at a distance up to 2^-52 (dist + diam)^2 / h (h the
//                        smallest height, diam the diameter of the face in the sheared plane) - beyond the slack only for
//                        a face with h < 2^-52 (slack + diam)^2 / slack, about 2e-10 of the box for a face as long as the
//                        box and 1e-13 for one of marching cubes', below what distinct fp32 corners of that size can form.
//                        One face as large as the mesh makes the reaches as large as the grid: every ray reads every cell
//                        of every slab it cannot exclude by t - slow, still exact.
// The evaluated (ray, face) pairs - every record read - are counted per thread, reduced per wave with shuffles and added by
// one lane with vector atomics (a 32-bit add and its carry); all counters are integer atomics: two runs give the same bytes.
//
// zs_mesh_rays_image makes its rays in the kernel (eval_3D.camera_rays_host): pixel (row i, col j) is at (j, i, 1),
// D = K^-1 (j, i, 1) by the adjugate, D / D_z, o = -mean / scale and d = D / scale rounded to fp32 - then any other ray.
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_MAX_FACES = 1 << 24;
constexpr int MR_MAX_RAYS = 1 << 28;
constexpr int MR_MAX_IMAGE = 16384;           // 16384^2 = 2^28 pixels
// design parameters, not measurements: the distance grid's (about two faces per cell, at most 64^3 cells, 48-byte records)
constexpr int MR_MAX_AXIS = 64;
constexpr int MR_RECORD_WORDS = 12;           // ax ay az bx | by bz cx cy | cz face - -
constexpr int MR_META_DOUBLES = 16;           // lo[3] cs[3] inv[3] hi[3] scale | reach_lo[3] reach_hi[3] as ints in the last three
constexpr int MR_META_REACH = 13;
constexpr int MR_PART = 6;                    // min[3] max[3]
constexpr double MR_SLACK = 1.0 / (1 << 20), MR_T_SLACK = 1e-12;
enum { STATUS_VERTEX = 1, STATUS_INDEX = 2, STATUS_QUERY = 4 };
enum { OUT_SKIPPED = 0, OUT_BAD_RAYS = 1, OUT_STATUS = 2, OUT_PAIRS_LO = 3, OUT_PAIRS_HI = 4, OUT_WORDS = 5, OUT_HITS = 5,
       OUT_IMAGE_WORDS = 6 };

int axis_cells(int n_faces) {
    int a = 1;
    while (a < MR_MAX_AXIS && 2ll * (a + 1) * (a + 1) * (a + 1) <= (long long)n_faces) a++;
    return a;
}

// the one index function of the build and the walk: monotone (not decreasing) in p
__device__ __forceinline__ int cell_coord(double p, double lo, double inv, int nc) {
    double t = (p - lo) * inv;
    t = fmin(fmax(t, 0.0), (double)(nc - 1));                        // (also maps NaN to 0)
    return (int)t;
}

// v[k] without an indexed register array (which the compiler would put into scratch)
template <typename T>
__device__ __forceinline__ T pick(T v0, T v1, T v2, int k) {
    return k == 0 ? v0 : (k == 1 ? v1 : v2);
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
__device__ __forceinline__ void block_reduce_part(double v[MR_PART], double (*lds)[MR_THREADS / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < MR_PART; k++) {
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
        for (int k = 0; k < MR_PART; k++) {
            for (int w = 1; w < MR_THREADS / 64; w++) lds[k][0] = k < 3 ? fmin(lds[k][0], lds[k][w]) : fmax(lds[k][0], lds[k][w]);
            v[k] = lds[k][0];
        }
    }
}

__device__ __forceinline__ void empty_part(double v[MR_PART]) {
#pragma unroll
    for (int k = 0; k < MR_PART; k++) v[k] = k < 3 ? INFINITY : -INFINITY;
}

// ---- the grid ----

__global__ __launch_bounds__(MR_THREADS) void face_bounds_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                 int n_faces, int n_verts, int *__restrict__ cell_of,
                                                                 double *__restrict__ partial, int *out) {
    __shared__ double lds[MR_PART][MR_THREADS / 64];
    const int f = blockIdx.x * MR_THREADS + threadIdx.x;
    double v[MR_PART];
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
        for (int k = 0; k < MR_PART; k++) partial[(size_t)blockIdx.x * MR_PART + k] = v[k];
    }
}

// (the reaches, the ints behind the thirteen doubles, were zeroed by the entry point's memset)
__global__ __launch_bounds__(MR_THREADS) void grid_meta_kernel(const double *__restrict__ partial, int n_partial, int na,
                                                               double *__restrict__ meta) {
    __shared__ double lds[MR_PART][MR_THREADS / 64];
    double v[MR_PART];
    empty_part(v);
    for (int i = threadIdx.x; i < n_partial; i += MR_THREADS)
#pragma unroll
        for (int k = 0; k < MR_PART; k++) {
            const double other = partial[(size_t)i * MR_PART + k];
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
        double inv = ext > 0.0 ? (double)na / ext : 0.0;
        if (!(inv > 0.0 && inv < INFINITY)) inv = 0.0;               // an extent too small to divide by: one slab
        meta[a] = lo;
        meta[3 + a] = inv > 0.0 ? ext / (double)na : 0.0;
        meta[6 + a] = inv;
        meta[9 + a] = hi;
        maxabs = fmax(maxabs, fmax(fabs(lo), fabs(hi)));
        extents = extents + ext;
    }
    meta[12] = maxabs + extents;
}

__global__ __launch_bounds__(MR_THREADS) void cell_count_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                int n_faces, int n_verts, double *__restrict__ meta, int na,
                                                                int *__restrict__ cell_of, int *__restrict__ count) {
    const int f = blockIdx.x * MR_THREADS + threadIdx.x;
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
    int *out = reinterpret_cast<int *>(meta + MR_META_REACH);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        int r = max(reach[k], 0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r = max(r, __shfl_xor(r, o, 64));
        if ((threadIdx.x & 63) == 0 && r > 0) atomicMax(out + k, r);
    }
}

// start: the exclusive scan of the counts
__global__ __launch_bounds__(MR_THREADS) void scatter_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                             int n_faces, int n_verts, int n_cells, const int *__restrict__ cell_of,
                                                             const int *__restrict__ start, int *__restrict__ cursor,
                                                             float4 *__restrict__ records) {
    const int f = blockIdx.x * MR_THREADS + threadIdx.x;
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

// ---- the rays ----

struct Ray {
    double ox, oy, oz;                                               // the origin, in the order kx, ky, kz
    double Sx, Sy, Sz;
    int kx, ky, kz;
};

struct Hit {
    double t, U, V, W, det;
    int face;
};

// the sheared corner of the ray's frame from the corner (x, y, z)
__device__ __forceinline__ void shear(const Ray &r, float x, float y, float z, double &sx, double &sy, double &sz) {
    const double px = (double)pick(x, y, z, r.kx) - r.ox;
    const double py = (double)pick(x, y, z, r.ky) - r.oy;
    const double pz = (double)pick(x, y, z, r.kz) - r.oz;
    sx = px - r.Sx * pz;
    sy = py - r.Sy * pz;
    sz = r.Sz * pz;
}

__device__ __forceinline__ void test_face(const Ray &r, double t_min, double t_max, const float4 r0, const float4 r1, const float4 r2,
                                          Hit &best) {
    double Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz;
    shear(r, r0.x, r0.y, r0.z, Ax, Ay, Az);
    shear(r, r0.w, r1.x, r1.y, Bx, By, Bz);
    shear(r, r1.z, r1.w, r2.x, Cx, Cy, Cz);
    const double U = Cx * By - Cy * Bx;
    const double V = Ax * Cy - Ay * Cx;
    const double W = Bx * Ay - By * Ax;
    const bool one_side = (U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0);
    const double det = (U + V) + W;
    const double t = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(one_side && det != 0.0 && t >= t_min && t <= t_max && fabs(t) < INFINITY)) return;
    const int f = __float_as_int(r2.y);
    if (t < best.t || (t == best.t && f < best.face)) {
        best.t = t;
        best.U = U;
        best.V = V;
        best.W = W;
        best.det = det;
        best.face = f;
    }
}

// IMAGE: ray i is the ray of pixel (i / W, i % W) of the camera (intr, mean, scale); the results are fp32 depth, face and
// side per pixel, and the hit pixels are counted.  Otherwise: origins and directions [n,3], out_t fp64 and the weights.
template <bool IMAGE>
__global__ __launch_bounds__(MR_THREADS) void query_kernel(const float *__restrict__ origins, const float *__restrict__ directions,
                                                           int n_rays, const float *__restrict__ intr, const float *__restrict__ mean,
                                                           const float *__restrict__ scale, int W, double t_min, double t_max,
                                                           const double *__restrict__ meta, int na, const int *__restrict__ start,
                                                           const float4 *__restrict__ records, int n_faces,
                                                           double *__restrict__ out_t, float *__restrict__ out_depth,
                                                           int *__restrict__ out_face, signed char *__restrict__ out_side,
                                                           double *__restrict__ out_bary, int *out) {
    const int i = blockIdx.x * MR_THREADS + threadIdx.x;
    unsigned pairs = 0;
    bool is_hit = false;
    if (i < n_rays) {
        float o0, o1, o2, d0, d1, d2;
        if (IMAGE) {
            const double pj = (double)(i % W), pi = (double)(i / W);
            const double k00 = (double)intr[0], k01 = (double)intr[1], k02 = (double)intr[2];
            const double k10 = (double)intr[3], k11 = (double)intr[4], k12 = (double)intr[5];
            const double k20 = (double)intr[6], k21 = (double)intr[7], k22 = (double)intr[8];
            const double c00 = k11 * k22 - k12 * k21, c01 = k02 * k21 - k01 * k22, c02 = k01 * k12 - k02 * k11;
            const double c10 = k12 * k20 - k10 * k22, c11 = k00 * k22 - k02 * k20, c12 = k02 * k10 - k00 * k12;
            const double c20 = k10 * k21 - k11 * k20, c21 = k01 * k20 - k00 * k21, c22 = k00 * k11 - k01 * k10;
            const double kdet = (k00 * c00 + k01 * c10) + k02 * c20;
            const double Dx = ((c00 * pj + c01 * pi) + c02) / kdet;
            const double Dy = ((c10 * pj + c11 * pi) + c12) / kdet;
            const double Dz = ((c20 * pj + c21 * pi) + c22) / kdet;
            const double s = (double)scale[0];
            const bool forward = Dz > 0.0 && Dz < INFINITY;
            o0 = (float)(-(double)mean[0] / s);
            o1 = (float)(-(double)mean[1] / s);
            o2 = (float)(-(double)mean[2] / s);
            d0 = forward ? (float)((Dx / Dz) / s) : NAN;
            d1 = forward ? (float)((Dy / Dz) / s) : NAN;
            d2 = forward ? (float)(1.0 / s) : NAN;
        } else {
            o0 = origins[(size_t)i * 3];
            o1 = origins[(size_t)i * 3 + 1];
            o2 = origins[(size_t)i * 3 + 2];
            d0 = directions[(size_t)i * 3];
            d1 = directions[(size_t)i * 3 + 1];
            d2 = directions[(size_t)i * 3 + 2];
        }
        Hit best;
        best.t = INFINITY;
        best.U = best.V = best.W = best.det = NAN;
        best.face = -1;
        const bool finite = isfinite(o0) && isfinite(o1) && isfinite(o2) && isfinite(d0) && isfinite(d1) && isfinite(d2);
        if (!(finite && (d0 != 0.f || d1 != 0.f || d2 != 0.f))) {
            best.t = NAN;
            atomicAdd(out + OUT_BAD_RAYS, 1);
            atomicOr(out + OUT_STATUS, STATUS_QUERY);
        } else if (t_min <= t_max) {                                 // (false for a NaN bound too: nothing can be hit)
            Ray r;
            const float m0 = fabsf(d0), m1 = fabsf(d1), m2 = fabsf(d2);
            r.kz = (m0 >= m1 && m0 >= m2) ? 0 : (m1 >= m2 ? 1 : 2);  // the first of the largest
            r.kx = r.kz == 2 ? 0 : r.kz + 1;
            r.ky = r.kx == 2 ? 0 : r.kx + 1;
            const double dz = (double)pick(d0, d1, d2, r.kz);
            if (dz < 0.0) {
                const int swap = r.kx;
                r.kx = r.ky;
                r.ky = swap;
            }
            const double dx = (double)pick(d0, d1, d2, r.kx), dy = (double)pick(d0, d1, d2, r.ky);
            r.ox = (double)pick(o0, o1, o2, r.kx);
            r.oy = (double)pick(o0, o1, o2, r.ky);
            r.oz = (double)pick(o0, o1, o2, r.kz);
            r.Sx = dx / dz;
            r.Sy = dy / dz;
            r.Sz = 1.0 / dz;

            // the walk: w = kz, the slabs of the major axis; u < v the two other axes of the grid (u = 0 unless w = 0)
            const int w = r.kz, u = w == 0 ? 1 : 0, v = w == 2 ? 1 : 2;
            const int *reach = reinterpret_cast<const int *>(meta + MR_META_REACH);
            const double lo_w = meta[w], cs_w = meta[3 + w], hi_w = meta[9 + w];
            const double lo_u = meta[u], inv_u = meta[6 + u], lo_v = meta[v], inv_v = meta[6 + v];
            const int nc_w = meta[6 + w] > 0.0 ? na : 1, nc_u = inv_u > 0.0 ? na : 1, nc_v = inv_v > 0.0 ? na : 1;
            const int rlo_w = reach[w], rhi_w = reach[3 + w];
            const int rlo_u = reach[u], rhi_u = reach[3 + u], rlo_v = reach[v], rhi_v = reach[3 + v];
            const int sw = w == 0 ? 1 : (w == 1 ? na : na * na), su = u == 0 ? 1 : na, sv = v == 1 ? na : na * na;
            const double o_w = r.oz;
            const double o_u = (double)pick(o0, o1, o2, u), o_v = (double)pick(o0, o1, o2, v);
            const double d_u = (double)pick(d0, d1, d2, u), d_v = (double)pick(d0, d1, d2, v);
            const double slack = MR_SLACK * (meta[12] + fmax(fabs(o_w), fmax(fabs(o_u), fabs(o_v))));
            const double t_slack = MR_T_SLACK * fmax(fabs(((lo_w - slack) - o_w) * r.Sz), fabs(((hi_w + slack) - o_w) * r.Sz));
            const bool ascending = dz > 0.0;
            for (int step = 0; step < nc_w; step++) {
                const int c = ascending ? step : nc_w - 1 - step;
                const int c_lo = c - rlo_w, c_hi = c + rhi_w;
                const double z_lo = (c_lo <= 0 ? lo_w : lo_w + (double)c_lo * cs_w) - slack;
                const double z_hi = (c_hi >= nc_w - 1 ? hi_w : lo_w + (double)(c_hi + 1) * cs_w) + slack;
                const double t_in = ((ascending ? z_lo : z_hi) - o_w) * r.Sz - t_slack;
                const double t_out = ((ascending ? z_hi : z_lo) - o_w) * r.Sz + t_slack;
                const double t_far = fmin(t_max, best.t);
                if (t_in > t_far) break;                             // t_in does not decrease from here on
                if (t_out < t_min) continue;
                const double tA = fmax(t_in, t_min), tB = fmin(t_out, t_far);            // both finite
                const double uA = o_u + tA * d_u, uB = o_u + tB * d_u;
                const double vA = o_v + tA * d_v, vB = o_v + tB * d_v;
                const int cu0 = cell_coord(fmin(uA, uB) - slack, lo_u, inv_u, nc_u), cu1 = cell_coord(fmax(uA, uB) + slack, lo_u, inv_u, nc_u);
                const int cv0 = cell_coord(fmin(vA, vB) - slack, lo_v, inv_v, nc_v), cv1 = cell_coord(fmax(vA, vB) + slack, lo_v, inv_v, nc_v);
                // a candidate's centre cell k has k - reach_lo <= cell(h) <= k + reach_hi for a point h of its box and the ray's extent
                const int u_lo = max(cu0 - rhi_u, 0), u_hi = min(cu1 + rlo_u, nc_u - 1);
                const int v_lo = max(cv0 - rhi_v, 0), v_hi = min(cv1 + rlo_v, nc_v - 1);
                // along x (stride 1) the cells u_lo .. u_hi are adjacent: one run of records
                const int run = su == 1 ? u_hi - u_lo + 1 : 1;
                for (int cv = v_lo; cv <= v_hi; cv++)
                    for (int cu = u_lo; cu <= u_hi; cu += run) {
                        const int cell = c * sw + cv * sv + cu * su;
                        const int e = min(start[cell + run], n_faces);
                        for (int p = max(start[cell], 0); p < e; p++) {
                            const float4 r0 = records[(size_t)p * 3], r1 = records[(size_t)p * 3 + 1], r2 = records[(size_t)p * 3 + 2];
                            pairs++;
                            test_face(r, t_min, t_max, r0, r1, r2, best);
                        }
                    }
            }
        }
        is_hit = best.face >= 0;
        const signed char side = is_hit ? (best.det > 0.0 ? 1 : -1) : 0;
        out_face[i] = best.face;
        out_side[i] = side;
        if (IMAGE) {
            out_depth[i] = (float)best.t;
        } else {
            out_t[i] = best.t;
            if (out_bary) {
                out_bary[(size_t)i * 3] = best.U / best.det;
                out_bary[(size_t)i * 3 + 1] = best.V / best.det;
                out_bary[(size_t)i * 3 + 2] = best.W / best.det;
            }
        }
    }
    if (IMAGE) {
        const int n_hit = __popcll(__ballot(is_hit));
        if ((threadIdx.x & 63) == 0 && n_hit) atomicAdd(out + OUT_HITS, n_hit);
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

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// meta | the workgroups' boxes | cell of every face | cell counts -> starts (na^3 + 1) | tile totals | cursors | records
struct RayScratch {
    size_t meta, partial, cell_of, start, tiles, cursor, records, total;
    int na, n_cells, n_partial;
};
RayScratch ray_scratch(int n_faces) {
    const size_t F = (size_t)n_faces;
    RayScratch s;
    s.na = axis_cells(n_faces);
    s.n_cells = s.na * s.na * s.na;
    s.n_partial = (n_faces + MR_THREADS - 1) / MR_THREADS;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    };
    s.meta = take(MR_META_DOUBLES * 8);
    s.partial = take((size_t)s.n_partial * MR_PART * 8);
    s.cell_of = take(F * 4);
    s.start = take(((size_t)s.n_cells + 1) * 4);
    s.tiles = take(((size_t)scan_tiles((long long)s.n_cells + 1) + 1) * 4);
    s.cursor = take((size_t)s.n_cells * 4);
    s.records = take(F * MR_RECORD_WORDS * 4);
    s.total = at;
    return s;
}

dim3 grid_for(long long n) { return dim3((unsigned)((n + MR_THREADS - 1) / MR_THREADS)); }

// the build and the query launch that both entry points share; the arguments were checked
int run_rays(const char *who, const float *vertices, const int *faces, int n_faces, int n_verts, const float *origins,
             const float *directions, int n_rays, const float *intr, const float *mean, const float *scale, int W, double t_min,
             double t_max, double *out_t, float *out_depth, int *out_face, signed char *out_side, double *out_bary, int *out_counts,
             int n_counts, void *scratch, hipStream_t st) {
    const RayScratch s = ray_scratch(n_faces);
    char *base = static_cast<char *>(scratch);
    double *meta = reinterpret_cast<double *>(base + s.meta), *partial = reinterpret_cast<double *>(base + s.partial);
    int *cell_of = reinterpret_cast<int *>(base + s.cell_of), *start = reinterpret_cast<int *>(base + s.start);
    int *tiles = reinterpret_cast<int *>(base + s.tiles), *cursor = reinterpret_cast<int *>(base + s.cursor);
    float4 *records = reinterpret_cast<float4 *>(base + s.records);
    const long long n_scan = (long long)s.n_cells + 1;
    const int nt = scan_tiles(n_scan);
    const dim3 block(MR_THREADS);

    // the meta block (its reaches start at zero); the counts, their sentinel, the tile totals and the cursors are adjacent
    if (hipMemsetAsync(out_counts, 0, (size_t)n_counts * sizeof(int), st) != hipSuccess ||
        hipMemsetAsync(base + s.meta, 0, MR_META_DOUBLES * 8, st) != hipSuccess ||
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
    if (out_depth)
        hipLaunchKernelGGL(query_kernel<true>, grid_for(n_rays), block, 0, st, origins, directions, n_rays, intr, mean, scale, W, t_min,
                           t_max, static_cast<const double *>(meta), s.na, static_cast<const int *>(start),
                           static_cast<const float4 *>(records), n_faces, out_t, out_depth, out_face, out_side, out_bary, out_counts);
    else
        hipLaunchKernelGGL(query_kernel<false>, grid_for(n_rays), block, 0, st, origins, directions, n_rays, intr, mean, scale, W,
                           t_min, t_max, static_cast<const double *>(meta), s.na, static_cast<const int *>(start),
                           static_cast<const float4 *>(records), n_faces, out_t, out_depth, out_face, out_side, out_bary, out_counts);
    return zs::check_launch(who) ? 1 : 0;
}

}  // namespace

extern "C" size_t zs_mesh_rays_scratch_bytes(int n_faces, int n_rays) {
    if (n_faces < 0 || n_rays < 0 || n_faces > MR_MAX_FACES || n_rays > MR_MAX_RAYS) return 0;
    if (n_rays == 0) return 0;
    return ray_scratch(n_faces).total;
}

extern "C" int zs_mesh_rays(const float *vertices, const int *faces, int n_faces, int n_verts, const float *origins,
                            const float *directions, int n_rays, double t_min, double t_max, double *out_t, int *out_face,
                            signed char *out_side, double *out_bary, int *out_counts, void *scratch, void *stream) {
    const char *who = "zs_mesh_rays";
    if (n_faces < 0 || n_verts < 0 || n_rays < 0) {
        zs::set_err("%s: negative size (n_faces=%d n_verts=%d n_rays=%d)", who, n_faces, n_verts, n_rays);
        return 0;
    }
    if (n_faces > MR_MAX_FACES || n_rays > MR_MAX_RAYS) {
        zs::set_err("%s: too large (n_faces=%d > 2^24 or n_rays=%d > 2^28)", who, n_faces, n_rays);
        return 0;
    }
    if (n_rays == 0) return 1;
    if ((n_faces > 0 && (!faces || (n_verts > 0 && !vertices))) || !origins || !directions || !out_t || !out_face || !out_side ||
        !out_counts || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("%s: scratch must be 8-byte aligned", who);
        return 0;
    }
    return run_rays(who, vertices, faces, n_faces, n_verts, origins, directions, n_rays, nullptr, nullptr, nullptr, 1, t_min, t_max,
                    out_t, nullptr, out_face, out_side, out_bary, out_counts, OUT_WORDS, scratch, static_cast<hipStream_t>(stream));
}

extern "C" int zs_mesh_rays_image(const float *vertices, const int *faces, int n_faces, int n_verts, const float *intr,
                                  const float *mean, const float *scale, int H, int W, double t_min, double t_max, float *out_depth,
                                  int *out_face, signed char *out_side, int *out_counts, void *scratch, void *stream) {
    const char *who = "zs_mesh_rays_image";
    if (n_faces < 0 || n_verts < 0 || H < 0 || W < 0) {
        zs::set_err("%s: negative size (n_faces=%d n_verts=%d H=%d W=%d)", who, n_faces, n_verts, H, W);
        return 0;
    }
    if (n_faces > MR_MAX_FACES || H > MR_MAX_IMAGE || W > MR_MAX_IMAGE || (long long)H * W > MR_MAX_RAYS) {
        zs::set_err("%s: too large (n_faces=%d > 2^24 or H x W = %d x %d > 2^28)", who, n_faces, H, W);
        return 0;
    }
    if (H == 0 || W == 0) return 1;
    if ((n_faces > 0 && (!faces || (n_verts > 0 && !vertices))) || !intr || !mean || !scale || !out_depth || !out_face || !out_side ||
        !out_counts || !scratch) {
        zs::set_err("%s: null pointer", who);
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(scratch) & 7) {
        zs::set_err("%s: scratch must be 8-byte aligned", who);
        return 0;
    }
    return run_rays(who, vertices, faces, n_faces, n_verts, nullptr, nullptr, H * W, intr, mean, scale, W, t_min, t_max, nullptr,
                    out_depth, out_face, out_side, nullptr, out_counts, OUT_IMAGE_WORDS, scratch, static_cast<hipStream_t>(stream));
}
