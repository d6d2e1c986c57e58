// Seen-surface mesh of a camera-frame point map on the GPU (gfx950).
//
// Replaces the Python double loop of create_seen_surface (utils/util_vis.py:137-170), which walks every pixel, calls
// torch.norm(...).item() per candidate edge and looks vertex indices up in a dict.  Same rules, same order:
//   vertex : pixel with z > 0 (and mask > 0.5 when a mask is given), numbered from 1 in raster order per image
//   cell (y, x), y < H-1, x < W-1, in raster order: the upper triangle (y,x), (y,x+1), (y+1,x) when the three corners are
//            vertices and |P(y,x) - P(y,x+1)| < thr and |P(y,x) - P(y+1,x)| < thr; then the lower triangle (y,x+1),
//            (y+1,x+1), (y+1,x) when its corners are vertices and |P(y,x+1) - P(y+1,x+1)| < thr and
//            |P(y,x+1) - P(y+1,x)| < thr;  |d| = sqrtf(dx*dx + dy*dy + dz*dz) as written (-ffp-contract=off)
// Order without atomics: a wave owns 64 consecutive pixels of one image (a UNIT); its entry is faces << 32 | vertices, one
// exclusive scan over all units of the batch (zs_scan.h, two launches) gives every unit the number of vertices and faces
// in front of it, the rank inside the unit is a popcount of the wave's ballot below the lane.  Every image starts on a
// unit boundary, so its first unit's offset is the image's base.  Five launches, every one of them spread over
// batch * ceil(H*W / 64) waves; nothing depends on the order of execution: two runs give the same bits.
#include "zs_common.h"
#include "zs_scan.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int SM_THREADS = 256, SM_WAVES = SM_THREADS / 64;

struct SeenMeshArgs {
    const float *xyz, *mask;
    int H, W, n_pix, units_per_image;        // n_pix = H * W
    long long n_units;                       // batch * units_per_image
    float thr;
};

__device__ __forceinline__ bool sm_valid(const SeenMeshArgs &a, size_t pix) {
    const bool z_ok = a.xyz[pix * 3 + 2] > 0.0f;              // NaN: false
    return z_ok && (a.mask == nullptr || a.mask[pix] > 0.5f);
}
__device__ __forceinline__ bool sm_near(const float *p, const float *q, float thr) {
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return sqrtf(dx * dx + dy * dy + dz * dz) < thr;          // NaN: false
}
// the wave's unit -> image, pixel of this lane (live = the pixel exists), and the pixel's flags
struct SeenMeshLane {
    int image, pix;          // pix: raster index inside the image
    size_t at;               // image * n_pix + pix
    bool live, valid, upper, lower;
};
__device__ __forceinline__ SeenMeshLane sm_lane(const SeenMeshArgs &a, long long unit, int lane, bool want_faces) {
    SeenMeshLane s;
    s.image = (int)(unit / a.units_per_image);
    s.pix = (int)(unit - (long long)s.image * a.units_per_image) * 64 + lane;
    s.live = s.pix < a.n_pix;
    s.at = (size_t)s.image * a.n_pix + (s.live ? s.pix : 0);
    s.valid = s.live && sm_valid(a, s.at);
    s.upper = s.lower = false;
    if (!want_faces || !s.live) return s;
    const int y = s.pix / a.W, x = s.pix - y * a.W;
    if (y >= a.H - 1 || x >= a.W - 1) return s;
    // corners: c00 = (y,x), c01 = (y,x+1), c10 = (y+1,x), c11 = (y+1,x+1) - all inside the image here
    const size_t i00 = s.at, i01 = s.at + 1, i10 = s.at + a.W, i11 = s.at + a.W + 1;
    const bool v01 = sm_valid(a, i01), v10 = sm_valid(a, i10), v11 = sm_valid(a, i11);
    const float *p00 = a.xyz + i00 * 3, *p01 = a.xyz + i01 * 3, *p10 = a.xyz + i10 * 3, *p11 = a.xyz + i11 * 3;
    if (s.valid && v01 && v10) s.upper = sm_near(p00, p01, a.thr) && sm_near(p00, p10, a.thr);
    if (v01 && v11 && v10) s.lower = sm_near(p01, p11, a.thr) && sm_near(p01, p10, a.thr);
    return s;
}
__device__ __forceinline__ int sm_rank(unsigned long long ballot, int lane) {       // set bits below this lane
    return __popcll(ballot & ((1ull << lane) - 1ull));
}

// launch 1: sums[unit] = faces << 32 | vertices of the unit; sums[n_units] = 0 (the scan turns it into the totals)
__global__ __launch_bounds__(SM_THREADS) void seen_mesh_count_kernel(SeenMeshArgs a, unsigned long long *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const long long unit = (long long)blockIdx.x * SM_WAVES + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[a.n_units] = 0;
    if (unit >= a.n_units) return;                           // whole waves leave: the ballots below see full units
    const SeenMeshLane s = sm_lane(a, unit, lane, true);
    const unsigned long long bv = __ballot(s.valid), bu = __ballot(s.upper), bl = __ballot(s.lower);
    if (lane == 0) sums[unit] = ((unsigned long long)(__popcll(bu) + __popcll(bl)) << 32) | (unsigned)__popcll(bv);
}

// launch 4 (after the scan): vertex index of every pixel, the compacted vertex rows, the counts of every image
__global__ __launch_bounds__(SM_THREADS) void seen_mesh_verts_kernel(SeenMeshArgs a, const unsigned long long *__restrict__ offsets,
                                                                     int *__restrict__ vert_id, int *__restrict__ vert_pixel,
                                                                     float *__restrict__ verts, int *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long unit = (long long)blockIdx.x * SM_WAVES + (threadIdx.x >> 6);
    if (unit >= a.n_units) return;
    const SeenMeshLane s = sm_lane(a, unit, lane, false);
    const unsigned long long bv = __ballot(s.valid);
    const long long first = (long long)s.image * a.units_per_image;
    const unsigned long long base = offsets[first];
    if (unit == first && lane == 0) {
        const unsigned long long end = offsets[first + a.units_per_image];
        counts[2 * s.image + 0] = (int)((unsigned)end - (unsigned)base);
        counts[2 * s.image + 1] = (int)((unsigned)(end >> 32) - (unsigned)(base >> 32));
    }
    if (!s.live) return;
    const int k = (int)((unsigned)offsets[unit] - (unsigned)base) + sm_rank(bv, lane);        // 0-based row
    vert_id[s.at] = s.valid ? k + 1 : 0;
    if (s.valid) {
        const size_t row = (size_t)s.image * a.n_pix + k;
        vert_pixel[row] = s.pix;
        verts[row * 3 + 0] = a.xyz[s.at * 3 + 0];
        verts[row * 3 + 1] = a.xyz[s.at * 3 + 1];
        verts[row * 3 + 2] = a.xyz[s.at * 3 + 2];
    }
}

// launch 5: the face rows (the same flags as launch 1, from the same input: the same counts)
__global__ __launch_bounds__(SM_THREADS) void seen_mesh_faces_kernel(SeenMeshArgs a, const unsigned long long *__restrict__ offsets,
                                                                     const int *__restrict__ vert_id, int *__restrict__ faces) {
    const int lane = threadIdx.x & 63;
    const long long unit = (long long)blockIdx.x * SM_WAVES + (threadIdx.x >> 6);
    if (unit >= a.n_units) return;
    const SeenMeshLane s = sm_lane(a, unit, lane, true);
    const unsigned long long bu = __ballot(s.upper), bl = __ballot(s.lower);
    if (!s.upper && !s.lower) return;
    const unsigned base = (unsigned)(offsets[(long long)s.image * a.units_per_image] >> 32);
    const int k = (int)((unsigned)(offsets[unit] >> 32) - base) + sm_rank(bu, lane) + sm_rank(bl, lane);
    const size_t cells = (size_t)(a.H - 1) * (a.W - 1);
    int *row = faces + ((size_t)s.image * 2 * cells + k) * 3;
    const int i01 = vert_id[s.at + 1], i10 = vert_id[s.at + a.W];
    if (s.upper) {
        row[0] = vert_id[s.at];
        row[1] = i01;
        row[2] = i10;
        row += 3;
    }
    if (s.lower) {
        row[0] = i01;
        row[1] = vert_id[s.at + a.W + 1];
        row[2] = i10;
    }
}

inline long long sm_units_per_image(int H, int W) { return ((long long)H * W + 63) / 64; }

}  // namespace

// workspace, in 8-byte words: unit sums, scanned in place [n_units + 1] | totals of the scan's tiles
extern "C" size_t zs_seen_mesh_workspace_bytes(int batch, int H, int W) {
    if (batch <= 0 || H <= 0 || W <= 0 || (long long)batch * H * W > (1LL << 30)) return 0;
    const long long n = (long long)batch * sm_units_per_image(H, W) + 1;
    return (size_t)(n + scan_tiles(n) + 1) * 8;
}

extern "C" int zs_seen_mesh(const float *xyz, const float *mask, int batch, int H, int W, float connect_thres, int *vert_id,
                            int *vert_pixel, float *verts, int *faces, int *counts, void *workspace, void *stream) {
    if (batch < 0 || H < 0 || W < 0) {
        zs::set_err("zs_seen_mesh: negative size (batch=%d H=%d W=%d)", batch, H, W);
        return 0;
    }
    if (!(connect_thres > 0.0f) || !isfinite(connect_thres)) {
        zs::set_err("zs_seen_mesh: bad threshold %g (finite and > 0)", (double)connect_thres);
        return 0;
    }
    if (batch == 0 || H == 0 || W == 0) return 1;
    if ((long long)batch * H * W > (1LL << 30)) {
        zs::set_err("zs_seen_mesh: too large (batch * H * W = %lld > 2^30)", (long long)batch * H * W);
        return 0;
    }
    const bool has_cells = H > 1 && W > 1;
    if (!xyz || !vert_id || !vert_pixel || !verts || !counts || !workspace || (has_cells && !faces)) {
        zs::set_err("zs_seen_mesh: null pointer");
        return 0;
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) {
        zs::set_err("zs_seen_mesh: workspace must be 8-byte aligned");
        return 0;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    SeenMeshArgs a;
    a.xyz = xyz;
    a.mask = mask;
    a.H = H;
    a.W = W;
    a.n_pix = H * W;
    a.units_per_image = (int)sm_units_per_image(H, W);
    a.n_units = (long long)batch * a.units_per_image;
    a.thr = connect_thres;
    unsigned long long *sums = static_cast<unsigned long long *>(workspace);
    const long long n = a.n_units + 1;
    const int tiles = scan_tiles(n);
    unsigned long long *tile_tot = sums + n;
    const dim3 grid((unsigned)((a.n_units + SM_WAVES - 1) / SM_WAVES)), block(SM_THREADS);
    hipLaunchKernelGGL(seen_mesh_count_kernel, grid, block, 0, s, a, sums);
    hipLaunchKernelGGL((scan_tiles_kernel<unsigned long long, false>), dim3(tiles), dim3(256), 0, s, sums, n, tile_tot);
    hipLaunchKernelGGL(scan_offsets_kernel<unsigned long long>, dim3(tiles), dim3(256), 0, s, sums, n,
                       static_cast<const unsigned long long *>(tile_tot), tiles, static_cast<unsigned long long *>(nullptr));
    hipLaunchKernelGGL(seen_mesh_verts_kernel, grid, block, 0, s, a, static_cast<const unsigned long long *>(sums), vert_id,
                       vert_pixel, verts, counts);
    if (has_cells)
        hipLaunchKernelGGL(seen_mesh_faces_kernel, grid, block, 0, s, a, static_cast<const unsigned long long *>(sums),
                           static_cast<const int *>(vert_id), faces);
    return zs::check_launch("zs_seen_mesh") ? 1 : 0;
}
