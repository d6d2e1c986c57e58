// The launch contract the two fused decoders (sdf_decoder.hip: exact fp32, sdf_decoder_split.hip: split fp16) share: the
// tile geometry, the layout of the caller's workspace, and the argument checks of the zs_sdf_query_* entry points.
#pragma once
#include "zs_common.h"
#include "sdf_layout.h"

#include <stddef.h>

namespace zs {
namespace qry {

// ---- tile geometry ---------------------------------------------------------------------------------------------- //
constexpr int WAVES = 4;
constexpr int PTS_PER_WAVE = 32;                    // a wave owns 32 query points for the whole network
constexpr int PTS_PER_BLOCK = WAVES * PTS_PER_WAVE;
constexpr int MAX_WGS = 256;                        // one persistent workgroup per CU
constexpr int ZSLAB_F4 = 3 * lay::NT * 4 * 64;      // per wave, float4: three skip layers' fp32 feat partial products

inline int decode_grid_size(int batch, int m) {
    const long long tiles = (long long)batch * ((m + PTS_PER_BLOCK - 1) / PTS_PER_BLOCK);
    return (int)(tiles < MAX_WGS ? tiles : MAX_WGS);
}

// ---- workspace (zs_sdf_workspace_bytes) ------------------------------------------------------------------------- //
// [slab region: MAX_WGS x WAVES x ZSLAB_F4 float4, 96 MiB][tail: 4 KiB]
//  * slab region: the fp32 kernel's per-wave slabs.  The split kernel never touches them; its launches keep the block-0
//    tables of their images at the head of the region, B0_TABLE_FLOATS per image, and behind the tables of all `batch`
//    images their compact block-0 streams, B0_STREAM_BYTES per image.
//  * tail + 0: timing stamps (ZS_EXP_TIMING builds); tail + 1 KiB: the split kernel's tile counter, then 16 ints further
//    one slot per workgroup.
//  * the fp32 kernel's attention dump (zs_sdf_attn_scratch_bytes) lies behind WORKSPACE_BYTES.
constexpr size_t SLAB_REGION_BYTES = (size_t)MAX_WGS * WAVES * ZSLAB_F4 * 16;
constexpr size_t TAIL_BYTES = 4096;
constexpr size_t TAIL_STAMPS = 0, TAIL_TILE_COUNTER = 1024;
constexpr size_t WORKSPACE_BYTES = SLAB_REGION_BYTES + TAIL_BYTES;
constexpr int B0_TABLE_FLOATS = 4096;

__host__ __device__ inline char *workspace_tail(void *workspace) { return static_cast<char *>(workspace) + SLAB_REGION_BYTES; }
__host__ __device__ inline unsigned long long *timing_stamps(void *workspace) {
    return reinterpret_cast<unsigned long long *>(workspace_tail(workspace) + TAIL_STAMPS);
}
__host__ __device__ inline int *tile_counter(void *workspace) {
    return reinterpret_cast<int *>(workspace_tail(workspace) + TAIL_TILE_COUNTER);
}
constexpr int B0_STREAM_KB = 8 * 34;                        // K-block slots of a compact block-0 stream: 34 per head
constexpr size_t B0_STREAM_BYTES = (size_t)B0_STREAM_KB * 2048;   // 544 KiB = 34 whole chunks
// tables AND streams (175 images); a launch of more images runs block 0's q/k/v GEMMs from the program and writes neither
inline bool block0_stream_fit(int batch) {
    return (size_t)batch * (B0_TABLE_FLOATS * sizeof(float) + B0_STREAM_BYTES) <= SLAB_REGION_BYTES;
}
inline char *block0_streams(void *workspace, int batch) {
    return static_cast<char *>(workspace) + (size_t)batch * B0_TABLE_FLOATS * sizeof(float);
}

// ---- a query: what one decode launch evaluates per image --------------------------------------------------------- //
struct Query {
    const float *points;    // point list [batch][m][3]; null: a grid range
    const float *axis;      // grid range: points [first_point, first_point + m) of the G^3 grid over axis[G], x slowest
    int G;
    long long first_point;
    int m;                  // points per image; 0: nothing to launch
    int apply_sigmoid;
};

inline bool check_programs(const char *who, const void *programs, size_t stride) {
    if (!programs) {
        set_err("%s: null pointer", who);
        return false;
    }
    if (stride % 16 != 0 || stride < (size_t)lay::PROGRAM_FLOATS * sizeof(float)) {
        set_err("%s: bad program stride %zu", who, stride);
        return false;
    }
    return true;
}

// The validators: false = zs_last_error() is set, the entry point `who` returns 0.  Nothing is dereferenced.
inline bool points_query(const char *who, const void *programs, size_t stride, int batch, const float *points, int m,
                         const float *out, const void *workspace, Query &q) {
    q = Query{points, nullptr, 0, 0LL, 0, 0};
    if (batch < 0 || m < 0) {
        set_err("%s: negative size (batch=%d m=%d)", who, batch, m);
        return false;
    }
    if (batch == 0 || m == 0) return true;
    if (!points || !out || !workspace) {
        set_err("%s: null pointer", who);
        return false;
    }
    if (!check_programs(who, programs, stride)) return false;
    if (batch * (((long long)m + PTS_PER_BLOCK - 1) / PTS_PER_BLOCK) > 0x7fffffffLL) {
        set_err("%s: too many tiles", who);
        return false;
    }
    q.m = m;
    return true;
}

// `piece`: what the caller should split when one launch would exceed 2^31 points ("range"; "slab" for the slice forms)
inline bool grid_range_query(const char *who, const char *piece, const void *programs, size_t stride, int batch,
                             const float *axis, int G, long long point_begin, long long point_end, int apply_sigmoid,
                             const float *out, const void *workspace, Query &q) {
    q = Query{nullptr, axis, G, point_begin, 0, apply_sigmoid};
    if (batch < 0 || G <= 0 || point_begin < 0 || point_end > (long long)G * G * G || point_begin > point_end) {
        set_err("%s: bad range (batch=%d G=%d points=[%lld,%lld))", who, batch, G, point_begin, point_end);
        return false;
    }
    const long long mm = point_end - point_begin;
    if (batch == 0 || mm == 0) return true;
    if (!programs || !axis || !out || !workspace) {
        set_err("%s: null pointer", who);
        return false;
    }
    if (mm > 0x7fffffffLL - PTS_PER_BLOCK) {
        set_err("%s: %lld points per launch exceed 2^31; split the %s", who, mm, piece);
        return false;
    }
    if (!check_programs(who, programs, stride)) return false;
    q.m = (int)mm;
    return true;
}

// the slice forms check their own range first, then are the grid range [slice_begin G^2, slice_end G^2)
inline bool grid_slices(const char *who, int batch, int G, int slice_begin, int slice_end) {
    if (batch < 0 || G <= 0 || slice_begin < 0 || slice_end > G || slice_begin > slice_end) {
        set_err("%s: bad range (batch=%d G=%d slices=[%d,%d))", who, batch, G, slice_begin, slice_end);
        return false;
    }
    return true;
}

}  // namespace qry
}  // namespace zs
