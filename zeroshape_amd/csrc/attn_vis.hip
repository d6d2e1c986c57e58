// Heat-map frames of the attention GIF on the GPU (gfx950): compute_level_grid(vis_attn=True)'s frame loop
// (utils/eval_3D.py:62-79) and show_att_on_image (utils/util_vis.py:267-293), stage for stage, in one launch.
//
// Input is the z-mean attention of the drawn grid columns (zs_sdf_grid_attn_zmean, csrc/sdf_decoder.hip):
// zmean[b][col][1 + R*R], R = H / win_size patches per side.  One workgroup composes one frame (b, f) in three
// passes over its H x W pixels; the upsampled map is recomputed in each pass instead of stored (12 flops per
// pixel against 600 KB per frame), and the two block-wide maxima between the passes are exact in any order, so
// a frame is bit-reproducible:
//   pass 1   a[R][R] = zmean[.., 0] + zmean[.., 1:]  (LDS);  m = max over pixels of v
//   pass 2   mm = max over pixels and channels of merged
//   pass 3   frame = merged / mm
// with, per pixel (i, j) and in fp32,
//   v       bilinear sample of a, align_corners = false, as torch's upsample_bilinear2d computes it:
//           scale = (float)R / H;  src = scale * (i + 0.5f) - 0.5f, clamped below at 0;  i0 = (int)src;
//           i1 = i0 + (i0 < R - 1);  l1 = src - i0;  l0 = 1 - l1   (the same along W)
//           v = l0h * (l0w * a00 + l1w * a01) + l1h * (l0w * a10 + l1w * a11)
//   level   (uint8)(255.0f * (v / m))    - truncation, as np.uint8(255 * mask)
//   merged  (float)lut[level][ch] / 255.0f + image[ch]
// Built with -ffp-contract=off: the numpy restatement in tests/test_gpu_attn_vis.py follows it operation for
// operation, and the three passes must compute the same v.
#include "zs_common.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int FRAME_THREADS = 1024;
constexpr int MAX_R = 64;

// maximum over the workgroup (every thread gets it); `red` holds one float per wave
__device__ __forceinline__ float block_max(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();                        // the previous maximum has been read by everyone
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = red[0];
    for (int w = 1; w < FRAME_THREADS / 64; w++) m = fmaxf(m, red[w]);
    return m;
}

struct Axis {      // one output coordinate's source pair and weights
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Axis source(int d, float scale, int R) {
    float src = scale * ((float)d + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Axis a;
    a.i0 = (int)src;
    a.i1 = a.i0 + (a.i0 < R - 1 ? 1 : 0);
    a.l1 = src - (float)a.i0;
    a.l0 = 1.0f - a.l1;
    return a;
}

__device__ __forceinline__ float upsampled(const float *a, int R, int i, int j, float sh, float sw) {
    const Axis h = source(i, sh, R), w = source(j, sw, R);
    const float a00 = a[h.i0 * R + w.i0], a01 = a[h.i0 * R + w.i1];
    const float a10 = a[h.i1 * R + w.i0], a11 = a[h.i1 * R + w.i1];
    return h.l0 * (w.l0 * a00 + w.l1 * a01) + h.l1 * (w.l0 * a10 + w.l1 * a11);
}

__device__ __forceinline__ int heat_level(float v, float m) {
    const int lv = (int)(255.0f * (v / m));
    return lv < 0 ? 0 : lv > 255 ? 255 : lv;      // (v <= m: only a degenerate map - m = 0 - could leave the table)
}

__global__ __launch_bounds__(FRAME_THREADS) void attn_frames_kernel(
    const float *__restrict__ zmean, int n_cols, const int *__restrict__ frame_col, int n_frames,
    const float *__restrict__ images, int H, int W, const uint8_t *__restrict__ lut, int R,
    float *__restrict__ frames) {
    __shared__ float a[MAX_R * MAX_R];
    __shared__ float heat[256 * 3];
    __shared__ float red[FRAME_THREADS / 64];
    const int f = blockIdx.x % n_frames, b = blockIdx.x / n_frames;
    int col = frame_col[f];
    col = col < 0 ? 0 : col < n_cols ? col : n_cols - 1;
    const float *z = zmean + ((size_t)b * n_cols + col) * (1 + R * R);
    for (int i = threadIdx.x; i < R * R; i += FRAME_THREADS) a[i] = z[0] + z[1 + i];
    for (int i = threadIdx.x; i < 256 * 3; i += FRAME_THREADS) heat[i] = (float)lut[i] / 255.0f;
    __syncthreads();

    const float sh = (float)R / (float)H, sw = (float)R / (float)W;
    const int pixels = H * W;
    const float *img = images + (size_t)b * 3 * pixels;
    float *out = frames + (size_t)blockIdx.x * pixels * 3;

    float m = -INFINITY;
    for (int p = threadIdx.x; p < pixels; p += FRAME_THREADS) m = fmaxf(m, upsampled(a, R, p / W, p % W, sh, sw));
    m = block_max(m, red);

    float mm = -INFINITY;
    for (int p = threadIdx.x; p < pixels; p += FRAME_THREADS) {
        const float *hc = heat + 3 * heat_level(upsampled(a, R, p / W, p % W, sh, sw), m);
        mm = fmaxf(mm, fmaxf(hc[0] + img[p], fmaxf(hc[1] + img[pixels + p], hc[2] + img[2 * pixels + p])));
    }
    mm = block_max(mm, red);

    for (int p = threadIdx.x; p < pixels; p += FRAME_THREADS) {
        const float *hc = heat + 3 * heat_level(upsampled(a, R, p / W, p % W, sh, sw), m);
        out[3 * (size_t)p + 0] = (hc[0] + img[p]) / mm;
        out[3 * (size_t)p + 1] = (hc[1] + img[pixels + p]) / mm;
        out[3 * (size_t)p + 2] = (hc[2] + img[2 * pixels + p]) / mm;
    }
}

}  // namespace

extern "C" int zs_attn_frames(const float *zmean, int batch, int n_cols, const int *frame_col, int n_frames,
                              const float *images, int H, int W, const uint8_t *lut, int R, float *frames,
                              void *stream) {
    if (batch < 0 || n_cols < 0 || n_frames < 0 || H <= 0 || W <= 0 || R < 1 || R > MAX_R) {
        zs::set_err("zs_attn_frames: bad size (batch=%d n_cols=%d n_frames=%d H=%d W=%d R=%d)", batch, n_cols,
                    n_frames, H, W, R);
        return 0;
    }
    if (batch == 0 || n_frames == 0) return 1;
    if (n_cols == 0) {
        zs::set_err("zs_attn_frames: frames requested of no columns");
        return 0;
    }
    if ((long long)H * W > 0x7fffffffLL / 3 || (long long)batch * n_frames > 0x7fffffffLL) {
        zs::set_err("zs_attn_frames: %d x %d pixels x %d x %d frames exceed one launch", H, W, batch, n_frames);
        return 0;
    }
    if (!zmean || !frame_col || !images || !lut || !frames) {
        zs::set_err("zs_attn_frames: null pointer");
        return 0;
    }
    hipLaunchKernelGGL(attn_frames_kernel, dim3(batch * n_frames), dim3(FRAME_THREADS), 0,
                       static_cast<hipStream_t>(stream), zmean, n_cols, frame_col, n_frames, images, H, W, lut, R,
                       frames);
    return zs::check_launch("zs_attn_frames") ? 1 : 0;
}
