// Prefix scans over many workgroups in two launches (shared by marching_cubes.hip and seen_mesh.hip).
// launch 1: a workgroup scans SCAN_TILE consecutive elements in place (a thread loads SCAN_ITEMS adjacent ones, so
// a wave reads one contiguous span; wave shuffles + one LDS exchange) and leaves its total in tile_tot[tile];
// launch 2: every workgroup adds the sum of the tile totals before its own (a few hundred values, summed in index
// order by each workgroup alike - deterministic) to its elements.  A single workgroup walking 10^5 elements took
// 50-240 us; this takes two launches of a few microseconds.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int SCAN_ITEMS = 8, SCAN_TILE = 256 * SCAN_ITEMS;
template <typename T>
__device__ __forceinline__ T block256_exclusive(T v, T *lds, T &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const T t = lds[w];
        if (w < wave) base += t;
        tot += t;
    }
    total = tot;
    return base + x - v;
}
// INCLUSIVE = false: data[i] <- sum of data[tile start .. i);  true: .. i]
template <typename T, bool INCLUSIVE>
__global__ __launch_bounds__(256) void scan_tiles_kernel(T *__restrict__ data, long long n, T *__restrict__ tile_tot) {
    __shared__ T lds[4];
    const long long b = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    T v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; e++) {
        v[e] = b + e < n ? data[b + e] : (T)0;
        s += v[e];
    }
    T total;
    T run = block256_exclusive<T>(s, lds, total);
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; e++) {
        if (INCLUSIVE) run += v[e];
        if (b + e < n) data[b + e] = run;
        if (!INCLUSIVE) run += v[e];
    }
    if (threadIdx.x == 0) tile_tot[blockIdx.x] = total;
}
template <typename T>
__global__ __launch_bounds__(256) void scan_offsets_kernel(T *__restrict__ data, long long n, const T *__restrict__ tile_tot,
                                                           int tiles, T *__restrict__ total_out) {
    __shared__ T lds[4];
    __shared__ T offset;
    // sum of the totals of the tiles before this one, in a fixed order: 256 strided partial sums, then the scan's tree
    T part = 0;
    for (int t = threadIdx.x; t < (int)blockIdx.x; t += 256) part += tile_tot[t];
    T total;
    (void)block256_exclusive<T>(part, lds, total);
    if (threadIdx.x == 0) offset = total;
    __syncthreads();
    const T off = offset;
    const long long b = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; e++)
        if (b + e < n) data[b + e] += off;
    if (total_out && blockIdx.x == tiles - 1 && threadIdx.x == 0) *total_out = off + tile_tot[tiles - 1];
}
inline int scan_tiles(long long n) { return (int)((n + SCAN_TILE - 1) / SCAN_TILE); }

}  // namespace
