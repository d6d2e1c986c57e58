// Split-fp16 ("f16x3") variant of the fused implicit-occupancy decoder for MI355X (gfx950).
//
// Same algorithm, same per-point dataflow and the same decoder program as csrc/sdf_decoder.hip
// (Implicit.forward, model/shape/implicit.py:251-288, hoisted latent half in the prologue), but
// every contraction runs on the 16-bit matrix pipe (v_mfma_f32_32x32x16_f16, 16x the rate of the
// fp32 MFMA) with both operands split into two fp16 halves, x ~= hi + lo:
//     A B  ~=  A_hi B_hi + A_hi B_lo + A_lo B_hi          (fp32 accumulation; A_lo B_lo dropped)
// 3 MFMAs of 32 cycles per K = 16 instead of 8 fp32 MFMAs of 64 cycles: 5.3x fewer matrix
// cycles at ~2^-22 relative operand error (fp32 itself is 1e-6 from fp64 on the seeded network; the
// same scheme on bf16 halves, same cost, measured 1.9e-5 and 10 flips; plain bf16 8e-3).  Halves
// are rounded to nearest even (v_cvt_pk_f16_f32, round 3; rounds 1-2 truncated with
// v_cvt_pkrtz_f16_f32, whose one-signed errors accumulate - csrc/zs_split16.h has the numbers):
// |x| < 65,520 keeps the full precision, far beyond what LayerNorm-ed activations and these weights
// reach (beyond it hi is inf and the result NaN); values below ~1e-4 lose relative (not absolute)
// precision to fp16 subnormals.  tests/test_gpu_decoder_split.py.
//
// What changes against the fp32 kernel, and why:
//  * The transposed chain survives: accumulator registers 8j..8j+7 of a 32x32 output tile are,
//    after a split into packed (hi, lo) fp16 pairs, exactly the B operand of K-block j of the
//    next layer.  The matching A operand of K-block j of a 32x32 weight unit is the fp32
//    program's records 8j..8j+7 of that unit, split the same way - so the split program has the
//    SAME unit order and byte size as the fp32 one and is derived from it on the device
//    (split_program_kernel), K/V records of the image included.
//  * Weight stream.  At this rate four waves streaming private copies of the 10 MB program would
//    pull ~50 TB/s through the vector memory path (64 B/clk/CU, L2 34 TB/s).  The four waves of a
//    workgroup run the same program in lock step, so each 16 KiB chunk (8 K-blocks) is staged ONCE
//    per workgroup into LDS by LDS-DMA (global_load_lds_dwordx4, two K-blocks per wave, two
//    buffers) and read back as A operands with conflict-free ds_read_b128 by all four waves.
//    One raw s_barrier per chunk (AStream below).  Ordering rules: cdna_hip_programming.md
//    section 5 (counted vmcnt by the issuing wave, then a barrier the reader has passed; restage
//    after an lgkmcnt-retired read + barrier).
//  * LDS: [params window 16 KiB][A staging 2 x 16 KiB][4 x 28 KiB activation slabs] = 160 KiB.
//    Params are paged in five windows per tile instead of two.  The slab holds the one array a
//    GEMM still re-reads from LDS as B operands per output tile: LN1's output (q, k, v), tiles
//    0..5 of it (24 of its 28 KiB; tiles 6 and 7 live in registers).  LN2's output (fc1) and both
//    activation arrays of impl_mlp stay in registers (LN2 IN REGISTERS, IMPL_MLP IN REGISTERS
//    below).
//  * No asm register ring: LDS reads and MFMAs are builtins, scheduled and hazard-padded by
//    hipcc (VGPR-form accumulators: -mllvm -amdgpu-mfma-vgpr-form, zeroshape_amd/build.py); only
//    the DMA, the barrier and the prefetch pin are asm.
//  * Activations of tile t (GELU, softplus, operand split) are fed value by value between the
//    MFMA groups of tile t+1 (software pipelines over the hidden tiles of the MLP - the split
//    program permutes those K-blocks accordingly - and over the output tiles of impl_mlp).
//  * The attention map (implicit.py:277) is only produced by the fp32 kernel.
#include "zs_common.h"
#include <stdlib.h>
#include "sdf_layout.h"
#include "sdf_math.h"
#include "zs_split16.h"
#include "sdf_query.h"
#include "../../include/zeroshape_hip.h"

#include <math.h>
#include <stdint.h>
#include <type_traits>

namespace {

using namespace zs::lay;
using namespace zs::qry;    // tile geometry, workspace layout, argument checks
using zs::dm::gelu_erf;
using zs::dm::softplus100;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr float S_GUARD = 64.0f;  // program.py: S_GUARD
constexpr int KB_U4 = 128;                          // one K-block: [hi: 64 lanes x 16 B][lo: 64 lanes x 16 B]
constexpr int CK = 8;                               // K-blocks per staged chunk: two per wave
constexpr int KPW = CK / WAVES;                     // K-blocks a wave stages per chunk
constexpr int CHUNK_BYTES = CK * KB_U4 * 16;        // 16 KiB
constexpr int NBUF = 2;
constexpr int KB_TOTAL = G_TOTAL / 2;               // 4,928 K-blocks = 14,784 MFMAs per wave tile
constexpr int PRM_WINDOW = 4096;                    // floats of params resident in LDS at a time
constexpr int STAGE_FLOATS = NBUF * CHUNK_BYTES / 4;
// IMPL_MLP IN REGISTERS (below) and LN2 IN REGISTERS leave the slab one user, LN1's output; -DZS_SPLIT_IMPL_SLAB and
// -DZS_SPLIT_LN_SLAB build the forms before them (for A/B runs of two libraries: nothing selects them at run time)
#ifndef ZS_SPLIT_IMPL_SLAB
constexpr bool IMPL_REGS = true;
#else
constexpr bool IMPL_REGS = false;
#endif
#ifndef ZS_SPLIT_LN_SLAB
constexpr bool LN2_REGS = true;
#else
constexpr bool LN2_REGS = false;
#endif
constexpr int SLAB_TILES = NT - 1;                  // tiles of an activation array the LDS has room for
constexpr int SLAB_U4 = SLAB_TILES * 4 * 64;        // ... as packed (hi, lo) K-blocks: 28 KiB per wave
// tiles actually kept there, the others in registers: with q/k/v the only reader the registers hold tile 6 as well
constexpr int SLAB_USED = IMPL_REGS && LN2_REGS ? SLAB_TILES - 1 : SLAB_TILES;
constexpr int ZTILES_F4 = NT * 4 * 64;              // one skip layer's fp32 feat partial products (workspace)
static_assert(ZSLAB_F4 == 3 * ZTILES_F4, "the workspace slab holds three skip layers' feat partial products");
static_assert(B0_TABLE_FLOATS == PRM_WINDOW, "block0_window_kernel / block0_stream_kernel index an image's table by PRM_WINDOW");
constexpr int LDS_FLOATS = PRM_WINDOW + STAGE_FLOATS + WAVES * SLAB_U4 * 4;
static_assert(LDS_FLOATS * 4 == 160 * 1024, "the kernel owns the whole LDS of a CU");
static_assert(KB_TOTAL % CK == 0 && CK % WAVES == 0 && KPW * 2048 <= 4096, "chunking");
// the stream prefetches NBUF chunks past its position: the last reads run into the zero tail of
// the records and (harmlessly) the params section behind it
static_assert((RING * GROUP_FLOATS + PARAM_FLOATS) * 4 >= NBUF * CHUNK_BYTES, "prefetch stays inside the program");

// params windows (floats, relative to the params section of the program; <= PRM_WINDOW each)
constexpr int W_PP = P_PP;                                   // point_proj table (1,024)
constexpr int W_BLK = P_BLK0;                                // + blk * P_BLK_STRIDE: one attention block (3,328)
constexpr int W_IA = P_LNFG;                                 // final norm, impl layers 0, 1, pair 0 (3,072)
constexpr int W_IB = P_IMPL_PAIR + P_IMPL_PAIR_STRIDE;       // pairs 1, 2, layer 8 (2,832)
static_assert(P_BLK_STRIDE <= PRM_WINDOW && W_IB - W_IA <= PRM_WINDOW && P_USED - W_IB <= PRM_WINDOW,
              "params windows");

#define DEV __device__ __forceinline__

// pin(ahi, alo): the prefetch reads issued above stay above (memory clobber) and the MFMAs that
// consume this K-block's A operand stay below (they read the statement's outputs).  Without it
// hipcc hoists MFMAs over the prefetch or sinks the prefetch down to its first use as soon as
// independent VALU work is around - either way the LDS latency is exposed at every K-block.
DEV void pin(u32x4 &a, u32x4 &b) { asm volatile("" : "+v"(a), "+v"(b) : : "memory"); }

// as_h / pk_f16 / split2 (x -> packed fp16 hi, lo: v_cvt_pk_f16_f32 + v_fma_mix_f32, 2 VALU per
// value) / mfma3: csrc/zs_split16.h, shared with the convolution engine
using zs::s16::mfma3;
using zs::s16::split2;

// a 32-feature x 32-point activation tile as the B operands of its two K-blocks:
// v[2 j + 0] = hi, v[2 j + 1] = lo of K-block j (accumulator registers 8 j .. 8 j + 7)
struct PT {
    u32x4 v[4];
};
template <typename T>
DEV PT pack_tile(const T &x) {
    PT p;
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            unsigned h, l;
            split2(x[8 * j + 2 * i], x[8 * j + 2 * i + 1], h, l);
            p.v[2 * j][i] = h;
            p.v[2 * j + 1][i] = l;
        }
    return p;
}

// One K-block (hi and lo halves, 2 x 64 lanes x 16 B): global -> LDS[lds_dst + 16 lane (+ 1024)].
// The instruction offset moves the global and the LDS address alike.  M0 (the LDS-DMA destination
// base) is not saved: hipcc has no use for it in this kernel (no LDS-direct, GWS, movrel or
// interpolation instructions; tools/check_split_isa.py audits the ISA for it).
DEV void glds_kblocks(const char *gsrc, unsigned lds_dst) {  // this wave's two K-blocks of a chunk
#ifdef ZS_EXP_NO_DMA   // energy ablation (tools/energy_ablation.sh): results are garbage, the timing is the point
    if (gsrc != nullptr) return;
#endif
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
                 "\n\tglobal_load_lds_dwordx4 %0, off offset:1024"
                 "\n\tglobal_load_lds_dwordx4 %0, off offset:2048"
                 "\n\tglobal_load_lds_dwordx4 %0, off offset:3072"
                 :
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}

// ---- weight stream: LDS-DMA staged chunks shared by the four waves ------------------ //
// Two buffers of 8 K-blocks: while chunk c is consumed, chunk c+1 lands.  One synchronisation per
// chunk, before its LAST K-block is multiplied (that K-block's A operand is already in registers):
// own share of chunk c+1 landed (vmcnt) and own reads of chunk c retired (lgkmcnt) -> s_barrier ->
// chunk c+2 is staged into the buffer just freed and the first A read of chunk c+1 is issued.
// Lead time of a chunk: one chunk period = 8 K-blocks.
// tools/ubench/mfma_f16_stream.hip prices the pieces (cycles per K-block of 3 MFMAs, one wave
// per SIMD, all CUs busy, 4-K-block chunks): MFMAs alone 96.1; + two ds_read_b128 105.5; + the
// barrier every four K-blocks 124.1 (~74 cycles per barrier: the skew of four waves); + the
// LDS-DMA 131.6; + two more ds_read_b128 for B operands from the slab 146.9.
// Measured alternatives on the whole kernel (129^3 grid): 4-K-block chunks: two buffers (lead 4
// K-blocks) +6 ms - the DMA latency is exposed at every barrier - three buffers the baseline of
// the 8-K-block version; register staging (global_load -> ds_write_b128 behind the barrier) +3
// ms; the DMAs moved from behind the barrier into the shadows of the first MFMAs of the chunk
// +0.5 ms; reads two K-blocks ahead +0.6 ms; two alternating accumulator chains +2 ms (extra
// adds; a single chain already issues back to back).
struct AStream {
    const u32x4 *buf[NBUF];   // this lane's view of the buffers, buf[0] = chunk being consumed
    unsigned dst[NBUF];       // LDS byte address of this wave's K-blocks in each (wave-uniform)
    u32x4 hi, lo;             // A operand of the next K-block (read in flight)
    const char *gsrc;         // this lane's source of this wave's K-blocks of the next chunk to stage

    DEV void init(const char *prog, u32x4 *stage, unsigned stage_addr, int wave, int lane) {
        const char *g = prog + wave * (KPW * KB_U4 * 16) + lane * 16;
        // the previous tile's reads and DMAs are retired in every wave before the buffers are reused
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int i = 0; i < NBUF; i++) {
            buf[i] = stage + i * (CK * KB_U4) + lane;
            dst[i] = stage_addr + i * CHUNK_BYTES + wave * (KPW * KB_U4 * 16);
            glds_kblocks(g + i * CHUNK_BYTES, dst[i]);
        }
        gsrc = g + NBUF * CHUNK_BYTES;
        asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");  // chunk 0 landed everywhere
        hi = buf[0][0];
        lo = buf[0][64];
    }
    // A operand of the K-block at position `pos` (0..7) of the current chunk; issues the read of
    // the next.  EXTRA_VM: vector-memory loads the caller has issued since the previous
    // synchronisation and does not need yet (they are younger than the DMAs waited for here:
    // the counted wait lets them stay in flight).
    template <int EXTRA_VM = 0>
    DEV void step(int pos, u32x4 &ahi, u32x4 &alo) {
        ahi = hi;
        alo = lo;
        if (pos == CK - 1) {
            static_assert(EXTRA_VM == 0 || EXTRA_VM == 4, "wait-count variants");
            if (EXTRA_VM == 4)
                asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            glds_kblocks(gsrc, dst[0]);
            gsrc += CHUNK_BYTES;
            const u32x4 *t = buf[0];
            const unsigned u = dst[0];
            buf[0] = buf[1];
            dst[0] = dst[1];
            buf[1] = t;
            dst[1] = u;
            hi = buf[0][0];
            lo = buf[0][64];
        } else {
#ifndef ZS_EXP_NO_AREAD   // energy ablation: one A read per chunk instead of eight
            hi = buf[0][(pos + 1) * KB_U4];
            lo = buf[0][(pos + 1) * KB_U4 + 64];
#endif
        }
    }
    // This wave's NEXT staged chunk comes from `base` (chunk-aligned in its own stream): block 0's compact stream hands over
    // to the program (BLOCK 0 STREAM below).  Only gsrc moves - nothing is in flight to it - so the buffers, the barriers and
    // the counted waits are untouched.
    DEV void seek(const char *base, int wave, int lane) { gsrc = base + wave * (KPW * KB_U4 * 16) + lane * 16; }
    DEV void drain() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }
};

// The LDS-resident activation array of a wave: tiles 0..SLAB_USED-1 in the slab, the others in registers (tile 7's
// 4 KiB per wave are what lets the staging buffers hold 8 K-blocks, i.e. half the barriers).
struct Slab {
    u32x4 *fl;  // this lane's view: [(tile * 4 + j * 2 + hl) * 64]
    PT tr[NT - SLAB_USED];
    DEV void store(int tile, const PT &p) {
        if (tile >= SLAB_USED) {
            tr[tile - SLAB_USED] = p;
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) fl[(tile * 4 + q) * 64] = p.v[q];
        }
    }
};

// One K-block = zs::s16::mfma3: three dependent MFMAs on one accumulator.  A dependent
// v_mfma_f32_32x32x16_f16 issues 32 cycles behind its producer (tools/ubench/mfma_f16_stream.hip:
// one chain and two alternating chains both run 96.1 cycles per K-block), so a second chain buys
// nothing.
DEV f32x16 zero16() {
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; r++) v[r] = 0.f;
    return v;
}

// ---- side work in the dependency gaps ---------------------------------------------------- //
// The three MFMAs of a K-block form a dependent chain (one accumulator): the 2nd and 3rd each wait
// ~32 cycles for their predecessor, and an in-order wave issues NOTHING behind a waiting MFMA.
// hipcc keeps source order (MFMA MFMA MFMA, then the activation code), so round 1's side work ran
// with only the third MFMA in flight.  tools/ubench/mfma_valu_place.hip (cycles per K-block, ideal
// 96): 12 plain VALU behind the three MFMAs 126.6, the same 12 as 4 + 4 + 4 in the gaps 101.6;
// 18: 138.6 vs 113.1; but 24: 157 either way, and a transcendental shares a gap with at most one
// plain instruction (exp + 1: 99.6; exp + 2: 124.6; exp + 3: 135-156).  Hence: side(kb, g) is
// called behind the g-th MFMA of K-block kb (source order, which hipcc keeps here; fencing it
// in with sched_barrier(0) spilled: kblock_gelu below), and the activations are cut into
// gap-sized stages (GeluStager, SoftplusStager below).
struct NoSide {
    DEV void operator()(int, int) const {}
};
template <typename SIDE>
DEV void mfma3_gaps(f32x16 &acc, const u32x4 &ahi, const u32x4 &alo, const u32x4 &bhi, const u32x4 &blo, int kb,
                    SIDE &side) {
    using zs::s16::as_h;
    if (std::is_same<SIDE, NoSide>::value) {   // nothing to place: leave the three MFMAs to hipcc
        mfma3(acc, ahi, alo, bhi, blo);
        return;
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h(alo), as_h(bhi), acc, 0, 0, 0);
    side(kb, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h(ahi), as_h(blo), acc, 0, 0, 0);
    side(kb, 1);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h(ahi), as_h(bhi), acc, 0, 0, 0);
    side(kb, 2);
}

// Collects the split B operands of an activation tile, one value at a time (index 0..15)
struct TilePacker {
    PT p;
    float prev;
    DEV void feed(int kb, float v) {
        if (kb & 1) {
            unsigned h, l;
            split2(prev, v, h, l);
            p.v[2 * (kb >> 3)][(kb & 7) >> 1] = h;
            p.v[2 * (kb >> 3) + 1][(kb & 7) >> 1] = l;
        }
        prev = v;
    }
};

// zs::dm::gelu_erf (same operations in the same order: bit-identical) cut into five stages:
// 3 plain | 1 plain + rcp | exp + 1 plain | 5 plain | 2 plain
struct GeluStager {
    float x, u, q, t, e, p;
    DEV void s0(float v) {
        x = v;
        u = fabsf(v) * 0.70710678118654752440f;
        q = (u * u) * -1.44269504088896340736f;
    }
    DEV void s1() { t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, u, 1.0f)); }
    DEV void s2() {
        e = __builtin_amdgcn_exp2f(q);
        p = fmaf(0.75052702f, t, -1.02753365f);
    }
    DEV void s3() {
        p = fmaf(p, t, 1.00509130f);
        p = fmaf(p, t, -0.20116957f);
        p = fmaf(p, t, 0.18019173f);
        p = p * t;
        u = u * p;
    }
    DEV float s4() const { return fmaf(-u, e, fmaxf(x, 0.0f)); }
    DEV float all(float v) {
        s0(v); s1(); s2(); s3();
        return s4();
    }
    // stage st (0..5; 5 = idle) of value `v`; the finished value goes to e.feed(idx, .)
    DEV void stage(int st, float v, int idx, TilePacker &pk) {
        if (st == 0) s0(v);
        else if (st == 1) s1();
        else if (st == 2) s2();
        else if (st == 3) s3();
        else if (st == 4) pk.feed(idx, s4());
    }
};
// zs::dm::softplus100 in three stages: 1 plain + exp | 1 plain + log | 2 plain
struct SoftplusStager {
    float x, t;
    DEV void s0(float v) {
        x = v;
        t = __builtin_amdgcn_exp2f(fabsf(v) * -144.26950408889634074f);
    }
    DEV void s1() { t = __builtin_amdgcn_logf(1.0f + t); }
    DEV float s2() const { return fmaf(t, 0.0069314718055994530942f, fmaxf(x, 0.0f)); }
};

// K-blocks with the activation of ONE value written into the dependency gaps by hand (inline asm:
// hipcc neither places side work there by itself nor survives being fenced into it - register
// spills, and its AGPR-copy rewrite pass crashes).  Same operations in the same order as
// zs::dm::gelu_erf / softplus100: bit-identical results.  The A / B operands are ordinary asm inputs
// (hipcc waits for their LDS reads in front of the statement); the VALU part touches no MFMA operand.
// gelu: 4 plain | rcp, exp, 1 plain | 7 plain
// (BREG: where the B operands live - "v", or "a" for an array pinned in the accumulator half; LEAD: that form's leading
// s_nop, see mfma3_breg below)
#ifndef ZS_EXP_TWO_TERM
#define ZS_KBLOCK_MFMA_LO_HI "v_mfma_f32_32x32x16_f16 %[acc], %[alo], %[bh], %[acc]\n\t"
#else
#define ZS_KBLOCK_MFMA_LO_HI
#endif
#define ZS_KBLOCK_GELU(NAME, BREG, LEAD) \
DEV float NAME(f32x16 &acc, const u32x4 &ahi, const u32x4 &alo, const u32x4 &bhi, const u32x4 &blo, float x) {             \
    float u, q, d, t, e, m, p;                                                                                             \
    const float c0 = 0.70710678118654752440f, c1 = 0.3275911f, c2 = -1.02753365f;                                          \
    asm volatile(                                                                                                          \
                 LEAD ZS_KBLOCK_MFMA_LO_HI                                                                                 \
                 "v_mul_f32_e64 %[u], |%[x]|, %[c0]\n\t"                                                                   \
                 "v_mul_f32_e32 %[q], %[u], %[u]\n\t"                                                                      \
                 "v_mul_f32_e32 %[q], 0xbfb8aa3b, %[q]\n\t"                                                                \
                 "v_fma_f32 %[d], %[u], %[c1], 1.0\n\t"                                                                    \
                 "v_mfma_f32_32x32x16_f16 %[acc], %[ahi], %[bl], %[acc]\n\t"                                               \
                 "v_rcp_f32_e32 %[t], %[d]\n\t"                                                                            \
                 "v_exp_f32_e32 %[e], %[q]\n\t"                                                                            \
                 "v_max_f32_e32 %[m], 0, %[x]\n\t"                                                                         \
                 "v_mfma_f32_32x32x16_f16 %[acc], %[ahi], %[bh], %[acc]\n\t"                                               \
                 "v_fmamk_f32 %[p], %[t], 0x3f40228a, %[c2]\n\t"                                                           \
                 "v_fmaak_f32 %[p], %[p], %[t], 0x3f80a6d5\n\t"                                                            \
                 "v_fmaak_f32 %[p], %[p], %[t], 0xbe4dff65\n\t"                                                            \
                 "v_fmaak_f32 %[p], %[p], %[t], 0x3e38842e\n\t"                                                            \
                 "v_mul_f32_e64 %[p], %[t], -%[p]\n\t"                                                                     \
                 "v_mul_f32_e32 %[p], %[u], %[p]\n\t"                                                                      \
                 "v_fmac_f32_e32 %[m], %[p], %[e]"                                                                         \
                 : [acc] "+v"(acc), [u] "=&v"(u), [q] "=&v"(q), [d] "=&v"(d), [t] "=&v"(t), [e] "=&v"(e), [m] "=&v"(m),    \
                   [p] "=&v"(p)                                                                                            \
                 : [alo] "v"(alo), [ahi] "v"(ahi), [bh] BREG(bhi), [bl] BREG(blo), [x] "v"(x), [c0] "s"(c0), [c1] "s"(c1), \
                   [c2] "v"(c2));                                                                                          \
    return m;                                                                                                              \
}
ZS_KBLOCK_GELU(kblock_gelu, "v", "")
ZS_KBLOCK_GELU(kblock_gelu_breg, "a", "s_nop 1\n\t")
#undef ZS_KBLOCK_GELU
// softplus100: 1 plain + exp | 2 plain + log | 1 plain
#define ZS_KBLOCK_SOFTPLUS(NAME, BREG, LEAD) \
DEV float NAME(f32x16 &acc, const u32x4 &ahi, const u32x4 &alo, const u32x4 &bhi, const u32x4 &blo, float x) {             \
    float t, m;                                                                                                            \
    const float c0 = -144.26950408889634074f;                                                                              \
    asm volatile(                                                                                                          \
                 LEAD ZS_KBLOCK_MFMA_LO_HI                                                                                 \
                 "v_mul_f32_e64 %[t], |%[x]|, %[c0]\n\t"                                                                   \
                 "v_exp_f32_e32 %[t], %[t]\n\t"                                                                            \
                 "v_mfma_f32_32x32x16_f16 %[acc], %[ahi], %[bl], %[acc]\n\t"                                               \
                 "v_max_f32_e32 %[m], 0, %[x]\n\t"                                                                         \
                 "v_add_f32_e32 %[t], 1.0, %[t]\n\t"                                                                       \
                 "v_log_f32_e32 %[t], %[t]\n\t"                                                                            \
                 "v_mfma_f32_32x32x16_f16 %[acc], %[ahi], %[bh], %[acc]\n\t"                                               \
                 "s_nop 0\n\t"                                                                                             \
                 "v_fmac_f32_e32 %[m], 0x3be32166, %[t]"                                                                   \
                 : [acc] "+v"(acc), [t] "=&v"(t), [m] "=&v"(m)                                                             \
                 : [alo] "v"(alo), [ahi] "v"(ahi), [bh] BREG(bhi), [bl] BREG(blo), [x] "v"(x), [c0] "s"(c0));              \
    return m;                                                                                                              \
}
ZS_KBLOCK_SOFTPLUS(kblock_softplus, "v", "")
ZS_KBLOCK_SOFTPLUS(kblock_softplus_breg, "a", "s_nop 1\n\t")
#undef ZS_KBLOCK_SOFTPLUS
#undef ZS_KBLOCK_MFMA_LO_HI

// The asm K-blocks hide their MFMAs from hipcc, which therefore pads no wait states between the last of them and a VALU
// read of the accumulator (the result of an 8-pass MFMA may be read 12 wait states after its issue; hipcc placed such a
// read 4 behind it).  Called in front of every VALU read of a tile that follows the asm GEMM that produced it by fewer
// instructions than that: the plain-C++ activation of the last output tile of each impl_mlp layer, and in the skip layers
// every hand-over of tile nt to the activation carried by tile nt + 1's first K-block (only three LDS reads, a wait and one
// independent MFMA lie between).  Everywhere else the distance is structural: the hand-overs of the plain layers and of
// layer 0 have the previous K-block's own tail (7+ VALU instructions behind its last MFMA, inside the same asm statement)
// plus the next step's reads in front of the read; the MLP's GELU hand-over has 16 K-blocks of fc2 in between.
DEV void mfma_settle(f32x16 &acc) { asm volatile("s_nop 7\n\ts_nop 3" : "+v"(acc)); }

// acc += W_tile X, X = KT packed tiles in registers; starts at a chunk boundary.
// SIDE: side(kb, g) runs behind the g-th MFMA of K-block kb
template <int KT, int EXTRA_VM = 0, typename SIDE = NoSide>
DEV void gemm_reg(AStream &s, const PT *X, f32x16 &acc, SIDE side = SIDE()) {  // starts chunk-aligned
#pragma unroll
    for (int kt = 0; kt < KT; kt++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            u32x4 ahi, alo;
            s.step((kt * 2 + j) & (CK - 1), ahi, alo);
            pin(ahi, alo);
            mfma3_gaps(acc, ahi, alo, X[kt].v[2 * j], X[kt].v[2 * j + 1], kt * 2 + j, side);
        }
}
// ... with X pinned in the ACCUMULATOR half of the register file (B operands of an MFMA may be AGPRs).
// For an array that lives through a whole phase and is only ever a B operand - feat / sqrt(2) in
// impl_mlp - this tells hipcc where it belongs: left to itself it shuffled such arrays between the
// two halves (hundreds of v_accvgpr moves per phase) and spilled.  Hazards hipcc does not pad for
// asm: the A operands arrive through its own s_waitcnt (they are asm inputs), the leading s_nop
// covers a VALU write of the accumulator just before the statement.
template <typename SIDE>
DEV void mfma3_breg(f32x16 &acc, const u32x4 &ahi, const u32x4 &alo, const u32x4 &bhi, const u32x4 &blo, int kb,
                    SIDE &side) {
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(alo), "a"(bhi));
    side(kb, 0);
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(ahi), "a"(blo));
    side(kb, 1);
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(ahi), "a"(bhi));
    side(kb, 2);
}
// VT: tiles 0..VT-1 of X are NOT pinned there - hipcc keeps them where it likes, the MFMAs take them from VGPRs
// (impl_mlp's second array: the accumulator half has no room for all of it, IMPL_MLP IN REGISTERS below)
template <int KT, int VT = 0, typename SIDE = NoSide>
DEV void gemm_areg(AStream &s, const PT *X, f32x16 &acc, SIDE side = SIDE()) {  // starts chunk-aligned
#pragma unroll
    for (int kt = 0; kt < KT; kt++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            u32x4 ahi, alo;
            s.step((kt * 2 + j) & (CK - 1), ahi, alo);
            pin(ahi, alo);
            if (kt < VT)
                mfma3_gaps(acc, ahi, alo, X[kt].v[2 * j], X[kt].v[2 * j + 1], kt * 2 + j, side);
            else
                mfma3_breg(acc, ahi, alo, X[kt].v[2 * j], X[kt].v[2 * j + 1], kt * 2 + j, side);
        }
}
// ... with the ACCUMULATOR pinned in the accumulator half of the register file: the residual stream
// y (128 registers, only ever updated by MFMAs and read by the LayerNorms) belongs there.  Left to
// hipcc (-amdgpu-mfma-vgpr-form) every update of a y tile moved it to VGPRs and back, and with
// side work between those MFMAs its "Rewrite AGPR-Copy-MFMA" pass crashes (ROCm 7.2).
template <typename SIDE>
DEV void mfma3_cacc(f32x16 &acc, const u32x4 &ahi, const u32x4 &alo, const u32x4 &bhi, const u32x4 &blo, int kb,
                    SIDE &side) {
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(alo), "v"(bhi));
    side(kb, 0);
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(ahi), "v"(blo));
    side(kb, 1);
    asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(ahi), "v"(bhi));
    side(kb, 2);
}
// one input tile (2 K-blocks) starting at chunk position pos0 (even); side sees K-blocks kb0, kb0 + 1.
// YACC: acc is a tile of the residual stream (AGPR-resident, see mfma3_cacc)
// NKB = 1: only the tile's first K-block (registers 0..7 of the input tile)
template <bool YACC = false, typename SIDE = NoSide, int NKB = 2>
DEV void gemm_one(AStream &s, const PT &X, f32x16 &acc, int pos0, int kb0 = 0, SIDE side = SIDE()) {
#pragma unroll
    for (int j = 0; j < NKB; j++) {
        u32x4 ahi, alo;
        s.step((pos0 + j) & (CK - 1), ahi, alo);
        pin(ahi, alo);
        if (YACC)
            mfma3_cacc(acc, ahi, alo, X.v[2 * j], X.v[2 * j + 1], kb0 + j, side);
        else
            mfma3_gaps(acc, ahi, alo, X.v[2 * j], X.v[2 * j + 1], kb0 + j, side);
    }
}
// 8 input tiles with the B operands read from the wave's LDS slab ([k-block][hi | lo][lane]),
// one K-block ahead of their use
// B operand of K-block kb of the slab-resident array (tiles SLAB_USED.. live in registers)
DEV void slab_b(const Slab &sl, int kb, u32x4 &bh, u32x4 &bl) {
    if (kb >= SLAB_USED * 2) {
        bh = sl.tr[(kb >> 1) - SLAB_USED].v[(kb & 1) * 2];
        bl = sl.tr[(kb >> 1) - SLAB_USED].v[(kb & 1) * 2 + 1];
    } else {
        bh = sl.fl[kb * KB_U4];
        bl = sl.fl[kb * KB_U4 + 64];
    }
}
// pos0: chunk position of the first K-block (0 or 4: a head consumes 92 K-blocks)
template <typename SIDE = NoSide>
DEV void gemm_lds(AStream &s, const Slab &sl, f32x16 &acc, int pos0 = 0, SIDE side = SIDE()) {
    u32x4 bh, bl;
    slab_b(sl, 0, bh, bl);
#pragma unroll
    for (int kb = 0; kb < NT * 2; kb++) {
        u32x4 ahi, alo;
        s.step((pos0 + kb) & (CK - 1), ahi, alo);
        u32x4 nh = bh, nl = bl;
        if (kb + 1 < NT * 2) slab_b(sl, kb + 1, nh, nl);  // after the step: its lgkmcnt(0) must not wait for this read
        pin(ahi, alo);
        mfma3_gaps(acc, ahi, alo, bh, bl, kb, side);
        bh = nh;
        bl = nl;
    }
}

// gemm_lds / gemm_reg with the activation ACT (0 gelu, 1 softplus100) of cur[kb] computed in the gaps of
// K-block kb (kblock_* above); fin(kb, value) receives the result, tail(kb) runs behind the K-block
template <int ACT, typename FIN, typename TAIL>
DEV void gemm_lds_act(AStream &s, const Slab &sl, f32x16 &acc, const f32x16 &cur, FIN fin, TAIL tail) {
    u32x4 bh, bl;
    slab_b(sl, 0, bh, bl);
#pragma unroll
    for (int kb = 0; kb < NT * 2; kb++) {
        u32x4 ahi, alo;
        s.step(kb & (CK - 1), ahi, alo);
        u32x4 nh = bh, nl = bl;
        if (kb + 1 < NT * 2) slab_b(sl, kb + 1, nh, nl);
        const float r = ACT == 0 ? kblock_gelu(acc, ahi, alo, bh, bl, cur[kb]) : kblock_softplus(acc, ahi, alo, bh, bl, cur[kb]);
        bh = nh;
        bl = nl;
        fin(kb, r);
        tail(kb);
    }
}
template <int ACT, typename FIN, typename TAIL>
DEV void gemm_reg_act(AStream &s, const PT *X, f32x16 &acc, const f32x16 &cur, FIN fin, TAIL tail) {
#pragma unroll
    for (int kt = 0; kt < NT; kt++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            u32x4 ahi, alo;
            const int kb = kt * 2 + j;
            s.step(kb & (CK - 1), ahi, alo);
            const float r = ACT == 0 ? kblock_gelu(acc, ahi, alo, X[kt].v[2 * j], X[kt].v[2 * j + 1], cur[kb])
                                     : kblock_softplus(acc, ahi, alo, X[kt].v[2 * j], X[kt].v[2 * j + 1], cur[kb]);
            fin(kb, r);
            tail(kb);
        }
}
// gemm_areg with the activation ACT of cur[kb] in the gaps of K-block kb
template <int ACT, int VT = 0, typename FIN, typename TAIL>
DEV void gemm_areg_act(AStream &s, const PT *X, f32x16 &acc, const f32x16 &cur, FIN fin, TAIL tail) {
#pragma unroll
    for (int kt = 0; kt < NT; kt++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            u32x4 ahi, alo;
            const int kb = kt * 2 + j;
            s.step(kb & (CK - 1), ahi, alo);
            const u32x4 &bh = X[kt].v[2 * j], &bl = X[kt].v[2 * j + 1];
            const float r = kt < VT ? (ACT == 0 ? kblock_gelu(acc, ahi, alo, bh, bl, cur[kb]) : kblock_softplus(acc, ahi, alo, bh, bl, cur[kb]))
                                    : (ACT == 0 ? kblock_gelu_breg(acc, ahi, alo, bh, bl, cur[kb])
                                                : kblock_softplus_breg(acc, ahi, alo, bh, bl, cur[kb]));
            fin(kb, r);
            tail(kb);
        }
}

// Sum / maximum of a value over the two lane halves of a point (lanes l and l ^ 32), on every lane:
// __shfl_xor(v, 32) = ds_bpermute, a ~150-cycle LDS round trip exposed on a lone wave, 60-70 times per wave tile.
// gfx950 has v_permlane32_swap: with two copies (a, b) of v it leaves a = [lo | lo], b = [hi | hi], so the sum is a + b
// without LDS.  Round 2 measured 1.2 % of the cycles for it and could not make it correct; round 3 pinned it down
// (tools/ubench/permlane_check.hip, 4 M lanes per form; tools/ab_permlane.py, tools/race_screen_split.py):
//   * __builtin_amdgcn_permlane32_swap is MISCOMPILED by this hipcc (ROCm 7.2): the generated code adds the first
//     result to itself (r[0] + r[0]) - every lane wrong, with or without wait states in front.  That is round 2's
//     "upper halves come back un-swapped";
//   * the asm form with `s_nop 4` on both sides (operands are two fresh v_mov copies, which hipcc pads against MFMA
//     results itself) is correct in isolation - 0 mismatches for VALU- and MFMA-produced values - and inside this kernel
//     the full grid stays 3.46e-6 from the fp32 kernel, the same maximum as the LDS form.  But identical launches are
//     then no longer BIT-reproducible: 0.6 % of the values differ in their last bits from run to run (40 repeats, 1.1 M
//     of 172 M values; also with only the sums switched over), where the LDS form differs in none.  The cause is not
//     identified (suspect: the swap issued under an MFMA that is still in flight); a fused decoder whose occupancy
//     indices are a parity contract cannot ship that.
//   * the gain it would buy: 28.66 vs 28.80 ms per grid (0.5 %) - the kernel's time is its energy.
// So the LDS form stays; -DZS_SPLIT_PERMLANE builds the asm form for whoever continues (ZS_SPLIT_PERMLANE_SUM_ONLY: sums only).
#ifndef ZS_SPLIT_PERMLANE
DEV float half_sum(float v) { return v + __shfl_xor(v, 32, 64); }
DEV float half_max(float v) { return fmaxf(v, __shfl_xor(v, 32, 64)); }
#else
DEV void half_pair(float v, float &lo, float &hi) {
    lo = v;
    hi = v;
    asm volatile("s_nop 4\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 4" : "+v"(lo), "+v"(hi));
}
DEV float half_sum(float v) {
    float lo, hi;
    half_pair(v, lo, hi);
    return lo + hi;
}
#ifdef ZS_SPLIT_PERMLANE_SUM_ONLY
DEV float half_max(float v) { return fmaxf(v, __shfl_xor(v, 32, 64)); }
#else
DEV float half_max(float v) {
    float lo, hi;
    half_pair(v, lo, hi);
    return fmaxf(lo, hi);
}
#endif
#endif

// row-param read from LDS: 16 floats for (tile, lane half)
DEV void rp(const float *prm, int off, int tile, int hi, float *v) {
    const f32x4 *q = reinterpret_cast<const f32x4 *>(prm + off + tile * 32 + hi * 16);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const f32x4 a = q[i];
        v[4 * i + 0] = a.x; v[4 * i + 1] = a.y; v[4 * i + 2] = a.z; v[4 * i + 3] = a.w;
    }
}
DEV f32x16 rp16(const float *prm, int off, int tile, int hi) {
    float t[16];
    rp(prm, off, tile, hi, t);
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; r++) v[r] = t[r];
    return v;
}
// BLOCK 0 TABLE.  Block 0's point row is pf = point_proj(xyz) = A p~ with p~ = (x, y, z, 1), so
//     LN1(pf) = rstd g (A - 1 m) p~ + b          (m: column mean of A; rstd: the point's scalar from ln_stats)
//     qkv     = rstd (T p~) + c,   T = Wqkv diag(g) (A - 1 m)  [768 x 4],   c = Wqkv b + bqkv
// for all 768 q/k/v rows of block 0.  T and c depend on the weights only (block0_window_kernel writes them in front of every
// launch).  The decode kernel does not read the table itself: block0_stream_kernel builds the compact stream's operands
// from it (BLOCK 0 STREAM below).
// Layout (floats): [b_proj 256][c 768, row-param order][T 3,072, [tile][hi][r][4]], tile = 3 head + {q, k, v}.
constexpr int B0_BPROJ = 0, B0_C = 256, B0_T = 1024;
static_assert(B0_T + HEADS * 3 * 128 == PRM_WINDOW, "the block-0 table is exactly one params window");
// BLOCK 0 STREAM.  With the table, q_h = rstd (T_q p~) + c_q is affine in u = (rstd x, rstd y, rstd z, rstd, 1), so the
// 224 latent logits of a head are S_h = U_h u, U_h = c K_h [T_q,h | c_q,h] (224 x 5; c = 32^-1/2 log2 e folded in: S comes
// out in the log2 domain), and q, k, v are [T | c] u.  A rank-5 contraction with both operands split is 15 products per
// output - the K = 16 of ONE MFMA on packed operands (lane l holds k = 8 (l >> 5) + e; xh = fp16(x), xl = fp16(s (x - xh)),
// xd = fp16(xh / s), s = B0S_LO_SCALE: remainders scaled out of fp16's subnormals, the power of two taken back by the hi
// copy they meet - zeroshape_amd/program.py has the numbers):
//     A, 32 rows x 16 (1 KiB)    lanes  0-31: [Uh0 Uh1 Uh2 Uh3 | Ud0 Ud1 Ud2 Ud3]   lanes 32-63: [Ul0 Ul1 Ul2 Ul3 | Uh4 Ud4 Ul4 0]
//     B, 16 x 32 points           lanes  0-31: [uh0 uh1 uh2 uh3 | ul0 ul1 ul2 ul3]   lanes 32-63: [ud0 ud1 ud2 ud3 | uh4 ul4 ud4 0]
// B is the same for every operand of a wave tile (rank5_b, once per tile).  block0_stream_kernel writes, per image and in
// front of every launch, a stream of block 0's own: per head 34 K-block slots in consumption order -
//     [q|k] [v|U0] V0 V0 [U1|U2] V1 V1 V2 V2 [U3|U4] V3 V3 V4 V4 [U5|U6] V5 V5 V6 proj x 16
// ([a|b]: packed operand a in the slot's hi half, b in its lo half, one MFMA each; V / proj: copies of the program's
// K-blocks; latent tile 6 has one V K-block: its second multiplies rows 208-223, all masked) - 97 MFMAs per head instead of
// 132, 8 x 34 = 272 slots = 34 whole chunks.  A head starts at chunk position 0, 2, 4, 6 in turn (34 = 4 chunks + 2).  Head
// 7's proj K-blocks are the stream's last two chunks; in front of them every wave's source moves to the program's K-block
// 736 (AStream::seek), where block 0's MLP section starts.  4,464 slots, 13,352 MFMAs per wave tile; the program itself is
// untouched (tests/test_block0_stream.py replays the schedule).
constexpr float B0S_LO_SCALE = 64.0f;             // program.py: B0S_LO_SCALE
constexpr int B0S_KB_HEAD = 34;
static_assert(B0_STREAM_KB == HEADS * B0S_KB_HEAD && B0_STREAM_KB % CK == 0 && B0_STREAM_BYTES == (size_t)B0_STREAM_KB * KB_U4 * 16,
              "the compact stream is whole chunks");
static_assert(B0S_KB_HEAD == 5 + (2 * LT - 1) + 2 * NT && L - 32 * (LT - 1) <= 16, "latent tile 6: rows 16-31 are padding");
// x - fp16 half of h: one v_fma_mix_f32, exact (as in zs::s16::split2)
DEV void rem2(unsigned h, float a, float b, float &ra, float &rb) {
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(h), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(h), "v"(b));
}
// the B operand of a wave tile's rank-5 MFMAs from u = (u0, u1, u2, u3, 1); bad: a component beyond the fp16 range (or not
// finite) - the tile is flagged for the fp32 re-evaluation like one outside the envelope (integer test: NaN-proof)
DEV u32x4 rank5_b(float u0, float u1, float u2, float u3, int hi, bool &bad) {
    using zs::s16::pk_f16;
    const unsigned lim = 0x477fe000u;  // 65504.0f
    bad = (__builtin_bit_cast(unsigned, u0) & 0x7fffffffu) > lim || (__builtin_bit_cast(unsigned, u1) & 0x7fffffffu) > lim ||
          (__builtin_bit_cast(unsigned, u2) & 0x7fffffffu) > lim || (__builtin_bit_cast(unsigned, u3) & 0x7fffffffu) > lim;
    const unsigned h01 = pk_f16(u0, u1), h23 = pk_f16(u2, u3);
    float r0, r1, r2, r3;
    rem2(h01, u0, u1, r0, r1);
    rem2(h23, u2, u3, r2, r3);
    const float s = B0S_LO_SCALE, is = 1.0f / B0S_LO_SCALE;
    const unsigned l01 = pk_f16(r0 * s, r1 * s), l23 = pk_f16(r2 * s, r3 * s);
    const unsigned d01 = pk_f16((u0 - r0) * is, (u1 - r1) * is), d23 = pk_f16((u2 - r2) * is, (u3 - r3) * is);   // u - r = uh exactly
    // u4 = 1: uh4 = 1 (0x3c00), ul4 = 0, ud4 = 2^-6 (0x2400)
    static_assert(B0S_LO_SCALE == 64.0f, "ud4's bit pattern");
    return hi ? u32x4{d01, d23, 0x00003c00u, 0x00002400u} : u32x4{h01, h23, l01, l23};
}
DEV f32x16 mfma_rank5(const u32x4 &a, const u32x4 &ub) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(zs::s16::as_h(a), zs::s16::as_h(ub), zero16(), 0, 0, 0);
}

// w.w + w.x*x + w.y*y + w.z*z for the 16 registers of (tile, hi): [tile][hi][r][4] table
DEV f32x16 xyz_affine(const float *prm, int off, int tile, int hi, float x, float y, float z) {
    const f32x4 *q = reinterpret_cast<const f32x4 *>(prm + off + tile * 128 + hi * 64);
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const f32x4 w = q[r];
        v[r] = fmaf(w.z, z, fmaf(w.y, y, fmaf(w.x, x, w.w)));
    }
    return v;
}

// Accumulator initialisers of the NEXT output tile, produced one step per K-block beside the current
// tile's GEMM (gemm side work).  A wave alone on its SIMD has nobody to hide an LDS round trip
// behind, and hipcc cannot hoist these reads over the stream's asm statements: the read of step
// r + 1 is issued in step r, ~100 cycles before its use.  (Round 1 read the whole table in front of
// every tile: 16 serialised round trips, ~1,000 cycles per tile with the matrix pipe idle.)
struct XyzInit {  // w.w + w.x x + w.y y + w.z z for the 16 registers of (tile, hi): [tile][hi][r][4] table
    const f32x4 *q;
    f32x4 w;
    f32x16 v;
    DEV void start(const float *prm, int off, int tile, int hi) {
        q = reinterpret_cast<const f32x4 *>(prm + off + tile * 128 + hi * 64);
        w = q[0];
    }
    DEV void step(int r, float x, float y, float z) {
        v[r] = fmaf(w.z, z, fmaf(w.y, y, fmaf(w.x, x, w.w)));
        if (r + 1 < 16) w = q[r + 1];
    }
};
struct RowInit {  // 16 floats of a row-param vector (bias) for (tile, hi)
    const f32x4 *q;
    f32x4 w;
    f32x16 v;
    DEV void start(const float *prm, int off, int tile, int hi) {
        q = reinterpret_cast<const f32x4 *>(prm + off + tile * 32 + hi * 16);
        w = q[0];
    }
    DEV void step(int r) {
        if ((r & 3) == 0) {
            v[r] = w.x; v[r + 1] = w.y; v[r + 2] = w.z; v[r + 3] = w.w;
            if (r + 4 < 16) w = q[(r >> 2) + 1];
        }
    }
};

DEV void ln_stats(const f32x16 *x, float &mean, float &rstd) {
    float s = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; kt++)
#pragma unroll
        for (int r = 0; r < 16; r++) s += x[kt][r];
    s = half_sum(s);
    mean = s * (1.0f / 256.0f);
    float v = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; kt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float d = x[kt][r] - mean;
            v = fmaf(d, d, v);
        }
    v = half_sum(v);
    rstd = 1.0f / sqrtf(v * (1.0f / 256.0f) + 1e-6f);
}
// LayerNorm -> packed B operands in the wave's LDS slab
DEV void layer_norm_lds(const f32x16 *x, Slab &sl, const float *prm, int g_off, int b_off, int hi) {
    float mean, rstd;
    ln_stats(x, mean, rstd);
#pragma unroll
    for (int kt = 0; kt < NT; kt++) {
        float g[16], b[16], t[16];
        rp(prm, g_off, kt, hi, g);
        rp(prm, b_off, kt, hi, b);
#pragma unroll
        for (int r = 0; r < 16; r++) t[r] = fmaf((x[kt][r] - mean) * rstd, g[r], b[r]);
        sl.store(kt, pack_tile(t));
    }
}
// LN2 IN REGISTERS.  fc1 re-reads LN2's output once per hidden tile: 32 passes over the 14 slab K-blocks per block, two
// ds_read_b128 each.  hp and fp of impl_mlp are not live in the attention blocks, so the eight packed tiles stay in
// registers instead - pinned in the accumulator half like fp (mfma3_breg; left to hipcc such an array spilled and crashed
// its AGPR-copy rewrite pass) - and fc1 runs like impl_mlp's even layers (gemm_areg, kblock_gelu_breg).  The same values
// reach every accumulator in the same order: bit-identical results.  LN1's output (q, k, v: 24 passes in block 1) stays in
// the slab: with it in registers, or only its tiles 4-7, hipcc spills (DESIGN 3b.4 has the numbers).
// -DZS_SPLIT_LN_SLAB builds the slab form (for A/B runs of two libraries: nothing selects it at run time).
// layer_norm_lds with the eight packed tiles returned in xn
DEV void layer_norm_reg(const f32x16 *x, PT *xn, const float *prm, int g_off, int b_off, int hi) {
    float mean, rstd;
    ln_stats(x, mean, rstd);
#pragma unroll
    for (int kt = 0; kt < NT; kt++) {
        float g[16], b[16], t[16];
        rp(prm, g_off, kt, hi, g);
        rp(prm, b_off, kt, hi, b);
#pragma unroll
        for (int r = 0; r < 16; r++) t[r] = fmaf((x[kt][r] - mean) * rstd, g[r], b[r]);
        xn[kt] = pack_tile(t);
        // tile by tile into the accumulator half (the statements keep their order): 1,392 / 1,333 static v_accvgpr moves
        // in the two kernels instead of 1,604 / 1,637 with the tiles left to pile up in VGPRs
#pragma unroll
        for (int q = 0; q < 4; q++) asm volatile("" : "+a"(xn[kt].v[q]));
    }
}

// one wave-uniform window of the params section -> LDS (all four waves)
DEV void load_params(float *prm, const float *prog_params, int start, int count) {
    __syncthreads();  // everyone is done with the previous window
    const f32x4 *src = reinterpret_cast<const f32x4 *>(prog_params + start);
    f32x4 *dst = reinterpret_cast<f32x4 *>(prm);
    for (int i = threadIdx.x; i < count / 4; i += WAVES * 64) dst[i] = src[i];
    __syncthreads();
}

// One latent tile of the point->latent attention of one head (attn_tile): S = K_tile q (2 K-blocks), online
// softmax update in the log2 domain, o += V_tile^T P (2 K-blocks).  MASK: last tile, rows >= 197
// are padding.
// softmax_pv is the part behind the logits S (c S is the log2-domain logit), V_tile's K-blocks from chunk position pos0.
// NKB = 1: the tile's second V K-block is not in the stream (its 16 rows are all masked: P = 0 exactly).
template <bool MASK, int NKB = 2>
DEV void softmax_pv(AStream &s, f32x16 &S, f32x16 &o, float &m_run, float &z_run, float c, int hi, int pos0) {
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        if (MASK) {
            const int rw = (r & 3) + 8 * (r >> 2) + 4 * hi;
            S[r] = rw < L - 32 * (LT - 1) ? S[r] : -INFINITY;
        }
        mt = fmaxf(mt, S[r]);
    }
    mt *= c;
    // Lazy reference: the running maximum (shared by the two lane halves of a point) is only moved -
    // with the exchange of the halves' maxima through LDS, the rescale factor and the rescaling of o -
    // when some logit of the wave exceeds it by more than 2^LAZY; otherwise the probabilities of this
    // tile are taken relative to the old reference (p <= 2^8: far inside the fp16 halves' range and
    // exact to the same relative precision).  After the first tile that is the rule, and it saves the
    // ~150-cycle LDS round trip and ~20 VALU instructions per tile.
    constexpr float LAZY = 8.0f;
    if (__builtin_amdgcn_ballot_w64(mt > m_run + LAZY) != 0) {   // wave-uniform
        mt = half_max(mt);
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        z_run *= alpha;
#pragma unroll
        for (int r = 0; r < 16; r++) o[r] *= alpha;
        m_run = m_new;
    }
    float zs_ = 0.f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float p = __builtin_amdgcn_exp2f(fmaf(S[r], c, -m_run));
        S[r] = p;
        zs_ += p;
    }
    z_run += zs_;
    gemm_one<false, NoSide, NKB>(s, pack_tile(S), o, pos0);
}
template <bool MASK>
DEV void attn_tile(AStream &s, const PT &q, f32x16 &o, float &m_run, float &z_run, float c, int hi,
                   int pos0) {
    f32x16 S = zero16();
    gemm_one(s, q, S, pos0);
    softmax_pv<MASK>(s, S, o, m_run, z_run, c, hi, pos0 + 2);
}

// The self logit joins the running softmax over the latents (reference m_run, lane-half sums z_run) and the head's output
// is normalised: o = (alpha o + p_self v) / z.
DEV void merge_self(f32x16 &o, const f32x16 &v, float m_run, float z_run, float s_self) {
    const float m_new = fmaxf(m_run, s_self);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    const float p_self = __builtin_amdgcn_exp2f(s_self - m_new);
    const float z = fmaf(half_sum(z_run), alpha, p_self);
    const float inv = 1.0f / z;
    const float a_i = alpha * inv, p_i = p_self * inv;
#pragma unroll
    for (int r = 0; r < 16; r++) o[r] = fmaf(p_i, v[r], o[r] * a_i);
}

#ifdef ZS_EXP_TIMING  // tools/phase_timing_split.py: cycle stamps of (block 0, wave 0, first tile) -> workspace tail
#define ZS_STAMP(i) do { if (dbg) dbg[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ZS_STAMP(i) do { } while (0)
#endif
// One wave: 32 points (lane & 31; both lane halves carry the same point).
// b0s: this image's compact block-0 stream (BLOCK 0 STREAM above; wave-uniform), or null: block 0 runs its q/k/v GEMMs like block 1
DEV float decode_tile(const char *prog, float *prm, u32x4 *stage, unsigned stage_addr, u32x4 *slab,
                      const char *b0s, float px, float py, float pz, int wave, int lane, float &guard,
                      unsigned long long *dbg) {
    const int hi = lane >> 5;
    const float *prog_params = reinterpret_cast<const float *>(prog) + REC_FLOATS;
    AStream s;
    s.init(b0s ? b0s : prog, stage, stage_addr, wave, lane);
    Slab sl;
    sl.fl = slab;
    ZS_STAMP(0);

    // point_proj (implicit.py:128-131); y is the residual stream, kept as accumulators
    load_params(prm, prog_params, W_PP, 1024);
    f32x16 y[NT];
#pragma unroll
    for (int kt = 0; kt < NT; kt++) y[kt] = xyz_affine(prm, 0, kt, hi, px, py, pz);

    ZS_STAMP(1);

    const float scale = 0.17677669529663688110f;  // 32 ** -0.5

#pragma unroll 1
    for (int blk = 0; blk < BLOCKS; blk++) {
        const bool strm = blk == 0 && b0s != nullptr;  // wave-uniform
        float rstd0 = 0.f;
        u32x4 ub = {0u, 0u, 0u, 0u};
        bool u_bad = false;
        if (strm) {
            // the block window stays for the whole block; LN1's output is not needed, only rstd: u, split and packed once
            load_params(prm, prog_params, W_BLK, P_BLK_STRIDE);
            float mean;
            ln_stats(y, mean, rstd0);
            ub = rank5_b(px * rstd0, py * rstd0, pz * rstd0, rstd0, hi, u_bad);
        } else {
            load_params(prm, prog_params, W_BLK + blk * P_BLK_STRIDE, P_BLK_STRIDE);
            layer_norm_lds(y, sl, prm, PB_LN1G, PB_LN1B, hi);
        }
        ZS_STAMP(2 + blk * 4);
        // y = x + proj_bias + sum_heads Wproj_h o_h
#pragma unroll
        for (int nt = 0; nt < NT; nt++) y[nt] += rp16(prm, PB_BPROJ, nt, hi);

        // one head: 48 (q, k, v) + 28 (7 latent tiles) + 16 (proj) = 92 K-blocks = 11.5 chunks, so
        // heads alternate between chunk positions 0 and 4 (P); all positions are compile-time
        auto head = [&](int hd, auto Ptag) {
            constexpr int P = decltype(Ptag)::value;
            f32x16 q = rp16(prm, PB_BQKV, hd * 3 + 0, hi);
            gemm_lds(s, sl, q, P);
            f32x16 k = rp16(prm, PB_BQKV, hd * 3 + 1, hi);
            gemm_lds(s, sl, k, P);
            f32x16 v = rp16(prm, PB_BQKV, hd * 3 + 2, hi);
            gemm_lds(s, sl, v, P);

            // logits are kept in the log2 domain: c = d^-1/2 * log2(e), softmax = 2^(c s - m)
            const float c = scale * 1.44269504088896340736f;
            float s_self = 0.f;  // self logit (implicit.py:44), fp32
            float qq = 0.f;      // |q|^2: envelope guard, see ENVELOPE below
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s_self = fmaf(q[r], k[r], s_self);
                qq = fmaf(q[r], q[r], qq);
            }
            s_self = half_sum(s_self) * c;
            {   // (scale |q| max_l |k_l|)^2, the Cauchy-Schwarz bound of this head's latent logits
                const float km = prog_params[P_KMAX + blk * HEADS + hd] * scale;  // scalar load
                guard = fmaxf(guard, half_sum(qq) * (km * km));
            }
            const PT qp = pack_tile(q);

            float m_run = -INFINITY, z_run = 0.f;
            f32x16 o = zero16();
            // unrolled: as a loop (`unroll 1`) this cost short launches 0.2 - 0.4 % once the table arm was gone
#pragma unroll
            for (int l2 = 0; l2 < (LT - 1) / 2; l2++) {
                attn_tile<false>(s, qp, o, m_run, z_run, c, hi, P);
                attn_tile<false>(s, qp, o, m_run, z_run, c, hi, (P + 4) & (CK - 1));
            }
            attn_tile<true>(s, qp, o, m_run, z_run, c, hi, P);
            merge_self(o, v, m_run, z_run, s_self);
            // y += Wproj[:, head] o_h
            const PT op = pack_tile(o);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) gemm_one(s, op, y[nt], (P + 4 + 2 * nt) & (CK - 1));
        };
        // one head of block 0 from the compact stream (BLOCK 0 STREAM): 34 slots from chunk position P
        auto head_b0s = [&](int hd, auto Ptag) {
            constexpr int P = decltype(Ptag)::value;
            u32x4 a0, a1;
            s.step(P & (CK - 1), a0, a1);                       // [q | k]
            pin(a0, a1);
            const f32x16 q = mfma_rank5(a0, ub), k = mfma_rank5(a1, ub);
            s.step((P + 1) & (CK - 1), a0, a1);                 // [v | U0]
            pin(a0, a1);
            const f32x16 v = mfma_rank5(a0, ub);
            f32x16 S = mfma_rank5(a1, ub);
            float s_self = 0.f, qq = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s_self = fmaf(q[r], k[r], s_self);
                qq = fmaf(q[r], q[r], qq);
            }
            s_self = half_sum(s_self) * (scale * 1.44269504088896340736f);
            {
                const float km = prog_params[P_KMAX + hd] * scale;  // scalar load
                guard = fmaxf(guard, half_sum(qq) * (km * km));
            }
            float m_run = -INFINITY, z_run = 0.f;
            f32x16 o = zero16();
            softmax_pv<false>(s, S, o, m_run, z_run, 1.0f, hi, P + 2);
#pragma unroll
            for (int i = 0; i < (LT - 1) / 2; i++) {
                s.step((P + 4 + 5 * i) & (CK - 1), a0, a1);     // [U(2i+1) | U(2i+2)]: the second operand waits in a1
                pin(a0, a1);
                S = mfma_rank5(a0, ub);
                softmax_pv<false>(s, S, o, m_run, z_run, 1.0f, hi, P + 5 + 5 * i);
                S = mfma_rank5(a1, ub);
                if (2 * i + 2 < LT - 1)
                    softmax_pv<false>(s, S, o, m_run, z_run, 1.0f, hi, P + 7 + 5 * i);
                else
                    softmax_pv<true, 1>(s, S, o, m_run, z_run, 1.0f, hi, P + 7 + 5 * i);
            }
            merge_self(o, v, m_run, z_run, s_self);
            const PT op = pack_tile(o);
            // head 7's proj K-blocks are the compact stream's last two chunks: their pos-7 steps stage the program's
            if (P == 6 && hd == HEADS - 1) s.seek(prog + HEADS * (G_HEAD / 2) * (KB_U4 * 16), wave, lane);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) gemm_one(s, op, y[nt], (P + 18 + 2 * nt) & (CK - 1));
        };
        static_assert((LT - 1) % 2 == 0 && (3 * NT * 2 + LT * 4 + NT * 2) % CK == 4, "head = 11.5 chunks");
        static_assert(B0S_KB_HEAD % CK == 2 && HEADS % 4 == 0 && (HEADS * (G_HEAD / 2)) % CK == 0,
                      "compact heads start at chunk positions 0, 2, 4, 6; the program resumes on a chunk boundary");
        if (strm) {
#pragma unroll 1
            for (int hd = 0; hd < HEADS; hd += 4) {
                head_b0s(hd, std::integral_constant<int, 0>());
                head_b0s(hd + 1, std::integral_constant<int, 2>());
                head_b0s(hd + 2, std::integral_constant<int, 4>());
                head_b0s(hd + 3, std::integral_constant<int, 6>());
            }
            // a component of u beyond the fp16 range: the tile goes to the exact kernel (guard = +inf)
            guard = __builtin_bit_cast(float, u_bad ? 0x7f800000u : __builtin_bit_cast(unsigned, guard));
        } else {
#pragma unroll 1
            for (int hd = 0; hd < HEADS; hd += 2) {
                head(hd, std::integral_constant<int, 0>());
                head(hd + 1, std::integral_constant<int, 4>());
            }
        }

        ZS_STAMP(3 + blk * 4);
        // MLP (timm Mlp): y += b2 + W2 gelu(W1 LN2(y) + b1), one hidden tile at a time
        PT xn[NT];  // LN2_REGS
        if constexpr (LN2_REGS)
            layer_norm_reg(y, xn, prm, PB_LN2G, PB_LN2B, hi);
        else
            layer_norm_lds(y, sl, prm, PB_LN2G, PB_LN2B, hi);
#pragma unroll
        for (int nt = 0; nt < NT; nt++) y[nt] += rp16(prm, PB_B2, nt, hi);
        ZS_STAMP(4 + blk * 4);
        // software pipeline over the hidden tiles (stream order: fc1(0), [fc1(t+1), fc2(t)]..., fc2(31)):
        // fc1 of tile t+1 carries the GELU + operand split of tile t and the bias fetch of tile t+2
        RowInit bi;
        f32x16 hid = rp16(prm, PB_B1, 0, hi);
        bi.start(prm, PB_B1, 1, hi);
        auto bias_side = [&](int kb, int g) {
            if (g == 2 && (kb & 3) == 1) bi.step(kb & ~3);
        };
        if constexpr (LN2_REGS) {
            gemm_areg<NT>(s, xn, hid, bias_side);
            mfma_settle(hid);   // fc1(0)'s last MFMA (mfma3_breg) is a few instructions in front of GELU(hid[0]) in fc1(1)
        } else {
            gemm_lds(s, sl, hid, 0, bias_side);
        }
#pragma unroll 1
        for (int ht = 0; ht < HT - 1; ht++) {
            f32x16 nxt = bi.v;
            bi.start(prm, PB_B1, ht + 2 < HT ? ht + 2 : HT - 1, hi);
            TilePacker e;
            auto fin = [&](int kb, float r) { e.feed(kb, r); };
            auto tail = [&](int kb) { if ((kb & 3) == 1) bi.step(kb & ~3); };
            if constexpr (LN2_REGS)
                gemm_areg_act<0>(s, xn, nxt, hid, fin, tail);
            else
                gemm_lds_act<0>(s, sl, nxt, hid, fin, tail);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) gemm_one(s, e.p, y[nt], (2 * nt) & (CK - 1));
            hid = nxt;
        }
        {
#pragma unroll
            for (int r = 0; r < 16; r++) hid[r] = gelu_erf(hid[r]);
            const PT hp = pack_tile(hid);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) gemm_one(s, hp, y[nt], (2 * nt) & (CK - 1));
        }
        ZS_STAMP(5 + blk * 4);
    }

    // final norm (implicit.py:275) -> feat, fp32 in registers
    load_params(prm, prog_params, W_IA, W_IB - W_IA);
    float h[NT * 16];
    {
        float mean, rstd;
        ln_stats(y, mean, rstd);
#pragma unroll
        for (int kt = 0; kt < NT; kt++) {
            float g[16], b[16];
            rp(prm, P_LNFG - W_IA, kt, hi, g);
            rp(prm, P_LNFB - W_IA, kt, hi, b);
#pragma unroll
            for (int r = 0; r < 16; r++) h[kt * 16 + r] = fmaf((y[kt][r] - mean) * rstd, g[r], b[r]);
        }
    }
    ZS_STAMP(10);
    // IMPL_MLP IN REGISTERS.  The layers of impl_mlp alternate between two packed activation arrays: the even layers (0 and
    // the skip layers 2, 4, 6) read hp and write hq, the odd layers read hq and write hp.  hq used to be the wave's slab -
    // every output tile of an odd layer re-read its 14 K-blocks with two ds_read_b128 each, 896 reads and 112 stores per
    // wave tile.  The residual stream y is dead here, so hq stays in registers beside hp and feat / sqrt(2) (fp): tiles
    // IMPL_VT..7 pinned in the accumulator half like fp (mfma3_breg, kblock_softplus_breg), tiles 0..IMPL_VT-1 left to
    // hipcc, which keeps them in VGPRs - fp and all of hq fill the 256 AGPRs, and the values that live across the whole
    // tile, which hipcc parks there in this phase, then go to scratch (DESIGN 3b.5 has the forms tried).  For the same
    // reason fp is packed in front of layer 0 and not behind it: feat in fp32 (128 registers) is dead before hq fills.
    // The same values reach every accumulator in the same order: bit-identical results.
    constexpr int IMPL_VT = 2;
    PT hp[NT];
    PT hq[NT];  // IMPL_REGS
    const float rsqrt2 = 0.70710678118654752440f;
    PT fp[NT];
    auto make_fp = [&]() {
#pragma unroll
        for (int kt = 0; kt < NT; kt++) {
            float t[16];
#pragma unroll
            for (int r = 0; r < 16; r++) t[r] = h[kt * 16 + r] * rsqrt2;
            fp[kt] = pack_tile(t);
            if constexpr (IMPL_REGS) {
#pragma unroll
                for (int q = 0; q < 4; q++) asm volatile("" : "+a"(fp[kt].v[q]));
            }
        }
    };
    if constexpr (IMPL_REGS) make_fp();
    auto to_odd = [&](int tile, const PT &p) {   // an even layer's packed output tile -> the odd layers' input array
        if constexpr (IMPL_REGS) {
            hq[tile] = p;
            if (tile >= IMPL_VT) {
#pragma unroll
                for (int q = 0; q < 4; q++) asm volatile("" : "+a"(hq[tile].v[q]));
            }
        } else {
            sl.store(tile, p);
        }
    };

    // impl_mlp (implicit.py:168-184): inputs = cat[xyz, feat].  Layer 0: feat (hp) -> hq
#pragma unroll
    for (int kt = 0; kt < NT; kt++) hp[kt] = pack_tile(h + kt * 16);
    // (software pipeline over the output tiles: tile nt's GEMM carries tile nt-1's activation)
    {
        f32x16 prev;
        XyzInit ini;
        ini.v = xyz_affine(prm, P_IMPL0 - W_IA, 0, hi, px, py, pz);
#pragma unroll
        for (int nt = 0; nt <= NT; nt++) {
            TilePacker e;
            if (nt < NT) {
                f32x16 acc = ini.v;
                if (nt + 1 < NT) ini.start(prm, P_IMPL0 - W_IA, nt + 1, hi);
                if (nt > 0)
                    gemm_reg_act<1>(s, hp, acc, prev, [&](int kb, float r) { e.feed(kb, r); },
                                    [&](int kb) { if (nt + 1 < NT) ini.step(kb, px, py, pz); });
                else
                    gemm_reg<NT, 0>(s, hp, acc, [&](int kb, int g) { if (g == 2) ini.step(kb, px, py, pz); });
                if (nt > 0) to_odd(nt - 1, e.p);
                prev = acc;
            } else {
                mfma_settle(prev);
#pragma unroll
                for (int kb = 0; kb < 16; kb++) e.feed(kb, softplus100(prev[kb]));
                to_odd(nt - 1, e.p);
            }
        }
    }
    ZS_STAMP(11);
    // the skip layers consume cat[x, xyz, feat] / sqrt(2): feat / sqrt(2) stays packed in registers
    // (the residual stream is dead by now) and is contracted inside each skip layer as 16 more
    // K-blocks per output tile - the split stream interleaves [x part | feat part] per tile
    // (split_source_kblock) - so nothing is parked in memory (round 1 parked 96 KiB of fp32
    // partial products per wave tile: 12.8 GB per 129^3 launch)
    if constexpr (!IMPL_REGS) make_fp();
    const float sx = px * rsqrt2, sy = py * rsqrt2, sz = pz * rsqrt2;

    ZS_STAMP(12);
    // layer 1 (plain): hq -> hp, pre-divided by sqrt(2) because layer 2 is a skip layer
    {
        f32x16 prev;
        RowInit ini;
        ini.v = rp16(prm, P_IMPL1 - W_IA, 0, hi);
#pragma unroll
        for (int nt = 0; nt <= NT; nt++) {
            TilePacker e;
            if (nt < NT) {
                f32x16 acc = ini.v;
                if (nt + 1 < NT) ini.start(prm, P_IMPL1 - W_IA, nt + 1, hi);
                auto fin = [&](int kb, float r) { e.feed(kb, r * rsqrt2); };
                auto tail = [&](int kb) { if (nt + 1 < NT) ini.step(kb); };
                auto side = [&](int kb, int g) { if (g == 2) ini.step(kb); };
                if constexpr (IMPL_REGS) {
                    if (nt > 0) {
                        mfma_settle(prev);   // prev's last MFMA (an asm K-block on hq[7]) is a few instructions back
                        gemm_areg_act<1, IMPL_VT>(s, hq, acc, prev, fin, tail);
                    } else {
                        gemm_areg<NT, IMPL_VT>(s, hq, acc, side);
                    }
                } else {
                    if (nt > 0)
                        gemm_lds_act<1>(s, sl, acc, prev, fin, tail);
                    else
                        gemm_lds(s, sl, acc, 0, side);
                }
                if (nt > 0) hp[nt - 1] = e.p;
                prev = acc;
            } else {
                mfma_settle(prev);
#pragma unroll
                for (int kb = 0; kb < 16; kb++) e.feed(kb, softplus100(prev[kb]) * rsqrt2);
                hp[nt - 1] = e.p;
            }
        }
    }
    ZS_STAMP(13);
    float out = 0.f;
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        if (i == 1) load_params(prm, prog_params, W_IB, P_USED - W_IB);
        const int pp = i == 0 ? P_IMPL_PAIR - W_IA : (i - 1) * P_IMPL_PAIR_STRIDE;
        // skip layer 2+2i: hp (x / sqrt(2)) and feat / sqrt(2) -> hq
        {
            f32x16 prev;
            XyzInit ini;
            ini.v = xyz_affine(prm, pp, 0, hi, sx, sy, sz);
#pragma unroll
            for (int nt = 0; nt <= NT; nt++) {
                TilePacker e;
                if (nt > 0) mfma_settle(prev);   // prev's last MFMA (gemm_areg) is a few instructions back
                if (nt < NT) {
                    f32x16 acc = ini.v;
                    if (nt + 1 < NT) ini.start(prm, pp, nt + 1, hi);
                    // the x part carries the previous tile's activation, the feat part the next tile's initialiser
                    if (nt > 0)
                        gemm_reg_act<1>(s, hp, acc, prev, [&](int kb, float r) { e.feed(kb, r); }, [&](int) {});
                    else
                        gemm_reg<NT>(s, hp, acc);
                    gemm_areg<NT>(s, fp, acc, [&](int kb, int g) {
                        if (g == 2 && nt + 1 < NT) ini.step(kb, sx, sy, sz);
                    });
                    if (nt > 0) to_odd(nt - 1, e.p);
                    prev = acc;
                } else {
#pragma unroll
                    for (int kb = 0; kb < 16; kb++) e.feed(kb, softplus100(prev[kb]));
                    to_odd(nt - 1, e.p);
                }
            }
        }
        // plain layer 3+2i: hq -> hp (/ sqrt(2) when the next layer is a skip layer);
        // the last one feeds layer 8 (256 -> 1), evaluated in fp32 on the spot
        const float post = i < 2 ? rsqrt2 : 1.0f;
        {
            f32x16 prev;
            RowInit ini, w8;  // bias of the next tile; layer 8 weights of the previous tile (last pair only)
            const float wsel = i == 2 ? 1.0f : 0.0f;
            ini.v = rp16(prm, pp + 1024, 0, hi);
#pragma unroll
            for (int r = 0; r < 16; r++) w8.v[r] = 0.f;
#pragma unroll
            for (int nt = 0; nt <= NT; nt++) {
                TilePacker e;
                // weights of tile nt - 1, fetched beside the previous GEMM; pairs 0 and 1 read whatever
                // finite parameters sit at that offset of their window and scale them away (a
                // branch on i here crashes hipcc's AGPR-copy rewrite pass, ROCm 7.2)
                const f32x16 w = w8.v * wsel;
                auto finish = [&](int kb, float v) {
                    const float t = v * post;
                    e.feed(kb, t);
                    out = fmaf(t, w[kb], out);
                };
                if (nt < NT) {
                    f32x16 acc = ini.v;
                    if (nt + 1 < NT) ini.start(prm, pp + 1024, nt + 1, hi);
                    w8.start(prm, P_W8 - W_IB, nt, hi);
                    auto tail = [&](int kb) {
                        if (nt + 1 < NT) ini.step(kb);
                        w8.step(kb);
                    };
                    auto side = [&](int kb, int g) { if (g == 2) tail(kb); };
                    if constexpr (IMPL_REGS) {
                        if (nt > 0) {
                            mfma_settle(prev);
                            gemm_areg_act<1, IMPL_VT>(s, hq, acc, prev, finish, tail);
                        } else {
                            gemm_areg<NT, IMPL_VT>(s, hq, acc, side);
                        }
                    } else {
                        if (nt > 0)
                            gemm_lds_act<1>(s, sl, acc, prev, finish, tail);
                        else
                            gemm_lds(s, sl, acc, 0, side);
                    }
                    if (nt > 0) hp[nt - 1] = e.p;
                    prev = acc;
                } else {
                    mfma_settle(prev);
#pragma unroll
                    for (int kb = 0; kb < 16; kb++) finish(kb, softplus100(prev[kb]));
                    hp[nt - 1] = e.p;
                }
            }
        }
    }
    ZS_STAMP(14);
    s.drain();
    out = half_sum(out);
    ZS_STAMP(15);
    return out + prm[P_B8 - W_IB];
}

template <bool GRID>
__global__ __launch_bounds__(WAVES * 64, 1) void sdf_decode_split_kernel(
    const char *__restrict__ programs, size_t program_stride_bytes, int batch,
    const float *__restrict__ points,  // !GRID: [batch][m][3]
    const float *__restrict__ axis,    //  GRID: [G]
    int G, long long first_point,      //  GRID: linear index of the first grid point
    int m,                             // points per image handled by this launch
    float *__restrict__ out, int apply_sigmoid, f32x4 *__restrict__ workspace,
    int *__restrict__ tile_flags,    // [tiles] zeroed by the caller, or null
    int static_order,                // 1: tile += gridDim.x, no counter (ZS_SPLIT_STATIC_TILES=1: the A/B arm of tools/ab_tile_order.py)
    const char *__restrict__ block0_streams) {  // [batch][B0_STREAM_BYTES] (block0_stream_kernel), or null: block 0's GEMMs
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    float *prm = lds;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    u32x4 *stage = reinterpret_cast<u32x4 *>(lds + PRM_WINDOW);
    const unsigned stage_addr = __builtin_amdgcn_readfirstlane(
        (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)(lds + PRM_WINDOW));
    u32x4 *fl = reinterpret_cast<u32x4 *>(lds + PRM_WINDOW + STAGE_FLOATS) + wave * SLAB_U4 + lane;

    const int tiles_per_img = (m + PTS_PER_BLOCK - 1) / PTS_PER_BLOCK;
    const int total = tiles_per_img * batch;
    // DYNAMIC tile order (round 4).  Every workgroup takes tile blockIdx.x first, then fetches the next index from a counter in
    // the workspace tail (one agent-scope atomic per 128-point tile of ~0.44 ms, issued when the tile is done: nothing of this
    // kernel's own is in flight then, so the hand-counted vmcnt waits of decode_tile are not disturbed).  A static
    // tile += gridDim.x deal makes the launch as slow as its unluckiest workgroup: one whose CU was still busy when the launch
    // started (the per-image probe launches of Implicit.prepare run beside it), or the 98 of 256 that get a ninth tile at
    // vox 64.  Thread 0 fetches, the index reaches the other waves through a per-workgroup slot in global memory (the kernel
    // owns all 160 KiB of LDS) behind one barrier.  D = total - gridDim.x indices are real; each workgroup's terminal fetch
    // is >= D, and the one that draws D + gridDim.x - 1 - the last fetch of the launch - puts the counter back to zero for
    // the next launch.  Which workgroup evaluates a tile does not change its result.
    // The counter is the LIBRARY's: launch_counter_reset() zeroes it on the stream in front of every launch (a
    // caller's un-zeroed workspace, or a faulted launch that left it non-zero, must not decide which tiles get evaluated),
    // and a fetched index is used only when it is a real one (unsigned compare).
    int *tile_counter = zs::qry::tile_counter(workspace);
    int *tile_slot = tile_counter + 16 + blockIdx.x;
    const int dyn_tiles = total > (int)gridDim.x ? total - (int)gridDim.x : 0;
    for (int tile = blockIdx.x;;) {
      if (tile < total) {
        const int img = tile / tiles_per_img;
        const int t = tile - img * tiles_per_img;
        const char *prog = programs + (size_t)img * program_stride_bytes;

        const int p = t * PTS_PER_BLOCK + wave * PTS_PER_WAVE + (lane & 31);
        const int pc = p < m ? p : m - 1;  // clamp: tail lanes recompute the last point
        float px, py, pz;
        if (GRID) {
            const long long gp = first_point + pc;
            const long long gg = (long long)G * G;
            const int ix = (int)(gp / gg);
            const int rem = (int)(gp - (long long)ix * gg);
            const int iy = rem / G;
            const int iz = rem - iy * G;
            px = axis[ix];
            py = axis[iy];
            pz = axis[iz];
        } else {
            const float *q = points + ((size_t)img * m + pc) * 3;
            px = q[0];
            py = q[1];
            pz = q[2];
        }
#ifdef ZS_EXP_TIMING
        unsigned long long *dbg = (blockIdx.x == 0 && threadIdx.x == 0 && tile == 0)
            ? timing_stamps(workspace) : nullptr;
#else
        unsigned long long *dbg = nullptr;
#endif
        float guard = 0.f;
        const char *b0s = block0_streams ? block0_streams + (size_t)img * B0_STREAM_BYTES : nullptr;
        float logit = decode_tile(prog, prm, stage, stage_addr, fl, b0s, px, py, pz, wave, lane, guard, dbg);
        if (apply_sigmoid) logit = 1.0f / (1.0f + expf(-logit));
        // ENVELOPE (zeroshape_amd/program.py, S_GUARD): outside it the tile is flagged for the
        // exact-fp32 kernel, and a program with non-finite / out-of-range operands yields NaN like
        // the reference's arithmetic would (integer tests: this file is built with -fno-honor-nans)
        const unsigned bad = reinterpret_cast<const unsigned *>(prog)[REC_FLOATS + P_FLAG];
        const bool pt_bad = (__builtin_bit_cast(unsigned, px) & 0x7f800000u) == 0x7f800000u ||
                            (__builtin_bit_cast(unsigned, py) & 0x7f800000u) == 0x7f800000u ||
                            (__builtin_bit_cast(unsigned, pz) & 0x7f800000u) == 0x7f800000u;
        if (bad || pt_bad) logit = __builtin_bit_cast(float, 0x7fc00000u);
        if (tile_flags) {
            const bool over = !(__builtin_bit_cast(unsigned, guard) <= __builtin_bit_cast(unsigned, S_GUARD * S_GUARD));
            if (__builtin_amdgcn_ballot_w64(over || bad != 0) != 0 && lane == 0) tile_flags[tile] = 1;
        }
        if (lane < 32 && p < m) out[(size_t)img * m + p] = logit;
      }
        if (static_order) {                   // wave-uniform
            tile += (int)gridDim.x;
            if (tile >= total) break;
            continue;
        }
        if (threadIdx.x == 0) {
            const int d = __hip_atomic_fetch_add(tile_counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == dyn_tiles + (int)gridDim.x - 1)
                __hip_atomic_store(tile_counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(tile_slot, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();                      // (also drains thread 0's store: s_waitcnt vmcnt(0) in front of the barrier)
        const int d = __builtin_amdgcn_readfirstlane(__hip_atomic_load(tile_slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if ((unsigned)d >= (unsigned)dyn_tiles) break;
        tile = (int)gridDim.x + d;
    }
}

// not finite, or beyond the fp16 range the split operands saturate at (integer test: NaN-proof)
DEV bool out_of_range(const f32x4 &v) {
    const unsigned lim = 0x477fe000u;  // 65504.0f
    return (__builtin_bit_cast(unsigned, v.x) & 0x7fffffffu) > lim || (__builtin_bit_cast(unsigned, v.y) & 0x7fffffffu) > lim ||
           (__builtin_bit_cast(unsigned, v.z) & 0x7fffffffu) > lim || (__builtin_bit_cast(unsigned, v.w) & 0x7fffffffu) > lim;
}

// Order of the split stream: the fp32 program's, except (a) inside the two MLP sections, where the
// kernel runs a software pipeline over the 32 hidden tiles (fc1 of tile t+1 before fc2 of tile
// t): fc1(0), [fc1(1), fc2(0)], ..., [fc1(31), fc2(30)], fc2(31), 16 K-blocks each; (b) in
// impl_mlp, where the feat halves of the skip layers are contracted inside their layers.
__host__ __device__ inline int split_source_kblock(int kb) {
    constexpr int KB_BLOCK = G_BLOCK / 2, KB_ATT = HEADS * G_HEAD / 2;
    static_assert(KB_BLOCK - KB_ATT == HT * 32, "an MLP section is 32 K-blocks per hidden tile");
    constexpr int KB_IMPL0 = BLOCKS * KB_BLOCK, KB_L = NT * NT * 2;  // impl_mlp section; K-blocks of a 256 x 256 layer
    if (kb >= KB_IMPL0 + G_IMPL / 2) return kb;  // zero tail
    if (kb >= KB_IMPL0) {
        // fp32 program: L0 | Z2 Z4 Z6 (feat halves of the skip layers) | L1 | L2x L3 | L4x L5 | L6x L7
        // split stream: L0 | L1 | for each pair: for each output tile [L(2+2i)x tile | Z(2+2i) tile], L(3+2i)
        const int p = kb - KB_IMPL0;
        if (p < KB_L) return kb;                                  // layer 0
        if (p < 2 * KB_L) return KB_IMPL0 + 4 * KB_L + (p - KB_L);  // layer 1
        const int q = p - 2 * KB_L, pair = q / (3 * KB_L), r = q - pair * 3 * KB_L;
        if (r >= 2 * KB_L) return KB_IMPL0 + (5 + 2 * pair + 1) * KB_L + (r - 2 * KB_L);  // plain layer 3 + 2 pair
        const int nt = r / (4 * NT), w = r - nt * 4 * NT;         // 16 x-part + 16 feat-part K-blocks per tile
        return w < 2 * NT ? KB_IMPL0 + (5 + 2 * pair) * KB_L + nt * 2 * NT + w
                          : KB_IMPL0 + (1 + pair) * KB_L + nt * 2 * NT + (w - 2 * NT);
    }
    const int blk = kb / KB_BLOCK, p = kb - blk * KB_BLOCK - KB_ATT;
    if (p < 16) return kb;  // attention section, or fc1(0)
    const int q = p - 16, it = q >> 5, r = q & 31;
    int src;
    if (it < HT - 1)
        src = r < 16 ? (it + 1) * 32 + r : it * 32 + r;  // fc1(it + 1) | fc2(it)
    else
        src = it * 32 + 16 + r;                          // fc2(31)
    return blk * KB_BLOCK + KB_ATT + src;
}

// fp32 decoder program -> split program: same units and size; K-block j of a unit holds
// records 8 j .. 8 j + 7 of that unit as [hi: lane x 8 fp16][lo: lane x 8 fp16]; params copied.
__global__ __launch_bounds__(256) void split_program_kernel(const float *__restrict__ src,
                                                            size_t src_stride_floats,
                                                            u32x4 *__restrict__ dst,
                                                            size_t dst_stride_u4) {
    const int img = blockIdx.y;
    const float *s = src + (size_t)img * src_stride_floats;
    u32x4 *d = dst + (size_t)img * dst_stride_u4;
    const int e = blockIdx.x * 256 + threadIdx.x;
    constexpr int REC_KB = REC_FLOATS / (KB_U4 * 4);  // K-blocks incl. the zero tail
    if (e < REC_KB * 64) {
        const int kb = e >> 6, lane = e & 63;
        const f32x4 *g = reinterpret_cast<const f32x4 *>(s) + (size_t)split_source_kblock(kb) * 128;  // two fp32 groups
        const f32x4 a = g[lane], b = g[64 + lane];
        if (out_of_range(a) || out_of_range(b)) atomicOr(reinterpret_cast<unsigned *>(d) + REC_FLOATS + P_FLAG, 1u);
        unsigned h[4], l[4];
        split2(a.x, a.y, h[0], l[0]);
        split2(a.z, a.w, h[1], l[1]);
        split2(b.x, b.y, h[2], l[2]);
        split2(b.z, b.w, h[3], l[3]);
        const u32x4 hi = {h[0], h[1], h[2], h[3]}, lo = {l[0], l[1], l[2], l[3]};
        d[(size_t)kb * KB_U4 + lane] = hi;
        d[(size_t)kb * KB_U4 + 64 + lane] = lo;
    } else {
        const int i = e - REC_KB * 64;
        // (the quads of P_FLAG - zeroed by the launcher - and P_KMAX are written elsewhere)
        if (i < PARAM_FLOATS / 4 && i != P_FLAG / 4 && (i < P_KMAX / 4 || i >= (P_KMAX + BLOCKS * HEADS) / 4)) {
            const f32x4 v = reinterpret_cast<const f32x4 *>(s + REC_FLOATS)[i];
            if (i < (P_USED + 3) / 4 && out_of_range(v))
                atomicOr(reinterpret_cast<unsigned *>(d) + REC_FLOATS + P_FLAG, 1u);
            d[REC_FLOATS / 4 + i] = __builtin_bit_cast(u32x4, v);
        }
    }
}

// largest |k_l| over the latent rows of (image, block, head), from the K records of the fp32
// program (record (lt, r) of lane l holds K[32 lt + (l & 31)][row(r, l >> 5)]) -> params[P_KMAX]
__global__ __launch_bounds__(256) void k_bound_kernel(const float *__restrict__ src, size_t src_stride_floats,
                                                      u32x4 *__restrict__ dst, size_t dst_stride_u4) {
    __shared__ float red[256];
    const int img = blockIdx.y, bh = blockIdx.x, blk = bh / HEADS, hd = bh - blk * HEADS;
    const float *kv = src + (size_t)img * src_stride_floats +
                      (size_t)(blk * G_BLOCK + hd * G_HEAD + G_QKV_HEAD) * GROUP_FLOATS;
    float sq = 0.f;
    const int t = threadIdx.x;
    if (t < LT * 32) {
        const int lt = t >> 5;
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f32x4 v = reinterpret_cast<const f32x4 *>(kv + (lt * 8 + g) * GROUP_FLOATS)[(t & 31) + 32 * half];
                sq = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, sq))));
            }
    }
    red[t] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] = fmaxf(red[t], red[t + o]);
        __syncthreads();
    }
    if (t == 0)
        reinterpret_cast<float *>(dst + (size_t)img * dst_stride_u4)[REC_FLOATS + P_KMAX + bh] = sqrtf(red[0]);
}

// BLOCK 0 TABLE of every image, from its SPLIT program (the launchers hold nothing else): weights are hi + lo of block 0's
// q/k/v K-blocks, g / b / A / the biases come from the params section; sums in double, rounded once.  One workgroup of four
// waves per (image, tile = 3 head + {q, k, v}): wave w takes K-blocks 4 w .. 4 w + 3 of the tile's 16, lane l of it owns
// output row l & 31 and the 8 input features per K-block its lane half holds in the records (K-block 2 kt + j, element e:
// feature 32 kt + row(8 j + e, l >> 5), which is position 32 kt + 16 (l >> 5) + 8 j + e of a row-param vector); the eight
// partial sums of a row meet through LDS in a fixed order.  Non-finite operands just propagate (P_FLAG turns such an image
// into NaN anyway).
constexpr int B0_THREADS = 256;
__global__ __launch_bounds__(B0_THREADS) void block0_window_kernel(const char *__restrict__ programs,
                                                                   size_t program_stride_bytes, float *__restrict__ tables) {
    __shared__ double red[B0_THREADS][5];
    __shared__ double msum[64][4];
    const int tile = blockIdx.x, img = blockIdx.y, t = threadIdx.x, wave = t >> 6, lane = t & 63, hl = lane >> 5;
    const char *prog = programs + (size_t)img * program_stride_bytes;
    const float *par = reinterpret_cast<const float *>(prog) + REC_FLOATS;
    float *out = tables + (size_t)img * PRM_WINDOW;
    // m = column mean of A (point_proj: one (w0, w1, w2, b) quad per feature): 64 partial sums of 4 features, then all of them
    if (t < 64) {
#pragma unroll
        for (int d = 0; d < 4; d++) {
            double a = 0.0;
#pragma unroll
            for (int f = 0; f < 4; f++) a += (double)par[P_PP + (4 * t + f) * 4 + d];
            msum[t][d] = a;
        }
    }
    __syncthreads();
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 64; i++)
#pragma unroll
        for (int d = 0; d < 4; d++) m[d] += msum[i][d];
#pragma unroll
    for (int d = 0; d < 4; d++) m[d] *= 1.0 / C;
    const int head = tile / 3, part = tile - head * 3;
    const u32x4 *kb0 = reinterpret_cast<const u32x4 *>(prog) + (size_t)(head * (G_HEAD / 2) + part * 2 * NT) * KB_U4;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // T[.][0..3], W b
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int kb = 4 * wave + k;
        const u32x4 h4 = kb0[kb * KB_U4 + lane], l4 = kb0[kb * KB_U4 + 64 + lane];
        const int f0 = (kb >> 1) * 32 + hl * 16 + (kb & 1) * 8;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const unsigned hw = h4[e >> 1] >> (16 * (e & 1)), lw = l4[e >> 1] >> (16 * (e & 1));
            const double w = (double)(float)__builtin_bit_cast(_Float16, (unsigned short)hw) +
                             (double)(float)__builtin_bit_cast(_Float16, (unsigned short)lw);
            const double wg = w * (double)par[P_BLK0 + PB_LN1G + f0 + e];
#pragma unroll
            for (int d = 0; d < 4; d++) acc[d] += wg * ((double)par[P_PP + (f0 + e) * 4 + d] - m[d]);
            acc[4] += w * (double)par[P_BLK0 + PB_LN1B + f0 + e];
        }
    }
#pragma unroll
    for (int d = 0; d < 5; d++) red[t][d] = acc[d];
    __syncthreads();
    if (t < 32) {
        // output row t of the tile sits in register r of lane half hh with row(r, hh) = t
        const int hh = (t >> 2) & 1, r = (t & 3) + 4 * (t >> 3), o = tile * 32 + hh * 16 + r;
        double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < B0_THREADS / 64; w++)
#pragma unroll
            for (int d = 0; d < 5; d++) sum[d] += red[w * 64 + t][d] + red[w * 64 + 32 + t][d];
#pragma unroll
        for (int d = 0; d < 4; d++) out[B0_T + o * 4 + d] = (float)sum[d];
        out[B0_C + o] = (float)(sum[4] + (double)par[P_BLK0 + PB_BQKV + o]);
    }
    if (tile < C / 32 && t < 32) out[B0_BPROJ + tile * 32 + t] = par[P_BLK0 + PB_BPROJ + tile * 32 + t];
}

// BLOCK 0 STREAM of every image, from its split program and its table (block0_window_kernel, earlier on the stream): one
// workgroup per (image, head).  The rows of the ten rank-5 operands meet in LDS in A-row order: q, k, v = [T | c] of the
// table; U_lt = c K_lt [T_q | c_q] summed in double over the head's 32 features in order, from hi + lo of the K records,
// rounded once to float.  Then the 10 packed half-slots and the 29 copied K-blocks go to their slots (host mirror:
// program.block0_stream).
DEV unsigned short f16_bits(float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }
DEV float f16_val(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
constexpr int B0S_OPERANDS = 3 + LT;
__global__ __launch_bounds__(B0_THREADS) void block0_stream_kernel(const char *__restrict__ programs, size_t program_stride_bytes,
                                                                   const float *__restrict__ tables, char *__restrict__ streams) {
    __shared__ float rows[B0S_OPERANDS][32][5];
    const int head = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const char *prog = programs + (size_t)img * program_stride_bytes;
    const float *tbl = tables + (size_t)img * PRM_WINDOW;
    u32x4 *out = reinterpret_cast<u32x4 *>(streams + (size_t)img * B0_STREAM_BYTES) + (size_t)head * B0S_KB_HEAD * KB_U4;
    constexpr int KB_HEAD = G_HEAD / 2, KB_QKV = G_QKV_HEAD / 2;
    if (t < 96) {
        // row `row` of the tile sits at (hh, r) of the row-param order, row(r, hh) = row
        const int part = t >> 5, row = t & 31, hh = (row >> 2) & 1, r = (row & 3) + 4 * (row >> 3);
        const int o = (head * 3 + part) * 32 + hh * 16 + r;
#pragma unroll
        for (int d = 0; d < 4; d++) rows[part][row][d] = tbl[B0_T + o * 4 + d];
        rows[part][row][4] = tbl[B0_C + o];
    }
    __syncthreads();
    if (t < LT * 32) {
        const int lt = t >> 5, row = t & 31;
        double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int f = 0; f < HD; f++) {
            const int hh = (f >> 2) & 1, r = (f & 3) + 4 * (f >> 3), j = r >> 3, e = r & 7;
            const unsigned short *rec = reinterpret_cast<const unsigned short *>(
                prog + (size_t)(head * KB_HEAD + KB_QKV + 4 * lt + j) * (KB_U4 * 16) + (row + 32 * hh) * 16);
            const double kv = (double)f16_val(rec[e]) + (double)f16_val(rec[512 + e]);     // lo half: 1 KiB further on
#pragma unroll
            for (int d = 0; d < 5; d++) acc[d] += kv * (double)rows[0][f][d];
        }
        const double c = 0.17677669529663688110 * 1.44269504088896340736;   // 32^-1/2 log2 e
#pragma unroll
        for (int d = 0; d < 5; d++) rows[3 + lt][row][d] = (float)(acc[d] * c);
    }
    __syncthreads();
    for (int i = t; i < B0S_OPERANDS * 64; i += B0_THREADS) {
        const int op = i >> 6, lane = i & 63, row = lane & 31, pair = op >> 1;
        unsigned short h[5], d[5], l[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const float x = rows[op][row][k];
            h[k] = f16_bits(x);
            const float hf = f16_val(h[k]);
            l[k] = f16_bits((x - hf) * B0S_LO_SCALE);
            d[k] = f16_bits(hf * (1.0f / B0S_LO_SCALE));
        }
        auto pk = [](unsigned short a, unsigned short b) { return (unsigned)a | ((unsigned)b << 16); };
        const u32x4 w = lane < 32 ? u32x4{pk(h[0], h[1]), pk(h[2], h[3]), pk(d[0], d[1]), pk(d[2], d[3])}
                                  : u32x4{pk(l[0], l[1]), pk(l[2], l[3]), pk(h[4], d[4]), pk(l[4], 0)};
        const int slot = pair < 2 ? pair : 5 * pair - 6;         // [q|k] 0, [v|U0] 1, [U1|U2] 4, [U3|U4] 9, [U5|U6] 14
        out[slot * KB_U4 + (op & 1) * 64 + lane] = w;
    }
    constexpr int NV = 2 * LT - 1, NCOPY = NV + 2 * NT;          // 13 V K-blocks, 16 proj K-blocks
    for (int i = t; i < NCOPY * KB_U4; i += B0_THREADS) {
        const int cb = i / KB_U4, w = i - cb * KB_U4;
        int src, dst;
        if (cb < NV) {
            const int lt = cb >> 1, j = cb & 1;
            src = KB_QKV + 4 * lt + 2 + j;
            dst = lt == 0 ? 2 + j : 4 + 5 * ((lt - 1) >> 1) + 1 + 2 * ((lt - 1) & 1) + j;
        } else {
            src = KB_HEAD - 2 * NT + (cb - NV);
            dst = B0S_KB_HEAD - 2 * NT + (cb - NV);
        }
        out[dst * KB_U4 + w] = reinterpret_cast<const u32x4 *>(prog)[(size_t)(head * KB_HEAD + src) * KB_U4 + w];
    }
}

// in front of every split launch: the block-0 tables of the launch's images -> the head of `workspace`, img * 16 KiB.  That
// region (96 MiB) is the exact-fp32 kernel's per-wave slabs, which the split kernel never touches; the fp32 re-evaluation
// that may follow on the stream overwrites it, and the next split launch writes it again.  The tables depend on the weights
// only and could be computed once per weight version, but the program's bytes are pinned (tests compare them with the host
// mirror word for word) and the entry points keep their signatures, so there is nowhere to keep them: 24 small workgroups per image
// per launch (microseconds) against ~8 % of the decode launch.  A plain kernel launch: capturable.
// Behind the tables of all images the compact block-0 streams, 544 KiB per image from 8 more small workgroups, which the
// decode kernel runs block 0 from.  -> the streams, or null: block 0 runs its q/k/v GEMMs from the program, like block 1 -
// with ZS_SPLIT_BLOCK0_GEMM=1 (read per launch: tools/ab_block0_tables.py alternates the two arms) and when tables and
// streams do not both fit (block0_stream_fit: more than 175 images per launch); neither kernel is launched then.
const char *launch_block0_arm(const void *split_programs, size_t program_stride_bytes, int batch, void *workspace,
                              hipStream_t st) {
    const char *e = getenv("ZS_SPLIT_BLOCK0_GEMM");
    if ((e && atoi(e) != 0) || !block0_stream_fit(batch)) return nullptr;
    float *tables = static_cast<float *>(workspace);
    hipLaunchKernelGGL(block0_window_kernel, dim3(HEADS * 3, batch), dim3(B0_THREADS), 0, st,
                       static_cast<const char *>(split_programs), program_stride_bytes, tables);
    char *streams = block0_streams(workspace, batch);
    hipLaunchKernelGGL(block0_stream_kernel, dim3(HEADS, batch), dim3(B0_THREADS), 0, st,
                       static_cast<const char *>(split_programs), program_stride_bytes, tables, streams);
    return streams;
}

// in front of every split launch: the dynamic tile order's counter (in the workspace tail) starts at zero whatever
// the caller's workspace held (a memset node when the stream is being captured); -> static_order of the launch
int launch_counter_reset(void *workspace, hipStream_t st) {
    const char *e = getenv("ZS_SPLIT_STATIC_TILES");                  // read per launch: tools/ab_tile_order.py alternates the arms in one process
    if (e && atoi(e) != 0) return 1;
    (void)hipMemsetAsync(tile_counter(workspace), 0, sizeof(int), st);
    return 0;
}

// The one launch of sdf_decode_split_kernel over the query q, behind the counter reset and the block-0 streams of its images.
int launch_decode_split(const char *who, const void *split_programs, size_t program_stride_bytes, int batch, const Query &q,
                        float *out, int *tile_flags, void *workspace, void *stream) {
    if (q.m == 0) return 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int static_order = launch_counter_reset(workspace, st);
    const char *b0s = launch_block0_arm(split_programs, program_stride_bytes, batch, workspace, st);
    hipLaunchKernelGGL(q.points ? sdf_decode_split_kernel<false> : sdf_decode_split_kernel<true>,
                       dim3(decode_grid_size(batch, q.m)), dim3(WAVES * 64), 0, st,
                       static_cast<const char *>(split_programs), program_stride_bytes, batch, q.points, q.axis, q.G,
                       q.first_point, q.m, out, q.apply_sigmoid, static_cast<f32x4 *>(workspace), tile_flags, static_order, b0s);
    return zs::check_launch(who) ? 1 : 0;
}

}  // namespace

extern "C" int zs_sdf_split_programs(const void *programs, size_t program_stride_bytes,
                                     void *split_programs, size_t split_stride_bytes, int batch,
                                     void *stream) {
    if (batch < 0 || batch > 65535) {
        zs::set_err("zs_sdf_split_programs: bad batch %d", batch);
        return 0;
    }
    if (batch == 0) return 1;
    if (!check_programs("zs_sdf_split_programs", programs, program_stride_bytes) ||
        !check_programs("zs_sdf_split_programs", split_programs, split_stride_bytes))
        return 0;
    const int elems = (REC_FLOATS / (KB_U4 * 4)) * 64 + PARAM_FLOATS / 4;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemset2DAsync(static_cast<char *>(split_programs) + (size_t)(REC_FLOATS + P_FLAG) * 4, split_stride_bytes,
                         0, 16, batch, st) != hipSuccess) {
        zs::set_err("zs_sdf_split_programs: hipMemset2DAsync failed");
        return 0;
    }
    hipLaunchKernelGGL(split_program_kernel, dim3((elems + 255) / 256, batch), dim3(256), 0, st,
                       static_cast<const float *>(programs), program_stride_bytes / sizeof(float),
                       static_cast<u32x4 *>(split_programs), split_stride_bytes / sizeof(u32x4));
    hipLaunchKernelGGL(k_bound_kernel, dim3(BLOCKS * HEADS, batch), dim3(256), 0, st,
                       static_cast<const float *>(programs), program_stride_bytes / sizeof(float),
                       static_cast<u32x4 *>(split_programs), split_stride_bytes / sizeof(u32x4));
    return zs::check_launch("zs_sdf_split_programs") ? 1 : 0;
}

extern "C" int zs_sdf_block0_tables(const void *split_programs, size_t program_stride_bytes, int batch, float *tables,
                                    void *stream) {
    if (batch < 0 || batch > 65535) {
        zs::set_err("zs_sdf_block0_tables: bad batch %d", batch);
        return 0;
    }
    if (batch == 0) return 1;
    if (!tables) {
        zs::set_err("zs_sdf_block0_tables: null pointer");
        return 0;
    }
    if (!check_programs("zs_sdf_block0_tables", split_programs, program_stride_bytes)) return 0;
    hipLaunchKernelGGL(block0_window_kernel, dim3(HEADS * 3, batch), dim3(B0_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const char *>(split_programs), program_stride_bytes, tables);
    return zs::check_launch("zs_sdf_block0_tables") ? 1 : 0;
}

extern "C" int zs_sdf_block0_streams(const void *split_programs, size_t program_stride_bytes, int batch, const float *tables,
                                     void *streams, void *stream) {
    if (batch < 0 || batch > 65535) {
        zs::set_err("zs_sdf_block0_streams: bad batch %d", batch);
        return 0;
    }
    if (batch == 0) return 1;
    if (!tables || !streams) {
        zs::set_err("zs_sdf_block0_streams: null pointer");
        return 0;
    }
    if (!check_programs("zs_sdf_block0_streams", split_programs, program_stride_bytes)) return 0;
    hipLaunchKernelGGL(block0_stream_kernel, dim3(HEADS, batch), dim3(B0_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const char *>(split_programs), program_stride_bytes, tables, static_cast<char *>(streams));
    return zs::check_launch("zs_sdf_block0_streams") ? 1 : 0;
}

extern "C" int zs_sdf_query_points_split(const void *split_programs, size_t program_stride_bytes,
                                         int batch, const float *points, int m, float *logits,
                                         int *tile_flags, void *workspace, void *stream) {
    static const char who[] = "zs_sdf_query_points_split";
    Query q;
    if (!points_query(who, split_programs, program_stride_bytes, batch, points, m, logits, workspace, q)) return 0;
    return launch_decode_split(who, split_programs, program_stride_bytes, batch, q, logits, tile_flags, workspace, stream);
}

extern "C" int zs_sdf_query_grid_range_split(const void *split_programs, size_t program_stride_bytes,
                                             int batch, const float *axis, int G, long long point_begin,
                                             long long point_end, int apply_sigmoid, float *out,
                                             int *tile_flags, void *workspace, void *stream) {
    static const char who[] = "zs_sdf_query_grid_range_split";
    Query q;
    if (!grid_range_query(who, "range", split_programs, program_stride_bytes, batch, axis, G, point_begin, point_end,
                          apply_sigmoid, out, workspace, q))
        return 0;
    return launch_decode_split(who, split_programs, program_stride_bytes, batch, q, out, tile_flags, workspace, stream);
}

extern "C" int zs_sdf_query_grid_split(const void *split_programs, size_t program_stride_bytes,
                                       int batch, const float *axis, int G, int slice_begin,
                                       int slice_end, int apply_sigmoid, float *out, int *tile_flags,
                                       void *workspace, void *stream) {
    static const char who[] = "zs_sdf_query_grid_split";
    Query q;
    if (!grid_slices(who, batch, G, slice_begin, slice_end) ||
        !grid_range_query(who, "slab", split_programs, program_stride_bytes, batch, axis, G,
                          (long long)slice_begin * G * G, (long long)slice_end * G * G, apply_sigmoid, out, workspace, q))
        return 0;
    return launch_decode_split(who, split_programs, program_stride_bytes, batch, q, out, tile_flags, workspace, stream);
}
