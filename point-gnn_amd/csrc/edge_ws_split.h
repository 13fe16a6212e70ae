// Split-precision forms of the weights-stationary edge kernel (edge_ws.h): the
// same fused stage
//     out[d] = max over edges (s -> d) of ReLU( ReLU(P[s] - Q[d]) W + b ),
// with the 300x300 product evaluated on the 16-bit matrix pipe instead of the
// fp32 one.  SECONDARY paths (bench.py `secondary_bf16x3`, edge_arith =
// 'bf16x3' / 'f16x2'): the fp32-MFMA kernel stays the default and the parity
// reference.  ONE kernel body, edge_ws_split_body<Arith, KB, NTG>; the two
// arithmetics are the policy structs Bf16x3 and F16x2 below, which hold what
// differs -- how a block is split, which MFMAs run in which order and when a
// fragment register is requested again, the accumulators and how they fold, the
// constants of the issue pattern -- and nothing else.
//
// Why.  v_mfma_f32_16x16x4_f32 runs at the VALU's rate (157 TFLOP/s, and
// nothing issues beside it: edge_ws.h); the 16-bit matrix core is 16x faster.
//
// Bf16x3.  An fp32 value is EXACTLY the sum of three bf16 values (8 + 8 + 8
// significand bits): x = x0 + x1 + x2, every residual exact in fp32.  With
// both operands split,
//     x w = sum_{i+j<=2} x_i w_j  +  (x1 w2 + x2 w1 + x2 w2),
// and the three dropped terms are below 2^-24 |x w| -- what one fp32 FMA
// commits.  Every kept product of two bf16 values is exact in fp32, so six bf16
// MFMAs accumulating in fp32 reproduce the fp32 product to fp32 rounding; what
// remains is the accumulation's own fp32 rounding, of which this form has
// fewer steps (one per 32-wide block and term instead of one per element).
// Measured on the bench frames: max |logit - float64 oracle| no larger than the
// fp32-MFMA kernel's (tests/test_gpu_bf16x3.py prints both).
//   Cost.  6 x v_mfma_f32_16x16x32_bf16 (16 cycles each) per 32 x 16 x 16 block
// = 96 cycles against 8 x 32 = 256 for fp32: 2.67x fewer matrix cycles; three
// bf16 images of the weights (6 bytes per weight) put 19 column tiles in FOUR
// groups of 5/5/5/4 (150 KiB) instead of three, i.e. the rows are gathered and
// split four times; and the split is VALU work per gathered element.
//   The split: first part rounded to nearest (v_cvt_pk_bf16_f32), the 16
// residual bits cut in two by truncation (v_and + exact v_sub, packed with
// v_perm): still x = x0 + x1 + x2 exactly, 60 instructions per block, dropped
// terms 1.2e-7 against the fp32 chain's 4.9e-6 (NumPy model, 20 000 x 300 x
// 300).  Tried and dropped: all three parts rounded (68 instructions: + 3 %);
// all three cut (60; dropped terms 2.6e-7, but its error against float64 is
// 1.4x the fp32 kernel's on the C = 256 test where the others' is 1.0x).
//
// F16x2.  BOTH operands are represented by TWO fp16 values,
//     x ~ x0 + x1' / 2^11,   x0 = fp16(x),  x1' = fp16((x - x0) 2^11)
// (round to nearest; the residual x - x0 is exact in fp32 and the scaling keeps
// it out of fp16's subnormals), and three fp16 MFMAs per 32-wide block,
//     x w ~ x0 w0  +  (x0 w1' + x1' w0) / 2^11,
// the first into one fp32 accumulator, the other two into a second one; every
// product of two fp16 values (11 + 11 significand bits) is exact in fp32.
// Against Bf16x3: half the matrix instructions, 44 instead of 60 split
// instructions per block and 4 bytes per weight in LDS -- THREE column groups
// (7/6/6 tiles, 140 KiB) instead of four, i.e. the rows are gathered and
// split three times.
//   What it gives up.  Each operand carries 22 significand bits, not 24: a
// relative representation error <= 2^-22 per element (the fp32 value's own is
// 2^-24), plus the dropped x1 w1 term (2^-22).  In the sum of 300 products the
// fp32 FMA chain's accumulated rounding dominates: NumPy model (20 000 x 300 x
// 300): this form's truncation error 9.3e-8 rms / 1.0e-6 max against the fp32
// chain's 2.7e-7 / 4.5e-6 -- the distance to float64 grows by ~6 %.  The
// parity tests hold it to the same bars as 'bf16x3' (tests/conftest.py:
// edge_arith).
//   Range.  fp16 ends at 65504.  The gathered operand h = ReLU(P[s] - Q[d]) is
// clamped there by the v_med3_f32 that is its ReLU (no extra instruction), and
// the kernel raises bit 0 of `status` when some h COULD have reached 32768 (an
// element of P or Q at or above 16384 in magnitude, or not a number: checked
// in the kernel's prologue): the caller reruns the stage in fp32 (run.py's
// frame loop does; a trained Point-GNN's activations are below 100).  The
// weights' image is built on the host, which refuses weights outside fp16's
// range.
//
// Layouts.  v_mfma_f32_16x16x32_bf16 / _f16, transposed product out^T = W^T h^T:
//   A (weights)      lane (g, i): W[32 kb + 8 g + j][16 t + i], j = 0..7
//   B (activations)  lane (g, n): h[row n][32 kb + 8 g + j],    j = 0..7
//   C / D            lane (g, n), register r <-> feature 16 t + 4 g + r of row n
// (C / D as in edge_ws.h, so the segmented-max epilogue is shared).  A lane's
// eight 16-bit values are four u32, element 2 m in the low half.  The image
// pgnn_pack_fc_bf16x3 / pgnn_pack_fc_f16x2 writes is [kb][t][part][lane][4 u32]
// (1 KiB fragments; f16x2: part 0 = w0, 1 = w1'), the layer's bias (fp32,
// 16 nt values) behind it.  Rows of P / Q are 304 floats: the last 32-block of
// C = 300 covers features 288..319, the lanes with g >= 2 re-read the row's
// last 16 bytes (finite values) against zero weights.
//
// Schedule (round 5; the round-4 body alternated a VALU phase -- gather, ReLU,
// split -- with an MFMA phase per half tile and left the overlap to the SIMD's
// two waves: it does not happen, profiles/r04_pmc_sq_bf16x3.txt shows VALU and
// matrix pipe busy together for 7 % of the matrix cycles and a kernel time
// equal to the SUM of the phases, at any wave priority).  What was measured,
// step by step (tools/micro/mfma_mix.hip -> profiles/r05_mfma_mix.txt,
// profiles/r05_bf16x3_steps.txt):
//   * beside a stream of v_mfma_f32_16x16x32_bf16 the MFMA takes two of the
//     four issue slots of its 16 cycles; v_sub / v_and / v_med3 / v_perm /
//     v_cvt_pk_bf16_f32 take one each: TWO per MFMA are free, every further one
//     costs 4 cycles, a DEPENDENT neighbour 3 more -- and one v_pk_add_f32
//     costs 14-16 cycles that overlap nothing (packed fp32 holds the matrix
//     pipe): as much as the MFMA itself.  The round-4 body had 12 per block.
//   * the overlap is therefore written into ONE wave's instruction stream: a
//     software pipeline over the tile's K blocks in which the kTerms NTG MFMAs
//     of block kb are interleaved (sched_group_barrier: one MFMA, two VALU)
//     with the split of block kb + 1 -- kSplitValu single-slot instructions,
//     stage by stage over the block's eight elements so that neighbours are
//     independent --, the fragment requests of block kb + 1 and the row
//     requests of blocks kb + DQ (Q) / kb + DP (P), across the tile boundary
//     (the next tile's first blocks are requested and split under the last
//     MFMAs of this one).
//   * the four 1 KiB row requests of a block are spread over it: issued back
//     to back they stall the in-order wave at the address path (16 cycles per
//     request): 677 us against 598.
//   * at the tile boundary the dst of the row above comes through a DPP row
//     shift, not __shfl_up: a ds_bpermute has to wait for lgkmcnt(0), i.e. for
//     the fifteen fragment requests of the next tile issued just before.
//   * f16x2's range guard is one pass over P and Q (8 MB) shared by all
//     workgroups instead of a running maximum of the first parts in the MFMA
//     loop: 4 instructions per block, 4 % of the kernel.
//   * tried and dropped: segment-aligned tiles with the tile's Q row held in
//     registers, distributed over the lanes and read through the DPP operand
//     row_newbcast:kb of the subtraction (v_subrev_f32_dpp; two row requests
//     per tile instead of twenty): + 4 % tiles, 594-600 us against 577 on the
//     same box at C = 300, 1438 against 1483 at C = 256.
//   * the timing ablations behind these figures (builds that computed WRONG
//     results: one part or one term only, fragments read once, no split
//     arithmetic, every row request to row 0, no segmented max, one wave per
//     SIMD) are no longer in the source; what they found is the list above and
//     profiles/r05_bf16x3_steps.txt.
//
//   live per lane (Bf16x3): parts of 2 blocks (24), raw P of 3 blocks (24), raw
//   Q of 2 (16), 3 NTG fragments (60), accumulators + carry (40); 189 VGPRs
#pragma once
#include <type_traits>
#include <utility>

#include "edge_ws.h"

#if defined(PGNN_B16_ABL) || defined(PGNN_F16_ABL) || defined(PGNN_B16_TRUNC)
#error "PGNN_B16_ABL / PGNN_F16_ABL / PGNN_B16_TRUNC: the ablation builds of the split kernels ended with the commit that merged them into edge_ws_split.h; this build would time the normal kernel"
#endif
// request distances: raw P rows are requested DP blocks ahead of their split,
// raw Q rows (L1-hot: mostly one dst per tile) DQ blocks; an f16x2 block is
// half as long as a bf16x3 one (3 MFMAs per column tile, not 6)
#ifndef PGNN_B16_DP
#define PGNN_B16_DP 3
#endif
#ifndef PGNN_B16_DQ
#define PGNN_B16_DQ 2
#endif
#ifndef PGNN_F16_DP
#define PGNN_F16_DP PGNN_B16_DP
#endif
#ifndef PGNN_F16_DQ
#define PGNN_F16_DQ PGNN_B16_DQ
#endif

namespace pgnn {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32;
typedef u32 v4u __attribute__((ext_vector_type(4)));

constexpr float kF16Scale = 2048.0f;  // 2^11
constexpr float kF16Max = 65504.0f;

// (lo, hi) -> packed bf16 / fp16 pair, round to nearest even: v_cvt_pk_bf16_f32
// / v_cvt_pk_f16_f32 (not an asm statement: the scheduler's instruction groups
// count it as VALU)
__device__ __forceinline__ u32 cvt_pk_bf16(float lo, float hi) {
  return __builtin_bit_cast(u32, __builtin_convertvector((v2f){lo, hi}, bf16x2));
}
__device__ __forceinline__ u32 cvt_pk_f16(float lo, float hi) {
  return __builtin_bit_cast(u32, __builtin_convertvector((v2f){lo, hi}, f16x2));
}

// (hi & 0xffff0000) | (lo >> 16): two floats' upper halves, i.e. their bf16
// truncations, packed
__device__ __forceinline__ u32 perm_hi16(u32 hi, u32 lo) {
  return __builtin_amdgcn_perm(hi, lo, 0x07060302u);
}

__device__ __forceinline__ v4f mfma_bf16(v4u a, v4u b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ v4f mfma_f16(v4u a, v4u b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(
      __builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// a - (float)half of `pk` (lo / hi): exact, ONE instruction (v_fma_mix_f32 with
// an fp16 first operand).  An asm statement: written in C, hipcc converts,
// subtracts with v_pk_add_f32 and scales with v_pk_mul_f32 -- packed fp32
// arithmetic holds the matrix pipe (see the header).
__device__ __forceinline__ float sub_half_lo(float a, u32 pk) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(pk), "v"(a));
  return r;
}
__device__ __forceinline__ float sub_half_hi(float a, u32 pk) {
  float r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=v"(r)
      : "v"(pk), "v"(a));
  return r;
}

// ReLU(p - q) of 8 consecutive features -> three packed bf16 parts, stage by
// stage over the eight elements; no packed fp32 arithmetic (see the header)
__device__ __forceinline__ void split_block_bf16(const v4f (&p)[2],
                                                 const v4f (&q)[2], v4u &x0,
                                                 v4u &x1, v4u &x2, float inf) {
  float a[8], r[8], s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = p[e >> 2][e & 3] - q[e >> 2][e & 3];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = max_nc(a[e], 0.0f, inf);
#pragma unroll
  for (int j = 0; j < 4; ++j) x0[j] = cvt_pk_bf16(a[2 * j], a[2 * j + 1]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[2 * j] = __uint_as_float(x0[j] << 16);
    r[2 * j + 1] = __uint_as_float(x0[j] & 0xffff0000u);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = a[e] - r[e];  // exact
#pragma unroll
  for (int j = 0; j < 4; ++j)
    x1[j] = perm_hi16(__float_as_uint(r[2 * j + 1]), __float_as_uint(r[2 * j]));
#pragma unroll
  for (int e = 0; e < 8; ++e)
    s[e] = __uint_as_float(__float_as_uint(r[e]) & 0xffff0000u);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = r[e] - s[e];  // exact, <= 8 bits
#pragma unroll
  for (int j = 0; j < 4; ++j)
    x2[j] = perm_hi16(__float_as_uint(s[2 * j + 1]), __float_as_uint(s[2 * j]));
}

// min(ReLU(p - q), 65504) of 8 consecutive features -> two packed fp16 parts
// (44 instructions, stage by stage); gmax: running packed-u16 maximum of x0
// (TRACK: pool_ws_f16.h's range guard)
template <bool TRACK = true>
__device__ __forceinline__ void split_block_f16(const v4f (&p)[2], const v4f (&q)[2],
                                                v4u &x0, v4u &x1, u32 &gmax) {
  float a[8], r[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = p[e >> 2][e & 3] - q[e >> 2][e & 3];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = __builtin_amdgcn_fmed3f(a[e], 0.0f, kF16Max);
#pragma unroll
  for (int j = 0; j < 4; ++j) x0[j] = cvt_pk_f16(a[2 * j], a[2 * j + 1]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[2 * j] = sub_half_lo(a[2 * j], x0[j]);
    r[2 * j + 1] = sub_half_hi(a[2 * j + 1], x0[j]);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = __builtin_ldexpf(r[e], 11);  // v_ldexp_f32
#pragma unroll
  for (int j = 0; j < 4; ++j) x1[j] = cvt_pk_f16(r[2 * j], r[2 * j + 1]);
  // (an asm statement: written with __builtin_elementwise_max on two-half
  // vectors, hipcc 7.2 keeps ONE of the four maxima)
  if constexpr (TRACK) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      asm("v_pk_max_u16 %0, %0, %1" : "+v"(gmax) : "v"(x0[j]));
  }
}

// f(std::integral_constant<int, I>) for every I of the sequence
template <class F, int... I>
__device__ __forceinline__ void for_each_int(F &&f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}

// ---- the two arithmetics -----------------------------------------------------
// A policy holds what differs between them, as data wherever that is possible:
// the kernel body executes it in its own loops, with the step table expanded at
// compile time (for_each_int).  Two forms that read better were tried and
// change the machine code: a policy function mma_block(acc, w, ...) is
// optimised on its own before it is inlined, and hipcc then orders the MFMAs
// differently; a run-time loop over the table computes the fragment addresses
// in another order (f16x2: + 2.4 % kernel time).
//   kParts      16-bit parts per operand (= fragments per (kb, t) of the image)
//   kAccs       fp32 accumulators per column tile (c = 0: acc, 1: alo); the
//               product is acc + kLoScale alo
//   kSplitValu  instructions of split() the scheduler's groups see
//   block(i)    step i of the kSteps of one K block, {op, part, xpart, c}: the
//               MFMAs of a term, accumulator c += w[part] x[xpart] over the
//               column tiles (kTerms of them; term-major:
//               consecutive MFMAs hit different accumulators) and, between
//               them, the requests that refill the registers of w[part] --
//               with the fragments of the NEXT block (block 0 again behind the
//               last; they are what the next block expects to find loaded), or
//               of THIS block (for a term further down)
//   frag_after  a fragment request is issued behind the block's m-th MFMA
struct WsSplitStep {
  enum Op { kMma, kNext, kThis } op;
  int part, xpart, c;
};

struct Bf16x3 {
  static constexpr int kParts = 3, kAccs = 1, kSplitValu = 60;
  static constexpr float kLoScale = 0.0f;
  static constexpr int DP = PGNN_B16_DP, DQ = PGNN_B16_DQ;
  static constexpr bool kRangeGuard = false;
  // in an order that frees a weight part's registers as early as possible --
  // (w2 x0) | (w1 x1) (w1 x0) | (w0 x2) (w0 x1) (w0 x0) --; a part's fragments
  // of the next block are requested when it is done
  static constexpr int kSteps = 9, kTerms = 6;
  static constexpr __host__ __device__ WsSplitStep block(int i) {
    constexpr WsSplitStep b[kSteps] = {
        {WsSplitStep::kMma, 2, 0, 0}, {WsSplitStep::kNext, 2, 0, 0},
        {WsSplitStep::kMma, 1, 1, 0}, {WsSplitStep::kMma, 1, 0, 0},
        {WsSplitStep::kNext, 1, 0, 0},
        {WsSplitStep::kMma, 0, 2, 0}, {WsSplitStep::kMma, 0, 1, 0},
        {WsSplitStep::kMma, 0, 0, 0}, {WsSplitStep::kNext, 0, 0, 0}};
    return b[i];
  }
  // after every second MFMA from the second term on
  static constexpr bool frag_after(int m, int ntg) {
    return m >= ntg && (m - ntg) % 2 == 1 && (m - ntg) / 2 < 3 * ntg;
  }
  static __device__ __forceinline__ v4f mfma(v4u a, v4u b, v4f c) {
    return mfma_bf16(a, b, c);
  }
  static __device__ __forceinline__ void split(const v4f (&p)[2],
                                               const v4f (&q)[2],
                                               v4u (&x)[kParts], float inf) {
    split_block_bf16(p, q, x[0], x[1], x[2], inf);
  }
};

struct F16x2 {
  // (36 of the split's 44 instructions are visible to the scheduler's groups:
  // the eight v_fma_mix_f32 are asm statements and place themselves)
  static constexpr int kParts = 2, kAccs = 2, kSplitValu = 36;
  static constexpr float kLoScale = 1.0f / kF16Scale;
  static constexpr int DP = PGNN_F16_DP, DQ = PGNN_F16_DQ;
  static constexpr bool kRangeGuard = true;
  // (w0 x0) -> hi | (w0 x1') -> lo | (w1' x0) -> lo.  w1' of THIS block is
  // requested under the first term (its registers were last read by the
  // previous block's last term), w0 of the next block under the last term.
  static constexpr int kSteps = 5, kTerms = 3;
  static constexpr __host__ __device__ WsSplitStep block(int i) {
    constexpr WsSplitStep b[kSteps] = {
        {WsSplitStep::kThis, 1, 0, 0}, {WsSplitStep::kMma, 0, 0, 0},
        {WsSplitStep::kMma, 0, 1, 1}, {WsSplitStep::kNext, 0, 0, 0},
        {WsSplitStep::kMma, 1, 0, 1}};
    return b[i];
  }
  // after every MFMA of the first and of the last term
  static constexpr bool frag_after(int m, int ntg) {
    return m < ntg || m >= 2 * ntg;
  }
  static __device__ __forceinline__ v4f mfma(v4u a, v4u b, v4f c) {
    return mfma_f16(a, b, c);
  }
  static __device__ __forceinline__ void split(const v4f (&p)[2],
                                               const v4f (&q)[2],
                                               v4u (&x)[kParts], float) {
    u32 unused = 0;
    split_block_f16<false>(p, q, x[0], x[1], unused);
  }
};

// tiles [tile_first, tile_last) of 16 edge rows, column tiles t0 .. t0+NTG-1
// whose fragments sit in `wl` ([KB][NTG][kParts][64] v4u)
template <class Arith, int KB, int NTG>
__device__ __forceinline__ void edge_ws_split_body(const EdgeWsArgs &a,
                                                   const v4u *__restrict__ wl,
                                                   int t0, const float *bias_lds,
                                                   int64_t tile_first,
                                                   int64_t tile_last, int lane,
                                                   const int64_t E) {
  constexpr int kParts = Arith::kParts, DP = Arith::DP, DQ = Arith::DQ;
  constexpr int kLo = Arith::kAccs == 2 ? NTG : 1;  // second accumulators
  static_assert(DP >= 2 && DQ >= 2 && DP < KB && DQ < KB, "request distances");
  constexpr int kMfmas = Arith::kTerms * NTG;  // of a block
  constexpr int kValuPerMfma = (Arith::kSplitValu + kMfmas - 1) / kMfmas;
  constexpr int kLoadEvery = kMfmas / 4;  // four row requests per block
  constexpr int kNext = KB - 1 - (DP > DQ ? DP : DQ);  // block that sets up the next tile's rows
  static_assert(kNext >= 0, "request distances");
  if (tile_first >= tile_last) return;
  const int n = lane & 15;
  const int64_t e_first = tile_first * 16;
  const int64_t e_end = tile_last * 16 < E ? tile_last * 16 : E;
  const v4f *__restrict__ P4 = reinterpret_cast<const v4f *>(a.P);
  const v4f *__restrict__ Q4 = reinterpret_cast<const v4f *>(a.Q);
  const int2 *__restrict__ e2 = reinterpret_cast<const int2 *>(a.edges);
  const int last = a.ldv4 - 1;

  // the open run: as in edge_ws_body
  int cur_d = e_first > 0 ? a.edges[2 * (e_first - 1) + 1] : -1;
  int d_after = e_end < E ? a.edges[2 * e_end + 1] : -1;
  cur_d = __builtin_amdgcn_readfirstlane(cur_d);
  d_after = __builtin_amdgcn_readfirstlane(d_after);
  bool cur_left_closed = false, cur_has = false;
  v4f carry[NTG];
#pragma unroll
  for (int t = 0; t < NTG; ++t)
    carry[t] = (v4f){kFloatLowest, kFloatLowest, kFloatLowest, kFloatLowest};
  const float inf = opaque_inf();

  // block kb of a row: v4f 8 kb + 2 g + i of the row; the tail block (lanes
  // g >= 2 of it lie behind the row's 4 * ldv4 floats) from a clamped offset.
  // 32-bit byte offsets from the (scalar) matrix bases, the tail block's
  // precomputed: no address arithmetic between the MFMAs (the launcher
  // refuses matrices of 4 GiB and more)
  struct Rows {
    u32 p, pt, q, qt;
  };
  auto rows_of = [&](int2 e, bool ok, int g, int toff) -> Rows {
    const int s = ok ? e.x : 0;
    const int d = ok ? e.y : -1;
    const int dq = ((unsigned)d < (unsigned)a.num_segments) ? d : 0;
    Rows r;
    r.p = ((u32)s * (u32)a.ldv4 + 2u * g) * 16u;
    r.q = ((u32)dq * (u32)a.ldv4 + 2u * g) * 16u;
    r.pt = r.p + 16u * toff;
    r.qt = r.q + 16u * toff;
    return r;
  };
  auto tail_off = [&](int g) {  // relative to row + 2 g
    const int t = 8 * (KB - 1) + 2 * g;
    return (t < last - 1 ? t : last - 1) - 2 * g;
  };
  auto load_blk = [&](const v4f *__restrict__ base, u32 off, u32 off_tail,
                      int kb, v4f (&o)[2]) {
    const char *__restrict__ b = reinterpret_cast<const char *>(base);
    const v4f *__restrict__ src = reinterpret_cast<const v4f *>(
        kb == KB - 1 ? b + (size_t)off_tail : b + (size_t)off + 128 * kb);
    o[0] = src[0];
    o[1] = src[1];
  };

  // ---- before the first tile: its indices, its first blocks, the parts of
  // block 0, the fragments of block 0
  bool cur_ok = e_first + n < E;
  int2 cur = e2[cur_ok ? e_first + n : 0];
  Rows rc = rows_of(cur, cur_ok, lane >> 4, tail_off(lane >> 4));
  // carried round the tile loop: raw P of blocks 1 .. DP-1, raw Q of blocks
  // 1 .. DQ-1 (in flight), the parts of block 0
  v4f pc[DP - 1][2], qc[DQ - 1][2];
  v4u Xc[kParts];
  {
    v4f p0[2], q0[2];
    load_blk(P4, rc.p, rc.pt, 0, p0);
    load_blk(Q4, rc.q, rc.qt, 0, q0);
#pragma unroll
    for (int k = 1; k < DQ; ++k) load_blk(Q4, rc.q, rc.qt, k, qc[k - 1]);
#pragma unroll
    for (int k = 1; k < DP; ++k) load_blk(P4, rc.p, rc.pt, k, pc[k - 1]);
    Arith::split(p0, q0, Xc, inf);
  }
  v4u w[kParts][NTG];
  {
    const v4u *__restrict__ wb = wl + lane;
#pragma unroll
    for (int t = 0; t < NTG; ++t)
#pragma unroll
      for (int i = 0; i < Arith::kSteps; ++i) {
        const WsSplitStep s = Arith::block(i);
        if (s.op == WsSplitStep::kNext)
          w[s.part][t] = wb[(t * kParts + s.part) * 64];
      }
  }

  for (int64_t tile = tile_first;; ++tile) {
    const bool fin = tile >= tile_last;
    const int64_t e0 = tile * 16;
    int lz;  // opaque per-tile lane id: see edge_ws_body
    asm volatile("v_mov_b32 %0, %1" : "=v"(lz) : "v"(lane));
    const int g = lz >> 4;
    const int toff = tail_off(g);
    int lz1 = lz + 64 * 64, lz2 = lz + 128 * 64;
    asm volatile("" : "+v"(lz1));
    asm volatile("" : "+v"(lz2));
    const v4u *__restrict__ wfrag[3] = {wl + lz, wl + lz1, wl + lz2};
    auto frag = [&](int kb, int t, int part) -> v4u {
      const int f = (kb * NTG + t) * kParts + part;
      return wfrag[f >> 6][(f & 63) * 64];
    };
    // (two arrays, not one [kAccs][NTG]: hipcc allocates that one differently)
    v4f acc[NTG], alo[kLo];
#pragma unroll
    for (int t = 0; t < kLo; ++t) alo[t] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NTG; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
    unsigned starts = 1u;  // virtual tile: "row 0 opens a run"
    int my_d = -1;
    if (!fin) {
      my_d = cur_ok ? cur.y : -1;
      // the next tile's indices: requested now, used a few blocks before the end
      const bool nxt_ok = tile + 1 < tile_last && e0 + 16 + n < E;
      const int2 nxt = e2[nxt_ok ? e0 + 16 + n : 0];
      Rows rn = rc;
      // Pb[k], Qb[k]: raw rows of block k; k >= KB: block k - KB of the next tile
      v4f Pb[KB + DP][2], Qb[KB + DQ][2];
      v4u X[KB + 1][kParts];
#pragma unroll
      for (int k = 1; k < DP; ++k) Pb[k][0] = pc[k - 1][0], Pb[k][1] = pc[k - 1][1];
#pragma unroll
      for (int k = 1; k < DQ; ++k) Qb[k][0] = qc[k - 1][0], Qb[k][1] = qc[k - 1][1];
#pragma unroll
      for (int i = 0; i < kParts; ++i) X[0][i] = Xc[i];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        __builtin_amdgcn_sched_barrier(0);
        // (the next tile's row offsets, an iteration before their first use,
        // in a scheduling region of their own: the issue pattern below counts
        // this region's instructions)
        if (kb == kNext) {
          rn = rows_of(nxt, nxt_ok, g, toff);
          __builtin_amdgcn_sched_barrier(0);
        }
        // row requests (vmcnt counts in order: Q, wanted sooner, before P)
        if (kb + DQ < KB)
          load_blk(Q4, rc.q, rc.qt, kb + DQ, Qb[kb + DQ]);
        else
          load_blk(Q4, rn.q, rn.qt, kb + DQ - KB, Qb[kb + DQ]);
        if (kb + DP < KB)
          load_blk(P4, rc.p, rc.pt, kb + DP, Pb[kb + DP]);
        else
          load_blk(P4, rn.p, rn.pt, kb + DP - KB, Pb[kb + DP]);
        // parts of the next block (block 0 of the next tile behind the last)
        Arith::split(Pb[kb + 1], Qb[kb + 1], X[kb + 1], inf);
        // the terms of this block and its fragment requests
        const int kn = kb + 1 < KB ? kb + 1 : 0;
        for_each_int(
            [&](auto i) {
              constexpr WsSplitStep s = Arith::block(i);
#pragma unroll
              for (int t = 0; t < NTG; ++t) {
                if constexpr (s.op == WsSplitStep::kMma && s.c == 0)
                  acc[t] = Arith::mfma(w[s.part][t], X[kb][s.xpart], acc[t]);
                else if constexpr (s.op == WsSplitStep::kMma)
                  alo[t] = Arith::mfma(w[s.part][t], X[kb][s.xpart], alo[t]);
                else
                  w[s.part][t] = frag(s.op == WsSplitStep::kNext ? kn : kb, t, s.part);
              }
            },
            std::make_integer_sequence<int, Arith::kSteps>{});
        // issue order: MFMA, kValuPerMfma VALU (bf16x3: the split is 60
        // instructions per block: two per MFMA at five column tiles, three at
        // four); the fragment requests where the arithmetic wants them; the
        // four row requests apart
#pragma unroll
        for (int m = 0; m < kMfmas; ++m) {
          __builtin_amdgcn_sched_group_barrier(0x8 /*MFMA*/, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x2 /*VALU*/, kValuPerMfma, 0);
          if (Arith::frag_after(m, NTG))
            __builtin_amdgcn_sched_group_barrier(0x100 /*DS read*/, 1, 0);
          if (m % kLoadEvery == 1 && m / kLoadEvery < 4)
            __builtin_amdgcn_sched_group_barrier(0x20 /*VMEM read*/, 1, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 1; k < DP; ++k)
        pc[k - 1][0] = Pb[KB + k][0], pc[k - 1][1] = Pb[KB + k][1];
#pragma unroll
      for (int k = 1; k < DQ; ++k)
        qc[k - 1][0] = Qb[KB + k][0], qc[k - 1][1] = Qb[KB + k][1];
#pragma unroll
      for (int i = 0; i < kParts; ++i) Xc[i] = X[KB][i];
      if constexpr (Arith::kAccs == 2) {
#pragma unroll
        for (int t = 0; t < NTG; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[t][r] = __builtin_fmaf(alo[t][r], Arith::kLoScale, acc[t][r]);
      }
      rc = rn;
      cur = nxt;
      cur_ok = nxt_ok;
      // ---- segmented max over the 16 rows: as in edge_ws_body, but the dst of
      // the row above comes through a DPP row shift (lane n - 1 of the same
      // 16-lane row; lane 0 keeps the open run's id), not __shfl_up
      const int prev = __builtin_amdgcn_update_dpp(cur_d, my_d, 0x111 /*row_shr:1*/,
                                                   0xF, 0xF, false);
      starts = (unsigned)(__ballot(my_d != prev) & 0xFFFFull);
    }  // !fin
    WsRun st = {cur_d, cur_left_closed, cur_has};
    ws_epilogue<NTG>(a, bias_lds, t0, lane, acc, carry, starts, my_d, st, fin,
                     d_after, inf);
    cur_d = st.cur_d;
    cur_left_closed = st.left_closed;
    cur_has = st.has;
    if (fin) break;
  }
}

// a.wp: the image of the layer in Arith's format (pgnn_pack_fc_bf16x3 /
// pgnn_pack_fc_f16x2); static partition of the 16-row tiles as in
// edge_ws_kernel (no tile pool).  status (nullable; kRangeGuard only): bit 0 is
// set when a gathered activation could reach 32768 (see the header)
template <class Arith, int KB, int NTMAX>
__global__ __launch_bounds__(64 * kWsWaves) void edge_ws_split_kernel(
    EdgeWsArgs a, int32_t *status) {
  constexpr int kParts = Arith::kParts;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  v4u *wl = reinterpret_cast<v4u *>(smem);
  float *bias_lds = reinterpret_cast<float *>(wl + KB * NTMAX * kParts * 64);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slice = blockIdx.x % a.xcds;
  const int local = blockIdx.x / a.xcds;
  const int grp = ws_group(a, slice, local, wave);
  const int t0 = a.tile0[grp];
  const int ntg = a.tile0[grp + 1] - t0;
  if constexpr (Arith::kRangeGuard) {
    // ---- range guard, before anything else (its loads overlap the weights'):
    // workgroup b scans rows b, b + gridDim.x, ... of P and Q.  No |P| or |Q|
    // at or above 16384 => every gathered ReLU(P[s] - Q[d]) is below 32768.
    if (status) {
      int nv = a.num_segments;
      if (a.nv_dev) {
        const int d = *a.nv_dev;
        nv = d < nv ? d : nv;
      }
      const v4f *__restrict__ P4 = reinterpret_cast<const v4f *>(a.P);
      const v4f *__restrict__ Q4 = reinterpret_cast<const v4f *>(a.Q);
      float m = 0.0f;
      bool bad = false;
      const int mine = nv > (int)blockIdx.x
                           ? (nv - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x
                           : 0;   // rows blockIdx.x + j * gridDim.x, j < mine
      for (int it = threadIdx.x; it < mine * a.ldv4; it += 64 * kWsWaves) {
        const int j = it / a.ldv4, c = it - j * a.ldv4;
        const size_t at = ((size_t)blockIdx.x + (size_t)j * gridDim.x) * a.ldv4 + c;
        const v4f p = P4[at], q = Q4[at];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          m = fmaxf(m, fmaxf(fabsf(p[i]), fabsf(q[i])));
          bad |= !(p[i] == p[i]) || !(q[i] == q[i]);   // NaN: fmaxf drops it
        }
      }
      if (bad || !(m < 16384.0f)) atomicOr(status, 1);
    }
  }
  // fragments (kb, t, part) of this group -> LDS [kb][t][part][lane]
  ws_stage<(KB * NTMAX * kParts + kWsWaves - 1) / kWsWaves>(
      a, wl, KB * ntg * kParts,
      [&](int f) {
        const int kb = f / (ntg * kParts), r = f - kb * ntg * kParts;  // r = t * kParts + part
        return (size_t)(kb * a.nt + t0) * kParts + r;
      },
      (size_t)KB * a.nt * kParts * 256, t0, ntg, bias_lds, wave, lane);
  __syncthreads();
  const int64_t n_edges = ws_edge_count(a.n_edges, a.n_dev);
  const WsShare s = ws_share(a, grp, slice, local, wave, (n_edges + 15) / 16);
  const int64_t span = s.last - s.first;
  const int64_t tile_first = s.first + span * s.wi / s.nw;
  const int64_t tile_last = s.first + span * (s.wi + 1) / s.nw;
  if (ntg == NTMAX)
    edge_ws_split_body<Arith, KB, NTMAX>(a, wl, t0, bias_lds, tile_first,
                                         tile_last, lane, n_edges);
  else
    edge_ws_split_body<Arith, KB, NTMAX - 1>(a, wl, t0, bias_lds, tile_first,
                                             tile_last, lane, n_edges);
}

}  // namespace pgnn
