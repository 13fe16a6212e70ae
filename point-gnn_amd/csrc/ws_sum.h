// Sum epilogue of the weights-stationary kernels (edge_ws.h, pool_ws.h):
//     out[d] = sum over edges (s -> d) of act( h W + b )
// -- tf.math.unsorted_segment_sum of the per-edge rows (gnn.py:111-114); the
// mean (gnn.py:116-119) is this sum followed by one finishing pass over `out`
// (scatter_max.hip, segment_mean_finish).
//
// A fragment of edge_ws.h, included there behind ws_epilogue: it uses that
// file's v4f, dpp_mov, WsRun and kFloatLowest and has the call signatures of
// ws_flush / ws_epilogue, so that a kernel body chooses between the two with
// its policy parameter (WsMax / WsSum) and nothing else about it changes.
//
// What is different from the max:
//   * bias and ReLU are NOT monotone maps that commute with the reduction:
//     max_r act(a_r + b) == act(max_r a_r + b), but sum_r act(a_r + b) is not
//     act(sum_r a_r + b).  They are applied to every row of the tile before it
//     is added -- the expression the EMIT kernels write their rows with
//     (edge_ws.h: acc[t][r] + bias, then the ReLU select), so the summed values
//     are bit for bit the rows those kernels emit.  4 NTG adds and selects per
//     tile more than the max;
//   * the identity of an open run is 0, and rows outside the run are added as
//     0 instead of being masked with lowest();
//   * a run that is not a whole segment is added to `out` with a float atomic
//     add, so `out` must hold 0 (not lowest()) when the kernel starts, and the
//     value of a segment that spans ranges depends on the order in which the
//     waves arrive (fp32 addition is not associative): run-to-run differences
//     of the last bits, as in TensorFlow's own kernel;
//   * the sum is not idempotent: a (row tile, column group) covered twice, a
//     run flushed twice or a pool chunk overlapping a static range -- all
//     invisible under max -- are wrong results here.
#pragma once

namespace pgnn {

// the policy parameter of the kernel bodies
struct WsMax {
  static constexpr bool kSum = false;
};
struct WsSum {
  static constexpr bool kSum = true;
};

template <int NTG>
__device__ __forceinline__ float ws_v0(const v4f (&v)[NTG], int i) {
  return i < 4 * NTG ? v[i >> 2][i & 3] : 0.0f;
}

// out[d][16 (t0 + t) + 4 g + r] <- sum over the 16 rows of `v` (rows that are
// finished: bias and ReLU applied): plainly when the run is a whole segment,
// with a float atomic add otherwise.  The reduce-scatter of ws_flush with + in
// place of the median-max: two DPP steps, two __shfl_xor steps, lane n ends up
// with the sums of registers n and 16 + n.
template <int NTG, class ARGS>
__device__ __forceinline__ void ws_flush_sum(const ARGS &a, const float *bias_lds,
                                             int t0, int lane, int d,
                                             const v4f (&v)[NTG], bool whole,
                                             float inf) {
  (void)bias_lds;
  (void)inf;
  if (d < 0 || d >= a.num_segments) return;  // wave-uniform
  int zero;  // (opaque: see ws_flush)
  asm volatile("s_mov_b32 %0, 0" : "=s"(zero));
  const int n = (lane & 15) + zero, g = lane >> 4;
  const bool b0 = n & 1, b1 = n & 2, b2 = n & 4, b3 = n & 8;
  float A[16], B[8], C[4], D[2];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (2 * j < 4 * NTG) {
      const float x0 = ws_v0<NTG>(v, 2 * j), x1 = ws_v0<NTG>(v, 2 * j + 1);
      A[j] = (b0 ? x1 : x0) + dpp_mov<0xB1>(b0 ? x0 : x1);
    } else {
      A[j] = 0.0f;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    B[k] = (b1 ? A[2 * k + 1] : A[2 * k]) +
           dpp_mov<0x4E>(b1 ? A[2 * k] : A[2 * k + 1]);
#pragma unroll
  for (int l = 0; l < 4; ++l)
    C[l] = (b2 ? B[2 * l + 1] : B[2 * l]) +
           __shfl_xor(b2 ? B[2 * l] : B[2 * l + 1], 4);
#pragma unroll
  for (int m = 0; m < 2; ++m)
    D[m] = (b3 ? C[2 * m + 1] : C[2 * m]) +
           __shfl_xor(b3 ? C[2 * m] : C[2 * m + 1], 8);
  float *orow = a.out + (int64_t)d * a.ldo + 16 * t0;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int i = 16 * m + n;  // register index this lane finishes
    if (i < 4 * NTG) {
      const int c = 16 * (i >> 2) + 4 * g + (i & 3);  // column inside the group
      if (whole)
        orow[c] = D[m];
      else
        atomicAdd(orow + c, D[m]);
    }
  }
}

// ws_epilogue for the sum: the same walk over the tile's runs, the rows
// finished (bias, ReLU) before they are added.
template <int NTG, class ARGS>
__device__ __forceinline__ void ws_epilogue_sum(
    const ARGS &a, const float *bias_lds, int t0, int lane,
    const v4f (&acc)[NTG], v4f (&carry)[NTG], unsigned starts, int my_d,
    WsRun &st, bool fin, int d_after, float inf) {
  const int n = lane & 15, g = lane >> 4;
  // the tile's rows: lane (g, n) holds features 16 (t0 + t) + 4 g .. + 3 of row n
  v4f y[NTG];
#pragma unroll
  for (int t = 0; t < NTG; ++t) {
    const v4f bb = *reinterpret_cast<const v4f *>(bias_lds + 16 * t + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = acc[t][r] + bb[r];
      if (16 * (t0 + t) + 4 * g + r >= a.relu_from) x = x > 0.0f ? x : 0.0f;
      y[t][r] = x;
    }
  }
  int cur_d = st.cur_d;
  bool cur_left_closed = st.left_closed, cur_has = st.has;
  int pos = 0;
  if (!(starts & 1u)) {
    // rows [0, f) continue the open run
    const int f = starts ? __builtin_ctz(starts) : 16;
    if (f == 16) {
#pragma unroll
      for (int t = 0; t < NTG; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[t][r] += y[t][r];
    } else {
      const bool in_run = n < f;
#pragma unroll
      for (int t = 0; t < NTG; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[t][r] += in_run ? y[t][r] : 0.0f;
    }
    cur_has = true;
    pos = f;
  }
  while (pos < 16) {  // wave-uniform; `pos` opens a run
    if (cur_has)
      ws_flush_sum<NTG>(a, bias_lds, t0, lane, cur_d, carry,
                        a.sorted && cur_left_closed &&
                            (!fin || d_after != cur_d),
                        inf);
    if (fin) break;
    const unsigned rest = starts & ~((2u << pos) - 1u);
    const int nextpos = rest ? __builtin_ctz(rest) : 16;
    const bool in_run = n >= pos && n < nextpos;
#pragma unroll
    for (int t = 0; t < NTG; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) carry[t][r] = in_run ? y[t][r] : 0.0f;
    cur_d = __builtin_amdgcn_readlane(my_d, pos);
    cur_left_closed = true;
    cur_has = true;
    pos = nextpos;
  }
  st.cur_d = cur_d;
  st.left_closed = cur_left_closed;
  st.has = cur_has;
}

}  // namespace pgnn
