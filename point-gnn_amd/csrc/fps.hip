// Farthest-point sampling (dataset/kitti_dataset.py:630-641: farthest_first
// and calc_distances).  Contract: include/pointgnn_hip.h, "farthest-point
// sampling".  The k rounds are strictly sequential, so ONE workgroup owns a
// segment for all of them and nothing waits on another workgroup.
//
// A round, with the previous pick's coordinates c in every thread:
//   lane   d_j = min(d_j, dist(c, j)) over the thread's points, and the
//          thread's best (largest d, then smallest index: its points are
//          visited in ascending index and only a strictly larger d replaces)
//   wave   6 xor-shuffle steps on the key (d bits, index); the winning lane's
//          coordinates are read out of its registers and lane 0 writes
//          {key, index, x, y, z} to the wave's LDS slot
//   block  ONE barrier; every thread then reads the kWaves slots and takes
//          the best: its coordinates are the next c.  The slots are double
//          buffered: a wave that writes round r + 2's slot has passed round
//          r + 1's barrier, which every wave reaches only after reading
//          round r's.
// d stays a double in the per-point loop (v_min_f64 / v_max_f64, one
// instruction each); the thread's best crosses lanes and waves as its bit
// pattern, which orders as the value (key_of).  The k rounds are a counted
// loop, so NaN / inf rows, which are outside the contract, cannot stop it from
// ending, and a pick is always some thread's own point.
//
// Tiers: a segment of at most P * kBlock points keeps x, y, z (input dtype)
// and d on chip -- in registers, float32's d of the last strides in LDS
// (kLdsStridesF32) -- point i in thread i % kBlock (coalesced first load); the
// unrolled per-point loop leaves at a workgroup-uniform bound, so a small
// segment does not pay for the whole register tile.  A larger segment streams
// its coordinates from L2 / HBM every round and keeps d in the workspace
// (thread t reads and writes only the entries t, t + kBlock, ...).
#include "pgnn_common.h"

namespace pgnn {
namespace {

constexpr int kBlock = PGNN_FPS_BLOCK;
constexpr int kWaves = kBlock / 64;
constexpr int kPointsF32 = PGNN_FPS_RESIDENT / PGNN_FPS_BLOCK;
constexpr int kPointsF64 = PGNN_FPS_RESIDENT_F64 / PGNN_FPS_BLOCK;
// float32: 40 strides of x, y, z and d are 200 registers of the 256 a wave
// has at two waves per SIMD, and the compiler spills; the d of the last
// strides lives in LDS instead (8 B per point, each thread its own column)
constexpr int kLdsStridesF32 = 14;
static_assert(kBlock % 64 == 0 && kPointsF32 * kBlock == PGNN_FPS_RESIDENT &&
                  kPointsF64 * kBlock == PGNN_FPS_RESIDENT_F64,
              "resident limits are whole strides of the workgroup");

template <typename T>
struct Slot {
  uint64_t key;
  int32_t idx, pad;
  T x, y, z;
};

// :631 on one row: float64, one rounding per operation (-ffp-contract=off)
__device__ __forceinline__ double dist(double cx, double cy, double cz,
                                       double x, double y, double z) {
  const double dx = cx - x, dy = cy - y, dz = cz - z;
  return (dx * dx + dy * dy) + dz * dz;
}

// A thread's running best is a double that is never NaN and never negative
// (it starts at 0 and is only replaced by a strictly larger d), so its bit
// pattern orders as its value: the wave and block steps compare integers.
__device__ __forceinline__ uint64_t key_of(double best) {
  return (uint64_t)__double_as_longlong(best);
}

__device__ __forceinline__ bool better(uint64_t k, int32_t i, uint64_t than_k,
                                       int32_t than_i) {
  return k > than_k || (k == than_k && i < than_i);
}

// The wave's best key in every lane, and the lane that holds it.
__device__ __forceinline__ int wave_best(uint64_t *key, int32_t *idx) {
  const uint64_t k0 = *key;
  const int32_t i0 = *idx;
  uint64_t k = k0;
  int32_t i = i0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint64_t ok = __shfl_xor((unsigned long long)k, m);
    const int32_t oi = __shfl_xor(i, m);
    const bool take = better(ok, oi, k, i);
    k = take ? ok : k;
    i = take ? oi : i;
  }
  *key = k;
  *idx = i;
  // (k, i) is some lane's own pair, so the ballot is never empty
  return __builtin_ctzll(__ballot(k0 == k && i0 == i));
}

// Lane 0 of every wave publishes the wave's best; after the round's one
// barrier every thread takes the block's best.  Returns its key.
template <typename T>
__device__ __forceinline__ uint64_t block_best(Slot<T> *slots, uint64_t wk,
                                               int32_t wi, T sx, T sy, T sz,
                                               int32_t *gi, T *cx, T *cy,
                                               T *cz) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    Slot<T> &s = slots[wave];
    s.key = wk;
    s.idx = wi;
    s.x = sx;
    s.y = sy;
    s.z = sz;
  }
  __syncthreads();
  uint64_t gk = slots[0].key;
  int32_t bi = slots[0].idx;
  int gw = 0;
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const uint64_t k = slots[w].key;
    const int32_t i = slots[w].idx;
    const bool take = better(k, i, gk, bi);
    gk = take ? k : gk;
    bi = take ? i : bi;
    gw = take ? w : gw;
  }
  *gi = bi;
  *cx = slots[gw].x;
  *cy = slots[gw].y;
  *cz = slots[gw].z;
  return gk;
}

template <typename T>
__device__ __forceinline__ void write_pick(int32_t *out_idx, T *out_xyz, int i,
                                           int32_t idx, T x, T y, T z) {
  out_idx[i] = idx;
  if (out_xyz) {
    out_xyz[3 * (size_t)i + 0] = x;
    out_xyz[3 * (size_t)i + 1] = y;
    out_xyz[3 * (size_t)i + 2] = z;
  }
}

// Rounds 1 .. k-1 with d and the coordinates in registers.  Returns the round
// that found max(d) == 0, or k.
template <typename T, int P, int PL>
__device__ __forceinline__ int rounds_resident(const T *__restrict__ pts,
                                               int n, int k, T cx, T cy, T cz,
                                               Slot<T> *slots,
                                               double *d_lds,
                                               int32_t *out_idx, T *out_xyz) {
  const int tid = threadIdx.x;
  const int npt = (n + kBlock - 1) / kBlock;  // <= P, workgroup-uniform
  constexpr int PR = P - PL;  // strides whose d is a register pair
  T x[P], y[P], z[P];
  double d[PR];
  double *const dl = d_lds + tid;  // this thread's column: no sharing
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = tid + j * kBlock;
    const bool in = i < n;
    x[j] = in ? pts[3 * (size_t)i + 0] : T(0);
    y[j] = in ? pts[3 * (size_t)i + 1] : T(0);
    z[j] = in ? pts[3 * (size_t)i + 2] : T(0);
    // +inf: the first round's min is the distance itself.  A row past the
    // segment keeps d == 0 and can never be a strict maximum.
    const double d0 = in ? __builtin_inf() : 0.0;
    if (j < PR) d[j < PR ? j : 0] = d0; else dl[(j - PR) * kBlock] = d0;
  }
  int buf = 0;
  for (int r = 1; r < k; ++r) {
    const double ax = (double)cx, ay = (double)cy, az = (double)cz;
    double bd = 0.0;
    int bj = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (j < npt) {
        const double nd =
            dist(ax, ay, az, (double)x[j], (double)y[j], (double)z[j]);
        const double old = j < PR ? d[j < PR ? j : 0] : dl[(j - PR) * kBlock];
        const double dj = fmin(old, nd);
        if (j < PR) d[j < PR ? j : 0] = dj; else dl[(j - PR) * kBlock] = dj;
        bj = dj > bd ? j : bj;
        bd = fmax(bd, dj);
      }
    }
    const int32_t bi = tid + bj * kBlock;
    uint64_t wk = key_of(bd);
    int32_t wi = bi;
    const int wl = wave_best(&wk, &wi);
    // the winner's register slot is wave-uniform: scalar branches, no selects
    const int wj = __builtin_amdgcn_readlane(bj, wl);
    T sx = T(0), sy = T(0), sz = T(0);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (j == wj) {
        sx = x[j];
        sy = y[j];
        sz = z[j];
      }
    }
    sx = __shfl(sx, wl);
    sy = __shfl(sy, wl);
    sz = __shfl(sz, wl);
    int32_t gi;
    const uint64_t gk = block_best(slots + buf * kWaves, wk, wi, sx, sy, sz,
                                   &gi, &cx, &cy, &cz);
    buf ^= 1;
    if (gk == 0) return r;
    if (tid == 0) write_pick(out_idx, out_xyz, r, gi, cx, cy, cz);
  }
  return k;
}

// The same rounds for a segment too large for the registers: coordinates are
// read again every round, d lives in the workspace, and the thread's best
// carries its coordinates along.
template <typename T>
__device__ __forceinline__ int rounds_streaming(const T *__restrict__ pts,
                                                int n, int k, T cx, T cy, T cz,
                                                double *__restrict__ d,
                                                Slot<T> *slots,
                                                int32_t *out_idx, T *out_xyz) {
  const int tid = threadIdx.x;
  int buf = 0;
  for (int r = 1; r < k; ++r) {
    const double ax = (double)cx, ay = (double)cy, az = (double)cz;
    const bool first = r == 1;
    double bd = 0.0;
    int32_t bi = 0x7FFFFFFF;
    T bx = T(0), by = T(0), bz = T(0);
#pragma unroll 4
    for (int64_t j = tid; j < n; j += kBlock) {  // (n may be near 2^31)
      const T px = pts[3 * (size_t)j + 0];
      const T py = pts[3 * (size_t)j + 1];
      const T pz = pts[3 * (size_t)j + 2];
      const double nd =
          dist(ax, ay, az, (double)px, (double)py, (double)pz);
      const double dj = first ? nd : fmin(d[j], nd);
      d[j] = dj;
      if (dj > bd) {
        bd = dj;
        bi = (int32_t)j;
        bx = px;
        by = py;
        bz = pz;
      }
    }
    uint64_t wk = key_of(bd);
    int32_t wi = bi;
    const int wl = wave_best(&wk, &wi);
    const T sx = __shfl(bx, wl), sy = __shfl(by, wl), sz = __shfl(bz, wl);
    int32_t gi;
    const uint64_t gk = block_best(slots + buf * kWaves, wk, wi, sx, sy, sz,
                                   &gi, &cx, &cy, &cz);
    buf ^= 1;
    if (gk == 0) return r;
    if (tid == 0) write_pick(out_idx, out_xyz, r, gi, cx, cy, cz);
  }
  return k;
}

template <typename T, int P, int PL>
__global__ __launch_bounds__(kBlock) void fps_kernel(
    const T *__restrict__ points, const int32_t *__restrict__ offsets,
    int n_points, const int32_t *__restrict__ start, int k,
    double *__restrict__ dist_ws, int32_t *__restrict__ out_idx,
    T *__restrict__ out_xyz, int32_t *__restrict__ num_distinct) {
  __shared__ Slot<T> slots[2 * kWaves];
  __shared__ double d_lds[PL > 0 ? PL * kBlock : 1];
  const int seg = blockIdx.x, tid = threadIdx.x;
  int lo = 0, hi = n_points;
  if (offsets) {
    lo = offsets[seg];
    hi = offsets[seg + 1];
  }
  // whatever the offsets hold, [lo, hi) lies inside the cloud
  lo = lo < 0 ? 0 : (lo > n_points ? n_points : lo);
  hi = hi < lo ? lo : (hi > n_points ? n_points : hi);
  const int n = hi - lo;
  out_idx += (size_t)seg * k;
  if (out_xyz) out_xyz += 3 * (size_t)seg * k;
  if (n == 0 || k == 0) {
    // an empty segment is marked; the empty single cloud writes nothing
    for (int i = tid; i < k && offsets; i += kBlock)
      write_pick(out_idx, out_xyz, i, -1, T(0), T(0), T(0));
    if (tid == 0) num_distinct[seg] = 0;
    return;
  }
  const T *pts = points + 3 * (size_t)lo;
  int s = start[seg];
  s = s < 0 ? 0 : (s >= n ? n - 1 : s);
  const T cx = pts[3 * (size_t)s + 0];
  const T cy = pts[3 * (size_t)s + 1];
  const T cz = pts[3 * (size_t)s + 2];
  if (tid == 0) write_pick(out_idx, out_xyz, 0, s, cx, cy, cz);
  const int nd = n <= P * kBlock
                     ? rounds_resident<T, P, PL>(pts, n, k, cx, cy, cz, slots,
                                                 d_lds, out_idx, out_xyz)
                     : rounds_streaming<T>(pts, n, k, cx, cy, cz, dist_ws + lo,
                                           slots, out_idx, out_xyz);
  // max(d) == 0 in round nd: np.argmax of an all-zero array is 0 from here on
  if (nd < k) {
    const T x0 = pts[0], y0 = pts[1], z0 = pts[2];
    for (int i = nd + tid; i < k; i += kBlock)
      write_pick(out_idx, out_xyz, i, 0, x0, y0, z0);
  }
  if (tid == 0) num_distinct[seg] = nd;
}

template <typename T, int P, int PL>
int farthest_first(const T *points, const int32_t *offsets, int64_t n_segments,
                   int64_t n_points, const int32_t *start, int32_t k,
                   void *workspace, size_t workspace_bytes, int32_t *out_idx,
                   T *out_xyz, int32_t *num_distinct, hipStream_t stream) {
  PGNN_REQUIRE(n_segments >= 0 && n_segments < (int64_t)1 << 31 &&
                   n_points >= 0 && n_points < (int64_t)1 << 31 && k >= 0,
               PGNN_E_INVALID, "farthest_first: bad size");
  PGNN_REQUIRE(offsets || n_segments == 1, PGNN_E_INVALID,
               "farthest_first: offsets == NULL needs n_segments == 1");
  if (n_segments == 0) return 0;
  PGNN_REQUIRE(num_distinct && (points || n_points == 0) &&
                   (out_idx || k == 0) &&
                   (start || n_points == 0 || k == 0),
               PGNN_E_INVALID, "farthest_first: null pointer");
  double *dist_ws = nullptr;
  if (n_points > (int64_t)P * kBlock) {
    Arena ar(workspace, workspace_bytes);
    dist_ws = ar.take<double>((size_t)n_points);
    PGNN_REQUIRE(dist_ws, PGNN_E_WORKSPACE,
                 "farthest_first: workspace too small "
                 "(see pgnn_farthest_first_workspace_bytes)");
  }
  hipLaunchKernelGGL((fps_kernel<T, P, PL>), dim3((unsigned)n_segments),
                     dim3(kBlock), 0, stream, points, offsets, (int)n_points,
                     start, (int)k, dist_ws, out_idx, out_xyz, num_distinct);
  PGNN_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace pgnn

using namespace pgnn;

extern "C" size_t pgnn_farthest_first_workspace_bytes(int64_t n_points,
                                                      int64_t n_segments,
                                                      int32_t k) {
  (void)n_segments;
  (void)k;
  // the running distances of the streaming tier; the smaller (float64)
  // resident limit serves both entries
  if (n_points <= PGNN_FPS_RESIDENT_F64) return 0;
  Arena ar(nullptr, 0);
  ar.take<double>((size_t)n_points);
  return align_up(ar.used, 256);
}

extern "C" int pgnn_farthest_first(const float *points, const int32_t *offsets,
                                   int64_t n_segments, int64_t n_points,
                                   const int32_t *start, int32_t k,
                                   void *workspace, size_t workspace_bytes,
                                   int32_t *out_idx, float *out_xyz,
                                   int32_t *num_distinct, void *stream) {
  PGNN_GUARD_BEGIN
  return farthest_first<float, kPointsF32, kLdsStridesF32>(
      points, offsets, n_segments, n_points, start, k, workspace,
      workspace_bytes, out_idx, out_xyz, num_distinct, (hipStream_t)stream);
  PGNN_GUARD_END
}

extern "C" int pgnn_farthest_first_f64(const double *points,
                                       const int32_t *offsets,
                                       int64_t n_segments, int64_t n_points,
                                       const int32_t *start, int32_t k,
                                       void *workspace, size_t workspace_bytes,
                                       int32_t *out_idx, double *out_xyz,
                                       int32_t *num_distinct, void *stream) {
  PGNN_GUARD_BEGIN
  return farthest_first<double, kPointsF64, 0>(
      points, offsets, n_segments, n_points, start, k, workspace,
      workspace_bytes, out_idx, out_xyz, num_distinct, (hipStream_t)stream);
  PGNN_GUARD_END
}
