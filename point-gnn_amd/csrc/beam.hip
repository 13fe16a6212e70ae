// LiDAR beam decimation (scripts/point_cloud_downsample.py:19-53): the
// elevation cosine of every point of a scan is clustered into n_beams beams
// and every rate-th beam is kept.  The script's KMeans is unseeded; here the
// clustering is DEFINED (include/pointgnn_hip.h, "beam decimation"): integer
// cosines q = rint(cos * 2^30), farthest-first initial centres with the
// smallest sorted index winning ties, Lloyd passes on the sorted q with exact
// int64 prefix sums.  The result depends on the input bits only.
//
// Stages of pgnn_beam_centers, all on the caller's stream, no host read:
//   prep     cos and the order-preserving key q ^ 0x80000000 of every row;
//            invalid rows get the top key and sort behind the valid ones
//   sort     radix_sort_pairs on the 32-bit keys
//   sums     int64 sum of every tile of sorted q
//   scan     exclusive int64 prefix sums S[0..n] (tile offset + in-tile scan)
//   cluster  ONE wave, lane = cluster: farthest-first initialisation and every
//            Lloyd pass; each search goes through an LDS table of every
//            stride-th key first, then a few dependent global loads
// pgnn_beam_select: keep test per row against the <= 64 kept intervals (LDS),
// then count / scan / write, the ordered compaction of ingest.hip.
#include <math.h>

#include "pgnn_common.h"
#include "sort.h"

namespace pgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxBeams = 64;
constexpr int kScanItems = 8;
constexpr int kScanTile = kBlock * kScanItems;  // rows per block of the scan
constexpr int kTable = 4096;                    // LDS search table entries
constexpr uint32_t kInvalidKey = 0xFFFFFFFFu;
constexpr double kScale = 1073741824.0;  // 2^30

// :22-25, :29: float32 norm (no FMA: the library is built with
// -ffp-contract=off), correctly rounded square root, float64 quotient
__device__ __forceinline__ bool beam_cos(const float4 r, double *cos_out) {
  const float sum = (r.x * r.x + r.y * r.y) + r.z * r.z;
  const float norm = (float)sqrt((double)sum);
  *cos_out = (double)r.z / (double)norm;
  return isfinite(r.x) && isfinite(r.y) && isfinite(r.z) && norm != 0.0f;
}

__device__ __forceinline__ int32_t key_to_q(uint32_t key) {
  return (int32_t)(key ^ 0x80000000u);
}

// ---- prep ---------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void beam_prep_kernel(
    const float4 *__restrict__ velo, int64_t n, uint32_t *__restrict__ keys,
    uint32_t *__restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double c;
  uint32_t key = kInvalidKey;
  if (beam_cos(velo[i], &c)) {
    // |cos| <= sqrt(1.5) (a squared component may round up by half a
    // denormal unit), so q fits an int32 and never reaches the top key
    const int32_t q = (int32_t)rint(c * kScale);
    key = (uint32_t)q ^ 0x80000000u;
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

// ---- int64 prefix sums of the sorted q ------------------------------------------
__device__ __forceinline__ int64_t q_or_zero(uint32_t key) {
  return key == kInvalidKey ? 0 : (int64_t)key_to_q(key);
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// block sum, valid in every thread
__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t *lds) {
  v = wave_sum_i64(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t t = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t += lds[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(kBlock) void beam_tile_sums_kernel(
    const uint32_t *__restrict__ keys, int64_t n,
    int64_t *__restrict__ tile_sums) {
  __shared__ int64_t lds[kWaves];
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  int64_t v = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t i = base + k * kBlock + threadIdx.x;
    if (i < n) v += q_or_zero(keys[i]);
  }
  v = block_sum_i64(v, lds);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = v;
}

// S[i] = sum of q over sorted rows < i, i in [0, n]
__global__ __launch_bounds__(kBlock) void beam_scan_kernel(
    const uint32_t *__restrict__ keys, int64_t n,
    const int64_t *__restrict__ tile_sums, int64_t *__restrict__ S) {
  __shared__ int64_t lds[kWaves];
  if (n == 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) S[0] = 0;
    return;
  }
  int64_t off = 0;
  for (int64_t b = threadIdx.x; b < (int64_t)blockIdx.x; b += kBlock)
    off += tile_sums[b];
  off = block_sum_i64(off, lds);
  // thread t owns rows base + t*8 .. + 7
  const int64_t first = (int64_t)blockIdx.x * kScanTile +
                        (int64_t)threadIdx.x * kScanItems;
  int64_t item[kScanItems];
  int64_t mine = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    item[k] = first + k < n ? q_or_zero(keys[first + k]) : 0;
    mine += item[k];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  int64_t run = off + inc - mine;
  for (int w = 0; w < wave; ++w) run += lds[w];
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (first + k < n) S[first + k] = run;
    run += item[k];
    if (first + k == n - 1) S[n] = run;
  }
}

// ---- cluster ------------------------------------------------------------------
// first i in [0, v) whose q fails `pred` (true for a prefix of the sorted q,
// false after it); v if none.  tab[t] = q of sorted row t * stride.
template <typename Pred>
__device__ __forceinline__ int first_false(const int32_t *tab, int ntab,
                                           int stride,
                                           const uint32_t *__restrict__ keys,
                                           int v, Pred pred) {
  int lo = 0, hi = ntab;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pred(tab[mid])) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return 0;
  // row (lo-1)*stride passes; row lo*stride fails when it exists
  int a = (lo - 1) * stride + 1;
  const int64_t top = (int64_t)lo * stride;
  int b = top < (int64_t)v ? (int)top : v;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (pred(key_to_q(keys[mid]))) a = mid + 1; else b = mid;
  }
  return a;
}

__device__ __forceinline__ int64_t wave_max_i64(int64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(v, d);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(kBlock) void beam_cluster_kernel(
    const uint32_t *__restrict__ keys, const int64_t *__restrict__ S,
    int64_t n, int B, int max_iter, double *__restrict__ centers,
    int32_t *__restrict__ info) {
  __shared__ int32_t tab[kTable];
  // valid rows sort in front of the invalid ones: v = first row with the top key
  int v;
  {
    int64_t a = 0, b = n;
    while (a < b) {
      const int64_t mid = (a + b) >> 1;
      if (keys[mid] != kInvalidKey) a = mid + 1; else b = mid;
    }
    v = (int)a;
  }
  const int stride = v > kTable ? (v + kTable - 1) / kTable : 1;
  const int ntab = (v + stride - 1) / stride;  // <= kTable
  for (int t = threadIdx.x; t < ntab; t += kBlock)
    tab[t] = key_to_q(keys[(int64_t)t * stride]);
  __syncthreads();
  if (threadIdx.x >= 64) return;  // one wave from here on, no more barriers
  const int lane = threadIdx.x;

  int status = 0, iterations = 0;
  double cd = 0.0;
  if (v < B) {
    status = 1;
  } else {
    // farthest-first.  Lanes 0..k-1 hold the chosen centres in ascending
    // order.  The points between two adjacent centres are farthest from both
    // next to their midpoint; above the largest centre it is the last point
    // (the smallest centre is s_0: nothing lies below).  Lane j < k-1 takes the
    // gap above centre j, lane k-1 the top end.
    int32_t c = tab[0];
    const int32_t s_last = key_to_q(keys[v - 1]);
    // the top end's candidate row never changes: found once, not in a branch
    // of its own beside the gap searches every round
    const int i_last = first_false(tab, ntab, stride, keys, v,
                                   [=](int32_t s) { return s < s_last; });
    for (int k = 1; k < B; ++k) {
      const int32_t cn = __shfl_down(c, 1);
      int64_t best_d = -1;
      int best_i = 0x7FFFFFFF;
      int32_t best_q = 0;
      if (lane < k - 1) {
        const int64_t sum = (int64_t)c + (int64_t)cn;
        const int ub = first_false(tab, ntab, stride, keys, v, [=](int32_t s) {
          return 2 * (int64_t)s <= sum;
        });  // >= 1: centre j itself passes; < v: centre j+1 fails
        // three independent loads: the rows either side of the midpoint and
        // the one below, which tells whether x has an earlier equal
        const int32_t x = key_to_q(keys[ub - 1]);
        const int32_t y = key_to_q(keys[ub]);
        const int32_t below = key_to_q(keys[ub >= 2 ? ub - 2 : 0]);
        int il = ub - 1;
        if (ub >= 2 && below == x)
          il = first_false(tab, ntab, stride, keys, v,
                           [=](int32_t s) { return s < x; });
        const int64_t dl = (int64_t)x - c, dr = (int64_t)cn - y;
        if (dr > dl) best_d = dr, best_i = ub, best_q = y;
        else best_d = dl, best_i = il, best_q = x;
      } else if (lane == k - 1) {
        best_d = (int64_t)s_last - c;
        best_q = s_last;
        best_i = i_last;
      }
      const int64_t max_d = wave_max_i64(best_d);
      if (max_d == 0) {  // fewer than B distinct q
        status = 2;
        break;
      }
      const int win_i = wave_min_i32(best_d == max_d ? best_i : 0x7FFFFFFF);
      const unsigned long long win =
          __ballot(best_d == max_d && best_i == win_i);
      const int32_t x = __shfl(best_q, __builtin_ctzll(win));
      const int p = __popcll(__ballot(lane < k && c < x));
      const int32_t up = __shfl_up(c, 1);
      c = lane > p ? up : (lane == p ? x : c);
    }
    if (status == 0) {
      cd = (double)c;
      int prev_hi = -1;
      status = 3;
      for (int it = 1; it <= max_iter; ++it) {
        const double cn = __shfl_down(cd, 1);
        int hi = v;
        if (lane < B - 1) {
          const double m = cd + cn;
          hi = first_false(tab, ntab, stride, keys, v, [=](int32_t s) {
            return 2.0 * (double)s <= m;
          });
        }
        int lo = __shfl_up(hi, 1);
        if (lane == 0) lo = 0;
        const int cnt = hi - lo;
        if (lane < B && cnt > 0)
          cd = (double)(S[hi] - S[lo]) / (double)cnt;
        iterations = it;
        const bool same = lane >= B || hi == prev_hi;
        prev_hi = hi;
        if (__all(same)) {
          status = 0;
          break;
        }
      }
    }
  }
  const bool ok = status == 0 || status == 3;
  if (lane < B) centers[lane] = ok ? cd * (1.0 / kScale) : 0.0;
  if (lane < 4)
    info[lane] = lane == 0 ? v : lane == 1 ? (ok ? iterations : 0)
                                : lane == 2 ? status : 0;
}

// ---- select -------------------------------------------------------------------
// :27-35: ext = [-1, centres, +1]; beam i = 0, rate, 2 rate, ... < B keeps the
// rows with (ext[i] + ext[i+1]) / 2 < cos < (ext[i+1] + ext[i+2]) / 2
struct KeptBounds {
  double lower[kMaxBeams], upper[kMaxBeams];
  int count;
};

__device__ __forceinline__ void load_bounds(KeptBounds *kb,
                                            const double *__restrict__ centers,
                                            int B, int rate,
                                            const int32_t *__restrict__ info) {
  const int count = rate >= B ? 1 : (B + rate - 1) / rate;
  const int t = threadIdx.x;
  if (t < count) {
    const int i = t * rate;  // < B
    const double e0 = i == 0 ? -1.0 : centers[i - 1];
    const double e1 = centers[i];
    const double e2 = i + 1 == B ? 1.0 : centers[i + 1];
    kb->lower[t] = (e0 + e1) / 2.0;
    kb->upper[t] = (e1 + e2) / 2.0;
  }
  if (t == 0) {
    const int st = info ? info[2] : 0;
    kb->count = (st == 1 || st == 2) ? 0 : count;
  }
  __syncthreads();
}

__device__ __forceinline__ bool beam_keep(const KeptBounds &kb,
                                          const float4 *__restrict__ velo,
                                          int64_t i, int64_t n) {
  if (i >= n) return false;
  double c;
  if (!beam_cos(velo[i], &c)) return false;
  bool keep = false;
  for (int t = 0; t < kb.count; ++t)
    keep = keep || (c > kb.lower[t] && c < kb.upper[t]);
  return keep;
}

__global__ __launch_bounds__(kBlock) void beam_select_count_kernel(
    const float4 *__restrict__ velo, int64_t n,
    const double *__restrict__ centers, int B, int rate,
    const int32_t *__restrict__ info, int32_t *__restrict__ counts,
    int n_blocks) {
  __shared__ KeptBounds kb;
  __shared__ int wave_tot[kWaves];
  load_bounds(&kb, centers, B, rate, info);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const unsigned long long bal = __ballot(beam_keep(kb, velo, i, n));
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kWaves; ++w) t += wave_tot[w];
    counts[blockIdx.x] = t;
    // the in-place exclusive scan leaves the total in the entry past the end
    if (blockIdx.x == 0) counts[n_blocks] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void beam_select_write_kernel(
    const float4 *__restrict__ velo, int64_t n,
    const double *__restrict__ centers, int B, int rate,
    const int32_t *__restrict__ info, const int32_t *__restrict__ block_offset,
    int n_blocks, float4 *__restrict__ out, int32_t *__restrict__ out_count) {
  __shared__ KeptBounds kb;
  __shared__ int wave_tot[kWaves];
  load_bounds(&kb, centers, B, rate, info);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool keep = beam_keep(kb, velo, i, n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) wave_tot[wave] = __popcll(bal);
  __syncthreads();
  int64_t slot = block_offset[blockIdx.x];
  for (int w = 0; w < wave; ++w) slot += wave_tot[w];
  slot += __popcll(bal & ((1ull << lane) - 1ull));
  if (keep) out[slot] = velo[i];  // :50 all four floats, bit for bit; slot <= i
  if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = block_offset[n_blocks];
}

__global__ void beam_zero_count_kernel(int32_t *out_count) { *out_count = 0; }

// ---- workspace ------------------------------------------------------------------
struct BeamLayout {
  uint32_t *keys_a, *vals_a, *keys_b, *vals_b;
  void *sort_ws;
  size_t sort_bytes;
  int64_t *tile_sums, *S;
  int32_t *counts;
};

inline int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }
inline int64_t tiles_of(int64_t n) { return (n + kScanTile - 1) / kScanTile; }

bool carve_beam(Arena &ar, int64_t n, BeamLayout *L) {
  const size_t m = (size_t)(n > 0 ? n : 1);
  L->sort_bytes = radix_sort_scratch_bytes((int64_t)m);
  L->keys_a = ar.take<uint32_t>(m);
  L->vals_a = ar.take<uint32_t>(m);
  L->keys_b = ar.take<uint32_t>(m);
  L->vals_b = ar.take<uint32_t>(m);
  L->sort_ws = ar.take<char>(L->sort_bytes);
  L->tile_sums = ar.take<int64_t>((size_t)tiles_of((int64_t)m));
  L->S = ar.take<int64_t>(m + 1);
  L->counts = ar.take<int32_t>((size_t)blocks_of((int64_t)m) + 1);
  return L->counts != nullptr;
}

}  // namespace
}  // namespace pgnn

using namespace pgnn;

extern "C" size_t pgnn_beam_workspace_bytes(int64_t n_points) {
  if (n_points < 0) return 0;
  Arena ar(nullptr, 0);
  BeamLayout L;
  carve_beam(ar, n_points, &L);
  return align_up(ar.used, 256);
}

extern "C" int pgnn_beam_centers(const float *velo_points, int64_t n_points,
                                 int32_t n_beams, int32_t max_iter,
                                 void *workspace, size_t workspace_bytes,
                                 double *centers, int32_t *info,
                                 void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_beams >= 2 && n_beams <= kMaxBeams, PGNN_E_INVALID,
               "beam_centers: n_beams must be 2..64");
  PGNN_REQUIRE(max_iter >= 1, PGNN_E_INVALID,
               "beam_centers: max_iter must be positive");
  PGNN_REQUIRE(n_points >= 0 && n_points < (int64_t)1 << 31, PGNN_E_INVALID,
               "beam_centers: bad size");
  PGNN_REQUIRE((velo_points || n_points == 0) && centers && info,
               PGNN_E_INVALID, "beam_centers: null pointer");
  Arena ar(workspace, workspace_bytes);
  BeamLayout L;
  PGNN_REQUIRE(carve_beam(ar, n_points, &L), PGNN_E_WORKSPACE,
               "beam_centers: workspace too small "
               "(see pgnn_beam_workspace_bytes)");
  uint32_t *keys = L.keys_a, *vals = L.vals_a;
  if (n_points > 0) {
    hipLaunchKernelGGL(beam_prep_kernel, dim3((unsigned)blocks_of(n_points)),
                       dim3(kBlock), 0, stream,
                       reinterpret_cast<const float4 *>(velo_points), n_points,
                       L.keys_a, L.vals_a);
    PGNN_HIP(hipGetLastError());
    int rc = radix_sort_pairs(L.keys_a, L.vals_a, L.keys_b, L.vals_b, n_points,
                              32, L.sort_ws, L.sort_bytes, &keys, &vals, stream);
    if (rc != 0) return rc;
    const unsigned tiles = (unsigned)tiles_of(n_points);
    hipLaunchKernelGGL(beam_tile_sums_kernel, dim3(tiles), dim3(kBlock), 0,
                       stream, keys, n_points, L.tile_sums);
    PGNN_HIP(hipGetLastError());
    hipLaunchKernelGGL(beam_scan_kernel, dim3(tiles), dim3(kBlock), 0, stream,
                       keys, n_points, L.tile_sums, L.S);
    PGNN_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(beam_cluster_kernel, dim3(1), dim3(kBlock), 0, stream,
                     keys, L.S, n_points, n_beams, max_iter, centers, info);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_beam_select(const float *velo_points, int64_t n_points,
                                const double *centers, int32_t n_beams,
                                int32_t rate, const int32_t *info,
                                void *workspace, size_t workspace_bytes,
                                float *out_points, int32_t *out_count,
                                void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_beams >= 2 && n_beams <= kMaxBeams, PGNN_E_INVALID,
               "beam_select: n_beams must be 2..64");
  PGNN_REQUIRE(rate >= 1, PGNN_E_INVALID, "beam_select: rate must be >= 1");
  PGNN_REQUIRE(n_points >= 0 && n_points < (int64_t)1 << 31, PGNN_E_INVALID,
               "beam_select: bad size");
  PGNN_REQUIRE(centers && out_count &&
                   (n_points == 0 || (velo_points && out_points)),
               PGNN_E_INVALID, "beam_select: null pointer");
  if (n_points == 0) {
    hipLaunchKernelGGL(beam_zero_count_kernel, dim3(1), dim3(1), 0, stream,
                       out_count);
    PGNN_HIP(hipGetLastError());
    return 0;
  }
  Arena ar(workspace, workspace_bytes);
  BeamLayout L;
  PGNN_REQUIRE(carve_beam(ar, n_points, &L), PGNN_E_WORKSPACE,
               "beam_select: workspace too small "
               "(see pgnn_beam_workspace_bytes)");
  const float4 *velo = reinterpret_cast<const float4 *>(velo_points);
  const int nb = (int)blocks_of(n_points);
  hipLaunchKernelGGL(beam_select_count_kernel, dim3((unsigned)nb), dim3(kBlock),
                     0, stream, velo, n_points, centers, n_beams, rate, info,
                     L.counts, nb);
  PGNN_HIP(hipGetLastError());
  int rc = exclusive_scan_inplace_i32(L.counts, (int64_t)nb + 1, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(beam_select_write_kernel, dim3((unsigned)nb), dim3(kBlock),
                     0, stream, velo, n_points, centers, n_beams, rate, info,
                     L.counts, nb, reinterpret_cast<float4 *>(out_points),
                     out_count);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}
