// Voxel-average down-sampling of a frame (dataset/kitti_dataset.py:16-48
// downsample_by_average_voxel) and the frame fetch that contains it (:612-628
// get_cam_points, :666-716 get_cam_points_in_image[_with_rgb]).
//
// ~120 k points, a few MB: L2-resident and launch-latency-bound.  Stages, all
// on the caller's stream, no host read:
//   pack     xyz|attr[0] (or the velodyne row through velo_to_cam) -> one 16-B
//            record per point + per-workgroup min/max of the coordinates
//   keys     int32 voxel key of every point (wrapping, like NumPy's int32)
//   sort     stable LSD radix sort of (key ^ 0x80000000, index): signed order,
//            equal keys stay in ascending original index
//   heads    voxels that start in each 256-row block, then an in-place scan
//   segment  every wave folds the voxels that START in its 64 sorted rows, in
//            sorted order, in float32; a voxel that runs past the wave's rows
//            is followed 64 rows at a time (coalesced), so one voxel may hold
//            every point; the mean is float64(sum) / float64(count)
// The fold order is DEFINED (ascending original index); NumPy's unstable
// argsort leaves it to the sort implementation for voxels of 3+ points.
#include <math.h>

#include "ingest_common.h"
#include "npy_divmod.h"
#include "sort.h"

namespace pgnn {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxParts = 256;  // workgroups of the pack stage (<= kBlock)
constexpr int kMaxAttr = 4;

__device__ __forceinline__ int64_t device_count(int64_t n,
                                                const int32_t *n_dev) {
  if (!n_dev) return n;
  const int64_t d = *n_dev;
  return d < 0 ? 0 : (d < n ? d : n);
}

// ---- pack + min/max ---------------------------------------------------------
struct PackSrc {
  const float *xyz;   // [n,3]            (plain form)
  const float *attr;  // [n,attr_dim]     (plain form, nullable)
  int attr_dim;
};

template <bool kVelo>
__global__ __launch_bounds__(kBlock) void voxel_pack_kernel(
    IngestArgs a, PackSrc src, int64_t n, const int32_t *__restrict__ n_dev,
    float4 *__restrict__ rec, float *__restrict__ parts /* [grid][6] */) {
  n = device_count(n, n_dev);
  float lo[3] = {INFINITY, INFINITY, INFINITY};
  float hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    float4 r;
    if (kVelo) {
      const float4 q = reinterpret_cast<const float4 *>(a.velo)[i];
      velo_to_cam_f32(a, q, &r.x, &r.y, &r.z);
      r.w = q.w;
    } else {
      r.x = src.xyz[3 * i];
      r.y = src.xyz[3 * i + 1];
      r.z = src.xyz[3 * i + 2];
      r.w = src.attr_dim > 0 ? src.attr[i * src.attr_dim] : 0.0f;
    }
    rec[i] = r;
    lo[0] = fminf(lo[0], r.x), hi[0] = fmaxf(hi[0], r.x);
    lo[1] = fminf(lo[1], r.y), hi[1] = fmaxf(hi[1], r.y);
    lo[2] = fminf(lo[2], r.z), hi[2] = fmaxf(hi[2], r.z);
  }
  __shared__ float red[kWaves][6];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], d));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d));
    }
  }
  if ((threadIdx.x & 63) == 0) {
    for (int c = 0; c < 3; ++c) {
      red[threadIdx.x >> 6][c] = lo[c];
      red[threadIdx.x >> 6][3 + c] = hi[c];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[0][threadIdx.x];
    for (int w = 1; w < kWaves; ++w)
      v = threadIdx.x < 3 ? fminf(v, red[w][threadIdx.x])
                          : fmaxf(v, red[w][threadIdx.x]);
    parts[blockIdx.x * 6 + threadIdx.x] = v;
  }
}

// ---- keys -------------------------------------------------------------------
// kitti_dataset.py:24-31: idx = ((xyz - min) // voxel).astype(int32), all
// float32; dim = max(idx) + 1 (the subtraction and the floor division are
// monotone, so max(idx) is the index of the maximum); key = ix + iy * dim_x +
// iz * dim_y * dim_x in wrapping 32-bit integers.
__global__ __launch_bounds__(kBlock) void voxel_key_kernel(
    const float4 *__restrict__ rec, int64_t n,
    const int32_t *__restrict__ n_dev, const float *__restrict__ parts,
    int n_parts, float voxel, uint32_t *__restrict__ keys,
    uint32_t *__restrict__ vals) {
  n = device_count(n, n_dev);
  __shared__ float red[kWaves][6];
  float m[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const float ident = c < 3 ? INFINITY : -INFINITY;
    m[c] = (int)threadIdx.x < n_parts ? parts[threadIdx.x * 6 + c] : ident;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const float o = __shfl_xor(m[c], d);
      m[c] = c < 3 ? fminf(m[c], o) : fmaxf(m[c], o);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = m[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    m[c] = red[0][c];
    for (int w = 1; w < kWaves; ++w)
      m[c] = c < 3 ? fminf(m[c], red[w][c]) : fmaxf(m[c], red[w][c]);
  }
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t dim_x =
      (uint32_t)(int32_t)npy_floor_divide_f32(m[3] - m[0], voxel) + 1u;
  const uint32_t dim_y =
      (uint32_t)(int32_t)npy_floor_divide_f32(m[4] - m[1], voxel) + 1u;
  const float4 r = rec[i];
  const uint32_t ix = (uint32_t)(int32_t)npy_floor_divide_f32(r.x - m[0], voxel);
  const uint32_t iy = (uint32_t)(int32_t)npy_floor_divide_f32(r.y - m[1], voxel);
  const uint32_t iz = (uint32_t)(int32_t)npy_floor_divide_f32(r.z - m[2], voxel);
  const uint32_t key = ix + iy * dim_x + iz * dim_y * dim_x;
  keys[i] = key ^ 0x80000000u;  // unsigned order of this = signed order of key
  vals[i] = (uint32_t)i;
}

// ---- segment heads per block --------------------------------------------------
__device__ __forceinline__ bool is_head(const uint32_t *__restrict__ keys,
                                        int64_t i, int64_t n) {
  return i < n && (i == 0 || keys[i] != keys[i - 1]);
}

__global__ __launch_bounds__(kBlock) void voxel_head_count_kernel(
    const uint32_t *__restrict__ keys, int64_t n,
    const int32_t *__restrict__ n_dev, int32_t *__restrict__ counts,
    int n_blocks) {
  n = device_count(n, n_dev);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const unsigned long long bal = __ballot(is_head(keys, i, n));
  __shared__ int wave_tot[kWaves];
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

// ---- segment fold -------------------------------------------------------------
// kCols = 4: x y z attr[0] (the 16-B record); 7: + attr[1..3] from `attr`.
template <int kCols>
__global__ __launch_bounds__(kBlock) void voxel_segment_kernel(
    const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
    const float4 *__restrict__ rec, const float *__restrict__ attr,
    int attr_dim, int64_t n, const int32_t *__restrict__ n_dev,
    const int32_t *__restrict__ block_offset, int n_blocks,
    double *__restrict__ out_xyz, double *__restrict__ out_attr,
    int32_t *__restrict__ out_lens, int64_t capacity,
    int32_t *__restrict__ out_count) {
  n = device_count(n, n_dev);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kBlock + wave * 64;
  const int64_t i = i0 + lane;
  const bool valid = i < n;
  const uint32_t key = valid ? keys[i] : 0u;
  const bool head = is_head(keys, i, n);

  auto load_row = [&](int64_t row, float *v) {
    const uint32_t p = vals[row];
    const float4 r = rec[p];
    v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
#pragma unroll
    for (int c = 4; c < kCols; ++c)
      v[c] = c - 3 < attr_dim ? attr[(int64_t)p * attr_dim + (c - 3)] : 0.0f;
  };

  float v[kCols], acc[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) v[c] = 0.0f;
  if (valid) load_row(i, v);
#pragma unroll
  for (int c = 0; c < kCols; ++c) acc[c] = v[c];

  const unsigned long long heads = __ballot(head);
  const unsigned long long valids = __ballot(valid);
  __shared__ int wave_tot[kWaves];
  if (lane == 0) wave_tot[wave] = __popcll(heads);
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = block_offset[n_blocks];
  if (heads == 0ull) return;  // wave-uniform: no voxel starts in these rows

  // rows of this voxel inside the wave: up to the next head / the last row
  const int n_valid = __popcll(valids);  // valid lanes are 0 .. n_valid-1
  const unsigned long long later =
      lane < 63 ? heads >> (lane + 1) : 0ull;
  const int end = later ? lane + 1 + __builtin_ctzll(later) : n_valid;
  int len = head ? end - lane : 0;
  for (int s = 1; __any(s < len); ++s) {
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
      const float t = __shfl(v[c], (lane + s) & 63);
      if (s < len) acc[c] += t;
    }
  }

  // the last voxel that starts here may go on in the rows after the wave's
  const int last_head = 63 - __builtin_clzll(heads);
  if (n_valid == 64 && i0 + 64 < n) {
    const uint32_t seg_key = __shfl(key, 63);
    float carry[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) carry[c] = __shfl(acc[c], last_head);
    int extra = 0;
    for (int64_t j0 = i0 + 64; j0 < n; j0 += 64) {
      const int64_t j = j0 + lane;
      const bool same = j < n && keys[j] == seg_key;
      const unsigned long long diff = ~__ballot(same);
      const int run = diff ? __builtin_ctzll(diff) : 64;  // wave-uniform
      if (run == 0) break;
      float w[kCols];
#pragma unroll
      for (int c = 0; c < kCols; ++c) w[c] = 0.0f;
      if (lane < run) load_row(j, w);
      for (int s = 0; s < run; ++s) {
#pragma unroll
        for (int c = 0; c < kCols; ++c) carry[c] += __shfl(w[c], s);
      }
      extra += run;
      if (run < 64) break;
    }
    if (lane == last_head) {
#pragma unroll
      for (int c = 0; c < kCols; ++c) acc[c] = carry[c];
      len += extra;
    }
  }

  if (!head) return;
  int64_t row = block_offset[blockIdx.x];
  for (int w = 0; w < wave; ++w) row += wave_tot[w];
  row += __popcll(heads & ((1ull << lane) - 1ull));
  if (row >= capacity) return;
  // :37-38 float32 sums / int64 counts -> float64
  const double d = (double)len;
  out_xyz[3 * row] = (double)acc[0] / d;
  out_xyz[3 * row + 1] = (double)acc[1] / d;
  out_xyz[3 * row + 2] = (double)acc[2] / d;
#pragma unroll
  for (int c = 3; c < kCols; ++c)
    if (c - 3 < attr_dim) out_attr[row * attr_dim + (c - 3)] = (double)acc[c] / d;
  if (out_lens) out_lens[row] = len;
}

// ---- crop of the float64 rows -------------------------------------------------
struct Crop64 {
  double u, v;
  bool keep;
};

// :675 front points (float64 rows against the Python float 0.1), :678-684
__device__ __forceinline__ Crop64 crop_point(const IngestArgs &a,
                                             const double *__restrict__ xyz,
                                             int64_t i) {
  Crop64 o;
  const double X = xyz[3 * i], Y = xyz[3 * i + 1], Z = xyz[3 * i + 2];
  o.keep = project_in_image(a, X, Y, Z, &o.u, &o.v) && Z > 0.1;
  return o;
}

__global__ __launch_bounds__(kBlock) void voxel_crop_count_kernel(
    IngestArgs a, const double *__restrict__ xyz, int64_t n,
    const int32_t *__restrict__ n_dev, int32_t *__restrict__ counts,
    int n_blocks) {
  n = device_count(n, n_dev);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool keep = i < n && crop_point(a, xyz, i).keep;
  __shared__ int wave_tot[kWaves];
  const unsigned long long bal = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kWaves; ++w) t += wave_tot[w];
    counts[blockIdx.x] = t;
    if (blockIdx.x == 0) counts[n_blocks] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void voxel_crop_write_kernel(
    IngestArgs a, const double *__restrict__ xyz,
    const double *__restrict__ refl, int64_t n,
    const int32_t *__restrict__ n_dev, const int32_t *__restrict__ block_offset,
    int n_blocks, double *__restrict__ out_xyz, double *__restrict__ out_attr,
    int attr_dim, int64_t capacity, int32_t *__restrict__ out_count) {
  n = device_count(n, n_dev);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  Crop64 o;
  o.keep = false;
  if (i < n) o = crop_point(a, xyz, i);
  __shared__ int wave_tot[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(o.keep);
  if (lane == 0) wave_tot[wave] = __popcll(bal);
  __syncthreads();
  int64_t slot = block_offset[blockIdx.x];
  for (int w = 0; w < wave; ++w) slot += wave_tot[w];
  slot += __popcll(bal & ((1ull << lane) - 1ull));
  if (o.keep && slot < capacity) {
    out_xyz[3 * slot] = xyz[3 * i];
    out_xyz[3 * slot + 1] = xyz[3 * i + 1];
    out_xyz[3 * slot + 2] = xyz[3 * i + 2];
    double *at = out_attr + slot * attr_dim;
    at[0] = refl[i];
    if (attr_dim == 4) {
      // :996 np.hstack([attr float64, rgb float32]) is float64
      float r, g, b;
      sample_rgb(a, o.u, o.v, &r, &g, &b);
      at[1] = (double)r;
      at[2] = (double)g;
      at[3] = (double)b;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = block_offset[n_blocks];
}

// ---- workspace ------------------------------------------------------------------
struct VoxelLayout {
  float4 *rec;
  float *parts;
  uint32_t *keys_a, *vals_a, *keys_b, *vals_b;
  void *sort_ws;
  size_t sort_bytes;
  int32_t *counts;
};

inline int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

bool carve_voxel(Arena &ar, int64_t n, VoxelLayout *L) {
  const size_t m = (size_t)(n > 0 ? n : 1);
  L->sort_bytes = radix_sort_scratch_bytes((int64_t)m);
  L->rec = ar.take<float4>(m);
  L->parts = ar.take<float>((size_t)kMaxParts * 6);
  L->keys_a = ar.take<uint32_t>(m);
  L->vals_a = ar.take<uint32_t>(m);
  L->keys_b = ar.take<uint32_t>(m);
  L->vals_b = ar.take<uint32_t>(m);
  L->sort_ws = ar.take<char>(L->sort_bytes);
  L->counts = ar.take<int32_t>((size_t)blocks_of((int64_t)m) + 1);
  return L->counts != nullptr;
}

struct ChainLayout {
  VoxelLayout vox;
  double *mid_xyz, *mid_refl;
  int32_t *mid_count, *crop_counts;
};

bool carve_chain(Arena &ar, int64_t n, ChainLayout *L) {
  const size_t m = (size_t)(n > 0 ? n : 1);
  carve_voxel(ar, n, &L->vox);
  L->mid_xyz = ar.take<double>(3 * m);
  L->mid_refl = ar.take<double>(m);
  L->mid_count = ar.take<int32_t>(1);
  L->crop_counts = ar.take<int32_t>((size_t)blocks_of((int64_t)m) + 1);
  return L->crop_counts != nullptr;
}

bool voxel_size_ok(double voxel_size) {
  // the reference applies the Python float to a float32 array: the division
  // runs in float32, so the float32 value has to be a positive finite number
  return isfinite(voxel_size) && voxel_size > 0.0 &&
         isfinite((float)voxel_size) && (float)voxel_size > 0.0f;
}

// keys -> sort -> heads -> scan -> segment over the packed records
int voxel_average_stages(const VoxelLayout &L, const float *attr, int attr_dim,
                         int64_t n, const int32_t *n_dev, int n_parts,
                         float voxel, double *out_xyz, double *out_attr,
                         int32_t *out_lens, int64_t capacity,
                         int32_t *out_count, hipStream_t stream) {
  const int nb = (int)blocks_of(n);
  hipLaunchKernelGGL(voxel_key_kernel, dim3((unsigned)nb), dim3(kBlock), 0,
                     stream, L.rec, n, n_dev, L.parts, n_parts, voxel, L.keys_a,
                     L.vals_a);
  PGNN_HIP(hipGetLastError());
  uint32_t *keys = nullptr, *vals = nullptr;
  int rc = radix_sort_pairs(L.keys_a, L.vals_a, L.keys_b, L.vals_b, n, 32,
                            L.sort_ws, L.sort_bytes, &keys, &vals, stream,
                            n_dev);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(voxel_head_count_kernel, dim3((unsigned)nb), dim3(kBlock),
                     0, stream, keys, n, n_dev, L.counts, nb);
  PGNN_HIP(hipGetLastError());
  rc = exclusive_scan_inplace_i32(L.counts, (int64_t)nb + 1, stream);
  if (rc != 0) return rc;
  if (attr_dim > 1) {
    hipLaunchKernelGGL(voxel_segment_kernel<3 + kMaxAttr>, dim3((unsigned)nb),
                       dim3(kBlock), 0, stream, keys, vals, L.rec, attr,
                       attr_dim, n, n_dev, L.counts, nb, out_xyz, out_attr,
                       out_lens, capacity, out_count);
  } else {
    hipLaunchKernelGGL(voxel_segment_kernel<4>, dim3((unsigned)nb),
                       dim3(kBlock), 0, stream, keys, vals, L.rec, attr,
                       attr_dim, n, n_dev, L.counts, nb, out_xyz, out_attr,
                       out_lens, capacity, out_count);
  }
  PGNN_HIP(hipGetLastError());
  return 0;
}

inline int pack_grid(int64_t n) {
  const int64_t nb = blocks_of(n);
  return (int)(nb < kMaxParts ? nb : kMaxParts);
}

}  // namespace
}  // namespace pgnn

using namespace pgnn;

extern "C" size_t pgnn_voxel_average_workspace_bytes(int64_t n_points,
                                                     int32_t attr_dim) {
  if (n_points < 0 || attr_dim < 0 || attr_dim > kMaxAttr) return 0;
  Arena ar(nullptr, 0);
  VoxelLayout L;
  carve_voxel(ar, n_points, &L);
  return align_up(ar.used, 256);
}

extern "C" int pgnn_voxel_average_f32(
    const float *xyz, const float *attr, int32_t attr_dim, int64_t n_points,
    const int32_t *n_dev, double voxel_size, void *workspace,
    size_t workspace_bytes, double *out_xyz, double *out_attr,
    int32_t *out_lens, int64_t capacity, int32_t *out_count, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_points > 0, PGNN_E_INVALID,
               "voxel_average: n_points must be positive (the reference "
               "raises on an empty cloud)");
  PGNN_REQUIRE(attr_dim >= 0 && attr_dim <= kMaxAttr, PGNN_E_INVALID,
               "voxel_average: attr_dim must be 0..4");
  PGNN_REQUIRE(voxel_size_ok(voxel_size), PGNN_E_INVALID,
               "voxel_average: voxel_size must be a positive finite number");
  PGNN_REQUIRE(n_points < (int64_t)1 << 31 && capacity >= 0, PGNN_E_INVALID,
               "voxel_average: bad size");
  if (attr == nullptr) attr_dim = 0;
  PGNN_REQUIRE(xyz && out_count &&
                   (capacity == 0 || (out_xyz && (attr_dim == 0 || out_attr))),
               PGNN_E_INVALID, "voxel_average: null pointer");
  Arena ar(workspace, workspace_bytes);
  VoxelLayout L;
  PGNN_REQUIRE(carve_voxel(ar, n_points, &L), PGNN_E_WORKSPACE,
               "voxel_average: workspace too small "
               "(see pgnn_voxel_average_workspace_bytes)");
  IngestArgs a = {};
  PackSrc src = {xyz, attr, attr_dim};
  const int grid = pack_grid(n_points);
  hipLaunchKernelGGL(voxel_pack_kernel<false>, dim3((unsigned)grid),
                     dim3(kBlock), 0, stream, a, src, n_points, n_dev, L.rec,
                     L.parts);
  PGNN_HIP(hipGetLastError());
  return voxel_average_stages(L, attr, attr_dim, n_points, n_dev, grid,
                              (float)voxel_size, out_xyz, out_attr, out_lens,
                              capacity, out_count, stream);
  PGNN_GUARD_END
}

extern "C" size_t pgnn_kitti_cam_points_voxel_in_image_workspace_bytes(
    int64_t n_points) {
  if (n_points < 0) return 0;
  Arena ar(nullptr, 0);
  ChainLayout L;
  carve_chain(ar, n_points, &L);
  return align_up(ar.used, 256);
}

extern "C" int pgnn_kitti_cam_points_voxel_in_image(
    const float *velo_points, int64_t n_points, const float *velo_to_cam_3x4,
    const double *cam_to_image_3x3, double image_width, double image_height,
    const uint8_t *image_bgr, int64_t image_rows, int64_t image_cols,
    double voxel_size, void *workspace, size_t workspace_bytes,
    double *out_xyz, double *out_attr, int32_t attr_dim, int64_t capacity,
    int32_t *out_count, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_points > 0 && n_points < (int64_t)1 << 31 && capacity >= 0 &&
                   out_count && (attr_dim == 1 || attr_dim == 4),
               PGNN_E_INVALID, "kitti_cam_points_voxel_in_image: bad argument");
  PGNN_REQUIRE(voxel_size_ok(voxel_size), PGNN_E_INVALID,
               "kitti_cam_points_voxel_in_image: voxel_size must be a "
               "positive finite number");
  PGNN_REQUIRE(velo_to_cam_3x4 && cam_to_image_3x3, PGNN_E_INVALID,
               "kitti_cam_points_voxel_in_image: null calibration (host "
               "pointers)");
  PGNN_REQUIRE(velo_points && (capacity == 0 || (out_xyz && out_attr)),
               PGNN_E_INVALID, "kitti_cam_points_voxel_in_image: null pointer");
  PGNN_REQUIRE(attr_dim == 1 || image_bgr == nullptr ||
                   (image_rows > 0 && image_cols > 0),
               PGNN_E_INVALID,
               "kitti_cam_points_voxel_in_image: bad image shape");
  Arena ar(workspace, workspace_bytes);
  ChainLayout L;
  PGNN_REQUIRE(carve_chain(ar, n_points, &L), PGNN_E_WORKSPACE,
               "kitti_cam_points_voxel_in_image: workspace too small (see "
               "pgnn_kitti_cam_points_voxel_in_image_workspace_bytes)");
  IngestArgs a = {};
  a.velo = velo_points;
  a.n = n_points;
  fill_calib(&a, velo_to_cam_3x4, cam_to_image_3x3);
  a.width = image_width;
  a.height = image_height;
  a.image = attr_dim == 4 ? image_bgr : nullptr;
  a.img_h = image_rows;
  a.img_w = image_cols;
  PackSrc src = {nullptr, nullptr, 1};
  const int grid = pack_grid(n_points);
  hipLaunchKernelGGL(voxel_pack_kernel<true>, dim3((unsigned)grid),
                     dim3(kBlock), 0, stream, a, src, n_points,
                     (const int32_t *)nullptr, L.vox.rec, L.vox.parts);
  PGNN_HIP(hipGetLastError());
  // the record's fourth float is the reflectance: attr_dim 1, no extra columns
  int rc = voxel_average_stages(L.vox, nullptr, 1, n_points, nullptr, grid,
                                (float)voxel_size, L.mid_xyz, L.mid_refl,
                                nullptr, n_points, L.mid_count, stream);
  if (rc != 0) return rc;
  const int nb = (int)blocks_of(n_points);
  hipLaunchKernelGGL(voxel_crop_count_kernel, dim3((unsigned)nb), dim3(kBlock),
                     0, stream, a, L.mid_xyz, n_points, L.mid_count,
                     L.crop_counts, nb);
  PGNN_HIP(hipGetLastError());
  rc = exclusive_scan_inplace_i32(L.crop_counts, (int64_t)nb + 1, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(voxel_crop_write_kernel, dim3((unsigned)nb), dim3(kBlock),
                     0, stream, a, L.mid_xyz, L.mid_refl, n_points,
                     L.mid_count, L.crop_counts, nb, out_xyz, out_attr,
                     attr_dim, capacity, out_count);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}
