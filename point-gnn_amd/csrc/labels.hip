// Training-target construction for the vertices of the last graph level
// (SURVEY.md §8(f) 4): which ground-truth box contains each vertex
// (dataset/kitti_dataset.py:143-162 sel_xyz_in_box3d, :1132-1284 the three
// assign_classaware_*_label_to_points variants) and the float64 flavour of the
// box encoder that train.py:120-130 feeds with those float64 boxes.
//
// The reference loops over the label boxes and overwrites NumPy slices, so a
// vertex inside several boxes keeps what the LAST one wrote; here one thread
// per vertex walks the (few dozen) boxes in the same order.  Float64 like the
// reference (`np.matmul(xyz_f32, normals_f64.T)`); latency-bound, negligible
// bytes.
#include <string.h>

#include "pgnn_common.h"
#include "sort.h"

namespace pgnn {
namespace {

// one ground-truth box, prepared on the host (box3d_to_normals, :118-141)
struct LabelRecord {
  double normals[9];  // rows wx, wy, wz
  double lower[3], upper[3];
  double action;      // 0 skip, 1 object (class + box + valid), 2 class only
  double cls;         // class value written for action 1 / 2
  double box[7];      // x3d, y3d, z3d, length, height, width, wrapped yaw
};
static_assert(sizeof(LabelRecord) == 24 * sizeof(double), "record layout");

// T: float32 vertices (inference-side callers) or float64 (train.py:100-118
// passes the float64 vertex_coord_list of the augmented cloud)
template <typename T>
__global__ void assign_labels_kernel(const T *__restrict__ xyz, int64_t n,
                                     const LabelRecord *__restrict__ rec,
                                     int n_rec, int32_t *__restrict__ cls,
                                     double *__restrict__ boxes,
                                     float *__restrict__ valid,
                                     int32_t *__restrict__ owner) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  int c = 0, own = -1, box_from = -1;
  float v = 0.0f;
  for (int r = 0; r < n_rec; ++r) {
    const LabelRecord &b = rec[r];
    if (b.action == 0.0) continue;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double p = (x * b.normals[3 * k] + y * b.normals[3 * k + 1]) +
                       z * b.normals[3 * k + 2];
      in = in && p > b.lower[k] && p < b.upper[k];
    }
    if (!in) continue;
    c = (int)b.cls;
    own = r;
    if (b.action == 1.0) {
      box_from = r;
      v = 1.0f;
    } else {
      v = 0.0f;  // class only: the box slot keeps what an earlier object wrote
    }
  }
  if (cls) cls[i] = c;
  if (valid) valid[i] = v;
  if (owner) owner[i] = own;
  if (boxes) {
#pragma unroll
    for (int k = 0; k < 7; ++k)
      boxes[7 * i + k] = box_from >= 0 ? rec[box_from].box[k] : 0.0;
  }
}

// box_encoding.py:231-263 evaluated in float64 (float64 boxes, float32 points,
// Python-float medians) and rounded to float32 once, as train.py:120-130 does
// with `.astype(np.float32)`.  table64 rows = {l, h, w, yaw_offset, active}.
template <typename T>
__global__ void box_encode_f64_kernel(const int32_t *__restrict__ labels,
                                      const T *__restrict__ xyz,
                                      const double *__restrict__ boxes,
                                      const double *__restrict__ table64,
                                      int n_table, int64_t rows, int per_row,
                                      float *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * per_row) return;
  const int64_t r = idx / per_row;
  const int col = (int)(idx - r * per_row);
  const double *b = boxes + idx * 7;
  double d[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) d[i] = b[i];
  d[0] = b[0] - (double)xyz[3 * r];
  d[1] = b[1] - (double)xyz[3 * r + 1];
  d[2] = b[2] - (double)xyz[3 * r + 2];
  const int lab = labels[r];
  if (col == 0 && lab >= 0 && lab < n_table && table64[5 * lab + 4] != 0.0) {
    const double l = table64[5 * lab], h = table64[5 * lab + 1],
                 w = table64[5 * lab + 2], yo = table64[5 * lab + 3];
    d[0] = d[0] / l;
    d[1] = d[1] / h;
    d[2] = d[2] / w;
    d[3] = log(b[3] / l);
    d[4] = log(b[4] / h);
    d[5] = log(b[5] / w);
    const double y = yo != 0.0 ? b[6] - yo : b[6];
    d[6] = y / 0.78539816339744830962;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) out[idx * 7 + i] = (float)d[i];
}

// box_encoding.py:301-343 (the canonical encoding) the same way: everything in
// float64, one rounding at the store.  a = the yaw relative to the anchor;
// the offset is rotated by it and divided by (l, w) for a horizontal anchor,
// (w, l) for a vertical one (:331-337).
template <typename T>
__global__ void box_encode_canonical_f64_kernel(
    const int32_t *__restrict__ labels, const T *__restrict__ xyz,
    const double *__restrict__ boxes, const double *__restrict__ table64,
    int n_table, int64_t rows, int per_row, float *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * per_row) return;
  const int64_t r = idx / per_row;
  const int col = (int)(idx - r * per_row);
  const double *b = boxes + idx * 7;
  double d[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) d[i] = b[i];
  d[0] = b[0] - (double)xyz[3 * r];
  d[1] = b[1] - (double)xyz[3 * r + 1];
  d[2] = b[2] - (double)xyz[3 * r + 2];
  const int lab = labels[r];
  if (col == 0 && lab >= 0 && lab < n_table && table64[5 * lab + 4] != 0.0) {
    const double l = table64[5 * lab], h = table64[5 * lab + 1],
                 w = table64[5 * lab + 2], yo = table64[5 * lab + 3];
    const double p = yo != 0.0 ? w : l, q = yo != 0.0 ? l : w;
    const double a = yo != 0.0 ? b[6] - yo : b[6];
    const double c = cos(a), s = sin(a);
    const double dx = d[0], dz = d[2];
    d[0] = (dx * c - dz * s) / p;
    d[1] = d[1] / h;
    d[2] = (dx * s + dz * c) / q;
    d[3] = log(b[3] / l);
    d[4] = log(b[4] / h);
    d[5] = log(b[5] / w);
    d[6] = a / 0.78539816339744830962;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) out[idx * 7 + i] = (float)d[i];
}

// ---- augmentation primitives (models/preprocess.py) on float64 points -------
// The reference's augmentations turn the float32 cloud into float64 with the
// first `xyz.dot(R.T)` and keep it there until train.py:124 casts back; the
// point-wise parts run here on a float64 [n,3] buffer.

// xyz <- xyz @ rot^T + shift for the selected points (select null: all)
__global__ void points_affine_kernel(double *__restrict__ xyz, int64_t n,
                                     const double r0, const double r1,
                                     const double r2, const double r3,
                                     const double r4, const double r5,
                                     const double r6, const double r7,
                                     const double r8, const double s0,
                                     const double s1, const double s2,
                                     int has_rot,
                                     const int32_t *__restrict__ select) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (select && select[i] == 0) return;
  double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  if (has_rot) {
    const double nx = (x * r0 + y * r1) + z * r2;
    const double ny = (x * r3 + y * r4) + z * r5;
    const double nz = (x * r6 + y * r7) + z * r8;
    x = nx;
    y = ny;
    z = nz;
  }
  xyz[3 * i] = x + s0;
  xyz[3 * i + 1] = y + s1;
  xyz[3 * i + 2] = z + s2;
}

// inside[i] = point i lies strictly inside box `rec` (sel_xyz_in_box3d on
// float64 points); *count += number of inside points with exclude[i] == 0
__global__ void points_in_box_f64_kernel(const double *__restrict__ xyz,
                                         int64_t n, LabelRecord rec,
                                         const int32_t *__restrict__ exclude,
                                         int32_t *__restrict__ inside,
                                         int32_t *__restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool in = false;
  if (i < n) {
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double p = (x * rec.normals[3 * k] + y * rec.normals[3 * k + 1]) +
                       z * rec.normals[3 * k + 2];
      in = in && p > rec.lower[k] && p < rec.upper[k];
    }
    if (inside) inside[i] = in ? 1 : 0;
    if (exclude && exclude[i] != 0) in = false;
  }
  if (count) {
    const unsigned long long bal = __ballot(in);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (int)__popcll(bal));
  }
}

// inside[i] = point i lies strictly inside ANY of the n_rec box records and
// exclude[i] == 0 (the union masks of remove_background / dilute_background,
// preprocess.py:359-360, :420-421; with one record and `exclude` the
// `new_mask & ~mask` of random_box_global_rotation, :211-213); *count += the
// number of such points.  Same predicate, in the same operation order, as
// points_in_box_f64_kernel.
__global__ void points_in_boxes_f64_kernel(const double *__restrict__ xyz,
                                           int64_t n,
                                           const LabelRecord *__restrict__ rec,
                                           int n_rec,
                                           const int32_t *__restrict__ exclude,
                                           int32_t *__restrict__ inside,
                                           int32_t *__restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool any = false;
  if (i < n) {
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    for (int r = 0; r < n_rec && !any; ++r) {
      const LabelRecord &b = rec[r];
      bool in = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double p = (x * b.normals[3 * k] + y * b.normals[3 * k + 1]) +
                         z * b.normals[3 * k + 2];
        in = in && p > b.lower[k] && p < b.upper[k];
      }
      any = in;
    }
    if (exclude && exclude[i] != 0) any = false;
    if (inside) inside[i] = any ? 1 : 0;
  }
  if (count) {
    const unsigned long long bal = __ballot(any);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (int)__popcll(bal));
  }
}

// ---- order-preserving compaction of the cloud ------------------------------
// xyz[mask] / attr[mask] of random_drop (:27), random_box_global_rotation
// (:220-221), remove_background (:427-428) and dilute_background (:367-371):
// count per block, exclusive scan of the block counts, write -- the shape of
// ingest.hip.  Within a block the rank of a kept point is the popcount of the
// wave's ballot below its lane plus the totals of the waves before it.
constexpr int kCompactBlock = 256;

__device__ __forceinline__ bool compact_kept(const int32_t *__restrict__ keep,
                                             const int32_t *__restrict__ drop,
                                             int64_t i, int64_t n) {
  return i < n && (!keep || keep[i] != 0) && !(drop && drop[i] != 0);
}

__global__ __launch_bounds__(kCompactBlock) void compact_count_kernel(
    const int32_t *__restrict__ keep, const int32_t *__restrict__ drop,
    int64_t n, int32_t *__restrict__ block_count) {
  const int64_t i = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
  const bool kept = compact_kept(keep, drop, i, n);
  __shared__ int wave_tot[kCompactBlock / 64];
  const unsigned long long bal = __ballot(kept);
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kCompactBlock / 64; ++w) t += wave_tot[w];
    block_count[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kCompactBlock) void compact_write_kernel(
    const double *__restrict__ xyz, const float *__restrict__ attr,
    int attr_dim, const int32_t *__restrict__ keep,
    const int32_t *__restrict__ drop, int64_t n,
    const int32_t *__restrict__ block_offset, double *__restrict__ out_xyz,
    float *__restrict__ out_attr, int64_t capacity,
    int32_t *__restrict__ out_count, int n_blocks) {
  const int64_t i = (int64_t)blockIdx.x * kCompactBlock + threadIdx.x;
  const bool kept = compact_kept(keep, drop, i, n);
  __shared__ int wave_tot[kCompactBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(kept);
  if (lane == 0) wave_tot[wave] = __popcll(bal);
  __syncthreads();
  int64_t slot = block_offset[blockIdx.x];
  for (int w = 0; w < wave; ++w) slot += wave_tot[w];
  slot += __popcll(bal & ((1ull << lane) - 1ull));
  if (kept && slot < capacity) {
    out_xyz[3 * slot] = xyz[3 * i];
    out_xyz[3 * slot + 1] = xyz[3 * i + 1];
    out_xyz[3 * slot + 2] = xyz[3 * i + 2];
    for (int k = 0; k < attr_dim; ++k)
      out_attr[slot * attr_dim + k] = attr[i * attr_dim + k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = block_offset[n_blocks];
}

// workspace: [block counts | block offsets (+ total) | scan scratch]
struct CompactLayout {
  int32_t *counts, *offsets;
  void *scan_ws;
  size_t scan_bytes;
};

bool carve_compact(Arena &ar, int64_t n_points, CompactLayout *L) {
  const size_t nb =
      (size_t)((n_points + kCompactBlock - 1) / kCompactBlock) + 2;
  L->scan_bytes = scan_scratch_bytes((int64_t)nb);
  L->counts = ar.take<int32_t>(nb);
  L->offsets = ar.take<int32_t>(nb + 1);
  L->scan_ws = ar.take<char>(L->scan_bytes > 0 ? L->scan_bytes : 1);
  return L->counts && L->offsets && L->scan_ws;
}

}  // namespace
}  // namespace pgnn

using namespace pgnn;

extern "C" size_t pgnn_points_compact_workspace_bytes(int64_t n_points) {
  if (n_points < 0) return 0;
  Arena ar(nullptr, 0);
  CompactLayout L;
  carve_compact(ar, n_points, &L);
  return align_up(ar.used, 256);
}

extern "C" int pgnn_points_compact_f64(
    const double *xyz, const float *attr, int32_t attr_dim, int64_t n_points,
    const int32_t *keep, const int32_t *drop, void *workspace,
    size_t workspace_bytes, double *out_xyz, float *out_attr, int64_t capacity,
    int32_t *out_count, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_points >= 0 && n_points <= 0x7fffffffll && capacity >= 0 &&
                   out_count && attr_dim >= 0 && attr_dim <= 4,
               PGNN_E_INVALID, "points_compact: bad argument");
  if (n_points == 0) {
    PGNN_HIP(hipMemsetAsync(out_count, 0, 4, stream));
    return 0;
  }
  if (!attr) attr_dim = 0;
  PGNN_REQUIRE(xyz && (capacity == 0 || (out_xyz && (attr_dim == 0 || out_attr))),
               PGNN_E_INVALID, "points_compact: null pointer");
  const int64_t nb = (n_points + kCompactBlock - 1) / kCompactBlock;
  Arena ar(workspace, workspace_bytes);
  CompactLayout L;
  PGNN_REQUIRE(carve_compact(ar, n_points, &L), PGNN_E_WORKSPACE,
               "points_compact: workspace too small "
               "(see pgnn_points_compact_workspace_bytes)");
  hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nb),
                     dim3(kCompactBlock), 0, stream, keep, drop, n_points,
                     L.counts);
  PGNN_HIP(hipGetLastError());
  int rc = exclusive_scan_i32(L.counts, L.offsets, nb, L.scan_ws, L.scan_bytes,
                              stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(compact_write_kernel, dim3((unsigned)nb),
                     dim3(kCompactBlock), 0, stream, xyz, attr, (int)attr_dim,
                     keep, drop, n_points, L.offsets, out_xyz, out_attr,
                     capacity, out_count, (int)nb);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_points_in_boxes_f64(const double *xyz, int64_t n_points,
                                        const double *box_records,
                                        int32_t n_boxes, const int32_t *exclude,
                                        int32_t *inside, int32_t *count,
                                        void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_points >= 0 && n_boxes >= 0, PGNN_E_INVALID,
               "points_in_boxes: bad size");
  if (count) PGNN_HIP(hipMemsetAsync(count, 0, 4, stream));
  if (n_points == 0) return 0;
  PGNN_REQUIRE(xyz && (box_records || n_boxes == 0), PGNN_E_INVALID,
               "points_in_boxes: null pointer");
  hipLaunchKernelGGL(points_in_boxes_f64_kernel,
                     dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0,
                     stream, xyz, n_points,
                     reinterpret_cast<const LabelRecord *>(box_records),
                     (int)n_boxes, exclude, inside, count);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_points_affine_f64(double *xyz, int64_t n_points,
                                      const double *rot_3x3,
                                      const double *shift_3,
                                      const int32_t *select, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_points >= 0, PGNN_E_INVALID, "points_affine: bad size");
  if (n_points == 0) return 0;
  PGNN_REQUIRE(xyz, PGNN_E_INVALID, "points_affine: null pointer");
  double r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, s[3] = {0, 0, 0};
  if (rot_3x3)
    for (int i = 0; i < 9; ++i) r[i] = rot_3x3[i];
  if (shift_3)
    for (int i = 0; i < 3; ++i) s[i] = shift_3[i];
  hipLaunchKernelGGL(points_affine_kernel,
                     dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0,
                     stream, xyz, n_points, r[0], r[1], r[2], r[3], r[4], r[5],
                     r[6], r[7], r[8], s[0], s[1], s[2], rot_3x3 ? 1 : 0,
                     select);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_points_in_box_f64(const double *xyz, int64_t n_points,
                                      const double *box_record_24,
                                      const int32_t *exclude, int32_t *inside,
                                      int32_t *count, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_points >= 0 && box_record_24, PGNN_E_INVALID,
               "points_in_box: bad argument");
  if (count) PGNN_HIP(hipMemsetAsync(count, 0, 4, stream));
  if (n_points == 0) return 0;
  PGNN_REQUIRE(xyz, PGNN_E_INVALID, "points_in_box: null pointer");
  LabelRecord rec;
  memcpy(&rec, box_record_24, sizeof rec);
  hipLaunchKernelGGL(points_in_box_f64_kernel,
                     dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0,
                     stream, xyz, n_points, rec, exclude, inside, count);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

namespace {
template <typename T>
int assign_impl(const T *xyz, int64_t n_points, const double *label_records,
                int32_t n_records, int32_t *cls_labels, double *boxes_3d,
                float *valid_boxes, int32_t *owner, hipStream_t stream) {
  PGNN_REQUIRE(n_points >= 0 && n_records >= 0, PGNN_E_INVALID,
               "assign_box_labels: bad size");
  if (n_points == 0) return 0;
  PGNN_REQUIRE(xyz && (label_records || n_records == 0), PGNN_E_INVALID,
               "assign_box_labels: null pointer");
  hipLaunchKernelGGL(assign_labels_kernel<T>,
                     dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0,
                     stream, xyz, n_points,
                     reinterpret_cast<const LabelRecord *>(label_records),
                     n_records, cls_labels, boxes_3d, valid_boxes, owner);
  PGNN_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int encode64_impl(const int32_t *cls_labels, const T *xyz, const double *boxes,
                  const double *class_table, int32_t n_table, int64_t n_rows,
                  int32_t boxes_per_row, float *encoded, hipStream_t stream,
                  bool canonical = false) {
  PGNN_REQUIRE(n_rows >= 0 && boxes_per_row > 0 && n_table >= 0,
               PGNN_E_INVALID, "box_encode_f64: bad size");
  if (n_rows == 0) return 0;
  PGNN_REQUIRE(cls_labels && xyz && boxes && encoded &&
                   (class_table || n_table == 0),
               PGNN_E_INVALID, "box_encode_f64: null pointer");
  const int64_t total = n_rows * boxes_per_row;
  hipLaunchKernelGGL(canonical ? box_encode_canonical_f64_kernel<T>
                               : box_encode_f64_kernel<T>,
                     dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     stream, cls_labels, xyz, boxes, class_table, n_table,
                     n_rows, boxes_per_row, encoded);
  PGNN_HIP(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" int pgnn_assign_box_labels(const float *xyz, int64_t n_points,
                                      const double *label_records,
                                      int32_t n_records, int32_t *cls_labels,
                                      double *boxes_3d, float *valid_boxes,
                                      int32_t *owner, void *stream_) {
  PGNN_GUARD_BEGIN
  return assign_impl(xyz, n_points, label_records, n_records, cls_labels,
                     boxes_3d, valid_boxes, owner, (hipStream_t)stream_);
  PGNN_GUARD_END
}

extern "C" int pgnn_assign_box_labels_f64(const double *xyz, int64_t n_points,
                                          const double *label_records,
                                          int32_t n_records,
                                          int32_t *cls_labels, double *boxes_3d,
                                          float *valid_boxes, int32_t *owner,
                                          void *stream_) {
  PGNN_GUARD_BEGIN
  return assign_impl(xyz, n_points, label_records, n_records, cls_labels,
                     boxes_3d, valid_boxes, owner, (hipStream_t)stream_);
  PGNN_GUARD_END
}

extern "C" int pgnn_box_encode_f64(const int32_t *cls_labels, const float *xyz,
                                   const double *boxes,
                                   const double *class_table, int32_t n_table,
                                   int64_t n_rows, int32_t boxes_per_row,
                                   float *encoded, void *stream_) {
  PGNN_GUARD_BEGIN
  return encode64_impl(cls_labels, xyz, boxes, class_table, n_table, n_rows,
                       boxes_per_row, encoded, (hipStream_t)stream_);
  PGNN_GUARD_END
}

extern "C" int pgnn_box_encode_f64_xyz64(const int32_t *cls_labels,
                                         const double *xyz, const double *boxes,
                                         const double *class_table,
                                         int32_t n_table, int64_t n_rows,
                                         int32_t boxes_per_row, float *encoded,
                                         void *stream_) {
  PGNN_GUARD_BEGIN
  return encode64_impl(cls_labels, xyz, boxes, class_table, n_table, n_rows,
                       boxes_per_row, encoded, (hipStream_t)stream_);
  PGNN_GUARD_END
}

extern "C" int pgnn_box_encode_canonical_f64(
    const int32_t *cls_labels, const float *xyz, const double *boxes,
    const double *class_table, int32_t n_table, int64_t n_rows,
    int32_t boxes_per_row, float *encoded, void *stream_) {
  PGNN_GUARD_BEGIN
  return encode64_impl(cls_labels, xyz, boxes, class_table, n_table, n_rows,
                       boxes_per_row, encoded, (hipStream_t)stream_, true);
  PGNN_GUARD_END
}

extern "C" int pgnn_box_encode_canonical_f64_xyz64(
    const int32_t *cls_labels, const double *xyz, const double *boxes,
    const double *class_table, int32_t n_table, int64_t n_rows,
    int32_t boxes_per_row, float *encoded, void *stream_) {
  PGNN_GUARD_BEGIN
  return encode64_impl(cls_labels, xyz, boxes, class_table, n_table, n_rows,
                       boxes_per_row, encoded, (hipStream_t)stream_, true);
  PGNN_GUARD_END
}
