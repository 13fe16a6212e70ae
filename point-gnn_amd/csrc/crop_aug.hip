// crop_aug object pasting (models/crop_aug.py:75-186 parser_without_collision):
// the whole trial search of one frame in ONE launch.
//
// The reference walks the sampled objects in order and, for each, up to
// max_trails random yaws; a trial needs a ground-height reduction over the
// points under the box (auto_box_height), the box-overlap test against every
// label and every box accepted so far, and a count of the points the box would
// swallow -- all over the CURRENT cloud, which an accepted trial changes
// (swallowed points go, the object's points are prepended).  The chain is
// sequential through that state, so ONE workgroup walks it: per sample one
// strided pass over the N + M points gathers the rows any of its trials could
// touch (the cloud does not fit in LDS and one CU reads it from L2 at ~4 us a
// pass), every trial is a handful of passes over that short list, block
// reductions decide, and the decision is uniform across the workgroup.  No
// other workgroup exists, so nothing waits on another.  Every loop is bounded
// by S * (max_trails + 1) * ceil((N + M) / threads).
//
// State: the working cloud `work` = [block of sample S-1, ..., block of sample
// 0, base cloud] with an int32 alive flag per row.  A sample's block is dead
// until it is accepted; an accepted trial kills the alive rows inside its box
// first.  An order-preserving compaction of `work` by the flags afterwards
// (pgnn_points_compact_f64) is the reference's cloud: each accepted object in
// front of everything before it.
//
// Float64 throughout, products and sums in the reference's order with no
// contraction (the build's -ffp-contract=off).  cos / sin of the DRAWN yaw come
// from the host (NumPy's values); cos / sin of the new label's yaw are the
// device's, so a box face or an integer corner coordinate can differ from
// NumPy's in the last bit -- the fixtures keep 1e-9 away from every decision.
#include "box_overlap.h"
#include "pgnn_common.h"

namespace pgnn {
namespace {

constexpr int kPlaceThreads = 512;
constexpr int kPlaceWaves = kPlaceThreads / 64;
constexpr int kMaxBoxes = 256;  // labels + samples whose Geom is kept in LDS

enum { kModeBox = 0, kModePoint = 1, kModeBoxAndPoint = 2 };

struct PlaceArgs {
  const double *base_xyz;
  int64_t n_base;
  const double *sample_xyz;
  const int32_t *sample_offsets;
  int32_t n_samples;
  int64_t n_sample_points;
  const double *sample_boxes;
  const int32_t *label_corners;
  int32_t n_labels;
  const double *draws;
  int32_t max_trails, mode, auto_box_height, must_have_ground;
  double max_overlap_rate, appr_factor, max_overlap_num_allowed;
  double expand[3];
  double *work_xyz;
  int32_t *alive;
  double *cand_xyz;
  int32_t *cand_idx;
  double *record;
};

// kitti_dataset.py:85-141 box3d_to_cam_points + box3d_to_normals for one
// label: edge directions (rows wx, wy, wz) and the bounds of a point's
// projections on them.  Row 0 is the height direction; rows 1 and 2 (the ones
// sel_xyz_in_box2d keeps, :164-182) do not depend on y3d.
struct BoxRec {
  double n[9], lower[3], upper[3];
};

__device__ __forceinline__ double dot3(const double *a, const double *b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ BoxRec box_record(double x3d, double y3d, double z3d, double length,
                             double height, double width, double c, double s,
                             const double *expand) {
  const double dh = height * (expand[0] - 1.0);
  const double w = width * expand[1], l = length * expand[2];
  const double top = dh / 2, bottom = -height - dh / 2;
  // corners 0, 1, 3, 4: (l/2, top, w/2), (l/2, top, -w/2), (-l/2, top, w/2),
  // (l/2, bottom, w/2), rotated by R(yaw) and moved to the centre
  const double lx[4] = {l / 2, l / 2, -l / 2, l / 2};
  const double ly[4] = {top, top, top, bottom};
  const double lz[4] = {w / 2, -w / 2, w / 2, w / 2};
  double p[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i][0] = ((lx[i] * c + ly[i] * 0.0) + lz[i] * s) + x3d;
    p[i][1] = ((lx[i] * 0.0 + ly[i] * 1.0) + lz[i] * 0.0) + y3d;
    p[i][2] = ((lx[i] * -s + ly[i] * 0.0) + lz[i] * c) + z3d;
  }
  BoxRec r;
  const int far[3] = {3, 1, 2};  // p[] slots of corners 4, 1, 3
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int d = 0; d < 3; ++d) r.n[3 * k + d] = p[0][d] - p[far[k]][d];
    r.lower[k] = dot3(&r.n[3 * k], p[far[k]]);
    r.upper[k] = dot3(&r.n[3 * k], p[0]);
  }
  return r;
}

// strict predicate of sel_xyz_in_box3d (first = 0) / sel_xyz_in_box2d
// (first = 1) in the operation order of points_in_box_f64_kernel
template <int kFirst>
__device__ __forceinline__ bool inside(const BoxRec &r, double x, double y,
                                       double z) {
  bool in = true;
#pragma unroll
  for (int k = kFirst; k < 3; ++k) {
    const double q = (x * r.n[3 * k] + y * r.n[3 * k + 1]) + z * r.n[3 * k + 2];
    in = in && q > r.lower[k] && q < r.upper[k];
  }
  return in;
}

// f(row, x, y, z, live) for every row of pts [n,3] (live = flags[row] != 0;
// flags null: every row), the workgroup striding over the rows.  A pass is a
// chain of L2 round trips: kUnroll rows per thread are loaded before any is
// looked at, so that many loads are in flight per wave (with one row per
// iteration a pass over 23 k rows took ~11 us, the latency of its 45 dependent
// iterations).
constexpr int kUnroll = 8;

template <typename F>
__device__ __forceinline__ void for_rows(const double *pts,
                                         const int32_t *flags, int64_t n,
                                         F &&f) {
  for (int64_t j0 = threadIdx.x; j0 < n;
       j0 += (int64_t)kPlaceThreads * kUnroll) {
    double x[kUnroll], y[kUnroll], z[kUnroll];
    int live[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t j = j0 + (int64_t)u * kPlaceThreads;
      const int64_t jj = j < n ? j : j0;  // j0 < n: a row that exists
      // unconditional loads: one under a branch is waited for at once and
      // the batch falls apart
      live[u] = flags ? flags[jj] : 1;
      x[u] = pts[3 * jj];
      y[u] = pts[3 * jj + 1];
      z[u] = pts[3 * jj + 2];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t j = j0 + (int64_t)u * kPlaceThreads;
      f(j, x[u], y[u], z[u], j < n && live[u] != 0);
    }
  }
}

// np.int32(appr_factor * boxes_3d_to_corners(box)) (nms.py:9-27,
// crop_aug.py:141-142) as the Geom overlap_3d takes: truncation toward zero.
__device__ Geom trial_geometry(double x3d, double y3d, double z3d,
                               double length, double height, double width,
                               double c, double s, double appr) {
  const double hl = length / 2, hw = width / 2;
  const double cx[4] = {hl, hl, -hl, -hl};
  const double cz[4] = {hw, -hw, -hw, hw};
  Geom g;
  const double y0 = (double)(int)(appr * (0.0 + y3d));
  const double y1 = (double)(int)(appr * (-height + y3d));
  g.lo[1] = fmin(y0, y1);
  g.hi[1] = fmax(y0, y1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    g.px[i] = (double)(int)(appr * (((cx[i] * c + 0.0) + cz[i] * s) + x3d));
    g.pz[i] = (double)(int)(appr * (((cx[i] * -s + 0.0) + cz[i] * c) + z3d));
  }
  g.lo[0] = fmin(fmin(g.px[0], g.px[1]), fmin(g.px[2], g.px[3]));
  g.hi[0] = fmax(fmax(g.px[0], g.px[1]), fmax(g.px[2], g.px[3]));
  g.lo[2] = fmin(fmin(g.pz[0], g.pz[1]), fmin(g.pz[2], g.pz[3]));
  g.hi[2] = fmax(fmax(g.pz[0], g.pz[1]), fmax(g.pz[2], g.pz[3]));
  double a2 = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3;
    a2 += g.px[i] * g.pz[j] - g.px[j] * g.pz[i];
  }
  g.area = fabs(a2) * 0.5;
  return g;
}

// a label's integer corner grid [8,3] as a Geom
__device__ Geom corner_geometry(const int32_t *c) {
  Geom g;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int lo = c[k], hi = c[k];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
      lo = min(lo, c[3 * i + k]);
      hi = max(hi, c[3 * i + k]);
    }
    g.lo[k] = (double)lo;
    g.hi[k] = (double)hi;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    g.px[i] = (double)c[3 * i];
    g.pz[i] = (double)c[3 * i + 2];
  }
  double a2 = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3;
    a2 += g.px[i] * g.pz[j] - g.px[j] * g.pz[i];
  }
  g.area = fabs(a2) * 0.5;
  return g;
}

// (max of v, sum of c) over the workgroup, the same value in every thread.
// max and integer sum: independent of the order of the points.
__device__ void block_max_sum(double v, int c, double *s_max, int *s_sum,
                              double *out_max, int *out_sum) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v = fmax(v, __shfl_xor(v, off));
    c += __shfl_xor(c, off);
  }
  if ((threadIdx.x & 63) == 0) {
    s_max[threadIdx.x >> 6] = v;
    s_sum[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  double m = s_max[0];
  int t = s_sum[0];
#pragma unroll
  for (int w = 1; w < kPlaceWaves; ++w) {
    m = fmax(m, s_max[w]);
    t += s_sum[w];
  }
  __syncthreads();  // the slots are free again
  *out_max = m;
  *out_sum = t;
}

__global__ __launch_bounds__(kPlaceThreads) void crop_aug_place_kernel(
    const PlaceArgs a) {
  __shared__ Geom s_box[kMaxBoxes];
  __shared__ double s_max[kPlaceWaves];
  __shared__ int s_sum[kPlaceWaves];
  __shared__ int s_bad, s_ncand;
  const int tid = threadIdx.x;
  const int S = a.n_samples;
  const int64_t M = a.n_sample_points, total = M + a.n_base;
  double *const work = a.work_xyz;
  int32_t *const alive = a.alive;
  const double kNaN = __longlong_as_double(0x7ff8000000000000ll);
  const double kNegInf = __longlong_as_double(0xfff0000000000000ll);

  // the blocks of `work` come from the offsets: refuse a table that is not
  // 0 = off[0] <= off[1] <= ... <= off[S] = M before anything is written
  if (tid == 0) {
    int bad = 0;
    if (S > 0) {
      if (a.sample_offsets[0] != 0 || (int64_t)a.sample_offsets[S] != M) bad = 1;
      for (int s = 0; s < S; ++s)
        if (a.sample_offsets[s + 1] < a.sample_offsets[s]) bad = 1;
    } else if (M != 0) {
      bad = 1;
    }
    s_bad = bad;
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) {
      a.record[3 * S] = -1.0;
      a.record[3 * S + 1] = -1.0;
    }
    return;
  }

  for (int64_t j = tid; j < total; j += kPlaceThreads) {
    if (j < M) {
      work[3 * j] = work[3 * j + 1] = work[3 * j + 2] = 0.0;
      alive[j] = 0;
    } else {
      const int64_t i = j - M;
      work[3 * j] = a.base_xyz[3 * i];
      work[3 * j + 1] = a.base_xyz[3 * i + 1];
      work[3 * j + 2] = a.base_xyz[3 * i + 2];
      alive[j] = 1;
    }
  }
  int nb = 0;
  if (a.mode != kModePoint) {
    nb = a.n_labels;
    for (int b = tid; b < nb; b += kPlaceThreads)
      s_box[b] = corner_geometry(a.label_corners + 24 * b);
  }
  __syncthreads();

  int cursor = 0;
  for (int s = 0; s < S; ++s) {
    const double *bx = a.sample_boxes + 7 * s;
    const double x3d = bx[0], y3d = bx[1], z3d = bx[2], length = bx[3],
                 height = bx[4], width = bx[5], yaw = bx[6];
    const int64_t src0 = a.sample_offsets[s];
    const int64_t cnt = a.sample_offsets[s + 1] - src0;
    const int64_t dst0 = M - a.sample_offsets[s + 1];
    int accepted = 0, draw_index = -1;
    double ground_out = kNaN;
    // Every trial turns the box about the y axis through the origin, which
    // keeps the centre's distance rc from that axis; a point inside the
    // (expanded) footprint is nearer to the centre than the footprint's half
    // diagonal rb.  So only the alive rows with |r - rc| <= rb can be inside
    // any trial's box: they are gathered once per sample (the cloud changes
    // only when the sample is accepted, which ends its trials) and the trials
    // read that list -- a few per cent of the cloud -- instead of the cloud.
    // The list's order is whatever the waves' atomics give; max, counts and
    // the kill are independent of it.
    if (tid == 0) s_ncand = 0;
    __syncthreads();
    if (a.max_trails > 0) {
      const double hl = length * a.expand[2] / 2, hw = width * a.expand[1] / 2;
      const double rc = sqrt(x3d * x3d + z3d * z3d);
      const double rb = sqrt(hl * hl + hw * hw);
      const double slack = 1e-6 * (rb + rc + 1.0);  // >> any rounding here
      const double r_lo = rc - rb - slack, r_hi = rc + rb + slack;
      const int lane = tid & 63;
      for_rows(work, alive, total,
               [&](int64_t j, double x, double y, double z, bool live) {
                 const double r = sqrt(x * x + z * z);
                 const bool hit = live && r >= r_lo && r <= r_hi;
                 const unsigned long long hits = __ballot(hit);
                 if (hits == 0) return;
                 const int leader = __ffsll((long long)hits) - 1;
                 int base = 0;
                 if (lane == leader) base = atomicAdd(&s_ncand, __popcll(hits));
                 base = __shfl(base, leader);
                 if (hit) {
                   const int slot =
                       base + __popcll(hits & ((1ull << lane) - 1ull));
                   a.cand_idx[slot] = (int32_t)j;
                   a.cand_xyz[3 * slot] = x;
                   a.cand_xyz[3 * slot + 1] = y;
                   a.cand_xyz[3 * slot + 2] = z;
                 }
               });
    }
    __syncthreads();
    const int64_t n_cand = s_ncand;
    for (int t = 0; t < a.max_trails && !accepted; ++t) {
      const int k = cursor++;
      const double delta = a.draws[3 * k], c = a.draws[3 * k + 1],
                   sn = a.draws[3 * k + 2];
      // crop_aug.py:104-113: the centre turned about the origin, yaw + delta
      const double nx = (x3d * c + y3d * 0.0) + z3d * sn;
      double ny = (x3d * 0.0 + y3d * 1.0) + z3d * 0.0;
      const double nz = (x3d * -sn + y3d * 0.0) + z3d * c;
      const double nyaw = yaw + delta;
      const double cy = cos(nyaw), sy = sin(nyaw);
      BoxRec rec = box_record(nx, ny, nz, length, height, width, cy, sy,
                              a.expand);
      double adjust = 0.0, ground = kNaN;
      if (a.auto_box_height) {
        // :116-123: the highest y (lowest point, y is down) under the box
        double m = kNegInf;
        int found = 0;
        for_rows(a.cand_xyz, nullptr, n_cand,
                 [&](int64_t, double x, double y, double z, bool live) {
                   if (live && inside<1>(rec, x, y, z)) {
                     m = fmax(m, y);
                     ++found;
                   }
                 });
        block_max_sum(m, found, s_max, s_sum, &m, &found);
        if (found > 0) {
          ground = m;
          adjust = ground - ny;
        } else if (a.must_have_ground) {
          continue;  // the trial is spent
        }
        ny = ny + adjust;
        rec = box_record(nx, ny, nz, length, height, width, cy, sy, a.expand);
      }
      bool ok = true;
      if (a.mode != kModePoint) {
        // :141-145: against every label and every box accepted so far.  The
        // trial's box goes to the free slot behind them, where an acceptance
        // leaves it.
        if (tid == 0)
          s_box[nb] = trial_geometry(nx, ny, nz, length, height, width, cy, sy,
                                     a.appr_factor);
        __syncthreads();
        int over = 0;
        for (int b = tid; b < nb; b += kPlaceThreads)
          if (!(overlap_3d(s_box[nb], s_box[b]) < a.max_overlap_rate)) over = 1;
        ok = __syncthreads_or(over) == 0;
      }
      if (ok && a.mode != kModeBox) {
        // :146-147, :163-164: the points the box would swallow
        int inside_n = 0;
        for_rows(a.cand_xyz, nullptr, n_cand,
                 [&](int64_t, double x, double y, double z, bool live) {
                   if (live && inside<0>(rec, x, y, z)) ++inside_n;
                 });
        double unused;
        block_max_sum(0.0, inside_n, s_max, s_sum, &unused, &inside_n);
        ok = (double)inside_n < a.max_overlap_num_allowed;
      }
      if (!ok) continue;
      // :167-181: the swallowed points go, the object comes in
      for_rows(a.cand_xyz, nullptr, n_cand,
               [&](int64_t i, double x, double y, double z, bool live) {
                 if (live && inside<0>(rec, x, y, z)) alive[a.cand_idx[i]] = 0;
               });
      __syncthreads();  // the block below is dead for every reader above
      for (int64_t p = tid; p < cnt; p += kPlaceThreads) {
        const double x = a.sample_xyz[3 * (src0 + p)],
                     y = a.sample_xyz[3 * (src0 + p) + 1],
                     z = a.sample_xyz[3 * (src0 + p) + 2];
        const int64_t j = dst0 + p;
        const double ry = (x * 0.0 + y * 1.0) + z * 0.0;
        work[3 * j] = (x * c + y * 0.0) + z * sn;
        work[3 * j + 1] = a.auto_box_height ? ry + adjust : ry;
        work[3 * j + 2] = (x * -sn + y * 0.0) + z * c;
        alive[j] = 1;
      }
      if (a.mode != kModePoint) ++nb;
      accepted = 1;
      draw_index = k;
      ground_out = ground;
      __syncthreads();  // the pasted rows and the new box are visible
    }
    if (tid == 0) {
      a.record[3 * s] = (double)accepted;
      a.record[3 * s + 1] = (double)draw_index;
      a.record[3 * s + 2] = ground_out;
    }
  }
  int n_alive = 0;
  for (int64_t j = tid; j < total; j += kPlaceThreads) n_alive += alive[j] != 0;
  double unused;
  block_max_sum(0.0, n_alive, s_max, s_sum, &unused, &n_alive);
  if (tid == 0) {
    a.record[3 * S] = (double)cursor;
    a.record[3 * S + 1] = (double)n_alive;
  }
}

}  // namespace
}  // namespace pgnn

using namespace pgnn;

extern "C" int pgnn_crop_aug_place(
    const double *base_xyz, int64_t n_base, const double *sample_xyz,
    const int32_t *sample_offsets, int32_t n_samples, int64_t n_sample_points,
    const double *sample_boxes, const int32_t *label_corners, int32_t n_labels,
    const double *draws, int32_t max_trails, int32_t overlap_mode,
    int32_t auto_box_height, int32_t must_have_ground, double max_overlap_rate,
    double appr_factor, double max_overlap_num_allowed,
    const double *expand_factor_3, double *work_xyz, int32_t *alive,
    double *cand_xyz, int32_t *cand_idx, double *record, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_base >= 0 && n_samples >= 0 && n_sample_points >= 0 &&
                   n_labels >= 0 && max_trails >= 0 && overlap_mode >= 0 &&
                   overlap_mode <= 2 && expand_factor_3 && record,
               PGNN_E_INVALID, "crop_aug_place: bad argument");
  const int64_t total = n_base + n_sample_points;
  PGNN_REQUIRE(total < (1ll << 30) &&
                   (int64_t)n_samples * max_trails < (1ll << 30),
               PGNN_E_UNSUPPORTED, "crop_aug_place: 2^30 points or draws");
  PGNN_REQUIRE(overlap_mode == kModePoint ||
                   (int64_t)n_labels + n_samples <= kMaxBoxes,
               PGNN_E_UNSUPPORTED,
               "crop_aug_place: more than 256 labels + samples (their boxes "
               "are kept in LDS)");
  PGNN_REQUIRE((n_base == 0 || base_xyz) && (total == 0 || (work_xyz && alive && cand_xyz && cand_idx)) &&
                   (n_sample_points == 0 || sample_xyz) &&
                   (n_samples == 0 || (sample_offsets && sample_boxes)) &&
                   (n_samples == 0 || max_trails == 0 || draws) &&
                   (overlap_mode == kModePoint || n_labels == 0 ||
                    label_corners),
               PGNN_E_INVALID, "crop_aug_place: null pointer");
  PlaceArgs a;
  a.base_xyz = base_xyz;
  a.n_base = n_base;
  a.sample_xyz = sample_xyz;
  a.sample_offsets = sample_offsets;
  a.n_samples = n_samples;
  a.n_sample_points = n_sample_points;
  a.sample_boxes = sample_boxes;
  a.label_corners = label_corners;
  a.n_labels = n_labels;
  a.draws = draws;
  a.max_trails = max_trails;
  a.mode = overlap_mode;
  a.auto_box_height = auto_box_height != 0;
  a.must_have_ground = must_have_ground != 0;
  a.max_overlap_rate = max_overlap_rate;
  a.appr_factor = appr_factor;
  a.max_overlap_num_allowed = max_overlap_num_allowed;
  for (int i = 0; i < 3; ++i) a.expand[i] = expand_factor_3[i];
  a.work_xyz = work_xyz;
  a.alive = alive;
  a.cand_xyz = cand_xyz;
  a.cand_idx = cand_idx;
  a.record = record;
  hipLaunchKernelGGL(crop_aug_place_kernel, dim3(1), dim3(kPlaceThreads), 0,
                     stream, a);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}
