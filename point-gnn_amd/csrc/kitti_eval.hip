// KITTI object-detection average precision (2D box, bird's-eye box, 3D box;
// 11- and 40-point interpolation) of a whole frame set, on the device.  The
// protocol is DESIGN.md §9.5; every name below (cleaning, matching, thresholds,
// curve) is a heading there.  All arithmetic is float64.
//
// Launch structure (nine launches and two offset uploads, whatever the number
// of frames; nothing is read back):
//   prep        per box: the 9 (class, difficulty) cleaning results packed into
//               one word; zeroes the counters and the score slots
//   scan        pair_off[f] = sum over earlier frames of n_gt * n_det
//   pairs       per (ground truth, detection) pair of a frame: the 2D / BEV /
//               3D union overlaps and the 2D detection-criterion overlap, once;
//               every later comparison reads these values
//   pass 1      matching without false positives: wave = frame, lane = one of
//               the 27 (metric, class, difficulty) combinations; records the
//               matched scores (one slot per ground truth) and n_gt
//   sort        per combination, descending (bitonic, one workgroup each)
//   thresholds  per combination, serial: the <= 41 score thresholds
//   pass 2      matching with false positives: wave = frame, lane = threshold,
//               blockIdx.y = combination; int64 atomics into [27][41][3]
//   finalize    precision, recall, running maximum, AP_R11 and AP_R40
//
// Orientation (AOS, the 2D metric only) adds no launch: the pairs kernel writes
// a fifth plane, sim = (1 + cos(alpha_gt - alpha_det)) / 2 of a pair, pass 2
// adds the plane's value at every true positive to a float64 per lane, each
// wave stores its 41 sums into its own slot, and finalize adds the slots in
// ascending wave index.  The grid depends on the number of frames only, so the
// sums are the same bits on every run.  All of it hangs on template flags: the
// kernels without orientation are the code they were before it existed.
//
// Pass 2 puts the thresholds of one (frame, combination) on the lanes of one
// wave: the loops over ground truths and detections, the cleaning flags, the
// overlaps and the `> MIN_OVERLAP` test are then the same in every lane (one
// pair in ~15 passes that test), and only `score < thresh` and the assigned
// bit differ.  The assigned set is a bit mask in LDS, word-major
// ([word][lane], 8-byte words: consecutive lanes on consecutive bank pairs, no
// conflicts), ceil(max detections / 64) words per lane, at most 32 KiB per
// workgroup of four waves.  Waves stride over frames and add their counts once
// at the end, so a counter sees one atomic per wave, not one per frame.
//
// pgnn_kitti_match keeps what the matching of one
// combination at one threshold decides, box by box: prep, scan and pairs as
// above, then kitti_match_kernel, described where it stands.
#include "box_overlap.h"

namespace pgnn {
namespace {

constexpr int kRow = PGNN_KITTI_ROW;
constexpr int kCombos = PGNN_KITTI_COMBOS;  // [metric][class][difficulty]
constexpr int kPts = PGNN_KITTI_SAMPLE_PTS;
constexpr int kMaxDet = PGNN_KITTI_MAX_DET;
constexpr int kMaxGt = PGNN_KITTI_MAX_GT;
constexpr int kSortTile = 4096;  // keys of one LDS tile of the sort (32 KiB)
constexpr int kWaves = 4;        // frames in flight per workgroup (passes 1, 2)

// columns of a box row (PGNN_KITTI_ROW doubles, see the header)
enum { X0, Y0, X1, Y1, BH, BW, BL, BX, BY, BZ, RY, TRUNC, OCC, SCORE };
// name codes
enum { kCar, kPed, kCyc, kVan, kSitting, kDontCare, kOther };
constexpr int kDontCareBit = 1 << 18;

// MIN_OVERLAP[metric][class], a kernel argument by value; a chain of selects,
// not an indexed load, since pass 1 has the combination on the lanes
struct OverlapTable {
  double v[9];
};
__device__ __forceinline__ double min_overlap(const OverlapTable &tab, int metric,
                                              int c) {
  const int k = metric * 3 + c;
  double r = tab.v[0];
#pragma unroll
  for (int q = 1; q < 9; ++q) r = k == q ? tab.v[q] : r;
  return r;
}
__device__ __forceinline__ double min_height(int d) { return d == 0 ? 40.0 : 25.0; }
__device__ __forceinline__ double max_occlusion(int d) { return (double)d; }
__device__ __forceinline__ double max_truncation(int d) {
  return d == 0 ? 0.15 : (d == 1 ? 0.3 : 0.5);
}

// §9.5 "Cleaning": ignored_gt / ignored_det in {-1, 0, 1}
__device__ int clean_gt(const double *r, int name, int c, int d) {
  const int valid =
      name == c ? 1
                : (((c == kCar && name == kVan) || (c == kPed && name == kSitting))
                       ? 0
                       : -1);
  const double height = fabs(r[Y1] - r[Y0]);
  const bool ignore = r[OCC] > max_occlusion(d) ||
                      r[TRUNC] > max_truncation(d) || height <= min_height(d);
  if (valid == 1 && !ignore) return 0;
  if (valid == 0 || (ignore && valid == 1)) return 1;
  return -1;
}

__device__ int clean_det(const double *r, int name, int c, int d) {
  const double height = fabs(r[Y1] - r[Y0]);
  if (height < min_height(d)) return 1;
  return name == c ? 0 : -1;
}

// flags word of a box: bits [2s, 2s+1], s = class * 3 + difficulty, hold
// ignored + 1; bit 18 marks a DontCare ground truth
__device__ __forceinline__ int flag_of(int32_t word, int s) {
  return ((word >> (2 * s)) & 3) - 1;
}

__global__ __launch_bounds__(256) void kitti_prep_kernel(
    const double *__restrict__ gt, const int32_t *__restrict__ gt_names,
    int64_t n_gt, const double *__restrict__ det,
    const int32_t *__restrict__ det_names, int64_t n_det,
    int32_t *__restrict__ gt_flags, int32_t *__restrict__ det_flags,
    unsigned long long *__restrict__ keys, int64_t n_keys,
    int64_t *__restrict__ counters, int64_t *__restrict__ n_gt_out,
    int32_t *__restrict__ n_rec, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < n_gt) {
      const double *r = gt + idx * kRow;
      const int name = gt_names[idx];
      int32_t w = name == kDontCare ? kDontCareBit : 0;
      for (int c = 0; c < 3; ++c)
        for (int d = 0; d < 3; ++d)
          w |= (clean_gt(r, name, c, d) + 1) << (2 * (c * 3 + d));
      gt_flags[idx] = w;
    }
    if (idx < n_det) {
      const double *r = det + idx * kRow;
      const int name = det_names[idx];
      int32_t w = 0;
      for (int c = 0; c < 3; ++c)
        for (int d = 0; d < 3; ++d)
          w |= (clean_det(r, name, c, d) + 1) << (2 * (c * 3 + d));
      det_flags[idx] = w;
    }
    if (idx < n_keys) keys[idx] = 0ull;
    if (idx < (int64_t)kCombos * kPts * 3) counters[idx] = 0;
    if (idx < kCombos) {
      n_gt_out[idx] = 0;
      n_rec[idx] = 0;
    }
  }
}

// pair_off[f] = sum_{g < f} n_gt(g) * n_det(g), pair_off[F] = the total; one
// workgroup, each thread a contiguous run of frames
__global__ __launch_bounds__(1024) void kitti_scan_kernel(
    const int32_t *__restrict__ gt_off, const int32_t *__restrict__ det_off,
    int64_t n_frames, int64_t *__restrict__ pair_off) {
  __shared__ int64_t part[1024];
  const int tid = threadIdx.x;
  const int64_t chunk = (n_frames + 1023) / 1024;
  int64_t begin = (int64_t)tid * chunk, end = begin + chunk;
  if (begin > n_frames) begin = n_frames;
  if (end > n_frames) end = n_frames;
  int64_t sum = 0;
  for (int64_t f = begin; f < end; ++f)
    sum += (int64_t)(gt_off[f + 1] - gt_off[f]) *
           (int64_t)(det_off[f + 1] - det_off[f]);
  part[tid] = sum;
  __syncthreads();
  for (int s = 1; s < 1024; s <<= 1) {
    const int64_t v = tid >= s ? part[tid - s] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int64_t run = part[tid] - sum;
  for (int64_t f = begin; f < end; ++f) {
    pair_off[f] = run;
    run += (int64_t)(gt_off[f + 1] - gt_off[f]) *
           (int64_t)(det_off[f + 1] - det_off[f]);
  }
  if (tid == 1023) pair_off[n_frames] = part[1023];
}

// §9.5 "Overlaps": the BEV rectangle of a box row
__device__ void bev_geom(const double *r, Geom &g) {
  const double c = cos(r[RY]), s = sin(r[RY]);
  const double hl = r[BL] / 2, hw = r[BW] / 2;
  const double dx[4] = {hl, hl, -hl, -hl};
  const double dz[4] = {hw, -hw, -hw, hw};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g.px[k] = c * dx[k] + s * dz[k] + r[BX];
    g.pz[k] = -s * dx[k] + c * dz[k] + r[BZ];
  }
}

// planes of the overlap workspace, each n_pairs doubles; a frame's block
// starts at pair_off[f], row-major [ground truth][detection]
enum { kOv2d, kOvBev, kOv3d, kOvDontCare, kOvSim };

// kMode: what is written.  kPairOverlaps: the four overlap planes into `ov`;
// kPairBoth: those and the orientation plane `sim`; kPairSim: `sim` alone.
enum { kPairOverlaps, kPairBoth, kPairSim };

// §9.5 "Orientation": sim of a pair, 0 unless the 2D union overlap is > 0 (a
// pair that can become a true positive of the 2D metric has one)
__device__ __forceinline__ double orientation_term(double o2, double alpha_gt,
                                                   double alpha_det) {
  return o2 > 0.0 ? (1.0 + cos(alpha_gt - alpha_det)) / 2.0 : 0.0;
}

template <int kMode>
__global__ __launch_bounds__(256) void kitti_pair_kernel(
    const int32_t *__restrict__ gt_off, const int32_t *__restrict__ det_off,
    const int64_t *__restrict__ pair_off, int64_t n_frames,
    const double *__restrict__ gt, const int32_t *__restrict__ gt_names,
    const double *__restrict__ det, double *__restrict__ ov, int64_t n_pairs,
    const double *__restrict__ gt_alpha, const double *__restrict__ det_alpha,
    double *__restrict__ sim) {
  for (int64_t f = blockIdx.x; f < n_frames; f += gridDim.x) {
    const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
    const int d0 = det_off[f], nd = det_off[f + 1] - d0;
    const int64_t base = pair_off[f];
    const int np = ng * nd;  // <= kMaxGt * kMaxDet
    for (int p = threadIdx.x; p < np; p += blockDim.x) {
      const int i = p / nd, j = p - i * nd;
      const double *b = gt + (int64_t)(g0 + i) * kRow;   // ground truth
      const double *a = det + (int64_t)(d0 + j) * kRow;  // detection
      // 2D
      const double w = fmin(a[X1], b[X1]) - fmax(a[X0], b[X0]);
      const double h = fmin(a[Y1], b[Y1]) - fmax(a[Y0], b[Y0]);
      double o2 = 0.0, odc = 0.0;
      if (!(w <= 0.0 || h <= 0.0)) {
        const double inter = w * h;
        const double area_a = (a[X1] - a[X0]) * (a[Y1] - a[Y0]);
        const double area_b = (b[X1] - b[X0]) * (b[Y1] - b[Y0]);
        o2 = inter / (area_a + area_b - inter);
        odc = inter / area_a;
      }
      if (kMode != kPairOverlaps)
        sim[base + p] = orientation_term(o2, gt_alpha[g0 + i], det_alpha[d0 + j]);
      if (kMode == kPairSim) continue;
      if (gt_names[g0 + i] != kDontCare) odc = 0.0;
      // BEV and 3D
      Geom ga, gb;
      bev_geom(a, ga);
      bev_geom(b, gb);
      const double inter_bev = clip_area(ga, gb);
      const double obev =
          inter_bev / (a[BL] * a[BW] + b[BL] * b[BW] - inter_bev);
      const double ymax = fmin(a[BY], b[BY]);
      const double ymin = fmax(a[BY] - a[BH], b[BY] - b[BH]);
      const double inter_vol = inter_bev * fmax(0.0, ymax - ymin);
      const double o3 = inter_vol / (a[BH] * a[BL] * a[BW] +
                                     b[BH] * b[BL] * b[BW] - inter_vol);
      ov[kOv2d * n_pairs + base + p] = o2;
      ov[kOvBev * n_pairs + base + p] = obev;
      ov[kOv3d * n_pairs + base + p] = o3;
      ov[kOvDontCare * n_pairs + base + p] = odc;
    }
  }
}

// a score as an unsigned key of the same order (-0.0 folded onto +0.0); key 0
// is the empty slot and sorts last
__device__ __forceinline__ unsigned long long score_key(double s) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(s + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_score(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// §9.5 "Matching" of one frame for one (metric, class, difficulty) at one
// threshold.  kFp = compute_fp.  `mask` is this lane's assigned set: word w at
// mask[w * 64].  Without kFp the matched scores go to keys[i] (the slot of
// ground truth i).  kAos (with kFp only): `sim` is the frame's block of the
// orientation plane and `similarity` gains sim[i][det_idx] at every true
// positive; no decision reads either.
template <bool kFp, bool kAos = false>
__device__ void match_frame(int ng, int nd, const int32_t *__restrict__ gfl,
                            const int32_t *__restrict__ dfl,
                            const double *__restrict__ drow,
                            const double *__restrict__ ov,
                            const double *__restrict__ ov_dc, int s,
                            double min_ov, double thresh, bool is_2d,
                            unsigned long long *mask, int words,
                            unsigned long long *keys, long long &tp,
                            long long &fp, long long &fn,
                            const double *__restrict__ sim = nullptr,
                            double *similarity = nullptr) {
  for (int w = 0; w < words; ++w) mask[w * 64] = 0ull;
  for (int i = 0; i < ng; ++i) {
    const int ig = flag_of(gfl[i], s);
    if (ig < 0) continue;
    int det_idx = -1;
    bool valid = false, assigned_ignored = false;
    double best = 0.0, max_overlap = 0.0;
    const double *row = ov + (int64_t)i * nd;
    for (int j = 0; j < nd; ++j) {
      const int idj = flag_of(dfl[j], s);
      if (idj < 0) continue;
      // every rule of step 3 asks for ov > MIN_OVERLAP
      const double o = row[j];
      if (!(o > min_ov)) continue;
      if ((mask[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
      const double sc = drow[(int64_t)j * kRow + SCORE];
      if (kFp) {
        if (sc < thresh) continue;
        if (idj == 0 && (o > max_overlap || assigned_ignored)) {
          max_overlap = o;
          det_idx = j;
          valid = true;
          assigned_ignored = false;
        } else if (idj == 1 && !valid) {
          det_idx = j;
          valid = true;
          assigned_ignored = true;
        }
      } else if (!valid || sc > best) {
        det_idx = j;
        best = sc;
        valid = true;
      }
    }
    if (det_idx < 0) {
      if (ig == 0) ++fn;
    } else {
      if (!(ig == 1 || flag_of(dfl[det_idx], s) == 1)) {
        ++tp;
        if (!kFp)
          keys[i] = score_key(drow[(int64_t)det_idx * kRow + SCORE]);
        if (kAos) *similarity += sim[(int64_t)i * nd + det_idx];
      }
      mask[(det_idx >> 6) * 64] |= 1ull << (det_idx & 63);
    }
  }
  if (kFp) {
    for (int j = 0; j < nd; ++j) {
      if (flag_of(dfl[j], s) != 0) continue;
      if ((mask[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
      if (drow[(int64_t)j * kRow + SCORE] < thresh) continue;
      ++fp;
    }
    if (is_2d) {
      long long nstuff = 0;
      for (int i = 0; i < ng; ++i) {
        if (!(gfl[i] & kDontCareBit)) continue;
        const double *row = ov_dc + (int64_t)i * nd;
        for (int j = 0; j < nd; ++j) {
          if (flag_of(dfl[j], s) != 0) continue;
          if ((mask[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
          if (drow[(int64_t)j * kRow + SCORE] < thresh) continue;
          if (row[j] > min_ov) {
            mask[(j >> 6) * 64] |= 1ull << (j & 63);
            ++nstuff;
          }
        }
      }
      fp -= nstuff;
    }
  }
}

// blockDim = (64, kWaves): threadIdx.y picks the frame, threadIdx.x < 27 the
// combination
__global__ __launch_bounds__(64 * kWaves) void kitti_pass1_kernel(
    const int32_t *__restrict__ gt_off, const int32_t *__restrict__ det_off,
    const int64_t *__restrict__ pair_off, int64_t n_frames,
    const int32_t *__restrict__ gt_flags, const int32_t *__restrict__ det_flags,
    const double *__restrict__ det, const double *__restrict__ ov,
    int64_t n_pairs, int words, unsigned long long *__restrict__ keys,
    int64_t n_pad, int64_t *__restrict__ n_gt_out, int32_t *__restrict__ n_rec,
    const OverlapTable table) {
  extern __shared__ unsigned long long lds_mask[];
  const int combo = threadIdx.x;
  if (combo >= kCombos) return;  // no barrier below
  unsigned long long *mask = lds_mask + (size_t)threadIdx.y * words * 64 + combo;
  const int metric = combo / 9, c = (combo / 3) % 3, s = combo % 9;
  const double min_ov = min_overlap(table, metric, c);
  long long tp = 0, fp = 0, fn = 0, n_gt = 0;
  for (int64_t f = (int64_t)blockIdx.x * kWaves + threadIdx.y; f < n_frames;
       f += (int64_t)gridDim.x * kWaves) {
    const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
    const int d0 = det_off[f], nd = det_off[f + 1] - d0;
    for (int i = 0; i < ng; ++i) n_gt += flag_of(gt_flags[g0 + i], s) == 0;
    match_frame<false>(ng, nd, gt_flags + g0, det_flags + d0,
                       det + (int64_t)d0 * kRow,
                       ov + metric * n_pairs + pair_off[f], nullptr, s,
                       min_ov, 0.0, false, mask, (nd + 63) >> 6,
                       keys + combo * n_pad + g0, tp, fp, fn);
  }
  if (n_gt)
    atomicAdd((unsigned long long *)n_gt_out + combo, (unsigned long long)n_gt);
  if (tp) atomicAdd(n_rec + combo, (int)tp);
}

// Descending bitonic sort of each combination's n_pad keys (a power of two),
// one workgroup per combination; steps whose stride fits a tile run in LDS.
__device__ __forceinline__ void bitonic_step(unsigned long long *a, int64_t i,
                                             int64_t l, bool down) {
  const unsigned long long x = a[i], y = a[l];
  if (down ? x < y : x > y) {
    a[i] = y;
    a[l] = x;
  }
}

__global__ __launch_bounds__(1024) void kitti_sort_kernel(
    unsigned long long *__restrict__ keys, int64_t n_pad) {
  __shared__ unsigned long long tile[kSortTile];
  unsigned long long *a = keys + (int64_t)blockIdx.x * n_pad;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int t = n_pad < kSortTile ? (int)n_pad : kSortTile;
  // merge size k: the steps of stride >= t in global memory, then those of
  // stride t/2 .. 1 tile by tile in LDS; the k == t round sorts each tile
  // from scratch (merge sizes 2 .. t in one visit)
  for (int64_t k = 2; k <= n_pad; k <<= 1) {
    if (k < t) continue;  // folded into the k == t round below
    for (int64_t j = k >> 1; j >= t; j >>= 1) {
      for (int64_t idx = tid; idx < n_pad / 2; idx += nt) {
        const int64_t i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1));
        bitonic_step(a, i, i | j, (i & k) == 0);
      }
      __syncthreads();
    }
    for (int64_t base = 0; base < n_pad; base += t) {
      for (int x = tid; x < t; x += nt) tile[x] = a[base + x];
      __syncthreads();
      for (int64_t kk = (k == t ? 2 : k); kk <= k; kk <<= 1) {
        for (int j = (int)(kk < t ? kk >> 1 : t >> 1); j > 0; j >>= 1) {
          for (int idx = tid; idx < t / 2; idx += nt) {
            const int i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1));
            bitonic_step(tile, i, i | j, ((base + i) & kk) == 0);
          }
          __syncthreads();
        }
      }
      for (int x = tid; x < t; x += nt) a[base + x] = tile[x];
      __syncthreads();
    }
  }
}

// §9.5 "Thresholds": one thread per combination
__global__ void kitti_threshold_kernel(
    const unsigned long long *__restrict__ keys, int64_t n_pad,
    const int64_t *__restrict__ n_gt, const int32_t *__restrict__ n_rec,
    double *__restrict__ thresholds, int32_t *__restrict__ n_thresholds) {
  const int combo = threadIdx.x;
  if (combo >= kCombos) return;
  const unsigned long long *v = keys + combo * n_pad;
  const int64_t n = n_rec[combo];
  const double total = (double)n_gt[combo];
  double current_recall = 0.0;
  int k = 0;
  for (int64_t i = 0; i < n && k < kPts; ++i) {
    const double l = (double)(i + 1) / total;
    const double r = i < n - 1 ? (double)(i + 2) / total : l;
    if ((r - current_recall) < (current_recall - l) && i < n - 1) continue;
    thresholds[combo * kPts + k++] = key_score(v[i]);
    current_recall += 1.0 / 40.0;
  }
  n_thresholds[combo] = k;
  for (; k < kPts; ++k) thresholds[combo * kPts + k] = 0.0;
}

// blockDim = (64, kWaves), grid = (frame groups, 27): threadIdx.x is the
// threshold, threadIdx.y the frame slot, blockIdx.y the combination.  kAos:
// the waves of the nine 2D combinations also sum the orientation plane over
// their true positives and store the sums at wave_sim[combo][wave][t], wave =
// blockIdx.x * kWaves + threadIdx.y; a lane past n_thresholds stores nothing.
template <bool kAos>
__global__ __launch_bounds__(64 * kWaves) void kitti_pass2_kernel(
    const int32_t *__restrict__ gt_off, const int32_t *__restrict__ det_off,
    const int64_t *__restrict__ pair_off, int64_t n_frames,
    const int32_t *__restrict__ gt_flags, const int32_t *__restrict__ det_flags,
    const double *__restrict__ det, const double *__restrict__ ov,
    int64_t n_pairs, int words, const double *__restrict__ thresholds,
    const int32_t *__restrict__ n_thresholds, int64_t *__restrict__ counters,
    const OverlapTable table, double *__restrict__ wave_sim) {
  extern __shared__ unsigned long long lds_mask[];
  const int combo = blockIdx.y, t = threadIdx.x;
  if (t >= n_thresholds[combo] || t >= kPts) return;  // no barrier below
  unsigned long long *mask = lds_mask + (size_t)threadIdx.y * words * 64 + t;
  const int metric = combo / 9, c = (combo / 3) % 3, s = combo % 9;
  const double thresh = thresholds[combo * kPts + t];
  const double min_ov = min_overlap(table, metric, c);
  long long tp = 0, fp = 0, fn = 0;
  double similarity = 0.0;
  for (int64_t f = (int64_t)blockIdx.x * kWaves + threadIdx.y; f < n_frames;
       f += (int64_t)gridDim.x * kWaves) {
    const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
    const int d0 = det_off[f], nd = det_off[f + 1] - d0;
    const int64_t base = pair_off[f];
    if (kAos && metric == 0)
      match_frame<true, true>(
          ng, nd, gt_flags + g0, det_flags + d0, det + (int64_t)d0 * kRow,
          ov + base, ov + kOvDontCare * n_pairs + base, s, min_ov, thresh, true,
          mask, (nd + 63) >> 6, nullptr, tp, fp, fn,
          ov + kOvSim * n_pairs + base, &similarity);
    else
      match_frame<true>(ng, nd, gt_flags + g0, det_flags + d0,
                        det + (int64_t)d0 * kRow, ov + metric * n_pairs + base,
                        ov + kOvDontCare * n_pairs + base, s, min_ov, thresh,
                        metric == 0, mask, (nd + 63) >> 6, nullptr, tp, fp, fn);
  }
  if (kAos && metric == 0) {
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    const int64_t wave = (int64_t)blockIdx.x * kWaves + threadIdx.y;
    wave_sim[(combo * waves + wave) * kPts + t] = similarity;
  }
  unsigned long long *out =
      (unsigned long long *)counters + ((int64_t)combo * kPts + t) * 3;
  if (tp) atomicAdd(out + 0, (unsigned long long)tp);
  if (fp) atomicAdd(out + 1, (unsigned long long)fp);
  if (fn) atomicAdd(out + 2, (unsigned long long)fn);
}

// §9.5 "Orientation", the curve: blockDim = (64, 9), threadIdx.y = one of the
// nine 2D combinations, threadIdx.x = threshold.  Each thread adds its
// threshold's wave slots in ascending wave index (41 neighbouring lanes read
// neighbouring doubles); thread 0 of a combination then takes the running
// maximum and the two sums, as for precision.
__device__ void orientation_curve(const int64_t *__restrict__ counters,
                                  const int32_t *__restrict__ n_thresholds,
                                  const double *__restrict__ wave_sim,
                                  int64_t waves, double *__restrict__ similarity,
                                  double *__restrict__ orientation,
                                  double *__restrict__ aos_r11,
                                  double *__restrict__ aos_r40) {
  const int combo = threadIdx.y, t = threadIdx.x;
  const int n = n_thresholds[combo];
  double *o = orientation + combo * kPts;
  if (t < kPts) {
    double sum = 0.0;
    if (t < n) {
      const double *slot = wave_sim + (int64_t)combo * waves * kPts + t;
#pragma unroll 8
      for (int64_t w = 0; w < waves; ++w) sum += slot[w * kPts];
    }
    const int64_t *k = counters + ((int64_t)combo * kPts + t) * 3;
    similarity[combo * kPts + t] = sum;
    o[t] = (t < n && k[0] + k[1] > 0) ? sum / ((double)k[0] + (double)k[1]) : 0.0;
  }
  __syncthreads();  // every thread of the workgroup arrives
  if (t != 0) return;
  for (int q = kPts - 2; q >= 0; --q) o[q] = fmax(o[q], o[q + 1]);
  double s11 = 0.0, s40 = 0.0;
  for (int q = 0; q < kPts; q += 4) s11 += o[q];
  for (int q = 1; q < kPts; ++q) s40 += o[q];
  aos_r11[combo] = s11 / 11.0;
  aos_r40[combo] = s40 / 40.0;
}

// §9.5 "Curve and AP": one thread per combination.  kAos: blockDim = (64, 9)
// and the orientation curve follows in the same launch.
template <bool kAos>
__global__ void kitti_finalize_kernel(
    const int64_t *__restrict__ counters,
    const int32_t *__restrict__ n_thresholds, double *__restrict__ precision,
    double *__restrict__ recall, double *__restrict__ ap_r11,
    double *__restrict__ ap_r40, const double *__restrict__ wave_sim,
    int64_t waves, double *__restrict__ similarity,
    double *__restrict__ orientation, double *__restrict__ aos_r11,
    double *__restrict__ aos_r40) {
  if (kAos)
    orientation_curve(counters, n_thresholds, wave_sim, waves, similarity,
                      orientation, aos_r11, aos_r40);
  const int combo = threadIdx.x;
  if (combo >= kCombos || threadIdx.y != 0) return;
  const int n = n_thresholds[combo];
  double *p = precision + combo * kPts, *r = recall + combo * kPts;
  for (int t = 0; t < kPts; ++t) {
    const int64_t *k = counters + ((int64_t)combo * kPts + t) * 3;
    const double tp = (double)k[0], fp = (double)k[1], fn = (double)k[2];
    // an empty denominator (no detection kept, no ground truth) gives 0
    p[t] = (t < n && k[0] + k[1] > 0) ? tp / (tp + fp) : 0.0;
    r[t] = (t < n && k[0] + k[2] > 0) ? tp / (tp + fn) : 0.0;
  }
  for (int t = kPts - 2; t >= 0; --t) p[t] = fmax(p[t], p[t + 1]);
  double s11 = 0.0, s40 = 0.0;
  for (int t = 0; t < kPts; t += 4) s11 += p[t];
  for (int t = 1; t < kPts; ++t) s40 += p[t];
  ap_r11[combo] = s11 / 11.0;
  ap_r40[combo] = s40 / 40.0;
}

int64_t next_pow2(int64_t n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

struct Sizes {
  int64_t n_frames, n_gt, n_det, n_pairs, n_pad;
  int max_det;
};

struct Workspace {
  int32_t *gt_off, *det_off, *gt_flags, *det_flags, *n_rec;
  int64_t *pair_off;
  double *ov, *wave_sim;
  unsigned long long *keys;
  size_t bytes;
};

// workgroups of pass 2 along x: kWaves frames each, at most 256 (the waves
// stride over the rest), so at most 1 024 waves per combination
int64_t pass2_groups(int64_t n_frames) {
  int64_t groups = (n_frames + kWaves - 1) / kWaves;
  if (groups < 1) groups = 1;
  return groups < 256 ? groups : 256;
}

// lays the workspace out; with base == nullptr only `bytes` is meaningful.
// with_aos: a fifth pair plane and the wave slots [9][waves][41] of pass 2.
Workspace carve(void *base, size_t size, int64_t n_frames, int64_t n_gt,
                int64_t n_det, int64_t n_pairs, bool with_eval,
                bool with_aos = false) {
  Arena arena(base, base ? size : 0);
  Workspace w;
  w.gt_off = arena.take<int32_t>((size_t)n_frames + 1);
  w.det_off = arena.take<int32_t>((size_t)n_frames + 1);
  w.pair_off = arena.take<int64_t>((size_t)n_frames + 1);
  w.gt_flags = w.det_flags = w.n_rec = nullptr;
  w.ov = w.wave_sim = nullptr;
  w.keys = nullptr;
  if (with_eval) {
    w.gt_flags = arena.take<int32_t>((size_t)(n_gt > 0 ? n_gt : 1));
    w.det_flags = arena.take<int32_t>((size_t)(n_det > 0 ? n_det : 1));
    w.n_rec = arena.take<int32_t>(kCombos);
    w.ov = arena.take<double>((size_t)(n_pairs > 0 ? n_pairs : 1) *
                              (with_aos ? 5 : 4));
    w.keys = arena.take<unsigned long long>((size_t)kCombos *
                                            (size_t)next_pow2(n_gt));
    if (with_aos)
      w.wave_sim = arena.take<double>(
          (size_t)9 * (size_t)(pass2_groups(n_frames) * kWaves) * kPts);
  }
  w.bytes = align_up(arena.used, 256);
  return w;
}

// host-side checks shared by the entries; fills `sz`
int check_offsets(const char *who, const int32_t *gt_off,
                  const int32_t *det_off, int64_t n_frames, Sizes *sz) {
  static thread_local char msg[160];
  if (n_frames < 0 || n_frames > PGNN_KITTI_MAX_FRAMES) {
    snprintf(msg, sizeof msg, "%s: n_frames out of range", who);
    return fail(n_frames < 0 ? PGNN_E_INVALID : PGNN_E_UNSUPPORTED, msg);
  }
  if (!gt_off || !det_off) {
    snprintf(msg, sizeof msg, "%s: null offsets", who);
    return fail(PGNN_E_INVALID, msg);
  }
  if (gt_off[0] != 0 || det_off[0] != 0) {
    snprintf(msg, sizeof msg, "%s: offsets must start at 0", who);
    return fail(PGNN_E_INVALID, msg);
  }
  sz->n_pairs = 0;
  sz->max_det = 0;
  for (int64_t f = 0; f < n_frames; ++f) {
    const int64_t ng = (int64_t)gt_off[f + 1] - gt_off[f];
    const int64_t nd = (int64_t)det_off[f + 1] - det_off[f];
    if (ng < 0 || nd < 0) {
      snprintf(msg, sizeof msg, "%s: offsets not ascending at frame %lld", who,
               (long long)f);
      return fail(PGNN_E_INVALID, msg);
    }
    if (ng > kMaxGt || nd > kMaxDet) {
      snprintf(msg, sizeof msg,
               "%s: frame %lld has %lld ground truths and %lld detections; "
               "the caps are %d and %d per frame",
               who, (long long)f, (long long)ng, (long long)nd, kMaxGt,
               kMaxDet);
      return fail(PGNN_E_UNSUPPORTED, msg);
    }
    sz->n_pairs += ng * nd;
    if (nd > sz->max_det) sz->max_det = (int)nd;
  }
  sz->n_frames = n_frames;
  sz->n_gt = gt_off[n_frames];
  sz->n_det = det_off[n_frames];
  sz->n_pad = next_pow2(sz->n_gt);
  return 0;
}

// the official table, or the caller's 3x3 host doubles after the check that
// every entry is finite and in [0, 1]
int overlap_table(const char *who, const double *min_overlap,
                  OverlapTable *table) {
  static thread_local char msg[160];
  static const double official[9] = {0.7, 0.5, 0.5, 0.7, 0.5,
                                     0.5, 0.7, 0.5, 0.5};
  const double *src = min_overlap ? min_overlap : official;
  for (int k = 0; k < 9; ++k) {
    if (!(src[k] >= 0.0 && src[k] <= 1.0)) {  // false for a NaN as well
      snprintf(msg, sizeof msg,
               "%s: min_overlap[%d][%d] = %g is not in [0, 1]", who, k / 3,
               k % 3, src[k]);
      return fail(PGNN_E_INVALID, msg);
    }
    table->v[k] = src[k];
  }
  return 0;
}

// kMode as kitti_pair_kernel's
template <int kMode>
int upload_and_pairs(const Workspace &w, const Sizes &sz,
                     const int32_t *gt_off, const int32_t *det_off,
                     const double *gt, const int32_t *gt_names,
                     const double *det, double *ov, const double *gt_alpha,
                     const double *det_alpha, double *sim,
                     hipStream_t stream) {
  const size_t off_bytes = ((size_t)sz.n_frames + 1) * sizeof(int32_t);
  PGNN_HIP(hipMemcpyAsync(w.gt_off, gt_off, off_bytes, hipMemcpyHostToDevice,
                          stream));
  PGNN_HIP(hipMemcpyAsync(w.det_off, det_off, off_bytes, hipMemcpyHostToDevice,
                          stream));
  hipLaunchKernelGGL(kitti_scan_kernel, dim3(1), dim3(1024), 0, stream,
                     w.gt_off, w.det_off, sz.n_frames, w.pair_off);
  PGNN_HIP(hipGetLastError());
  if (sz.n_pairs > 0) {
    const unsigned grid = (unsigned)(sz.n_frames < 8192 ? sz.n_frames : 8192);
    hipLaunchKernelGGL(kitti_pair_kernel<kMode>, dim3(grid), dim3(256), 0,
                       stream, w.gt_off, w.det_off, w.pair_off, sz.n_frames, gt,
                       gt_names, det, ov, sz.n_pairs, gt_alpha, det_alpha, sim);
    PGNN_HIP(hipGetLastError());
  }
  return 0;
}

// the outputs of an evaluation; the last four only with orientation
struct EvalOut {
  double *precision, *recall;
  int64_t *counters;
  double *thresholds;
  int32_t *n_thresholds;
  int64_t *n_gt;
  double *ap_r11, *ap_r40, *similarity, *orientation, *aos_r11, *aos_r40;
};

// the launches of one evaluation, after every check
template <bool kAos>
int launch_eval(const Workspace &w, const Sizes &sz, const int32_t *gt_offsets,
                const int32_t *det_offsets, const double *gt_boxes,
                const int32_t *gt_names, const double *det_boxes,
                const int32_t *det_names, const double *gt_alpha,
                const double *det_alpha, const OverlapTable &table,
                const EvalOut &o, hipStream_t stream) {
  const int64_t n_keys = (int64_t)kCombos * sz.n_pad;
  int64_t total = n_keys;
  if (sz.n_gt > total) total = sz.n_gt;
  if (sz.n_det > total) total = sz.n_det;
  if (total < (int64_t)kCombos * kPts * 3) total = (int64_t)kCombos * kPts * 3;
  const int64_t prep_blocks = (total + 255) / 256;
  hipLaunchKernelGGL(kitti_prep_kernel,
                     dim3((unsigned)(prep_blocks < 4096 ? prep_blocks : 4096)),
                     dim3(256), 0, stream, gt_boxes, gt_names, sz.n_gt,
                     det_boxes, det_names, sz.n_det, w.gt_flags, w.det_flags,
                     w.keys, n_keys, o.counters, o.n_gt, w.n_rec, total);
  PGNN_HIP(hipGetLastError());
  if (int rc = upload_and_pairs<kAos ? kPairBoth : kPairOverlaps>(
          w, sz, gt_offsets, det_offsets, gt_boxes, gt_names, det_boxes, w.ov,
          gt_alpha, det_alpha, kAos ? w.ov + kOvSim * sz.n_pairs : nullptr,
          stream))
    return rc;

  // passes 1 and 2: kWaves frames per workgroup, waves stride over the rest
  int words = (sz.max_det + 63) / 64;
  if (words < 1) words = 1;
  const size_t lds = (size_t)kWaves * words * 64 * sizeof(unsigned long long);
  int64_t groups = (sz.n_frames + kWaves - 1) / kWaves;
  if (groups < 1) groups = 1;
  const unsigned grid1 = (unsigned)(groups < 2048 ? groups : 2048);
  const unsigned grid2 = (unsigned)pass2_groups(sz.n_frames);
  hipLaunchKernelGGL(kitti_pass1_kernel, dim3(grid1), dim3(64, kWaves), lds,
                     stream, w.gt_off, w.det_off, w.pair_off, sz.n_frames,
                     w.gt_flags, w.det_flags, det_boxes, w.ov, sz.n_pairs,
                     words, w.keys, sz.n_pad, o.n_gt, w.n_rec, table);
  PGNN_HIP(hipGetLastError());
  hipLaunchKernelGGL(kitti_sort_kernel, dim3(kCombos), dim3(1024), 0, stream,
                     w.keys, sz.n_pad);
  PGNN_HIP(hipGetLastError());
  hipLaunchKernelGGL(kitti_threshold_kernel, dim3(1), dim3(64), 0, stream,
                     w.keys, sz.n_pad, o.n_gt, w.n_rec, o.thresholds,
                     o.n_thresholds);
  PGNN_HIP(hipGetLastError());
  hipLaunchKernelGGL(kitti_pass2_kernel<kAos>, dim3(grid2, kCombos),
                     dim3(64, kWaves), lds, stream, w.gt_off, w.det_off,
                     w.pair_off, sz.n_frames, w.gt_flags, w.det_flags,
                     det_boxes, w.ov, sz.n_pairs, words, o.thresholds,
                     o.n_thresholds, o.counters, table, w.wave_sim);
  PGNN_HIP(hipGetLastError());
  hipLaunchKernelGGL(kitti_finalize_kernel<kAos>, dim3(1),
                     dim3(64, kAos ? 9 : 1), 0, stream, o.counters,
                     o.n_thresholds, o.precision, o.recall, o.ap_r11, o.ap_r40,
                     w.wave_sim, (int64_t)grid2 * kWaves, o.similarity,
                     o.orientation, o.aos_r11, o.aos_r40);
  PGNN_HIP(hipGetLastError());
  return 0;
}

// checks, then launches; `who` names the entry in the messages
int eval_entry(const char *who, const int32_t *gt_offsets,
               const int32_t *det_offsets, int64_t n_frames,
               const double *gt_boxes, const int32_t *gt_names,
               const double *det_boxes, const int32_t *det_names,
               void *workspace, size_t workspace_bytes, const double *gt_alpha,
               const double *det_alpha, const double *min_overlap,
               const EvalOut &o, hipStream_t stream) {
  static thread_local char msg[160];
  Sizes sz;
  if (int rc = check_offsets(who, gt_offsets, det_offsets, n_frames, &sz))
    return rc;
  const bool aos = gt_alpha && det_alpha;
  snprintf(msg, sizeof msg, "%s: null box or name pointer", who);
  PGNN_REQUIRE((sz.n_gt == 0 || (gt_boxes && gt_names)) &&
                   (sz.n_det == 0 || (det_boxes && det_names)),
               PGNN_E_INVALID, msg);
  snprintf(msg, sizeof msg, "%s: null workspace or output pointer", who);
  PGNN_REQUIRE(workspace && o.precision && o.recall && o.counters &&
                   o.thresholds && o.n_thresholds && o.n_gt && o.ap_r11 &&
                   o.ap_r40,
               PGNN_E_INVALID, msg);
  snprintf(msg, sizeof msg,
           "%s: gt_alpha and det_alpha must both be given or both be null",
           who);
  PGNN_REQUIRE((gt_alpha != nullptr) == (det_alpha != nullptr), PGNN_E_INVALID,
               msg);
  snprintf(msg, sizeof msg, "%s: null orientation output pointer", who);
  PGNN_REQUIRE(!aos || (o.similarity && o.orientation && o.aos_r11 && o.aos_r40),
               PGNN_E_INVALID, msg);
  OverlapTable table;
  if (int rc = overlap_table(who, min_overlap, &table)) return rc;
  const Workspace w = carve(workspace, workspace_bytes, sz.n_frames, sz.n_gt,
                            sz.n_det, sz.n_pairs, true, aos);
  snprintf(msg, sizeof msg, "%s: workspace too small", who);
  PGNN_REQUIRE(w.bytes <= workspace_bytes, PGNN_E_WORKSPACE, msg);
  return aos ? launch_eval<true>(w, sz, gt_offsets, det_offsets, gt_boxes,
                                 gt_names, det_boxes, det_names, gt_alpha,
                                 det_alpha, table, o, stream)
             : launch_eval<false>(w, sz, gt_offsets, det_offsets, gt_boxes,
                                  gt_names, det_boxes, det_names, nullptr,
                                  nullptr, table, o, stream);
}

bool sizes_in_range(int64_t n_frames, int64_t n_gt, int64_t n_det,
                    int64_t n_pairs) {
  return !(n_frames < 0 || n_frames > PGNN_KITTI_MAX_FRAMES || n_gt < 0 ||
           n_det < 0 || n_pairs < 0 || n_gt > INT32_MAX || n_det > INT32_MAX ||
           n_pairs > n_gt * n_det);
}

// ---- per-box outcomes of one combination at one threshold ----
//
// One wave per frame, the lanes over the frame's boxes: lane l owns the
// detections j = l, l + 64, ... and the ground truths i = l, l + 64, ...
// Everything a box's later steps need to know about it (is this detection
// taken, which ground truth took it, which detection did this ground truth
// take) is written and read by its owning lane only: the taken set is 16 bits
// of a register, the partners live in the output arrays themselves.
//
//   matching   serial over the ground truths of ig >= 0, as match_frame<true>
//              walks them.  The serial inner loop's choice is the valid
//              (idj == 0) candidate of the largest overlap, the smallest index
//              on ties, else the first idj == 1 candidate: each lane finds
//              that among its own detections, six xor-shuffles find it for the
//              wave.
//   detections lane = detection.  A left-over one walks its column of the
//              frame's pair block once (the lanes read neighbouring doubles):
//              the first absorbing DontCare row, b and x.
//   truths     lane = ground truth.  An unmatched one walks its row once.
//   totals     an LDS histogram per workgroup, one int64 atomic per code.
constexpr int kDetCodes = PGNN_KITTI_DET_CODES;
constexpr int kMatchTotals = PGNN_KITTI_MATCH_TOTALS;
static_assert(kMaxDet <= 64 * 32, "the taken set is one 32-bit register");

struct MatchOut {
  int32_t *gt_outcome, *gt_partner, *det_outcome, *det_partner;
  double *det_overlap;
  int64_t *totals;
};

__global__ __launch_bounds__(64 * kWaves) void kitti_match_kernel(
    const int32_t *__restrict__ gt_off, const int32_t *__restrict__ det_off,
    const int64_t *__restrict__ pair_off, int64_t n_frames,
    const int32_t *__restrict__ gt_flags, const int32_t *__restrict__ det_flags,
    const double *__restrict__ det, const double *__restrict__ ov_metric,
    const double *__restrict__ ov_dontcare, int s, double min_ov, double thresh,
    double loc_floor, bool is_2d, const MatchOut out) {
  __shared__ unsigned hist[kMatchTotals];
  const int lane = threadIdx.x;
  const int tid = threadIdx.y * 64 + lane;
  if (tid < kMatchTotals) hist[tid] = 0u;
  __syncthreads();
  for (int64_t f = (int64_t)blockIdx.x * kWaves + threadIdx.y; f < n_frames;
       f += (int64_t)gridDim.x * kWaves) {
    const int g0 = gt_off[f], ng = gt_off[f + 1] - g0;
    const int d0 = det_off[f], nd = det_off[f + 1] - d0;
    const int32_t *gfl = gt_flags + g0, *dfl = det_flags + d0;
    const double *drow = det + (int64_t)d0 * kRow;
    const double *fo = ov_metric + pair_off[f];
    const double *fdc = ov_dontcare + pair_off[f];
    int32_t *gp = out.gt_partner + g0, *dp = out.det_partner + d0;

    // this lane's detections: bit k speaks of detection k * 64 + lane
    unsigned open = 0u;   // idj >= 0 and score >= thresh: may be assigned
    unsigned valid = 0u;  // idj == 0
    unsigned taken = 0u;
    for (int j = lane, k = 0; j < nd; j += 64, ++k) {
      const int idj = flag_of(dfl[j], s);
      if (idj >= 0 && !(drow[(int64_t)j * kRow + SCORE] < thresh))
        open |= 1u << k;
      if (idj == 0) valid |= 1u << k;
      dp[j] = -1;
    }
    for (int i = lane; i < ng; i += 64) gp[i] = -1;

    // §9.5 "Matching", compute_fp
    for (int i = 0; i < ng; ++i) {
      if (flag_of(gfl[i], s) < 0) continue;  // the same in every lane
      const double *row = fo + (int64_t)i * nd;
      double best = 0.0;  // a candidate's overlap is > min_ov >= 0
      int best_j = INT32_MAX, small_j = INT32_MAX;
      for (int j = lane, k = 0; j < nd; j += 64, ++k) {
        if (!(((open & ~taken) >> k) & 1u)) continue;
        const double o = row[j];
        if (!(o > min_ov)) continue;
        if ((valid >> k) & 1u) {
          if (o > best) {
            best = o;
            best_j = j;
          }
        } else if (j < small_j) {
          small_j = j;
        }
      }
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        const double o2 = __shfl_xor(best, m);
        const int j2 = __shfl_xor(best_j, m);
        const int s2 = __shfl_xor(small_j, m);
        if (o2 > best || (o2 == best && j2 < best_j)) {
          best = o2;
          best_j = j2;
        }
        small_j = s2 < small_j ? s2 : small_j;
      }
      const int det_idx = best_j != INT32_MAX ? best_j : small_j;
      if (det_idx == INT32_MAX) continue;
      if ((det_idx & 63) == lane) {
        taken |= 1u << (det_idx >> 6);
        dp[det_idx] = i;
      }
      if ((i & 63) == lane) gp[i] = det_idx;
    }

    // detections
    for (int j = lane, k = 0; j < nd; j += 64, ++k) {
      const int idj = flag_of(dfl[j], s);
      int code, partner = -1;
      double with = 0.0;
      if (idj < 0) {
        code = PGNN_KITTI_DET_OTHER;
      } else if (!((open >> k) & 1u)) {
        code = PGNN_KITTI_DET_BELOW;
      } else if ((taken >> k) & 1u) {
        partner = dp[j];
        code = (flag_of(gfl[partner], s) == 0 && idj == 0)
                   ? PGNN_KITTI_DET_TP
                   : PGNN_KITTI_DET_MATCHED_IGNORED;
        with = fo[(int64_t)partner * nd + j];
      } else if (idj == 1) {
        code = PGNN_KITTI_DET_IGNORED_SMALL;
      } else {
        // b: over the ground truths of ig >= 0; x: over those of ig == -1
        // that are no DontCare; an overlap of 0 names no ground truth
        double b = 0.0, x = 0.0;
        int b_i = -1, x_i = -1, dc_i = -1;
        for (int i = 0; i < ng; ++i) {
          const int32_t w = gfl[i];
          const double o = fo[(int64_t)i * nd + j];
          if (flag_of(w, s) >= 0) {
            if (o > b) {
              b = o;
              b_i = i;
            }
          } else if (w & kDontCareBit) {
            if (is_2d && dc_i < 0 && fdc[(int64_t)i * nd + j] > min_ov)
              dc_i = i;
          } else if (o > x) {
            x = o;
            x_i = i;
          }
        }
        if (dc_i >= 0) {
          code = PGNN_KITTI_DET_DONTCARE;
          partner = dc_i;
          with = fdc[(int64_t)dc_i * nd + j];
        } else if (b > min_ov) {
          code = PGNN_KITTI_DET_FP_DUPLICATE;
          partner = b_i;
          with = b;
        } else if (x >= loc_floor && x > b) {
          code = PGNN_KITTI_DET_FP_CONFUSION;
          partner = x_i;
          with = x;
        } else if (b >= loc_floor) {
          code = PGNN_KITTI_DET_FP_LOCALISATION;
          partner = b_i;
          with = b;
        } else {
          code = PGNN_KITTI_DET_FP_BACKGROUND;
        }
      }
      out.det_outcome[d0 + j] = code;
      dp[j] = partner;
      out.det_overlap[d0 + j] = with;
      atomicAdd(&hist[code], 1u);
    }

    // ground truths
    for (int i = lane; i < ng; i += 64) {
      const int ig = flag_of(gfl[i], s);
      int code, partner = gp[i];
      if (ig < 0) {
        code = PGNN_KITTI_GT_OTHER;
      } else if (ig == 1) {
        code = partner >= 0 ? PGNN_KITTI_GT_IGNORED_MATCHED
                            : PGNN_KITTI_GT_IGNORED;
      } else if (partner >= 0) {
        code = flag_of(dfl[partner], s) == 0 ? PGNN_KITTI_GT_TP
                                             : PGNN_KITTI_GT_MATCHED_SMALL;
      } else {
        const double *row = fo + (int64_t)i * nd;
        double low = 0.0, loc = 0.0;
        int low_j = -1, loc_j = -1;
        for (int j = 0; j < nd; ++j) {
          const int idj = flag_of(dfl[j], s);
          if (idj < 0) continue;
          const double o = row[j];
          if (drow[(int64_t)j * kRow + SCORE] < thresh) {
            if (o > min_ov && o > low) {
              low = o;
              low_j = j;
            }
          } else if (idj == 0 && o >= loc_floor && o <= min_ov &&
                     (loc_j < 0 || o > loc)) {
            loc = o;
            loc_j = j;
          }
        }
        if (low_j >= 0) {
          code = PGNN_KITTI_GT_FN_LOW_SCORE;
          partner = low_j;
        } else if (loc_j >= 0) {
          code = PGNN_KITTI_GT_FN_LOCALISATION;
          partner = loc_j;
        } else {
          code = PGNN_KITTI_GT_FN_MISSED;
        }
      }
      out.gt_outcome[g0 + i] = code;
      gp[i] = partner;
      atomicAdd(&hist[kDetCodes + code], 1u);
    }
  }
  __syncthreads();  // every thread arrives: no return above
  if (tid < kMatchTotals && hist[tid])
    atomicAdd((unsigned long long *)out.totals + tid,
              (unsigned long long)hist[tid]);
}

// the workspace of pgnn_kitti_match: the offsets, flags and four pair planes
// of an evaluation, and the words kitti_prep_kernel clears beside the flags
struct MatchWorkspace {
  Workspace w;
  int64_t *counters, *n_gt;
};

MatchWorkspace carve_match(void *base, size_t size, int64_t n_frames,
                           int64_t n_gt, int64_t n_det, int64_t n_pairs) {
  Arena arena(base, base ? size : 0);
  MatchWorkspace m;
  Workspace &w = m.w;
  w.gt_off = arena.take<int32_t>((size_t)n_frames + 1);
  w.det_off = arena.take<int32_t>((size_t)n_frames + 1);
  w.pair_off = arena.take<int64_t>((size_t)n_frames + 1);
  w.gt_flags = arena.take<int32_t>((size_t)(n_gt > 0 ? n_gt : 1));
  w.det_flags = arena.take<int32_t>((size_t)(n_det > 0 ? n_det : 1));
  w.n_rec = arena.take<int32_t>(kCombos);
  w.ov = arena.take<double>((size_t)(n_pairs > 0 ? n_pairs : 1) * 4);
  w.wave_sim = nullptr;
  w.keys = nullptr;
  m.counters = arena.take<int64_t>((size_t)kCombos * kPts * 3);
  m.n_gt = arena.take<int64_t>(kCombos);
  w.bytes = align_up(arena.used, 256);
  return m;
}

int match_entry(const int32_t *gt_offsets, const int32_t *det_offsets,
                int64_t n_frames, const double *gt_boxes,
                const int32_t *gt_names, const double *det_boxes,
                const int32_t *det_names, const double *min_overlap_host,
                int32_t metric, int32_t cls, int32_t difficulty,
                double score_threshold, double loc_floor, void *workspace,
                size_t workspace_bytes, const MatchOut &o, hipStream_t stream) {
  const char *who = "kitti_match";
  Sizes sz;
  if (int rc = check_offsets(who, gt_offsets, det_offsets, n_frames, &sz))
    return rc;
  PGNN_REQUIRE((sz.n_gt == 0 || (gt_boxes && gt_names)) &&
                   (sz.n_det == 0 || (det_boxes && det_names)),
               PGNN_E_INVALID, "kitti_match: null box or name pointer");
  PGNN_REQUIRE(workspace && o.totals &&
                   (sz.n_gt == 0 || (o.gt_outcome && o.gt_partner)) &&
                   (sz.n_det == 0 ||
                    (o.det_outcome && o.det_partner && o.det_overlap)),
               PGNN_E_INVALID, "kitti_match: null workspace or output pointer");
  PGNN_REQUIRE(metric >= 0 && metric < 3 && cls >= 0 && cls < 3 &&
                   difficulty >= 0 && difficulty < 3,
               PGNN_E_INVALID,
               "kitti_match: metric, cls and difficulty are 0, 1 or 2");
  PGNN_REQUIRE(score_threshold - score_threshold == 0.0,  // no NaN, no inf
               PGNN_E_INVALID,
               "kitti_match: score_threshold is not finite");
  PGNN_REQUIRE(loc_floor >= 0.0 && loc_floor <= 1.0,  // false for a NaN
               PGNN_E_INVALID, "kitti_match: loc_floor is not in [0, 1]");
  OverlapTable table;
  if (int rc = overlap_table(who, min_overlap_host, &table)) return rc;
  const MatchWorkspace m = carve_match(workspace, workspace_bytes, sz.n_frames,
                                       sz.n_gt, sz.n_det, sz.n_pairs);
  const Workspace &w = m.w;
  PGNN_REQUIRE(w.bytes <= workspace_bytes, PGNN_E_WORKSPACE,
               "kitti_match: workspace too small");

  // the evaluation's own prep and pair launches: the same flags and overlaps
  int64_t total = (int64_t)kCombos * kPts * 3;
  if (sz.n_gt > total) total = sz.n_gt;
  if (sz.n_det > total) total = sz.n_det;
  const int64_t prep_blocks = (total + 255) / 256;
  hipLaunchKernelGGL(kitti_prep_kernel,
                     dim3((unsigned)(prep_blocks < 4096 ? prep_blocks : 4096)),
                     dim3(256), 0, stream, gt_boxes, gt_names, sz.n_gt,
                     det_boxes, det_names, sz.n_det, w.gt_flags, w.det_flags,
                     (unsigned long long *)nullptr, (int64_t)0, m.counters,
                     m.n_gt, w.n_rec, total);
  PGNN_HIP(hipGetLastError());
  PGNN_HIP(hipMemsetAsync(o.totals, 0, kMatchTotals * sizeof(int64_t), stream));
  if (int rc = upload_and_pairs<kPairOverlaps>(
          w, sz, gt_offsets, det_offsets, gt_boxes, gt_names, det_boxes, w.ov,
          nullptr, nullptr, nullptr, stream))
    return rc;
  int64_t groups = (sz.n_frames + kWaves - 1) / kWaves;
  if (groups < 1) groups = 1;
  hipLaunchKernelGGL(kitti_match_kernel,
                     dim3((unsigned)(groups < 2048 ? groups : 2048)),
                     dim3(64, kWaves), 0, stream, w.gt_off, w.det_off,
                     w.pair_off, sz.n_frames, w.gt_flags, w.det_flags,
                     det_boxes, w.ov + metric * sz.n_pairs,
                     w.ov + kOvDontCare * sz.n_pairs, cls * 3 + difficulty,
                     table.v[metric * 3 + cls], score_threshold, loc_floor,
                     metric == 0, o);
  PGNN_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace pgnn

extern "C" size_t pgnn_kitti_eval_workspace_bytes(int64_t n_frames,
                                                  int64_t n_gt, int64_t n_det,
                                                  int64_t n_pairs) {
  if (!pgnn::sizes_in_range(n_frames, n_gt, n_det, n_pairs)) return 0;
  return pgnn::carve(nullptr, 0, n_frames, n_gt, n_det, n_pairs, true).bytes;
}

extern "C" size_t pgnn_kitti_eval_ex_workspace_bytes(int64_t n_frames,
                                                     int64_t n_gt,
                                                     int64_t n_det,
                                                     int64_t n_pairs,
                                                     int32_t with_aos) {
  if (!pgnn::sizes_in_range(n_frames, n_gt, n_det, n_pairs)) return 0;
  return pgnn::carve(nullptr, 0, n_frames, n_gt, n_det, n_pairs, true,
                     with_aos != 0)
      .bytes;
}

extern "C" int pgnn_kitti_pair_overlaps(
    const int32_t *gt_offsets, const int32_t *det_offsets, int64_t n_frames,
    const double *gt_boxes, const int32_t *gt_names, const double *det_boxes,
    void *workspace, size_t workspace_bytes, double *overlaps, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  pgnn::Sizes sz;
  if (int rc = pgnn::check_offsets("kitti_pair_overlaps", gt_offsets,
                                   det_offsets, n_frames, &sz))
    return rc;
  PGNN_REQUIRE((sz.n_gt == 0 || (gt_boxes && gt_names)) &&
                   (sz.n_det == 0 || det_boxes) &&
                   (sz.n_pairs == 0 || overlaps) && workspace,
               PGNN_E_INVALID, "kitti_pair_overlaps: null pointer");
  const pgnn::Workspace w =
      pgnn::carve(workspace, workspace_bytes, sz.n_frames, sz.n_gt, sz.n_det,
                  sz.n_pairs, false);
  PGNN_REQUIRE(w.bytes <= workspace_bytes, PGNN_E_WORKSPACE,
               "kitti_pair_overlaps: workspace too small");
  return pgnn::upload_and_pairs<pgnn::kPairOverlaps>(
      w, sz, gt_offsets, det_offsets, gt_boxes, gt_names, det_boxes, overlaps,
      nullptr, nullptr, nullptr, stream);
  PGNN_GUARD_END
}

extern "C" int pgnn_kitti_pair_orientation(
    const int32_t *gt_offsets, const int32_t *det_offsets, int64_t n_frames,
    const double *gt_boxes, const double *det_boxes, const double *gt_alpha,
    const double *det_alpha, void *workspace, size_t workspace_bytes,
    double *sim, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  pgnn::Sizes sz;
  if (int rc = pgnn::check_offsets("kitti_pair_orientation", gt_offsets,
                                   det_offsets, n_frames, &sz))
    return rc;
  PGNN_REQUIRE((sz.n_gt == 0 || (gt_boxes && gt_alpha)) &&
                   (sz.n_det == 0 || (det_boxes && det_alpha)) &&
                   (sz.n_pairs == 0 || sim) && workspace,
               PGNN_E_INVALID, "kitti_pair_orientation: null pointer");
  const pgnn::Workspace w =
      pgnn::carve(workspace, workspace_bytes, sz.n_frames, sz.n_gt, sz.n_det,
                  sz.n_pairs, false);
  PGNN_REQUIRE(w.bytes <= workspace_bytes, PGNN_E_WORKSPACE,
               "kitti_pair_orientation: workspace too small");
  return pgnn::upload_and_pairs<pgnn::kPairSim>(
      w, sz, gt_offsets, det_offsets, gt_boxes, nullptr, det_boxes, nullptr,
      gt_alpha, det_alpha, sim, stream);
  PGNN_GUARD_END
}

extern "C" int pgnn_kitti_eval(
    const int32_t *gt_offsets, const int32_t *det_offsets, int64_t n_frames,
    const double *gt_boxes, const int32_t *gt_names, const double *det_boxes,
    const int32_t *det_names, void *workspace, size_t workspace_bytes,
    double *precision, double *recall, int64_t *counters, double *thresholds,
    int32_t *n_thresholds, int64_t *n_gt, double *ap_r11, double *ap_r40,
    void *stream_) {
  PGNN_GUARD_BEGIN
  const pgnn::EvalOut out = {precision, recall,  counters, thresholds,
                             n_thresholds, n_gt, ap_r11,   ap_r40,
                             nullptr,   nullptr, nullptr,  nullptr};
  return pgnn::eval_entry("kitti_eval", gt_offsets, det_offsets, n_frames,
                          gt_boxes, gt_names, det_boxes, det_names, workspace,
                          workspace_bytes, nullptr, nullptr, nullptr, out,
                          (hipStream_t)stream_);
  PGNN_GUARD_END
}

extern "C" int pgnn_kitti_eval_ex(
    const int32_t *gt_offsets, const int32_t *det_offsets, int64_t n_frames,
    const double *gt_boxes, const int32_t *gt_names, const double *det_boxes,
    const int32_t *det_names, void *workspace, size_t workspace_bytes,
    double *precision, double *recall, int64_t *counters, double *thresholds,
    int32_t *n_thresholds, int64_t *n_gt, double *ap_r11, double *ap_r40,
    const double *gt_alpha, const double *det_alpha, const double *min_overlap,
    double *similarity, double *orientation, double *aos_r11, double *aos_r40,
    void *stream_) {
  PGNN_GUARD_BEGIN
  const pgnn::EvalOut out = {precision,  recall,      counters, thresholds,
                             n_thresholds, n_gt,      ap_r11,   ap_r40,
                             similarity, orientation, aos_r11,  aos_r40};
  return pgnn::eval_entry("kitti_eval_ex", gt_offsets, det_offsets, n_frames,
                          gt_boxes, gt_names, det_boxes, det_names, workspace,
                          workspace_bytes, gt_alpha, det_alpha, min_overlap,
                          out, (hipStream_t)stream_);
  PGNN_GUARD_END
}

extern "C" size_t pgnn_kitti_match_workspace_bytes(int64_t n_frames,
                                                   int64_t n_gt, int64_t n_det,
                                                   int64_t n_pairs) {
  if (!pgnn::sizes_in_range(n_frames, n_gt, n_det, n_pairs)) return 0;
  return pgnn::carve_match(nullptr, 0, n_frames, n_gt, n_det, n_pairs).w.bytes;
}

extern "C" int pgnn_kitti_match(
    const int32_t *gt_offsets, const int32_t *det_offsets, int64_t n_frames,
    const double *gt_boxes, const int32_t *gt_names, const double *det_boxes,
    const int32_t *det_names, const double *min_overlap, int32_t metric,
    int32_t cls, int32_t difficulty, double score_threshold, double loc_floor,
    void *workspace, size_t workspace_bytes, int32_t *gt_outcome,
    int32_t *gt_partner, int32_t *det_outcome, int32_t *det_partner,
    double *det_overlap, int64_t *totals, void *stream_) {
  PGNN_GUARD_BEGIN
  const pgnn::MatchOut out = {gt_outcome,  gt_partner,  det_outcome,
                              det_partner, det_overlap, totals};
  return pgnn::match_entry(gt_offsets, det_offsets, n_frames, gt_boxes,
                           gt_names, det_boxes, det_names, min_overlap, metric,
                           cls, difficulty, score_threshold, loc_floor,
                           workspace, workspace_bytes, out,
                           (hipStream_t)stream_);
  PGNN_GUARD_END
}
