// overlapped_boxes_3d_fast_poly (models/nms.py:64-88) for one pair of boxes
// whose corner geometry is already built: shared by the NMS kernels
// (detect.hip) and the crop_aug placement kernel (crop_aug.hip), which build
// their Geom records differently (float32 boxes there, integer corner grids
// here) and must agree on everything after that.
#pragma once
#include "pgnn_common.h"

namespace pgnn {
namespace {

struct Geom {
  double px[4], pz[4];  // BEV polygon (corners 0-3, x and z)
  double lo[3], hi[3];  // axis-aligned bounds over the 8 corners
  double area;          // |polygon area|
};

// Area of (quadrilateral a) ∩ (convex quadrilateral b): Sutherland-Hodgman
// clipping of a against the four half-planes of b, shoelace on the result.
// Stands in for shapely's `p1.intersection(p2).area` (nms.py:82).
// Every array index below is a compile-time constant after unrolling (vertex
// pushes are select chains), so the polygon lives in VGPRs: the first version
// indexed dynamically, went through scratch memory and spent ~13 us per call
// in the latency-bound scan kernel.
constexpr int kMaxVerts = 8;  // a quad gains at most one vertex per clip

__device__ __forceinline__ void push_vertex(double (&tx)[kMaxVerts],
                                            double (&tz)[kMaxVerts], int &m,
                                            double x, double z) {
#pragma unroll
  for (int k = 0; k < kMaxVerts; ++k) {
    tx[k] = (m == k) ? x : tx[k];
    tz[k] = (m == k) ? z : tz[k];
  }
  ++m;
}

__device__ double clip_area(const Geom &a, const Geom &b) {
  double sx[kMaxVerts], sz[kMaxVerts];
#pragma unroll
  for (int i = 0; i < kMaxVerts; ++i) {
    sx[i] = a.px[i & 3];
    sz[i] = a.pz[i & 3];
  }
  int n = 4;
  double orient = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3;
    orient += b.px[i] * b.pz[j] - b.px[j] * b.pz[i];
  }
  if (orient == 0.0) return 0.0;
  const double sgn = orient > 0.0 ? 1.0 : -1.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double ex = b.px[e], ez = b.pz[e];
    const double dx = b.px[(e + 1) & 3] - ex, dz = b.pz[(e + 1) & 3] - ez;
    double d[kMaxVerts];
#pragma unroll
    for (int i = 0; i < kMaxVerts; ++i)
      d[i] = sgn * (dx * (sz[i] - ez) - dz * (sx[i] - ex));
    double tx[kMaxVerts], tz[kMaxVerts];
#pragma unroll
    for (int i = 0; i < kMaxVerts; ++i) tx[i] = tz[i] = 0.0;
    int m = 0;
#pragma unroll
    for (int i = 0; i < kMaxVerts; ++i) {
      if (i < n) {
        const bool last = i + 1 == n;
        const int jn = (i + 1) & (kMaxVerts - 1);
        const double jx = last ? sx[0] : sx[jn];
        const double jz = last ? sz[0] : sz[jn];
        const double dj = last ? d[0] : d[jn];
        const double di = d[i];
        if (di >= 0.0) push_vertex(tx, tz, m, sx[i], sz[i]);
        if ((di >= 0.0) != (dj >= 0.0)) {
          const double t = di / (di - dj);
          push_vertex(tx, tz, m, sx[i] + t * (jx - sx[i]),
                      sz[i] + t * (jz - sz[i]));
        }
      }
    }
    n = m < kMaxVerts ? m : kMaxVerts;
#pragma unroll
    for (int i = 0; i < kMaxVerts; ++i) {
      sx[i] = tx[i];
      sz[i] = tz[i];
    }
  }
  if (n < 3) return 0.0;
  double a2 = 0.0;
#pragma unroll
  for (int i = 0; i < kMaxVerts; ++i) {
    if (i < n) {
      const bool last = i + 1 == n;
      const int jn = (i + 1) & (kMaxVerts - 1);
      const double jx = last ? sx[0] : sx[jn];
      const double jz = last ? sz[0] : sz[jn];
      a2 += sx[i] * jz - jx * sz[i];
    }
  }
  return fabs(a2) * 0.5;
}

// overlapped_boxes_3d_fast_poly for one pair (nms.py:64-88): `single` is the
// reference's single_box, `other` one entry of box_list.
__device__ double overlap_3d(const Geom &single, const Geom &other) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (single.hi[k] < other.lo[k] || single.lo[k] > other.hi[k]) return 0.0;
  const double shared_area = clip_area(single, other);
  const double shared_y =
      fmin(other.hi[1], single.hi[1]) - fmax(other.lo[1], single.lo[1]);
  const double inter = shared_y * shared_area;
  const double uni = (other.hi[1] - other.lo[1]) * other.area +
                     (single.hi[1] - single.lo[1]) * single.area;
  return (double)(float)inter / (uni - inter);
}

}  // namespace
}  // namespace pgnn
