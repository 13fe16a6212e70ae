// Per-point arithmetic of the KITTI frame ingest, shared by the float32 crop
// (ingest.hip) and the voxel-averaged float64 crop (voxel_avg.hip).
#pragma once
#include "pgnn_common.h"

namespace pgnn {

struct IngestArgs {
  const float *velo;  // [n,4] x y z reflectance
  int64_t n;
  float r[9];         // velo_to_cam[:3,:3] as float32, row-major
  float t[3];         // velo_to_cam[:3,3] as float32
  double p[9];        // cam_to_image[:, :3] (float64 holding P2's float32)
  double width, height;
  const uint8_t *image;  // optional [H,W,3] BGR (cv2.imread layout)
  int64_t img_h, img_w;
};

// host: the calibration blocks of the C ABI (host pointers) into the launch
inline void fill_calib(IngestArgs *a, const float *velo_to_cam_3x4,
                       const double *cam_to_image_3x3) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      a->r[3 * r + c] = velo_to_cam_3x4[4 * r + c];
      a->p[3 * r + c] = cam_to_image_3x3[3 * r + c];
    }
    a->t[r] = velo_to_cam_3x4[4 * r + 3];
  }
}

// kitti_dataset.py:1002-1005: float32 matmul + float32 add.  The products are
// accumulated in k order with fused multiply-adds, which is what the sgemm
// micro-kernels NumPy dispatches to do; the parity test states the (<= 1 ulp)
// bound for BLAS builds that associate differently.
__device__ __forceinline__ void velo_to_cam_f32(const IngestArgs &a,
                                                const float4 q, float *x,
                                                float *y, float *z) {
  *x = __fmaf_rn(q.z, a.r[2], __fmaf_rn(q.y, a.r[1], q.x * a.r[0])) + a.t[0];
  *y = __fmaf_rn(q.z, a.r[5], __fmaf_rn(q.y, a.r[4], q.x * a.r[3])) + a.t[1];
  *z = __fmaf_rn(q.z, a.r[8], __fmaf_rn(q.y, a.r[7], q.x * a.r[6])) + a.t[2];
}

// :678-684 projection in float64 and the strict image test
__device__ __forceinline__ bool project_in_image(const IngestArgs &a, double X,
                                                 double Y, double Z, double *u,
                                                 double *v) {
  const double iu = (X * a.p[0] + Y * a.p[1]) + Z * a.p[2];
  const double iv = (X * a.p[3] + Y * a.p[4]) + Z * a.p[5];
  const double iw = (X * a.p[6] + Y * a.p[7]) + Z * a.p[8];
  *u = iu / iw;
  *v = iv / iw;
  return *u > 0.0 && *u < a.width && *v > 0.0 && *v < a.height;
}

// :994-995 image[int32(v), int32(u), ::-1] / 255 (BGR -> RGB)
__device__ __forceinline__ void sample_rgb(const IngestArgs &a, double u,
                                           double v, float *r, float *g,
                                           float *b) {
  const int64_t px = (int64_t)(int)u, py = (int64_t)(int)v;
  *r = 0.0f, *g = 0.0f, *b = 0.0f;
  if (a.image && px >= 0 && px < a.img_w && py >= 0 && py < a.img_h) {
    const uint8_t *c = a.image + (py * a.img_w + px) * 3;
    *b = (float)c[0] / 255.0f;
    *g = (float)c[1] / 255.0f;
    *r = (float)c[2] / 255.0f;
  }
}

}  // namespace pgnn
