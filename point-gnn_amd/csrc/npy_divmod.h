// NumPy's floating-point floor_divide, shared by the keypoint grid (graph.hip)
// and the voxel-average down-sampling (voxel_avg.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace pgnn {

// NumPy's floor_divide for floating point (npy_divmod in
// numpy/core/src/npymath/npy_math_internal.h.src), divisor > 0: the exact
// floor of a / b for the given operands -- fmod is exact, so unlike
// floor(a / b) the result never jumps a cell when the rounded quotient lands
// on an integer.
__device__ __forceinline__ float npy_floor_divide_f32(float a, float b) {
  float mod = fmodf(a, b);
  float div = (a - mod) / b;
  if (mod != 0.0f && mod < 0.0f) div -= 1.0f;  // sign of b (> 0) != sign of mod
  if (div == 0.0f) return 0.0f;
  float fl = floorf(div);
  if (div - fl > 0.5f) fl += 1.0f;
  return fl;
}
__device__ __forceinline__ double npy_floor_divide_f64(double a, double b) {
  double mod = fmod(a, b);
  double div = (a - mod) / b;
  if (mod != 0.0 && mod < 0.0) div -= 1.0;
  if (div == 0.0) return 0.0;
  double fl = floor(div);
  if (div - fl > 0.5) fl += 1.0;
  return fl;
}

}  // namespace pgnn
