// Headless rasteriser: points and line segments of a frame drawn into a uint8
// RGB image on the device (include/pointgnn_hip.h, "rendering").  Every step
// is an IEEE float64 + - * /, a floor or integer arithmetic, so the NumPy
// restatement in tests/_render.py equals the image with ==.
//
// One uint64 key per pixel, updated with a 64-bit atomic max; the larger key
// wins, so the result does not depend on the order the lanes arrive in:
//   0                                        nothing drawn
//   bit 62 | ~ord(float32 depth) << 30 | ~i  point i   (smaller depth, then the
//                                            smaller index, is the larger key)
//   bit 63 | s                               segment s (the larger index wins;
//                                            any segment beats any point)
// pgnn_render_resolve turns keys into colours.
//
// Text (pgnn_render_text, "text" below) is a pass of its own over a finished
// image, with a uint32 key plane and the 5 x 7 font of font5x7.h.
#include <math.h>

#include "font5x7.h"
#include "pgnn_common.h"

namespace {

using pgnn::fail;

constexpr int kBlock = 256;
constexpr unsigned kMaxGrid = 4096;           // every kernel strides over its work
constexpr unsigned long long kSegLayer = 1ull << 63;
constexpr unsigned long long kPointLayer = 1ull << 62;
constexpr int kIndexBits = 30;                // points per call < 2^30
constexpr unsigned long long kIndexMask = (1ull << kIndexBits) - 1;
constexpr double kCoordLimit = 1073741824.0;  // 2^30: a segment end at or beyond it drops
constexpr int kShort = 16;  // pixels a lane draws by itself; longer: the wave

struct View {
  double m[12];  // rows hu, hv, hw
  double d[4];   // depth row
  double near;
  int32_t w, h;
};

__device__ __forceinline__ double affine(const double *r, double x, double y,
                                         double z) {
  return ((r[0] * x + r[1] * y) + r[2] * z) + r[3];
}

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < INFINITY; }

__device__ __forceinline__ void put_key(unsigned long long *keys, int64_t pix,
                                        unsigned long long key) {
  // keys only grow: a pixel that already holds a larger one needs no atomic
  unsigned long long cur = __hip_atomic_load(keys + pix, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
  if (cur >= key) return;
  __hip_atomic_fetch_max(keys + pix, key, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void render_clear_kernel(unsigned long long *keys, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = 0;
}

template <typename T>
__global__ void render_points_kernel(const T *__restrict__ xyz, int64_t n,
                                     View v, int p, unsigned long long *keys) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1],
           z = (double)xyz[3 * i + 2];
    double hu = affine(v.m, x, y, z), hv = affine(v.m + 4, x, y, z),
           hw = affine(v.m + 8, x, y, z), dep = affine(v.d, x, y, z);
    if (!(finite64(hu) && finite64(hv) && finite64(hw) && finite64(dep)))
      continue;
    if (!(hw >= v.near)) continue;
    double u = floor(hu / hw), w = floor(hv / hw);
    if (!(u >= 0.0 && u < (double)v.w && w >= 0.0 && w < (double)v.h)) continue;
    int px = (int)u, py = (int)w;
    float df = (float)dep;
    if (df == 0.0f) df = 0.0f;  // -0 and +0 are one depth
    uint32_t bits = __float_as_uint(df);
    uint32_t ord = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    unsigned long long key = kPointLayer |
                             ((unsigned long long)(uint32_t)~ord << kIndexBits) |
                             (kIndexMask - (unsigned long long)i);
    int x1 = min(px + p, v.w), y1 = min(py + p, v.h);
    for (int yy = py; yy < y1; ++yy)
      for (int xx = px; xx < x1; ++xx)
        put_key(keys, (int64_t)yy * v.w + xx, key);
  }
}

// One segment after projection, clipping and the cut to the canvas: pixels
// k0..k1 of (a0 + k s, b0 + floordiv(2 k db + n, 2 n)), a the major axis.
struct SegPlan {
  int64_t a0, b0, db, n, k0, k1;
  int32_t s, swap, t, pad;
};

__device__ __forceinline__ int64_t floordiv64(int64_t num, int64_t den) {
  int64_t q = num / den;  // den > 0
  if (num % den != 0 && num < 0) --q;
  return q;
}

template <typename T>
__device__ bool plan_segment(const T *__restrict__ s, const View &v, int t,
                             SegPlan &pl) {
  double ax = (double)s[0], ay = (double)s[1], az = (double)s[2];
  double bx = (double)s[3], by = (double)s[4], bz = (double)s[5];
  double ua = affine(v.m, ax, ay, az), va = affine(v.m + 4, ax, ay, az),
         wa = affine(v.m + 8, ax, ay, az);
  double ub = affine(v.m, bx, by, bz), vb = affine(v.m + 4, bx, by, bz),
         wb = affine(v.m + 8, bx, by, bz);
  if (!(finite64(ua) && finite64(va) && finite64(wa) && finite64(ub) &&
        finite64(vb) && finite64(wb)))
    return false;
  bool a_behind = wa < v.near, b_behind = wb < v.near;
  if (a_behind && b_behind) return false;
  if (a_behind) {
    double c = (v.near - wa) / (wb - wa);
    ua = ua + c * (ub - ua);
    va = va + c * (vb - va);
    wa = v.near;
  } else if (b_behind) {
    double c = (v.near - wb) / (wa - wb);
    ub = ub + c * (ua - ub);
    vb = vb + c * (va - vb);
    wb = v.near;
  }
  double fx0 = floor(ua / wa), fy0 = floor(va / wa);
  double fx1 = floor(ub / wb), fy1 = floor(vb / wb);
  if (!(fabs(fx0) < kCoordLimit && fabs(fy0) < kCoordLimit &&
        fabs(fx1) < kCoordLimit && fabs(fy1) < kCoordLimit))
    return false;  // NaN fails too
  int64_t x0 = (int64_t)fx0, y0 = (int64_t)fy0, x1 = (int64_t)fx1,
          y1 = (int64_t)fy1;
  int64_t dx = x1 - x0, dy = y1 - y0;
  int64_t adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  pl.swap = ady > adx;
  int64_t da = pl.swap ? dy : dx;
  pl.a0 = pl.swap ? y0 : x0;
  pl.b0 = pl.swap ? x0 : y0;
  pl.db = pl.swap ? dx : dy;
  pl.n = pl.swap ? ady : adx;
  pl.s = da < 0 ? -1 : 1;
  pl.t = t;
  // only the k whose major coordinate is on the canvas or one pixel beside it
  // (a stamp of thickness <= 3 reaches one pixel): work bounded by the canvas
  int64_t lo = -1, hi = pl.swap ? v.h : v.w;
  if (pl.s > 0) {
    pl.k0 = max((int64_t)0, lo - pl.a0);
    pl.k1 = min(pl.n, hi - pl.a0);
  } else {
    pl.k0 = max((int64_t)0, pl.a0 - hi);
    pl.k1 = min(pl.n, pl.a0 - lo);
  }
  return pl.k0 <= pl.k1;
}

__device__ __forceinline__ void draw_pixel(const SegPlan &pl, int64_t k,
                                           const View &v,
                                           unsigned long long *keys,
                                           unsigned long long key) {
  int64_t a = pl.a0 + k * pl.s;
  int64_t b = pl.b0;
  if (pl.n > 0) b += floordiv64(2 * k * pl.db + pl.n, 2 * pl.n);
  int64_t x = pl.swap ? b : a, y = pl.swap ? a : b;
  int lo = -((pl.t - 1) / 2), hi = pl.t / 2;
  if (x + hi < 0 || x + lo >= v.w || y + hi < 0 || y + lo >= v.h) return;
  for (int oy = lo; oy <= hi; ++oy) {
    int64_t yy = y + oy;
    if (yy < 0 || yy >= v.h) continue;
    for (int ox = lo; ox <= hi; ++ox) {
      int64_t xx = x + ox;
      if (xx < 0 || xx >= v.w) continue;
      put_key(keys, yy * v.w + xx, key);
    }
  }
}

// Lanes over segments for the short ones (graph edges: a few pixels each);
// a segment of more than kShort pixels is drawn by its whole wave, lanes
// over k (box edges across the canvas).
template <typename T>
__global__ __launch_bounds__(kBlock) void render_segments_kernel(
    const T *__restrict__ seg, int64_t n_seg, View v,
    const uint8_t *__restrict__ thick, int t_uniform,
    unsigned long long *keys) {
  __shared__ SegPlan plans[kBlock];
  const int lane = threadIdx.x & 63, wave_base = threadIdx.x & ~63;
  for (int64_t base = blockIdx.x * (int64_t)kBlock; base < n_seg;
       base += (int64_t)gridDim.x * kBlock) {
    int64_t i = base + threadIdx.x;
    SegPlan pl;
    bool ok = false;
    if (i < n_seg) {
      int t = thick ? (int)thick[i] : t_uniform;
      ok = t >= 1 && t <= 3 && plan_segment(seg + 6 * i, v, t, pl);
    }
    bool wide = ok && (pl.k1 - pl.k0 + 1) > kShort;
    if (ok && !wide) {
      unsigned long long key = kSegLayer | (unsigned long long)i;
      for (int64_t k = pl.k0; k <= pl.k1; ++k) draw_pixel(pl, k, v, keys, key);
    }
    if (wide) plans[threadIdx.x] = pl;
    __syncthreads();
    unsigned long long todo = __ballot(wide);
    while (todo) {
      int j = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const SegPlan q = plans[wave_base + j];
      unsigned long long key =
          kSegLayer | (unsigned long long)(base + wave_base + j);
      for (int64_t k = q.k0 + lane; k <= q.k1; k += 64)
        draw_pixel(q, k, v, keys, key);
    }
    __syncthreads();
  }
}

__global__ void render_resolve_kernel(
    const unsigned long long *__restrict__ keys, int64_t n_pix,
    const uint8_t *__restrict__ pcol, int64_t n_pcol,
    const uint8_t *__restrict__ scol, int64_t n_scol,
    const uint8_t *__restrict__ bg_image, uint32_t bg_rgb,
    uint8_t *__restrict__ image) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_pix;
       i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long key = keys[i];
    const uint8_t *c = nullptr;
    if (key & kSegLayer) {
      int64_t s = (int64_t)(key & ~kSegLayer);
      if (n_scol == 1) c = scol;
      else if (s < n_scol) c = scol + 3 * s;
    } else if (key & kPointLayer) {
      int64_t p = (int64_t)(kIndexMask - (key & kIndexMask));
      if (n_pcol == 1) c = pcol;
      else if (p < n_pcol) c = pcol + 3 * p;
    }
    uint8_t r, g, b;
    if (c) {
      r = c[0], g = c[1], b = c[2];
    } else if (bg_image) {
      r = bg_image[3 * i], g = bg_image[3 * i + 1], b = bg_image[3 * i + 2];
    } else {
      r = (uint8_t)(bg_rgb >> 16), g = (uint8_t)(bg_rgb >> 8), b = (uint8_t)bg_rgb;
    }
    image[3 * i] = r;
    image[3 * i + 1] = g;
    image[3 * i + 2] = b;
  }
}

template <typename T>
__global__ void render_colorize_kernel(const T *__restrict__ values, int64_t n,
                                       double lo, double hi,
                                       const uint8_t *__restrict__ table,
                                       uint8_t *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double f = floor(((double)values[i] - lo) / (hi - lo) * 255.0);
    int idx = f >= 255.0 ? 255 : f >= 0.0 ? (int)f : 0;  // NaN -> 0
    out[3 * i] = table[3 * idx];
    out[3 * i + 1] = table[3 * idx + 1];
    out[3 * i + 2] = table[3 * idx + 2];
  }
}

// rows of `out` [n_edges, 2, 3]: src[edges[e,0]], dst[edges[e,1]]; an index
// outside its array gives NaN (the segment is then dropped when drawn)
__global__ void render_graph_segments_kernel(
    const float *__restrict__ src, int64_t n_src, const float *__restrict__ dst,
    int64_t n_dst, const int32_t *__restrict__ edges, int64_t n_edges,
    float *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       i < 2 * n_edges; i += (int64_t)gridDim.x * blockDim.x) {
    int end = (int)(i & 1);
    int64_t j = edges[i];
    const float *tab = end ? dst : src;
    bool ok = j >= 0 && j < (end ? n_dst : n_src);
    float nan = __uint_as_float(0x7FC00000u);
    out[3 * i] = ok ? tab[3 * j] : nan;
    out[3 * i + 1] = ok ? tab[3 * j + 1] : nan;
    out[3 * i + 2] = ok ? tab[3 * j + 2] : nan;
  }
}

// ---- text ---------------------------------------------------------------------
// A pass over a finished image with a key plane of its own: one uint32 per
// pixel, (string + 1) << 1 | is_glyph, atomic max.  The later string wins
// and, within a string, the glyph wins over the plate.
__constant__ pgnn::Font5x7 d_font = pgnn::kFont5x7;

constexpr int kAdvance = pgnn::kFontCols + 1;  // columns from glyph to glyph
constexpr int kMaxScale = 4;

__device__ __forceinline__ void put_key32(uint32_t *keys, int64_t pix,
                                          uint32_t key) {
  uint32_t cur = __hip_atomic_load(keys + pix, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
  if (cur >= key) return;
  __hip_atomic_fetch_max(keys + pix, key, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void text_clear_kernel(uint32_t *keys, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = 0;
}

// One wave per string, its lanes over (glyph row, visible character) and then
// over the pixels of the clipped plate: the work of a string is bounded by
// the canvas, and a character left or right of it is never visited.
__global__ __launch_bounds__(kBlock) void text_stamp_kernel(
    const uint8_t *__restrict__ chars, const int32_t *__restrict__ offsets,
    int64_t n_strings,
    const int32_t *__restrict__ anchors, const uint8_t *__restrict__ scales,
    int scale_uniform, int plates, int32_t w, int32_t h, uint32_t *keys) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // chars holds offsets[n_strings] bytes: a string that ends beyond is dropped
  const int64_t total = chars ? (int64_t)offsets[n_strings] : 0;
  for (int64_t j = wave; j < n_strings; j += n_waves) {
    const int64_t begin = offsets[j], end = offsets[j + 1];
    if (begin < 0 || end <= begin || end > total) continue;  // empty, malformed
    const int64_t s = scales ? (int64_t)scales[j] : (int64_t)scale_uniform;
    if (s < 1 || s > kMaxScale) continue;
    const int64_t n = end - begin;
    const int64_t x = anchors[2 * j], y = anchors[2 * j + 1];
    const int64_t adv = kAdvance * s;
    const uint32_t key = (uint32_t)(j + 1) << 1;
    // characters with a glyph column on the canvas:
    //   x + i adv + 5 s > 0  and  x + i adv < w
    if (y + pgnn::kFontRows * s > 0 && y < h) {
      int64_t i_lo = floordiv64(-x - pgnn::kFontCols * s, adv) + 1;
      int64_t i_hi = floordiv64((int64_t)w - 1 - x, adv);
      if (i_lo < 0) i_lo = 0;
      if (i_hi > n - 1) i_hi = n - 1;
      const int64_t n_vis = i_hi - i_lo + 1;
      for (int64_t item = lane; item < n_vis * pgnn::kFontRows; item += 64) {
        const int r = (int)(item / n_vis);
        const int64_t i = i_lo + item % n_vis;
        const int64_t py0 = y + r * s;
        if (py0 + s <= 0 || py0 >= h) continue;
        int code = (int)chars[begin + i] - pgnn::kFontFirst;
        if (code < 0 || code >= pgnn::kFontGlyphs) code = '?' - pgnn::kFontFirst;
        const unsigned bits = d_font.rows[code][r];
        for (int c = 0; c < pgnn::kFontCols; ++c) {
          if (!(bits >> (pgnn::kFontCols - 1 - c) & 1u)) continue;
          const int64_t px0 = x + (kAdvance * i + c) * s;
          for (int64_t yy = py0; yy < py0 + s; ++yy) {
            if (yy < 0 || yy >= h) continue;
            for (int64_t xx = px0; xx < px0 + s; ++xx) {
              if (xx < 0 || xx >= w) continue;
              put_key32(keys, yy * w + xx, key | 1u);
            }
          }
        }
      }
    }
    if (plates) {
      // [x - s, x + (6 n - 1) s + s) x [y - s, y + 7 s + s), cut to the canvas
      int64_t x0 = x - s, x1 = x + kAdvance * n * s;
      int64_t y0 = y - s, y1 = y + (pgnn::kFontRows + 1) * s;
      if (x0 < 0) x0 = 0;
      if (y0 < 0) y0 = 0;
      if (x1 > w) x1 = w;
      if (y1 > h) y1 = h;
      if (x0 < x1 && y0 < y1) {
        const int64_t cw = x1 - x0, area = cw * (y1 - y0);
        for (int64_t p = lane; p < area; p += 64)
          put_key32(keys, (y0 + p / cw) * w + (x0 + p % cw), key);
      }
    }
  }
}

__global__ void text_resolve_kernel(const uint32_t *__restrict__ keys,
                                    int64_t n_pix,
                                    const uint8_t *__restrict__ colors,
                                    int64_t n_colors,
                                    const uint8_t *__restrict__ plate_colors,
                                    int64_t n_plate_colors,
                                    uint8_t *__restrict__ image) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_pix;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t key = keys[i];
    if (key == 0) continue;  // no string owns the pixel: its bytes stay
    const int64_t j = (int64_t)(key >> 1) - 1;
    const uint8_t *c = (key & 1u) ? colors + (n_colors == 1 ? 0 : 3 * j)
                                  : plate_colors +
                                        (n_plate_colors == 1 ? 0 : 3 * j);
    image[3 * i] = c[0];
    image[3 * i + 1] = c[1];
    image[3 * i + 2] = c[2];
  }
}

unsigned grid_of(int64_t n) {
  int64_t g = (n + kBlock - 1) / kBlock;
  return (unsigned)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

bool canvas_ok(int32_t w, int32_t h) {
  return w >= 1 && w <= PGNN_RENDER_MAX_DIM && h >= 1 &&
         h <= PGNN_RENDER_MAX_DIM;
}

size_t key_bytes(int32_t w, int32_t h) {
  return pgnn::align_up((size_t)w * (size_t)h * sizeof(unsigned long long), 256);
}

// -> error message or nullptr
const char *load_view(const double *m, const double *d, double near, int32_t w,
                      int32_t h, View *v) {
  if (!m) return "null view matrix";
  if (!canvas_ok(w, h)) return "width and height must be 1..4096";
  if (!(fabs(near) < INFINITY)) return "near must be finite";
  for (int i = 0; i < 12; ++i) v->m[i] = m[i];
  for (int i = 0; i < 4; ++i) v->d[i] = d ? d[i] : 0.0;
  v->near = near;
  v->w = w;
  v->h = h;
  return nullptr;
}

}  // namespace

extern "C" size_t pgnn_render_workspace_bytes(int32_t width, int32_t height) {
  if (!canvas_ok(width, height)) return 0;
  return key_bytes(width, height);
}

extern "C" int pgnn_render_clear(int32_t width, int32_t height, void *workspace,
                                 size_t workspace_bytes, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(canvas_ok(width, height), PGNN_E_INVALID,
               "render_clear: width and height must be 1..4096");
  PGNN_REQUIRE(workspace, PGNN_E_INVALID, "render_clear: null pointer");
  PGNN_REQUIRE(workspace_bytes >= key_bytes(width, height), PGNN_E_WORKSPACE,
               "render_clear: workspace too small "
               "(see pgnn_render_workspace_bytes)");
  int64_t n = (int64_t)width * height;
  hipLaunchKernelGGL(render_clear_kernel, dim3(grid_of(n)), dim3(kBlock), 0,
                     stream, (unsigned long long *)workspace, n);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_render_points(const void *xyz, int32_t is_f64,
                                  int64_t n_points, const double *view_m,
                                  const double *view_d, double near,
                                  int32_t width, int32_t height,
                                  int32_t point_size, void *workspace,
                                  size_t workspace_bytes, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  View v;
  PGNN_REQUIRE(view_d, PGNN_E_INVALID, "render_points: null depth row");
  const char *bad = load_view(view_m, view_d, near, width, height, &v);
  if (bad) return fail(PGNN_E_INVALID, bad);
  PGNN_REQUIRE(point_size >= 1 && point_size <= 3, PGNN_E_INVALID,
               "render_points: point_size must be 1..3");
  PGNN_REQUIRE(n_points >= 0 && n_points < (int64_t)1 << kIndexBits,
               PGNN_E_INVALID, "render_points: n_points must be 0..2^30-1");
  PGNN_REQUIRE(workspace && (xyz || n_points == 0), PGNN_E_INVALID,
               "render_points: null pointer");
  PGNN_REQUIRE(workspace_bytes >= key_bytes(width, height), PGNN_E_WORKSPACE,
               "render_points: workspace too small "
               "(see pgnn_render_workspace_bytes)");
  if (n_points == 0) return 0;
  unsigned long long *keys = (unsigned long long *)workspace;
  if (is_f64)
    hipLaunchKernelGGL(render_points_kernel<double>, dim3(grid_of(n_points)),
                       dim3(kBlock), 0, stream, (const double *)xyz, n_points,
                       v, (int)point_size, keys);
  else
    hipLaunchKernelGGL(render_points_kernel<float>, dim3(grid_of(n_points)),
                       dim3(kBlock), 0, stream, (const float *)xyz, n_points, v,
                       (int)point_size, keys);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_render_segments(const void *segments, int32_t is_f64,
                                    int64_t n_segments, const double *view_m,
                                    double near, int32_t width, int32_t height,
                                    const uint8_t *thickness_per_segment,
                                    int32_t thickness, void *workspace,
                                    size_t workspace_bytes, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  View v;
  const char *bad = load_view(view_m, nullptr, near, width, height, &v);
  if (bad) return fail(PGNN_E_INVALID, bad);
  PGNN_REQUIRE(thickness_per_segment || (thickness >= 1 && thickness <= 3),
               PGNN_E_INVALID, "render_segments: thickness must be 1..3");
  PGNN_REQUIRE(n_segments >= 0 && n_segments < (int64_t)1 << 40, PGNN_E_INVALID,
               "render_segments: bad size");
  PGNN_REQUIRE(workspace && (segments || n_segments == 0), PGNN_E_INVALID,
               "render_segments: null pointer");
  PGNN_REQUIRE(workspace_bytes >= key_bytes(width, height), PGNN_E_WORKSPACE,
               "render_segments: workspace too small "
               "(see pgnn_render_workspace_bytes)");
  if (n_segments == 0) return 0;
  unsigned long long *keys = (unsigned long long *)workspace;
  if (is_f64)
    hipLaunchKernelGGL(render_segments_kernel<double>,
                       dim3(grid_of(n_segments)), dim3(kBlock), 0, stream,
                       (const double *)segments, n_segments, v,
                       thickness_per_segment, (int)thickness, keys);
  else
    hipLaunchKernelGGL(render_segments_kernel<float>, dim3(grid_of(n_segments)),
                       dim3(kBlock), 0, stream, (const float *)segments,
                       n_segments, v, thickness_per_segment, (int)thickness,
                       keys);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_render_resolve(int32_t width, int32_t height,
                                   const void *workspace, size_t workspace_bytes,
                                   const uint8_t *point_colors,
                                   int64_t n_point_colors,
                                   const uint8_t *segment_colors,
                                   int64_t n_segment_colors,
                                   const uint8_t *background_image,
                                   uint32_t background_rgb, uint8_t *image,
                                   void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(canvas_ok(width, height), PGNN_E_INVALID,
               "render_resolve: width and height must be 1..4096");
  PGNN_REQUIRE(n_point_colors >= 0 && n_segment_colors >= 0, PGNN_E_INVALID,
               "render_resolve: bad size");
  PGNN_REQUIRE(workspace && image && (point_colors || n_point_colors == 0) &&
                   (segment_colors || n_segment_colors == 0),
               PGNN_E_INVALID, "render_resolve: null pointer");
  PGNN_REQUIRE(workspace_bytes >= key_bytes(width, height), PGNN_E_WORKSPACE,
               "render_resolve: workspace too small "
               "(see pgnn_render_workspace_bytes)");
  int64_t n = (int64_t)width * height;
  hipLaunchKernelGGL(render_resolve_kernel, dim3(grid_of(n)), dim3(kBlock), 0,
                     stream, (const unsigned long long *)workspace, n,
                     point_colors, n_point_colors, segment_colors,
                     n_segment_colors, background_image, background_rgb, image);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_render_colorize(const void *values, int32_t is_f64,
                                    int64_t n, double lo, double hi,
                                    const uint8_t *table, uint8_t *colors,
                                    void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n >= 0, PGNN_E_INVALID, "render_colorize: bad size");
  PGNN_REQUIRE(table && ((values && colors) || n == 0), PGNN_E_INVALID,
               "render_colorize: null pointer");
  if (n == 0) return 0;
  if (is_f64)
    hipLaunchKernelGGL(render_colorize_kernel<double>, dim3(grid_of(n)),
                       dim3(kBlock), 0, stream, (const double *)values, n, lo,
                       hi, table, colors);
  else
    hipLaunchKernelGGL(render_colorize_kernel<float>, dim3(grid_of(n)),
                       dim3(kBlock), 0, stream, (const float *)values, n, lo,
                       hi, table, colors);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_render_graph_segments(const float *src_xyz, int64_t n_src,
                                          const float *dst_xyz, int64_t n_dst,
                                          const int32_t *edges, int64_t n_edges,
                                          float *segments, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(n_src >= 0 && n_dst >= 0 && n_edges >= 0, PGNN_E_INVALID,
               "render_graph_segments: bad size");
  PGNN_REQUIRE((src_xyz || n_src == 0) && (dst_xyz || n_dst == 0) &&
                   ((edges && segments) || n_edges == 0),
               PGNN_E_INVALID, "render_graph_segments: null pointer");
  if (n_edges == 0) return 0;
  hipLaunchKernelGGL(render_graph_segments_kernel, dim3(grid_of(2 * n_edges)),
                     dim3(kBlock), 0, stream, src_xyz, n_src, dst_xyz, n_dst,
                     edges, n_edges, segments);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}

namespace {

size_t text_key_bytes(int32_t w, int32_t h) {
  return pgnn::align_up((size_t)w * (size_t)h * sizeof(uint32_t), 256);
}

}  // namespace

extern "C" size_t pgnn_render_text_workspace_bytes(int32_t width,
                                                   int32_t height) {
  if (!canvas_ok(width, height)) return 0;
  return text_key_bytes(width, height);
}

extern "C" int pgnn_render_font(uint8_t *table_host) {
  PGNN_GUARD_BEGIN
  PGNN_REQUIRE(table_host, PGNN_E_INVALID, "render_font: null pointer");
  for (int g = 0; g < pgnn::kFontGlyphs; ++g)
    for (int r = 0; r < pgnn::kFontRows; ++r)
      table_host[g * pgnn::kFontRows + r] = pgnn::kFont5x7.rows[g][r];
  return 0;
  PGNN_GUARD_END
}

extern "C" int pgnn_render_text(uint8_t *image, int32_t width, int32_t height,
                                const uint8_t *chars, const int32_t *offsets,
                                int64_t n_strings, const int32_t *anchors,
                                const uint8_t *scales, int32_t scale,
                                const uint8_t *colors, int64_t n_colors,
                                const uint8_t *plate_colors,
                                int64_t n_plate_colors, void *workspace,
                                size_t workspace_bytes, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(canvas_ok(width, height), PGNN_E_INVALID,
               "render_text: width and height must be 1..4096");
  PGNN_REQUIRE(scales || (scale >= 1 && scale <= kMaxScale), PGNN_E_INVALID,
               "render_text: scale must be 1..4");
  PGNN_REQUIRE(n_strings >= 0 && n_strings < (int64_t)1 << 30, PGNN_E_INVALID,
               "render_text: n_strings must be 0..2^30-1");
  PGNN_REQUIRE(n_colors == 1 || n_colors == n_strings, PGNN_E_INVALID,
               "render_text: n_colors must be 1 or n_strings");
  PGNN_REQUIRE(n_plate_colors == 0 || n_plate_colors == 1 ||
                   n_plate_colors == n_strings,
               PGNN_E_INVALID,
               "render_text: n_plate_colors must be 0, 1 or n_strings");
  PGNN_REQUIRE((colors || n_colors == 0) &&
                   (plate_colors || n_plate_colors == 0),
               PGNN_E_INVALID, "render_text: null pointer");
  if (n_strings == 0) return 0;
  PGNN_REQUIRE(image && offsets && anchors && workspace, PGNN_E_INVALID,
               "render_text: null pointer");
  PGNN_REQUIRE(workspace_bytes >= text_key_bytes(width, height),
               PGNN_E_WORKSPACE,
               "render_text: workspace too small "
               "(see pgnn_render_text_workspace_bytes)");
  uint32_t *keys = (uint32_t *)workspace;
  int64_t n = (int64_t)width * height;
  hipLaunchKernelGGL(text_clear_kernel, dim3(grid_of(n)), dim3(kBlock), 0,
                     stream, keys, n);
  PGNN_HIP(hipGetLastError());
  hipLaunchKernelGGL(text_stamp_kernel, dim3(grid_of(n_strings * 64)),
                     dim3(kBlock), 0, stream, chars, offsets, n_strings,
                     anchors, scales, (int)scale, (int)(n_plate_colors != 0),
                     width, height, keys);
  PGNN_HIP(hipGetLastError());
  hipLaunchKernelGGL(text_resolve_kernel, dim3(grid_of(n)), dim3(kBlock), 0,
                     stream, (const uint32_t *)keys, n, colors, n_colors,
                     plate_colors, n_plate_colors, image);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}
