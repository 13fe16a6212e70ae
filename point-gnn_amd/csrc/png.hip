// PNG scanline unfilter (include/pointgnn_hip.h, "PNG scanline unfilter"):
// the inflated stream of an 8-bit, non-interlaced PNG -> uint8 [H, W, 3].
// Inflate stays on the host (pointgnn_amd/png.py); nothing is decoded here.
//
// A byte depends on its left neighbour (a), the byte above (b) and the byte
// above-left (c): the image is one skewed wavefront.  ONE workgroup of kRows
// lanes, lane = row.  At step t a lane works on pixel x = t - skew, where
// skew = row + kChunk * wave: inside a wave the row above is one step ahead
// and its result arrives by a shuffle from the lane below; the last row of the
// wave above is kChunk + 1 steps ahead and its results arrive through an LDS
// ring, so that ONE barrier per kChunk steps orders them, not one per step.
//   ring slot = x mod kRing.  In one chunk the consumer reads pixels
//   [X, X + kChunk) and the producer writes [X + kChunk + 1, X + 2 kChunk]:
//   what is read was written in an earlier chunk, behind a barrier, and a slot
//   is written again kRing / kChunk = 4 chunks after it was read.
// A pixel's C <= 4 bytes travel in one dword.  a is the lane's previous result,
// c the b of its previous step.  The filtered bytes of the next chunk are
// loaded while this chunk is worked on, and both they and the image bytes
// move a chunk at a time as whole dwords (see the step loop).
// Images taller than kRows run in bands; the last UNFILTERED row of a band
// reaches lane 0 of the next band through the workspace, one dword per pixel
// and one row per band (no address is written twice), a block-scope fence and
// a barrier between the band that writes and the band that reads.
// Every barrier is reached by all kRows lanes: the trip counts depend on the
// band only, lanes without a pixel predicate their work.
#include "pgnn_common.h"

namespace pgnn {
namespace {

constexpr int kRows = 512;  // rows in flight = lanes of the workgroup
constexpr int kWaves = kRows / 64;
constexpr int kChunk = 8;   // steps per barrier; also the extra skew per wave
constexpr int kRing = 32;   // LDS ring entries per wave, >= 2 kChunk + 1
constexpr int kOutWords = 3 * kChunk / 4;  // dwords of image per lane and chunk

__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  // p = a + b - c: |p - a| = |b - c|, |p - b| = |a - c|, |p - c| = |a + b - 2c|
  // (one absolute-difference instruction each: the operands are below 2^16,
  // so the upper halves the instruction also sums are zero)
  const uint32_t pa = __builtin_amdgcn_sad_u16(b, c, 0u);
  const uint32_t pb = __builtin_amdgcn_sad_u16(a, c, 0u);
  const uint32_t pc = __builtin_amdgcn_sad_u16(a + b, 2u * c, 0u);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// One pixel: C bytes packed little-endian in a dword, the bytes above them
// zero.  None / Sub / Up / Average work on the four bytes at once (no carry
// crosses a byte: the sums are split into the low seven bits and the top bit);
// Paeth goes byte by byte, and only where a lane of the wave has such a row.
template <int C>
__device__ __forceinline__ uint32_t reconstruct(uint32_t ftype, uint32_t f,
                                                uint32_t a, uint32_t b,
                                                uint32_t c) {
  // floor((a + b) / 2) per byte, the sum in nine bits
  const uint32_t avg = (a & b) + (((a ^ b) >> 1) & 0x7F7F7F7Fu);
  uint32_t pred = 0;
  pred = ftype == 1 ? a : pred;
  pred = ftype == 2 ? b : pred;
  pred = ftype == 3 ? avg : pred;
  if (ftype == 4) {
    pred = 0;
#pragma unroll
    for (int k = 0; k < C; ++k)
      pred |= paeth((a >> (8 * k)) & 255u, (b >> (8 * k)) & 255u,
                    (c >> (8 * k)) & 255u)
              << (8 * k);
  }
  // f + pred modulo 256 per byte
  return ((f & 0x7F7F7F7Fu) + (pred & 0x7F7F7F7Fu)) ^
         ((f ^ pred) & 0x80808080u);
}

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

// pixel s of a chunk whose kChunk * C bytes sit in the dwords w[]
template <int C>
__device__ __forceinline__ uint32_t chunk_pixel(const uint32_t *w, int s) {
  const int bit = 8 * C * s, i = bit >> 5, sh = bit & 31;
  uint32_t v = w[i] >> sh;
  if (sh + 8 * C > 32) v |= w[i + 1] << (32 - sh);
  return C < 4 ? v & ((1u << (8 * (C & 3))) - 1u) : v;
}

// kind: 0 grey (+ alpha), 1 colour (+ alpha), 2 palette index
template <int C, int KIND>
__global__ __launch_bounds__(kRows) void png_unfilter_kernel(
    const uint8_t *__restrict__ raw, int64_t width, int64_t height,
    const uint8_t *__restrict__ palette, int palette_entries, int bgr,
    uint32_t *carry, uint8_t *__restrict__ image) {
  __shared__ uint32_t ring[kWaves][kRing];
  __shared__ uint32_t pal[256];  // packed R | G << 8 | B << 16; 0 past the end
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (KIND == 2) {
    for (int i = tid; i < 256; i += kRows) {
      uint32_t v = 0;
      if (i < palette_entries)
        v = (uint32_t)palette[3 * i] | (uint32_t)palette[3 * i + 1] << 8 |
            (uint32_t)palette[3 * i + 2] << 16;
      pal[i] = v;
    }
  }
  for (int i = tid; i < kWaves * kRing; i += kRows) (&ring[0][0])[i] = 0;
  __syncthreads();

  constexpr int kInWords = kChunk * C / 4;  // dwords of stream per chunk
  const int64_t stride = 1 + width * C;
  const int64_t skew = tid + kChunk * wave;
  const int64_t n_bands = (height + kRows - 1) / kRows;
  for (int64_t band = 0; band < n_bands; ++band) {
    const int64_t row0 = band * kRows;
    const int64_t rows = height - row0 < kRows ? height - row0 : kRows;
    const bool active = tid < rows;
    const int64_t row = row0 + tid;
    const uint8_t *in = raw + (active ? row * stride + 1 : 1);
    uint8_t *out = image + (active ? row * width * 3 : 0);
    const uint32_t ftype = active ? raw[row * stride] : 0;
    // row 0 of a later band reads the row above from the band before
    const bool from_carry = tid == 0 && band > 0;
    const uint32_t *carry_in = carry + (band > 0 ? (band - 1) * width : 0);
    const bool to_carry = tid == kRows - 1 && band + 1 < n_bands;
    uint32_t *carry_out = carry + band * width;
    // uniform trip count: the last active lane's last pixel
    const int64_t last = rows - 1;
    const int64_t steps = width + last + kChunk * (last >> 6);
    const int64_t n_chunks = (steps + kChunk - 1) / kChunk;

    // A lane's chunk is kChunk * C contiguous bytes of its row and 3 * kChunk
    // contiguous bytes of the image.  Inside the row they move as whole
    // (unaligned) dwords, two loads and two stores per chunk; byte by byte only
    // in the two chunks that hang over a row's ends.  A byte access per pixel
    // makes every instruction touch 64 cache lines, one per row, and the
    // address path of the one CU, not its VALUs, then sets the pace.
    uint32_t cur[kInWords], nxt[kInWords], cur_up[kChunk], nxt_up[kChunk];
    auto load_chunk = [&](int64_t chunk, uint32_t *w, uint32_t *up) {
      const int64_t x0 = chunk * kChunk - skew;
#pragma unroll
      for (int i = 0; i < kInWords; ++i) w[i] = 0;
#pragma unroll
      for (int s = 0; s < kChunk; ++s) up[s] = 0;
      if (active && x0 >= 0 && x0 + kChunk <= width) {
        const u32_unaligned *p = (const u32_unaligned *)(in + x0 * C);
#pragma unroll
        for (int i = 0; i < kInWords; ++i) w[i] = p[i];
        if (from_carry) {
#pragma unroll
          for (int s = 0; s < kChunk; ++s) up[s] = carry_in[x0 + s];
        }
      } else if (active && x0 + kChunk > 0 && x0 < width) {
#pragma unroll
        for (int s = 0; s < kChunk; ++s) {
          const int64_t x = x0 + s;
          if (x >= 0 && x < width) {
#pragma unroll
            for (int k = 0; k < C; ++k)
              w[(s * C + k) >> 2] |= (uint32_t)in[x * C + k]
                                     << (8 * ((s * C + k) & 3));
            if (from_carry) up[s] = carry_in[x];
          }
        }
      }
    };
    load_chunk(0, cur, cur_up);
    uint32_t a = 0, c = 0, prev = 0;
    for (int64_t chunk = 0; chunk < n_chunks; ++chunk) {
      load_chunk(chunk + 1, nxt, nxt_up);  // past the end: nothing is loaded
      const int64_t x0 = chunk * kChunk - skew;
      uint32_t ow[kOutWords];
#pragma unroll
      for (int i = 0; i < kOutWords; ++i) ow[i] = 0;
#pragma unroll
      for (int s = 0; s < kChunk; ++s) {
        const int64_t x = x0 + s;
        const bool valid = active && x >= 0 && x < width;
        uint32_t b = __shfl_up(prev, 1);  // every lane takes part
        if (lane == 0)
          b = wave > 0 ? ring[wave - 1][(int)(x & (kRing - 1))] : cur_up[s];
        if (x <= 0) a = c = 0;
        const uint32_t res =
            reconstruct<C>(ftype, chunk_pixel<C>(cur, s), a, b, c);
        c = b;
        a = res;
        prev = res;
        if (valid) {
          if (lane == 63) ring[wave][(int)(x & (kRing - 1))] = res;
          if (to_carry) carry_out[x] = res;
        }
        // the pixel's three output bytes, first in memory lowest
        uint32_t px;
        if (KIND == 0) {
          px = (res & 255u) * 0x010101u;
        } else {
          const uint32_t rgb = KIND == 1 ? res & 0xFFFFFFu : pal[res & 255u];
          px = bgr ? ((rgb & 255u) << 16 | (rgb & 0xFF00u) | (rgb >> 16 & 255u))
                   : rgb;
        }
        ow[(24 * s) >> 5] |= px << ((24 * s) & 31);
        if (((24 * s) & 31) > 8) ow[((24 * s) >> 5) + 1] |=
            px >> (32 - ((24 * s) & 31));
      }
      if (active && x0 >= 0 && x0 + kChunk <= width) {
        u32_unaligned *p = (u32_unaligned *)(out + x0 * 3);
#pragma unroll
        for (int i = 0; i < kOutWords; ++i) p[i] = ow[i];
      } else if (active && x0 + kChunk > 0 && x0 < width) {
#pragma unroll
        for (int s = 0; s < kChunk; ++s) {
          const int64_t x = x0 + s;
          if (x >= 0 && x < width) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
              out[x * 3 + k] = (uint8_t)(ow[(3 * s + k) >> 2] >>
                                         (8 * ((3 * s + k) & 3)));
          }
        }
      }
      __syncthreads();  // this chunk's ring writes, before the next one's reads
#pragma unroll
      for (int i = 0; i < kInWords; ++i) cur[i] = nxt[i];
#pragma unroll
      for (int s = 0; s < kChunk; ++s) cur_up[s] = nxt_up[s];
    }
    // the carried row: written above by the last lane, read by lane 0 next
    __threadfence_block();
    __syncthreads();
  }
}

int channels_of(int32_t color_type) {
  switch (color_type) {
    case 0: return 1;
    case 2: return 3;
    case 3: return 1;
    case 4: return 2;
    case 6: return 4;
    default: return 0;
  }
}

// height * (1 + 4 width) and the workspace size must fit an int64
bool sizes_ok(int64_t width, int64_t height) {
  if (width < 1 || height < 1) return false;
  int64_t row = 0, total = 0;
  if (__builtin_mul_overflow(width, (int64_t)4, &row)) return false;
  if (__builtin_add_overflow(row, (int64_t)1, &row)) return false;
  return !__builtin_mul_overflow(row, height, &total);
}

}  // namespace
}  // namespace pgnn

using namespace pgnn;

extern "C" size_t pgnn_png_unfilter_workspace_bytes(int64_t width,
                                                    int64_t height) {
  if (!sizes_ok(width, height)) return 0;
  // one carried row per band but the last; never empty
  const int64_t bands = (height + kRows - 1) / kRows;
  const int64_t carried = bands > 1 ? bands - 1 : 1;
  return align_up((size_t)carried * (size_t)width * sizeof(uint32_t), 256);
}

extern "C" int pgnn_png_unfilter(const uint8_t *raw, int64_t width,
                                 int64_t height, int32_t color_type,
                                 const uint8_t *palette,
                                 int32_t palette_entries, int32_t bgr,
                                 void *workspace, size_t workspace_bytes,
                                 uint8_t *image, void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  PGNN_REQUIRE(sizes_ok(width, height), PGNN_E_INVALID,
               "pgnn_png_unfilter: width and height must be >= 1 and the "
               "stream size must fit an int64");
  const int C = channels_of(color_type);
  PGNN_REQUIRE(C != 0, PGNN_E_INVALID,
               "pgnn_png_unfilter: color_type must be 0, 2, 3, 4 or 6");
  PGNN_REQUIRE(raw && image && workspace, PGNN_E_INVALID,
               "pgnn_png_unfilter: null pointer");
  PGNN_REQUIRE(color_type != 3 ||
                   (palette && palette_entries >= 1 && palette_entries <= 256),
               PGNN_E_INVALID,
               "pgnn_png_unfilter: color_type 3 needs a palette of 1..256 "
               "entries");
  PGNN_REQUIRE(workspace_bytes >=
                   pgnn_png_unfilter_workspace_bytes(width, height),
               PGNN_E_WORKSPACE,
               "pgnn_png_unfilter: workspace too small "
               "(see pgnn_png_unfilter_workspace_bytes)");
  uint32_t *carry = (uint32_t *)workspace;
  const int b = bgr != 0;
#define PGNN_PNG_LAUNCH(C_, KIND_)                                            \
  hipLaunchKernelGGL((png_unfilter_kernel<C_, KIND_>), dim3(1), dim3(kRows),  \
                     0, stream, raw, width, height, palette,                  \
                     (int)palette_entries, b, carry, image)
  switch (color_type) {
    case 0: PGNN_PNG_LAUNCH(1, 0); break;
    case 2: PGNN_PNG_LAUNCH(3, 1); break;
    case 3: PGNN_PNG_LAUNCH(1, 2); break;
    case 4: PGNN_PNG_LAUNCH(2, 0); break;
    default: PGNN_PNG_LAUNCH(4, 1); break;
  }
#undef PGNN_PNG_LAUNCH
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}
