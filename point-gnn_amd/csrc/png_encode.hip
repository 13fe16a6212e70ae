// PNG encode (include/pointgnn_hip.h, "PNG encode"): a device uint8 [H, W, 3]
// image -> the zlib stream "pgnn deflate v1".  The header defines the bytes;
// this file is one way to compute them.  Three launches.
//
// 1. png_deflate_chunks_kernel: one workgroup of 1024 lanes per chunk of at
//    most 32 KiB of the scanline stream S (at most one workgroup per CU: with
//    more chunks than CUs a workgroup takes every grid-th chunk).  The chunk
//    is cut into segments of 32 bytes, one per lane.
//      stage    S (a filter byte 0 in front of every image row) into LDS;
//      masks    a lane takes its 32 bytes and the 4 before them in registers
//               and compares them with the bytes 1, 3 and R positions back: one
//               32-bit mask per candidate distance, bit k = "position k
//               equals its source and the source is inside the chunk".  The
//               run of ones starting at bit k is L_d, continued into the
//               following segments through `lead` (ones at a segment's start;
//               a match is capped at 258, so at most 9 segments are looked at);
//      tokens   every position's token (literal byte, or length and candidate)
//               is stored, 16 bits each, whether the parse visits it or not;
//               walking its segment backwards a lane also notes, per
//               position, where a parse that enters there LEAVES the segment
//               (9 bits: at most 257 past its end);
//      chain    one lane follows those exits from position 0: at most one
//               step per segment, two LDS reads each, instead of one step per
//               token.  It leaves each segment's entry position behind;
//      bits     every lane walks its segment from its entry: bit lengths, an
//               exclusive scan over the workgroup, then the codes OR-ed into
//               LDS words with 32-bit LDS atomics (a token has at most 31
//               bits: two words);
//      store    the chunk's bytes go to its worst-case slot as 16-byte
//               stores; its byte count and Adler pair beside them.
// 2. png_deflate_scan_kernel: one workgroup scans byte counts and Adler pairs
//    over the chunks (1024 per pass) and writes the total length.
// 3. png_deflate_pack_kernel: a lane per dword of `out`: header, slots and
//    trailer, a binary search over the chunk offsets finds the source.
// Nothing is read on the host and no size that depends on the data leaves the
// device.  Launches of one stream order the three kernels.
#include "pgnn_common.h"

namespace pgnn {
namespace {

constexpr int kThreads = 1024;    // lanes per chunk = segments per chunk
constexpr int kSeg = 32;          // stream bytes per lane
constexpr int kMaxChunk = kThreads * kSeg;
constexpr int kMaxMatch = 258;
constexpr uint32_t kMod = 65521;  // Adler-32

// floor((9 len + 20) / 8) + 4: the header's slot(len)
constexpr int64_t slot_bytes(int64_t len) { return (9 * len + 20) / 8 + 4; }

// LDS of the chunk kernel, byte offsets.  The packed bits overlay the staged
// stream (dead once the masks are in registers) and 4 KiB behind it.
constexpr int kFront = 16;  // zero bytes in front of S: S[-4..-1] are read
constexpr int kBitsBytes = (int)((slot_bytes(kMaxChunk) + 15) / 16 * 16) + 16;
constexpr int kExitOff = kBitsBytes;                // uint8 [32768]
constexpr int kTokOff = kExitOff + kMaxChunk;       // uint16 [32768]
constexpr int kEntryOff = kTokOff + 2 * kMaxChunk;  // uint8 [1024]
constexpr int kLeadOff = kEntryOff + kThreads;      // uint8 [3][1024]
constexpr int kLenTabOff = kLeadOff + 3 * kThreads; // uint32 [256]
constexpr int kScratchOff = kLenTabOff + 1024;      // per-wave sums
constexpr int kLdsBytes = kScratchOff + 16 * 16;
static_assert(kFront + kMaxChunk + 16 <= kBitsBytes, "S inside the overlay");
static_assert(kBitsBytes % 16 == 0 && kTokOff % 4 == 0 && kLenTabOff % 4 == 0 &&
                  kScratchOff % 8 == 0,
              "alignment");
static_assert(kLdsBytes <= 160 * 1024, "gfx950 LDS");
constexpr int kNoEntry = 255;

// token: bits 0..7 the literal, or length - 3; bits 8..9 0 = literal, 1..3 =
// match at candidate 1, 3, R; bit 15 the high bit of the segment exit
constexpr uint32_t kTokSel = 8, kTokExitHi = 15;

constexpr uint32_t rev_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// the length symbol of RFC 1951 3.2.5 with its extra bits, as they go into the
// stream (first bit lowest), and the bit count << 16
constexpr uint32_t length_entry(int length) {
  constexpr int base[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,
                            15, 17, 19, 23, 27, 31, 35, 43, 51,  59,
                            67, 83, 99, 115, 131, 163, 195, 227, 258};
  constexpr int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2,
                             2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  int k = 0;
  for (int j = 0; j < 29; ++j)
    if (base[j] <= length) k = j;
  const int sym = 257 + k;
  const uint32_t code = sym < 280 ? sym - 256 : 0xC0 + sym - 280;
  const int n = sym < 280 ? 7 : 8;
  return (rev_bits(code, n) | (uint32_t)(length - base[k]) << n) |
         (uint32_t)(n + extra[k]) << 16;
}

struct LengthTable {
  uint32_t v[256];
};
constexpr LengthTable make_length_table() {
  LengthTable t{};
  for (int i = 0; i < 256; ++i) t.v[i] = length_entry(i + 3);
  return t;
}
__device__ const LengthTable kLengthTable = make_length_table();

// the bits of a distance: 5-bit code, first bit lowest, then the extra bits
struct DistBits {
  uint32_t bits, n;
};
__device__ __forceinline__ DistBits distance_bits(uint32_t d) {
  // d >= 3 here: m = d - 1 >= 2, k = floor(log2 m) >= 1; codes 2k and 2k + 1
  // split [2^k + 1, 2^(k+1)] in halves, k - 1 extra bits each
  const uint32_t m = d - 1, k = 31 - __clz(m);
  const uint32_t code = 2 * k + ((m >> (k - 1)) & 1u), eb = k - 1;
  DistBits r;
  r.bits = (__brev(code) >> 27) | (m & ((1u << eb) - 1u)) << 5;
  r.n = 5 + eb;
  return r;
}

__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo,
                                           uint32_t shift) {
  return __builtin_amdgcn_alignbit(hi, lo, shift);  // ({hi, lo} >> shift), 0..31
}

// bit j of the result: byte j of a equals byte j of b
__device__ __forceinline__ uint32_t equal_bytes(uint32_t a, uint32_t b) {
  const uint32_t x = a ^ b;
  return (uint32_t)((x & 0xFFu) == 0) | (uint32_t)((x & 0xFF00u) == 0) << 1 |
         (uint32_t)((x & 0xFF0000u) == 0) << 2 |
         (uint32_t)((x & 0xFF000000u) == 0) << 3;
}

// ones from bit k of `mask` upwards, continued by `carry` when they reach
// bit 31; capped at the longest match
__device__ __forceinline__ int run_from(uint32_t mask, int k, int carry) {
  int c = __builtin_ctzll(~(uint64_t)(mask >> k));  // <= 32 - k
  if (c == kSeg - k) c += carry;
  return c < kMaxMatch ? c : kMaxMatch;
}

struct TokenBits {
  uint32_t bits, n;
};
__device__ __forceinline__ TokenBits token_bits(uint32_t tok,
                                                const uint32_t *len_tab,
                                                DistBits row) {
  const uint32_t sel = (tok >> kTokSel) & 3u, v = tok & 255u;
  TokenBits r;
  if (sel == 0) {
    const uint32_t code = v < 144 ? 0x30 + v : 0x190 + v - 144;
    r.n = v < 144 ? 8 : 9;
    r.bits = __brev(code) >> (32 - r.n);
  } else {
    const uint32_t e = len_tab[v], ln = e >> 16;
    // distance 1 is code 0, distance 3 code 2 = 00010, first bit lowest
    const uint32_t db = sel == 1 ? 0u : sel == 2 ? 8u : row.bits;
    const uint32_t dn = sel == 3 ? row.n : 5u;
    r.bits = (e & 0xFFFFu) | db << ln;  // at most 13 + 18 bits
    r.n = ln + dn;
  }
  return r;
}

__device__ __forceinline__ void or_bits(uint32_t *words, uint32_t bit_pos,
                                        uint32_t bits) {
  const uint64_t v = (uint64_t)bits << (bit_pos & 31u);
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  if (lo) atomicOr(&words[bit_pos >> 5], lo);
  if (hi) atomicOr(&words[(bit_pos >> 5) + 1], hi);
}

__global__ __launch_bounds__(kThreads) void png_deflate_chunks_kernel(
    const uint8_t *__restrict__ image, int64_t width, int64_t row_stride,
    int32_t chunk, int64_t n, int64_t n_chunks, int64_t slot_stride,
    uint8_t *__restrict__ slots, int32_t *__restrict__ chunk_bytes,
    uint32_t *__restrict__ adler_a, uint32_t *__restrict__ adler_b) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint32_t *const s32 = (uint32_t *)(lds + kFront);  // S, dword k = S[4k..]
  uint32_t *const bits32 = (uint32_t *)lds;          // the overlay
  uint8_t *const exit_lo = lds + kExitOff;
  uint16_t *const tok16 = (uint16_t *)(lds + kTokOff);
  uint8_t *const entry = lds + kEntryOff;
  uint8_t *const lead = lds + kLeadOff;
  uint32_t *const len_tab = (uint32_t *)(lds + kLenTabOff);
  uint32_t *const wave_bits = (uint32_t *)(lds + kScratchOff);
  uint32_t *const wave_a = wave_bits + 16;
  unsigned long long *const wave_b =
      (unsigned long long *)(lds + kScratchOff + 128);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t R = 3 * width + 1;
  const bool use_row = R <= 32768;
  const int row_d = use_row ? (int)R : 0;
  DistBits row_bits = {0u, 0u};
  if (use_row) row_bits = distance_bits((uint32_t)R);

  if (tid < 256) len_tab[tid] = kLengthTable.v[tid];
  entry[tid] = kNoEntry;

  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t a = c * chunk;
    const int len = (int)(n - a < chunk ? n - a : chunk);
    const int nseg = (len + kSeg - 1) / kSeg;
    const bool last = c == n_chunks - 1;

    // ---- stage: S[a, a + 32 nseg) as dwords, zeros past the chunk's end ----
    {
      const int64_t row0 = a / R, col0 = a - row0 * R;
      if (tid < kFront / 4) bits32[tid] = 0;
      for (int q = tid; q < nseg * (kSeg / 4); q += kThreads) {
        const int off = 4 * q;
        int64_t row, col;
        if (R < (1 << 24)) {  // col0 + off < 2^25
          const uint32_t t = (uint32_t)col0 + (uint32_t)off;
          const uint32_t dr = t / (uint32_t)R;
          row = row0 + dr;
          col = t - dr * (uint32_t)R;
        } else {              // off < R: at most one row further
          col = col0 + off;
          row = row0;
          if (col >= R) col -= R, ++row;
        }
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (off + j < len && col != 0)
            v |= (uint32_t)image[row * row_stride + (col - 1)] << (8 * j);
          if (++col == R) col = 0, ++row;
        }
        s32[q] = v;
      }
    }
    __syncthreads();

    // ---- masks --------------------------------------------------------------
    const int i0 = tid * kSeg;
    uint32_t w[9];  // w[k + 1] = S[i0 + 4k ..], w[0] the four bytes before
    uint32_t m1 = 0, m3 = 0, mr = 0, sum_a = 0, sum_b = 0;
    if (tid < nseg) {
#pragma unroll
      for (int k = 0; k < 9; ++k) w[k] = s32[tid * 8 - 1 + k];
      uint32_t u[9];  // the dwords around S[i0 - R ..]
      const int base = i0 - row_d, qi = base >> 2;  // floor, base may be < 0
      const uint32_t sh = (uint32_t)(base & 3) * 8;
#pragma unroll
      for (int k = 0; k < 9; ++k)
        u[k] = (use_row && qi + k >= -(kFront / 4)) ? s32[qi + k] : 0u;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        m1 |= equal_bytes(w[k + 1], funnel(w[k + 1], w[k], 24)) << (4 * k);
        m3 |= equal_bytes(w[k + 1], funnel(w[k + 1], w[k], 8)) << (4 * k);
        mr |= equal_bytes(w[k + 1], funnel(u[k + 1], u[k], sh)) << (4 * k);
      }
      // sources before the chunk, positions past its end
      const int left = len - i0;  // >= 1
      const uint32_t inside = left >= kSeg ? ~0u : (1u << left) - 1u;
      m1 &= inside & (tid == 0 ? ~1u : ~0u);
      m3 &= inside & (tid == 0 ? ~7u : ~0u);
      const int first = row_d - i0;  // first position whose source is >= a
      mr &= inside & (!use_row || first >= kSeg ? 0u
                      : first <= 0              ? ~0u
                                                : ~0u << first);
      lead[tid] = (uint8_t)__builtin_ctzll(~(uint64_t)m1);
      lead[kThreads + tid] = (uint8_t)__builtin_ctzll(~(uint64_t)m3);
      lead[2 * kThreads + tid] = (uint8_t)__builtin_ctzll(~(uint64_t)mr);
      // Adler: A = 1 + sum S[i], B = len + sum (len - i) S[i], i from 0.  Bytes
      // past the end are 0.  A lane's sums stay below 2^32: 32 * 255 and
      // 32 * 255 * 32768 = 2.7e8.
#pragma unroll
      for (int k = 0; k < kSeg; ++k) {
        const uint32_t v = (w[(k >> 2) + 1] >> (8 * (k & 3))) & 255u;
        sum_a += v;
        sum_b += v * (uint32_t)(len - i0 - k);
      }
    }
    __syncthreads();

    // ---- tokens and segment exits ------------------------------------------
    if (tid < nseg) {
      int carry[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        int acc = 0;
        for (int k = tid + 1; k < nseg && acc < kMaxMatch; ++k) {
          const int l = lead[d * kThreads + k];
          acc += l;
          if (l < kSeg) break;
        }
        carry[d] = acc;
      }
#pragma unroll
      for (int k = kSeg - 1; k >= 0; --k) {
        const int l1 = run_from(m1, k, carry[0]);
        const int l3 = run_from(m3, k, carry[1]);
        const int lr = run_from(mr, k, carry[2]);
        int best = l1;
        uint32_t sel = 1;
        if (l3 > best) best = l3, sel = 2;
        if (lr > best) best = lr, sel = 3;
        uint32_t tok;
        int next;
        if (best >= 3) {
          tok = sel << kTokSel | (uint32_t)(best - 3);
          next = k + best;
        } else {
          tok = (w[(k >> 2) + 1] >> (8 * (k & 3))) & 255u;
          next = k + 1;
        }
        // where a parse entering at k leaves the segment, past its end: this
        // token's end, or the exit of the position it ends on (already done;
        // positions past the chunk's end are literals and chain to the end)
        uint32_t out = (uint32_t)(next - kSeg);
        if (next < kSeg)
          out = exit_lo[i0 + next] |
                (uint32_t)(tok16[i0 + next] >> kTokExitHi) << 8;
        tok16[i0 + k] = (uint16_t)(tok | (out >> 8) << kTokExitHi);
        exit_lo[i0 + k] = (uint8_t)out;
      }
    }
    __syncthreads();

    // ---- chain: one lane, one step per segment it enters ---------------------
    const int out_words = (int)((slot_bytes(len) + 15) / 16) * 4;
    for (int i = tid; i < out_words; i += kThreads) bits32[i] = 0;
    if (tid == 0) {
      int pos = 0;
      while (pos < len) {
        const int seg = pos >> 5;
        entry[seg] = (uint8_t)(pos & (kSeg - 1));
        const int out = exit_lo[pos] | (tok16[pos] >> kTokExitHi) << 8;
        pos = (seg + 1) * kSeg + out;
      }
    }
    __syncthreads();

    // ---- bits ---------------------------------------------------------------
    const int end = i0 + kSeg < len ? i0 + kSeg : len;
    int start = end;
    if (tid < nseg && entry[tid] != kNoEntry) start = i0 + entry[tid];
    entry[tid] = kNoEntry;  // for the next chunk
    uint32_t my_bits = 0;
    for (int j = start; j < end;) {
      const uint32_t tok = tok16[j];
      my_bits += token_bits(tok, len_tab, row_bits).n;
      j += (tok >> kTokSel) & 3u ? (int)(tok & 255u) + 3 : 1;
    }
    // exclusive scan of the bit counts (at most 9 * 32768), sums of the Adler
    // terms: sum_b adds up to 255 * 32768 * 32769 / 2 = 1.4e11, in 64 bits
    uint32_t incl = my_bits, red_a = sum_a;
    unsigned long long red_b = sum_b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
      red_a += __shfl_xor(red_a, d);
      red_b += __shfl_xor(red_b, d);
    }
    if (lane == 63) wave_bits[wave] = incl;
    if (lane == 0) wave_a[wave] = red_a, wave_b[wave] = red_b;
    __syncthreads();
    uint32_t before = 0, total_bits = 0;
    for (int k = 0; k < kThreads / 64; ++k) {
      const uint32_t t = wave_bits[k];
      if (k < wave) before += t;
      total_bits += t;
    }
    // 3 header bits, the tokens, 7 zero bits of end-of-block; then either the
    // padding, or 3 zero bits of stored header, padding, 00 00 FF FF
    uint32_t bit_pos = 3 + before + incl - my_bits;
    for (int j = start; j < end;) {
      const uint32_t tok = tok16[j];
      const TokenBits t = token_bits(tok, len_tab, row_bits);
      or_bits(bits32, bit_pos, t.bits);
      bit_pos += t.n;
      j += (tok >> kTokSel) & 3u ? (int)(tok & 255u) + 3 : 1;
    }
    const uint32_t block_bits = 3 + total_bits + 7;
    int n_bytes = last ? (int)((block_bits + 7) / 8)
                       : (int)((block_bits + 3 + 7) / 8) + 4;
    // never more than the slot (9 bits per byte at most): the stores below and
    // the packer stay inside it whatever the tokens were
    n_bytes = n_bytes < (int)slot_bytes(len) ? n_bytes : (int)slot_bytes(len);
    if (tid == 0) {
      or_bits(bits32, 0, (last ? 1u : 0u) | 2u);  // BFINAL, BTYPE = 01
      if (!last) or_bits(bits32, 8u * (uint32_t)(n_bytes - 2), 0xFFFFu);
      uint32_t sa = 0;
      unsigned long long sb = 0;
      for (int k = 0; k < kThreads / 64; ++k) sa += wave_a[k], sb += wave_b[k];
      chunk_bytes[c] = n_bytes;
      adler_a[c] = (1u + sa) % kMod;  // at most 1 + 255 * 32768
      adler_b[c] = (uint32_t)(((unsigned long long)len + sb) % kMod);
    }
    __syncthreads();

    // ---- store: whole 16-byte pieces; the slot is that long -------------------
    {
      const uint4 *src = (const uint4 *)lds;
      uint4 *dst = (uint4 *)(slots + c * slot_stride);
      for (int i = tid; i < (n_bytes + 15) / 16; i += kThreads) dst[i] = src[i];
    }
    __syncthreads();  // the overlay becomes S again
  }
}

// (count, A, B, length mod 65521) of a run of chunks; `then` appends a run
struct Run {
  int64_t bytes;
  uint32_t a, b, len;
  __device__ Run then(const Run &r) const {
    Run o;
    o.bytes = bytes + r.bytes;
    o.a = (a + r.a + kMod - 1u) % kMod;
    // every term is below 2^16 except the product, below 2^32: 64 bits hold
    // the sum.  a - 1 as a + 65520: a may be 0.
    o.b = (uint32_t)(((uint64_t)b + r.b +
                      (uint64_t)r.len * ((a + kMod - 1u) % kMod)) % kMod);
    o.len = (len + r.len) % kMod;
    return o;
  }
};

__global__ __launch_bounds__(kThreads) void png_deflate_scan_kernel(
    int64_t n_chunks, int32_t chunk, int64_t n,
    const int32_t *__restrict__ chunk_bytes, const uint32_t *__restrict__ adler_a,
    const uint32_t *__restrict__ adler_b, int64_t *__restrict__ offsets,
    uint32_t *__restrict__ adler, int64_t *__restrict__ out_bytes) {
  __shared__ Run runs[kThreads];
  const int tid = threadIdx.x;
  Run carry = {0, 1u, 0u, 0u};  // the empty run
  for (int64_t c0 = 0; c0 < n_chunks; c0 += kThreads) {
    const int64_t c = c0 + tid;
    Run mine = {0, 1u, 0u, 0u};
    if (c < n_chunks) {
      const int64_t len = n - c * chunk < chunk ? n - c * chunk : chunk;
      mine.bytes = chunk_bytes[c];
      mine.a = adler_a[c];
      mine.b = adler_b[c];
      mine.len = (uint32_t)(len % kMod);
    }
    const int64_t my_bytes = mine.bytes;
    // inclusive scan, the earlier run on the left
    for (int d = 1; d < kThreads; d <<= 1) {
      runs[tid] = mine;
      __syncthreads();
      if (tid >= d) mine = runs[tid - d].then(mine);
      __syncthreads();
    }
    runs[tid] = mine;
    __syncthreads();
    if (c < n_chunks) offsets[c] = carry.bytes + mine.bytes - my_bytes;
    carry = carry.then(runs[kThreads - 1]);
    __syncthreads();
  }
  if (tid == 0) {
    offsets[n_chunks] = carry.bytes;
    *adler = carry.b << 16 | carry.a;
    *out_bytes = carry.bytes + 6;
  }
}

__global__ __launch_bounds__(256) void png_deflate_pack_kernel(
    int64_t n_chunks, int64_t slot_stride, const uint8_t *__restrict__ slots,
    const int64_t *__restrict__ offsets, const uint32_t *__restrict__ adler,
    uint8_t *__restrict__ out) {
  const int64_t total = offsets[n_chunks], out_len = total + 6;
  const uint32_t trailer = *adler;
  // the chunk that holds byte q of the blocks: offsets ascend strictly
  auto chunk_of = [&](int64_t q) {
    int64_t lo = 0, hi = n_chunks;
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (offsets[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
  };
  auto byte_at = [&](int64_t p) -> uint32_t {
    if (p < 2) return p == 0 ? 0x78u : 0x01u;
    if (p >= 2 + total) return (trailer >> (8 * (5 + total - p))) & 255u;
    const int64_t c = chunk_of(p - 2);
    return slots[c * slot_stride + (p - 2 - offsets[c])];
  };
  const int64_t n_words = (out_len + 3) / 4;
  for (int64_t wi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       wi < n_words; wi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = 4 * wi, q = p - 2;
    if (q >= 0 && q + 3 < total) {
      const int64_t c = chunk_of(q);
      if (q + 3 < offsets[c + 1]) {
        // four bytes of one slot: two aligned dwords of it (the slot has 4
        // spare bytes behind its longest content), shifted
        const int64_t rel = q - offsets[c];
        const uint32_t *s = (const uint32_t *)(slots + c * slot_stride) +
                            (rel >> 2);
        ((uint32_t *)out)[wi] = funnel(s[1], s[0], (uint32_t)(rel & 3) * 8);
        continue;
      }
    }
    if (p + 4 <= out_len) {
      ((uint32_t *)out)[wi] = byte_at(p) | byte_at(p + 1) << 8 |
                              byte_at(p + 2) << 16 | byte_at(p + 3) << 24;
    } else {
      for (int64_t j = p; j < out_len; ++j) out[j] = (uint8_t)byte_at(j);
    }
  }
}

struct Sizes {
  int64_t n, n_chunks, capacity, slot_stride;
};

// false: arguments out of range, or a size beyond int64 / 2^31 - 1 chunks
bool sizes_of(int64_t height, int64_t width, int32_t chunk, Sizes *s) {
  if (height < 1 || width < 1) return false;
  if (chunk < 256 || chunk > kMaxChunk || chunk % 256 != 0) return false;
  int64_t row = 0;
  if (__builtin_mul_overflow(width, (int64_t)3, &row)) return false;
  if (__builtin_add_overflow(row, (int64_t)1, &row)) return false;
  if (__builtin_mul_overflow(row, height, &s->n)) return false;
  const int64_t full = s->n / chunk, rest = s->n % chunk;
  s->n_chunks = full + (rest != 0);
  if (s->n_chunks > 0x7fffffff) return false;
  // 16-byte pieces are stored, and the packer reads one dword further
  s->slot_stride = (int64_t)align_up((size_t)slot_bytes(chunk) + 4, 16);
  int64_t all = 0;
  if (__builtin_mul_overflow(s->n_chunks, s->slot_stride + 64, &all))
    return false;
  s->capacity = 6 + full * slot_bytes(chunk) + (rest ? slot_bytes(rest) : 0);
  return true;
}

struct Workspace {
  uint8_t *slots;
  int32_t *chunk_bytes;
  uint32_t *adler_a, *adler_b, *adler;
  int64_t *offsets;
  size_t used;
  Workspace(void *p, size_t bytes, const Sizes &s) {
    Arena arena(p, bytes);
    const size_t k = (size_t)s.n_chunks;
    slots = arena.take<uint8_t>(k * (size_t)s.slot_stride);
    chunk_bytes = arena.take<int32_t>(k);
    adler_a = arena.take<uint32_t>(k);
    adler_b = arena.take<uint32_t>(k);
    offsets = arena.take<int64_t>(k + 1);
    adler = arena.take<uint32_t>(1);
    used = arena.used;
  }
};

}  // namespace
}  // namespace pgnn

using namespace pgnn;

extern "C" size_t pgnn_png_encode_workspace_bytes(int64_t height, int64_t width,
                                                  int32_t chunk_bytes) {
  Sizes s;
  if (!sizes_of(height, width, chunk_bytes, &s)) return 0;
  return align_up(Workspace(nullptr, 0, s).used, 256);
}

extern "C" int pgnn_png_encode(const uint8_t *image, int64_t height,
                               int64_t width, int64_t row_stride_bytes,
                               int32_t chunk_bytes, void *workspace,
                               size_t workspace_bytes, uint8_t *out,
                               int64_t out_capacity, int64_t *out_bytes_dev,
                               void *stream_) {
  PGNN_GUARD_BEGIN
  hipStream_t stream = (hipStream_t)stream_;
  Sizes s;
  PGNN_REQUIRE(sizes_of(height, width, chunk_bytes, &s), PGNN_E_INVALID,
               "pgnn_png_encode: height and width must be >= 1, chunk_bytes a "
               "multiple of 256 in 256..32768, and the stream at most "
               "2^31 - 1 chunks");
  PGNN_REQUIRE(row_stride_bytes >= 3 * width, PGNN_E_INVALID,
               "pgnn_png_encode: row_stride_bytes below 3 * width");
  PGNN_REQUIRE(image && workspace && out && out_bytes_dev, PGNN_E_INVALID,
               "pgnn_png_encode: null pointer");
  PGNN_REQUIRE(((uintptr_t)out & 3) == 0, PGNN_E_INVALID,
               "pgnn_png_encode: out must be 4-byte aligned");
  PGNN_REQUIRE(out_capacity >= s.capacity, PGNN_E_INVALID,
               "pgnn_png_encode: out_capacity below the worst case (see the "
               "header's formula)");
  PGNN_REQUIRE(workspace_bytes >=
                   pgnn_png_encode_workspace_bytes(height, width, chunk_bytes),
               PGNN_E_WORKSPACE,
               "pgnn_png_encode: workspace too small "
               "(see pgnn_png_encode_workspace_bytes)");
  PGNN_REQUIRE(((uintptr_t)workspace & 15) == 0, PGNN_E_INVALID,
               "pgnn_png_encode: workspace must be 16-byte aligned");
  const Workspace ws(workspace, workspace_bytes, s);
  int rc = ensure_dynamic_lds((const void *)png_deflate_chunks_kernel,
                              (size_t)kLdsBytes);
  if (rc) return rc;
  // a workgroup fills a CU's LDS: one per CU, each striding over the chunks
  const int64_t cus = device_cu_count();
  const unsigned grid = (unsigned)(s.n_chunks < cus ? s.n_chunks : cus);
  hipLaunchKernelGGL(png_deflate_chunks_kernel, dim3(grid), dim3(kThreads),
                     (size_t)kLdsBytes, stream, image, width, row_stride_bytes,
                     chunk_bytes, s.n, s.n_chunks, s.slot_stride, ws.slots,
                     ws.chunk_bytes, ws.adler_a, ws.adler_b);
  PGNN_HIP(hipGetLastError());
  hipLaunchKernelGGL(png_deflate_scan_kernel, dim3(1), dim3(kThreads), 0,
                     stream, s.n_chunks, chunk_bytes, s.n, ws.chunk_bytes,
                     ws.adler_a, ws.adler_b, ws.offsets, ws.adler,
                     out_bytes_dev);
  PGNN_HIP(hipGetLastError());
  const int64_t words = (s.capacity + 3) / 4, blocks = (words + 255) / 256;
  hipLaunchKernelGGL(png_deflate_pack_kernel,
                     dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256),
                     0, stream, s.n_chunks, s.slot_stride, ws.slots, ws.offsets,
                     ws.adler, out);
  PGNN_HIP(hipGetLastError());
  return 0;
  PGNN_GUARD_END
}
