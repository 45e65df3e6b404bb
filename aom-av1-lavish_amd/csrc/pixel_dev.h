// pixel_dev.h -- device and launch helpers shared by the pixel-domain kernels
// (pixel.hip, pixel_comp.hip): wave / lane-group sums, word-wide unaligned
// loads and the word-chunk layout of a block over the lanes of a wave.
#pragma once
#include "lavish_internal.h"

namespace lavish {

__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// A job's rows are cut into chunks of C = min(4, words per row) 4-byte words,
// each lane takes whole chunks with byte-addressed loads (16 / 8 / 4 bytes;
// the queues allow unaligned access), and a wave holds 64 / LPJ jobs of LPJ
// = min(64, chunks) lanes each, so a 4x4 job uses 4 lanes, not a wave.
struct U8Shape {
  int lw4;   // log2(w / 4)
  int lc;    // log2(words per chunk)
  int lcpr;  // log2(chunks per row)
  int lpj;   // lanes per job (power of two, <= 64)
  int chunks;
};

__device__ __forceinline__ void load_words(const uint8_t* p, int c, uint32_t (&w)[4]) {
  if (c == 4) {
    const u32x4u v = *(const __attribute__((address_space(1))) u32x4u*)p;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else if (c == 2) {
    const u32x2u v = *(const __attribute__((address_space(1))) u32x2u*)p;
    w[0] = v.x; w[1] = v.y; w[2] = 0; w[3] = 0;
  } else {
    w[0] = *(const __attribute__((address_space(1))) u32u*)p;
    w[1] = 0; w[2] = 0; w[3] = 0;
  }
}

// sum over the LPJ-lane group of a job (every lane of the group gets it)
__device__ __forceinline__ uint32_t group_sum(uint32_t v, int lpj) {
  for (int m = 1; m < lpj; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ void load_words16(const uint16_t* p, int c, uint32_t (&w)[4]) {
  load_words((const uint8_t*)p, c, w);
}

static int ilog2(int v) { return 31 - __builtin_clz(v); }

// the u16 word-chunk layout (2 samples per word, chunks of <= 8 samples)
static bool u16_shape(int w, int rows, U8Shape& sh) {
  if (w < 2 || (w & (w - 1)) || rows < 1 || (rows & (rows - 1))) return false;
  sh.lw4 = ilog2(w / 2);  // log2(words per row)
  sh.lc = sh.lw4 < 2 ? sh.lw4 : 2;
  sh.lcpr = sh.lw4 - sh.lc;
  sh.chunks = rows << sh.lcpr;
  sh.lpj = sh.chunks < 64 ? sh.chunks : 64;
  return true;
}

// the u8 word-chunk layout of a w x h block with `rows` rows read; false when
// w or rows is not a power of two >= 4 / >= 1
static bool u8_shape(int w, int rows, U8Shape& sh) {
  if (w < 4 || (w & (w - 1)) || rows < 1 || (rows & (rows - 1))) return false;
  sh.lw4 = ilog2(w / 4);
  sh.lc = sh.lw4 < 2 ? sh.lw4 : 2;
  sh.lcpr = sh.lw4 - sh.lc;
  sh.chunks = rows << sh.lcpr;
  sh.lpj = sh.chunks < 64 ? sh.chunks : 64;
  return true;
}

// the variance filters' 2-tap kernels (bilinear_filters_2t, aom_dsp/variance.h)
__device__ __forceinline__ int bil_tap(int off, int k) { return k ? 16 * off : 128 - 16 * off; }

}  // namespace lavish
