// subpel_dev.h -- what the sub-pel search kernels share (subpel.hip: the
// single-reference searches; subpel_comp.hip: the compound, masked and OBMC
// ones): the wave shape (Sp), the byte-window loads, the horizontal 8-tap
// pass, the wave reduction, the kernel tables and the best-mv record.
// Everything that reads a search's context (its Ctx, the per-segment errors,
// the mv costs) stays with its kernel.
#pragma once
#include "interp_kernels.h"
#include "lavish_internal.h"

namespace lavish {
namespace {

// [kind][phase][tap] (interp_kernels.h): 0 the 8-tap regular, 4 the 4-tap
// regular kernels (av1_get_filter's USE_8_TAPS / USE_4_TAPS)
__constant__ int16_t kUpK[6][16][8] = LAVISH_K8_INIT;

__constant__ uint8_t kBil2t[8][2] = {{128, 0}, {112, 16}, {96, 32}, {80, 48},
                                     {64, 64}, {48, 80},  {32, 96}, {16, 112}};

__device__ __forceinline__ uint32_t wave_total(uint32_t v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// 5 consecutive bytes at p as (dword of bytes 0..3, byte 4) from two
// dword-aligned loads
__device__ __forceinline__ void load5(const uint8_t* p, uint32_t& lo, uint32_t& hi) {
  typedef const __attribute__((address_space(1))) uint32_t* gptr;
  const uintptr_t a = (uintptr_t)p;
  const gptr q = (gptr)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t w0 = q[0], w1 = q[1];
  lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
  hi = (sh == 0 ? w1 : (w1 >> (8 * sh))) & 0xFF;
}

template <int W, int H>
struct Sp {
  static constexpr int SEG = W * H / 4;              // 4-pixel row segments
  static constexpr int NSEG = (SEG + 63) / 64;       // segments per lane
  static constexpr int SPR = W / 4;                  // segments per row
  // the job-invariant words (the source; second_pred and the mask in
  // subpel_comp.hip) live in VGPRs up to 8 per lane (64x32 / 32x64 and
  // smaller); larger blocks re-read them with the candidate rows
  static constexpr bool kCache = NSEG <= 8;
  static constexpr int NS = kCache ? NSEG : 1;
};

// 12 consecutive bytes at p as three dwords (dword-aligned loads + alignbyte)
__device__ __forceinline__ void load12(const uint8_t* p, uint32_t (&d)[3]) {
  typedef const __attribute__((address_space(1))) uint32_t* gptr;
  const uintptr_t a = (uintptr_t)p;
  const gptr q = (gptr)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
  d[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
  d[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
  d[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
}
__device__ __forceinline__ int byte_at(const uint32_t (&d)[3], int i) {
  return (d[i >> 2] >> (8 * (i & 3))) & 0xFF;
}
__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// aom_convolve8_horiz of 4 pixels: src bytes p[-3 .. 7]
__device__ __forceinline__ void hconv4(const uint8_t* p, const int (&k)[8], int (&o)[4]) {
  uint32_t d[3];
  load12(p - 3, d);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int sum = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) sum += byte_at(d, i + t) * k[t];
    o[i] = clip8((sum + 64) >> 7);  // ROUND_POWER_OF_TWO(sum, FILTER_BITS), clip_pixel
  }
}

struct Best {
  int row, col;
  uint32_t besterr, sse1;
  int distortion;
};

}  // namespace
}  // namespace lavish
