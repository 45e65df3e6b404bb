// conv_dev.h -- what the CONV_BUF convolutions (compound.hip, scale.hip,
// warp.hip) share: the rounding constants of a ConvolveParams with the
// compound finish, and the caller's filters as a kernel-argument table.
#pragma once
#include "lavish_internal.h"

namespace lavish {

constexpr int kFBits = 7;  // FILTER_BITS
constexpr int kMaxTaps = 12;

// the roundings of one ConvolveParams at one bit depth (convolve.c:306-313),
// by value in a kernel's arguments
struct ConvRound {
  int r0, r1, offset_bits, round_offset, round_bits, is_compound, do_average, dist_wtd, fwd, bck;
};

inline ConvRound conv_round(const LavishConvolveParams& cp, int bd) {
  ConvRound r{};
  r.r0 = cp.round_0;
  r.r1 = cp.round_1;
  r.offset_bits = bd + 2 * kFBits - cp.round_0;
  r.round_offset = (1 << (r.offset_bits - cp.round_1)) + (1 << (r.offset_bits - cp.round_1 - 1));
  r.round_bits = 2 * kFBits - cp.round_0 - cp.round_1;
  r.is_compound = cp.is_compound;
  r.do_average = cp.do_average;
  r.dist_wtd = cp.use_dist_wtd_comp_avg;
  r.fwd = cp.fwd_offset;
  r.bck = cp.bck_offset;
  return r;
}

// the compound second pass: the stored CONV_BUF value and this pass's res
// averaged (plain, or distance-weighted by DIST_PRECISION_BITS), the offset
// removed, rounded; the caller clips
__device__ __forceinline__ int conv_average(const ConvRound& r, int32_t stored, int32_t res) {
  int32_t t = r.dist_wtd ? (stored * r.fwd + res * r.bck) >> 4 : (stored + res) >> 1;
  t -= r.round_offset;
  return (t + ((1 << r.round_bits) >> 1)) >> r.round_bits;
}

// the 16 phases of the caller's two filters (av1_get_interp_filter_subpel_kernel
// rows), zero past the tap count
struct ConvTaps {
  int tx, ty;  // tap counts
  int16_t fx[16][kMaxTaps], fy[16][kMaxTaps];
};

// false: a tap count that is odd or outside 2..kMaxTaps, or a null row
inline bool conv_taps(const LavishInterpFilterParams* fpx, const LavishInterpFilterParams* fpy,
                      ConvTaps& t) {
  if (fpx->taps < 2 || fpx->taps > kMaxTaps || fpy->taps < 2 || fpy->taps > kMaxTaps ||
      (fpx->taps & 1) || (fpy->taps & 1) || !fpx->filter_ptr || !fpy->filter_ptr)
    return false;
  t.tx = fpx->taps;
  t.ty = fpy->taps;
  for (int p = 0; p < 16; ++p)
    for (int k = 0; k < kMaxTaps; ++k) {
      t.fx[p][k] = k < t.tx ? fpx->filter_ptr[t.tx * p + k] : 0;
      t.fy[p][k] = k < t.ty ? fpy->filter_ptr[t.ty * p + k] : 0;
    }
  return true;
}

}  // namespace lavish
