// quant_qm_dev.h -- device forms of the reference's quantization-matrix
// arithmetic, shared by the matrix quantizers (quant_qm.hip) and the matrix
// form of the trellis walk (trellis.hip).
//
// A matrix is a caller's device table of n = av1_get_max_eob(tx_size) bytes,
// raster-indexed like the reference's qm_ptr[rc]; nullptr is the flat level
// (weight 1 << AOM_QM_BITS).  None of quant_dev.h's 24-bit forms carry over:
// abs_coeff * wt * quant needs 64 bits and the weighted dequantizer no longer
// fits an int16.
#pragma once
#include "quant_dev.h"

namespace lavish {
namespace qm {

constexpr int kQmBits = 5;  // AOM_QM_BITS

__device__ __forceinline__ int weight(const uint8_t* m, int rc) {
  return m ? (int)m[rc] : 1 << kQmBits;
}

// (dequant * iwt + 16) >> 5: the helpers' `dequant` (av1_quantize.c:104-106,
// aom_dsp/quantize.c:160-162) and get_dqv (txb_rdopt_utils.h:39-46)
__device__ __forceinline__ int32_t weighted_dequant(int32_t dequant, int iwt) {
  return (dequant * iwt + (1 << (kQmBits - 1))) >> kQmBits;
}

// ROUND_POWER_OF_TWO(v, LS)
template <int LS>
__device__ __forceinline__ int32_t round_ls(int32_t v) {
  return (v + ((1 << LS) >> 1)) >> LS;
}

// The quantized magnitude (tmp32 / abs_qcoeff) of one coefficient through
// quantize_fp_helper_c / highbd_quantize_fp_helper_c (av1_quantize.c:70-198)
// with weight wt.  !HBD: clamp64 of |coeff| + round to int16 BEFORE the weight.
template <int LS, bool HBD>
__device__ __forceinline__ int32_t fp_mag(int32_t a, bool ac, const QP& qp, int wt) {
  const int32_t deq = ac ? qp.dequant[1] : qp.dequant[0];
  const int32_t rnd = round_ls<LS>(ac ? qp.round[1] : qp.round[0]);
  const int32_t qt = ac ? qp.quant[1] : qp.quant[0];
  if ((int64_t)a * wt < (deq << (kQmBits - (1 + LS)))) return 0;
  int64_t t = (int64_t)a + rnd;
  if constexpr (!HBD) t = t > 32767 ? 32767 : (t < -32768 ? -32768 : t);
  return (int32_t)((t * wt * qt) >> (16 - LS + kQmBits));
}

// aom_quantize_b_helper_c / aom_highbd_quantize_b_helper_c (aom_dsp/
// quantize.c:108-169, 261-316).  The pre-scan (lowbd: trailing run, highbd:
// index list) and the quantization pass test the same thing per coefficient,
// |coeff| * wt >= zbin * 32 as an int product, so one test serves both (the
// product is the reference's int multiply: exact for |coeff| < 2^23).
template <int LS, bool HBD>
__device__ __forceinline__ int32_t b_mag(int32_t a, bool ac, const QP& qp, int wt) {
  const int32_t zb = round_ls<LS>(ac ? qp.zbin[1] : qp.zbin[0]);
  const int32_t rnd = round_ls<LS>(ac ? qp.round[1] : qp.round[0]);
  const int32_t qt = ac ? qp.quant[1] : qp.quant[0];
  const int32_t qs = ac ? qp.quant_shift[1] : qp.quant_shift[0];
  if ((int32_t)((uint32_t)a * (uint32_t)wt) < zb * (1 << kQmBits)) return 0;
  int64_t t = (int64_t)(a + rnd);
  if constexpr (!HBD) t = t > 32767 ? 32767 : (t < -32768 ? -32768 : t);
  t *= wt;
  return (int32_t)(((((t * qt) >> 16) + t) * qs) >> (16 - LS + kQmBits));
}

// quantize_dc / highbd_quantize_dc (av1_quantize.c:374-405, 516-545): round =
// round_QTX[0], quant = quant_fp_QTX[0]
template <int LS, bool HBD>
__device__ __forceinline__ int32_t dc_mag(int32_t a, int32_t round0, int32_t quant0, int wt) {
  int64_t t = (int64_t)(a + round_ls<LS>(round0));
  if constexpr (!HBD) t = t > 32767 ? 32767 : (t < -32768 ? -32768 : t);
  return (int32_t)((t * wt * quant0) >> (16 - LS + kQmBits));
}

// (tmp32 * dequant) >> log_scale: an int multiply that wraps, on the signed
// magnitude (a negative per-call quant makes it negative; >> rounds down)
template <int LS>
__device__ __forceinline__ int32_t dequant_mag(int32_t mag, int32_t dequant_w) {
  return (int32_t)((uint32_t)mag * (uint32_t)dequant_w) >> LS;
}

// get_coeff_dist with the QM-PSNR matrix (txb_rdopt_utils.h:48-64)
__device__ __forceinline__ int64_t coeff_dist_qm(int32_t t, int32_t d, int shift, int wt) {
  int64_t diff = (int32_t)((t - d) * (1 << shift));
  diff *= wt;
  return (diff * diff + (1 << (2 * kQmBits - 1))) >> (2 * kQmBits);
}

// one term of av1_block_error_qm (tx_search.c:1049-1071)
__device__ __forceinline__ int64_t err_term_qm(int64_t v, int wt) {
  v *= wt;
  return (v * v + (1 << (2 * kQmBits - 1))) >> (2 * kQmBits);
}

}  // namespace qm
}  // namespace lavish
