/*
 * lavish_dsp_cfl.h -- the chroma-from-luma RTCD entries of liblavish_hip.so.
 *
 * The reference's nine CfL entries (av1/common/av1_rtcd_defs.pl:616-643) are
 * getters: each takes a TX_SIZE and returns a pointer to the function of that
 * size, NULL for the five sizes with a 64-point side.  They are declared here,
 * suffixed `_hip` like the shims of lavish_dsp.h, together with the 14
 * functions per family they return.  Those functions take the reference's
 * caller-owned HOST buffers (recon_buf_q3 / ac_buf_q3 at CFL_BUF_LINE stride)
 * and stage them through the library's device kernels: they are
 * lavish_cfl_subsample_host, lavish_cfl_subtract_average_host and
 * lavish_cfl_predict_host of lavish_dsp.h at a fixed size.  Drop-in parity, not
 * speed; the batch calls of lavish_dsp.h are the performance boundary.
 *
 * The function-pointer types are the reference's (av1_rtcd_defs.pl:59-74)
 * under names of this library; TX_SIZE is its uint8_t.
 */
#ifndef LAVISH_DSP_CFL_H_
#define LAVISH_DSP_CFL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void (*lavish_cfl_subsample_lbd_fn)(const uint8_t *input, int input_stride,
                                            uint16_t *output_q3);
typedef void (*lavish_cfl_subsample_hbd_fn)(const uint16_t *input, int input_stride,
                                            uint16_t *output_q3);
typedef void (*lavish_cfl_subtract_average_fn)(const uint16_t *src, int16_t *dst);
typedef void (*lavish_cfl_predict_lbd_fn)(const int16_t *src, uint8_t *dst, int dst_stride,
                                          int alpha_q3);
typedef void (*lavish_cfl_predict_hbd_fn)(const int16_t *src, uint16_t *dst, int dst_stride,
                                          int alpha_q3, int bd);

/* the 14 CfL sizes, in TX_SIZE order */
#define LAVISH_CFL_SIZES(X, a)                                                        \
  X(a, 4, 4) X(a, 8, 8) X(a, 16, 16) X(a, 32, 32) X(a, 4, 8) X(a, 8, 4) X(a, 8, 16)   \
  X(a, 16, 8) X(a, 16, 32) X(a, 32, 16) X(a, 4, 16) X(a, 16, 4) X(a, 8, 32) X(a, 32, 8)
#define LAVISH_CFL_SUBSAMPLINGS(X) \
  LAVISH_CFL_SIZES(X, 420) LAVISH_CFL_SIZES(X, 422) LAVISH_CFL_SIZES(X, 444)

#define LAVISH_CFL_DECL_SUBSAMPLE(sub, W, H)                                           \
  void cfl_subsample_lbd_##sub##_##W##x##H##_hip(const uint8_t *input, int input_stride, \
                                                 uint16_t *output_q3);                 \
  void cfl_subsample_hbd_##sub##_##W##x##H##_hip(const uint16_t *input, int input_stride, \
                                                 uint16_t *output_q3);
#define LAVISH_CFL_DECL_REST(a, W, H)                                                  \
  void cfl_subtract_average_##W##x##H##_hip(const uint16_t *src, int16_t *dst);         \
  void cfl_predict_lbd_##W##x##H##_hip(const int16_t *pred_buf_q3, uint8_t *dst,        \
                                       int dst_stride, int alpha_q3);                  \
  void cfl_predict_hbd_##W##x##H##_hip(const int16_t *pred_buf_q3, uint16_t *dst,       \
                                       int dst_stride, int alpha_q3, int bd);
LAVISH_CFL_SUBSAMPLINGS(LAVISH_CFL_DECL_SUBSAMPLE)
LAVISH_CFL_SIZES(LAVISH_CFL_DECL_REST, 0)
#undef LAVISH_CFL_DECL_SUBSAMPLE
#undef LAVISH_CFL_DECL_REST

/* av1_rtcd_defs.pl:616-643; NULL for TX_64X64, TX_32X64, TX_64X32, TX_16X64,
 * TX_64X16; tx_size is taken modulo TX_SIZES_ALL (19) as the reference does */
lavish_cfl_subtract_average_fn cfl_get_subtract_average_fn_hip(uint8_t tx_size);
lavish_cfl_subsample_lbd_fn cfl_get_luma_subsampling_420_lbd_hip(uint8_t tx_size);
lavish_cfl_subsample_lbd_fn cfl_get_luma_subsampling_422_lbd_hip(uint8_t tx_size);
lavish_cfl_subsample_lbd_fn cfl_get_luma_subsampling_444_lbd_hip(uint8_t tx_size);
lavish_cfl_subsample_hbd_fn cfl_get_luma_subsampling_420_hbd_hip(uint8_t tx_size);
lavish_cfl_subsample_hbd_fn cfl_get_luma_subsampling_422_hbd_hip(uint8_t tx_size);
lavish_cfl_subsample_hbd_fn cfl_get_luma_subsampling_444_hbd_hip(uint8_t tx_size);
lavish_cfl_predict_lbd_fn cfl_get_predict_lbd_fn_hip(uint8_t tx_size);
lavish_cfl_predict_hbd_fn cfl_get_predict_hbd_fn_hip(uint8_t tx_size);

#ifdef __cplusplus
}
#endif
#endif /* LAVISH_DSP_CFL_H_ */
