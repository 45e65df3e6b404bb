/*
 * lavish_dsp.h -- C ABI of liblavish_hip.so, the MI355X (gfx950) backend for
 * the per-block RDO hot path of aom-av1-lavish (a libaom v3.6.0 fork).
 *
 * Two layers:
 *
 *  1. Per-call RTCD shims.  Same prototypes as the reference's rtcd entries,
 *     suffixed `_hip`, so a maintainer can add `hip` as an RTCD arch
 *      and `specialize` these names.  They take the
 *     reference's caller-owned HOST buffers, stage them through a per-thread
 *     device scratch and run the same HIP kernels as the batch layer.  One
 *     block per call cannot amortise a kernel launch: these exist for drop-in
 *     parity, not speed.
 *
 *  2. Batch API (`lavish_*`).  Device pointers, asynchronous on a caller
 *     stream (hipStream_t passed as void*; NULL = default stream), a whole
 *     residual plane / candidate list per launch.  This is the performance
 *     boundary used by bench.py.
 *
 * Types follow the reference: tran_low_t == int32_t, tran_high_t == int64_t
 * (aom_dsp/aom_dsp_common.h:63-64); TX_SIZE / TX_TYPE are the uint8_t enums of
 * aom_dsp/txfm_common.h:25-71.  Highbd pixel pointers in the shims are the
 * reference's tagged pointers (CONVERT_TO_BYTEPTR, aom_ports/mem.h:79-80).
 *
 * Errors: the reference has no error channel; on a HIP failure the library
 * records a sticky status (lavish_hip_status) and, by default, prints the
 * failure and aborts.  There is no CPU fallback.
 */
#ifndef LAVISH_DSP_H_
#define LAVISH_DSP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Library state                                                            */
/* ------------------------------------------------------------------------ */
/* 0 when no HIP error has been seen, else the first hipError_t value. */
int lavish_hip_status(void);
const char *lavish_hip_status_string(void);
/* 1 (default): abort() on a HIP error; 0: record the status and continue. */
void lavish_hip_set_abort_on_error(int on);
/* Select the HIP device used by the per-call shims (default: current). */
int lavish_hip_init(int device);
/* ABI version: 0x00MMmmpp */
int lavish_hip_version(void);

/* TxfmParam of aom_dsp/txfm_common.h:89-101 (same field order / padding). */
typedef struct LavishTxfmParam {
  uint8_t tx_type;
  uint8_t tx_size;
  int lossless;
  int bd;
  int is_hbd;
  uint8_t tx_set_type;
  int eob;
} LavishTxfmParam;

/* ------------------------------------------------------------------------ */
/* Quantizer tables                                                         */
/* ------------------------------------------------------------------------ */
/* The two-entry ([0]=DC, [1]=AC) tables a quantizer reads, i.e. one row of
 * the reference's QUANTS/Dequants (av1/encoder/av1_quantize.h).  For the fp
 * quantizer `round`/`quant` hold round_fp/quant_fp.
 * The batch entry points (lavish_txq_plane / _frame / _frame_search with
 * LAVISH_QUANT_FP, every lavish_rdo_plane* / lavish_rdo_frame* call) take fp
 * rows with quant >= 0, dequant > 0 and quant * dequant <= 2^17 only, as
 * av1_build_quantizer makes them (quant_fp = 2^16 / dequant), and return -9
 * otherwise, nothing launched; LAVISH_QUANT_B rows and the per-call
 * quantizer shims take any int16. */
typedef struct LavishQuantParams {
  int16_t zbin[2];
  int16_t round[2];
  int16_t quant[2];
  int16_t quant_shift[2];
  int16_t dequant[2];
} LavishQuantParams;

enum { LAVISH_QUANT_FP = 0, LAVISH_QUANT_B = 1, LAVISH_QUANT_NONE = 2 };

/* av1_build_quantizer (av1/encoder/av1_quantize.c:590-686, including the
 * fork's quant_sharpness) for the luma plane at one qindex.
 * kind = LAVISH_QUANT_FP or LAVISH_QUANT_B selects which round/quant pair is
 * returned.  Returns 0 on success. */
int lavish_build_quant_params(int bit_depth, int qindex, int quant_sharpness,
                              int y_dc_delta_q, int kind,
                              LavishQuantParams *out);

/* av1_scan_orders[tx_size][tx_type] (av1/common/scan.c); host pointers. */
const int16_t *lavish_scan(int tx_size, int tx_type);
const int16_t *lavish_iscan(int tx_size, int tx_type);

/* ------------------------------------------------------------------------ */
/* Batch API (device pointers)                                              */
/* ------------------------------------------------------------------------ */
/* Forward transform + quantize every full tx_size block of a residual plane
 * for every TX type set in type_mask (the body of search_tx_type's per-type
 * loop, av1/encoder/tx_search.c:2148-2312: av1_xform -> av1_quant,
 * av1/encoder/encodemb.c:295-341).
 *   residual : int16 plane, `stride` elements per row, width x height.
 *   blocks   : B = (width / W) * (height / H), raster order (full blocks).
 *   tx_size  : any of the 19 sizes; the 64-point ones keep the reference's
 *              packed 32x32 (or 32x16 / 16x32) low-frequency quadrant.
 *   slots    : the set bits of type_mask in ascending TX_TYPE order; every
 *              set type must be valid for tx_size (EXT_TX_SET rules).
 *   outputs  : qcoeff/dqcoeff[slot][block][n], eob[slot][block], with
 *              n = av1_get_max_eob(tx_size); coeff (nullable) receives the
 *              unquantized transform output in the same layout.
 *   quant    : LAVISH_QUANT_FP (av1_quantize_fp*), LAVISH_QUANT_B
 *              (aom_quantize_b*), LAVISH_QUANT_NONE (transform only);
 *              log_scale = av1_get_tx_scale(tx_size); bit_depth > 8 selects
 *              the highbd quantizers.
 * Returns 0 on success, a negative value on invalid arguments. */
int lavish_txq_plane(const int16_t *residual, int stride, int width,
                     int height, int tx_size, uint32_t type_mask,
                     int bit_depth, int quant_kind,
                     const LavishQuantParams *qp, int32_t *qcoeff,
                     int32_t *dqcoeff, uint16_t *eob, int32_t *coeff,
                     void *stream);

/* Streams the per-size kernels of lavish_rdo_frame are dealt over: 1 .. 3
 * -- the caller's stream + streams - 1 internal streams, forked and joined
 * by events (default 3; 1: every size on the caller's stream, for isolated
 * per-kernel timings under a profiler).  Results are identical.  Returns -1
 * for other values.  No reference counterpart. */
int lavish_set_fan_width(int streams);

/* Frame batch: lavish_txq_plane for every TX size whose bit is set in
 * size_mask (bit = TX_SIZE), with type_masks[tx_size] and per-size output
 * pointers qcoeff[tx_size] / dqcoeff[tx_size] / eob[tx_size] (arrays of 19
 * entries, unused entries ignored).  The independent per-size kernels run
 * concurrently on internal streams forked from and joined back to `stream`;
 * the call is asynchronous with respect to the host like the others. */
int lavish_txq_frame(const int16_t *residual, int stride, int width,
                     int height, uint32_t size_mask,
                     const uint32_t *type_masks, int bit_depth,
                     int quant_kind, const LavishQuantParams *qp,
                     int32_t *const *qcoeff, int32_t *const *dqcoeff,
                     uint16_t *const *eob, void *stream);

/* Quantize `nblocks` coefficient blocks of n words each (contiguous) with one
 * scan order (device pointers to scan / iscan of n entries). */
int lavish_quantize_batch(const int32_t *coeff, int n, int nblocks,
                          const int16_t *scan, const int16_t *iscan,
                          int log_scale, int bit_depth, int quant_kind,
                          const LavishQuantParams *qp, int32_t *qcoeff,
                          int32_t *dqcoeff, uint16_t *eob, void *stream);

/* ---- av1_quant: quantizer selection ------------------
 * The tables av1_quant reads from MACROBLOCK_PLANE (*_QTX, [0] DC, [1] AC;
 * av1/encoder/block.h), as av1_build_quantizer fills them. */
typedef struct LavishPlaneQuant {
  int16_t zbin[2], round_fp[2], quant_fp[2], round[2], quant[2], quant_shift[2],
      dequant[2];
} LavishPlaneQuant;
int lavish_build_plane_quant(int bit_depth, int qindex, int quant_sharpness,
                             int y_dc_delta_q, LavishPlaneQuant *out);

/* xform_quant_idx (AV1_XFORM_QUANT, av1/encoder/encodemb.h) plus the
 * search_tx_type selection */
enum {
  LAVISH_AV1_QUANT_FP = 0,   /* av1_quantize_fp_facade / highbd */
  LAVISH_AV1_QUANT_B = 1,    /* av1_quantize_b_facade / highbd */
  LAVISH_AV1_QUANT_DC = 2,   /* av1_quantize_dc_facade / highbd */
  LAVISH_AV1_QUANT_SKIP = 3, /* AV1_XFORM_QUANT_SKIP_QUANT: outputs untouched */
  /* search_tx_type (tx_search.c:2140-2169): skip_trellis ? B : FP, then per
   * block skip_trellis_opt_based_on_satd (:1923-1955) -> B without trellis
   * when the satd gate fires, else FP with trellis */
  LAVISH_AV1_QUANT_SATD_GATE = 4
};

/* av1_quant (av1/encoder/encodemb.c:308-341) over nblocks contiguous blocks
 * of n = av1_get_max_eob(tx_size) coefficients (device): the facade of `mode`
 * (is_hbd = bit_depth > 8, log_scale of tx_size, scan of (tx_size, tx_type),
 * no quantization matrix) -> qcoeff / dqcoeff [nblocks][n], eob[nblocks].
 * SATD_GATE mode: skip_trellis, coeff_opt_satd_threshold
 * (coeff_opt_thresholds[1], UINT_MAX = off), qstep (dequant_QTX[1] >>
 * (hbd ? bd - 5 : 3)) and the optional per-block dc_only flags as the
 * reference passes them.  flags (device, nullable) [nblocks]: bit 0 =
 * use_optimize_b (the caller's trellis, av1_optimize_b, is still due for
 * these), bits 1-2 = the quantizer used.  Returns 0 or negative on bad
 * arguments. */
int lavish_av1_quant_batch(const int32_t *coeff, int nblocks, int tx_size,
                           int tx_type, int bit_depth, const LavishPlaneQuant *pq,
                           int mode, int skip_trellis,
                           unsigned coeff_opt_satd_threshold, int qstep,
                           const uint8_t *dc_only, int32_t *qcoeff, int32_t *dqcoeff,
                           uint16_t *eob, uint8_t *flags, void *stream);

/* ---- quantization matrices (av1_quant with using_qmatrix) ----------------
 * A matrix is a caller-supplied DEVICE table of n = av1_get_max_eob(tx_size)
 * uint8 weights, raster-indexed like the reference's qm_ptr[rc]: a slice of
 * the caller's copy of one [3344] level table (wt_matrix_ref / iwt_matrix_ref,
 * av1/common/quant_common.c) at lavish_qm_table_offset(tx_size).  NULL is the
 * flat level 15. */
/* aom_get_qmlevel (av1/common/quant_common.h:57-59); host. */
int lavish_qm_level(int qindex, int first, int last);
/* Element offset, inside one [3344] level table, of the matrix of
 * av1_get_adjusted_tx_size(tx_size) as av1_qm_init lays the sizes out
 * (quant_common.c:283-309); the 64-point sizes return the offset of the size
 * whose matrix they reuse.  -1 for a bad size; host. */
int lavish_qm_table_offset(int tx_size);

/* lavish_quantize_batch through the *_helper_c bodies (quantize_fp_helper_c /
 * highbd_quantize_fp_helper_c, av1/encoder/av1_quantize.c:70-198;
 * aom_[highbd_]quantize_b_helper_c, aom_dsp/quantize.c:108-169,261-316):
 * qm / iqm (device, n entries) each nullable on its own.  bit_depth 8 / 10 /
 * 12.  Returns 0 or negative on bad arguments, nothing launched. */
int lavish_quantize_qm_batch(const int32_t *coeff, int n, int nblocks,
                             const int16_t *scan, const int16_t *iscan,
                             int log_scale, int bit_depth, int quant_kind,
                             const LavishQuantParams *qp, const uint8_t *qm,
                             const uint8_t *iqm, int32_t *qcoeff,
                             int32_t *dqcoeff, uint16_t *eob, void *stream);

/* lavish_av1_quant_batch with the block's matrices and an optional fused
 * dist_block_tx_domain (tx_search.c:1073-1116).
 *   qm / iqm : as av1_setup_qmatrix would hand them for a 2-D type; for
 *              tx_type >= IDTX they are treated as NULL here (av1_get_qmatrix,
 *              quant_common.c:249-275).  FP / B / SATD_GATE take the helper
 *              bodies only when both are non-NULL (av1_quantize.c:272,344 and
 *              the highbd facades) and write lavish_av1_quant_batch's bits
 *              otherwise; DC weights with each pointer on its own
 *              (quantize_dc, :374-405).
 *   dist_mode: 0 none; 1 av1_block_error / av1_highbd_block_error; 2
 *              use_qm_dist_metric: av1_block_error_qm (:1049-1071, no bd
 *              shift) when the effective qm is non-NULL, else as 1.  1 and 2
 *              write dist / sse [nblocks] (device int64), RIGHT_SIGNED_SHIFT
 *              by (MAX_TX_SCALE - tx_scale) * 2 included.  SKIP mode leaves
 *              qcoeff / dqcoeff / eob untouched and measures the dqcoeff found.
 * Returns 0, or negative, nothing launched: -1 size / type, -2 depth, -3
 * mode, -4 NULL pointer, -5 dist_mode, -6 dist / sse NULL with dist_mode > 0. */
int lavish_av1_quant_qm_batch(const int32_t *coeff, int nblocks, int tx_size,
                              int tx_type, int bit_depth,
                              const LavishPlaneQuant *pq, int mode,
                              int skip_trellis,
                              unsigned coeff_opt_satd_threshold, int qstep,
                              const uint8_t *dc_only, const uint8_t *qm,
                              const uint8_t *iqm, int dist_mode,
                              int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob,
                              uint8_t *flags, int64_t *dist, int64_t *sse,
                              void *stream);

/* av1_block_error_qm (tx_search.c:1049-1071) for nblocks blocks of n words:
 * sum over i of ((coeff[i] - dqcoeff[i]) * qmatrix[scan[i]])^2, rounded >> 10
 * per term, into err [nblocks], and the same of coeff[i] into ssz (device
 * int64; no shift applied).  qmatrix / scan: device, n entries. */
int lavish_block_error_qm_batch(const int32_t *coeff, const int32_t *dqcoeff,
                                int n, int nblocks, const uint8_t *qmatrix,
                                const int16_t *scan, int64_t *err,
                                int64_t *ssz, void *stream);

/* ---- coefficient rate ---------------------------- */
/* MACROBLOCK::coeff_costs, field for field (CoeffCosts, av1/encoder/block.h:
 * 172-211): LV_MAP_COEFF_COST per [txs_ctx][plane_type] and LV_MAP_EOB_COST
 * per [eob_multi_size][plane_type], as av1_fill_coeff_costs leaves them (the
 * caller copies x->coeff_costs to the device once per frame / cdf update). */
typedef struct LavishCoeffCost {
  int32_t txb_skip_cost[13][2];  /* TXB_SKIP_CONTEXTS */
  int32_t base_eob_cost[4][3];   /* SIG_COEF_CONTEXTS_EOB */
  int32_t base_cost[42][8];      /* SIG_COEF_CONTEXTS */
  int32_t eob_extra_cost[9][2];  /* EOB_COEF_CONTEXTS */
  int32_t dc_sign_cost[3][2];    /* DC_SIGN_CONTEXTS */
  int32_t lps_cost[21][26];      /* LEVEL_CONTEXTS x (COEFF_BASE_RANGE + 1) * 2 */
} LavishCoeffCost;
typedef struct LavishEobCost {
  int32_t eob_cost[2][11];
} LavishEobCost;
typedef struct LavishCoeffCosts {
  LavishCoeffCost coeff_costs[5][2]; /* [TX_SIZES][PLANE_TYPES] */
  LavishEobCost eob_costs[7][2];
} LavishCoeffCosts;
/* TXB_CTX (av1/common/txb_common.h:22-25) */
typedef struct LavishTxbCtx {
  int32_t txb_skip_ctx; /* 0..12 */
  int32_t dc_sign_ctx;  /* 0..2 */
} LavishTxbCtx;

enum {
  LAVISH_COEFF_RATE_EXACT = 0,    /* av1_cost_coeffs_txb (txb_rdopt.c:599-624) */
  LAVISH_COEFF_RATE_LAPLACIAN = 1 /* av1_cost_coeffs_txb_laplacian, adjust_eob 0 */
};

/* Replaces av1_cost_coeffs_txb / av1_cost_coeffs_txb_laplacian (av1/encoder/
 * txb_rdopt.c:599-660; cost_coeffs, tx_search.c:1903-1921, is the caller) for
 * nblocks blocks of one (tx_size, tx_type, plane): qcoeff [nblocks][n], n =
 * av1_get_max_eob(tx_size), raster order as the quantizer writes it (the kept
 * 32x32 quadrant for 64-point sizes); eob [nblocks] = p->eobs (the scan
 * position after the last nonzero coefficient, as the quantizers return it);
 * costs / txb_ctx (nullable: all {0, 0}) / rate [nblocks] on the device;
 * tx_type_cost = get_tx_type_cost's value (txb_rdopt.c:263-294; a
 * MACROBLOCK-level table lookup the caller owns), added for plane 0 when
 * eob > 0.  Returns 0 or negative on bad arguments. */
int lavish_cost_coeffs_txb_batch(const LavishCoeffCosts *costs, const int32_t *qcoeff,
                                 const uint16_t *eob, int nblocks, int plane, int tx_size,
                                 int tx_type, const LavishTxbCtx *txb_ctx, int tx_type_cost,
                                 int mode, int32_t *rate, void *stream);

/* Replaces av1_optimize_b (av1/encoder/encodemb.c:87-103) -> av1_optimize_txb
 * (txb_rdopt.c:326-449), the trellis search_tx_type runs on FP-quantized
 * blocks flagged use_optimize_b, for nblocks blocks of one (tx_size,
 * tx_type, plane), no quantization matrix.  Device arrays [nblocks][n] (n =
 * av1_get_max_eob): tcoeff (p->coeff) in; qcoeff / dqcoeff updated in place;
 * eob [nblocks] in / out; txb_ctx nullable ({0, 0}); rate [nblocks] out
 * (rate_cost, incl. the skip / non-skip and tx-type cost); entropy_ctx
 * [nblocks] out, nullable (p->txb_entropy_ctx = av1_get_txb_entropy_context).
 * rdmult = x->rdmult, is_inter = is_inter_block, sharpness =
 * oxcf.algo_cfg.sharpness, dequant = p->dequant_QTX[0..1] (host).  eob 0:
 * rate = txb_skip_cost[ctx][1] (the early exit; segments with
 * optimize_seg_arr 0 or lossless are the caller's to skip).  Returns 0 or
 * negative on bad arguments. */
int lavish_optimize_b_batch(const LavishCoeffCosts *costs, const int32_t *tcoeff,
                            int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob, int nblocks,
                            int plane, int tx_size, int tx_type, int bit_depth, int is_inter,
                            int rdmult, int sharpness, const int16_t *dequant,
                            const LavishTxbCtx *txb_ctx, int tx_type_cost, int32_t *rate,
                            uint8_t *entropy_ctx, void *stream);

/* lavish_optimize_b_batch with the block's matrices (device, n entries,
 * raster): iqm weights get_dqv per coefficient (txb_rdopt_utils.h:39-46;
 * NULL: flat); qm_dist is the matrix of get_coeff_dist under
 * AOM_DIST_METRIC_QM_PSNR (:48-64; NULL: the default metric).  Both are
 * treated as NULL for tx_type >= IDTX.  With both NULL the results are
 * lavish_optimize_b_batch's. */
int lavish_optimize_b_qm_batch(const LavishCoeffCosts *costs, const int32_t *tcoeff,
                               int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob,
                               int nblocks, int plane, int tx_size, int tx_type,
                               int bit_depth, int is_inter, int rdmult, int sharpness,
                               const int16_t *dequant, const uint8_t *iqm,
                               const uint8_t *qm_dist, const LavishTxbCtx *txb_ctx,
                               int tx_type_cost, int32_t *rate, uint8_t *entropy_ctx,
                               void *stream);

/* ---- pixel-domain batch kernels ----------------------------------------- */
/* One job = one block.  Offsets are in ELEMENTS (u8 or u16 samples / int16
 * residual words) from the plane base pointers passed to the call.  Which
 * fields a kernel reads is stated per call. */
typedef struct LavishPixJob {
  int64_t src_off;    /* first operand (src) */
  int64_t ref_off[4]; /* second operand(s): ref / candidate positions */
  int64_t aux_off;    /* second_pred / diff / coefficient offset */
  int32_t xoff, yoff; /* sub-pixel offsets (1/8 pel, 0..7) */
} LavishPixJob;

/* SAD of a w x h block against nrefs (1..4) reference positions
 * (aom_dsp/sad.c:22-129, highbd :240-330).
 *   mode 0: aom_sad, 1: aom_sad_skip (2 x SAD of even rows),
 *        2: aom_sad_avg against ROUND_POWER_OF_TWO(ref + second_pred, 1)
 *           with second_pred at second_pred + job.aux_off, stride w.
 *   highbd: 0 = u8 planes, 1 = u16 planes (plain device pointers).
 *   sad_out[job * nrefs + k]. */
int lavish_sad_batch(const void *src, int src_stride, const void *ref,
                     int ref_stride, int w, int h, const LavishPixJob *jobs,
                     int njobs, int nrefs, int mode, const void *second_pred,
                     int highbd, uint32_t *sad_out, void *stream);

/* Variance family, d = a[src_off] - b[ref_off[0]]
 * (aom_dsp/variance.c:38-145,321-408,454-670).
 *   kind 0: variance (var_out, sse_out), 1: mse (var_out = sse),
 *        2: get_var (sse_out, sum_out), 3: sub-pixel variance of the
 *        bilinear-filtered a (job.xoff/yoff; reads (h+1) x (w+1) of a),
 *        4: sse as int64 (aom_sse / aom_highbd_sse; sse64_out),
 *        5: sub-pixel avg variance (second_pred + job.aux_off, stride w).
 *   bit_depth 8/10/12 selects the highbd rounding (highbd = 1 only).
 * Unused output pointers may be NULL. */
int lavish_variance_batch(const void *a, int a_stride, const void *b,
                          int b_stride, int w, int h, const LavishPixJob *jobs,
                          int njobs, int kind, int bit_depth, int highbd,
                          const void *second_pred, uint32_t *var_out,
                          uint32_t *sse_out, int32_t *sum_out,
                          int64_t *sse64_out, void *stream);

/* diff[aux_off + r*diff_stride + c] = src[src_off..] - pred[ref_off[0]..]
 * (aom_subtract_block / aom_highbd_subtract_block, aom_dsp/subtract.c). */
int lavish_subtract_batch(int rows, int cols, int16_t *diff, int diff_stride,
                          const void *src, int src_stride, const void *pred,
                          int pred_stride, const LavishPixJob *jobs,
                          int njobs, int highbd, void *stream);

/* aom_sum_squares_2d_i16 (aom_dsp/sum_squares.c:16-30) at src + src_off. */
int lavish_sum_squares_batch(const int16_t *src, int stride, int w, int h,
                             const LavishPixJob *jobs, int njobs,
                             uint64_t *out, void *stream);

/* aom_hadamard_{4x4,8x8,16x16,32x32} (highbd = 0) and
 * aom_highbd_hadamard_{8x8,16x16,32x32} (highbd = 1), aom_dsp/avg.c:102-507:
 * src_diff + job.src_off (stride) -> coeff + job.aux_off (n*n words). */
int lavish_hadamard_batch(int n, int highbd, const int16_t *src_diff,
                          int stride, const LavishPixJob *jobs, int njobs,
                          int32_t *coeff, void *stream);

/* aom_satd (aom_dsp/avg.c:509-516) of nblocks contiguous blocks. */
int lavish_satd_batch(const int32_t *coeff, int length, int nblocks, int *out,
                      void *stream);

/* av1_block_error (bit_depth 0) / av1_highbd_block_error (bit_depth 8/10/12)
 * (av1/encoder/rdopt.c:635-682) of nblocks contiguous blocks of n words. */
int lavish_block_error_batch(const int32_t *coeff, const int32_t *dqcoeff,
                             int n, int nblocks, int bit_depth, int64_t *err,
                             int64_t *ssz, void *stream);

/* aom_hadamard_lp_{8x8,16x16} (aom_dsp/avg.c:207-316): int16 coefficients
 * (n = 8 or 16, else -1). */
int lavish_hadamard_lp_batch(int n, const int16_t *src_diff, int stride,
                             const LavishPixJob *jobs, int njobs,
                             int16_t *coeff, void *stream);
/* aom_satd_lp (aom_dsp/avg.c:518-524) of nblocks contiguous int16 blocks. */
int lavish_satd_lp_batch(const int16_t *coeff, int length, int nblocks,
                         int *out, void *stream);
/* av1_block_error_lp (av1/encoder/rdopt.c:650-660). */
int lavish_block_error_lp_batch(const int16_t *coeff, const int16_t *dqcoeff,
                                int n, int nblocks, int64_t *err,
                                void *stream);
/* (sum, sum of squares) of a w x h int16 block at src + job.src_off:
 * aom_sum_sse_2d_i16 (aom_dsp/sum_squares.c:75-90) and aom_get_blk_sse_sum
 * (aom_dsp/blk_sse_sum.c:14-27).  Either output may be NULL. */
int lavish_sum_sse_batch(const int16_t *src, int stride, int w, int h,
                         const LavishPixJob *jobs, int njobs, int32_t *sum,
                         int64_t *sse, void *stream);

/* ---- compound pixel kernels: masked, OBMC, distance-weighted -------------
 * The msdf / msvf / osdf / ovf / osvf / jsdaf / jsvaf members of
 * aom_variance_fn_ptr_t (aom_dsp/variance.h:84-103) and the prediction
 * helpers they reduce to.  One job = one block; offsets in ELEMENTS of the
 * array they index.  (w, h) must be one of the 22 encoder block sizes.
 *   blend      AOM_BLEND_A64(m, a, b) = (m*a + (64-m)*b + 32) >> 6
 *   dist-wtd   (second*bck_offset + ref*fwd_offset + 8) >> 4, with
 *              fwd_offset >= 0, bck_offset >= 0, fwd_offset + bck_offset == 16
 *              (quant_dist_lookup_table, av1/common/common_data.h:421-426)
 * Every call returns 0 for njobs <= 0 and a negative value, before any
 * device work, for arguments it does not take.  The job record is 72 bytes. */
typedef struct LavishCompJob {
  int64_t src_off;     /* source block (comp_pred block for the pred call)        */
  int64_t ref_off[4];  /* reference / predictor positions                          */
  int64_t second_off;  /* second_pred block, stride w; OBMC: wsrc block (int32)    */
  int64_t mask_off;    /* u8 mask block (mask_stride); OBMC: int32 mask block      */
  int32_t xoff, yoff;  /* 1/8-pel bilinear offsets, 0..7                           */
  int32_t invert_mask; /* masked modes: nonzero swaps the blend operands           */
  int32_t reserved;
} LavishCompJob;

/* SAD of src against the compound prediction of each of nrefs (1..4) refs.
 *   mode 0: masked (aom_dsp/sad_av1.c:21-67, highbd :95-133):
 *           invert_mask == 0 -> blend(mask, ref, second_pred), else
 *           blend(mask, second_pred, ref);
 *        1: distance-weighted average (aom_dsp/sad.c:57-64, highbd :290-298).
 *   sad_out[job * nrefs + k]. */
int lavish_comp_sad_batch(const void *src, int src_stride, const void *ref,
                          int ref_stride, int w, int h,
                          const LavishCompJob *jobs, int njobs, int nrefs,
                          int mode, const void *second_pred,
                          const uint8_t *mask, int mask_stride, int fwd_offset,
                          int bck_offset, int highbd, uint32_t *sad_out,
                          void *stream);

/* Variance of (bilinear-filtered a + job.src_off, reading (h+1) x (w+1),
 * combined with second_pred) against b + job.ref_off[0].
 *   kind 0: masked sub-pixel variance (aom_dsp/variance.c:749-814, highbd
 *           :817-929), 1: distance-weighted sub-pixel avg variance
 *           (variance.c:165-181, highbd to :664).
 *   bit_depth 8/10/12 selects the highbd rounding (highbd = 1 only).
 * Either output may be NULL. */
int lavish_comp_variance_batch(const void *a, int a_stride, const void *b,
                               int b_stride, int w, int h,
                               const LavishCompJob *jobs, int njobs, int kind,
                               int bit_depth, int highbd,
                               const void *second_pred, const uint8_t *mask,
                               int mask_stride, int fwd_offset, int bck_offset,
                               uint32_t *var_out, uint32_t *sse_out,
                               void *stream);

/* OBMC: wsrc + job.second_off and mask + job.mask_off are contiguous w x h
 * int32 blocks; pre + job.ref_off[k] is the predictor.
 *   kind 0: SAD (aom_dsp/sad_av1.c:163-186, highbd :215-239) against npre
 *           (1..4) predictors, out[job * npre + k];
 *        1: variance (aom_dsp/variance.c:933-961, highbd :1040-1123),
 *           out[job] = variance, sse_out[job] (may be NULL);
 *        2: as 1 on the bilinear-filtered predictor (job.xoff / yoff).
 *   npre must be 1 unless kind is 0. */
int lavish_obmc_batch(const void *pre, int pre_stride, int w, int h,
                      const LavishCompJob *jobs, int njobs, int npre, int kind,
                      int bit_depth, int highbd, const int32_t *wsrc,
                      const int32_t *mask, uint32_t *out, uint32_t *sse_out,
                      void *stream);

/* comp_pred + job.src_off (contiguous w x h) from pred + job.second_off
 * (contiguous w x h) and ref + job.ref_off[0] (ref_stride).
 *   mode 0: aom_comp_avg_pred, 1: aom_dist_wtd_comp_avg_pred,
 *        2: aom_comp_mask_pred (invert_mask == 0 -> blend(mask, ref, pred))
 *   (aom_dsp/variance.c:285-318, 707-767, 817-837).  Jobs of one call must not
 *   overlap in comp_pred. */
int lavish_comp_pred_batch(void *comp_pred, const void *pred, int w, int h,
                           const void *ref, int ref_stride,
                           const LavishCompJob *jobs, int njobs, int mode,
                           const uint8_t *mask, int mask_stride,
                           int fwd_offset, int bck_offset, int highbd,
                           void *stream);

/* ---- mask building and blending: a64 blends, diff-weighted masks, OBMC ----
 * What lies between the first-pass convolves and the compound / OBMC
 * searches above: the blends of av1_make_masked_inter_predictor and
 * av1_build_obmc_inter_prediction, the DIFFWTD masks, the wsrc / mask streams
 * lavish_obmc_batch and the OBMC searches read, and the residual reductions
 * pick_wedge / pick_interinter_seg choose a mask with.  One job = one block;
 * offsets in ELEMENTS of the array they index; device pointers; asynchronous
 * on `stream`.  Every call returns 0 for njobs <= 0 and a negative value,
 * before any device work, for arguments it does not take.
 * conv_params (a host struct, read before the call returns): round_0 and
 * round_1 only, as the first pass that filled the d16 buffers had them. */
typedef struct LavishConvolveParams LavishConvolveParams;

/* dst + job.src_off = blend of src0 + job.ref_off[0] and src1 + job.ref_off[1]
 * under mask + job.mask_off, each with its own stride; w, h powers of two,
 * 1..128 (4..128 with d16).
 *   kind 0: 2-D mask, aom_blend_a64_mask / aom_highbd_blend_a64_mask
 *           (aom_dsp/blend_a64_mask.c:229-349); subw / subh (0 or 1): the mask
 *           is twice as wide / high and is averaged down (both: the rounded
 *           mean of 2x2, one: AOM_BLEND_AVG of the pair); mask_stride >=
 *           w << subw.  With d16 the inputs are CONV_BUF_TYPE (uint16) blocks
 *           and dst is u8 (highbd 0) or u16: aom_lowbd_blend_a64_d16_mask /
 *           aom_highbd_blend_a64_d16_mask (blend_a64_mask.c:36-223).
 *        1: mask[x], aom_[highbd_]blend_a64_hmask (blend_a64_hmask.c:21-70);
 *        2: mask[y], aom_[highbd_]blend_a64_vmask (blend_a64_vmask.c:21-70).
 *   highbd: u16 pixels, bit_depth 8 / 10 / 12; else u8 and bit_depth 8.
 * dst may be src0 or src1 when the strides are equal (in place); otherwise
 * the jobs' dst blocks must not overlap any block the call reads. */
int lavish_blend_a64_batch(void *dst, int dst_stride, const void *src0,
                           int src0_stride, const void *src1, int src1_stride,
                           const uint8_t *mask, int mask_stride, int w, int h,
                           const LavishCompJob *jobs, int njobs, int kind,
                           int subw, int subh, int d16, int highbd,
                           int bit_depth,
                           const LavishConvolveParams *conv_params,
                           void *stream);

/* mask + job.mask_off (contiguous w x h) from src0 + job.ref_off[0] and src1 +
 * job.ref_off[1]; job.invert_mask 0: DIFFWTD_38, else DIFFWTD_38_INV.
 * av1_build_compound_diffwtd_mask (u8), _highbd (highbd 1: u16, the
 * difference >> (bit_depth - 8) first) and _d16 (d16 1: CONV_BUF_TYPE, the
 * difference rounded by 2 * FILTER_BITS - round_0 - round_1 + bit_depth - 8)
 * (av1/common/reconinter.c:296-439).  w, h powers of two, 4..128. */
int lavish_diffwtd_mask_batch(uint8_t *mask, const void *src0, int src0_stride,
                              const void *src1, int src1_stride, int w, int h,
                              const LavishCompJob *jobs, int njobs, int d16,
                              int highbd, int bit_depth,
                              const LavishConvolveParams *conv_params,
                              void *stream);

/* The OBMC pair.  The neighbour walk (foreach_overlappable_nb_above / _left,
 * av1/common/obmc.h:20-87) needs mode info and stays with the caller; a job
 * carries its result as two bitmaps: bit k of above_mask (left_mask) is set
 * when mi column (row) k of the block lies in the span of a neighbour the
 * walk visited (128 pixels = 32 bits).  above + job.above_off and left +
 * job.left_off address the neighbours' predictions at the block's own
 * top-left (pixel (x, y) of the block is at off + y * stride + x); only the
 * pixels the bitmaps select are read.  obmc_masks: a 127-byte device table,
 * av1_get_obmc_mask(n) for n = 1, 2, 4 .. 64 back to back (length n starts
 * at byte n - 1).  (bw, bh): an encoder block size of at least 8x8.  The
 * record is 48 bytes. */
typedef struct LavishObmcJob {
  int64_t src_off;    /* source block; the blend call: the dst block              */
  int64_t above_off;  /* above prediction at the block's top-left                 */
  int64_t left_off;   /* left prediction at the block's top-left                  */
  int64_t wsrc_off;   /* int32 wsrc block, contiguous bw x bh (wsrc call only)    */
  int64_t mask_off;   /* int32 mask block, contiguous bw x bh (wsrc call only)    */
  uint32_t above_mask, left_mask;
} LavishObmcJob;

/* calc_target_weighted_pred (av1/encoder/rdopt.c:6362-6580): the wsrc and
 * mask blocks lavish_obmc_batch and the OBMC searches read. */
int lavish_obmc_wsrc_batch(const void *src, int src_stride, const void *above,
                           int above_stride, const void *left, int left_stride,
                           int bw, int bh, const LavishObmcJob *jobs, int njobs,
                           const uint8_t *obmc_masks, int highbd, int32_t *wsrc,
                           int32_t *mask, void *stream);

/* av1_build_obmc_inter_prediction (av1/common/reconinter.c:844-945) on one
 * plane, in place on dst + job.src_off: (bw, bh) is the luma block size and
 * the plane's block is (bw >> subsampling_x) x (bh >> subsampling_y), with
 * the halved spans and overlaps and av1_skip_u4x4_pred_in_obmc
 * (reconinter.c:812-830).  Offsets and strides are the plane's. */
int lavish_obmc_blend_batch(void *dst, int dst_stride, const void *above,
                            int above_stride, const void *left, int left_stride,
                            int bw, int bh, int subsampling_x, int subsampling_y,
                            const LavishObmcJob *jobs, int njobs,
                            const uint8_t *obmc_masks, int highbd, void *stream);

/* The residual reductions of pick_wedge / pick_interinter_seg
 * (av1/encoder/wedge_utils.c:52-125) over job.n contiguous elements, n a
 * multiple of 64 in 64 .. 16384.  The record is 48 bytes.
 *   kind 0: av1_wedge_compute_delta_squares: (int16_t *)out + job.out_off =
 *           clamp(a^2 - b^2, INT16_MIN, INT16_MAX);
 *        1: av1_wedge_sse_from_residuals: a = r1, b = d;
 *           ((uint64_t *)out)[job] = ROUND_POWER_OF_TWO(sum of
 *           clamp(64 * r1 + m * d, INT16_MIN, INT16_MAX)^2, 12);
 *        2: av1_wedge_sign_from_residuals: a = ds (b unused);
 *           ((int8_t *)out)[job] = sum of ds * m > job.limit. */
typedef struct LavishWedgeJob {
  int64_t a_off;    /* r1 / ds / a                                                */
  int64_t b_off;    /* d / b                                                      */
  int64_t m_off;    /* u8 mask (kinds 1, 2)                                       */
  int64_t out_off;  /* kind 0: the d block                                        */
  int64_t limit;    /* kind 2                                                     */
  int32_t n;
  int32_t reserved;
} LavishWedgeJob;
int lavish_wedge_batch(const int16_t *a, const int16_t *b, const uint8_t *m,
                       const LavishWedgeJob *jobs, int njobs, int kind,
                       void *out, void *stream);

/* Per-call shims (host buffers) with the reference's prototypes; highbd pixel
 * pointers arrive tagged (CONVERT_TO_BYTEPTR).
 * aom_dsp/aom_dsp_rtcd_defs.pl:701 */
void aom_lowbd_blend_a64_d16_mask_hip(uint8_t *dst, uint32_t dst_stride,
                                      const uint16_t *src0, uint32_t src0_stride,
                                      const uint16_t *src1, uint32_t src1_stride,
                                      const uint8_t *mask, uint32_t mask_stride,
                                      int w, int h, int subw, int subh,
                                      LavishConvolveParams *conv_params);
/* aom_dsp_rtcd_defs.pl:703 */
void aom_blend_a64_mask_hip(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0,
                            uint32_t src0_stride, const uint8_t *src1,
                            uint32_t src1_stride, const uint8_t *mask,
                            uint32_t mask_stride, int w, int h, int subw, int subh);
/* aom_dsp_rtcd_defs.pl:704 */
void aom_blend_a64_hmask_hip(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0,
                             uint32_t src0_stride, const uint8_t *src1,
                             uint32_t src1_stride, const uint8_t *mask, int w, int h);
/* aom_dsp_rtcd_defs.pl:705 */
void aom_blend_a64_vmask_hip(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0,
                             uint32_t src0_stride, const uint8_t *src1,
                             uint32_t src1_stride, const uint8_t *mask, int w, int h);
/* aom_dsp_rtcd_defs.pl:711 */
void aom_highbd_blend_a64_mask_hip(uint8_t *dst, uint32_t dst_stride,
                                   const uint8_t *src0, uint32_t src0_stride,
                                   const uint8_t *src1, uint32_t src1_stride,
                                   const uint8_t *mask, uint32_t mask_stride, int w,
                                   int h, int subw, int subh, int bd);
/* aom_dsp_rtcd_defs.pl:712 */
void aom_highbd_blend_a64_hmask_hip(uint8_t *dst, uint32_t dst_stride,
                                    const uint8_t *src0, uint32_t src0_stride,
                                    const uint8_t *src1, uint32_t src1_stride,
                                    const uint8_t *mask, int w, int h, int bd);
/* aom_dsp_rtcd_defs.pl:713 */
void aom_highbd_blend_a64_vmask_hip(uint8_t *dst, uint32_t dst_stride,
                                    const uint8_t *src0, uint32_t src0_stride,
                                    const uint8_t *src1, uint32_t src1_stride,
                                    const uint8_t *mask, int w, int h, int bd);
/* aom_dsp_rtcd_defs.pl:714 */
void aom_highbd_blend_a64_d16_mask_hip(uint8_t *dst, uint32_t dst_stride,
                                       const uint16_t *src0, uint32_t src0_stride,
                                       const uint16_t *src1, uint32_t src1_stride,
                                       const uint8_t *mask, uint32_t mask_stride,
                                       int w, int h, int subw, int subh,
                                       LavishConvolveParams *conv_params,
                                       const int bd);
/* av1/common/av1_rtcd_defs.pl:257 (mask_type: DIFFWTD_MASK_TYPE, a uint8_t) */
void av1_build_compound_diffwtd_mask_hip(uint8_t *mask, uint8_t mask_type,
                                         const uint8_t *src0, int src0_stride,
                                         const uint8_t *src1, int src1_stride, int h,
                                         int w);
/* av1_rtcd_defs.pl:261 */
void av1_build_compound_diffwtd_mask_highbd_hip(uint8_t *mask, uint8_t mask_type,
                                                const uint8_t *src0, int src0_stride,
                                                const uint8_t *src1, int src1_stride,
                                                int h, int w, int bd);
/* av1_rtcd_defs.pl:265 */
void av1_build_compound_diffwtd_mask_d16_hip(uint8_t *mask, uint8_t mask_type,
                                             const uint16_t *src0, int src0_stride,
                                             const uint16_t *src1, int src1_stride,
                                             int h, int w,
                                             LavishConvolveParams *conv_params, int bd);
/* av1_rtcd_defs.pl:440 */
uint64_t av1_wedge_sse_from_residuals_hip(const int16_t *r1, const int16_t *d,
                                          const uint8_t *m, int N);
/* av1_rtcd_defs.pl:442 */
int8_t av1_wedge_sign_from_residuals_hip(const int16_t *ds, const uint8_t *m, int N,
                                         int64_t limit);
/* av1_rtcd_defs.pl:444 */
void av1_wedge_compute_delta_squares_hip(int16_t *d, const int16_t *a,
                                         const int16_t *b, int N);

/* ---- lossless 4x4 Walsh-Hadamard ----------------------------------------
 * av1_fwht4x4 (hybrid_fwd_txfm.c:24-76): src_diff + job.src_off (stride) ->
 * 16 words at coeff + job.aux_off. */
int lavish_fwht4x4_batch(const int16_t *src_diff, int stride,
                         const LavishPixJob *jobs, int njobs, int32_t *coeff,
                         void *stream);

/* ---- inverse transform + reconstruction (a17) ---------------------------
 * av1_inverse_transform_block (av1/common/idct.c:304-322) for a list of
 * blocks of one tx_size: dst (u8 when highbd = 0, then bit_depth must be 8;
 * u16 otherwise) += inverse 2-D transform of the block's dqcoeff, clipped to
 * the bit depth.  Blocks with eob == 0 are left untouched (the reference
 * returns early).  coeff_off addresses av1_get_max_eob(tx_size) words in the
 * reference's layout (64-point sizes: the packed 32-column quadrant).  Jobs of
 * one call must not overlap in dst. */
typedef struct LavishInvJob {
  int64_t dst_off;   /* element offset of the block's top-left pixel */
  int64_t coeff_off; /* word offset of the block's dqcoeff */
  int32_t tx_type;
  int32_t eob;
} LavishInvJob;

int lavish_inv_txfm_add_batch(const int32_t *dqcoeff, int tx_size,
                              const LavishInvJob *jobs, int njobs, void *dst,
                              int dst_stride, int bit_depth, int highbd,
                              void *stream);
/* The lossless TX_4X4 inverse (av1_highbd_iwht4x4_add, idct.c:34-40): per
 * job the 16-coefficient WHT when eob > 1, the DC-only form when eob == 1,
 * nothing when eob == 0; same job / destination conventions. */
int lavish_iwht4x4_add_batch(const int32_t *dqcoeff, const LavishInvJob *jobs,
                             int njobs, void *dst, int dst_stride,
                             int bit_depth, int highbd, void *stream);

/* ---- C4: fused TX-type RDO ----------------------------------------------
 * For every full tx_size block of (src - pred) (u16 planes, bit_depth 8/10/12)
 * and every TX type in type_mask: forward transform -> av1_highbd_quantize_fp
 * -> aom_satd(coeff) -> av1_highbd_block_error -> TX-domain distortion shift
 * (tx_search.c:1077-1116) -> rate_estimator (tpl_model.c:214-226) ->
 * RDCOST(rdmult, rate, dist) (rd.h:31-33); the block keeps the first type
 * with the strictly lowest cost.  Outputs per block (raster order): the
 * decision record and the winner's qcoeff / dqcoeff (n words each,
 * n = av1_get_max_eob). */
typedef struct LavishRdoBlock {
  int32_t best_type;
  int32_t eob;
  int32_t rate;   /* rate_estimator (<< AV1_PROB_COST_SHIFT) */
  int32_t satd;   /* aom_satd of the winner's coefficients */
  int64_t dist;   /* TX-domain distortion after the tx-scale shift */
  int64_t sse;
  int64_t rdcost;
} LavishRdoBlock;

int lavish_rdo_plane(const uint16_t *src, const uint16_t *pred, int stride,
                     int width, int height, int tx_size, uint32_t type_mask,
                     int bit_depth, const LavishQuantParams *qp, int rdmult,
                     LavishRdoBlock *out, int32_t *qcoeff, int32_t *dqcoeff,
                     void *stream);
/* The same with the per-block allowed_tx_mask / search order that
 * lavish_prune_tx_2d_batch produces (device arrays, either may be NULL):
 * block b only considers types set in block_mask[b] (0 = DCT_DCT only,
 * get_tx_mask's rule) that appear in block_map[b][0..15], and equal costs go
 * to the type earlier in block_map[b] (search_tx_type's txk_map loop,
 * tx_search.c:2148-2246).  type_mask is the evaluated superset.
 * pixel_domain: 0 TX-domain distortion, 1 pixel-domain (sizes <= 32). */
int lavish_rdo_plane_masked(const uint16_t *src, const uint16_t *pred, int stride,
                            int width, int height, int tx_size, uint32_t type_mask,
                            int bit_depth, const LavishQuantParams *qp, int rdmult,
                            const uint16_t *block_mask, const uint8_t *block_map,
                            int pixel_domain, LavishRdoBlock *out, int32_t *qcoeff,
                            int32_t *dqcoeff, void *stream);
/* The TX-domain decision ranked by the coefficient rate: per type, rate =
 * av1_cost_coeffs_txb (txb_rdopt.c:599-624, the cost_coeffs of
 * search_tx_type, tx_search.c:1903-1921,2172-2176) on the FP-quantized block
 * instead of rate_estimator, with the luma tables of the device CoeffCosts
 * `costs`, per-block TXB_CTX txb_ctx (device, nullable: {0, 0}) and
 * tx_type_costs[16] = get_tx_type_cost per tx type for this tx_size (host,
 * nullable: 0).  Records' rate is that rate.  Masks as above. */
int lavish_rdo_plane_rate(const uint16_t *src, const uint16_t *pred, int stride,
                          int width, int height, int tx_size, uint32_t type_mask,
                          int bit_depth, const LavishQuantParams *qp, int rdmult,
                          const LavishCoeffCosts *costs, const LavishTxbCtx *txb_ctx,
                          const int32_t *tx_type_costs, const uint16_t *block_mask,
                          const uint8_t *block_map, LavishRdoBlock *out,
                          int32_t *qcoeff, int32_t *dqcoeff, void *stream);

/* Frame level: lavish_rdo_plane for every size set in size_mask (bit =
 * TX_SIZE) with type_masks[tx_size] and per-size outputs (arrays of 19
 * pointers), the sizes running concurrently on internal streams. */
int lavish_rdo_frame(const uint16_t *src, const uint16_t *pred, int stride,
                     int width, int height, uint32_t size_mask,
                     const uint32_t *type_masks, int bit_depth,
                     const LavishQuantParams *qp, int rdmult,
                     LavishRdoBlock *const *records, int32_t *const *qcoeff,
                     int32_t *const *dqcoeff, void *stream);

/* Pixel-domain distortion: search_tx_type with
 * use_transform_domain_distortion == 0 and predict_dc_level 0
 * (tx_search.c:2060-2103, 2187-2231).  Same outputs; per block
 * block_sse = ROUND_POWER_OF_TWO(sum of squared residual, 2 (bd-8)) * 16 and,
 * per type: eob 0 -> dist = block_sse; otherwise dist = dist_block_px_domain
 * (tx_search.c:969-1017: recon = pred + av1_inverse_transform_block,
 * 16 * the highbd-rounded sse of src - recon), a high-energy block
 * (block_sse >= 128*128*pels) keeping the TX-domain distortion when that is
 * larger, and TX_64X64 with high energy using TX-domain + the energy outside
 * the kept quadrant unless that energy is small; sse = block_sse.  The 64-point
 * sizes take exactly one type (DCT_DCT); -6 otherwise.
 * Replaces the search_tx_type distortion step (tx_search.c:2187-2231). */
int lavish_rdo_plane_px(const uint16_t *src, const uint16_t *pred, int stride,
                        int width, int height, int tx_size, uint32_t type_mask,
                        int bit_depth, const LavishQuantParams *qp, int rdmult,
                        LavishRdoBlock *out, int32_t *qcoeff, int32_t *dqcoeff,
                        void *stream);
int lavish_rdo_frame_px(const uint16_t *src, const uint16_t *pred, int stride,
                        int width, int height, uint32_t size_mask,
                        const uint32_t *type_masks, int bit_depth,
                        const LavishQuantParams *qp, int rdmult,
                        LavishRdoBlock *const *records, int32_t *const *qcoeff,
                        int32_t *const *dqcoeff, void *stream);

/* Per 64x64 superblock: the candidate size (of size_mask) whose blocks tile
 * the SB with the lowest summed rd cost (ties: the larger size) -> sb_tx_size
 * (255 when none tiles it); then recon = pred + the chosen blocks' inverse
 * transforms with their best types (lavish_inv_txfm_add_batch semantics:
 * eob 0 leaves the prediction).  u16 planes, `stride` elements. */
int lavish_rdo_reconstruct(uint32_t size_mask,
                           const LavishRdoBlock *const *records,
                           const int32_t *const *dqcoeff, int width,
                           int height, const uint16_t *pred, uint16_t *recon,
                           int stride, int bit_depth, uint8_t *sb_tx_size,
                           void *stream);

/* The C4 step captured once for fixed buffers: lavish_rdo_frame (all sizes
 * of size_mask) + lavish_rdo_reconstruct recorded into a HIP graph that
 * lavish_rdo_graph_launch replays with one launch on any stream (device
 * pointers and parameters are the capture's; replays of one graph must not
 * overlap).  No reference counterpart: a launch-count aid for callers that
 * run the step on many small rectangles.  Creation runs the step once
 * (uncaptured) after the work already queued on `stream` and waits for it:
 * it WRITES records, qcoeff, dqcoeff, recon and sb_tx_size.  The graph owns
 * its reconstruction scratch and the internal streams / fork-join events its
 * capture forked over (none shared with uncaptured calls on the thread).
 * -8: capture / instantiation failed. */
typedef struct LavishRdoGraph LavishRdoGraph;
int lavish_rdo_graph_create(const uint16_t *src, const uint16_t *pred, int stride,
                            int width, int height, uint32_t size_mask,
                            const uint32_t *type_masks, int bit_depth,
                            const LavishQuantParams *qp, int rdmult,
                            LavishRdoBlock *const *records, int32_t *const *qcoeff,
                            int32_t *const *dqcoeff, uint16_t *recon, uint8_t *sb_tx_size,
                            void *stream, LavishRdoGraph **graph);
int lavish_rdo_graph_launch(LavishRdoGraph *graph, void *stream);
void lavish_rdo_graph_destroy(LavishRdoGraph *graph);

/* ---- C3: DIAMOND full-pixel motion search ------------------------------
 * av1_full_pixel_search with search_method DIAMOND (av1/encoder/mcomp.c:
 * 1755-1895 -> full_pixel_diamond :1479-1526 -> diamond_search_sad
 * :1318-1477), one (block, reference) per job, 8-bit planes.
 * Offsets in bytes from src / ref; ref_off is the block origin at mv (0,0);
 * both planes must be padded so that every mv inside the limits (as
 * av1_set_mv_limits computes them) addresses memory, plus 3 bytes of slack
 * after each row end. */
typedef struct LavishDiamondJob {
  int64_t src_off;
  int64_t ref_off;
  int16_t start_row, start_col;   /* FULLPEL_MV start */
  int16_t ref_mv_row, ref_mv_col; /* MV (1/8 pel) the mv cost refers to */
  int16_t col_min, col_max, row_min, row_max; /* FullMvLimits */
} LavishDiamondJob;

typedef struct LavishDiamondResult {
  int16_t best_row, best_col; /* FULLPEL_MV */
  int32_t bestsme;  /* returned var cost: aom_variance + mv_err_cost */
  int32_t steps;    /* DIAMOND: 8-site steps; pattern methods: candidate rounds */
  int32_t searches; /* DIAMOND: diamond_search_sad runs; pattern methods
                       (lavish_full_pixel_search_batch, BIGDIA family): the
                       SAD blocks read (start, in-range candidates, cost list) */
} LavishDiamondResult;

/* mv_cost_type: MV_COST_TYPE (av1/encoder/mcomp.h:31-38) 1 L1_LOWRES,
 * 2 L1_MIDRES, 3 L1_HDRES, 4 NONE (ENTROPY needs the entropy context's cost
 * tables: -2).  use_downsampled_sad: sdf/sdx4df = aom_sad_skip_* for blocks
 * >= 16 high with the reference's quality recheck.  w x h: any
 * @encoder_block_sizes entry (else -3). */
int lavish_diamond_search_batch(const uint8_t *src, int src_stride,
                                const uint8_t *ref, int ref_stride, int w,
                                int h, const LavishDiamondJob *jobs, int njobs,
                                int step_param, int mv_cost_type,
                                int use_downsampled_sad,
                                LavishDiamondResult *out, void *stream);

/* FAST_BIGDIA (search_method of the TPL model at speed >= 5 and of
 * bsize-dependent full-pel searches): fast_bigdia_search -> bigdia_search ->
 * pattern_search (av1/encoder/mcomp.c:498-550, 1017-1316) with
 * do_init_search 0, then get_mvpred_var_cost; the downsampled-SAD recheck of
 * av1_full_pixel_search (:1840-1873) as for DIAMOND.  Same jobs / results as
 * lavish_diamond_search_batch (steps = candidate rounds, searches = passes). */
int lavish_fast_bigdia_search_batch(const uint8_t *src, int src_stride,
                                    const uint8_t *ref, int ref_stride, int w,
                                    int h, const LavishDiamondJob *jobs,
                                    int njobs, int step_param,
                                    int mv_cost_type, int use_downsampled_sad,
                                    LavishDiamondResult *out, void *stream);

/* MV_COST_PARAMS (av1/encoder/mcomp.h:69-85) for any mv_cost_type.  The
 * tables are DEVICE pointers: mvjcost[MV_JOINTS] and mvcost[0] / [1] at the
 * centre (index MV_MAX = 16383) of 2 * MV_MAX + 1 entries each, as
 * x->mv_costs->mv_cost_stack is addressed (av1/encoder/block.h); needed for
 * MV_COST_ENTROPY only.  sad_per_bit / error_per_bit: x->sadperbit /
 * x->errorperbit (av1_set_error_per_bit / av1_set_sad_per_bit). */
typedef struct LavishMvCostParams {
  int32_t mv_cost_type; /* MV_COST_TYPE: 0 ENTROPY, 1..3 L1_{LOW,MID,HD}RES, 4 NONE */
  int32_t sad_per_bit;
  int32_t error_per_bit;
  int32_t reserved;
  const int32_t *mvjcost;
  const int32_t *mvcost[2];
} LavishMvCostParams;

/* av1_full_pixel_search (av1/encoder/mcomp.c:1755-1873, no mesh refinement)
 * for search_method (SEARCH_METHODS, mcomp_structs.h:56-86) DIAMOND 0,
 * BIGDIA 5 (pattern_search with do_init_search), FAST_DIAMOND 8,
 * FAST_BIGDIA 9, VFAST_DIAMOND 10 (BIGDIA sites, do_init_search 0, start
 * scale clamps of :1291-1316), any mv cost (cost: HOST pointer to the
 * parameters), the downsampled-SAD recheck, and -- when cost_lists (device,
 * int32 [njobs][5]) is not NULL -- the cost list the reference returns for
 * the sub-pel search (calc_int_sad_list: centre, left, bottom, right, top;
 * INT_MAX where out of range); passing a cost list changes the BIGDIA-family
 * walk exactly as in the reference (last_s).  Returns 0, -1 bad step_param,
 * -2 bad cost parameters, -3 unsupported w x h, -4 unsupported method. */
int lavish_full_pixel_search_batch(const uint8_t *src, int src_stride,
                                   const uint8_t *ref, int ref_stride, int w,
                                   int h, const LavishDiamondJob *jobs,
                                   int njobs, int search_method, int step_param,
                                   const LavishMvCostParams *cost,
                                   int use_downsampled_sad,
                                   LavishDiamondResult *out, int32_t *cost_lists,
                                   void *stream);

/* Candidate-row layout of the reference buffer for the full-pel searches
 * (the build's own addition, no reference counterpart; results are
 * identical with or without it).  The searches read, per candidate, rows
 * y, y + 2, ... (downsampled SAD) of a w <= 16 byte segment at any column:
 * in the linear plane every such row is a separate cache line.  The tiled
 * copy splits the buffer's rows by parity (two fields) and each field into
 * 32-byte-wide column strips starting every 16 bytes (strip k holds bytes
 * [16k, 16k + 32) of every field row, consecutive field rows 32 bytes
 * apart), so a 16-byte segment lies in one strip and a downsampled 16-row
 * candidate in 2-3 cache lines instead of 8.  2x the buffer's bytes.
 *   rows: rows of the whole buffer (all reference planes stacked, stride
 *   `ref_stride`); the tiled copy must be rebuilt when the buffer changes. */
typedef struct LavishRefTiles {
  const uint8_t *data; /* device; lavish_ref_tiles_bytes(stride, rows) bytes */
  int64_t field_bytes; /* bytes of one field (the odd field follows the even) */
  int32_t field_rows;  /* (rows + 1) / 2 */
  int32_t stride;      /* the linear buffer's stride (= ref_stride) */
} LavishRefTiles;
int64_t lavish_ref_tiles_bytes(int stride, int rows);
/* Fills tiles->data (caller-allocated, device) from the linear buffer and
 * sets the other fields; asynchronous on `stream`.  -1 on bad arguments or
 * a copy of 2 GiB or more. */
int lavish_ref_tiles_build(const uint8_t *ref, int stride, int rows, uint8_t *data,
                           LavishRefTiles *tiles, void *stream);
/* lavish_full_pixel_search_batch reading candidate rows from the tiled copy
 * of the same `ref` buffer (w <= 16; other sizes, or tiles == NULL, run the
 * linear form).  Same results. */
int lavish_full_pixel_search_batch_tiled(const uint8_t *src, int src_stride,
                                         const uint8_t *ref, int ref_stride,
                                         const LavishRefTiles *tiles, int w, int h,
                                         const LavishDiamondJob *jobs, int njobs,
                                         int search_method, int step_param,
                                         const LavishMvCostParams *cost,
                                         int use_downsampled_sad,
                                         LavishDiamondResult *out,
                                         int32_t *cost_lists, void *stream);

/* The mesh fields of FULLPEL_MOTION_SEARCH_PARAMS (av1/encoder/mcomp.h:
 * 114-123), with the pattern set the search reads
 * (mesh_patterns[is_intra_mode]: sf->mv_sf.mesh_patterns or
 * intrabc_mesh_patterns, speed_features.c:25-44,2292-2308). */
typedef struct LavishMeshParams {
  int32_t run_mesh_search;
  int32_t force_mesh_thresh;
  int32_t prune_mesh_search;
  int32_t mesh_search_mv_diff_threshold;
  int32_t fine_search_interval;
  int32_t is_intra_mode;
  int32_t range[4]; /* MESH_PATTERN range / interval per step (MAX_MESH_STEP 4) */
  int32_t interval[4];
} LavishMeshParams;
/* lavish_full_pixel_search_batch[_tiled] followed by the exhaustive mesh
 * refinement of av1_full_pixel_search (mcomp.c:1818-1838, 1875-1893 ->
 * full_pixel_exhaustive :1603-1680 -> exhaustive_mesh_search :1529-1601):
 * per job, when run_mesh_search or (NSTEP / NSTEP_8PT) the variance exceeds
 * force_mesh_thresh >> (10 - mi_size_wide_log2 - mi_size_high_log2), unless
 * pruned (not intra, the search moved <= mesh_search_mv_diff_threshold),
 * the mesh passes around the search's best with the search's sdf; its var
 * cost replaces the result when smaller, and the cost list (when
 * cost_lists) is the one around the mesh's best either way, as the reference
 * writes it.  An illegal first pattern (range outside [7, 256], interval
 * outside [1, range]) makes the mesh a no-op, as in the reference.  mesh:
 * HOST pointer (NULL: no mesh); tiles may be NULL.  Same returns as
 * lavish_full_pixel_search_batch, and -6 when a later pass the walk can
 * reach has an interval < 1. */
int lavish_full_pixel_search_batch_mesh(const uint8_t *src, int src_stride,
                                        const uint8_t *ref, int ref_stride,
                                        const LavishRefTiles *tiles, int w, int h,
                                        const LavishDiamondJob *jobs, int njobs,
                                        int search_method, int step_param,
                                        const LavishMvCostParams *cost,
                                        int use_downsampled_sad,
                                        const LavishMeshParams *mesh,
                                        LavishDiamondResult *out, int32_t *cost_lists,
                                        void *stream);

/* The compound, masked and OBMC full-pel searches (csrc/mcomp_comp.hip),
 * 8-bit, one wave per job.  A job is a LavishDiamondJob plus where its
 * job-invariant blocks lie in the buffers the call takes: second_pred
 * (compact, stride w) and the blend mask (rows mask_stride apart), or for
 * OBMC the int32 wsrc / mask blocks (compact, offsets in int32 elements;
 * base.src_off is not read). */
typedef struct LavishCompSearchJob { /* 56 bytes */
  LavishDiamondJob base; /* offsets, start, ref_mv, limits: as today */
  int64_t second_off; /* second_pred block, u8, stride w; OBMC: wsrc block (int32, w*h) */
  int64_t mask_off;   /* u8 mask block (mask_stride); OBMC: int32 mask block (w*h) */
  int32_t invert_mask; /* masked form: nonzero swaps the blend operands */
  int32_t reserved;
} LavishCompSearchJob;

typedef struct LavishCompSearchResult { /* 16 bytes */
  int16_t best_row, best_col;
  int16_t second_row, second_col; /* -32768, -32768: invalid */
  int32_t bestsme; /* the full-pel and OBMC searches: var + mv cost; the
                      8-point refinement: best_sad */
  int32_t steps;   /* step / round iterations executed over all runs */
} LavishCompSearchResult;

/* av1_full_pixel_search (mcomp.c:1755-1895) with ms_buffers.second_pred set,
 * search_method DIAMOND 0, NSTEP 1 or NSTEP_8PT 2: diamond_search_sad's
 * second_pred branch (:1377-1405, sites one at a time, msdf when `mask` is
 * given, else sdaf) under full_pixel_diamond (:1479-1526), the cost of each
 * run get_mvpred_compound_var_cost (:695-727: msvf / svaf at sub-pel offset
 * (0, 0)); no mesh (:1822), no cost list.  second_row / second_col: the
 * reference's second_best_mv, as it leaves it (the position the last move
 * of the last run left; invalid when no run moved).  There is no
 * use_downsampled_sad argument: with second_pred the walk never reads sdf,
 * so the quality recheck has nothing to check.  second_pred / mask:
 * device; mask NULL: the rounded average.  Returns 0, -1 bad step_param,
 * -2 bad cost parameters, -3 unsupported w x h, -4 a method outside the
 * three, -7 a NULL buffer or mask_stride < w. */
int lavish_comp_full_pixel_search_batch(const uint8_t *src, int src_stride,
                                        const uint8_t *ref, int ref_stride, int w,
                                        int h, const LavishCompSearchJob *jobs,
                                        int njobs, int search_method, int step_param,
                                        const LavishMvCostParams *cost,
                                        const uint8_t *second_pred, const uint8_t *mask,
                                        int mask_stride, LavishCompSearchResult *out,
                                        void *stream);

/* av1_refining_search_8p_c (mcomp.c:1683-1753): from the clamped start up to
 * 3 rounds over the 8 neighbours not yet visited, the SAD
 * get_mvpred_compound_sad (second_pred NULL: the plain sdf; mask NULL: sdaf).
 * bestsme = best_sad (SAD + mv SAD cost); second_row / second_col repeat the
 * best mv.  Returns as above. */
int lavish_refining_search_8p_batch(const uint8_t *src, int src_stride,
                                    const uint8_t *ref, int ref_stride, int w, int h,
                                    const LavishCompSearchJob *jobs, int njobs,
                                    const LavishMvCostParams *cost,
                                    const uint8_t *second_pred, const uint8_t *mask,
                                    int mask_stride, LavishCompSearchResult *out,
                                    void *stream);

/* av1_obmc_full_pixel_search (mcomp.c:2328-2342): fast_obmc_search 0
 * obmc_full_pixel_diamond (:2293-2326) over the sites of search_method (as
 * above), else obmc_refining_search_sad (:2190-2233; search_method and
 * step_param are still checked); the SAD osdf, the cost get_obmc_mvpred_var
 * (ovf + mv cost).  wsrc / obmc_mask: device int32.  second_row /
 * second_col are invalid.  Returns as above. */
int lavish_obmc_full_pixel_search_batch(const uint8_t *ref, int ref_stride, int w, int h,
                                        const LavishCompSearchJob *jobs, int njobs,
                                        int search_method, int step_param,
                                        const LavishMvCostParams *cost,
                                        int fast_obmc_search, const int32_t *wsrc,
                                        const int32_t *obmc_mask,
                                        LavishCompSearchResult *out, void *stream);

/* C2 and the C3 search in one launch: lavish_txq_frame(residual, ...) and
 * lavish_full_pixel_search_batch_tiled(src, ..., 16, 16, jobs, njobs,
 * DIAMOND, ...) with the same results, run as one grid (the 64-point sizes
 * and the 32-point class of the transform first, as lavish_txq_frame runs
 * them; then the <= 16-point class's workgroups and the search's job groups
 * interleaved in the dispatch order, a search unit of 8 workgroups every
 * `every` units from the start).  The search must be the 16x16 DIAMOND with
 * a tiled reference copy.  -6: every < 1.  No reference counterpart: the
 * reference runs the two on the encoder's threads. */
int lavish_txq_frame_search(const int16_t *residual, int stride, int width, int height,
                            uint32_t size_mask, const uint32_t *type_masks, int bit_depth,
                            int quant_kind, const LavishQuantParams *qp,
                            int32_t *const *qcoeff, int32_t *const *dqcoeff,
                            uint16_t *const *eob, const uint8_t *src, int src_stride,
                            const uint8_t *ref, int ref_stride, const LavishRefTiles *tiles,
                            const LavishDiamondJob *jobs, int njobs, int step_param,
                            const LavishMvCostParams *cost, int use_downsampled_sad,
                            LavishDiamondResult *out, int32_t *cost_lists, int every,
                            void *stream);

/* Process-wide cap on the workgroups of the 16x16 DIAMOND search of
 * lavish_full_pixel_search_batch[_tiled] (rounded up to 8; 0 = no cap, one
 * workgroup per 32 jobs).  A scheduling knob for running the search beside
 * another stream's work (the search holds fewer CU slots and runs longer);
 * results do not depend on it.  Default 0; -1 for a
 * negative value.  No reference counterpart (the reference's search runs on
 * the encoder's threads). */
int lavish_set_search_workgroup_cap(int workgroups);

/* How a capped 16x16 DIAMOND search deals its 8-job wave units: 1 (default)
 * every wave pulls its next unit from one of 8 queues (one per XCD label
 * blockIdx % 8, the label's units a contiguous range of blocks); 0 the
 * static grid-stride over virtual workgroups.  Results do not depend on it;
 * -1 for another value.  No reference counterpart. */
int lavish_set_search_schedule(int queued);

/* Which kernel runs a 16x16 DIAMOND search over tiled references with
 * use_downsampled_sad: 0 (default) auto -- the lean kernel (at most 64 VGPRs,
 * so a search wave fits on a SIMD beside four transform workgroups; jobs
 * whose downsampled-SAD result fails the quality recheck are rerun by a
 * follow-up launch on the same stream) when the grid is capped and
 * queue-fed, the full kernels otherwise; 1 always the full kernels; 2 the
 * lean kernel at any grid (uncapped: the queues cover every unit).  Results
 * do not depend on it; -1 for another value.  No reference counterpart. */
int lavish_set_search_variant(int variant);

/* ---- sub-pixel refinement ------------------------
 * av1_find_best_sub_pixel_tree_pruned_more (av1/encoder/mcomp.c:2907-2981;
 * subpel_search_method SUBPEL_TREE_PRUNED_MORE, speed >= 4) without a cost
 * list or a repeated-mv list, unscaled reference: setup_center_error at the
 * start, then two_level_checks_fast at half, quarter (forced_stop <
 * HALF_PEL) and eighth pel (allow_hp && forced_stop == EIGHTH_PEL), every
 * check check_better_fast with svf = aom_sub_pixel_variance (bilinear) +
 * mv_err_cost_.  8-bit planes.  One job per (block, reference): offsets as
 * LavishDiamondJob, start / ref mv and the SubpelMvLimits
 * (av1_set_subpel_mv_search_range, mcomp.h:357-373) in 1/8 pel.  The
 * search reads up to H+1 rows and W+5 bytes per row from the floor of every
 * in-range candidate.  forced_stop: 0 EIGHTH_PEL .. 3 FULL_PEL;
 * iters_per_step 1 or 2; mv_cost_type as lavish_diamond_search_batch. */
typedef struct LavishSubpelJob {
  int64_t src_off, ref_off;
  int16_t start_row, start_col;    /* full-pel best x 8 */
  int16_t ref_mv_row, ref_mv_col;
  int16_t col_min, col_max, row_min, row_max;
} LavishSubpelJob;

typedef struct LavishSubpelResult {
  int16_t best_row, best_col;      /* 1/8 pel */
  uint32_t besterr;                /* variance + mv cost of the best mv */
  int32_t distortion;              /* its variance */
  uint32_t sse;
} LavishSubpelResult;

int lavish_subpel_search_batch(const uint8_t *src, int src_stride,
                               const uint8_t *ref, int ref_stride, int w, int h,
                               const LavishSubpelJob *jobs, int njobs,
                               int forced_stop, int allow_hp,
                               int iters_per_step, int mv_cost_type,
                               LavishSubpelResult *out, void *stream);

/* The same, chained on the device after lavish_diamond_search_batch: job j
 * starts at fullpel[j].best_{row,col} x 8 (the jobs' start fields are
 * ignored), so the full-pel and sub-pel searches of a frame need no host
 * round trip. */
int lavish_subpel_search_after_diamond(const uint8_t *src, int src_stride,
                                       const uint8_t *ref, int ref_stride, int w,
                                       int h, const LavishSubpelJob *jobs,
                                       const LavishDiamondResult *fullpel,
                                       int njobs, int forced_stop, int allow_hp,
                                       int iters_per_step, int mv_cost_type,
                                       LavishSubpelResult *out, void *stream);

/* The general form: subpel_search_method (SUBPEL_SEARCH_METHODS,
 * mcomp_structs.h) 0 SUBPEL_TREE (av1_find_best_sub_pixel_tree,
 * mcomp.c:3128-3200, with subpel_search_type USE_2_TAPS_ORIG: the svf error,
 * first_level_check_fast + second_level_check_v2 per level; no cost list),
 * 1 SUBPEL_TREE_PRUNED (av1_find_best_sub_pixel_tree_pruned,
 * mcomp.c:2992-3126) or 2 SUBPEL_TREE_PRUNED_MORE (:2907-2990); any mv cost
 * (cost: HOST pointer, tables on the device, as for
 * lavish_full_pixel_search_batch -- the hp tables when allow_hp); cost_lists
 * (device int32 [njobs][5] or NULL): the full-pel search's cost lists, which
 * steer the first (half-pel) step exactly as in the reference.  fullpel
 * (device, or NULL to use the jobs' start fields): start = its best x 8.
 * Returns 0, -1 bad forced_stop, -2 bad cost parameters, -3 unsupported
 * w x h, -4 bad iters_per_step, -6 unsupported method. */
int lavish_find_best_sub_pixel_tree_batch(
    const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, int w,
    int h, const LavishSubpelJob *jobs, const LavishDiamondResult *fullpel,
    int njobs, int subpel_search_method, int forced_stop, int allow_hp,
    int iters_per_step, const LavishMvCostParams *cost, const int32_t *cost_lists,
    LavishSubpelResult *out, void *stream);
/* The same with var_params.subpel_search_type (SUBPEL_SEARCH_TYPE,
 * av1/common/filter.h:45-50: 0 USE_2_TAPS_ORIG, 1 USE_2_TAPS, 2 USE_4_TAPS,
 * 3 USE_8_TAPS; else -7).  SUBPEL_TREE with a type other than
 * USE_2_TAPS_ORIG ranks by upsampled_pref_error (av1/encoder/mcomp.c:
 * 2402-2491, check_better / first_level_check / second_level_check_v2's
 * check_better branch) -- aom_upsampled_pred_c's prediction
 * (av1/encoder/reconinter_enc.c:424-496, unscaled reference) -- which for
 * USE_2_TAPS equals the bilinear svf.  The pruned methods take the svf for
 * every type (check_better_fast on an unscaled reference), as in the
 * reference.  The speed-0..3 default is SUBPEL_TREE with USE_8_TAPS
 * (speed_features.c:1929-1931). */
int lavish_find_best_sub_pixel_tree_batch_ex(
    const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, int w,
    int h, const LavishSubpelJob *jobs, const LavishDiamondResult *fullpel,
    int njobs, int subpel_search_method, int subpel_search_type, int forced_stop,
    int allow_hp, int iters_per_step, const LavishMvCostParams *cost,
    const int32_t *cost_lists, LavishSubpelResult *out, void *stream);

/* ---- high bit depth (8 / 10 / 12 bits on uint16_t planes) ----------------
 * The single-reference searches with the members highbd_set_var_fns binds
 * (av1/encoder/encoder_utils.h:130-230,572-), csrc/mcomp_hbd.hip and
 * csrc/subpel_hbd.hip, one wave per job.  Jobs and results are the 8-bit
 * entry points' records; src_stride, ref_stride and the jobs' src_off /
 * ref_off are in ELEMENTS (uint16_t), not bytes.  bit_depth: 8, 10 or 12
 * (pixel values below 1 << bit_depth).
 *
 * lavish_highbd_full_pixel_search_batch: av1_full_pixel_search
 * (av1/encoder/mcomp.c:1755-1873, no mesh) for search_method DIAMOND 0,
 * NSTEP 1 or NSTEP_8PT 2 (the pattern methods: -4), sdf / sdx4df / sdsf =
 * aom_highbd_sad{W}x{H}[x4d] / aom_highbd_sad_skip_{W}x{H} under the
 * _bits8 / _bits10 / _bits12 wrappers (the block's SAD >> 0 / 2 / 4, before
 * the mv SAD cost is added), vf = aom_highbd_{8,10,12}_variance{W}x{H}, any
 * mv cost, use_downsampled_sad with the recheck on the wrapped SADs, and
 * the cost list (calc_int_sad_list) when cost_lists is not NULL.
 * Padding: both planes must be padded so that every mv inside the limits
 * addresses memory; the kernel reads rows of exactly w elements at the
 * pixel's own address: no slack before a row's start or after its end.
 * Returns 0 (also for njobs <= 0), -7 NULL src / ref / jobs / out or a
 * bit_depth outside {8, 10, 12}, -4 unsupported method, -1 bad step_param,
 * -2 bad cost parameters, -3 unsupported w x h; every refusal comes before
 * any device work and leaves out untouched. */
int lavish_highbd_full_pixel_search_batch(
    const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride,
    int w, int h, int bit_depth, const LavishDiamondJob *jobs, int njobs,
    int search_method, int step_param, const LavishMvCostParams *cost,
    int use_downsampled_sad, LavishDiamondResult *out, int32_t *cost_lists,
    void *stream);

/* lavish_highbd_find_best_sub_pixel_tree_batch: the sub-pel methods of
 * lavish_find_best_sub_pixel_tree_batch (SUBPEL_TREE with USE_2_TAPS_ORIG,
 * SUBPEL_TREE_PRUNED, SUBPEL_TREE_PRUNED_MORE) with svf =
 * aom_highbd_{8,10,12}_sub_pixel_variance{W}x{H} (aom_dsp/variance.c:
 * 454-670) and setup_center_error through the high-bit-depth vf; fullpel and
 * cost_lists (device) are what lavish_highbd_full_pixel_search_batch wrote,
 * so the pair chains on the device as the 8-bit pair does.
 * Padding: for every mv inside the SubpelMvLimits the (w + 1) x (h + 1)
 * elements at the mv's full-pel floor must address memory (the bilinear
 * filter's own reach); the kernel reads exactly those: no further slack.
 * Returns 0 (also for njobs <= 0), -7 NULL src / ref / jobs / out or a
 * bit_depth outside {8, 10, 12}, then as the 8-bit call: -1 bad forced_stop,
 * -2 bad cost parameters, -4 bad iters_per_step, -6 unsupported method,
 * -3 unsupported w x h; all before any device work. */
int lavish_highbd_find_best_sub_pixel_tree_batch(
    const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride,
    int w, int h, int bit_depth, const LavishSubpelJob *jobs,
    const LavishDiamondResult *fullpel, int njobs, int subpel_search_method,
    int forced_stop, int allow_hp, int iters_per_step,
    const LavishMvCostParams *cost, const int32_t *cost_lists,
    LavishSubpelResult *out, void *stream);
/* The same with var_params.subpel_search_type (0 USE_2_TAPS_ORIG .. 3
 * USE_8_TAPS; else -7), as lavish_find_best_sub_pixel_tree_batch_ex adds it to
 * the 8-bit call (csrc/subpel_up_hbd.hip).  SUBPEL_TREE with USE_4_TAPS /
 * USE_8_TAPS ranks by upsampled_pref_error's is_cur_buf_hbd branch
 * (av1/encoder/mcomp.c:2428-2448): aom_highbd_upsampled_pred_c's prediction
 * (av1/encoder/reconinter_enc.c:562-640, unscaled reference: every
 * aom_highbd_convolve8 pass rounded by FILTER_BITS and clipped to
 * (1 << bit_depth) - 1, the 2-D case's intermediate rows included), then the
 * depth's vf; with USE_2_TAPS it equals the bilinear svf.  The pruned methods
 * take the svf for every type.  Type 0 is the call above exactly.
 * Padding with SUBPEL_TREE and USE_4_TAPS / USE_8_TAPS: for every mv inside
 * the SubpelMvLimits the (w + 7) x (h + 7) elements that start 3 rows and 3
 * elements before the mv's full-pel floor must address memory, plus one
 * element before and after each row of that window (the horizontal pass loads
 * the aligned dwords that contain its 11 pixels). */
int lavish_highbd_find_best_sub_pixel_tree_batch_ex(
    const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride,
    int w, int h, int bit_depth, const LavishSubpelJob *jobs,
    const LavishDiamondResult *fullpel, int njobs, int subpel_search_method,
    int subpel_search_type, int forced_stop, int allow_hp, int iters_per_step,
    const LavishMvCostParams *cost, const int32_t *cost_lists,
    LavishSubpelResult *out, void *stream);

/* The compound, masked and OBMC sub-pel searches (csrc/subpel_comp.hip),
 * 8-bit, unscaled reference, one wave per job: what follows
 * lavish_comp_full_pixel_search_batch / lavish_refining_search_8p_batch in
 * av1_joint_motion_search and av1_compound_single_motion_search
 * (motion_search_facade.c:642-676, 786-793) and
 * lavish_obmc_full_pixel_search_batch in av1_single_motion_search's
 * OBMC_CAUSAL leg (:441-445).  A job is a LavishSubpelJob plus where its
 * job-invariant blocks lie, as in LavishCompSearchJob. */
typedef struct LavishCompSubpelJob { /* 56 bytes */
  LavishSubpelJob base; /* offsets, start (1/8 pel), ref mv, SubpelMvLimits: as today */
  int64_t second_off; /* second_pred block, u8, stride w; OBMC: wsrc block (int32, w*h) */
  int64_t mask_off;   /* u8 mask block (mask_stride); OBMC: int32 mask block (w*h) */
  int32_t invert_mask;
  int32_t reserved;
} LavishCompSubpelJob;

/* av1_find_best_sub_pixel_tree (mcomp.c:3128-3196), _pruned (:2992-3126) or
 * _pruned_more (:2907-2990) with ms_buffers.second_pred set, cost_list and
 * last_mv_search_list NULL as the encoder passes them on this path (the
 * pruned methods therefore start with two_level_checks_fast).  The centre
 * error is setup_center_error's second_pred branch (aom_comp_avg_pred /
 * aom_comp_mask_pred of the block at the start's full-pel floor, then vf);
 * the candidates estimated_pref_error (svaf, or msvf with `mask`), and for
 * SUBPEL_TREE with a subpel_search_type other than USE_2_TAPS_ORIG
 * upsampled_pref_error's second_pred branches (the centre then at the start
 * itself).  Methods, types, forced_stop, iters_per_step and cost as
 * lavish_find_best_sub_pixel_tree_batch_ex.  second_pred / mask: device;
 * mask NULL: the rounded average.
 * fullpel (device, or NULL to use the jobs' start fields): the results of
 * one of the three full-pel calls above for the same jobs; start_from 0
 * starts at best x 8, start_from 1 at second x 8 (the try_second call,
 * motion_search_facade.c:663-669).  With start_from 1 a job whose second mv
 * is invalid (-32768) or outside the job's SubpelMvLimits is not searched:
 * its record is besterr INT_MAX, best_row = best_col = -32768, distortion
 * and sse 0; the caller keeps the lower besterr.
 * Returns 0 (also njobs <= 0: nothing done), -1 bad forced_stop, -2 bad cost
 * parameters, -3 unsupported w x h, -4 bad iters_per_step, -6 bad method,
 * -7 bad search type, -8 a NULL buffer, mask_stride < w with a mask or
 * start_from outside 0 / 1, -9 start_from 1 without fullpel; every refusal
 * before any device work. */
int lavish_comp_find_best_sub_pixel_tree_batch(
    const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, int w, int h,
    const LavishCompSubpelJob *jobs, const LavishCompSearchResult *fullpel, int start_from,
    int njobs, int subpel_search_method, int subpel_search_type, int forced_stop, int allow_hp,
    int iters_per_step, const LavishMvCostParams *cost, const uint8_t *second_pred,
    const uint8_t *mask, int mask_stride, LavishSubpelResult *out, void *stream);

/* av1_find_best_obmc_sub_pixel_tree_up (mcomp.c:3761-3803): the errors osvf
 * (USE_2_TAPS_ORIG) or aom_upsampled_pred_c then ovf.  As the reference:
 * with USE_2_TAPS_ORIG the centre error is read at mv (0, 0), not at the
 * start (setup_obmc_center_error, :3530-3545; the mv cost is the start's),
 * and the candidates are priced by estimate_obmc_mvcost (:3561-3583: the
 * rate of the diff x 8, (rate * error_per_bit + 4096) >> 13; 0 for
 * MV_COST_NONE); the other types use mv_err_cost_ and the start.  wsrc /
 * obmc_mask: device int32; base.src_off is not read.  fullpel: the results
 * of lavish_obmc_full_pixel_search_batch, or NULL.  Returns as above, and
 * -2 for an L1 cost type with USE_2_TAPS_ORIG (the reference asserts). */
int lavish_obmc_find_best_sub_pixel_tree_batch(
    const uint8_t *ref, int ref_stride, int w, int h, const LavishCompSubpelJob *jobs,
    const LavishCompSearchResult *fullpel, int njobs, int subpel_search_type, int forced_stop,
    int allow_hp, int iters_per_step, const LavishMvCostParams *cost, const int32_t *wsrc,
    const int32_t *obmc_mask, LavishSubpelResult *out, void *stream);

/* ---- high bit depth: the compound, masked and OBMC searches ---------------
 * The five calls above (lavish_comp_full_pixel_search_batch,
 * lavish_refining_search_8p_batch, lavish_obmc_full_pixel_search_batch,
 * lavish_comp_find_best_sub_pixel_tree_batch and
 * lavish_obmc_find_best_sub_pixel_tree_batch) over uint16_t planes holding
 * bit_depth-bit pixels (8, 10 or 12), csrc/mcomp_comp_hbd.hip and
 * csrc/subpel_comp_hbd.hip, one wave per job, with the members
 * highbd_set_var_fns binds (av1/encoder/encoder_utils.h): sdaf =
 * aom_highbd_sad{W}x{H}_avg, msdf = aom_highbd_masked_sad{W}x{H}, osdf =
 * aom_highbd_obmc_sad{W}x{H} under their _bits8 / _bits10 / _bits12 wrappers
 * (the whole block's SAD >> 0 / 2 / 4, before the mv SAD cost is added);
 * svaf = aom_highbd_{8,10,12}_sub_pixel_avg_variance{W}x{H}, msvf =
 * aom_highbd_{8,10,12}_masked_sub_pixel_variance{W}x{H}, ovf / osvf =
 * aom_highbd_[10_|12_]obmc_[sub_pixel_]variance{W}x{H}; setup_center_error
 * through aom_highbd_comp_avg_pred / aom_highbd_comp_mask_pred and vf.
 * Jobs and results are the 8-bit calls' records.  src_stride, ref_stride and
 * the jobs' src_off / ref_off are in ELEMENTS (uint16_t); second_pred is
 * uint16_t (compact blocks, stride w, second_off in elements); mask stays
 * uint8_t with mask_stride, wsrc / obmc_mask int32_t.  Everything else --
 * the searches, second_best_mv, fullpel chaining with start_from 0 / 1 and
 * its INT_MAX / -32768 record, the three OBMC sub-pel peculiarities -- is the
 * 8-bit twin's.  The sub-pel calls without subpel_search_type take the
 * bilinear error (USE_2_TAPS_ORIG), as
 * lavish_highbd_find_best_sub_pixel_tree_batch; their _ex forms below add the
 * type.
 * Padding: as the 8-bit twins, in elements: exactly the w x h blocks (full
 * pel) or the (w + 1) x (h + 1) windows (sub pel) the reference reads.
 * Return codes are the twins', and a bit_depth outside {8, 10, 12} returns
 * -7 (full pel) or -8 (sub pel); every refusal comes before any device work
 * and leaves out untouched; njobs <= 0 returns 0. */
int lavish_highbd_comp_full_pixel_search_batch(
    const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride,
    int w, int h, int bit_depth, const LavishCompSearchJob *jobs, int njobs,
    int search_method, int step_param, const LavishMvCostParams *cost,
    const uint16_t *second_pred, const uint8_t *mask, int mask_stride,
    LavishCompSearchResult *out, void *stream);

int lavish_highbd_refining_search_8p_batch(
    const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride,
    int w, int h, int bit_depth, const LavishCompSearchJob *jobs, int njobs,
    const LavishMvCostParams *cost, const uint16_t *second_pred,
    const uint8_t *mask, int mask_stride, LavishCompSearchResult *out,
    void *stream);

int lavish_highbd_obmc_full_pixel_search_batch(
    const uint16_t *ref, int ref_stride, int w, int h, int bit_depth,
    const LavishCompSearchJob *jobs, int njobs, int search_method,
    int step_param, const LavishMvCostParams *cost, int fast_obmc_search,
    const int32_t *wsrc, const int32_t *obmc_mask, LavishCompSearchResult *out,
    void *stream);

int lavish_highbd_comp_find_best_sub_pixel_tree_batch(
    const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride,
    int w, int h, int bit_depth, const LavishCompSubpelJob *jobs,
    const LavishCompSearchResult *fullpel, int start_from, int njobs,
    int subpel_search_method, int forced_stop, int allow_hp,
    int iters_per_step, const LavishMvCostParams *cost,
    const uint16_t *second_pred, const uint8_t *mask, int mask_stride,
    LavishSubpelResult *out, void *stream);

int lavish_highbd_obmc_find_best_sub_pixel_tree_batch(
    const uint16_t *ref, int ref_stride, int w, int h, int bit_depth,
    const LavishCompSubpelJob *jobs, const LavishCompSearchResult *fullpel,
    int njobs, int forced_stop, int allow_hp, int iters_per_step,
    const LavishMvCostParams *cost, const int32_t *wsrc,
    const int32_t *obmc_mask, LavishSubpelResult *out, void *stream);

/* The two sub-pel calls above with var_params.subpel_search_type where the
 * 8-bit twins have it (0 USE_2_TAPS_ORIG .. 3 USE_8_TAPS; else -7),
 * csrc/subpel_up_hbd.hip.  Type 0, and the pruned methods at any type, are
 * the calls above exactly.  SUBPEL_TREE with another type ranks by
 * upsampled_pref_error's is_cur_buf_hbd branch: aom_highbd_upsampled_pred_c
 * (USE_2_TAPS: the bilinear kernels of av1_get_filter through the same
 * passes) combined as aom_highbd_comp_avg_upsampled_pred /
 * aom_highbd_comp_mask_upsampled_pred, then the depth's vf, with the centre
 * error read at the start mv itself (upsampled_setup_center_error).  OBMC
 * with a type other than 0: upsampled_setup_obmc_center_error at the start,
 * candidates priced by mv_err_cost_ (the L1 cost types are accepted), the
 * error aom_highbd_upsampled_pred then ovf.  fullpel / start_from chaining,
 * the try_second record and the return codes are the calls' above.
 * Padding where the upsampled prediction runs: for every mv inside the
 * SubpelMvLimits the (w + 7) x (h + 7) elements that start 3 rows and 3
 * elements before the mv's full-pel floor, plus one element before and after
 * each row of that window. */
int lavish_highbd_comp_find_best_sub_pixel_tree_batch_ex(
    const uint16_t *src, int src_stride, const uint16_t *ref, int ref_stride,
    int w, int h, int bit_depth, const LavishCompSubpelJob *jobs,
    const LavishCompSearchResult *fullpel, int start_from, int njobs,
    int subpel_search_method, int subpel_search_type, int forced_stop,
    int allow_hp, int iters_per_step, const LavishMvCostParams *cost,
    const uint16_t *second_pred, const uint8_t *mask, int mask_stride,
    LavishSubpelResult *out, void *stream);

int lavish_highbd_obmc_find_best_sub_pixel_tree_batch_ex(
    const uint16_t *ref, int ref_stride, int w, int h, int bit_depth,
    const LavishCompSubpelJob *jobs, const LavishCompSearchResult *fullpel,
    int njobs, int subpel_search_type, int forced_stop, int allow_hp,
    int iters_per_step, const LavishMvCostParams *cost, const int32_t *wsrc,
    const int32_t *obmc_mask, LavishSubpelResult *out, void *stream);

/* ---- Inter prediction -----------------------------
 * av1_enc_build_one_inter_predictor (av1/encoder/reconinter_enc.c:47-51) for
 * a batch of single-reference translational blocks: init_subpel_params
 * (av1/common/reconinter.h:131-165, unscaled, border clamp), the block-size
 * filter choice (filter.h:253-259) and convolve_2d_facade_single
 * (av1/common/convolve.c:614-634 / highbd :1106-1128).
 *   ref: plane origin (buf0) of the reference, with the reference's
 *        AOM_BORDER_IN_PIXELS >> ss border around it (per direction; 12-tap
 *        MULTITAP_SHARP2 reads one more row / column at the clamp extremes,
 *        as the C does); ref_width / height: the plane's size (the clamp
 *        window).
 *   w, h: 2..128 (powers of two); ss_x / ss_y: the plane's subsampling.
 *   highbd 0: u8 planes (bit_depth 8); 1: u16 planes, bit_depth 8/10/12.
 * dst[job.dst_off + y * dst_stride + x] receives the prediction. */
typedef struct LavishInterPredJob {
  int64_t ref_off;             /* element offset of this job's reference plane origin */
  int64_t dst_off;             /* element offset of the block's first output pixel */
  int32_t pix_row, pix_col;    /* block position in the plane (pixels) */
  int16_t mv_row, mv_col;      /* MV, 1/8 luma pel */
  uint8_t filter_x, filter_y;  /* InterpFilter: 0 REGULAR 1 SMOOTH 2 SHARP 3 BILINEAR 4 SHARP2 */
  uint8_t pad[2];
} LavishInterPredJob;

int lavish_build_inter_pred_batch(const void *ref, int ref_stride, int ref_width,
                                  int ref_height, int ss_x, int ss_y, int w, int h,
                                  const LavishInterPredJob *jobs, int njobs,
                                  void *dst, int dst_stride, int bit_depth,
                                  int highbd, void *stream);
/* The interpolation kernels the library itself uses, as data:
 * av1_get_interp_filter_params_with_block_size(interp_filter, size)
 * (av1/common/filter.h:253-259) -> out[16][taps] (one row per 1/16 phase),
 * returns taps (8, or 12 for MULTITAP_SHARP2), -1 on bad arguments.  For
 * callers that build LavishInterpFilterParams (the RTCD convolve shims, the
 * compound batch) without the reference's tables at hand.  Host only. */
int lavish_interp_kernels(int interp_filter, int size, int16_t *out);
/* The same with job j's mv taken from a sub-pel search result (chained on
 * the device after lavish_subpel_search_batch / _after_diamond). */
int lavish_build_inter_pred_after_subpel(const void *ref, int ref_stride,
                                         int ref_width, int ref_height, int ss_x,
                                         int ss_y, int w, int h,
                                         const LavishInterPredJob *jobs,
                                         const LavishSubpelResult *mvs, int njobs,
                                         void *dst, int dst_stride, int bit_depth,
                                         int highbd, void *stream);

/* ---- TPL block transform leg ----------------------
 * For every full bsize x bsize block of a width x height frame (raster
 * order; bsize 8 / 16 / 32 with TX = the block, tpl_model.c uses 16): the
 * inter cost of each of nrefs predictions (tpl_get_satd_cost,
 * av1/encoder/tpl_model.c:199-210: subtract, av1_quick_txfm DCT_DCT,
 * aom_satd), the cheapest reference (lowest cost, earlier reference on
 * ties), and on its prediction txfm_quant_rdcost (:225-247):
 * get_quantize_error (:98-135, quantize_fp with qp built for
 * LAVISH_QUANT_FP, block error and sse >> (TX_32X32 ? 0 : 2), each >= 1),
 * rate_estimator (:212-223) and recon = prediction + the inverse transform.
 *   src: plane origin, src_stride elements; preds: reference k's
 *   prediction plane at preds + k * pred_plane elements (same geometry);
 *   recon: output plane.  8-bit: uint8_t planes; 10 / 12-bit: uint16_t.
 *   ref_costs (device, optional): int32 [nblocks][nrefs] inter costs.
 * Returns 0, or -1 bad bsize, -2 bad bit_depth, -3 NULL argument, -4 bad
 * nrefs / preds, -5 bad geometry. */
typedef struct LavishTplBlock {
  int32_t best_ref;    /* index of the cheapest prediction */
  int32_t inter_cost;  /* its satd cost */
  int32_t rate_cost;   /* rate_estimator, << AV1_PROB_COST_SHIFT */
  int32_t eob;
  int64_t recon_error; /* get_quantize_error's recon_error */
  int64_t sse;         /* and sse */
} LavishTplBlock;

int lavish_tpl_block_batch(const void *src, int src_stride, const void *preds,
                           int64_t pred_plane, int pred_stride, int nrefs,
                           int width, int height, int bsize, int bit_depth,
                           const LavishQuantParams *qp, LavishTplBlock *out,
                           void *recon, int recon_stride, int32_t *ref_costs,
                           void *stream);

/* ---- TPL motion search with start-mv candidates --
 * Replaces the per-reference loop of mode_estimation
 * (av1/encoder/tpl_model.c:632-743) for a frame of 16x16 TPL blocks
 * (set_tpl_stats_block_size, :136-144): centre mvs = zero, then the above,
 * left and above-right blocks' tpl mvs of the same reference unless
 * is_alike_mv (:319-333, threshold by skip_alike_starting_mv), the optional
 * third-pass mv in slot 0 (:687-703); with prune_starting_mv the full-SAD
 * ranking at the clamped full-pel centres and the cut (:705-728); then
 * motion_estimation (:249-303) per centre -- av1_full_pixel_search with
 * ref_mv = the centre, tpl_sf.search_method, step_param =
 * AOMMIN(reduce_first_step_size, 9), the caller's mv costs and
 * use_downsampled_sad, a cost list when cost_lists != NULL -- keeping the
 * lowest sub-pel error (strict <).  subpel_force_stop must be FULL_PEL
 * (speed >= 5, speed_features.c:1212-1216; else -6): the tpl mv is the
 * full-pel best x 8.  Blocks depend on their finished neighbours: the call
 * runs as a device wavefront (one wave per reference x block row).
 *   jobs: [nrefs][rows * cols] LavishDiamondJob in raster order (offsets;
 *     limits = x->mv_limits of av1_set_mv_limits with tpl border_in_pixels;
 *     start / ref_mv fields ignored); the src / ref planes as for
 *     lavish_full_pixel_search_batch.
 *   third_pass_mvs: NULL or int_mv [nrefs][rows * cols] (INVALID_MV =
 *     0x80008000 for none).
 *   out (device): mvs int_mv [nrefs][rows * cols] = tpl_stats->mv[rf_idx]
 *     (row in the low 16 bits); out: the winning full-pel search's
 *     LavishDiamondResult; cost_lists (or NULL) its cost list; centers (or
 *     NULL) its centre mv (int_mv).
 *   sync: device int32 scratch of lavish_tpl_motion_sync_ints(nrefs, rows)
 *     entries (zeroed by the call); after the stream drains, sync[1] != 0
 *     means a wait timed out (results invalid).  mvs is filled with
 *     INVALID_MV first and each entry published once, when final.
 * Returns 0, -1 bad geometry / parameters, -2 bad costs, -4 bad method,
 * -6 subpel_force_stop != FULL_PEL. */
typedef struct LavishTplMvParams {
  int search_method;          /* tpl_sf.search_method (SEARCH_METHODS value) */
  int step_param;             /* tpl_sf.reduce_first_step_size */
  int use_downsampled_sad;    /* mv_sf.use_downsampled_sad */
  int prune_starting_mv;      /* tpl_sf.prune_starting_mv, 0..3 */
  int skip_alike_starting_mv; /* tpl_sf.skip_alike_starting_mv, 0..2 */
  int subpel_force_stop;      /* tpl_sf.subpel_force_stop: FULL_PEL (3) */
} LavishTplMvParams;

int64_t lavish_tpl_motion_sync_ints(int nrefs, int rows);
int lavish_tpl_motion_search(const uint8_t *src, int src_stride,
                             const uint8_t *ref, int ref_stride,
                             const LavishDiamondJob *jobs, int cols, int rows,
                             int nrefs, const LavishTplMvParams *p,
                             const LavishMvCostParams *cost,
                             const int32_t *third_pass_mvs, int32_t *mvs,
                             LavishDiamondResult *out, int32_t *cost_lists,
                             int32_t *centers, int32_t *sync, void *stream);

/* ---- TX-type pruning features ---------------------
 * Every full bw x bh block of an int16 residual plane (raster order):
 * av1_get_horver_correlation_full (av1/encoder/rdopt.c:514-609) -> hcorr /
 * vcorr[block] (bw, bh in 2..128). */
int lavish_horver_correlation_batch(const int16_t *residual, int stride,
                                    int width, int height, int bw, int bh,
                                    float *hcorr, float *vcorr, void *stream);
/* prune_tx_2D's two neural-net inputs (av1/encoder/tx_search.c:1516-1529)
 * per tx_size block: hfeatures[block][16] = get_energy_distribution_finer's
 * column projection (tx_search.c:1411-1473) in [0, n-1) and hcorr at n-1
 * (n = w <= 8 ? w : w / 2); vfeatures likewise for rows; unused entries 0.
 * tx sizes up to 32x32 (else -2).  Bit-exact single precision. */
int lavish_tx_prune_features_batch(const int16_t *residual, int stride,
                                   int width, int height, int tx_size,
                                   float *hfeatures, float *vfeatures,
                                   void *stream);

/* Layout of NN_CONFIG (av1/encoder/ml.h:24-34): a caller passes the
 * reference's own models (e.g. av1_tx_type_nnconfig_map_hor[tx_size]).
 * Models are uploaded once per distinct content. */
typedef struct LavishNNConfig {
  int num_inputs;
  int num_outputs;
  int num_hidden_layers;
  int num_hidden_nodes[10];
  const float *weights[11];
  const float *bias[11];
} LavishNNConfig;

/* prune_tx_2D (av1/encoder/tx_search.c:1487-1641) for every full tx_size
 * block of an int16 residual plane (raster order): features, the two nets
 * (av1_nn_predict_c with reduce_prec), av1_nn_fast_softmax_16_c, the
 * adaptive threshold of (tx_set_type, prune_2d_txfm_mode), the sorting
 * network and the TX_TYPE_PRUNE_4/5 cumulative cut.
 *   allowed_in[block] (or allowed_default for every block when NULL): the
 *   incoming allowed_tx_mask; allowed_out[block]: the pruned mask;
 *   txk_map[block][16]: the search order (TX_TYPE values, 255 unused),
 *   identity where prune_tx_2D leaves it untouched (tx set other than
 *   ALL16 / DTT9_IDTX_1DDCT, mode 0, or nn_hor / nn_ver NULL).
 * Float results follow the C functions bit for bit.  -2: tx size or
 * threshold outside the reference's tables; -3: model shape unsupported
 * (outputs != 4, > 16 inputs, differing depths, > 128 nodes). */
int lavish_prune_tx_2d_batch(const int16_t *residual, int stride, int width,
                             int height, int tx_size, int tx_set_type,
                             int prune_2d_txfm_mode, const LavishNNConfig *nn_hor,
                             const LavishNNConfig *nn_ver,
                             const uint16_t *allowed_in, uint16_t allowed_default,
                             uint16_t *allowed_out, uint8_t *txk_map,
                             void *stream);
/* av1_nn_predict_c (av1/encoder/ml.c:31-70) for n input vectors
 * (inputs[n][num_inputs] -> outputs[n][num_outputs], device memory). */
int lavish_nn_predict_batch(const float *inputs, const LavishNNConfig *nn_config,
                            int reduce_prec, float *outputs, int n, void *stream);

/* ------------------------------------------------------------------------ */
/* Per-call RTCD shims (host pointers)                                      */
/* ------------------------------------------------------------------------ */
/* av1_fwd_txfm2d_WxH (av1/common/av1_rtcd_defs.pl:358-399); the 64-point
 * sizes reproduce the reference's in-place zero + re-pack of the whole W*H
 * output buffer (av1/encoder/av1_fwd_txfm2d.c:240-311). */
#define LAVISH_FWD2D(w, h)                                                   \
  void av1_fwd_txfm2d_##w##x##h##_hip(const int16_t *input, int32_t *output, \
                                      int stride, uint8_t tx_type, int bd);
LAVISH_FWD2D(4, 4)
LAVISH_FWD2D(64, 64)
LAVISH_FWD2D(32, 64)
LAVISH_FWD2D(64, 32)
LAVISH_FWD2D(16, 64)
LAVISH_FWD2D(64, 16)
LAVISH_FWD2D(8, 8)
LAVISH_FWD2D(16, 16)
LAVISH_FWD2D(32, 32)
LAVISH_FWD2D(4, 8)
LAVISH_FWD2D(8, 4)
LAVISH_FWD2D(8, 16)
LAVISH_FWD2D(16, 8)
LAVISH_FWD2D(16, 32)
LAVISH_FWD2D(32, 16)
LAVISH_FWD2D(4, 16)
LAVISH_FWD2D(16, 4)
LAVISH_FWD2D(8, 32)
LAVISH_FWD2D(32, 8)
#undef LAVISH_FWD2D

/* av1_lowbd_fwd_txfm (av1/common/av1_rtcd_defs.pl:355,
 * av1/encoder/hybrid_fwd_txfm.c:244); a lossless TX_4X4 takes av1_fwht4x4 */
void av1_lowbd_fwd_txfm_hip(const int16_t *src_diff, int32_t *coeff,
                            int diff_stride, LavishTxfmParam *txfm_param);
/* lossless Walsh-Hadamard (av1/common/av1_rtcd_defs.pl:351,217-218;
 * hybrid_fwd_txfm.c:24-76, av1_inv_txfm2d.c:20-107); tagged u16 dest */
void av1_fwht4x4_hip(const int16_t *input, int32_t *output, int stride);
void av1_highbd_iwht4x4_16_add_hip(const int32_t *input, uint8_t *dest,
                                   int dest_stride, int bd);
void av1_highbd_iwht4x4_1_add_hip(const int32_t *input, uint8_t *dest,
                                  int dest_stride, int bd);
/* BitDepthInfo of av1/common/blockd.h:952-960 */
typedef struct LavishBitDepthInfo {
  int bit_depth;
  int use_highbitdepth_buf;
} LavishBitDepthInfo;
/* av1_quick_txfm (av1/encoder/hybrid_fwd_txfm.c:315-336, the TPL model's
 * transform): aom_hadamard_{4x4..32x32} when use_hadamard, else the DCT_DCT
 * forward transform of tx_size. */
void av1_quick_txfm_hip(int use_hadamard, uint8_t tx_size,
                        LavishBitDepthInfo bd_info, const int16_t *src_diff,
                        int src_stride, int32_t *coeff);

/* quantizers (aom_dsp/aom_dsp_rtcd_defs.pl:655-694,
 * av1/common/av1_rtcd_defs.pl:334-344,428) */
#define LAVISH_QUANT_PROTO(name)                                              \
  void name(const int32_t *coeff_ptr, intptr_t n_coeffs,                      \
            const int16_t *zbin_ptr, const int16_t *round_ptr,                \
            const int16_t *quant_ptr, const int16_t *quant_shift_ptr,         \
            int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,                        \
            const int16_t *dequant_ptr, uint16_t *eob_ptr,                    \
            const int16_t *scan, const int16_t *iscan);
LAVISH_QUANT_PROTO(av1_quantize_fp_hip)
LAVISH_QUANT_PROTO(av1_quantize_fp_32x32_hip)
LAVISH_QUANT_PROTO(av1_quantize_fp_64x64_hip)
LAVISH_QUANT_PROTO(aom_quantize_b_hip)
LAVISH_QUANT_PROTO(aom_quantize_b_32x32_hip)
LAVISH_QUANT_PROTO(aom_quantize_b_64x64_hip)
LAVISH_QUANT_PROTO(aom_highbd_quantize_b_hip)
LAVISH_QUANT_PROTO(aom_highbd_quantize_b_32x32_hip)
LAVISH_QUANT_PROTO(aom_highbd_quantize_b_64x64_hip)
#undef LAVISH_QUANT_PROTO
/* aom_quantize_b_helper (av1/common/av1_rtcd_defs.pl:346) */
void aom_quantize_b_helper_hip(const int32_t *coeff_ptr, intptr_t n_coeffs,
                               const int16_t *zbin_ptr, const int16_t *round_ptr,
                               const int16_t *quant_ptr,
                               const int16_t *quant_shift_ptr,
                               int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,
                               const int16_t *dequant_ptr, uint16_t *eob_ptr,
                               const int16_t *scan, const int16_t *iscan,
                               const uint8_t *qm_ptr, const uint8_t *iqm_ptr,
                               const int log_scale);
void av1_highbd_quantize_fp_hip(const int32_t *coeff_ptr, intptr_t count,
                                const int16_t *zbin_ptr,
                                const int16_t *round_ptr,
                                const int16_t *quant_ptr,
                                const int16_t *quant_shift_ptr,
                                int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,
                                const int16_t *dequant_ptr, uint16_t *eob_ptr,
                                const int16_t *scan, const int16_t *iscan,
                                int log_scale);

/* ---- inverse transform shims (av1/common/av1_rtcd_defs.pl:137-243) ---- */
#define LAVISH_TX_SIZES_ALL(X)                                               \
  X(4, 4) X(8, 8) X(16, 16) X(32, 32) X(64, 64) X(4, 8) X(8, 4) X(8, 16)    \
  X(16, 8) X(16, 32) X(32, 16) X(32, 64) X(64, 32) X(4, 16) X(16, 4)        \
  X(8, 32) X(32, 8) X(16, 64) X(64, 16)
#define LAVISH_INV2D(w, h)                                                   \
  void av1_inv_txfm2d_add_##w##x##h##_hip(const int32_t *input,             \
                                          uint16_t *output, int stride,     \
                                          uint8_t tx_type, int bd);
LAVISH_TX_SIZES_ALL(LAVISH_INV2D)
#undef LAVISH_INV2D
void av1_inv_txfm_add_hip(const int32_t *dqcoeff, uint8_t *dst, int stride,
                          const LavishTxfmParam *txfm_param);
void av1_highbd_inv_txfm_add_hip(const int32_t *input, uint8_t *dest,
                                 int stride,
                                 const LavishTxfmParam *txfm_param);
#define LAVISH_HBD_INV(w, h)                                                 \
  void av1_highbd_inv_txfm_add_##w##x##h##_hip(                             \
      const int32_t *input, uint8_t *dest, int stride,                      \
      const LavishTxfmParam *txfm_param);
LAVISH_HBD_INV(4, 4) LAVISH_HBD_INV(8, 8) LAVISH_HBD_INV(4, 8)
LAVISH_HBD_INV(8, 4) LAVISH_HBD_INV(4, 16) LAVISH_HBD_INV(16, 4)
LAVISH_HBD_INV(8, 16) LAVISH_HBD_INV(16, 8) LAVISH_HBD_INV(16, 32)
LAVISH_HBD_INV(32, 16) LAVISH_HBD_INV(32, 32) LAVISH_HBD_INV(32, 64)
LAVISH_HBD_INV(64, 32) LAVISH_HBD_INV(64, 64) LAVISH_HBD_INV(8, 32)
LAVISH_HBD_INV(32, 8) LAVISH_HBD_INV(16, 64) LAVISH_HBD_INV(64, 16)
#undef LAVISH_HBD_INV

/* ---- pixel shims ---------------------------------------------------------
 * @encoder_block_sizes of aom_dsp/aom_dsp_rtcd_defs.pl:42-58. */
#define LAVISH_ENCODER_BLOCK_SIZES(X)                                     \
  X(128, 128) X(128, 64) X(64, 128) X(64, 64) X(64, 32) X(32, 64)         \
  X(32, 32) X(32, 16) X(16, 32) X(16, 16) X(16, 8) X(8, 16) X(8, 8)       \
  X(8, 4) X(4, 8) X(4, 4) X(4, 16) X(16, 4) X(8, 32) X(32, 8) X(16, 64)   \
  X(64, 16)

/* aom_dsp_rtcd_defs.pl:764-766,1003-1006 (lowbd) and :882-884,1139-1141
 * (highbd) */
#define LAVISH_SAD_PROTOS(w, h)                                               \
  unsigned int aom_sad##w##x##h##_hip(const uint8_t *src_ptr, int src_stride, \
                                      const uint8_t *ref_ptr, int ref_stride); \
  unsigned int aom_sad_skip_##w##x##h##_hip(const uint8_t *src_ptr,           \
                                            int src_stride,                   \
                                            const uint8_t *ref_ptr,           \
                                            int ref_stride);                  \
  unsigned int aom_sad##w##x##h##_avg_hip(                                    \
      const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr,         \
      int ref_stride, const uint8_t *second_pred);                            \
  void aom_sad##w##x##h##x4d_hip(const uint8_t *src_ptr, int src_stride,      \
                                 const uint8_t *const ref_ptr[4],             \
                                 int ref_stride, uint32_t sad_array[4]);      \
  void aom_sad##w##x##h##x3d_hip(const uint8_t *src_ptr, int src_stride,      \
                                 const uint8_t *const ref_ptr[4],             \
                                 int ref_stride, uint32_t sad_array[4]);      \
  void aom_sad##w##x##h##x4d_avg_hip(                                         \
      const uint8_t *src_ptr, int src_stride,                                 \
      const uint8_t *const ref_ptr[4], int ref_stride,                        \
      const uint8_t *second_pred, uint32_t sad_array[4]);                     \
  void aom_sad_skip_##w##x##h##x4d_hip(const uint8_t *src_ptr,                \
                                       int src_stride,                        \
                                       const uint8_t *const ref_ptr[4],       \
                                       int ref_stride, uint32_t sad_array[4]); \
  unsigned int aom_highbd_sad##w##x##h##_hip(                                 \
      const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr,         \
      int ref_stride);                                                        \
  unsigned int aom_highbd_sad_skip_##w##x##h##_hip(                           \
      const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr,         \
      int ref_stride);                                                        \
  unsigned int aom_highbd_sad##w##x##h##_avg_hip(                             \
      const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr,         \
      int ref_stride, const uint8_t *second_pred);                            \
  void aom_highbd_sad##w##x##h##x4d_hip(const uint8_t *src_ptr,               \
                                        int src_stride,                       \
                                        const uint8_t *const ref_ptr[],       \
                                        int ref_stride, uint32_t *sad_array); \
  void aom_highbd_sad##w##x##h##x3d_hip(const uint8_t *src_ptr,               \
                                        int src_stride,                       \
                                        const uint8_t *const ref_ptr[],       \
                                        int ref_stride, uint32_t *sad_array); \
  void aom_highbd_sad_skip_##w##x##h##x4d_hip(                                \
      const uint8_t *src_ptr, int src_stride,                                 \
      const uint8_t *const ref_ptr[], int ref_stride, uint32_t *sad_array);

/* aom_dsp_rtcd_defs.pl:1363-1365 (lowbd) and :1476-1478 (highbd 8/10/12) */
#define LAVISH_VAR_PROTOS_BD(pre, w, h)                                       \
  unsigned int pre##variance##w##x##h##_hip(const uint8_t *src_ptr,           \
                                            int source_stride,                \
                                            const uint8_t *ref_ptr,           \
                                            int ref_stride, uint32_t *sse);   \
  uint32_t pre##sub_pixel_variance##w##x##h##_hip(                            \
      const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset,    \
      const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);                 \
  uint32_t pre##sub_pixel_avg_variance##w##x##h##_hip(                        \
      const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset,    \
      const uint8_t *ref_ptr, int ref_stride, uint32_t *sse,                  \
      const uint8_t *second_pred);
#define LAVISH_VAR_PROTOS(w, h)                  \
  LAVISH_VAR_PROTOS_BD(aom_, w, h)               \
  LAVISH_VAR_PROTOS_BD(aom_highbd_8_, w, h)      \
  LAVISH_VAR_PROTOS_BD(aom_highbd_10_, w, h)     \
  LAVISH_VAR_PROTOS_BD(aom_highbd_12_, w, h)

LAVISH_ENCODER_BLOCK_SIZES(LAVISH_SAD_PROTOS)
LAVISH_ENCODER_BLOCK_SIZES(LAVISH_VAR_PROTOS)

/* layout mirror of DIST_WTD_COMP_PARAMS (av1/common/blockd.h:554-558) */
typedef struct LavishDistWtdCompParams {
  int use_dist_wtd_comp_avg;
  int fwd_offset;
  int bck_offset;
} LavishDistWtdCompParams;

/* masked / OBMC / distance-weighted SAD: aom_dsp_rtcd_defs.pl:767, 889, 963,
 * 970, 981, 990, 1007 */
#define LAVISH_COMP_SAD_PROTOS(w, h)                                          \
  unsigned int aom_masked_sad##w##x##h##_hip(                                 \
      const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, \
      const uint8_t *second_pred, const uint8_t *msk, int msk_stride,         \
      int invert_mask);                                                       \
  void aom_masked_sad##w##x##h##x4d_hip(                                      \
      const uint8_t *src, int src_stride, const uint8_t *ref[4],              \
      int ref_stride, const uint8_t *second_pred, const uint8_t *msk,         \
      int msk_stride, int invert_mask, unsigned sads[4]);                     \
  unsigned int aom_highbd_masked_sad##w##x##h##_hip(                          \
      const uint8_t *src8, int src_stride, const uint8_t *ref8,               \
      int ref_stride, const uint8_t *second_pred8, const uint8_t *msk,        \
      int msk_stride, int invert_mask);                                       \
  unsigned int aom_obmc_sad##w##x##h##_hip(const uint8_t *pre, int pre_stride, \
                                           const int32_t *wsrc,               \
                                           const int32_t *mask);              \
  unsigned int aom_highbd_obmc_sad##w##x##h##_hip(                            \
      const uint8_t *pre, int pre_stride, const int32_t *wsrc,                \
      const int32_t *mask);                                                   \
  unsigned int aom_dist_wtd_sad##w##x##h##_avg_hip(                           \
      const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr,         \
      int ref_stride, const uint8_t *second_pred,                             \
      const LavishDistWtdCompParams *jcp_param);                              \
  unsigned int aom_highbd_dist_wtd_sad##w##x##h##_avg_hip(                    \
      const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr,         \
      int ref_stride, const uint8_t *second_pred,                             \
      const LavishDistWtdCompParams *jcp_param);

/* masked / distance-weighted sub-pixel variance: aom_dsp_rtcd_defs.pl:1366,
 * 1513, 1522, 1530 (pre: aom_, aom_highbd_8_, aom_highbd_10_, aom_highbd_12_) */
#define LAVISH_COMP_VAR_PROTOS_BD(pre, w, h)                                  \
  unsigned int pre##masked_sub_pixel_variance##w##x##h##_hip(                 \
      const uint8_t *src, int src_stride, int xoffset, int yoffset,           \
      const uint8_t *ref, int ref_stride, const uint8_t *second_pred,         \
      const uint8_t *msk, int msk_stride, int invert_mask,                    \
      unsigned int *sse);                                                     \
  uint32_t pre##dist_wtd_sub_pixel_avg_variance##w##x##h##_hip(               \
      const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset,    \
      const uint8_t *ref_ptr, int ref_stride, uint32_t *sse,                  \
      const uint8_t *second_pred, const LavishDistWtdCompParams *jcp_param);
/* OBMC variance: aom_dsp_rtcd_defs.pl:1542-1543, 1552-1553 (pre: aom_,
 * aom_highbd_, aom_highbd_10_, aom_highbd_12_) */
#define LAVISH_OBMC_VAR_PROTOS_BD(pre, w, h)                                  \
  unsigned int pre##obmc_variance##w##x##h##_hip(                             \
      const uint8_t *pre_, int pre_stride, const int32_t *wsrc,               \
      const int32_t *mask, unsigned int *sse);                                \
  unsigned int pre##obmc_sub_pixel_variance##w##x##h##_hip(                   \
      const uint8_t *pre_, int pre_stride, int xoffset, int yoffset,          \
      const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
#define LAVISH_COMP_VAR_PROTOS(w, h)                  \
  LAVISH_COMP_VAR_PROTOS_BD(aom_, w, h)               \
  LAVISH_COMP_VAR_PROTOS_BD(aom_highbd_8_, w, h)      \
  LAVISH_COMP_VAR_PROTOS_BD(aom_highbd_10_, w, h)     \
  LAVISH_COMP_VAR_PROTOS_BD(aom_highbd_12_, w, h)     \
  LAVISH_OBMC_VAR_PROTOS_BD(aom_, w, h)               \
  LAVISH_OBMC_VAR_PROTOS_BD(aom_highbd_, w, h)        \
  LAVISH_OBMC_VAR_PROTOS_BD(aom_highbd_10_, w, h)     \
  LAVISH_OBMC_VAR_PROTOS_BD(aom_highbd_12_, w, h)

LAVISH_ENCODER_BLOCK_SIZES(LAVISH_COMP_SAD_PROTOS)
LAVISH_ENCODER_BLOCK_SIZES(LAVISH_COMP_VAR_PROTOS)

/* compound prediction helpers: aom_dsp_rtcd_defs.pl:1602-1606, 1772-1775,
 * 2029-2034.  (width, height) must be one of the 22 encoder block sizes. */
void aom_comp_avg_pred_hip(uint8_t *comp_pred, const uint8_t *pred, int width,
                           int height, const uint8_t *ref, int ref_stride);
void aom_dist_wtd_comp_avg_pred_hip(uint8_t *comp_pred, const uint8_t *pred,
                                    int width, int height, const uint8_t *ref,
                                    int ref_stride,
                                    const LavishDistWtdCompParams *jcp_param);
void aom_comp_mask_pred_hip(uint8_t *comp_pred, const uint8_t *pred, int width,
                            int height, const uint8_t *ref, int ref_stride,
                            const uint8_t *mask, int mask_stride,
                            int invert_mask);
void aom_highbd_comp_avg_pred_hip(uint8_t *comp_pred8, const uint8_t *pred8,
                                  int width, int height, const uint8_t *ref8,
                                  int ref_stride);
void aom_highbd_dist_wtd_comp_avg_pred_hip(
    uint8_t *comp_pred8, const uint8_t *pred8, int width, int height,
    const uint8_t *ref8, int ref_stride,
    const LavishDistWtdCompParams *jcp_param);
void aom_highbd_comp_mask_pred_hip(uint8_t *comp_pred, const uint8_t *pred8,
                                   int width, int height, const uint8_t *ref8,
                                   int ref_stride, const uint8_t *mask,
                                   int mask_stride, int invert_mask);

/* aom_dsp_rtcd_defs.pl:1303-1318,1326-1333 */
#define LAVISH_MSE_PROTOS(pre)                                                 \
  void pre##get16x16var_hip(const uint8_t *src_ptr, int source_stride,        \
                            const uint8_t *ref_ptr, int ref_stride,           \
                            unsigned int *sse, int *sum);                     \
  void pre##get8x8var_hip(const uint8_t *src_ptr, int source_stride,          \
                          const uint8_t *ref_ptr, int ref_stride,             \
                          unsigned int *sse, int *sum);                       \
  unsigned int pre##mse16x16_hip(const uint8_t *src_ptr, int source_stride,   \
                                 const uint8_t *ref_ptr, int recon_stride,    \
                                 unsigned int *sse);                          \
  unsigned int pre##mse16x8_hip(const uint8_t *src_ptr, int source_stride,    \
                                const uint8_t *ref_ptr, int recon_stride,     \
                                unsigned int *sse);                           \
  unsigned int pre##mse8x16_hip(const uint8_t *src_ptr, int source_stride,    \
                                const uint8_t *ref_ptr, int recon_stride,     \
                                unsigned int *sse);                           \
  unsigned int pre##mse8x8_hip(const uint8_t *src_ptr, int source_stride,     \
                               const uint8_t *ref_ptr, int recon_stride,      \
                               unsigned int *sse);
LAVISH_MSE_PROTOS(aom_)
LAVISH_MSE_PROTOS(aom_highbd_8_)
LAVISH_MSE_PROTOS(aom_highbd_10_)
LAVISH_MSE_PROTOS(aom_highbd_12_)

/* aom_dsp_rtcd_defs.pl:725-746 */
void aom_subtract_block_hip(int rows, int cols, int16_t *diff_ptr,
                            ptrdiff_t diff_stride, const uint8_t *src_ptr,
                            ptrdiff_t src_stride, const uint8_t *pred_ptr,
                            ptrdiff_t pred_stride);
void aom_highbd_subtract_block_hip(int rows, int cols, int16_t *diff_ptr,
                                   ptrdiff_t diff_stride,
                                   const uint8_t *src_ptr,
                                   ptrdiff_t src_stride,
                                   const uint8_t *pred_ptr,
                                   ptrdiff_t pred_stride);
int64_t aom_sse_hip(const uint8_t *a, int a_stride, const uint8_t *b,
                    int b_stride, int width, int height);
int64_t aom_highbd_sse_hip(const uint8_t *a8, int a_stride, const uint8_t *b8,
                           int b_stride, int width, int height);
uint64_t aom_sum_squares_2d_i16_hip(const int16_t *src, int stride, int width,
                                    int height);

/* aom_dsp_rtcd_defs.pl:1244-1278 */
void aom_hadamard_4x4_hip(const int16_t *src_diff, ptrdiff_t src_stride,
                          int32_t *coeff);
void aom_hadamard_8x8_hip(const int16_t *src_diff, ptrdiff_t src_stride,
                          int32_t *coeff);
void aom_hadamard_16x16_hip(const int16_t *src_diff, ptrdiff_t src_stride,
                            int32_t *coeff);
void aom_hadamard_32x32_hip(const int16_t *src_diff, ptrdiff_t src_stride,
                            int32_t *coeff);
void aom_highbd_hadamard_8x8_hip(const int16_t *src_diff,
                                 ptrdiff_t src_stride, int32_t *coeff);
void aom_highbd_hadamard_16x16_hip(const int16_t *src_diff,
                                   ptrdiff_t src_stride, int32_t *coeff);
void aom_highbd_hadamard_32x32_hip(const int16_t *src_diff,
                                   ptrdiff_t src_stride, int32_t *coeff);
int aom_satd_hip(const int32_t *coeff, int length);

/* aom_dsp_rtcd_defs.pl:1256-1263,1278 (int16 "low precision" forms) */
void aom_hadamard_lp_8x8_hip(const int16_t *src_diff, ptrdiff_t src_stride,
                             int16_t *coeff);
void aom_hadamard_lp_16x16_hip(const int16_t *src_diff, ptrdiff_t src_stride,
                               int16_t *coeff);
void aom_hadamard_lp_8x8_dual_hip(const int16_t *src_diff, ptrdiff_t src_stride,
                                  int16_t *coeff);
int aom_satd_lp_hip(const int16_t *coeff, int length);
/* aom_dsp_rtcd_defs.pl:770,731 */
uint64_t aom_sum_sse_2d_i16_hip(const int16_t *src, int src_stride, int width,
                                int height, int *sum);
void aom_get_blk_sse_sum_hip(const int16_t *data, int stride, int bw, int bh,
                             int *x_sum, int64_t *x2_sum);

/* av1/common/av1_rtcd_defs.pl:331 */
int64_t av1_block_error_lp_hip(const int16_t *coeff, const int16_t *dqcoeff,
                               intptr_t block_size);
/* av1/common/av1_rtcd_defs.pl:328,423 */
int64_t av1_block_error_hip(const int32_t *coeff, const int32_t *dqcoeff,
                            intptr_t block_size, int64_t *ssz);
int64_t av1_highbd_block_error_hip(const int32_t *coeff,
                                   const int32_t *dqcoeff,
                                   intptr_t block_size, int64_t *ssz, int bd);
/* av1_get_horver_correlation_full (av1/common/av1_rtcd_defs.pl:469) */
void av1_get_horver_correlation_full_hip(const int16_t *diff, int stride, int w,
                                         int h, float *hcorr, float *vcorr);

/* av1_nn_predict (av1/common/av1_rtcd_defs.pl:472) */
void av1_nn_predict_hip(const float *input_nodes, const LavishNNConfig *nn_config,
                        int reduce_prec, float *output);

/* Convolution (av1/common/av1_rtcd_defs.pl:565-575, aom_dsp_rtcd_defs.pl:449,461).
 * Layout mirrors of InterpFilterParams (av1/common/filter.h:105-109) and
 * ConvolveParams (av1/common/convolve.h:21-32). */
typedef struct LavishInterpFilterParams {
  const int16_t *filter_ptr;
  uint16_t taps;
  uint8_t interp_filter;
} LavishInterpFilterParams;
typedef struct LavishConvolveParams {
  int do_average;
  uint16_t *dst;
  int dst_stride;
  int round_0;
  int round_1;
  int plane;
  int is_compound;
  int use_dist_wtd_comp_avg;
  int fwd_offset;
  int bck_offset;
} LavishConvolveParams;
void av1_convolve_2d_sr_hip(const uint8_t *src, int src_stride, uint8_t *dst,
                            int dst_stride, int w, int h,
                            const LavishInterpFilterParams *filter_params_x,
                            const LavishInterpFilterParams *filter_params_y,
                            const int subpel_x_qn, const int subpel_y_qn,
                            LavishConvolveParams *conv_params);
void av1_convolve_x_sr_hip(const uint8_t *src, int src_stride, uint8_t *dst,
                           int dst_stride, int w, int h,
                           const LavishInterpFilterParams *filter_params_x,
                           const int subpel_x_qn, LavishConvolveParams *conv_params);
void av1_convolve_y_sr_hip(const uint8_t *src, int src_stride, uint8_t *dst,
                           int dst_stride, int w, int h,
                           const LavishInterpFilterParams *filter_params_y,
                           const int subpel_y_qn);
void av1_highbd_convolve_2d_sr_hip(const uint16_t *src, int src_stride,
                                   uint16_t *dst, int dst_stride, int w, int h,
                                   const LavishInterpFilterParams *filter_params_x,
                                   const LavishInterpFilterParams *filter_params_y,
                                   const int subpel_x_qn, const int subpel_y_qn,
                                   LavishConvolveParams *conv_params, int bd);
void av1_highbd_convolve_x_sr_hip(const uint16_t *src, int src_stride,
                                  uint16_t *dst, int dst_stride, int w, int h,
                                  const LavishInterpFilterParams *filter_params_x,
                                  const int subpel_x_qn,
                                  LavishConvolveParams *conv_params, int bd);
void av1_highbd_convolve_y_sr_hip(const uint16_t *src, int src_stride,
                                  uint16_t *dst, int dst_stride, int w, int h,
                                  const LavishInterpFilterParams *filter_params_y,
                                  const int subpel_y_qn, int bd);
void aom_convolve_copy_hip(const uint8_t *src, ptrdiff_t src_stride, uint8_t *dst,
                           ptrdiff_t dst_stride, int w, int h);
void aom_highbd_convolve_copy_hip(const uint16_t *src, ptrdiff_t src_stride,
                                  uint16_t *dst, ptrdiff_t dst_stride, int w, int h);


/* ---- affine warp --------------------------------
 * Replaces av1_warp_affine_c (av1/common/warped_motion.c:538-666) and
 * av1_highbd_warp_affine_c (:264-388) for a batch of prediction blocks of
 * one reference plane.  A job is one block: its warp matrix (wmmat[0..5])
 * and shear parameters (av1_get_shear_params), the block position p_col /
 * p_row / p_width / p_height in the predicted plane, the element offset of
 * the reference plane origin (ref_off: several planes may be stacked) and of
 * the block's top-left in pred / conv_dst.  conv_params: round_0, round_1,
 * is_compound, do_average, use_dist_wtd_comp_avg, fwd_offset, bck_offset as
 * the reference reads them (its dst / dst_stride are replaced by conv_dst /
 * dst_stride).  Device pointers; asynchronous on `stream`.  highbd: u16
 * samples (bit_depth 8/10/12), else u8 (bit_depth 8).  Returns 0, or < 0 on
 * rejected arguments. */
typedef struct LavishWarpJob {
  int32_t mat[6];
  int16_t alpha, beta, gamma, delta;
  int32_t p_col, p_row, p_width, p_height;
  int64_t ref_off;
  int64_t pred_off;
  int64_t dst_off;
} LavishWarpJob;
int lavish_warp_affine_batch(const void *ref, int width, int height, int stride, void *pred,
                             int p_stride, uint16_t *conv_dst, int dst_stride,
                             const LavishWarpJob *jobs, int njobs, int subsampling_x,
                             int subsampling_y, int bit_depth, int highbd,
                             const LavishConvolveParams *conv_params, void *stream);
/* av1_get_shear_params (warped_motion.c:218-247) on a host matrix: out =
 * alpha, beta, gamma, delta; returns 1 when the model is usable by the warp
 * filter, else 0. */
int lavish_get_shear_params(const int32_t *mat, int16_t *out);
/* av1/common/av1_rtcd_defs.pl:548,544 (per-call shims, host buffers) */
void av1_warp_affine_hip(const int32_t *mat, const uint8_t *ref, int width, int height,
                         int stride, uint8_t *pred, int p_col, int p_row, int p_width,
                         int p_height, int p_stride, int subsampling_x, int subsampling_y,
                         LavishConvolveParams *conv_params, int16_t alpha, int16_t beta,
                         int16_t gamma, int16_t delta);
void av1_highbd_warp_affine_hip(const int32_t *mat, const uint16_t *ref, int width,
                                int height, int stride, uint16_t *pred, int p_col, int p_row,
                                int p_width, int p_height, int p_stride, int subsampling_x,
                                int subsampling_y, int bd, LavishConvolveParams *conv_params,
                                int16_t alpha, int16_t beta, int16_t gamma, int16_t delta);


/* ---- compound (CONV_BUF) convolutions -----------
 * Replaces av1_dist_wtd_convolve_{2d_copy,x,y,2d}_c and the highbd forms
 * (av1/common/convolve.c:291-489,790-988) for a batch of w x h blocks
 * sharing the x / y filters (InterpFilterParams as the caller holds them:
 * host filter_ptr, taps <= 12) and the conv params (round_0, round_1,
 * do_average, use_dist_wtd_comp_avg, fwd_offset, bck_offset; its dst /
 * dst_stride are replaced by conv_dst / conv_stride).  Per block: the source
 * position (element offset of the block's integer position), the prediction
 * and CONV_BUF offsets and the sub-pel phases (1/16 pel), which choose the
 * path as convolve_2d_facade_compound does.  w, h <= 128.  Device pointers;
 * asynchronous on `stream`. */
typedef struct LavishCompoundJob {
  int64_t src_off;
  int64_t dst_off;
  int64_t conv_off;
  int32_t subpel_x_qn, subpel_y_qn;
} LavishCompoundJob;
int lavish_dist_wtd_convolve_batch(const void *src, int src_stride, void *dst, int dst_stride,
                                   uint16_t *conv_dst, int conv_stride, int w, int h,
                                   const LavishCompoundJob *jobs, int njobs,
                                   const LavishInterpFilterParams *filter_params_x,
                                   const LavishInterpFilterParams *filter_params_y,
                                   const LavishConvolveParams *conv_params, int bit_depth,
                                   int highbd, void *stream);
/* av1/common/av1_rtcd_defs.pl:568-579 (per-call shims, host buffers) */
void av1_dist_wtd_convolve_2d_hip(const uint8_t *src, int src_stride, uint8_t *dst,
                                  int dst_stride, int w, int h,
                                  const LavishInterpFilterParams *filter_params_x,
                                  const LavishInterpFilterParams *filter_params_y,
                                  const int subpel_x_qn, const int subpel_y_qn,
                                  LavishConvolveParams *conv_params);
void av1_dist_wtd_convolve_2d_copy_hip(const uint8_t *src, int src_stride, uint8_t *dst,
                                       int dst_stride, int w, int h,
                                       LavishConvolveParams *conv_params);
void av1_dist_wtd_convolve_x_hip(const uint8_t *src, int src_stride, uint8_t *dst,
                                 int dst_stride, int w, int h,
                                 const LavishInterpFilterParams *filter_params_x,
                                 const int subpel_x_qn, LavishConvolveParams *conv_params);
void av1_dist_wtd_convolve_y_hip(const uint8_t *src, int src_stride, uint8_t *dst,
                                 int dst_stride, int w, int h,
                                 const LavishInterpFilterParams *filter_params_y,
                                 const int subpel_y_qn, LavishConvolveParams *conv_params);
void av1_highbd_dist_wtd_convolve_2d_hip(const uint16_t *src, int src_stride, uint16_t *dst,
                                         int dst_stride, int w, int h,
                                         const LavishInterpFilterParams *filter_params_x,
                                         const LavishInterpFilterParams *filter_params_y,
                                         const int subpel_x_qn, const int subpel_y_qn,
                                         LavishConvolveParams *conv_params, int bd);
void av1_highbd_dist_wtd_convolve_x_hip(const uint16_t *src, int src_stride, uint16_t *dst,
                                        int dst_stride, int w, int h,
                                        const LavishInterpFilterParams *filter_params_x,
                                        const int subpel_x_qn,
                                        LavishConvolveParams *conv_params, int bd);
void av1_highbd_dist_wtd_convolve_y_hip(const uint16_t *src, int src_stride, uint16_t *dst,
                                        int dst_stride, int w, int h,
                                        const LavishInterpFilterParams *filter_params_y,
                                        const int subpel_y_qn,
                                        LavishConvolveParams *conv_params, int bd);
void av1_highbd_dist_wtd_convolve_2d_copy_hip(const uint16_t *src, int src_stride,
                                              uint16_t *dst, int dst_stride, int w, int h,
                                              LavishConvolveParams *conv_params, int bd);

/* ---- scaled convolution --------------------------
 * Replaces av1_convolve_2d_scale_c / av1_highbd_convolve_2d_scale_c
 * (av1/common/convolve.c:488-574,992-1078) -- the inter predictor of a
 * reference of another resolution (convolve_2d_scale_wrapper :576-588) --
 * for a batch of w x h blocks sharing the x / y filters (host
 * InterpFilterParams, taps <= 12) and the conv params (round_0, round_1,
 * is_compound, do_average, use_dist_wtd_comp_avg, fwd_offset, bck_offset;
 * its dst / dst_stride are replaced by conv_dst / conv_stride).  Per block:
 * the element offset of the block's integer source position, the
 * prediction and CONV_BUF offsets, and the scaled start positions and steps
 * in 1/1024 pel (SCALE_SUBPEL_BITS): subpel_*_qn in [0, 1023], *_step_qn in
 * [1, 2048] (a block outside them is left untouched).  w a power of two in
 * [2, 128], h in [1, 128].  Device pointers; asynchronous on `stream`.
 * highbd: u16 samples (bit_depth 8/10/12), else u8.  Returns 0, or < 0 on
 * rejected arguments. */
typedef struct LavishScaleJob {
  int64_t src_off;
  int64_t dst_off;
  int64_t conv_off;
  int32_t subpel_x_qn, x_step_qn, subpel_y_qn, y_step_qn;
} LavishScaleJob;
int lavish_convolve_2d_scale_batch(const void *src, int src_stride, void *dst, int dst_stride,
                                   uint16_t *conv_dst, int conv_stride, int w, int h,
                                   const LavishScaleJob *jobs, int njobs,
                                   const LavishInterpFilterParams *filter_params_x,
                                   const LavishInterpFilterParams *filter_params_y,
                                   const LavishConvolveParams *conv_params, int bit_depth,
                                   int highbd, void *stream);
/* av1/common/av1_rtcd_defs.pl:580,583 (per-call shims, host buffers) */
void av1_convolve_2d_scale_hip(const uint8_t *src, int src_stride, uint8_t *dst,
                               int dst_stride, int w, int h,
                               const LavishInterpFilterParams *filter_params_x,
                               const LavishInterpFilterParams *filter_params_y,
                               const int subpel_x_qn, const int x_step_qn,
                               const int subpel_y_qn, const int y_step_qn,
                               LavishConvolveParams *conv_params);
void av1_highbd_convolve_2d_scale_hip(const uint16_t *src, int src_stride, uint16_t *dst,
                                      int dst_stride, int w, int h,
                                      const LavishInterpFilterParams *filter_params_x,
                                      const LavishInterpFilterParams *filter_params_y,
                                      const int subpel_x_qn, const int x_step_qn,
                                      const int subpel_y_qn, const int y_step_qn,
                                      LavishConvolveParams *conv_params, int bd);

/* ---- intra prediction ------------------------------------------------------
 * lavish_intra_pred_batch is build_intra_predictors / build_intra_predictors_high
 * (av1/common/reconintra.c:1133-1477) for a list of jobs, bit-exact: edge
 * assembly from the counts, the non-directional predictors, the directional
 * path (corner filter, edge filter, upsampling, z1 / z2 / z3) and filter
 * intra.  A job carries what av1_predict_intra_block hands down
 * (reconintra.c:1634-1650); the availability walk (has_top_right /
 * has_bottom_left, get_intra_edge_filter_type) stays with the caller.
 * Planes and jobs are device memory; pixels are uint8_t for bit_depth 8 and
 * uint16_t for 10 / 12.  Jobs of any sizes and modes mix in one call.  A job
 * reads only the pixels its counts declare available, and reads all of them
 * before its first store, so dst may be the plane ref points into; jobs of one
 * call must not read what another job of the call writes.  Asynchronous on
 * `stream`.  Returns 0, or a negative value for a refused argument (null
 * plane, bit_depth not 8 / 10 / 12); njobs <= 0 is a no-op.  A job whose
 * tx_size / mode / filter_intra_mode is out of range (or filter intra above
 * 32x32, or a directional mode whose p_angle is not its base angle + 3 * delta,
 * delta in -3 .. 3) is skipped on the device: validate on the host
 * (lavish_dsp.intra.intra_jobs does).  The record is 48 bytes. */
typedef struct LavishIntraJob {
  int64_t ref_off;  /* element offset of the block's top-left pixel in ref        */
  int64_t dst_off;  /* and in dst                                                 */
  uint8_t tx_size;  /* TX_4X4 .. TX_64X16 (0 .. 18)                               */
  uint8_t mode;     /* DC_PRED .. PAETH_PRED (0 .. 12)                            */
  uint8_t filter_intra_mode;      /* 0 .. 4; 5 (FILTER_INTRA_MODES): none         */
  uint8_t disable_edge_filter;
  uint8_t intra_edge_filter_type; /* 0 or 1                                       */
  uint8_t reserved[3];
  int32_t p_angle;                /* directional modes: base angle + 3 * delta    */
  int32_t n_top_px, n_topright_px;    /* -1 for a corner count: not needed        */
  int32_t n_left_px, n_bottomleft_px;
  int32_t reserved2;
} LavishIntraJob;
int lavish_intra_pred_batch(const void *ref, int ref_stride, void *dst, int dst_stride,
                            const LavishIntraJob *jobs, int njobs, int bit_depth,
                            void *stream);
/* the tables of csrc/intra_tables.h (for tests): which = 0 smooth weights
 * [124], 1 derivative by angle [90], 2 filter-intra taps [5][8][8], 3 edge
 * kernels [3][5], 4 mode to angle [13]; copies up to `cap` values into out as
 * int32 and returns the table's length (0: no such table) */
int lavish_intra_table(int which, int32_t *out, int cap);

/* Per-call shims (host buffers) with the reference's prototypes.
 * aom_dsp/aom_dsp_rtcd_defs.pl:60-86: the ten predictor families over the 19
 * block sizes, 8-bit and highbd (uint16_t pointers, not tagged): 380 entries.
 * above / left are read at the reference's extents (above[-1] for paeth). */
#define LAVISH_INTRA_SIZES(X, t)                                                     \
  X(t, 4, 4) X(t, 8, 8) X(t, 16, 16) X(t, 32, 32) X(t, 64, 64) X(t, 4, 8) X(t, 8, 4) \
  X(t, 8, 16) X(t, 16, 8) X(t, 16, 32) X(t, 32, 16) X(t, 32, 64) X(t, 64, 32)        \
  X(t, 4, 16) X(t, 16, 4) X(t, 8, 32) X(t, 32, 8) X(t, 16, 64) X(t, 64, 16)
#define LAVISH_INTRA_TYPES(X)                                                          \
  LAVISH_INTRA_SIZES(X, dc) LAVISH_INTRA_SIZES(X, dc_top) LAVISH_INTRA_SIZES(X, dc_left) \
  LAVISH_INTRA_SIZES(X, dc_128) LAVISH_INTRA_SIZES(X, v) LAVISH_INTRA_SIZES(X, h)      \
  LAVISH_INTRA_SIZES(X, paeth) LAVISH_INTRA_SIZES(X, smooth)                           \
  LAVISH_INTRA_SIZES(X, smooth_v) LAVISH_INTRA_SIZES(X, smooth_h)
#define LAVISH_INTRA_DECL(t, W, H)                                                   \
  void aom_##t##_predictor_##W##x##H##_hip(uint8_t *dst, ptrdiff_t y_stride,         \
                                           const uint8_t *above, const uint8_t *left); \
  void aom_highbd_##t##_predictor_##W##x##H##_hip(uint16_t *dst, ptrdiff_t y_stride, \
                                                  const uint16_t *above,             \
                                                  const uint16_t *left, int bd);
LAVISH_INTRA_TYPES(LAVISH_INTRA_DECL)
#undef LAVISH_INTRA_DECL
/* av1/common/av1_rtcd_defs.pl:105-114 */
void av1_dr_prediction_z1_hip(uint8_t *dst, ptrdiff_t stride, int bw, int bh,
                              const uint8_t *above, const uint8_t *left,
                              int upsample_above, int dx, int dy);
void av1_dr_prediction_z2_hip(uint8_t *dst, ptrdiff_t stride, int bw, int bh,
                              const uint8_t *above, const uint8_t *left,
                              int upsample_above, int upsample_left, int dx, int dy);
void av1_dr_prediction_z3_hip(uint8_t *dst, ptrdiff_t stride, int bw, int bh,
                              const uint8_t *above, const uint8_t *left,
                              int upsample_left, int dx, int dy);
/* tx_size: TX_SIZE; up to 32x32 */
void av1_filter_intra_predictor_hip(uint8_t *dst, ptrdiff_t stride, uint8_t tx_size,
                                    const uint8_t *above, const uint8_t *left, int mode);
/* av1_rtcd_defs.pl:247-253 */
void av1_highbd_dr_prediction_z1_hip(uint16_t *dst, ptrdiff_t stride, int bw, int bh,
                                     const uint16_t *above, const uint16_t *left,
                                     int upsample_above, int dx, int dy, int bd);
void av1_highbd_dr_prediction_z2_hip(uint16_t *dst, ptrdiff_t stride, int bw, int bh,
                                     const uint16_t *above, const uint16_t *left,
                                     int upsample_above, int upsample_left, int dx, int dy,
                                     int bd);
void av1_highbd_dr_prediction_z3_hip(uint16_t *dst, ptrdiff_t stride, int bw, int bh,
                                     const uint16_t *above, const uint16_t *left,
                                     int upsample_left, int dx, int dy, int bd);
/* av1_rtcd_defs.pl:605-613: in place on p (the upsampler
 * writes p[-2 .. 2 * sz - 2], both ends included: 2 * sz + 1 elements) */
void av1_filter_intra_edge_hip(uint8_t *p, int sz, int strength);
void av1_upsample_intra_edge_hip(uint8_t *p, int sz);
void av1_filter_intra_edge_high_hip(uint16_t *p, int sz, int strength);
void av1_upsample_intra_edge_high_hip(uint16_t *p, int sz, int bd);

/* ---- chroma from luma (UV_CFL_PRED) -----------------------------------------
 * av1/common/cfl.c and the alpha estimate of cfl_pick_plane_parameter
 * (av1/encoder/intra_mode_search.c:608-643), bit-exact.  Planes, AC cells and
 * job tables are device memory; pixels are uint8_t (highbd 0, bit_depth 8) or
 * uint16_t (highbd 1, bit_depth 8 / 10 / 12).  The transform sizes are the 14
 * with both sides <= 32.  A job table is a plain int64_t [njobs][COLS] array,
 * its columns named below.  An AC cell is the reference's ac_buf_q3: 32 x 32
 * int16_t at CFL_BUF_LINE (32) stride, of which only the W x H corner of the
 * chroma tx_size is written and read.  Every *_elems argument is the number of
 * elements of its plane: a job whose tx_size, cell index or rectangle falls
 * outside what the call declares is skipped on the device and writes nothing
 * (validate on the host: lavish_dsp.cfl's builders do).  Asynchronous on
 * `stream`.  Return 0, or negative: -1 null pointer, -5 bit depth / highbd,
 * -6 subsampling (sub_x, sub_y) = (0, 1) or outside 0 .. 1 (the reference
 * routes (0, 1) to its 4:4:4 function by accident of cfl_subsampling_lbd),
 * -7 stride / element count.  njobs <= 0 is a no-op. */
enum { LAVISH_CFL_AC_LUMA_OFF, LAVISH_CFL_AC_LUMA_W, LAVISH_CFL_AC_LUMA_H,
       LAVISH_CFL_AC_TX_SIZE, LAVISH_CFL_AC_COLS };
enum { LAVISH_CFL_PRED_CELL, LAVISH_CFL_PRED_DST_OFF, LAVISH_CFL_PRED_TX_SIZE,
       LAVISH_CFL_PRED_ALPHA_Q3, LAVISH_CFL_PRED_COLS };
enum { LAVISH_CFL_SEARCH_CELL, LAVISH_CFL_SEARCH_SRC_OFF, LAVISH_CFL_SEARCH_DC_OFF,
       LAVISH_CFL_SEARCH_TX_SIZE, LAVISH_CFL_SEARCH_COLS };
/* cfl_store (cfl.c:324-369) followed by cfl_compute_parameters (:177-185): job
 * j subsamples the stored luma rectangle (element offset LUMA_OFF, LUMA_W x
 * LUMA_H luma pixels, multiples of 4 up to 32, no larger after subsampling than
 * the chroma TX_SIZE), pads it to the transform (cfl_pad), subtracts the
 * rounded average and writes cell j of ac_cells. */
int lavish_cfl_ac_batch(const void *luma, int luma_stride, int64_t luma_elems, int sub_x,
                        int sub_y, const int64_t *jobs, int njobs, int16_t *ac_cells,
                        int bit_depth, int highbd, void *stream);
/* cfl_predict_lbd_c / cfl_predict_hbd_c (cfl.c:147-172) in place on dst, which
 * holds the DC prediction on entry: dst = clip(dst + ROUND_POWER_OF_TWO_SIGNED(
 * ALPHA_Q3 * ac, 6)), ALPHA_Q3 in -16 .. 16.  Many jobs may read one cell; the
 * blocks of a call's jobs must not overlap. */
int lavish_cfl_predict_batch(const int16_t *ac_cells, int64_t ncells, void *dst, int dst_stride,
                             int64_t dst_elems, const int64_t *jobs, int njobs, int bit_depth,
                             int highbd, void *stream);
/* The fast leg of cfl_pick_plane_parameter for one chroma plane of a block per
 * job: costs[j][idx], idx 0 .. 32, is aom_satd of the DCT_DCT forward 2-D
 * transform of src - cfl prediction with alpha_q3 = idx - 16 on the DC
 * prediction block at DC_OFF of dc (read, never written); est_idx[j] is the
 * index the reference's walk ends on (up from 16 while the cost falls
 * strictly, then down from 15 against the same running best).  One transform
 * block per plane (the uv transform of a block <= 32x32 is the plane block). */
int lavish_cfl_alpha_search_batch(const int16_t *ac_cells, int64_t ncells, const void *src,
                                  int src_stride, int64_t src_elems, const void *dc,
                                  int dc_stride, int64_t dc_elems, const int64_t *jobs,
                                  int njobs, int32_t *costs, uint8_t *est_idx, int bit_depth,
                                  int highbd, void *stream);
/* Host: the two estimates as the block's parameters (intra_mode_search.c:
 * 747-752, 802-804).  Returns 0 when both are CFL_INDEX_ZERO (16): no valid CfL
 * mode, *alpha_idx = *joint_sign = 0; otherwise 1 with *alpha_idx =
 * (cfl_alpha_u << 4) + cfl_alpha_v and *joint_sign = cfl_sign_u * CFL_SIGNS +
 * cfl_sign_v - 1.  -1 for an estimate outside 0 .. 32. */
int lavish_cfl_joint(int est_u, int est_v, uint8_t *alpha_idx, int8_t *joint_sign);
/* Size-generic per-call forms on host buffers (the entries of
 * lavish_dsp_cfl.h are these at the 14 sizes); width / height in {4, 8, 16,
 * 32}, output_q3 / src / dst / ac_buf_q3 at CFL_BUF_LINE stride as in the
 * reference.  cfl_luma_subsampling_{420,422,444}_{lbd,hbd}_c (width x height
 * luma pixels in), subtract_average_c, cfl_predict_{lbd,hbd}_c. */
void lavish_cfl_subsample_host(const void *input, int input_stride, uint16_t *output_q3,
                               int width, int height, int sub_x, int sub_y, int highbd);
void lavish_cfl_subtract_average_host(const uint16_t *src, int16_t *dst, int width, int height);
void lavish_cfl_predict_host(const int16_t *ac_buf_q3, void *dst, int dst_stride, int alpha_q3,
                             int bit_depth, int width, int height, int highbd);

#ifdef __cplusplus
}
#endif
#endif /* LAVISH_DSP_H_ */
