// quant_qm.hip -- the quantization-matrix forms of av1_quant and of the
// transform-domain distortion for a batch of blocks on gfx950 (SURVEY.md
// section 8 row a9, with `using_qmatrix` set).
//
// Reference, per block and transform type (search_tx_type, av1/encoder/
// tx_search.c:2148-2169):
//   av1_setup_qmatrix (encodemb.c:374-380) -> av1_get_qmatrix / _iqmatrix
//     (av1/common/quant_common.c:249-275): the segment's matrices of
//     av1_get_adjusted_tx_size(tx_size), NULL (flat) for tx_type >= IDTX;
//   av1_quant -> the facades of av1/encoder/av1_quantize.c:266-563.  FP and B
//     take the helper bodies only when BOTH pointers are set (:272,344 and
//     the highbd forms): quantize_fp_helper_c (:70-122),
//     highbd_quantize_fp_helper_c (:125-198), aom_quantize_b_helper_c /
//     aom_highbd_quantize_b_helper_c (aom_dsp/quantize.c:108-169,261-316);
//     otherwise the flat quantizers of quant_facade.hip.  The DC facades
//     (:374-420, 516-563) weight with each pointer on its own;
//   dist_block_tx_domain (tx_search.c:1073-1116): av1_block_error /
//     av1_highbd_block_error, or av1_block_error_qm (:1049-1071) when
//     use_qm_dist_metric is set and the matrix is not NULL -- raster coeff[i]
//     against qmatrix[scan[i]], and no >> 2 (bd - 8) on high bit depth --
//     then RIGHT_SIGNED_SHIFT by (MAX_TX_SCALE - tx_scale) * 2.
// The matrices are the caller's device tables (n bytes, raster); the level
// tables themselves (wt_matrix_ref / iwt_matrix_ref) stay with the caller.
//
// One wave64 per block like av1_quant_kernel: the satd gate, the n
// coefficients lane-strided through quant_qm_dev.h, the eob as a max-reduce
// of the inverse scan, and the distortion sums from the coefficients the
// lanes still hold.
#include <climits>

#include "lavish_internal.h"
#include "quant_qm_dev.h"

namespace lavish {

int quantize_qm_batch(const int32_t* coeff, int n, int nblocks, const int16_t* scan,
                      int log_scale, int bd, int quant_kind, const LavishQuantParams* qp,
                      const uint8_t* qm, const uint8_t* iqm, int32_t* qcoeff, int32_t* dqcoeff,
                      uint16_t* eob, hipStream_t s);

namespace {

// sqrt_tx_pixels_2d (av1/encoder/tx_search.c:76-78)
__constant__ int kSqrtPx[19] = {4, 8, 16, 32, 32, 6, 6, 12, 12, 23, 23, 32, 32, 8, 8, 16, 16, 23, 23};

struct QmArgs {
  const int32_t* coeff;
  const int16_t* iscan;
  const int16_t* scan;
  const uint8_t* dc_only;
  const uint8_t* qm;   // effective: nullptr for tx_type >= IDTX
  const uint8_t* iqm;
  int32_t* qcoeff;
  int32_t* dqcoeff;
  uint16_t* eob;
  uint8_t* flags;
  int64_t* dist;
  int64_t* sse;
  int n, nblocks, tx_size, bd, mode, skip_trellis, qstep, dist_mode;
  unsigned threshold;
  QP fp, b;  // FP: round_fp / quant_fp in round / quant; B: the b tables
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += (int64_t)__shfl_xor((long long)v, m);
  return v;
}

// RIGHT_SIGNED_SHIFT by (MAX_TX_SCALE - tx_scale) * 2; the 64-point sizes'
// count of -2 shifts left, as rdo_kern.h's tx_dist has it
template <int LS>
__device__ __forceinline__ int64_t tx_shift(int64_t v) {
  constexpr int sh = (1 - LS) * 2;
  if constexpr (sh >= 0) return v >= 0 ? v >> sh : -((-v) >> sh);
  else return (int64_t)((uint64_t)v << -sh);
}

template <int LS, bool HBD>
__global__ __launch_bounds__(64) void av1_quant_qm_kernel(QmArgs a) {
  const int blk = blockIdx.x, lane = threadIdx.x;
  const int32_t* c = a.coeff + (int64_t)blk * a.n;
  int kind = a.mode;
  int optb = 0;
  if (a.mode == LAVISH_AV1_QUANT_SATD_GATE) {  // reads the raw coefficients: as av1_quant_kernel
    if (a.skip_trellis || a.threshold == UINT_MAX) {
      kind = a.skip_trellis ? LAVISH_AV1_QUANT_B : LAVISH_AV1_QUANT_FP;
      optb = !a.skip_trellis;
    } else {
      const bool dc = a.dc_only != nullptr && a.dc_only[blk] != 0;
      int s = 0;
      if (dc) {
        s = abs(c[0]);
      } else {
        for (int i = lane; i < a.n; i += 64) s += abs(c[i]);
        s = wave_sum(s);
      }
      const int shift = 1 - LS;  // MAX_TX_SCALE - av1_get_tx_scale
      s = shift < 0 ? s << -shift : s >> shift;
      s >>= a.bd - 8;
      const bool skip = (uint64_t)(int64_t)s >
                        (uint64_t)a.threshold * (uint64_t)(int64_t)a.qstep *
                            (uint64_t)kSqrtPx[a.tx_size];
      kind = skip ? LAVISH_AV1_QUANT_B : LAVISH_AV1_QUANT_FP;
      optb = !skip;
    }
  }
  if (lane == 0 && a.flags) a.flags[blk] = (uint8_t)(optb | (kind << 1));
  const bool skipq = kind == LAVISH_AV1_QUANT_SKIP;  // outputs untouched; the distortion reads them
  if (skipq && a.dist_mode == 0) return;
  int32_t* q = a.qcoeff + (int64_t)blk * a.n;
  int32_t* dq = a.dqcoeff + (int64_t)blk * a.n;
  const bool helper = a.qm != nullptr && a.iqm != nullptr;  // the facades' rule
  const bool fp = kind == LAVISH_AV1_QUANT_FP;
  const bool qmdist = a.dist_mode == 2 && a.qm != nullptr;
  int last = 0;
  int64_t err = 0, ssz = 0;
  for (int i = lane; i < a.n; i += 64) {
    const int32_t x = c[i];
    const int32_t sgn = x >> 31;
    const int32_t ax = (x ^ sgn) - sgn;
    const bool ac = i != 0;
    int32_t qv = 0, dv = 0;
    if (skipq) {
      dv = dq[i];
    } else if (kind == LAVISH_AV1_QUANT_DC) {
      if (i == 0) {
        const int32_t mag = qm::dc_mag<LS, HBD>(ax, a.b.round[0], a.fp.quant[0], qm::weight(a.qm, 0));
        const int32_t dm = qm::dequant_mag<LS>(
            mag, qm::weighted_dequant(a.fp.dequant[0], qm::weight(a.iqm, 0)));
        qv = (mag ^ sgn) - sgn;
        dv = (dm ^ sgn) - sgn;
        last = mag != 0 ? 1 : 0;
      }
    } else if (helper) {
      const int wt = a.qm[i];
      const int32_t mag = fp ? qm::fp_mag<LS, HBD>(ax, ac, a.fp, wt) : qm::b_mag<LS, HBD>(ax, ac, a.b, wt);
      const int32_t dm = qm::dequant_mag<LS>(
          mag, qm::weighted_dequant(ac ? a.fp.dequant[1] : a.fp.dequant[0], a.iqm[i]));
      qv = (mag ^ sgn) - sgn;
      dv = (dm ^ sgn) - sgn;
      last = mag != 0 ? max(last, a.iscan[i] + 1) : last;
    } else {  // flat: av1_quant_kernel's code
      qv = fp ? quant_one<LS, LAVISH_QUANT_FP, HBD>(x, ac, a.fp)
              : quant_one<LS, LAVISH_QUANT_B, HBD>(x, ac, a.b);
      dv = dequant_one<LS>(qv, ac, fp ? a.fp : a.b);
      last = qv != 0 ? max(last, a.iscan[i] + 1) : last;
    }
    if (!skipq) {
      q[i] = qv;
      dq[i] = dv;
    }
    if (a.dist_mode != 0) {
      if (qmdist) {  // av1_block_error_qm: coeff[i] with qmatrix[scan[i]]
        const int wt = a.qm[a.scan[i]];
        err += qm::err_term_qm((int64_t)(x - dv), wt);
        ssz += qm::err_term_qm((int64_t)x, wt);
      } else if (HBD) {  // av1_highbd_block_error_c
        const int64_t d = x - dv;
        err += d * d;
        ssz += (int64_t)x * (int64_t)x;
      } else {  // av1_block_error_c: int products
        const uint32_t d = (uint32_t)(x - dv);
        err += (int32_t)(d * d);
        ssz += (int32_t)((uint32_t)x * (uint32_t)x);
      }
    }
  }
  if (!skipq) {
    last = wave_max(last);
    if (lane == 0) a.eob[blk] = (uint16_t)last;
  }
  if (a.dist_mode != 0) {
    err = wave_sum64(err);
    ssz = wave_sum64(ssz);
    if (lane == 0) {
      if (HBD && !qmdist) {
        const int sh = 2 * (a.bd - 8);
        const int64_t r = (int64_t)1 << (sh - 1);
        err = (err + r) >> sh;
        ssz = (ssz + r) >> sh;
      }
      a.dist[blk] = tx_shift<LS>(err);
      a.sse[blk] = tx_shift<LS>(ssz);
    }
  }
}

// the four helpers on their own, walking `scan` like quant_kernel (txq.hip);
// each of qm / iqm nullable as the helper bodies allow
template <int LS>
__global__ __launch_bounds__(256) void quantize_qm_kernel(const int32_t* coeff, int n,
                                                          const int16_t* scan, int kind, int highbd,
                                                          QP qp, const uint8_t* qmat,
                                                          const uint8_t* iqmat, int32_t* qcoeff,
                                                          int32_t* dqcoeff, uint16_t* eob) {
  __shared__ int red[4];
  const size_t base = (size_t)blockIdx.x * n;
  const int tid = threadIdx.x;
  int last = 0;
  for (int i = tid; i < n; i += 256) {
    const int rc = scan[i];
    const int32_t x = coeff[base + rc];
    const int32_t sgn = x >> 31;
    const int32_t ax = (x ^ sgn) - sgn;
    const bool ac = rc != 0;
    const int wt = qm::weight(qmat, rc);
    int32_t mag;
    if (kind == LAVISH_QUANT_FP)
      mag = highbd ? qm::fp_mag<LS, true>(ax, ac, qp, wt) : qm::fp_mag<LS, false>(ax, ac, qp, wt);
    else
      mag = highbd ? qm::b_mag<LS, true>(ax, ac, qp, wt) : qm::b_mag<LS, false>(ax, ac, qp, wt);
    const int32_t dm = qm::dequant_mag<LS>(
        mag, qm::weighted_dequant(ac ? qp.dequant[1] : qp.dequant[0], qm::weight(iqmat, rc)));
    qcoeff[base + rc] = (mag ^ sgn) - sgn;
    dqcoeff[base + rc] = (dm ^ sgn) - sgn;
    if (mag != 0) last = max(last, i + 1);
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) last = max(last, __shfl_xor(last, m));
  if ((tid & 63) == 0) red[tid >> 6] = last;
  __syncthreads();
  if (tid == 0) eob[blockIdx.x] = (uint16_t)max(max(red[0], red[1]), max(red[2], red[3]));
}

// av1_block_error_qm alone: one wave per block
__global__ __launch_bounds__(64) void block_error_qm_kernel(const int32_t* coeff,
                                                            const int32_t* dqcoeff, int n,
                                                            const uint8_t* qmat, const int16_t* scan,
                                                            int64_t* err, int64_t* ssz) {
  const int blk = blockIdx.x, lane = threadIdx.x;
  const int32_t* c = coeff + (int64_t)blk * n;
  const int32_t* d = dqcoeff + (int64_t)blk * n;
  int64_t e = 0, s = 0;
  for (int i = lane; i < n; i += 64) {
    const int wt = qmat[scan[i]];
    const int32_t x = c[i];
    e += qm::err_term_qm((int64_t)(x - d[i]), wt);
    s += qm::err_term_qm((int64_t)x, wt);
  }
  e = wave_sum64(e);
  s = wave_sum64(s);
  if (lane == 0) {
    err[blk] = e;
    ssz[blk] = s;
  }
}

QP qp_fp(const LavishPlaneQuant& p) {
  QP q{};
  for (int i = 0; i < 2; ++i) {
    q.zbin[i] = p.zbin[i];
    q.round[i] = p.round_fp[i];
    q.quant[i] = p.quant_fp[i];
    q.quant_shift[i] = p.quant_shift[i];
    q.dequant[i] = p.dequant[i];
  }
  return q;
}
QP qp_b(const LavishPlaneQuant& p) {
  QP q{};
  for (int i = 0; i < 2; ++i) {
    q.zbin[i] = p.zbin[i];
    q.round[i] = p.round[i];
    q.quant[i] = p.quant[i];
    q.quant_shift[i] = p.quant_shift[i];
    q.dequant[i] = p.dequant[i];
  }
  return q;
}

}  // namespace

int quantize_qm_batch(const int32_t* coeff, int n, int nblocks, const int16_t* scan,
                      int log_scale, int bd, int quant_kind, const LavishQuantParams* qp,
                      const uint8_t* qmat, const uint8_t* iqmat, int32_t* qcoeff,
                      int32_t* dqcoeff, uint16_t* eob, hipStream_t s) {
  if (n <= 0 || qp == nullptr) return -1;
  if (log_scale < 0 || log_scale > 2) return -2;
  if (quant_kind != LAVISH_QUANT_FP && quant_kind != LAVISH_QUANT_B) return -3;
  if (bd != 8 && bd != 10 && bd != 12) return -4;
  if (coeff == nullptr || scan == nullptr || qcoeff == nullptr || dqcoeff == nullptr ||
      eob == nullptr)
    return -5;
  if (nblocks <= 0) return 0;
  QP q{};
  for (int i = 0; i < 2; ++i) {
    q.zbin[i] = qp->zbin[i];
    q.round[i] = qp->round[i];
    q.quant[i] = qp->quant[i];
    q.quant_shift[i] = qp->quant_shift[i];
    q.dequant[i] = qp->dequant[i];
  }
  const int hb = bd > 8;
#define LAVISH_QQ(LS)                                                                         \
  if (log_scale == LS)                                                                        \
    hipLaunchKernelGGL(quantize_qm_kernel<LS>, dim3(nblocks), dim3(256), 0, s, coeff, n, scan, \
                       quant_kind, hb, q, qmat, iqmat, qcoeff, dqcoeff, eob);
  LAVISH_QQ(0)
  LAVISH_QQ(1)
  LAVISH_QQ(2)
#undef LAVISH_QQ
  LAVISH_CHECK(hipGetLastError());
  return 0;
}

}  // namespace lavish

using namespace lavish;

// aom_get_qmlevel (av1/common/quant_common.h:57-59)
extern "C" int lavish_qm_level(int qindex, int first, int last) {
  return first + (qindex * (last + 1 - first)) / 256;  // QINDEX_RANGE
}

// av1_qm_init's layout of one [QM_TOTAL_SIZE = 3344] level table
// (av1/common/quant_common.c:283-309): the sizes that are their own
// av1_get_adjusted_tx_size are laid out in TX_SIZE order, tx_size_2d entries
// each; the 64-point sizes reuse 32x32 / 32x16 / 16x32
extern "C" int lavish_qm_table_offset(int tx_size) {
  if (tx_size < 0 || tx_size >= 19) return -1;
  static const int adjusted[19] = {0, 1, 2, 3, 3, 5, 6, 7, 8, 9, 10, 3, 3, 13, 14, 15, 16, 9, 10};
  int current = 0;
  for (int t = 0; t < adjusted[tx_size]; ++t)
    if (adjusted[t] == t) current += tx_w(t) * tx_h(t);
  return current;
}

extern "C" int lavish_quantize_qm_batch(const int32_t* coeff, int n, int nblocks,
                                        const int16_t* scan, const int16_t* iscan, int log_scale,
                                        int bit_depth, int quant_kind, const LavishQuantParams* qp,
                                        const uint8_t* qm, const uint8_t* iqm, int32_t* qcoeff,
                                        int32_t* dqcoeff, uint16_t* eob, void* stream) {
  (void)iscan;  // the reference helpers walk `scan` only
  return quantize_qm_batch(coeff, n, nblocks, scan, log_scale, bit_depth, quant_kind, qp, qm, iqm,
                           qcoeff, dqcoeff, eob, (hipStream_t)stream);
}

extern "C" int lavish_av1_quant_qm_batch(const int32_t* coeff, int nblocks, int tx_size,
                                         int tx_type, int bit_depth, const LavishPlaneQuant* pq,
                                         int mode, int skip_trellis,
                                         unsigned coeff_opt_satd_threshold, int qstep,
                                         const uint8_t* dc_only, const uint8_t* qm,
                                         const uint8_t* iqm, int dist_mode, int32_t* qcoeff,
                                         int32_t* dqcoeff, uint16_t* eob, uint8_t* flags,
                                         int64_t* dist, int64_t* sse, void* stream) {
  if (tx_size < 0 || tx_size >= 19 || tx_type < 0 || tx_type >= 16) return -1;
  if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -2;
  if (mode < LAVISH_AV1_QUANT_FP || mode > LAVISH_AV1_QUANT_SATD_GATE) return -3;
  if (pq == nullptr || coeff == nullptr || qcoeff == nullptr || dqcoeff == nullptr ||
      eob == nullptr)
    return -4;
  if (dist_mode < 0 || dist_mode > 2) return -5;
  if (dist_mode > 0 && (dist == nullptr || sse == nullptr)) return -6;
  if (nblocks <= 0) return 0;
  const bool flat_type = tx_type >= 9;  // av1_get_qmatrix: 1-D and identity types are flat
  QmArgs a{};
  a.coeff = coeff;
  a.iscan = dev_iscan(tx_size, tx_type);
  a.scan = dev_scan(tx_size, tx_type);
  a.dc_only = dc_only;
  a.qm = flat_type ? nullptr : qm;
  a.iqm = flat_type ? nullptr : iqm;
  a.qcoeff = qcoeff;
  a.dqcoeff = dqcoeff;
  a.eob = eob;
  a.flags = flags;
  a.dist = dist;
  a.sse = sse;
  a.n = max_eob(tx_size);
  a.nblocks = nblocks;
  a.tx_size = tx_size;
  a.bd = bit_depth;
  a.mode = mode;
  a.skip_trellis = skip_trellis;
  a.qstep = qstep;
  a.dist_mode = dist_mode;
  a.threshold = coeff_opt_satd_threshold;
  a.fp = qp_fp(*pq);
  a.b = qp_b(*pq);
  const int ls = tx_scale(tx_size);
  hipStream_t s = (hipStream_t)stream;
  const bool hbd = bit_depth > 8;
#define LAVISH_QF(LS)                                                                           \
  if (ls == LS) {                                                                               \
    if (hbd) hipLaunchKernelGGL((av1_quant_qm_kernel<LS, true>), dim3(nblocks), dim3(64), 0, s, a); \
    else hipLaunchKernelGGL((av1_quant_qm_kernel<LS, false>), dim3(nblocks), dim3(64), 0, s, a);    \
  }
  LAVISH_QF(0)
  LAVISH_QF(1)
  LAVISH_QF(2)
#undef LAVISH_QF
  LAVISH_CHECK(hipGetLastError());
  return 0;
}

extern "C" int lavish_block_error_qm_batch(const int32_t* coeff, const int32_t* dqcoeff, int n,
                                           int nblocks, const uint8_t* qmatrix,
                                           const int16_t* scan, int64_t* err, int64_t* ssz,
                                           void* stream) {
  if (n <= 0) return -1;
  if (coeff == nullptr || dqcoeff == nullptr || qmatrix == nullptr || scan == nullptr ||
      err == nullptr || ssz == nullptr)
    return -4;
  if (nblocks <= 0) return 0;
  hipLaunchKernelGGL(block_error_qm_kernel, dim3(nblocks), dim3(64), 0, (hipStream_t)stream, coeff,
                     dqcoeff, n, qmatrix, scan, err, ssz);
  LAVISH_CHECK(hipGetLastError());
  return 0;
}
