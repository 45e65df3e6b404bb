"""numpy restatement of the reference's quantization-matrix arithmetic, for
the free-parameter cases of tests/test_gpu_qm.py (the fixture rows come from
the reference itself; tests/test_qm_cpu.py holds this file against them).

  quantize_fp   quantize_fp_helper_c / highbd_quantize_fp_helper_c
                (av1/encoder/av1_quantize.c:70-122, 125-198)
  quantize_b    aom_quantize_b_helper_c / aom_highbd_quantize_b_helper_c
                (aom_dsp/quantize.c:108-169, 261-316)
  quantize_dc   quantize_dc / highbd_quantize_dc (av1_quantize.c:374-405,
                516-545)
  block_error_qm, block_error, dist_block_tx_domain
                (av1/encoder/tx_search.c:1049-1116, rdopt.c:635-682)
  get_dqv, coeff_dist
                (av1/encoder/txb_rdopt_utils.h:39-64)

All arithmetic is int64 with the reference's int casts restated as 32-bit
wraps.  A NULL matrix is None (weight 32 = 1 << AOM_QM_BITS)."""
import numpy as np

AOM_QM_BITS = 5
QM_TOTAL_SIZE = 3344
TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
# LavishPlaneQuant field order of the fixture's "qtab" [bd][qindex][field][2]
QTAB_FIELDS = ("zbin", "round_fp", "quant_fp", "round", "quant", "quant_shift", "dequant")


def tx_scale(s):  # av1_get_tx_scale (av1/common/idct.c:24-28)
    p = TX_W[s] * TX_H[s]
    return int(p > 256) + int(p > 1024)


def adjusted_tx_size(s):  # av1_get_adjusted_tx_size (av1/common/blockd.h:1361-1370)
    return {4: 3, 11: 3, 12: 3, 17: 9, 18: 10}.get(s, s)


def max_eob(s):
    return min(TX_W[s], 32) * min(TX_H[s], 32)


def wrap32(v):
    """(int) of an int64 value."""
    v = np.asarray(v, np.int64)
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def rshift_signed(v, sh):
    """RIGHT_SIGNED_SHIFT (av1/common/common.h); a negative count shifts left,
    as dist_block_tx_domain's (MAX_TX_SCALE - tx_scale) * 2 gives for the
    64-point sizes."""
    v = int(v)
    if sh < 0:
        return v << -sh
    return v >> sh if v >= 0 else -((-v) >> sh)


def matrix(F, level, plane, tx_size, offsets=None):
    """(qm, iqm) of the fixture's stored level tables: av1_qm_init's pointers
    (quant_common.c:283-309); level 15 is NULL."""
    if level == 15:
        return None, None
    offsets = F["table_offsets"] if offsets is None else offsets
    li = list(F["levels"]).index(level)
    o, n = int(offsets[tx_size]), max_eob(tx_size)
    c = int(plane >= 1)
    return F["wt"][li, c, o:o + n], F["iwt"][li, c, o:o + n]


def _w(m, n):
    return np.full(n, 1 << AOM_QM_BITS, np.int64) if m is None else np.asarray(m, np.int64)


def _finish(c, absq, dequant_w, ls, scan):
    sign = c < 0
    q = np.where(sign, -absq, absq)
    adq = wrap32(absq * dequant_w) >> ls  # an int multiply: wraps
    dq = np.where(sign, -adq, adq)
    nz = np.nonzero(absq[scan])[0]
    return q.astype(np.int32), dq.astype(np.int32), int(nz[-1]) + 1 if len(nz) else 0


def _pair(v, n):
    ac = np.arange(n) != 0
    return np.where(ac, int(v[1]), int(v[0])).astype(np.int64)


def quantize_fp(coeff, rnd, quant, dequant, scan, qm, iqm, ls, hbd):
    c = np.asarray(coeff, np.int64)
    n = len(c)
    wt, iwt = _w(qm, n), _w(iqm, n)
    deq, qt = _pair(dequant, n), _pair(quant, n)
    rounding = (_pair(rnd, n) + ((1 << ls) >> 1)) >> ls  # ROUND_POWER_OF_TWO
    dequant_w = (deq * iwt + (1 << (AOM_QM_BITS - 1))) >> AOM_QM_BITS
    a = np.abs(c)
    passed = a * wt >= (deq << (AOM_QM_BITS - (1 + ls)))
    t = a + rounding
    if not hbd:
        t = np.clip(t, -32768, 32767)  # clamp64 before the weight (:110)
    absq = wrap32((t * wt * qt) >> (16 - ls + AOM_QM_BITS))
    absq = np.where(passed, absq, 0)
    return _finish(c, absq, dequant_w, ls, np.asarray(scan, np.int64))


def quantize_b(coeff, zbin, rnd, quant, quant_shift, dequant, scan, qm, iqm, ls, hbd):
    c = np.asarray(coeff, np.int64)
    n = len(c)
    wt, iwt = _w(qm, n), _w(iqm, n)
    zb = (_pair(zbin, n) + ((1 << ls) >> 1)) >> ls
    rounding = (_pair(rnd, n) + ((1 << ls) >> 1)) >> ls
    deq, qt, qs = _pair(dequant, n), _pair(quant, n), _pair(quant_shift, n)
    dequant_w = (deq * iwt + (1 << (AOM_QM_BITS - 1))) >> AOM_QM_BITS
    a = np.abs(c)
    # the pre-scan and the quantization pass test the same thing per
    # coefficient (|coeff| * wt >= zbin * 32) for |coeff| * wt < 2^31
    passed = a * wt >= zb * (1 << AOM_QM_BITS)
    t = a + rounding
    if not hbd:
        t = np.clip(t, -32768, 32767)  # the int16 clamp before the weight (:150)
    t = t * wt
    absq = wrap32((((t * qt) >> 16) + t) * qs >> (16 - ls + AOM_QM_BITS))
    absq = np.where(passed, absq, 0)
    return _finish(c, absq, dequant_w, ls, np.asarray(scan, np.int64))


def quantize_dc(coeff, rnd0, quant0, dequant0, qm, iqm, ls, hbd):
    c = np.asarray(coeff, np.int64)
    n = len(c)
    wt = 32 if qm is None else int(qm[0])
    iwt = 32 if iqm is None else int(iqm[0])
    t = abs(int(c[0])) + ((int(rnd0) + ((1 << ls) >> 1)) >> ls)
    if not hbd:
        t = max(-32768, min(32767, t))
    absq = int(wrap32((t * wt * int(quant0)) >> (16 - ls + AOM_QM_BITS)))
    dequant_w = (int(dequant0) * iwt + 16) >> AOM_QM_BITS
    adq = int(wrap32(absq * dequant_w)) >> ls
    q, dq = np.zeros(n, np.int32), np.zeros(n, np.int32)
    q[0] = -absq if c[0] < 0 else absq
    dq[0] = -adq if c[0] < 0 else adq
    return q, dq, int(absq != 0)


def block_error_qm(coeff, dqcoeff, qmatrix, scan):
    """av1_block_error_qm: coeff[i] (raster) with qmatrix[scan[i]], as written."""
    c, d = np.asarray(coeff, np.int64), np.asarray(dqcoeff, np.int64)
    w = np.asarray(qmatrix, np.int64)[np.asarray(scan, np.int64)]
    dd, cc = (c - d) * w, c * w
    r = 1 << (2 * AOM_QM_BITS - 1)
    return (int(((dd * dd + r) >> (2 * AOM_QM_BITS)).sum()),
            int(((cc * cc + r) >> (2 * AOM_QM_BITS)).sum()))


def block_error(coeff, dqcoeff, bd):
    """av1_block_error_c (int products) / av1_highbd_block_error_c."""
    c, d = np.asarray(coeff, np.int64), np.asarray(dqcoeff, np.int64)
    if bd == 8:
        diff = wrap32(c - d)
        return int(wrap32(diff * diff).sum()), int(wrap32(c * c).sum())
    sh = 2 * (bd - 8)
    r = 1 << (sh - 1)
    return int((((c - d) ** 2).sum() + r) >> sh), int(((c * c).sum() + r) >> sh)


def dist_block_tx_domain(coeff, dqcoeff, tx_size, bd, qmatrix, scan, use_qm_dist_metric):
    if qmatrix is None or not use_qm_dist_metric:
        e, s = block_error(coeff, dqcoeff, bd)
    else:
        e, s = block_error_qm(coeff, dqcoeff, qmatrix, scan)  # no bd shift (:1098-1100)
    sh = (1 - tx_scale(tx_size)) * 2
    return rshift_signed(e, sh), rshift_signed(s, sh)


def get_dqv(dequant, ci, iqmatrix):
    dqv = int(dequant[int(ci != 0)])
    if iqmatrix is not None:
        dqv = (int(iqmatrix[ci]) * dqv + (1 << (AOM_QM_BITS - 1))) >> AOM_QM_BITS
    return dqv


def coeff_dist(tcoeff, dqcoeff, shift, qmatrix, ci):
    diff = (int(tcoeff) - int(dqcoeff)) * (1 << shift)
    if qmatrix is None:
        return diff * diff
    diff *= int(qmatrix[ci])
    return (diff * diff + (1 << (2 * AOM_QM_BITS - 1))) >> (2 * AOM_QM_BITS)
