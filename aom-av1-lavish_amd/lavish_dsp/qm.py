"""Quantization matrices on the MI355X backend: av1_quant, the trellis and the
transform-domain distortion with `using_qmatrix` set (av1/encoder/
av1_quantize.c:70-563, aom_dsp/quantize.c:108-316, av1/encoder/
txb_rdopt_utils.h:39-64, av1/encoder/tx_search.c:1049-1116).

The matrices are the caller's: QmTables holds a copy of the reference's
wt_matrix_ref / iwt_matrix_ref level tables on the device and hands out the
(qm, iqm) views a block runs with, as av1_set_qmatrix + av1_setup_qmatrix
would choose them."""
import ctypes

import numpy as np

from . import (PlaneQuant, QuantParams, _lib, _p, _p_t, _stream_ptr, max_eob)

_vp, _i32 = ctypes.c_void_p, ctypes.c_int32

NUM_QM_LEVELS = 16
QM_TOTAL_SIZE = 3344
IDTX = 9  # tx types from IDTX on (identity and 1-D) run flat
DIST_NONE, DIST_TX_DOMAIN, DIST_QM_PSNR = range(3)

_lib.lavish_qm_level.argtypes = [_i32, _i32, _i32]
_lib.lavish_qm_level.restype = _i32
_lib.lavish_qm_table_offset.argtypes = [_i32]
_lib.lavish_qm_table_offset.restype = _i32
_lib.lavish_quantize_qm_batch.argtypes = [_vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32,
                                          ctypes.POINTER(QuantParams), _vp, _vp, _vp, _vp, _vp,
                                          _vp]
_lib.lavish_quantize_qm_batch.restype = _i32
_lib.lavish_av1_quant_qm_batch.argtypes = [_vp, _i32, _i32, _i32, _i32,
                                           ctypes.POINTER(PlaneQuant), _i32, _i32,
                                           ctypes.c_uint32, _i32, _vp, _vp, _vp, _i32, _vp, _vp,
                                           _vp, _vp, _vp, _vp, _vp]
_lib.lavish_av1_quant_qm_batch.restype = _i32
_lib.lavish_block_error_qm_batch.argtypes = [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]
_lib.lavish_block_error_qm_batch.restype = _i32
_lib.lavish_optimize_b_qm_batch.argtypes = [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32,
                                            _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp,
                                            _vp]
_lib.lavish_optimize_b_qm_batch.restype = _i32
_lib.aom_quantize_b_helper_hip.argtypes = [_vp, ctypes.c_ssize_t, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _i32]
_lib.aom_quantize_b_helper_hip.restype = None


def qm_level(qindex, first, last):
    """aom_get_qmlevel (av1/common/quant_common.h:57-59)."""
    return _lib.lavish_qm_level(qindex, first, last)


def table_offset(tx_size):
    """Element offset of tx_size's matrix inside one [3344] level table
    (av1_qm_init, av1/common/quant_common.c:283-309)."""
    off = _lib.lavish_qm_table_offset(tx_size)
    if off < 0:
        raise ValueError("bad tx_size %d" % tx_size)
    return off


class QmTables:
    """The caller's level tables on the device: wt / iwt uint8
    [15][2][3344] (level, luma / chroma, QM_TOTAL_SIZE), as wt_matrix_ref /
    iwt_matrix_ref are laid out."""

    def __init__(self, wt, iwt, device="cuda"):
        import torch
        shape = (NUM_QM_LEVELS - 1, 2, QM_TOTAL_SIZE)
        wt = np.ascontiguousarray(wt, np.uint8)
        iwt = np.ascontiguousarray(iwt, np.uint8)
        assert wt.shape == shape and iwt.shape == shape
        self.wt = torch.from_numpy(wt).to(device)
        self.iwt = torch.from_numpy(iwt).to(device)

    def views(self, level, plane, tx_size, tx_type=0):
        """(qm, iqm) device views of n = max_eob(tx_size) weights for a block
        of `plane` at `level`; (None, None) for level 15 and for identity /
        1-D types (av1_get_qmatrix, quant_common.c:249-275)."""
        if level == NUM_QM_LEVELS - 1 or tx_type >= IDTX:
            return None, None
        assert 0 <= level < NUM_QM_LEVELS - 1
        off, n = table_offset(tx_size), max_eob(tx_size)
        c = int(plane >= 1)
        return self.wt[level, c, off:off + n], self.iwt[level, c, off:off + n]


def _mat(m, n):
    import torch
    if m is None:
        return None
    assert m.dtype == torch.uint8 and m.is_cuda and m.is_contiguous() and m.numel() >= n
    return _p_t(m)


def _check(rc, name):
    if rc != 0:
        raise ValueError("%s rejected its arguments (rc=%d)" % (name, rc))


def quantize_qm_batch(coeff, scan, log_scale, qp, qm=None, iqm=None, bit_depth=8, quant_kind=0,
                      stream=None):
    """lavish_quantize_qm_batch: coeff device int32 [nblocks, n], scan device
    int16 [n], qm / iqm device uint8 [n] or None.  Returns (qcoeff, dqcoeff,
    eob)."""
    import torch
    nb, n = coeff.shape
    assert coeff.dtype == torch.int32 and coeff.is_contiguous() and coeff.is_cuda
    assert scan.dtype == torch.int16 and scan.numel() >= n and scan.is_cuda
    q, dq = torch.empty_like(coeff), torch.empty_like(coeff)
    eob = torch.empty((nb,), dtype=torch.int16, device=coeff.device)
    _check(_lib.lavish_quantize_qm_batch(_p_t(coeff), n, nb, _p_t(scan), None, log_scale,
                                         bit_depth, quant_kind, ctypes.byref(qp), _mat(qm, n),
                                         _mat(iqm, n), _p_t(q), _p_t(dq), _p_t(eob),
                                         _stream_ptr(stream)), "lavish_quantize_qm_batch")
    return q, dq, eob


def av1_quant_qm_batch(coeff, tx_size, tx_type, bit_depth, pq, mode, qm=None, iqm=None,
                       dist_mode=DIST_NONE, skip_trellis=0, threshold=0xFFFFFFFF, qstep=0,
                       dc_only=None, out=None, stream=None):
    """lavish_av1_quant_qm_batch over a device int32 [nblocks, n] tensor.
    Returns (qcoeff, dqcoeff, eob, flags, dist, sse); dist / sse are device
    int64 [nblocks], or None with DIST_NONE.  out: (qcoeff, dqcoeff, eob) to
    write into (AV1_QUANT_SKIP leaves them as they are)."""
    import torch
    n = max_eob(tx_size)
    assert coeff.dtype == torch.int32 and coeff.is_contiguous() and coeff.shape[-1] == n
    assert coeff.is_cuda
    nb = coeff.numel() // n
    if out is None:
        qc, dq = torch.empty_like(coeff), torch.empty_like(coeff)
        eob = torch.empty(nb, dtype=torch.int16, device=coeff.device)
    else:
        qc, dq, eob = out
        assert qc.dtype == dq.dtype == torch.int32 and qc.numel() == dq.numel() == coeff.numel()
        assert eob.dtype in (torch.int16, torch.uint16) and eob.numel() >= nb
    flags = torch.empty(nb, dtype=torch.uint8, device=coeff.device)
    dist = sse = None
    if dist_mode != DIST_NONE:
        dist = torch.empty(nb, dtype=torch.int64, device=coeff.device)
        sse = torch.empty(nb, dtype=torch.int64, device=coeff.device)
    if dc_only is not None:
        assert dc_only.dtype == torch.uint8 and dc_only.numel() >= nb and dc_only.is_cuda
    _check(_lib.lavish_av1_quant_qm_batch(
        _p_t(coeff), nb, tx_size, tx_type, bit_depth, ctypes.byref(pq), mode, skip_trellis,
        threshold, qstep, _p_t(dc_only) if dc_only is not None else None, _mat(qm, n),
        _mat(iqm, n), dist_mode, _p_t(qc), _p_t(dq), _p_t(eob), _p_t(flags),
        _p_t(dist) if dist is not None else None, _p_t(sse) if sse is not None else None,
        _stream_ptr(stream)), "lavish_av1_quant_qm_batch")
    return qc, dq, eob, flags, dist, sse


def block_error_qm_batch(coeff, dqcoeff, qmatrix, scan, stream=None):
    """lavish_block_error_qm_batch (av1_block_error_qm): coeff / dqcoeff
    device int32 [nblocks, n], qmatrix device uint8 [n], scan device int16 [n].
    Returns (err, ssz), device int64 [nblocks]."""
    import torch
    nb, n = coeff.shape
    for t in (coeff, dqcoeff):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert dqcoeff.shape == coeff.shape
    assert scan.dtype == torch.int16 and scan.numel() >= n and scan.is_cuda
    err = torch.empty(nb, dtype=torch.int64, device=coeff.device)
    ssz = torch.empty(nb, dtype=torch.int64, device=coeff.device)
    _check(_lib.lavish_block_error_qm_batch(_p_t(coeff), _p_t(dqcoeff), n, nb, _mat(qmatrix, n),
                                            _p_t(scan), _p_t(err), _p_t(ssz),
                                            _stream_ptr(stream)), "lavish_block_error_qm_batch")
    return err, ssz


def optimize_b_qm_batch(costs, tcoeff, qcoeff, dqcoeff, eob, tx_size, tx_type, bit_depth, rdmult,
                        dequant, iqm=None, qm_dist=None, plane=0, is_inter=1, sharpness=0,
                        txb_ctx=None, tx_type_cost=0, rate=None, entropy_ctx=None, stream=None):
    """lavish_optimize_b_qm_batch: txb.optimize_b_batch with iqm (get_dqv's
    weights) and qm_dist (the QM-PSNR matrix of get_coeff_dist), device uint8
    [n] or None.  qcoeff / dqcoeff / eob are updated in place.  Returns (rate,
    entropy_ctx)."""
    import torch
    n = max_eob(tx_size)
    for t in (tcoeff, qcoeff, dqcoeff):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.shape[-1] == n and t.is_cuda
    nb = qcoeff.numel() // n
    assert tcoeff.numel() == qcoeff.numel() == dqcoeff.numel()
    assert eob.dtype in (torch.int16, torch.uint16) and eob.numel() >= nb and eob.is_cuda
    if txb_ctx is not None:
        assert txb_ctx.dtype == torch.int32 and txb_ctx.is_contiguous()
        assert txb_ctx.numel() >= 2 * nb and txb_ctx.is_cuda
    if rate is None:
        rate = torch.empty(nb, dtype=torch.int32, device=qcoeff.device)
    if entropy_ctx is None:
        entropy_ctx = torch.empty(nb, dtype=torch.uint8, device=qcoeff.device)
    dqv = np.ascontiguousarray(dequant, np.int16)
    assert dqv.shape == (2,)
    _check(_lib.lavish_optimize_b_qm_batch(
        _vp(costs.t.data_ptr()), _p_t(tcoeff), _p_t(qcoeff), _p_t(dqcoeff), _p_t(eob), nb, plane,
        tx_size, tx_type, bit_depth, is_inter, rdmult, sharpness, dqv.ctypes.data_as(_vp),
        _mat(iqm, n), _mat(qm_dist, n), _p_t(txb_ctx) if txb_ctx is not None else None,
        tx_type_cost, _p_t(rate), _p_t(entropy_ctx), _stream_ptr(stream)),
        "lavish_optimize_b_qm_batch")
    return rate, entropy_ctx


def aom_quantize_b_helper(coeff_ptr, n_coeffs, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr,
                          qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, scan, iscan, qm_ptr,
                          iqm_ptr, log_scale):
    """aom_quantize_b_helper_hip on host (numpy) buffers; qm_ptr / iqm_ptr
    uint8 arrays or None."""
    _lib.aom_quantize_b_helper_hip(
        _p(coeff_ptr), n_coeffs, _p(zbin_ptr), _p(round_ptr), _p(quant_ptr), _p(quant_shift_ptr),
        _p(qcoeff_ptr), _p(dqcoeff_ptr), _p(dequant_ptr), _p(eob_ptr), _p(scan), _p(iscan),
        _p(qm_ptr) if qm_ptr is not None else None,
        _p(iqm_ptr) if iqm_ptr is not None else None, log_scale)
