"""Intra prediction (include/lavish_dsp.h, "intra prediction").

Two layers, as in blend.py:

* ``intra_jobs`` builds and validates a LavishIntraJob array on the host,
  ``intra_pred_batch`` runs it on torch device planes (asynchronous on the
  current torch stream);
* per-call functions named like the reference's rtcd entries
  (``aom_dc_predictor_16x16``, ``aom_highbd_smooth_predictor_8x32``,
  ``av1_dr_prediction_z2``, ``av1_filter_intra_edge`` ...) on numpy arrays with
  the reference's argument meaning -- they call the ``*_hip`` shims.  above /
  left are (array, index) pairs where the function reads below index 0.
"""
import ctypes

import numpy as np

from . import TX_H, TX_SIZES, TX_W, _lib, _stream_ptr
from .pixel import _check, _d

_vp, _i32, _pd = ctypes.c_void_p, ctypes.c_int32, ctypes.c_ssize_t

INTRA_JOB_DTYPE = np.dtype([("ref_off", "<i8"), ("dst_off", "<i8"), ("tx_size", "u1"),
                            ("mode", "u1"), ("filter_intra_mode", "u1"),
                            ("disable_edge_filter", "u1"), ("intra_edge_filter_type", "u1"),
                            ("reserved", "u1", (3,)), ("p_angle", "<i4"), ("n_top_px", "<i4"),
                            ("n_topright_px", "<i4"), ("n_left_px", "<i4"),
                            ("n_bottomleft_px", "<i4"), ("reserved2", "<i4")], align=True)
assert INTRA_JOB_DTYPE.itemsize == 48

(DC_PRED, V_PRED, H_PRED, D45_PRED, D135_PRED, D113_PRED, D157_PRED, D203_PRED, D67_PRED,
 SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, PAETH_PRED) = range(13)
INTRA_MODES = 13
FILTER_INTRA_MODES = 5  # filter_intra_mode: none
MODE_TO_ANGLE = (0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0)
PRED_TYPES = ("dc", "dc_top", "dc_left", "dc_128", "v", "h", "paeth", "smooth", "smooth_v",
              "smooth_h")

_lib.lavish_intra_pred_batch.argtypes = [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp]
_lib.lavish_intra_pred_batch.restype = _i32
_lib.lavish_intra_table.argtypes = [_i32, _vp, _i32]
_lib.lavish_intra_table.restype = _i32

SHIM_NAMES = ["aom_%s%s_predictor_%s" % (hb, t, s) for t in PRED_TYPES for s in TX_SIZES
              for hb in ("", "highbd_")]
for _n in SHIM_NAMES:
    _f = getattr(_lib, _n + "_hip")
    _f.argtypes = [_vp, _pd, _vp, _vp] + ([_i32] if "highbd" in _n else [])
    _f.restype = None
_DR = [_vp, _pd, _i32, _i32, _vp, _vp]
for _n, _a in (("av1_dr_prediction_z1", _DR + [_i32] * 3), ("av1_dr_prediction_z2", _DR + [_i32] * 4),
               ("av1_dr_prediction_z3", _DR + [_i32] * 3),
               ("av1_highbd_dr_prediction_z1", _DR + [_i32] * 4),
               ("av1_highbd_dr_prediction_z2", _DR + [_i32] * 5),
               ("av1_highbd_dr_prediction_z3", _DR + [_i32] * 4),
               ("av1_filter_intra_predictor", [_vp, _pd, ctypes.c_uint8, _vp, _vp, _i32]),
               ("av1_filter_intra_edge", [_vp, _i32, _i32]),
               ("av1_upsample_intra_edge", [_vp, _i32]),
               ("av1_filter_intra_edge_high", [_vp, _i32, _i32]),
               ("av1_upsample_intra_edge_high", [_vp, _i32, _i32])):
    _f = getattr(_lib, _n + "_hip")
    _f.argtypes = _a
    _f.restype = None
    SHIM_NAMES.append(_n)
BATCH_NAMES = ["lavish_intra_pred_batch"]


def intra_table(which):
    """Table `which` of csrc/intra_tables.h as an int32 array (lavish_intra_table)."""
    n = _lib.lavish_intra_table(which, None, 0)
    out = np.zeros(n, np.int32)
    _lib.lavish_intra_table(which, out.ctypes.data_as(_vp), n)
    return out


# ---------------------------------------------------------- batch layer --
def intra_jobs(ref_off, dst_off, tx_size, mode, p_angle=None, filter_intra_mode=FILTER_INTRA_MODES,
               disable_edge_filter=0, intra_edge_filter_type=0, n_top_px=None, n_topright_px=-1,
               n_left_px=None, n_bottomleft_px=-1):
    """A validated INTRA_JOB_DTYPE array (LavishIntraJob) from scalars or
    equal-length sequences, the values av1_predict_intra_block hands to
    build_intra_predictors.  p_angle defaults to the mode's base angle,
    n_top_px / n_left_px to the full dimension.  Raises ValueError for what
    the kernel must not be given."""
    cols = [np.atleast_1d(np.asarray(v, np.int64)) if v is not None else None
            for v in (ref_off, dst_off, tx_size, mode, p_angle, filter_intra_mode,
                      disable_edge_filter, intra_edge_filter_type, n_top_px, n_topright_px,
                      n_left_px, n_bottomleft_px)]
    n = max(len(c) for c in cols if c is not None)
    cols = [np.broadcast_to(c, (n,)) if c is not None else None for c in cols]
    (ro, do, tx, md, pa, fi, dis, ft, nt, ntr, nl, nbl) = cols
    if ((tx < 0) | (tx > 18)).any():
        raise ValueError("tx_size outside 0 .. 18")
    if ((md < 0) | (md >= INTRA_MODES)).any():
        raise ValueError("mode outside DC_PRED .. PAETH_PRED")
    if ((fi < 0) | (fi > FILTER_INTRA_MODES)).any():
        raise ValueError("filter_intra_mode outside 0 .. 5")
    w, h = np.array(TX_W)[tx], np.array(TX_H)[tx]
    use_fi = fi != FILTER_INTRA_MODES
    if (use_fi & ((w > 32) | (h > 32))).any():
        raise ValueError("filter intra above 32x32")
    if pa is None:
        pa = np.array(MODE_TO_ANGLE)[md]
    is_dr = (md >= V_PRED) & (md <= D67_PRED) & ~use_fi
    if (is_dr & ((pa <= 0) | (pa >= 270))).any():
        raise ValueError("directional mode with p_angle outside (0, 270)")
    delta3 = pa - np.array(MODE_TO_ANGLE)[md]
    if (is_dr & ((np.abs(delta3) > 9) | (delta3 % 3 != 0))).any():
        raise ValueError("p_angle is not the mode's base angle + 3 * delta, delta in -3 .. 3")
    if ((ft < 0) | (ft > 1)).any():
        raise ValueError("intra_edge_filter_type outside 0 .. 1")
    nt = w if nt is None else nt
    nl = h if nl is None else nl
    if ((nt < 0) | (nl < 0) | (ntr < -1) | (nbl < -1)).any():
        raise ValueError("negative pixel count")
    if ((nt > w) | (ntr > w) | (nl > h) | (nbl > h)).any():
        raise ValueError("pixel count above the block dimension")
    if ((ntr > 0) & (nt != w)).any():
        raise ValueError("n_topright_px > 0 needs n_top_px == the block width")
    if ((nbl > 0) & (nl != h)).any():
        raise ValueError("n_bottomleft_px > 0 needs n_left_px == the block height")
    jobs = np.zeros(n, INTRA_JOB_DTYPE)
    for name, v in (("ref_off", ro), ("dst_off", do), ("tx_size", tx), ("mode", md),
                    ("p_angle", pa), ("filter_intra_mode", fi), ("disable_edge_filter", dis != 0),
                    ("intra_edge_filter_type", ft), ("n_top_px", nt), ("n_topright_px", ntr),
                    ("n_left_px", nl), ("n_bottomleft_px", nbl)):
        jobs[name] = v
    return jobs


def intra_jobs_tensor(jobs, device):
    """Upload an INTRA_JOB_DTYPE numpy array as a device byte tensor."""
    import torch
    assert jobs.dtype == INTRA_JOB_DTYPE
    return torch.from_numpy(np.ascontiguousarray(jobs).view(np.uint8).copy()).to(device)


def intra_pred_batch(ref, dst, jobs, bit_depth=8, ref_stride=None, dst_stride=None, stream=None):
    """lavish_intra_pred_batch.  ref / dst: device tensors, 2-D planes (stride =
    row stride) or 1-D with the strides given; uint8 for bit_depth 8, 16-bit
    (int16 / uint16 tensors) for 10 / 12.  dst may be ref.  jobs: an
    intra_jobs_tensor."""
    if ref.element_size() != (1 if bit_depth == 8 else 2) or dst.element_size() != ref.element_size():
        raise ValueError("pixels are uint8 for bit_depth 8 and 16-bit for 10 / 12")
    nj = jobs.numel() // INTRA_JOB_DTYPE.itemsize
    _check(_lib.lavish_intra_pred_batch(
        _d(ref), ref.stride(0) if ref_stride is None else ref_stride,
        _d(dst), dst.stride(0) if dst_stride is None else dst_stride, _d(jobs), nj, bit_depth,
        _stream_ptr(stream)), "lavish_intra_pred_batch")


# ------------------------------------------------- per-call RTCD mirror --
def _at(a, i=0):
    """Pointer to element i of a contiguous 1-D numpy array (or to a view's first)."""
    assert a.strides[-1] == a.itemsize
    return _vp(a.ctypes.data + i * a.itemsize)


def _make_pred(name, highbd):
    f = getattr(_lib, name + "_hip")
    dt = np.uint16 if highbd else np.uint8

    def pred(dst, y_stride, above, left, bd=None, above_index=0, left_index=0):
        assert dst.dtype == dt and above.dtype == dt and left.dtype == dt
        args = [_at(dst), y_stride, _at(above, above_index), _at(left, left_index)]
        f(*(args + ([bd] if highbd else [])))
    pred.__name__ = name
    pred.__doc__ = "aom_dsp_rtcd_defs.pl:60-86; above_index / left_index: where [0] is"
    return pred


for _n in SHIM_NAMES:
    if "_predictor_" in _n and _n.startswith("aom_"):
        globals()[_n] = _make_pred(_n, "highbd" in _n)


def _dr(name, highbd, dst, stride, bw, bh, above, ai, left, li, tail):
    dt = np.uint16 if highbd else np.uint8
    assert dst.dtype == dt and above.dtype == dt and left.dtype == dt
    getattr(_lib, name + "_hip")(_at(dst), stride, bw, bh, _at(above, ai), _at(left, li), *tail)


def av1_dr_prediction_z1(dst, stride, bw, bh, above, left, upsample_above, dx, dy, above_index=0,
                         left_index=0):
    """av1_rtcd_defs.pl:105."""
    _dr("av1_dr_prediction_z1", 0, dst, stride, bw, bh, above, above_index, left, left_index,
        [upsample_above, dx, dy])


def av1_dr_prediction_z2(dst, stride, bw, bh, above, left, upsample_above, upsample_left, dx, dy,
                         above_index=0, left_index=0):
    _dr("av1_dr_prediction_z2", 0, dst, stride, bw, bh, above, above_index, left, left_index,
        [upsample_above, upsample_left, dx, dy])


def av1_dr_prediction_z3(dst, stride, bw, bh, above, left, upsample_left, dx, dy, above_index=0,
                         left_index=0):
    _dr("av1_dr_prediction_z3", 0, dst, stride, bw, bh, above, above_index, left, left_index,
        [upsample_left, dx, dy])


def av1_highbd_dr_prediction_z1(dst, stride, bw, bh, above, left, upsample_above, dx, dy, bd,
                                above_index=0, left_index=0):
    _dr("av1_highbd_dr_prediction_z1", 1, dst, stride, bw, bh, above, above_index, left,
        left_index, [upsample_above, dx, dy, bd])


def av1_highbd_dr_prediction_z2(dst, stride, bw, bh, above, left, upsample_above, upsample_left,
                                dx, dy, bd, above_index=0, left_index=0):
    _dr("av1_highbd_dr_prediction_z2", 1, dst, stride, bw, bh, above, above_index, left,
        left_index, [upsample_above, upsample_left, dx, dy, bd])


def av1_highbd_dr_prediction_z3(dst, stride, bw, bh, above, left, upsample_left, dx, dy, bd,
                                above_index=0, left_index=0):
    _dr("av1_highbd_dr_prediction_z3", 1, dst, stride, bw, bh, above, above_index, left,
        left_index, [upsample_left, dx, dy, bd])


def av1_filter_intra_predictor(dst, stride, tx_size, above, left, mode, above_index=0,
                               left_index=0):
    """av1_rtcd_defs.pl:113: reads above[-1 .. w) and left[0 .. h)."""
    assert dst.dtype == np.uint8 and above.dtype == np.uint8 and left.dtype == np.uint8
    _lib.av1_filter_intra_predictor_hip(_at(dst), stride, tx_size, _at(above, above_index),
                                        _at(left, left_index), mode)


def av1_filter_intra_edge(p, sz, strength, index=0):
    """av1_rtcd_defs.pl:605: in place on p[index .. index + sz)."""
    assert p.dtype == np.uint8
    _lib.av1_filter_intra_edge_hip(_at(p, index), sz, strength)


def av1_upsample_intra_edge(p, sz, index=2):
    """In place: reads p[index - 1 .. index + sz), writes p[index - 2 .. index + 2 sz - 2]
    (both ends included)."""
    assert p.dtype == np.uint8 and index >= 2
    _lib.av1_upsample_intra_edge_hip(_at(p, index), sz)


def av1_filter_intra_edge_high(p, sz, strength, index=0):
    assert p.dtype == np.uint16
    _lib.av1_filter_intra_edge_high_hip(_at(p, index), sz, strength)


def av1_upsample_intra_edge_high(p, sz, bd, index=2):
    assert p.dtype == np.uint16 and index >= 2
    _lib.av1_upsample_intra_edge_high_hip(_at(p, index), sz, bd)
