"""Chroma from luma (include/lavish_dsp.h, "chroma from luma").

* ``cfl_ac_jobs`` / ``cfl_predict_jobs`` / ``cfl_search_jobs`` build and
  validate the int64 job tables on the host (ValueError for what the kernels
  must not be given), ``cfl_jobs_tensor`` uploads one;
* ``cfl_ac_batch``, ``cfl_predict_batch`` and ``cfl_alpha_search_batch`` run
  them on torch device planes, asynchronous on the current torch stream;
* ``cfl_joint`` turns the two estimates into (cfl_alpha_idx, cfl_alpha_signs);
* ``cfl_subsample``, ``cfl_subtract_average`` and ``cfl_predict`` are the
  size-generic per-call forms on numpy arrays (host buffers at CFL_BUF_LINE
  stride, as the reference's).

Pixels are uint8 (bit_depth 8) or 16-bit (int16 / uint16 tensors; bit_depth
8 / 10 / 12); which one is read off the tensor's element size.  The RTCD
getters of include/lavish_dsp_cfl.h are C entry points and are not bound here.
"""
import ctypes

import numpy as np

from . import TX_H, TX_W, _lib, _stream_ptr
from .pixel import _check, _d

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

CFL_BUF_LINE = 32
CFL_BUF_SQUARE = CFL_BUF_LINE * CFL_BUF_LINE
CFL_MAGS_SIZE = 33
CFL_INDEX_ZERO = 16
CFL_TX_SIZES = tuple(t for t in range(19) if TX_W[t] <= 32 and TX_H[t] <= 32)
# job table columns (the enums of the header)
AC_COLS = ("luma_off", "luma_w", "luma_h", "tx_size")
PRED_COLS = ("cell", "dst_off", "tx_size", "alpha_q3")
SEARCH_COLS = ("cell", "src_off", "dc_off", "tx_size")

_lib.lavish_cfl_ac_batch.argtypes = [_vp, _i32, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp]
_lib.lavish_cfl_ac_batch.restype = _i32
_lib.lavish_cfl_predict_batch.argtypes = [_vp, _i64, _vp, _i32, _i64, _vp, _i32, _i32, _i32, _vp]
_lib.lavish_cfl_predict_batch.restype = _i32
_lib.lavish_cfl_alpha_search_batch.argtypes = [_vp, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _vp,
                                               _i32, _vp, _vp, _i32, _i32, _vp]
_lib.lavish_cfl_alpha_search_batch.restype = _i32
_lib.lavish_cfl_joint.argtypes = [_i32, _i32, _vp, _vp]
_lib.lavish_cfl_joint.restype = _i32
_lib.lavish_cfl_subsample_host.argtypes = [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32]
_lib.lavish_cfl_subsample_host.restype = None
_lib.lavish_cfl_subtract_average_host.argtypes = [_vp, _vp, _i32, _i32]
_lib.lavish_cfl_subtract_average_host.restype = None
_lib.lavish_cfl_predict_host.argtypes = [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32]
_lib.lavish_cfl_predict_host.restype = None
BATCH_NAMES = ["lavish_cfl_ac_batch", "lavish_cfl_predict_batch", "lavish_cfl_alpha_search_batch"]


# ------------------------------------------------------------ job tables --
def _cols(*vals):
    cols = [np.atleast_1d(np.asarray(v, np.int64)) for v in vals]
    n = max(len(c) for c in cols)
    return [np.broadcast_to(c, (n,)) for c in cols]


def _check_tx(tx):
    if ((tx < 0) | (tx > 18)).any():
        raise ValueError("tx_size outside 0 .. 18")
    w, h = np.array(TX_W)[tx], np.array(TX_H)[tx]
    if ((w > 32) | (h > 32)).any():
        raise ValueError("CfL has no 64-point transform size")
    return w, h


def _check_rect(what, off, w, h, stride, elems):
    if (off < 0).any():
        raise ValueError("negative %s offset" % what)
    if stride is None or elems is None:
        return
    if (w > stride).any() or (off + (h - 1) * stride + w > elems).any():
        raise ValueError("%s block outside its plane" % what)


def check_subsampling(sub_x, sub_y):
    if sub_x not in (0, 1) or sub_y not in (0, 1):
        raise ValueError("subsampling outside 0 .. 1")
    if (sub_x, sub_y) == (0, 1):
        raise ValueError("(sub_x, sub_y) = (0, 1) is not a CfL layout")


def cfl_ac_jobs(luma_off, luma_w, luma_h, tx_size, sub_x, sub_y, luma_stride=None,
                luma_elems=None):
    """The [n, 4] int64 table of lavish_cfl_ac_batch (AC_COLS) from scalars or
    equal-length sequences: the stored luma rectangle and the chroma tx_size.
    With luma_stride / luma_elems the rectangles are checked against the plane."""
    check_subsampling(sub_x, sub_y)
    off, lw, lh, tx = _cols(luma_off, luma_w, luma_h, tx_size)
    w, h = _check_tx(tx)
    if ((lw % 4 != 0) | (lh % 4 != 0) | (lw < 4) | (lh < 4)).any():
        raise ValueError("luma extent is not a positive multiple of 4")
    if ((lw > CFL_BUF_LINE) | (lh > CFL_BUF_LINE)).any():
        raise ValueError("luma extent above 32")
    if (((lw >> sub_x) > w) | ((lh >> sub_y) > h)).any():
        raise ValueError("stored luma extent larger than the transform")
    _check_rect("luma", off, lw, lh, luma_stride, luma_elems)
    return np.ascontiguousarray(np.stack([off, lw, lh, tx], axis=1))


def cfl_predict_jobs(cell, dst_off, tx_size, alpha_q3, ncells=None, dst_stride=None,
                     dst_elems=None):
    """The [n, 4] int64 table of lavish_cfl_predict_batch (PRED_COLS)."""
    ce, off, tx, al = _cols(cell, dst_off, tx_size, alpha_q3)
    w, h = _check_tx(tx)
    if ((al < -16) | (al > 16)).any():
        raise ValueError("alpha_q3 outside -16 .. 16")
    if (ce < 0).any() or (ncells is not None and (ce >= ncells).any()):
        raise ValueError("AC cell index outside the cells")
    _check_rect("dst", off, w, h, dst_stride, dst_elems)
    return np.ascontiguousarray(np.stack([ce, off, tx, al], axis=1))


def cfl_search_jobs(cell, src_off, dc_off, tx_size, ncells=None, src_stride=None, src_elems=None,
                    dc_stride=None, dc_elems=None):
    """The [n, 4] int64 table of lavish_cfl_alpha_search_batch (SEARCH_COLS)."""
    ce, so, do, tx = _cols(cell, src_off, dc_off, tx_size)
    w, h = _check_tx(tx)
    if (ce < 0).any() or (ncells is not None and (ce >= ncells).any()):
        raise ValueError("AC cell index outside the cells")
    _check_rect("src", so, w, h, src_stride, src_elems)
    _check_rect("dc", do, w, h, dc_stride, dc_elems)
    return np.ascontiguousarray(np.stack([ce, so, do, tx], axis=1))


def cfl_jobs_tensor(jobs, device):
    """Upload a job table (int64 [n, 4]) as a device tensor."""
    import torch
    assert jobs.dtype == np.int64 and jobs.ndim == 2 and jobs.shape[1] == 4
    return torch.from_numpy(np.ascontiguousarray(jobs).copy()).to(device)


# ---------------------------------------------------------- batch layer --
def _plane(t, bit_depth, stride):
    highbd = t.element_size() == 2
    if t.element_size() not in (1, 2) or bit_depth not in ((8, 10, 12) if highbd else (8,)):
        raise ValueError("pixels are uint8 at bit_depth 8 or 16-bit at 8 / 10 / 12")
    return highbd, (t.stride(0) if stride is None else stride), t.numel()


def cfl_ac_batch(luma, jobs, sub_x, sub_y, bit_depth=8, luma_stride=None, out=None, stream=None):
    """lavish_cfl_ac_batch.  luma: a device plane (2-D, or 1-D with luma_stride);
    jobs: a cfl_jobs_tensor of cfl_ac_jobs.  Returns the AC cells, an int16
    [njobs, 32, 32] device tensor (job j's W x H corner of cell j is written)."""
    import torch
    highbd, stride, elems = _plane(luma, bit_depth, luma_stride)
    nj = jobs.shape[0]
    if out is None:
        out = torch.zeros((nj, CFL_BUF_LINE, CFL_BUF_LINE), dtype=torch.int16, device=luma.device)
    assert out.dtype == torch.int16 and out.is_contiguous() and out.numel() >= nj * CFL_BUF_SQUARE
    _check(_lib.lavish_cfl_ac_batch(_d(luma), stride, elems, sub_x, sub_y, _vp(jobs.data_ptr()), nj,
                                    _vp(out.data_ptr()), bit_depth, int(highbd),
                                    _stream_ptr(stream)), "lavish_cfl_ac_batch")
    return out


def cfl_predict_batch(ac_cells, dst, jobs, bit_depth=8, dst_stride=None, stream=None):
    """lavish_cfl_predict_batch, in place on dst (which holds the DC prediction)."""
    highbd, stride, elems = _plane(dst, bit_depth, dst_stride)
    assert ac_cells.is_contiguous() and ac_cells.element_size() == 2
    _check(_lib.lavish_cfl_predict_batch(_vp(ac_cells.data_ptr()), ac_cells.numel() // CFL_BUF_SQUARE,
                                         _d(dst), stride, elems, _vp(jobs.data_ptr()),
                                         jobs.shape[0], bit_depth, int(highbd),
                                         _stream_ptr(stream)), "lavish_cfl_predict_batch")


def cfl_alpha_search_batch(ac_cells, src, dc, jobs, bit_depth=8, src_stride=None, dc_stride=None,
                           stream=None):
    """lavish_cfl_alpha_search_batch.  Returns (costs int32 [njobs, 33],
    est_idx uint8 [njobs]) device tensors."""
    import torch
    highbd, ss, se = _plane(src, bit_depth, src_stride)
    hb2, ds, de = _plane(dc, bit_depth, dc_stride)
    if highbd != hb2:
        raise ValueError("src and dc differ in pixel type")
    assert ac_cells.is_contiguous() and ac_cells.element_size() == 2
    nj = jobs.shape[0]
    costs = torch.zeros((nj, CFL_MAGS_SIZE), dtype=torch.int32, device=src.device)
    est = torch.zeros((nj,), dtype=torch.uint8, device=src.device)
    _check(_lib.lavish_cfl_alpha_search_batch(
        _vp(ac_cells.data_ptr()), ac_cells.numel() // CFL_BUF_SQUARE, _d(src), ss, se, _d(dc), ds,
        de, _vp(jobs.data_ptr()), nj, _vp(costs.data_ptr()), _vp(est.data_ptr()), bit_depth,
        int(highbd), _stream_ptr(stream)), "lavish_cfl_alpha_search_batch")
    return costs, est


def cfl_joint(est_u, est_v):
    """lavish_cfl_joint: (valid, cfl_alpha_idx, cfl_alpha_signs); valid 0 when
    both estimates are CFL_INDEX_ZERO."""
    a, s = ctypes.c_uint8(0), ctypes.c_int8(0)
    rc = _lib.lavish_cfl_joint(int(est_u), int(est_v), ctypes.addressof(a), ctypes.addressof(s))
    if rc < 0:
        raise ValueError("estimate outside 0 .. 32")
    return rc, a.value, s.value


# ------------------------------------------------------ host-buffer layer --
def _at(a, i=0):
    assert a.strides[-1] == a.itemsize
    return _vp(a.ctypes.data + i * a.itemsize)


def cfl_subsample(input, input_stride, output_q3, width, height, sub_x, sub_y, input_index=0,
                  output_index=0):
    """cfl_luma_subsampling_{420,422,444}_{lbd,hbd}_c: width x height luma pixels
    of `input` (uint8 or uint16, 1-D) into output_q3 (uint16, CFL_BUF_LINE stride)."""
    check_subsampling(sub_x, sub_y)
    assert input.dtype in (np.uint8, np.uint16) and output_q3.dtype == np.uint16
    _lib.lavish_cfl_subsample_host(_at(input, input_index), input_stride,
                                   _at(output_q3, output_index), width, height, sub_x, sub_y,
                                   int(input.dtype == np.uint16))


def cfl_subtract_average(src, dst, width, height, src_index=0, dst_index=0):
    """subtract_average_c at the size's round_offset / num_pel_log2: src uint16,
    dst int16, both at CFL_BUF_LINE stride."""
    assert src.dtype == np.uint16 and dst.dtype == np.int16
    _lib.lavish_cfl_subtract_average_host(_at(src, src_index), _at(dst, dst_index), width, height)


def cfl_predict(ac_buf_q3, dst, dst_stride, alpha_q3, width, height, bit_depth=8, ac_index=0,
                dst_index=0):
    """cfl_predict_lbd_c / cfl_predict_hbd_c in place on dst (uint8 or uint16)."""
    assert ac_buf_q3.dtype == np.int16 and dst.dtype in (np.uint8, np.uint16)
    _lib.lavish_cfl_predict_host(_at(ac_buf_q3, ac_index), _at(dst, dst_index), dst_stride, alpha_q3,
                                 bit_depth, width, height, int(dst.dtype == np.uint16))
