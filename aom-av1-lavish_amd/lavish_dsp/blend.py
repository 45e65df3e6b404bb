"""Mask building and blending: the a64 blends, the diff-weighted compound
masks, the OBMC weighted source / prediction and the wedge residual
reductions (include/lavish_dsp.h, "mask building and blending").

Two layers, as in pixel.py:

* per-call functions named like the reference's rtcd entries
  (``aom_blend_a64_mask``, ``av1_build_compound_diffwtd_mask_d16``,
  ``av1_wedge_sse_from_residuals`` ...) on numpy arrays with the reference's
  argument meaning -- they call the ``*_hip`` shims;
* batch functions (``blend_a64_batch``, ``diffwtd_mask_batch``,
  ``obmc_wsrc_batch``, ``obmc_blend_batch``, ``wedge_batch``) on torch device
  tensors, asynchronous on the current torch stream.
"""
import ctypes

import numpy as np

from . import _lib, _stream_ptr
from .inter import ConvolveParams
from .pixel import COMP_JOB_DTYPE, _check, _d, comp_jobs_tensor  # noqa: F401

_vp, _i32, _u32, _u8 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint8
_CP = ctypes.POINTER(ConvolveParams)

OBMC_JOB_DTYPE = np.dtype([("src_off", "<i8"), ("above_off", "<i8"), ("left_off", "<i8"),
                           ("wsrc_off", "<i8"), ("mask_off", "<i8"), ("above_mask", "<u4"),
                           ("left_mask", "<u4")], align=True)
assert OBMC_JOB_DTYPE.itemsize == 48
WEDGE_JOB_DTYPE = np.dtype([("a_off", "<i8"), ("b_off", "<i8"), ("m_off", "<i8"),
                            ("out_off", "<i8"), ("limit", "<i8"), ("n", "<i4"),
                            ("reserved", "<i4")], align=True)
assert WEDGE_JOB_DTYPE.itemsize == 48

BLEND_MASK, BLEND_HMASK, BLEND_VMASK = 0, 1, 2
WEDGE_DELTA_SQUARES, WEDGE_SSE, WEDGE_SIGN = 0, 1, 2
DIFFWTD_38, DIFFWTD_38_INV = 0, 1
OBMC_MASK_LENGTHS = (1, 2, 4, 8, 16, 32, 64)  # the table: length n at byte n - 1

for _n, _a in (
        ("lavish_blend_a64_batch", [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp,
                                    _i32, _i32, _i32, _i32, _i32, _i32, _i32, _CP, _vp]),
        ("lavish_diffwtd_mask_batch", [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _i32,
                                       _i32, _i32, _CP, _vp]),
        ("lavish_obmc_wsrc_batch", [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp,
                                    _i32, _vp, _vp, _vp]),
        ("lavish_obmc_blend_batch", [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp,
                                     _i32, _vp, _i32, _vp]),
        ("lavish_wedge_batch", [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp])):
    getattr(_lib, _n).argtypes = _a
    getattr(_lib, _n).restype = _i32

_BLEND = [_vp, _u32, _vp, _u32, _vp, _u32, _vp]
for _n, _a, _r in (
        ("aom_blend_a64_mask", _BLEND + [_u32, _i32, _i32, _i32, _i32], None),
        ("aom_blend_a64_hmask", _BLEND + [_i32, _i32], None),
        ("aom_blend_a64_vmask", _BLEND + [_i32, _i32], None),
        ("aom_highbd_blend_a64_mask", _BLEND + [_u32, _i32, _i32, _i32, _i32, _i32], None),
        ("aom_highbd_blend_a64_hmask", _BLEND + [_i32, _i32, _i32], None),
        ("aom_highbd_blend_a64_vmask", _BLEND + [_i32, _i32, _i32], None),
        ("aom_lowbd_blend_a64_d16_mask", _BLEND + [_u32, _i32, _i32, _i32, _i32, _CP], None),
        ("aom_highbd_blend_a64_d16_mask", _BLEND + [_u32, _i32, _i32, _i32, _i32, _CP, _i32],
         None),
        ("av1_build_compound_diffwtd_mask", [_vp, _u8, _vp, _i32, _vp, _i32, _i32, _i32], None),
        ("av1_build_compound_diffwtd_mask_highbd",
         [_vp, _u8, _vp, _i32, _vp, _i32, _i32, _i32, _i32], None),
        ("av1_build_compound_diffwtd_mask_d16",
         [_vp, _u8, _vp, _i32, _vp, _i32, _i32, _i32, _CP, _i32], None),
        ("av1_wedge_sse_from_residuals", [_vp, _vp, _vp, _i32], ctypes.c_uint64),
        ("av1_wedge_sign_from_residuals", [_vp, _vp, _i32, ctypes.c_int64], ctypes.c_int8),
        ("av1_wedge_compute_delta_squares", [_vp, _vp, _vp, _i32], None)):
    _f = getattr(_lib, _n + "_hip")
    _f.argtypes = _a
    _f.restype = _r
SHIM_NAMES = ["aom_blend_a64_mask", "aom_blend_a64_hmask", "aom_blend_a64_vmask",
              "aom_highbd_blend_a64_mask", "aom_highbd_blend_a64_hmask",
              "aom_highbd_blend_a64_vmask", "aom_lowbd_blend_a64_d16_mask",
              "aom_highbd_blend_a64_d16_mask", "av1_build_compound_diffwtd_mask",
              "av1_build_compound_diffwtd_mask_highbd", "av1_build_compound_diffwtd_mask_d16",
              "av1_wedge_sse_from_residuals", "av1_wedge_sign_from_residuals",
              "av1_wedge_compute_delta_squares"]
BATCH_NAMES = ["lavish_blend_a64_batch", "lavish_diffwtd_mask_batch", "lavish_obmc_wsrc_batch",
               "lavish_obmc_blend_batch", "lavish_wedge_batch"]


def conv_params(round_0, round_1):
    """The two fields the d16 forms read (is_compound's round_1 is 7)."""
    cp = ConvolveParams()
    cp.round_0, cp.round_1, cp.is_compound = round_0, round_1, 1
    return cp


# ------------------------------------------------- per-call RTCD mirror --
def _p(a, highbd=False):
    """Pointer to the first element of a numpy view; highbd pixel pointers are
    tagged (CONVERT_TO_BYTEPTR)."""
    assert a.strides[-1] == a.itemsize
    return _vp(a.ctypes.data >> 1) if highbd else _vp(a.ctypes.data)


def _chk_px(hb, *arrs):
    for a in arrs:
        assert a.dtype == (np.uint16 if hb else np.uint8)


def aom_blend_a64_mask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask,
                       mask_stride, w, h, subw, subh):
    """aom_dsp_rtcd_defs.pl:703.  Arrays are views starting at the block's
    first element; strides in elements.  dst may be src0 or src1."""
    _chk_px(0, dst, src0, src1, mask)
    _lib.aom_blend_a64_mask_hip(_p(dst), dst_stride, _p(src0), src0_stride, _p(src1),
                                src1_stride, _p(mask), mask_stride, w, h, subw, subh)


def aom_blend_a64_hmask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, w, h):
    _chk_px(0, dst, src0, src1, mask)
    _lib.aom_blend_a64_hmask_hip(_p(dst), dst_stride, _p(src0), src0_stride, _p(src1),
                                 src1_stride, _p(mask), w, h)


def aom_blend_a64_vmask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, w, h):
    _chk_px(0, dst, src0, src1, mask)
    _lib.aom_blend_a64_vmask_hip(_p(dst), dst_stride, _p(src0), src0_stride, _p(src1),
                                 src1_stride, _p(mask), w, h)


def aom_highbd_blend_a64_mask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask,
                              mask_stride, w, h, subw, subh, bd):
    _chk_px(1, dst, src0, src1)
    _lib.aom_highbd_blend_a64_mask_hip(_p(dst, 1), dst_stride, _p(src0, 1), src0_stride,
                                       _p(src1, 1), src1_stride, _p(mask), mask_stride, w, h,
                                       subw, subh, bd)


def aom_highbd_blend_a64_hmask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, w, h,
                               bd):
    _chk_px(1, dst, src0, src1)
    _lib.aom_highbd_blend_a64_hmask_hip(_p(dst, 1), dst_stride, _p(src0, 1), src0_stride,
                                        _p(src1, 1), src1_stride, _p(mask), w, h, bd)


def aom_highbd_blend_a64_vmask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, w, h,
                               bd):
    _chk_px(1, dst, src0, src1)
    _lib.aom_highbd_blend_a64_vmask_hip(_p(dst, 1), dst_stride, _p(src0, 1), src0_stride,
                                        _p(src1, 1), src1_stride, _p(mask), w, h, bd)


def aom_lowbd_blend_a64_d16_mask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask,
                                 mask_stride, w, h, subw, subh, conv_params):
    """aom_dsp_rtcd_defs.pl:701: src0 / src1 are CONV_BUF_TYPE (uint16)."""
    _chk_px(0, dst, mask)
    _chk_px(1, src0, src1)
    _lib.aom_lowbd_blend_a64_d16_mask_hip(_p(dst), dst_stride, _p(src0), src0_stride, _p(src1),
                                          src1_stride, _p(mask), mask_stride, w, h, subw, subh,
                                          ctypes.byref(conv_params))


def aom_highbd_blend_a64_d16_mask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask,
                                  mask_stride, w, h, subw, subh, conv_params, bd):
    _chk_px(1, dst, src0, src1)
    _lib.aom_highbd_blend_a64_d16_mask_hip(_p(dst, 1), dst_stride, _p(src0), src0_stride,
                                           _p(src1), src1_stride, _p(mask), mask_stride, w, h,
                                           subw, subh, ctypes.byref(conv_params), bd)


def av1_build_compound_diffwtd_mask(mask, mask_type, src0, src0_stride, src1, src1_stride, h, w):
    """av1_rtcd_defs.pl:257: mask receives the contiguous w x h block."""
    _chk_px(0, mask, src0, src1)
    _lib.av1_build_compound_diffwtd_mask_hip(_p(mask), mask_type, _p(src0), src0_stride,
                                             _p(src1), src1_stride, h, w)


def av1_build_compound_diffwtd_mask_highbd(mask, mask_type, src0, src0_stride, src1, src1_stride,
                                           h, w, bd):
    _chk_px(1, src0, src1)
    _lib.av1_build_compound_diffwtd_mask_highbd_hip(_p(mask), mask_type, _p(src0, 1), src0_stride,
                                                    _p(src1, 1), src1_stride, h, w, bd)


def av1_build_compound_diffwtd_mask_d16(mask, mask_type, src0, src0_stride, src1, src1_stride, h,
                                        w, conv_params, bd):
    _chk_px(1, src0, src1)
    _lib.av1_build_compound_diffwtd_mask_d16_hip(_p(mask), mask_type, _p(src0), src0_stride,
                                                 _p(src1), src1_stride, h, w,
                                                 ctypes.byref(conv_params), bd)


def av1_wedge_sse_from_residuals(r1, d, m, N):
    assert r1.dtype == np.int16 and d.dtype == np.int16 and m.dtype == np.uint8
    return int(_lib.av1_wedge_sse_from_residuals_hip(_p(r1), _p(d), _p(m), N))


def av1_wedge_sign_from_residuals(ds, m, N, limit):
    assert ds.dtype == np.int16 and m.dtype == np.uint8
    return int(_lib.av1_wedge_sign_from_residuals_hip(_p(ds), _p(m), N, limit))


def av1_wedge_compute_delta_squares(d, a, b, N):
    assert d.dtype == np.int16 and a.dtype == np.int16 and b.dtype == np.int16
    _lib.av1_wedge_compute_delta_squares_hip(_p(d), _p(a), _p(b), N)


# ---------------------------------------------------------- batch layer --
def obmc_jobs_tensor(jobs, device):
    """Upload an OBMC_JOB_DTYPE numpy array (LavishObmcJob) as a device byte tensor."""
    import torch
    assert jobs.dtype == OBMC_JOB_DTYPE
    return torch.from_numpy(np.ascontiguousarray(jobs).view(np.uint8).copy()).to(device)


def wedge_jobs_tensor(jobs, device):
    """Upload a WEDGE_JOB_DTYPE numpy array (LavishWedgeJob) as a device byte tensor."""
    import torch
    assert jobs.dtype == WEDGE_JOB_DTYPE
    return torch.from_numpy(np.ascontiguousarray(jobs).view(np.uint8).copy()).to(device)


def _stride(t):
    return t.stride(0) if t.dim() == 2 else 0


def blend_a64_batch(dst, src0, src1, mask, w, h, jobs, kind=BLEND_MASK, subw=0, subh=0,
                    d16=False, bit_depth=8, conv_params=None, dst_stride=None, src0_stride=None,
                    src1_stride=None, mask_stride=None, stream=None):
    """lavish_blend_a64_batch.  dst / src0 / src1 / mask: device tensors, 2-D
    planes (stride = row stride) or 1-D with the strides given; jobs: a
    comp_jobs_tensor (src_off = dst block, ref_off[0] / [1] = src0 / src1,
    mask_off).  Pixels are uint8, or 16-bit (int16 / uint16 tensors) for highbd
    and for the d16 inputs.  In place on dst, which may be src0 or src1."""
    highbd = dst.element_size() == 2
    nj = jobs.numel() // COMP_JOB_DTYPE.itemsize
    _check(_lib.lavish_blend_a64_batch(
        _d(dst), _stride(dst) if dst_stride is None else dst_stride,
        _d(src0), _stride(src0) if src0_stride is None else src0_stride,
        _d(src1), _stride(src1) if src1_stride is None else src1_stride,
        _d(mask), _stride(mask) if mask_stride is None else mask_stride, w, h, _d(jobs), nj, kind,
        subw, subh, int(d16), int(highbd), bit_depth,
        ctypes.byref(conv_params) if conv_params is not None else None, _stream_ptr(stream)),
        "lavish_blend_a64_batch")


def diffwtd_mask_batch(mask, src0, src1, w, h, jobs, d16=False, bit_depth=8, conv_params=None,
                       src0_stride=None, src1_stride=None, stream=None):
    """lavish_diffwtd_mask_batch: mask (1-D uint8 device tensor) receives the
    contiguous w x h blocks at job.mask_off; job.invert_mask is the mask type."""
    highbd = (not d16) and src0.element_size() == 2
    nj = jobs.numel() // COMP_JOB_DTYPE.itemsize
    _check(_lib.lavish_diffwtd_mask_batch(
        _d(mask), _d(src0), _stride(src0) if src0_stride is None else src0_stride, _d(src1),
        _stride(src1) if src1_stride is None else src1_stride, w, h, _d(jobs), nj, int(d16),
        int(highbd), bit_depth, ctypes.byref(conv_params) if conv_params is not None else None,
        _stream_ptr(stream)), "lavish_diffwtd_mask_batch")


def obmc_wsrc_batch(src, above, left, bw, bh, jobs, obmc_masks, wsrc, mask, stream=None):
    """lavish_obmc_wsrc_batch: src / above / left 2-D device planes; wsrc / mask
    1-D int32 device tensors receiving contiguous bw x bh blocks; obmc_masks the
    127-byte uint8 device table; jobs from obmc_jobs_tensor."""
    nj = jobs.numel() // OBMC_JOB_DTYPE.itemsize
    _check(_lib.lavish_obmc_wsrc_batch(
        _d(src), src.stride(0), _d(above), above.stride(0), _d(left), left.stride(0), bw, bh,
        _d(jobs), nj, _d(obmc_masks), int(src.element_size() == 2), _d(wsrc), _d(mask),
        _stream_ptr(stream)), "lavish_obmc_wsrc_batch")


def obmc_blend_batch(dst, above, left, bw, bh, jobs, obmc_masks, subsampling_x=0,
                     subsampling_y=0, stream=None):
    """lavish_obmc_blend_batch, in place on the 2-D plane dst; (bw, bh) is the
    luma block size, offsets and strides are the plane's."""
    nj = jobs.numel() // OBMC_JOB_DTYPE.itemsize
    _check(_lib.lavish_obmc_blend_batch(
        _d(dst), dst.stride(0), _d(above), above.stride(0), _d(left), left.stride(0), bw, bh,
        subsampling_x, subsampling_y, _d(jobs), nj, _d(obmc_masks),
        int(dst.element_size() == 2), _stream_ptr(stream)), "lavish_obmc_blend_batch")


def wedge_batch(a, b, m, jobs, kind, out=None, stream=None):
    """lavish_wedge_batch on 1-D device tensors (a, b int16; m uint8).  kind 0
    writes int16 into `out` (required) at job.out_off; kind 1 returns the sse
    as int64 [njobs] (values below 2^63), kind 2 the signs as int8 [njobs]."""
    import torch
    nj = jobs.numel() // WEDGE_JOB_DTYPE.itemsize
    if out is None:
        assert kind != WEDGE_DELTA_SQUARES
        out = torch.empty(nj, dtype=torch.int64 if kind == WEDGE_SSE else torch.int8,
                          device=a.device)
    _check(_lib.lavish_wedge_batch(_d(a), _d(b), _d(m), _d(jobs), nj, kind, _d(out),
                                   _stream_ptr(stream)), "lavish_wedge_batch")
    return out
