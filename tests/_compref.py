"""numpy restatement of the masked / OBMC / distance-weighted pixel kinds
(aom_dsp/sad_av1.c, aom_dsp/sad.c:57-64, aom_dsp/variance.c:165-181, 285-318,
707-976, 1040-1170) and the reader of tests/golden/fix_pixel_comp.npz.

Blocks are 2-D integer arrays; a "filtered" operand is the (h + 1) x (w + 1)
window the bilinear filter reads.  Every function also takes a stack of blocks
([n, h, w], per-block parameters as [n] arrays) and then returns [n] results.
test_pixel_comp_cpu.py pins every function here to the fixture (the
reference's own outputs); the GPU batch tests then use them on their own
planes.

The fixture generator (tests/golden/gen_fix_pixel_comp.py) builds its inputs
through case_inputs() too, so generator and tests read a case the same way.
"""
import numpy as np

M32 = 0xFFFFFFFF

# kinds of the fixture's case table
MSAD, MSAD_X4D, MSVAR, OSAD, OVAR, OSVAR, JSAD, JSVAR, PRED_AVG, PRED_DIST, PRED_MASK = range(11)
KIND_NAMES = ["masked_sad", "masked_sad_x4d", "masked_sub_pixel_variance", "obmc_sad",
              "obmc_variance", "obmc_sub_pixel_variance", "dist_wtd_sad_avg",
              "dist_wtd_sub_pixel_avg_variance", "comp_avg_pred", "dist_wtd_comp_avg_pred",
              "comp_mask_pred"]
# columns of the case table
COLS = ["kind", "w", "h", "bd", "highbd", "a_off", "b_off", "s_off", "m_off", "xoff", "yoff",
        "invert", "fwd", "bck", "variant", "ret", "sse"]
# variant: 0 the stored planes; 1 / 2 blend mask all 0 / all 64; 3 / 4 OBMC
# mask all 0 / all 4096; 5 every pixel of A, second_pred at the maximum, B
# and wsrc all zero, OBMC mask all 4096


def x4d_offsets(b_stride):
    """The 4 references of an x4d case, as element offsets from b_off."""
    return (0, 1, b_stride, b_stride + 3)


def _i(a):
    return np.asarray(a).astype(np.int64)


def blend_a64(m, a, b):
    return (m * a + (64 - m) * b + 32) >> 6


def dist_wtd(second, ref, fwd, bck):
    return (second * bck + ref * fwd + 8) >> 4


def _b(v):
    """A per-block parameter (scalar or [n]) shaped to broadcast over h x w."""
    return _i(v)[..., None, None]


def bilinear(win, xoff, yoff):
    """(h+1) x (w+1) window -> h x w, the two rounded passes."""
    win = _i(win)
    h, w = win.shape[-2] - 1, win.shape[-1] - 1
    f1, g1 = 16 * _b(xoff), 16 * _b(yoff)
    f0, g0 = 128 - f1, 128 - g1
    hp = (win[..., :, :w] * f0 + win[..., :, 1:w + 1] * f1 + 64) >> 7
    return (hp[..., :h, :] * g0 + hp[..., 1:h + 1, :] * g1 + 64) >> 7


def mask_pred(ref, pred, mask, invert):
    """aom_comp_mask_pred: `ref` is the strided operand, `pred` the compact one."""
    ref, pred, mask = _i(ref), _i(pred), _i(mask)
    return np.where(_b(invert) != 0, blend_a64(mask, pred, ref), blend_a64(mask, ref, pred))


def avg_pred(ref, pred):
    return (_i(pred) + _i(ref) + 1) >> 1


def dist_wtd_pred(ref, pred, fwd, bck):
    return dist_wtd(_i(pred), _i(ref), fwd, bck)


def _sum(a):
    return a.sum(axis=(-2, -1))


def variance_tail(sum64, sse64, bd, n):
    """(var, sse) from exact sums: lowbd and highbd-8 wrap as uint32, 10 / 12
    round the sums ((x + half) >> n, an arithmetic shift) and clamp at 0."""
    sum64, sse64 = _i(sum64), _i(sse64)
    s32 = lambda v: ((v + (1 << 31)) & M32) - (1 << 31)
    if bd == 8:
        sse, sm = sse64 & M32, s32(sum64)
        return (sse - ((sm * sm) // n)) & M32, sse
    sh, ss = (2, 4) if bd == 10 else (4, 8)
    sse = ((sse64 + (1 << (ss - 1))) >> ss) & M32
    sm = s32((sum64 + (1 << (sh - 1))) >> sh)  # numpy's >> of int64 is arithmetic, like C's
    return np.maximum(0, sse - (sm * sm) // n), sse


def variance(a, b, bd):
    d = _i(a) - _i(b)
    return variance_tail(_sum(d), _sum(d * d), bd, d.shape[-2] * d.shape[-1])


def masked_sad(src, ref, second, mask, invert):
    return _sum(np.abs(mask_pred(ref, second, mask, invert) - _i(src))) & M32


def dist_wtd_sad_avg(src, ref, second, fwd, bck):
    return _sum(np.abs(dist_wtd_pred(ref, second, fwd, bck) - _i(src))) & M32


def masked_sub_pixel_variance(win, xoff, yoff, ref, second, mask, invert, bd):
    return variance(mask_pred(bilinear(win, xoff, yoff), second, mask, invert), ref, bd)


def dist_wtd_sub_pixel_avg_variance(win, xoff, yoff, ref, second, fwd, bck, bd):
    return variance(dist_wtd_pred(bilinear(win, xoff, yoff), second, fwd, bck), ref, bd)


def obmc_sad(pre, wsrc, mask):
    return _sum((np.abs(_i(wsrc) - _i(pre) * _i(mask)) + 2048) >> 12) & M32


def obmc_variance(pre, wsrc, mask, bd):
    v = _i(wsrc) - _i(pre) * _i(mask)
    r = (np.abs(v) + 2048) >> 12
    d = np.where(v < 0, -r, r)  # ROUND_POWER_OF_TWO_SIGNED
    return variance_tail(_sum(d), _sum(d * d), bd, d.shape[-2] * d.shape[-1])


def obmc_sub_pixel_variance(win, xoff, yoff, wsrc, mask, bd):
    return obmc_variance(bilinear(win, xoff, yoff), wsrc, mask, bd)


# ---------------------------------------------------------------- fixture --
class Case:
    pass


def case_inputs(F, row):
    """The arrays of one case: flat planes positioned at the case's first
    element (+ strides), the compact second_pred / wsrc / OBMC mask blocks."""
    c = Case()
    for k, v in zip(COLS, row):
        setattr(c, k, int(v))
    w, h, bd = c.w, c.h, c.bd
    c.dtype = np.uint16 if c.highbd else np.uint8
    mx = (1 << bd) - 1
    a, b = F["a_bd%d" % bd], F["b_bd%d" % bd]
    second = F["second_bd%d" % bd][c.s_off:c.s_off + w * h]
    mask = F["mask"]
    wsrc = F["wsrc_bd%d" % bd][c.s_off:c.s_off + w * h]
    mo = c.m_off if c.kind in (OSAD, OVAR, OSVAR) else 0  # m_off indexes the u8 mask otherwise
    omask = F["omask"][mo:mo + w * h]
    if c.variant in (1, 2):
        mask = np.full_like(mask, 0 if c.variant == 1 else 64)
    if c.variant in (3, 4):
        omask = np.full_like(omask, 0 if c.variant == 3 else 4096)
    if c.variant == 5:
        a, b = np.full_like(a, mx), np.zeros_like(b)
        second, wsrc = np.full_like(second, mx), np.zeros_like(wsrc)
        omask = np.full_like(omask, 4096)
    c.a_stride, c.b_stride, c.mask_stride = a.shape[1], b.shape[1], mask.shape[1]
    c.a = np.ascontiguousarray(a.astype(c.dtype)).reshape(-1)[c.a_off:]
    c.b = np.ascontiguousarray(b.astype(c.dtype)).reshape(-1)[c.b_off:]
    c.mask = np.ascontiguousarray(mask.astype(np.uint8)).reshape(-1)[c.m_off:]
    c.second = np.ascontiguousarray(second.astype(c.dtype))
    c.wsrc = np.ascontiguousarray(wsrc.astype(np.int32))
    c.omask = np.ascontiguousarray(omask.astype(np.int32))
    return c


def window(flat, stride, w, h):
    """h x w block at the start of a flat strided plane."""
    idx = np.arange(h)[:, None] * stride + np.arange(w)[None, :]
    return flat[idx]


def expected(c):
    """The restatement's result for a case: (ret, sse), the 4 x4d SADs, or the
    predicted block."""
    w, h = c.w, c.h
    win = lambda: window(c.a, c.a_stride, w + 1, h + 1)
    A = lambda: window(c.a, c.a_stride, w, h)
    B = lambda off=0: window(c.b[off:], c.b_stride, w, h)
    S = c.second.reshape(h, w)
    M = lambda: window(c.mask, c.mask_stride, w, h)
    W, OM = c.wsrc.reshape(h, w), c.omask.reshape(h, w)
    k = c.kind
    if k == MSAD:
        return masked_sad(A(), B(), S, M(), c.invert), 0
    if k == MSAD_X4D:
        return [masked_sad(A(), B(o), S, M(), c.invert) for o in x4d_offsets(c.b_stride)]
    if k == MSVAR:
        return masked_sub_pixel_variance(win(), c.xoff, c.yoff, B(), S, M(), c.invert, c.bd)
    if k == OSAD:
        return obmc_sad(A(), W, OM), 0
    if k == OVAR:
        return obmc_variance(A(), W, OM, c.bd)
    if k == OSVAR:
        return obmc_sub_pixel_variance(win(), c.xoff, c.yoff, W, OM, c.bd)
    if k == JSAD:
        return dist_wtd_sad_avg(A(), B(), S, c.fwd, c.bck), 0
    if k == JSVAR:
        return dist_wtd_sub_pixel_avg_variance(win(), c.xoff, c.yoff, B(), S, c.fwd, c.bck, c.bd)
    if k == PRED_AVG:
        return avg_pred(B(), S)
    if k == PRED_DIST:
        return dist_wtd_pred(B(), S, c.fwd, c.bck)
    if k == PRED_MASK:
        return mask_pred(B(), S, M(), c.invert)
    raise ValueError(k)


def rtcd_name(c):
    """The reference's function name of a case (no _c / _hip suffix)."""
    s = "%dx%d" % (c.w, c.h)
    hb = "aom_highbd_" if c.highbd else "aom_"
    vb = "aom_highbd_%d_" % c.bd if c.highbd else "aom_"
    ob = ("aom_highbd_" if c.bd == 8 else "aom_highbd_%d_" % c.bd) if c.highbd else "aom_"
    return {MSAD: hb + "masked_sad" + s, MSAD_X4D: "aom_masked_sad%sx4d" % s,
            MSVAR: vb + "masked_sub_pixel_variance" + s, OSAD: hb + "obmc_sad" + s,
            OVAR: ob + "obmc_variance" + s, OSVAR: ob + "obmc_sub_pixel_variance" + s,
            JSAD: hb + "dist_wtd_sad%s_avg" % s,
            JSVAR: vb + "dist_wtd_sub_pixel_avg_variance" + s, PRED_AVG: hb + "comp_avg_pred",
            PRED_DIST: hb + "dist_wtd_comp_avg_pred", PRED_MASK: hb + "comp_mask_pred"}[c.kind]
