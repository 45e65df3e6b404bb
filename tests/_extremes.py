"""Worst-case pixel patterns for the interpolation filters (numpy only).

For a kernel row k[0..T-1] and mx = 2^bd - 1
    HI(k)[m] = mx where k[m] > 0 else 0      (the largest tap sum)
    LO(k)[m] = mx where k[m] < 0 else 0      (the smallest)
The aligned window of a (kx, ky) pair, polarity max, has HI(kx) in the rows
under a positive ky tap and LO(kx) elsewhere; polarity min is the reverse.
Tiled with period Tx x Ty it makes a plane in which one output pixel of every
cell -- the anchor and its translates -- sees the aligned window and the
others see its rotations.  A direction without a filter (the x-only, y-only
and copy paths) is the one-tap kernel [1].

anchor_values() restates the arithmetic of the anchor pixel in plain Python
integers, once with no narrowing and once with the horizontal intermediate
truncated to int16 as the C reference's im_block does.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_T = json.load(open(os.path.join(HERE, "golden", "ref_tables.json")))
_F = _T["interp_filters"]
WARPED_FILTER = np.array(_T["warped_filter"], np.int64)         # [193, 8]

# (name, InterpFilter, block size that selects the table, table)
KINDS = [("REGULAR", 0, 8, "av1_sub_pel_filters_8"),
         ("SMOOTH", 1, 8, "av1_sub_pel_filters_8smooth"),
         ("SHARP", 2, 8, "av1_sub_pel_filters_8sharp"),
         ("BILINEAR", 3, 8, "av1_bilinear_filters"),
         ("REGULAR4", 0, 4, "av1_sub_pel_filters_4"),
         ("SMOOTH4", 1, 4, "av1_sub_pel_filters_4smooth"),
         ("SHARP2", 4, 8, "av1_sub_pel_filters_12sharp")]
KIND_NAMES = [k[0] for k in KINDS]
REGULAR, SMOOTH, SHARP, BILINEAR, REGULAR4, SMOOTH4, SHARP2 = range(7)
ONE = np.array([1], np.int64)

# rpot(2^(bd+6) + sum k.p, round_0) at the extremes, per bit depth: (lo, hi)
BOUNDS = {"SHARP": {8: (263, 7913), 10: (1031, 31721), 12: (1026, 31738)},
          "REGULAR": {8: (1156, 7021), 10: (4612, 28141), 12: (4609, 28155)},
          "WARP": {8: (550, 7626), 10: (2182, 30570), 12: (2177, 30587)},
          "SHARP2": {8: (-119, 8296), 10: (-503, 33256), 12: (-510, 33274)}}


def kernel(kind, phase):
    """Kernel row of KINDS[kind] at a 1/16 phase (int64 [8] or [12])."""
    return np.array(_F[KINDS[kind][3]][phase], np.int64)


def kind_filter(kind):
    """(InterpFilter, block size) that make the reference choose this table."""
    return KINDS[kind][1], KINDS[kind][2]


def pos_neg(k):
    k = np.asarray(k, np.int64)
    return int(k[k > 0].sum()), int(k[k < 0].sum())


def extreme_phase(kind):
    """The phase 1..15 with the largest positive tap sum (it also has the most
    negative one, the row summing to 128); the lowest such phase."""
    return max(range(1, 16), key=lambda p: (pos_neg(kernel(kind, p))[0], -p))


def extreme_warp_row():
    return max(range(193), key=lambda r: (pos_neg(WARPED_FILTER[r])[0], -r))


def rpot(v, n):
    return (v + ((1 << n) >> 1)) >> n


def conv_rounds(bd, compound):
    """(round_0, round_1) of get_conv_params_no_round."""
    r0 = 3 + max(bd + 7 - 3 + 2 - 16, 0)
    return r0, (7 if compound else 14 - r0)


def hi(k, mx):
    return np.where(np.asarray(k) > 0, mx, 0).astype(np.int64)


def lo(k, mx):
    return np.where(np.asarray(k) < 0, mx, 0).astype(np.int64)


def window(kx, ky, bd, polarity):
    """The aligned Ty x Tx window; polarity 1: max, 0: min."""
    mx = (1 << bd) - 1
    kx = ONE if kx is None else np.asarray(kx, np.int64)
    ky = ONE if ky is None else np.asarray(ky, np.int64)
    a, b = (hi(kx, mx), lo(kx, mx)) if polarity else (lo(kx, mx), hi(kx, mx))
    return np.stack([a if t > 0 else b for t in ky])


def _fo(t):
    return t // 2 - 1 if t > 1 else 0


def periodic(win, shape, anchor):
    """A plane of `shape` in which the output pixel at `anchor` (row, col of the
    plane) sees `win`: win[m, n] lies at (ay - fo_y + m, ax - fo_x + n), tiled."""
    ty, tx = win.shape
    ys = (np.arange(shape[0]) - anchor[0] + _fo(ty)) % ty
    xs = (np.arange(shape[1]) - anchor[1] + _fo(tx)) % tx
    return win[np.ix_(ys, xs)]


def source(win, w, h, anchor):
    """The source window of a w x h block whose output pixel `anchor` (row, col
    inside the block) is aligned: ((h + Ty - 1) x (w + Tx - 1) plane, (row, col)
    of the block's integer position in it)."""
    ty, tx = win.shape
    oy, ox = _fo(ty), _fo(tx)
    return periodic(win, (h + ty - 1, w + tx - 1), (anchor[0] + oy, anchor[1] + ox)), (oy, ox)


def anchors(w, h, n):
    """n anchors rotating over a w x h block: the four edges, every column
    residue mod 4 and every row (so every residue mod 16 a block has)."""
    base = [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0)]
    out = []
    for i in range(n):
        out.append(base[i] if i < 4 else ((i * 5 + 1) % h, (i * 3 + 2) % w))
    return out


def _i16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def anchor_values(win, kx, ky, bd, round_0, round_1, compound, narrow=None):
    """The anchor pixel of the aligned window `win`, in plain integers.
    Returns dict(ims, im, final, final_i16, wraps):
      ims        the horizontal intermediates of the window's rows (2-D only)
      im         the extreme one (the largest if any exceeds int16, else the
                 one farthest from mid-range)
      final      the output (pixel, or CONV_BUF value when compound) without
                 any narrowing
      final_i16  the same with every intermediate truncated to int16, and the
                 single-prediction sum narrowed as the function at hand does:
                 narrow "u16" (the scaled functions' CONV_BUF_TYPE res), "i16"
                 (av1_convolve_2d_sr_c's int16_t res) or None
      wraps      an intermediate leaves the int16 range, or the sum leaves
                 the range `narrow` names
    kx / ky None select the y-only / x-only / copy formulas."""
    mx = (1 << bd) - 1
    clip = lambda v: max(0, min(mx, v))
    ob = bd + 14 - round_0
    roff = (1 << (ob - round_1)) + (1 << (ob - round_1 - 1))
    win = [[int(v) for v in row] for row in win]
    if kx is not None and ky is not None:
        kx, ky = [int(v) for v in kx], [int(v) for v in ky]
        ims = [rpot((1 << (bd + 6)) + sum(a * b for a, b in zip(kx, row)), round_0)
               for row in win]

        def fin(im, faithful=False):
            res = rpot((1 << ob) + sum(a * b for a, b in zip(ky, im)), round_1)
            if compound:
                return res
            if narrow == "u16":
                bites.append(res != res & 0xFFFF)
                res = res & 0xFFFF if faithful else res
            res -= roff
            if narrow == "i16":
                bites.append(res != _i16(res))
                res = _i16(res) if faithful else res
            return clip(rpot(res, 14 - round_0 - round_1))
        bites = []
        mid = 1 << (bd + 6 - round_0)
        final, final_i16 = fin(ims), fin([_i16(v) for v in ims], True)
        return dict(ims=ims, im=max(ims, key=lambda v: abs(v - mid)), final=final,
                    final_i16=final_i16, wraps=any(v != _i16(v) for v in ims) or any(bites))
    if kx is not None:      # x only: one row
        s = sum(a * int(b) for a, b in zip(kx, win[0]))
        if compound:
            f = (1 << (7 - round_1)) * rpot(s, round_0) + roff
        else:
            f = clip(rpot(rpot(s, round_0), 7 - round_0))
    elif ky is not None:    # y only: one column
        s = sum(int(a) * row[0] for a, row in zip(ky, win))
        if compound:
            f = rpot(s * (1 << (7 - round_0)), round_1) + roff
        else:
            f = clip(rpot(s, 7))
    else:                   # copy
        f = (win[0][0] << (14 - round_0 - round_1)) + roff if compound else win[0][0]
    return dict(ims=[], im=None, final=f, final_i16=f, wraps=False)


def saturation_planes(shape, bd):
    """all-max, all-0, 1-pixel checkerboard, vertical and horizontal 0/max stripes."""
    mx = (1 << bd) - 1
    y, x = np.indices(shape)
    return {"max": np.full(shape, mx, np.int64), "zero": np.zeros(shape, np.int64),
            "checker": ((y + x) & 1) * mx, "vstripes": (x & 1) * mx, "hstripes": (y & 1) * mx}
