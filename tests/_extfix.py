"""Accessors of tests/golden/fix_interp_extremes.npz (layout: the docstring of
tests/golden/gen_fix_interp_extremes.py) and the coverage it promises."""
import os
from types import SimpleNamespace

import numpy as np

import _extremes as X

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SINGLE, COMPOUND, SCALE = 0, 1, 2
UNIT_NAMES = ["single", "compound", "scale"]
CONV_FIELDS = ["unit", "highbd", "bd", "w", "h", "path", "kind_x", "kind_y", "phase_x", "phase_y",
               "subpel_x_qn", "x_step_qn", "subpel_y_qn", "y_step_qn", "polarity", "aligned",
               "ay", "ax", "mode", "round_0", "round_1", "fwd_offset", "bck_offset", "src_off",
               "src_h", "src_w", "org_y", "org_x", "out_off", "conv_in"]
WARP_FIELDS = ["bd", "mode", "polarity", "aligned", "row_x", "row_y", "ay", "ax", "m0", "m1", "m2",
               "m3", "m4", "m5", "alpha", "beta", "gamma", "delta", "width", "height", "stride",
               "p_col", "p_row", "p_width", "p_height", "round_0", "round_1", "fwd_offset",
               "bck_offset", "ref_off", "out_off", "conv_in"]

_F = None


def load():
    global _F
    if _F is None:
        _F = dict(np.load(os.path.join(GOLD, "fix_interp_extremes.npz")))
        assert list(_F["conv_fields"]) == CONV_FIELDS and list(_F["warp_fields"]) == WARP_FIELDS
    return _F


def narrow_of(unit, highbd):
    """How the unit's single-prediction sum is narrowed (X.anchor_values)."""
    return "u16" if unit == SCALE else "i16" if unit == SINGLE and not highbd else None


def conv_params(c):
    """The oracle's conv-param dict of a case (mode 0 single, 1 compound first
    pass, 2 average, 3 distance-weighted average)."""
    return dict(do_average=int(c.mode >= 2), round_0=c.round_0, round_1=c.round_1,
                is_compound=int(c.mode > 0), use_dist_wtd_comp_avg=int(c.mode == 3),
                fwd_offset=c.fwd_offset, bck_offset=c.bck_offset)


def conv_case(F, k):
    """Row k of conv_rows with its arrays: src (2-D, pixel dtype), off (element
    offset of the block in it), dst_in / buf_in (fresh copies) and the
    reference's dst / buf, all h x w."""
    c = SimpleNamespace(**{n: int(v) for n, v in zip(CONV_FIELDS, F["conv_rows"][k])})
    c.k = k
    c.pdt = np.uint16 if c.highbd else np.uint8
    n = c.w * c.h
    c.src = np.ascontiguousarray(
        F["conv_src"][c.src_off:c.src_off + c.src_h * c.src_w].reshape(c.src_h, c.src_w)
        .astype(c.pdt))
    c.off = c.org_y * c.src_w + c.org_x
    c.dst_in = np.full((c.h, c.w), F["fills"][0], c.pdt)
    if c.conv_in >= 0:
        o = int(F["conv_rows"][c.conv_in][CONV_FIELDS.index("out_off")])
        c.buf_in = F["conv_buf"][o:o + n].reshape(c.h, c.w).copy()
    else:
        c.buf_in = np.full((c.h, c.w), F["fills"][1], np.uint16)
    c.dst = F["conv_dst"][c.out_off:c.out_off + n].reshape(c.h, c.w)
    c.buf = F["conv_buf"][c.out_off:c.out_off + n].reshape(c.h, c.w)
    return c


def warp_case(F, k):
    c = SimpleNamespace(**{n: int(v) for n, v in zip(WARP_FIELDS, F["warp_rows"][k])})
    c.k = k
    c.pdt = np.uint16 if c.bd > 8 else np.uint8
    n = c.p_width * c.p_height
    c.ref = np.ascontiguousarray(
        F["warp_ref"][c.ref_off:c.ref_off + c.height * c.stride].reshape(c.height, c.stride)
        .astype(c.pdt))
    c.mat = [getattr(c, "m%d" % i) for i in range(6)]
    c.prm = (c.alpha, c.beta, c.gamma, c.delta)
    c.pred_in = np.full((c.p_height, c.p_width), F["fills"][0], c.pdt)
    if c.conv_in >= 0:
        o = int(F["warp_rows"][c.conv_in][WARP_FIELDS.index("out_off")])
        c.buf_in = F["warp_buf"][o:o + n].reshape(c.p_height, c.p_width).copy()
    else:
        c.buf_in = np.full((c.p_height, c.p_width), F["fills"][1], np.uint16)
    c.pred = F["warp_pred"][c.out_off:c.out_off + n].reshape(c.p_height, c.p_width)
    c.buf = F["warp_buf"][c.out_off:c.out_off + n].reshape(c.p_height, c.p_width)
    return c


def conv_kernels(c):
    """(kx, ky) of an aligned case from the reference's tables; None for a
    direction its path does not filter."""
    return (X.kernel(c.kind_x, c.phase_x) if c.path & 1 else None,
            X.kernel(c.kind_y, c.phase_y) if c.path & 2 else None)


def seen_window(plane, oy, ox, kx, ky):
    """The taps' window of the output pixel at (oy, ox) of `plane`."""
    ty = 1 if ky is None else len(ky)
    tx = 1 if kx is None else len(kx)
    y0 = oy - (ty // 2 - 1 if ty > 1 else 0)
    x0 = ox - (tx // 2 - 1 if tx > 1 else 0)
    return plane[y0:y0 + ty, x0:x0 + tx].astype(np.int64)


def conv_anchor(c):
    """(plain-integer values of the anchor from the stored source, the
    reference's stored anchor output) of an aligned first-pass / single case."""
    kx, ky = conv_kernels(c)
    win = seen_window(c.src, c.org_y + c.ay, c.org_x + c.ax, kx, ky)
    v = X.anchor_values(win, kx, ky, c.bd, c.round_0, c.round_1, c.mode > 0,
                        narrow=narrow_of(c.unit, c.highbd))
    v["win"] = win
    return v, int((c.buf if c.mode else c.dst)[c.ay, c.ax])


def coverage(conv_rows, warp_rows):
    """The phase / kind / path coverage the fixture promises, on the row tables."""
    J = {n: i for i, n in enumerate(CONV_FIELDS)}
    R = np.asarray(conv_rows)
    al = R[R[:, J["aligned"]] == 1]

    def phases(unit, path, mode, kind, hb, bd):
        m = ((al[:, J["unit"]] == unit) & (al[:, J["path"]] == path) & (al[:, J["mode"]] == mode)
             & (al[:, J["kind_x" if path & 1 else "kind_y"]] == kind) & (al[:, J["bd"]] == bd)
             & (al[:, J["highbd"]] == hb) & (al[:, J["kind_x"]] == al[:, J["kind_y"]]))
        return {(int(r[J["phase_x" if path & 1 else "phase_y"]]), int(r[J["polarity"]]))
                for r in al[m]}
    every = {(p, s) for p in range(1, 16) for s in (0, 1)}
    for hb, bd in ((0, 8), (1, 8), (1, 10), (1, 12)):
        for kind in range(7):
            ext = {(X.extreme_phase(kind), s) for s in (0, 1)}
            if (hb, bd) != (1, 8):
                for path in (1, 2, 3):
                    assert phases(SINGLE, path, 0, kind, hb, bd) == every, (bd, kind, path)
                assert phases(COMPOUND, 3, 1, kind, hb, bd) == every, (bd, kind)
                for path in (1, 2):
                    assert phases(COMPOUND, path, 1, kind, hb, bd) == ext, (bd, kind, path)
                for mode in (2, 3):
                    assert phases(COMPOUND, 3, mode, kind, hb, bd) == ext, (bd, kind, mode)
            want = every if kind in (X.SHARP, X.SHARP2) else ext
            for mode in (0, 1):
                assert phases(SCALE, 3, mode, kind, hb, bd) == want, (hb, bd, kind, mode)
        un = R[(R[:, J["aligned"]] == 0) & (R[:, J["highbd"]] == hb) & (R[:, J["bd"]] == bd)]
        assert {(int(r[J["x_step_qn"]]), int(r[J["kind_x"]]), int(r[J["mode"]])) for r in un} == \
            {(s, kd, m) for s in (2048, 512, 1365) for kd in (X.SHARP, X.SHARP2) for m in range(4)}
    pairs = {(int(r[J["fwd_offset"]]), int(r[J["bck_offset"]])) for r in R[R[:, J["mode"]] == 3]}
    assert len(pairs) == 8
    WJ = {n: i for i, n in enumerate(WARP_FIELDS)}
    Wr = np.asarray(warp_rows)
    for bd in (8, 10, 12):
        a = Wr[(Wr[:, WJ["bd"]] == bd) & (Wr[:, WJ["aligned"]] == 1)]
        for mode in (0, 1):
            for pol in (0, 1):
                s = a[(a[:, WJ["mode"]] == mode) & (a[:, WJ["polarity"]] == pol)]
                assert set(s[:, WJ["row_x"]]) == set(range(64, 128)), (bd, mode, pol)
                assert set(s[:, WJ["row_y"]]) == set(range(64, 128)), (bd, mode, pol)
        assert (a[:, WJ["mode"]] >= 2).sum() == 128
        sh = Wr[(Wr[:, WJ["bd"]] == bd) & (Wr[:, WJ["aligned"]] == 0)]
        assert len(sh) >= 6 * 9
        for f in ("alpha", "beta", "gamma", "delta"):
            assert np.abs(sh[:, WJ[f]]).max() >= 9216, (bd, f)
