"""Golden fixture of the interpolation filters on worst-case pixels, from the
reference's own C text executed by cinterp.py (as gen_fixtures.py does).

  fix_interp_extremes.npz
    conv_rows [n, len(conv_fields)]   single-reference (unit 0), compound (1)
                                      and scaled (2) convolutions
    conv_src                          ragged source windows: row k's is
                                      src_h x src_w at src_off, the block at
                                      (org_y, org_x) of it
    conv_dst, conv_buf                ragged w x h outputs at out_off: the
                                      prediction and the CONV_BUF.  Inputs are
                                      not stored: dst starts as fills[0]
                                      everywhere, the CONV_BUF as fills[1], or
                                      as the stored CONV_BUF of row conv_in
                                      for the averaging modes
    warp_rows / warp_ref / warp_pred / warp_buf   the same for the affine warp
                                      (the whole reference plane is stored)

The pixels are the aligned periodic windows of tests/_extremes.py: every
positive tap over 2^bd - 1 and every negative one over 0 (polarity 1) or the
reverse (0), for one output pixel (the anchor, (ay, ax)) of the block.

Reference functions (all `_c`): av1_convolve_{x,y,2d}_sr, av1_dist_wtd_convolve_
{2d_copy,x,y,2d}, av1_convolve_2d_scale, av1_warp_affine, their av1_highbd_
forms, and av1_get_shear_params.

Usage: python tests/golden/gen_fix_interp_extremes.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cinterp as C  # noqa: E402
import _extremes as X  # noqa: E402
from _extfix import (COMPOUND, CONV_FIELDS, SCALE, SINGLE, WARP_FIELDS, coverage,  # noqa: E402
                     narrow_of)
from gen_fixtures import QUANT_DIST, REF, _get, _set, check_errors  # noqa: E402

DIST_PAIRS = QUANT_DIST + [(b, a) for a, b in QUANT_DIST]
DST_FILL, BUF_FILL = 0x5A, 0x1234
VARIANTS = [(0, 8), (1, 8), (1, 10), (1, 12)]  # (highbd, bd) of the scaled functions


def tu_convolve():
    tu = C.TU(REF, ["aom/aom_integer.h", "aom_ports/mem.h", "aom_dsp/aom_dsp_common.h",
                    "aom_dsp/aom_filter.h", "av1/common/enums.h", "av1/common/filter.h",
                    "av1/common/convolve.h", "av1/common/convolve.c"],
              C.reference_defines(REF))
    check_errors(tu, ["av1_convolve_2d_sr_c", "av1_highbd_convolve_y_sr_c",
                      "av1_dist_wtd_convolve_2d_copy_c", "av1_highbd_dist_wtd_convolve_2d_c",
                      "av1_convolve_2d_scale_c", "av1_highbd_convolve_2d_scale_c",
                      "av1_get_interp_filter_params_with_block_size"])
    return tu


def tu_warp():
    tu = C.TU(REF, ["aom/aom_integer.h", "aom_ports/mem.h", "aom_dsp/aom_dsp_common.h",
                    "av1/common/enums.h", "av1/common/mv.h", "av1/common/convolve.h",
                    "av1/common/warped_motion.h", "av1/common/warped_motion.c"],
              C.reference_defines(REF))
    check_errors(tu, ["av1_warp_affine_c", "av1_highbd_warp_affine_c", "av1_get_shear_params"])
    return tu


def conv_params(tu, mode, r0, r1, conv, stride, fwd, bck):
    """ConvolveParams of mode 0 single, 1 compound first pass, 2 average,
    3 distance-weighted average."""
    cp = tu.struct_obj("ConvolveParams")
    _set(cp.buf[0], do_average=int(mode >= 2),
         dst=conv if mode else C.Pointer(None, 0, tu.ctype("CONV_BUF_TYPE")),
         dst_stride=stride if mode else 0, round_0=r0, round_1=r1, plane=0,
         is_compound=int(mode > 0), use_dist_wtd_comp_avg=int(mode == 3), fwd_offset=fwd,
         bck_offset=bck)
    return cp


class Conv:
    """Executes and collects the rows of the three convolution units."""

    def __init__(self, tu):
        self.tu = tu
        self.fpw = tu.func("av1_get_interp_filter_params_with_block_size")
        self.rows, self.src, self.dst, self.buf = [], [], [], []
        self.so = self.oo = 0
        self.n = 0

    def anchor(self, w, h):
        self.n += 1
        return X.anchors(w, h, 4 + w * h)[self.n % (4 + w * h)]

    def add(self, unit, hb, bd, w, h, path, kinds, phases, polarity, mode=0, pair=(0, 0),
            conv_in=-1, steps=(1024, 1024), subpel=None, src=None, org=None, anchor=None):
        """One reference call.  src None: the aligned window of (kinds, phases,
        polarity) around a rotating anchor.  Returns the row index."""
        tu = self.tu
        et = "uint16_t" if hb else "uint8_t"
        kx = X.kernel(kinds[0], phases[0]) if path & 1 else None
        ky = X.kernel(kinds[1], phases[1]) if path & 2 else None
        aligned = src is None
        if aligned:
            anchor = self.anchor(w, h) if anchor is None else anchor
            src, org = X.source(X.window(kx, ky, bd, polarity), w, h, anchor)
        else:
            anchor = (-1, -1)
        r0, r1 = X.conv_rounds(bd, mode > 0)
        sp = tu.buffer(et, src.reshape(-1).tolist())
        SS = src.shape[1]
        blk = C.Pointer(sp.buf, org[0] * SS + org[1], sp.ty)
        dp = tu.buffer(et, [DST_FILL] * (w * h))
        c_in = self.buf[conv_in].tolist() if conv_in >= 0 else [BUF_FILL] * (w * h)
        cb = tu.buffer("CONV_BUF_TYPE", c_in)
        cp = conv_params(tu, mode, r0, r1, cb, w, *pair)
        fpx = self.fpw(*X.kind_filter(kinds[0]))
        fpy = self.fpw(*X.kind_filter(kinds[1]))
        if subpel is None:
            subpel = (phases[0] << 6 if path & 1 else 0, phases[1] << 6 if path & 2 else 0)
        sx, sy = subpel[0] >> 6, subpel[1] >> 6
        a = [blk, SS, dp, w, w, h]
        if unit == SCALE:
            a += [fpx, fpy, subpel[0], steps[0], subpel[1], steps[1], cp]
            fn = "convolve_2d_scale_c"
        elif unit == SINGLE:
            a += [[], [fpx, sx, cp], [fpy, sy], [fpx, fpy, sx, sy, cp]][path]
            fn = ["", "convolve_x_sr_c", "convolve_y_sr_c", "convolve_2d_sr_c"][path]
        else:
            a += [[cp], [fpx, sx, cp], [fpy, sy, cp], [fpx, fpy, sx, sy, cp]][path]
            fn = ["dist_wtd_convolve_2d_copy_c", "dist_wtd_convolve_x_c", "dist_wtd_convolve_y_c",
                  "dist_wtd_convolve_2d_c"][path]
        if hb:
            a.append(bd)
        tu.func(("av1_highbd_" if hb else "av1_") + fn)(*a)
        self.rows.append([unit, hb, bd, w, h, path, kinds[0], kinds[1], phases[0], phases[1],
                          subpel[0], steps[0], subpel[1], steps[1], polarity, int(aligned),
                          anchor[0], anchor[1], mode, r0, r1, pair[0], pair[1], self.so,
                          src.shape[0], src.shape[1], org[0], org[1], self.oo, conv_in])
        self.src.append(src.reshape(-1).astype(np.uint16))
        self.dst.append(np.array(dp.buf, np.uint16))
        self.buf.append(np.array(cb.buf, np.uint16))
        self.so += src.size
        self.oo += w * h
        k = len(self.rows) - 1
        if aligned:
            self.check_anchor(k, kx, ky, polarity)
        return k

    def check_anchor(self, k, kx, ky, polarity):
        """The inputs are what they are meant to be: the reference's anchor
        output is the plain-integer value (int16 intermediates)."""
        r = dict(zip(CONV_FIELDS, self.rows[k]))
        if r["mode"] >= 2:
            return
        v = X.anchor_values(X.window(kx, ky, r["bd"], polarity), kx, ky, r["bd"], r["round_0"],
                            r["round_1"], r["mode"] > 0, narrow=narrow_of(r["unit"], r["highbd"]))
        got = int((self.buf if r["mode"] else self.dst)[k][r["ay"] * r["w"] + r["ax"]])
        assert got == v["final_i16"] & 0xFFFF, (r, v, got)
        self.last = v


def size_of(kind):
    return (4, 4) if X.kind_filter(kind)[1] == 4 else (8, 8)


def gen_single(cv, stats):
    for bd in (8, 10, 12):
        hb = int(bd > 8)
        for kind in range(7):
            w, h = size_of(kind)
            for phase in range(1, 16):
                for pol in (1, 0):
                    for path in (1, 2, 3):
                        cv.add(SINGLE, hb, bd, w, h, path, (kind, kind), (phase, phase), pol)
                        note(stats, "single2d", cv, kind, phase, bd, pol, path)
        ps, p2 = X.extreme_phase(X.SHARP), X.extreme_phase(X.SHARP2)
        for pol in (1, 0):
            cv.add(SINGLE, hb, bd, 8, 8, 3, (X.SHARP, X.SHARP2), (ps, p2), pol)
            cv.add(SINGLE, hb, bd, 8, 8, 3, (X.SHARP2, X.SHARP), (p2, ps), pol)
        print("  single bd %d: %d rows  %.0fs" % (bd, len(cv.rows), time.time() - T0), flush=True)


def note(stats, name, cv, kind, phase, bd, pol, path):
    """Collects what the generator's assertions need of the last aligned 2-D row."""
    if path != 3:
        return
    v = cv.last
    k = len(cv.rows) - 1
    r = dict(zip(CONV_FIELDS, cv.rows[k]))
    got = int((cv.buf if r["mode"] else cv.dst)[k][r["ay"] * r["w"] + r["ax"]])
    plain = v["final"] & 0xFFFF if r["mode"] else v["final"]
    if kind == X.SHARP2 and bd > 8 and v["wraps"] and got != plain:
        stats.setdefault(("wrap", name, bd), []).append(k)
    if kind == X.SHARP2 and bd == 8 and min(v["ims"]) < 0:
        stats.setdefault(("negative", name), []).append(k)
    name8 = X.KIND_NAMES[kind]
    if name8 in X.BOUNDS and phase == X.extreme_phase(kind):
        want = X.BOUNDS[name8][bd][pol]
        assert (max if pol else min)(v["ims"]) == want, (name, name8, bd, pol, v["ims"], want)
        stats.setdefault(("bound", name8, bd, pol), []).append(k)


def gen_compound(cv, stats):
    for bd in (8, 10, 12):
        hb = int(bd > 8)
        first = {}
        for kind in range(7):
            w, h = size_of(kind)
            pe = X.extreme_phase(kind)
            for phase in range(1, 16):
                for pol in (1, 0):
                    anchor = (h - 1, 1) if phase == pe else None
                    k = cv.add(COMPOUND, hb, bd, w, h, 3, (kind, kind), (phase, phase), pol,
                               mode=1, anchor=anchor)
                    note(stats, "compound2d", cv, kind, phase, bd, pol, 3)
                    if phase == pe:
                        first[kind, pol] = k
            for pol in (1, 0):
                for path in (1, 2):
                    cv.add(COMPOUND, hb, bd, w, h, path, (kind, kind), (pe, pe), pol, mode=1)
            # averages over the stored first pass: the same anchor, so the two
            # aligned pixels meet
            for pol in (1, 0):
                for cpol in (1, 0):
                    for i, pair in enumerate([(0, 0)] + DIST_PAIRS):
                        cv.add(COMPOUND, hb, bd, w, h, 3, (kind, kind), (pe, pe), pol,
                               mode=3 if i else 2, pair=pair, conv_in=first[kind, cpol],
                               anchor=(h - 1, 1))
        # copy: the all-max and all-0 blocks
        copies = {pol: cv.add(COMPOUND, hb, bd, 8, 8, 0, (0, 0), (0, 0), pol, mode=1)
                  for pol in (1, 0)}
        for pol in (1, 0):
            for cpol in (1, 0):
                for i, pair in enumerate([(0, 0)] + DIST_PAIRS):
                    cv.add(COMPOUND, hb, bd, 8, 8, 0, (0, 0), (0, 0), pol, mode=3 if i else 2,
                           pair=pair, conv_in=copies[cpol])
        print("  compound bd %d: %d rows  %.0fs" % (bd, len(cv.rows), time.time() - T0),
              flush=True)


def gen_scale(cv, stats):
    for hb, bd in VARIANTS:
        for kind in range(7):
            w, h = size_of(kind)
            all_phases = kind in (X.SHARP, X.SHARP2)
            for phase in (range(1, 16) if all_phases else (X.extreme_phase(kind),)):
                for pol in (1, 0):
                    for mode in (0, 1):
                        cv.add(SCALE, hb, bd, w, h, 3, (kind, kind), (phase, phase), pol, mode=mode)
                        note(stats, "scale", cv, kind, phase, bd, pol, 3)
        # unaligned steps over the periodic extreme planes
        n = 0
        for step in (2048, 512, 1365):
            for kind in (X.SHARP, X.SHARP2):
                pe = X.extreme_phase(kind)
                k_ = X.kernel(kind, pe)
                T = len(k_)
                spx, spy = (n * 320 + 64) % 1024, (n * 448 + 704) % 1024
                ext = ((7 * step + 1023) >> 10) + T + 1
                win = X.window(k_, k_, bd, n & 1)
                src = X.periodic(win, (ext, ext), (n % 5, n % 7))
                org = (T // 2 - 1, T // 2 - 1)
                kw = dict(steps=(step, step), subpel=(spx, spy), src=src, org=org)
                cv.add(SCALE, hb, bd, 8, 8, 3, (kind, kind), (pe, pe), n & 1, mode=0, **kw)
                k1 = cv.add(SCALE, hb, bd, 8, 8, 3, (kind, kind), (pe, pe), n & 1, mode=1, **kw)
                cv.add(SCALE, hb, bd, 8, 8, 3, (kind, kind), (pe, pe), n & 1, mode=2, conv_in=k1,
                       **kw)
                cv.add(SCALE, hb, bd, 8, 8, 3, (kind, kind), (pe, pe), n & 1, mode=3, conv_in=k1,
                       pair=DIST_PAIRS[n % 8], **kw)
                n += 1
        print("  scale hb %d bd %d: %d rows  %.0fs" % (hb, bd, len(cv.rows), time.time() - T0),
              flush=True)


# large-shear candidates (m2, m3, m4, m5): the largest |alpha|, |beta|, |gamma|
# and |delta| that 4|a| + 7|b| < 2^16 and 4|g| + 4|d| < 2^16 leave room for
SHEAR = [(65536 + 16192, 0, 0, 65536), (65536 - 16192, 0, 0, 65536), (65536, 9280, 0, 65536),
         (65536, -9280, 0, 65536), (65536, 0, 16192, 65536), (65536, 0, -16192, 65536),
         (65536, 0, 0, 65536 + 16192), (65536, 0, 0, 65536 - 16192),
         (65536 + 8000, -4500, 8000, 65536 - 8000), (65536 - 8000, 4500, -8000, 65536 + 8100)]


class Warp:
    def __init__(self, tu):
        self.tu = tu
        self.rows, self.ref, self.pred, self.buf = [], [], [], []
        self.ro = self.oo = 0

    def shear(self, mat):
        tu = self.tu
        wm = tu.struct_obj("WarpedMotionParams")
        wmat = _get(wm.buf[0], "wmmat")
        for i in range(6):
            wmat[i] = mat[i]
        ok = tu.func("av1_get_shear_params")(wm)
        return ok, tuple(_get(wm.buf[0], k) for k in ("alpha", "beta", "gamma", "delta"))

    def add(self, bd, mode, polarity, ref, mat, prm, p_col, p_row, pw, ph, rows=(-1, -1),
            anchor=(-1, -1), conv_in=-1, pair=(0, 0), new_ref=True):
        tu = self.tu
        hb = bd > 8
        et = "uint16_t" if hb else "uint8_t"
        H, W = ref.shape
        r0, r1 = X.conv_rounds(bd, mode > 0)
        rp = tu.buffer(et, ref.reshape(-1).tolist())
        pbuf = tu.buffer(et, [DST_FILL] * (pw * ph))
        c_in = self.buf[conv_in].tolist() if conv_in >= 0 else [BUF_FILL] * (pw * ph)
        cb = tu.buffer("CONV_BUF_TYPE", c_in)
        cp = conv_params(tu, mode, r0, r1, cb, pw, *pair)
        a = [tu.buffer("int32_t", list(mat)), rp, W, H, W, pbuf, p_col, p_row, pw, ph, pw, 0, 0]
        if hb:
            tu.func("av1_highbd_warp_affine_c")(*a, bd, cp, *prm)
        else:
            tu.func("av1_warp_affine_c")(*a, cp, *prm)
        if new_ref:
            self.ref_off = self.ro
            self.ref.append(ref.reshape(-1).astype(np.uint16))
            self.ro += ref.size
        self.rows.append([bd, mode, polarity, int(rows[0] >= 0), rows[0], rows[1], anchor[0],
                          anchor[1]] + list(mat) + list(prm) +
                         [W, H, W, p_col, p_row, pw, ph, r0, r1, pair[0], pair[1], self.ref_off,
                          self.oo, conv_in])
        self.pred.append(np.array(pbuf.buf, np.uint16))
        self.buf.append(np.array(cb.buf, np.uint16))
        self.oo += pw * ph
        return len(self.rows) - 1


def gen_warp(wp, stats):
    er = X.extreme_warp_row()
    assert 64 <= er < 128, er
    for bd in (8, 10, 12):
        for q in range(64):
            # filter rows 64 + q horizontally and 64 + q' vertically: every row
            # 64..127 in each direction, the extreme one paired with itself
            qx, qy = q, (5 * (q - (er - 64)) + er - 64) % 64
            kx, ky = X.WARPED_FILTER[64 + qx], X.WARPED_FILTER[64 + qy]
            mat = [qx << 10, qy << 10, 1 << 16, 0, 0, 1 << 16]
            for pol in (1, 0):
                anchor = X.anchors(8, 8, 68)[(q * 2 + pol + bd) % 68]
                win = X.window(kx, ky, bd, pol)
                ref, org = X.source(win, 8, 8, anchor)
                assert org == (3, 3) and ref.shape == (15, 15)
                kw = dict(rows=(64 + qx, 64 + qy), anchor=anchor)
                k0 = wp.add(bd, 0, pol, ref, mat, (0, 0, 0, 0), 3, 3, 8, 8, **kw)
                k1 = wp.add(bd, 1, pol, ref, mat, (0, 0, 0, 0), 3, 3, 8, 8, new_ref=False, **kw)
                pair = DIST_PAIRS[(q + pol) % 8] if q & 1 else (0, 0)
                wp.add(bd, 3 if q & 1 else 2, pol, ref, mat, (0, 0, 0, 0), 3, 3, 8, 8,
                       conv_in=k1, pair=pair, new_ref=False, **kw)
                for k, comp in ((k0, False), (k1, True)):
                    r0, r1 = X.conv_rounds(bd, comp)
                    v = X.anchor_values(win, kx, ky, bd, r0, r1, comp)
                    got = int((wp.buf if comp else wp.pred)[k][anchor[0] * 8 + anchor[1]])
                    assert not v["wraps"] and got == v["final"], (bd, q, pol, v, got)
                if qx == qy == er - 64:
                    want = X.BOUNDS["WARP"][bd][pol]
                    assert (max if pol else min)(v["ims"]) == want, (bd, pol, v["ims"], want)
                    stats.setdefault(("bound", "WARP", bd, pol), []).append(k0)
        # large shears over a period-8 extreme plane; blocks whose 8x8 units
        # cross each edge of the reference
        W, H = 32, 24
        ke = X.WARPED_FILTER[er]
        n = 0
        for m2, m3, m4, m5 in SHEAR:
            mat = [(n * 9157 + 300) % 65536 - 20000 * (n & 1), (n * 5413 + 1700) % 65536, m2, m3,
                   m4, m5]
            ok, prm = wp.shear(mat)
            if not ok:
                continue
            ref = X.periodic(X.window(ke, ke, bd, n & 1), (H, W), (n % 8, (n * 3) % 8))
            first = True
            for (pc, pr, pw, ph) in ((0, 0, 8, 8), (W - 8, H - 8, 8, 8), (8, 8, 16, 8)):
                k1 = -1
                for mode in (0, 1, 2):
                    k = wp.add(bd, mode, n & 1, ref, mat, prm, pc, pr, pw, ph,
                               conv_in=k1 if mode == 2 else -1, new_ref=first)
                    first = False
                    k1 = k if mode == 1 else k1
            stats.setdefault(("shear", bd), []).append(prm)
            n += 1
        assert n >= 6, n
        print("  warp bd %d: %d rows  %.0fs" % (bd, len(wp.rows), time.time() - T0), flush=True)


def main():
    global T0
    T0 = time.time()
    stats = {}
    cv = Conv(tu_convolve())
    gen_single(cv, stats)
    gen_compound(cv, stats)
    gen_scale(cv, stats)
    wp = Warp(tu_warp())
    gen_warp(wp, stats)
    coverage(cv.rows, wp.rows)
    for bd in (10, 12):
        for name in ("single2d", "compound2d", "scale"):
            assert stats.get(("wrap", name, bd)), ("no SHARP2 int16 wrap", name, bd)
    for name in ("single2d", "compound2d", "scale"):
        assert stats.get(("negative", name)), ("no negative bd-8 intermediate", name)
    for name in ("SHARP", "REGULAR", "SHARP2", "WARP"):
        for bd in (8, 10, 12):
            for pol in (0, 1):
                assert stats.get(("bound", name, bd, pol)), ("bound not reached", name, bd, pol)
    wrap_rows = sorted(k for key, v in stats.items() if key[0] == "wrap" for k in v)
    out = {"conv_rows": np.array(cv.rows, np.int32), "conv_src": np.concatenate(cv.src),
           "conv_dst": np.concatenate(cv.dst), "conv_buf": np.concatenate(cv.buf),
           "conv_fields": np.array(CONV_FIELDS), "fills": np.array([DST_FILL, BUF_FILL]),
           "wrap_rows": np.array(wrap_rows, np.int32),
           "warp_rows": np.array(wp.rows, np.int32), "warp_ref": np.concatenate(wp.ref),
           "warp_pred": np.concatenate(wp.pred), "warp_buf": np.concatenate(wp.buf),
           "warp_fields": np.array(WARP_FIELDS)}
    path = os.path.join(HERE, "fix_interp_extremes.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d + %d rows, %d wrap rows, %d bytes, %.0f s" % (
        path, len(cv.rows), len(wp.rows), len(wrap_rows), os.path.getsize(path),
        time.time() - T0))


if __name__ == "__main__":
    main()
