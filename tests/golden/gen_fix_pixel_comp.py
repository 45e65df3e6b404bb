"""Golden fixtures of the masked / OBMC / distance-weighted pixel kinds, from
the reference's own C text executed by cinterp.py (as gen_fixtures.py does).

  fix_pixel_comp.npz
    a_bd{8,10,12}, b_bd{8,10,12}   two pixel planes per bit depth (_pix: one in
                                   eight near the extremes); strides 141 / 152
    second_bd*                     second_pred samples (compact w x h blocks)
    mask                           blend mask plane, 0..64, stride 137
    wsrc_bd*, omask                OBMC int32 streams: wsrc in
                                   [-(2^bd-1)*4096, (2^bd-1)*4096], mask 0..4096
    cases [n, 17]                  tests/_compref.py COLS; ret / sse are the
                                   reference's return value and *sse (ret is
                                   the row of x4d / the offset in pred_out for
                                   the x4d and prediction kinds)
    x4d [m, 4], pred_out           masked_sad x4d results; predicted blocks

Reference functions (all `_c`): aom_masked_sad*, aom_masked_sad*x4d,
aom_masked_sub_pixel_variance*, aom_obmc_sad*, aom_obmc_variance*,
aom_obmc_sub_pixel_variance*, aom_dist_wtd_sad*_avg,
aom_dist_wtd_sub_pixel_avg_variance*, their aom_highbd_ forms, and
aom[_highbd]_{comp_avg,dist_wtd_comp_avg,comp_mask}_pred.

Usage: python tests/golden/gen_fix_pixel_comp.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cinterp as C  # noqa: E402
import _compref as R  # noqa: E402
from gen_fixtures import ACMRandom, BLOCK_SIZES, REF, _pix, _set, check_errors  # noqa: E402

A_SHAPE, B_SHAPE, MASK_SHAPE = (131, 141), (131, 152), (130, 137)
NBLK = 128 * 128
QUANT_DIST = [(9, 7), (11, 5), (12, 4), (13, 3)]  # quant_dist_lookup_table (common_data.h:421)
DIST_PAIRS = QUANT_DIST + [(b, a) for a, b in QUANT_DIST]
SUBPEL = [(0, 0), (7, 3), (4, 4), (2, 7), (5, 0), (0, 6), (7, 7), (1, 2)]
EDGE_SIZES = [(4, 4), (16, 16), (128, 128)]
PRED_SIZES = [(4, 4), (4, 16), (8, 8), (16, 4), (16, 16), (32, 8), (64, 32)]
VARIANTS = [(8, 0), (8, 1), (10, 1), (12, 1)]  # (bd, highbd)


def tu_pixel_comp():
    return C.TU(REF, ["aom/aom_integer.h", "aom_ports/mem.h", "aom_dsp/aom_dsp_common.h",
                      "aom_dsp/aom_filter.h", "aom_dsp/blend.h", "aom_dsp/variance.h",
                      "aom_dsp/sad.c", "aom_dsp/variance.c", "aom_dsp/avg.c", "aom_dsp/sse.c",
                      "aom_dsp/subtract.c", "aom_dsp/sum_squares.c", "aom_dsp/blk_sse_sum.c",
                      "av1/encoder/rdopt.c", "aom_dsp/sad_av1.c"],
                C.reference_defines(REF))


def make_inputs():
    rnd = ACMRandom(0xbaba + 41)
    F = {}
    for bd in (8, 10, 12):
        mx = (1 << bd) - 1
        F["a_bd%d" % bd] = np.array(_pix(rnd, A_SHAPE[0] * A_SHAPE[1], bd), np.uint16).reshape(A_SHAPE)
        F["b_bd%d" % bd] = np.array(_pix(rnd, B_SHAPE[0] * B_SHAPE[1], bd), np.uint16).reshape(B_SHAPE)
        F["second_bd%d" % bd] = np.array(_pix(rnd, NBLK + 64, bd), np.uint16)
        span = 2 * mx * 4096 + 1
        F["wsrc_bd%d" % bd] = np.array(
            [((rnd.rand16() << 16) | rnd.rand16()) % span - mx * 4096 for _ in range(NBLK + 64)],
            np.int32)
    # blend mask: one in four at an end of the range
    m = []
    for _ in range(MASK_SHAPE[0] * MASK_SHAPE[1]):
        r = rnd.rand16()
        m.append((0, 64, 1, 63)[(r >> 2) & 3] if r & 3 == 0 else (r >> 4) % 65)
    F["mask"] = np.array(m, np.uint8).reshape(MASK_SHAPE)
    om = []
    for _ in range(NBLK + 64):
        r = rnd.rand16()
        om.append((0, 4096)[(r >> 3) & 1] if r & 7 == 0 else (r >> 3) % 4097)
    F["omask"] = np.array(om, np.int32)
    return F


class Runner:
    """Executes one case row with the reference's function."""

    def __init__(self, tu, F):
        self.tu, self.F = tu, F
        self.x4d, self.pred = [], []

    def ptrs(self, c):
        tu = self.tu
        et = "uint16_t" if c.highbd else "uint8_t"
        tag = (lambda p: tu.tagged(p)) if c.highbd else (lambda p: p)
        w, h = c.w, c.h
        # only the part of each plane the call can touch, from the case's first element
        na = h * c.a_stride + w + 2
        nb = (h + 1) * c.b_stride + w + 4
        self.bbuf = tu.buffer(et, c.b[:nb].tolist())
        return dict(a=tag(tu.buffer(et, c.a[:na].tolist())), b=tag(self.bbuf),
                    second=tag(tu.buffer(et, c.second.tolist())),
                    mask=tu.buffer("uint8_t", c.mask[:h * c.mask_stride].tolist()),
                    wsrc=tu.buffer("int32_t", c.wsrc.tolist()),
                    omask=tu.buffer("int32_t", c.omask.tolist()))

    def run(self, row):
        """Returns (ret, sse) to store in the row."""
        tu = self.tu
        c = R.case_inputs(self.F, row)
        p = self.ptrs(c)
        fn = tu.func(R.rtcd_name(c) + "_c")
        u32 = lambda v: v & 0xFFFFFFFF
        sse = tu.buffer("uint32_t", 1)
        jcp = tu.struct_obj("DIST_WTD_COMP_PARAMS")
        _set(jcp.buf[0], use_dist_wtd_comp_avg=1, fwd_offset=c.fwd, bck_offset=c.bck)
        k = c.kind
        if k == R.MSAD:
            return u32(fn(p["a"], c.a_stride, p["b"], c.b_stride, p["second"], p["mask"],
                          c.mask_stride, c.invert)), 0
        if k == R.MSAD_X4D:
            refs = [C.Pointer(self.bbuf.buf, o, self.bbuf.ty) for o in R.x4d_offsets(c.b_stride)]
            arr = C.Pointer(refs, 0, C.Ptr(C.UCHAR))
            o4 = tu.buffer("uint32_t", 4)
            fn(p["a"], c.a_stride, arr, c.b_stride, p["second"], p["mask"], c.mask_stride,
               c.invert, o4)
            self.x4d.append([u32(v) for v in o4.buf])
            return len(self.x4d) - 1, 0
        if k == R.MSVAR:
            v = fn(p["a"], c.a_stride, c.xoff, c.yoff, p["b"], c.b_stride, p["second"], p["mask"],
                   c.mask_stride, c.invert, sse)
            return u32(v), u32(sse.buf[0])
        if k == R.OSAD:
            return u32(fn(p["a"], c.a_stride, p["wsrc"], p["omask"])), 0
        if k == R.OVAR:
            v = fn(p["a"], c.a_stride, p["wsrc"], p["omask"], sse)
            return u32(v), u32(sse.buf[0])
        if k == R.OSVAR:
            v = fn(p["a"], c.a_stride, c.xoff, c.yoff, p["wsrc"], p["omask"], sse)
            return u32(v), u32(sse.buf[0])
        if k == R.JSAD:
            return u32(fn(p["a"], c.a_stride, p["b"], c.b_stride, p["second"], jcp)), 0
        if k == R.JSVAR:
            v = fn(p["a"], c.a_stride, c.xoff, c.yoff, p["b"], c.b_stride, sse, p["second"], jcp)
            return u32(v), u32(sse.buf[0])
        # prediction helpers
        et = "uint16_t" if c.highbd else "uint8_t"
        out = tu.buffer(et, [0] * (c.w * c.h))
        o = tu.tagged(out) if c.highbd else out
        if k == R.PRED_AVG:
            fn(o, p["second"], c.w, c.h, p["b"], c.b_stride)
        elif k == R.PRED_DIST:
            fn(o, p["second"], c.w, c.h, p["b"], c.b_stride, jcp)
        else:
            fn(o, p["second"], c.w, c.h, p["b"], c.b_stride, p["mask"], c.mask_stride, c.invert)
        off = sum(len(x) for x in self.pred)
        self.pred.append([int(v) for v in out.buf])
        return off, 0


def case_rows():
    """Every case row with ret = sse = 0 (filled by the Runner)."""
    rows = []
    n = [0]

    def add(kind, w, h, bd, hb, xoff=0, yoff=0, invert=0, pair=(0, 0), variant=0):
        i = n[0]
        n[0] += 1
        a_off = (i % 3) * A_SHAPE[1] + (i * 5) % 3      # rows 0..2, columns 0..2: odd offsets too
        b_off = ((i + 1) % 3) * B_SHAPE[1] + (i * 7) % 3
        s_off = (i * 11) % 64
        m_off = ((i + 2) % 2) * MASK_SHAPE[1] + (i * 3) % 4 if kind not in (
            R.OSAD, R.OVAR, R.OSVAR) else (i * 13) % 64
        rows.append([kind, w, h, bd, hb, a_off, b_off, s_off, m_off, xoff, yoff, invert,
                     pair[0], pair[1], variant, 0, 0])

    for si, (w, h) in enumerate(BLOCK_SIZES):
        for vi, (bd, hb) in enumerate(VARIANTS):
            t = si * 4 + vi
            # (0, 0), one offset with a 7, and a rotating third
            sub = [SUBPEL[0], SUBPEL[1 + 2 * (t % 2)], SUBPEL[2 + t % 6]]
            add(R.MSAD, w, h, bd, hb, invert=0)
            add(R.MSAD, w, h, bd, hb, invert=1)
            if not hb:
                add(R.MSAD_X4D, w, h, bd, hb, invert=t % 2)
            for k, (xo, yo) in enumerate(sub):
                add(R.MSVAR, w, h, bd, hb, xo, yo, invert=(t + k) % 2)
            add(R.OSAD, w, h, bd, hb)
            add(R.OVAR, w, h, bd, hb)
            for xo, yo in sub:
                add(R.OSVAR, w, h, bd, hb, xo, yo)
            add(R.JSAD, w, h, bd, hb, pair=DIST_PAIRS[t % 8])
            add(R.JSAD, w, h, bd, hb, pair=DIST_PAIRS[(t + 4) % 8])
            for k, (xo, yo) in enumerate(sub):
                add(R.JSVAR, w, h, bd, hb, xo, yo, pair=DIST_PAIRS[(t + 3 * k + 1) % 8])
    for (w, h) in EDGE_SIZES:
        for (bd, hb) in VARIANTS:
            for variant in (1, 2):
                add(R.MSAD, w, h, bd, hb, invert=variant - 1, variant=variant)
                add(R.MSVAR, w, h, bd, hb, 3, 5, invert=2 - variant, variant=variant)
            for variant in (3, 4):
                add(R.OSAD, w, h, bd, hb, variant=variant)
                add(R.OVAR, w, h, bd, hb, variant=variant)
                add(R.OSVAR, w, h, bd, hb, 7, 1, variant=variant)
    for kind, kw in ((R.MSAD, {}), (R.MSVAR, dict(xoff=4, yoff=7)), (R.OSAD, {}), (R.OVAR, {}),
                     (R.OSVAR, dict(xoff=7, yoff=4)), (R.JSAD, dict(pair=(9, 7))),
                     (R.JSVAR, dict(xoff=1, yoff=7, pair=(3, 13)))):
        add(kind, 128, 128, 12, 1, variant=5, **kw)
    for pi, (w, h) in enumerate(PRED_SIZES):
        for (bd, hb) in ((8, 0), (10, 1), (12, 1)):
            add(R.PRED_AVG, w, h, bd, hb)
            add(R.PRED_DIST, w, h, bd, hb, pair=DIST_PAIRS[(pi * 3 + bd) % 8])
            add(R.PRED_MASK, w, h, bd, hb, invert=0)
            add(R.PRED_MASK, w, h, bd, hb, invert=1)
    return rows


def main():
    tu = tu_pixel_comp()
    check_errors(tu, ["aom_masked_sad4x4_c", "aom_obmc_variance4x4_c",
                      "aom_highbd_12_dist_wtd_sub_pixel_avg_variance128x128_c",
                      "aom_highbd_comp_mask_pred_c"])
    F = make_inputs()
    rows = case_rows()
    run = Runner(tu, F)
    t0 = time.time()
    for i, row in enumerate(rows):
        row[R.COLS.index("ret")], row[R.COLS.index("sse")] = run.run(row)
        if i % 100 == 0:
            print("  case %d / %d  %.0fs" % (i, len(rows), time.time() - t0), flush=True)
    F["cases"] = np.array(rows, np.int64)
    F["x4d"] = np.array(run.x4d, np.int64)
    F["pred_out"] = np.array([v for p in run.pred for v in p], np.uint16)
    path = os.path.join(HERE, "fix_pixel_comp.npz")
    np.savez_compressed(path, **F)
    print("wrote %s: %d cases, %d bytes" % (path, len(rows), os.path.getsize(path)))


if __name__ == "__main__":
    main()
