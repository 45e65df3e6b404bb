"""Golden fixture of the mask-building and blending layer, from the
reference's own C text executed by cinterp.py (as gen_fix_pixel_comp.py does).

  fix_blend.npz
    pa_bd{8,10,12}, pb_bd*     two pixel planes per bit depth (_pix: one in eight
                               near the extremes); strides 141 / 152
    da_bd*, db_bd*             CONV_BUF_TYPE planes of the same shapes, inside
                               d16_range[bd] = (lo, hi): the smallest and the
                               largest value the compound first pass can write
                               (2-D sharp filter at its extreme phase on the
                               worst-case window, tests/_extremes.py), one in
                               four at an end
    mask2d, mask1d             blend masks, 0..64 (one in four at an end);
                               mask1d starts with obmc_masks
    obmc_masks                 av1_get_obmc_mask(n), n = 1, 2, 4 .. 64, back to
                               back: the 127-byte table the OBMC calls take
    wedge_masks_{W}x{H}        [16 wedges, 2 signs, H, W] of the 9 wedge block
                               sizes (init_wedge_master_masks + init_wedge_masks)
    blend_cases, blend_out     tests/_blendref.py B_COLS; the blended blocks
    dw_cases, dw_out           D_COLS; the diff-weighted masks
    wedge_cases, wedge_out     W_COLS (ret: the sse / the sign / the offset of
                               the delta squares in wedge_out); res8_*, res12_*
                               the residual streams, wedge_m the masks
    obmc_cases                 O_COLS, one row per (scene of
                               _blendref.OBMC_SCENES, plane): the bitmaps a
                               visitor of this generator recorded on the
                               reference's neighbour walk, and
    obmc_wsrc, obmc_mask       calc_target_weighted_pred's two blocks (luma),
    obmc_pred                  av1_build_obmc_inter_prediction's plane

Reference functions executed: aom_blend_a64_{mask,hmask,vmask}_c, their
aom_highbd_ forms, aom_{lowbd,highbd}_blend_a64_d16_mask_c,
av1_build_compound_diffwtd_mask{,_highbd,_d16}_c, calc_target_weighted_pred and
av1_build_obmc_inter_prediction whole (foreach_overlappable_nb_above / _left,
is_neighbor_overlappable, av1_skip_u4x4_pred_in_obmc, av1_get_obmc_mask) over
an xd->mi grid built here, av1_wedge_{sse,sign}_from_residuals_c,
av1_wedge_compute_delta_squares_c, init_wedge_master_masks, init_wedge_masks.
The pixel forms of the reference assert only w, h >= 1, so the 2x2 and the
1- and 2-wide chroma OBMC spans are in; the lowbd d16 form asserts w, h >= 4.

Usage: python tests/golden/gen_fix_blend.py
"""
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cinterp as C  # noqa: E402
import _blendref as R  # noqa: E402
import _extremes as X  # noqa: E402
from gen_fixtures import ACMRandom, REF, _get, _pix, _set, check_errors  # noqa: E402

A_SHAPE, B_SHAPE = (R.PLANE_ROWS, R.A_STRIDE), (R.PLANE_ROWS, R.B_STRIDE)
MASK_SHAPE = (R.MASK_ROWS, R.MASK_STRIDE)
SIZES, SMALL, SUBS, WEDGE_SIZES = R.SIZES, R.SMALL, R.SUBS, R.WEDGE_SIZES
YV12_FLAG_HIGHBITDEPTH = 8  # aom_scale/yv12config.h

VISITOR = """
void lavish_record_nb(MACROBLOCKD *xd, int rel_mi_row, int rel_mi_col, uint8_t op_mi_size,
                      int dir, MB_MODE_INFO *nb_mi, void *fun_ctxt, const int num_planes) {
  uint32_t *bits = (uint32_t *)fun_ctxt;
  const int start = dir ? rel_mi_row : rel_mi_col;
  for (int k = 0; k < op_mi_size; ++k) bits[dir] |= 1u << (start + k);
}
void lavish_record_walk(const AV1_COMMON *cm, MACROBLOCKD *xd, uint32_t *bits) {
  const BLOCK_SIZE bsize = xd->mi[0]->bsize;
  bits[0] = 0;
  bits[1] = 0;
  foreach_overlappable_nb_above(cm, xd, max_neighbor_obmc[mi_size_wide_log2[bsize]],
                                lavish_record_nb, bits);
  foreach_overlappable_nb_left(cm, xd, max_neighbor_obmc[mi_size_high_log2[bsize]],
                               lavish_record_nb, bits);
}
"""


def hbd_obmc_text():
    """build_obmc_inter_pred_above / _left and av1_build_obmc_inter_prediction
    (av1/common/reconinter.c) read from the reference and renamed lavish_hbd_*,
    with their four `&base[index]` written `(base + (index))`: cinterp.py takes
    the address of an element only inside a buffer it knows, and a highbd plane
    pointer is a tagged address (CONVERT_TO_BYTEPTR).  The two spellings mean
    the same in C; the 8-bit scenes execute the reference's own text."""
    with open(os.path.join(REF, "av1/common/reconinter.c")) as fh:
        lines = fh.read().split("\n")
    a = next(i for i, l in enumerate(lines) if "void build_obmc_inter_pred_above(" in l)
    b = next(i for i, l in enumerate(lines) if "void av1_setup_obmc_dst_bufs(" in l)
    text, n = re.subn(r"&(pd->dst\.buf|ctxt->adjacent\[plane\])\[([^\]]+)\]", r"(\1 + (\2))",
                      "\n".join(lines[a:b]))
    assert n == 4, n
    for nm in ("build_obmc_inter_pred_above", "build_obmc_inter_pred_left",
               "av1_build_obmc_inter_prediction"):
        text = text.replace(nm, "lavish_hbd_" + nm)
    return text, "<reconinter.c:%d-%d>" % (a + 1, b)


def tu_blend():
    tu = C.TU(REF, ["aom/aom_integer.h", "aom_ports/mem.h", "aom_dsp/aom_dsp_common.h",
                    "aom_dsp/aom_filter.h", "aom_dsp/blend.h", "aom_dsp/variance.h",
                    "aom_dsp/aom_convolve.c", "aom_dsp/blend_a64_mask.c",
                    "aom_dsp/blend_a64_hmask.c", "aom_dsp/blend_a64_vmask.c",
                    "av1/common/common_data.c", "av1/common/reconinter.c",
                    "av1/encoder/wedge_utils.c",
                    "av1/encoder/rdopt.c"],
              C.reference_defines(REF))
    tu.add_source(VISITOR, "<gen_fix_blend.py visitor>")
    tu.add_source(*hbd_obmc_text())
    check_errors(tu, ["aom_blend_a64_mask_c", "aom_blend_a64_hmask_c", "aom_blend_a64_vmask_c",
                      "aom_highbd_blend_a64_mask_c", "aom_highbd_blend_a64_hmask_c",
                      "aom_highbd_blend_a64_vmask_c", "aom_lowbd_blend_a64_d16_mask_c",
                      "aom_highbd_blend_a64_d16_mask_c", "av1_build_compound_diffwtd_mask_c",
                      "av1_build_compound_diffwtd_mask_highbd_c",
                      "av1_build_compound_diffwtd_mask_d16_c", "calc_target_weighted_pred",
                      "av1_build_obmc_inter_prediction", "foreach_overlappable_nb_above",
                      "foreach_overlappable_nb_left", "is_neighbor_overlappable",
                      "av1_skip_u4x4_pred_in_obmc", "av1_get_obmc_mask",
                      "av1_wedge_sse_from_residuals_c", "av1_wedge_sign_from_residuals_c",
                      "av1_wedge_compute_delta_squares_c", "init_wedge_master_masks",
                      "init_wedge_masks", "lavish_record_walk",
                      "lavish_hbd_av1_build_obmc_inter_prediction"])
    return tu


def d16_range(bd):
    """(lo, hi) of the CONV_BUF_TYPE values of the compound first pass."""
    r0, r1 = X.conv_rounds(bd, True)
    k = X.kernel(X.SHARP, X.extreme_phase(X.SHARP))
    return tuple(X.anchor_values(X.window(k, k, bd, pol), k, k, bd, r0, r1, True)["final"]
                 for pol in (0, 1))


def obmc_table(tu):
    tab = []
    for n in R.OBMC_LENGTHS:
        p = tu.func("av1_get_obmc_mask")(n)
        tab += [int(p.buf[p.off + i]) for i in range(n)]
    return np.array(tab, np.uint8)


def wedge_masks(tu):
    """init_wedge_master_masks + init_wedge_masks, then wedge_mask_buf cut up in
    the order init_wedge_masks fills it (bsize order, wedge, sign)."""
    tu.func("init_wedge_master_masks")()
    tu.func("init_wedge_masks")()
    buf = tu.global_value("wedge_mask_buf")
    E = tu.enums
    out, pos = {}, 0
    for w, h in sorted(WEDGE_SIZES, key=lambda s: E["BLOCK_%dX%d" % s]):
        n = 16 * 2 * w * h
        out["wedge_masks_%dx%d" % (w, h)] = np.array(buf[pos:pos + n], np.uint8).reshape(16, 2, h,
                                                                                         w)
        pos += n
    return out


def make_inputs(tu):
    rnd = ACMRandom(0xbaba + 57)
    F = {}
    rng = []
    for bd in (8, 10, 12):
        F["pa_bd%d" % bd] = np.array(_pix(rnd, A_SHAPE[0] * A_SHAPE[1], bd), np.uint16).reshape(A_SHAPE)
        F["pb_bd%d" % bd] = np.array(_pix(rnd, B_SHAPE[0] * B_SHAPE[1], bd), np.uint16).reshape(B_SHAPE)
        lo, hi = d16_range(bd)
        assert 0 <= lo < hi <= 0xFFFF, (bd, lo, hi)
        rng.append((lo, hi))
        for nm, shp in (("da", A_SHAPE), ("db", B_SHAPE)):
            v = []
            for _ in range(shp[0] * shp[1]):
                r = rnd.rand16()
                v.append((lo, hi)[(r >> 2) & 1] if r & 3 == 0 else lo + (r >> 3) * 7 % (hi - lo + 1))
            F["%s_bd%d" % (nm, bd)] = np.array(v, np.uint16).reshape(shp)
    F["d16_range"] = np.array(rng, np.int64)

    def masks(n):
        m = []
        for _ in range(n):
            r = rnd.rand16()
            m.append((0, 64, 1, 63)[(r >> 2) & 3] if r & 3 == 0 else (r >> 4) % 65)
        return m
    F["mask2d"] = np.array(masks(MASK_SHAPE[0] * MASK_SHAPE[1]), np.uint8).reshape(MASK_SHAPE)
    F["obmc_masks"] = obmc_table(tu)
    F["mask1d"] = np.concatenate([F["obmc_masks"], np.array(masks(400), np.uint8)])
    F.update(wedge_masks(tu))
    # residual streams: 8-bit range (the clamp of the sse never engages) and 12-bit range
    for nm, lim in (("res8", 255), ("res12", 4095)):
        for ab in "ab":
            F["%s_%s" % (nm, ab)] = np.array(
                [rnd.rand16() % (2 * lim + 1) - lim
                 for _ in range((16384 if lim == 4095 else 1024) + 64)], np.int16)
    # masks of the wedge cases: the 32x32, 8x8 and 16x8 wedge masks, then a 0..64 stream
    wm = [F["wedge_masks_32x32"][5, 0].reshape(-1), F["wedge_masks_8x8"][3, 1].reshape(-1),
          F["wedge_masks_16x8"][9, 0].reshape(-1), np.array(masks(16384 + 64), np.uint8)]
    F["wedge_m"] = np.concatenate(wm).astype(np.uint8)
    return F


# ------------------------------------------------------------------ cases --
def blend_rows():
    rows, n = [], [0]

    def add(form, w, h, sub=(0, 0), bd=8, hb=0, variant=0, r=(0, 0)):
        i = n[0]
        n[0] += 1
        s0 = (i % 3) * R.A_STRIDE + (i * 5) % 3
        s1 = ((i + 1) % 3) * R.B_STRIDE + (i * 7) % 3
        if form == R.F_HMASK:
            m = w - 1 if w <= 64 and i % 2 == 0 else 127 + (i * 3) % 16
        elif form == R.F_VMASK:
            m = h - 1 if h <= 64 and i % 2 == 0 else 127 + (i * 3) % 16
        else:
            m = (i % 2) * R.MASK_STRIDE + (i * 3) % 4
        rows.append([form, w, h, sub[0], sub[1], bd, hb, variant, s0, s1, m, r[0], r[1], 0])

    d16v = [(8, 0), (10, 1), (12, 1)]
    for si, (w, h) in enumerate(SIZES):
        big = w == 128
        for k, sub in enumerate(SUBS):
            if not big or k < 2:
                add(R.F_MASK, w, h, sub)
            if not big or k == 2:
                add(R.F_MASK, w, h, sub, bd=(10, 12, 12, 8)[(k + si) % 4], hb=1)
        for form in (R.F_HMASK, R.F_VMASK):
            if not big or form == R.F_HMASK:
                add(form, w, h)
            if not big or form == R.F_VMASK:
                add(form, w, h, bd=10 + 2 * (si % 2), hb=1)
        for k, sub in enumerate(SUBS):
            for vi, (bd, hb) in enumerate(d16v):
                if big and (k, vi) not in ((3, 0), (0, 2)):
                    continue
                add(R.F_D16, w, h, sub, bd=bd, hb=hb, r=X.conv_rounds(bd, True))
    for (w, h) in ((4, 4), (64, 32)):
        for variant in (1, 2):
            add(R.F_MASK, w, h, SUBS[variant], variant=variant)
            add(R.F_MASK, w, h, SUBS[3 - variant], bd=12, hb=1, variant=variant)
            add(R.F_D16, w, h, bd=10, hb=1, variant=variant, r=X.conv_rounds(10, True))
        for bd, hb in ((8, 0), (8, 1), (10, 1), (12, 1)):
            add(R.F_MASK, w, h, SUBS[bd % 3], bd=bd, hb=hb, variant=3)
        add(R.F_HMASK, w, h, bd=12, hb=1, variant=3)
        add(R.F_VMASK, w, h, variant=3)
    for (w, h) in ((4, 4), (64, 32), (128, 128)):
        for bd, hb in d16v:
            if w == 128 and bd != 12:
                continue
            for variant in (3, 4, 5):
                add(R.F_D16, w, h, SUBS[(variant + bd) % 4], bd=bd, hb=hb, variant=variant,
                    r=X.conv_rounds(bd, True))
    for (w, h) in SMALL:
        for sub in SUBS:
            add(R.F_MASK, w, h, sub)
        add(R.F_MASK, w, h, SUBS[w % 4], bd=10, hb=1)
        add(R.F_HMASK, w, h)
        add(R.F_VMASK, w, h)
        add(R.F_HMASK, w, h, bd=12, hb=1)
        add(R.F_VMASK, w, h, bd=10, hb=1)
    return rows


def diffwtd_rows():
    rows, n = [], [0]

    def add(form, w, h, bd, mask_type, variant=0):
        i = n[0]
        n[0] += 1
        r = X.conv_rounds(bd, True) if form == 2 else (0, 0)
        rows.append([form, w, h, bd, mask_type, variant, (i % 3) * R.A_STRIDE + (i * 5) % 3,
                     ((i + 1) % 3) * R.B_STRIDE + (i * 7) % 3, r[0], r[1], 0])

    for si, (w, h) in enumerate([(8, 8), (4, 16), (16, 4), (64, 32), (128, 128)]):
        for mt in (0, 1):
            if w == 128 and mt != si % 2:
                add(2, w, h, 12, mt)
                continue
            add(0, w, h, 8, mt)
            for bd in (8, 10, 12):
                add(1, w, h, bd, mt)
                add(2, w, h, bd, mt)
    for (w, h) in ((8, 8), (16, 4)):
        for bd in (8, 10, 12):
            for mt in (0, 1):
                add(2, w, h, bd, mt, variant=5)  # clamps at 64
                add(2, w, h, bd, mt, variant=6)  # stays at 38
                add(1, w, h, bd, mt, variant=6)
            add(0 if bd == 8 else 1, w, h, bd, bd == 10, variant=6)
    return rows


def wedge_rows(F):
    rows = []
    m32, m8, m16x8, mr = 0, 1024, 1024 + 64, 1024 + 64 + 128
    n = [0]

    def add(kind, N, variant, m_off, limit=0):
        i = n[0]
        n[0] += 1
        rows.append([kind, N, (i * 2) % 64, (i * 6 + 1) % 64, m_off, variant, limit, 0])

    for N, m_off in ((64, m8), (128, m16x8), (1024, m32), (16384, mr)):
        for variant in (0, 1, 2)[N == 16384:]:  # (the 8-bit streams stop at 1024)
            add(0, N, variant, m_off)
            add(1, N, variant, m_off)
        for variant in (0, 1)[N == 16384:]:
            add(2, N, variant, m_off + (0 if N != 16384 else 3), 0)
            add(2, N, variant, m_off, 12345)
    # acc == limit (not greater), and one below it
    for N, m_off in ((64, m8), (1024, m32)):
        row = [2, N, 0, 1, m_off, 0, 0, 0]
        c = R.wedge_case(F, row)
        acc = R.wedge_sign_acc(c.a, c.m)
        rows.append([2, N, 0, 1, m_off, 0, acc, 0])
        rows.append([2, N, 0, 1, m_off, 0, acc - 1, 0])
    return rows


# ---------------------------------------------------------------- runners --
def _embed(tu, et, block, stride):
    """A block in a buffer of row stride `stride` (the gaps hold 0)."""
    h, w = block.shape
    buf = np.zeros((h, stride), np.int64)
    buf[:, :w] = block
    return tu.buffer(et, buf.reshape(-1).tolist())


class Runner:
    def __init__(self, tu, F):
        self.tu, self.F = tu, F

    def cp(self, r0, r1):
        cp = self.tu.struct_obj("ConvolveParams")
        _set(cp.buf[0], round_0=r0, round_1=r1, is_compound=1)
        return cp

    def blend(self, row):
        tu = self.tu
        c = R.blend_case(self.F, row)
        w, h = c.w, c.h
        d16 = c.form == R.F_D16
        pet = "uint16_t" if c.highbd else "uint8_t"
        set_ = "uint16_t" if d16 or c.highbd else "uint8_t"
        tag = (lambda p: tu.tagged(p)) if c.highbd else (lambda p: p)
        ds, s0s, s1s = w + 1, w + 3, w + 2
        dst = tu.buffer(pet, [0] * (h * ds))
        s0, s1 = _embed(tu, set_, c.s0, s0s), _embed(tu, set_, c.s1, s1s)
        if not d16:
            s0, s1 = tag(s0), tag(s1)
        if c.form in (R.F_HMASK, R.F_VMASK):
            mask = tu.buffer("uint8_t", c.mask.tolist())
            name = ("aom_highbd_" if c.highbd else "aom_") + \
                ("blend_a64_hmask_c" if c.form == R.F_HMASK else "blend_a64_vmask_c")
            args = [tag(dst), ds, s0, s0s, s1, s1s, mask, w, h] + ([c.bd] if c.highbd else [])
        else:
            ms = c.mask.shape[1] + 5
            mask = _embed(tu, "uint8_t", c.mask, ms)
            args = [tag(dst), ds, s0, s0s, s1, s1s, mask, ms, w, h, c.subw, c.subh]
            if d16:
                name = "aom_highbd_blend_a64_d16_mask_c" if c.highbd else \
                    "aom_lowbd_blend_a64_d16_mask_c"
                args += [self.cp(c.r0, c.r1)] + ([c.bd] if c.highbd else [])
            else:
                name = "aom_highbd_blend_a64_mask_c" if c.highbd else "aom_blend_a64_mask_c"
                args += [c.bd] if c.highbd else []
        tu.func(name)(*args)
        return np.array(dst.buf, np.int64).reshape(h, ds)[:, :w]

    def diffwtd(self, row):
        tu = self.tu
        c = R.diffwtd_case(self.F, row)
        w, h = c.w, c.h
        et = "uint8_t" if c.form == 0 else "uint16_t"
        s0s, s1s = w + 2, w + 7
        s0, s1 = _embed(tu, et, c.s0, s0s), _embed(tu, et, c.s1, s1s)
        mask = tu.buffer("uint8_t", [0] * (w * h))
        if c.form == 0:
            tu.func("av1_build_compound_diffwtd_mask_c")(mask, c.mask_type, s0, s0s, s1, s1s, h, w)
        elif c.form == 1:
            tu.func("av1_build_compound_diffwtd_mask_highbd_c")(
                mask, c.mask_type, tu.tagged(s0), s0s, tu.tagged(s1), s1s, h, w, c.bd)
        else:
            tu.func("av1_build_compound_diffwtd_mask_d16_c")(
                mask, c.mask_type, s0, s0s, s1, s1s, h, w, self.cp(c.r0, c.r1), c.bd)
        return np.array(mask.buf, np.int64).reshape(h, w)

    def wedge(self, row):
        """kind 0: the d array; else the return value."""
        tu = self.tu
        c = R.wedge_case(self.F, row)
        a, b = tu.buffer("int16_t", c.a.tolist()), tu.buffer("int16_t", c.b.tolist())
        m = tu.buffer("uint8_t", c.m.tolist())
        if c.kind == 0:
            d = tu.buffer("int16_t", [0] * c.n)
            tu.func("av1_wedge_compute_delta_squares_c")(d, a, b, c.n)
            return np.array(d.buf, np.int64)
        if c.kind == 1:
            return int(tu.func("av1_wedge_sse_from_residuals_c")(a, b, m, c.n))
        return int(tu.func("av1_wedge_sign_from_residuals_c")(a, m, c.n, c.limit))

    # ---- OBMC: the reference's walk over an mi grid built for the scene ----
    def scene_objects(self, sc):
        tu, E = self.tu, self.tu.enums
        hbd = sc["bd"] > 8
        stride = sc["mi_cols"] + 40
        rows = sc["mi_rows"] + 40
        grid = [None] * (rows * stride)
        mbt = tu.ctype("MB_MODE_INFO")

        def mbmi(w, h, inter):
            p = tu.struct_obj("MB_MODE_INFO")
            _set(p.buf[0], bsize=E["BLOCK_%dX%d" % (w, h)])
            rf = _get(p.buf[0], "ref_frame")
            rf[0], rf[1] = (E["LAST_FRAME"] if inter else E["INTRA_FRAME"]), E["NONE_FRAME"]
            return p
        cur = mbmi(sc["bw"], sc["bh"], 1)
        r0, c0 = sc["mi_row"], sc["mi_col"]
        for y in range(sc["bh"] // 4):
            for x in range(sc["bw"] // 4):
                grid[(r0 + y) * stride + c0 + x] = cur
        k = c0
        for (w, h, inter) in sc["above"]:
            p = mbmi(w, h, inter)
            for q in range(w // 4):
                grid[(r0 - 1) * stride + k + q] = p
            k += w // 4
        k = r0
        for (w, h, inter) in sc["left"]:
            p = mbmi(w, h, inter)
            for q in range(h // 4):
                grid[(k + q) * stride + c0 - 1] = p
            k += h // 4
        cm = tu.struct_obj("AV1_COMMON")
        seq = tu.struct_obj("SequenceHeader")
        _set(seq.buf[0], monochrome=int(sc["nplanes"] == 1))
        _set(cm.buf[0], seq_params=seq)
        _set(_get(cm.buf[0], "mi_params"), mi_rows=sc["mi_rows"], mi_cols=sc["mi_cols"])
        ybuf = tu.struct_obj("YV12_BUFFER_CONFIG")
        _set(ybuf.buf[0], flags=YV12_FLAG_HIGHBITDEPTH if hbd else 0)
        xd = tu.struct_obj("MACROBLOCKD")
        _set(xd.buf[0], mi=C.Pointer(grid, r0 * stride + c0, C.Ptr(mbt)), mi_stride=stride,
             mi_row=r0, mi_col=c0, width=sc["bw"] // 4, height=sc["bh"] // 4,
             up_available=sc["up"], left_available=sc["lf"], cur_buf=ybuf, bd=sc["bd"])
        return cm, xd

    def obmc(self, si, offs):
        """One scene: offs[plane] = (src_off, above_off, left_off).  Returns
        (bits, wsrc, mask, {plane: pred})."""
        tu, F = self.tu, self.F
        sc = R.OBMC_SCENES[si]
        hbd = sc["bd"] > 8
        et = "uint16_t" if hbd else "uint8_t"
        tag = (lambda p: tu.tagged(p)) if hbd else (lambda p: p)
        cm, xd = self.scene_objects(sc)
        bits = tu.buffer("uint32_t", [0, 0])
        tu.func("lavish_record_walk")(cm, xd, bits)
        bw, bh = sc["bw"], sc["bh"]
        planes = _get(xd.buf[0], "plane")
        dsts, aboves, lefts, strides = [], [], [], []
        for p in range(3):
            ss = int(p > 0)
            pl = min(p, sc["nplanes"] - 1, 1)
            row = [si, pl, int(pl > 0), int(pl > 0), 0, 0] + list(offs[pl]) + [0, 0]
            c = R.obmc_case(F, row)
            if p >= sc["nplanes"]:
                dsts.append(None)
                aboves.append(None)
                lefts.append(None)
                strides.append((0, 0, 0))
                continue
            st = (c.pw + 3, c.pw + 1, c.pw + 6)
            dsts.append(_embed(tu, et, c.src, st[0]))
            aboves.append(_embed(tu, et, c.above, st[1]))
            lefts.append(_embed(tu, et, c.left, st[2]))
            strides.append(st)
            _set(planes[p], subsampling_x=ss, subsampling_y=ss)
            _set(_get(planes[p], "dst"), buf=tag(dsts[p]), stride=st[0])
        # calc_target_weighted_pred: luma
        x = self.x
        wsrc, mask = tu.buffer("int32_t", [0] * (bw * bh)), tu.buffer("int32_t", [0] * (bw * bh))
        _set(_get(x.buf[0], "obmc_buffer"), wsrc=wsrc, mask=mask)
        _set(_get(_get(x.buf[0], "plane")[0], "src"), buf=tag(dsts[0]), stride=strides[0][0])
        tu.func("calc_target_weighted_pred")(cm, x, xd, tag(aboves[0]), strides[0][1],
                                             tag(lefts[0]), strides[0][2])
        ws = np.array(wsrc.buf, np.int64).reshape(bh, bw)
        mk = np.array(mask.buf, np.int64).reshape(bh, bw)
        # av1_build_obmc_inter_prediction: every plane of the scene, in place
        up = C.Ptr(C.UCHAR)
        tu.func(("lavish_hbd_" if hbd else "") + "av1_build_obmc_inter_prediction")(
            cm, xd, C.Pointer([tag(a) if a is not None else None for a in aboves], 0, up),
            tu.buffer("int", [s[1] for s in strides]),
            C.Pointer([tag(a) if a is not None else None for a in lefts], 0, up),
            tu.buffer("int", [s[2] for s in strides]))
        preds = {}
        for p in range(min(sc["nplanes"], 2)):
            pw, ph = bw >> int(p > 0), bh >> int(p > 0)
            preds[p] = np.array(dsts[p].buf, np.int64).reshape(ph, strides[p][0])[:, :pw]
        return (int(bits.buf[0]), int(bits.buf[1])), ws, mk, preds

    @property
    def x(self):
        if not hasattr(self, "_x"):
            self._x = self.tu.struct_obj("MACROBLOCK")
        return self._x


def obmc_offsets(si):
    """(src_off, above_off, left_off) of the scene's luma and chroma planes."""
    return [((si % 3) * R.A_STRIDE + (si * 5) % 3 + 7 * p,
             ((si + 1) % 3) * R.B_STRIDE + (si * 7) % 3 + 5 * p,
             ((si + 2) % 3) * R.B_STRIDE + (si * 3) % 5 + 11 + 9 * p) for p in range(2)]


def main():
    t0 = time.time()
    tu = tu_blend()
    F = make_inputs(tu)
    print("inputs %.0fs" % (time.time() - t0), flush=True)
    run = Runner(tu, F)
    rows, out = blend_rows(), []
    for i, row in enumerate(rows):
        row[-1] = sum(len(o) for o in out)
        out.append(run.blend(row).reshape(-1))
        if i % 50 == 0:
            print("  blend %d / %d  %.0fs" % (i, len(rows), time.time() - t0), flush=True)
    F["blend_cases"], F["blend_out"] = np.array(rows, np.int64), np.concatenate(out).astype(np.uint16)
    rows, out = diffwtd_rows(), []
    for row in rows:
        row[-1] = sum(len(o) for o in out)
        out.append(run.diffwtd(row).reshape(-1))
    F["dw_cases"], F["dw_out"] = np.array(rows, np.int64), np.concatenate(out).astype(np.uint8)
    print("  diffwtd %d  %.0fs" % (len(rows), time.time() - t0), flush=True)
    rows, out = wedge_rows(F), []
    for row in rows:
        r = run.wedge(row)
        if row[0] == 0:
            row[-1] = sum(len(o) for o in out)
            out.append(r)
        else:
            row[-1] = r
    F["wedge_cases"], F["wedge_out"] = np.array(rows, np.int64), np.concatenate(out).astype(np.int16)
    print("  wedge %d  %.0fs" % (len(rows), time.time() - t0), flush=True)
    rows, ws, mk, pr = [], [], [], []
    for si, sc in enumerate(R.OBMC_SCENES):
        offs = obmc_offsets(si)
        bits, w_, m_, preds = run.obmc(si, offs)
        for p, pred in sorted(preds.items()):
            rows.append([si, p, int(p > 0), int(p > 0), bits[0], bits[1]] + list(offs[p]) +
                        [sum(len(o) for o in ws) if p == 0 else -1, sum(len(o) for o in pr)])
            pr.append(pred.reshape(-1))
        ws.append(w_.reshape(-1))
        mk.append(m_.reshape(-1))
        print("  obmc %s  %.0fs" % (sc["name"], time.time() - t0), flush=True)
    F["obmc_cases"] = np.array(rows, np.int64)
    F["obmc_wsrc"], F["obmc_mask"] = (np.concatenate(v).astype(np.int32) for v in (ws, mk))
    F["obmc_pred"] = np.concatenate(pr).astype(np.uint16)
    bad = R.coverage_problems(F)
    if bad:
        raise SystemExit("fixture incomplete: %s" % bad)
    path = os.path.join(HERE, "fix_blend.npz")
    np.savez_compressed(path, **F)
    size = os.path.getsize(path)
    print("wrote %s: %d bytes" % (path, size))
    if size >= 1 << 20:
        raise SystemExit("fixture too large")


if __name__ == "__main__":
    main()
