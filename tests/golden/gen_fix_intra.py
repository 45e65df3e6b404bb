"""Golden fixture of the intra prediction layer, from the reference's own C
text executed by cinterp.py (as gen_fix_blend.py does).

  fix_intra.npz
    plane_bd{8,10,12}   one pixel plane per bit depth (_pix: one in eight near
                        an extreme), _intraref.PLANE_ROWS x PLANE_STRIDE; a
                        case's `plane` column 1 means the all-maximum plane
    cases, out          tests/_intraref.py I_COLS: the arguments of
                        build_intra_predictors[_high]; out the w x h blocks
    edge_bd{8,10,12}    1-D pixel streams the shim cases take above / left from
    shim_cases,         S_COLS: the per-call functions run directly
    shim_out
    tab_*               the reference's tables, read out of its globals:
                        smooth_weights, dr_intra_derivative,
                        av1_filter_intra_taps, mode_to_angle_map; the edge
                        kernels are av1_filter_intra_edge_c's response to a
                        unit impulse of 16 (the kernel is local to it)

Reference functions executed: init_intra_predictors_internal,
build_intra_predictors and build_intra_predictors_high whole (through the
pred / dc_pred function-pointer tables into the macro-generated predictors of
aom_dsp/intrapred.c), and directly every aom_[highbd_]{dc,dc_top,dc_left,
dc_128,v,h,paeth,smooth,smooth_v,smooth_h}_predictor_WxH_c, the six
av1_[highbd_]dr_prediction_z{1,2,3}_c, av1_filter_intra_predictor_c,
av1_filter_intra_edge[_high]_c and av1_upsample_intra_edge[_high]_c.

The generator stops unless _intraref.coverage_problems() is empty.  One of its
conditions, both edges upsampled in z2, cannot be met through
build_intra_predictors (the above edge is upsampled for p_angle < 130, the
left one for p_angle > 140); it is met by direct av1_dr_prediction_z2_c cases.

Usage: python tests/golden/gen_fix_intra.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cinterp as C  # noqa: E402
import _intraref as R  # noqa: E402
from gen_fixtures import ACMRandom, REF, TX_NAMES, _pix, check_errors  # noqa: E402

TX_W, TX_H = R.TX_W, R.TX_H
STRIDE = R.PLANE_STRIDE
ANGLE = [0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0]  # checked against tab_mode_to_angle
A_OFF, L_OFF = 300, 700


def tu_intra():
    tu = C.TU(REF, ["aom/aom_integer.h", "aom_ports/mem.h", "aom_dsp/aom_dsp_common.h",
                    "av1/common/enums.h", "av1/common/common_data.h", "av1/common/common_data.c",
                    "aom_dsp/intrapred.c", "av1/common/reconintra.c"], C.reference_defines(REF))
    need = ["build_intra_predictors", "build_intra_predictors_high",
            "init_intra_predictors_internal", "av1_filter_intra_predictor_c",
            "av1_filter_intra_edge_c", "av1_filter_intra_edge_high_c",
            "av1_upsample_intra_edge_c", "av1_upsample_intra_edge_high_c"]
    need += ["av1_%sdr_prediction_z%d_c" % (hb, z) for hb in ("", "highbd_") for z in (1, 2, 3)]
    need += ["aom_%s%s_predictor_%s_c" % (hb, t, s) for hb in ("", "highbd_")
             for t in R.PRED_TYPES for s in TX_NAMES]
    check_errors(tu, need)
    tu.func("init_intra_predictors_internal")()
    return tu


def flat(v):
    if isinstance(v, (list, tuple)):
        return [x for e in v for x in flat(e)]
    return [int(v)]


def tables(tu):
    F = {"tab_smooth_weights": np.array(flat(tu.global_value("smooth_weights")), np.int64),
         "tab_dr_intra_derivative": np.array(flat(tu.global_value("dr_intra_derivative")), np.int64),
         "tab_filter_intra_taps": np.array(flat(tu.global_value("av1_filter_intra_taps")),
                                           np.int64).reshape(5, 8, 8),
         "tab_mode_to_angle": np.array(flat(tu.global_value("mode_to_angle_map")), np.int64)}
    ker = []
    for strength in (1, 2, 3):
        p = tu.buffer("uint8_t", [0] * 4 + [16] + [0] * 4)
        tu.func("av1_filter_intra_edge_c")(p, 9, strength)
        ker.append([int(p.buf[6 - j]) for j in range(5)])  # p[i] = 16 * k[4 - i + 2] / 16
    F["tab_edge_kernel"] = np.array(ker, np.int64)
    assert list(F["tab_mode_to_angle"]) == ANGLE
    return F


# ------------------------------------------------------------------ cases --
def case_rows():
    rows, n = [], [0]

    def add(bd, tx, mode, ang=None, fi=5, dis=0, ft=0, counts=None, plane=0):
        i = n[0]
        n[0] += 1
        w, h = TX_W[tx], TX_H[tx]
        off = (1 + i % 3) * STRIDE + 1 + (i * 5) % 7
        if ang is None:
            ang = ANGLE[mode]
        dr = R.V_PRED <= mode <= R.D67_PRED and fi == 5
        if counts is None:  # everything available, as av1_predict_intra_block counts it
            counts = (w, w if dr and ang < 90 else -1, h, h if dr and ang > 180 else -1)
        rows.append([bd, plane, off, tx, mode, ang, fi, dis, ft] + list(counts) + [0])

    ND = (R.DC_PRED, R.SMOOTH_PRED, R.SMOOTH_V_PRED, R.SMOOTH_H_PRED, R.PAETH_PRED)
    DR = tuple(range(R.V_PRED, R.D67_PRED + 1))
    for tx in range(19):
        w, h = TX_W[tx], TX_H[tx]
        big = w * h > 1024
        for bd in (8, 10, 12):
            for mode in ND:
                add(bd, tx, mode, ft=(tx + mode) & 1)
        for k, mode in enumerate(DR):
            add((8, 8, 10, 8, 12)[(tx + k) % 5], tx, mode, ft=(tx + k) & 1)
        if w + h <= 32:
            for k, mode in enumerate(DR):
                for d in range(-3, 4):
                    bd = (8, 8, 10, 8, 8, 12)[(tx + k + d) % 6]
                    for dis, ft in ((0, 0), (0, 1), (1, 0)):
                        if d == 0 and (dis, ft) == (0, (tx + k) & 1):
                            continue  # the delta-0 case above
                        add(bd, tx, mode, ANGLE[mode] + 3 * d, dis=dis, ft=ft)
        # count patterns
        bd = (8, 10, 8, 12)[tx % 4]
        heavy = (R.D135_PRED, R.PAETH_PRED, R.SMOOTH_PRED)
        some = (heavy[tx % 3],) if big else heavy
        cut = (max(1, w // 2), -1, max(1, h // 2), -1)
        for mode in (R.DC_PRED,) + some:
            for counts in ((0, -1, 0, -1), (w, -1, 0, -1), (0, -1, h, -1), cut,
                           (w, -1, max(1, h - 3), -1), (max(1, w - 3), -1, h, -1)):
                add(bd, tx, mode, ft=tx & 1, counts=counts)
        for mode, ang in ((R.V_PRED, 90), (R.H_PRED, 180), (R.D45_PRED, 45 + 3 * (tx % 4)),
                          (R.D203_PRED, 203 - 3 * (tx % 3))):
            for counts in ((0, -1, 0, -1), (w, -1, 0, -1), (0, -1, h, -1)) + \
                    (() if big else (cut,)):
                add(8 if big else bd, tx, mode, ang, ft=tx & 1, counts=counts)
        for k, ntr in enumerate((-1, 0, max(1, w // 2), w)):
            add(8 if big else (8, 10, 12, 8)[k], tx, (R.D45_PRED, R.D67_PRED)[k & 1],
                (45, 67)[k & 1] + 3 * ((tx + k) % 7 - 3), ft=k & 1, counts=(w, ntr, h, -1))
            add(8 if big else (10, 8, 8, 12)[k], tx, R.D203_PRED, 203 + 3 * ((tx + k) % 7 - 3),
                ft=(k >> 1) & 1, counts=(w, -1, h, (-1, 0, max(1, h // 2), h)[k]))
        if w <= 32 and h <= 32:
            for fi in range(5):
                add((8, 10, 12)[(tx + fi) % 3], tx, R.DC_PRED, 0, fi=fi)
            add(8, tx, R.DC_PRED, 0, fi=tx % 5, counts=(0, -1, 0, -1))
            add(10, tx, R.DC_PRED, 0, fi=(tx + 1) % 5, counts=(max(1, w // 2), -1, h, -1))
            add(8, tx, R.DC_PRED, 0, fi=(tx + 2) % 5, counts=(w, -1, 0, -1))
    # the all-maximum plane
    for bd in (8, 10, 12):
        for tx, mode, ang, fi in ((4, R.SMOOTH_PRED, 0, 5), (2, R.D135_PRED, 138, 5),
                                  (0, R.D45_PRED, 48, 5), (1, R.D113_PRED, 116, 5),
                                  (3, R.PAETH_PRED, 0, 5), (9, R.DC_PRED, 0, 5),
                                  (13, R.DC_PRED, 0, 5), (1, R.DC_PRED, 0, 0),
                                  (2, R.DC_PRED, 0, 3), (6, R.DC_PRED, 0, 4),
                                  (8, R.D203_PRED, 212, 5)):
            add(bd, tx, mode, ang, fi=fi, plane=1)
    return rows


def shim_rows():
    rows = []

    def add(kind, bd, w, h, p0=0, p1=0, p2=0):
        i = len(rows)
        rows.append([kind, bd, w, h, A_OFF + i % 5, L_OFF + (i * 3) % 7, p0, p1, p2, 0])

    for tx in range(19):
        for k in range(10):
            add(k, 8, TX_W[tx], TX_H[tx], 0)
            add(k, (10, 12)[(tx + k) & 1], TX_W[tx], TX_H[tx], 1)
    zs = [(4, 4), (8, 8), (16, 16), (4, 16), (16, 4), (8, 4), (32, 8), (8, 32), (64, 16), (64, 64)]
    for i, (w, h) in enumerate(zs):
        for bd in (8, (10, 12)[i & 1]):
            small = w + h <= 16
            for ua in (0, 1) if small else (0,):
                add(R.K_Z1, bd, w, h, ua, 0, (3, 36, 45, 58, 87, 14, 67)[(i + ua) % 7])
                add(R.K_Z3, bd, w, h, 0, ua, (183, 216, 225, 267, 203, 194)[(i + ua) % 6])
                for ul in (0, 1) if small else (0,):
                    add(R.K_Z2, bd, w, h, ua, ul, (93, 113, 135, 157, 177, 122, 148)[(i + ua + 2 * ul) % 7])
    for tx in range(19):
        if TX_W[tx] <= 32 and TX_H[tx] <= 32:
            for m in ((tx % 5, (tx + 2) % 5) if TX_W[tx] * TX_H[tx] > 256 else range(5)):
                add(R.K_FILTER_INTRA, 8, TX_W[tx], TX_H[tx], m)
    for sz in (2, 5, 9, 13, 17, 25, 33, 49, 65, 81, 129):
        for strength in (0, 1, 2, 3):
            add(R.K_FILTER_EDGE, 8, sz, 1, strength)
            add(R.K_FILTER_EDGE, (10, 12)[strength & 1], sz, 1, strength)
    for sz in (4, 8, 12, 16):
        for bd in (8, 10, 12):
            add(R.K_UPSAMPLE, bd, sz, 1)
    return rows


# ---------------------------------------------------------------- runners --
class Runner:
    def __init__(self, tu, F):
        self.tu, self.F = tu, F
        self.planes = {}

    def plane(self, bd, which):
        if (bd, which) not in self.planes:
            self.planes[(bd, which)] = R.plane_of(self.F, bd, which).tolist()
        return self.planes[(bd, which)]

    def case(self, row):
        tu = self.tu
        c = R.intra_case(self.F, row)
        hb = c.bd > 8
        et = "uint16_t" if hb else "uint8_t"
        ref = tu.buffer(et, self.plane(c.bd, c.plane))
        ds = c.w + 3
        dst = tu.buffer(et, [0] * (c.h * ds))
        r = C.Pointer(ref.buf, c.ref_off, ref.ty)
        tag = (lambda p: tu.tagged(p)) if hb else (lambda p: p)
        args = [tag(r), STRIDE, tag(dst), ds, c.mode, c.p_angle, c.fi_mode, c.tx_size,
                c.disable_edge_filter, c.n_top, c.n_topright, c.n_left, c.n_bottomleft,
                c.filter_type]
        if hb:
            tu.func("build_intra_predictors_high")(*(args + [c.bd]))
        else:
            tu.func("build_intra_predictors")(*args)
        return np.array(dst.buf, np.int64).reshape(c.h, ds)[:, :c.w]

    def shim(self, row):
        tu = self.tu
        c = R.shim_case(self.F, row)
        hb = c.bd > 8
        et = "uint16_t" if hb else "uint8_t"
        pre = "highbd_" if hb else ""
        edge = tu.buffer(et, self.F["edge_bd%d" % c.bd].tolist())
        above = C.Pointer(edge.buf, c.a_off, edge.ty)
        left = C.Pointer(edge.buf, c.l_off, edge.ty)
        w, h, k = c.w, c.h, c.kind
        bd = [c.bd] if hb else []
        if k == R.K_FILTER_EDGE:
            tu.func("av1_filter_intra_edge%s_c" % ("_high" if hb else ""))(above, w, c.p0)
            return np.array(edge.buf[c.a_off:c.a_off + w], np.int64)
        if k == R.K_UPSAMPLE:
            tu.func("av1_upsample_intra_edge%s_c" % ("_high" if hb else ""))(*([above, w] + bd))
            return np.array(edge.buf[c.a_off - 2:c.a_off + 2 * w - 1], np.int64)
        ds = w + 5
        dst = tu.buffer(et, [0] * (h * ds))
        if k < 10:
            tu.func("aom_%s%s_predictor_%dx%d_c" % (pre, R.PRED_TYPES[k], w, h))(
                *([dst, ds, above, left] + bd))
        elif k == R.K_FILTER_INTRA:
            tx = [i for i in range(19) if (TX_W[i], TX_H[i]) == (w, h)][0]
            tu.func("av1_filter_intra_predictor_c")(dst, ds, tx, above, left, c.p0)
        else:
            dx, dy = R.get_dx_dy(c.p2)
            z = k - R.K_Z1 + 1
            ups = [c.p0] if z == 1 else [c.p1] if z == 3 else [c.p0, c.p1]
            tu.func("av1_%sdr_prediction_z%d_c" % (pre, z))(
                *([dst, ds, w, h, above, left] + ups + [dx, dy] + bd))
        return np.array(dst.buf, np.int64).reshape(h, ds)[:, :w].reshape(-1)


def main():
    t0 = time.time()
    tu = tu_intra()
    F = tables(tu)
    rnd = ACMRandom(0xbaba + 61)
    for bd in (8, 10, 12):
        F["plane_bd%d" % bd] = np.array(_pix(rnd, R.PLANE_ROWS * STRIDE, bd),
                                        np.uint16).reshape(R.PLANE_ROWS, STRIDE)
        F["edge_bd%d" % bd] = np.array(_pix(rnd, R.EDGE_LEN, bd), np.uint16)
    run = Runner(tu, F)
    rows, out, pos = case_rows(), [], 0
    for i, row in enumerate(rows):
        row[-1] = pos
        o = run.case(row).reshape(-1)
        out.append(o)
        pos += len(o)
        if i % 500 == 0:
            print("  case %d / %d  %.0fs" % (i, len(rows), time.time() - t0), flush=True)
    F["cases"], F["out"] = np.array(rows, np.int64), np.concatenate(out).astype(np.uint16)
    rows, out, pos = shim_rows(), [], 0
    for i, row in enumerate(rows):
        row[-1] = pos
        o = run.shim(row)
        assert len(o) == R.shim_out_len(R.shim_case(F, row))
        out.append(o)
        pos += len(o)
    F["shim_cases"], F["shim_out"] = np.array(rows, np.int64), np.concatenate(out).astype(np.uint16)
    print("  %d cases, %d shim cases  %.0fs" % (len(F["cases"]), len(rows), time.time() - t0),
          flush=True)
    bad = R.coverage_problems(F)
    if bad:
        raise SystemExit("fixture incomplete: %s" % bad)
    path = os.path.join(HERE, "fix_intra.npz")
    np.savez_compressed(path, **F)
    size = os.path.getsize(path)
    print("wrote %s: %d bytes" % (path, size))
    if size >= 1 << 20:
        raise SystemExit("fixture too large")


if __name__ == "__main__":
    main()
