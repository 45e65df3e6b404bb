#!/usr/bin/env python3
"""fix_qm.npz: the quantization-matrix paths of search_tx_type, produced by
executing the reference's own C text (tests/golden/cinterp.py), like
gen_fixtures.py.

Executed from the reference:
  av1_qm_init (av1/common/quant_common.c:283-309) -> the level tables and
    the per-size offsets; aom_get_qmlevel (quant_common.h:57-59);
  av1_set_qmatrix (av1/encoder/av1_quantize.c:758-777) and av1_setup_qmatrix
    (encodemb.c:374-380), so the (qmatrix, iqmatrix) a row runs with are the
    reference's own choice, NULL for level 15 and for tx_type >= IDTX;
  av1_quant (encodemb.c:308-341) with FP / B / DC -> the facades of
    av1_quantize.c:266-563 and through them quantize_fp_helper_c,
    highbd_quantize_fp_helper_c, aom_[highbd_]quantize_b_helper_c, quantize_dc
    and highbd_quantize_dc ("q_*" arrays);
  the four helpers called directly, with both matrices, qm only and iqm only
    ("h_*" arrays; aom_quantize_b_helper_c is form 1, hbd 0);
  dist_block_tx_domain (tx_search.c:1073-1116) with use_qm_dist_metric 0 and
    1, and av1_block_error_qm (:1049-1071) on the same buffers;
  av1_optimize_b (encodemb.c:87-103) with using_qmatrix and dist_metric
    AOM_DIST_METRIC_PSNR / AOM_DIST_METRIC_QM_PSNR ("t_*" arrays).

Coefficient blocks: fix_txfm.npz outputs at several scales, the all-maximum
block of the depth, a DC-only block and a block of zeros.  Blocks of n
coefficients are stored back to back; a row's "index" is its element offset.

The |abs_qcoeff * dequant| > 2^31 wrap: no quantizer av1_build_quantizer
makes reaches it.  With a matrix the level is about |coeff| * wt / (32 *
dequant) and the weighted dequantizer about dequant * iwt / 32, so the
product stays near |coeff| * wt * iwt / 1024 < 2^26 for every depth (the
generator asserts that no stored row wraps).  tests/test_gpu_qm.py covers the
wrap with free int16 parameters against tests/_qmref.py.

The generator stops unless the conditions listed in check_conditions() hold.

Usage: python tests/golden/gen_fix_qm.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_fixtures as G  # noqa: E402

C = G.C
_get, _set = G._get, G._set

LEVELS = (0, 7, 14)
QM_TOTAL = 3344
SIZES = (0, 1, 14, 3, 4, 18)      # 4x4 8x8 16x4 32x32 64x64 64x16
TYPES16 = (0, 3, 9, 10, 11, 6)    # 2-D, 2-D, IDTX, V_DCT (vert), H_DCT (horiz), 2-D
QINDEX = (0, 120, 255, 0)
QMLEVEL_ARGS = ((5, 9), (0, 15), (9, 9))
FP, B, DC = 0, 1, 2
KINDS = ("decay", "txfm", "decay", "max", "decay", "decay", "dc", "txfm", "decay", "zero", "decay")

Q_FIELDS = ["bd", "tx_size", "tx_type", "qindex", "plane", "level", "mode", "force", "qm_set",
            "iqm_set", "eob", "eob_flat", "dist1", "sse1", "dist2", "sse2", "err_qm", "ssz_qm",
            "n", "index"]
H_FIELDS = ["form", "hbd", "bd", "tx_size", "tx_type", "qindex", "plane", "level", "log_scale",
            "qm_set", "iqm_set", "eob", "eob_flat", "n", "index"]
T_FIELDS = ["bd", "tx_size", "tx_type", "qindex", "plane", "is_inter", "sharpness", "rdmult",
            "level", "txb_skip_ctx", "dc_sign_ctx", "tx_type_cost", "eob_in", "qm_set", "iqm_set",
            "eob0", "rate0", "entropy0", "eob1", "rate1", "entropy1", "differs_flat_iqm", "n",
            "index"]


def types_of(s):
    m = max(G.TX_W[s], G.TX_H[s])
    return (0,) if m == 64 else ((0, 9) if m == 32 else TYPES16)


def coeff_block(txfm_fix, rnd, s, t, bd, kind, scales=(1, 4, 16, 64), deq=0):
    """kind "txfm": a fix_txfm output divided by one of `scales`; "decay": one
    rescaled to fall linearly from 4 * deq >> log_scale at DC (deq: the AC
    dequantizer of the row) to nothing along the anti-diagonals, so the eob lands inside
    the block where the matrix weights move it; "dc": only DC kept; "max":
    +-(2^(bd + 7) - 1) everywhere; "zero"."""
    n = G.max_eob(s)
    lim = 1 << (bd + 7)
    if kind == "max":
        return np.full(n, lim - 1, np.int64) * np.where(np.arange(n) % 3 == 1, -1, 1)
    if kind == "zero":
        return np.zeros(n, np.int64)
    src = txfm_fix["out_%d_%d" % (s, t)]
    b = rnd.generate(len(src))
    scale = scales[rnd.generate(len(scales))]
    c = np.clip(src[b].astype(np.int64)[:n] // scale << (bd - 8), -lim, lim - 1)
    if kind == "decay":
        w, h = min(G.TX_W[s], 32), min(G.TX_H[s], 32)
        i = np.arange(n)
        ls = (G.TX_W[s] * G.TX_H[s] > 256) + (G.TX_W[s] * G.TX_H[s] > 1024)
        c = np.clip(c * (4 * deq >> ls) * (w + h - 1 - i // h - i % h) //
                    (max(1, int(np.abs(c).max())) * (w + h - 1)), -lim, lim - 1)
    if kind == "dc":
        c[1:] = 0
        if c[0] == 0:
            c[0] = -(lim >> 3)
    return c


class Ref:
    """The reference's state for one run: AV1_COMP with av1_qm_init's
    pointers, a MACROBLOCK, per-depth quantizer tables and cost tables."""

    def __init__(self):
        tu = C.TU(G.REF, ["av1/encoder/encoder.h", "av1/encoder/txb_rdopt.c",
                          "av1/encoder/tx_search.c", "av1/encoder/encodetxb.c",
                          "av1/common/txb_common.c", "av1/common/scan.c",
                          "av1/encoder/encodemb.c", "av1/encoder/av1_quantize.c",
                          "aom_dsp/quantize.c", "av1/common/quant_common.c",
                          "av1/common/idct.c", "av1/encoder/rdopt.c"],
                 C.reference_defines(G.REF))
        G.check_errors(tu, ["av1_qm_init", "av1_set_qmatrix", "av1_setup_qmatrix", "av1_quant",
                            "av1_setup_quant", "av1_build_quantizer", "quantize_fp_helper_c",
                            "highbd_quantize_fp_helper_c", "aom_quantize_b_helper_c",
                            "aom_highbd_quantize_b_helper_c", "dist_block_tx_domain",
                            "av1_block_error_qm", "av1_optimize_b", "aom_get_qmlevel"])
        self.tu, self.E = tu, tu.enums
        self.cpi = tu.struct_obj("AV1_COMP")
        CP = self.cpi.buf[0]
        _get(CP, "optimize_seg_arr")[0] = 1
        cm = _get(CP, "common")
        self.qparams = _get(cm, "quant_params")
        self.qpp = C.Pointer(cm.vals, cm.st.index["quant_params"], tu.ctype("CommonQuantParams"))
        tu.func("av1_qm_init")(self.qpp, 3)
        self.x = tu.struct_obj("MACROBLOCK")
        X = self.X = self.x.buf[0]
        self.xd = _get(X, "e_mbd")
        self.xd_p = C.Pointer(X.vals, X.st.index["e_mbd"], tu.ctype("MACROBLOCKD"))
        self.mbmi = tu.struct_obj("MB_MODE_INFO")
        _set(self.xd, mi=tu.buffer("MB_MODE_INFO *", [self.mbmi]))
        self.cur_buf = tu.struct_obj("YV12_BUFFER_CONFIG")
        _set(self.xd, cur_buf=self.cur_buf)
        self.quant = {}
        self.wt = np.array(tu.global_value("wt_matrix_ref"), np.uint8).reshape(15, 2, QM_TOTAL)
        self.iwt = np.array(tu.global_value("iwt_matrix_ref"), np.uint8).reshape(15, 2, QM_TOTAL)

    # -- tables ------------------------------------------------------------
    def table_offsets(self):
        """Element offset of gqmatrix[0][0][t] inside its level table."""
        g = _get(self.qparams, "gqmatrix")
        return np.array([g[t].off for t in range(19)], np.int32)

    def qmlevels(self):
        fn = self.tu.func("aom_get_qmlevel")
        return np.array([[fn(q, a, b) for q in range(256)] for a, b in QMLEVEL_ARGS], np.int32)

    def global_qm(self, level, plane, s):
        if level == 15:
            return None, None
        i = (level * 3 + plane) * 19 + s
        return _get(self.qparams, "gqmatrix")[i], _get(self.qparams, "giqmatrix")[i]

    def scan(self, s, t):
        so = self.tu.global_value("av1_scan_orders")
        e = so[s * 16 + t]
        return e.vals[e.st.index["scan"]], e.vals[e.st.index["iscan"]]

    def scan_np(self, s, t):
        sp = self.scan(s, t)[0]
        return np.array(sp.buf[sp.off:sp.off + G.max_eob(s)], np.int64)

    def qtab(self):
        """[bd 8 / 10 / 12][qindex][zbin, round_fp, quant_fp, round, quant,
        quant_shift, dequant][DC, AC] of av1_build_quantizer's y rows."""
        out = np.zeros((3, 256, 7, 2), np.int16)
        for i, bd in enumerate((8, 10, 12)):
            Q, D = self.tables(bd)
            for j, nm in enumerate(("y_zbin", "y_round_fp", "y_quant_fp", "y_round", "y_quant",
                                    "y_quant_shift", "y_dequant_QTX")):
                src = _get(D, nm) if nm == "y_dequant_QTX" else _get(Q, nm)
                out[i, :, j, :] = np.array(src, np.int64).reshape(256, 8)[:, :2]
        return out

    def tables(self, bd):
        if bd not in self.quant:
            quants = self.tu.struct_obj("QUANTS")
            deq = self.tu.struct_obj("Dequants")
            self.tu.func("av1_build_quantizer")(bd, 0, 0, 0, 0, 0, quants, deq, 0)
            self.quant[bd] = (quants.buf[0], deq.buf[0])
        return self.quant[bd]

    def dequant_ac(self, bd, qindex):
        return int(_get(self.tables(bd)[1], "y_dequant_QTX")[8 * qindex + 1])

    def qrow(self, bd, qindex, name):
        Q, D = self.tables(bd)
        src = _get(D, name) if name == "y_dequant_QTX" else _get(Q, name)
        return C.Pointer(src, 8 * qindex, self.tu.ctype("int16_t"))

    # -- block state ---------------------------------------------------------
    def setup_block(self, bd, s, plane, qindex, level, c, inter=1):
        tu = self.tu
        n = G.max_eob(s)
        p0 = _get(self.X, "plane")[plane]
        for fld, nm in (("quant_fp_QTX", "y_quant_fp"), ("round_fp_QTX", "y_round_fp"),
                        ("quant_QTX", "y_quant"), ("quant_shift_QTX", "y_quant_shift"),
                        ("zbin_QTX", "y_zbin"), ("round_QTX", "y_round"),
                        ("dequant_QTX", "y_dequant_QTX")):
            _set(p0, **{fld: self.qrow(bd, qindex, nm)})
        self.cb = tu.buffer("tran_low_t", [int(v) for v in c])
        self.qb, self.db = tu.buffer("tran_low_t", n), tu.buffer("tran_low_t", n)
        self.eb = tu.buffer("uint16_t", 1)
        self.ec = tu.buffer("uint8_t", 1)
        _set(p0, coeff=self.cb, qcoeff=self.qb, dqcoeff=self.db, eobs=self.eb,
             txb_entropy_ctx=self.ec)
        _set(self.xd, bd=bd)
        _set(self.cur_buf.buf[0], flags=8 if bd > 8 else 0)  # YV12_FLAG_HIGHBITDEPTH
        _set(self.X, seg_skip_block=0)
        M = self.mbmi.buf[0]
        _get(M, "ref_frame")[0] = self.E["LAST_FRAME"] if inter else self.E["INTRA_FRAME"]
        _set(M, mode=self.E["DC_PRED"], segment_id=0)
        _set(self.qparams, using_qmatrix=1, qmatrix_level_y=level, qmatrix_level_u=level,
             qmatrix_level_v=level)
        tu.func("av1_set_qmatrix")(self.qpp, 0, self.xd_p)

    def quant_param(self, s, t, plane, mode, use_optimize_b=0):
        qp = self.tu.struct_obj("QUANT_PARAM")
        idx = {FP: "AV1_XFORM_QUANT_FP", B: "AV1_XFORM_QUANT_B", DC: "AV1_XFORM_QUANT_DC"}[mode]
        self.tu.func("av1_setup_quant")(s, use_optimize_b, self.E[idx], 0, qp)
        if self.tu.func("av1_use_qmatrix")(self.qpp, self.xd_p, 0):
            self.tu.func("av1_setup_qmatrix")(self.qpp, self.xd_p, plane, s, t, qp)
        return qp

    def run_quant(self, bd, s, t, plane, qp):
        tp = self.tu.struct_obj("TxfmParam")
        _set(tp.buf[0], tx_type=t, tx_size=s, is_hbd=int(bd > 8), bd=bd)
        self.tu.func("av1_quant")(self.x, plane, 0, tp, qp)
        return (np.array(self.qb.buf, np.int32), np.array(self.db.buf, np.int32),
                int(self.eb.buf[0]))

    # -- rows ------------------------------------------------------------------
    def facade_row(self, bd, s, t, qindex, plane, level, mode, force, c):
        """av1_quant with the reference's matrices (force 1: iqmatrix set to
        NULL afterwards, 2: qmatrix), then dist_block_tx_domain both ways."""
        tu = self.tu
        self.setup_block(bd, s, plane, qindex, level, c)
        qp = self.quant_param(s, t, plane, mode)
        P = qp.buf[0]
        if force == 1:
            _set(P, iqmatrix=None)
        elif force == 2:
            _set(P, qmatrix=None)
        qm, iqm = _get(P, "qmatrix"), _get(P, "iqmatrix")
        q, dq, eob = self.run_quant(bd, s, t, plane, qp)
        n = G.max_eob(s)
        scan, _ = self.scan(s, t)
        out = {"qcoeff": q, "dqcoeff": dq, "eob": eob, "qm_set": int(qm is not None),
               "iqm_set": int(iqm is not None)}
        tsp = _get(self.X, "txfm_search_params")
        for metric in (0, 1):
            _set(tsp, use_qm_dist_metric=metric)
            d, e = tu.buffer("int64_t", 1), tu.buffer("int64_t", 1)
            tu.func("dist_block_tx_domain")(self.x, plane, 0, s, qm, scan, d, e)
            out["dist%d" % (metric + 1)], out["sse%d" % (metric + 1)] = d.buf[0], e.buf[0]
        out["err_qm"] = out["ssz_qm"] = 0
        if qm is not None:
            e = tu.buffer("int64_t", 1)
            out["err_qm"] = tu.func("av1_block_error_qm")(self.cb, self.db, n, qm, scan, e)
            out["ssz_qm"] = e.buf[0]
        # the same row with flat matrices, for the generator's conditions
        _set(P, qmatrix=None, iqmatrix=None)
        out["eob_flat"] = self.run_quant(bd, s, t, plane, qp)[2]
        return out

    HELPERS = {(0, 0): "quantize_fp_helper_c", (0, 1): "highbd_quantize_fp_helper_c",
               (1, 0): "aom_quantize_b_helper_c", (1, 1): "aom_highbd_quantize_b_helper_c"}

    def helper_row(self, form, bd, s, t, qindex, plane, level, use_qm, use_iqm, c):
        tu = self.tu
        n = G.max_eob(s)
        ls = (G.TX_W[s] * G.TX_H[s] > 256) + (G.TX_W[s] * G.TX_H[s] > 1024)
        scan, iscan = self.scan(s, t)
        gq, giq = self.global_qm(level, plane, s)
        fn = tu.func(self.HELPERS[(form, int(bd > 8))])
        rnd, qnt = ("y_round_fp", "y_quant_fp") if form == 0 else ("y_round", "y_quant")
        res = []
        for qm, iqm in ((gq if use_qm else None, giq if use_iqm else None), (None, None)):
            cb = tu.buffer("tran_low_t", [int(v) for v in c])
            qb, db = tu.buffer("tran_low_t", [77] * n), tu.buffer("tran_low_t", [77] * n)
            eb = tu.buffer("uint16_t", 1)
            fn(cb, n, self.qrow(bd, qindex, "y_zbin"), self.qrow(bd, qindex, rnd),
               self.qrow(bd, qindex, qnt), self.qrow(bd, qindex, "y_quant_shift"), qb, db,
               self.qrow(bd, qindex, "y_dequant_QTX"), eb, scan, iscan, qm, iqm, ls)
            res.append((np.array(qb.buf, np.int32), np.array(db.buf, np.int32), int(eb.buf[0])))
        return {"qcoeff": res[0][0], "dqcoeff": res[0][1], "eob": res[0][2],
                "eob_flat": res[1][2], "log_scale": ls}

    def set_costs(self, cc_tabs, eob_tabs, itx, atx):
        ccs = _get(self.X, "coeff_costs")
        k = 0
        for obj in _get(ccs, "coeff_costs"):
            for fld in ("txb_skip_cost", "base_eob_cost", "base_cost", "eob_extra_cost",
                        "dc_sign_cost", "lps_cost"):
                cell = _get(obj, fld)
                cell[:] = [int(v) for v in cc_tabs[k:k + len(cell)]]
                k += len(cell)
        k = 0
        for obj in _get(ccs, "eob_costs"):
            cell = _get(obj, "eob_cost")
            cell[:] = [int(v) for v in eob_tabs[k:k + len(cell)]]
            k += len(cell)
        mc = _get(self.X, "mode_costs")
        _get(mc, "inter_tx_type_costs")[:] = [int(v) for v in itx]
        _get(mc, "intra_tx_type_costs")[:] = [int(v) for v in atx]

    def trellis_row(self, bd, s, t, qindex, plane, inter, sharp, rdmult, level, skip_ctx, dc_ctx,
                    c):
        """av1_quant (FP, with the matrices) then av1_optimize_b three times on
        that output: metric PSNR, metric QM_PSNR, and PSNR with a flat
        iqmatrix (only for the generator's conditions)."""
        tu = self.tu
        self.setup_block(bd, s, plane, qindex, level, c, inter)
        _set(self.X, rdmult=rdmult)
        oxcf = _get(self.cpi.buf[0], "oxcf")
        _set(_get(oxcf, "algo_cfg"), sharpness=sharp)
        qp = self.quant_param(s, t, plane, FP, 1)
        P = qp.buf[0]
        out = {"qm_set": int(_get(P, "qmatrix") is not None),
               "iqm_set": int(_get(P, "iqmatrix") is not None)}
        q_in, dq_in, eob_in = self.run_quant(bd, s, t, plane, qp)
        out.update(qcoeff_in=q_in, dqcoeff_in=dq_in, eob_in=eob_in)
        out["tx_type_cost"] = tu.func("get_tx_type_cost")(self.x, self.xd_p, plane, s, t, 0)
        pd = _get(self.xd, "plane")[plane]
        adj = tu.func("av1_get_adjusted_tx_size")(s)
        seg_iqm = _get(pd, "seg_iqmatrix")
        runs = {}
        for key, metric, flat in ((0, "AOM_DIST_METRIC_PSNR", 0), (1, "AOM_DIST_METRIC_QM_PSNR", 0),
                                  ("flat", "AOM_DIST_METRIC_PSNR", 1)):
            self.qb.buf[:] = [int(v) for v in q_in]
            self.db.buf[:] = [int(v) for v in dq_in]
            self.eb.buf[0] = eob_in
            self.ec.buf[0] = 0
            _set(_get(oxcf, "tune_cfg"), dist_metric=self.E[metric])
            keep = seg_iqm[adj]
            if flat:
                seg_iqm[adj] = None
            ctx = tu.struct_obj("TXB_CTX")
            _set(ctx.buf[0], txb_skip_ctx=skip_ctx, dc_sign_ctx=dc_ctx)
            rate = tu.buffer("int", 1)
            eob = tu.func("av1_optimize_b")(self.cpi, self.x, plane, 0, s, t, ctx, rate)
            seg_iqm[adj] = keep
            runs[key] = (np.array(self.qb.buf, np.int32), np.array(self.db.buf, np.int32),
                         int(eob), int(rate.buf[0]), int(self.ec.buf[0]))
        for m in (0, 1):
            out["qcoeff%d" % m], out["dqcoeff%d" % m] = runs[m][0], runs[m][1]
            out["eob%d" % m], out["rate%d" % m], out["entropy%d" % m] = runs[m][2:]
        out["differs_flat_iqm"] = int(runs[0][2:4] != runs["flat"][2:4] or
                                      not np.array_equal(runs[0][0], runs["flat"][0]))
        return out


def trellis_tables(rnd):
    cc = np.array([rnd.generate(4000) for _ in range(10 * G.CC_COEFF_COST)], np.int32)
    eo = np.array([rnd.generate(4000) for _ in range(14 * G.CC_EOB_COST)], np.int32)
    return cc, eo


def gen_facade(ref, txfm_fix):
    rnd = G.ACMRandom(0xbaba + 31)
    rows, arrs = [], {"coeff": [], "qcoeff": [], "dqcoeff": []}
    k = off = 0
    for bd in (8, 10, 12):
        for s in SIZES:
            n = G.max_eob(s)
            for t in types_of(s):
                for mode in (FP, B, DC):
                    for qindex in (0, 120, 255):
                        kind = KINDS[k % len(KINDS)]
                        plane = (k // 2) % 2
                        level = 15 if k % 16 == 9 else LEVELS[k % 3]
                        force = (0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 2, 0, 0)[k % 13]
                        k += 1
                        c = coeff_block(txfm_fix, rnd, s, t, bd, kind, deq=ref.dequant_ac(bd, qindex))
                        o = ref.facade_row(bd, s, t, qindex, plane, level, mode, force, c)
                        rows.append([bd, s, t, qindex, plane, level, mode, force, o["qm_set"],
                                     o["iqm_set"], o["eob"], o["eob_flat"], o["dist1"], o["sse1"],
                                     o["dist2"], o["sse2"], o["err_qm"], o["ssz_qm"], n, off])
                        arrs["coeff"].append(np.asarray(c, np.int32))
                        arrs["qcoeff"].append(o["qcoeff"])
                        arrs["dqcoeff"].append(o["dqcoeff"])
                        off += n
            print("  facade bd %d size %d: %d rows" % (bd, s, len(rows)), flush=True)
    out = {"q_rows": np.array(rows, np.int64), "q_fields": np.array(Q_FIELDS)}
    for kk, v in arrs.items():
        out["q_" + kk] = np.concatenate(v)
    return out


def gen_helpers(ref, txfm_fix):
    rnd = G.ACMRandom(0xbaba + 32)
    rows, arrs = [], {"coeff": [], "qcoeff": [], "dqcoeff": []}
    k = off = 0
    for form in (0, 1):
        for bd in (8, 10, 12):
            for s in SIZES:
                n = G.max_eob(s)
                ty = types_of(s)
                for j in range(6):
                    t = ty[j % len(ty)]
                    use_qm, use_iqm = ((1, 1), (1, 1), (1, 0), (1, 1), (0, 1), (1, 1))[j]
                    qindex = QINDEX[k % 4]
                    # the rows that cannot move the eob share one slot each: the
                    # special blocks go with qm only, the near-flat level 14
                    # with iqm only
                    kind = ("max", "dc", "zero")[(k // 6) % 3] if j == 2 else "decay"
                    plane = (k // 3) % 2
                    level = 14 if j == 4 else LEVELS[k % 2]
                    k += 1
                    c = coeff_block(txfm_fix, rnd, s, t, bd, kind, (4, 16, 64),
                                    ref.dequant_ac(bd, qindex))
                    o = ref.helper_row(form, bd, s, t, qindex, plane, level, use_qm, use_iqm, c)
                    rows.append([form, int(bd > 8), bd, s, t, qindex, plane, level,
                                 o["log_scale"], use_qm, use_iqm, o["eob"], o["eob_flat"], n, off])
                    arrs["coeff"].append(np.asarray(c, np.int32))
                    arrs["qcoeff"].append(o["qcoeff"])
                    arrs["dqcoeff"].append(o["dqcoeff"])
                    off += n
            print("  helpers form %d bd %d: %d rows" % (form, bd, len(rows)), flush=True)
    out = {"h_rows": np.array(rows, np.int64), "h_fields": np.array(H_FIELDS)}
    for kk, v in arrs.items():
        out["h_" + kk] = np.concatenate(v)
    return out


def trellis_cases():
    """(bd, s, t, plane, inter) of every trellis configuration."""
    cases = []
    for bd in (8, 10, 12):
        for s in SIZES:
            for t in types_of(s):
                for plane, inter in ((0, 1), (0, 0), (1, 1)):
                    if bd == 12 and (plane, inter) != (0, 1):
                        continue
                    cases.append((bd, s, t, plane, inter))
    return cases


def gen_trellis(ref, txfm_fix):
    rnd = G.ACMRandom(0xbaba + 33)
    cc, eo = trellis_tables(rnd)
    itx = [rnd.generate(3000) for _ in range(len(_get(_get(ref.X, "mode_costs"),
                                                      "inter_tx_type_costs")))]
    atx = [rnd.generate(3000) for _ in range(len(_get(_get(ref.X, "mode_costs"),
                                                      "intra_tx_type_costs")))]
    ref.set_costs(cc, eo, itx, atx)
    names = ("coeff", "qcoeff_in", "dqcoeff_in", "qcoeff0", "dqcoeff0", "qcoeff1", "dqcoeff1")
    rows, arrs = [], {k: [] for k in names}
    k = off = 0
    for bd, s, t, plane, inter in trellis_cases():
        n = G.max_eob(s)
        qindex = (60, 120, 200, 255)[k % 4]
        level = LEVELS[k % 3]
        sharp = (k // 2) % 2
        rdmult = 20000 + rnd.generate(400000)
        k += 1
        for kind in ("txfm", "decay"):  # two blocks per configuration: one batch on the device
            c = coeff_block(txfm_fix, rnd, s, t, bd, kind, (1, 2, 4, 16),
                            4 * ref.dequant_ac(bd, qindex))
            skip_ctx, dc_ctx = rnd.generate(13), rnd.generate(3)
            o = ref.trellis_row(bd, s, t, qindex, plane, inter, sharp, rdmult, level, skip_ctx,
                                dc_ctx, c)
            rows.append([bd, s, t, qindex, plane, inter, sharp, rdmult, level, skip_ctx, dc_ctx,
                         o["tx_type_cost"], o["eob_in"], o["qm_set"], o["iqm_set"], o["eob0"],
                         o["rate0"], o["entropy0"], o["eob1"], o["rate1"], o["entropy1"],
                         o["differs_flat_iqm"], n, off])
            o["coeff"] = np.asarray(c, np.int32)
            for nm in names:
                arrs[nm].append(o[nm])
            off += n
        if k % 10 == 0:
            print("  trellis: %d rows" % len(rows), flush=True)
    out = {"t_rows": np.array(rows, np.int64), "t_fields": np.array(T_FIELDS),
           "t_coeff_costs": cc, "t_eob_costs": eo}
    for nm in names:
        out["t_" + nm] = np.concatenate(arrs[nm])
    return out


def _col(rows, fields, name):
    return rows[:, list(fields).index(name)]


def _blocks(flat, rows, fields):
    n, idx = _col(rows, fields, "n"), _col(rows, fields, "index")
    return [flat[i:i + k] for i, k in zip(idx, n)]


def check_conditions(F, ref):
    """The fixture is only written when it reaches the paths it is for."""
    sys.path.insert(0, os.path.dirname(HERE))
    import _qmref as R
    fails = []

    def need(ok, what):
        print("  %-4s %s" % ("ok" if ok else "FAIL", what))
        if not ok:
            fails.append(what)

    H, hf = F["h_rows"], list(F["h_fields"])
    Q, qf = F["q_rows"], list(F["q_fields"])
    for form in (0, 1):
        for bd in (8, 10, 12):
            m = (_col(H, hf, "form") == form) & (_col(H, hf, "bd") == bd)
            d = int((_col(H, hf, "eob")[m] != _col(H, hf, "eob_flat")[m]).sum())
            need(3 * d >= int(m.sum()), "helper form %d bd %d: %d of %d eobs differ from flat"
                 % (form, bd, d, int(m.sum())))
    # the int16 clamp: a stored 8-bit row whose |coeff| + round exceeds 32767
    for name, rows, fields, formcol, flat in (("helper", H, hf, "form", F["h_coeff"]),
                                              ("facade", Q, qf, "mode", F["q_coeff"])):
        for form in (0, 1):
            hit = 0
            for r, c in zip(rows, _blocks(flat, rows, fields)):
                if r[fields.index("bd")] != 8 or r[fields.index(formcol)] != form:
                    continue
                # the helper path: either matrix in a direct call, both at the facade
                on = r[fields.index("qm_set")] + r[fields.index("iqm_set")]
                if on < (1 if name == "helper" else 2):
                    continue
                if r[fields.index("eob")] and np.abs(c).max() >= 32767:
                    hit += 1
            need(hit > 0, "%s form %d: int16 clamp engaged in %d 8-bit rows" % (name, form, hit))
    # no table-built row wraps |q| * dequant (see the module docstring)
    worst = 0
    for rows, fields, flat in ((H, hf, F["h_qcoeff"]), (Q, qf, F["q_qcoeff"])):
        for r, q in zip(rows, _blocks(flat, rows, fields)):
            g = dict(zip(fields, r))
            deq = F["qtab"][(8, 10, 12).index(g["bd"]), g["qindex"], 6].astype(np.int64)
            worst = max(worst, int(np.abs(q.astype(np.int64)).max()) * ((int(deq.max()) * 255 + 16) >> 5))
    need(worst < 1 << 31, "no table-built row can wrap |q| * dequant (worst product %d)" % worst)
    for name, rows, fields in (("helper", H, hf), ("facade", Q, qf)):
        a = int(((_col(rows, fields, "qm_set") == 1) & (_col(rows, fields, "iqm_set") == 0)).sum())
        b = int(((_col(rows, fields, "qm_set") == 0) & (_col(rows, fields, "iqm_set") == 1)).sum())
        need(a > 0 and b > 0, "%s: %d rows qm only, %d rows iqm only" % (name, a, b))
    # block error: weight at scan[i] against weight at i; the bd shift
    at_i = shifted = 0
    offs = F["table_offsets"]
    for r, c, dq in zip(Q, _blocks(F["q_coeff"], Q, qf), _blocks(F["q_dqcoeff"], Q, qf)):
        g = dict(zip(qf, r))
        if not g["qm_set"]:
            continue
        qm = R.matrix(F, g["level"], g["plane"], g["tx_size"], offs)[0]
        scan = ref.scan_np(g["tx_size"], g["tx_type"])
        e, _ = R.block_error_qm(c, dq, qm, scan)
        assert e == g["err_qm"], "block_error_qm restatement"
        e2, _ = R.block_error_qm(c, dq, qm, np.arange(len(c)))
        at_i += int(e2 != e)
        if g["bd"] > 8:
            ls = R.tx_scale(g["tx_size"])
            sh = (1 - ls) * 2
            full = R.rshift_signed(e, sh)
            assert full == g["dist2"]
            shifted += int(R.rshift_signed(e >> (2 * (g["bd"] - 8)), sh) != g["dist2"])
    need(at_i > 0, "block error: %d rows change with the weight taken at i" % at_i)
    need(shifted > 0, "QM-PSNR highbd: %d rows change if the bd shift is applied" % shifted)
    T, tf = F["t_rows"], list(F["t_fields"])
    qi, q0, q1 = (_blocks(F["t_" + k], T, tf) for k in ("qcoeff_in", "qcoeff0", "qcoeff1"))
    changed = sum(int(not np.array_equal(a, b)) for a, b in zip(qi, q0))
    need(3 * changed >= len(T), "trellis: %d of %d blocks changed by the walk" % (changed, len(T)))
    df = int(_col(T, tf, "differs_flat_iqm").sum())
    need(df >= 10, "trellis: %d blocks differ from the flat-iqm run" % df)
    dm = sum(int(not np.array_equal(a, b) or r[tf.index("eob0")] != r[tf.index("eob1")] or
                 r[tf.index("rate0")] != r[tf.index("rate1")]) for a, b, r in zip(q0, q1, T))
    need(dm >= 10, "trellis: %d blocks differ between the two metrics" % dm)
    tt = set(_col(T, tf, "tx_type").tolist())
    need({0, 10, 11} <= tt and 9 in tt, "trellis: classes 2D / vert / horiz and IDTX present")
    need(set(_col(T, tf, "sharpness").tolist()) == {0, 1}, "trellis: sharpness 0 and 1")
    pi = set(zip(_col(T, tf, "plane").tolist(), _col(T, tf, "is_inter").tolist()))
    need({(0, 1), (0, 0), (1, 1)} <= pi, "trellis: luma inter, luma intra, chroma")
    if fails:
        raise SystemExit("fixture conditions not met:\n  " + "\n  ".join(fails))


def main():
    txfm_fix = dict(np.load(os.path.join(HERE, "fix_txfm.npz")))
    ref = Ref()
    F = {"levels": np.array(LEVELS, np.int32),
         "wt": ref.wt[list(LEVELS)].copy(), "iwt": ref.iwt[list(LEVELS)].copy(),
         "table_offsets": ref.table_offsets(), "qmlevel": ref.qmlevels(), "qtab": ref.qtab(),
         "qmlevel_args": np.array(QMLEVEL_ARGS, np.int32)}
    F.update(gen_helpers(ref, txfm_fix))
    F.update(gen_facade(ref, txfm_fix))
    F.update(gen_trellis(ref, txfm_fix))
    check_conditions(F, ref)
    path = os.path.join(HERE, "fix_qm.npz")
    np.savez_compressed(path, **F)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
