"""Self-check of the fixture pin: re-derive a sample of the committed golden
fixtures from the reference's own C text at test time
(tests/golden/cinterp.py over /root/reference), so the npz -> reference link
does not rest on gen_fixtures.py having been run once.

Only in the dev container: /root/reference does not exist on the GPU box, so
every test here skips there.  CPU only, a few seconds."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                                reason="reference sources absent (GPU box)")


@pytest.fixture(scope="module")
def G():
    sys.path.insert(0, GOLD)
    import gen_fixtures
    return gen_fixtures


def test_fwd_txfm_rederived(G):
    """av1_fwd_txfm2d_8x16_c re-executed on fix_txfm's stored inputs."""
    tu = G.tu_txfm()
    F = dict(np.load(os.path.join(GOLD, "fix_txfm.npz")))
    s = 7
    fn = tu.func("av1_fwd_txfm2d_%s_c" % G.TX_NAMES[s])
    W, H = G.TX_W[s], G.TX_H[s]
    for t in (0, 5, 12):
        for k in (0, 3, 7):
            blk, bd = F["in_%d_%d" % (s, t)][k], int(F["bd_%d_%d" % (s, t)][k])
            padded = np.zeros((H, W + 3), np.int16)
            padded[:, :W] = blk
            o = tu.buffer("int32_t", [0x5A5A5A5A] * (W * H))
            fn(tu.buffer("int16_t", padded.reshape(-1).tolist()), o, W + 3, t, bd)
            np.testing.assert_array_equal(np.array(o.buf, np.int32), F["out_%d_%d" % (s, t)][k])


def test_quantizer_rederived(G):
    """av1_build_quantizer (bd 8, sharpness 0) and av1_quantize_fp_32x32_c at
    qindex 128 re-executed on fix_quant's stored coefficients."""
    tu = G.tu_quant()
    Q = dict(np.load(os.path.join(GOLD, "fix_qparams.npz")))
    rows = G.build_quantizer(tu, 8, 0)
    for f, v in rows.items():
        np.testing.assert_array_equal(v, Q["%s_bd8_sh0" % f])
    F = dict(np.load(os.path.join(GOLD, "fix_quant.npz")))
    ci = [i for i, c in enumerate(G.QUANT_CASES) if c[0] == "av1_quantize_fp_32x32_c"][0]
    name, s, ls, hb, kind = G.QUANT_CASES[ci]
    scan, iscan = G.dct_scan(tu, s)
    n = G.max_eob(s)
    q = 128
    key = "%d_%d_q%d" % (ci, 8, q)
    for k in range(2):
        c = F["coeff_" + key][k]
        qp, dp = tu.buffer("int32_t", [77] * n), tu.buffer("int32_t", [77] * n)
        ep = tu.buffer("uint16_t", 1)
        i16 = lambda a: tu.buffer("int16_t", a.tolist())
        tu.func(name)(tu.buffer("int32_t", c.tolist()), n, i16(rows["y_zbin"][q]),
                      i16(rows["y_round_fp"][q]), i16(rows["y_quant_fp"][q]),
                      i16(rows["y_quant_shift"][q]), qp, dp, i16(rows["y_dequant_QTX"][q]), ep,
                      i16(scan), i16(iscan))
        np.testing.assert_array_equal(np.array(qp.buf, np.int32), F["qcoeff_" + key][k])
        np.testing.assert_array_equal(np.array(dp.buf, np.int32), F["dqcoeff_" + key][k])
        assert ep.buf[0] == F["eob_" + key][k]


def test_txfeat_rederived(G):
    """av1_get_horver_correlation_full_c on fix_txfeat's stored 16x16 blocks
    (float bit patterns)."""
    from cinterp import TU, reference_defines
    tu = TU(REF, ["aom/aom_integer.h", "aom_ports/mem.h", "aom_dsp/aom_dsp_common.h",
                  "av1/encoder/rdopt.c"], reference_defines(REF))
    if not tu.has_func("av1_get_horver_correlation_full_c"):
        tu = TU(REF, ["av1/encoder/encoder.h", "av1/encoder/rdopt.c"], reference_defines(REF))
    F = dict(np.load(os.path.join(GOLD, "fix_txfeat.npz")))
    hv = tu.func("av1_get_horver_correlation_full_c")
    done = 0
    for k, (s, w, h, kind, off) in enumerate(F["rows"]):
        if (w, h) != (16, 16):
            continue
        blk = F["blocks"][off:off + w * h]
        hc, vc = tu.buffer("float", 1), tu.buffer("float", 1)
        hv(tu.buffer("int16_t", blk.tolist()), w, w, h, hc, vc)
        got = np.array([hc.buf[0], vc.buf[0]], np.float32).view(np.int32)
        np.testing.assert_array_equal(got, F["features"][k][32:34])
        done += 1
    assert done >= 5


def test_interp_extremes_rederived():
    """fix_interp_extremes: the three MULTITAP_SHARP2 cases per bit depth whose
    int16 intermediate wraps (av1_highbd_convolve_2d_sr_c,
    av1_highbd_dist_wtd_convolve_2d_c, av1_highbd_convolve_2d_scale_c at the
    kernel's extreme phase), the lowbd scaled case whose uint16 sum wraps, and
    a warp case on filter row 127, re-executed on the stored inputs."""
    sys.path.insert(0, GOLD)
    import gen_fix_interp_extremes as GX
    import _extfix as E
    import _extremes as X
    F = E.load()
    J = {n: i for i, n in enumerate(E.CONV_FIELDS)}
    R = F["conv_rows"]
    pe = X.extreme_phase(X.SHARP2)
    picks = []
    for unit, mode in ((E.SINGLE, 0), (E.COMPOUND, 1), (E.SCALE, 0)):
        for bd in (10, 12):
            m = [k for k in F["wrap_rows"] if tuple(R[k][[J[n] for n in (
                "unit", "mode", "bd", "phase_x", "phase_y", "kind_y")]]) ==
                (unit, mode, bd, pe, pe, X.SHARP2)]
            assert m, (unit, bd)
            picks.append(m[0])
    m = np.flatnonzero((R[:, J["unit"]] == E.SCALE) & (R[:, J["highbd"]] == 0) &
                       (R[:, J["kind_x"]] == X.SHARP2) & (R[:, J["phase_x"]] == pe) &
                       (R[:, J["polarity"]] == 0) & (R[:, J["mode"]] == 0) &
                       (R[:, J["aligned"]] == 1))
    picks.append(int(m[0]))
    cv = GX.Conv(GX.tu_convolve())
    for k in picks:
        c = E.conv_case(F, k)
        v, got = E.conv_anchor(c)
        assert v["wraps"] and got != v["final"] & 0xFFFF, k
        cv.add(c.unit, c.highbd, c.bd, c.w, c.h, c.path, (c.kind_x, c.kind_y),
               (c.phase_x, c.phase_y), c.polarity, mode=c.mode,
               steps=(c.x_step_qn, c.y_step_qn), subpel=(c.subpel_x_qn, c.subpel_y_qn),
               src=c.src.astype(np.int64), org=(c.org_y, c.org_x))
        np.testing.assert_array_equal(cv.dst[-1].reshape(c.h, c.w), c.dst, err_msg=str(k))
        np.testing.assert_array_equal(cv.buf[-1].reshape(c.h, c.w), c.buf, err_msg=str(k))
    WJ = {n: i for i, n in enumerate(E.WARP_FIELDS)}
    Wr = F["warp_rows"]
    wp = GX.Warp(GX.tu_warp())
    for mode in (0, 1):
        k = int(np.flatnonzero((Wr[:, WJ["row_x"]] == 127) & (Wr[:, WJ["bd"]] == 10) &
                               (Wr[:, WJ["mode"]] == mode) & (Wr[:, WJ["polarity"]] == 1))[0])
        c = E.warp_case(F, k)
        wp.add(c.bd, c.mode, c.polarity, c.ref.astype(np.int64), c.mat, c.prm, c.p_col, c.p_row,
               c.p_width, c.p_height)
        np.testing.assert_array_equal(wp.pred[-1].reshape(c.pred.shape), c.pred, err_msg=str(k))
        np.testing.assert_array_equal(wp.buf[-1].reshape(c.buf.shape), c.buf, err_msg=str(k))


def test_mcomp_extremes_rederived():
    """fix_mcomp_extremes: one full-pel case of each family (a flat tie, a
    ramp, a periodic tile, a single-point window, a saturated 16x16 block,
    the lowest and the highest lambda) and three sub-pel cases (a cost list, a limit edge, a
    high lambda) re-executed from the reference on the stored planes."""
    sys.path.insert(0, GOLD)
    import gen_fix_mcomp_extremes as GM
    import _mvextremes as X
    from lavish_dsp import motion as M
    F = X.load_fixture()
    t = {}     # (the package's tables: gen_fix_mcomp_extremes checks them when it runs)
    for hp, nm in ((False, "lp"), (True, "hp")):
        t["mvjcost_" + nm], t["mvcost_" + nm] = M.default_mv_cost_tables(hp)
    for which, run, want in (
            ("fp", GM.fullpel_rows, ["flat_255_0", "ramp_x", "periodic_8", "point", "sat69",
                                     "lambda71", "lambda77"]),
            ("sp", GM.subpel_rows, ["sub_tie", "edge", "sub_lambda71"])):
        names = [str(n) for n in F[which + "_names"]]
        kinds = [str(k) for k in F[which + "_kinds"]]
        fp = {c.name: c for c in X.fixture_fullpel()}
        if which == "sp":
            cases = {c.name: c for c in X.fixture_subpel(
                GM.fullpel_results(list(fp.values()), F["fp_rows"]))}
        else:
            cases = fp
        picks = []
        for w in want:
            m = [i for i, (n, k) in enumerate(zip(names, kinds)) if n.startswith(w) or k == w]
            assert m, w
            picks.append(m[0])
        rows = run(t, {}, [(i, cases[names[i]]) for i in picks])
        stored = F[which + "_rows"]
        stored = np.concatenate([stored[stored[:, 0] == i] for i in picks])
        np.testing.assert_array_equal(rows, stored)
