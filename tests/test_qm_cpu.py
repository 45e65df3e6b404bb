"""The quantization-matrix path without a GPU:
* tests/_qmref.py (the numpy restatement the free-parameter GPU cases are
  compared with) equals every quantizer and distortion row the reference
  wrote into tests/golden/fix_qm.npz, and its get_dqv the trellis rows;
* the host helpers lavish_qm_level / lavish_qm_table_offset equal the recorded
  aom_get_qmlevel values and av1_qm_init's pointers;
* a sample of the fixture re-derived from the reference's C text (skipped
  where the reference sources are absent, as test_fixture_rederive.py is)."""
import os
import sys

import numpy as np
import pytest

import _qmref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(GOLD, "fix_qm.npz")))


@pytest.fixture(scope="module")
def L():
    import lavish_dsp
    return lavish_dsp


def rows(F, prefix):
    fields = [str(f) for f in F[prefix + "_fields"]]
    return [dict(zip(fields, (int(v) for v in r))) for r in F[prefix + "_rows"]]


def blk(F, name, g):
    return F[name][g["index"]:g["index"] + g["n"]]


def qtab(F, g):
    """LavishPlaneQuant fields of the row's (bd, qindex): [7][2]."""
    return F["qtab"][(8, 10, 12).index(g["bd"]), g["qindex"]]


def test_qmref_equals_helper_rows(F, L):
    n_rows = 0
    for g in rows(F, "h"):
        qm, iqm = R.matrix(F, g["level"], g["plane"], g["tx_size"])
        qm = qm if g["qm_set"] else None
        iqm = iqm if g["iqm_set"] else None
        scan = L.scan_order(g["tx_size"], g["tx_type"])[0]
        t = qtab(F, g)
        c = blk(F, "h_coeff", g)
        if g["form"] == 0:
            q, dq, eob = R.quantize_fp(c, t[1], t[2], t[6], scan, qm, iqm, g["log_scale"],
                                       g["hbd"])
        else:
            q, dq, eob = R.quantize_b(c, t[0], t[3], t[4], t[5], t[6], scan, qm, iqm,
                                      g["log_scale"], g["hbd"])
        np.testing.assert_array_equal(q, blk(F, "h_qcoeff", g), str(g))
        np.testing.assert_array_equal(dq, blk(F, "h_dqcoeff", g), str(g))
        assert eob == g["eob"], g
        n_rows += 1
    assert n_rows >= 200


def test_qmref_equals_facade_and_distortion_rows(F, L):
    helper = dc = qmdist = 0
    for g in rows(F, "q"):
        qm, iqm = R.matrix(F, g["level"], g["plane"], g["tx_size"])
        qm = qm if g["qm_set"] else None
        iqm = iqm if g["iqm_set"] else None
        # what the fixture says the reference chose: NULL for level 15 and flat types
        assert g["qm_set"] == int(g["level"] != 15 and g["tx_type"] < 9 and g["force"] != 2), g
        assert g["iqm_set"] == int(g["level"] != 15 and g["tx_type"] < 9 and g["force"] != 1), g
        scan = L.scan_order(g["tx_size"], g["tx_type"])[0]
        t = qtab(F, g)
        c = blk(F, "q_coeff", g)
        ls, hbd = R.tx_scale(g["tx_size"]), g["bd"] > 8
        both = qm is not None and iqm is not None
        if g["mode"] == 2:
            q, dq, eob = R.quantize_dc(c, t[3][0], t[2][0], t[6][0], qm, iqm, ls, hbd)
            dc += 1
        elif g["mode"] == 0:  # the facade rule: the helper only with both matrices
            q, dq, eob = R.quantize_fp(c, t[1], t[2], t[6], scan, qm if both else None,
                                       iqm if both else None, ls, hbd)
        else:
            q, dq, eob = R.quantize_b(c, t[0], t[3], t[4], t[5], t[6], scan, qm if both else None,
                                      iqm if both else None, ls, hbd)
        helper += int(both and g["mode"] != 2)
        np.testing.assert_array_equal(q, blk(F, "q_qcoeff", g), str(g))
        np.testing.assert_array_equal(dq, blk(F, "q_dqcoeff", g), str(g))
        assert eob == g["eob"], g
        for metric in (0, 1):
            d, s = R.dist_block_tx_domain(c, dq, g["tx_size"], g["bd"], qm, scan, metric)
            assert (d, s) == (g["dist%d" % (metric + 1)], g["sse%d" % (metric + 1)]), (g, metric)
        if qm is not None:
            assert R.block_error_qm(c, dq, qm, scan) == (g["err_qm"], g["ssz_qm"]), g
            qmdist += 1
    assert helper >= 100 and dc >= 100 and qmdist >= 200


def test_qmref_get_dqv_equals_trellis_rows(F, L):
    """Every coefficient the walk lowered: dqcoeff = sign * ((|q| * get_dqv) >>
    shift), with the weighted dequantizer of its position."""
    lowered = 0
    for g in rows(F, "t"):
        _, iqm = R.matrix(F, g["level"], g["plane"], g["tx_size"])
        iqm = iqm if g["iqm_set"] else None
        deq = qtab(F, g)[6]
        shift = R.tx_scale(g["tx_size"])
        qi, q0, dq0 = blk(F, "t_qcoeff_in", g), blk(F, "t_qcoeff0", g), blk(F, "t_dqcoeff0", g)
        for ci in np.nonzero((qi != q0) & (q0 != 0))[0]:
            a = abs(int(q0[ci]))
            adq = (a * R.get_dqv(deq, int(ci), iqm)) >> shift
            assert int(dq0[ci]) == (-adq if q0[ci] < 0 else adq), (g, ci)
            lowered += 1
    assert lowered >= 100


def test_qm_level_matches_reference(F, L):
    from lavish_dsp import qm
    for (first, last), want in zip(F["qmlevel_args"], F["qmlevel"]):
        got = [qm.qm_level(q, int(first), int(last)) for q in range(256)]
        assert got == want.tolist(), (first, last)
    assert F["qmlevel"].shape == (3, 256)


def test_qm_table_offset_matches_reference(F, L):
    from lavish_dsp import qm
    assert [qm.table_offset(s) for s in range(19)] == F["table_offsets"].tolist()
    lib = L.lib()
    assert lib.lavish_qm_table_offset(19) == -1 and lib.lavish_qm_table_offset(-1) == -1
    # sizes that reuse another size's matrix (av1_get_adjusted_tx_size)
    for s in range(19):
        assert qm.table_offset(s) == qm.table_offset(R.adjusted_tx_size(s))
        assert qm.table_offset(s) + R.max_eob(s) <= R.QM_TOTAL_SIZE


def test_fixture_conditions_hold(F):
    """What the generator stops on, re-read from the committed file."""
    H, Q, T = rows(F, "h"), rows(F, "q"), rows(F, "t")
    for form in (0, 1):
        for bd in (8, 10, 12):
            sel = [g for g in H if g["form"] == form and g["bd"] == bd]
            assert 3 * sum(g["eob"] != g["eob_flat"] for g in sel) >= len(sel) > 0
    for tab in (H, Q):
        assert any(g["qm_set"] and not g["iqm_set"] for g in tab)
        assert any(g["iqm_set"] and not g["qm_set"] for g in tab)
    assert sum(g["differs_flat_iqm"] for g in T) >= 10
    assert sum((g["eob0"], g["rate0"]) != (g["eob1"], g["rate1"]) or
               not np.array_equal(blk(F, "t_qcoeff0", g), blk(F, "t_qcoeff1", g)) for g in T) >= 10
    changed = sum(not np.array_equal(blk(F, "t_qcoeff_in", g), blk(F, "t_qcoeff0", g)) for g in T)
    assert 3 * changed >= len(T)
    assert {0, 9, 10, 11} <= {g["tx_type"] for g in T}
    assert {g["sharpness"] for g in T} == {0, 1}
    assert {(0, 1), (0, 0), (1, 1)} <= {(g["plane"], g["is_inter"]) for g in T}
    assert {g["bd"] for g in Q} == {8, 10, 12} and {g["qindex"] for g in Q} == {0, 120, 255}
    assert os.path.getsize(os.path.join(GOLD, "fix_qm.npz")) < 1 << 20


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_sample_rederived_from_reference(F):
    """av1_qm_init's tables and offsets, and a sample of helper, facade and
    trellis rows, executed again from the reference's C text."""
    sys.path.insert(0, GOLD)
    import gen_fix_qm as GQ
    ref = GQ.Ref()
    lv = list(GQ.LEVELS)
    np.testing.assert_array_equal(ref.wt[lv], F["wt"])
    np.testing.assert_array_equal(ref.iwt[lv], F["iwt"])
    np.testing.assert_array_equal(ref.table_offsets(), F["table_offsets"])
    np.testing.assert_array_equal(ref.qmlevels(), F["qmlevel"])
    np.testing.assert_array_equal(ref.qtab(), F["qtab"])
    H = [g for g in rows(F, "h") if g["n"] <= 64]
    for g in H[::9]:
        o = ref.helper_row(g["form"], g["bd"], g["tx_size"], g["tx_type"], g["qindex"],
                           g["plane"], g["level"], g["qm_set"], g["iqm_set"], blk(F, "h_coeff", g))
        np.testing.assert_array_equal(o["qcoeff"], blk(F, "h_qcoeff", g))
        np.testing.assert_array_equal(o["dqcoeff"], blk(F, "h_dqcoeff", g))
        assert (o["eob"], o["eob_flat"]) == (g["eob"], g["eob_flat"])
    Q = [g for g in rows(F, "q") if g["n"] <= 64]
    for g in Q[::23]:
        o = ref.facade_row(g["bd"], g["tx_size"], g["tx_type"], g["qindex"], g["plane"],
                           g["level"], g["mode"], g["force"], blk(F, "q_coeff", g))
        np.testing.assert_array_equal(o["qcoeff"], blk(F, "q_qcoeff", g))
        np.testing.assert_array_equal(o["dqcoeff"], blk(F, "q_dqcoeff", g))
        for k in ("eob", "qm_set", "iqm_set", "dist1", "sse1", "dist2", "sse2", "err_qm",
                  "ssz_qm"):
            assert o[k] == g[k], (k, g)
    rnd = GQ.G.ACMRandom(0xbaba + 33)
    GQ.trellis_tables(rnd)  # the generator's draw order: tables first
    mc = GQ._get(ref.X, "mode_costs")
    itx = [rnd.generate(3000) for _ in range(len(GQ._get(mc, "inter_tx_type_costs")))]
    atx = [rnd.generate(3000) for _ in range(len(GQ._get(mc, "intra_tx_type_costs")))]
    ref.set_costs(F["t_coeff_costs"], F["t_eob_costs"], itx, atx)
    T = [g for g in rows(F, "t") if g["n"] <= 64]
    for g in T[::17]:
        o = ref.trellis_row(g["bd"], g["tx_size"], g["tx_type"], g["qindex"], g["plane"],
                            g["is_inter"], g["sharpness"], g["rdmult"], g["level"],
                            g["txb_skip_ctx"], g["dc_sign_ctx"], blk(F, "t_coeff", g))
        for k in ("qcoeff_in", "dqcoeff_in", "qcoeff0", "dqcoeff0", "qcoeff1", "dqcoeff1"):
            np.testing.assert_array_equal(o[k], blk(F, "t_" + k, g), k)
        for k in ("eob_in", "tx_type_cost", "eob0", "rate0", "entropy0", "eob1", "rate1",
                  "entropy1", "differs_flat_iqm"):
            assert o[k] == g[k], (k, g)
