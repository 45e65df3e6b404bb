"""The coefficient-rate layer at its extremes, on the CPU: the C oracle
(orc_cost_coeffs_txb*, orc_optimize_b, orc_rdo_plane_rate) against
tests/golden/fix_txb_extremes.npz (executed from the reference by
gen_fix_txb_extremes.py), and the input conditions that
tests/test_gpu_txb_extremes.py relies on, asserted here on the oracle's
outputs alone -- before any device is involved."""
import os
import sys
import zlib

import numpy as np
import pytest

import _oracle as O
import _txbextremes as X

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def F():
    return X.load_fixture()


def test_oracle_equals_cost_rows(F):
    """orc_cost_coeffs_txb, exact and Laplacian, on every stored row; the
    block rebuilt from the row is the block the reference was given."""
    J = {n: i for i, n in enumerate(X.C_FIELDS)}
    blob = X.tables(int(F["table_seed"][0]))
    cache = {}
    kinds = set()
    for r in F["c_rows"]:
        which, s, t, plane, b = (int(r[J[k]]) for k in ("set", "tx_size", "tx_type", "plane",
                                                         "block"))
        key = (which, s, t)
        if key not in cache:
            cache[key] = (X.level_blocks(s, t) if which == 0 else X.probe_blocks(s, t))[:2]
        q, eob = cache[key]
        assert zlib.crc32(q[b].tobytes()) == r[J["crc"]], key + (b,)
        assert eob[b] == r[J["eob"]]
        for lap, col in ((False, "rate"), (True, "rate_laplacian")):
            got = O.cost_coeffs_txb(blob, q[b], int(eob[b]), plane, s, t, int(r[J["txb_skip_ctx"]]),
                                    int(r[J["dc_sign_ctx"]]), int(r[J["tx_type_cost"]]), lap)
            assert got == r[J[col]], (key, b, col)
        kinds.add((which, X.tx_class(t)))
    assert kinds == {(w, c) for w in (0, 1) for c in (0, 1, 2)}
    assert len(F["c_rows"]) >= 300


def test_oracle_equals_trellis_rows(F):
    """orc_optimize_b on the reference quantizer's output of every stored row;
    the oracle's own FP quantizer gives that output too."""
    J = {n: i for i, n in enumerate(X.T_FIELDS)}
    blob = X.tables(int(F["table_seed"][0]))
    for r in F["t_rows"]:
        g = {k: int(r[J[k]]) for k in X.T_FIELDS}
        n, i = g["n"], g["index"]
        s, t, bd = g["tx_size"], g["tx_type"], g["bd"]
        c = X.coeffs(X.KINDS[g["kind"]], s, t, bd, 1, g["seed"], g["sparse_mag"])[0]
        q_in, dq_in = F["t_qcoeff_in"][i:i + n], F["t_dqcoeff_in"][i:i + n]
        oq, od, oe = X.quantize_fp(c[None], s, t, bd, g["qindex"])
        np.testing.assert_array_equal(oq[0], q_in, err_msg=str(g))
        np.testing.assert_array_equal(od[0], dq_in, err_msg=str(g))
        assert oe[0] == g["eob_in"]
        dqv = O.quant_arrays(O.build_quant(bd, g["qindex"]))["dequant"]
        e, rate, ec, q, d = O.optimize_b(blob, c, q_in, dq_in, g["eob_in"], g["plane"], s, t, bd,
                                         g["is_inter"], g["rdmult"], g["sharpness"], dqv,
                                         g["txb_skip_ctx"], g["dc_sign_ctx"], g["tx_type_cost"])
        assert (e, rate, ec) == (g["eob"], g["rate"], g["entropy_ctx"]), g
        np.testing.assert_array_equal(q, q_in + F["t_qcoeff_delta"][i:i + n], err_msg=str(g))
        np.testing.assert_array_equal(d, dq_in + F["t_dqcoeff_delta"][i:i + n], err_msg=str(g))


def test_fixture_conditions_hold(F):
    """What the generator stops on, re-read from the committed file."""
    c = X.trellis_conditions(F["t_rows"], F["t_qcoeff_in"], F["t_dqcoeff_in"],
                             F["t_qcoeff_in"] + F["t_qcoeff_delta"],
                             F["t_dqcoeff_in"] + F["t_dqcoeff_delta"])
    print(c)
    for k, v in c.items():
        assert v == 9 if k == "class_bd_pairs" else v >= 4, (k, v)
    J = {n: i for i, n in enumerate(X.T_FIELDS)}
    T = F["t_rows"]
    assert set(T[:, J["qindex"]].tolist()) == {0, 128, 255}
    assert set(T[:, J["rdmult"]].tolist()) == {200, 60000, 1 << 20}
    assert set(T[:, J["sharpness"]].tolist()) == {0, 2}
    assert {3, 4, 11, 18} <= set(T[:, J["tx_size"]].tolist())
    assert {(0, 1), (0, 0), (1, 1)} <= set(zip(T[:, J["plane"]].tolist(),
                                               T[:, J["is_inter"]].tolist()))
    assert os.path.getsize(X.FIXTURE) < 1 << 20


@pytest.mark.parametrize("s,t", X.PROBE_CASES)
def test_probe_sets_on_oracle(s, t):
    """The neighbours the oracle's contexts read are the reference's: five
    for get_nz_mag wherever all five lie inside the block."""
    blob = X.tables(11)
    assert X.table_cells_distinct(blob, s, 0)
    q, eob, index = X.probe_blocks(s, t)
    rates = O.cost_coeffs_txb_batch(blob, q, eob, 0, s, t, None, 0, False)
    X.check_probe_sets(rates, index, s, t)


@pytest.mark.parametrize("s,t", X.LEVEL_CASES)
def test_level_blocks_reach_their_targets(s, t):
    X.check_level_blocks(s, t)


@pytest.mark.parametrize("s,nb", X.STRIDE_CASES)
def test_stride_blocks_alternate_per_slot(s, nb):
    """The grid-stride batches: every slot's two passes differ in kind, and
    the oracle prices the two kinds differently."""
    q, eob, ctx = X.stride_blocks(s, nb)
    blob = X.tables(40 + s)
    r = O.cost_coeffs_txb_batch(blob, q[:64], eob[:64], 0, s, 0, ctx[:64], 99, False)
    assert r[eob[:64] > 3].min() > 10 * r[eob[:64] <= 3].max()


@pytest.mark.parametrize("s,t", X.TRELLIS_CASES)
def test_trellis_inputs_reach_their_targets(s, t):
    """The per-(size, type) conditions of the device test, on the oracle."""
    got = X.trellis_group(s, t)
    print(s, t, X.check_trellis_group(got, s, t))


def test_sparse_kind_reaches_update_skip():
    for bd in (8, 10, 12):
        got = X.sparse_group(bd)
        print(bd, X.check_sparse_group(got))


@pytest.mark.parametrize("s", X.RDO_SIZES)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_rdo_planes_reach_their_targets(s, bd):
    """The C4 planes: level >= 15 share at qindex 0, a block with every
    neighbour sum saturated, the levels around both clips at the middle
    qindex, a partial last tile -- on the oracle's winners."""
    for which in ("q0", "mid"):
        case = X.rdo_case(s, bd, which)
        exp, eq, ed = X.rdo_oracle(case)
        print(s, bd, which, X.check_rdo_case(case, exp, eq))


@pytest.mark.parametrize("s,bd", sorted(X.RDO_BIG))
def test_rdo_big_planes_reach_their_targets(s, bd):
    case = X.rdo_case(s, bd, "q0", big=True)
    exp, eq, ed = X.rdo_oracle(case)
    print(s, bd, X.check_rdo_case(case, exp, eq))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_sample_rederived_from_reference(F):
    """A sample of cost and trellis rows executed again from the reference's
    C text: byte for byte the stored rows and arrays."""
    sys.path.insert(0, GOLD)
    import gen_fix_txb_extremes as GX
    ref = GX.make_ref()
    cases = GX.cost_cases()
    picks = [(w, s, t, p, blocks[::7]) for w, s, t, p, blocks in cases
             if (w, s, t) in ((0, 2, 0), (0, 14, 11), (0, 13, 10), (0, 17, 0), (1, 7, 0),
                              (1, 2, 10))]
    rows = GX.cost_rows(ref, picks, log=False)
    J = {n: i for i, n in enumerate(X.C_FIELDS)}
    stored = {tuple(r[[J[k] for k in ("set", "tx_size", "tx_type", "block")]]): r
              for r in F["c_rows"]}
    assert len(rows) >= 30
    for r in rows:
        np.testing.assert_array_equal(r, stored[tuple(r[[J[k] for k in ("set", "tx_size",
                                                                        "tx_type", "block")]])])
    tc = GX.trellis_cases()
    T, TJ = F["t_rows"], {n: i for i, n in enumerate(X.T_FIELDS)}
    assert len(tc) == len(T)
    # one row of each class at bd 12, a 64-point size, a sparse row, bd 8 and 10
    want = [lambda r: r["bd"] == 12 and r["t"] == 0 and r["s"] == 2,
            lambda r: r["bd"] == 12 and r["t"] == 10, lambda r: r["bd"] == 12 and r["t"] == 11,
            lambda r: r["bd"] == 12 and r["s"] == 18, lambda r: r["kind"] == 3 and r["bd"] == 12,
            lambda r: r["bd"] == 8 and r["s"] == 3, lambda r: r["bd"] == 10 and r["qindex"] == 255]
    idx = [next(i for i, r in enumerate(tc) if w(r)) for w in want]
    out = GX.trellis_rows(ref, [tc[i] for i in idx], log=False)
    for k, i in enumerate(idx):
        got, have = out["t_rows"][k], T[i]
        skip = TJ["index"]
        np.testing.assert_array_equal(np.delete(got, skip), np.delete(have, skip))
        n, a, b = int(have[TJ["n"]]), int(got[skip]), int(have[skip])
        for nm in ("t_qcoeff_in", "t_dqcoeff_in", "t_qcoeff_delta", "t_dqcoeff_delta"):
            np.testing.assert_array_equal(out[nm][a:a + n], F[nm][b:b + n], err_msg=nm)
