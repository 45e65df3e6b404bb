"""The coefficient-rate layer on the device at its extremes: the three kernels
that share csrc/coeffcost_dev.h -- cost_coeffs_kernel
(lavish_cost_coeffs_txb_batch), trellis_kernel (lavish_optimize_b_batch and
its QM instantiation) and the RATE branch of the C4 decision kernel
(lavish_rdo_plane_rate) -- against tests/golden/fix_txb_extremes.npz (the
reference's own results) and against the oracle on the full input sets of
tests/_txbextremes.py.  Integer arithmetic: every comparison is bit-exact.
The input conditions are those of tests/test_txb_extremes_cpu.py, asserted
again here on the oracle's outputs, so no case can quietly stop reaching its
target."""
import numpy as np
import pytest

import _oracle as O
import _txbextremes as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp
    return lavish_dsp


@pytest.fixture(scope="module")
def F():
    return X.load_fixture()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _rates(costs, q, eob, s, t, plane, ctx, ttc, mode):
    from lavish_dsp import txb
    r = txb.cost_coeffs_txb_batch(costs, _dev(q), _dev(eob), s, t, plane,
                                  None if ctx is None else _dev(ctx), ttc, mode)
    return r.cpu().numpy()


# ---------------------------------------------------------------------------
# cost_coeffs_txb_batch
# ---------------------------------------------------------------------------
def test_cost_coeffs_fixture_rows(L, F):
    from lavish_dsp import txb
    J = {n: i for i, n in enumerate(X.C_FIELDS)}
    costs = txb.CoeffCosts(X.tables(int(F["table_seed"][0])))
    groups = {}
    for r in F["c_rows"]:
        key = tuple(int(r[J[k]]) for k in ("set", "tx_size", "tx_type", "plane", "tx_type_cost"))
        groups.setdefault(key, []).append(r)
    done = 0
    for (which, s, t, plane, ttc), rows in groups.items():
        q, eob = (X.level_blocks(s, t) if which == 0 else X.probe_blocks(s, t))[:2]
        idx = [int(r[J["block"]]) for r in rows]
        ctx = np.array([[r[J["txb_skip_ctx"]], r[J["dc_sign_ctx"]]] for r in rows], np.int32)
        for mode, col in ((txb.COEFF_RATE_EXACT, "rate"), (txb.COEFF_RATE_LAPLACIAN,
                                                          "rate_laplacian")):
            got = _rates(costs, q[idx], eob[idx], s, t, plane, ctx, ttc, mode)
            np.testing.assert_array_equal(got, [r[J[col]] for r in rows],
                                          err_msg="set %d size %d type %d %s" % (which, s, t, col))
        done += len(rows)
    assert done == len(F["c_rows"])


def _both_modes_planes_ctx(costs, blob, q, eob, s, t, seed):
    """Exact and Laplacian, planes 0 and 1, with and without txb_ctx, against
    the oracle.  -> the exact plane-0 rates without contexts (device, oracle)."""
    rng = np.random.default_rng(seed)
    nb = len(q)
    ctx = np.stack([rng.integers(0, 13, nb), rng.integers(0, 3, nb)], 1).astype(np.int32)
    keep = None
    for plane in (0, 1):
        for lap in (False, True):
            for c, ttc in ((ctx, 777), (None, 0)):
                want = O.cost_coeffs_txb_batch(blob, q, eob, plane, s, t, c, ttc, lap)
                got = _rates(costs, q, eob, s, t, plane, c, ttc, int(lap))
                np.testing.assert_array_equal(got, want, err_msg="size %d type %d plane %d lap %d "
                                              "ctx %d" % (s, t, plane, lap, c is not None))
                if plane == 0 and not lap and c is None:
                    keep = (got, want)
    return keep


@pytest.mark.parametrize("s,t", X.LEVEL_CASES)
def test_cost_coeffs_level_blocks(L, s, t):
    from lavish_dsp import txb
    q, eob, _ = X.check_level_blocks(s, t)
    blob = X.tables(300 + s)
    _both_modes_planes_ctx(txb.CoeffCosts(blob), blob, q, eob, s, t, 5)


@pytest.mark.parametrize("s,t", X.PROBE_CASES)
def test_cost_coeffs_neighbour_probes(L, s, t):
    """For every class and zone the set of offsets whose neighbour changes the
    rate is the oracle's, and the oracle's is the reference's five."""
    from lavish_dsp import txb
    blob = X.tables(11)
    assert X.table_cells_distinct(blob, s, 0)
    q, eob, index = X.probe_blocks(s, t)
    got, want = _both_modes_planes_ctx(txb.CoeffCosts(blob), blob, q, eob, s, t, 6)
    X.check_probe_sets(want, index, s, t)
    assert X.probe_sets(got, index) == X.probe_sets(want, index)


@pytest.mark.parametrize("s,nb", X.STRIDE_CASES)
def test_cost_coeffs_grid_stride_passes(L, s, nb):
    """Batches past the 2048-workgroup grid cap (_txbextremes.GRID_CAP): the
    workgroups take a second, partial pass over LDS level maps that the
    first pass left full (or nearly empty)."""
    from lavish_dsp import txb
    q, eob, ctx = X.stride_blocks(s, nb)
    blob = X.tables(40 + s)
    costs = txb.CoeffCosts(blob)
    for lap in (False, True):
        want = O.cost_coeffs_txb_batch(blob, q, eob, 0, s, 0, ctx, 99, lap)
        got = _rates(costs, q, eob, s, 0, 0, ctx, 99, int(lap))
        np.testing.assert_array_equal(got, want, err_msg="lap %d" % lap)


# ---------------------------------------------------------------------------
# optimize_b_batch
# ---------------------------------------------------------------------------
def _trellis_device(costs, r, qm=None):
    """One launch on a run of _txbextremes._trellis_run(); qm: None (the flat
    call), "null" (the QM call, both matrices NULL) or "iqm32"."""
    import torch
    from lavish_dsp import qm as qmod, txb
    tc, qc, dq, eob = _dev(r["c"]), _dev(r["q_in"]), _dev(r["dq_in"]), _dev(r["eob_in"])
    ctx = _dev(r["ctx"])
    args = (costs, tc, qc, dq, eob, r["s"], r["t"], r["bd"], r["rdmult"], r["dqv"])
    kw = dict(plane=r["plane"], is_inter=r["inter"], sharpness=r["sharp"], txb_ctx=ctx,
              tx_type_cost=r["ttc"])
    if qm is None:
        rate, ec = txb.optimize_b_batch(*args, **kw)
    else:
        iqm = None
        if qm == "iqm32":
            iqm = torch.full((O.max_eob(r["s"]),), 32, dtype=torch.uint8, device="cuda")
        rate, ec = qmod.optimize_b_qm_batch(*args, iqm=iqm, qm_dist=None, **kw)
    torch.cuda.synchronize()
    return dict(rate=rate.cpu().numpy(), entropy=ec.cpu().numpy(),
                eob=eob.cpu().numpy().view(np.uint16), q=qc.cpu().numpy(), dq=dq.cpu().numpy())


def _same(got, want, msg):
    for k in ("eob", "rate", "entropy", "q", "dq"):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (msg, k))


def test_optimize_b_fixture_rows(L, F):
    from lavish_dsp import txb
    J = {n: i for i, n in enumerate(X.T_FIELDS)}
    costs = txb.CoeffCosts(X.tables(int(F["table_seed"][0])))
    for row in F["t_rows"]:
        g = {k: int(row[J[k]]) for k in X.T_FIELDS}
        n, i = g["n"], g["index"]
        s, t, bd = g["tx_size"], g["tx_type"], g["bd"]
        c = X.coeffs(X.KINDS[g["kind"]], s, t, bd, 1, g["seed"], g["sparse_mag"])
        q_in, dq_in = F["t_qcoeff_in"][None, i:i + n], F["t_dqcoeff_in"][None, i:i + n]
        r = dict(s=s, t=t, bd=bd, rdmult=g["rdmult"], plane=g["plane"], inter=g["is_inter"],
                 sharp=g["sharpness"], ttc=g["tx_type_cost"], c=c, q_in=q_in, dq_in=dq_in,
                 eob_in=np.array([g["eob_in"]], np.uint16),
                 ctx=np.array([[g["txb_skip_ctx"], g["dc_sign_ctx"]]], np.int32),
                 dqv=O.quant_arrays(O.build_quant(bd, g["qindex"]))["dequant"])
        want = dict(eob=[g["eob"]], rate=[g["rate"]], entropy=[g["entropy_ctx"]],
                    q=q_in + F["t_qcoeff_delta"][None, i:i + n],
                    dq=dq_in + F["t_dqcoeff_delta"][None, i:i + n])
        _same(_trellis_device(costs, r), want, str(g))


def _run_group(costs, runs):
    for r in runs:
        msg = "size %d type %d bd %d q %d rdmult %d %s nb %d" % (
            r["s"], r["t"], r["bd"], r["qindex"], r["rdmult"], r["kind"], r["nb"])
        _same(_trellis_device(costs, r), r, msg)
        _same(_trellis_device(costs, r, "null"), r, msg + " qm NULL")
        _same(_trellis_device(costs, r, "iqm32"), r, msg + " iqm 32")


@pytest.mark.parametrize("s,t", X.TRELLIS_CASES)
def test_optimize_b_12bit_extremes(L, s, t):
    from lavish_dsp import txb
    runs = X.trellis_group(s, t)
    print(X.check_trellis_group(runs, s, t))
    _run_group(txb.CoeffCosts(X.tables(X.TRELLIS_TABLE_SEED)), runs)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_optimize_b_sparse_update_skip(L, bd):
    from lavish_dsp import txb
    runs = X.sparse_group(bd)
    print(X.check_sparse_group(runs))
    _run_group(txb.CoeffCosts(X.tables(X.TRELLIS_TABLE_SEED)), runs)


# ---------------------------------------------------------------------------
# rdo_plane_rate
# ---------------------------------------------------------------------------
def _rdo_cases(L, cases):
    import torch
    from lavish_dsp import txb
    for case in cases:
        s, bd, which = case["s"], case["bd"], case["which"]
        exp, eq, ed = X.rdo_oracle(case)
        print(which, X.check_rdo_case(case, exp, eq))
        costs = txb.CoeffCosts(case["blob"])
        qp = L.build_quant_params(bd, case["qindex"], L.QUANT_FP)
        ctx = _dev(case["ctx"])
        out = txb.rdo_plane_rate(_dev(case["src"]), _dev(case["pred"]), s, case["tmask"], qp,
                                 case["rdmult"], costs, ctx, case["ttc"],
                                 block_mask=_dev(case["masks"]), bit_depth=bd)
        torch.cuda.synchronize()
        got = L.rdo_records(out)
        for f in ("best_type", "eob", "rate", "satd", "dist", "sse", "rdcost"):
            np.testing.assert_array_equal(got[f], exp[f], err_msg="%s %s" % (which, f))
        np.testing.assert_array_equal(out["qcoeff"].cpu().numpy(), eq, err_msg=which)
        np.testing.assert_array_equal(out["dqcoeff"].cpu().numpy(), ed, err_msg=which)
        # each record's rate is cost_coeffs_txb_batch on its coefficients
        for t in np.unique(exp["best_type"]):
            sel = np.flatnonzero(exp["best_type"] == t)
            r = _rates(costs, eq[sel], exp["eob"][sel].astype(np.uint16), s, int(t), 0,
                       case["ctx"][sel], int(case["ttc"][t]), txb.COEFF_RATE_EXACT)
            np.testing.assert_array_equal(r, got["rate"][sel], err_msg="%s type %d" % (which, t))


@pytest.mark.parametrize("s", X.RDO_SIZES)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_rdo_rate_extremes(L, s, bd):
    _rdo_cases(L, [X.rdo_case(s, bd, which) for which in ("q0", "mid")])


@pytest.mark.parametrize("s,bd", sorted(X.RDO_BIG))
def test_rdo_rate_extremes_one_wave_per_tile(L, s, bd):
    """2048 tiles and more: the kernel's unsplit form."""
    _rdo_cases(L, [X.rdo_case(s, bd, "q0", big=True)])
