"""GPU parity of the quantization-matrix path (lavish_dsp/qm.py) against the
reference's own execution (tests/golden/fix_qm.npz, no oracle in the loop):
every fixture row through lavish_av1_quant_qm_batch (dist_mode 0 / 1 / 2),
lavish_quantize_qm_batch, lavish_block_error_qm_batch,
lavish_optimize_b_qm_batch and aom_quantize_b_helper_hip, bit for bit; the
new calls against the flat ones where the reference runs flat; the
|q| * dequant wrap with free int16 parameters against tests/_qmref.py; and
the argument checks.

Batches: a row's block first and last in a batch of 67 (the facade's one
wave per block: a grid that is no multiple of anything), the trellis's pairs
tiled to 33 and 65 blocks (its waves carry 32 or 64 blocks)."""
import ctypes
import os

import numpy as np
import pytest

import _qmref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 0x5A5A5A5A


class Ctx:
    """The fixture on the device, shared by the tests of this module."""

    def __init__(self):
        import torch
        import lavish_dsp as L
        from lavish_dsp import qm, txb
        assert torch.cuda.is_available()
        self.torch, self.L, self.qm, self.txb = torch, L, qm, txb
        self.F = F = dict(np.load(os.path.join(GOLD, "fix_qm.npz")))
        wt = np.zeros((15, 2, R.QM_TOTAL_SIZE), np.uint8)
        iwt = np.zeros_like(wt)
        for i, lv in enumerate(F["levels"]):
            wt[lv], iwt[lv] = F["wt"][i], F["iwt"][i]
        self.tabs = qm.QmTables(wt, iwt)
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(F[k])).cuda()
                    for k in F if k[1] == "_" and F[k].dtype == np.int32 and F[k].ndim == 1}
        self.scans = {}

    def rows(self, prefix):
        fields = [str(f) for f in self.F[prefix + "_fields"]]
        return [dict(zip(fields, (int(v) for v in r))) for r in self.F[prefix + "_rows"]]

    def blk(self, name, g):
        return self.dev[name][g["index"]:g["index"] + g["n"]]

    def host(self, name, g):
        return self.F[name][g["index"]:g["index"] + g["n"]]

    def batch(self, name, g, peers, nb):
        """[nb, n]: g's block first and last, its peers' blocks between."""
        if nb == 1:
            return self.blk(name, g).reshape(1, -1).clone()
        mid = [self.blk(name, peers[i % len(peers)]) for i in range(nb - 2)]
        return self.torch.stack([self.blk(name, g)] + mid + [self.blk(name, g)])

    def scan(self, s, t):
        if (s, t) not in self.scans:
            self.scans[(s, t)] = self.torch.from_numpy(self.L.scan_order(s, t)[0]).cuda()
        return self.scans[(s, t)]

    def plane_quant(self, bd, qindex):
        pq = self.L.PlaneQuant()
        t = self.F["qtab"][(8, 10, 12).index(bd), qindex]
        for j, name in enumerate(R.QTAB_FIELDS):
            setattr(pq, name, (ctypes.c_int16 * 2)(int(t[j][0]), int(t[j][1])))
        return pq

    def quant_params(self, bd, qindex, form):
        qp = self.L.QuantParams()
        t = self.F["qtab"][(8, 10, 12).index(bd), qindex]
        src = {"zbin": 0, "round": 1 if form == 0 else 3, "quant": 2 if form == 0 else 4,
               "quant_shift": 5, "dequant": 6}
        for name, j in src.items():
            setattr(qp, name, (ctypes.c_int16 * 2)(int(t[j][0]), int(t[j][1])))
        return qp

    def views(self, g, tx_type=0):
        """The row's matrices as a caller holds them for a 2-D type (the
        calls null them for flat types themselves); a matrix the row ran
        without (force) is dropped."""
        qm, iqm = self.tabs.views(g["level"], g["plane"], g["tx_size"], tx_type)
        if g.get("force") == 1:
            iqm = None
        if g.get("force") == 2:
            qm = None
        return qm, iqm


@pytest.fixture(scope="module")
def X():
    return Ctx()


def same_n(rows):
    by = {}
    for g in rows:
        by.setdefault((g["n"], g["bd"]), []).append(g)
    return by


def test_av1_quant_qm_batch_vs_reference(X):
    torch, qm = X.torch, X.qm
    rows = X.rows("q")
    peers = same_n(rows)
    helper = 0
    for i, g in enumerate(rows):
        m, im = X.views(g)
        pq = X.plane_quant(g["bd"], g["qindex"])
        for dist_mode in (0, 1, 2):
            nb = 67 if (i + dist_mode) % 3 == 0 else 1
            coeff = X.batch("q_coeff", g, peers[(g["n"], g["bd"])], nb)
            qc, dq, eob, flags, dist, sse = qm.av1_quant_qm_batch(
                coeff, g["tx_size"], g["tx_type"], g["bd"], pq, g["mode"], m, im, dist_mode)
            torch.cuda.synchronize()
            for b in {0, nb - 1}:
                msg = "%s dist_mode %d block %d of %d" % (g, dist_mode, b, nb)
                np.testing.assert_array_equal(qc[b].cpu().numpy(), X.host("q_qcoeff", g), msg)
                np.testing.assert_array_equal(dq[b].cpu().numpy(), X.host("q_dqcoeff", g), msg)
                assert int(eob[b]) & 0xFFFF == g["eob"], msg
                assert int(flags[b]) == g["mode"] << 1, msg
                if dist_mode:
                    want = (g["dist%d" % dist_mode], g["sse%d" % dist_mode])
                    assert (int(dist[b]), int(sse[b])) == want, msg
        helper += int(g["qm_set"] and g["iqm_set"])
    assert helper >= 200 and len(rows) >= 500


def test_quantize_qm_batch_vs_reference(X):
    torch, qm = X.torch, X.qm
    rows = X.rows("h")
    peers = same_n(rows)
    for i, g in enumerate(rows):
        m, im = X.tabs.views(g["level"], g["plane"], g["tx_size"])
        nb = 67 if i % 3 == 0 else 1
        coeff = X.batch("h_coeff", g, peers[(g["n"], g["bd"])], nb)
        q, dq, eob = qm.quantize_qm_batch(
            coeff, X.scan(g["tx_size"], g["tx_type"]), g["log_scale"],
            X.quant_params(g["bd"], g["qindex"], g["form"]), m if g["qm_set"] else None,
            im if g["iqm_set"] else None, g["bd"], g["form"])
        torch.cuda.synchronize()
        for b in {0, nb - 1}:
            np.testing.assert_array_equal(q[b].cpu().numpy(), X.host("h_qcoeff", g), str(g))
            np.testing.assert_array_equal(dq[b].cpu().numpy(), X.host("h_dqcoeff", g), str(g))
            assert int(eob[b]) & 0xFFFF == g["eob"], g
    assert len(rows) >= 200


def test_aom_quantize_b_helper_shim_vs_reference(X):
    """aom_quantize_b_helper_c's rows (form B, low bit depth) through the
    per-call shim, host buffers."""
    n_rows = 0
    for g in X.rows("h"):
        if g["form"] != 1 or g["hbd"]:
            continue
        hq, hi = R.matrix(X.F, g["level"], g["plane"], g["tx_size"])
        t = X.F["qtab"][0, g["qindex"]]
        n = g["n"]
        scan, iscan = X.L.scan_order(g["tx_size"], g["tx_type"])
        q = np.full(n, SENTINEL, np.int32)
        dq = np.full(n, SENTINEL, np.int32)
        eob = np.zeros(1, np.uint16)
        row8 = lambda v: np.ascontiguousarray(np.concatenate([v, [v[1]] * 6]), np.int16)
        X.qm.aom_quantize_b_helper(
            np.ascontiguousarray(X.host("h_coeff", g)), n, row8(t[0]), row8(t[3]), row8(t[4]),
            row8(t[5]), q, dq, row8(t[6]), eob, scan, iscan,
            np.ascontiguousarray(hq) if g["qm_set"] else None,
            np.ascontiguousarray(hi) if g["iqm_set"] else None, g["log_scale"])
        np.testing.assert_array_equal(q, X.host("h_qcoeff", g), str(g))
        np.testing.assert_array_equal(dq, X.host("h_dqcoeff", g), str(g))
        assert int(eob[0]) == g["eob"], g
        n_rows += 1
    assert n_rows >= 30
    assert X.L.status()[0] == 0, X.L.status()


def test_block_error_qm_batch_vs_reference(X):
    torch, qm = X.torch, X.qm
    rows = [g for g in X.rows("q") if g["qm_set"]]
    peers = same_n(rows)
    for i, g in enumerate(rows):
        m, _ = X.views(g)
        nb = 67 if i % 3 == 0 else 1
        p = peers[(g["n"], g["bd"])]
        err, ssz = qm.block_error_qm_batch(X.batch("q_coeff", g, p, nb),
                                           X.batch("q_dqcoeff", g, p, nb), m,
                                           X.scan(g["tx_size"], g["tx_type"]))
        torch.cuda.synchronize()
        for b in {0, nb - 1}:
            assert (int(err[b]), int(ssz[b])) == (g["err_qm"], g["ssz_qm"]), (g, b)
    assert len(rows) >= 200


def _trellis_batch(X, pair, nb):
    """The configuration's blocks tiled to nb: device inputs and the fixture
    rows block by block."""
    torch = X.torch
    order = [pair[i % len(pair)] for i in range(nb)]
    st = lambda name: torch.stack([X.blk(name, g) for g in order]).contiguous()
    eob = torch.tensor([g["eob_in"] for g in order], dtype=torch.int16, device="cuda")
    ctx = torch.tensor([[g["txb_skip_ctx"], g["dc_sign_ctx"]] for g in order], dtype=torch.int32,
                       device="cuda")
    return order, st("t_coeff"), st("t_qcoeff_in"), st("t_dqcoeff_in"), eob, ctx


def test_optimize_b_qm_batch_vs_reference(X):
    torch, qm, txb = X.torch, X.qm, X.txb
    F = X.F
    costs = txb.CoeffCosts(txb.coeff_costs_blob(F["t_coeff_costs"], F["t_eob_costs"]))
    rows = X.rows("t")
    keys = ("bd", "tx_size", "tx_type", "qindex", "plane", "is_inter", "sharpness", "rdmult",
            "level", "tx_type_cost")
    groups = {}
    for g in rows:
        groups.setdefault(tuple(g[k] for k in keys), []).append(g)
    checked = 0
    for k, (key, pair) in enumerate(groups.items()):
        g = pair[0]
        m, im = X.tabs.views(g["level"], g["plane"], g["tx_size"])  # flat types: nulled inside
        deq = F["qtab"][(8, 10, 12).index(g["bd"]), g["qindex"], 6]
        for metric in (0, 1):
            nb = (33, 65, len(pair), len(pair))[(k + metric) % 4]
            order, tc, qc, dq, eob, ctx = _trellis_batch(X, pair, nb)
            rate, ec = qm.optimize_b_qm_batch(
                costs, tc, qc, dq, eob, g["tx_size"], g["tx_type"], g["bd"], g["rdmult"], deq,
                im, m if metric else None, g["plane"], g["is_inter"], g["sharpness"], ctx,
                g["tx_type_cost"])
            torch.cuda.synchronize()
            msg = "%s metric %d nb %d" % (key, metric, nb)
            sfx = str(metric)
            np.testing.assert_array_equal(rate.cpu().numpy(), [r["rate" + sfx] for r in order], msg)
            np.testing.assert_array_equal(eob.cpu().numpy().view(np.uint16),
                                          [r["eob" + sfx] for r in order], msg)
            np.testing.assert_array_equal(ec.cpu().numpy(), [r["entropy" + sfx] for r in order],
                                          msg)
            np.testing.assert_array_equal(
                qc.cpu().numpy(), np.stack([X.host("t_qcoeff" + sfx, r) for r in order]), msg)
            np.testing.assert_array_equal(
                dq.cpu().numpy(), np.stack([X.host("t_dqcoeff" + sfx, r) for r in order]), msg)
            checked += 1
    assert checked == 2 * len(groups) and len(groups) >= 100


FLAT_CASES = [(0, 0, 8), (1, 3, 10), (14, 9, 8), (14, 10, 12), (3, 0, 10), (4, 0, 8), (18, 0, 12)]


@pytest.mark.parametrize("s,t,bd", FLAT_CASES)
def test_flat_cases_write_the_old_calls_bits(X, s, t, bd):
    """Both matrices NULL, only one given at the facade, and identity / 1-D
    types with both given: the new calls against the old ones on the same
    inputs (GPU to GPU)."""
    torch, L, qm, txb = X.torch, X.L, X.qm, X.txb
    rows = [g for g in X.rows("q") if g["tx_size"] == s and g["bd"] == bd]
    coeff = torch.stack([X.blk("q_coeff", rows[i % len(rows)]) for i in range(67)])
    nb = coeff.shape[0]
    m, im = X.tabs.views(7, 0, s)
    qindex = 120
    pq = X.plane_quant(bd, qindex)
    qstep = int(pq.dequant[1]) >> ((bd - 5) if bd > 8 else 3)
    dc_only = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    if t >= 9:
        variants = [(m, im)]
    else:
        variants = [(None, None), (m, None), (None, im)]
    eq = lambda a, b: np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    for vq, vi in variants:
        for mode, skip, thr in ((L.AV1_QUANT_FP, 0, 0xFFFFFFFF), (L.AV1_QUANT_B, 0, 0xFFFFFFFF),
                                (L.AV1_QUANT_SATD_GATE, 0, 23), (L.AV1_QUANT_SATD_GATE, 1, 23),
                                (L.AV1_QUANT_DC, 0, 0xFFFFFFFF)):
            if mode == L.AV1_QUANT_DC and (vq is not None or vi is not None) and t < 9:
                continue  # the DC facade weights with one matrix alone (quantize_dc)
            old = L.av1_quant_batch(coeff, s, t, bd, pq, mode, skip, thr, qstep, dc_only)
            new = qm.av1_quant_qm_batch(coeff, s, t, bd, pq, mode, vq, vi, qm.DIST_QM_PSNR
                                        if vq is None or t >= 9 else qm.DIST_TX_DOMAIN, skip, thr,
                                        qstep, dc_only)
            torch.cuda.synchronize()
            for a, b in zip(old, new[:4]):
                eq(a, b)
            # the flat distortion: dist_block_tx_domain's plain form on these outputs
            c, d = coeff.cpu().numpy(), new[1].cpu().numpy()
            for b in (0, nb - 1):
                want = R.dist_block_tx_domain(c[b], d[b], s, bd, None, None, 0)
                assert (int(new[4][b]), int(new[5][b])) == want
    # lavish_quantize_qm_batch with no matrix against lavish_quantize_batch
    ls = R.tx_scale(s)
    for form in (0, 1):
        qp = X.quant_params(bd, qindex, form)
        old = L.quantize_batch(coeff, X.scan(s, t), ls, qp, bd, form)
        new = qm.quantize_qm_batch(coeff, X.scan(s, t), ls, qp, None, None, bd, form)
        torch.cuda.synchronize()
        for a, b in zip(old, new):
            eq(a, b)
    # the trellis: NULL matrices, or any matrices on a flat type
    rng = np.random.default_rng(7 + s)
    costs = txb.CoeffCosts(rng.integers(30, 4000, txb.COEFF_COSTS_CELLS).astype(np.int32))
    q0, d0, e0, _ = L.av1_quant_batch(coeff, s, t, bd, pq, L.AV1_QUANT_FP)
    deq = np.array([pq.dequant[0], pq.dequant[1]], np.int16)
    ctx = torch.from_numpy(np.stack([rng.integers(0, 13, nb), rng.integers(0, 3, nb)],
                                    1).astype(np.int32)).cuda()
    a = [x.clone() for x in (q0, d0, e0)]
    b = [x.clone() for x in (q0, d0, e0)]
    ra = txb.optimize_b_batch(costs, coeff, a[0], a[1], a[2], s, t, bd, 60000, deq, 0, 1, 0, ctx,
                              77)
    tm = (m, im) if t >= 9 else (None, None)
    rb = qm.optimize_b_qm_batch(costs, coeff, b[0], b[1], b[2], s, t, bd, 60000, deq, tm[1],
                                tm[0], 0, 1, 0, ctx, 77)
    torch.cuda.synchronize()
    for u, v in zip(a + list(ra), b + list(rb)):
        eq(u, v)


def test_satd_gate_with_matrices_picks_the_helper_outputs(X):
    """SATD_GATE with both matrices: per block the FP or B helper output its
    own flags name (the gate reads the raw coefficients and does not change)."""
    torch, L, qm = X.torch, X.L, X.qm
    s, t, bd = 1, 0, 8
    rows = [g for g in X.rows("q") if g["tx_size"] == s and g["bd"] == bd]
    coeff = torch.stack([X.blk("q_coeff", g) for g in rows])
    m, im = X.tabs.views(0, 0, s)
    pq = X.plane_quant(bd, 120)
    qstep = int(pq.dequant[1]) >> 3
    gate = qm.av1_quant_qm_batch(coeff, s, t, bd, pq, L.AV1_QUANT_SATD_GATE, m, im, 2, 0, 23, qstep)
    flat = L.av1_quant_batch(coeff, s, t, bd, pq, L.AV1_QUANT_SATD_GATE, 0, 23, qstep)
    fp = qm.av1_quant_qm_batch(coeff, s, t, bd, pq, L.AV1_QUANT_FP, m, im, 2)
    b = qm.av1_quant_qm_batch(coeff, s, t, bd, pq, L.AV1_QUANT_B, m, im, 2)
    torch.cuda.synchronize()
    fl = gate[3].cpu().numpy()
    np.testing.assert_array_equal(fl, flat[3].cpu().numpy())
    assert set((fl >> 1).tolist()) == {0, 1}  # both outcomes occur
    for k in (0, 1, 2, 4, 5):
        want = np.where((fl >> 1 == 0).reshape([-1] + [1] * (gate[k].dim() - 1)),
                        fp[k].cpu().numpy(), b[k].cpu().numpy())
        np.testing.assert_array_equal(gate[k].cpu().numpy(), want)


@pytest.mark.parametrize("form,hbd,ls", [(0, 0, 0), (0, 1, 1), (1, 0, 2), (1, 1, 0), (0, 1, 2),
                                         (1, 1, 1)])
def test_free_int16_parameters_and_the_dequant_wrap(X, form, hbd, ls):
    """Any int16 tables (negative quant included) and weights up to 255: the
    level times the weighted dequantizer passes 2^31 and wraps as the
    reference's int multiply does.  Against tests/_qmref.py."""
    torch, qm = X.torch, X.qm
    rng = np.random.default_rng(100 * form + 10 * hbd + ls)
    n, nb = 64, 5
    scan_h = X.L.scan_order(1, 0)[0]
    wt = rng.integers(1, 256, n).astype(np.uint8)
    iwt = np.full(n, 255, np.uint8)
    wrapped = 0
    for case in range(4):
        lim = 1 << (15 if not hbd else 19)
        c = rng.integers(-lim, lim, (nb, n)).astype(np.int32)
        c[1] >>= 6
        c[2, 1:] = 0
        qp = X.L.QuantParams()
        t = {"zbin": rng.integers(-400, 3000, 2), "round": rng.integers(-300, 3000, 2),
             "quant": np.array([32767, 30000 if case else -30000]),
             "quant_shift": rng.integers(1 << 13, 1 << 15, 2),
             "dequant": np.array([32767, 32000])}
        if case == 3:
            t = {k: rng.integers(-32768, 32768, 2) for k in t}
        for name, v in t.items():
            setattr(qp, name, (ctypes.c_int16 * 2)(int(v[0]), int(v[1])))
        q, dq, eob = qm.quantize_qm_batch(
            torch.from_numpy(c).cuda(), torch.from_numpy(scan_h).cuda(), ls, qp,
            torch.from_numpy(wt).cuda(), torch.from_numpy(iwt).cuda(), 10 if hbd else 8, form)
        torch.cuda.synchronize()
        for b in range(nb):
            if form == 0:
                want = R.quantize_fp(c[b], t["round"], t["quant"], t["dequant"], scan_h, wt, iwt,
                                     ls, hbd)
            else:
                want = R.quantize_b(c[b], t["zbin"], t["round"], t["quant"], t["quant_shift"],
                                    t["dequant"], scan_h, wt, iwt, ls, hbd)
            np.testing.assert_array_equal(q[b].cpu().numpy(), want[0], "case %d block %d" % (case, b))
            np.testing.assert_array_equal(dq[b].cpu().numpy(), want[1], "case %d block %d" % (case, b))
            assert int(eob[b]) & 0xFFFF == want[2]
            dqw = (int(t["dequant"][1]) * 255 + 16) >> 5
            wrapped += int(np.abs(want[0].astype(np.int64)).max() * abs(dqw) >= 1 << 31)
    assert wrapped > 0


def test_skip_mode_measures_the_dqcoeff_it_finds(X):
    """AV1_QUANT_SKIP leaves qcoeff / dqcoeff / eob as they are
    (AV1_XFORM_QUANT_SKIP_QUANT); with a dist_mode it is dist_block_tx_domain
    of the buffers' contents: the fixture's figures on the fixture's dqcoeff."""
    torch, L, qm = X.torch, X.L, X.qm
    rows = X.rows("q")[::7]
    for g in rows:
        m, im = X.views(g)
        pq = X.plane_quant(g["bd"], g["qindex"])
        coeff = X.blk("q_coeff", g).reshape(1, -1).clone()
        qc = X.blk("q_qcoeff", g).reshape(1, -1).clone()
        dq = X.blk("q_dqcoeff", g).reshape(1, -1).clone()
        eob = torch.tensor([g["eob"]], dtype=torch.int16, device="cuda")
        for dist_mode in (1, 2):
            r = qm.av1_quant_qm_batch(coeff, g["tx_size"], g["tx_type"], g["bd"], pq,
                                      L.AV1_QUANT_SKIP, m, im, dist_mode, out=(qc, dq, eob))
            torch.cuda.synchronize()
            want = (g["dist%d" % dist_mode], g["sse%d" % dist_mode])
            assert (int(r[4][0]), int(r[5][0])) == want, (g, dist_mode)
            assert int(r[3][0]) == L.AV1_QUANT_SKIP << 1
        np.testing.assert_array_equal(qc[0].cpu().numpy(), X.host("q_qcoeff", g))
        np.testing.assert_array_equal(dq[0].cpu().numpy(), X.host("q_dqcoeff", g))
        assert int(eob[0]) == g["eob"]
    assert len(rows) >= 70


def test_twice_into_the_same_buffers(X):
    torch, L, qm = X.torch, X.L, X.qm
    s, t, bd = 3, 0, 10
    rows = [g for g in X.rows("q") if g["tx_size"] == s and g["bd"] == bd][:9]
    coeff = torch.stack([X.blk("q_coeff", g) for g in rows])
    m, im = X.tabs.views(0, 1, s)
    pq = X.plane_quant(bd, 120)
    out = None
    res = []
    for _ in range(2):
        r = qm.av1_quant_qm_batch(coeff, s, t, bd, pq, L.AV1_QUANT_B, m, im, 2, out=out)
        torch.cuda.synchronize()
        out = r[:3]
        res.append([x.cpu().numpy().copy() for x in r])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def _raw_calls(X, which, nblocks=1, tx_size=0, bd=8, dist_mode=0, with_dist=True):
    """One raw call of each named batch entry point with arguments that must
    launch nothing, on sentinel-filled outputs; returns the codes and whether
    any output changed."""
    torch, L = X.torch, X.L
    lib = L.lib()
    vp = ctypes.c_void_p
    n = 16
    c = torch.zeros((1, n), dtype=torch.int32, device="cuda")
    outs = [torch.full((1, n), 77, dtype=torch.int32, device="cuda") for _ in range(2)]
    eob = torch.full((1,), 7, dtype=torch.int16, device="cuda")
    d64 = [torch.full((1,), 77, dtype=torch.int64, device="cuda") for _ in range(2)]
    rate = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    m = torch.full((n,), 32, dtype=torch.uint8, device="cuda")
    scan = X.scan(0, 0)
    pq = X.plane_quant(8, 120)
    qp = X.quant_params(8, 120, 0)
    costs = X.txb.CoeffCosts(np.full(X.txb.COEFF_COSTS_CELLS, 100, np.int32))
    deq = np.array([8, 8], np.int16)
    p = lambda t: vp(t.data_ptr())
    calls = {
        "facade": lambda: lib.lavish_av1_quant_qm_batch(
            p(c), nblocks, tx_size, 0, bd, ctypes.byref(pq), 0, 0, 0xFFFFFFFF, 0, None, p(m), p(m),
            dist_mode, p(outs[0]), p(outs[1]), p(eob), None, p(d64[0]) if with_dist else None,
            p(d64[1]) if with_dist else None, None),
        "quantize": lambda: lib.lavish_quantize_qm_batch(
            p(c), n, nblocks, p(scan), None, 0, bd, 0, ctypes.byref(qp), p(m), p(m), p(outs[0]),
            p(outs[1]), p(eob), None),
        "block_error": lambda: lib.lavish_block_error_qm_batch(
            p(c), p(c), n, nblocks, p(m), p(scan), p(d64[0]), p(d64[1]), None),
        "trellis": lambda: lib.lavish_optimize_b_qm_batch(
            p(costs.t), p(c), p(outs[0]), p(outs[1]), p(eob), nblocks, 0, tx_size, 0, bd, 1, 100,
            0, deq.ctypes.data_as(vp), p(m), p(m), None, 0, p(rate), None, None),
    }
    codes = {k: calls[k]() for k in which}
    torch.cuda.synchronize()
    touched = any(int((t != 77).sum()) for t in outs + [rate] + d64) or int(eob[0]) != 7
    return codes, touched


def test_nblocks_zero_returns_zero(X):
    codes, touched = _raw_calls(X, ("facade", "quantize", "block_error", "trellis"), nblocks=0)
    assert codes == {"facade": 0, "quantize": 0, "block_error": 0, "trellis": 0}
    assert not touched
    assert X.L.status()[0] == 0


def test_bad_arguments_are_refused(X):
    codes, touched = _raw_calls(X, ("facade", "trellis"), tx_size=19)
    assert codes == {"facade": -1, "trellis": -1} and not touched
    codes, touched = _raw_calls(X, ("facade", "quantize", "trellis"), bd=9)
    assert codes == {"facade": -2, "quantize": -4, "trellis": -4} and not touched
    codes, touched = _raw_calls(X, ("facade",), dist_mode=3)
    assert codes == {"facade": -5} and not touched
    for mode in (1, 2):
        codes, touched = _raw_calls(X, ("facade",), dist_mode=mode, with_dist=False)
        assert codes == {"facade": -6} and not touched
    # refused calls write nothing: the facade's outputs of a refused call alone
    lib, torch = X.L.lib(), X.torch
    out = torch.full((16,), 77, dtype=torch.int32, device="cuda")
    pq = X.plane_quant(8, 120)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for args in ((19, 8, 0), (0, 9, 0), (0, 8, 3), (0, 8, 1)):
        rc = lib.lavish_av1_quant_qm_batch(p(out), 1, args[0], 0, args[1], ctypes.byref(pq), 0, 0,
                                           0xFFFFFFFF, 0, None, None, None, args[2], p(out),
                                           p(out), p(out), None, None, None, None)
        assert rc < 0
    torch.cuda.synchronize()
    assert int((out != 77).sum()) == 0
    with pytest.raises(ValueError, match="rc=-2"):
        X.qm.av1_quant_qm_batch(torch.zeros((1, 16), dtype=torch.int32, device="cuda"), 0, 0, 9,
                                pq, 0)
    assert X.L.status()[0] == 0
