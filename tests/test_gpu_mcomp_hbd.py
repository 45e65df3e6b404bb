"""GPU parity of the high-bit-depth full-pel and sub-pel search batches
(csrc/mcomp_hbd.hip and csrc/subpel_hbd.hip through lavish_dsp.motion), every
record field compared with equality, outputs into poisoned buffers:
* every case of tests/golden/fix_mcomp_hbd.npz (av1_full_pixel_search and the
  three sub-pel searches executed from the reference with the high-bit-depth
  members) through both entry points against the fixture directly -- the
  sub-pel call chained on the device results and cost lists, and again from
  the fixture's starts and cost lists;
* all 22 block sizes at 10 bits, one NSTEP job each and its sub-pel search,
  against tests/_hbdsearch_ref.py (the size dispatch and the uncached path);
* 1, 5 and 9 jobs at 16x16 (partial workgroups);
* the hard cases: 12-bit all-maximum against all-zero at 128x128, noise with
  the low bits set at every depth, windows of one row / one column and a
  start outside the window, a high-lambda ENTROPY job, the downsampled SAD on
  both sides of its recheck at 16x16 and 64x16;
* the return codes, with the output left untouched."""
import ctypes

import numpy as np
import pytest

import _compsearch_ref as S
import _compsubpel_ref as CS
import _hbdsearch_ref as H
import _mvextremes as X

pytestmark = pytest.mark.gpu

METHODS = {H.DIAMOND: "diamond", H.NSTEP: "nstep", H.NSTEP_8PT: "nstep_8pt"}
SP_METHODS = {H.TREE: "tree", H.PRUNED: "pruned", H.PRUNED_MORE: "pruned_more"}
ALL_SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16),
             (32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (4, 16),
             (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.motion as M
    return M


@pytest.fixture(scope="module")
def F():
    return H.load_fixture()


class Dev:
    """Device planes and cost tables, each uploaded once."""

    def __init__(self, M):
        import torch
        self.M, self.torch = M, torch
        self.planes = {}
        self.costs = {hp: M.MvCosts(*M.default_mv_cost_tables(bool(hp)), device="cuda")
                      for hp in (0, 1)}

    def put(self, key, src, refs):
        if key not in self.planes:
            up = lambda a: self.torch.from_numpy(np.array(a).view(np.int16)).cuda()
            self.planes[key] = (src.reshape(-1), refs.reshape(-1), up(src), up(refs))
        return self.planes[key]

    def kind(self, kind, bd, bw=16, bh=16):
        return self.put(H.plane_key(kind, bd, bw, bh), *H.planes(kind, bd, bw, bh))

    def cost(self, ctype, epb, spb, hp):
        if ctype == X.ENTROPY:
            return self.costs[int(bool(hp))].cost_params(spb, epb, self.M.MV_COST_ENTROPY)
        return self.M.l1_cost_params(ctype)

    def poisoned(self, nbytes):
        return self.torch.full((nbytes,), 0x55, dtype=self.torch.uint8, device="cuda")

    def fullpel(self, P, bw, bh, bd, jobs, cost, method, step_param, skip=False, use_cl=True):
        """One full-pel call into poisoned outputs: (device result bytes,
        device cost lists or None, [n, 5] results, [n, 5] cost lists)."""
        M = self.M
        n = len(jobs)
        out = self.poisoned(n * M.RESULT_DTYPE.itemsize)
        cl = self.torch.full((n, 5), 0x55555555, dtype=self.torch.int32, device="cuda")
        res, cls = M.highbd_full_pixel_search_batch(
            P[2], P[3], bw, bh, M.to_device(jobs), cost, bit_depth=bd, method=METHODS[method],
            step_param=step_param, use_downsampled_sad=bool(skip), cost_list=bool(use_cl),
            out=out, cost_lists=cl if use_cl else None)
        self.torch.cuda.synchronize()
        r = M.results_numpy(res)
        got = np.stack([r[f].astype(np.int64) for f in H.FULL_FIELDS], 1)
        return res, cls, got, (cls.cpu().numpy().astype(np.int64) if use_cl else None)

    def subpel(self, P, bw, bh, bd, sjobs, cost, method, forced_stop, allow_hp, iters,
               fullpel=None, cost_lists=None):
        M = self.M
        out = self.poisoned(len(sjobs) * M.SUBPEL_RESULT_DTYPE.itemsize)
        M.highbd_find_best_sub_pixel_tree_batch(
            P[2], P[3], bw, bh, M.to_device(sjobs), cost, bit_depth=bd,
            method=SP_METHODS[method], forced_stop=forced_stop, allow_hp=bool(allow_hp),
            iters_per_step=iters, fullpel=fullpel, cost_lists=cost_lists, out=out)
        self.torch.cuda.synchronize()
        r = M.subpel_results_numpy(out)
        return np.stack([r[f].astype(np.int64) for f in H.SUB_FIELDS], 1)


@pytest.fixture(scope="module")
def dev(M):
    return Dev(M)


def compare(bad, msg, fields, got, exp):
    exp = np.asarray(exp, np.int64)
    for i, f in enumerate(fields):
        if not np.array_equal(got[:, i], exp[:, i]):
            j = int(np.flatnonzero(got[:, i] != exp[:, i])[0])
            bad.append("%s %s: job %d got %d expected %d (%d differ)" % (
                msg, f, j, got[j, i], exp[j, i], int((got[:, i] != exp[:, i]).sum())))


CL_FIELDS = ["cl0", "cl1", "cl2", "cl3", "cl4"]


# ------------------------------------------------- the reference's own rows --
def test_every_fixture_case_through_both_entry_points(M, dev, F):
    import torch
    bad, n = [], 0
    for g in H.fixture_groups(F):
        p, J = g.prm, g.J
        P = dev.put("fix_" + g.plane, F["src__" + g.plane], F["refs__" + g.plane])
        msg = "case %d %r" % (g.index, p)
        cost = dev.cost(p["cost"], p["error_per_bit"], p["sad_per_bit"], p["hp_tables"])
        res, cls, got, gcl = dev.fullpel(P, p["bw"], p["bh"], p["bd"], g.jobs, cost, p["method"],
                                         p["step_param"], p["skip"], p["use_cl"])
        compare(bad, msg, H.FULL_FIELDS, got, g.rows[:, J["best_row"]:J["searches"] + 1])
        wcl = g.rows[:, J["cl0"]:J["cl4"] + 1]
        if p["use_cl"]:
            compare(bad, msg, CL_FIELDS, gcl, wcl)
        scost = dev.cost(p["cost"], p["error_per_bit"], 0, p["sp_allow_hp"])
        want = g.rows[:, J["sp_best_row"]:J["sp_sse"] + 1]
        sp = (p["sp_method"], p["sp_forced_stop"], p["sp_allow_hp"], p["sp_iters"])
        # chained: the device's own full-pel records and cost lists, the
        # jobs' start fields poisoned
        sj = g.sjobs.copy()
        sj["start_row"] = sj["start_col"] = 0x5555
        chained = dev.subpel(P, p["bw"], p["bh"], p["bd"], sj, scost, *sp, fullpel=res,
                             cost_lists=cls if p["sp_use_cl"] and p["use_cl"] else None)
        compare(bad, msg + " chained", H.SUB_FIELDS, chained, want)
        # from the fixture's starts and cost lists
        fcl = torch.from_numpy(wcl.astype(np.int32)).cuda() if p["sp_use_cl"] else None
        direct = dev.subpel(P, p["bw"], p["bh"], p["bd"], g.sjobs, scost, *sp, cost_lists=fcl)
        compare(bad, msg + " direct", H.SUB_FIELDS, direct, want)
        n += len(got)
    assert n == len(F["rows"]) >= 80
    assert not bad, "\n".join(bad[:10])


# ----------------------------------------------------------------- dispatch --
def restated(P, bw, bh, bd, jobs, cost_t, method, step_param, skip, sp, ref_mv):
    """The restatement of a full-pel call and of the sub-pel call chained on
    it: (full-pel [n, 5], cost lists, sub-pel jobs, sub-pel [n, 5])."""
    ctype, epb, spb, hp = cost_t
    exp, cl = H.run_fullpel(P[0], P[1], X.STRIDE, bw, bh, jobs, S.cost_of(ctype, epb, spb, hp),
                            bd, method, step_param, skip)
    sj = CS.subpel_records(jobs, bw, bh)
    spm, fstop, allow_hp, iters = sp
    sexp = H.run_subpel(P[0], P[1], X.STRIDE, bw, bh, sj, S.cost_of(ctype, epb, 0, allow_hp), bd,
                        spm, fstop, bool(allow_hp), iters, fullpel=exp[:, :2], cost_lists=cl)
    return exp, cl, sj, sexp


def check_pair(dev, bad, msg, P, bw, bh, bd, jobs, cost_t, method, step_param, skip=False,
               sp=(H.PRUNED_MORE, 0, 1, 2), ref_mv=(0, 0)):
    exp, cl, sj, sexp = restated(P, bw, bh, bd, jobs, cost_t, method, step_param, skip, sp, ref_mv)
    ctype, epb, spb, hp = cost_t
    res, cls, got, gcl = dev.fullpel(P, bw, bh, bd, jobs, dev.cost(ctype, epb, spb, hp), method,
                                     step_param, skip, True)
    compare(bad, msg, H.FULL_FIELDS, got, exp)
    compare(bad, msg, CL_FIELDS, gcl, cl)
    sgot = dev.subpel(P, bw, bh, bd, sj, dev.cost(ctype, epb, 0, sp[2]), *sp, fullpel=res,
                      cost_lists=cls)
    compare(bad, msg + " sub-pel", H.SUB_FIELDS, sgot, sexp)
    return exp, sexp


LOW = (X.ENTROPY, X.LOW_LAMBDA[0], X.LOW_LAMBDA[1], 1)


def test_every_block_size_at_10_bits(dev):
    bad = []
    P = dev.kind("smooth", 10)
    for i, (bw, bh) in enumerate(ALL_SIZES):
        jobs = X.frame(bw, bh, (0, 0), (1 + i % 3, -2 + i % 4))
        jobs = jobs[[(5 * i) % len(jobs)]]
        check_pair(dev, bad, "%dx%d" % (bw, bh), P, bw, bh, 10, jobs, LOW, H.NSTEP, 9,
                   sp=((H.PRUNED_MORE, H.TREE, H.PRUNED)[i % 3], 0, 1, 1 + i % 2))
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("njobs", [1, 5, 9])
def test_partial_workgroups(dev, njobs):
    bad = []
    P = dev.kind("smooth", 10)
    jobs = X.spread(X.frame(16, 16, (13, -21), (2, -3)), njobs, njobs)[:njobs]
    assert len(jobs) == njobs
    check_pair(dev, bad, "%d jobs" % njobs, P, 16, 16, 10, jobs, LOW, H.NSTEP, 8)
    assert not bad, "\n".join(bad[:10])


# --------------------------------------------------------------- hard cases --
def test_all_maximum_against_all_zero_at_12_bits_128x128(dev):
    bad = []
    for kind in ("flat_255_0", "flat_0_255"):
        P = dev.kind(kind, 12)
        jobs = X.frame(128, 128)[:1]
        exp, _ = check_pair(dev, bad, kind, P, 128, 128, 12, jobs, LOW, H.NSTEP, 10)
        # sse = 4095^2 * 2^14 needs 38 bits; rounded by 8 it is the variance's
        # first term, and sum^2 / N takes all of it away
        assert sorted({int(v) for a in P[:2] for v in (a.min(), a.max())}) == [0, 4095]
        assert exp[0, 2] == H.FullEnv(P[0], P[1], X.STRIDE, 128, 128, jobs[0],
                                      S.cost_of(*LOW), 12).mverr(exp[0, 0], exp[0, 1])
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_noise_with_the_low_bits_set(dev, bd):
    bad = []
    P = dev.kind("noise", bd)
    for k, (bw, bh) in enumerate(((8, 8), (16, 16))):
        jobs = X.spread(X.frame(bw, bh, (13, -21), (1, -2)), 4, bd + k)
        check_pair(dev, bad, "%dx%d bd %d" % (bw, bh, bd), P, bw, bh, bd, jobs,
                   (X.ENTROPY, 37 + bd, 4, 0), (H.DIAMOND, H.NSTEP_8PT)[k], 5, ref_mv=(13, -21),
                   sp=(H.TREE, 0, 0, 2))
    assert not bad, "\n".join(bad[:10])


def test_narrowed_windows_and_a_start_outside(dev):
    bad = []
    P = dev.kind("periodic_2", 10)
    base = X.spread(X.frame(16, 16, (13, -21), (2, -3)), 3, 1)
    clamped = base.copy()
    clamped["row_max"] = np.minimum(clamped["row_max"], clamped["start_row"] - 2)
    clamped["col_min"] = np.maximum(clamped["col_min"], clamped["start_col"] + 3)
    for name, jobs in (("row", X.narrowed(base, "row", (3, -2))),
                       ("col", X.narrowed(base, "col", (3, -2))), ("clamped", clamped)):
        exp, _ = check_pair(dev, bad, name, P, 16, 16, 10, jobs, (X.L1, 37, 4, 0), H.NSTEP, 4,
                            ref_mv=(13, -21))
        assert (exp[:, 0] >= jobs["row_min"]).all() and (exp[:, 0] <= jobs["row_max"]).all()
        assert (exp[:, 1] >= jobs["col_min"]).all() and (exp[:, 1] <= jobs["col_max"]).all()
    assert not bad, "\n".join(bad[:10])


def test_high_lambda_entropy(dev):
    bad = []
    P = dev.kind("noise", 10)
    for epb, ref_mv, hp in X.HIGH_LAMBDA:
        jobs = X.spread(X.frame(8, 8, ref_mv, (0, 0)), 2, hp)
        if epb == X.HIGH_LAMBDA[0][0]:      # the rate it needs is (0, 0)'s alone
            jobs["ref_off"] = jobs["src_off"]
        check_pair(dev, bad, "epb %d" % epb, P, 8, 8, 10, jobs,
                   (X.ENTROPY, epb, X.SAD_PER_BIT_TOP, hp), H.DIAMOND, 6, ref_mv=ref_mv,
                   sp=(H.PRUNED_MORE, 0, hp, 1))
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("bw,bh", [(16, 16), (64, 16)])
def test_downsampled_sad_on_both_sides_of_the_recheck(dev, bw, bh):
    bad, redo = [], {}
    for kind in ("periodic_2", "stripes"):
        P = dev.kind(kind, 10)
        jobs = X.spread(X.frame(bw, bh, (0, 0), (1, 2)), 2, 3)
        check_pair(dev, bad, "%s %dx%d" % (kind, bw, bh), P, bw, bh, 10, jobs, LOW, H.NSTEP, 7,
                   skip=True)
        flags = []
        for jb in jobs:
            tr = {}
            H.full_pixel_search(H.FullEnv(P[0], P[1], X.STRIDE, bw, bh, jb, S.cost_of(*LOW), 10,
                                          True), H.NSTEP, 7, tr)
            flags.append(bool(tr["redo"]))
        redo[kind] = flags
    assert not any(redo["periodic_2"]) and all(redo["stripes"]), redo
    assert not bad, "\n".join(bad[:10])


# ------------------------------------------------------------- return codes --
def test_return_codes_leave_the_output_untouched(M, dev):
    import lavish_dsp
    L = lavish_dsp.lib()
    vp = ctypes.c_void_p
    P = dev.kind("smooth", 10)
    jobs = M.to_device(X.frame(16, 16)[:2])
    out = dev.poisoned(2 * 16)
    cl = dev.torch.full((2, 5), 0x55555555, dtype=dev.torch.int32, device="cuda")
    good = dev.cost(X.ENTROPY, 37, 4, 0)
    notab = M.MvCostParams(X.ENTROPY, 4, 37, 0)

    def full(w=16, h=16, bd=10, method=1, step=5, cost=good, src=True, o=True, njobs=2):
        return L.lavish_highbd_full_pixel_search_batch(
            vp(P[2].data_ptr()) if src else None, X.STRIDE, vp(P[3].data_ptr()), X.STRIDE, w, h,
            bd, vp(jobs.data_ptr()), njobs, method, step,
            ctypes.byref(cost) if cost is not None else None, 0,
            vp(out.data_ptr()) if o else None, vp(cl.data_ptr()), None)

    def sub(w=16, h=16, bd=10, method=2, fstop=0, iters=1, cost=good, src=True, o=True, njobs=2):
        return L.lavish_highbd_find_best_sub_pixel_tree_batch(
            vp(P[2].data_ptr()) if src else None, X.STRIDE, vp(P[3].data_ptr()), X.STRIDE, w, h,
            bd, vp(jobs.data_ptr()), None, njobs, method, fstop, 1, iters,
            ctypes.byref(cost) if cost is not None else None, None,
            vp(out.data_ptr()) if o else None, None)

    assert full(step=-1) == -1 and full(step=15) == -1 and full(method=2, step=16) == -1
    assert full(cost=None) == -2 and full(cost=notab) == -2
    assert full(w=12) == -3 and full(w=16, h=15) == -3
    assert full(method=5) == -4 and full(method=9) == -4 and full(method=3) == -4
    assert full(bd=9) == -7 and full(bd=16) == -7 and full(src=False) == -7
    assert full(o=False) == -7
    assert full(njobs=0, bd=9) == 0 and full(njobs=-1, w=12) == 0
    assert sub(fstop=4) == -1 and sub(cost=None) == -2 and sub(cost=notab) == -2
    assert sub(w=12) == -3 and sub(iters=3) == -4 and sub(method=3) == -6
    assert sub(bd=9) == -7 and sub(src=False) == -7 and sub(o=False) == -7
    assert sub(njobs=0, bd=9) == 0
    dev.torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x55).all() and (cl.cpu().numpy() == 0x55555555).all()
    # and the same buffers take a good call
    assert full() == 0 and sub() == 0
    dev.torch.cuda.synchronize()
    assert not (out.cpu().numpy() == 0x55).all()
