"""GPU parity of the high-bit-depth compound, masked and OBMC search batches
(csrc/mcomp_comp_hbd.hip and csrc/subpel_comp_hbd.hip through
lavish_dsp.motion), every record field compared with equality, outputs into
poisoned buffers:
* every case of tests/golden/fix_mcomp_comp_hbd.npz (the five searches
  executed from the reference with the high-bit-depth members) through the
  five entry points against the fixture directly -- the sub-pel calls chained
  on the device records for both start_from values followed by
  pick_lower_besterr, and again from the fixture's starts;
* all 22 block sizes at 10 bits, one NSTEP job per form with its sub-pel
  search, against tests/_hbdcomp_ref.py (the size dispatch, the LDS and L2
  paths on both sides of the 512-pixel cut-over);
* 1, 5 and 9 jobs at 16x16 (partial workgroups);
* the hard cases: 12-bit all-maximum against all-zero at 128x128 in every
  form, noise with the low bits set at every depth, windows of one row / one
  column and a start outside the window, a high-lambda ENTROPY job;
* the return codes, with the output left untouched."""
import ctypes

import numpy as np
import pytest

import _compsubpel_ref as CS
import _hbdcomp_ref as HC
import _hbdsearch_ref as H
import _mvextremes as X

pytestmark = pytest.mark.gpu

S, P_ = HC.S, HC.P
METHODS = {S.DIAMOND: "diamond", S.NSTEP: "nstep", S.NSTEP_8PT: "nstep_8pt"}
SP_METHODS = {CS.TREE: "tree", CS.PRUNED: "pruned", CS.PRUNED_MORE: "pruned_more"}
ALL_SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16),
             (32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (4, 16),
             (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
NONE_ROW = [CS.NO_SEARCH[f] for f in HC.SUB_FIELDS]


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.motion as M
    return M


@pytest.fixture(scope="module")
def F():
    return HC.load_fixture()


class Pools:
    """The four invariant pools, on the host and on the device."""

    def __init__(self, torch, second, mask, wsrc, omask, mask_stride=0):
        self.second, self.mask = np.asarray(second, np.uint16), np.asarray(mask, np.uint8)
        self.wsrc, self.omask = np.asarray(wsrc, np.int32), np.asarray(omask, np.int32)
        self.mask_stride = mask_stride
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.d_second = up(self.second.view(np.int16))
        self.d_mask, self.d_wsrc, self.d_omask = up(self.mask), up(self.wsrc), up(self.omask)

    def host(self, mask_stride=None):
        return dict(second=self.second, mask=self.mask, wsrc=self.wsrc, omask=self.omask,
                    mask_stride=self.mask_stride if mask_stride is None else mask_stride)


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

    def full(self, search, form, P, bw, bh, bd, cjobs, cost, pools, method=S.DIAMOND,
             step_param=0, fast=0, mask_stride=None):
        """One full-pel call into a poisoned output: (device record bytes,
        [n, 6] results)."""
        M = self.M
        out = self.poisoned(len(cjobs) * M.COMP_RESULT_DTYPE.itemsize)
        jobs = M.to_device(cjobs)
        ms = pools.mask_stride if mask_stride is None else mask_stride
        if search == HC.OBMC:
            M.highbd_obmc_full_pixel_search_batch(
                P[3], X.STRIDE, bw, bh, jobs, cost, pools.d_wsrc, pools.d_omask, bit_depth=bd,
                method=METHODS[method], step_param=step_param, fast_obmc_search=bool(fast),
                out=out)
        elif search == HC.REFINE8:
            M.highbd_refining_search_8p_batch(
                P[2], P[3], bw, bh, jobs, cost, None if form == HC.PLAIN else pools.d_second,
                pools.d_mask if form == HC.MASK else None, ms, bit_depth=bd, out=out)
        else:
            M.highbd_comp_full_pixel_search_batch(
                P[2], P[3], bw, bh, jobs, cost, pools.d_second,
                pools.d_mask if form == HC.MASK else None, ms, bit_depth=bd,
                method=METHODS[method], step_param=step_param, out=out)
        self.torch.cuda.synchronize()
        r = M.comp_results_numpy(out)
        return out, np.stack([r[f].astype(np.int64) for f in HC.FULL_FIELDS], 1)

    def sub(self, form, P, bw, bh, bd, csj, cost, pools, method, forced_stop, allow_hp, iters,
            fullpel=None, start_from=0, mask_stride=None):
        """One sub-pel call (form: _compsubpel_ref's AVG / MASK / OBMC) into a
        poisoned output: (device record bytes, [n, 5] results)."""
        M = self.M
        out = self.poisoned(len(csj) * M.SUBPEL_RESULT_DTYPE.itemsize)
        jobs = M.to_device(csj)
        ms = pools.mask_stride if mask_stride is None else mask_stride
        if form == CS.OBMC:
            M.highbd_obmc_find_best_sub_pixel_tree_batch(
                P[3], X.STRIDE, bw, bh, jobs, cost, pools.d_wsrc, pools.d_omask, bit_depth=bd,
                forced_stop=forced_stop, allow_hp=bool(allow_hp), iters_per_step=iters,
                fullpel=fullpel, out=out)
        else:
            M.highbd_comp_find_best_sub_pixel_tree_batch(
                P[2], P[3], bw, bh, jobs, cost, pools.d_second,
                pools.d_mask if form == CS.MASK else None, ms, bit_depth=bd,
                method=SP_METHODS[method], forced_stop=forced_stop, allow_hp=bool(allow_hp),
                iters_per_step=iters, fullpel=fullpel, start_from=start_from, out=out)
        self.torch.cuda.synchronize()
        return out, self.sub_numpy(out)

    def sub_numpy(self, out):
        r = self.M.subpel_results_numpy(out)
        return np.stack([r[f].astype(np.int64) for f in HC.SUB_FIELDS], 1)


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


# ------------------------------------------------- the reference's own rows --
def test_every_fixture_case_through_the_five_entry_points(M, dev, F):
    bad, n, nsub = [], 0, 0
    pools = Pools(dev.torch, F["second"], F["mask"], F["wsrc"], F["omask"])
    for g in HC.fixture_groups(F):
        p, J = g.prm, g.J
        bw, bh, bd, ms = p["bw"], p["bh"], p["bd"], p["mask_stride"]
        Pl = dev.put("fixc_" + g.plane, F["src__" + g.plane], F["refs__" + g.plane])
        msg = "case %d %r" % (g.index, p)
        cost = dev.cost(p["cost"], p["error_per_bit"], p["sad_per_bit"], p["hp_tables"])
        res, got = dev.full(p["search"], p["form"], Pl, bw, bh, bd, g.cjobs, cost, pools,
                            p["method"], p["step_param"], p["fast_obmc"], ms)
        compare(bad, msg, HC.FULL_FIELDS, got, g.rows[:, J["best_row"]:J["steps"] + 1])
        n += len(got)
        if not p["has_sp"]:
            continue
        scost = dev.cost(p["cost"], p["error_per_bit"], 0, p["sp_allow_hp"])
        sp = (p["sp_method"], p["sp_forced_stop"], p["sp_allow_hp"], p["sp_iters"])
        form = HC.sp_form(p)
        want0, want1 = HC.sp_rows(g, 0), HC.sp_rows(g, 1)
        # chained: the device's own full-pel records, the jobs' start fields
        # poisoned
        sj = g.sjobs.copy()
        sj["base"]["start_row"] = sj["base"]["start_col"] = 0x5555
        out0, c0 = dev.sub(form, Pl, bw, bh, bd, sj, scost, pools, *sp, fullpel=res,
                           mask_stride=ms)
        compare(bad, msg + " chained 0", HC.SUB_FIELDS, c0, want0)
        if p["search"] == HC.COMP:
            out1, c1 = dev.sub(form, Pl, bw, bh, bd, sj, scost, pools, *sp, fullpel=res,
                               start_from=1, mask_stride=ms)
            compare(bad, msg + " chained 1", HC.SUB_FIELDS, c1, want1)
            picked = dev.sub_numpy(M.pick_lower_besterr(out0, out1))
            compare(bad, msg + " picked", HC.SUB_FIELDS, picked, CS.pick_lower(want0, want1))
        # from the fixture's starts
        for which, want in ((0, want0), (1, want1)):
            keep = np.flatnonzero(want[:, 2] != HC.INT_MAX) if which else np.arange(len(want))
            if which and (p["search"] != HC.COMP or not len(keep)):
                continue
            dj = g.sjobs[keep].copy()
            a = J["second_row"] if which else J["best_row"]
            dj["base"]["start_row"] = 8 * g.rows[keep, a]
            dj["base"]["start_col"] = 8 * g.rows[keep, a + 1]
            _, d = dev.sub(form, Pl, bw, bh, bd, dj, scost, pools, *sp, mask_stride=ms)
            compare(bad, msg + " direct %d" % which, HC.SUB_FIELDS, d, want[keep])
            nsub += len(keep)
    assert n == len(F["rows"]) >= 150 and nsub > n
    assert not bad, "\n".join(bad[:10])


# ----------------------------------------------------------------- dispatch --
def make_pools(dev, Pl, bw, bh, bd, jobs, seed, second="near", mask="random", obmc="near"):
    """Invariant blocks for JOB_DTYPE records `jobs`: (Pools, second_off,
    mask_off) -- the offsets serve the compound forms and, as wsrc / mask
    offsets, OBMC (each pool holds one block per job at the same index)."""
    rng = np.random.default_rng(seed)
    n, top, ms = bw * bh, (1 << bd) - 1, bw + 3
    idx = np.arange(bh)[:, None] * X.STRIDE + np.arange(bw)[None, :]
    sec, msk, ws, om = [], [], [], []
    for jb in jobs:
        src = Pl[0][int(jb["src_off"]) + idx].astype(np.int64)
        if second == "max":
            sec.append(np.full(n, top))
        else:
            sec.append(np.clip(src + rng.integers(-3, 4, src.shape), 0, top).reshape(-1))
        m = rng.integers(0, 65, (bh, ms))
        msk.append(m.reshape(-1))
        if obmc == "full":       # wsrc 4095 x 4096 against mask 4096 (and a reference of 0)
            ws.append(np.full(n, top * 4096))
            om.append(np.full(n, 4096))
        else:
            mm = rng.integers(1024, 4097, n)
            nb = np.clip(src.reshape(-1) + rng.integers(-3, 4, n), 0, top)
            ws.append(src.reshape(-1) * 4096 - nb * (4096 - mm))
            om.append(mm)
    k = np.arange(len(jobs))
    # (an odd lead-in: the second_pred blocks are addressed at any element offset)
    pools = Pools(dev.torch, np.concatenate([[7]] + sec), np.concatenate(msk),
                  np.concatenate([[0] * n] + ws), np.concatenate([[0] * n] + om), ms)
    return pools, dict(avg=(1 + k * n, 0 * k), mask=(1 + k * n, k * bh * ms),
                       obmc=(n + k * n, n + k * n))


def check_forms(dev, bad, msg, Pl, bw, bh, bd, jobs, cost_t, method, step_param,
                sp=(CS.PRUNED_MORE, 0, 1, 2), seed=1, forms=("avg", "mask", "obmc"), invert=0,
                refine=True, obmc_sub=True, **pool_kw):
    """The searches of every form over `jobs`, each with the sub-pel search
    chained on its device records, against the restatement; returns the
    restated full-pel rows per form."""
    M = dev.M
    ctype, epb, spb, hp = cost_t
    pools, offs = make_pools(dev, Pl, bw, bh, bd, jobs, seed, **pool_kw)
    hc, hs = S.cost_of(ctype, epb, spb, hp), S.cost_of(ctype, epb, 0, sp[2])
    dc, ds = dev.cost(ctype, epb, spb, hp), dev.cost(ctype, epb, 0, sp[2])
    sjb = CS.subpel_records(jobs, bw, bh)
    spm, fstop, allow_hp, iters = sp
    out = {}
    for name in forms:
        so, mo = offs[name]
        cj = M.comp_jobs(jobs, so, mo, invert)
        csj = M.comp_subpel_jobs(sjb, so, mo, invert)
        runs = {"avg": [(HC.COMP, HC.AVG, 0)], "mask": [(HC.COMP, HC.MASK, 0)],
                "obmc": [(HC.OBMC, HC.PLAIN, 0), (HC.OBMC, HC.PLAIN, 1)]}[name]
        if refine and name != "obmc":
            runs.append((HC.REFINE8, runs[0][1], 0))
        for search, form, fast in runs:
            tag = "%s %s search %d fast %d" % (msg, name, search, fast)
            exp = HC.run_fullpel(search, form, Pl[0], Pl[1], X.STRIDE, bw, bh, cj, hc, bd, method,
                                 step_param, fast, **pools.host())
            res, got = dev.full(search, form, Pl, bw, bh, bd, cj, dc, pools, method, step_param,
                                fast)
            compare(bad, tag, HC.FULL_FIELDS, got, exp)
            out[(name, search, fast)] = exp
            if search == HC.OBMC and (ctype == X.L1 or not obmc_sub):
                continue
            sform = CS.OBMC if search == HC.OBMC else HC.SP_FORM[form]
            for which in ((0, 1) if search == HC.COMP else (0,)):
                sexp = HC.run_subpel(sform, Pl[0], Pl[1], X.STRIDE, bw, bh, csj, hs, bd, spm,
                                     fstop, bool(allow_hp), iters, fullpel=exp[:, :4],
                                     start_from=which, **pools.host())
                _, sgot = dev.sub(sform, Pl, bw, bh, bd, csj, ds, pools, spm, fstop, allow_hp,
                                  iters, fullpel=res, start_from=which)
                compare(bad, tag + " sub-pel %d" % which, HC.SUB_FIELDS, sgot, sexp)
    # the plain 8-point refinement (no second_pred)
    if refine:
        cj = M.comp_jobs(jobs, 0, 0, 0)
        exp = HC.run_fullpel(HC.REFINE8, HC.PLAIN, Pl[0], Pl[1], X.STRIDE, bw, bh, cj, hc, bd)
        _, got = dev.full(HC.REFINE8, HC.PLAIN, Pl, bw, bh, bd, cj, dc, pools)
        compare(bad, msg + " plain refine", HC.FULL_FIELDS, got, exp)
    return out


LOW = (X.ENTROPY, X.LOW_LAMBDA[0], X.LOW_LAMBDA[1], 1)


def test_every_block_size_at_10_bits(dev):
    bad = []
    Pl = dev.kind("smooth", 10)
    for i, (bw, bh) in enumerate(ALL_SIZES):
        jobs = X.frame(bw, bh, (0, 0), (1 + i % 3, -2 + i % 4))
        jobs = jobs[[(5 * i) % len(jobs)]]
        check_forms(dev, bad, "%dx%d" % (bw, bh), Pl, bw, bh, 10, jobs, LOW, S.NSTEP, 9,
                    sp=((CS.PRUNED_MORE, CS.TREE, CS.PRUNED)[i % 3], 0, 1, 1 + i % 2), seed=i,
                    invert=i % 2, refine=bw * bh in (512, 1024))
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("njobs", [1, 5, 9])
def test_partial_workgroups(dev, njobs):
    bad = []
    Pl = dev.kind("smooth", 10)
    jobs = X.spread(X.frame(16, 16, (13, -21), (2, -3)), njobs, njobs)[:njobs]
    assert len(jobs) == njobs
    check_forms(dev, bad, "%d jobs" % njobs, Pl, 16, 16, 10, jobs, LOW, S.NSTEP, 8, seed=njobs)
    assert not bad, "\n".join(bad[:10])


# --------------------------------------------------------------- hard cases --
def test_all_maximum_against_all_zero_at_12_bits_128x128(dev):
    bad = []
    jobs = X.frame(128, 128)[:1]
    # source 0, reference and second_pred 4095: the average and every blend
    # are 4095 against 0
    Pl = dev.kind("flat_0_255", 12)
    assert sorted({int(v) for a in Pl[:2] for v in (a.min(), a.max())}) == [0, 4095]
    out = check_forms(dev, bad, "max", Pl, 128, 128, 12, jobs, LOW, S.NSTEP, 10,
                      forms=("avg", "mask"), second="max")
    # OBMC: wsrc 4095 x 4096 and mask 4096 against a reference of 0
    Pz = dev.kind("flat_255_0", 12)
    assert int(Pz[1].max()) == 0
    out.update(check_forms(dev, bad, "max", Pz, 128, 128, 12, jobs, LOW, S.NSTEP, 10,
                           forms=("obmc",), obmc="full", refine=False))
    # sse = 4095^2 * 2^14 needs 38 bits; rounded by 8 it is the variance's
    # first term, and sum^2 / N takes all of it away: bestsme is the mv cost
    for key in (("avg", HC.COMP, 0), ("mask", HC.COMP, 0), ("obmc", HC.OBMC, 0)):
        e = HC.FullEnv(None, Pz[1], X.STRIDE, 128, 128, jobs[0], S.cost_of(*LOW), 12)
        assert out[key][0, 4] == e.mverr(out[key][0, 0], out[key][0, 1]), key
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_noise_with_the_low_bits_set(dev, bd):
    bad = []
    Pl = dev.kind("noise", bd)
    for k, (bw, bh) in enumerate(((8, 8), (16, 16))):
        jobs = X.spread(X.frame(bw, bh, (13, -21), (1, -2)), 4, bd + k)
        check_forms(dev, bad, "%dx%d bd %d" % (bw, bh, bd), Pl, bw, bh, bd, jobs,
                    (X.ENTROPY, 37 + bd, 4, 0), (S.DIAMOND, S.NSTEP_8PT)[k], 5,
                    sp=(CS.TREE, 0, 0, 2), seed=bd + k, invert=k)
    assert not bad, "\n".join(bad[:10])


def test_narrowed_windows_and_a_start_outside(dev):
    bad = []
    Pl = dev.kind("periodic_2", 10)
    base = X.spread(X.frame(16, 16, (13, -21), (2, -3)), 3, 1)
    clamped = base.copy()
    clamped["row_max"] = np.minimum(clamped["row_max"], clamped["start_row"] - 2)
    clamped["col_min"] = np.maximum(clamped["col_min"], clamped["start_col"] + 3)
    for name, jobs in (("row", X.narrowed(base, "row", (3, -2))),
                       ("col", X.narrowed(base, "col", (3, -2))), ("clamped", clamped)):
        out = check_forms(dev, bad, name, Pl, 16, 16, 10, jobs, (X.L1, 37, 4, 0), S.NSTEP, 4)
        for exp in out.values():
            assert (exp[:, 0] >= jobs["row_min"]).all() and (exp[:, 0] <= jobs["row_max"]).all()
            assert (exp[:, 1] >= jobs["col_min"]).all() and (exp[:, 1] <= jobs["col_max"]).all()
    assert not bad, "\n".join(bad[:10])


def test_high_lambda_entropy(dev):
    bad = []
    Pl = dev.kind("noise", 10)
    for epb, ref_mv, hp in X.HIGH_LAMBDA:
        jobs = X.spread(X.frame(8, 8, ref_mv, (0, 0)), 2, hp)
        if epb == X.HIGH_LAMBDA[0][0]:      # the rate it needs is (0, 0)'s alone
            jobs["ref_off"] = jobs["src_off"]
        # (the OBMC sub-pel search is left out: estimate_obmc_mvcost's int
        # product overflows at these lambdas in the reference itself)
        check_forms(dev, bad, "epb %d" % epb, Pl, 8, 8, 10, jobs,
                    (X.ENTROPY, epb, X.SAD_PER_BIT_TOP, hp), S.DIAMOND, 6,
                    sp=(CS.PRUNED_MORE, 0, hp, 1), obmc_sub=False)
    assert not bad, "\n".join(bad[:10])


# ------------------------------------------------------------- return codes --
def test_return_codes_leave_the_output_untouched(M, dev):
    import lavish_dsp
    L = lavish_dsp.lib()
    vp = ctypes.c_void_p
    Pl = dev.kind("smooth", 10)
    base = X.frame(16, 16)[:2]
    pools, offs = make_pools(dev, Pl, 16, 16, 10, base, 3)
    jobs = M.to_device(M.comp_jobs(base, *offs["mask"]))
    sjobs = M.to_device(M.comp_subpel_jobs(CS.subpel_records(base, 16, 16), *offs["mask"]))
    out = dev.poisoned(2 * 16)
    good = dev.cost(X.ENTROPY, 37, 4, 0)
    l1 = dev.cost(X.L1, 37, 4, 0)
    notab = M.MvCostParams(X.ENTROPY, 4, 37, 0)
    src, ref, o = vp(Pl[2].data_ptr()), vp(Pl[3].data_ptr()), vp(out.data_ptr())
    sec, msk = vp(pools.d_second.data_ptr()), vp(pools.d_mask.data_ptr())
    ws, om = vp(pools.d_wsrc.data_ptr()), vp(pools.d_omask.data_ptr())
    jp, sp = vp(jobs.data_ptr()), vp(sjobs.data_ptr())
    cb = lambda c: ctypes.byref(c) if c is not None else None

    def comp(w=16, h=16, bd=10, method=1, step=5, cost=good, s=src, njobs=2, ms=19):
        return L.lavish_highbd_comp_full_pixel_search_batch(
            s, X.STRIDE, ref, X.STRIDE, w, h, bd, jp, njobs, method, step, cb(cost), sec, msk, ms,
            o, None)

    def refine(w=16, h=16, bd=10, cost=good, s=src, njobs=2, second=sec, ms=19):
        return L.lavish_highbd_refining_search_8p_batch(
            s, X.STRIDE, ref, X.STRIDE, w, h, bd, jp, njobs, cb(cost), second, msk, ms, o, None)

    def obmc(w=16, h=16, bd=10, method=1, step=5, cost=good, w_=ws, njobs=2):
        return L.lavish_highbd_obmc_full_pixel_search_batch(
            ref, X.STRIDE, w, h, bd, jp, njobs, method, step, cb(cost), 0, w_, om, o, None)

    def csub(w=16, h=16, bd=10, method=2, fstop=0, iters=1, cost=good, s=src, njobs=2, ms=19,
             start_from=0):
        return L.lavish_highbd_comp_find_best_sub_pixel_tree_batch(
            s, X.STRIDE, ref, X.STRIDE, w, h, bd, sp, None, start_from, njobs, method, fstop, 1,
            iters, cb(cost), sec, msk, ms, o, None)

    def osub(w=16, h=16, bd=10, fstop=0, iters=1, cost=good, w_=ws, njobs=2):
        return L.lavish_highbd_obmc_find_best_sub_pixel_tree_batch(
            ref, X.STRIDE, w, h, bd, sp, None, njobs, fstop, 1, iters, cb(cost), w_, om, o, None)

    assert comp(step=-1) == -1 and comp(step=15) == -1 and comp(method=2, step=16) == -1
    assert comp(cost=None) == -2 and comp(cost=notab) == -2
    assert comp(w=12) == -3 and comp(h=15) == -3 and comp(method=5) == -4
    assert comp(bd=9) == -7 and comp(bd=16) == -7 and comp(s=None) == -7 and comp(ms=15) == -7
    assert refine(cost=None) == -2 and refine(w=12) == -3 and refine(bd=11) == -7
    assert refine(s=None) == -7 and refine(second=None) == -7 and refine(ms=15) == -7
    assert obmc(step=15) == -1 and obmc(cost=notab) == -2 and obmc(w=12) == -3
    assert obmc(method=9) == -4 and obmc(bd=9) == -7 and obmc(w_=None) == -7
    assert csub(fstop=4) == -1 and csub(cost=None) == -2 and csub(w=12) == -3
    assert csub(iters=3) == -4 and csub(method=3) == -6 and csub(bd=9) == -8
    assert csub(s=None) == -8 and csub(ms=15) == -8 and csub(start_from=2) == -8
    assert csub(start_from=1) == -9
    assert osub(fstop=-1) == -1 and osub(cost=l1) == -2 and osub(w=12) == -3
    assert osub(iters=0) == -4 and osub(bd=13) == -8 and osub(w_=None) == -8
    for f in (comp, refine, obmc, csub, osub):
        assert f(njobs=0, bd=9) == 0 and f(njobs=-1, w=12) == 0
    dev.torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x55).all()
    # and the same buffers take a good call each
    for f in (comp, refine, obmc, csub, osub):
        out.fill_(0x55)
        assert f() == 0
        dev.torch.cuda.synchronize()
        assert not (out.cpu().numpy() == 0x55).all()
