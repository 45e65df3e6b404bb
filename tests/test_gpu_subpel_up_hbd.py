"""GPU parity of the high-bit-depth upsampled sub-pel error
(csrc/subpel_up_hbd.hip through the three highbd_*find_best_sub_pixel_tree_batch
calls of lavish_dsp.motion with search_type), every record field compared with
equality, outputs into poisoned buffers:
* every case of tests/golden/fix_subpel_up_hbd.npz (the reference's own rows)
  against the fixture directly;
* against tests/_hbdup_ref.py: 64x32 (the first size whose invariants are
  re-read) and 128x128 in every form, and 1, 5 and 7 jobs (partial workgroups);
* the full-pel searches chained on the device: plain, compound with start_from
  0 and 1 and pick_lower_besterr (one job without a usable second mv), OBMC;
* planes whose values fit 8 bits: at depth 8 the call equals the 8-bit
  find_best_sub_pixel_tree_batch(search_type=USE_8_TAPS) in every field; at
  depth 10 candidate by candidate (all 64 sub-pel phases), sse and distortion
  through the depth's rounding;
* type 0 through the _ex symbols equals the symbols without it, byte for byte,
  on fix_mcomp_hbd.npz and fix_mcomp_comp_hbd.npz;
* the refusals."""
import ctypes
import math

import numpy as np
import pytest

import _compsubpel_ref as CS
import _hbdcomp_ref as HC
import _hbdsearch_ref as H
import _hbdup_ref as U
import _mvextremes as X

pytestmark = pytest.mark.gpu

S = U.S
FIELDS = U.RESULT_FIELDS
FORMS = (U.PLAIN, U.AVG, U.MASK, U.OBMC)
LOW = (X.ENTROPY, X.LOW_LAMBDA[0], 1)     # (cost type, error_per_bit, hp tables)


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.motion as M
    return M


@pytest.fixture(scope="module")
def F():
    return U.load_fixture()


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
        return self.put(U.plane_key(kind, bd, bw, bh), *U.planes(kind, bd, bw, bh))

    def cost(self, ctype, epb, hp, spb=0):
        if ctype == X.ENTROPY:
            return self.costs[int(bool(hp))].cost_params(spb, epb, self.M.MV_COST_ENTROPY)
        return self.M.l1_cost_params(ctype)

    def poisoned(self, nbytes):
        return self.torch.full((nbytes,), 0x55, dtype=self.torch.uint8, device="cuda")

    def sub(self, form, P, bw, bh, bd, csj, cost, pools, stype, forced_stop, allow_hp, iters,
            fullpel=None, start_from=0, mask_stride=None, method="tree"):
        """One sub-pel call of a form into a poisoned output: (device record
        bytes, [n, 5] results)."""
        M = self.M
        out = self.poisoned(len(csj) * M.SUBPEL_RESULT_DTYPE.itemsize)
        kw = dict(bit_depth=bd, forced_stop=forced_stop, allow_hp=bool(allow_hp),
                  iters_per_step=iters, fullpel=fullpel, out=out, search_type=stype)
        if form == U.OBMC:
            M.highbd_obmc_find_best_sub_pixel_tree_batch(
                P[3], X.STRIDE, bw, bh, M.to_device(csj), cost, pools.d_wsrc, pools.d_omask, **kw)
        elif form == U.PLAIN:
            M.highbd_find_best_sub_pixel_tree_batch(
                P[2], P[3], bw, bh, M.to_device(np.ascontiguousarray(csj["base"])), cost,
                method=method, **kw)
        else:
            ms = pools.mask_stride if mask_stride is None else mask_stride
            M.highbd_comp_find_best_sub_pixel_tree_batch(
                P[2], P[3], bw, bh, M.to_device(csj), cost, pools.d_second,
                pools.d_mask if form == U.MASK else None, ms, method=method,
                start_from=start_from, **kw)
        self.torch.cuda.synchronize()
        return out, self.sub_numpy(out)

    def sub_numpy(self, out):
        r = self.M.subpel_results_numpy(out)
        return np.stack([r[f].astype(np.int64) for f in FIELDS], 1)


@pytest.fixture(scope="module")
def dev(M):
    return Dev(M)


def compare(bad, msg, got, exp):
    exp = np.asarray(exp, np.int64)
    for i, f in enumerate(FIELDS):
        if not np.array_equal(got[:, i], exp[:, i]):
            j = int(np.flatnonzero(got[:, i] != exp[:, i])[0])
            bad.append("%s %s: job %d got %d expected %d (%d differ)" % (
                msg, f, j, got[j, i], exp[j, i], int((got[:, i] != exp[:, i]).sum())))


# ------------------------------------------------- the reference's own rows --
def test_every_fixture_case_through_the_three_calls(dev, F):
    bad, n = [], 0
    pools = Pools(dev.torch, F["second"], F["mask"], F["wsrc"], F["omask"])
    for g in U.fixture_groups(F):
        p = g.prm
        Pl = dev.put("fixu_" + g.plane, F["src__" + g.plane], F["refs__" + g.plane])
        cost = dev.cost(p["cost"], p["error_per_bit"], p["allow_hp"])
        _, got = dev.sub(p["form"], Pl, p["bw"], p["bh"], p["bd"], g.cjobs, cost, pools,
                         p["search_type"], p["forced_stop"], p["allow_hp"], p["iters"],
                         mask_stride=p["mask_stride"])
        compare(bad, "case %d %r" % (g.index, p), got, g.rows[:, g.J["best_row"]:])
        n += len(got)
    assert n == len(F["rows"]) >= 150
    assert not bad, "\n".join(bad[:10])


# ---------------------------------------------------------- the restatement --
def make_pools(dev, Pl, bw, bh, bd, jobs, seed):
    """Invariant blocks for job records `jobs` (src_off read): (Pools, the
    (second_off, mask_off) per form) -- each pool holds one block per job."""
    rng = np.random.default_rng(seed)
    n, top, ms = bw * bh, (1 << bd) - 1, bw + 3
    idx = np.arange(bh)[:, None] * X.STRIDE + np.arange(bw)[None, :]
    sec, msk, ws, om = [], [], [], []
    for jb in jobs:
        src = Pl[0][int(jb["src_off"]) + idx].astype(np.int64)
        sec.append(np.clip(src + rng.integers(-3, 4, src.shape), 0, top).reshape(-1))
        msk.append(rng.integers(0, 65, (bh, ms)).reshape(-1))
        mm = rng.integers(1024, 4097, n)
        nb = np.clip(src.reshape(-1) + rng.integers(-3, 4, n), 0, top)
        ws.append(src.reshape(-1) * 4096 - nb * (4096 - mm))
        om.append(mm)
    k = np.arange(len(jobs))
    # (an odd lead-in: the second_pred blocks are addressed at any element offset)
    pools = Pools(dev.torch, np.concatenate([[7]] + sec), np.concatenate(msk),
                  np.concatenate([[0] * n] + ws), np.concatenate([[0] * n] + om), ms)
    return pools, {U.PLAIN: (0 * k, 0 * k), U.AVG: (1 + k * n, 0 * k),
                   U.MASK: (1 + k * n, k * bh * ms), U.OBMC: (n + k * n, n + k * n)}


def check_forms(dev, bad, msg, Pl, bw, bh, bd, sjobs, stype, sp=(0, 1, 2), cost_t=LOW, seed=1,
                forms=FORMS, invert=0):
    """Every form's search over SUBPEL job records against the restatement."""
    M = dev.M
    ctype, epb, hp = cost_t
    pools, offs = make_pools(dev, Pl, bw, bh, bd, sjobs, seed)
    fstop, allow_hp, iters = sp
    hc, dc = S.cost_of(ctype, epb, 0, allow_hp), dev.cost(ctype, epb, allow_hp)
    for form in forms:
        csj = M.comp_subpel_jobs(sjobs, *offs[form], invert)
        exp = U.run_batch(form, Pl[0], Pl[1], X.STRIDE, bw, bh, csj, hc, bd, stype, fstop,
                          bool(allow_hp), iters, **pools.host())
        _, got = dev.sub(form, Pl, bw, bh, bd, csj, dc, pools, stype, fstop, allow_hp, iters)
        compare(bad, "%s %s type %d" % (msg, U.FORM_NAMES[form], stype), got, exp)


def subpel_jobs(bw, bh, n, salt, starts, ref_mv=(0, 0)):
    fp = X.spread(X.frame(bw, bh, ref_mv), max(n, 3), salt)[:n]
    return CS.subpel_records(fp, bw, bh, [starts[i % len(starts)] for i in range(len(fp))])


STARTS = [(0, -8), (5, -3), (-8, 12), (3, 6), (-11, 15)]


@pytest.mark.parametrize("bw,bh,bd,stype", [
    (64, 32, 10, U.USE_8_TAPS), (128, 128, 12, U.USE_8_TAPS), (32, 64, 8, U.USE_4_TAPS),
    (64, 64, 10, U.USE_2_TAPS)])
def test_sizes_whose_invariants_are_re_read(dev, bw, bh, bd, stype):
    bad = []
    Pl = dev.kind("smooth", bd)
    sj = subpel_jobs(bw, bh, 3, bw + bd, STARTS)
    check_forms(dev, bad, "%dx%d bd %d" % (bw, bh, bd), Pl, bw, bh, bd, sj, stype, seed=bw + bh,
                invert=bd == 10)
    assert not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("njobs", [1, 5, 7])
def test_partial_workgroups(dev, njobs):
    bad = []
    for kind, bd, stype in (("smooth", 10, U.USE_8_TAPS), ("edges", 12, U.USE_4_TAPS)):
        Pl = dev.kind(kind, bd)
        sj = subpel_jobs(16, 16, njobs, njobs, STARTS, (13, -21))
        assert len(sj) == njobs
        check_forms(dev, bad, "%d jobs %s" % (njobs, kind), Pl, 16, 16, bd, sj, stype,
                    seed=njobs)
    assert not bad, "\n".join(bad[:10])


# ------------------------------------------------- chaining on the device --
def test_full_pel_searches_chain_into_the_ex_calls(M, dev):
    """No record passes through the host on the device's path: the full-pel
    call's output tensor is the sub-pel call's fullpel.  (The expected rows
    start from the full-pel records read back.)"""
    bad = []
    bw = bh = 16
    bd = 10
    Pl = dev.kind("smooth", bd)
    fp = X.spread(X.frame(bw, bh, (0, 0), (1, -2)), 5, 3)[:5]
    # the last job's window is a single point: its full-pel search never
    # moves, so it has no second-best mv
    fp[-1:] = X.narrowed(fp[-1:], "point", (1, -2))
    sj = CS.subpel_records(fp, bw, bh)
    sj["start_row"] = sj["start_col"] = 0x5555          # (never read: fullpel is given)
    pools, offs = make_pools(dev, Pl, bw, bh, bd, fp, 11)
    ctype, epb, hp = LOW
    hc, dc = S.cost_of(ctype, epb, 0, 1), dev.cost(ctype, epb, 1)
    dcf = dev.cost(ctype, epb, 1, X.LOW_LAMBDA[1])
    sp = (0, 1, 2)
    for stype in (U.USE_8_TAPS, U.USE_2_TAPS):
        # plain
        res, _ = M.highbd_full_pixel_search_batch(Pl[2], Pl[3], bw, bh, M.to_device(fp), dcf,
                                                  bit_depth=bd, method="nstep", step_param=7)
        best = M.results_numpy(res)
        fpl = np.stack([best["best_row"], best["best_col"]], 1).astype(np.int64)
        csj = M.comp_subpel_jobs(sj, 0, 0, 0)
        _, got = dev.sub(U.PLAIN, Pl, bw, bh, bd, csj, dc, pools, stype, *sp, fullpel=res)
        exp = U.run_batch(U.PLAIN, Pl[0], Pl[1], X.STRIDE, bw, bh, csj, hc, bd, stype, sp[0], True,
                          sp[2], fullpel=fpl, **pools.host())
        compare(bad, "plain chained type %d" % stype, got, exp)
        # compound (average, mask): both starts and the pick
        for form in (U.AVG, U.MASK):
            cj = M.comp_jobs(fp, *offs[form], 0)
            res = M.highbd_comp_full_pixel_search_batch(
                Pl[2], Pl[3], bw, bh, M.to_device(cj), dcf, pools.d_second,
                pools.d_mask if form == U.MASK else None, pools.mask_stride, bit_depth=bd,
                method="nstep", step_param=7)
            r = M.comp_results_numpy(res)
            fpl = np.stack([r[f] for f in ("best_row", "best_col", "second_row", "second_col")],
                           1).astype(np.int64)
            assert fpl[-1, 2] == M.INVALID_MV and (fpl[:-1, 2] != M.INVALID_MV).any()
            csj = M.comp_subpel_jobs(sj, *offs[form], 0)
            outs, exps = [], []
            for which in (0, 1):
                out, got = dev.sub(form, Pl, bw, bh, bd, csj, dc, pools, stype, *sp, fullpel=res,
                                   start_from=which)
                exp = U.run_batch(form, Pl[0], Pl[1], X.STRIDE, bw, bh, csj, hc, bd, stype, sp[0],
                                  True, sp[2], fullpel=fpl, start_from=which, **pools.host())
                compare(bad, "%s chained %d type %d" % (U.FORM_NAMES[form], which, stype), got,
                        exp)
                outs.append(out)
                exps.append(exp)
            assert exps[1][-1].tolist() == [CS.NO_SEARCH[f] for f in FIELDS]
            picked = dev.sub_numpy(M.pick_lower_besterr(*outs))
            compare(bad, "%s picked type %d" % (U.FORM_NAMES[form], stype), picked,
                    CS.pick_lower(*exps))
        # OBMC
        cj = M.comp_jobs(fp, *offs[U.OBMC], 0)
        res = M.highbd_obmc_full_pixel_search_batch(
            Pl[3], X.STRIDE, bw, bh, M.to_device(cj), dcf, pools.d_wsrc, pools.d_omask,
            bit_depth=bd, method="nstep", step_param=7)
        r = M.comp_results_numpy(res)
        fpl = np.stack([r["best_row"], r["best_col"]], 1).astype(np.int64)
        csj = M.comp_subpel_jobs(sj, *offs[U.OBMC], 0)
        _, got = dev.sub(U.OBMC, Pl, bw, bh, bd, csj, dc, pools, stype, *sp, fullpel=res)
        exp = U.run_batch(U.OBMC, Pl[0], Pl[1], X.STRIDE, bw, bh, csj, hc, bd, stype, sp[0], True,
                          sp[2], fullpel=fpl, **pools.host())
        compare(bad, "obmc chained type %d" % stype, got, exp)
    assert not bad, "\n".join(bad[:10])


# ----------------------------------------------------- beside the 8-bit call --
def _eight_bit_planes(dev):
    """Smooth planes between 64 and 191 (no 8-tap overshoot reaches 0 or 255,
    so the 8-bit clip and the deeper one never differ), as u8 and as u16."""
    s, r = H.planes("smooth", 8)
    s8, r8 = (s >> 1) + 64, (r >> 1) + 64
    up = lambda a, t: dev.torch.from_numpy(np.ascontiguousarray(a.astype(t))).cuda()
    return (s8, r8, up(s8, np.uint8), up(r8, np.uint8), up(s8, np.int16), up(r8, np.int16))


def test_depth_8_on_u16_equals_the_8_bit_call(M, dev):
    s8, r8, ds8, dr8, ds16, dr16 = _eight_bit_planes(dev)
    sj = subpel_jobs(16, 16, 6, 2, STARTS)
    cost = dev.cost(X.ENTROPY, 37, 1)
    want = M.find_best_sub_pixel_tree_batch(ds8, dr8, 16, 16, M.to_device(sj), cost, method="tree",
                                            allow_hp=True, iters_per_step=2,
                                            search_type=M.USE_8_TAPS)
    got = M.highbd_find_best_sub_pixel_tree_batch(ds16, dr16, 16, 16, M.to_device(sj), cost,
                                                  bit_depth=8, method="tree", allow_hp=True,
                                                  iters_per_step=2, search_type=M.USE_8_TAPS)
    dev.torch.cuda.synchronize()
    assert np.array_equal(M.subpel_results_numpy(got), M.subpel_results_numpy(want))
    moved = M.subpel_results_numpy(got)
    assert ((moved["best_row"] != sj["start_row"]) | (moved["best_col"] != sj["start_col"])).any()


def test_depth_10_on_8_bit_values_equals_the_8_bit_call_candidate_by_candidate(M, dev):
    """At depth 10 the variance is taken from rounded sums, so a search's
    ranking is its own; what must agree is every candidate.  forced_stop
    FULL_PEL makes the result the centre error at the (sub-pel) start: one
    job per phase pair.  sse10 = (sse8 + 8) >> 4; the 8-bit record gives the
    sum only through sse8 - var8 = floor(sum^2 / N), and the 10-bit distortion
    must be max(0, sse10 - ((sum + 2) >> 2)^2 / N) for a sum that fits it."""
    s8, r8, ds8, dr8, ds16, dr16 = _eight_bit_planes(dev)
    n = 8 * 8
    starts = [(-8 + r, 8 + c) for r in range(8) for c in range(8)]
    sj = subpel_jobs(8, 8, 64, 5, starts)
    assert len(sj) == 64
    cost = M.l1_cost_params(X.NONE)
    kw = dict(method="tree", forced_stop=3, search_type=M.USE_8_TAPS)
    a = M.subpel_results_numpy(M.find_best_sub_pixel_tree_batch(
        ds8, dr8, 8, 8, M.to_device(sj), cost, **kw))
    b = M.subpel_results_numpy(M.highbd_find_best_sub_pixel_tree_batch(
        ds16, dr16, 8, 8, M.to_device(sj), cost, bit_depth=10, **kw))
    for f in ("best_row", "best_col"):
        assert np.array_equal(a[f], b[f]) and np.array_equal(a[f], sj[f.replace("best", "start")])
    assert np.array_equal(b["sse"].astype(np.int64), (a["sse"].astype(np.int64) + 8) >> 4)
    assert np.array_equal(b["besterr"].astype(np.int64), b["distortion"].astype(np.int64))
    for i in range(64):
        sse8, var8 = int(a["sse"][i]), int(a["distortion"][i])
        q = sse8 - var8                             # floor(sum^2 / N)
        lo, hi = math.isqrt(q * n), math.isqrt(q * n + n - 1)
        sums = [s * sg for s in range(lo, hi + 1) for sg in (1, -1) if (s * s) // n == q]
        assert sums, i
        fits = {max(0, ((sse8 + 8) >> 4) - (((s + 2) >> 2) ** 2) // n) for s in sums}
        assert int(b["distortion"][i]) in fits, (i, int(b["distortion"][i]), fits)


# --------------------------------------------- type 0 is the existing call --
def _raw(L, name, *args):
    rc = getattr(L, name)(*args)
    assert rc == 0, (name, rc)


def test_type_0_through_ex_equals_the_calls_without_it(M, dev):
    import lavish_dsp
    L = lavish_dsp.lib()
    vp = ctypes.c_void_p
    n = 0
    # fix_mcomp_hbd.npz: the single-reference searches, every method
    FH = H.load_fixture()
    for g in H.fixture_groups(FH):
        p = g.prm
        Pl = dev.put("fixh_" + g.plane, FH["src__" + g.plane], FH["refs__" + g.plane])
        cost = dev.cost(p["cost"], p["error_per_bit"], p["sp_allow_hp"])
        jobs = M.to_device(g.sjobs)
        cl = None
        if p["sp_use_cl"]:
            cl = dev.torch.from_numpy(np.ascontiguousarray(
                g.rows[:, g.J["cl0"]:g.J["cl4"] + 1].astype(np.int32))).cuda()
        outs = [dev.poisoned(len(g.sjobs) * 16) for _ in range(2)]
        head = [vp(Pl[2].data_ptr()), X.STRIDE, vp(Pl[3].data_ptr()), X.STRIDE, p["bw"], p["bh"],
                p["bd"], vp(jobs.data_ptr()), None, len(g.sjobs), p["sp_method"]]
        tail = [p["sp_forced_stop"], p["sp_allow_hp"], p["sp_iters"], ctypes.byref(cost),
                None if cl is None else vp(cl.data_ptr())]
        _raw(L, "lavish_highbd_find_best_sub_pixel_tree_batch", *head, *tail,
             vp(outs[0].data_ptr()), None)
        _raw(L, "lavish_highbd_find_best_sub_pixel_tree_batch_ex", *head, 0, *tail,
             vp(outs[1].data_ptr()), None)
        dev.torch.cuda.synchronize()
        assert dev.torch.equal(outs[0], outs[1]), (g.index, p)
        want = g.rows[:, g.J["sp_best_row"]:g.J["sp_sse"] + 1]
        assert np.array_equal(dev.sub_numpy(outs[1]), want), (g.index, p)
        n += len(want)
    # fix_mcomp_comp_hbd.npz: compound, masked and OBMC, from the best mv
    FC = HC.load_fixture()
    pools = Pools(dev.torch, FC["second"], FC["mask"], FC["wsrc"], FC["omask"])
    for g in HC.fixture_groups(FC):
        p, J = g.prm, g.J
        if not p["has_sp"]:
            continue
        Pl = dev.put("fixc_" + g.plane, FC["src__" + g.plane], FC["refs__" + g.plane])
        cost = dev.cost(p["cost"], p["error_per_bit"], p["sp_allow_hp"])
        sj = g.sjobs.copy()
        sj["base"]["start_row"] = 8 * g.rows[:, J["best_row"]]
        sj["base"]["start_col"] = 8 * g.rows[:, J["best_col"]]
        jobs = M.to_device(sj)
        outs = [dev.poisoned(len(sj) * 16) for _ in range(2)]
        tail = [p["sp_forced_stop"], p["sp_allow_hp"], p["sp_iters"], ctypes.byref(cost)]
        if p["search"] == HC.OBMC:
            head = [vp(Pl[3].data_ptr()), X.STRIDE, p["bw"], p["bh"], p["bd"], vp(jobs.data_ptr()),
                    None, len(sj)]
            tail += [vp(pools.d_wsrc.data_ptr()), vp(pools.d_omask.data_ptr())]
            name = "lavish_highbd_obmc_find_best_sub_pixel_tree_batch"
        else:
            head = [vp(Pl[2].data_ptr()), X.STRIDE, vp(Pl[3].data_ptr()), X.STRIDE, p["bw"],
                    p["bh"], p["bd"], vp(jobs.data_ptr()), None, 0, len(sj), p["sp_method"]]
            tail += [vp(pools.d_second.data_ptr()),
                     vp(pools.d_mask.data_ptr()) if p["form"] == HC.MASK else None,
                     p["mask_stride"]]
            name = "lavish_highbd_comp_find_best_sub_pixel_tree_batch"
        _raw(L, name, *head, *tail, vp(outs[0].data_ptr()), None)
        _raw(L, name + "_ex", *head, 0, *tail, vp(outs[1].data_ptr()), None)
        dev.torch.cuda.synchronize()
        assert dev.torch.equal(outs[0], outs[1]), (g.index, p)
        assert np.array_equal(dev.sub_numpy(outs[1]), HC.sp_rows(g, 0)), (g.index, p)
        n += len(sj)
    assert n > 200


# ---------------------------------------------------------------- refusals --
def test_refusals_leave_the_output_untouched(M, dev):
    Pl = dev.kind("smooth", 10)
    sj = subpel_jobs(16, 16, 2, 1, STARTS)
    pools, offs = make_pools(dev, Pl, 16, 16, 10, sj, 3)
    good, l1 = dev.cost(X.ENTROPY, 37, 0), dev.cost(X.L1, 37, 0)

    def rc_of(form, cost=good, **kw):
        csj = M.comp_subpel_jobs(sj, *offs[form], 0)
        try:
            out, _ = dev.sub(form, Pl, 16, 16, 10, csj, cost, pools, kw.pop("stype", 3), 0, 0, 1,
                             **kw)
        except ValueError as e:
            return int(str(e).split("rc=")[1].rstrip(")"))
        assert not (out.cpu().numpy() == 0x55).all()
        return 0
    for form in FORMS:
        assert rc_of(form, stype=4) == -7 and rc_of(form, stype=-1) == -7
        assert rc_of(form, stype=3) == 0
    # estimate_obmc_mvcost asserts on the L1 types; mv_err_cost_ takes them
    assert rc_of(U.OBMC, l1, stype=0) == -2 and rc_of(U.OBMC, l1, stype=3) == 0
    assert rc_of(U.OBMC, l1, stype=1) == 0
    for form in (U.AVG, U.MASK):
        assert rc_of(form, stype=3, start_from=1) == -9
        assert rc_of(form, stype=0, start_from=1) == -9
    # a refused call writes nothing
    out = dev.poisoned(2 * 16)
    with pytest.raises(ValueError, match=r"rc=-7"):
        M.highbd_find_best_sub_pixel_tree_batch(Pl[2], Pl[3], 16, 16, M.to_device(sj), good,
                                                bit_depth=10, method="tree", search_type=4,
                                                out=out)
    dev.torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x55).all()
