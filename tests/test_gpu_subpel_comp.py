"""GPU parity of the compound, masked and OBMC sub-pel search batches
(csrc/subpel_comp.hip through lavish_dsp.motion), every record field compared
with equality, outputs into poisoned buffers:
* every row of tests/golden/fix_subpel_comp.npz (av1_find_best_sub_pixel_tree
  / _pruned / _pruned_more with second_pred and
  av1_find_best_obmc_sub_pixel_tree_up executed from the reference) against
  the fixture directly, starts given in the jobs;
* the chain on the device: the full-pel batch of fix_mcomp_comp.npz's groups,
  then the sub-pel call with fullpel= from the best and from the second-best
  mv, then pick_lower_besterr, against tests/_compsubpel_ref.py fed that
  fixture's full-pel results (the INT_MAX record of jobs without a usable
  second mv included);
* the block sizes the fixture cannot reach against the restatement: 4x16,
  16x4 and 8x32 (segment / row geometry), 64x32 (the last size with cached
  words), 64x64 (the first that re-reads) and 128x128;
* batch geometry: 1, 3, 5 and 80 jobs, a non-default stream, the invariant
  blocks addressed in reversed job order, both invert_mask values in a batch."""
import numpy as np
import pytest

import _compsearch_ref as S
import _compsubpel_ref as CS
import _mvextremes as X

pytestmark = pytest.mark.gpu

FIELDS = CS.RESULT_FIELDS
METHOD_NAMES = {CS.TREE: "tree", CS.PRUNED: "pruned", CS.PRUNED_MORE: "pruned_more"}


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.motion as M
    return M


@pytest.fixture(scope="module")
def F():
    return CS.load_fixture()


class Dev:
    """Device planes, pools and cost tables, each uploaded once."""

    def __init__(self, M, F):
        import torch
        self.M, self.torch, self.F = M, torch, F
        self.planes, self.pools, self.memo = {}, {}, {}
        self.costs = {hp: M.MvCosts(*M.default_mv_cost_tables(bool(hp)), device="cuda")
                      for hp in (0, 1)}

    def get(self, plane):
        if plane not in self.planes:
            src, refs = self.F["src__" + plane], self.F["refs__" + plane]
            self.planes[plane] = (src, refs, self.torch.from_numpy(src.copy()).cuda(),
                                  self.torch.from_numpy(refs.copy()).cuda())
        return self.planes[plane]

    def pool(self, key, arr):
        if key not in self.pools:
            self.pools[key] = self.torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        return self.pools[key]

    def cost(self, ctype, epb, hp, spb=0):
        if ctype == X.ENTROPY:
            return self.costs[int(bool(hp))].cost_params(spb, epb, self.M.MV_COST_ENTROPY)
        return self.M.l1_cost_params(ctype)

    def poisoned(self, n):
        return self.torch.full((n * self.M.SUBPEL_RESULT_DTYPE.itemsize,), 0x55,
                               dtype=self.torch.uint8, device="cuda")

    def run(self, prm, plane, cjobs, P, fullpel=None, start_from=0, stream=None, sync=True):
        """One sub-pel batch call into a poisoned output; P = (memo key, host
        pools {second, mask, wsrc, omask}).  Returns the device bytes."""
        M = self.M
        _, _, ts, tr = self.get(plane)
        pk, pools = P
        d = lambda n: self.pool((pk, n), pools[n])
        out = self.poisoned(len(cjobs))
        cost = self.cost(prm["cost"], prm["error_per_bit"], prm["allow_hp"])
        kw = dict(search_type=prm["search_type"], forced_stop=prm["forced_stop"],
                  allow_hp=bool(prm["allow_hp"]), iters_per_step=prm["iters"], fullpel=fullpel,
                  out=out, stream=stream)
        jobs = M.to_device(cjobs)
        if prm["form"] == CS.OBMC:
            M.obmc_find_best_sub_pixel_tree_batch(tr, X.STRIDE, prm["bw"], prm["bh"], jobs, cost,
                                                  d("wsrc"), d("omask"), **kw)
        else:
            M.comp_find_best_sub_pixel_tree_batch(
                ts, tr, prm["bw"], prm["bh"], jobs, cost, d("second"),
                d("mask") if prm["form"] == CS.MASK else None, prm["mask_stride"],
                METHOD_NAMES[prm["method"]], start_from=start_from, **kw)
        if sync:
            self.torch.cuda.synchronize()
        return out

    def expected(self, key, prm, plane, cjobs, P, **kw):
        if key not in self.memo:
            src, refs = self.get(plane)[:2]
            pools = P[1]
            self.memo[key] = CS.run_batch(
                prm["form"], src.reshape(-1), refs.reshape(-1), X.STRIDE, prm["bw"], prm["bh"],
                cjobs, S.cost_of(prm["cost"], prm["error_per_bit"], 0, prm["allow_hp"]),
                prm["method"], prm["search_type"], prm["forced_stop"], bool(prm["allow_hp"]),
                prm["iters"], pools["second"], pools["mask"], prm["mask_stride"], pools["wsrc"],
                pools["omask"], **kw)
        return self.memo[key]


@pytest.fixture(scope="module")
def dev(M, F):
    return Dev(M, F)


def compare(bad, msg, got, exp):
    for i, f in enumerate(FIELDS):
        g = got[f].astype(np.int64)
        if not np.array_equal(g, exp[:, i]):
            j = int(np.flatnonzero(g != exp[:, i])[0])
            bad.append("%s %s: job %d got %d expected %d (%d differ)" % (
                msg, f, j, g[j], exp[j, i], int((g != exp[:, i]).sum())))


def params(form, bw, bh, method=CS.PRUNED_MORE, search_type=0, allow_hp=1, forced_stop=0, iters=2,
           cost=X.ENTROPY, epb=37, mask_stride=0):
    return dict(form=form, bw=bw, bh=bh, method=method, search_type=search_type,
                allow_hp=allow_hp, forced_stop=forced_stop, iters=iters, cost=cost,
                error_per_bit=epb, mask_stride=mask_stride)


# ------------------------------------------------- the reference's own rows --
def test_every_fixture_row(M, dev, F):
    J = {n: i for i, n in enumerate(CS.ROW_FIELDS)}
    P = ("fixture", {k: F[k] for k in ("second", "mask", "wsrc", "omask")})
    bad, n = [], 0
    for g in CS.fixture_groups(F):
        got = M.subpel_results_numpy(dev.run(g.prm, g.plane, g.cjobs, P))
        compare(bad, "case %d %r" % (g.index, g.prm), got, g.rows[:, J["best_row"]:J["sse"] + 1])
        n += len(got)
    assert n == len(F["rows"]) >= 150
    assert not bad, "\n".join(bad[:10])


# ------------------------------------------------------------------- chain --
# the sub-pel parameters the chained groups rotate through:
# (method, search type, allow_hp, forced_stop, iters_per_step)
CHAIN = [(CS.PRUNED_MORE, 0, 1, 0, 1), (CS.TREE, 3, 1, 0, 2), (CS.PRUNED, 0, 0, 1, 2),
         (CS.TREE, 0, 1, 0, 2), (CS.TREE, 2, 1, 0, 1)]


def test_chain_after_the_full_pel_batches(M, dev, F):
    """Full pel to eighth pel with no host round trip: the device's full-pel
    records feed the sub-pel call (they equal the fixture's, which
    test_gpu_mcomp_comp.py pins), from the best and the second-best mv, and
    pick_lower_besterr keeps the lower."""
    import torch
    MC = S.load_fixture()
    JM = {n: i for i, n in enumerate(S.ROW_FIELDS)}
    pools = {k: MC[k] for k in ("second", "mask", "wsrc", "omask")}
    P = ("chain", pools)
    d = lambda n: dev.pool(("chain", n), pools[n])
    bad, n, nosearch, second_won = [], 0, 0, 0
    for g in S.fixture_groups(MC):
        p = g.prm
        if p["search"] != S.OBMC and p["form"] == S.PLAIN:
            continue
        obmc = p["search"] == S.OBMC
        form = CS.OBMC if obmc else (CS.AVG if p["form"] == S.AVG else CS.MASK)
        method, stype, hp, fstop, iters = CHAIN[g.index % len(CHAIN)]
        # estimate_obmc_mvcost asserts on L1, and at the high lambdas its
        # diff x 8 leaves the cost tables: those groups take the 8-tap error
        if obmc and stype == 0 and (p["cost"] == X.L1 or p["error_per_bit"] > 1000):
            stype = 3
        prm = params(form, p["bw"], p["bh"], method, stype, hp, fstop, iters, p["cost"],
                     p["error_per_bit"], p["mask_stride"] if form == CS.MASK else 0)
        _, _, ts, tr = dev.get(g.kind)
        fcost = dev.cost(p["cost"], p["error_per_bit"], p["hp_tables"], p["sad_per_bit"])
        name = S.METHOD_NAMES[p["method"]]
        jobs = M.to_device(g.cjobs)
        if p["search"] == S.COMP:
            fp = M.comp_full_pixel_search_batch(ts, tr, p["bw"], p["bh"], jobs, fcost, d("second"),
                                                d("mask") if form == CS.MASK else None,
                                                p["mask_stride"], name, p["step_param"])
        elif p["search"] == S.REFINE8:
            fp = M.refining_search_8p_batch(ts, tr, p["bw"], p["bh"], jobs, fcost, d("second"),
                                            d("mask") if form == CS.MASK else None,
                                            p["mask_stride"])
        else:
            fp = M.obmc_full_pixel_search_batch(tr, X.STRIDE, p["bw"], p["bh"], jobs, fcost,
                                                d("wsrc"), d("omask"), name, p["step_param"],
                                                bool(p["fast_obmc"]))
        sj = CS.subpel_records(g.cjobs["base"], p["bw"], p["bh"])
        cj = M.comp_subpel_jobs(sj, g.cjobs["second_off"], g.cjobs["mask_off"],
                                g.cjobs["invert_mask"])
        # the restatement is fed the fixture's own full-pel rows
        fix_fp = np.zeros(len(g.rows), M.COMP_RESULT_DTYPE)
        for f in ("best_row", "best_col", "second_row", "second_col"):
            fix_fp[f] = g.rows[:, JM[f]]
        # an hp search prices with the hp tables whatever the full-pel call used
        sub = dict(prm)
        a = dev.run(sub, g.kind, cj, P, fullpel=fp, sync=False)
        ea = dev.expected(("chain", g.index, 0), sub, g.kind, cj, P, fullpel=fix_fp)
        if obmc:
            got, exp = a, ea
        else:
            b = dev.run(sub, g.kind, cj, P, fullpel=fp, start_from=1, sync=False)
            eb = dev.expected(("chain", g.index, 1), sub, g.kind, cj, P, fullpel=fix_fp,
                              start_from=1)
            torch.cuda.synchronize()
            compare(bad, "group %d second" % g.index, M.subpel_results_numpy(b), eb)
            nosearch += int((eb[:, 2] == CS.INT_MAX).sum())
            got, exp = M.pick_lower_besterr(a, b), CS.pick_lower(ea, eb)
            second_won += int((eb[:, 2] < ea[:, 2]).sum())
            assert got.is_cuda
        torch.cuda.synchronize()
        compare(bad, "group %d %r" % (g.index, sub), M.subpel_results_numpy(got), exp)
        n += len(exp)
    assert n >= 120 and nosearch >= 5, (n, nosearch, second_won)
    assert not bad, "\n".join(bad[:10])


def test_pick_lower_besterr_is_strict(M):
    import torch
    a = np.zeros(4, M.SUBPEL_RESULT_DTYPE)
    b = np.zeros(4, M.SUBPEL_RESULT_DTYPE)
    a["besterr"], b["besterr"] = [10, 10, CS.INT_MAX, 0x80000005], [10, 9, 7, CS.INT_MAX]
    a["best_row"], b["best_row"] = 1, 2
    got = M.subpel_results_numpy(M.pick_lower_besterr(M.to_device(a), M.to_device(b)))
    assert got["best_row"].tolist() == [1, 2, 2, 2] and got["besterr"].tolist() == [
        10, 9, 7, CS.INT_MAX]


# --------------------------------------------------- sizes beyond the fixture --
def smooth_jobs(plane, bw, bh, n, salt, ref_mv=(5, -11), whole=False):
    """n sub-pel jobs of the smooth frame (whole: its first n) starting on the
    full pel nearest the match (every third one pel off)."""
    fp = X.frame(bw, bh, ref_mv)
    fp = fp[:n].copy() if whole else X.spread(fp, max(n, 3), salt)[:n]
    starts = []
    for i, jb in enumerate(fp):
        k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
        sh = CS.SHIFTS[plane][k]
        starts.append((8 * ((sh[0] + 4) >> 3), 8 * (((sh[1] + 4) >> 3) + (i % 3 == 2))))
    return CS.subpel_records(fp, bw, bh, starts)


def size_pools(bw, bh, sj, src, seed):
    """Invariant blocks near the source for jobs `sj`, one per job: (pools,
    second_off, mask_off, wsrc_off, mask_stride); mask rows bw + 5 apart, the
    u8 blocks at odd offsets."""
    rng = np.random.default_rng(seed)
    n, ms, nj = bw * bh, bw + 5, len(sj)
    idx = np.arange(bh)[:, None] * X.STRIDE + np.arange(bw)[None, :]
    blocks = np.stack([src.reshape(-1)[int(jb["src_off"]) + idx].reshape(-1).astype(np.int64)
                       for jb in sj])
    second = rng.integers(0, 256, nj * (n + 3) + 8).astype(np.uint8)
    so = np.arange(nj) * (n + 3) + 1
    for i in range(nj):
        second[so[i]:so[i] + n] = np.clip(blocks[i] + rng.integers(-3, 4, n), 0, 255)
    mask = rng.integers(0, 65, nj * (bh * ms + 1) + 8).astype(np.uint8)
    mo = np.arange(nj) * (bh * ms + 1) + 3
    om = rng.integers(1024, 4097, (nj, n))
    ws = blocks * 4096 - np.clip(blocks + rng.integers(-4, 5, om.shape), 0, 255) * (4096 - om)
    pools = dict(second=second, mask=mask, wsrc=ws.reshape(-1).astype(np.int32),
                 omask=om.reshape(-1).astype(np.int32))
    return pools, so, mo, np.arange(nj) * n, ms


BEYOND = [(4, 16, 5), (16, 4, 5), (8, 32, 5), (64, 32, 4), (64, 64, 3), (128, 128, 1)]
# (form, method, search type, allow_hp, forced_stop, iters_per_step, cost)
CALLS = [(CS.AVG, CS.PRUNED_MORE, 0, 1, 0, 2, X.ENTROPY), (CS.AVG, CS.TREE, 3, 1, 0, 2, X.L1),
         (CS.MASK, CS.TREE, 0, 1, 0, 2, X.ENTROPY), (CS.MASK, CS.PRUNED, 1, 0, 1, 2, X.NONE),
         (CS.MASK, CS.TREE, 2, 1, 0, 1, X.ENTROPY), (CS.OBMC, CS.TREE, 0, 1, 0, 2, X.ENTROPY),
         (CS.OBMC, CS.TREE, 3, 1, 0, 2, X.L1), (CS.OBMC, CS.TREE, 1, 0, 1, 1, X.NONE)]


@pytest.mark.parametrize("bw,bh,njobs", BEYOND, ids=lambda v: str(v))
def test_sizes_beyond_the_fixture(M, dev, bw, bh, njobs):
    bad, moved = [], 0
    plane = "smooth_a"
    src = dev.get(plane)[0]
    sj = smooth_jobs(plane, bw, bh, njobs, bw + bh)
    pools, so, mo, wo, ms = size_pools(bw, bh, sj, src, 1000 * bw + bh)
    P = ((plane, bw, bh), pools)
    for ci, (form, method, stype, hp, fstop, iters, ctype) in enumerate(CALLS):
        prm = params(form, bw, bh, method, stype, hp, fstop, iters, ctype, 41 + ci,
                     ms if form == CS.MASK else 0)
        cj = (M.comp_subpel_jobs(sj, wo, wo) if form == CS.OBMC else
              M.comp_subpel_jobs(sj, so, mo, np.arange(njobs) % 2))
        exp = dev.expected((plane, bw, bh, ci), prm, plane, cj, P)
        got = M.subpel_results_numpy(dev.run(prm, plane, cj, P))
        compare(bad, "%dx%d call %d" % (bw, bh, ci), got, exp)
        moved += int(((exp[:, 0] != sj["start_row"]) | (exp[:, 1] != sj["start_col"])).sum())
    assert moved >= len(CALLS) * njobs // 3
    assert not bad, "\n".join(bad[:10])


# ------------------------------------------------------------ batch geometry --
GEOM_CALLS = [(CS.AVG, CS.PRUNED_MORE, 0), (CS.MASK, CS.TREE, 0), (CS.MASK, CS.TREE, 3),
              (CS.OBMC, CS.TREE, 0), (CS.OBMC, CS.TREE, 2)]


def geometry(dev):
    """80 16x16 jobs of the smooth frame, job i on the invariant blocks of
    index 79 - i."""
    if "geom" not in dev.memo:
        src = dev.get("smooth_b")[0]
        sj = smooth_jobs("smooth_b", 16, 16, 120, 0, whole=True)[40:].copy()
        assert len(sj) == 80
        pools, so, mo, wo, ms = size_pools(16, 16, sj[::-1], src, 77)
        dev.memo["geom"] = (sj, pools, so[::-1], mo[::-1], wo[::-1], ms)
    return dev.memo["geom"]


@pytest.mark.parametrize("njobs", [1, 3, 5, 80])
def test_batch_geometry(M, dev, njobs):
    import torch
    sj, pools, so, mo, wo, ms = geometry(dev)
    P = ("geom", pools)
    assert so[0] > so[1] and wo[0] > wo[1]           # reversed: read per job, not by index
    stream = torch.cuda.Stream()
    bad = []
    for ci, (form, method, stype) in enumerate(GEOM_CALLS):
        full = (M.comp_subpel_jobs(sj, wo, wo) if form == CS.OBMC else
                M.comp_subpel_jobs(sj, so, mo, np.arange(80) % 2))
        prm = params(form, 16, 16, method, stype, mask_stride=ms if form == CS.MASK else 0)
        exp = dev.expected(("geom", ci), prm, "smooth_b", full, P)
        for st in (None, stream):
            if st is not None:
                st.wait_stream(torch.cuda.current_stream())     # (the uploads)
            got = M.subpel_results_numpy(dev.run(prm, "smooth_b", full[:njobs], P, stream=st))
            compare(bad, "call %d n %d stream %s" % (ci, njobs, st is not None), got,
                    exp[:njobs])
    assert not bad, "\n".join(bad[:10])


def test_output_past_the_batch_is_untouched(M, dev):
    """5 jobs (a partial second workgroup) into a buffer of 8 records."""
    import torch
    sj, pools, so, mo, wo, ms = geometry(dev)
    cj = M.comp_subpel_jobs(sj, so, mo)[:5]
    out = dev.poisoned(8)
    ts, tr = dev.get("smooth_b")[2:4]
    M.comp_find_best_sub_pixel_tree_batch(ts, tr, 16, 16, M.to_device(cj), dev.cost(X.L1, 0, 0),
                                          dev.pool(("geom", "second"), pools["second"]),
                                          out=out[:5 * 16])
    torch.cuda.synchronize()
    assert (out[5 * 16:].cpu().numpy() == 0x55).all()
    assert (M.subpel_results_numpy(out[:5 * 16])["sse"] > 0).all()


def test_wrappers_raise_on_a_refusal(M, dev):
    import torch
    ts, tr = dev.get("smooth_b")[2:4]
    jobs = torch.zeros(M.COMP_SUBPEL_JOB_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    sec = torch.zeros(256, dtype=torch.uint8, device="cuda")
    w32 = torch.zeros(256, dtype=torch.int32, device="cuda")
    cost = M.l1_cost_params()
    with pytest.raises(ValueError):
        M.comp_find_best_sub_pixel_tree_batch(ts, tr, 16, 16, jobs, cost, sec, start_from=1)
    with pytest.raises(ValueError):
        M.comp_find_best_sub_pixel_tree_batch(ts, tr, 16, 16, jobs, cost, sec, mask=sec,
                                              mask_stride=8)
    with pytest.raises(ValueError):
        M.comp_find_best_sub_pixel_tree_batch(ts, tr, 12, 12, jobs, cost, sec)
    with pytest.raises(ValueError):     # an L1 cost under estimate_obmc_mvcost
        M.obmc_find_best_sub_pixel_tree_batch(tr, X.STRIDE, 16, 16, jobs, cost, w32, w32)
