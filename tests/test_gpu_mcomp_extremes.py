"""GPU parity of the motion searches on tied, saturated and high-lambda inputs
(tests/_mvextremes.py): every kernel route against av1_full_pixel_search /
av1_find_best_sub_pixel_tree* executed from the reference
(tests/golden/fix_mcomp_extremes.npz, no oracle in the loop) and against the
oracle on the full 80-block x 2-reference frame of each content kind -- every
record field (best_row, best_col, bestsme, steps; `searches`, which the oracle
does not hold, against variant 1's bytes) and the five cost-list entries, into
poisoned buffers.

What the content is for: exact ties between the 8 sites of a step (the packed
keys (sad + cost) * 8 + site and the reduction order carry the reference's
first-strictly-better rule), difference sums whose square needs 64 bits
(sum * sum from 64x64 up), and rate * error_per_bit past 2^31 (the product is
formed in mcomp_dev.h, mcomp_lj.hip, subpel.hip and the TPL wavefront).
tests/test_mcomp_extremes_cpu.py asserts that the content has those
properties and pins the oracle on it."""
import numpy as np
import pytest

import _mvextremes as X
import _oracle as O

pytestmark = pytest.mark.gpu

TIE_KINDS = X.TIE_KINDS
SIZES = [(4, 4), (8, 8), (16, 16), (16, 8), (32, 32)]
BIG = [(64, 64), (128, 128)]
JOBSETS = ["at_ref", "off_ref", "point", "row", "col"]
COSTS = [X.ENTROPY, X.L1, X.NONE]
FIELDS = ("best_row", "best_col", "bestsme", "steps")
SUB_FIELDS = ("best_row", "best_col", "besterr", "distortion", "sse")
LOW = (37, 4, (13, -21), 0)          # (error_per_bit, sad_per_bit, ref_mv, hp tables)
HIGH = [(epb, X.SAD_PER_BIT_TOP, ref_mv, hp) for epb, ref_mv, hp in X.HIGH_LAMBDA]


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.motion as M
    return M


class Dev:
    """Device planes, tiles and cost tables of the content kinds, and the
    oracle's answers, each made once."""

    def __init__(self, M):
        import torch
        self.M, self.torch = M, torch
        self.planes, self.tabs, self.costs, self.memo = {}, {}, {}, {}
        for hp in (0, 1):
            self.tabs[hp] = M.default_mv_cost_tables(bool(hp))
            self.costs[hp] = M.MvCosts(*self.tabs[hp], device="cuda")

    def get(self, kind, bw, bh):
        key = X.plane_key(kind, bw, bh)
        if key not in self.planes:
            src, refs = X.planes(kind, bw, bh)
            ts = self.torch.from_numpy(src.copy()).cuda()   # (the shared planes are read-only)
            tr = self.torch.from_numpy(refs.copy()).cuda()
            self.planes[key] = (src, refs, ts, tr, self.M.RefTiles(tr, X.STRIDE).build())
        return self.planes[key]

    def cost(self, ctype, lam):
        epb, spb, _, hp = lam
        if ctype == X.ENTROPY:
            return self.costs[hp].cost_params(spb, epb, self.M.MV_COST_ENTROPY)
        return self.M.l1_cost_params(ctype)

    def oracle(self, kind, bw, bh, jobs, jkey, method, sp, ctype, lam, skip, mesh=None):
        key = (kind, bw, bh, jkey, method, sp, ctype, lam, skip, mesh is not None)
        if key not in self.memo:
            src, refs = self.get(kind, bw, bh)[:2]
            epb, spb, _, hp = lam
            mvj, mvc = self.tabs[hp]
            self.memo[key] = O.full_pixel_search_batch(
                src.reshape(-1), refs.reshape(-1), X.STRIDE, bw, bh, jobs, method, sp, ctype,
                spb, epb, mvj, mvc, skip=bool(skip), cost_list=True, threads=8, mesh=mesh)
        return self.memo[key]

    def search(self, kind, bw, bh, jobs, method, sp, ctype, lam, skip, tiled, mesh=None,
               want_cl=True):
        """One full_pixel_search_batch into poisoned outputs: (records, cost lists)."""
        M, torch = self.M, self.torch
        _, _, ts, tr, tiles = self.get(kind, bw, bh)
        n = len(jobs)
        out = torch.full((n * M.RESULT_DTYPE.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
        cl = torch.full((n, 5), -7, dtype=torch.int32, device="cuda") if want_cl else None
        M.full_pixel_search_batch(ts, tr, bw, bh, M.to_device(jobs), self.cost(ctype, lam),
                                  method, sp, bool(skip), want_cl, out=out, cost_lists=cl,
                                  tiles=tiles if tiled else None, mesh=mesh)
        torch.cuda.synchronize()
        return out.cpu().numpy(), (cl.cpu().numpy() if want_cl else None)


@pytest.fixture(scope="module")
def dev(M):
    return Dev(M)


def jobset(name, bw, bh, ref_mv):
    at = ((ref_mv[0] + 4) >> 3, (ref_mv[1] + 4) >> 3)
    if name == "at_ref":
        return X.frame(bw, bh, ref_mv, at if max(abs(at[0]), abs(at[1])) < 32 else (0, 0))
    if name == "off_ref":
        return X.frame(bw, bh, ref_mv, (0, -1) if max(abs(at[0]), abs(at[1])) >= 32
                       else (at[0] + 3, at[1] - 2))
    return X.narrowed(X.frame(bw, bh, ref_mv, (0, 0)), name, (0, 0) if abs(at[0]) >= 32
                      else (3, -2))


def compare(bad, msg, got_out, got_cl, exp, ecl, M, fields=FIELDS):
    res = got_out.view(M.RESULT_DTYPE)
    for f in fields:
        if not np.array_equal(res[f], exp[f]):
            i = int(np.flatnonzero(res[f] != exp[f])[0])
            bad.append("%s %s: job %d got %d expected %d (%d differ)" % (
                msg, f, i, res[f][i], exp[f][i], int((res[f] != exp[f]).sum())))
    if got_cl is not None and not np.array_equal(got_cl, ecl):
        i = int(np.flatnonzero((got_cl != ecl).any(axis=1))[0])
        bad.append("%s cost list: job %d got %s expected %s" % (msg, i, got_cl[i], ecl[i]))


# ------------------------------------------------- the reference's own rows --
@pytest.mark.parametrize("tiled", [False, True])
def test_fullpel_vs_reference(M, dev, tiled):
    """Every full-pel row of the fixture, linear and tiled: best mv, returned
    cost and cost list."""
    import torch
    F = X.load_fixture()
    bad, n = [], 0
    for g in X.fixture_groups(F, "fp"):
        p = g.params
        src, refs = torch.from_numpy(g.src).cuda(), torch.from_numpy(g.refs).cuda()
        tiles = M.RefTiles(refs, X.STRIDE).build() if tiled else None
        cp = dev.cost(p["cost"], (p["error_per_bit"], p["sad_per_bit"], None, p["hp_tables"]))
        nj = len(g.jobs)
        out = torch.full((nj * M.RESULT_DTYPE.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
        cl = torch.full((nj, 5), -7, dtype=torch.int32, device="cuda")
        M.full_pixel_search_batch(src, refs, g.bw, g.bh, M.to_device(g.jobs), cp,
                                  X.FP_METHODS[p["method"]], p["step_param"], bool(p["skip"]),
                                  bool(p["use_cl"]), out=out, cost_lists=cl, tiles=tiles)
        torch.cuda.synchronize()
        exp = {"best_row": g.rows[:, g.J["best_row"]], "best_col": g.rows[:, g.J["best_col"]],
               "bestsme": g.rows[:, g.J["var"]]}
        compare(bad, "%s %s %dx%d" % (g.name, g.kind, g.bw, g.bh), out.cpu().numpy(),
                cl.cpu().numpy() if p["use_cl"] else None, exp,
                g.rows[:, g.J["cl0"]:g.J["cl4"] + 1], M, ("best_row", "best_col", "bestsme"))
        n += nj
    assert n == len(F["fp_rows"])
    assert not bad, "\n".join(bad)


def test_subpel_vs_reference(M, dev):
    """Every sub-pel row of the fixture through
    lavish_find_best_sub_pixel_tree_batch."""
    import torch
    F = X.load_fixture()
    bad, n = [], 0
    for g in X.fixture_groups(F, "sp"):
        p = g.params
        src, refs = torch.from_numpy(g.src).cuda(), torch.from_numpy(g.refs).cuda()
        cp = dev.cost(p["cost"], (p["error_per_bit"], 0, None, p["allow_hp"]))
        cls = (torch.from_numpy(np.ascontiguousarray(
            g.rows[:, g.J["cl0"]:g.J["cl4"] + 1].astype(np.int32))).cuda()
            if p["use_cl"] else None)
        out = torch.full((len(g.jobs) * M.SUBPEL_RESULT_DTYPE.itemsize,), 0x55,
                         dtype=torch.uint8, device="cuda")
        M.find_best_sub_pixel_tree_batch(src, refs, g.bw, g.bh, M.to_device(g.jobs), cp,
                                         X.SUBPEL_METHODS[p["method"]], p["forced_stop"],
                                         bool(p["allow_hp"]), p["iters_per_step"],
                                         cost_lists=cls, out=out, search_type=p["search_type"])
        torch.cuda.synchronize()
        res = M.subpel_results_numpy(out)
        for f in SUB_FIELDS:
            if not np.array_equal(res[f].astype(np.int64), g.rows[:, g.J[f]]):
                bad.append("%s %s %dx%d %s: got %s expected %s" % (
                    g.name, g.kind, g.bw, g.bh, f, res[f], g.rows[:, g.J[f]]))
        n += len(g.rows)
    assert n == len(F["sp_rows"])
    assert not bad, "\n".join(bad)


# --------------------------------------------- full frames against the oracle --
def frame_sweep(M, dev, kind, tiled, lam, sizes, costs, salt=0):
    """Every method x step_param {0, 3} x size of `sizes` on the kind's full
    frame; the job set (start at / off ref_mv, point / row / column windows),
    the cost type and the downsampled SAD rotate so that every method meets
    every job set."""
    bad, n = [], 0
    for si, (bw, bh) in enumerate(sizes):
        for mi, method in enumerate(M.SEARCH_METHODS):
            for sp in (0, 3):
                jname = JOBSETS[(si + mi + sp + salt) % len(JOBSETS)]
                ctype = costs[(si + 2 * mi + sp) % len(costs)]
                skip = (mi + si + sp) & 1
                jobs = jobset(jname, bw, bh, lam[2])
                exp, ecl = dev.oracle(kind, bw, bh, jobs, jname, method, sp, ctype, lam, skip)
                got, gcl = dev.search(kind, bw, bh, jobs, method, sp, ctype, lam, skip, tiled)
                compare(bad, "%s %dx%d %s sp %d %s cost %d skip %d" % (
                    kind, bw, bh, method, sp, jname, ctype, skip), got, gcl, exp, ecl, M)
                n += 1
    assert not bad, "%d of %d calls differ:\n%s" % (len(bad), n, "\n".join(bad[:40]))


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("kind", TIE_KINDS)
def test_fullpel_frames(M, dev, kind, tiled):
    frame_sweep(M, dev, kind, tiled, LOW, SIZES, COSTS)


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("kind", ["flat_255_0", "flat_0_255", "split", "one_sided"])
def test_fullpel_saturated(M, dev, kind, tiled):
    """64x64 and 128x128: |difference sum|^2 past 2^32 (flat, one-sided) and
    the largest sse (split; the point windows hold it at mv (0, 0))."""
    frame_sweep(M, dev, kind, tiled, LOW, BIG, COSTS, salt=2)


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("lam", HIGH, ids=lambda l: "epb%d" % l[0])
@pytest.mark.parametrize("kind", ["noise", "flat_128_128", "periodic_16"])
def test_fullpel_high_lambda(M, dev, kind, lam, tiled):
    """rate * error_per_bit past 2^31 in every method's mv_err_cost."""
    frame_sweep(M, dev, kind, tiled, lam, SIZES[:3] + BIG[:1], [X.ENTROPY])


# ---------------------- 16x16 tiled DIAMOND with the downsampled SAD (mcomp_lj) --
LJ_KINDS = TIE_KINDS + ["noise", "stripes"]


@pytest.mark.parametrize("lam", [LOW, HIGH[0], HIGH[2]], ids=lambda l: "epb%d" % l[0])
@pytest.mark.parametrize("kind", LJ_KINDS)
def test_lj_routes(M, dev, kind, lam):
    """diamond_lj_dyn_kernel (variant FULL), the lean kernel and its redo
    kernel (variant LEAN), caps {0, 8}, queued and static, each twice in a
    row: the oracle's records and cost lists, and variant 1's bytes
    (`searches` included)."""
    from test_gpu_lj_lean import second_pass_share
    bad = []
    for ci, ctype in enumerate(COSTS if lam is LOW else [X.ENTROPY]):
        for sp in (0, 3):
            jname = JOBSETS[(ci + sp) % 2] if lam is LOW else "off_ref"
            jobs = jobset(jname, 16, 16, lam[2])
            exp, ecl = dev.oracle(kind, 16, 16, jobs, jname, "diamond", sp, ctype, lam, 1)
            if kind in ("checker", "periodic_2", "stripes") and lam is LOW:
                src, refs = dev.get(kind, 16, 16)[:2]
                noskip, _ = dev.oracle(kind, 16, 16, jobs, jname, "diamond", sp, ctype, lam, 0)
                lower, upper = second_pass_share(src, refs, jobs, exp, noskip)
                print("%s second-pass share between %.3f and %.3f" % (kind, lower, upper))
                # by construction (see _mvextremes.stripes(); on the checker and the 2x2
                # tile every row carries the same share of any SAD, so twice
                # the even rows' SAD is the full one and no job is sent back)
                assert (lower, upper) == ((1.0, 1.0) if kind == "stripes" else (0.0, 0.0))
            M.set_search_variant(M.SEARCH_VARIANT_FULL)
            try:
                base, base_cl = dev.search(kind, 16, 16, jobs, "diamond", sp, ctype, lam, 1, True)
                for variant in (M.SEARCH_VARIANT_FULL, M.SEARCH_VARIANT_LEAN):
                    for cap in (0, 8):
                        for queued in (True, False):
                            M.set_search_variant(variant)
                            M.set_search_workgroup_cap(cap)
                            M.set_search_schedule(queued)
                            for it in range(2):
                                msg = "%s %s cost %d sp %d variant %d cap %d queued %d pass %d" % (
                                    kind, jname, ctype, sp, variant, cap, queued, it)
                                got, gcl = dev.search(kind, 16, 16, jobs, "diamond", sp, ctype,
                                                      lam, 1, True)
                                compare(bad, msg, got, gcl, exp, ecl, M)
                                if not np.array_equal(got, base):
                                    bad.append(msg + " record bytes differ from variant 1's")
                                if not np.array_equal(gcl, base_cl):
                                    bad.append(msg + " cost lists differ from variant 1's")
            finally:
                M.set_search_variant(M.SEARCH_VARIANT_AUTO)
                M.set_search_workgroup_cap(0)
                M.set_search_schedule(True)
    assert not bad, "%d differ:\n%s" % (len(bad), "\n".join(bad[:40]))


# --------------------------------------------------------------------- mesh --
@pytest.mark.parametrize("kind", ["flat_128_128", "periodic_8"])
def test_mesh(M, dev, kind):
    """The exhaustive mesh refinement where every site of a pass ties (flat)
    or every eighth matches exactly (periodic-8)."""
    from test_gpu_mcomp_fixtures import MESH_SETS
    pats, run, thr, prune, diff, fine, intra = MESH_SETS[0]
    mesh = M.MeshParams.make(pats, run, thr, prune, diff, fine, intra)
    omesh = O.OrcMeshParams(run, thr, prune, diff, fine, intra)
    for i, (r, iv) in enumerate(pats):
        omesh.range[i], omesh.interval[i] = r, iv
    bad = []
    for k, (method, (bw, bh), tiled) in enumerate([("diamond", (16, 16), True),
                                                   ("nstep", (8, 8), False),
                                                   ("hex", (16, 16), False)]):
        jobs = jobset(JOBSETS[k % 2], bw, bh, LOW[2])
        exp, ecl = dev.oracle(kind, bw, bh, jobs, JOBSETS[k % 2], method, 1, X.ENTROPY, LOW, k & 1,
                              mesh=omesh)
        got, gcl = dev.search(kind, bw, bh, jobs, method, 1, X.ENTROPY, LOW, k & 1, tiled,
                              mesh=mesh)
        compare(bad, "%s mesh %s %dx%d" % (kind, method, bw, bh), got, gcl, exp, ecl, M,
                ("best_row", "best_col", "bestsme"))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ sub-pel --
SUB_KINDS = ["flat_128_128", "flat_255_0", "flat_0_255", "checker", "split", "ramp_x", "ramp_y"]
SUB_ROUTES = [("tree", 0), ("tree", 3), ("pruned", 0), ("pruned_more", 0)]  # (method, taps)


def subpel_starts(dev, kind, bw, bh, lam, edges):
    """(sub-pel jobs, full-pel records or None, cost lists or None): from the
    oracle's DIAMOND results and cost lists, or on the edges and corners of
    the jobs' limits."""
    from lavish_dsp import motion as M
    if edges:
        return X.subpel_edge_jobs(bw, bh, lam[2]), None, None
    jobs = jobset("off_ref", bw, bh, lam[2])
    fp, cl = dev.oracle(kind, bw, bh, jobs, "off_ref", "diamond", 1, X.ENTROPY, lam, 0)
    return M.subpel_jobs(X.W, X.H, X.BORDER, bw, bh, jobs, fp, lam[2]), fp, cl


def subpel_tree_sweep(M, dev, kind, lam, edges, sizes):
    import torch
    bad, n = [], 0
    for bw, bh in sizes:
        src, refs, ts, tr, _ = dev.get(kind, bw, bh)
        sj, fp, cl = subpel_starts(dev, kind, bw, bh, lam, edges)
        dj = M.to_device(sj)
        dcl = torch.from_numpy(cl).cuda() if cl is not None else None
        k = 0
        for method, taps in SUB_ROUTES:
            for use_cl in ((0, 1) if cl is not None and method != "tree" else (0,)):
                for fstop in (M.EIGHTH_PEL, M.QUARTER_PEL, M.HALF_PEL):
                    for hp in (0, 1):
                        for iters in (1, 2):
                            ctype = X.ENTROPY if (lam is not LOW or k % 3) else X.L1
                            k += 1
                            tab = 1 if lam[3] else hp
                            mvj, mvc = dev.tabs[tab]
                            exp = O.subpel_search_batch(
                                src.reshape(-1), refs.reshape(-1), X.STRIDE, bw, bh, sj,
                                X.SUBPEL_METHODS.index(method), fstop, bool(hp), iters, ctype,
                                lam[0], mvj, mvc, cl if use_cl else None, threads=8,
                                search_type=taps)
                            out = torch.full((len(sj) * 16,), 0x55, dtype=torch.uint8,
                                             device="cuda")
                            M.find_best_sub_pixel_tree_batch(
                                ts, tr, bw, bh, dj, dev.cost(ctype, (lam[0], 0, None, tab)),
                                method, fstop, bool(hp), iters,
                                cost_lists=dcl if use_cl else None, out=out, search_type=taps)
                            torch.cuda.synchronize()
                            got = M.subpel_results_numpy(out)
                            n += 1
                            for f in SUB_FIELDS:
                                if not np.array_equal(got[f], exp[f]):
                                    i = int(np.flatnonzero(got[f] != exp[f])[0])
                                    bad.append(
                                        "%s %dx%d %s taps %d cl %d stop %d hp %d iters %d cost %d "
                                        "%s: job %d got %d expected %d" % (
                                            kind, bw, bh, method, taps, use_cl, fstop, hp, iters,
                                            ctype, f, i, got[f][i], exp[f][i]))
    assert not bad, "%d of %d calls differ:\n%s" % (len(bad), n, "\n".join(bad[:40]))


@pytest.mark.parametrize("edges", [False, True], ids=["from_fullpel", "limit_edges"])
@pytest.mark.parametrize("kind", SUB_KINDS)
def test_subpel_tree_batch(M, dev, kind, edges):
    """find_best_sub_pixel_tree_batch: three methods, USE_2_TAPS_ORIG and
    USE_8_TAPS, with and without the cost lists, forced_stop, allow_hp,
    iters_per_step -- from the full-pel results and from every edge and
    corner of the sub-pel limits."""
    subpel_tree_sweep(M, dev, kind, LOW, edges, [(16, 16), (8, 8)])


@pytest.mark.parametrize("kind", ["flat_255_0", "split"])
def test_subpel_tree_batch_saturated(M, dev, kind):
    subpel_tree_sweep(M, dev, kind, LOW, False, BIG)


@pytest.mark.parametrize("lam", HIGH, ids=lambda l: "epb%d" % l[0])
@pytest.mark.parametrize("kind", ["noise", "checker"])
def test_subpel_tree_batch_high_lambda(M, dev, kind, lam):
    subpel_tree_sweep(M, dev, kind, lam, False, [(16, 16), (4, 4)])


@pytest.mark.parametrize("edges", [False, True], ids=["from_fullpel", "limit_edges"])
@pytest.mark.parametrize("kind", SUB_KINDS)
def test_subpel_search_batch_and_after_diamond(M, dev, kind, edges):
    """lavish_subpel_search_batch (pruned_more, the L1 / none costs) and its
    device-chained form lavish_subpel_search_after_diamond."""
    import torch
    bad = []
    for bw, bh in [(16, 16), (8, 8), (64, 64)]:
        src, refs, ts, tr, _ = dev.get(kind, bw, bh)
        sj, fp, _ = subpel_starts(dev, kind, bw, bh, LOW, edges)
        dj = M.to_device(sj)
        blank = sj.copy()
        blank["start_row"] = blank["start_col"] = 0
        k = 0
        for fstop in (M.EIGHTH_PEL, M.QUARTER_PEL, M.HALF_PEL):
            for hp in (False, True):
                for iters in (1, 2):
                    ctype = (1, 2, 3, 4)[k % 4]
                    k += 1
                    exp = O.subpel_batch(src.reshape(-1), refs.reshape(-1), X.STRIDE, bw, bh, sj,
                                         fstop, hp, iters, ctype, threads=8)
                    out = torch.full((len(sj) * 16,), 0x55, dtype=torch.uint8, device="cuda")
                    M.subpel_search_batch(ts, tr, bw, bh, dj, fstop, hp, iters, ctype, out=out)
                    outs = [("batch", out)]
                    if fp is not None:
                        out2 = torch.full((len(sj) * 16,), 0x55, dtype=torch.uint8, device="cuda")
                        M.subpel_after_diamond(ts, tr, bw, bh, M.to_device(blank),
                                               M.to_device(fp), fstop, hp, iters, ctype, out=out2)
                        outs.append(("after_diamond", out2))
                    torch.cuda.synchronize()
                    for name, o in outs:
                        got = M.subpel_results_numpy(o)
                        for f in SUB_FIELDS:
                            if not np.array_equal(got[f], exp[f]):
                                bad.append("%s %s %dx%d stop %d hp %d iters %d cost %d %s" % (
                                    name, kind, bw, bh, fstop, hp, iters, ctype, f))
    assert not bad, "\n".join(bad[:40])


# ---------------------------------------------------------------------- TPL --
def tpl_planes(kind, w, h, border):
    pw, ph = w + 2 * border, h + 2 * border
    if kind == "flat":
        src = np.full((ph, pw), 128, np.uint8)
    else:
        tile = np.random.default_rng(23).integers(0, 256, (16, 16))
        src = np.tile(tile, (ph // 16 + 1, pw // 16 + 1))[:ph, :pw].astype(np.uint8)
    return np.ascontiguousarray(src), np.ascontiguousarray(np.stack([src, src]))


@pytest.mark.parametrize("lam", [LOW, HIGH[2]], ids=lambda l: "epb%d" % l[0])
@pytest.mark.parametrize("ci", [0, 4])
@pytest.mark.parametrize("kind", ["flat", "periodic_16"])
def test_tpl_motion_search(M, kind, ci, lam):
    """The TPL wavefront where every start-mv candidate ties (flat) or
    matches exactly (periodic-16): prune_starting_mv / skip_alike_starting_mv
    keep the reference's first; 96x64 x 2 references; the entropy cost at
    error_per_bit 37 and 131071."""
    import torch
    import lavish_dsp.tpl as T
    from test_gpu_tplmv import CASES
    method, sp, skip, prune, alike, third = CASES[ci]
    w, h, R, border = 96, 64, 2, 160
    src, refs = tpl_planes(kind, w, h, border)
    st = src.shape[1]
    cols, rows = w // 16, h // 16
    jobs = M.frame_jobs(w, h, st, border, src.size, 16, 16, R, ref_mv=lam[2], mv_border=32)
    epb, spb, _, hp = lam
    mvj, mvc = M.default_mv_cost_tables(bool(hp))
    tp = None
    if third:
        rng = np.random.default_rng(41)
        tp = T.pack_mv(rng.integers(-20, 21, size=len(jobs)), rng.integers(-20, 21, size=len(jobs)))
        tp[rng.random(len(jobs)) < 0.3] = T.INVALID_MV
    emv, efp, ecl, ecen = O.tpl_motion_search(src.reshape(-1), refs.reshape(-1), st, jobs, cols,
                                              rows, R, method, sp, skip, prune, alike, spb, epb,
                                              mvj, mvc, 0, tp)
    cost = M.MvCosts(mvj, mvc, device="cuda").cost_params(spb, epb, M.MV_COST_ENTROPY)
    out = T.tpl_motion_search(torch.from_numpy(src).cuda(), torch.from_numpy(refs).cuda(),
                              M.to_device(jobs), cols, rows, R, cost, method, sp, skip, prune,
                              alike, torch.from_numpy(tp).cuda() if tp is not None else None)
    torch.cuda.synchronize()
    assert T.tpl_motion_failures(out) == 0
    gfp = M.results_numpy(out["fp"])
    np.testing.assert_array_equal(out["mvs"].cpu().numpy(), emv)
    np.testing.assert_array_equal(out["centers"].cpu().numpy(), ecen)
    for f in FIELDS:
        np.testing.assert_array_equal(gfp[f], efp[f], err_msg=f)
    np.testing.assert_array_equal(out["cl"].cpu().numpy(), ecl)
