"""numpy restatement of the compound, masked and OBMC sub-pel searches
(av1/encoder/mcomp.c: av1_find_best_sub_pixel_tree :3128-3196, _pruned
:2992-3126 and _pruned_more :2907-2990 with ms_buffers.second_pred and no cost
list / repeat list; av1_find_best_obmc_sub_pixel_tree_up :3761-3803),
sequential as the reference runs them, over tests/_compref.py's bilinear /
avg_pred / mask_pred / variance / obmc_variance and a numpy
aom_upsampled_pred_c (av1/encoder/reconinter_enc.c:424-496, unscaled) -- and
the reader of tests/golden/fix_subpel_comp.npz.

The 8-tap-layout kernels of av1_get_filter come from the library's own table
(lavish_dsp.inter.interp_kernels, pinned to the reference's in
test_capi_cpu.py), not from a copy here.

test_subpel_comp_cpu.py pins search() to the fixture (the reference's own
results) and, with form PLAIN, to the CPU oracle of the single-reference
search; the GPU tests then use it at the sizes the fixture cannot reach.
"""
import collections
import os

import numpy as np

import _compref as R
import _compsearch_ref as S
import _mvextremes as X

PLAIN, AVG, MASK, OBMC = 0, 1, 2, 3                  # forms of the error
TREE, PRUNED, PRUNED_MORE = 0, 1, 2                  # SUBPEL_SEARCH_METHODS
USE_2_TAPS_ORIG, USE_2_TAPS, USE_4_TAPS, USE_8_TAPS = range(4)
EIGHTH_PEL, QUARTER_PEL, HALF_PEL, FULL_PEL = range(4)
INT_MAX, INVALID, M32 = 0x7FFFFFFF, -32768, 0xFFFFFFFF
RESULT_FIELDS = ["best_row", "best_col", "besterr", "distortion", "sse"]
NO_SEARCH = dict(best_row=INVALID, best_col=INVALID, besterr=INT_MAX, distortion=0, sse=0)

# the smooth plane sets of the fixture (tests/golden/gen_fix_subpel_comp.py):
# the shift of reference k in 1/8 pel (row, col), the mv at which it matches
# the source.  smooth_b's second reference sits on a full pel
SHIFTS = {"smooth_a": [(3, -5), (-10, 13)], "smooth_b": [(-6, 2), (-8, 16)]}

_kernels = {}


def up_kernels(search_type):
    """av1_get_filter(search_type)'s kernels in the 8-tap layout: [16, 8]."""
    if search_type not in _kernels:
        from lavish_dsp import inter
        k = inter.interp_kernels(0, 8 if search_type == USE_8_TAPS else 4).astype(np.int64)
        if k.shape[1] == 4:     # the 4-tap kernels sit in the middle of the 8-tap layout
            k = np.pad(k, ((0, 0), (2, 2)))
        _kernels[search_type] = k
    return _kernels[search_type]


def upsampled_pred(ref, off, stride, w, h, sx, sy, search_type):
    """aom_upsampled_pred_c for an unscaled reference: the block at flat
    offset `off`, sub-pel (sx, sy) in 1/8 pel.  USE_2_TAPS is the bilinear
    kernel through the same passes, which is _compref.bilinear's arithmetic."""
    def win(y0, nrows, x0, ncols):
        idx = (np.arange(nrows)[:, None] + y0) * stride + np.arange(ncols)[None, :] + x0
        return ref[off + idx].astype(np.int64)
    if search_type == USE_2_TAPS:
        return R.bilinear(win(0, h + 1, 0, w + 1), sx, sy)
    if not sx and not sy:
        return win(0, h, 0, w)
    K = up_kernels(search_type)

    def horiz(a, k):        # a: [rows, w + 7] from column -3
        acc = sum(a[:, t:t + w] * k[t] for t in range(8))
        return np.clip((acc + 64) >> 7, 0, 255)

    def vert(a, k):         # a: [h + 7, w] from row -3
        acc = sum(a[t:t + h, :] * k[t] for t in range(8))
        return np.clip((acc + 64) >> 7, 0, 255)
    if not sy:
        return horiz(win(0, h, -3, w + 7), K[2 * sx])
    if not sx:
        return vert(win(-3, h + 7, 0, w), K[2 * sy])
    return vert(horiz(win(-3, h + 7, -3, w + 7), K[2 * sx]), K[2 * sy])


class Env:
    """One job: the flat planes, the invariant blocks, the limits and costs."""

    def __init__(self, src, ref, stride, bw, bh, job, cost, form=PLAIN, second=None, mask=None,
                 invert=0, wsrc=None, omask=None):
        self.ref, self.stride, self.bw, self.bh = ref, stride, bw, bh
        self.ref_off = int(job["ref_off"])
        if form != OBMC:
            idx = np.arange(bh)[:, None] * stride + np.arange(bw)[None, :]
            self.src = src[int(job["src_off"]) + idx].astype(np.int64)
        self.lim = [int(job[f]) for f in ("col_min", "col_max", "row_min", "row_max")]
        self.ref_mv = (int(job["ref_mv_row"]), int(job["ref_mv_col"]))
        self.start = (int(job["start_row"]), int(job["start_col"]))
        self.cost, self.form = cost, form
        self.second, self.mask, self.invert = second, mask, invert
        self.wsrc, self.omask = wsrc, omask

    def in_range(self, r, c):
        """av1_is_subpelmv_in_range"""
        return self.lim[0] <= c <= self.lim[1] and self.lim[2] <= r <= self.lim[3]

    def err(self, r, c, search_type):
        """(variance, sse) of the form's prediction at the 1/8-pel mv (r, c):
        the bilinear one (svf / svaf / msvf / osvf) with USE_2_TAPS_ORIG or
        USE_2_TAPS, else the upsampled prediction, combined, then vf / ovf."""
        st = USE_2_TAPS if search_type == USE_2_TAPS_ORIG else search_type
        off = self.ref_off + (r >> 3) * self.stride + (c >> 3)
        p = upsampled_pred(self.ref, off, self.stride, self.bw, self.bh, c & 7, r & 7, st)
        if self.form == OBMC:
            v, sse = R.obmc_variance(p, self.wsrc, self.omask, 8)
        else:
            if self.form == AVG:
                p = R.avg_pred(p, self.second)
            elif self.form == MASK:
                p = R.mask_pred(p, self.second, self.mask, self.invert)
            v, sse = R.variance(p, self.src, 8)
        return int(v), int(sse)

    def _rate(self, dr, dc):
        return int(X.mv_rate(self.cost.mvjcost, self.cost.mvcost, dr, dc, (0, 0)))

    def mv_err_cost(self, r, c):
        """mv_err_cost_ (mcomp.c:290-323)"""
        dr, dc = r - self.ref_mv[0], c - self.ref_mv[1]
        if self.cost.ctype == 0:
            return (self._rate(dr, dc) * self.cost.epb + 8192) >> 14
        return (S.SSE_LAMBDA[self.cost.ctype] * (abs(dr) + abs(dc))) >> 3

    def obmc_estimate_cost(self, r, c):
        """estimate_obmc_mvcost (mcomp.c:3561-3583): the diff through
        GET_MV_SUBPEL, int arithmetic, 13 bits; the L1 types assert."""
        if self.cost.ctype == 4:
            return 0
        assert self.cost.ctype == 0, "L1 norm is not tuned for estimated obmc mvcost"
        v = self._rate(8 * (r - self.ref_mv[0]), 8 * (c - self.ref_mv[1])) * self.cost.epb + 4096
        v = ((v + (1 << 31)) & M32) - (1 << 31)
        return (v >> 13) & M32


def search(e, method=PRUNED_MORE, search_type=USE_2_TAPS_ORIG, forced_stop=EIGHTH_PEL,
           allow_hp=False, iters=1, start=None, obmc_centre_at_start=False, trace=None):
    """One sub-pel search of job `e` from `start` (default: the job's): a
    result dict (RESULT_FIELDS).  An OBMC job runs the OBMC tree whatever
    `method` says.  obmc_centre_at_start: give the USE_2_TAPS_ORIG OBMC search
    the start's own error instead of mv (0, 0)'s (what the reference's TODO
    describes; only to show that the difference matters).  trace: a dict that
    receives `oob` (candidates outside the limits) and `second_level` (levels
    whose second-level check ran)."""
    start = e.start if start is None else start
    obmc = e.form == OBMC
    tree = obmc or method == TREE
    orig = search_type == USE_2_TAPS_ORIG
    # the pruned methods take the bilinear error for every type
    etype = search_type if tree else USE_2_TAPS_ORIG
    tr = trace if trace is not None else {}
    tr.update(oob=0, second_level=0)
    b = dict(best_row=start[0], best_col=start[1])

    if obmc:
        at = (0, 0) if orig and not obmc_centre_at_start else start
    elif tree and not orig:
        at = start
    else:       # setup_center_error: the block get_buf_from_mv points at
        at = (start[0] & ~7, start[1] & ~7)
    var, sse = e.err(at[0], at[1], etype)
    b.update(distortion=var, sse=sse, besterr=(var + e.mv_err_cost(*start)) & M32)

    def check(r, c):
        if not e.in_range(r, c):
            tr["oob"] += 1
            return INT_MAX
        var, sse = e.err(r, c, etype)
        mvc = e.obmc_estimate_cost(r, c) if obmc and orig else e.mv_err_cost(r, c)
        cost = (mvc + var) & M32
        if cost < b["besterr"]:
            b.update(best_row=r, best_col=c, besterr=cost, distortion=var, sse=sse)
        return cost

    def first_level(tr_, tc, h):
        left, right = check(tr_, tc - h), check(tr_, tc + h)
        up, down = check(tr_ - h, tc), check(tr_ + h, tc)
        dr, dc = (-h if up <= down else h), (-h if left <= right else h)    # get_best_diag_step
        check(tr_ + dr, tc + dc)
        return dr, dc

    def two_level_checks_fast(tr_, tc, h):
        dr, dc = first_level(tr_, tc, h)
        if iters <= 1:
            return
        br, bc = b["best_row"], b["best_col"]
        if tr_ != br and tc != bc:          # second_level_check_fast (:2608-2671)
            check(br, bc + dc)
            check(br + dr, bc)
        elif tr_ == br and tc != bc:
            check(br + h, bc + dc)
            check(br - h, bc + dc)
            check(br - dr, bc)
        elif tr_ != br and tc == bc:
            check(br + dr, bc + h)
            check(br + dr, bc - h)
            check(br, bc - dc)

    def tree_level(h):
        tr_, tc = b["best_row"], b["best_col"]
        dr, dc = first_level(tr_, tc, h)
        br, bc = b["best_row"], b["best_col"]
        if (br, bc) == (tr_, tc) or iters <= 1:
            return
        tr["second_level"] += 1             # second_level_check_v2 (:2728-2779)
        if tr_ == br:
            dr = -dr
        elif tc == bc:
            dc = -dc
        before = b["besterr"]
        check(br + dr, bc)
        check(br, bc + dc)
        if b["besterr"] != before:
            check(br + dr, bc + dc)

    if tree:
        rounds = min(FULL_PEL - forced_stop, 3 - (0 if allow_hp else 1))
        for it in range(rounds):
            tree_level(4 >> it)
    elif forced_stop != FULL_PEL:
        two_level_checks_fast(start[0], start[1], 4)
        if forced_stop < HALF_PEL:
            two_level_checks_fast(b["best_row"], b["best_col"], 2)
        if allow_hp and forced_stop == EIGHTH_PEL:
            two_level_checks_fast(b["best_row"], b["best_col"], 1)
    return b


# ------------------------------------------------------------------ batches --
def make_env(form, src, ref, stride, bw, bh, cj, cost, second=None, mask=None, mask_stride=0,
             wsrc=None, omask=None):
    """The Env of one COMP_SUBPEL_JOB_DTYPE record over flat planes and pools."""
    n = bw * bh
    so, mo = int(cj["second_off"]), int(cj["mask_off"])
    jb = cj["base"]
    if form == OBMC:
        return Env(None, ref, stride, bw, bh, jb, cost, OBMC,
                   wsrc=wsrc[so:so + n].astype(np.int64).reshape(bh, bw),
                   omask=omask[mo:mo + n].astype(np.int64).reshape(bh, bw))
    sec = msk = None
    if form != PLAIN:
        sec = second[so:so + n].astype(np.int64).reshape(bh, bw)
    if form == MASK:
        msk = R.window(mask[mo:], mask_stride, bw, bh).astype(np.int64)
    return Env(src, ref, stride, bw, bh, jb, cost, form, sec, msk, int(cj["invert_mask"]))


def run_batch(form, src, ref, stride, bw, bh, cjobs, cost, method=PRUNED_MORE,
              search_type=USE_2_TAPS_ORIG, forced_stop=EIGHTH_PEL, allow_hp=False, iters=1,
              second=None, mask=None, mask_stride=0, wsrc=None, omask=None, fullpel=None,
              start_from=0):
    """The restatement over COMP_SUBPEL_JOB_DTYPE records: [n, 5] int64
    (RESULT_FIELDS).  fullpel: COMP_RESULT_DTYPE records to start from, as the
    device call takes them (start_from 1: the second-best mv; a job without a
    usable one gives NO_SEARCH)."""
    out = []
    for i, cj in enumerate(cjobs):
        e = make_env(form, src, ref, stride, bw, bh, cj, cost, second, mask, mask_stride, wsrc,
                     omask)
        start = None
        if fullpel is not None:
            f = fullpel[i]
            fr, fc = ((int(f["second_row"]), int(f["second_col"])) if start_from else
                      (int(f["best_row"]), int(f["best_col"])))
            start = (8 * fr, 8 * fc)
            if start_from and (INVALID in (fr, fc) or not e.in_range(*start)):
                out.append([NO_SEARCH[f] for f in RESULT_FIELDS])
                continue
        r = search(e, method, search_type, forced_stop, allow_hp, iters, start)
        out.append([r[f] for f in RESULT_FIELDS])
    return np.array(out, np.int64).reshape(-1, 5)


def block_limits(src_off, bw, bh, ref_mv):
    """The SubpelMvLimits of the block at flat offset src_off of the
    _mvextremes frame (av1_set_mv_limits, then
    av1_set_subpel_mv_search_range), as motion.subpel_limits restates them."""
    from lavish_dsp import motion as M
    org = src_off - X.BORDER * X.STRIDE - X.BORDER
    y, x = org // X.STRIDE, org % X.STRIDE
    mi_rows, mi_cols = ((X.H + 7) & ~7) // 4, ((X.W + 7) & ~7) // 4
    return M.subpel_limits(M.block_mv_limits(mi_rows, mi_cols, y // 4, x // 4, bh // 4, bw // 4,
                                             X.BORDER), ref_mv)


def subpel_records(fp_jobs, bw, bh, starts=None):
    """SUBPEL_JOB_DTYPE records continuing full-pel JOB records: the block's
    own SubpelMvLimits, the start `starts` ([n, 2], 1/8 pel) or (0, 0)."""
    from lavish_dsp import motion as M
    sj = np.zeros(len(fp_jobs), M.SUBPEL_JOB_DTYPE)
    for i, jb in enumerate(fp_jobs):
        ref_mv = (int(jb["ref_mv_row"]), int(jb["ref_mv_col"]))
        lim = block_limits(int(jb["src_off"]), bw, bh, ref_mv)
        sj["col_min"][i], sj["col_max"][i], sj["row_min"][i], sj["row_max"][i] = lim
    for f in ("src_off", "ref_off", "ref_mv_row", "ref_mv_col"):
        sj[f] = fp_jobs[f]
    if starts is not None:
        sj["start_row"], sj["start_col"] = np.asarray(starts).T
    return sj


def pick_lower(a, b):
    """Per row a, unless b's besterr is strictly lower (facade.c:670)."""
    return np.where((b[:, 2] < a[:, 2])[:, None], b, a)


# ------------------------------------------------------------------ fixture --
CASE_FIELDS = ["form", "bw", "bh", "method", "search_type", "allow_hp", "forced_stop", "iters",
               "cost", "error_per_bit", "mask_stride", "plane"]
ROW_FIELDS = (["case"] + X.JOB_FIELDS + ["second_off", "mask_off", "invert_mask"] +
              RESULT_FIELDS)
Group = collections.namedtuple("Group", "index prm plane cjobs rows")


def load_fixture():
    """fix_subpel_comp.npz joined with what it continues: fix_mcomp_comp.npz's
    planes, and its pools in front of the fixture's own part (every offset
    indexes the joined pool)."""
    F = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                  "fix_subpel_comp.npz")))
    MC = S.load_fixture()
    F.update({k: v for k, v in MC.items() if k.startswith(("src__", "refs__"))})
    for k in ("second", "mask", "wsrc", "omask"):
        F[k] = np.concatenate([MC[k], F[k + "_own"]])
    return F


def job_records(rows, J):
    from lavish_dsp import motion as M
    rec = np.zeros(len(rows), M.SUBPEL_JOB_DTYPE)
    for f in X.JOB_FIELDS:
        rec[f] = rows[:, J[f]]
    return M.comp_subpel_jobs(rec, rows[:, J["second_off"]], rows[:, J["mask_off"]],
                              rows[:, J["invert_mask"]])


def fixture_groups(F):
    """The stored cases: parameters (a dict), the plane set's name, the
    COMP_SUBPEL_JOB_DTYPE records and the reference's rows."""
    J = {n: i for i, n in enumerate(ROW_FIELDS)}
    assert [str(s) for s in F["row_fields"]] == ROW_FIELDS
    assert [str(s) for s in F["case_fields"]] == CASE_FIELDS
    for ci, vals in enumerate(F["cases"]):
        prm = dict(zip(CASE_FIELDS, (int(v) for v in vals)))
        rows = F["rows"][F["rows"][:, 0] == ci]
        yield Group(ci, prm, str(F["planes"][prm["plane"]]), job_records(rows, J), rows)


def group_cost(prm):
    return S.cost_of(prm["cost"], prm["error_per_bit"], 0, prm["allow_hp"])


def group_expected(F, g, **kw):
    """A group's rows through the restatement: [n, 5] (RESULT_FIELDS)."""
    p = g.prm
    return run_batch(p["form"], F["src__" + g.plane].reshape(-1), F["refs__" + g.plane].reshape(-1),
                     X.STRIDE, p["bw"], p["bh"], g.cjobs, group_cost(p), p["method"],
                     p["search_type"], p["forced_stop"], bool(p["allow_hp"]), p["iters"],
                     F["second"], F["mask"], p["mask_stride"], F["wsrc"], F["omask"], **kw)


# ---------------------------------------------------------------- coverage --
def check_coverage(F):
    """The conditions a fixture that pins something meets; returns the counts
    (the generator stops unless its rows meet them;
    tests/test_subpel_comp_cpu.py asserts the same on the committed file)."""
    J = {n: i for i, n in enumerate(ROW_FIELDS)}
    facts = {}
    for form in (AVG, MASK, OBMC):
        f = dict(rows=0, moved=0, half=0, quarter=0, eighth=0, second_level=0, oob=0)
        for g in fixture_groups(F):
            if g.prm["form"] != form:
                continue
            p = g.prm
            for cj, row in zip(g.cjobs, g.rows):
                r, c = int(row[J["best_row"]]), int(row[J["best_col"]])
                f["rows"] += 1
                f["moved"] += (r, c) != (int(row[J["start_row"]]), int(row[J["start_col"]]))
                low = (r | c) & 7
                f["half"] += low == 4
                f["quarter"] += low in (2, 6)
                f["eighth"] += bool(low & 1)
                e = make_env(form, F["src__" + g.plane].reshape(-1),
                                F["refs__" + g.plane].reshape(-1), X.STRIDE, p["bw"], p["bh"], cj,
                                group_cost(p), F["second"], F["mask"], p["mask_stride"],
                                F["wsrc"], F["omask"])
                tr = {}
                search(e, p["method"], p["search_type"], p["forced_stop"], bool(p["allow_hp"]),
                          p["iters"], trace=tr)
                f["second_level"] += tr["second_level"] > 0
                f["oob"] += tr["oob"] > 0
        assert 3 * f["moved"] >= f["rows"], (form, f)
        assert f["half"] and f["quarter"] and f["eighth"] and f["second_level"] and f["oob"], \
            (form, f)
        facts[form] = f
    # OBMC USE_2_TAPS_ORIG from a nonzero start: mv (0, 0)'s centre error
    ob = dict(nonzero=0, centre_differs=0, changes_result=0)
    for g in fixture_groups(F):
        p = g.prm
        if p["form"] != OBMC or p["search_type"] != USE_2_TAPS_ORIG:
            continue
        for cj in g.cjobs:
            e = make_env(OBMC, None, F["refs__" + g.plane].reshape(-1), X.STRIDE, p["bw"],
                            p["bh"], cj, group_cost(p), wsrc=F["wsrc"], omask=F["omask"])
            if e.start == (0, 0):
                continue
            ob["nonzero"] += 1
            ob["centre_differs"] += e.err(0, 0, 0) != e.err(e.start[0], e.start[1], 0)
            args = (p["method"], p["search_type"], p["forced_stop"], bool(p["allow_hp"]),
                    p["iters"])
            a, b = search(e, *args), search(e, *args, obmc_centre_at_start=True)
            ob["changes_result"] += (a["best_row"], a["best_col"]) != (b["best_row"], b["best_col"])
    assert ob["nonzero"] and ob["centre_differs"] and ob["changes_result"], ob
    facts["obmc_centre"] = ob
    return facts
