"""numpy restatement of the high-bit-depth compound, masked and OBMC motion
searches -- av1_full_pixel_search with second_pred, av1_refining_search_8p_c,
av1_obmc_full_pixel_search, av1_find_best_sub_pixel_tree / _pruned /
_pruned_more with second_pred and av1_find_best_obmc_sub_pixel_tree_up
(USE_2_TAPS_ORIG) of av1/encoder/mcomp.c with the members highbd_set_var_fns
binds (av1/encoder/encoder_utils.h) -- and the reader of
tests/golden/fix_mcomp_comp_hbd.npz.

Nothing is walked here: the searches are _compsearch_ref's and
_compsubpel_ref's over Env subclasses.  Only the sources are new:
  * the SAD: sdaf / msdf / osdf under their _bits8 / _bits10 / _bits12
    wrappers, (the whole block's SAD) >> (bd - 8) before the mv SAD cost;
  * the variance: svaf / msvf at offset (0, 0) and ovf at the depth
    (_compref.variance / obmc_variance: 8 bits truncate, 10 / 12 round the
    sums and clamp at 0);
  * the sub-pel error: the u16 bilinear passes (_pixref.bilinear, highbd),
    aom_highbd_comp_avg_pred / _comp_mask_pred or the OBMC difference, then
    the depth's variance; the centre error the same at the full-pel floor
    (setup_center_error's is_cur_buf_hbd branch), or at mv (0, 0) for OBMC.

test_mcomp_comp_hbd_cpu.py pins every function here to the fixture (the
reference's own results); the GPU tests then use them at the sizes the
fixture cannot reach.
"""
import collections
import os

import numpy as np

import _compref as R
import _compsearch_ref as S
import _compsubpel_ref as P
import _mvextremes as X
import _pixref as PX

COMP, REFINE8, OBMC = S.COMP, S.REFINE8, S.OBMC
PLAIN, AVG, MASK = S.PLAIN, S.AVG, S.MASK
INVALID, INT_MAX = S.INVALID, 0x7FFFFFFF
FULL_FIELDS = S.RESULT_FIELDS
SUB_FIELDS = P.RESULT_FIELDS


# ----------------------------------------------------------------- full pel --
class FullEnv(S.Env):
    """One full-pel job over flat uint16 planes at bit depth bd.  per_row:
    shift each row's SAD instead of the block's (what the reference does not
    do; only to show that the difference matters)."""

    def __init__(self, src, ref, stride, bw, bh, job, cost, bd, form=PLAIN, second=None,
                 mask=None, invert=0, wsrc=None, omask=None):
        S.Env.__init__(self, src, ref, stride, bw, bh, job, cost, form, second, mask, invert,
                       wsrc, omask)
        self.bd, self.per_row = bd, False
        self.start = (int(job["start_row"]), int(job["start_col"]))

    def row_sads(self, r, c):
        """aom_highbd_sad_avg / _masked_sad / _obmc_sad (or the plain SAD), per row."""
        if self.wsrc is not None:
            return ((np.abs(self.wsrc - self.block(r, c) * self.omask) + 2048) >> 12).sum(axis=1)
        return np.abs(self.pred(r, c) - self.src).sum(axis=1)

    def sad(self, r, c):
        if (r, c) not in self.memo:
            d, sh = self.row_sads(r, c), self.bd - 8
            self.memo[(r, c)] = int((d >> sh).sum()) if self.per_row else int(d.sum()) >> sh
        return self.memo[(r, c)]

    def var(self, r, c):
        if self.wsrc is not None:
            return int(R.obmc_variance(self.block(r, c), self.wsrc, self.omask, self.bd)[0])
        # (svaf / msvf: the prediction first -- the sign of the sum matters to
        # the 10 / 12-bit rounding; the plain form is vf(src, ref))
        if self.form == PLAIN:
            return int(R.variance(self.src, self.block(r, c), self.bd)[0])
        return int(R.variance(self.pred(r, c), self.src, self.bd)[0])


def full_env(search, form, src, ref, stride, bw, bh, cj, cost, bd, second=None, mask=None,
             mask_stride=0, wsrc=None, omask=None):
    """The FullEnv of one COMP_JOB_DTYPE record over flat planes and pools."""
    n = bw * bh
    so, mo = int(cj["second_off"]), int(cj["mask_off"])
    if search == OBMC:
        return FullEnv(None, ref, stride, bw, bh, cj["base"], cost, bd,
                       wsrc=wsrc[so:so + n].astype(np.int64).reshape(bh, bw),
                       omask=omask[mo:mo + n].astype(np.int64).reshape(bh, bw))
    sec = msk = None
    if form != PLAIN:
        sec = second[so:so + n].astype(np.int64).reshape(bh, bw)
    if form == MASK:
        msk = R.window(mask[mo:], mask_stride, bw, bh).astype(np.int64)
    return FullEnv(src, ref, stride, bw, bh, cj["base"], cost, bd, form, sec, msk,
                   int(cj["invert_mask"]))


def full_search(e, search, method, step_param, fast):
    if search == COMP:
        return S.comp_full_pixel_search(e, method, step_param)
    if search == REFINE8:
        return S.refining_search_8p(e)
    return S.obmc_full_pixel_search(e, method, step_param, fast)


def run_fullpel(search, form, src, ref, stride, bw, bh, cjobs, cost, bd, method=S.DIAMOND,
                step_param=0, fast=0, second=None, mask=None, mask_stride=0, wsrc=None,
                omask=None):
    """The restatement over COMP_JOB_DTYPE records: [n, 6] int64 (FULL_FIELDS)."""
    out = []
    for cj in cjobs:
        e = full_env(search, form, src, ref, stride, bw, bh, cj, cost, bd, second, mask,
                     mask_stride, wsrc, omask)
        r = full_search(e, search, method, step_param, fast)
        out.append([r[f] for f in FULL_FIELDS])
    return np.array(out, np.int64).reshape(-1, 6)


# ------------------------------------------------------------------ sub pel --
class SubEnv(P.Env):
    """One sub-pel job over flat uint16 planes at bit depth bd."""

    def __init__(self, src, ref, stride, bw, bh, job, cost, bd, form, second=None, mask=None,
                 invert=0, wsrc=None, omask=None):
        P.Env.__init__(self, src, ref, stride, bw, bh, job, cost, form, second, mask, invert,
                       wsrc, omask)
        self.bd = bd
        self.win = np.arange(bh + 1)[:, None] * stride + np.arange(bw + 1)[None, :]

    def err(self, r, c, search_type):
        """svaf / msvf / osvf at the 1/8-pel mv: (var, sse)."""
        off = self.ref_off + (r >> 3) * self.stride + (c >> 3)
        p = PX.bilinear(self.ref[off + self.win], c & 7, r & 7, highbd=True)
        if self.form == P.OBMC:
            v, sse = R.obmc_variance(p, self.wsrc, self.omask, self.bd)
        else:
            if self.form == P.AVG:
                p = R.avg_pred(p, self.second)
            else:
                p = R.mask_pred(p, self.second, self.mask, self.invert)
            v, sse = R.variance(p, self.src, self.bd)
        return int(v), int(sse)


def sub_env(form, src, ref, stride, bw, bh, cj, cost, bd, second=None, mask=None, mask_stride=0,
            wsrc=None, omask=None):
    """The SubEnv of one COMP_SUBPEL_JOB_DTYPE record (form: P.AVG / MASK / OBMC)."""
    n = bw * bh
    so, mo = int(cj["second_off"]), int(cj["mask_off"])
    if form == P.OBMC:
        return SubEnv(None, ref, stride, bw, bh, cj["base"], cost, bd, P.OBMC,
                      wsrc=wsrc[so:so + n].astype(np.int64).reshape(bh, bw),
                      omask=omask[mo:mo + n].astype(np.int64).reshape(bh, bw))
    sec = second[so:so + n].astype(np.int64).reshape(bh, bw)
    msk = R.window(mask[mo:], mask_stride, bw, bh).astype(np.int64) if form == P.MASK else None
    return SubEnv(src, ref, stride, bw, bh, cj["base"], cost, bd, form, sec, msk,
                  int(cj["invert_mask"]))


def run_subpel(form, src, ref, stride, bw, bh, cjobs, cost, bd, method=P.PRUNED_MORE,
               forced_stop=P.EIGHTH_PEL, allow_hp=False, iters=1, second=None, mask=None,
               mask_stride=0, wsrc=None, omask=None, fullpel=None, start_from=0):
    """The restatement over COMP_SUBPEL_JOB_DTYPE records: [n, 5] int64
    (SUB_FIELDS).  fullpel: [n, >= 4] (best row, best col, second row, second
    col) to start from, as the device call chains (start_from 1: the
    second-best mv; a job without a usable one gives P.NO_SEARCH)."""
    out = []
    for i, cj in enumerate(cjobs):
        e = sub_env(form, src, ref, stride, bw, bh, cj, cost, bd, second, mask, mask_stride, wsrc,
                    omask)
        start = None
        if fullpel is not None:
            fr, fc = (int(v) for v in fullpel[i][2 * start_from:2 * start_from + 2])
            start = (8 * fr, 8 * fc)
            if start_from and (INVALID in (fr, fc) or not e.in_range(*start)):
                out.append([P.NO_SEARCH[f] for f in SUB_FIELDS])
                continue
        r = P.search(e, method, P.USE_2_TAPS_ORIG, forced_stop, allow_hp, iters, start)
        out.append([r[f] for f in SUB_FIELDS])
    return np.array(out, np.int64).reshape(-1, 5)


# ------------------------------------------------------------------ fixture --
CASE_FIELDS = ["search", "form", "bd", "bw", "bh", "method", "step_param", "cost",
               "error_per_bit", "sad_per_bit", "hp_tables", "mask_stride", "fast_obmc", "has_sp",
               "sp_method", "sp_forced_stop", "sp_allow_hp", "sp_iters", "plane"]
SP_LIMITS = ["sp_col_min", "sp_col_max", "sp_row_min", "sp_row_max"]
ROW_FIELDS = (["case"] + X.JOB_FIELDS + ["second_off", "mask_off", "invert_mask"] + FULL_FIELDS +
              SP_LIMITS + ["sp0_" + f for f in SUB_FIELDS] + ["sp1_" + f for f in SUB_FIELDS])
Group = collections.namedtuple("Group", "index prm plane cjobs sjobs rows J")
SP_FORM = {AVG: P.AVG, MASK: P.MASK}


def load_fixture():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "fix_mcomp_comp_hbd.npz")))


def sp_form(prm):
    return P.OBMC if prm["search"] == OBMC else SP_FORM[prm["form"]]


def fixture_groups(F):
    """The stored cases: parameters, the plane set's name, the COMP_JOB_DTYPE
    and COMP_SUBPEL_JOB_DTYPE records (the sub-pel jobs carry the
    SubpelMvLimits; their start fields stay 0: the searches start from the
    full-pel records) and the reference's rows."""
    from lavish_dsp import motion as M
    J = {n: i for i, n in enumerate(ROW_FIELDS)}
    assert [str(s) for s in F["row_fields"]] == ROW_FIELDS
    assert [str(s) for s in F["case_fields"]] == CASE_FIELDS
    for ci, vals in enumerate(F["cases"]):
        prm = dict(zip(CASE_FIELDS, (int(v) for v in vals)))
        rows = F["rows"][F["rows"][:, 0] == ci]
        cj = S.comp_job_records(rows, J)
        sj = np.zeros(len(rows), M.SUBPEL_JOB_DTYPE)
        for f in ("src_off", "ref_off", "ref_mv_row", "ref_mv_col"):
            sj[f] = cj["base"][f]
        for f in ("col_min", "col_max", "row_min", "row_max"):
            sj[f] = rows[:, J["sp_" + f]]
        csj = M.comp_subpel_jobs(sj, cj["second_off"], cj["mask_off"], cj["invert_mask"])
        yield Group(ci, prm, str(F["planes"][prm["plane"]]), cj, csj, rows, J)


def group_cost(prm, subpel=False):
    return S.cost_of(prm["cost"], prm["error_per_bit"], prm["sad_per_bit"],
                     prm["sp_allow_hp"] if subpel else prm["hp_tables"])


def group_planes(F, g):
    return F["src__" + g.plane].reshape(-1), F["refs__" + g.plane].reshape(-1)


def group_fullpel(F, g):
    """A group's rows through the full-pel restatement: [n, 6]."""
    p = g.prm
    src, ref = group_planes(F, g)
    return run_fullpel(p["search"], p["form"], src, ref, X.STRIDE, p["bw"], p["bh"], g.cjobs,
                       group_cost(p), p["bd"], p["method"], p["step_param"], p["fast_obmc"],
                       F["second"], F["mask"], p["mask_stride"], F["wsrc"], F["omask"])


def group_subpel(F, g, start_from, fullpel=None):
    """A group's rows through the sub-pel restatement from the fixture's
    full-pel records (or `fullpel`): [n, 5]."""
    p = g.prm
    src, ref = group_planes(F, g)
    fp = g.rows[:, g.J["best_row"]:g.J["second_col"] + 1] if fullpel is None else fullpel
    return run_subpel(sp_form(p), src, ref, X.STRIDE, p["bw"], p["bh"], g.sjobs,
                      group_cost(p, True), p["bd"], p["sp_method"], p["sp_forced_stop"],
                      bool(p["sp_allow_hp"]), p["sp_iters"], F["second"], F["mask"],
                      p["mask_stride"], F["wsrc"], F["omask"], fullpel=fp, start_from=start_from)


def sp_rows(g, start_from):
    a = g.J["sp%d_best_row" % start_from]
    return g.rows[:, a:a + 5]


# ----------------------------------------------------------------- coverage --
def form_name(p, invert=0):
    if p["search"] == OBMC:
        return "obmc_fast" if p["fast_obmc"] else "obmc"
    return ("plain", "avg", "mask_inv" if invert else "mask")[p["form"]]


def check_coverage(F):
    """What a fixture that pins something contains, from the reference's rows
    and the inputs alone; returns the counts (the generator stops unless its
    rows meet them; tests/test_mcomp_comp_hbd_cpu.py asserts the same on the
    committed file)."""
    f = collections.Counter()
    combos = set()
    sub = collections.Counter()
    for g in fixture_groups(F):
        p, J = g.prm, g.J
        bd, bw, bh, n = p["bd"], p["bw"], p["bh"], p["bw"] * p["bh"]
        src, ref = group_planes(F, g)
        cost = group_cost(p)
        combos.add((bd, "c", p["cost"]))
        if p["search"] != REFINE8:
            combos.add((bd, "m", p["method"]))
        if p["form"] == MASK and p["mask_stride"] > bw:
            f["mask_stride_wide"] += 1
        fam = "ovf" if p["search"] == OBMC else "msvf" if p["form"] == MASK else "svaf"
        sad_fam = {"ovf": "osdf", "msvf": "msdf", "svaf": "sdaf"}[fam]
        for cj, sj, row in zip(g.cjobs, g.sjobs, g.rows):
            name = form_name(p, int(cj["invert_mask"]))
            combos.add((bd, p["search"], name))
            br, bc = int(row[J["best_row"]]), int(row[J["best_col"]])
            sr, sc = int(row[J["second_row"]]), int(row[J["second_col"]])
            e = full_env(p["search"], p["form"], src, ref, X.STRIDE, bw, bh, cj, cost, bd,
                         F["second"], F["mask"], p["mask_stride"], F["wsrc"], F["omask"])
            if bd > 8 and e.block(br, bc).max() & ((1 << (bd - 8)) - 1):
                f["low_bits"] += 1
            if bd > 8 and p["form"] != PLAIN or p["search"] == OBMC and bd > 8:
                q = full_env(p["search"], p["form"], src, ref, X.STRIDE, bw, bh, cj, cost, bd,
                             F["second"], F["mask"], p["mask_stride"], F["wsrc"], F["omask"])
                q.per_row = True
                alt = full_search(q, p["search"], p["method"], p["step_param"], p["fast_obmc"])
                f["per_row_%s_%d" % (sad_fam, bd)] += (alt["best_row"], alt["best_col"]) != (br, bc)
            if p["search"] == COMP:
                f["second_valid" if sr != INVALID else "second_invalid"] += 1
            if p["form"] != PLAIN or p["search"] == OBMC:
                # the variance at the best mv: the sums before their rounding
                if p["search"] == OBMC:
                    v = e.wsrc - e.block(br, bc) * e.omask
                    rr = (np.abs(v) + 2048) >> 12
                    d = np.where(v < 0, -rr, rr)
                else:
                    d = e.pred(br, bc) - e.src
                sm, ss = int(d.sum()), int((d * d).sum())
                if bd > 8:
                    sh = bd - 8
                    if sm < 0 and (sm + (1 << (sh - 1))) >> sh != -((-sm + (1 << (sh - 1))) >> sh):
                        f["neg_round_" + fam] += 1
                    _, sse_r, sum_r = PX.variance_tail(sm, ss, bd, n)
                    f["clamped_" + fam] += int(PX.before_clamp(sse_r, sum_r, n)) < 0
                if bd == 12 and p["search"] != OBMC and \
                        {int(e.src.min()), int(e.src.max()), int(e.pred(br, bc).min()),
                         int(e.pred(br, bc).max())} == {0, 4095}:
                    f["max_vs_zero"] += 1
            if not p["has_sp"]:
                continue
            # the sub-pel rows
            combos.add((bd, "sub", "obmc" if p["search"] == OBMC else name))
            for k in (0, 1):
                a = J["sp%d_best_row" % k]
                r, c, err = (int(v) for v in row[a:a + 3])
                if k == 1:
                    if p["search"] != COMP:
                        continue
                    if err == INT_MAX:
                        f["sp1_int_max"] += 1
                        continue
                    f["sp1_searched"] += 1
                st = (8 * sr, 8 * sc) if k else (8 * br, 8 * bc)
                key = "obmc" if p["search"] == OBMC else "mask" if p["form"] == MASK else "avg"
                sub[key + "_rows"] += 1
                sub[key + "_moved"] += (r, c) != st
                low = (r | c) & 7
                sub["half"] += low == 4
                sub["quarter"] += low in (2, 6)
                sub["eighth"] += bool(low & 1)
                se = sub_env(sp_form(p), src, ref, X.STRIDE, bw, bh, sj, group_cost(p, True), bd,
                             F["second"], F["mask"], p["mask_stride"], F["wsrc"], F["omask"])
                tr = {}
                got = P.search(se, p["sp_method"], P.USE_2_TAPS_ORIG, p["sp_forced_stop"],
                               bool(p["sp_allow_hp"]), p["sp_iters"], st, trace=tr)
                sub["second_level"] += tr["second_level"] > 0
                sub["oob"] += tr["oob"] > 0
                if p["search"] == OBMC:
                    alt = P.search(se, p["sp_method"], P.USE_2_TAPS_ORIG, p["sp_forced_stop"],
                                   bool(p["sp_allow_hp"]), p["sp_iters"], st,
                                   obmc_centre_at_start=True)
                    sub["obmc_centre_matters"] += any(alt[k2] != got[k2] for k2 in SUB_FIELDS)
    for bd in (8, 10, 12):
        for m in (S.DIAMOND, S.NSTEP, S.NSTEP_8PT):
            assert (bd, "m", m) in combos, (bd, m)
        for c in (X.ENTROPY, X.L1, X.NONE):
            assert (bd, "c", c) in combos, (bd, c)
        for search, names in ((COMP, ("avg", "mask", "mask_inv")),
                              (REFINE8, ("plain", "avg", "mask", "mask_inv")),
                              (OBMC, ("obmc", "obmc_fast"))):
            for nm in names:
                assert (bd, search, nm) in combos, (bd, search, nm)
        for nm in ("avg", "mask", "mask_inv", "obmc"):
            assert (bd, "sub", nm) in combos, (bd, "sub", nm)
    need = ["mask_stride_wide", "low_bits", "second_valid", "second_invalid", "sp1_int_max",
            "sp1_searched", "max_vs_zero"]
    need += ["per_row_%s_%d" % (s, bd) for s in ("sdaf", "msdf", "osdf") for bd in (10, 12)]
    need += [k + fam for k in ("neg_round_", "clamped_") for fam in ("svaf", "msvf", "ovf")]
    for k in need:
        assert f[k] > 0, (k, dict(f))
    for key in ("avg", "mask", "obmc"):
        assert 3 * sub[key + "_moved"] >= sub[key + "_rows"] > 0, dict(sub)
    for k in ("half", "quarter", "eighth", "second_level", "oob", "obmc_centre_matters"):
        assert sub[k] > 0, (k, dict(sub))
    return dict(f), dict(sub)
