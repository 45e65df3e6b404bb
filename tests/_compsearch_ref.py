"""numpy restatement of the compound, masked and OBMC full-pel searches
(av1/encoder/mcomp.c: av1_full_pixel_search with second_pred :1755-1895 over
diamond_search_sad's second_pred branch :1377-1405 and full_pixel_diamond
:1479-1526; av1_refining_search_8p_c :1683-1753; av1_obmc_full_pixel_search
:2173-2342), sequential as the reference runs them, over the block functions
of tests/_compref.py and the mv rates of tests/_mvextremes.py -- and the
reader of tests/golden/fix_mcomp_comp.npz.

The site tables are derived from the radii (1 << k for DIAMOND; r -> max(
(int)(1.5 r + 0.5), r + 1) for the first 12 NSTEP stages, tangent max((int)
(0.41 r), 1) once r > 5), not copied.

test_mcomp_comp_cpu.py pins every function here to the fixture (the
reference's own results); the GPU tests then use them at the sizes the
fixture cannot reach.
"""
import collections
import os

import numpy as np

import _compref as R
import _mvextremes as X

INVALID = -32768
COMP, REFINE8, OBMC = 0, 1, 2                    # the three searches
PLAIN, AVG, MASK = 0, 1, 2                       # forms of the block SAD
DIAMOND, NSTEP, NSTEP_8PT = 0, 1, 2              # SEARCH_METHODS values
METHOD_NAMES = {DIAMOND: "diamond", NSTEP: "nstep", NSTEP_8PT: "nstep_8pt"}
SAD_LAMBDA = {0: 0, 1: 32, 2: 15, 3: 8, 4: 0}    # mvsad_err_cost_'s L1 lambdas
SSE_LAMBDA = {0: 0, 1: 2, 2: 0, 3: 1, 4: 0}      # mv_err_cost_'s
NEIGHBORS8 = [(-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (1, -1), (-1, 1), (1, 1)]
NEIGHBORS4 = [(-1, 0), (0, -1), (0, 1), (1, 0)]


def site_table(method):
    """Per step (index 0 the smallest radius): (radius, [(dr, dc)] sites)."""
    def pts(r, t, n):
        s = [(-r, 0), (r, 0), (0, -r), (0, r), (-r, -t), (r, t), (-t, r), (t, -r), (-r, t),
             (r, -t), (t, r), (-t, -r)]
        return s[:n]
    if method == DIAMOND:
        return [(1 << k, pts(1 << k, 1 << k, 8)) for k in range(11)]
    out, r = [], 1
    for k in range(16 if method == NSTEP_8PT else 15):
        if r <= 5 or method == NSTEP_8PT:
            out.append((r, pts(r, r, 8)))
        else:
            out.append((r, pts(r, max(int(0.41 * r), 1), 12)))
        if k < 12:
            r = int(max(r * 1.5 + 0.5, r + 1))
    return out


_tables = {m: site_table(m) for m in (DIAMOND, NSTEP, NSTEP_8PT)}


def num_steps(method):
    return len(_tables[method])


Cost = collections.namedtuple("Cost", "ctype epb spb mvjcost mvcost")


class Env:
    """One job: its planes (flat), the invariant blocks and the mv costs."""

    def __init__(self, src, ref, stride, bw, bh, job, cost, form=PLAIN, second=None, mask=None,
                 invert=0, wsrc=None, omask=None):
        self.ref, self.stride, self.bw, self.bh = ref, stride, bw, bh
        self.idx = np.arange(bh)[:, None] * stride + np.arange(bw)[None, :]
        self.ref_off = int(job["ref_off"])
        if src is not None:
            self.src = src[int(job["src_off"]) + self.idx].astype(np.int64)
        self.lim = [int(job[f]) for f in ("col_min", "col_max", "row_min", "row_max")]
        self.ref_mv = (int(job["ref_mv_row"]), int(job["ref_mv_col"]))
        # get_fullmv_from_mv (mv.h:28): (x + 3 + (x >= 0)) >> 3
        self.full_ref = tuple((v + 3 + (v >= 0)) >> 3 for v in self.ref_mv)
        self.cost, self.form = cost, form
        self.second, self.mask, self.invert = second, mask, invert
        self.wsrc, self.omask = wsrc, omask
        self.memo = {}

    def in_range(self, r, c):
        return self.lim[0] <= c <= self.lim[1] and self.lim[2] <= r <= self.lim[3]

    def clamp(self, r, c):
        return (min(max(r, self.lim[2]), self.lim[3]), min(max(c, self.lim[0]), self.lim[1]))

    def block(self, r, c):
        return self.ref[self.ref_off + r * self.stride + c + self.idx].astype(np.int64)

    def pred(self, r, c):
        if self.form == MASK:
            return R.mask_pred(self.block(r, c), self.second, self.mask, self.invert)
        if self.form == AVG:
            return R.avg_pred(self.block(r, c), self.second)
        return self.block(r, c)

    def sad(self, r, c):
        """get_mvpred_compound_sad, or osdf for an OBMC job."""
        if (r, c) not in self.memo:
            if self.wsrc is not None:
                v = int(R.obmc_sad(self.block(r, c), self.wsrc, self.omask))
            else:
                v = int(np.abs(self.pred(r, c) - self.src).sum())
            self.memo[(r, c)] = v
        return self.memo[(r, c)]

    def var(self, r, c):
        """svaf / msvf at offset (0, 0), vf, or ovf."""
        if self.wsrc is not None:
            return int(R.obmc_variance(self.block(r, c), self.wsrc, self.omask, 8)[0])
        return int(R.variance(self.src, self.pred(r, c), 8)[0])

    def _rate(self, dr, dc):
        return int(X.mv_rate(self.cost.mvjcost, self.cost.mvcost, dr, dc, (0, 0)))

    def mvsad(self, r, c):
        """mvsad_err_cost_ (mcomp.c:329-350) of a full-pel mv."""
        dr, dc = (r - self.full_ref[0]) * 8, (c - self.full_ref[1]) * 8
        if self.cost.ctype == 0:
            return (self._rate(dr, dc) * self.cost.spb + 256) >> 9
        return (SAD_LAMBDA[self.cost.ctype] * (abs(dr) + abs(dc))) >> 3

    def mverr(self, r, c):
        """mv_err_cost_ (mcomp.c:290-314) of a full-pel mv."""
        dr, dc = r * 8 - self.ref_mv[0], c * 8 - self.ref_mv[1]
        if self.cost.ctype == 0:
            return (self._rate(dr, dc) * self.cost.epb + 8192) >> 14
        return (SSE_LAMBDA[self.cost.ctype] * (abs(dr) + abs(dc))) >> 3

    def var_cost(self, r, c):
        v = self.var(r, c) + self.mverr(r, c)
        return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)       # (an int in the reference)


def _scan(e, best, r, c, sites):
    """The two-stage strict `<` over `sites` around (r, c): (best, site or -1)."""
    hit = -1
    for i, (dr, dc) in enumerate(sites):
        if dr is None or not e.in_range(r + dr, c + dc):
            continue
        s = e.sad(r + dr, c + dc)
        if s < best:
            s += e.mvsad(r + dr, c + dc)
            if s < best:
                best, hit = s, i
    return best, hit


def diamond_search_sad(e, method, start, search_step, second, st):
    """The second_pred branch of diamond_search_sad: (best mv, num00,
    second_best)."""
    tab = _tables[method]
    r, c = e.clamp(*start)
    best = e.mvsad(r, c) + e.sad(r, c)
    off_center, center = False, 0
    step = len(tab) - search_step - 1
    while step >= 0:
        rad, sites = tab[step]
        best, hit = _scan(e, best, r, c, sites)
        st["steps"] += 1
        if hit >= 0:
            second = (r, c)
            r, c = r + sites[hit][0], c + sites[hit][1]
            off_center = True
        if not off_center:
            center += 1
        if hit < 0 and step > 2:
            while step > 2 and tab[step - 1][0] == tab[step][0]:
                center += 1
                step -= 1
        step -= 1
    return (r, c), center, second


def comp_full_pixel_search(e, method, step_param):
    """av1_full_pixel_search with second_pred (or plain: no mesh, no cost
    list): a result record as a dict."""
    st = {"steps": 0}
    start = e.start
    second = (INVALID, INVALID)
    best, n, second = diamond_search_sad(e, method, start, step_param, second, st)
    sme = e.var_cost(*best)
    further = num_steps(method) - 1 - step_param
    while n < further:
        n += 1
        mv, num00, second = diamond_search_sad(e, method, start, step_param + n, second, st)
        t = e.var_cost(*mv)
        if t < sme:
            sme, best = t, mv
        n += num00
    return dict(best_row=best[0], best_col=best[1], second_row=second[0], second_col=second[1],
                bestsme=sme, steps=st["steps"])


def refining_search_8p(e):
    r, c = e.clamp(*e.start)
    best = e.sad(r, c) + e.mvsad(r, c)
    seen = {(r, c)}
    steps = 0
    for _ in range(3):
        # the 7x7 grid follows the centre: a neighbour is at most 3 away from
        # the start after 3 rounds, so the grid never clips and a set does
        sites = [(None, None) if (r + dr, c + dc) in seen else (dr, dc) for dr, dc in NEIGHBORS8]
        seen |= {(r + dr, c + dc) for dr, dc in NEIGHBORS8}
        best, hit = _scan(e, best, r, c, sites)
        steps += 1
        if hit < 0:
            break
        r, c = r + NEIGHBORS8[hit][0], c + NEIGHBORS8[hit][1]
    return dict(best_row=r, best_col=c, second_row=r, second_col=c, bestsme=best, steps=steps)


def obmc_diamond_search_sad(e, method, start, search_step, st):
    tab = _tables[method]
    r0, c0 = e.clamp(*start)
    r, c = r0, c0
    best = e.sad(r, c) + e.mvsad(r, c)
    num00 = 0
    for step in range(len(tab) - search_step - 1, -1, -1):
        sites = tab[step][1]
        best, hit = _scan(e, best, r, c, sites)
        st["steps"] += 1
        if hit >= 0:
            r, c = r + sites[hit][0], c + sites[hit][1]
        elif (r, c) == (r0, c0):     # by position, as the reference (mcomp.c:2286)
            num00 += 1
    return (r, c), num00


def obmc_full_pixel_search(e, method, step_param, fast):
    st = {"steps": 0}
    if fast:
        r, c = e.clamp(*e.start)
        best = e.sad(r, c) + e.mvsad(r, c)
        for _ in range(8):
            best, hit = _scan(e, best, r, c, NEIGHBORS4)
            st["steps"] += 1
            if hit < 0:
                break
            r, c = r + NEIGHBORS4[hit][0], c + NEIGHBORS4[hit][1]
        sme, bmv = e.var_cost(r, c), (r, c)
    else:
        bmv, n = obmc_diamond_search_sad(e, method, e.start, step_param, st)
        sme = e.var_cost(*bmv)
        further = num_steps(method) - 1 - step_param
        num00 = 0
        while n < further:
            n += 1
            if num00:
                num00 -= 1
                continue
            mv, num00 = obmc_diamond_search_sad(e, method, e.start, step_param + n, st)
            t = e.var_cost(*mv)
            if t < sme:
                sme, bmv = t, mv
    return dict(best_row=bmv[0], best_col=bmv[1], second_row=INVALID, second_col=INVALID,
                bestsme=sme, steps=st["steps"])


# ------------------------------------------------------------------ batches --
RESULT_FIELDS = ["best_row", "best_col", "second_row", "second_col", "bestsme", "steps"]


def cost_of(ctype, epb, spb, hp=False):
    from lavish_dsp import motion as M
    mj, mc = M.default_mv_cost_tables(bool(hp))
    return Cost(int(ctype), int(epb), int(spb), mj, mc)


def run_batch(search, form, src, ref, stride, bw, bh, cjobs, cost, method=DIAMOND, step_param=0,
              fast=0, second=None, mask=None, mask_stride=0, wsrc=None, omask=None):
    """The restatement over COMP_JOB_DTYPE records `cjobs` (flat planes and
    pools, as the device calls take them): a list of result dicts."""
    out = []
    n = bw * bh
    for cj in cjobs:
        jb = cj["base"]
        so, mo = int(cj["second_off"]), int(cj["mask_off"])
        if search == OBMC:
            e = Env(None, ref, stride, bw, bh, jb, cost,
                    wsrc=wsrc[so:so + n].astype(np.int64).reshape(bh, bw),
                    omask=omask[mo:mo + n].astype(np.int64).reshape(bh, bw))
        else:
            sec = msk = None
            if form != PLAIN:
                sec = second[so:so + n].astype(np.int64).reshape(bh, bw)
            if form == MASK:
                msk = R.window(mask[mo:], mask_stride, bw, bh).astype(np.int64)
            e = Env(src, ref, stride, bw, bh, jb, cost, form, sec, msk, int(cj["invert_mask"]))
        e.start = (int(jb["start_row"]), int(jb["start_col"]))
        if search == COMP:
            out.append(comp_full_pixel_search(e, method, step_param))
        elif search == REFINE8:
            out.append(refining_search_8p(e))
        else:
            out.append(obmc_full_pixel_search(e, method, step_param, fast))
    return out


# ------------------------------------------------------------------ fixture --
CASE_FIELDS = ["search", "form", "bw", "bh", "method", "step_param", "cost", "error_per_bit",
               "sad_per_bit", "hp_tables", "mask_stride", "fast_obmc", "kind"]
ROW_FIELDS = (["case"] + X.JOB_FIELDS + ["second_off", "mask_off", "invert_mask"] +
              RESULT_FIELDS)
Group = collections.namedtuple("Group", "index prm kind cjobs rows")


def load_fixture():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "fix_mcomp_comp.npz")))


def comp_job_records(rows, J):
    from lavish_dsp import motion as M
    rec = np.zeros(len(rows), M.JOB_DTYPE)
    for f in X.JOB_FIELDS:
        rec[f] = rows[:, J[f]]
    return M.comp_jobs(rec, rows[:, J["second_off"]], rows[:, J["mask_off"]],
                       rows[:, J["invert_mask"]])


def fixture_groups(F):
    """The stored cases: parameters (a dict), plane kind, the COMP_JOB_DTYPE
    records and the reference's rows."""
    J = {n: i for i, n in enumerate(ROW_FIELDS)}
    assert [str(s) for s in F["row_fields"]] == ROW_FIELDS
    assert [str(s) for s in F["case_fields"]] == CASE_FIELDS
    for ci, vals in enumerate(F["cases"]):
        prm = dict(zip(CASE_FIELDS, (int(v) for v in vals)))
        rows = F["rows"][F["rows"][:, 0] == ci]
        yield Group(ci, prm, str(F["kinds"][prm["kind"]]), comp_job_records(rows, J), rows)


def group_expected(F, g):
    """A group's rows through the restatement: [n, 6] (RESULT_FIELDS)."""
    p = g.prm
    res = run_batch(p["search"], p["form"], F["src__" + g.kind].reshape(-1),
                    F["refs__" + g.kind].reshape(-1), X.STRIDE, p["bw"], p["bh"], g.cjobs,
                    cost_of(p["cost"], p["error_per_bit"], p["sad_per_bit"], p["hp_tables"]),
                    p["method"], p["step_param"], p["fast_obmc"], F["second"], F["mask"],
                    p["mask_stride"], F["wsrc"], F["omask"])
    return np.array([[r[f] for f in RESULT_FIELDS] for r in res], np.int64)
