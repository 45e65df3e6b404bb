"""Golden fixture of the compound, masked and OBMC full-pel searches, from the
reference's own C text executed by cinterp.py (the executor extends
gen_fixtures.py's FullpelRef: aom_dsp/sad_av1.c joins the translation unit,
the msdf / sdaf / msvf / svaf / osdf / ovf members and the second_pred / mask
/ wsrc / obmc_mask buffers are set).

  fix_mcomp_comp.npz
    src__<kind>, refs__<kind>  the planes of tests/_mvextremes.py
    second, mask               uint8 pools the rows' second_off / mask_off
                               index (second_pred blocks compact, mask blocks
                               at the case's mask_stride)
    wsrc, omask                int32 pools of the OBMC rows (compact blocks)
    kinds, case_fields, cases  one case per call: the search (0
                               av1_full_pixel_search with second_pred, 1
                               av1_refining_search_8p_c, 2
                               av1_obmc_full_pixel_search), the form (0 plain,
                               1 average, 2 mask) and the parameters
    row_fields, rows           one search each: the job, its offsets and
                               invert_mask, and the reference's best mv,
                               second_best_mv and return value; `steps` (the
                               reference reports none) is the count of
                               tests/_compsearch_ref.py, whose walk the
                               other five fields pin

Every row is also run through tests/_compsearch_ref.py here and must agree:
a disagreement stops the generation.

No OBMC walk that returns to its start exists, on these planes or any other:
obmc_diamond_search_sad moves only to a position whose cost (osdf + mv SAD
cost, a function of the position alone) is strictly below best_sad, which
starts as the start position's own cost and only falls, so the start can
never be entered again.  The position test of num00 (mcomp.c:2286,
best_address == init_ref) therefore equals "has not moved yet"; a search of
4000 random NSTEP jobs with the restatement found none either.  The kernel
and the restatement still compare positions, as the reference does.

Usage: python tests/golden/gen_fix_mcomp_comp.py
Generation time: 26 s on one CPU core for 181 rows in 91 cases (the blocks are
4x4 to 16x16, most searches start at step_param 5 or later); the file is
163 KB.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "aom-av1-lavish_amd"))
import _compsearch_ref as S  # noqa: E402
import _mvextremes as X  # noqa: E402
import cinterp as C  # noqa: E402
from gen_fixtures import (MS_INIT, MV_MAX, REF, FullpelRef, _get, _set, check_errors,  # noqa: E402
                          nmv_cost_tables)

METHODS = ["DIAMOND", "NSTEP", "NSTEP_8PT"]           # index = SEARCH_METHODS value
COST_NAMES = {X.ENTROPY: "MV_COST_ENTROPY", X.L1: "MV_COST_L1_HDRES", X.NONE: "MV_COST_NONE"}
KINDS = ["flat_128_128", "flat_0_255", "ramp_x", "periodic_2", "noise"]
SIZES = [(4, 4), (8, 8), (16, 8), (16, 16)]


class CompRef(FullpelRef):
    """FullpelRef with the compound / OBMC members: the three searches."""

    def __init__(self, tables, stride, width, height, border):
        self.tu = tu = C.TU(REF, ["aom_dsp/sad.c", "aom_dsp/variance.c", "aom_dsp/sad_av1.c",
                                  "av1/encoder/mcomp.c"], C.reference_defines(REF))
        check_errors(tu, ["av1_full_pixel_search", "av1_set_mv_search_range",
                          "av1_refining_search_8p_c", "av1_obmc_full_pixel_search",
                          "aom_masked_sad4x4_c", "aom_obmc_variance4x4_c"] +
                     sorted({MS_INIT[m][0] for m in METHODS}))
        self.E = tu.enums
        self.stride, self.W, self.H, self.BORDER = stride, width, height, border
        self.cfgs = {}
        for m in METHODS:
            cfg = tu.struct_obj("search_site_config")
            fname, level = MS_INIT[m]
            tu.func(fname)(cfg, stride, level)
            self.cfgs[m] = cfg
        self.tabs = {}
        for nm in ("lp", "hp"):
            mj = tu.buffer("int", tables["mvjcost_" + nm].tolist())
            mc = [tu.buffer("int", tables["mvcost_" + nm][k].tolist()) for k in range(2)]
            self.tabs[nm] = (mj, [C.Pointer(c.buf, MV_MAX, c.ty) for c in mc])
        self.vtabs = {}

    def vtab(self, bw, bh):
        if (bw, bh) not in self.vtabs:
            vtab = FullpelRef.vtab(self, bw, bh)
            fn, sz = self.tu.func, "%dx%d" % (bw, bh)
            _set(vtab.buf[0], msdf=fn("aom_masked_sad" + sz), sdaf=fn("aom_sad%s_avg" % sz),
                 msvf=fn("aom_masked_sub_pixel_variance" + sz),
                 svaf=fn("aom_sub_pixel_avg_variance" + sz), osdf=fn("aom_obmc_sad" + sz),
                 ovf=fn("aom_obmc_variance" + sz))
        return self.vtabs[(bw, bh)]

    def params(self, bw, bh, mname, ctype, src_off, k, ref_off, ref_mv, lims, epb, spb, hp,
               second=None, mask=None, mask_stride=0, invert=0, wsrc=None, omask=None, fast=0):
        tu, E, stride = self.tu, self.E, self.stride
        vtab = self.vtab(bw, bh)
        sbuf = tu.struct_obj("struct buf_2d")
        _set(sbuf.buf[0], buf=C.Pointer(self.src_buf.buf, src_off, C.UCHAR), stride=stride,
             width=bw, height=bh)
        rbuf = tu.struct_obj("struct buf_2d")
        _set(rbuf.buf[0], buf=C.Pointer(self.ref_bufs[k].buf, ref_off, C.UCHAR), stride=stride,
             width=self.W, height=self.H)
        ms = tu.struct_obj("FULLPEL_MOTION_SEARCH_PARAMS")
        P = ms.buf[0]
        _set(P, bsize=E["BLOCK_%dX%d" % (bw, bh)], vfp=vtab, search_method=E[mname],
             search_sites=self.cfgs[mname], run_mesh_search=0, prune_mesh_search=0,
             mesh_search_mv_diff_threshold=4, force_mesh_thresh=0, fine_search_interval=0,
             is_intra_mode=0, fast_obmc_search=fast)
        buf = lambda t, a: None if a is None else tu.buffer(t, np.asarray(a).reshape(-1).tolist())
        _set(_get(P, "ms_buffers"), ref=rbuf, src=sbuf, second_pred=buf("uint8_t", second),
             mask=buf("uint8_t", mask), mask_stride=mask_stride, inv_mask=invert,
             wsrc=buf("int32_t", wsrc), obmc_mask=buf("int32_t", omask))
        L = tu.struct_obj("FullMvLimits").buf[0]
        _set(L, col_min=lims[0], col_max=lims[1], row_min=lims[2], row_max=lims[3])
        _set(P, mv_limits=L)
        rmv = tu.struct_obj("MV")
        _set(rmv.buf[0], row=ref_mv[0], col=ref_mv[1])
        mcp = _get(P, "mv_cost_params")
        mj, mc = self.tabs["hp" if hp else "lp"]
        _set(mcp, ref_mv=rmv, full_ref_mv=tu.func("get_fullmv_from_mv")(rmv),
             mv_cost_type=E[ctype], mvjcost=mj, error_per_bit=epb, sad_per_bit=spb)
        _get(mcp, "mvcost")[0], _get(mcp, "mvcost")[1] = mc[0], mc[1]
        vt = vtab.buf[0]
        _set(P, sdf=_get(vt, "sdf"), sdx4df=_get(vt, "sdx4df"), sdx3df=_get(vt, "sdx3df"))
        return ms

    def run(self, search, ms, start, step_param):
        """(best row, best col, second row, second col, return value)."""
        tu = self.tu
        smv = C.new_obj(tu.ctype("FULLPEL_MV"))
        _set(smv, row=start[0], col=start[1])
        best = tu.struct_obj("FULLPEL_MV")
        if search == S.COMP:
            sec = tu.struct_obj("FULLPEL_MV")
            v = tu.func("av1_full_pixel_search")(smv, ms, step_param, None, best, sec)
            second = mv_of(sec.buf[0])
        elif search == S.REFINE8:
            v = tu.func("av1_refining_search_8p_c")(ms, smv, best)
            second = (_get(best.buf[0], "row"), _get(best.buf[0], "col"))   # facade.c:621
        else:
            v = tu.func("av1_obmc_full_pixel_search")(smv, ms, step_param, best)
            second = (S.INVALID, S.INVALID)
        bm = best.buf[0]
        return [_get(bm, "row"), _get(bm, "col"), second[0], second[1], v]


def mv_of(obj):
    """(row, col) of a FULLPEL_MV cell.  MARK_MV_INVALID (mv.h:31-34) writes
    as_int through an int_mv cast, which the interpreter keeps as one 32-bit
    value in the first member: its two little-endian int16 halves."""
    row, col = _get(obj, "row"), _get(obj, "col")
    if not -32768 <= row <= 32767:
        s16 = lambda v: ((v & 0xFFFF) ^ 0x8000) - 0x8000
        row, col = s16(row), s16(row >> 16)
    return row, col


# ------------------------------------------------------------------- cases --
class Pools:
    def __init__(self, seed=4177):
        self.rng = np.random.default_rng(seed)
        self.second, self.mask, self.wsrc, self.omask = [], [], [], []

    def _add(self, pool, a):
        off = sum(len(x) for x in pool)
        pool.append(np.asarray(a).reshape(-1))
        return off

    def second_block(self, what, bw, bh, src=None, ref=None):
        if what == "random":
            a = self.rng.integers(0, 256, bw * bh)
        elif what == "max":
            a = np.full(bw * bh, 255)
        else:   # the average with `ref` (the candidate at the target mv) is exactly src
            a = np.clip(2 * src.astype(np.int64) - ref, 0, 255)
        # (an odd lead-in: the blocks are addressed at any byte offset)
        self._add(self.second, self.rng.integers(0, 256, int(self.rng.integers(0, 4))))
        return self._add(self.second, a)

    def mask_block(self, what, bw, bh, stride):
        m = self.rng.integers(0, 65, (bh, stride))     # (the columns past w are never read)
        if what == "zero":
            m[:, :bw] = 0
        elif what == "full":
            m[:, :bw] = 64
        elif what == "ramp":     # diagonal 0..64
            y, x = np.mgrid[0:bh, 0:bw]
            m[:, :bw] = (64 * (x + y)) // (bw + bh - 2)
        return self._add(self.mask, m)

    def obmc_block(self, what, src_block):
        n = src_block.size
        if what == "zero":
            m = np.zeros(n, np.int64)
        elif what == "full":       # with pre 255 and wsrc 0: the largest per-pixel term
            m = np.full(n, 4096)
        else:
            m = self.rng.integers(0, 4097, n)
        if what == "full":
            w = np.zeros(n, np.int64)
        else:     # src * 4096 less the neighbour's weighted prediction
            w = src_block.reshape(-1).astype(np.int64) * 4096 - \
                self.rng.integers(0, 256, n) * (4096 - m)
        return self._add(self.wsrc, w), self._add(self.omask, m)


def case(search, form, bw, bh, kind, method=0, step_param=0, cost=X.ENTROPY, epb=X.LOW_LAMBDA[0],
         spb=X.LOW_LAMBDA[1], hp=0, fast=0, ref_mv=(0, 0), start=(0, 0), njobs=2, salt=0,
         second="random", mask="random", invert=0, limits=None, obmc="random", target=None,
         starts=None):
    return dict(search=search, form=form, bw=bw, bh=bh, kind=kind, method=method,
                step_param=step_param, cost=cost, epb=epb, spb=spb, hp=hp, fast=fast,
                ref_mv=ref_mv, start=start, njobs=njobs, salt=salt, second=second, mask=mask,
                invert=invert, limits=limits, obmc=obmc, target=target, starts=starts)


def last_step(method):
    return S.num_steps(method) - 1


def all_cases():
    cs = []
    k = 0
    costs = (X.ENTROPY, X.L1, X.NONE)
    masks = ("ramp", "random", "zero", "full")
    # the compound forms under every method and plane kind
    for form, invert in ((S.AVG, 0), (S.MASK, 0), (S.MASK, 1)):
        for method in range(3):
            for kind in ("flat_128_128", "ramp_x", "periodic_2", "noise"):
                sp = (0, 5, last_step(method))[k % 3]
                bw, bh = SIZES[k % 2] if sp == 0 else SIZES[1 + k % 3]
                ref_mv = [(0, 0), (13, -21), (-40, 33)][k % 3]
                at = ((ref_mv[0] + 4) >> 3, (ref_mv[1] + 4) >> 3)
                start = at if k % 2 else (at[0] + 5 - k % 7, at[1] - 4 + k % 5)
                cs.append(case(S.COMP, form, bw, bh, kind, method, sp, costs[k % 3], ref_mv=ref_mv,
                               start=start, salt=k, mask=masks[k % 4], invert=invert))
                k += 1
    # windows narrowed to a point, a row, a column; a start outside the window
    for lim in ("point", "row", "col", "clamped"):
        for form in (S.AVG, S.MASK):
            cs.append(case(S.COMP, form, *SIZES[k % 3], ("periodic_2", "noise")[k % 2], k % 3,
                           (0, 5)[k % 2], costs[k % 2], ref_mv=(13, -21), start=(2, -3), salt=k,
                           mask=masks[k % 2], invert=k % 2, limits=lim))
            k += 1
        cs.append(case(S.REFINE8, (S.PLAIN, S.AVG, S.MASK)[k % 3], *SIZES[k % 4], "noise",
                       cost=costs[k % 2], ref_mv=(13, -21), start=(2, -3), salt=k, limits=lim))
        k += 1
        cs.append(case(S.OBMC, S.PLAIN, *SIZES[k % 3], "noise", k % 3, 5, costs[k % 2],
                       ref_mv=(13, -21), start=(2, -3), salt=k, limits=lim, fast=k % 2))
        k += 1
    # the largest SAD and variance: second_pred 255 on an all-0 source
    cs.append(case(S.COMP, S.AVG, 16, 16, "flat_0_255", 0, 5, njobs=1, second="max"))
    cs.append(case(S.COMP, S.MASK, 16, 16, "flat_0_255", 1, 5, njobs=1, second="max", mask="zero"))
    cs.append(case(S.REFINE8, S.MASK, 16, 16, "flat_0_255", njobs=1, second="max", mask="full",
                   invert=1))
    # the exact match of the average form off the start: on ramp_x (v = x >> 1)
    # the candidates of columns target - 2 .. target, any row, average to the
    # source exactly (the rounding absorbs a difference of -1), nothing else does
    for method in range(3):
        cs.append(case(S.COMP, S.AVG, 8, 8, "ramp_x", method, (5, 0, 5)[method], X.NONE, njobs=1,
                       salt=method, second="match", target=(2, -6)))
    cs.append(case(S.REFINE8, S.AVG, 8, 8, "ramp_x", cost=X.NONE, njobs=1, second="match",
                   target=(-1, -2)))
    # a lambda at which rate * error_per_bit passes 2^31
    epb, ref_mv, hp = X.HIGH_LAMBDA[1]
    cs.append(case(S.COMP, S.AVG, 8, 8, "noise", 0, 5, X.ENTROPY, epb, X.SAD_PER_BIT_TOP, hp,
                   ref_mv=ref_mv))
    cs.append(case(S.OBMC, S.PLAIN, 8, 8, "noise", 1, 5, X.ENTROPY, epb, X.SAD_PER_BIT_TOP, hp,
                   ref_mv=ref_mv))
    # the 8-point refinement: every form on every kind ...
    for form in (S.PLAIN, S.AVG, S.MASK):
        for kind in ("flat_128_128", "ramp_x", "periodic_2", "noise"):
            cs.append(case(S.REFINE8, form, *SIZES[k % 4], kind, cost=costs[k % 3],
                           ref_mv=(13, -21), start=(k % 3, -3 + k % 4), salt=k,
                           mask=masks[k % 4], invert=k % 2))
            k += 1
    # ... and walks of 0, 1 and 3 moves, straight and diagonal, that the mv
    # cost alone decides (a flat reference: every SAD is the same)
    for form in (S.AVG, S.PLAIN):
        cs.append(case(S.REFINE8, form, 8, 8, "flat_128_128", cost=X.L1, njobs=6,
                       starts=[(0, 0), (1, 0), (3, 0), (3, 3), (-2, 1), (0, -5)]))
    # OBMC: both branches, every method
    for fast in (0, 1):
        for method in range(3 if not fast else 1):
            for kind in ("flat_128_128", "periodic_2", "noise"):
                sp = (0, 5, last_step(method))[k % 3]
                bw, bh = SIZES[k % 2] if sp == 0 else SIZES[1 + k % 3]
                cs.append(case(S.OBMC, S.PLAIN, bw, bh, kind, method, sp, costs[k % 3],
                               ref_mv=(13, -21), start=(k % 5 - 2, 3 - k % 4), salt=k, fast=fast))
                k += 1
    for fast in (0, 1):
        # every SAD 0: the mv cost and the site order decide alone
        cs.append(case(S.OBMC, S.PLAIN, 8, 8, "noise", fast, 5, X.ENTROPY, ref_mv=(13, -21),
                       start=(6, -7), fast=fast, obmc="zero"))
        cs.append(case(S.OBMC, S.PLAIN, 16, 16, "flat_0_255", 2 * fast, 5, X.L1, njobs=1,
                       fast=fast, obmc="full"))
    return cs


def case_jobs(c):
    """JOB_DTYPE records of a case."""
    jobs = X.frame(c["bw"], c["bh"], c["ref_mv"], c["start"])
    n = len(c["starts"]) if c["starts"] else c["njobs"]
    jobs = X.spread(jobs, max(n, 3), c["salt"])[:n]
    lim = c["limits"]
    if lim in ("point", "row", "col"):
        jobs = X.narrowed(jobs, lim, (3, -2))
    elif lim == "clamped":          # the start lies outside the window on both axes
        jobs["row_max"] = np.minimum(jobs["row_max"], jobs["start_row"] - 2)
        jobs["col_min"] = np.maximum(jobs["col_min"], jobs["start_col"] + 3)
    if c["starts"]:
        at = ((c["ref_mv"][0] + 4) >> 3, (c["ref_mv"][1] + 4) >> 3)
        for jb, (dr, dc) in zip(jobs, c["starts"]):
            jb["start_row"], jb["start_col"] = at[0] + dr, at[1] + dc
    return jobs


def block(plane, off, bw, bh):
    idx = np.arange(bh)[:, None] * X.STRIDE + np.arange(bw)[None, :]
    return plane.reshape(-1)[off + idx]


def build_case(c, pools):
    """(case parameters with mask_stride, COMP_JOB records) of a case."""
    from lavish_dsp import motion as M
    src, refs = X.planes(c["kind"])
    jobs = case_jobs(c)
    bw, bh = c["bw"], c["bh"]
    c["mask_stride"] = bw + (8 if c["mask"] == "ramp" else 3 * (c["salt"] % 2))
    so, mo = [], []
    for jb in jobs:
        sblk = block(src, int(jb["src_off"]), bw, bh)
        if c["search"] == S.OBMC:
            a, b = pools.obmc_block(c["obmc"], sblk)
        else:
            a = b = 0
            if c["form"] != S.PLAIN:
                tgt = c["target"] or (0, 0)
                rblk = block(refs, int(jb["ref_off"]) + tgt[0] * X.STRIDE + tgt[1], bw, bh)
                a = pools.second_block(c["second"], bw, bh, sblk, rblk)
            if c["form"] == S.MASK:
                b = pools.mask_block(c["mask"], bw, bh, c["mask_stride"])
        so.append(a)
        mo.append(b)
    return M.comp_jobs(jobs, so, mo, c["invert"])


def main():
    t0 = time.time()
    from lavish_dsp import motion as M  # noqa: F401
    t = nmv_cost_tables()
    for hp in (False, True):
        mj, mc = M.default_mv_cost_tables(hp)
        nm = "hp" if hp else "lp"
        assert np.array_equal(mj, t["mvjcost_" + nm]) and np.array_equal(mc, t["mvcost_" + nm])
    pools = Pools()
    cases = all_cases()
    built = [build_case(c, pools) for c in cases]

    out = {"second": np.concatenate(pools.second).astype(np.uint8),
           "mask": np.concatenate(pools.mask).astype(np.uint8),
           "wsrc": np.concatenate(pools.wsrc).astype(np.int32),
           "omask": np.concatenate(pools.omask).astype(np.int32)}
    for kind in KINDS:
        out["src__" + kind], out["refs__" + kind] = X.planes(kind)
    R = CompRef(t, X.STRIDE, X.W, X.H, X.BORDER)
    rows, loaded = [], None
    for ci, (c, cj) in enumerate(zip(cases, built)):
        if loaded != c["kind"]:
            R.set_planes(*X.planes(c["kind"]))
            loaded = c["kind"]
        bw, bh, n = c["bw"], c["bh"], c["bw"] * c["bh"]
        for j in cj:
            jb = j["base"]
            so, mo = int(j["second_off"]), int(j["mask_off"])
            k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
            kw = {}
            if c["search"] == S.OBMC:
                kw = dict(wsrc=out["wsrc"][so:so + n], omask=out["omask"][mo:mo + n],
                          fast=c["fast"])
            else:
                if c["form"] != S.PLAIN:
                    kw["second"] = out["second"][so:so + n]
                if c["form"] == S.MASK:
                    kw.update(mask=out["mask"][mo:mo + bh * c["mask_stride"]],
                              mask_stride=c["mask_stride"], invert=int(j["invert_mask"]))
            ms = R.params(bw, bh, METHODS[c["method"]], COST_NAMES[c["cost"]],
                          int(jb["src_off"]), k, int(jb["ref_off"]) - k * X.PLANE, c["ref_mv"],
                          [int(jb[f]) for f in ("col_min", "col_max", "row_min", "row_max")],
                          c["epb"], c["spb"], c["hp"], **kw)
            res = R.run(c["search"], ms, (int(jb["start_row"]), int(jb["start_col"])),
                        c["step_param"])
            rows.append([ci] + [int(jb[f]) for f in X.JOB_FIELDS] +
                        [so, mo, int(j["invert_mask"])] + res + [0])
        print("  case %3d/%d  search %d form %d %2dx%-2d %-12s %4d rows  %.0fs" % (
            ci, len(cases), c["search"], c["form"], bw, bh, c["kind"], len(rows),
            time.time() - t0), flush=True)
    out["kinds"] = np.array(KINDS)
    out["case_fields"] = np.array(S.CASE_FIELDS)
    out["cases"] = np.array([[c["search"], c["form"], c["bw"], c["bh"], c["method"],
                              c["step_param"], c["cost"], c["epb"], c["spb"], c["hp"],
                              c["mask_stride"], c["fast"], KINDS.index(c["kind"])]
                             for c in cases], np.int64)
    out["row_fields"] = np.array(S.ROW_FIELDS)
    out["rows"] = np.array(rows, np.int64)
    out["geom"] = np.array([X.W, X.H, X.BORDER, X.NREF], np.int32)
    # the restatement must agree before anything is written
    J = {n: i for i, n in enumerate(S.ROW_FIELDS)}
    for g in S.fixture_groups(out):
        want = g.rows[:, J["best_row"]:J["bestsme"] + 1]
        got = S.group_expected(out, g)
        assert np.array_equal(want, got[:, :5]), (g.index, g.prm, want.tolist(), got.tolist())
        out["rows"][out["rows"][:, 0] == g.index, J["steps"]] = got[:, 5]
    path = os.path.join(HERE, "fix_mcomp_comp.npz")
    np.savez_compressed(path, **out)
    print("%d rows in %d cases, %d bytes, %.0f s" % (len(rows), len(cases), os.path.getsize(path),
                                                      time.time() - t0))


if __name__ == "__main__":
    main()
