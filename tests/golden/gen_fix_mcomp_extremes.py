"""Golden fixture of the motion searches on tied, saturated and high-lambda
inputs, from the reference's own C text executed by cinterp.py (as
gen_fixtures.py does; the executors are its FullpelRef and SubpelRef).

  fix_mcomp_extremes.npz
    src__<key>, refs__<key>   the planes of tests/_mvextremes.py, by
                              plane_key(kind, bw, bh)
    fp_names, fp_kinds, fp_params [n, len(FP_PARAM_FIELDS)]
                              the full-pel cases (_mvextremes.fixture_fullpel)
    fp_rows [m, len(FP_ROW_FIELDS)]   one av1_full_pixel_search each: the job,
                              the best mv, the returned cost, the cost list
    sp_names, sp_kinds, sp_params, sp_rows   the same for
                              av1_find_best_sub_pixel_tree{,_pruned,
                              _pruned_more} (_mvextremes.fixture_subpel, from
                              the full-pel rows' best mvs and cost lists)

The mv cost tables are the package's (lavish_dsp/data/nmv_cost_default.npz),
checked here against av1_build_nmv_cost_table.

Usage: python tests/golden/gen_fix_mcomp_extremes.py
Generation time: 53 s on one CPU core for 293 full-pel and 211 sub-pel rows
(about 0.1 s a row: the blocks are mostly 4x4, 8x8 and 16x16); the file is
166 KB.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "aom-av1-lavish_amd"))
import _mvextremes as X  # noqa: E402
from gen_fixtures import FullpelRef, SubpelRef, nmv_cost_tables  # noqa: E402

COST_NAMES = {X.ENTROPY: "MV_COST_ENTROPY", X.L1: "MV_COST_L1_HDRES", X.NONE: "MV_COST_NONE"}
STOP_NAMES = ["EIGHTH_PEL", "QUARTER_PEL", "HALF_PEL"]
FP_PARAM_FIELDS = ["bw", "bh", "method", "use_cl", "cost", "skip", "step_param", "error_per_bit",
                   "sad_per_bit", "ref_mv_row", "ref_mv_col", "hp_tables"]
JOB_FIELDS = ["src_off", "ref_off", "start_row", "start_col", "ref_mv_row", "ref_mv_col",
              "col_min", "col_max", "row_min", "row_max"]
FP_ROW_FIELDS = ["case"] + JOB_FIELDS + ["best_row", "best_col", "var", "cl0", "cl1", "cl2",
                                         "cl3", "cl4"]
SP_PARAM_FIELDS = ["bw", "bh", "method", "allow_hp", "forced_stop", "iters_per_step", "cost",
                   "use_cl", "error_per_bit", "ref_mv_row", "ref_mv_col", "search_type"]
SP_ROW_FIELDS = ["case"] + JOB_FIELDS + ["best_row", "best_col", "besterr", "distortion", "sse",
                                         "cl0", "cl1", "cl2", "cl3", "cl4"]


def tables():
    """The default-context tables from the reference; the package data must
    be the same (the tests read that)."""
    from lavish_dsp import motion as M
    t = nmv_cost_tables()
    for hp in (False, True):
        mj, mc = M.default_mv_cost_tables(hp)
        nm = "hp" if hp else "lp"
        assert np.array_equal(mj, t["mvjcost_" + nm]) and np.array_equal(mc, t["mvcost_" + nm])
    return t


def with_planes(runner, out, case, loaded):
    key = X.plane_key(case.kind, case.bw, case.bh)
    if loaded.get("key") != key:
        src, refs = X.planes(case.kind, case.bw, case.bh)
        runner.set_planes(src, refs)
        loaded["key"] = key
    if "src__" + key not in out:
        out["src__" + key], out["refs__" + key] = X.planes(case.kind, case.bw, case.bh)


def job_row(jb):
    return [int(jb[f]) for f in JOB_FIELDS]


def fullpel_rows(t, out, cases, runner=None):
    """fp_rows of `cases` ((index, Case) pairs), executed from the reference."""
    R = runner or FullpelRef([m.upper() for m in X.FP_METHODS], t, X.STRIDE, X.W, X.H, X.BORDER)
    rows, loaded = [], {}
    for ci, c in cases:
        with_planes(R, out, c, loaded)
        p = c.params
        for jb in c.jobs:
            k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
            lims = [int(jb[f]) for f in ("col_min", "col_max", "row_min", "row_max")]
            row, col, var, cl = R.search(
                c.bw, c.bh, p.method.upper(), p.use_cl, COST_NAMES[p.cost], p.skip, p.step_param,
                int(jb["src_off"]), k, int(jb["ref_off"]) - k * X.PLANE, p.ref_mv,
                (int(jb["start_row"]), int(jb["start_col"])), lims, p.epb, p.spb, hp=bool(p.hp))
            rows.append([ci] + job_row(jb) + [row, col, var] + cl)
        print("  %-10s %-13s %3dx%-3d %4d rows" % (c.name, c.kind, c.bw, c.bh, len(rows)),
              flush=True)
    return np.array(rows, np.int64)


def fullpel_results(cases, rows):
    """{case name: (best mvs, cost lists)} of the cases with a cost list, as
    _mvextremes.fixture_subpel takes them."""
    J = {n: i for i, n in enumerate(FP_ROW_FIELDS)}
    res = {}
    for ci, c in enumerate(cases):
        if not c.params.use_cl:
            continue
        r = rows[rows[:, 0] == ci]
        best = np.zeros(len(r), [("best_row", "<i2"), ("best_col", "<i2")])
        best["best_row"], best["best_col"] = r[:, J["best_row"]], r[:, J["best_col"]]
        res[c.name] = (best, r[:, J["cl0"]:J["cl4"] + 1].astype(np.int32))
    return res


def subpel_rows(t, out, cases, runner=None):
    R = runner or SubpelRef(t, X.STRIDE, X.W, X.H, X.BORDER)
    rows, loaded = [], {}
    for ci, c in cases:
        with_planes(R, out, c, loaded)
        p = c.params
        for i, jb in enumerate(c.jobs):
            k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
            cl = [int(v) for v in c.facts[i]] if p.use_cl else None
            slims = [int(jb[f]) for f in ("col_min", "col_max", "row_min", "row_max")]
            _, row, col, err, dist, sse = R.search(
                c.bw, c.bh, p.method.upper(), p.hp, STOP_NAMES[p.forced_stop], p.iters,
                COST_NAMES[p.cost], cl, p.epb, int(jb["src_off"]), k,
                int(jb["ref_off"]) - k * X.PLANE, p.ref_mv,
                (int(jb["start_row"]), int(jb["start_col"])), slims=slims)
            rows.append([ci] + job_row(jb) + [row, col, err, dist, sse] +
                        (cl if cl is not None else [X.INT_MAX] * 5))
        print("  %-14s %-13s %3dx%-3d %4d rows" % (c.name, c.kind, c.bw, c.bh, len(rows)),
              flush=True)
    return np.array(rows, np.int64)


def fp_params(cases):
    return np.array([[c.bw, c.bh, X.FP_METHODS.index(c.params.method), c.params.use_cl,
                      c.params.cost, c.params.skip, c.params.step_param, c.params.epb,
                      c.params.spb, c.params.ref_mv[0], c.params.ref_mv[1], c.params.hp]
                     for c in cases],
                    np.int64)


def sp_params(cases):
    return np.array([[c.bw, c.bh, X.SUBPEL_METHODS.index(c.params.method), c.params.hp,
                      c.params.forced_stop, c.params.iters, c.params.cost, c.params.use_cl,
                      c.params.epb, c.params.ref_mv[0], c.params.ref_mv[1],
                      c.params.search_type] for c in cases], np.int64)


def main():
    t0 = time.time()
    t = tables()
    out = {}
    fcases = X.fixture_fullpel()
    frows = fullpel_rows(t, out, list(enumerate(fcases)))
    out["fp_names"] = np.array([c.name for c in fcases])
    out["fp_kinds"] = np.array([c.kind for c in fcases])
    out["fp_params"], out["fp_param_fields"] = fp_params(fcases), np.array(FP_PARAM_FIELDS)
    out["fp_rows"], out["fp_row_fields"] = frows, np.array(FP_ROW_FIELDS)
    scases = X.fixture_subpel(fullpel_results(fcases, frows))
    out["sp_names"] = np.array([c.name for c in scases])
    out["sp_kinds"] = np.array([c.kind for c in scases])
    out["sp_params"], out["sp_param_fields"] = sp_params(scases), np.array(SP_PARAM_FIELDS)
    out["sp_rows"] = subpel_rows(t, out, list(enumerate(scases)))
    out["sp_row_fields"] = np.array(SP_ROW_FIELDS)
    out["geom"] = np.array([X.W, X.H, X.BORDER, X.NREF], np.int32)
    path = os.path.join(HERE, "fix_mcomp_extremes.npz")
    np.savez_compressed(path, **out)
    print("%d full-pel and %d sub-pel rows, %d bytes, %.0f s" % (
        len(out["fp_rows"]), len(out["sp_rows"]), os.path.getsize(path), time.time() - t0))


if __name__ == "__main__":
    main()
