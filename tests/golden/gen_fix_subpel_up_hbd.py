"""Golden fixture of the high-bit-depth sub-pel searches that rank by the
upsampled prediction, from the reference's own C text executed by cinterp.py
(through gen_fix_mcomp_hbd.py's HbdTU / HbdRef: uint16 planes behind tagged
pointers): av1_find_best_sub_pixel_tree (plain, with second_pred, with
second_pred and a mask under both inv_mask values) and
av1_find_best_obmc_sub_pixel_tree_up with subpel_search_type USE_2_TAPS,
USE_4_TAPS and USE_8_TAPS at 8, 10 and 12 bits, with the aom_highbd_* members
highbd_set_var_fns binds (vf, svf, svaf, msvf, ovf, osvf at the depth).  The
translation unit is aom_dsp/sad.c, sad_av1.c, variance.c, aom_convolve.c,
av1/encoder/mcomp.c and reconinter_enc.c; xd->cur_buf carries
YV12_FLAG_HIGHBITDEPTH, so upsampled_pref_error takes its
aom_highbd_upsampled_pred / _comp_avg_ / _comp_mask_upsampled_pred branch.

  fix_subpel_up_hbd.npz
    planes                   the plane sets' names (cases["plane"] indexes
                             them): those of tests/_hbdsearch_ref.py that
                             fix_mcomp_hbd.npz already stores are read from
                             there; src__<set>, refs__<set> only of this
                             fixture's own (the step edges)
    second, mask, wsrc, omask   the pools the rows' offsets index (uint16,
                             uint8, int32, int32)
    case_fields, cases       one case per call: form, depth, block size, the
                             search type and the search's parameters
    row_fields, rows         one job each (a SUBPEL job record, its pool
                             offsets and invert_mask) and the reference's
                             result

Jobs on the smooth and negclamp planes are fix_mcomp_hbd.npz's own rows and
start from its full-pel results x 8 (every third one moved to a sub-pel
start, since the centre is read at the start itself).

Every row is also run through tests/_hbdup_ref.py here and must agree, and the
rows must contain what _hbdup_ref.check_coverage lists: a disagreement or a
missing item stops the generation.

Usage: python tests/golden/gen_fix_subpel_up_hbd.py [--dry] [--jobs N]
--dry takes the rows from the restatement instead of the reference (seconds)
and writes nothing: it shows whether a set of cases meets the coverage list.
--jobs N runs the cases in N processes (each builds its own translation
unit); the file does not depend on N.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "aom-av1-lavish_amd"))
import _compsubpel_ref as CS  # noqa: E402
import _hbdsearch_ref as H  # noqa: E402
import _hbdup_ref as U  # noqa: E402
import _mvextremes as X  # noqa: E402
from gen_fix_mcomp_comp_hbd import Pools, block, save_npz  # noqa: E402

COST_NAMES = {X.ENTROPY: "MV_COST_ENTROPY", X.L1: "MV_COST_L1_HDRES", X.NONE: "MV_COST_NONE"}
FSTOPS = ["EIGHTH_PEL", "QUARTER_PEL", "HALF_PEL", "FULL_PEL"]
STYPES = ["USE_2_TAPS_ORIG", "USE_2_TAPS", "USE_4_TAPS", "USE_8_TAPS"]
SIZES = [(4, 4), (8, 8), (16, 8), (16, 16)]
MAX_BYTES = 1 << 20
SUB_STARTS = [(2, -3), (5, 4), (-1, 6)]     # 1/8-pel offsets of the sub-pel starts


def make_ref(tables):
    """The executor (imports the interpreter: only a real run needs it)."""
    import cinterp as C
    from gen_fix_mcomp_hbd import HbdRef, HbdTU
    from gen_fixtures import MV_MAX, REF, _get, _set, check_errors

    class HbdUpRef(HbdRef):
        """HbdRef over the translation unit that reaches the upsampled
        predictors, with the compound / OBMC members and buffers."""

        def __init__(self):
            self.tu = tu = HbdTU(REF, ["aom_dsp/sad.c", "aom_dsp/sad_av1.c", "aom_dsp/variance.c",
                                       "aom_dsp/aom_convolve.c", "av1/encoder/mcomp.c",
                                       "av1/encoder/reconinter_enc.c"], C.reference_defines(REF))
            check_errors(tu, ["av1_find_best_sub_pixel_tree",
                              "av1_find_best_obmc_sub_pixel_tree_up",
                              "aom_highbd_upsampled_pred_c", "aom_highbd_comp_avg_upsampled_pred_c",
                              "aom_highbd_comp_mask_upsampled_pred", "aom_highbd_convolve8_horiz_c",
                              "aom_highbd_convolve8_vert_c", "aom_highbd_comp_mask_pred_c"])
            self.E = tu.enums
            self.stride, self.W, self.H, self.BORDER = X.STRIDE, X.W, X.H, X.BORDER
            self.tabs = {}
            for nm in ("lp", "hp"):
                mj = tu.buffer("int", tables["mvjcost_" + nm].tolist())
                mc = [tu.buffer("int", tables["mvcost_" + nm][k].tolist()) for k in range(2)]
                self.tabs[nm] = (mj, [C.Pointer(c.buf, MV_MAX, c.ty) for c in mc])
            self.vtabs = {}
            # xd: mi[0] not intrabc, unscaled reference, a high-bit-depth
            # current buffer (is_cur_buf_hbd)
            self.xd = tu.struct_obj("MACROBLOCKD")
            mbmi = tu.struct_obj("MB_MODE_INFO")
            sf = tu.struct_obj("struct scale_factors")
            _set(sf.buf[0], x_scale_fp=1 << 14, y_scale_fp=1 << 14)
            ybuf = tu.struct_obj("YV12_BUFFER_CONFIG")
            _set(ybuf.buf[0], flags=self.E.get("YV12_FLAG_HIGHBITDEPTH", 8))
            _set(self.xd.buf[0], mi=C.Pointer([mbmi], 0, C.Ptr(tu.ctype("MB_MODE_INFO"))),
                 cur_buf=ybuf)
            _get(self.xd.buf[0], "block_ref_scale_factors")[0] = sf
            self.cm = tu.struct_obj("AV1_COMMON")

        def vtab(self, bw, bh, bd):
            if (bw, bh, bd) not in self.vtabs:
                sz, fn = "%dx%d" % (bw, bh), self.tu.func
                p = "aom_highbd_%d_" % bd
                ob = "aom_highbd_" if bd == 8 else p          # HIGHBD_OBFP_WRAPPER_8
                vtab = self.tu.struct_obj("aom_variance_fn_ptr_t")
                _set(vtab.buf[0], vf=fn(p + "variance" + sz),
                     svf=fn(p + "sub_pixel_variance" + sz),
                     svaf=fn(p + "sub_pixel_avg_variance" + sz),
                     msvf=fn(p + "masked_sub_pixel_variance" + sz),
                     ovf=fn(ob + "obmc_variance" + sz),
                     osvf=fn(ob + "obmc_sub_pixel_variance" + sz))
                self.vtabs[(bw, bh, bd)] = vtab
            return self.vtabs[(bw, bh, bd)]

        def run(self, c, jb, k, inv):
            """[best row, best col, besterr, distortion, sse] of one job."""
            tu, E = self.tu, self.E
            bw, bh = c["bw"], c["bh"]
            _set(self.xd.buf[0], bd=c["bd"])
            ms = tu.struct_obj("SUBPEL_MOTION_SEARCH_PARAMS")
            P = ms.buf[0]
            _set(_get(P, "mv_limits"), col_min=int(jb["col_min"]), col_max=int(jb["col_max"]),
                 row_min=int(jb["row_min"]), row_max=int(jb["row_max"]))
            _set(P, allow_hp=c["allow_hp"], cost_list=None, forced_stop=E[FSTOPS[c["forced_stop"]]],
                 iters_per_step=c["iters"])
            self.cost_params(_get(P, "mv_cost_params"),
                             (int(jb["ref_mv_row"]), int(jb["ref_mv_col"])), COST_NAMES[c["cost"]],
                             c["epb"], 0, c["allow_hp"], False)
            vp = _get(P, "var_params")
            _set(vp, vfp=self.vtab(bw, bh, c["bd"]), w=bw, h=bh,
                 subpel_search_type=E[STYPES[c["search_type"]]])
            sbuf, rbuf = self.bufs(bw, bh, int(jb["src_off"]), k,
                                   int(jb["ref_off"]) - k * X.PLANE)
            buf = lambda t, a: (None if a is None else
                                tu.buffer(t, np.asarray(a).reshape(-1).tolist()))
            sec = buf("uint16_t", inv.get("second"))
            _set(_get(vp, "ms_buffers"), ref=rbuf, src=sbuf,
                 second_pred=None if sec is None else tu.tagged(C.Pointer(sec.buf, 0, sec.ty)),
                 mask=buf("uint8_t", inv.get("mask")), mask_stride=inv.get("mask_stride", 0),
                 inv_mask=inv.get("invert", 0), wsrc=buf("int32_t", inv.get("wsrc")),
                 obmc_mask=buf("int32_t", inv.get("omask")))
            smv = C.new_obj(tu.ctype("MV"))
            _set(smv, row=int(jb["start_row"]), col=int(jb["start_col"]))
            best = tu.struct_obj("MV")
            dist, sse = tu.buffer("int", 1), tu.buffer("unsigned int", 1)
            f = ("av1_find_best_obmc_sub_pixel_tree_up" if c["form"] == U.OBMC
                 else "av1_find_best_sub_pixel_tree")
            err = tu.func(f)(self.xd, self.cm, ms, smv, best, dist, sse, None)
            bm = best.buf[0]
            return [_get(bm, "row"), _get(bm, "col"), err & CS.M32, dist.buf[0],
                    sse.buf[0] & CS.M32]

    return HbdUpRef()


# ------------------------------------------------------------------- cases --
# (allow_hp, forced_stop, iters_per_step, cost type)
COMBOS = [(1, 0, 2, X.ENTROPY), (0, 1, 1, X.L1), (1, 0, 1, X.NONE), (1, 1, 2, X.L1),
          (0, 0, 2, X.ENTROPY), (1, 2, 2, X.NONE), (1, 0, 2, X.L1)]
FORMS = [(U.PLAIN, 0), (U.AVG, 0), (U.MASK, 0), (U.MASK, 1), (U.OBMC, 0)]


def case(form, bd, bw, bh, st, combo, kind, invert=0, epb=37, jobs=None, second="near",
         mask="random", obmc="near", **extra):
    hp, fstop, iters, cost = combo
    c = dict(form=form, bd=bd, bw=bw, bh=bh, search_type=st, allow_hp=hp, forced_stop=fstop,
             iters=iters, cost=cost, epb=epb, kind=kind, invert=invert, jobs=jobs, second=second,
             mask=mask, obmc=obmc)
    c.update(extra)
    return c


def committed_jobs(MH, kind, bd, which=None, size=None):
    """SUBPEL job records of fix_mcomp_hbd.npz's rows on a plane set, starting
    at its full-pel results x 8: the groups of kind at bd (the which-th of
    them below 32x32, or the one of the given size)."""
    groups = [g for g in H.fixture_groups(MH) if g.plane.startswith("%s_bd%d" % (kind, bd))
              and ((g.prm["bw"], g.prm["bh"]) == size if size else g.prm["bw"] < 32)]
    g = groups[(which or 0) % len(groups)]
    return g.prm["bw"], g.prm["bh"], g.sjobs.copy()


def frame_jobs(bw, bh, n, salt, start, ref_mv=(0, 0), ref_only=None):
    """SUBPEL job records of n blocks of the frame with the block's own
    SubpelMvLimits, all starting at `start` (1/8 pel)."""
    fp = X.spread(X.frame(bw, bh, ref_mv), max(n, 3), salt)[:n]
    if ref_only is not None:
        fp["ref_off"] = fp["src_off"] + ref_only * X.PLANE
    return CS.subpel_records(fp, bw, bh, [start] * len(fp))


def all_cases(MH):
    cs = []
    k = 0
    # every depth x type x form (both inv_mask values) on smooth content, from
    # the committed full-pel results; the third job of each from a sub-pel start
    for bd in (8, 10, 12):
        for st in (U.USE_2_TAPS, U.USE_4_TAPS, U.USE_8_TAPS):
            for form, inv in FORMS:
                if form == U.MASK and inv != (st + bd // 2) % 2:
                    continue
                bw, bh, jobs = committed_jobs(MH, "smooth", bd, k)
                dr, dc = SUB_STARTS[k % 3]
                jobs["start_row"][-1] += dr
                jobs["start_col"][-1] += dc
                cs.append(case(form, bd, bw, bh, st, COMBOS[k % 7], "smooth", inv, jobs=jobs,
                               mask=("ramp", "random")[k % 2], salt=k))
                k += 1
    # 4x4 (no committed full-pel rows): starts around the smooth shifts
    for i, (form, inv) in enumerate(FORMS):
        jobs = frame_jobs(4, 4, 3, k, (0, 0))
        jobs["start_row"], jobs["start_col"] = [0, 8, -11], [-8, 0, 12]
        cs.append(case(form, (10, 12, 8)[i % 3], 4, 4, (U.USE_8_TAPS, U.USE_4_TAPS)[i % 2],
                       COMBOS[k % 7], "smooth", inv, jobs=jobs, salt=k))
        k += 1
    # periodic content (every full-pel candidate of the same parity ties) from
    # quarter- and eighth-pel starts, the sizes and types rotating
    for bd in (8, 10, 12):
        for i, (form, inv) in enumerate(FORMS):
            bw, bh = SIZES[(i + bd // 2) % 4]
            jobs = frame_jobs(bw, bh, 3, k, (0, 0), ref_mv=(13, -21))
            jobs["start_row"], jobs["start_col"] = [10, 16, -3], [-22, -17, 8]
            cs.append(case(form, bd, bw, bh, 1 + (i + bd // 2) % 3, COMBOS[(k + 2) % 7],
                           "periodic_2", inv, jobs=jobs, second="random", salt=k))
            k += 1
    # step edges between 0 and the depth's maximum: the passes clip at both
    # ends and the clipped intermediate matters
    for bd in (8, 10, 12):
        for i, (form, inv) in enumerate(FORMS):
            st = (U.USE_8_TAPS, U.USE_4_TAPS, U.USE_8_TAPS, U.USE_8_TAPS, U.USE_4_TAPS)[i]
            bw, bh = SIZES[1 + (i + bd) % 3]
            jobs = frame_jobs(bw, bh, 2, k, (8, 16) if i % 2 else (-16, 8))
            jobs["start_row"][-1] += 3
            jobs["start_col"][-1] -= 2
            cs.append(case(form, bd, bw, bh, st, COMBOS[(k + i) % 7], "edges", inv, jobs=jobs,
                           second="random" if i == 1 else "near", salt=k))
            k += 1
    # the 12-bit variance negative before its clamp: at mv (0, 0) the
    # prediction less the source is negclamp's source less its reference
    # (FULL_PEL: the centre error is the result)
    for form, extra in ((U.AVG, dict(second="over")), (U.OBMC, dict(obmc="exact"))):
        jobs = frame_jobs(16, 16, 1, k, (0, 0), ref_only=0)
        cs.append(case(form, 12, 16, 16, U.USE_8_TAPS, (1, 3, 1, X.NONE), "negclamp", jobs=jobs,
                       salt=k, **extra))
        k += 1
    # candidates outside the limits: the start on the limits' corner
    for form, inv in FORMS:
        bw, bh, jobs = committed_jobs(MH, "smooth", 10, k)
        jobs["col_max"], jobs["row_max"] = jobs["start_col"], jobs["start_row"]
        cs.append(case(form, 10, bw, bh, U.USE_8_TAPS, COMBOS[0], "smooth", inv, jobs=jobs[:2],
                       salt=k))
        k += 1
    # one 32x32 row per form (the invariants no longer fit the registers)
    for i, (form, inv) in enumerate(FORMS):
        if form == U.MASK and inv:
            continue
        bw, bh, jobs = committed_jobs(MH, "smooth", 10, size=(32, 32))
        cs.append(case(form, 10, 32, 32, (U.USE_8_TAPS, U.USE_4_TAPS, U.USE_8_TAPS, 0,
                                          U.USE_2_TAPS)[i], COMBOS[(0, 3, 0, 0, 6)[i]], "smooth",
                       inv, jobs=jobs[:1], salt=k))
        k += 1
    return cs


def build_case(c, pools):
    """The COMP_SUBPEL_JOB records of a case (and its mask_stride)."""
    from lavish_dsp import motion as M
    bw, bh, bd = c["bw"], c["bh"], c["bd"]
    src, refs = U.planes(c["kind"], bd, bw, bh)
    c["mask_stride"] = (bw + (8 if c["mask"] == "ramp" else 3 * (c["salt"] % 2))
                        if c["form"] == U.MASK else 0)
    so, mo = [], []
    for jb in c["jobs"]:
        sblk = block(src, int(jb["src_off"]), bw, bh)
        rblk = block(refs, int(jb["ref_off"]), bw, bh)
        a = b = 0
        if c["form"] == U.OBMC:
            a, b = pools.obmc_block(c["obmc"], bd, sblk, rblk)
        elif c["form"] != U.PLAIN:
            a = pools.second_block(c["second"], bd, sblk, rblk)
            if c["form"] == U.MASK:
                b = pools.mask_block(c["mask"], bw, bh, c["mask_stride"])
        so.append(a)
        mo.append(b)
    return M.comp_subpel_jobs(c["jobs"], so, mo, c["invert"])


_R = None


def run_case(args):
    """case_rows in a worker process, on its own executor."""
    global _R
    if _R is None:
        from gen_fixtures import nmv_cost_tables
        _R = make_ref(nmv_cost_tables())
    return case_rows(_R, *args)


def case_rows(R, c, cj, pools, src, refs):
    """The reference's rows of the jobs cj of a case."""
    R.set_planes(src, refs)
    n, rows = c["bw"] * c["bh"], []
    for j in cj:
        jb = j["base"]
        so, mo = int(j["second_off"]), int(j["mask_off"])
        k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
        inv = {}
        if c["form"] == U.OBMC:
            inv = dict(wsrc=pools["wsrc"][so:so + n], omask=pools["omask"][mo:mo + n])
        elif c["form"] != U.PLAIN:
            inv["second"] = pools["second"][so:so + n]
            if c["form"] == U.MASK:
                inv.update(mask=pools["mask"][mo:mo + c["bh"] * c["mask_stride"]],
                           mask_stride=c["mask_stride"], invert=int(j["invert_mask"]))
        rows.append(R.run(c, jb, k, inv))
    return rows


def main():
    dry = "--dry" in sys.argv[1:]
    nproc = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 1
    t0 = time.time()
    MH = H.load_fixture()
    pools = Pools(seed=7331)
    cases = all_cases(MH)
    built = [build_case(c, pools) for c in cases]
    cat = lambda p, t: np.concatenate(p + [np.zeros(1, np.int64)]).astype(t)
    out = {"second": cat(pools.second, np.uint16), "mask": cat(pools.mask, np.uint8),
           "wsrc": cat(pools.wsrc, np.int32), "omask": cat(pools.omask, np.int32)}
    names, sets = [], {}
    for c in cases:
        key = U.plane_key(c["kind"], c["bd"], c["bw"], c["bh"])
        if key not in names:
            names.append(key)
            sets[key] = U.planes(c["kind"], c["bd"], c["bw"], c["bh"])
            if "src__" + key in MH:     # shared with fix_mcomp_hbd.npz: not stored again
                assert np.array_equal(MH["src__" + key], sets[key][0]) and \
                    np.array_equal(MH["refs__" + key], sets[key][1]), key
            else:
                out["src__" + key], out["refs__" + key] = sets[key]
        c["plane"] = names.index(key)
    if dry:
        results = []
        for c, cj in zip(cases, built):
            src, refs = sets[names[c["plane"]]]
            results.append(U.run_batch(
                c["form"], src.reshape(-1), refs.reshape(-1), X.STRIDE, c["bw"], c["bh"], cj,
                U.S.cost_of(c["cost"], c["epb"], 0, c["allow_hp"]), c["bd"], c["search_type"],
                c["forced_stop"], bool(c["allow_hp"]), c["iters"], out["second"], out["mask"],
                c["mask_stride"], out["wsrc"], out["omask"]).tolist())
    else:
        work = [(c, cj, out, *sets[names[c["plane"]]]) for c, cj in zip(cases, built)]
        if nproc > 1:
            import multiprocessing as mp
            with mp.get_context("fork").Pool(nproc) as pool:
                results = pool.map(run_case, work, chunksize=1)
        else:
            results = []
            for ci, w in enumerate(work):
                results.append(run_case(w))
                print("  case %3d/%d  %.0fs" % (ci, len(work), time.time() - t0), flush=True)
    rows = []
    for ci, (c, cj, res) in enumerate(zip(cases, built, results)):
        for j, r in zip(cj, res):
            rows.append([ci] + [int(j["base"][f]) for f in X.JOB_FIELDS] +
                        [int(j["second_off"]), int(j["mask_off"]), int(j["invert_mask"])] +
                        [int(v) for v in r])
    out["planes"] = np.array(names)
    out["case_fields"] = np.array(U.CASE_FIELDS)
    out["cases"] = np.array([[c["form"], c["bd"], c["bw"], c["bh"], c["search_type"],
                              c["allow_hp"], c["forced_stop"], c["iters"], c["cost"], c["epb"],
                              c["mask_stride"], c["plane"]] for c in cases], np.int64)
    out["row_fields"] = np.array(U.ROW_FIELDS)
    out["rows"] = np.array(rows, np.int64)
    out["geom"] = np.array([X.W, X.H, X.BORDER, X.NREF], np.int32)
    # the restatement must agree, and the coverage hold, before anything is written
    F = dict(out)
    for key in names:
        F["src__" + key], F["refs__" + key] = sets[key]
    for g in U.fixture_groups(F):
        got = U.group_expected(F, g)
        want = g.rows[:, g.J["best_row"]:]
        assert np.array_equal(want, got), (g.index, g.prm, want.tolist(), got.tolist())
    print(U.check_coverage(F))
    if dry:
        print("dry run: %d rows in %d cases, %.0f s; nothing written" % (
            len(rows), len(cases), time.time() - t0))
        return
    path = os.path.join(HERE, "fix_subpel_up_hbd.npz")
    save_npz(path, out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print("%d rows in %d cases, %d bytes, %.0f s" % (len(rows), len(cases), size,
                                                      time.time() - t0))


if __name__ == "__main__":
    main()
