"""Golden fixture of the high-bit-depth compound, masked and OBMC searches,
from the reference's own C text executed by cinterp.py (through
gen_fix_mcomp_hbd.py's HbdTU / HbdRef: uint16 planes behind tagged pointers):
av1_full_pixel_search with second_pred, av1_refining_search_8p_c,
av1_obmc_full_pixel_search, av1_find_best_sub_pixel_tree / _pruned /
_pruned_more with second_pred and av1_find_best_obmc_sub_pixel_tree_up, with
the members highbd_set_var_fns binds.  The _bits8 / _bits10 / _bits12 SAD
wrappers are the reference's own macro text: MAKE_BFP_SAD_WRAPPER,
MAKE_BFP_SAD4D_WRAPPER, MAKE_BFP_SADAVG_WRAPPER,
MAKE_MBFP_COMPOUND_SAD_WRAPPER and MAKE_OBFP_SAD_WRAPPER and their invocation
lines are read from av1/encoder/encoder_utils.h by name and expanded by the
interpreter's preprocessor.  xd->cur_buf carries YV12_FLAG_HIGHBITDEPTH, so
setup_center_error takes its aom_highbd_comp_*_pred branch.

  fix_mcomp_comp_hbd.npz
    src__<set>, refs__<set>  the plane sets of tests/_hbdsearch_ref.py
    second                   uint16 pool the rows' second_off index (compact)
    mask                     uint8 pool (blocks at the case's mask_stride)
    wsrc, omask              int32 pools of the OBMC rows (compact blocks)
    case_fields, cases       one case per full-pel call and the sub-pel
                             search that continues it (has_sp 0: none)
    row_fields, rows         one job each: the reference's full-pel record
                             (`steps` is tests/_hbdcomp_ref.py's count), the
                             SubpelMvLimits, the reference's sub-pel result
                             from best x 8 (sp0_*) and, for the compound
                             full-pel search, from second_best x 8 (sp1_*:
                             the INT_MAX / -32768 record where try_second
                             does not search)

Every row is also run through tests/_hbdcomp_ref.py here and must agree, and
the rows must contain what _hbdcomp_ref.check_coverage lists: a disagreement
or a missing item stops the generation.

Usage: python tests/golden/gen_fix_mcomp_comp_hbd.py [--dry]
--dry takes the rows from the restatement instead of the reference (seconds)
and writes nothing: it shows whether a set of cases meets the coverage list.
"""
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "aom-av1-lavish_amd"))
import _compsubpel_ref as CS  # noqa: E402
import _hbdcomp_ref as HC  # noqa: E402
import _hbdsearch_ref as H  # noqa: E402
import _mvextremes as X  # noqa: E402

S = HC.S
METHODS = ["DIAMOND", "NSTEP", "NSTEP_8PT"]           # index = SEARCH_METHODS value
COST_NAMES = {X.ENTROPY: "MV_COST_ENTROPY", X.L1: "MV_COST_L1_HDRES", X.NONE: "MV_COST_NONE"}
SP_FN = {CS.TREE: "av1_find_best_sub_pixel_tree",
         CS.PRUNED: "av1_find_best_sub_pixel_tree_pruned",
         CS.PRUNED_MORE: "av1_find_best_sub_pixel_tree_pruned_more"}
FSTOPS = ["EIGHTH_PEL", "QUARTER_PEL", "HALF_PEL", "FULL_PEL"]
SIZES = [(4, 4), (8, 8), (16, 8), (16, 16)]
WRAPPERS = {"MAKE_BFP_SAD_WRAPPER": "aom_highbd_sad%s", "MAKE_BFP_SAD4D_WRAPPER":
            "aom_highbd_sad%sx4d", "MAKE_BFP_SADAVG_WRAPPER": "aom_highbd_sad%s_avg",
            "MAKE_MBFP_COMPOUND_SAD_WRAPPER": "aom_highbd_masked_sad%s",
            "MAKE_OBFP_SAD_WRAPPER": "aom_highbd_obmc_sad%s"}
MAX_BYTES = 1 << 20


def wrapper_text(ref_root, sizes):
    """The wrapper macros' definitions and, for `sizes`, their invocations,
    as encoder_utils.h writes them."""
    with open(os.path.join(ref_root, "av1/encoder/encoder_utils.h")) as fh:
        lines = fh.read().split("\n")
    out = []
    for name in WRAPPERS:
        a = next(i for i, l in enumerate(lines) if l.startswith("#define %s(" % name))
        b = a
        while lines[b].rstrip().endswith("\\"):
            b += 1
        out += lines[a:b + 1]
    want = {pat % ("%dx%d" % sz) for pat in WRAPPERS.values() for sz in sizes}
    want |= {"aom_highbd_sad%dx%dx3d" % sz for sz in sizes}
    pat = re.compile(r"^(%s)\((\w+)\)$" % "|".join(WRAPPERS))
    found = set()
    for l in lines:
        m = pat.match(l.strip())
        if m and m.group(2) in want and m.group(2) not in found:
            found.add(m.group(2))
            out.append(l)
    return "\n".join(out) + "\n", found


def make_ref(tables, sizes):
    """The executor (imports the interpreter: only a real run needs it)."""
    import cinterp as C
    from gen_fix_mcomp_hbd import HbdRef, HbdTU
    from gen_fixtures import MS_INIT, MV_MAX, REF, _get, _set, check_errors

    class HbdCompRef(HbdRef):
        """HbdRef with aom_dsp/sad_av1.c in the translation unit and the
        compound / OBMC members and buffers."""

        def __init__(self):
            self.tu = tu = HbdTU(REF, ["aom_dsp/sad.c", "aom_dsp/variance.c", "aom_dsp/sad_av1.c",
                                       "av1/encoder/mcomp.c"], C.reference_defines(REF))
            check_errors(tu, ["av1_full_pixel_search", "av1_set_mv_search_range",
                              "av1_refining_search_8p_c", "av1_obmc_full_pixel_search",
                              "av1_find_best_obmc_sub_pixel_tree_up", "aom_highbd_comp_avg_pred_c",
                              "aom_highbd_comp_mask_pred_c"] + sorted(SP_FN.values()) +
                         sorted({MS_INIT[m][0] for m in METHODS}))
            self.E = tu.enums
            self.stride, self.W, self.H, self.BORDER = X.STRIDE, X.W, X.H, X.BORDER
            self.cfgs = {}
            for m in METHODS:
                cfg = tu.struct_obj("search_site_config")
                fname, level = MS_INIT[m]
                tu.func(fname)(cfg, X.STRIDE, level)
                self.cfgs[m] = cfg
            self.tabs = {}
            for nm in ("lp", "hp"):
                mj = tu.buffer("int", tables["mvjcost_" + nm].tolist())
                mc = [tu.buffer("int", tables["mvcost_" + nm][k].tolist()) for k in range(2)]
                self.tabs[nm] = (mj, [C.Pointer(c.buf, MV_MAX, c.ty) for c in mc])
            self.vtabs = {}
            text, self.wrapped = wrapper_text(REF, sizes)
            tu.add_source(text, "<encoder_utils.h wrappers>")
            check_errors(tu, ["%s_bits%d" % (n, bd) for n in sorted(self.wrapped)
                              for bd in (8, 10, 12)])
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
                wr = lambda name: fn("%s_bits%d" % (name, bd))
                vtab = self.tu.struct_obj("aom_variance_fn_ptr_t")
                _set(vtab.buf[0], sdf=wr("aom_highbd_sad" + sz),
                     sdx4df=wr("aom_highbd_sad%sx4d" % sz),
                     sdx3df=(wr("aom_highbd_sad%sx3d" % sz)
                             if "aom_highbd_sad%sx3d" % sz in self.wrapped else None),
                     sdaf=wr("aom_highbd_sad%s_avg" % sz), msdf=wr("aom_highbd_masked_sad" + sz),
                     osdf=wr("aom_highbd_obmc_sad" + sz), vf=fn(p + "variance" + sz),
                     svf=fn(p + "sub_pixel_variance" + sz),
                     svaf=fn(p + "sub_pixel_avg_variance" + sz),
                     msvf=fn(p + "masked_sub_pixel_variance" + sz),
                     ovf=fn(ob + "obmc_variance" + sz),
                     osvf=fn(ob + "obmc_sub_pixel_variance" + sz))
                self.vtabs[(bw, bh, bd)] = vtab
            return self.vtabs[(bw, bh, bd)]

        def ms_buffers(self, mb, bw, bh, src_off, k, ref_off, inv):
            tu = self.tu
            sbuf, rbuf = self.bufs(bw, bh, src_off, k, ref_off)
            buf = lambda t, a: None if a is None else tu.buffer(t, np.asarray(a).reshape(-1).tolist())
            sec = buf("uint16_t", inv.get("second"))
            _set(mb, ref=rbuf, src=sbuf,
                 second_pred=None if sec is None else tu.tagged(C.Pointer(sec.buf, 0, sec.ty)),
                 mask=buf("uint8_t", inv.get("mask")), mask_stride=inv.get("mask_stride", 0),
                 inv_mask=inv.get("invert", 0), wsrc=buf("int32_t", inv.get("wsrc")),
                 obmc_mask=buf("int32_t", inv.get("omask")))

        def full(self, c, jb, k, inv):
            """[best row, best col, second row, second col, return value]."""
            tu, E = self.tu, self.E
            bw, bh, mname = c["bw"], c["bh"], METHODS[c["method"]]
            vtab = self.vtab(bw, bh, c["bd"])
            ms = tu.struct_obj("FULLPEL_MOTION_SEARCH_PARAMS")
            P = ms.buf[0]
            _set(P, bsize=E["BLOCK_%dX%d" % (bw, bh)], vfp=vtab, search_method=E[mname],
                 search_sites=self.cfgs[mname], run_mesh_search=0, prune_mesh_search=0,
                 mesh_search_mv_diff_threshold=4, force_mesh_thresh=0x7FFFFFFF,
                 fine_search_interval=0, is_intra_mode=0, fast_obmc_search=c["fast"])
            self.ms_buffers(_get(P, "ms_buffers"), bw, bh, int(jb["src_off"]), k,
                            int(jb["ref_off"]) - k * X.PLANE, inv)
            L = tu.struct_obj("FullMvLimits").buf[0]
            _set(L, col_min=int(jb["col_min"]), col_max=int(jb["col_max"]),
                 row_min=int(jb["row_min"]), row_max=int(jb["row_max"]))
            _set(P, mv_limits=L)
            self.cost_params(_get(P, "mv_cost_params"), c["ref_mv"], COST_NAMES[c["cost"]],
                             c["epb"], c["spb"], c["hp"], True)
            vt = vtab.buf[0]
            _set(P, sdf=_get(vt, "sdf"), sdx4df=_get(vt, "sdx4df"), sdx3df=_get(vt, "sdx3df"))
            smv = C.new_obj(tu.ctype("FULLPEL_MV"))
            _set(smv, row=int(jb["start_row"]), col=int(jb["start_col"]))
            best = tu.struct_obj("FULLPEL_MV")
            if c["search"] == HC.COMP:
                from gen_fix_mcomp_comp import mv_of
                sec = tu.struct_obj("FULLPEL_MV")
                v = tu.func("av1_full_pixel_search")(smv, ms, c["step_param"], None, best, sec)
                second = mv_of(sec.buf[0])
            elif c["search"] == HC.REFINE8:
                v = tu.func("av1_refining_search_8p_c")(ms, smv, best)
                second = (_get(best.buf[0], "row"), _get(best.buf[0], "col"))   # facade.c:621
            else:
                v = tu.func("av1_obmc_full_pixel_search")(smv, ms, c["step_param"], best)
                second = (HC.INVALID, HC.INVALID)
            bm = best.buf[0]
            return [_get(bm, "row"), _get(bm, "col"), second[0], second[1], v]

        def sub(self, c, jb, k, inv, slims, start):
            """[best row, best col, besterr, distortion, sse]."""
            tu, E = self.tu, self.E
            bw, bh = c["bw"], c["bh"]
            spm, fstop, hp, iters = c["sp"]
            _set(self.xd.buf[0], bd=c["bd"])
            ms = tu.struct_obj("SUBPEL_MOTION_SEARCH_PARAMS")
            P = ms.buf[0]
            _set(_get(P, "mv_limits"), col_min=slims[0], col_max=slims[1], row_min=slims[2],
                 row_max=slims[3])
            _set(P, allow_hp=hp, cost_list=None, forced_stop=E[FSTOPS[fstop]],
                 iters_per_step=iters)
            self.cost_params(_get(P, "mv_cost_params"), c["ref_mv"], COST_NAMES[c["cost"]],
                             c["epb"], 0, hp, False)
            vp = _get(P, "var_params")
            _set(vp, vfp=self.vtab(bw, bh, c["bd"]), w=bw, h=bh,
                 subpel_search_type=E["USE_2_TAPS_ORIG"])
            self.ms_buffers(_get(vp, "ms_buffers"), bw, bh, int(jb["src_off"]), k,
                            int(jb["ref_off"]) - k * X.PLANE, inv)
            smv = C.new_obj(tu.ctype("MV"))
            _set(smv, row=start[0], col=start[1])
            best = tu.struct_obj("MV")
            dist, sse = tu.buffer("int", 1), tu.buffer("unsigned int", 1)
            f = ("av1_find_best_obmc_sub_pixel_tree_up" if c["search"] == HC.OBMC
                 else SP_FN[spm])
            err = tu.func(f)(self.xd, self.cm, ms, smv, best, dist, sse, None)
            bm = best.buf[0]
            return [_get(bm, "row"), _get(bm, "col"), err & CS.M32, dist.buf[0],
                    sse.buf[0] & CS.M32]

    return HbdCompRef()


# ------------------------------------------------------------------- pools --
class Pools:
    def __init__(self, seed=6151):
        self.rng = np.random.default_rng(seed)
        self.second, self.mask, self.wsrc, self.omask = [], [], [], []

    def _add(self, pool, a):
        off = sum(len(x) for x in pool)
        pool.append(np.asarray(a).reshape(-1))
        return off

    def second_block(self, what, bd, src, ref):
        top = (1 << bd) - 1
        if what == "max":
            a = np.full(src.size, top)
        elif what == "over":      # the average with the reference block is 2 * src - ref
            a = 4 * src - 3 * ref
        elif what == "over_full": # (taken whole, under a zero mask)
            a = 2 * src - ref
        elif what == "random":
            a = self.rng.integers(0, top + 1, src.size)
        else:                     # "near": the source, off by a few low bits
            a = np.clip(src + self.rng.integers(-3, 4, src.shape), 0, top)
        # (an odd lead-in: the blocks are addressed at any element offset)
        self._add(self.second, self.rng.integers(0, top + 1, int(self.rng.integers(0, 4))))
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

    def obmc_block(self, what, bd, src, ref):
        n, top = src.size, (1 << bd) - 1
        src, ref = src.reshape(-1), ref.reshape(-1)
        if what == "full":       # pre at its maximum against wsrc 0: the largest term
            m, w = np.full(n, 4096), np.zeros(n, np.int64)
        elif what == "exact":    # wsrc - pre * mask = (src - ref) * 4096 at mv (0, 0)
            m = self.rng.integers(1024, 4097, n)
            w = (src - ref) * 4096 + ref * m
        else:                    # src * 4096 less the neighbour's weighted prediction
            m = self.rng.integers(1024, 4097, n)
            nb = np.clip(src + self.rng.integers(-3, 4, n), 0, top)
            w = src * 4096 - nb * (4096 - m)
        return self._add(self.wsrc, w), self._add(self.omask, m)


# ------------------------------------------------------------------- cases --
# (method, forced_stop, allow_hp, iters_per_step) of the sub-pel search
SP_COMBOS = [(CS.TREE, 0, 1, 2), (CS.PRUNED, 0, 1, 2), (CS.PRUNED_MORE, 0, 1, 1),
             (CS.TREE, 1, 0, 1), (CS.PRUNED_MORE, 2, 0, 2), (CS.PRUNED, 1, 0, 1)]
FORMS = [(HC.COMP, HC.AVG, 0), (HC.COMP, HC.MASK, 0), (HC.COMP, HC.MASK, 1),
         (HC.REFINE8, HC.PLAIN, 0), (HC.REFINE8, HC.AVG, 0), (HC.REFINE8, HC.MASK, 0),
         (HC.REFINE8, HC.MASK, 1), (HC.OBMC, HC.PLAIN, 0), (HC.OBMC, HC.PLAIN, 1)]


def case(search, form, bd, bw, bh, kind, method=0, step_param=5, cost=X.ENTROPY,
         epb=X.LOW_LAMBDA[0], spb=X.LOW_LAMBDA[1], hp=0, fast=0, invert=0, sp=SP_COMBOS[0],
         ref_mv=(0, 0), start=(0, 0), njobs=2, salt=0, limits=None, second="near", mask="random",
         obmc="near", has_sp=1, ref_only=None):
    if search == HC.OBMC:
        sp = (CS.TREE,) + tuple(sp[1:])
        has_sp = has_sp and cost != X.L1      # (estimate_obmc_mvcost asserts on the L1 types)
    if search == HC.REFINE8 and form == HC.PLAIN:
        has_sp = 0
    return dict(search=search, form=form, bd=bd, bw=bw, bh=bh, kind=kind, method=method,
                step_param=step_param, cost=cost, epb=epb, spb=spb, hp=sp[2] if has_sp else hp,
                fast=fast, invert=invert, sp=tuple(sp), ref_mv=ref_mv, start=start, njobs=njobs,
                salt=salt, limits=limits, second=second, mask=mask, obmc=obmc,
                has_sp=int(bool(has_sp)), ref_only=ref_only)


def all_cases():
    cs = []
    k = 0
    costs = (X.ENTROPY, X.L1, X.NONE)
    masks = ("ramp", "random", "full", "zero")
    # every depth x search x form on smooth content (the sub-pel searches
    # move), the methods, cost types and sub-pel combinations rotating
    for bi, bd in enumerate((8, 10, 12)):
        for fi, (search, form, x) in enumerate(FORMS):
            method = (fi + bi) % 3
            cost = costs[(fi + bi + (search == HC.OBMC)) % 3]
            cs.append(case(search, form, bd, *SIZES[1 + k % 3], "smooth", method, 6 + k % 2, cost,
                           fast=x if search == HC.OBMC else 0,
                           invert=x if search != HC.OBMC else 0, sp=SP_COMBOS[k % 6],
                           start=(1 - k % 3, k % 4 - 1), njobs=3, salt=k, mask=masks[k % 2]))
            k += 1
    # each depth under each method and each cost type (the forms rotating)
    for bi, bd in enumerate((8, 10, 12)):
        for method in range(3):
            search, form, x = FORMS[(k * 2) % 9 if (k * 2) % 9 not in (3, 4, 5, 6) else 0]
            ref_mv = [(0, 0), (13, -21), (-40, 33)][k % 3]
            at = ((ref_mv[0] + 4) >> 3, (ref_mv[1] + 4) >> 3)
            cs.append(case(search, form, bd, *SIZES[k % 4], ("periodic_2", "ramp_x")[k % 2],
                           method, (5, 0)[k % 4 == 0], costs[(bi + method) % 3],
                           fast=0, invert=x if search != HC.OBMC else 0, sp=SP_COMBOS[k % 6],
                           ref_mv=ref_mv, start=(at[0] + 2 - k % 5, at[1] - 1 + k % 3), salt=k,
                           second="random", mask=masks[k % 4], obmc="near"))
            k += 1
    # low-bit noise on a flat plane: the shift per block and per row differ
    for bd in (10, 12):
        for search, form, x in ((HC.COMP, HC.AVG, 0), (HC.COMP, HC.MASK, 0), (HC.REFINE8, HC.AVG, 0),
                                (HC.REFINE8, HC.MASK, 1), (HC.OBMC, HC.PLAIN, 0),
                                (HC.OBMC, HC.PLAIN, 1)):
            cs.append(case(search, form, bd, *SIZES[1 + k % 3], "flat_128_128", k % 3, 7, X.NONE,
                           fast=x if search == HC.OBMC else 0,
                           invert=x if search != HC.OBMC else 0, sp=SP_COMBOS[k % 6],
                           start=(2, -3), njobs=4, salt=k, mask=masks[k % 2]))
            k += 1
    # the variance negative before its clamp: at mv (0, 0) the prediction less
    # the source is negclamp's source less its reference (d, and d + 1 in the
    # first k pixels)
    for bd, (bw, bh) in ((10, (8, 8)), (12, (16, 16))):
        for search, form in ((HC.COMP, HC.AVG), (HC.COMP, HC.MASK), (HC.OBMC, HC.PLAIN)):
            cs.append(case(search, form, bd, bw, bh, "negclamp", k % 3, 9, X.NONE, njobs=1, salt=k,
                           second="over" if form == HC.AVG else "over_full", mask="zero",
                           obmc="exact", sp=SP_COMBOS[3], ref_only=0))
            k += 1
    # 12-bit maximum against zero
    cs.append(case(HC.COMP, HC.AVG, 12, 16, 16, "flat_0_255", 0, 6, njobs=1, second="max"))
    cs.append(case(HC.COMP, HC.MASK, 12, 16, 16, "flat_0_255", 1, 6, X.L1, njobs=1, second="max",
                   mask="zero", invert=1))
    cs.append(case(HC.REFINE8, HC.MASK, 12, 8, 8, "flat_0_255", njobs=1, second="max",
                   mask="full"))
    cs.append(case(HC.OBMC, HC.PLAIN, 12, 16, 16, "flat_0_255", 2, 6, X.NONE, njobs=1,
                   obmc="full"))
    # windows narrowed to a row, a column; a start outside the window
    for lim in ("row", "col", "clamped"):
        for search, form, x in (FORMS[k % 3], FORMS[7 + k % 2]):
            cs.append(case(search, form, (10, 12, 8)[k % 3], *SIZES[k % 4], "periodic_2", k % 3, 5,
                           costs[k % 3 if search != HC.OBMC else 0], fast=x if search == HC.OBMC
                           else 0, invert=x if search != HC.OBMC else 0, ref_mv=(13, -21),
                           start=(2, -3), salt=k, limits=lim, sp=SP_COMBOS[k % 6],
                           second="random"))
            k += 1
    # sub-pel candidates outside the limits: the full-pel result on a corner
    # of the SubpelMvLimits
    for search, form in ((HC.COMP, HC.AVG), (HC.COMP, HC.MASK), (HC.OBMC, HC.PLAIN)):
        cs.append(case(search, form, 10, 8, 8, "smooth", 0, 7, X.NONE, limits="edge",
                       sp=SP_COMBOS[0], salt=k))
        k += 1
    # OBMC from a nonzero start on the full-pel match: given the start's own
    # error the search would stay; mv (0, 0)'s moves it
    for bd in (8, 10, 12):
        cs.append(case(HC.OBMC, HC.PLAIN, bd, *SIZES[1 + k % 3], "smooth", 1, 8, X.ENTROPY,
                       sp=SP_COMBOS[0], start=(-1, 2), njobs=2, salt=k, ref_only=1))
        k += 1
    # a lambda at which rate * error_per_bit passes 2^31
    epb, ref_mv, hp = X.HIGH_LAMBDA[1]
    cs.append(case(HC.COMP, HC.AVG, 10, 8, 8, "periodic_2", 0, 6, X.ENTROPY, epb,
                   X.SAD_PER_BIT_TOP, hp, ref_mv=ref_mv, has_sp=0, second="random"))
    cs.append(case(HC.OBMC, HC.PLAIN, 12, 8, 8, "periodic_2", 1, 6, X.ENTROPY, epb,
                   X.SAD_PER_BIT_TOP, hp, ref_mv=ref_mv, has_sp=0))
    # one 32x32 row per form
    for search, form, x in FORMS:
        if search == HC.REFINE8 and form != HC.AVG:
            continue
        cs.append(case(search, form, 10, 32, 32, "smooth", 1, 8, costs[k % 3 if search != HC.OBMC
                                                                      else 0],
                       fast=x if search == HC.OBMC else 0, invert=x if search != HC.OBMC else 0,
                       njobs=1, start=(1, 0), sp=SP_COMBOS[k % 3], salt=k))
        k += 1
    return cs


def case_jobs(c):
    jobs = X.frame(c["bw"], c["bh"], c["ref_mv"], c["start"])
    jobs = X.spread(jobs, max(c["njobs"], 3), c["salt"])[:c["njobs"]]
    if c["ref_only"] is not None:       # every job on that reference
        jobs["ref_off"] = jobs["src_off"] + c["ref_only"] * X.PLANE
    lim = c["limits"]
    if lim in ("row", "col"):
        jobs = X.narrowed(jobs, lim, (3, -2))
    elif lim == "clamped":          # the start lies outside the window on both axes
        jobs["row_max"] = np.minimum(jobs["row_max"], jobs["start_row"] - 2)
        jobs["col_min"] = np.maximum(jobs["col_min"], jobs["start_col"] + 3)
    return jobs


def block(plane, off, bw, bh):
    idx = np.arange(bh)[:, None] * X.STRIDE + np.arange(bw)[None, :]
    return plane.reshape(-1)[off + idx].astype(np.int64)


def build_case(c, pools):
    """The COMP_JOB records of a case (and its mask_stride)."""
    from lavish_dsp import motion as M
    bw, bh, bd = c["bw"], c["bh"], c["bd"]
    src, refs = H.planes(c["kind"], bd, bw, bh)
    jobs = case_jobs(c)
    c["mask_stride"] = (bw + (8 if c["mask"] == "ramp" else 3 * (c["salt"] % 2))
                        if c["form"] == HC.MASK else 0)
    so, mo = [], []
    for jb in jobs:
        sblk = block(src, int(jb["src_off"]), bw, bh)
        rblk = block(refs, int(jb["ref_off"]), bw, bh)
        a = b = 0
        if c["search"] == HC.OBMC:
            a, b = pools.obmc_block(c["obmc"], bd, sblk, rblk)
        elif c["form"] != HC.PLAIN:
            a = pools.second_block(c["second"], bd, sblk, rblk)
            if c["form"] == HC.MASK:
                b = pools.mask_block(c["mask"], bw, bh, c["mask_stride"])
        so.append(a)
        mo.append(b)
    return M.comp_jobs(jobs, so, mo, c["invert"])


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give
    the same bytes on every run."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o600 << 16
            with z.open(zi, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(a), allow_pickle=False)


def main():
    from lavish_dsp import motion as M
    dry = "--dry" in sys.argv[1:]
    t0 = time.time()
    pools = Pools()
    cases = all_cases()
    built = [build_case(c, pools) for c in cases]
    out = {"second": np.concatenate(pools.second).astype(np.uint16),
           "mask": np.concatenate(pools.mask).astype(np.uint8),
           "wsrc": np.concatenate(pools.wsrc).astype(np.int32),
           "omask": np.concatenate(pools.omask).astype(np.int32)}
    names = []
    for c in cases:
        key = H.plane_key(c["kind"], c["bd"], c["bw"], c["bh"])
        if key not in names:
            names.append(key)
            out["src__" + key], out["refs__" + key] = H.planes(c["kind"], c["bd"], c["bw"], c["bh"])
        c["plane"] = names.index(key)
    R = None
    if not dry:
        from gen_fixtures import nmv_cost_tables
        R = make_ref(nmv_cost_tables(), sorted({(c["bw"], c["bh"]) for c in cases}))
    rows, loaded = [], None
    for ci, (c, cj) in enumerate(zip(cases, built)):
        bw, bh, bd, n = c["bw"], c["bh"], c["bd"], c["bw"] * c["bh"]
        key = names[c["plane"]]
        src, ref = out["src__" + key].reshape(-1), out["refs__" + key].reshape(-1)
        if R is not None and loaded != key:
            R.set_planes(out["src__" + key], out["refs__" + key])
            loaded = key
        cost = S.cost_of(c["cost"], c["epb"], c["spb"], c["hp"])
        spm, fstop, sphp, iters = c["sp"]
        scost = S.cost_of(c["cost"], c["epb"], 0, sphp)
        for j in cj:
            jb = j["base"]
            so, mo = int(j["second_off"]), int(j["mask_off"])
            k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
            inv = {}
            if c["search"] == HC.OBMC:
                inv = dict(wsrc=out["wsrc"][so:so + n], omask=out["omask"][mo:mo + n])
            else:
                if c["form"] != HC.PLAIN:
                    inv["second"] = out["second"][so:so + n]
                if c["form"] == HC.MASK:
                    inv.update(mask=out["mask"][mo:mo + bh * c["mask_stride"]],
                               mask_stride=c["mask_stride"], invert=int(j["invert_mask"]))
            pool_kw = dict(second=out["second"], mask=out["mask"], mask_stride=c["mask_stride"],
                           wsrc=out["wsrc"], omask=out["omask"])
            if R is not None:
                fp = R.full(c, jb, k, inv)
            else:
                e = HC.full_env(c["search"], c["form"], src, ref, X.STRIDE, bw, bh, j, cost, bd,
                                **pool_kw)
                r = HC.full_search(e, c["search"], c["method"], c["step_param"], c["fast"])
                fp = [r[f] for f in HC.FULL_FIELDS[:5]]
            slims = list(CS.block_limits(int(jb["src_off"]), bw, bh, c["ref_mv"]))
            if c["limits"] == "edge":   # the result sits on the limits' corner
                slims[1], slims[3] = 8 * fp[1], 8 * fp[0]
            sps = []
            for which in (0, 1):
                st = (8 * fp[2 * which], 8 * fp[2 * which + 1])
                ok = c["has_sp"] and (which == 0 or (
                    c["search"] == HC.COMP and HC.INVALID not in fp[2:4] and
                    slims[0] <= st[1] <= slims[1] and slims[2] <= st[0] <= slims[3]))
                if not ok:
                    sps += [CS.NO_SEARCH[f] for f in HC.SUB_FIELDS]
                elif R is not None:
                    sps += R.sub(c, jb, k, inv, slims, st)
                else:
                    sj = np.zeros(1, M.SUBPEL_JOB_DTYPE)
                    for f in ("src_off", "ref_off", "ref_mv_row", "ref_mv_col"):
                        sj[f] = jb[f]
                    sj["col_min"], sj["col_max"], sj["row_min"], sj["row_max"] = slims
                    csj = M.comp_subpel_jobs(sj, so, mo, int(j["invert_mask"]))[0]
                    se = HC.sub_env(HC.P.OBMC if c["search"] == HC.OBMC else HC.SP_FORM[c["form"]],
                                    src, ref, X.STRIDE, bw, bh, csj, scost, bd, **pool_kw)
                    r = CS.search(se, spm, CS.USE_2_TAPS_ORIG, fstop, bool(sphp), iters, st)
                    sps += [r[f] for f in HC.SUB_FIELDS]
            rows.append([ci] + [int(jb[f]) for f in X.JOB_FIELDS] +
                        [so, mo, int(j["invert_mask"])] + fp + [0] + slims + sps)
        print("  case %3d/%d  bd %2d search %d form %d %2dx%-2d %-12s %4d rows  %.0fs" % (
            ci, len(cases), bd, c["search"], c["form"], bw, bh, c["kind"], len(rows),
            time.time() - t0), flush=True)
    out["planes"] = np.array(names)
    out["case_fields"] = np.array(HC.CASE_FIELDS)
    out["cases"] = np.array([[c["search"], c["form"], c["bd"], c["bw"], c["bh"], c["method"],
                              c["step_param"], c["cost"], c["epb"], c["spb"], c["hp"],
                              c["mask_stride"], c["fast"], c["has_sp"]] + list(c["sp"]) +
                             [c["plane"]] for c in cases], np.int64)
    out["row_fields"] = np.array(HC.ROW_FIELDS)
    out["rows"] = np.array(rows, np.int64)
    out["geom"] = np.array([X.W, X.H, X.BORDER, X.NREF], np.int32)
    # the restatement must agree before anything is written
    for g in HC.fixture_groups(out):
        J = g.J
        got = HC.group_fullpel(out, g)
        want = g.rows[:, J["best_row"]:J["bestsme"] + 1]
        assert np.array_equal(want, got[:, :5]), (g.index, g.prm, want.tolist(), got.tolist())
        out["rows"][out["rows"][:, 0] == g.index, J["steps"]] = got[:, 5]
        if g.prm["has_sp"]:
            for which in ((0, 1) if g.prm["search"] == HC.COMP else (0,)):
                sgot = HC.group_subpel(out, g, which)
                swant = HC.sp_rows(g, which)
                assert np.array_equal(swant, sgot), (g.index, which, g.prm, swant.tolist(),
                                                     sgot.tolist())
    print(HC.check_coverage(out))
    if dry:
        print("dry run: %d rows in %d cases, %.0f s; nothing written" % (
            len(rows), len(cases), time.time() - t0))
        return
    path = os.path.join(HERE, "fix_mcomp_comp_hbd.npz")
    save_npz(path, out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print("%d rows in %d cases, %d bytes, %.0f s" % (len(rows), len(cases), size,
                                                      time.time() - t0))


if __name__ == "__main__":
    main()
