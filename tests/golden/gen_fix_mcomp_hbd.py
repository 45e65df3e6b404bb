"""Golden fixture of the high-bit-depth single-reference searches, from the
reference's own C text executed by cinterp.py (through HbdTU, which lets the
interpreter take an element's address behind a tagged pointer).  The executor
extends gen_fixtures.py's FullpelRef: the planes are uint16 buffers behind tagged
pointers (CONVERT_TO_BYTEPTR), the vfp members are the aom_highbd_* functions
highbd_set_var_fns binds, and the _bits8 / _bits10 / _bits12 SAD wrappers are
the reference's own macro text -- the definitions of MAKE_BFP_SAD_WRAPPER,
MAKE_BFP_SAD4D_WRAPPER, MAKE_SDSF_SKIP_SAD_WRAPPER and
MAKE_SDSF_SKIP_SAD_4D_WRAPPER and their invocation lines are read from
av1/encoder/encoder_utils.h by name at generation time and expanded by the
interpreter's preprocessor (the header as a whole needs the encoder's
top-level structs).

  fix_mcomp_hbd.npz
    src__<set>, refs__<set>  the plane sets of tests/_hbdsearch_ref.py
                             (planes, cases["plane"] indexes them)
    case_fields, cases       one case per call pair: bit depth, block size,
                             the full-pel parameters and the parameters of
                             the sub-pel search that follows it
    row_fields, rows         one job each: the full-pel job, the reference's
                             best mv, return value and cost list (INT_MAX x 5
                             when the case passes none), the SubpelMvLimits
                             and the reference's sub-pel result from that
                             best mv with that cost list; `steps` /
                             `searches` (the reference reports none) are the
                             counts of tests/_hbdsearch_ref.py, whose walk
                             the other fields pin

Every row is also run through tests/_hbdsearch_ref.py here and must agree,
and the rows must contain what _hbdsearch_ref.check_coverage lists: a
disagreement or a missing item stops the generation.

Usage: python tests/golden/gen_fix_mcomp_hbd.py
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
import _hbdsearch_ref as H  # noqa: E402
import _mvextremes as X  # noqa: E402
import cinterp as C  # noqa: E402
from gen_fixtures import (MS_INIT, MV_MAX, REF, FullpelRef, _get, _set, check_errors,  # noqa: E402
                          nmv_cost_tables)

METHODS = ["DIAMOND", "NSTEP", "NSTEP_8PT"]           # index = SEARCH_METHODS value
COST_NAMES = {X.ENTROPY: "MV_COST_ENTROPY", X.L1: "MV_COST_L1_HDRES", X.NONE: "MV_COST_NONE"}
SP_FN = {CS.TREE: "av1_find_best_sub_pixel_tree",
         CS.PRUNED: "av1_find_best_sub_pixel_tree_pruned",
         CS.PRUNED_MORE: "av1_find_best_sub_pixel_tree_pruned_more"}
FSTOPS = ["EIGHTH_PEL", "QUARTER_PEL", "HALF_PEL", "FULL_PEL"]
SIZES = [(4, 4), (8, 8), (16, 8), (16, 16)]
WRAPPERS = ["MAKE_BFP_SAD_WRAPPER", "MAKE_BFP_SAD4D_WRAPPER", "MAKE_SDSF_SKIP_SAD_WRAPPER",
            "MAKE_SDSF_SKIP_SAD_4D_WRAPPER"]


def wrapper_text(sizes):
    """The four wrapper macros' definitions and, for `sizes`, their
    invocations, as encoder_utils.h writes them."""
    with open(os.path.join(REF, "av1/encoder/encoder_utils.h")) as fh:
        lines = fh.read().split("\n")
    out = []
    for name in WRAPPERS:
        a = next(i for i, l in enumerate(lines) if l.startswith("#define %s(" % name))
        b = a
        while lines[b].rstrip().endswith("\\"):
            b += 1
        out += lines[a:b + 1]
    want = set()
    for bw, bh in sizes:
        sz = "%dx%d" % (bw, bh)
        want |= {"aom_highbd_sad" + sz, "aom_highbd_sad%sx4d" % sz, "aom_highbd_sad%sx3d" % sz,
                 "aom_highbd_sad_skip_" + sz, "aom_highbd_sad_skip_%sx4d" % sz}
    pat = re.compile(r"^(%s)\((\w+)\)$" % "|".join(WRAPPERS))
    found = set()
    for l in lines:
        m = pat.match(l.strip())
        if m and m.group(2) in want and m.group(2) not in found:
            found.add(m.group(2))
            out.append(l)
    return "\n".join(out) + "\n", found


class HbdTU(C.TU):
    """cinterp's translation unit, taking `&p[i]` of a wild pointer as p + i:
    a highbd plane pointer is a tagged address (CONVERT_TO_BYTEPTR), of which
    get_buf_from_fullmv and get_buf_from_mv (mcomp.h:387, mcomp.c:2366) take
    an element's address, and the interpreter locates elements only inside
    buffers it knows.  The two spellings mean the same in C; every other
    expression goes to cinterp unchanged."""

    def unop(self, fs, e):
        inner = e[2]
        if e[1] == "&" and inner[0] == "index":
            bf, bt = self.rvalue(fs, inner[1])
            xf, xt = self.rvalue(fs, inner[2])
            if isinstance(bt, C.Ptr) and C.is_int(xt) and \
                    not isinstance(bt.to, (C.Struct, C.Arr)):
                el, es = bt.to, C.slots(bt.to)

                def f(fr):
                    p = bf(fr)
                    if p.buf is None:
                        return C.Pointer(None, p.off + xf(fr) * C.sizeof(el), el)
                    o = p.off + xf(fr) * es
                    if o < 0:
                        raise C.CError("out-of-bounds access at offset %d" % o)
                    return C.Pointer(p.buf, o, el)
                return f, C.Ptr(el)
        return C.TU.unop(self, fs, e)


class HbdRef(FullpelRef):
    """FullpelRef over uint16 planes with the high-bit-depth members, and the
    three sub-pel searches in the same translation unit."""

    def __init__(self, tables, stride, width, height, border, sizes):
        # (FullpelRef's own set-up, over an HbdTU)
        self.tu = tu = HbdTU(REF, ["aom_dsp/sad.c", "aom_dsp/variance.c", "av1/encoder/mcomp.c"],
                             C.reference_defines(REF))
        check_errors(tu, ["av1_full_pixel_search", "av1_set_mv_search_range"] +
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
        text, self.wrapped = wrapper_text(sizes)
        tu.add_source(text, "<encoder_utils.h wrappers>")
        check_errors(tu, sorted(SP_FN.values()) + ["av1_set_subpel_mv_search_range"] +
                     ["%s_bits%d" % (n, bd) for n in sorted(self.wrapped) for bd in (8, 10, 12)])
        # xd: mi[0] not intrabc, unscaled reference (as SubpelRef sets it up)
        self.xd = tu.struct_obj("MACROBLOCKD")
        mbmi = tu.struct_obj("MB_MODE_INFO")
        sf = tu.struct_obj("struct scale_factors")
        _set(sf.buf[0], x_scale_fp=1 << 14, y_scale_fp=1 << 14)
        _set(self.xd.buf[0], mi=C.Pointer([mbmi], 0, C.Ptr(tu.ctype("MB_MODE_INFO"))))
        _get(self.xd.buf[0], "block_ref_scale_factors")[0] = sf

    def set_planes(self, src_np, refs_np):
        self.src_buf = self.tu.buffer("uint16_t", src_np.reshape(-1).tolist())
        self.ref_bufs = [self.tu.buffer("uint16_t", r.reshape(-1).tolist()) for r in refs_np]

    def plane_ptr(self, buf, off):
        return self.tu.tagged(C.Pointer(buf.buf, off, buf.ty))

    def vtab(self, bw, bh, bd):
        if (bw, bh, bd) not in self.vtabs:
            sz = "%dx%d" % (bw, bh)

            def fn(name):
                return self.tu.func("%s_bits%d" % (name, bd)) if name in self.wrapped else None
            vtab = self.tu.struct_obj("aom_variance_fn_ptr_t")
            _set(vtab.buf[0], sdf=fn("aom_highbd_sad" + sz), sdsf=fn("aom_highbd_sad_skip_" + sz),
                 sdx4df=fn("aom_highbd_sad%sx4d" % sz), sdx3df=fn("aom_highbd_sad%sx3d" % sz),
                 sdsx4df=fn("aom_highbd_sad_skip_%sx4d" % sz),
                 vf=self.tu.func("aom_highbd_%d_variance%s" % (bd, sz)),
                 svf=self.tu.func("aom_highbd_%d_sub_pixel_variance%s" % (bd, sz)))
            self.vtabs[(bw, bh, bd)] = vtab
        return self.vtabs[(bw, bh, bd)]

    def bufs(self, bw, bh, src_off, k, ref_off):
        tu, stride = self.tu, self.stride
        sbuf = tu.struct_obj("struct buf_2d")
        _set(sbuf.buf[0], buf=self.plane_ptr(self.src_buf, src_off), stride=stride, width=bw,
             height=bh)
        rbuf = tu.struct_obj("struct buf_2d")
        _set(rbuf.buf[0], buf=self.plane_ptr(self.ref_bufs[k], ref_off), stride=stride,
             width=self.W, height=self.H)
        return sbuf, rbuf

    def cost_params(self, mcp, ref_mv, ctype, epb, spb, hp, full):
        tu = self.tu
        rmv = tu.struct_obj("MV")
        _set(rmv.buf[0], row=ref_mv[0], col=ref_mv[1])
        mj, mc = self.tabs["hp" if hp else "lp"]
        _set(mcp, ref_mv=rmv, mv_cost_type=self.E[ctype], mvjcost=mj, error_per_bit=epb,
             sad_per_bit=spb)
        if full:
            _set(mcp, full_ref_mv=tu.func("get_fullmv_from_mv")(rmv))
        _get(mcp, "mvcost")[0], _get(mcp, "mvcost")[1] = mc[0], mc[1]

    def fullpel(self, bw, bh, bd, mname, use_cl, ctype, skip, step_param, src_off, k, ref_off,
                ref_mv, start, lims, epb, spb, hp):
        """(best row, best col, var, the five cost-list entries)."""
        tu, E = self.tu, self.E
        vtab = self.vtab(bw, bh, bd)
        sbuf, rbuf = self.bufs(bw, bh, src_off, k, ref_off)
        ms = tu.struct_obj("FULLPEL_MOTION_SEARCH_PARAMS")
        P = ms.buf[0]
        _set(P, bsize=E["BLOCK_%dX%d" % (bw, bh)], vfp=vtab, search_method=E[mname],
             search_sites=self.cfgs[mname], run_mesh_search=0, prune_mesh_search=0,
             mesh_search_mv_diff_threshold=4, force_mesh_thresh=0x7FFFFFFF,
             fine_search_interval=0, is_intra_mode=0, fast_obmc_search=0)
        _set(_get(P, "ms_buffers"), ref=rbuf, src=sbuf, second_pred=None, mask=None,
             mask_stride=0, inv_mask=0, wsrc=None, obmc_mask=None)
        L = tu.struct_obj("FullMvLimits").buf[0]
        _set(L, col_min=lims[0], col_max=lims[1], row_min=lims[2], row_max=lims[3])
        _set(P, mv_limits=L)
        self.cost_params(_get(P, "mv_cost_params"), ref_mv, ctype, epb, spb, hp, True)
        sk = skip and bh >= 16
        vt = vtab.buf[0]
        _set(P, sdf=_get(vt, "sdsf" if sk else "sdf"),
             sdx4df=_get(vt, "sdsx4df" if sk else "sdx4df"),
             sdx3df=_get(vt, "sdsx4df" if sk else "sdx3df"))
        smv = C.new_obj(tu.ctype("FULLPEL_MV"))
        _set(smv, row=start[0], col=start[1])
        best = tu.struct_obj("FULLPEL_MV")
        cl = tu.buffer("int", [0x7FFFFFFF] * 5) if use_cl else None
        var = tu.func("av1_full_pixel_search")(smv, ms, step_param, cl, best, None)
        bm = best.buf[0]
        return [_get(bm, "row"), _get(bm, "col"), var] + \
            (list(cl.buf) if use_cl else [0x7FFFFFFF] * 5)

    def subpel(self, bw, bh, bd, meth, hp, fstop, iters, ctype, cl_vals, epb, src_off, k, ref_off,
               ref_mv, start, slims):
        """(best row, best col, besterr, distortion, sse)."""
        tu, E = self.tu, self.E
        ms = tu.struct_obj("SUBPEL_MOTION_SEARCH_PARAMS")
        P = ms.buf[0]
        _set(_get(P, "mv_limits"), col_min=slims[0], col_max=slims[1], row_min=slims[2],
             row_max=slims[3])
        cl = tu.buffer("int", [int(v) for v in cl_vals]) if cl_vals is not None else None
        _set(P, allow_hp=hp, cost_list=cl, forced_stop=E[FSTOPS[fstop]], iters_per_step=iters)
        self.cost_params(_get(P, "mv_cost_params"), ref_mv, ctype, epb, 0, hp, False)
        sbuf, rbuf = self.bufs(bw, bh, src_off, k, ref_off)
        vp = _get(P, "var_params")
        _set(vp, vfp=self.vtab(bw, bh, bd), w=bw, h=bh,
             subpel_search_type=E["USE_2_TAPS_ORIG" if meth == CS.TREE else "USE_2_TAPS"])
        _set(_get(vp, "ms_buffers"), ref=rbuf, src=sbuf, second_pred=None, mask=None,
             mask_stride=0, inv_mask=0, wsrc=None, obmc_mask=None)
        smv = C.new_obj(tu.ctype("MV"))
        _set(smv, row=start[0], col=start[1])
        best = tu.struct_obj("MV")
        dist, sse = tu.buffer("int", 1), tu.buffer("unsigned int", 1)
        err = tu.func(SP_FN[meth])(self.xd, None, ms, smv, best, dist, sse, None)
        bm = best.buf[0]
        return [_get(bm, "row"), _get(bm, "col"), err, dist.buf[0], sse.buf[0]]


# ------------------------------------------------------------------- cases --
def case(bd, bw, bh, kind, method=0, step_param=5, cost=X.ENTROPY, epb=X.LOW_LAMBDA[0],
         spb=X.LOW_LAMBDA[1], hp=0, skip=0, use_cl=1, sp=(CS.PRUNED_MORE, 0, 0, 1, 1),
         ref_mv=(0, 0), start=(0, 0), njobs=2, salt=0, limits=None):
    """sp: (method, forced_stop, allow_hp, iters, use_cl) of the sub-pel search."""
    return dict(bd=bd, bw=bw, bh=bh, kind=kind, method=method, step_param=step_param, cost=cost,
                epb=epb, spb=spb, hp=hp, skip=skip, use_cl=use_cl, sp=sp, ref_mv=ref_mv,
                start=start, njobs=njobs, salt=salt, limits=limits)


SP_COMBOS = [(CS.PRUNED_MORE, 0, 1, 1, 1), (CS.PRUNED, 0, 1, 2, 1), (CS.TREE, 0, 1, 2, 0),
             (CS.PRUNED_MORE, 1, 0, 2, 0), (CS.TREE, 1, 0, 1, 0), (CS.PRUNED, 2, 0, 1, 1),
             (CS.TREE, 0, 0, 2, 0), (CS.PRUNED_MORE, 0, 1, 2, 1), (CS.PRUNED, 0, 1, 1, 0)]


def all_cases():
    cs = []
    k = 0
    costs = (X.ENTROPY, X.L1, X.NONE)
    kinds = ("flat_128_128", "ramp_x", "periodic_2", "smooth")
    # every depth under every method, the cost types rotating so that each
    # depth meets all three
    for bi, bd in enumerate((8, 10, 12)):
        for method in range(3):
            sp_ = (5, 6, 0)[(k + bi) % 3]
            bw, bh = SIZES[k % 2] if sp_ == 0 else SIZES[1 + k % 3]
            ref_mv = [(0, 0), (13, -21), (-40, 33)][k % 3]
            at = ((ref_mv[0] + 4) >> 3, (ref_mv[1] + 4) >> 3)
            start = at if k % 2 else (at[0] + 5 - k % 7, at[1] - 4 + k % 5)
            cs.append(case(bd, bw, bh, kinds[k % 4], method, sp_, costs[(bi + method) % 3],
                           ref_mv=ref_mv, start=start, salt=k, use_cl=k % 3 != 2,
                           sp=SP_COMBOS[k % 9], hp=SP_COMBOS[k % 9][2]))
            k += 1
    # smooth content: the sub-pel searches move (every depth, every method)
    for bd in (8, 10, 12):
        for i in range(3):
            cs.append(case(bd, *SIZES[1 + (k % 3)], "smooth", k % 3, 6, costs[k % 3], salt=k,
                           njobs=3, sp=SP_COMBOS[(k + i) % 9], hp=SP_COMBOS[(k + i) % 9][2],
                           start=(1, -1), use_cl=1))
            k += 1
    # low-bit noise on a flat plane: the shift per block and per row differ
    for bd in (10, 12):
        for method in range(3):
            cs.append(case(bd, *SIZES[1 + method], "flat_128_128", method, 7, X.NONE, salt=k,
                           njobs=3, start=(2, -3), sp=SP_COMBOS[k % 9], hp=SP_COMBOS[k % 9][2]))
            k += 1
    # the downsampled SAD: kept (periodic content) and redone (stripes)
    for bd in (8, 10, 12):
        cs.append(case(bd, 16, 16, "periodic_2", k % 3, 6, costs[k % 3], skip=1, salt=k))
        k += 1
        cs.append(case(bd, 16, 16, "stripes", k % 3, 7, costs[k % 3], skip=1, salt=k,
                       start=(1, 2)))
        k += 1
    # the variance: negative before the clamp; the largest sums
    for bd, (bw, bh) in ((10, (8, 8)), (12, (16, 16)), (10, (16, 16))):
        cs.append(case(bd, bw, bh, "negclamp", k % 3, 7, X.NONE, njobs=1, salt=k))
        k += 1
    cs.append(case(12, 16, 16, "flat_255_0", 0, 6, njobs=1))
    cs.append(case(12, 16, 16, "flat_0_255", 1, 6, X.L1, njobs=1))
    cs.append(case(12, 8, 8, "flat_0_255", 2, 7, X.NONE, njobs=1, sp=SP_COMBOS[2], hp=1))
    # windows narrowed to a row, a column; a start outside the window
    for lim in ("row", "col", "clamped"):
        cs.append(case((10, 12, 8)[k % 3], *SIZES[k % 4], "periodic_2", k % 3, 5, costs[k % 2],
                       ref_mv=(13, -21), start=(2, -3), salt=k, limits=lim, sp=SP_COMBOS[k % 9],
                       hp=SP_COMBOS[k % 9][2]))
        k += 1
    # sub-pel candidates outside the limits: a search that ends on the
    # window's edge (the SubpelMvLimits are the block's own)
    cs.append(case(10, 8, 8, "smooth", 0, 7, X.NONE, njobs=2, limits="edge", sp=SP_COMBOS[2],
                   hp=1))
    # a lambda at which rate * error_per_bit passes 2^31
    epb, ref_mv, hp = X.HIGH_LAMBDA[1]
    cs.append(case(10, 8, 8, "periodic_2", 0, 6, X.ENTROPY, epb, X.SAD_PER_BIT_TOP, hp,
                   ref_mv=ref_mv, sp=(CS.PRUNED_MORE, 0, hp, 1, 1)))
    # one 32x32 row (the source no longer fits the registers)
    cs.append(case(10, 32, 32, "smooth", 1, 8, X.ENTROPY, njobs=1, skip=1, start=(1, 0),
                   sp=SP_COMBOS[0], hp=1))
    return cs


def case_jobs(c):
    jobs = X.frame(c["bw"], c["bh"], c["ref_mv"], c["start"])
    jobs = X.spread(jobs, max(c["njobs"], 3), c["salt"])[:c["njobs"]]
    lim = c["limits"]
    if lim in ("row", "col"):
        jobs = X.narrowed(jobs, lim, (3, -2))
    elif lim == "clamped":          # the start lies outside the window on both axes
        jobs["row_max"] = np.minimum(jobs["row_max"], jobs["start_row"] - 2)
        jobs["col_min"] = np.maximum(jobs["col_min"], jobs["start_col"] + 3)
    return jobs


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
    t0 = time.time()
    t = nmv_cost_tables()
    cases = all_cases()
    sizes = sorted({(c["bw"], c["bh"]) for c in cases})
    R = HbdRef(t, X.STRIDE, X.W, X.H, X.BORDER, sizes)
    out, names = {}, []
    rows, loaded = [], None
    for ci, c in enumerate(cases):
        bw, bh, bd = c["bw"], c["bh"], c["bd"]
        key = H.plane_key(c["kind"], bd, bw, bh)
        if key not in names:
            names.append(key)
            out["src__" + key], out["refs__" + key] = H.planes(c["kind"], bd, bw, bh)
        if loaded != key:
            R.set_planes(out["src__" + key], out["refs__" + key])
            loaded = key
        c["plane"] = names.index(key)
        spm, fstop, sphp, iters, sp_cl = c["sp"]
        for jb in case_jobs(c):
            k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
            so, ro = int(jb["src_off"]), int(jb["ref_off"]) - k * X.PLANE
            lims = [int(jb[f]) for f in ("col_min", "col_max", "row_min", "row_max")]
            fp = R.fullpel(bw, bh, bd, METHODS[c["method"]], c["use_cl"], COST_NAMES[c["cost"]],
                           c["skip"], c["step_param"], so, k, ro, c["ref_mv"],
                           (int(jb["start_row"]), int(jb["start_col"])), lims, c["epb"], c["spb"],
                           c["hp"])
            slims = list(CS.block_limits(so, bw, bh, c["ref_mv"]))
            if c["limits"] == "edge":   # the result sits on the limits' corner
                slims[1], slims[3] = 8 * fp[1], 8 * fp[0]
            sp = R.subpel(bw, bh, bd, spm, sphp, fstop, iters, COST_NAMES[c["cost"]],
                          fp[3:8] if sp_cl else None, c["epb"], so, k, ro, c["ref_mv"],
                          (8 * fp[0], 8 * fp[1]), slims)
            rows.append([ci] + [int(jb[f]) for f in X.JOB_FIELDS] + fp[:3] + [0, 0] + fp[3:8] +
                        slims + sp)
        print("  case %3d/%d  bd %2d %2dx%-2d %-12s %4d rows  %.0fs" % (
            ci, len(cases), bd, bw, bh, c["kind"], len(rows), time.time() - t0), flush=True)
    out["planes"] = np.array(names)
    out["case_fields"] = np.array(H.CASE_FIELDS)
    out["cases"] = np.array([[c["bd"], c["bw"], c["bh"], c["method"], c["step_param"], c["cost"],
                              c["epb"], c["spb"], c["hp"], c["skip"], c["use_cl"]] +
                             list(c["sp"]) + [c["plane"]] for c in cases], np.int64)
    out["row_fields"] = np.array(H.ROW_FIELDS)
    out["rows"] = np.array(rows, np.int64)
    out["geom"] = np.array([X.W, X.H, X.BORDER, X.NREF], np.int32)
    # the restatement must agree before anything is written
    for g in H.fixture_groups(out):
        J = g.J
        got, cl = H.group_fullpel(out, g)
        want = g.rows[:, J["best_row"]:J["bestsme"] + 1]
        assert np.array_equal(want, got[:, :3]), (g.index, g.prm, want.tolist(), got.tolist())
        if g.prm["use_cl"]:
            assert np.array_equal(g.rows[:, J["cl0"]:J["cl4"] + 1], cl), (g.index, g.prm)
        sel = out["rows"][:, 0] == g.index
        out["rows"][sel, J["steps"]] = got[:, 3]
        out["rows"][sel, J["searches"]] = got[:, 4]
        sgot = H.group_subpel(out, g)
        swant = g.rows[:, J["sp_best_row"]:J["sp_sse"] + 1]
        assert np.array_equal(swant, sgot), (g.index, g.prm, swant.tolist(), sgot.tolist())
    print(H.check_coverage(out))
    path = os.path.join(HERE, "fix_mcomp_hbd.npz")
    save_npz(path, out)
    print("%d rows in %d cases, %d bytes, %.0f s" % (len(rows), len(cases), os.path.getsize(path),
                                                      time.time() - t0))


if __name__ == "__main__":
    main()
