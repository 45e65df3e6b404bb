"""CPU tests of the high-bit-depth compound, masked and OBMC search layer (no
GPU):
* include/lavish_dsp.h declares, and the library exports, the five batch calls;
* every argument the calls refuse is refused with its return code before any
  device work (the pointers are garbage);
* tests/_hbdcomp_ref.py equals every row of
  tests/golden/fix_mcomp_comp_hbd.npz (the reference's own results), every
  field, full-pel and sub-pel from both starts;
* the fixture covers what it should (the checks its generator stops on);
* a sample of the fixture re-derived from the reference's C text (skipped
  where the reference sources are absent);
* every kernel of csrc/mcomp_comp_hbd.hip and csrc/subpel_comp_hbd.hip in the
  built library runs without scratch or spilled VGPRs."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _hbdcomp_ref as HC
import _mvextremes as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "lavish_dsp.h")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")
COMP, REFINE, OBMC, CSUB, OSUB = CALLS = (
    "lavish_highbd_comp_full_pixel_search_batch", "lavish_highbd_refining_search_8p_batch",
    "lavish_highbd_obmc_full_pixel_search_batch",
    "lavish_highbd_comp_find_best_sub_pixel_tree_batch",
    "lavish_highbd_obmc_find_best_sub_pixel_tree_batch")
S, P = HC.S, HC.P


def _lib():
    import lavish_dsp
    import lavish_dsp.motion  # noqa: F401  (sets the argtypes)
    return lavish_dsp.lib()


def test_header_declares_and_library_exports_the_calls():
    out = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True, capture_output=True,
                         text=True).stdout
    declared = set(re.findall(r"\b(lavish_\w+)\s*\(", out))
    L = _lib()
    from lavish_dsp import motion as M
    for name in CALLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert callable(getattr(M, name[len("lavish_"):])), name


# ---------------------------------------------------------------- rejects --
_vp = ctypes.c_void_p
GARBAGE = _vp(0xDEAD0000)      # never dereferenced: the calls return first


def _cost(ctype=X.NONE, tables=True):
    from lavish_dsp import motion as M
    c = M.MvCostParams(ctype, 4, 37, 0)
    if tables:
        c.mvjcost = c.mvcost[0] = c.mvcost[1] = 0xDEAD0000
    return c


def _c(cost):
    return None if cost is None else ctypes.byref(_cost(*(() if cost == "ok" else cost)))


def _p(on):
    return GARBAGE if on else None


def comp_args(w=16, h=16, bd=10, njobs=1, method=1, step_param=5, cost="ok", src=True, ref=True,
              jobs=True, out=True, second=True, mask=False, mask_stride=16):
    return [_p(src), 64, _p(ref), 64, w, h, bd, _p(jobs), njobs, method, step_param, _c(cost),
            _p(second), _p(mask), mask_stride, _p(out), None]


def refine_args(w=16, h=16, bd=10, njobs=1, cost="ok", src=True, ref=True, jobs=True, out=True,
                second=True, mask=False, mask_stride=16):
    return [_p(src), 64, _p(ref), 64, w, h, bd, _p(jobs), njobs, _c(cost), _p(second), _p(mask),
            mask_stride, _p(out), None]


def obmc_args(w=16, h=16, bd=10, njobs=1, method=1, step_param=5, cost="ok", ref=True, jobs=True,
              out=True, wsrc=True, omask=True, fast=0):
    return [_p(ref), 64, w, h, bd, _p(jobs), njobs, method, step_param, _c(cost), fast, _p(wsrc),
            _p(omask), _p(out), None]


def csub_args(w=16, h=16, bd=10, njobs=1, method=2, forced_stop=0, iters=1, cost="ok", src=True,
              ref=True, jobs=True, out=True, second=True, mask=False, mask_stride=16,
              fullpel=False, start_from=0):
    return [_p(src), 64, _p(ref), 64, w, h, bd, _p(jobs), _p(fullpel), start_from, njobs, method,
            forced_stop, 1, iters, _c(cost), _p(second), _p(mask), mask_stride, _p(out), None]


def osub_args(w=16, h=16, bd=10, njobs=1, forced_stop=0, iters=1, cost="ok", ref=True, jobs=True,
              out=True, wsrc=True, omask=True):
    return [_p(ref), 64, w, h, bd, _p(jobs), None, njobs, forced_stop, 1, iters, _c(cost),
            _p(wsrc), _p(omask), _p(out), None]


BAD_SIZES = [(12, 12), (4, 32), (32, 4), (256, 256), (0, 0), (8, 64), (16, 15)]
BAD_DEPTHS = (9, 0, 7, 11, 13, 16, -8)
BAD_COSTS = [None, (-1,), (5,), (X.ENTROPY, False)]
BAD_METHODS = [(dict(method=m), -4) for m in (-1, 3, 4, 5, 6, 7, 8, 9, 10, 11)]
BAD_STEPS = [(dict(method=m, step_param=s), -1)
             for m, s in ((0, -1), (0, 11), (1, 15), (2, 16), (0, 1 << 20))]


def _nulls(names, rc):
    return [(dict(**{k: False}), rc) for k in names]


REJECTS = {
    COMP: (comp_args,
           [(dict(w=w, h=h), -3) for w, h in BAD_SIZES] +
           [(dict(bd=b), -7) for b in BAD_DEPTHS] +
           _nulls(("src", "ref", "jobs", "out", "second"), -7) +
           [(dict(mask=True, mask_stride=15), -7)] + BAD_METHODS + BAD_STEPS +
           [(dict(cost=c), -2) for c in BAD_COSTS] +
           # the order: method, step_param, cost, then pointers and depth, size
           [(dict(method=5, step_param=99, cost=None, bd=9, w=12), -4),
            (dict(step_param=99, cost=None, bd=9, w=12), -1), (dict(cost=None, bd=9, w=12), -2),
            (dict(bd=9, w=12), -7)]),
    REFINE: (refine_args,
             [(dict(w=w, h=h), -3) for w, h in BAD_SIZES] +
             [(dict(bd=b), -7) for b in BAD_DEPTHS] +
             _nulls(("src", "ref", "jobs", "out"), -7) +
             [(dict(mask=True, mask_stride=15), -7), (dict(mask=True, second=False), -7)] +
             [(dict(cost=c), -2) for c in BAD_COSTS] +
             [(dict(cost=None, bd=9, w=12), -2), (dict(bd=9, w=12), -7)]),
    OBMC: (obmc_args,
           [(dict(w=w, h=h), -3) for w, h in BAD_SIZES] +
           [(dict(bd=b), -7) for b in BAD_DEPTHS] +
           _nulls(("ref", "jobs", "out", "wsrc", "omask"), -7) + BAD_METHODS + BAD_STEPS +
           [(dict(cost=c), -2) for c in BAD_COSTS] +
           [(dict(method=5, step_param=99, cost=None, bd=9, w=12), -4), (dict(bd=9, w=12), -7)]),
    CSUB: (csub_args,
           [(dict(w=w, h=h), -3) for w, h in BAD_SIZES] +
           [(dict(bd=b), -8) for b in BAD_DEPTHS] +
           _nulls(("src", "ref", "jobs", "out", "second"), -8) +
           [(dict(mask=True, mask_stride=15), -8), (dict(start_from=2), -8),
            (dict(start_from=-1), -8), (dict(start_from=1), -9)] +
           [(dict(forced_stop=f), -1) for f in (-1, 4)] +
           [(dict(cost=c), -2) for c in BAD_COSTS] +
           [(dict(iters=i), -4) for i in (0, 3)] +
           [(dict(method=m), -6) for m in (-1, 3)] +
           # the order: forced_stop, cost, iters, method, size, then pointers and depth
           [(dict(forced_stop=4, cost=None, iters=0, method=3, w=12, bd=9), -1),
            (dict(cost=None, iters=0, method=3, w=12, bd=9), -2),
            (dict(iters=0, method=3, w=12, bd=9), -4), (dict(method=3, w=12, bd=9), -6),
            (dict(w=12, bd=9), -3), (dict(bd=9, start_from=1), -8)]),
    OSUB: (osub_args,
           [(dict(w=w, h=h), -3) for w, h in BAD_SIZES] +
           [(dict(bd=b), -8) for b in BAD_DEPTHS] +
           _nulls(("ref", "jobs", "out", "wsrc", "omask"), -8) +
           [(dict(forced_stop=f), -1) for f in (-1, 4)] +
           [(dict(cost=c), -2) for c in BAD_COSTS] +
           # estimate_obmc_mvcost asserts on the L1 types
           [(dict(cost=(t,)), -2) for t in (1, 2, 3)] +
           [(dict(iters=i), -4) for i in (0, 3)] +
           [(dict(cost=(3,), w=12, bd=9), -2), (dict(w=12, bd=9), -3)]),
}
REJECT_CASES = [(name, kw, rc) for name, (_, cases) in REJECTS.items() for kw, rc in cases]


@pytest.mark.parametrize("name,kw,rc", REJECT_CASES,
                         ids=lambda v: str(v).replace(" ", "").replace("lavish_highbd_", ""))
def test_calls_refuse_bad_arguments_before_any_device_work(name, kw, rc):
    assert getattr(_lib(), name)(*REJECTS[name][0](**kw)) == rc


def test_no_jobs_is_a_no_op():
    L = _lib()
    for n in (0, -3):
        for name, (args, _) in REJECTS.items():
            assert getattr(L, name)(*args(njobs=n, w=12, bd=9, cost=None)) == 0, name


# ---------------------------------------------------------------- fixture --
@pytest.fixture(scope="module")
def F():
    return HC.load_fixture()


def test_full_pel_restatement_equals_every_fixture_row(F):
    bad, n = [], 0
    for g in HC.fixture_groups(F):
        J = g.J
        got = HC.group_fullpel(F, g)
        want = g.rows[:, J["best_row"]:J["steps"] + 1]
        n += len(want)
        if not np.array_equal(want, got):
            bad.append((g.index, g.prm, want.tolist(), got.tolist()))
    assert n == len(F["rows"]) and not bad, bad[:3]


def test_sub_pel_restatement_equals_every_fixture_row(F):
    bad, n = [], 0
    none = [P.NO_SEARCH[f] for f in HC.SUB_FIELDS]
    for g in HC.fixture_groups(F):
        for which in (0, 1):
            want = HC.sp_rows(g, which)
            if not g.prm["has_sp"] or (which and g.prm["search"] != HC.COMP):
                assert (want == none).all(), (g.index, which)
                continue
            got = HC.group_subpel(F, g, which)
            n += len(want)
            if not np.array_equal(want, got):
                bad.append((g.index, which, g.prm, want.tolist(), got.tolist()))
    assert n > len(F["rows"]) and not bad, bad[:3]


def test_fixture_covers_what_it_should(F):
    full, sub = HC.check_coverage(F)     # (asserts every item; the counts for the record)
    for fam in ("sdaf", "msdf", "osdf"):
        assert full["per_row_%s_10" % fam] and full["per_row_%s_12" % fam]
    for fam in ("svaf", "msvf", "ovf"):
        assert full["neg_round_" + fam] and full["clamped_" + fam]
    assert full["second_valid"] and full["second_invalid"] and full["sp1_int_max"]
    assert full["mask_stride_wide"] and full["low_bits"] and full["max_vs_zero"]
    assert sub["obmc_centre_matters"] and sub["oob"] and sub["second_level"]
    groups = list(HC.fixture_groups(F))
    assert {(g.prm["bw"], g.prm["bh"]) for g in groups} == {(4, 4), (8, 8), (16, 8), (16, 16),
                                                           (32, 32)}
    # one 32x32 row per form
    big = [(g.prm["search"], g.prm["form"], int(c["invert_mask"]), g.prm["fast_obmc"])
           for g in groups if g.prm["bw"] == 32 for c in g.cjobs]
    assert len(big) == len(set(big)) == 6
    assert {g.prm["sp_method"] for g in groups if g.prm["has_sp"]} == {P.TREE, P.PRUNED,
                                                                      P.PRUNED_MORE}
    assert {g.prm["sp_forced_stop"] for g in groups if g.prm["has_sp"]} >= {0, 1, 2}
    assert {g.prm["sp_iters"] for g in groups} == {1, 2}
    assert any(g.prm["error_per_bit"] == X.HIGH_LAMBDA[1][0] for g in groups)
    b = np.concatenate([g.cjobs["base"] for g in groups])
    assert ((b["row_min"] == b["row_max"]) & (b["col_min"] < b["col_max"])).any()
    assert ((b["row_min"] < b["row_max"]) & (b["col_min"] == b["col_max"])).any()
    assert ((b["start_row"] > b["row_max"]) & (b["start_col"] < b["col_min"])).any()
    for g in groups:
        sh = g.prm["bd"] - 8
        src, ref = HC.group_planes(F, g)
        assert int(src.max()) < 1 << g.prm["bd"] and int(ref.max()) < 1 << g.prm["bd"]
        if sh and not g.plane.startswith("flat_0") and not g.plane.startswith("flat_255"):
            assert (src & ((1 << sh) - 1)).any() and (ref & ((1 << sh) - 1)).any(), g.plane
    assert F["second"].dtype == np.uint16 and F["mask"].dtype == np.uint8
    assert F["wsrc"].dtype == np.int32 and F["omask"].dtype == np.int32
    assert int(F["mask"].max()) <= 64 and int(F["omask"].max()) <= 4096
    assert os.path.getsize(os.path.join(GOLD, "fix_mcomp_comp_hbd.npz")) < (1 << 20)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_fixture_sample_rederived_from_the_reference_text(F):
    """The first row of one small case per search, re-executed from the C
    text (full-pel, then sub-pel from the best mv), and the wrappers are the
    reference's macro text."""
    sys.path.insert(0, GOLD)
    import gen_fix_mcomp_comp_hbd as G
    from gen_fixtures import REF as REF_ROOT, nmv_cost_tables
    sizes = [(8, 8), (16, 8)]
    text, found = G.wrapper_text(REF_ROOT, sizes)
    assert ">> 2" in text and ">> 4" in text
    assert {"aom_highbd_sad8x8_avg", "aom_highbd_masked_sad8x8", "aom_highbd_obmc_sad8x8"} <= found
    R = G.make_ref(nmv_cost_tables(), sizes)
    done = set()
    for g in HC.fixture_groups(F):
        p, J = g.prm, g.J
        key = (p["search"], p["bd"] > 8)
        if key in done or (p["bw"], p["bh"]) not in sizes or p["step_param"] < 5 or \
                not p["has_sp"] or len(done) >= 4:
            continue
        R.set_planes(F["src__" + g.plane], F["refs__" + g.plane])
        cj, row = g.cjobs[0], g.rows[0]
        jb = cj["base"]
        n, so, mo = p["bw"] * p["bh"], int(cj["second_off"]), int(cj["mask_off"])
        k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
        if p["search"] == HC.OBMC:
            inv = dict(wsrc=F["wsrc"][so:so + n], omask=F["omask"][mo:mo + n])
        else:
            inv = dict(second=F["second"][so:so + n])
            if p["form"] == HC.MASK:
                inv.update(mask=F["mask"][mo:mo + p["bh"] * p["mask_stride"]],
                           mask_stride=p["mask_stride"], invert=int(cj["invert_mask"]))
        c = dict(search=p["search"], form=p["form"], bd=p["bd"], bw=p["bw"], bh=p["bh"],
                 method=p["method"], step_param=p["step_param"], cost=p["cost"],
                 epb=p["error_per_bit"], spb=p["sad_per_bit"], hp=p["hp_tables"],
                 fast=p["fast_obmc"], ref_mv=(int(jb["ref_mv_row"]), int(jb["ref_mv_col"])),
                 sp=(p["sp_method"], p["sp_forced_stop"], p["sp_allow_hp"], p["sp_iters"]))
        fp = R.full(c, jb, k, inv)
        assert fp == row[J["best_row"]:J["bestsme"] + 1].tolist(), (g.index, p)
        slims = [int(row[J[f]]) for f in HC.SP_LIMITS]
        sp = R.sub(c, jb, k, inv, slims, (8 * fp[0], 8 * fp[1]))
        assert sp == HC.sp_rows(g, 0)[0].tolist(), (g.index, p)
        done.add(key)
    assert len(done) == 4 and {k[0] for k in done} >= {HC.COMP, HC.OBMC}


# ---------------------------------------------------------------- kernels --
def test_new_kernels_use_no_scratch():
    """Code-object metadata (tools/kernel_resources.py) of every
    hbd_csearch_kernel (22 block sizes x 4 forms) and hbd_csubpel_kernel (22
    x 3 forms) instantiation: no scratch, no spilled VGPR, and an LDS slice of
    at most 16 KB a workgroup (full-pel) or none (sub-pel)."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler") or \
            shutil.which("c++filt") is None:
        pytest.skip("ROCm code-object tools not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    res = KR.kernel_resources(os.path.join(ROOT, "aom-av1-lavish_amd", "liblavish_hip.so"))
    names = sorted(res)
    for kern, count, lds in (("hbd_csearch_kernel<", 88, 16384), ("hbd_csubpel_kernel<", 66, 0)):
        mine = [(d, res[n]) for n, d in zip(names, KR.demangled(names)) if kern in d]
        assert len(mine) == count, (kern, len(mine))
        for name, v in mine:
            assert v.get("private_segment_fixed_size", 0) == 0, (name, v)
            assert v.get("vgpr_spill_count", 0) == 0, (name, v)
            assert v.get("group_segment_fixed_size", 0) <= lds, (name, v)
