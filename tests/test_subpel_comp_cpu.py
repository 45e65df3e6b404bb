"""CPU tests of the compound / masked / OBMC sub-pel search layer (no GPU):
* include/lavish_dsp.h declares, and the library exports, the two batch
  calls; the record sizes and offsets match ctypes and the numpy dtype;
* every argument the calls refuse is refused with its code before any device
  work (the pointers are NULL or valid host buffers); the same for the four
  single-reference calls, whose checks are the same shared validator;
* tests/_compsubpel_ref.py equals every row of tests/golden/
  fix_subpel_comp.npz (the reference's own results), every field, and with no
  second_pred the CPU oracle of the single-reference search;
* the fixture covers what it should, and moves;
* a sample of the fixture re-derived from the reference's C text (skipped
  where the reference sources are absent);
* the resources of csrc/subpel_comp.hip's kernels in the built library."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _compsearch_ref as S
import _compsubpel_ref as CS
import _mvextremes as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "lavish_dsp.h")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")
CALLS = ["lavish_comp_find_best_sub_pixel_tree_batch",
         "lavish_obmc_find_best_sub_pixel_tree_batch"]


def test_header_declares_and_library_exports_the_calls(tmp_path):
    import lavish_dsp
    from lavish_dsp import motion as M
    out = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True, capture_output=True,
                         text=True).stdout
    declared = set(re.findall(r"\b(lavish_\w+)\s*\(", out))
    assert not [n for n in CALLS if n not in declared]
    L = lavish_dsp.lib()
    assert not [n for n in CALLS if not hasattr(L, n)]
    src = ('#include "lavish_dsp.h"\n'
           '_Static_assert(sizeof(LavishCompSubpelJob) == 56, "job record");\n'
           '_Static_assert(sizeof(LavishSubpelJob) == 32, "base record");\n'
           '_Static_assert(sizeof(LavishSubpelResult) == 16, "result record");\n'
           '_Static_assert(__builtin_offsetof(LavishCompSubpelJob, base) == 0, "");\n'
           '_Static_assert(__builtin_offsetof(LavishCompSubpelJob, second_off) == 32, "");\n'
           '_Static_assert(__builtin_offsetof(LavishCompSubpelJob, mask_off) == 40, "");\n'
           '_Static_assert(__builtin_offsetof(LavishCompSubpelJob, invert_mask) == 48, "");\n'
           '_Static_assert(__builtin_offsetof(LavishSubpelResult, besterr) == 4, "");\n')
    path = tmp_path / "sizes.c"
    path.write_text(src)
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-I",
                        os.path.dirname(HEADER), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    class Job(ctypes.Structure):
        _fields_ = [("src_off", ctypes.c_int64), ("ref_off", ctypes.c_int64)] + \
                   [(n, ctypes.c_int16) for n in X.JOB_FIELDS[2:]] + \
                   [("second_off", ctypes.c_int64), ("mask_off", ctypes.c_int64),
                    ("invert_mask", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    D = M.COMP_SUBPEL_JOB_DTYPE
    assert ctypes.sizeof(Job) == D.itemsize == 56
    assert Job.second_off.offset == D.fields["second_off"][1] == 32
    assert Job.mask_off.offset == D.fields["mask_off"][1] == 40
    assert Job.invert_mask.offset == D.fields["invert_mask"][1] == 48
    assert D.fields["base"][0] == M.SUBPEL_JOB_DTYPE and D.fields["base"][1] == 0
    j = M.comp_subpel_jobs(np.zeros(3, M.SUBPEL_JOB_DTYPE), [5, 6, 7], 9, [0, 1, 0])
    assert j["second_off"].tolist() == [5, 6, 7] and j["mask_off"].tolist() == [9, 9, 9]
    assert j["invert_mask"].tolist() == [0, 1, 0] and j.dtype == D


# ---------------------------------------------------------------- rejects --
class Args:
    """Argument lists of the two calls; every pointer is NULL or a host
    buffer large enough for what it stands for, so nothing invented is ever
    handed over."""

    def __init__(self):
        from lavish_dsp import motion as M
        self.M = M
        self.buf = np.zeros(1 << 16, np.int32)      # planes, jobs, pools, tables, results
        self.p = ctypes.c_void_p(self.buf.ctypes.data)

    def cost(self, ctype=X.NONE, tables=True):
        c = self.M.MvCostParams(ctype, 4, 37, 0)
        if tables:
            mid = self.buf.ctypes.data + 4 * (1 << 15)
            c.mvjcost, c.mvcost[0], c.mvcost[1] = self.buf.ctypes.data, mid, mid
        return c

    def _cost(self, cost):
        return None if cost is None else ctypes.byref(self.cost(*(() if cost == "ok" else cost)))

    def comp(self, w=16, h=16, njobs=1, method=2, stype=0, fstop=0, hp=1, iters=1, cost="ok",
             second=True, mask=True, ms=None, src=True, ref=True, jobs=True, out=True,
             fullpel=False, start_from=0):
        p = self.p
        return [p if src else None, 64, p if ref else None, 64, w, h, p if jobs else None,
                p if fullpel else None, start_from, njobs, method, stype, fstop, hp, iters,
                self._cost(cost), p if second else None, p if mask else None,
                w if ms is None else ms, p if out else None, None]

    def obmc(self, w=16, h=16, njobs=1, stype=0, fstop=0, hp=1, iters=1, cost="ok", wsrc=True,
             mask=True, ref=True, jobs=True, out=True, fullpel=False):
        p = self.p
        return [p if ref else None, 64, w, h, p if jobs else None, p if fullpel else None, njobs,
                stype, fstop, hp, iters, self._cost(cost), p if wsrc else None,
                p if mask else None, p if out else None, None]


BAD_SIZES = [(12, 12), (4, 32), (32, 4), (256, 256), (0, 0), (8, 64), (16, 15)]
BAD_COSTS = [None, (-1,), (5,), (X.ENTROPY, False)]
REJECTS = (
    [(f, dict(fstop=v), -1) for f in ("comp", "obmc") for v in (-1, 4)] +
    [(f, dict(cost=c), -2) for f in ("comp", "obmc") for c in BAD_COSTS] +
    # estimate_obmc_mvcost asserts on the L1 types
    [("obmc", dict(cost=(t,), stype=0), -2) for t in (1, 2, 3)] +
    [("comp", dict(w=w, h=h, ms=300), -3) for w, h in BAD_SIZES] +
    [("obmc", dict(w=w, h=h), -3) for w, h in BAD_SIZES] +
    [(f, dict(iters=v), -4) for f in ("comp", "obmc") for v in (0, 3, -1)] +
    [("comp", dict(method=v), -6) for v in (-1, 3, 4)] +
    [(f, dict(stype=v), -7) for f in ("comp", "obmc") for v in (-1, 4)] +
    [("comp", kw, -8) for kw in (dict(second=False), dict(second=False, mask=False), dict(ms=15),
                                 dict(w=128, h=128, ms=127), dict(src=False), dict(ref=False),
                                 dict(jobs=False), dict(out=False), dict(start_from=2),
                                 dict(start_from=-1), dict(start_from=2, fullpel=True))] +
    [("obmc", kw, -8) for kw in (dict(wsrc=False), dict(mask=False), dict(ref=False),
                                 dict(jobs=False), dict(out=False))] +
    [("comp", dict(start_from=1), -9)])
FUNCS = dict(zip(("comp", "obmc"), CALLS))


def _lib():
    import lavish_dsp
    import lavish_dsp.motion  # noqa: F401  (sets the argtypes)
    return lavish_dsp.lib()


@pytest.mark.parametrize("which,kw,code", REJECTS, ids=lambda v: str(v).replace(" ", ""))
def test_bad_arguments_are_refused_with_their_code(which, kw, code):
    a = Args()
    assert getattr(_lib(), FUNCS[which])(*getattr(a, which)(**kw)) == code


def test_l1_cost_is_fine_for_obmc_beyond_2_taps_orig():
    """obmc_check_better prices with mv_err_cost_, which takes any cost type:
    only the refusal's other causes remain (here a NULL wsrc)."""
    a = Args()
    for t in (1, 2, 3):
        assert _lib().lavish_obmc_find_best_sub_pixel_tree_batch(
            *a.obmc(cost=(t,), stype=3, wsrc=False)) == -8


@pytest.mark.parametrize("which", sorted(FUNCS))
def test_no_jobs_is_a_no_op(which):
    a = Args()
    assert getattr(_lib(), FUNCS[which])(*getattr(a, which)(njobs=0)) == 0
    assert getattr(_lib(), FUNCS[which])(*getattr(a, which)(njobs=-3, w=12, h=12)) == 0


# ------------------------------------------------- the plain calls' rejects --
class PlainArgs(Args):
    """Argument lists of the four single-reference calls (as Args: NULL or a
    valid host buffer; they all return before any device work)."""

    def _pre(self, w, h, fullpel):
        p = self.p
        return [p, 64, p, 64, w, h, p] + ([] if fullpel is None else [p if fullpel else None])

    def ex(self, w=16, h=16, njobs=1, method=2, stype=0, fstop=0, hp=1, iters=1, cost="ok",
           fullpel=True):
        return self._pre(w, h, fullpel) + [njobs, method, stype, fstop, hp, iters,
                                           self._cost(cost), None, self.p, None]

    def tree(self, w=16, h=16, njobs=1, method=2, fstop=0, hp=1, iters=1, cost="ok",
             fullpel=True):
        return self._pre(w, h, fullpel) + [njobs, method, fstop, hp, iters, self._cost(cost),
                                           None, self.p, None]

    def l1(self, w=16, h=16, njobs=1, fstop=0, hp=1, iters=1, ctype=X.L1, fullpel=None):
        return self._pre(w, h, fullpel) + [njobs, fstop, hp, iters, ctype, self.p, None]

    def l1fp(self, fullpel=True, **kw):
        return self.l1(fullpel=fullpel, **kw)


PLAIN_FUNCS = dict(ex="lavish_find_best_sub_pixel_tree_batch_ex",
                   tree="lavish_find_best_sub_pixel_tree_batch",
                   l1="lavish_subpel_search_batch", l1fp="lavish_subpel_search_after_diamond")
COSTLY = ("ex", "tree")        # the calls that take a LavishMvCostParams
BAD = dict(w=12, h=12)         # a bad size: the last refusal of all
PLAIN_REJECTS = (
    # one fault each
    [("ex", dict(stype=v), -7) for v in (-1, 4)] +
    [(f, dict(fstop=v), -1) for f in PLAIN_FUNCS for v in (-1, 4)] +
    [(f, dict(cost=c), -2) for f in COSTLY for c in BAD_COSTS] +
    [(f, dict(ctype=v), -2) for f in ("l1", "l1fp") for v in (0, -1, 5)] +
    [(f, dict(iters=v), -4) for f in PLAIN_FUNCS for v in (0, 3, -1)] +
    [(f, dict(method=v), -6) for f in COSTLY for v in (-1, 3, 4)] +
    [(f, dict(w=w, h=h), -3) for f in PLAIN_FUNCS for w, h in BAD_SIZES] +
    [("l1fp", dict(fullpel=False), -5)] +
    # two faults: -7 before -1 before -2 before -4 before -6 before -3
    [("ex", dict(stype=4, fstop=4), -7), ("ex", dict(stype=-1, **BAD), -7)] +
    [(f, dict(fstop=4, cost=None), -1) for f in COSTLY] +
    [(f, dict(fstop=-1, ctype=0), -1) for f in ("l1", "l1fp")] +
    [(f, dict(cost=None, iters=0), -2) for f in COSTLY] +
    [(f, dict(cost=(X.ENTROPY, False), method=3), -2) for f in COSTLY] +
    [(f, dict(ctype=0, iters=3), -2) for f in ("l1", "l1fp")] +
    [(f, dict(ctype=0, **BAD), -2) for f in ("l1", "l1fp")] +
    [(f, dict(iters=3, method=3), -4) for f in COSTLY] +
    [(f, dict(iters=0, **BAD), -4) for f in PLAIN_FUNCS] +
    [(f, dict(method=-1, **BAD), -6) for f in COSTLY] +
    # _after_diamond looks at fullpel before anything else, the job count included
    [("l1fp", dict(fullpel=False, **kw), -5) for kw in (dict(fstop=4), dict(ctype=0), dict(iters=0),
                                                        BAD, dict(njobs=0), dict(njobs=-3))] +
    # no jobs: a no-op whatever else is wrong
    [(f, dict(njobs=n, fstop=4, iters=0, **BAD), 0) for f in PLAIN_FUNCS for n in (0, -3)] +
    [(f, dict(njobs=0, cost=None, method=3), 0) for f in COSTLY] +
    [("ex", dict(njobs=0, stype=4), 0)] +
    [(f, dict(njobs=0, ctype=0), 0) for f in ("l1", "l1fp")])


@pytest.mark.parametrize("which,kw,code", PLAIN_REJECTS, ids=lambda v: str(v).replace(" ", ""))
def test_plain_calls_refuse_bad_arguments_with_their_code(which, kw, code):
    """The single-reference calls' codes and their precedence: no jobs 0, then
    search type -7, forced_stop -1, cost -2 (the L1 calls: mv_cost_type 0 too),
    iters_per_step -4, method -6, size -3; lavish_subpel_search_after_diamond
    answers a NULL fullpel with -5 first of all."""
    a = PlainArgs()
    assert getattr(_lib(), PLAIN_FUNCS[which])(*getattr(a, which)(**kw)) == code


# ---------------------------------------------------------------- fixture --
@pytest.fixture(scope="module")
def F():
    return CS.load_fixture()


def test_restatement_equals_every_fixture_row(F):
    J = {n: i for i, n in enumerate(CS.ROW_FIELDS)}
    bad, n = [], 0
    for g in CS.fixture_groups(F):
        want = g.rows[:, J["best_row"]:J["sse"] + 1]
        got = CS.group_expected(F, g)
        n += len(want)
        if not np.array_equal(want, got):
            bad.append((g.index, g.prm, want.tolist(), got.tolist()))
    assert n == len(F["rows"]) and not bad, bad[:3]


def test_restatement_equals_the_oracle_on_the_plain_form():
    """With no second_pred the walk is the single-reference one the CPU oracle
    (orc_subpel_search_batch_ex) already pins to the reference: the jobs of
    fix_subpel_up.npz (SUBPEL_TREE, USE_2_TAPS / 4 / 8) and of fix_subpel.npz
    (the three methods, USE_2_TAPS_ORIG, no cost list), blocks up to 32x32."""
    import _oracle as O
    from _mcomp_fix import subpel_groups
    from lavish_dsp import motion as M
    mc = dict(np.load(os.path.join(GOLD, "fix_mcomp.npz")))
    stride = mc["src"].shape[1]
    src, ref = mc["src"].reshape(-1), mc["refs"].reshape(-1)
    n, seen = 0, set()
    for fix in ("fix_subpel_up.npz", "fix_subpel.npz"):
        Fp = dict(np.load(os.path.join(GOLD, fix)))
        for case, bw, bh, epb, rec, _, rows, _J in subpel_groups(Fp, mc):
            if bw * bh > 32 * 32:
                continue
            if fix == "fix_subpel_up.npz":
                (stype, hp, fstop, iters, ctype), meth = (int(v) for v in case), 0
            else:
                (meth, hp, fstop, iters, ctype, _cl), stype = (int(v) for v in case), 0
            tab = "hp" if hp else "lp"
            res = O.subpel_search_batch(mc["src"], mc["refs"], stride, bw, bh, rec, meth, fstop,
                                        bool(hp), iters, ctype, epb, mc["mvjcost_" + tab],
                                        mc["mvcost_" + tab], None, search_type=stype)
            cost = S.Cost(ctype, epb, 0, mc["mvjcost_" + tab], mc["mvcost_" + tab])
            cj = M.comp_subpel_jobs(rec.astype(M.SUBPEL_JOB_DTYPE), 0)
            got = CS.run_batch(CS.PLAIN, src, ref, stride, bw, bh, cj, cost, meth, stype, fstop,
                               bool(hp), iters)
            want = np.stack([res[f].astype(np.int64) for f in CS.RESULT_FIELDS], 1)
            np.testing.assert_array_equal(got, want, err_msg="%s %s %dx%d" % (
                fix, list(case), bw, bh))
            n += len(rec)
            seen.add((meth, stype))
    assert n > 100 and seen >= {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0)}


def test_fixture_covers_what_it_should(F):
    groups = list(CS.fixture_groups(F))
    forms = {(g.prm["form"], int(v)) for g in groups for v in g.cjobs["invert_mask"]}
    assert forms == {(CS.AVG, 0), (CS.MASK, 0), (CS.MASK, 1), (CS.OBMC, 0)}
    comp = [g for g in groups if g.prm["form"] != CS.OBMC]
    for form in (CS.AVG, CS.MASK):
        assert {g.prm["method"] for g in comp if g.prm["form"] == form} == {0, 1, 2}
    for sel in (comp, [g for g in groups if g.prm["form"] == CS.OBMC]):
        assert {g.prm["search_type"] for g in sel} == {0, 1, 2, 3}
        assert {g.prm["allow_hp"] for g in sel} == {0, 1}
        assert {g.prm["forced_stop"] for g in sel} == {0, 1, 2, 3}
        assert {g.prm["iters"] for g in sel} == {1, 2}
        assert {g.prm["cost"] for g in sel} == {X.ENTROPY, X.L1, X.NONE}
        assert {(g.prm["bw"], g.prm["bh"]) for g in sel} >= {(4, 4), (8, 8), (16, 8), (16, 16),
                                                              (32, 32)}
    for form in (CS.AVG, CS.MASK, CS.OBMC):
        assert any((g.prm["bw"], g.prm["bh"]) == (32, 32) for g in groups if g.prm["form"] == form)
    # the reference asserts on an L1 cost under estimate_obmc_mvcost
    assert not [g for g in groups if g.prm["form"] == CS.OBMC and g.prm["search_type"] == 0 and
                g.prm["cost"] == X.L1]
    assert all(g.prm["mask_stride"] > g.prm["bw"] for g in groups
               if g.prm["form"] == CS.MASK and g.plane.startswith("smooth"))
    # the chain: starts that are fix_mcomp_comp.npz's best and second-best mvs
    MC = S.load_fixture()
    JM = {n: i for i, n in enumerate(S.ROW_FIELDS)}
    J = {n: i for i, n in enumerate(CS.ROW_FIELDS)}
    best = {(int(r[JM["src_off"]]), int(r[JM["ref_off"]]), int(r[JM["second_off"]]),
             8 * int(r[JM["best_row"]]), 8 * int(r[JM["best_col"]])) for r in MC["rows"]}
    second = {(int(r[JM["src_off"]]), int(r[JM["ref_off"]]), int(r[JM["second_off"]]),
               8 * int(r[JM["second_row"]]), 8 * int(r[JM["second_col"]])) for r in MC["rows"]
              if r[JM["second_row"]] != S.INVALID} - best
    mine = {(int(r[J["src_off"]]), int(r[J["ref_off"]]), int(r[J["second_off"]]),
             int(r[J["start_row"]]), int(r[J["start_col"]])) for r in F["rows"]}
    assert len(mine & best) >= 20 and len(mine & second) >= 5
    assert os.path.getsize(os.path.join(GOLD, "fix_subpel_comp.npz")) < (1 << 19)


def test_fixture_moves(F):
    """The generator's own conditions on the committed file: per form a third
    of the rows end away from their start, rows end at half, quarter and
    eighth pel, second_level_check_v2 (or its OBMC twin) ran, a candidate lay
    outside the limits; and OBMC USE_2_TAPS_ORIG rows from a nonzero start
    whose centre error at mv (0, 0) differs from the start's, which in some
    changes the final mv."""
    facts = CS.check_coverage(F)      # (asserts each condition)
    assert set(facts) == {CS.AVG, CS.MASK, CS.OBMC, "obmc_centre"}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_fixture_sample_rederived_from_the_reference_text(F):
    """The first row of one small case per form and error kind (bilinear /
    upsampled), re-executed from the C text."""
    sys.path.insert(0, GOLD)
    import gen_fix_subpel_comp as G
    from gen_fixtures import nmv_cost_tables
    R = G.CompSubpelRef(nmv_cost_tables(), X.STRIDE, X.W, X.H, X.BORDER)
    J = {n: i for i, n in enumerate(CS.ROW_FIELDS)}
    done = set()
    for g in CS.fixture_groups(F):
        p = g.prm
        cj = g.cjobs[0]
        key = (p["form"], int(cj["invert_mask"]), p["search_type"] >= 2 and p["method"] == 0)
        if key in done or p["bw"] * p["bh"] > 64 or p["forced_stop"] == CS.FULL_PEL:
            continue
        R.set_planes(F["src__" + g.plane], F["refs__" + g.plane])
        n = p["bw"] * p["bh"]
        jb = cj["base"]
        so, mo = int(cj["second_off"]), int(cj["mask_off"])
        k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
        if p["form"] == CS.OBMC:
            kw = dict(wsrc=F["wsrc"][so:so + n], omask=F["omask"][mo:mo + n])
        else:
            kw = dict(second=F["second"][so:so + n])
            if p["form"] == CS.MASK:
                kw.update(mask=F["mask"][mo:mo + p["bh"] * p["mask_stride"]],
                          invert=int(cj["invert_mask"]))
        got = R.run(p, jb, k, **kw)
        assert got == g.rows[0, J["best_row"]:J["sse"] + 1].tolist(), (g.index, p)
        done.add(key)
    assert {k[:2] for k in done} == {(CS.AVG, 0), (CS.MASK, 0), (CS.MASK, 1), (CS.OBMC, 0)}
    assert {k[2] for k in done} == {False, True}


# ---------------------------------------------------------------- kernels --
def _resources():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler") or \
            shutil.which("c++filt") is None:
        pytest.skip("ROCm code-object tools not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    res = KR.kernel_resources(os.path.join(ROOT, "aom-av1-lavish_amd", "liblavish_hip.so"))
    names = sorted(res)
    return [(d, res[n]) for n, d in zip(names, KR.demangled(names))]


def test_new_kernels_resources():
    """comp_subpel_kernel<W, H, FORM, UP>: 22 block sizes x 3 forms x the two
    errors.  The bilinear instantiations use no scratch and spill nothing; an
    upsampled one uses no more scratch than subpel_kernel<W, H> of the same
    size in the same library."""
    res = _resources()
    plain = {}
    for d, v in res:
        m = re.search(r"\bsubpel_kernel<(\d+), (\d+)>", d)
        if m:
            plain[(int(m.group(1)), int(m.group(2)))] = v.get("private_segment_fixed_size", 0)
    assert len(plain) == 22
    mine = []
    for d, v in res:
        m = re.search(r"comp_subpel_kernel<(\d+), (\d+), (\d+), (true|false)>", d)
        if m:
            mine.append(((int(m.group(1)), int(m.group(2))), int(m.group(3)),
                         m.group(4) == "true", v))
    assert len(mine) == 22 * 3 * 2, len(mine)
    for size, form, up, v in mine:
        scratch = v.get("private_segment_fixed_size", 0)
        if up:
            assert scratch <= plain[size], (size, form, v)
        else:
            assert scratch == 0, (size, form, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, \
                (size, form, v)
