"""CPU tests of the compound / masked / OBMC full-pel search layer (no GPU):
* include/lavish_dsp.h declares, and the library exports, the three batch
  calls; the record sizes match ctypes and the numpy dtypes;
* every argument the calls refuse is refused with a negative return before
  any device work (the pointers are host buffers or garbage);
* tests/_compsearch_ref.py equals every row of tests/golden/fix_mcomp_comp.npz
  (the reference's own results), every field;
* the fixture covers what it should;
* a sample of the fixture re-derived from the reference's C text (skipped
  where the reference sources are absent);
* every kernel of csrc/mcomp_comp.hip in the built library runs without
  scratch or spilled VGPRs."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _compsearch_ref as S
import _mvextremes as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "lavish_dsp.h")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")
CALLS = ["lavish_comp_full_pixel_search_batch", "lavish_refining_search_8p_batch",
         "lavish_obmc_full_pixel_search_batch"]


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
           '_Static_assert(sizeof(LavishCompSearchJob) == 56, "job record");\n'
           '_Static_assert(sizeof(LavishCompSearchResult) == 16, "result record");\n'
           '_Static_assert(__builtin_offsetof(LavishCompSearchJob, second_off) == 32, "");\n'
           '_Static_assert(__builtin_offsetof(LavishCompSearchJob, invert_mask) == 48, "");\n'
           '_Static_assert(__builtin_offsetof(LavishCompSearchResult, bestsme) == 8, "");\n')
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

    class Result(ctypes.Structure):
        _fields_ = [(n, ctypes.c_int16) for n in S.RESULT_FIELDS[:4]] + \
                   [("bestsme", ctypes.c_int32), ("steps", ctypes.c_int32)]

    assert ctypes.sizeof(Job) == M.COMP_JOB_DTYPE.itemsize == 56
    assert ctypes.sizeof(Result) == M.COMP_RESULT_DTYPE.itemsize == 16
    assert Job.second_off.offset == M.COMP_JOB_DTYPE.fields["second_off"][1] == 32
    assert Job.invert_mask.offset == M.COMP_JOB_DTYPE.fields["invert_mask"][1] == 48
    assert Result.bestsme.offset == M.COMP_RESULT_DTYPE.fields["bestsme"][1] == 8
    j = M.comp_jobs(np.zeros(3, M.JOB_DTYPE), [5, 6, 7], 9, [0, 1, 0])
    assert j["second_off"].tolist() == [5, 6, 7] and j["mask_off"].tolist() == [9, 9, 9]
    assert j["invert_mask"].tolist() == [0, 1, 0] and j.dtype == M.COMP_JOB_DTYPE


# ---------------------------------------------------------------- rejects --
_vp = ctypes.c_void_p
GARBAGE = _vp(0xDEAD0000)      # never dereferenced: the calls return first


class Args:
    """Argument lists of the three calls; every pointer is garbage or a host
    buffer, so a call that started device work would fault or report."""

    def __init__(self):
        from lavish_dsp import motion as M
        self.M = M
        self.tab = np.zeros(8, np.int32)
        self.tp = self.tab.__array_interface__["data"][0]

    def cost(self, ctype=X.L1, tables=True):
        c = self.M.MvCostParams(ctype, 4, 37, 0)
        if tables:
            c.mvjcost, c.mvcost[0], c.mvcost[1] = self.tp, self.tp, self.tp
        return c

    def comp(self, w=16, h=16, njobs=1, method=0, step_param=5, cost="ok", second=True,
             mask=True, ms=None, src=True, out=True):
        p = GARBAGE
        c = None if cost is None else ctypes.byref(self.cost(*(() if cost == "ok" else cost)))
        return [p if src else None, 64, p, 64, w, h, p, njobs, method, step_param, c,
                p if second else None, p if mask else None, w if ms is None else ms,
                p if out else None, None]

    def refine(self, w=16, h=16, njobs=1, cost="ok", second=True, mask=True, ms=None, src=True,
               out=True, method=None, step_param=None):
        p = GARBAGE
        c = None if cost is None else ctypes.byref(self.cost(*(() if cost == "ok" else cost)))
        return [p if src else None, 64, p, 64, w, h, p, njobs, c, p if second else None,
                p if mask else None, w if ms is None else ms, p if out else None, None]

    def obmc(self, w=16, h=16, njobs=1, method=0, step_param=5, cost="ok", fast=0, wsrc=True,
             mask=True, out=True):
        p = GARBAGE
        c = None if cost is None else ctypes.byref(self.cost(*(() if cost == "ok" else cost)))
        return [p, 64, w, h, p, njobs, method, step_param, c, fast, p if wsrc else None,
                p if mask else None, p if out else None, None]


BAD_SIZES = [(12, 12), (4, 32), (32, 4), (256, 256), (0, 0), (8, 64), (16, 15)]
BAD_METHODS = [-1, 3, 4, 5, 6, 7, 8, 9, 10, 11]     # CLAMPED_DIAMOND and the pattern methods
BAD_COSTS = [None, (-1,), (5,), (X.ENTROPY, False)]
REJECTS = (
    [(f, dict(w=w, h=h, ms=300)) for f in ("comp", "refine") for w, h in BAD_SIZES] +
    [("obmc", dict(w=w, h=h)) for w, h in BAD_SIZES] +
    [(f, dict(method=m)) for f in ("comp", "obmc") for m in BAD_METHODS] +
    [(f, dict(method=m, step_param=s)) for f in ("comp", "obmc")
     for m, s in ((0, -1), (0, 11), (1, 15), (2, 16), (0, 1 << 20))] +
    [("obmc", dict(method=m, step_param=s, fast=1)) for m, s in ((3, 0), (0, 11))] +
    [(f, dict(cost=c)) for f in ("comp", "refine", "obmc") for c in BAD_COSTS] +
    [("comp", dict(second=False)), ("comp", dict(second=False, mask=False)),
     ("comp", dict(ms=15)), ("comp", dict(w=128, h=128, ms=127)), ("comp", dict(src=False)),
     ("comp", dict(out=False)),
     ("refine", dict(second=False)),            # a mask with nothing to blend
     ("refine", dict(ms=15)), ("refine", dict(src=False)), ("refine", dict(out=False)),
     ("obmc", dict(wsrc=False)), ("obmc", dict(mask=False)), ("obmc", dict(out=False)),
     ("obmc", dict(wsrc=False, fast=1))])
FUNCS = dict(zip(("comp", "refine", "obmc"), CALLS))


def _lib():
    import lavish_dsp
    import lavish_dsp.motion  # noqa: F401  (sets the argtypes)
    return lavish_dsp.lib()


@pytest.mark.parametrize("which,kw", REJECTS, ids=lambda v: str(v).replace(" ", ""))
def test_bad_arguments_are_refused_before_any_device_work(which, kw):
    a = Args()
    assert getattr(_lib(), FUNCS[which])(*getattr(a, which)(**kw)) < 0


@pytest.mark.parametrize("which", sorted(FUNCS))
def test_no_jobs_is_a_no_op(which):
    a = Args()
    assert getattr(_lib(), FUNCS[which])(*getattr(a, which)(njobs=0)) == 0
    assert getattr(_lib(), FUNCS[which])(*getattr(a, which)(njobs=-3, w=12, h=12)) == 0


# ---------------------------------------------------------------- fixture --
@pytest.fixture(scope="module")
def F():
    return S.load_fixture()


def test_site_tables_from_the_radii():
    d = S.site_table(S.DIAMOND)
    assert [r for r, _ in d] == [1 << k for k in range(11)] and all(len(s) == 8 for _, s in d)
    n = S.site_table(S.NSTEP)
    assert [r for r, _ in n] == [1, 2, 3, 5, 8, 12, 18, 27, 41, 62, 93, 140, 210, 210, 210]
    assert [len(s) for _, s in n] == [8] * 4 + [12] * 11
    assert n[4][1][4:8] == [(-8, -3), (8, 3), (-3, 8), (3, -8)]      # tangent (int)(0.41 * 8)
    n8 = S.site_table(S.NSTEP_8PT)
    assert len(n8) == 16 and all(len(s) == 8 for _, s in n8) and n8[5][1][4] == (-12, -12)


def test_restatement_equals_every_fixture_row(F):
    J = {n: i for i, n in enumerate(S.ROW_FIELDS)}
    bad, n = [], 0
    for g in S.fixture_groups(F):
        want = g.rows[:, J["best_row"]:J["steps"] + 1]
        got = S.group_expected(F, g)
        n += len(want)
        if not np.array_equal(want, got):
            bad.append((g.index, g.prm, want.tolist(), got.tolist()))
    assert n == len(F["rows"]) and not bad, bad[:3]


def test_fixture_covers_what_it_should(F):
    groups = list(S.fixture_groups(F))
    J = {n: i for i, n in enumerate(S.ROW_FIELDS)}
    key = lambda g: (g.prm["search"], g.prm["form"])
    assert {key(g) for g in groups} >= {(S.COMP, S.AVG), (S.COMP, S.MASK), (S.REFINE8, S.PLAIN),
                                        (S.REFINE8, S.AVG), (S.REFINE8, S.MASK),
                                        (S.OBMC, S.PLAIN)}
    comp = [g for g in groups if g.prm["search"] == S.COMP]
    for form in (S.AVG, S.MASK):
        assert {(g.prm["method"], g.kind) for g in comp if g.prm["form"] == form} >= {
            (m, k) for m in range(3) for k in ("flat_128_128", "ramp_x", "periodic_2", "noise")}
    assert {int(v) for g in comp for v in g.cjobs["invert_mask"]} == {0, 1}
    assert {(g.prm["bw"], g.prm["bh"]) for g in groups} == {(4, 4), (8, 8), (16, 8), (16, 16)}
    for m in range(3):
        assert {g.prm["step_param"] for g in comp if g.prm["method"] == m} >= {
            0, 5, S.num_steps(m) - 1}
    assert {g.prm["cost"] for g in groups} == {X.ENTROPY, X.L1, X.NONE}
    assert any(g.prm["error_per_bit"] == X.HIGH_LAMBDA[1][0] for g in groups)
    assert any(g.prm["mask_stride"] > g.prm["bw"] for g in comp if g.prm["form"] == S.MASK)
    obmc = [g for g in groups if g.prm["search"] == S.OBMC]
    assert {(g.prm["method"], g.prm["fast_obmc"]) for g in obmc} >= {(0, 0), (1, 0), (2, 0),
                                                                      (0, 1)}
    # windows of one point / row / column, and starts outside the window
    b = np.concatenate([g.cjobs["base"] for g in groups])
    assert ((b["row_min"] == b["row_max"]) & (b["col_min"] == b["col_max"])).any()
    assert ((b["row_min"] == b["row_max"]) & (b["col_min"] < b["col_max"])).any()
    assert ((b["row_min"] < b["row_max"]) & (b["col_min"] == b["col_max"])).any()
    assert ((b["start_row"] > b["row_max"]) & (b["start_col"] < b["col_min"])).any()
    # the searches move, and second_best_mv is both invalid and set
    rows = F["rows"]
    moved = (rows[:, J["best_row"]] != np.clip(rows[:, J["start_row"]], rows[:, J["row_min"]],
                                               rows[:, J["row_max"]]))
    assert moved.sum() > len(rows) // 5
    crow = np.isin(rows[:, 0], [g.index for g in comp])
    assert (rows[crow, J["second_row"]] == S.INVALID).any()
    assert (rows[crow, J["second_row"]] != S.INVALID).any()
    # the average form's exact matches (second_pred = 2 * src - ref at a target
    # column): found off the start, variance and mv cost 0
    ex = [g for g in comp if g.kind == "ramp_x" and g.prm["cost"] == X.NONE and len(g.rows) == 1]
    assert len(ex) == 3 and {g.prm["method"] for g in ex} == {0, 1, 2}
    for g in ex:
        assert g.rows[0, J["bestsme"]] == 0 and -8 <= g.rows[0, J["best_col"]] <= -6
        assert g.rows[0, J["start_col"]] == 0
    # the 8-point refinement: walks of 0, 1 and 3 moves, a diagonal among them
    r8 = np.isin(rows[:, 0], [g.index for g in groups if g.prm["search"] == S.REFINE8])
    dr = rows[r8, J["best_row"]] - np.clip(rows[r8, J["start_row"]], rows[r8, J["row_min"]],
                                           rows[r8, J["row_max"]])
    dc = rows[r8, J["best_col"]] - np.clip(rows[r8, J["start_col"]], rows[r8, J["col_min"]],
                                           rows[r8, J["col_max"]])
    far = np.maximum(np.abs(dr), np.abs(dc))
    assert {0, 1, 3} <= set(far.tolist()) and ((np.abs(dr) == 3) & (np.abs(dc) == 3)).any()
    # the largest SAD: 255 on every pixel of a 16x16 block
    assert (rows[r8, J["bestsme"]] >= 255 * 256).any()
    assert os.path.getsize(os.path.join(GOLD, "fix_mcomp_comp.npz")) < (1 << 19)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_fixture_sample_rederived_from_the_reference_text(F):
    """The first row of one small case per search and form, re-executed from
    the C text."""
    sys.path.insert(0, GOLD)
    import gen_fix_mcomp_comp as G
    from gen_fixtures import nmv_cost_tables
    R = G.CompRef(nmv_cost_tables(), X.STRIDE, X.W, X.H, X.BORDER)
    J = {n: i for i, n in enumerate(S.ROW_FIELDS)}
    done = set()
    for g in S.fixture_groups(F):
        p = g.prm
        key = (p["search"], p["form"], p["fast_obmc"])
        if key in done or p["bw"] * p["bh"] > 64 or p["step_param"] < 5 and p["search"] != S.REFINE8:
            continue
        R.set_planes(F["src__" + g.kind], F["refs__" + g.kind])
        cj, n = g.cjobs[0], p["bw"] * p["bh"]
        jb = cj["base"]
        so, mo = int(cj["second_off"]), int(cj["mask_off"])
        k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
        kw = {}
        if p["search"] == S.OBMC:
            kw = dict(wsrc=F["wsrc"][so:so + n], omask=F["omask"][mo:mo + n],
                      fast=p["fast_obmc"])
        else:
            if p["form"] != S.PLAIN:
                kw["second"] = F["second"][so:so + n]
            if p["form"] == S.MASK:
                kw.update(mask=F["mask"][mo:mo + p["bh"] * p["mask_stride"]],
                          mask_stride=p["mask_stride"], invert=int(cj["invert_mask"]))
        ms = R.params(p["bw"], p["bh"], G.METHODS[p["method"]], G.COST_NAMES[p["cost"]],
                      int(jb["src_off"]), k, int(jb["ref_off"]) - k * X.PLANE,
                      (int(jb["ref_mv_row"]), int(jb["ref_mv_col"])),
                      [int(jb[f]) for f in ("col_min", "col_max", "row_min", "row_max")],
                      p["error_per_bit"], p["sad_per_bit"], p["hp_tables"], **kw)
        got = R.run(p["search"], ms, (int(jb["start_row"]), int(jb["start_col"])),
                    p["step_param"])
        assert got == g.rows[0, J["best_row"]:J["bestsme"] + 1].tolist(), (g.index, p)
        done.add(key)
    assert {k[:2] for k in done} >= {(S.COMP, S.AVG), (S.COMP, S.MASK), (S.REFINE8, S.PLAIN),
                                     (S.REFINE8, S.AVG), (S.REFINE8, S.MASK), (S.OBMC, S.PLAIN)}
    assert {k[2] for k in done if k[0] == S.OBMC} == {0, 1}


# ---------------------------------------------------------------- kernels --
def test_new_kernels_use_no_scratch():
    """Code-object metadata (tools/kernel_resources.py) of every comp_kernel
    instantiation: 22 block sizes x 4 forms, no scratch, no spilled VGPR."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler") or \
            shutil.which("c++filt") is None:
        pytest.skip("ROCm code-object tools not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    res = KR.kernel_resources(os.path.join(ROOT, "aom-av1-lavish_amd", "liblavish_hip.so"))
    names = sorted(res)
    mine = [(d, res[n]) for n, d in zip(names, KR.demangled(names)) if "comp_kernel<" in d]
    assert len(mine) == 22 * 4, len(mine)
    for name, v in mine:
        assert v.get("private_segment_fixed_size", 0) == 0, (name, v)
        assert v.get("vgpr_spill_count", 0) == 0, (name, v)
