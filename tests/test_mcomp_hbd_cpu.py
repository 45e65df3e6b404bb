"""CPU tests of the high-bit-depth full-pel / sub-pel search layer (no GPU):
* include/lavish_dsp.h declares, and the library exports, the two batch calls;
* every argument the calls refuse is refused with its return code before any
  device work (the pointers are garbage);
* tests/_hbdsearch_ref.py equals every row of tests/golden/fix_mcomp_hbd.npz
  (the reference's own results), every field, full-pel and sub-pel;
* the fixture covers what it should (the checks its generator stops on);
* a sample of the fixture re-derived from the reference's C text (skipped
  where the reference sources are absent);
* every kernel of csrc/mcomp_hbd.hip and csrc/subpel_hbd.hip in the built
  library runs without scratch or spilled VGPRs."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _hbdsearch_ref as H
import _mvextremes as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "lavish_dsp.h")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")
FULL, SUB = ("lavish_highbd_full_pixel_search_batch",
             "lavish_highbd_find_best_sub_pixel_tree_batch")


def _lib():
    import lavish_dsp
    import lavish_dsp.motion  # noqa: F401  (sets the argtypes)
    return lavish_dsp.lib()


def test_header_declares_and_library_exports_the_calls():
    out = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True, capture_output=True,
                         text=True).stdout
    declared = set(re.findall(r"\b(lavish_\w+)\s*\(", out))
    assert FULL in declared and SUB in declared
    L = _lib()
    assert hasattr(L, FULL) and hasattr(L, SUB)
    from lavish_dsp import motion as M
    assert callable(M.highbd_full_pixel_search_batch)
    assert callable(M.highbd_find_best_sub_pixel_tree_batch)


# ---------------------------------------------------------------- rejects --
_vp = ctypes.c_void_p
GARBAGE = _vp(0xDEAD0000)      # never dereferenced: the calls return first


def _cost(ctype=X.L1, tables=True):
    from lavish_dsp import motion as M
    c = M.MvCostParams(ctype, 4, 37, 0)
    if tables:
        c.mvjcost = c.mvcost[0] = c.mvcost[1] = 0xDEAD0000
    return c


def full_args(w=16, h=16, bd=10, njobs=1, method=1, step_param=5, cost="ok", src=True, ref=True,
              jobs=True, out=True):
    p = GARBAGE
    c = None if cost is None else ctypes.byref(_cost(*(() if cost == "ok" else cost)))
    return [p if src else None, 64, p if ref else None, 64, w, h, bd, p if jobs else None, njobs,
            method, step_param, c, 0, p if out else None, None, None]


def sub_args(w=16, h=16, bd=10, njobs=1, method=2, forced_stop=0, iters=1, cost="ok", src=True,
             ref=True, jobs=True, out=True):
    p = GARBAGE
    c = None if cost is None else ctypes.byref(_cost(*(() if cost == "ok" else cost)))
    return [p if src else None, 64, p if ref else None, 64, w, h, bd, p if jobs else None, None,
            njobs, method, forced_stop, 1, iters, c, None, p if out else None, None]


BAD_SIZES = [(12, 12), (4, 32), (32, 4), (256, 256), (0, 0), (8, 64), (16, 15)]
BAD_COSTS = [None, (-1,), (5,), (X.ENTROPY, False)]
FULL_REJECTS = (
    [(dict(w=w, h=h), -3) for w, h in BAD_SIZES] +
    [(dict(bd=b), -7) for b in (9, 0, 7, 11, 13, 16, -8)] +
    [(dict(**{k: False}), -7) for k in ("src", "ref", "jobs", "out")] +
    # CLAMPED_DIAMOND and the pattern methods
    [(dict(method=m), -4) for m in (-1, 3, 4, 5, 6, 7, 8, 9, 10, 11)] +
    [(dict(method=m, step_param=s), -1)
     for m, s in ((0, -1), (0, 11), (1, 15), (2, 16), (0, 1 << 20))] +
    [(dict(cost=c), -2) for c in BAD_COSTS] +
    # the order: pointers and depth, method, step_param, cost, size
    [(dict(bd=9, method=5, step_param=99, cost=None, w=12), -7),
     (dict(method=5, step_param=99, cost=None, w=12), -4),
     (dict(step_param=99, cost=None, w=12), -1), (dict(cost=None, w=12), -2)])
SUB_REJECTS = (
    [(dict(w=w, h=h), -3) for w, h in BAD_SIZES] +
    [(dict(bd=b), -7) for b in (9, 0, 7, 11, 13, 16, -8)] +
    [(dict(**{k: False}), -7) for k in ("src", "ref", "jobs", "out")] +
    [(dict(forced_stop=f), -1) for f in (-1, 4)] +
    [(dict(cost=c), -2) for c in BAD_COSTS] +
    [(dict(iters=i), -4) for i in (0, 3)] +
    [(dict(method=m), -6) for m in (-1, 3)])


@pytest.mark.parametrize("kw,rc", FULL_REJECTS, ids=lambda v: str(v).replace(" ", ""))
def test_full_pel_refuses_bad_arguments_before_any_device_work(kw, rc):
    assert getattr(_lib(), FULL)(*full_args(**kw)) == rc


@pytest.mark.parametrize("kw,rc", SUB_REJECTS, ids=lambda v: str(v).replace(" ", ""))
def test_sub_pel_refuses_bad_arguments_before_any_device_work(kw, rc):
    assert getattr(_lib(), SUB)(*sub_args(**kw)) == rc


def test_no_jobs_is_a_no_op():
    L = _lib()
    for n in (0, -3):
        assert getattr(L, FULL)(*full_args(njobs=n, w=12, bd=9, method=5, cost=None)) == 0
        assert getattr(L, SUB)(*sub_args(njobs=n, w=12, bd=9, method=5, cost=None)) == 0


# ---------------------------------------------------------------- fixture --
@pytest.fixture(scope="module")
def F():
    return H.load_fixture()


def test_full_pel_restatement_equals_every_fixture_row(F):
    bad, n = [], 0
    for g in H.fixture_groups(F):
        J = g.J
        got, cl = H.group_fullpel(F, g)
        want = g.rows[:, J["best_row"]:J["searches"] + 1]
        n += len(want)
        if not np.array_equal(want, got):
            bad.append((g.index, g.prm, want.tolist(), got.tolist()))
        wcl = g.rows[:, J["cl0"]:J["cl4"] + 1]
        if g.prm["use_cl"]:
            if not np.array_equal(wcl, cl):
                bad.append((g.index, g.prm, wcl.tolist(), cl.tolist()))
        else:
            assert (wcl == H.INT_MAX).all()
    assert n == len(F["rows"]) and not bad, bad[:3]


def test_sub_pel_restatement_equals_every_fixture_row(F):
    bad, n = [], 0
    for g in H.fixture_groups(F):
        J = g.J
        got = H.group_subpel(F, g)
        want = g.rows[:, J["sp_best_row"]:J["sp_sse"] + 1]
        n += len(want)
        if not np.array_equal(want, got):
            bad.append((g.index, g.prm, want.tolist(), got.tolist()))
    assert n == len(F["rows"]) and not bad, bad[:3]


def test_fixture_covers_what_it_should(F):
    full, sub = H.check_coverage(F)     # (asserts every item; the counts for the record)
    assert full["per_row_differs"] and full["skip_kept"] and full["skip_redo"]
    assert full["sum_negative"] and full["clamped"] and full["max_vs_zero"]
    assert 3 * sub["moved"] >= sub["rows"]
    groups = list(H.fixture_groups(F))
    assert {(g.prm["bw"], g.prm["bh"]) for g in groups} == {(4, 4), (8, 8), (16, 8), (16, 16),
                                                           (32, 32)}
    assert sum(len(g.rows) for g in groups if g.prm["bw"] == 32) == 1
    sp = [g.prm["step_param"] for g in groups for _ in g.rows]
    assert 2 * sum(s >= 5 for s in sp) > len(sp)
    assert {g.prm["sp_method"] for g in groups} == {H.TREE, H.PRUNED, H.PRUNED_MORE}
    assert {g.prm["sp_forced_stop"] for g in groups} >= {0, 1, 2}
    assert {g.prm["sp_iters"] for g in groups} == {1, 2}
    assert {g.prm["sp_allow_hp"] for g in groups} == {0, 1}
    assert any(g.prm["error_per_bit"] == X.HIGH_LAMBDA[1][0] for g in groups)
    b = np.concatenate([g.jobs for g in groups])
    assert ((b["row_min"] == b["row_max"]) & (b["col_min"] < b["col_max"])).any()
    assert ((b["row_min"] < b["row_max"]) & (b["col_min"] == b["col_max"])).any()
    assert ((b["start_row"] > b["row_max"]) & (b["start_col"] < b["col_min"])).any()
    # the low bd - 8 bits of the stored planes are in use
    for g in groups:
        sh = g.prm["bd"] - 8
        src, ref = H.group_planes(F, g)
        assert int(src.max()) < 1 << g.prm["bd"] and int(ref.max()) < 1 << g.prm["bd"]
        if sh and not g.plane.startswith("flat_0") and not g.plane.startswith("flat_255"):
            assert (src & ((1 << sh) - 1)).any() and (ref & ((1 << sh) - 1)).any(), g.plane
    assert os.path.getsize(os.path.join(GOLD, "fix_mcomp_hbd.npz")) < (1 << 18)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_fixture_sample_rederived_from_the_reference_text(F):
    """The first row of one small case per depth, re-executed from the C text
    (full-pel and sub-pel), and the wrappers are the reference's macro text."""
    sys.path.insert(0, GOLD)
    import gen_fix_mcomp_hbd as G
    from gen_fixtures import nmv_cost_tables
    text, found = G.wrapper_text([(8, 8), (16, 16)])
    assert ">> 2" in text and ">> 4" in text and "sad_array[i] >>= 4" in text
    assert "aom_highbd_sad16x16x4d" in found and "aom_highbd_sad_skip_16x16" in found
    R = G.HbdRef(nmv_cost_tables(), X.STRIDE, X.W, X.H, X.BORDER, [(8, 8), (16, 8), (16, 16)])
    done = set()
    for g in H.fixture_groups(F):
        p, J = g.prm, g.J
        if p["bd"] in done or p["bw"] * p["bh"] > 128 or p["step_param"] < 5:
            continue
        R.set_planes(F["src__" + g.plane], F["refs__" + g.plane])
        jb, row = g.jobs[0], g.rows[0]
        k = (int(jb["ref_off"]) - int(jb["src_off"])) // X.PLANE
        so, ro = int(jb["src_off"]), int(jb["ref_off"]) - k * X.PLANE
        ref_mv = (int(jb["ref_mv_row"]), int(jb["ref_mv_col"]))
        fp = R.fullpel(p["bw"], p["bh"], p["bd"], G.METHODS[p["method"]], p["use_cl"],
                       G.COST_NAMES[p["cost"]], p["skip"], p["step_param"], so, k, ro, ref_mv,
                       (int(jb["start_row"]), int(jb["start_col"])),
                       [int(jb[f]) for f in ("col_min", "col_max", "row_min", "row_max")],
                       p["error_per_bit"], p["sad_per_bit"], p["hp_tables"])
        assert fp[:3] == row[J["best_row"]:J["bestsme"] + 1].tolist(), (g.index, p)
        assert fp[3:] == row[J["cl0"]:J["cl4"] + 1].tolist(), (g.index, p)
        sp = R.subpel(p["bw"], p["bh"], p["bd"], p["sp_method"], p["sp_allow_hp"],
                      p["sp_forced_stop"], p["sp_iters"], G.COST_NAMES[p["cost"]],
                      fp[3:] if p["sp_use_cl"] else None, p["error_per_bit"], so, k, ro, ref_mv,
                      (8 * fp[0], 8 * fp[1]),
                      [int(row[J["sp_" + f]]) for f in ("col_min", "col_max", "row_min",
                                                        "row_max")])
        assert sp == row[J["sp_best_row"]:J["sp_sse"] + 1].tolist(), (g.index, p)
        done.add(p["bd"])
    assert done == {8, 10, 12}


# ---------------------------------------------------------------- kernels --
def test_new_kernels_use_no_scratch():
    """Code-object metadata (tools/kernel_resources.py) of every
    hbd_fullpel_kernel and hbd_subpel_kernel instantiation: 22 block sizes
    each, no scratch, no spilled VGPR, no LDS."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler") or \
            shutil.which("c++filt") is None:
        pytest.skip("ROCm code-object tools not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    res = KR.kernel_resources(os.path.join(ROOT, "aom-av1-lavish_amd", "liblavish_hip.so"))
    names = sorted(res)
    for kern in ("hbd_fullpel_kernel<", "hbd_subpel_kernel<"):
        mine = [(d, res[n]) for n, d in zip(names, KR.demangled(names)) if kern in d]
        assert len(mine) == 22, (kern, len(mine))
        for name, v in mine:
            assert v.get("private_segment_fixed_size", 0) == 0, (name, v)
            assert v.get("vgpr_spill_count", 0) == 0, (name, v)
            assert v.get("group_segment_fixed_size", 0) == 0, (name, v)
            assert v.get("vgpr_count", 0) <= 128, (name, v)
