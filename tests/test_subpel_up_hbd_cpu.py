"""CPU tests of the high-bit-depth upsampled sub-pel error (no GPU):
* include/lavish_dsp.h declares, and the library exports, the three _ex calls
  with subpel_search_type where the 8-bit calls have it;
* what the _ex calls refuse is refused with its return code before any device
  work (the pointers are garbage);
* tests/_hbdup_ref.py equals every row of tests/golden/fix_subpel_up_hbd.npz
  (the reference's own results), every field;
* the fixture covers what it should (the checks its generator stops on);
* a sample of the fixture re-derived from the reference's C text (skipped where
  the reference sources are absent);
* the 88 hbd_upsampled_kernel instantiations in the built library: no LDS, no
  spill count above the 8-bit twin's, scratch no larger than the 8-bit twin's
  (comp_subpel_kernel<W, H, FORM, true>; the plain form: subpel_kernel<W, H>)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _hbdup_ref as U
import _mvextremes as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "lavish_dsp.h")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")
PLAIN_EX, COMP_EX, OBMC_EX = CALLS = (
    "lavish_highbd_find_best_sub_pixel_tree_batch_ex",
    "lavish_highbd_comp_find_best_sub_pixel_tree_batch_ex",
    "lavish_highbd_obmc_find_best_sub_pixel_tree_batch_ex")
P = U.P


def _lib():
    import lavish_dsp
    import lavish_dsp.motion  # noqa: F401  (sets the argtypes)
    return lavish_dsp.lib()


def _params(proto):
    return [re.sub(r"\s+", " ", a).strip() for a in proto.split(",")]


def test_header_declares_the_ex_prototypes_and_library_exports_them():
    out = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True, capture_output=True,
                         text=True).stdout
    protos = dict(re.findall(r"\bint\s+(lavish_\w+)\s*\(([^)]*)\)\s*;", out))
    L = _lib()
    from lavish_dsp import motion as M
    for name in CALLS:
        assert name in protos, name
        assert hasattr(L, name), name
        fn = getattr(L, name)
        ex, old = _params(protos[name]), _params(protos[name[:-len("_ex")]])
        # the old prototype with `int subpel_search_type` put in, nothing else
        at = ex.index("int subpel_search_type")
        assert ex[:at] + ex[at + 1:] == old, name
        # after the method, or after njobs for OBMC: where the 8-bit calls have it
        assert ex[at - 1] == ("int njobs" if name == OBMC_EX else "int subpel_search_method")
        twin = _params(protos[{PLAIN_EX: "lavish_find_best_sub_pixel_tree_batch_ex",
                               COMP_EX: "lavish_comp_find_best_sub_pixel_tree_batch",
                               OBMC_EX: "lavish_obmc_find_best_sub_pixel_tree_batch"}[name]])
        assert twin[twin.index("int subpel_search_type") - 1] == ex[at - 1], name
        assert len(fn.argtypes) == len(ex) and fn.restype is ctypes.c_int32, name
    import inspect
    for f in (M.highbd_find_best_sub_pixel_tree_batch, M.highbd_comp_find_best_sub_pixel_tree_batch,
              M.highbd_obmc_find_best_sub_pixel_tree_batch):
        assert inspect.signature(f).parameters["search_type"].default == M.USE_2_TAPS_ORIG


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


def plain_args(w=16, h=16, bd=10, njobs=1, method=0, stype=3, forced_stop=0, iters=1, cost="ok",
               src=True, ref=True, jobs=True, out=True):
    return [_p(src), 64, _p(ref), 64, w, h, bd, _p(jobs), None, njobs, method, stype, forced_stop,
            1, iters, _c(cost), None, _p(out), None]


def comp_args(w=16, h=16, bd=10, njobs=1, method=0, stype=3, forced_stop=0, iters=1, cost="ok",
              src=True, ref=True, jobs=True, out=True, second=True, mask=False, mask_stride=16,
              fullpel=False, start_from=0):
    return [_p(src), 64, _p(ref), 64, w, h, bd, _p(jobs), _p(fullpel), start_from, njobs, method,
            stype, forced_stop, 1, iters, _c(cost), _p(second), _p(mask), mask_stride, _p(out),
            None]


def obmc_args(w=16, h=16, bd=10, njobs=1, stype=3, forced_stop=0, iters=1, cost="ok", ref=True,
              jobs=True, out=True, wsrc=True, omask=True):
    return [_p(ref), 64, w, h, bd, _p(jobs), None, njobs, stype, forced_stop, 1, iters, _c(cost),
            _p(wsrc), _p(omask), _p(out), None]


BAD_SIZES = [(12, 12), (4, 32), (32, 4), (256, 256), (0, 0), (16, 15)]
BAD_DEPTHS = (9, 0, 11, 13, 16)
BAD_COSTS = [None, (-1,), (5,), (X.ENTROPY, False)]
TYPES = (0, 1, 2, 3)


def _nulls(names, rc):
    return [(dict(**{k: False}), rc) for k in names]


REJECTS = {
    PLAIN_EX: (plain_args,
               [(dict(stype=t), -7) for t in (-1, 4, 99)] +
               [(dict(stype=t, w=w, h=h), -3) for t in TYPES for w, h in BAD_SIZES[:2]] +
               [(dict(bd=b), -7) for b in BAD_DEPTHS] + _nulls(("src", "ref", "jobs", "out"), -7) +
               [(dict(forced_stop=f), -1) for f in (-1, 4)] +
               [(dict(cost=c), -2) for c in BAD_COSTS] + [(dict(iters=i), -4) for i in (0, 3)] +
               [(dict(method=m), -6) for m in (-1, 3)] +
               # the order: pointers and depth, type, forced_stop, cost, iters, method, size
               [(dict(stype=4, forced_stop=4, cost=None, w=12), -7),
                (dict(forced_stop=4, cost=None, iters=0, method=3, w=12), -1),
                (dict(method=3, w=12), -6)]),
    COMP_EX: (comp_args,
              [(dict(stype=t), -7) for t in (-1, 4, 99)] +
              [(dict(stype=t, w=w, h=h), -3) for t in TYPES for w, h in BAD_SIZES] +
              [(dict(stype=t, bd=b), -8) for t in (0, 3) for b in BAD_DEPTHS] +
              [(dict(stype=t, **kw), rc) for t in (0, 1, 3)
               for kw, rc in _nulls(("src", "ref", "jobs", "out", "second"), -8) +
               [(dict(mask=True, mask_stride=15), -8), (dict(start_from=2), -8),
                (dict(start_from=-1), -8), (dict(start_from=1), -9)]] +
              [(dict(forced_stop=f), -1) for f in (-1, 4)] +
              [(dict(cost=c), -2) for c in BAD_COSTS] + [(dict(iters=i), -4) for i in (0, 3)] +
              [(dict(method=m), -6) for m in (-1, 3)] +
              # the order: type, forced_stop, cost, iters, method, size, pointers and depth
              [(dict(stype=4, forced_stop=4, cost=None, iters=0, method=3, w=12, bd=9), -7),
               (dict(forced_stop=4, cost=None, iters=0, method=3, w=12, bd=9), -1),
               (dict(w=12, bd=9), -3), (dict(bd=9, start_from=1), -8)]),
    OBMC_EX: (obmc_args,
              [(dict(stype=t), -7) for t in (-1, 4, 99)] +
              [(dict(stype=t, w=w, h=h), -3) for t in TYPES for w, h in BAD_SIZES] +
              [(dict(stype=t, bd=b), -8) for t in (0, 3) for b in BAD_DEPTHS] +
              [(dict(stype=t, **kw), rc) for t in (0, 2)
               for kw, rc in _nulls(("ref", "jobs", "out", "wsrc", "omask"), -8)] +
              [(dict(forced_stop=f), -1) for f in (-1, 4)] +
              [(dict(cost=c), -2) for c in BAD_COSTS] + [(dict(iters=i), -4) for i in (0, 3)] +
              # estimate_obmc_mvcost asserts on the L1 types: USE_2_TAPS_ORIG alone
              # refuses them (the other types get past the cost check: w = 12 -> -3)
              [(dict(stype=0, cost=(t,)), -2) for t in (1, 2, 3)] +
              [(dict(stype=s, cost=(t,), w=12), -3) for s in (1, 2, 3) for t in (1, 2, 3)]),
}
REJECT_CASES = [(name, kw, rc) for name, (_, cases) in REJECTS.items() for kw, rc in cases]


@pytest.mark.parametrize("name,kw,rc", REJECT_CASES,
                         ids=lambda v: str(v).replace(" ", "").replace("lavish_highbd_", ""))
def test_ex_calls_refuse_bad_arguments_before_any_device_work(name, kw, rc):
    assert getattr(_lib(), name)(*REJECTS[name][0](**kw)) == rc


def test_no_jobs_is_a_no_op():
    L = _lib()
    for n in (0, -3):
        for name, (args, _) in REJECTS.items():
            assert getattr(L, name)(*args(njobs=n, w=12, bd=9, cost=None, stype=7)) == 0, name


# ---------------------------------------------------------------- fixture --
@pytest.fixture(scope="module")
def F():
    return U.load_fixture()


def test_restatement_equals_every_fixture_row(F):
    bad, n = [], 0
    for g in U.fixture_groups(F):
        got = U.group_expected(F, g)
        want = g.rows[:, g.J["best_row"]:]
        n += len(want)
        if not np.array_equal(want, got):
            bad.append((g.index, g.prm, want.tolist(), got.tolist()))
    assert n == len(F["rows"]) and not bad, bad[:3]


def test_fixture_covers_what_it_should(F):
    f, forms = U.check_coverage(F)       # (asserts every item; the counts for the record)
    for bd in (8, 10, 12):
        assert f["clip_low_%d" % bd] and f["clip_high_%d" % bd] and f["mid_clip_%d" % bd]
    assert f["clip255_differs"] and f["taps8_vs_bilinear"] and f["clamped_12"] and f["obmc_l1"]
    assert f["centre_differs"] and f["oob"] and f["second_level"]
    assert f["half"] and f["quarter"] and f["eighth"]
    groups = list(U.fixture_groups(F))
    assert {(g.prm["bw"], g.prm["bh"]) for g in groups} == {(4, 4), (8, 8), (16, 8), (16, 16),
                                                           (32, 32)}
    # one 32x32 row per form
    big = [g.prm["form"] for g in groups if g.prm["bw"] == 32 for _ in g.cjobs]
    assert sorted(big) == [U.PLAIN, U.AVG, U.MASK, U.OBMC]
    assert {g.prm["search_type"] for g in groups} == {1, 2, 3}
    assert {g.prm["forced_stop"] for g in groups} == {0, 1, 2, 3}
    assert {g.prm["iters"] for g in groups} == {1, 2}
    assert {g.prm["allow_hp"] for g in groups} == {0, 1}
    assert {g.prm["cost"] for g in groups} == {X.ENTROPY, X.L1, X.NONE}
    assert 150 <= len(F["rows"]) <= 260
    for g in groups:
        src, ref = U.group_planes(F, g)
        assert int(src.max()) < 1 << g.prm["bd"] and int(ref.max()) < 1 << g.prm["bd"]
    assert F["second"].dtype == np.uint16 and F["mask"].dtype == np.uint8
    assert F["wsrc"].dtype == np.int32 and F["omask"].dtype == np.int32
    assert int(F["mask"].max()) <= 64 and int(F["omask"].max()) <= 4096
    assert os.path.getsize(os.path.join(GOLD, "fix_subpel_up_hbd.npz")) < 400 * 1024


def test_every_window_lies_inside_the_planes(F):
    """Every in-range candidate's (w + 7) x (h + 7) window, with one element
    of slack either side, stays inside its plane: the border is wider than
    the SubpelMvLimits reach plus 4."""
    for g in U.fixture_groups(F):
        bw, bh = g.prm["bw"], g.prm["bh"]
        b = g.cjobs["base"]
        k = (b["ref_off"] - b["src_off"]) // X.PLANE
        org = b["ref_off"] - k * X.PLANE
        y, x = org // X.STRIDE, org % X.STRIDE
        assert (y + (b["row_min"] >> 3) - 3 >= 0).all() and (x + (b["col_min"] >> 3) - 4 >= 0).all()
        assert (y + (b["row_max"] >> 3) + bh + 4 < X.PH).all()
        assert (x + (b["col_max"] >> 3) + bw + 4 < X.PW).all()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_fixture_sample_rederived_from_the_reference_text(F):
    """The first row of one small case per form x {2 taps, 4 / 8 taps},
    re-executed from the C text."""
    sys.path.insert(0, GOLD)
    import gen_fix_subpel_up_hbd as G
    from gen_fixtures import nmv_cost_tables
    R = G.make_ref(nmv_cost_tables())
    done = set()
    for g in U.fixture_groups(F):
        p = g.prm
        key = (p["form"], p["search_type"] > U.USE_2_TAPS)
        if key in done or p["bw"] * p["bh"] > 128:
            continue
        src, refs = F["src__" + g.plane], F["refs__" + g.plane]
        c = dict(p, epb=p["error_per_bit"])
        got = G.case_rows(R, c, g.cjobs[:1], F, src, refs)
        assert got[0] == g.rows[0, g.J["best_row"]:].tolist(), (g.index, p)
        done.add(key)
    assert len(done) == 8, done


# ---------------------------------------------------------------- kernels --
def test_upsampled_kernels_stay_within_their_8bit_twins_resources():
    """Code-object metadata (tools/kernel_resources.py) of every
    hbd_upsampled_kernel<W, H, FORM> (22 block sizes x 4 forms): no LDS, no
    SGPR or VGPR spill count above the 8-bit twin's, scratch no larger than
    comp_subpel_kernel<W, H, FORM, true>'s (the plain form: subpel_kernel<W,
    H>'s) in the same library."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler") or \
            shutil.which("c++filt") is None:
        pytest.skip("ROCm code-object tools not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    res = KR.kernel_resources(os.path.join(ROOT, "aom-av1-lavish_amd", "liblavish_hip.so"))
    names = sorted(res)
    table = dict(zip(KR.demangled(names), (res[n] for n in names)))
    mine = {d: v for d, v in table.items() if "hbd_upsampled_kernel<" in d}
    assert len(mine) == 88, len(mine)
    assert not any("hbd_subpel_kernel<" in d or "hbd_csubpel_kernel<" in d for d in mine)
    seen = set()
    for name, v in mine.items():
        w, h, form = (int(x) for x in re.search(r"hbd_upsampled_kernel<(\d+), (\d+), (\d+)>",
                                                name).groups())
        seen.add((w, h, form))
        pat = (r"(^|[ :])subpel_kernel<%d, %d>" % (w, h) if form == 0 else
               r"comp_subpel_kernel<%d, %d, %d, true>" % (w, h, form))
        twins = [t for d, t in table.items() if re.search(pat, d)]
        assert len(twins) == 1, (name, len(twins))
        t = twins[0]
        assert v.get("group_segment_fixed_size", 0) == 0, (name, v)
        for k in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
            assert v.get(k, 0) <= t.get(k, 0), (name, k, v, t)
    assert len(seen) == 88 and {f for _, _, f in seen} == {0, 1, 2, 3}
