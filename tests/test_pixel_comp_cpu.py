"""CPU tests of the masked / OBMC / distance-weighted pixel layer (no GPU):
* include/lavish_dsp.h declares, and the library exports, the 512 new `_hip`
  names and the four batch calls;
* the new symbols of one block size assign to the reference's function-pointer
  types (aom_dsp/variance.h:53-82, written out here) without a warning;
* every argument the batch calls refuse is refused with a negative return
  before any device work;
* tests/_compref.py equals every entry of tests/golden/fix_pixel_comp.npz;
* a sample of that fixture re-derived from the reference's C text (skipped
  where the reference sources are absent)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _compref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "lavish_dsp.h")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")

SIZES = [(128, 128), (128, 64), (64, 128), (64, 64), (64, 32), (32, 64), (32, 32), (32, 16),
         (16, 32), (16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4), (4, 16), (16, 4),
         (8, 32), (32, 8), (16, 64), (64, 16)]
BATCH_CALLS = ["lavish_comp_sad_batch", "lavish_comp_variance_batch", "lavish_obmc_batch",
               "lavish_comp_pred_batch"]


def new_names():
    names = []
    for w, h in SIZES:
        s = "%dx%d" % (w, h)
        names += ["aom_masked_sad" + s, "aom_masked_sad%sx4d" % s, "aom_obmc_sad" + s,
                  "aom_dist_wtd_sad%s_avg" % s, "aom_masked_sub_pixel_variance" + s,
                  "aom_obmc_variance" + s, "aom_obmc_sub_pixel_variance" + s,
                  "aom_dist_wtd_sub_pixel_avg_variance" + s,
                  "aom_highbd_masked_sad" + s, "aom_highbd_obmc_sad" + s,
                  "aom_highbd_dist_wtd_sad%s_avg" % s]
        for bd in (8, 10, 12):
            names += ["aom_highbd_%d_masked_sub_pixel_variance%s" % (bd, s),
                      "aom_highbd_%d_dist_wtd_sub_pixel_avg_variance%s" % (bd, s)]
        for pre in ("aom_highbd_", "aom_highbd_10_", "aom_highbd_12_"):
            names += [pre + "obmc_variance" + s, pre + "obmc_sub_pixel_variance" + s]
    for pre in ("aom_", "aom_highbd_"):
        names += [pre + "comp_avg_pred", pre + "dist_wtd_comp_avg_pred", pre + "comp_mask_pred"]
    return [n + "_hip" for n in names]


def test_header_declares_and_library_exports_the_new_symbols():
    import lavish_dsp
    names = new_names()
    assert len(names) == 512 and len(set(names)) == 512
    out = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True, capture_output=True,
                         text=True).stdout
    declared = set(re.findall(r"\b(lavish_\w+|aom_\w+_hip)\s*\(", out))
    assert not [n for n in names + BATCH_CALLS if n not in declared]
    L = lavish_dsp.lib()
    assert not [n for n in names + BATCH_CALLS if not hasattr(L, n)]


FN_TYPES = """
typedef LavishDistWtdCompParams DIST_WTD_COMP_PARAMS;
typedef unsigned int (*aom_dist_wtd_sad_avg_fn_t)(
    const uint8_t *a, int a_stride, const uint8_t *b, int b_stride,
    const uint8_t *second_pred, const DIST_WTD_COMP_PARAMS *jcp_param);
typedef unsigned int (*aom_dist_wtd_subp_avg_variance_fn_t)(
    const uint8_t *a, int a_stride, int xoffset, int yoffset, const uint8_t *b,
    int b_stride, unsigned int *sse, const uint8_t *second_pred,
    const DIST_WTD_COMP_PARAMS *jcp_param);
typedef unsigned int (*aom_masked_sad_fn_t)(const uint8_t *src, int src_stride,
                                            const uint8_t *ref, int ref_stride,
                                            const uint8_t *second_pred,
                                            const uint8_t *msk, int msk_stride,
                                            int invert_mask);
typedef unsigned int (*aom_masked_subpixvariance_fn_t)(
    const uint8_t *src, int src_stride, int xoffset, int yoffset,
    const uint8_t *ref, int ref_stride, const uint8_t *second_pred,
    const uint8_t *msk, int msk_stride, int invert_mask, unsigned int *sse);
typedef unsigned int (*aom_obmc_sad_fn_t)(const uint8_t *pred, int pred_stride,
                                          const int32_t *wsrc, const int32_t *msk);
typedef unsigned int (*aom_obmc_variance_fn_t)(const uint8_t *pred, int pred_stride,
                                               const int32_t *wsrc, const int32_t *msk,
                                               unsigned int *sse);
typedef unsigned int (*aom_obmc_subpixvariance_fn_t)(
    const uint8_t *pred, int pred_stride, int xoffset, int yoffset,
    const int32_t *wsrc, const int32_t *msk, unsigned int *sse);
typedef void (*masked_sad_x4d_fn_t)(const uint8_t *src, int src_stride, const uint8_t *ref[4],
                                    int ref_stride, const uint8_t *second_pred,
                                    const uint8_t *msk, int msk_stride, int invert_mask,
                                    unsigned sads[4]);
typedef void (*comp_avg_pred_fn_t)(uint8_t *comp_pred, const uint8_t *pred, int width,
                                   int height, const uint8_t *ref, int ref_stride);
typedef void (*dist_wtd_comp_avg_pred_fn_t)(uint8_t *comp_pred, const uint8_t *pred, int width,
                                            int height, const uint8_t *ref, int ref_stride,
                                            const DIST_WTD_COMP_PARAMS *jcp_param);
typedef void (*comp_mask_pred_fn_t)(uint8_t *comp_pred, const uint8_t *pred, int width,
                                    int height, const uint8_t *ref, int ref_stride,
                                    const uint8_t *mask, int mask_stride, int invert_mask);
"""


@pytest.mark.parametrize("size", ["16x16", "4x16", "128x64"])
def test_symbols_assign_to_the_reference_function_pointer_types(size, tmp_path):
    """The seven lowbd members (+ x4d) and every highbd form of one block size,
    and the six prediction helpers."""
    assign = []
    for pre in ("aom_", "aom_highbd_"):
        assign += [("aom_masked_sad_fn_t", pre + "masked_sad" + size),
                   ("aom_obmc_sad_fn_t", pre + "obmc_sad" + size),
                   ("aom_dist_wtd_sad_avg_fn_t", pre + "dist_wtd_sad%s_avg" % size),
                   ("comp_avg_pred_fn_t", pre + "comp_avg_pred"),
                   ("dist_wtd_comp_avg_pred_fn_t", pre + "dist_wtd_comp_avg_pred"),
                   ("comp_mask_pred_fn_t", pre + "comp_mask_pred")]
    assign.append(("masked_sad_x4d_fn_t", "aom_masked_sad%sx4d" % size))
    for pre in ("aom_", "aom_highbd_8_", "aom_highbd_10_", "aom_highbd_12_"):
        assign += [("aom_masked_subpixvariance_fn_t", pre + "masked_sub_pixel_variance" + size),
                   ("aom_dist_wtd_subp_avg_variance_fn_t",
                    pre + "dist_wtd_sub_pixel_avg_variance" + size)]
    for pre in ("aom_", "aom_highbd_", "aom_highbd_10_", "aom_highbd_12_"):
        assign += [("aom_obmc_variance_fn_t", pre + "obmc_variance" + size),
                   ("aom_obmc_subpixvariance_fn_t", pre + "obmc_sub_pixel_variance" + size)]
    src = '#include "lavish_dsp.h"\n' + FN_TYPES
    src += "".join("%s p%d = %s_hip;\n" % (t, i, n) for i, (t, n) in enumerate(assign))
    src += ("_Static_assert(sizeof(LavishCompJob) == 72, \"job record\");\n"
            "_Static_assert(sizeof(LavishDistWtdCompParams) == 3 * sizeof(int), \"jcp\");\n")
    path = tmp_path / "assign.c"
    path.write_text(src)
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall",
                        "-Werror=incompatible-pointer-types", "-I", os.path.dirname(HEADER),
                        str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------- rejects --
_vp, _i = ctypes.c_void_p, ctypes.c_int32


def _calls():
    import lavish_dsp
    import lavish_dsp.pixel  # noqa: F401  (sets the argtypes)
    return lavish_dsp.lib()


class Args:
    """Argument lists of the four batch calls with every pointer a live host
    buffer (never dereferenced: the calls under test return before any work)."""

    def __init__(self):
        self.buf = np.zeros(4096, np.uint8)
        self.p = _vp(self.buf.__array_interface__["data"][0])

    def sad(self, w=16, h=16, njobs=1, nrefs=1, mode=0, second=True, mask=True, ms=None,
            fwd=9, bck=7, highbd=0):
        p = self.p
        return [p, 64, p, 64, w, h, p, njobs, nrefs, mode, p if second else None,
                p if mask else None, w if ms is None else ms, fwd, bck, highbd, p, None]

    def var(self, w=16, h=16, njobs=1, kind=0, bd=8, second=True, mask=True, ms=None, fwd=9,
            bck=7, highbd=1):
        p = self.p
        return [p, 64, p, 64, w, h, p, njobs, kind, bd, highbd, p if second else None,
                p if mask else None, w if ms is None else ms, fwd, bck, p, p, None]

    def obmc(self, w=16, h=16, njobs=1, npre=1, kind=0, bd=8, wsrc=True, mask=True, highbd=1):
        p = self.p
        return [p, 64, w, h, p, njobs, npre, kind, bd, highbd, p if wsrc else None,
                p if mask else None, p, p, None]

    def pred(self, w=16, h=16, njobs=1, mode=0, pred=True, mask=True, ms=None, fwd=9, bck=7,
             highbd=0):
        p = self.p
        return [p, p if pred else None, w, h, p, 64, p, njobs, mode, p if mask else None,
                w if ms is None else ms, fwd, bck, highbd, None]


BAD_SIZES = [(12, 12), (4, 32), (32, 4), (256, 256), (0, 0), (8, 64), (16, 15)]
BAD_OFFSETS = [(8, 7), (9, 8), (-1, 17), (17, -1), (0, 0)]

REJECTS = (
    [("sad", dict(nrefs=n)) for n in (0, 5, -1)] + [("sad", dict(mode=m)) for m in (-1, 2)] +
    [("sad", dict(mode=m, second=False)) for m in (0, 1)] + [("sad", dict(mask=False))] +
    [("sad", dict(ms=15)), ("sad", dict(w=128, h=128, ms=127))] +
    [("sad", dict(mode=1, fwd=f, bck=b)) for f, b in BAD_OFFSETS] +
    [("sad", dict(w=w, h=h, ms=300)) for w, h in BAD_SIZES] +
    [("var", dict(kind=k)) for k in (-1, 2)] + [("var", dict(bd=b)) for b in (9, 0, 16)] +
    [("var", dict(kind=k, second=False)) for k in (0, 1)] + [("var", dict(mask=False))] +
    [("var", dict(ms=15))] + [("var", dict(kind=1, fwd=f, bck=b)) for f, b in BAD_OFFSETS] +
    [("var", dict(w=w, h=h, ms=300)) for w, h in BAD_SIZES] +
    [("obmc", dict(kind=k)) for k in (-1, 3)] + [("obmc", dict(npre=n)) for n in (0, 5)] +
    [("obmc", dict(kind=k, npre=2)) for k in (1, 2)] + [("obmc", dict(bd=b)) for b in (11, 7)] +
    [("obmc", dict(wsrc=False)), ("obmc", dict(mask=False))] +
    [("obmc", dict(w=w, h=h)) for w, h in BAD_SIZES] +
    [("pred", dict(mode=m)) for m in (-1, 3)] + [("pred", dict(pred=False))] +
    [("pred", dict(mode=2, mask=False)), ("pred", dict(mode=2, ms=15))] +
    [("pred", dict(mode=1, fwd=f, bck=b)) for f, b in BAD_OFFSETS] +
    [("pred", dict(w=w, h=h, ms=300)) for w, h in BAD_SIZES])
FUNCS = {"sad": "lavish_comp_sad_batch", "var": "lavish_comp_variance_batch",
         "obmc": "lavish_obmc_batch", "pred": "lavish_comp_pred_batch"}


@pytest.mark.parametrize("which,kw", REJECTS, ids=lambda v: str(v).replace(" ", ""))
def test_bad_arguments_are_refused_before_any_device_work(which, kw):
    L = _calls()
    a = Args()
    assert getattr(L, FUNCS[which])(*getattr(a, which)(**kw)) < 0


@pytest.mark.parametrize("which", sorted(FUNCS))
def test_no_jobs_is_a_no_op(which):
    L = _calls()
    a = Args()
    assert getattr(L, FUNCS[which])(*getattr(a, which)(njobs=0)) == 0
    assert getattr(L, FUNCS[which])(*getattr(a, which)(njobs=-3, w=12, h=12)) == 0


# ---------------------------------------------------------------- fixture --
@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(GOLD, "fix_pixel_comp.npz")))


def stored(F, c):
    if c.kind == R.MSAD_X4D:
        return [int(v) for v in F["x4d"][c.ret]]
    if c.kind >= R.PRED_AVG:
        return F["pred_out"][c.ret:c.ret + c.w * c.h].astype(np.int64).reshape(c.h, c.w)
    return (c.ret, c.sse)


def test_fixture_covers_what_it_should(F):
    rows = F["cases"]
    col = {k: rows[:, i] for i, k in enumerate(R.COLS)}
    main = col["variant"] == 0
    for kind in (R.MSAD, R.MSVAR, R.OSAD, R.OVAR, R.OSVAR, R.JSAD, R.JSVAR):
        got = {(w, h, bd, hb) for w, h, bd, hb in rows[main & (col["kind"] == kind)][:, 1:5]}
        assert got == {(w, h, bd, hb) for (w, h) in SIZES
                       for bd, hb in ((8, 0), (8, 1), (10, 1), (12, 1))}
    assert {(w, h) for w, h in rows[col["kind"] == R.MSAD_X4D][:, 1:3]} == set(SIZES)
    for kind in (R.MSAD, R.MSVAR, R.PRED_MASK):
        assert set(col["invert"][col["kind"] == kind]) == {0, 1}
    sub = {(x, y) for x, y in rows[col["kind"] == R.MSVAR][:, 9:11]}
    assert (0, 0) in sub and any(7 in s for s in sub) and len(sub) >= 3
    pairs = {(f, b) for f, b in rows[np.isin(col["kind"], (R.JSAD, R.JSVAR))][:, 12:14]}
    q = [(9, 7), (11, 5), (12, 4), (13, 3)]
    assert pairs >= set(q) | {(b, a) for a, b in q}
    assert F["a_bd8"].shape[1] > 129 and F["mask"].shape[1] not in (w for w, _ in SIZES)
    for v in (1, 2, 3, 4):
        assert {(w, h) for w, h in rows[col["variant"] == v][:, 1:3]} == {(4, 4), (16, 16),
                                                                           (128, 128)}
    assert (col["variant"] == 5).sum() >= 5
    # some highbd OBMC sums are negative (the rounding the fixture must catch)
    assert (F["wsrc_bd10"] < 0).any() and (F["wsrc_bd12"] > 0).any()
    assert os.path.getsize(os.path.join(GOLD, "fix_pixel_comp.npz")) < (1 << 20)


def test_numpy_restatement_equals_every_fixture_entry(F):
    bad = []
    for row in F["cases"]:
        c = R.case_inputs(F, row)
        want, got = stored(F, c), R.expected(c)
        if c.kind >= R.PRED_AVG:
            ok = np.array_equal(want, got)
        else:
            ok = list(want) == list(got)
        if not ok:
            bad.append((R.rtcd_name(c), row.tolist(), got if c.kind < R.PRED_AVG else "block"))
    assert not bad, bad[:5]


def test_signed_sum_rounding_is_an_arithmetic_shift():
    """(sum + half) >> n of a negative int64 (variance.c:1081, 1092): not
    sign-symmetric; a symmetric restatement gives another variance here."""
    # sum64 = -258 at 10 bits: (-258 + 2) >> 2 = -64; rounding |sum| gives -65
    assert R.variance_tail(-258, 256 * 16 * 16, 10, 16) == (4096 - 64 * 64 // 16, 4096)
    assert R.variance_tail(-259, 256 * 16 * 16, 10, 16) == (4096 - 65 * 65 // 16, 4096)
    # 12 bits: (-24 + 8) >> 4 = -1, not -2
    assert R.variance_tail(-24, 16 << 8, 12, 16) == (16 - 1 // 16, 16)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_fixture_sample_rederived_from_the_reference_text(F):
    """One masked, one OBMC and one distance-weighted kind (and a prediction
    helper) at 8x8 / 16x8, every bit depth, re-executed from the C text."""
    sys.path.insert(0, GOLD)
    import gen_fix_pixel_comp as G
    run = G.Runner(G.tu_pixel_comp(), F)
    done = set()
    for row in F["cases"]:
        c = R.case_inputs(F, row)
        if (c.w, c.h) not in ((8, 8), (16, 8)) or c.kind not in (R.MSVAR, R.MSAD, R.OVAR, R.OSAD,
                                                                   R.JSVAR, R.PRED_MASK):
            continue
        ret, sse = run.run(list(row))
        if c.kind >= R.PRED_AVG:
            np.testing.assert_array_equal(np.array(run.pred[-1]).reshape(c.h, c.w), stored(F, c))
        else:
            assert (ret, sse) == (c.ret, c.sse), R.rtcd_name(c)
        done.add((c.kind, c.bd, c.highbd))
    assert len(done) >= 5 * 4 + 3
