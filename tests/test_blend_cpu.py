"""CPU tests of the mask-building and blending layer (no GPU):
* tests/_blendref.py equals every entry of tests/golden/fix_blend.npz (the
  reference's own outputs), and the restated neighbour walk gives the bitmaps
  the generator's visitor recorded on the reference's walk;
* the fixture covers what it should;
* a sample of it re-derived from the reference's C text (skipped where the
  reference sources are absent);
* include/lavish_dsp.h declares, and the library exports, the 5 batch calls
  and the 14 `_hip` shims, whose prototypes are the reference's;
* every argument the batch calls refuse is refused with a negative return
  before any device work;
* no instantiation of the new kernels uses scratch or spills."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _blendref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "lavish_dsp.h")
REF = os.environ.get("LAVISH_REFERENCE", "/root/reference")

BATCH_CALLS = ["lavish_blend_a64_batch", "lavish_diffwtd_mask_batch", "lavish_obmc_wsrc_batch",
               "lavish_obmc_blend_batch", "lavish_wedge_batch"]
SHIMS = ["aom_blend_a64_mask", "aom_blend_a64_hmask", "aom_blend_a64_vmask",
         "aom_highbd_blend_a64_mask", "aom_highbd_blend_a64_hmask", "aom_highbd_blend_a64_vmask",
         "aom_lowbd_blend_a64_d16_mask", "aom_highbd_blend_a64_d16_mask",
         "av1_build_compound_diffwtd_mask", "av1_build_compound_diffwtd_mask_highbd",
         "av1_build_compound_diffwtd_mask_d16", "av1_wedge_sse_from_residuals",
         "av1_wedge_sign_from_residuals", "av1_wedge_compute_delta_squares"]


@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(GOLD, "fix_blend.npz")))


# ---------------------------------------------------------------- fixture --
def test_fixture_covers_what_it_should(F):
    assert R.coverage_problems(F) == []
    assert os.path.getsize(os.path.join(GOLD, "fix_blend.npz")) < 1000000
    # the obmc table is the reference's: weights rise towards 64 and each
    # length starts at byte n - 1
    assert [int(F["obmc_masks"][n - 1]) for n in R.OBMC_LENGTHS] == [64, 45, 39, 36, 34, 33, 33]
    for (w, h) in R.WEDGE_SIZES:
        m = F["wedge_masks_%dx%d" % (w, h)]
        assert m.shape == (16, 2, h, w) and m.max() == 64 and m.min() == 0
        assert (m[:, 0].astype(int) + m[:, 1] == 64).all()  # the two signs are complements


def test_restatement_equals_every_blend_entry(F):
    bad = []
    for row in F["blend_cases"]:
        c = R.blend_case(F, row)
        want = F["blend_out"][c.out_off:c.out_off + c.w * c.h].astype(np.int64).reshape(c.h, c.w)
        if not np.array_equal(R.blend_expected(c), want):
            bad.append(row.tolist())
    assert not bad, bad[:5]


def test_restatement_equals_every_diffwtd_entry(F):
    bad = []
    for row in F["dw_cases"]:
        c = R.diffwtd_case(F, row)
        want = F["dw_out"][c.out_off:c.out_off + c.w * c.h].astype(np.int64).reshape(c.h, c.w)
        if not np.array_equal(R.diffwtd_expected(c), want):
            bad.append(row.tolist())
    assert not bad, bad[:5]


def test_restatement_equals_every_wedge_entry(F):
    bad = []
    for row in F["wedge_cases"]:
        c = R.wedge_case(F, row)
        got = R.wedge_expected(c)
        if c.kind == 0:
            ok = np.array_equal(got, F["wedge_out"][c.ret:c.ret + c.n].astype(np.int64))
        else:
            ok = got == c.ret
        if not ok:
            bad.append(row.tolist())
    assert not bad, bad[:5]


def test_restatement_equals_every_obmc_entry(F):
    tab = F["obmc_masks"]
    for row in F["obmc_cases"]:
        c = R.obmc_case(F, row)
        sc = c.sc
        assert (c.above_mask, c.left_mask) == R.scene_bitmaps(sc), sc["name"]
        n = c.pw * c.ph
        pred = R.obmc_blend(c.src, c.above, c.left, c.above_mask, c.left_mask, sc["bw"], sc["bh"],
                            c.ssx, c.ssy, tab)
        want = F["obmc_pred"][c.pred_off:c.pred_off + n].astype(np.int64).reshape(c.ph, c.pw)
        assert np.array_equal(pred, want), (sc["name"], c.plane)
        if c.plane == 0:
            ws, mk = R.obmc_wsrc(c.src, c.above, c.left, c.above_mask, c.left_mask, tab)
            for got, key in ((ws, "obmc_wsrc"), (mk, "obmc_mask")):
                want = F[key][c.wsrc_off:c.wsrc_off + n].astype(np.int64).reshape(c.ph, c.pw)
                assert np.array_equal(got, want), (sc["name"], key)


def test_wsrc_fits_int32_at_12_bits():
    """The bound the kernel's comment states: |wsrc| < 2^24, 0 <= mask <= 4096."""
    tab = np.concatenate([np.full(n, v, np.uint8) for n in R.OBMC_LENGTHS for v in (0,)])
    mx = np.full((64, 64), 4095)
    z = np.zeros((64, 64), np.int64)
    for t in (tab, tab + 33, tab + 64):
        for src, nb in ((mx, z), (z, mx), (mx, mx)):
            ws, mk = R.obmc_wsrc(src, nb, nb, 0xFFFF, 0xFFFF, t)
            assert np.abs(ws).max() < 1 << 24 and mk.min() >= 0 and mk.max() <= 4096


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "av1")),
                    reason="reference sources absent (GPU box)")
def test_fixture_sample_rederived_from_the_reference_text(F):
    """Every blend form and bit depth at 8x8 / 4x16 / 2x2, the diff-weighted
    masks at 8x8, the wedge reductions at N = 64 / 128 and five OBMC scenes,
    re-executed from the C text."""
    sys.path.insert(0, GOLD)
    import gen_fix_blend as G
    run = G.Runner(G.tu_blend(), F)
    done = set()
    for row in F["blend_cases"]:
        c = R.blend_case(F, row)
        if (c.w, c.h) not in ((8, 8), (4, 16), (2, 2)):
            continue
        want = F["blend_out"][c.out_off:c.out_off + c.w * c.h].astype(np.int64).reshape(c.h, c.w)
        assert np.array_equal(run.blend(row), want), row.tolist()
        done.add((c.form, c.bd, c.highbd))
    assert len(done) >= 4 * 3
    for row in F["dw_cases"]:
        c = R.diffwtd_case(F, row)
        if (c.w, c.h) == (8, 8):
            want = F["dw_out"][c.out_off:c.out_off + 64].astype(np.int64).reshape(8, 8)
            assert np.array_equal(run.diffwtd(row), want), row.tolist()
    for row in F["wedge_cases"]:
        c = R.wedge_case(F, row)
        if c.n <= 128:
            got = run.wedge(row)
            if c.kind == 0:
                assert np.array_equal(got, F["wedge_out"][c.ret:c.ret + c.n].astype(np.int64))
            else:
                assert got == c.ret, row.tolist()
    names = ("16x16_4wide", "64x64_8wide", "32x32_intra_mid", "16x16_bd10", "16x8")
    for si, sc in enumerate(R.OBMC_SCENES):
        if sc["name"] not in names:
            continue
        rows = [r for r in F["obmc_cases"] if r[0] == si]
        bits, ws, mk, preds = run.obmc(si, G.obmc_offsets(si))
        for r in rows:
            c = R.obmc_case(F, r)
            n = c.pw * c.ph
            assert bits == (c.above_mask, c.left_mask)
            assert np.array_equal(preds[c.plane].reshape(-1), F["obmc_pred"][c.pred_off:c.pred_off + n])
            if c.plane == 0:
                assert np.array_equal(ws.reshape(-1), F["obmc_wsrc"][c.wsrc_off:c.wsrc_off + n])
                assert np.array_equal(mk.reshape(-1), F["obmc_mask"][c.wsrc_off:c.wsrc_off + n])


# ------------------------------------------------------------ the C ABI ----
def test_header_declares_and_library_exports_the_new_symbols():
    import lavish_dsp
    names = BATCH_CALLS + [n + "_hip" for n in SHIMS]
    out = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True, capture_output=True,
                         text=True).stdout
    declared = set(re.findall(r"\b(lavish_\w+|a(?:om|v1)_\w+_hip)\s*\(", out))
    assert not [n for n in names if n not in declared]
    L = lavish_dsp.lib()
    assert not [n for n in names if not hasattr(L, n)]
    import lavish_dsp.blend as B
    assert B.SHIM_NAMES == SHIMS and B.BATCH_NAMES == BATCH_CALLS
    assert not [n for n in SHIMS if not callable(getattr(B, n))]


# the reference's prototypes (aom_dsp_rtcd_defs.pl:701-718, av1_rtcd_defs.pl:257-266,
# 440-445) as function-pointer types
FN_TYPES = """
typedef uint16_t CONV_BUF_TYPE;
typedef uint8_t DIFFWTD_MASK_TYPE;
typedef LavishConvolveParams ConvolveParams;
typedef void (*d16_lowbd_t)(uint8_t *dst, uint32_t dst_stride, const CONV_BUF_TYPE *src0,
    uint32_t src0_stride, const CONV_BUF_TYPE *src1, uint32_t src1_stride, const uint8_t *mask,
    uint32_t mask_stride, int w, int h, int subw, int subh, ConvolveParams *conv_params);
typedef void (*d16_highbd_t)(uint8_t *dst, uint32_t dst_stride, const CONV_BUF_TYPE *src0,
    uint32_t src0_stride, const CONV_BUF_TYPE *src1, uint32_t src1_stride, const uint8_t *mask,
    uint32_t mask_stride, int w, int h, int subw, int subh, ConvolveParams *conv_params,
    const int bd);
typedef void (*mask_t)(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0,
    uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask,
    uint32_t mask_stride, int w, int h, int subw, int subh);
typedef void (*hvmask_t)(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0,
    uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, int w,
    int h);
typedef void (*hb_mask_t)(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0,
    uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask,
    uint32_t mask_stride, int w, int h, int subw, int subh, int bd);
typedef void (*hb_hvmask_t)(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0,
    uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, int w,
    int h, int bd);
typedef void (*dw_t)(uint8_t *mask, DIFFWTD_MASK_TYPE mask_type, const uint8_t *src0,
    int src0_stride, const uint8_t *src1, int src1_stride, int h, int w);
typedef void (*dw_hb_t)(uint8_t *mask, DIFFWTD_MASK_TYPE mask_type, const uint8_t *src0,
    int src0_stride, const uint8_t *src1, int src1_stride, int h, int w, int bd);
typedef void (*dw_d16_t)(uint8_t *mask, DIFFWTD_MASK_TYPE mask_type, const CONV_BUF_TYPE *src0,
    int src0_stride, const CONV_BUF_TYPE *src1, int src1_stride, int h, int w,
    ConvolveParams *conv_params, int bd);
typedef uint64_t (*wsse_t)(const int16_t *r1, const int16_t *d, const uint8_t *m, int N);
typedef int8_t (*wsign_t)(const int16_t *ds, const uint8_t *m, int N, int64_t limit);
typedef void (*wds_t)(int16_t *d, const int16_t *a, const int16_t *b, int N);
"""
ASSIGN = [("d16_lowbd_t", "aom_lowbd_blend_a64_d16_mask"),
          ("d16_highbd_t", "aom_highbd_blend_a64_d16_mask"), ("mask_t", "aom_blend_a64_mask"),
          ("hvmask_t", "aom_blend_a64_hmask"), ("hvmask_t", "aom_blend_a64_vmask"),
          ("hb_mask_t", "aom_highbd_blend_a64_mask"), ("hb_hvmask_t", "aom_highbd_blend_a64_hmask"),
          ("hb_hvmask_t", "aom_highbd_blend_a64_vmask"), ("dw_t", "av1_build_compound_diffwtd_mask"),
          ("dw_hb_t", "av1_build_compound_diffwtd_mask_highbd"),
          ("dw_d16_t", "av1_build_compound_diffwtd_mask_d16"),
          ("wsse_t", "av1_wedge_sse_from_residuals"), ("wsign_t", "av1_wedge_sign_from_residuals"),
          ("wds_t", "av1_wedge_compute_delta_squares")]


def test_shims_assign_to_the_reference_function_pointer_types(tmp_path):
    assert sorted(n for _, n in ASSIGN) == sorted(SHIMS)
    src = '#include "lavish_dsp.h"\n' + FN_TYPES
    src += "".join("%s p%d = %s_hip;\n" % (t, i, n) for i, (t, n) in enumerate(ASSIGN))
    src += ("_Static_assert(sizeof(LavishObmcJob) == 48, \"obmc job record\");\n"
            "_Static_assert(sizeof(LavishWedgeJob) == 48, \"wedge job record\");\n")
    path = tmp_path / "assign.c"
    path.write_text(src)
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall",
                        "-Werror=incompatible-pointer-types", "-I", os.path.dirname(HEADER),
                        str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------- rejects --
_vp = ctypes.c_void_p


def _calls():
    import lavish_dsp
    import lavish_dsp.blend  # noqa: F401  (sets the argtypes)
    return lavish_dsp.lib()


class Args:
    """Argument lists of the five batch calls with every pointer a live host
    buffer (never dereferenced: the calls under test return before any work)."""

    def __init__(self):
        from lavish_dsp.blend import conv_params
        self.buf = np.zeros(4096, np.uint8)
        self.p = _vp(self.buf.__array_interface__["data"][0])
        self.cp = conv_params

    def _cp(self, cp, r0, r1):
        self.keep = self.cp(r0, r1)
        return ctypes.byref(self.keep) if cp else None

    def blend(self, w=16, h=16, njobs=1, kind=0, subw=0, subh=0, d16=0, highbd=0, bd=8, ms=None,
              cp=True, r0=3, r1=7, dst=True, src1=True, mask=True):
        p = self.p
        return [p if dst else None, 64, p, 64, p if src1 else None, 64, p if mask else None,
                (w << subw) if ms is None else ms, w, h, p, njobs, kind, subw, subh, d16, highbd,
                bd, self._cp(cp, r0, r1), None]

    def diffwtd(self, w=16, h=16, njobs=1, d16=0, highbd=0, bd=8, cp=True, r0=3, r1=7, mask=True):
        p = self.p
        return [p if mask else None, p, 64, p, 64, w, h, p, njobs, d16, highbd, bd,
                self._cp(cp, r0, r1), None]

    def wsrc(self, bw=16, bh=16, njobs=1, tab=True, highbd=0, wsrc=True):
        p = self.p
        return [p, 64, p, 64, p, 64, bw, bh, p, njobs, p if tab else None, highbd,
                p if wsrc else None, p, None]

    def oblend(self, bw=16, bh=16, njobs=1, ssx=0, ssy=0, tab=True, highbd=0, dst=True):
        p = self.p
        return [p if dst else None, 64, p, 64, p, 64, bw, bh, ssx, ssy, p, njobs,
                p if tab else None, highbd, None]

    def wedge(self, njobs=1, kind=1, a=True, b=True, m=True, out=True):
        p = self.p
        return [p if a else None, p if b else None, p if m else None, p, njobs, kind,
                p if out else None, None]


BAD_POW2 = [(12, 16), (16, 12), (256, 16), (16, 256), (0, 16), (16, 0), (-4, 4)]
BAD_OBMC = [(4, 4), (4, 8), (8, 4), (4, 16), (16, 4), (12, 12), (8, 64), (256, 256), (0, 0)]
REJECTS = (
    [("blend", dict(kind=k)) for k in (-1, 3)] +
    [("blend", dict(subw=2)), ("blend", dict(subh=-1)), ("blend", dict(kind=1, subw=1)),
     ("blend", dict(kind=2, subh=1)), ("blend", dict(kind=1, d16=1)), ("blend", dict(ms=15)),
     ("blend", dict(subw=1, ms=31)), ("blend", dict(dst=False)), ("blend", dict(src1=False)),
     ("blend", dict(mask=False)), ("blend", dict(bd=10)), ("blend", dict(highbd=1, bd=9)),
     ("blend", dict(d16=1, cp=False)), ("blend", dict(d16=1, r0=8, r1=7)),
     ("blend", dict(d16=1, r0=-1)), ("blend", dict(d16=1, w=2, h=8)),
     ("blend", dict(d16=1, w=8, h=1))] +
    [("blend", dict(w=w, h=h, ms=600)) for w, h in BAD_POW2] +
    [("diffwtd", dict(w=w, h=h)) for w, h in BAD_POW2 + [(2, 8), (8, 2)]] +
    [("diffwtd", dict(bd=10)), ("diffwtd", dict(highbd=1, bd=11)), ("diffwtd", dict(d16=1, bd=9)),
     ("diffwtd", dict(d16=1, cp=False)), ("diffwtd", dict(d16=1, r0=9, r1=7)),
     ("diffwtd", dict(mask=False))] +
    [("wsrc", dict(bw=w, bh=h)) for w, h in BAD_OBMC] +
    [("wsrc", dict(tab=False)), ("wsrc", dict(wsrc=False))] +
    [("oblend", dict(bw=w, bh=h)) for w, h in BAD_OBMC] +
    [("oblend", dict(tab=False)), ("oblend", dict(dst=False)), ("oblend", dict(ssx=2)),
     ("oblend", dict(ssy=-1))] +
    [("wedge", dict(kind=k)) for k in (-1, 3)] +
    [("wedge", dict(a=False)), ("wedge", dict(out=False)), ("wedge", dict(kind=0, b=False)),
     ("wedge", dict(kind=1, b=False)), ("wedge", dict(kind=1, m=False)),
     ("wedge", dict(kind=2, m=False))])
FUNCS = {"blend": "lavish_blend_a64_batch", "diffwtd": "lavish_diffwtd_mask_batch",
         "wsrc": "lavish_obmc_wsrc_batch", "oblend": "lavish_obmc_blend_batch",
         "wedge": "lavish_wedge_batch"}


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
    assert getattr(L, FUNCS[which])(*getattr(a, which)(njobs=-3)) == 0


# ---------------------------------------------------------------- kernels --
def test_new_kernels_use_no_scratch():
    """Code-object metadata (tools/kernel_resources.py) of every instantiation
    of the kernels of blend.hip: no scratch, no spilled VGPR, and at most
    128 VGPRs (four waves per SIMD)."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler") or \
            shutil.which("c++filt") is None:
        pytest.skip("ROCm code-object tools not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    res = KR.kernel_resources(os.path.join(ROOT, "aom-av1-lavish_amd", "liblavish_hip.so"))
    names = sorted(res)
    kinds = ("::blend_kernel<", "::diffwtd_kernel<", "::obmc_wsrc_kernel<", "::obmc_blend_kernel<",
             "::wedge_kernel(")
    mine = [(d, res[n]) for n, d in zip(names, KR.demangled(names)) if any(k in d for k in kinds)]
    assert len(mine) == 3 + 2 + 2 + 2 + 1, [d for d, _ in mine]
    for name, v in mine:
        assert v.get("private_segment_fixed_size", 0) == 0, (name, v)
        assert v.get("vgpr_spill_count", 0) == 0, (name, v)
        assert v.get("vgpr_count", 0) <= 128, (name, v)
