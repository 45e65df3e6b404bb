"""include/lavish_dsp_cfl.h against the reference and against the library (CPU):

* each `cfl_get_*_hip` getter has the function type of the reference's `_c`
  getter of the same name as build/cmake/rtcd.pl emits it (return type, a
  pointer to the size's function, included), checked by gcc's
  __builtin_types_compatible_p in a unit of this test's own; doctored copies of
  the header are rejected;
* the library exports every function the header declares;
* the kernels of csrc/cfl.hip use no scratch and spill nothing.

The first part needs the reference sources and skips where they are absent."""
import ctypes
import os
import re
import sys

import pytest

import _rtcd as R

HEADER = os.path.join(R.ROOT, "include", "lavish_dsp_cfl.h")
GETTERS = ["cfl_get_subtract_average_fn", "cfl_get_predict_lbd_fn", "cfl_get_predict_hbd_fn"] + \
    ["cfl_get_luma_subsampling_%d_%s" % (s, b) for s in (420, 422, 444) for b in ("lbd", "hbd")]
needs_reference = pytest.mark.skipif(not R.have_reference(),
                                     reason="reference sources absent (GPU box)")


def _pre():
    with open(HEADER) as f:
        return R.preprocessed(f.read())


def _check(tmp, pre, unit):
    """names of the getters whose `_c` and `_hip` function types differ"""
    src = R._UNIT_HEAD % "" + pre + "\n"
    for n in GETTERS:
        src += ('_Static_assert(__builtin_types_compatible_p(__typeof__(%s_c), '
                '__typeof__(%s_hip)), "MISMATCH %s");\n' % (n, n, n))
    r = R._compile(tmp, unit, src)
    bad = sorted(set(re.findall(r"MISMATCH (\w+)", r.stderr)))
    other = [l for l in r.stderr.splitlines() if "error" in l and "MISMATCH" not in l]
    assert not other, "\n".join(other[:20])
    assert (r.returncode == 0) == (not bad), r.stderr[-2000:]
    return bad


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rtcd_cfl")
    return tmp, R.rtcd_headers(tmp)


@needs_reference
def test_getters_have_the_reference_types(ref):
    tmp, c_names = ref
    assert set(GETTERS) <= c_names, sorted(set(GETTERS) - c_names)
    assert _check(tmp, _pre(), "cfl_types.c") == []


@needs_reference
@pytest.mark.parametrize("old,new,expect", [
    ("cfl_get_predict_lbd_fn_hip(uint8_t tx_size)", "cfl_get_predict_lbd_fn_hip(int tx_size)",
     ["cfl_get_predict_lbd_fn"]),
    ("(*lavish_cfl_predict_hbd_fn)(const int16_t *src, uint16_t *dst, int dst_stride, int alpha_q3, "
     "int bd)", "(*lavish_cfl_predict_hbd_fn)(const int16_t *src, uint16_t *dst, int dst_stride, "
     "int alpha_q3)", ["cfl_get_predict_hbd_fn"]),
    ("(*lavish_cfl_subtract_average_fn)(const uint16_t *src", "(*lavish_cfl_subtract_average_fn)(uint16_t *src",
     ["cfl_get_subtract_average_fn"]),
], ids=["int-for-TX_SIZE", "returned-type-loses-bd", "returned-type-loses-const"])
def test_doctored_header_is_rejected(ref, old, new, expect):
    tmp, _ = ref
    pre = _pre()
    flat = lambda s: " ".join(s.split())  # noqa: E731
    one = flat(pre)
    assert one.count(flat(old)) == 1, old
    bad_pre = one.replace(flat(old), flat(new)).replace(";", ";\n")
    assert _check(tmp, bad_pre, "cfl_doctored.c") == expect


def _declared():
    body = re.sub(r"typedef[^;]*;", ";", _pre())
    return sorted(set(re.findall(r"\b(cfl_\w+_hip)\s*\(", body)))


def test_library_exports_every_symbol_of_the_header():
    import lavish_dsp as L
    names = _declared()
    assert len(names) == 9 + 14 * (6 + 3), len(names)
    lib = ctypes.CDLL(L.LIB_PATH)   # a handle of this test's own
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    for n in ("lavish_cfl_ac_batch", "lavish_cfl_predict_batch", "lavish_cfl_alpha_search_batch",
              "lavish_cfl_joint", "lavish_cfl_subsample_host", "lavish_cfl_subtract_average_host",
              "lavish_cfl_predict_host"):
        assert hasattr(lib, n), n
    assert set(GETTERS) <= {n[:-4] for n in names}


def test_cfl_kernels_use_no_scratch():
    import lavish_dsp as L
    sys.path.insert(0, os.path.join(R.ROOT, "tools"))
    import kernel_resources as KR
    res = KR.kernel_resources(L.LIB_PATH)
    names = sorted(res)
    mine = {d: res[n] for n, d in zip(names, KR.demangled(names))
            if re.search(r"::(AcArgs|PredArgs|SearchArgs)\)", d or "")}
    # two pixel types each, and the search's exact (12-bit) instantiation
    assert len(mine) == 2 + 2 + 3, sorted(mine)
    for k, v in mine.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
