"""The RTCD boundary against the reference, mechanically (CPU, no GPU):

A. every `av1_*_hip` / `aom_*_hip` prototype of include/lavish_dsp.h has the
   function type of the reference's `_c` prototype of the same name, as the
   reference's own build/cmake/rtcd.pl emits it from aom_dsp_rtcd_defs.pl and
   av1_rtcd_defs.pl for a generic target (gcc's __builtin_types_compatible_p:
   an `int` for a `ptrdiff_t`, an `unsigned` for an `int` or a dropped `const`
   on a pointee is a mismatch);
B. the five structs the shims read a caller's struct through (LavishTxfmParam,
   LavishConvolveParams, LavishInterpFilterParams, LavishDistWtdCompParams,
   LavishNNConfig) have the reference structs' size and, field by field, their
   offsets, sizes and types.

Both run the same machinery on doctored copies of the header and require it
to reject them.  The generated headers and units live in pytest's temporary
directory.  Needs the reference sources: skips where they are absent."""
import re

import pytest

import _rtcd as R

pytestmark = pytest.mark.skipif(not R.have_reference(),
                                reason="reference sources absent (GPU box)")

# `_hip` shims without a `_c` prototype in the reference's RTCD tables, one
# line of reason each.  A name listed here that has a partner fails the test.
NO_RTCD_PARTNER = {
    # hybrid_fwd_txfm.c:315 defines it as a plain function (declared in
    # hybrid_fwd_txfm.h), not through add_proto; it takes BitDepthInfo by value
    "av1_quick_txfm",
}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rtcd")
    return tmp, R.rtcd_headers(tmp)


@pytest.fixture(scope="module")
def pre():
    return R.preprocessed()


def _doctor(pre, name, old, new):
    """`old` -> `new` once, inside the prototype of `name`."""
    m = re.search(r"\b%s\s*\([^()]*\)" % name, pre)
    assert m and m.group(0).count(old) >= 1, (name, old)
    return pre[:m.start()] + m.group(0).replace(old, new, 1) + pre[m.end():]


# ------------------------------------------------------------ A: prototypes --
def test_shim_prototypes_match_reference(ref, pre):
    tmp, c_names = ref
    shared, bad = R.check_prototypes(tmp, pre, c_names)
    assert not bad, "prototype differs from the reference's: %s" % bad
    assert len(shared) >= 1600, len(shared)
    lone = set(R.hip_names(pre)) - c_names
    assert lone == NO_RTCD_PARTNER, (sorted(lone - NO_RTCD_PARTNER),
                                     sorted(NO_RTCD_PARTNER - lone))
    assert not NO_RTCD_PARTNER & c_names


@pytest.mark.parametrize("name,old,new", [
    ("aom_hadamard_8x8_hip", "ptrdiff_t src_stride", "int src_stride"),
    ("aom_subtract_block_hip", "ptrdiff_t pred_stride", "int pred_stride"),
    ("aom_satd_hip", "int length", "unsigned int length"),
    ("aom_sad16x16_hip", "int ref_stride", "unsigned int ref_stride"),
    ("aom_satd_hip", "const int32_t *coeff", "int32_t *coeff"),
    ("aom_sad64x64x4d_hip", "const uint8_t *const ref_ptr[4]", "uint8_t *const ref_ptr[4]"),
    ("av1_block_error_hip", "int64_t av1_block_error_hip", "int av1_block_error_hip"),
    ("av1_inv_txfm_add_hip", "const LavishTxfmParam *", "const LavishConvolveParams *"),
], ids=["ptrdiff-int", "ptrdiff-int-last", "int-unsigned", "int-unsigned-stride", "const-pointee",
        "const-pointee-array", "return-narrowed", "other-struct"])
def test_doctored_prototype_is_rejected(ref, pre, name, old, new):
    """The check of A on a header with one prototype changed: exactly that
    name is reported."""
    tmp, c_names = ref
    if name == "av1_block_error_hip":
        i = pre.index(old)
        bad_pre = pre[:i] + new + pre[i + len(old):]
    else:
        bad_pre = _doctor(pre, name, old, new)
    assert bad_pre != pre
    shared, bad = R.check_prototypes(tmp, bad_pre, c_names, unit="doctored_types.c")
    assert bad == [name[:-4]], bad
    assert len(shared) >= 1600


# --------------------------------------------------------------- B: mirrors --
def test_mirror_structs_match_reference(ref, pre):
    tmp, _ = ref
    assert R.check_mirrors(tmp, pre) == []
    mine = {n: len(f) for n, f in R.structs(pre) if n in R.MIRRORS}
    assert mine == R.reference_field_counts()


def _edit_struct(pre, name, old, new):
    m = re.search(r"typedef\s+struct\s+%s\s*\{[^{}]*\}" % name, pre)
    assert m and old in m.group(0), (name, old)
    return pre[:m.start()] + m.group(0).replace(old, new, 1) + pre[m.end():]


@pytest.mark.parametrize("name,old,new,expect", [
    ("LavishTxfmParam", "uint8_t tx_set_type", "int tx_set_type", "LavishTxfmParam.tx_set_type: size"),
    ("LavishTxfmParam", "uint8_t tx_size", "int8_t tx_size", "LavishTxfmParam.tx_size: type"),
    ("LavishConvolveParams", "int round_0; int round_1;", "int round_1; int round_0;",
     "LavishConvolveParams.round_0: offset"),
    ("LavishInterpFilterParams", "uint16_t taps", "uint32_t taps",
     "LavishInterpFilterParams.taps: size"),
    ("LavishNNConfig", "int num_hidden_nodes[10]", "int num_hidden_nodes[11]",
     "LavishNNConfig.num_hidden_nodes: size"),  # (sizeof stays 232: padding absorbs it)
    ("LavishDistWtdCompParams", "int bck_offset;", "int bck_offset; int extra;",
     "does not compile"),
], ids=["widened", "signedness", "swapped", "widened-padding", "array-length", "added-field"])
def test_doctored_mirror_is_rejected(ref, pre, name, old, new, expect):
    tmp, _ = ref
    flat = " ".join(pre.split())
    bad = _edit_struct(flat, name, old, new)
    diffs = R.check_mirrors(tmp, bad, unit="doctored_mirrors.c")
    assert any(d.startswith(expect) for d in diffs), diffs
