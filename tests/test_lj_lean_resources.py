"""Code-object resources of the lean 16x16 DIAMOND search kernel
(diamond_lj_lean_kernel, csrc/mcomp_lj.hip) in the built library, read with
tools/kernel_resources.py: the kernel exists to fit on a SIMD beside four
workgroups of the <= 16-point transform class (txq_multi_kernel<0>), so its
VGPR allocation, scratch and LDS are part of what it computes for."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ceil8(v):  # the VGPR allocation granule
    return (v + 7) & ~7


@pytest.fixture(scope="module")
def kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    res = KR.kernel_resources(os.path.join(ROOT, "aom-av1-lavish_amd", "liblavish_hip.so"))
    names = sorted(res)
    by = {d: res[n] for n, d in zip(names, KR.demangled(names))}

    def one(part):
        hits = [v for k, v in by.items() if part in k]
        assert len(hits) == 1, (part, len(hits))
        return hits[0]

    return one("diamond_lj_lean_kernel<4>"), one("txq_multi_kernel<0>")


def test_lean_kernel_fits_64_vgprs_without_scratch(kernels):
    lean, _ = kernels
    assert ceil8(lean["vgpr_count"]) <= 64, lean
    assert lean.get("agpr_count", 0) == 0, lean
    assert lean["private_segment_fixed_size"] == 0 and lean["vgpr_spill_count"] == 0, lean
    assert lean["group_segment_fixed_size"] <= 7168, lean


def test_lean_wave_fits_beside_four_transform_workgroups(kernels):
    """512 VGPRs per SIMD: one wave of each of four transform workgroups and
    a lean search wave."""
    lean, txq = kernels
    assert 4 * ceil8(txq["vgpr_count"]) + ceil8(lean["vgpr_count"]) <= 512, (txq, lean)
