"""CPU tests (no GPU) of the host-side facts the kernels' input edges rest
on: the scaled convolution's blocks-per-workgroup formula, the range
certificate of the FAST transform arithmetic (tools/range_analysis.py) and
the quantizer rows lavish_build_quant_params makes against the conditions
the fp fast forms assume."""
import os
import sys

import numpy as np
import pytest

import _fastpath as FP
import _oracle as O

sys.path.insert(0, os.path.join(FP.ROOT, "tools"))


def _scale_nb(w, h):
    # scale_batch's blocks per workgroup (csrc/scale.hip, "a.nb = ..."): the
    # largest power of two n <= 16 with n w h <= 256, one for larger blocks
    nb = 1
    while nb < 16 and 2 * nb * w * h <= 256:
        nb *= 2
    return nb


def test_scale_blocks_per_workgroup_divides():
    """The kernel gives each block slot 256 / nb threads: nb must divide 256
    and the slots' pixels must fit the workgroup, for every accepted shape (w
    a power of two in 2 .. 128, any h in 1 .. 128).  The earlier min(16, 256 /
    (w h)) failed the first at e.g. 8x3 (nb 10): threads 250 .. 255 fell into
    an eleventh slot."""
    for w in (2, 4, 8, 16, 32, 64, 128):
        for h in range(1, 129):
            nb = _scale_nb(w, h)
            assert 256 % nb == 0 and 1 <= nb <= 16, (w, h, nb)
            assert nb * w * h <= 256 or nb == 1, (w, h, nb)
            # never fewer than half the slots the plain quotient allowed
            assert 2 * nb > min(16, max(256 // (w * h), 1)), (w, h, nb)
    assert _scale_nb(16, 16) == 1 and _scale_nb(8, 3) == 8 and _scale_nb(4, 4) == 16


def _size_of(W, H):
    return [s for s in range(19) if O.TX_W[s] == W and O.TX_H[s] == H][0]


def test_fast_range_certificate():
    """tools/range_analysis.py at T = kFastResidualMax (parsed from
    quant_dev.h): every multiply operand of the FAST path fits 24 bits, every
    32-bit sum fits, the coefficient bound is below 2^19 (rdo_kern.h's CHEAP
    and block-error forms) and 2^21 (quant_dev.h's F24 forms), and the
    oracle's coefficients over the adversarial sign patterns stay inside the
    bound."""
    import range_analysis as RA
    T = FP.fast_residual_max()
    for (W, H) in RA.SHIFT:
        op, sm = RA.analyse(W, H, T)
        cb = RA.coeff_bound(W, H, T)
        assert op < 2 ** 23, (W, H, op)
        assert sm < 2 ** 31, (W, H, sm)
        assert cb < 2 ** 19 and cb < 2 ** 21, (W, H, cb)
        s = _size_of(W, H)
        n = O.max_eob(s)
        worst = 0
        for t in range(16):
            if not O.type_valid(s, t):
                continue
            for b in FP.adversarial_blocks(s, t, T):
                worst = max(worst, int(np.abs(O.fwd_txfm2d(b, t, s)[:n]).max()))
        assert worst <= cb, (W, H, worst, cb)
        assert worst >= T << 4, (W, H, worst)  # the set is not idle: DC alone is ~32 T at 4x4


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_built_fp_params_meet_fast_form_conditions(bd):
    """Every fp row of lavish_build_quant_params has quant >= 0, dequant > 0
    and quant * dequant <= 2^16 (quant_fp = 2^16 / dequant): the batch entry
    points' parameter check (quant_fp_params_ok, csrc/lavish_internal.h)
    refuses nothing av1_build_quantizer makes."""
    import lavish_dsp
    for q in range(256):
        for sharp in (0, 3):
            d = lavish_dsp.build_quant_params(bd, q, lavish_dsp.QUANT_FP, sharp).as_dict()
            qt, dq = d["quant"].astype(np.int64), d["dequant"].astype(np.int64)
            assert (qt >= 0).all() and (dq > 0).all(), (bd, q, d)
            assert (qt * dq <= 1 << 16).all(), (bd, q, d)
            assert (qt * dq > 1 << 15).all() or q == 0, (bd, q, d)
