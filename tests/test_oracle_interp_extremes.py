"""The oracle's interpolation restatements on worst-case pixels: every case of
tests/golden/fix_interp_extremes.npz (the reference's av1_convolve_*_sr_c,
av1_dist_wtd_convolve_*_c, av1_convolve_2d_scale_c, av1_warp_affine_c and
their highbd forms, executed on the aligned 0 / max windows of
tests/_extremes.py) through O.convolve_block, O.dist_wtd_convolve,
O.convolve_2d_scale and O.warp_affine, bit-exact; the plain-integer
restatement of the aligned pixel against the stored outputs; and the coverage
the fixture promises, re-checked on the loaded file.  CPU only."""
import numpy as np
import pytest

import _extfix as E
import _extremes as X
import _oracle as O


@pytest.fixture(scope="module")
def F():
    return E.load()


def _oracle_conv(c):
    """(dst, buf) of a conv case through the oracle."""
    fi = [X.kind_filter(c.kind_x), X.kind_filter(c.kind_y)]
    dst, buf = c.dst_in.copy(), c.buf_in.copy()
    if c.unit == E.SCALE:
        O.convolve_2d_scale(c.src, c.src_w, dst, c.w, c.w, c.h, O.interp_table(*fi[0]),
                            O.interp_table(*fi[1]), c.subpel_x_qn, c.x_step_qn, c.subpel_y_qn,
                            c.y_step_qn, E.conv_params(c), buf, c.w, c.bd, c.highbd,
                            src_off=c.off)
        return dst, buf
    fx = O.interp_kernel(*fi[0], c.phase_x)
    fy = O.interp_kernel(*fi[1], c.phase_y)
    if c.unit == E.SINGLE:
        return O.convolve_block(c.src, c.off, c.src_w, c.w, c.h, c.path, fx, fy, c.round_0,
                                c.round_1, c.bd), buf
    O.dist_wtd_convolve(c.path, c.src, c.src_w, dst, c.w, c.w, c.h, fx, fy, E.conv_params(c),
                        buf, c.w, c.bd, c.highbd, src_off=c.off)
    return dst, buf


@pytest.mark.parametrize("unit", [E.SINGLE, E.COMPOUND, E.SCALE], ids=E.UNIT_NAMES)
def test_conv_oracle_matches_reference(F, unit):
    rows = np.flatnonzero(F["conv_rows"][:, 0] == unit)
    assert len(rows) > 600
    for k in rows:
        c = E.conv_case(F, k)
        dst, buf = _oracle_conv(c)
        np.testing.assert_array_equal(dst, c.dst, err_msg="row %d %s" % (k, vars(c)))
        np.testing.assert_array_equal(buf, c.buf, err_msg="row %d buf" % k)


def test_warp_oracle_matches_reference(F):
    for k in range(len(F["warp_rows"])):
        c = E.warp_case(F, k)
        pred, buf = c.pred_in.copy(), c.buf_in.copy()
        O.warp_affine(c.mat, c.ref, c.width, c.height, c.stride, pred, c.p_col, c.p_row,
                      c.p_width, c.p_height, c.p_width, 0, 0, c.bd, int(c.bd > 8),
                      E.conv_params(c), buf, c.p_width, c.prm)
        np.testing.assert_array_equal(pred, c.pred, err_msg="row %d" % k)
        np.testing.assert_array_equal(buf, c.buf, err_msg="row %d buf" % k)
        if c.aligned and c.mode < 2:
            ok, prm = O.get_shear_params(c.mat)
            assert ok and prm == (0, 0, 0, 0)
        elif not c.aligned:
            assert O.get_shear_params(c.mat) == (1, c.prm)


def test_plain_integers_match_reference(F):
    """The aligned pixel restated in unbounded integers equals the stored
    output wherever no intermediate leaves int16, and equals the value with
    int16 intermediates everywhere; the stored window is the aligned one; the
    wrap, negative-intermediate and bound cases the fixture promises exist."""
    seen = {}
    anchors = set()
    J = {n: i for i, n in enumerate(E.CONV_FIELDS)}
    R = F["conv_rows"]
    for k in np.flatnonzero((R[:, J["aligned"]] == 1) & (R[:, J["mode"]] < 2)):
        c = E.conv_case(F, k)
        kx, ky = E.conv_kernels(c)
        v, got = E.conv_anchor(c)
        np.testing.assert_array_equal(v["win"], X.window(kx, ky, c.bd, c.polarity), err_msg=str(k))
        plain = v["final"] & 0xFFFF if c.mode else v["final"]
        if not v["wraps"]:
            assert got == plain, (k, v, got)
        assert got == v["final_i16"] & 0xFFFF, (k, v, got)
        anchors.add((c.w, c.ay, c.ax))
        if c.path != 3 or c.kind_x != c.kind_y or c.phase_x != c.phase_y:
            continue
        name = E.UNIT_NAMES[c.unit]
        if c.kind_x == X.SHARP2 and c.bd > 8 and v["wraps"] and got != plain:
            seen["wrap", name, c.bd] = k
            assert k in F["wrap_rows"]
        if c.kind_x == X.SHARP2 and c.bd == 8 and min(v["ims"]) < 0:
            seen["negative", name] = k
        kn = X.KIND_NAMES[c.kind_x]
        if kn in X.BOUNDS and c.phase_x == X.extreme_phase(c.kind_x) and \
                (max if c.polarity else min)(v["ims"]) == X.BOUNDS[kn][c.bd][c.polarity]:
            seen["bound", kn, name, c.bd, c.polarity] = k
    for name in E.UNIT_NAMES:
        assert ("negative", name) in seen, name
        for bd in (10, 12):
            assert ("wrap", name, bd) in seen, (name, bd)
        for bd in (8, 10, 12):
            for pol in (0, 1):
                for kn in ("SHARP", "REGULAR", "SHARP2"):
                    assert ("bound", kn, name, bd, pol) in seen, (kn, name, bd, pol)
    # the phase-7 case of the issue: 0 where unwrapped arithmetic gives the maximum
    for bd, mx in ((10, 1023), (12, 4095)):
        c = E.conv_case(F, seen["wrap", "single", bd])
        sel = [k for k in F["wrap_rows"] if tuple(R[k][[J[n] for n in (
            "unit", "bd", "phase_x", "polarity", "mode")]]) == (E.SINGLE, bd, 7, 1, 0)]
        assert sel, bd
        c = E.conv_case(F, sel[0])
        v, got = E.conv_anchor(c)
        assert (v["final"], got) == (mx, 0)
    # the anchors rotate: the block's edges, every column mod 4, every row
    for w in (4, 8):
        a = {(y, x) for (bw, y, x) in anchors if bw == w}
        assert {(0, 0), (w - 1, w - 1), (0, w - 1), (w - 1, 0)} <= a
        assert {y for y, x in a} == set(range(w)) and {x for y, x in a} == set(range(w))


def test_warp_plain_integers_match_reference(F):
    seen = set()
    er = X.extreme_warp_row()
    for k in range(len(F["warp_rows"])):
        c = E.warp_case(F, k)
        if not c.aligned or c.mode >= 2:
            continue
        kx, ky = X.WARPED_FILTER[c.row_x], X.WARPED_FILTER[c.row_y]
        win = E.seen_window(c.ref, c.p_row + c.ay, c.p_col + c.ax, kx, ky)
        np.testing.assert_array_equal(win, X.window(kx, ky, c.bd, c.polarity))
        v = X.anchor_values(win, kx, ky, c.bd, c.round_0, c.round_1, c.mode > 0)
        # the reference keeps the warp's intermediate in int32: nothing may wrap
        assert not v["wraps"] and all(0 <= i < 32768 for i in v["ims"]), (k, v)
        assert int((c.buf if c.mode else c.pred)[c.ay, c.ax]) == v["final"], (k, v)
        if c.row_x == c.row_y == er and \
                (max if c.polarity else min)(v["ims"]) == X.BOUNDS["WARP"][c.bd][c.polarity]:
            seen.add((c.bd, c.polarity, c.mode))
    assert seen == {(bd, p, m) for bd in (8, 10, 12) for p in (0, 1) for m in (0, 1)}


def test_coverage(F):
    E.coverage(F["conv_rows"], F["warp_rows"])
    J = {n: i for i, n in enumerate(E.CONV_FIELDS)}
    R = F["conv_rows"]
    # the cross pairs SHARP x SHARP2 and SHARP2 x SHARP, each at its extreme phase
    ps, p2 = X.extreme_phase(X.SHARP), X.extreme_phase(X.SHARP2)
    for bd in (8, 10, 12):
        for kx, ky, px, py in ((X.SHARP, X.SHARP2, ps, p2), (X.SHARP2, X.SHARP, p2, ps)):
            m = ((R[:, J["unit"]] == E.SINGLE) & (R[:, J["bd"]] == bd) & (R[:, J["kind_x"]] == kx)
                 & (R[:, J["kind_y"]] == ky) & (R[:, J["phase_x"]] == px)
                 & (R[:, J["phase_y"]] == py))
            assert set(R[m][:, J["polarity"]]) == {0, 1}
    # copy: the all-max and all-0 blocks, first pass and averaged
    m = (R[:, J["unit"]] == E.COMPOUND) & (R[:, J["path"]] == 0)
    assert {(int(r[J["bd"]]), int(r[J["polarity"]]), int(r[J["mode"]])) for r in R[m]} == \
        {(bd, p, md) for bd in (8, 10, 12) for p in (0, 1) for md in (1, 2, 3)}


def test_helper_table():
    """BOUNDS is what the kernels' tap sums give (DESIGN.md's table)."""
    for name, kind in (("SHARP", X.SHARP), ("REGULAR", X.REGULAR), ("SHARP2", X.SHARP2)):
        k = X.kernel(kind, X.extreme_phase(kind))
        P, N = X.pos_neg(k)
        for bd in (8, 10, 12):
            mx, r0 = (1 << bd) - 1, X.conv_rounds(bd, False)[0]
            assert (X.rpot((1 << (bd + 6)) + N * mx, r0),
                    X.rpot((1 << (bd + 6)) + P * mx, r0)) == X.BOUNDS[name][bd]
    assert X.pos_neg(X.kernel(X.SHARP, X.extreme_phase(X.SHARP))) == (184, -56)
    assert X.pos_neg(X.kernel(X.REGULAR, X.extreme_phase(X.REGULAR))) == (156, -28)
    assert X.pos_neg(X.kernel(X.SHARP2, X.extreme_phase(X.SHARP2))) == (196, -68)
    assert X.pos_neg(X.WARPED_FILTER[X.extreme_warp_row()]) == (175, -47)
