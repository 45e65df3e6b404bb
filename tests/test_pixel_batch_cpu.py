"""CPU pin of tests/_pixref.py, the expected values of test_gpu_pixel_batch.py
(no GPU):
* every function of _pixref equals every matching case of
  tests/golden/fix_pixel.npz (the reference's own `_c` outputs), bit for bit;
* and the C oracle on the seeded planes, job lists, edge blocks, residual
  planes and coefficient rows the GPU module runs on;
* the preconditions of the GPU module hold on those inputs: the saturating
  8-bit job, a negative variance before the clamp at 10 / 12 bits in every
  job list, odd offsets, sums of both signs, int16 wraps in the Hadamard
  inputs."""
import os

import numpy as np
import pytest

import _oracle as O
import _pixref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUBPEL_OFFSETS = [(0, 0), (3, 0), (0, 5), (4, 4), (7, 2)]
JOB_DTYPE = np.dtype([("src_off", "<i8"), ("ref_off", "<i8", (4,)), ("aux_off", "<i8"),
                      ("xoff", "<i4"), ("yoff", "<i4")], align=True)


def view(flat, off, h, w, stride=R.PW):
    """The (h + 1) x (w + 1) strided view of a flat plane at an element offset."""
    a = flat[off:]
    return np.lib.stride_tricks.as_strided(a, (h + 1, w + 1), (stride * a.itemsize, a.itemsize))


@pytest.fixture(scope="module")
def FP():
    return dict(np.load(os.path.join(GOLD, "fix_pixel.npz")))


def test_job_record_is_the_library_one():
    import lavish_dsp.pixel as P
    assert P.JOB_DTYPE == JOB_DTYPE


# ---------------------------------------------------------------- fixture --
@pytest.mark.parametrize("W,H", R.SIZES)
@pytest.mark.parametrize("bd", [8, 10])
def test_sad_variance_equal_the_fixture(FP, W, H, bd):
    k = "%dx%d_bd%d" % (W, H, bd)
    a, b = FP["src_" + k], FP["ref_" + k]
    A, B = a[:H, :W], b[:H, :W]
    assert R.sad(A, B) == FP["sad_" + k][0]
    assert R.sad_skip(A, B) == FP["sadskip_" + k][0]
    got4 = R.sad(A[None], R.windows(b, [0, 1, 3, W + 2], H, W))
    np.testing.assert_array_equal(got4, FP["sadx4d_" + k])
    assert list(R.variance(A, B, bd)[:2]) == list(FP["var_" + k])
    got = [R.sub_pixel_variance(a[:H + 1, :W + 1], xo, yo, B, bd, bd > 8)[:2]
           for xo, yo in SUBPEL_OFFSETS]
    np.testing.assert_array_equal(np.array(got, np.int64), FP["subvar_" + k])
    # the same five as one stack with per-block offsets
    xs, ys = zip(*SUBPEL_OFFSETS)
    st = R.sub_pixel_variance(np.stack([a[:H + 1, :W + 1]] * 5), xs, ys, np.stack([B] * 5), bd,
                              bd > 8)
    np.testing.assert_array_equal(np.stack(st[:2], 1), FP["subvar_" + k])


def test_hadamard_satd_equal_the_fixture(FP):
    seen = 0
    for n in (4, 8, 16, 32):
        for bd in (8, 10):
            k = "%d_bd%d" % (n, bd)
            if "had_" + k not in FP:
                continue
            res = FP["hres_" + k][:, :n]
            got = R.hadamard(res, n, highbd=bd > 8)
            np.testing.assert_array_equal(got, FP["had_" + k], err_msg=k)
            assert R.satd(got) == FP["satd_" + k][0]
            seen += 1
            if "hadlp_" + k in FP:
                lp = R.hadamard_lp(res, n)
                np.testing.assert_array_equal(lp, FP["hadlp_" + k], err_msg=k)
                assert R.satd_lp(lp) == FP["satdlp_" + k][0]
                seen += 1
    assert seen == 4 + 3 + 2


def test_block_error_equals_the_fixture(FP):
    for n in (16, 64, 256, 1024, 4096):
        c, d = FP["be_c_%d" % n], FP["be_d_%d" % n]
        assert list(R.block_error(c, d)) == list(FP["be_%d" % n])
        for bd in (10, 12):
            assert list(R.block_error(c, d, bd)) == list(FP["behb_%d_bd%d" % (n, bd)])
        assert R.block_error_lp(FP["belp_c_%d" % n], FP["belp_d_%d" % n]) == FP["belp_%d" % n][0]


def test_subtract_sse_sums_equal_the_fixture(FP):
    for (w, h) in ((4, 4), (8, 4), (16, 16), (7, 5), (64, 64), (32, 8), (128, 128)):
        for bd in (8, 10):
            k = "%dx%d_bd%d" % (w, h, bd)
            src, prd = FP["s_src_" + k][:, :w], FP["s_pred_" + k][:, :w]
            exp = FP["sub_" + k]
            diff = R.subtract(src, prd)
            assert diff.dtype == np.int16
            np.testing.assert_array_equal(diff, exp[:, :w], err_msg=k)
            assert R.sse(src, prd) == FP["sse_" + k][0]
            assert R.sum_squares_2d_i16(diff) == FP["sumsq_" + k][0]
            assert list(R.sum_sse_2d_i16(diff)) == list(FP["sumsse_" + k])
            assert list(R.get_blk_sse_sum(diff)) == list(FP["blksse_" + k])
    assert R.sum_sse_2d_i16(np.full((4, 4), 3), sum_in=-50) == (144, -2)


# ----------------------------------------------------------------- oracle --
ALL_SHAPES = R.SIZES + [(12, 8), (20, 36)]


@pytest.mark.parametrize("w,h", ALL_SHAPES)
@pytest.mark.parametrize("bd,hb", R.CONFIGS)
def test_sad_variance_equal_the_oracle_on_the_seeded_jobs(w, h, bd, hb):
    """Every job of the list the GPU module runs, edge blocks included."""
    B = R.Planes(w, h, bd, hb, JOB_DTYPE)
    j = B.jobs
    S, Sw, P2 = B.S(), B.S(dw=1), B.P2()
    fs, fr = B.src.reshape(-1), B.ref.reshape(-1)
    refs = [B.R(k=k) for k in range(4)]
    want = {"sad": [R.sad(S, r) for r in refs], "skip": [R.sad_skip(S, r) for r in refs],
            "avg": [R.sad_avg(S, r, P2) for r in refs]}
    var = {8: R.variance(S, refs[0], 8), bd: R.variance(S, refs[0], bd)}
    sse = R.sse(S, refs[0])
    sub = R.sub_pixel_variance(Sw, j["xoff"], j["yoff"], refs[0], bd, hb)
    sav = R.sub_pixel_variance(Sw, j["xoff"], j["yoff"], refs[0], bd, hb, P2)
    assert B.nj == R.max_jobs(w, h)
    for i in range(B.nj):
        a = view(fs, j["src_off"][i], h, w)
        sec = B.second[j["aux_off"][i]:]
        for k in range(4):
            b = view(fr, j["ref_off"][i, k], h - 1, w - 1)
            assert want["sad"][k][i] == O.sad(a, R.PW, b, R.PW, w, h, hb)
            assert want["avg"][k][i] == O.sad(a, R.PW, b, R.PW, w, h, hb, second_pred=sec)
            if h % 2 == 0:
                assert want["skip"][k][i] == O.sad(a, R.PW, b, R.PW, w, h, hb, skip=True)
        b = view(fr, j["ref_off"][i, 0], h - 1, w - 1)
        v, s, sm = (x[i] for x in var[bd])
        assert (v, s) == O.variance(a, R.PW, b, R.PW, w, h, bd, hb)
        assert (s, s) == O.mse(a, R.PW, b, R.PW, w, h, bd, hb)
        assert (s, sm) == O.get_var(a, R.PW, b, R.PW, w, h, bd, hb)
        assert sse[i] == O.sse(a, R.PW, b, R.PW, w, h, hb)
        xo, yo = int(j["xoff"][i]), int(j["yoff"][i])
        assert (sub[0][i], sub[1][i]) == O.sub_pixel_variance(a, R.PW, xo, yo, b, R.PW, w, h, bd,
                                                              hb)
        assert (sav[0][i], sav[1][i]) == O.sub_pixel_variance(a, R.PW, xo, yo, b, R.PW, w, h, bd,
                                                              hb, sec)


@pytest.mark.parametrize("w,h", ALL_SHAPES)
@pytest.mark.parametrize("bd,hb", R.CONFIGS)
def test_job_lists_hold_what_the_gpu_module_relies_on(w, h, bd, hb):
    B = R.Planes(w, h, bd, hb, JOB_DTYPE)
    j, n = B.jobs, w * h
    assert (j["src_off"] & 1).any() and (j["ref_off"][:, 0] & 1).any()
    assert j["src_off"][0] & 1 and j["ref_off"][0, 0] & 1  # also in the one-job prefix
    assert (j["aux_off"] & 1).all()
    assert {(x, y) for x, y in zip(j["xoff"], j["yoff"])} >= {(x, y) for x in range(8)
                                                              for y in range(8)}
    # every address a kernel may form lies inside the planes
    assert j["src_off"].max() + h * R.PW + w + 1 <= B.src.size
    assert j["ref_off"].max() + (h - 1) * R.PW + w <= B.ref.size
    assert j["aux_off"].max() + n <= B.second.size
    v, s, sm = R.variance(B.S(), B.R(), bd)
    assert (sm < 0).any() and (sm > 0).any()
    mx = (1 << bd) - 1
    e, f = R.J_MAX0, R.J_0MAX
    sh, ss = {8: (0, 0), 10: (2, 4), 12: (4, 8)}[bd]
    assert (s[e], sm[e]) == (((n * mx * mx + ((1 << ss) >> 1)) >> ss) & R.M32,
                             (n * mx + ((1 << sh) >> 1)) >> sh)
    assert (s[f], sm[f]) == (s[e], (-n * mx + ((1 << sh) >> 1)) >> sh)
    assert s[R.J_MAX0_B] == s[e]
    assert R.sad(B.S(), B.R())[R.J_CHECK] == (n // 2) * mx
    if bd > 8:
        assert B.neg is not None
        for q in (R.J_NEG, R.J_NEG_B):
            if q < B.nj:
                assert R.before_clamp(s[q], sm[q], n) < 0 and v[q] == 0, (B.neg, s[q], sm[q])
    # the last job of the 67- and of the 259-job prefix is an edge block too
    assert B.nj in (67, 259) and (R.J_MAX0_B, R.J_NEG_B) == (67 - 1, 259 - 1)


def test_the_saturating_8_bit_job():
    """128x128 all-255 against all-0: sse = 16384 * 65025 (below 2^32, while
    a.a alone is, and 2 a.b would be, beyond what a narrower sum holds)."""
    B = R.Planes(128, 128, 8, False, JOB_DTYPE)
    v, s, sm = R.variance(B.S(1), B.R(1), 8)
    assert s[0] == 16384 * 65025 and sm[0] == 16384 * 255
    a = view(B.src.reshape(-1), B.jobs["src_off"][0], 128, 128)
    b = view(B.ref.reshape(-1), B.jobs["ref_off"][0, 0], 127, 127)
    assert O.get_var(a, R.PW, b, R.PW, 128, 128) == (16384 * 65025, 16384 * 255)
    assert sm[0] > 0 and v[0] == (s[0] - (16384 * 255) ** 2 // 16384) & R.M32 == 0
    v, s, sm = R.variance(B.R(1), B.S(1), 8)
    assert (v[0], s[0], sm[0]) == (0, 16384 * 65025, -16384 * 255)


def test_blocks_with_a_negative_variance_before_the_clamp():
    # 10 bits, 4x4: differences of 2 in two pixels, 3 in fourteen
    d = np.array([2] * 2 + [3] * 14).reshape(4, 4)
    v, s, sm = R.variance(d + 100, np.full((4, 4), 100), 10)
    assert (s, sm, R.before_clamp(s, sm, 16), v) == (8, 12, -1, 0)
    # 12 bits, 4x4: eight differences of 11, eight of 12
    d = np.array([11] * 8 + [12] * 8).reshape(4, 4)
    v, s, sm = R.variance(d + 7, np.full((4, 4), 7), 12)
    assert (s, sm, R.before_clamp(s, sm, 16), v) == (8, 12, -1, 0)
    # and the search finds one for every size
    for w, h in R.SIZES + [(12, 8), (20, 36)]:
        for bd in (10, 12):
            d, k = R.neg_clamp_diffs(w, h, bd)
            blk = np.full(w * h, d)
            blk[:k] += 1
            _, s, sm = R.variance(blk.reshape(h, w), np.zeros((h, w)), bd)
            assert R.before_clamp(s, sm, w * h) < 0, (w, h, bd)
    # at 8 bits the same quantity wraps instead (no clamp)
    assert R.variance_tail(-258, 256 * 16 * 16, 10, 16)[:2] == (4096 - 64 * 64 // 16, 4096)
    assert R.variance_tail(-24, 16 << 8, 12, 16)[:2] == (16, 16)


# ------------------------------------------------- residuals, coefficients --
RES_SHAPES = [(4, 4), (16, 8), (7, 5), (64, 64)]


@pytest.mark.parametrize("kind", ["255", "4095", "wrap"])
def test_residual_kinds_equal_the_oracle(kind):
    plane = R.residual_plane(kind, 5)
    flat, cols = plane.reshape(-1), plane.shape[1]
    for n in (4, 8, 16, 32):
        offs = R.residual_offsets(plane, n, n, 67, n)
        X = R.windows(plane, offs, n, n)
        forms = [("low", R.hadamard(X, n))]
        if n >= 8:
            forms.append(("high", R.hadamard(X, n, highbd=True)))
        if n in (8, 16):
            forms.append(("lp", R.hadamard_lp(X, n)))
        for name, got in forms:
            for i, o in enumerate(offs):
                want = (O.hadamard_lp(n, flat[o:], cols) if name == "lp" else
                        O.hadamard(n, flat[o:], cols, highbd=name == "high"))
                np.testing.assert_array_equal(got[i], want, err_msg="%s %d job %d" % (name, n, i))
    for w, h in RES_SHAPES:
        offs = R.residual_offsets(plane, h, w, 67, w + h)
        X = R.windows(plane, offs, h, w)
        sq, (ss, sm), (bs, b2) = R.sum_squares_2d_i16(X), R.sum_sse_2d_i16(X), R.get_blk_sse_sum(X)
        for i, o in enumerate(offs):
            assert sq[i] == O.sum_squares_2d_i16(flat[o:], cols, w, h)
            assert (sm[i], ss[i]) == O.sum_sse(flat[o:], cols, w, h) == (bs[i], b2[i])


def test_hadamard_inputs_wrap_an_int16_intermediate():
    """The wide and the int16 evaluation differ on the built-in areas of the
    "wrap" plane and agree on the +-255 plane."""
    wrap, low = R.residual_plane("wrap", 5), R.residual_plane("255", 5)
    for n in (4, 8, 16, 32):
        offs = R.residual_offsets(wrap, n, n, 5, n)
        X = R.windows(wrap, offs, n, n)
        assert (X[0] == 32767).all() and (X[1] == -32768).all()
        differ = (R.hadamard(X, n) != R.hadamard(X, n, wide=True)).any(-1)
        assert differ[0] and differ[2], n
        Y = R.windows(low, offs, n, n)
        np.testing.assert_array_equal(R.hadamard(Y, n), R.hadamard(Y, n, wide=True))
    for n in (8, 16):
        X = R.windows(wrap, R.residual_offsets(wrap, n, n, 5, n), n, n)
        assert (R.hadamard_lp(X, n) != R.hadamard_lp(X, n, wide=True)).any(-1)[0]
    # 4x4 of 32767: the first pass stores b0 + b2 = 65534 as -2, the second makes -4 of four -2
    assert R.hadamard(np.full((4, 4), 32767), 4)[0] == -4
    assert R.hadamard(np.full((4, 4), 32767), 4, wide=True)[0] == 2 * 65534


@pytest.mark.parametrize("length", [16, 64, 256, 1024])
def test_coefficient_kinds_equal_the_oracle(length):
    c, d = R.coeff_rows(length, 67, length)
    assert (np.abs(c.astype(np.int64)) >= 1 << 16).any(1).all()
    low, wide = R.block_error(c, d), R.block_error(c, d, 8)
    assert (low[0] != wide[0]).any() and (low[1] != wide[1]).any()  # the int squares wrap
    sat = R.satd(c)
    hb = {bd: R.block_error(c, d, bd) for bd in (8, 10, 12)}
    for i in range(67):
        assert sat[i] == O.satd(c[i], length)
        assert (low[0][i], low[1][i]) == O.block_error(c[i], d[i], length)
        for bd in (8, 10, 12):
            assert (hb[bd][0][i], hb[bd][1][i]) == O.block_error(c[i], d[i], length, bd)
    c, d = R.coeff_rows_lp(length, 67, length)
    exact = ((c.astype(np.int64) - d) ** 2).sum(1)
    lp, sat = R.block_error_lp(c, d), R.satd_lp(c)
    assert (lp != exact).any() and int(c.min()) == -32768 and int(c.max()) == 32767
    for i in range(67):
        assert lp[i] == O.block_error_lp(c[i], d[i], length)
        assert sat[i] == O.satd_lp(c[i], length)


def test_subtract_equals_the_oracle_on_the_seeded_jobs():
    for bd, hb in R.CONFIGS:
        for w, h in RES_SHAPES:
            B = R.Planes(w, h, bd, hb, JOB_DTYPE, njobs=67)
            got = R.subtract(B.S(), B.R())
            fs, fr = B.src.reshape(-1), B.ref.reshape(-1)
            for i in range(0, 67, 6):
                diff = np.zeros((h, w), np.int16)
                O.subtract_block(h, w, diff, w, fs[B.jobs["src_off"][i]:], R.PW,
                                 fr[B.jobs["ref_off"][i, 0]:], R.PW, highbd=hb)
                np.testing.assert_array_equal(got[i], diff)
