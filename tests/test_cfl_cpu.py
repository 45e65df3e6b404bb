"""The chroma-from-luma layer without a GPU: tests/_cflref.py against every row
of tests/golden/fix_cfl.npz (the reference's own outputs), the fixture's
coverage conditions re-asserted from the committed file, lavish_cfl_joint over
all 33 x 33 pairs against the reference's mapping, the job-table builders' refusals, the batch calls' argument checks (they
return before anything is launched), and the restatement tests/_cflref.py on
inputs whose answer is known by construction."""
import ctypes
import os

import numpy as np
import pytest

import _cflref as R


@pytest.fixture(scope="module")
def K():
    import lavish_dsp.cfl as K
    return K


@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "fix_cfl.npz")))


# ------------------------------------------------------------ the fixture --
def test_restatement_equals_every_getter_row(F):
    rows = [R.getter_row(F, r) for r in F["getter_rows"]]
    bad = [(i, g.getter, g.tx, g.bd) for i, g in enumerate(rows)
           if not np.array_equal(R.getter_expected(g), g.out)]
    assert not bad, bad[:8]
    # every getter at every size; the u8 families at 8 bits, the others at 8 / 10 / 12
    assert {(g.getter, g.tx) for g in rows} == {(n, t) for n in R.GETTERS for t in R.CFL_TX}


def test_restatement_equals_every_block_row(F):
    """cfl_store_block / cfl_store_tx + cfl_predict_block: the AC block from the
    stored luma rectangle alone, then the prediction"""
    bad = []
    for i, r in enumerate(R.block_row(F, row) for row in F["block_rows"]):
        ac = R.ac_block(r.luma, r.sub[0], r.sub[1], r.tx)
        if not np.array_equal(ac, r.ac) or \
                not np.array_equal(R.predict(ac, r.dc, r.alpha_q3, r.bd), r.pred):
            bad.append((i, r.tx, r.bd, r.sub, r.luma.shape))
    assert not bad, bad[:8]
    shapes = [(r.luma.shape[1] >> r.sub[0] < r.w, r.luma.shape[0] >> r.sub[1] < r.h)
              for r in (R.block_row(F, row) for row in F["block_rows"])]
    assert {(True, False), (False, True), (True, True), (False, False)} <= set(shapes)


def test_restatement_equals_every_search_row(F):
    """the estimate, and the costs the reference evaluated at the indices it
    evaluated; its walk looked at exactly the indices the restatement's does"""
    bad = []
    for i, r in enumerate(R.search_row(F, row) for row in F["search_rows"]):
        ac = R.ac_block(r.luma, r.sub[0], r.sub[1], r.tx)
        c, e = R.search(ac, r.src, r.dc, r.tx, r.bd)
        seen = R.walk(c)[1]
        if not np.array_equal(ac, r.ac) or e != r.est or not np.array_equal(seen, r.mask) or \
                not np.array_equal(c[r.mask], r.costs[r.mask]):
            bad.append((i, r.tx, r.bd, r.sub, e, r.est))
    assert not bad, bad[:8]


def test_fixture_coverage_conditions(F):
    assert R.coverage_problems(F) == []
    assert len(F["search_rows"]) >= 42 + 28 and len(F["block_rows"]) >= 42 + 8


def test_joint_over_all_pairs(K, F):
    seen = set()
    for u in range(33):
        for v in range(33):
            got = K.cfl_joint(u, v)
            assert got == R.joint(u, v), (u, v)
            assert got == tuple(int(x) for x in F["joint_map"][u, v]), (u, v)
            valid, aidx, js = got
            assert valid == int((u, v) != (16, 16))
            if valid:
                assert 0 <= js < 8 and 0 <= aidx < 256
                seen.add((aidx, js))
    # (alpha index, joint sign) does not tell a zero alpha's unused magnitude
    # apart, and nothing else: 8 joint signs over 16 x 16, 16 x 1 or 1 x 16
    assert len(seen) == 4 * 256 + 4 * 16
    # the corners by hand (CFL_SIGN_ZERO 0, NEG 1, POS 2; joint = 3 su + sv - 1)
    assert K.cfl_joint(16, 16) == (0, 0, 0)
    assert K.cfl_joint(32, 0) == (1, (15 << 4) + 15, 2 * 3 + 1 - 1)
    assert K.cfl_joint(16, 17) == (1, 0, 0 * 3 + 2 - 1)
    assert K.cfl_joint(15, 16) == (1, 0, 1 * 3 + 0 - 1)
    for bad in ((-1, 0), (33, 0), (0, 33)):
        with pytest.raises(ValueError):
            K.cfl_joint(*bad)


def test_idx_to_alpha_is_idx_minus_16():
    assert [R.idx_to_alpha_q3(i) for i in range(33)] == list(range(-16, 17))


def test_builders_refuse_what_the_kernels_must_not_get(K):
    ok = K.cfl_ac_jobs([0, 40], 16, [16, 8], [1, 6], 1, 1, luma_stride=64, luma_elems=64 * 64)
    assert ok.dtype == np.int64 and ok.shape == (2, 4)
    assert ok.tolist() == [[0, 16, 16, 1], [40, 16, 8, 6]]
    for tx in (4, 11, 12, 17, 18, -1, 19):   # the 64-point sizes and beyond
        with pytest.raises(ValueError):
            K.cfl_ac_jobs(0, 8, 8, tx, 0, 0)
        with pytest.raises(ValueError):
            K.cfl_predict_jobs(0, 0, tx, 0)
        with pytest.raises(ValueError):
            K.cfl_search_jobs(0, 0, 0, tx)
    for a in (-17, 17, 100):
        with pytest.raises(ValueError):
            K.cfl_predict_jobs(0, 0, 0, a)
    assert K.cfl_predict_jobs(0, 0, 0, [-16, 16]).shape == (2, 4)
    for lw, lh in ((6, 8), (8, 2), (0, 8), (8, 36), (40, 8), (-4, 8)):
        with pytest.raises(ValueError):
            K.cfl_ac_jobs(0, lw, lh, 3, 0, 0)
    with pytest.raises(ValueError):   # 16 stored columns for an 8-wide transform
        K.cfl_ac_jobs(0, 16, 8, 1, 0, 0)
    with pytest.raises(ValueError):   # 4:2:0: 32 luma rows store 16, the transform has 8
        K.cfl_ac_jobs(0, 16, 32, 1, 1, 1)
    K.cfl_ac_jobs(0, 16, 16, 1, 1, 1)
    for sub in ((0, 1), (2, 0), (-1, 0)):
        with pytest.raises(ValueError):
            K.cfl_ac_jobs(0, 8, 8, 1, *sub)
    with pytest.raises(ValueError):   # the rectangle leaves its plane
        K.cfl_ac_jobs(64 * 60, 8, 8, 1, 0, 0, luma_stride=64, luma_elems=64 * 64)
    with pytest.raises(ValueError):
        K.cfl_search_jobs(2, 0, 0, 1, ncells=2)
    with pytest.raises(ValueError):
        K.cfl_search_jobs(0, -1, 0, 1)
    with pytest.raises(ValueError):
        K.cfl_predict_jobs(0, 64 * 64 - 8, 1, 0, dst_stride=64, dst_elems=64 * 64)


def test_batch_calls_refuse_bad_arguments_before_launching():
    import lavish_dsp as L
    lib = ctypes.CDLL(L.LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    ac = lib.lavish_cfl_ac_batch
    ac.argtypes = [vp, i32, i64, i32, i32, vp, i32, vp, i32, i32, vp]
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    assert ac(None, 8, 64, 0, 0, None, 0, None, 8, 0, None) == 0      # njobs 0: a no-op
    assert ac(None, 8, 64, 0, 0, p, 1, p, 8, 0, None) == -1
    assert ac(p, 8, 64, 0, 1, p, 1, p, 8, 0, None) == -6              # (sub_x, sub_y) = (0, 1)
    assert ac(p, 8, 64, 2, 0, p, 1, p, 8, 0, None) == -6
    assert ac(p, 8, 64, 0, 0, p, 1, p, 10, 0, None) == -5             # 10 bits on uint8 pixels
    assert ac(p, 8, 64, 0, 0, p, 1, p, 9, 1, None) == -5
    assert ac(p, 2, 64, 0, 0, p, 1, p, 8, 0, None) == -7
    pr = lib.lavish_cfl_predict_batch
    pr.argtypes = [vp, i64, vp, i32, i64, vp, i32, i32, i32, vp]
    assert pr(p, 1, None, 8, 64, p, 1, 8, 0, None) == -1
    assert pr(p, 1, p, 8, 64, p, 1, 12, 0, None) == -5
    assert pr(p, 0, p, 8, 64, p, 1, 8, 0, None) == -7
    se = lib.lavish_cfl_alpha_search_batch
    se.argtypes = [vp, i64, vp, i32, i64, vp, i32, i64, vp, i32, vp, vp, i32, i32, vp]
    assert se(p, 1, p, 8, 64, p, 8, 64, p, 1, None, p, 8, 0, None) == -1
    assert se(p, 1, p, 8, 64, p, 8, 64, p, 1, p, p, 11, 1, None) == -5
    assert se(p, 1, p, 8, 64, p, 8, 8, p, 1, p, p, 8, 0, None) == -7
    assert L.status()[0] == 0


# ------------------------------------------------------ the restatement ----
def test_padding_replicates_the_last_column_then_the_last_row():
    q = np.arange(6).reshape(2, 3) + 1
    got = R.pad(q, 8, 4)
    assert got[:2, :3].tolist() == q.tolist()
    assert (got[0, 3:] == 3).all() and (got[1, 3:] == 6).all()
    assert (got[2:] == got[1]).all()


def test_subsampling_and_average_by_hand():
    luma = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]])
    assert R.subsample(luma, 1, 1).tolist() == [[28, 44], [92, 108]]
    assert R.subsample(luma, 1, 0)[0].tolist() == [12, 28]
    assert R.subsample(luma, 0, 0)[3].tolist() == [104, 112, 120, 128]
    with pytest.raises(AssertionError):
        R.subsample(luma, 0, 1)
    q = np.full((4, 4), 7)
    q[0, 0] = 16                           # sum 121, + 8, >> 4 = 8
    assert R.subtract_average(q)[0, 0] == 8 and R.subtract_average(q)[1, 1] == -1
    # all-maximum luma at 12 bits: the largest q3 and sum, a zero AC
    assert (R.ac_block(np.full((32, 32), 4095), 0, 0, 3) == 0).all()
    assert int(R.subsample(np.full((32, 32), 4095), 0, 0).sum()) == 1024 * 32760


def test_prediction_rounds_away_from_zero_and_clips():
    ac = np.array([[8, -8, 4, -4]])
    assert R.scaled_luma_q0(4, ac).tolist() == [[1, -1, 0, 0]]     # 32/64 rounds to 1, 16/64 to 0
    assert R.scaled_luma_q0(-4, ac).tolist() == [[-1, 1, 0, 0]]
    assert R.predict(np.array([[3200, -3200]]), np.array([[250, 3]]), 16, 8).tolist() == [[255, 0]]
    assert R.predict(np.array([[3200, -3200]]), np.array([[4000, 3]]), 16, 12).tolist() == [[4095, 0]]


def test_the_walk_carries_best_over_and_stops_on_equal_cost():
    c = np.full(33, 1000)
    c[16], c[17], c[18], c[19] = 500, 400, 400, 100      # stops at 18: equal is not lower
    est, seen = R.walk(c)
    assert est == 17 and seen[18] and not seen[19] and seen[15] and not seen[14]
    assert est != int(np.argmin(c))
    # both neighbours lower: 15 beats 16 but not the upward leg's best
    c = np.full(33, 1000)
    c[16], c[17], c[15], c[14] = 500, 300, 400, 350
    assert R.walk(c)[0] == 17
    assert R.walk(c, restart=True)[0] == 14              # what the reference does not do
    c[15], c[14] = 250, 200                              # now the downward leg wins in both
    assert R.walk(c)[0] == 14 and R.walk(c, restart=True)[0] == 14
    c = np.arange(33)[::-1].copy()                       # falls all the way up
    assert R.walk(c)[0] == 32
    assert R.walk(np.arange(33))[0] == 0


def test_a_planted_alpha_costs_nothing_at_every_size_and_depth():
    rng = np.random.default_rng(8)
    for tx in R.CFL_TX:
        for bd in (8, 10, 12):
            luma = R.smooth_luma(rng, min(2 * R.TX_W[tx], 32), min(2 * R.TX_H[tx], 32), bd)
            ac = R.ac_block(luma, 1, 1, tx)
            if np.abs(ac).max() < 64:
                continue
            for alpha in (-16, -5, 0, 9, 16):
                src, dc = R.planted_chroma(rng, ac, alpha, bd, noise=0)
                costs, est = R.search(ac, src, dc, tx, bd)
                assert costs[alpha + 16] == 0, (tx, bd, alpha)   # the prediction is the source
                assert costs[est] <= costs[16] and (est == 16 or costs[est] < costs[16])
