"""The motion searches on tied, saturated and high-lambda inputs, CPU side:
the oracle (oracle/oracle_mcomp.c, oracle_subpel.c) against
av1_full_pixel_search and av1_find_best_sub_pixel_tree{,_pruned,_pruned_more}
executed from the reference (tests/golden/fix_mcomp_extremes.npz, made by
tests/golden/gen_fix_mcomp_extremes.py), bit for bit on every row; and the
conditions that make the content of tests/_mvextremes.py what it claims to be
-- exact ties, saturated sums, rate * error_per_bit past 2^31, starts on the
sub-pel limits.  These are conditions of the inputs, not measurements."""
import numpy as np
import pytest

import _mvextremes as X
import _oracle as O


@pytest.fixture(scope="module")
def F():
    return X.load_fixture()


@pytest.fixture(scope="module")
def tables():
    from lavish_dsp import motion as M
    return {hp: M.default_mv_cost_tables(hp) for hp in (0, 1)}


def test_fixture_is_the_builders(F):
    """The stored planes, jobs and parameters are what _mvextremes builds
    today (the GPU tests take their frames from the same builders)."""
    fp = X.fixture_fullpel()
    groups = list(X.fixture_groups(F, "fp"))
    assert [g.name for g in groups] == [c.name for c in fp]
    n = 0
    for g, c in zip(groups, fp):
        src, refs = X.planes(c.kind, c.bw, c.bh)
        np.testing.assert_array_equal(g.src, src)
        np.testing.assert_array_equal(g.refs, refs)
        np.testing.assert_array_equal(g.jobs, c.jobs, err_msg=c.name)
        p = g.params
        assert (g.kind, g.bw, g.bh) == (c.kind, c.bw, c.bh)
        assert (X.FP_METHODS[p["method"]], p["use_cl"], p["cost"], p["skip"], p["step_param"],
                p["error_per_bit"], p["sad_per_bit"], (p["ref_mv_row"], p["ref_mv_col"]),
                p["hp_tables"]) == tuple(c.params), c.name
        n += len(c.jobs)
    assert n == len(F["fp_rows"]) and 250 <= n <= 350
    assert 120 <= len(F["sp_rows"]) <= 250
    used = {(X.FP_METHODS[g.params["method"]], g.params["cost"]) for g in groups}
    assert {m for m, _ in used} == set(X.FP_METHODS)
    assert {c for _, c in used} == {X.ENTROPY, X.L1, X.NONE}
    assert {g.params["skip"] for g in groups} == {0, 1} == {g.params["use_cl"] for g in groups}
    sp = list(X.fixture_groups(F, "sp"))
    assert {X.SUBPEL_METHODS[g.params["method"]] for g in sp} == set(X.SUBPEL_METHODS)
    assert {g.params["use_cl"] for g in sp} == {0, 1}


def oracle_fullpel(g, tables):
    p = g.params
    mvj, mvc = tables[p["hp_tables"]]
    return O.full_pixel_search_batch(
        g.src.reshape(-1), g.refs.reshape(-1), X.STRIDE, g.bw, g.bh, g.jobs,
        X.FP_METHODS[p["method"]], p["step_param"], p["cost"], p["sad_per_bit"],
        p["error_per_bit"], mvj, mvc, skip=bool(p["skip"]), cost_list=bool(p["use_cl"]))


def oracle_subpel(g, tables):
    p = g.params
    mvj, mvc = tables[p["allow_hp"]]
    cl = (np.ascontiguousarray(g.rows[:, g.J["cl0"]:g.J["cl4"] + 1].astype(np.int32))
          if p["use_cl"] else None)
    return O.subpel_search_batch(
        g.src.reshape(-1), g.refs.reshape(-1), X.STRIDE, g.bw, g.bh, g.jobs, p["method"],
        p["forced_stop"], bool(p["allow_hp"]), p["iters_per_step"], p["cost"],
        p["error_per_bit"], mvj, mvc, cl, search_type=p["search_type"])


def test_oracle_fullpel_vs_reference(F, tables):
    n = 0
    for g in X.fixture_groups(F, "fp"):
        res, cl = oracle_fullpel(g, tables)
        msg = "%s %s %dx%d %r" % (g.name, g.kind, g.bw, g.bh, g.params)
        np.testing.assert_array_equal(res["best_row"], g.rows[:, g.J["best_row"]], err_msg=msg)
        np.testing.assert_array_equal(res["best_col"], g.rows[:, g.J["best_col"]], err_msg=msg)
        np.testing.assert_array_equal(res["bestsme"], g.rows[:, g.J["var"]], err_msg=msg)
        if g.params["use_cl"]:
            np.testing.assert_array_equal(cl, g.rows[:, g.J["cl0"]:g.J["cl4"] + 1], err_msg=msg)
        n += len(g.rows)
    assert n == len(F["fp_rows"])


def test_oracle_subpel_vs_reference(F, tables):
    n = 0
    for g in X.fixture_groups(F, "sp"):
        res = oracle_subpel(g, tables)
        msg = "%s %s %dx%d %r" % (g.name, g.kind, g.bw, g.bh, g.params)
        for f in ("best_row", "best_col", "besterr", "distortion", "sse"):
            np.testing.assert_array_equal(res[f].astype(np.int64), g.rows[:, g.J[f]],
                                          err_msg=msg + " " + f)
        n += len(g.rows)
    assert n == len(F["sp_rows"])


# ------------------------------------------------------------ preconditions --
def _facts(F, prefix):
    out = {}
    for g in X.fixture_groups(F, "fp"):
        if g.kind.startswith(prefix):
            for name, (n, bad) in X.tie_facts(g.kind, g.bw, g.bh, g.jobs).items():
                a, b = out.get(name, (0, 0))
                out[name] = (a + n, b + bad)
    return out


def test_flat_sites_tie(F):
    """flat: the 8 sites of a step (radius 1 and 8) and the centre of every
    job have one SAD."""
    f = _facts(F, "flat")
    assert f["flat_sites_equal"][0] >= 100 and f["flat_sites_equal"][1] == 0, f


def test_ramp_sites_tie(F):
    """ramp: for every job and every even radius inside its window,
    SAD(+d) == SAD(-d) > 0 along the ramp and SAD == SAD(centre) across it."""
    f = _facts(F, "ramp")
    assert f["ramp_along_pairs_equal"][0] >= 200 and f["ramp_along_pairs_equal"][1] == 0, f
    assert f["ramp_across_equals_centre"][0] >= 200 and f["ramp_across_equals_centre"][1] == 0, f


def test_periodic_multiples_match(F):
    """periodic: every in-window site at a multiple of P (within 32) has SAD 0."""
    f = _facts(F, "periodic")
    assert f["periodic_multiples_match"][0] >= 500 and f["periodic_multiples_match"][1] == 0, f


def test_checker_parity(F):
    f = _facts(F, "checker")
    assert f["checker_parity"][0] >= 60 and f["checker_parity"][1] == 0, f


def test_saturated_sums(F):
    """At least one job per size in {64x64, 128x128} has |sum|^2 >= 2^32 and
    one the largest sse with a zero sum; a 16x16 job reaches sse == 256 *
    65025 -- at the mv the search starts from, and (split: a single-point
    window) returns."""
    big, full_sse, sse16 = set(), set(), 0
    for g in X.fixture_groups(F, "fp"):
        if not g.name.startswith("sat"):
            continue
        s = X.saturation_facts(g.kind, g.bw, g.bh, g.jobs)
        if max(s["sum_sq"]) >= 1 << 32:
            big.add((g.bw, g.bh))
        if max(s["sse"]) == g.bw * g.bh * 65025:
            full_sse.add((g.bw, g.bh))
            if g.kind == "split":   # held at (0, 0): the returned cost is that variance
                assert (g.rows[:, g.J["var"]] >= g.bw * g.bh * 65025).all()
        sse16 += (g.bw, g.bh) == (16, 16) and max(s["sse"]) == 256 * 65025
    assert {(64, 64), (128, 128)} <= big, big
    assert {(64, 64), (128, 128)} <= full_sse, full_sse
    assert sse16 >= 1


def test_high_lambda_product_passes_2_31(F, tables):
    """high-lambda: for every job the reference's rate * error_per_bit at the
    mv it returned is >= 2^31 (int64 from the tables) -- full-pel and sub-pel."""
    n = 0
    for which in ("fp", "sp"):
        for g in X.fixture_groups(F, which):
            if "lambda" not in g.name:
                continue
            p = g.params
            assert p["error_per_bit"] in {e for e, _, _ in X.HIGH_LAMBDA} and p["cost"] == X.ENTROPY
            mvj, mvc = tables[p["hp_tables"] if which == "fp" else p["allow_hp"]]
            scale = 8 if which == "fp" else 1
            rate = X.mv_rate(mvj, mvc, g.rows[:, g.J["best_row"]] * scale,
                             g.rows[:, g.J["best_col"]] * scale,
                             (p["ref_mv_row"], p["ref_mv_col"]))
            assert (rate * p["error_per_bit"] >= 1 << 31).all(), (g.name, rate)
            far = np.minimum(abs(g.jobs["ref_mv_row"]), abs(g.jobs["ref_mv_col"]))
            assert (far >= 60 * 8).all()
            n += len(g.rows)
    assert n >= 50
    assert max(abs(r[0]) for _, r, _ in X.HIGH_LAMBDA) >= 300 * 8


def test_subpel_limit_starts(F):
    """limits: every edge and corner start has a first-level candidate out of
    range (corners two), every edge and corner occurs."""
    n = 0
    for g in X.fixture_groups(F, "sp"):
        if not g.name.startswith("edge"):
            continue
        out = X.limit_facts(g.jobs)
        assert sorted(out) == [1, 1, 1, 1, 2, 2, 2, 2], (g.name, out)
        n += len(out)
    assert n >= 40


def test_degenerate_windows(F):
    """The hand-set windows are a point, a row and a column, inside the
    block's own window (so inside the padded plane)."""
    seen = set()
    for g, c in zip(X.fixture_groups(F, "fp"), X.fixture_fullpel()):
        for mode in ("point", "row", "col"):
            if g.name.startswith(mode):
                j = g.jobs
                one_row, one_col = j["row_min"] == j["row_max"], j["col_min"] == j["col_max"]
                assert one_row.all() == (mode != "col") and one_col.all() == (mode != "row")
                seen.add(mode)
        own = X.frame(g.bw, g.bh, c.params.ref_mv)
        own = {int(o["src_off"]): o for o in own[:len(own) // X.NREF]}
        for j in g.jobs:
            o = own[int(j["src_off"])]
            assert o["row_min"] <= j["row_min"] <= j["row_max"] <= o["row_max"]
            assert o["col_min"] <= j["col_min"] <= j["col_max"] <= o["col_max"]
    assert seen == {"point", "row", "col"}
