"""GPU parity of the lean 8-jobs-per-wave DIAMOND search
(diamond_lj_lean_kernel + diamond_lj_redo_kernel, csrc/mcomp_lj.hip;
lavish_set_search_variant(2)) against the oracle's av1_full_pixel_search
(_oracle.full_pixel_search_batch) and against the full kernels
(lavish_set_search_variant(1)): the records (best_row, best_col, bestsme,
steps, searches) and the cost lists, exactly.  The oracle's records carry no
searches count (its fourth word is reserved), so that field is held to
variant 1's, byte for byte with the rest of the record.

16x16 blocks over tiled references with the downsampled SAD; every call runs
twice in a row on one stream into poisoned outputs, so the queue and redo
counters must be re-zeroed by the call itself."""
import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

BORDER = 160
W, H, NREFS = 160, 128, 7          # 80 blocks x 7 references = 560 jobs = 70 wave units
FIELDS = ("best_row", "best_col", "bestsme", "steps")  # (what the oracle's records hold)
ENTROPY, L1, NONE = 0, 1, 4        # MV_COST_ENTROPY, MV_COST_L1_LOWRES, MV_COST_NONE
QINDEX, RDMULT = 120, 30000        # the entropy cost's sad_per_bit / error_per_bit


def redo_planes():
    """motion_planes content where, in every other block of every reference
    (a checkerboard that alternates with the reference), the even rows are
    the source's and the odd rows the source's with every pixel moved by 8
    (bit 3 flipped): the downsampled SAD (even block rows) finds an
    exact match at mv (0, 0) where the full SAD is 1024, so the quality
    recheck sends those jobs to the second pass -- which ends there again,
    still the best full SAD around."""
    import lavish_dsp.synth as synth
    src, refs = synth.motion_planes(W, H, NREFS, BORDER, seed=311)
    refs = refs.copy()
    for k in range(NREFS):
        for by in range(H // 16):
            for bx in range(W // 16):
                if (bx + by + k) & 1:
                    y, x = BORDER + 16 * by, BORDER + 16 * bx
                    blk = src[y:y + 16, x:x + 16]
                    refs[k, y:y + 16:2, x:x + 16] = blk[0::2]
                    refs[k, y + 1:y + 16:2, x:x + 16] = blk[1::2] ^ 0x08
    return src, refs


def second_pass_share(src, refs, jobs, with_skip, without_skip):
    """Bounds on the share of jobs whose downsampled-SAD search failed the
    quality recheck (mcomp.c:1840-1867), from the oracle's results with and
    without use_downsampled_sad.
    lower: the recheck fails at the returned mv -- had the first pass ended
    there, the job would have been sent to the second, so the mv is the
    second pass's.  upper: the second pass is the search without the
    downsampled SAD from the same start, so its jobs return that search's mv
    and cost with more steps than it alone."""
    stride = src.shape[1]
    s, r = src.reshape(-1).astype(np.int64), refs.reshape(-1).astype(np.int64)
    rows = np.arange(16)[:, None] * stride + np.arange(16)[None, :]
    lower = upper = 0
    for jb, t, f in zip(jobs, with_skip, without_skip):
        a = s[int(jb["src_off"]) + rows]
        b = r[int(jb["ref_off"]) + int(t["best_row"]) * stride + int(t["best_col"]) + rows]
        d = np.abs(a - b)
        sad, ssad = int(d.sum()), 2 * int(d[0::2].sum())
        lower += sad > 16 and abs(ssad - sad) * 10 >= max(sad, 1) * 9
        upper += (all(t[k] == f[k] for k in ("best_row", "best_col", "bestsme")) and
                  t["steps"] > f["steps"])
    return lower / len(jobs), upper / len(jobs)


class Env:
    """Device planes, tiles and job sets of one pair of planes; the oracle's
    results per (job set, cost type, step_param), computed once."""

    def __init__(self, src, refs):
        import torch
        import lavish_dsp.motion as M
        self.M, self.torch = M, torch
        self.src, self.refs = src, refs
        self.stride = src.shape[1]
        self.ts, self.tr = torch.from_numpy(src).cuda(), torch.from_numpy(refs).cuda()
        self.tiles = M.RefTiles(self.tr, self.stride).build()
        self.mvj, self.mvc = M.default_mv_cost_tables(False)
        self.spb, self.epb = M.sad_per_bit(QINDEX), M.error_per_bit(RDMULT)
        self.costs = M.MvCosts(self.mvj, self.mvc, device="cuda")
        self.jobsets, self.dev, self.expected = {}, {}, {}

    def jobs(self, name):
        if name not in self.jobsets:
            M = self.M
            if name == "six":       # 48x32 x 1 reference: one unit, two surplus lane groups
                j = M.frame_jobs(48, 32, self.stride, BORDER, self.src.size, 16, 16, 1, (13, -21),
                                 (2, -3))
            elif name.startswith("start"):  # a start mv outside the window (clamped to it)
                st, rmv = {"start_a": ((-900, 700), (0, 0)),
                           "start_b": ((300, -300), (-40, 33))}[name]
                j = M.frame_jobs(W, H, self.stride, BORDER, self.src.size, 16, 16, 2, rmv, st)
            else:  # ("redo": from mv (0, 0), where redo_planes() puts its half matches)
                j = M.frame_jobs(W, H, self.stride, BORDER, self.src.size, 16, 16, NREFS,
                                 (13, -21), (0, 0) if name == "redo" else (2, -3))
                if name == "thirteen":  # a second unit of 5
                    j = j[:13]
            self.jobsets[name] = j
            self.dev[name] = M.to_device(j)
        return self.jobsets[name]

    def oracle(self, name, cost, step_param, skip=True):
        key = (name, cost, step_param, skip)
        if key not in self.expected:
            ent = cost == ENTROPY
            self.expected[key] = O.full_pixel_search_batch(
                self.src.reshape(-1), self.refs.reshape(-1), self.stride, 16, 16, self.jobs(name),
                "diamond", step_param, cost, self.spb if ent else 0, self.epb if ent else 0,
                self.mvj if ent else None, self.mvc if ent else None, skip=skip, cost_list=True,
                threads=8)
        return self.expected[key]

    def run(self, name, cost, step_param, want_cl, variant, cap):
        """One search into poisoned outputs: (record bytes, cost lists or None)."""
        M, torch = self.M, self.torch
        n = len(self.jobs(name))
        out = torch.full((n * M.RESULT_DTYPE.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
        cl = torch.full((n, 5), -7, dtype=torch.int32, device="cuda") if want_cl else None
        cp = (self.costs.cost_params(self.spb, self.epb, M.MV_COST_ENTROPY) if cost == ENTROPY
              else M.l1_cost_params(cost))
        M.set_search_variant(variant)
        M.set_search_workgroup_cap(cap)
        try:
            M.full_pixel_search_batch(self.ts, self.tr, 16, 16, self.dev[name], cp, "diamond",
                                      step_param, True, want_cl, out=out, cost_lists=cl,
                                      tiles=self.tiles)
            torch.cuda.synchronize()
        finally:
            M.set_search_variant(M.SEARCH_VARIANT_AUTO)
            M.set_search_workgroup_cap(0)
        return out.cpu().numpy(), (cl.cpu().numpy() if want_cl else None)

    def check(self, name, cost, step_param, want_cl, cap):
        """Variant 2 twice in a row, against the oracle and against variant 1."""
        M = self.M
        exp, ecl = self.oracle(name, cost, step_param)
        full_out, full_cl = self.run(name, cost, step_param, want_cl, M.SEARCH_VARIANT_FULL, cap)
        for it in range(2):
            got_out, got_cl = self.run(name, cost, step_param, want_cl, M.SEARCH_VARIANT_LEAN, cap)
            msg = "%s cost %d step_param %d cap %d pass %d" % (name, cost, step_param, cap, it)
            res = got_out.view(M.RESULT_DTYPE)
            for f in FIELDS:
                np.testing.assert_array_equal(res[f], exp[f], err_msg=msg + " " + f)
            np.testing.assert_array_equal(got_out, full_out, err_msg=msg + " vs variant 1")
            if want_cl:
                np.testing.assert_array_equal(got_cl, ecl, err_msg=msg + " cost list")
                np.testing.assert_array_equal(got_cl, full_cl, err_msg=msg + " cost list vs 1")


@pytest.fixture(scope="module")
def env():
    import lavish_dsp.synth as synth
    return Env(*synth.motion_planes(W, H, NREFS, BORDER, seed=77))


@pytest.fixture(scope="module")
def redo_env():
    return Env(*redo_planes())


@pytest.mark.parametrize("want_cl", [True, False])
@pytest.mark.parametrize("step_param", [0, 3])
@pytest.mark.parametrize("cost", [ENTROPY, L1, NONE])
def test_lean_frame_capped(env, cost, step_param, want_cl):
    """560 jobs = 70 units = 24 workgroups, capped to 8 or 16: the queue path
    with many units per wave.  The frame's edge blocks' mv windows clip the
    sites at every radius that leaves them."""
    assert len(env.jobs("frame")) == 560
    env.check("frame", cost, step_param, want_cl, 8 if want_cl else 16)


@pytest.mark.parametrize("cost", [ENTROPY, L1, NONE])
def test_lean_frame_uncapped(env, cost):
    """Variant 2 without a cap: the queues cover every unit of the full grid."""
    env.check("frame", cost, 3, True, 0)


@pytest.mark.parametrize("name,njobs", [("six", 6), ("thirteen", 13)])
@pytest.mark.parametrize("cost", [ENTROPY, L1, NONE])
def test_lean_partial_units(env, cost, name, njobs):
    """A unit with surplus lane groups: they repeat the last job and store
    nothing."""
    assert len(env.jobs(name)) == njobs
    env.check(name, cost, 0, True, 0)
    env.check(name, cost, 3, False, 0)


@pytest.mark.parametrize("name", ["start_a", "start_b"])
def test_lean_start_outside_window(env, name):
    """A start mv outside the mv window is clamped to its corner, where the
    window clips the sites on two sides at every radius."""
    env.check(name, L1, 0, True, 8)
    env.check(name, ENTROPY, 3, True, 0)


@pytest.mark.parametrize("cost,step_param,cap", [(NONE, 3, 8), (L1, 0, 16), (ENTROPY, 3, 0)])
def test_lean_redo_list(redo_env, cost, step_param, cap):
    """Jobs whose downsampled-SAD result fails the quality recheck go through
    the redo list: between a quarter and three quarters of the jobs here, by
    the oracle's own results."""
    e = redo_env
    jobs = e.jobs("redo")
    with_skip, _ = e.oracle("redo", cost, step_param)
    without_skip, _ = e.oracle("redo", cost, step_param, skip=False)
    lower, upper = second_pass_share(e.src, e.refs, jobs, with_skip, without_skip)
    print("second-pass share between %.3f and %.3f" % (lower, upper))
    assert 0.25 <= lower <= upper <= 0.75, (lower, upper)
    e.check("redo", cost, step_param, True, cap)
