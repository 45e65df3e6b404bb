"""GPU parity of the C3 DIAMOND full-pixel motion search
(lavish_diamond_search_batch) against the oracle's restatement of
av1_full_pixel_search / full_pixel_diamond / diamond_search_sad
(oracle/oracle_mcomp.c): best mv, returned var cost and the number of
diamond steps must match exactly for every (block, reference) job."""
import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

BORDER = 160


@pytest.fixture(scope="module")
def planes():
    import lavish_dsp.synth as synth
    W, H = 480, 272
    src, refs = synth.motion_planes(W, H, 3, BORDER, seed=77)
    return W, H, src, refs


def _run(M, planes, bw, bh, step_param=0, cost=3, skip=False, ref_mv=(0, 0), start=(0, 0),
         sub=1, method="diamond"):
    import torch
    W, H, src, refs = planes
    stride = src.shape[1]
    jobs = M.frame_jobs(W, H, stride, BORDER, src.size, bw, bh, refs.shape[0], ref_mv, start)
    jobs = jobs[::sub]
    ts = torch.from_numpy(src).cuda()
    tr = torch.from_numpy(refs).cuda()
    got = M.results_numpy(M.diamond_search_batch(ts, tr, bw, bh, M.to_device(jobs), step_param,
                                                 cost, skip, method=method))
    exp = O.diamond_batch(src.reshape(-1), refs.reshape(-1), stride, bw, bh, jobs, step_param,
                          cost, skip, threads=8, method=method)
    for f in ("best_row", "best_col", "bestsme", "steps"):
        np.testing.assert_array_equal(got[f], exp[f], err_msg=f)
    return got


@pytest.fixture(scope="module")
def M():
    import lavish_dsp.motion as M
    return M


@pytest.mark.parametrize("bw,bh", [(16, 16), (8, 8), (32, 32), (64, 64), (4, 4), (16, 8),
                                   (8, 32), (64, 16), (128, 128), (32, 64)])
def test_diamond_sizes(M, planes, bw, bh):
    got = _run(M, planes, bw, bh, sub=1 if bw * bh <= 1024 else 1)
    # the synthetic references are displaced by (3k, -2k): most blocks find it
    assert (np.abs(got["best_row"]) + np.abs(got["best_col"]) > 0).mean() > 0.5


@pytest.mark.parametrize("cost", [1, 2, 3, 4])
def test_diamond_cost_types(M, planes, cost):
    _run(M, planes, 16, 16, cost=cost, ref_mv=(13, -21))


@pytest.mark.parametrize("step_param", [0, 3, 7, 10])
def test_diamond_step_param(M, planes, step_param):
    _run(M, planes, 16, 16, step_param=step_param, start=(2, -3))


@pytest.mark.parametrize("bw,bh", [(16, 16), (32, 32), (8, 16)])
def test_diamond_downsampled_sad(M, planes, bw, bh):
    _run(M, planes, bw, bh, skip=True)


def test_diamond_edges_and_clamped_start(M, planes):
    """Start mvs outside the limits are clamped; blocks on the frame edge
    exercise the per-site range checks (not all_in)."""
    _run(M, planes, 16, 16, start=(-900, 700))
    _run(M, planes, 16, 16, start=(300, -300), ref_mv=(-40, 33))


@pytest.fixture(scope="module")
def tiled16(M, planes):
    """The 16x16 DIAMOND search over tiled references (the form that reaches
    launch_lj, csrc/mcomp_lj.hip) on the module's planes: device buffers, and
    the oracle's results per (cost type, use_downsampled_sad), computed once."""
    import torch
    W, H, src, refs = planes
    stride = src.shape[1]
    jobs = M.frame_jobs(W, H, stride, BORDER, src.size, 16, 16, refs.shape[0], (13, -21), (2, -3))
    # launch_lj's grid: eight jobs per wave, four waves per workgroup, rounded
    # to 8 workgroups -- a cap of 8 must cut it
    nwg = ((((len(jobs) + 7) // 8 + 3) // 4) + 7) & ~7
    assert nwg > 8, nwg
    ts, tr = torch.from_numpy(src).cuda(), torch.from_numpy(refs).cuda()
    tiles = M.RefTiles(tr, ts.stride(0)).build()
    dj = M.to_device(jobs)
    out = torch.empty(len(jobs) * M.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    expected = {}

    def run(cost, skip):
        out.fill_(0x55)
        M.full_pixel_search_batch(ts, tr, 16, 16, dj, M.l1_cost_params(cost), "diamond", 1,
                                  skip, out=out, tiles=tiles)
        torch.cuda.synchronize()
        if (cost, skip) not in expected:
            expected[cost, skip] = O.diamond_batch(src.reshape(-1), refs.reshape(-1), stride, 16,
                                                   16, jobs, 1, cost, skip, threads=8)
        return M.results_numpy(out), expected[cost, skip]

    return run


@pytest.mark.parametrize("queued", [True, False])
@pytest.mark.parametrize("cap", [8, 64, 0])
@pytest.mark.parametrize("cost", [3, 4])  # MV_COST_L1_HDRES, MV_COST_NONE
def test_capped_search_non_entropy_cost(M, tiled16, cost, cap, queued):
    """A capped grid with a cost type that runs no mvcost_dec_kernel: the
    queue counters are cleared by their own launch (lj_queue_zero).  Stale
    counters would leave results unwritten, so each combination runs twice in
    a row into poisoned outputs."""
    M.set_search_workgroup_cap(cap)
    M.set_search_schedule(queued)
    try:
        for it in range(2):
            got, exp = tiled16(cost, True)
            for f in ("best_row", "best_col", "bestsme", "steps"):
                np.testing.assert_array_equal(got[f], exp[f], err_msg="pass %d %s" % (it, f))
    finally:
        M.set_search_workgroup_cap(0)
        M.set_search_schedule(True)


# ---- FAST_BIGDIA (pattern_search) ----

@pytest.mark.parametrize("bw,bh", [(16, 16), (8, 8), (32, 32), (64, 64), (4, 4), (16, 8),
                                   (8, 32), (128, 128), (4, 16)])
def test_bigdia_sizes(M, planes, bw, bh):
    got = _run(M, planes, bw, bh, step_param=6, method="bigdia")
    assert (np.abs(got["best_row"]) + np.abs(got["best_col"]) > 0).mean() > 0.3


@pytest.mark.parametrize("step_param", [0, 6, 8, 9, 10])
def test_bigdia_step_param(M, planes, step_param):
    _run(M, planes, 16, 16, step_param=step_param, start=(3, -2), method="bigdia")


@pytest.mark.parametrize("cost", [1, 2, 3, 4])
def test_bigdia_cost_types_and_skip(M, planes, cost):
    _run(M, planes, 16, 16, step_param=6, cost=cost, ref_mv=(13, -21), skip=True,
         method="bigdia")


def test_bigdia_edges(M, planes):
    _run(M, planes, 16, 16, step_param=6, start=(-900, 700), method="bigdia")
    _run(M, planes, 32, 32, step_param=8, start=(300, -300), ref_mv=(-40, 33), method="bigdia")


# ---- NSTEP / NSTEP_8PT (diamond_search_sad over the nstep sites) ----

# (bw, bh, use_downsampled_sad): one row per lane (4x4, 8x8), 16x8, the largest
# block whose source stays in VGPRs (64x16), the smallest that re-reads it
# through L2 (32x64); the downsampled SAD where it applies
NSTEP_SHAPES = [(4, 4, False), (8, 8, False), (16, 8, False), (64, 16, False), (32, 64, False),
                (16, 16, True), (32, 64, True)]
NSTEP_JOBS = 320  # per batch: a few seconds with the oracle


def nstep_jobs(M, planes, bw, bh):
    """Starts in the interior and starts clamped onto a limit, every
    reference, sub-sampled evenly over the frame."""
    W, H, src, refs = planes
    sets = [M.frame_jobs(W, H, src.shape[1], BORDER, src.size, bw, bh, refs.shape[0], (13, -21),
                         start) for start in ((2, -3), (-900, 700), (300, -300))]
    return np.concatenate([j[::max(1, 3 * len(j) // NSTEP_JOBS)] for j in sets])


@pytest.mark.parametrize("step_param", [0, 13])
@pytest.mark.parametrize("bw,bh,skip", NSTEP_SHAPES)
@pytest.mark.parametrize("method", ["nstep", "nstep_8pt"])
def test_nstep_steps_and_cost_lists(M, planes, method, bw, bh, skip, step_param):
    """Every record field and the cost lists of the plain NSTEP / NSTEP_8PT
    search against the oracle: `steps` is what a walk can get wrong (the
    equal-radius skip over the 210s, the run loop's num00) while landing on
    the same mv.  step_param 13 leaves NSTEP two steps."""
    import torch
    W, H, src, refs = planes
    jobs = nstep_jobs(M, planes, bw, bh)
    mvj, mvc = M.default_mv_cost_tables(False)
    spb, epb = M.sad_per_bit(128), M.error_per_bit(1 << 14)
    exp, ecl = O.full_pixel_search_batch(src.reshape(-1), refs.reshape(-1), src.shape[1], bw, bh,
                                         jobs, method, step_param, 0, spb, epb, mvj, mvc,
                                         skip=skip, cost_list=True, threads=8)
    if step_param == 0:
        # the equal-radius skip both fires and does not: a degenerate batch
        # (every walk alike) would pass without exercising it
        assert len(np.unique(exp["steps"])) >= 3, np.unique(exp["steps"])
    cost = M.MvCosts(mvj, mvc).cost_params(spb, epb)
    out, cl = M.full_pixel_search_batch(torch.from_numpy(src).cuda(), torch.from_numpy(refs).cuda(),
                                        bw, bh, M.to_device(jobs), cost, method, step_param, skip,
                                        cost_list=True)
    got = M.results_numpy(out)
    for f in ("best_row", "best_col", "bestsme", "steps"):
        np.testing.assert_array_equal(got[f], exp[f], err_msg=f)
    np.testing.assert_array_equal(cl.cpu().numpy(), ecl)
