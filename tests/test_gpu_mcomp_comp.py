"""GPU parity of the compound, masked and OBMC full-pel search batches
(csrc/mcomp_comp.hip through lavish_dsp.motion), every record field compared
with equality, outputs into poisoned buffers:
* every row of tests/golden/fix_mcomp_comp.npz (av1_full_pixel_search with
  second_pred, av1_refining_search_8p_c and av1_obmc_full_pixel_search
  executed from the reference) against the fixture directly;
* the block sizes the fixture cannot reach against tests/_compsearch_ref.py
  (which test_mcomp_comp_cpu.py pins to that fixture): 4x16, 16x4 and 8x32
  (row / word geometry), 32x32 (the last LDS-staged size), 64x64 and 64x16
  (the first that re-read the invariants through L2) and 128x128;
* batch geometry: 1, kDkWaves - 1, kDkWaves + 1 and 80 jobs, a non-default
  stream, the invariant blocks addressed in reversed job order."""
import numpy as np
import pytest

import _compsearch_ref as S
import _mvextremes as X

pytestmark = pytest.mark.gpu

FIELDS = S.RESULT_FIELDS
K_DK_WAVES = 4                       # LAVISH_DK_WAVES: jobs (waves) per workgroup
LOW = (X.LOW_LAMBDA[0], X.LOW_LAMBDA[1], 0)      # (error_per_bit, sad_per_bit, hp tables)
REF_MV = (13, -21)


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.motion as M
    return M


class Dev:
    """Device planes, pools and cost tables, and the restatement's answers,
    each made once."""

    def __init__(self, M):
        import torch
        self.M, self.torch = M, torch
        self.planes, self.memo, self.pools = {}, {}, {}
        self.costs = {hp: M.MvCosts(*M.default_mv_cost_tables(bool(hp)), device="cuda")
                      for hp in (0, 1)}

    def get(self, kind, arrays=None):
        if kind not in self.planes:
            src, refs = arrays if arrays is not None else X.planes(kind)
            self.planes[kind] = (src, refs, self.torch.from_numpy(src.copy()).cuda(),
                                 self.torch.from_numpy(refs.copy()).cuda())
        return self.planes[kind]

    def pool(self, key, arr):
        if key not in self.pools:
            self.pools[key] = self.torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        return self.pools[key]

    def cost(self, ctype, lam=LOW):
        epb, spb, hp = lam
        if ctype == X.ENTROPY:
            return self.costs[hp].cost_params(spb, epb, self.M.MV_COST_ENTROPY)
        return self.M.l1_cost_params(ctype)

    def run(self, search, form, kind, bw, bh, cjobs, ctype, lam, method, sp, fast, P, ms,
            stream=None):
        """One batch call into a poisoned output: COMP_RESULT_DTYPE records.
        P: the host pools {second, mask, wsrc, omask} under a memo key."""
        M, torch = self.M, self.torch
        _, _, ts, tr = self.get(kind)
        pk, pools = P
        d = lambda n: self.pool((pk, n), pools[n])
        out = torch.full((len(cjobs) * M.COMP_RESULT_DTYPE.itemsize,), 0x55, dtype=torch.uint8,
                         device="cuda")
        jobs, cost, name = M.to_device(cjobs), self.cost(ctype, lam), S.METHOD_NAMES[method]
        if search == S.COMP:
            M.comp_full_pixel_search_batch(ts, tr, bw, bh, jobs, cost, d("second"),
                                           d("mask") if form == S.MASK else None, ms, name, sp,
                                           out=out, stream=stream)
        elif search == S.REFINE8:
            M.refining_search_8p_batch(ts, tr, bw, bh, jobs, cost,
                                       d("second") if form != S.PLAIN else None,
                                       d("mask") if form == S.MASK else None, ms, out=out,
                                       stream=stream)
        else:
            M.obmc_full_pixel_search_batch(tr, X.STRIDE, bw, bh, jobs, cost, d("wsrc"),
                                           d("omask"), name, sp, bool(fast), out=out,
                                           stream=stream)
        torch.cuda.synchronize()
        return M.comp_results_numpy(out)

    def expected(self, key, search, form, kind, bw, bh, cjobs, ctype, lam, method, sp, fast, P,
                 ms):
        if key not in self.memo:
            src, refs = self.get(kind)[:2]
            pools = P[1]
            res = S.run_batch(search, form, src.reshape(-1), refs.reshape(-1), X.STRIDE, bw, bh,
                              cjobs, S.cost_of(ctype, lam[0], lam[1], lam[2]), method, sp, fast,
                              pools["second"], pools["mask"], ms, pools["wsrc"], pools["omask"])
            self.memo[key] = np.array([[r[f] for f in FIELDS] for r in res], np.int64)
        return self.memo[key]


@pytest.fixture(scope="module")
def dev(M):
    return Dev(M)


def compare(bad, msg, got, exp):
    for i, f in enumerate(FIELDS):
        g = got[f].astype(np.int64)
        if not np.array_equal(g, exp[:, i]):
            j = int(np.flatnonzero(g != exp[:, i])[0])
            bad.append("%s %s: job %d got %d expected %d (%d differ)" % (
                msg, f, j, g[j], exp[j, i], int((g != exp[:, i]).sum())))


# ------------------------------------------------- the reference's own rows --
def test_every_fixture_row(M, dev):
    F = S.load_fixture()
    J = {n: i for i, n in enumerate(S.ROW_FIELDS)}
    P = ("fixture", {k: F[k] for k in ("second", "mask", "wsrc", "omask")})
    bad, n = [], 0
    for g in S.fixture_groups(F):
        p = g.prm
        dev.get(g.kind, (F["src__" + g.kind], F["refs__" + g.kind]))
        got = dev.run(p["search"], p["form"], g.kind, p["bw"], p["bh"], g.cjobs, p["cost"],
                      (p["error_per_bit"], p["sad_per_bit"], p["hp_tables"]), p["method"],
                      p["step_param"], p["fast_obmc"], P, p["mask_stride"])
        compare(bad, "case %d %r" % (g.index, p), got, g.rows[:, J["best_row"]:J["steps"] + 1])
        n += len(got)
    assert n == len(F["rows"]) >= 150
    assert not bad, "\n".join(bad[:10])


# --------------------------------------------------- sizes beyond the fixture --
def size_pools(bw, bh, jobs, src, seed):
    """Random invariant blocks for `jobs`, one per job: (pools, second_off,
    mask_off, wsrc_off); mask rows bw + 5 apart, the u8 blocks at odd offsets."""
    rng = np.random.default_rng(seed)
    n, ms = bw * bh, bw + 5
    second = rng.integers(0, 256, len(jobs) * (n + 3) + 8).astype(np.uint8)
    mask = rng.integers(0, 65, len(jobs) * (bh * ms + 1) + 8).astype(np.uint8)
    so = np.arange(len(jobs)) * (n + 3) + 1
    mo = np.arange(len(jobs)) * (bh * ms + 1) + 3
    idx = np.arange(bh)[:, None] * X.STRIDE + np.arange(bw)[None, :]
    om = rng.integers(0, 4097, (len(jobs), n))
    om[rng.integers(0, 8, om.shape) == 0] = 4096
    ws = np.stack([src.reshape(-1)[int(jb["src_off"]) + idx].reshape(-1).astype(np.int64) * 4096
                   for jb in jobs]) - rng.integers(0, 256, om.shape) * (4096 - om)
    pools = dict(second=second, mask=mask, wsrc=ws.reshape(-1).astype(np.int32),
                 omask=om.reshape(-1).astype(np.int32))
    return pools, so, mo, np.arange(len(jobs)) * n, ms


BEYOND = [(4, 16, 5), (16, 4, 5), (8, 32, 5), (32, 32, 5), (32, 32, 0), (64, 64, 5), (64, 16, 5),
          (128, 128, 5)]
# (search, form, method, fast, cost type) of the calls each size runs
CALLS = [(S.COMP, S.AVG, S.DIAMOND, 0, X.ENTROPY), (S.COMP, S.MASK, S.NSTEP, 0, X.L1),
         (S.COMP, S.AVG, S.NSTEP_8PT, 0, X.NONE), (S.REFINE8, S.PLAIN, 0, 0, X.ENTROPY),
         (S.REFINE8, S.AVG, 0, 0, X.L1), (S.REFINE8, S.MASK, 0, 0, X.ENTROPY),
         (S.OBMC, S.PLAIN, S.NSTEP_8PT, 0, X.ENTROPY), (S.OBMC, S.PLAIN, S.DIAMOND, 0, X.L1),
         (S.OBMC, S.PLAIN, S.NSTEP, 0, X.NONE), (S.OBMC, S.PLAIN, S.DIAMOND, 1, X.ENTROPY)]


@pytest.mark.parametrize("bw,bh,sp", BEYOND, ids=lambda v: str(v))
def test_sizes_beyond_the_fixture(M, dev, bw, bh, sp):
    bad = []
    for kind in ("noise", "periodic_2"):
        src = dev.get(kind)[0]
        base = X.frame(bw, bh, REF_MV, (3, -2))
        base = X.spread(base, 2 if bw * bh > 4096 else 3, bw + bh)
        for i, jb in enumerate(base):      # starts on and off the exact match
            jb["start_row"], jb["start_col"] = [(0, -1), (3, -2), (-4, 6)][i % 3]
        pools, so, mo, wo, ms = size_pools(bw, bh, base, src, 1000 * bw + bh)
        P = ((kind, bw, bh), pools)
        for ci, (search, form, method, fast, ctype) in enumerate(CALLS):
            if sp == 0 and (search == S.REFINE8 or fast):
                continue                  # (no step_param: the sp 5 case ran them)
            if search == S.OBMC:
                cj = M.comp_jobs(base, wo, wo)
            else:
                cj = M.comp_jobs(base, so, mo, np.arange(len(base)) % 2)
            key = (kind, bw, bh, sp, ci)
            exp = dev.expected(key, search, form, kind, bw, bh, cj, ctype, LOW, method, sp, fast,
                               P, ms)
            got = dev.run(search, form, kind, bw, bh, cj, ctype, LOW, method, sp, fast, P, ms)
            compare(bad, "%s %dx%d sp %d call %d" % (kind, bw, bh, sp, ci), got, exp)
    assert not bad, "\n".join(bad[:10])


# ------------------------------------------------------------ batch geometry --
GEOM_CALLS = [(S.COMP, S.AVG, S.DIAMOND, 0), (S.COMP, S.MASK, S.NSTEP, 0),
              (S.REFINE8, S.MASK, 0, 0), (S.OBMC, S.PLAIN, S.DIAMOND, 0),
              (S.OBMC, S.PLAIN, S.DIAMOND, 1)]


def geometry(M, dev):
    """80 16x16 jobs of the noise frame, job i on the invariant blocks of
    index 79 - i, and the restatement's rows per call of GEOM_CALLS."""
    if "geom" not in dev.memo:
        src = dev.get("noise")[0]
        jobs = X.frame(16, 16, REF_MV, (2, -3))[40:120].copy()
        jobs["start_row"] += (np.arange(80) % 5).astype(np.int16)
        pools, so, mo, wo, ms = size_pools(16, 16, jobs[::-1], src, 77)
        dev.memo["geom"] = (jobs, pools, so[::-1], mo[::-1], wo[::-1], ms)
    return dev.memo["geom"]


@pytest.mark.parametrize("njobs", [1, K_DK_WAVES - 1, K_DK_WAVES + 1, 80])
def test_batch_geometry(M, dev, njobs):
    import torch
    jobs, pools, so, mo, wo, ms = geometry(M, dev)
    P = ("geom", pools)
    assert so[0] > so[1] and wo[0] > wo[1]           # reversed: read per job, not by index
    stream = torch.cuda.Stream()
    bad = []
    for ci, (search, form, method, fast) in enumerate(GEOM_CALLS):
        full = M.comp_jobs(jobs, wo, wo) if search == S.OBMC else \
            M.comp_jobs(jobs, so, mo, np.arange(80) % 2)
        exp = dev.expected(("geom", ci), search, form, "noise", 16, 16, full, X.ENTROPY, LOW,
                           method, 5, fast, P, ms)
        for st in (None, stream):
            if st is not None:
                st.wait_stream(torch.cuda.current_stream())     # (the uploads)
            got = dev.run(search, form, "noise", 16, 16, full[:njobs], X.ENTROPY, LOW, method, 5,
                          fast, P, ms, stream=st)
            compare(bad, "call %d n %d stream %s" % (ci, njobs, st is not None), got,
                    exp[:njobs])
    assert not bad, "\n".join(bad[:10])


def test_output_past_the_batch_is_untouched(M, dev):
    """5 jobs (a partial second workgroup) into a buffer of 8 records."""
    import torch
    jobs, pools, so, mo, wo, ms = geometry(M, dev)
    cj = M.comp_jobs(jobs, so, mo)[:5]
    out = torch.full((8 * M.COMP_RESULT_DTYPE.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    M.comp_full_pixel_search_batch(dev.get("noise")[2], dev.get("noise")[3], 16, 16,
                                   M.to_device(cj), dev.cost(X.L1), dev.pool(("geom", "second"),
                                                                             pools["second"]),
                                   step_param=5, out=out[:5 * 16])
    torch.cuda.synchronize()
    assert (out[5 * 16:].cpu().numpy() == 0x55).all()
    assert (M.comp_results_numpy(out[:5 * 16])["steps"] > 0).all()


def test_wrappers_raise_on_a_refusal(M, dev):
    import torch
    ts, tr = dev.get("noise")[2:4]
    jobs = torch.zeros(M.COMP_JOB_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    sec = torch.zeros(256, dtype=torch.uint8, device="cuda")
    w32 = torch.zeros(256, dtype=torch.int32, device="cuda")
    cost = M.l1_cost_params()
    with pytest.raises(ValueError):
        M.comp_full_pixel_search_batch(ts, tr, 16, 16, jobs, cost, sec, method="hex")
    with pytest.raises(ValueError):
        M.comp_full_pixel_search_batch(ts, tr, 16, 16, jobs, cost, sec, mask=sec, mask_stride=8)
    with pytest.raises(ValueError):
        M.refining_search_8p_batch(ts, tr, 12, 12, jobs, cost)
    with pytest.raises(ValueError):
        M.obmc_full_pixel_search_batch(tr, X.STRIDE, 16, 16, jobs, cost, w32, w32, step_param=11)
