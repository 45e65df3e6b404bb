"""GPU parity of the chroma-from-luma layer, bit-exact everywhere:
* every row of tests/golden/fix_cfl.npz (the reference's own outputs) through
  lavish_cfl_ac_batch, lavish_cfl_predict_batch and
  lavish_cfl_alpha_search_batch in mixed-size calls, and every getter row
  through its `_hip` getter into guarded host buffers;
* every `_hip` getter of include/lavish_dsp_cfl.h at the 14 sizes into guarded
  host buffers, against tests/_cflref.py (the numpy restatement of cfl.c and
  of cfl_pick_plane_parameter's fast leg over the oracle's transform);
* seeded batches against it in mixed-size calls and at 4x4, 4x16, 16x4, 8x16, 32x8 and
  32x32 with 1, 17 and 65 jobs;
* two jobs sharing one AC cell, a repeated call, jobs a builder would refuse;
* the chain DC_PRED (lavish_intra_pred_batch) -> AC -> alpha search ->
  lavish_cfl_joint -> predict on one 64x64 chroma area."""
import ctypes
import os

import numpy as np
import pytest

import _cflref as R

pytestmark = pytest.mark.gpu

GUARD16 = 0x5A5A
SUBS = [(1, 1), (1, 0), (0, 0)]
# (bit depth, 16-bit pixels)
DEPTHS = [(8, 0), (8, 1), (10, 1), (12, 1)]


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.cfl as K
    return K


@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "fix_cfl.npz")))


def _dt(hbd):
    return np.uint16 if hbd else np.uint8


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host(t, hbd):
    a = t.cpu().numpy()
    return a.view(np.uint16) if hbd else a


class Job:
    """one block: luma [lh, lw] (the stored rectangle), src / dc [H, W]"""
    def __init__(self, tx, luma, src, dc):
        self.tx, self.luma, self.src, self.dc = tx, luma, src, dc
        self.w, self.h = R.TX_W[tx], R.TX_H[tx]


def _seeded_job(rng, tx, bd, sub, k):
    w, h = R.TX_W[tx], R.TX_H[tx]
    sx, sy = sub
    # the stored extent: full, or cut in width / height / both (frame edge), in
    # luma multiples of 4 no larger than 32
    fw, fh = min(w << sx, 32), min(h << sy, 32)
    lw = fw if k % 4 in (0, 2) else max(4, (fw // 2) & ~3)
    lh = fh if k % 4 in (0, 1) else max(4, (fh // 2) & ~3)
    maxv = (1 << bd) - 1
    if k % 5 == 4:  # extremes: the largest q3 magnitudes, clipping at both ends
        luma = np.where(rng.integers(0, 2, (lh, lw)) > 0, maxv, 0)
        src = np.where(rng.integers(0, 2, (h, w)) > 0, maxv, 0)
        dc = np.full((h, w), int(rng.choice([0, maxv, maxv // 2])))
    else:
        luma = R.smooth_luma(rng, lw, lh, bd)
        ac = R.ac_block(luma, sx, sy, tx)
        src, dc = R.planted_chroma(rng, ac, int(rng.integers(-16, 17)), bd, noise=int(rng.integers(0, 4)))
    return Job(tx, np.asarray(luma, np.int64), np.asarray(src, np.int64), np.asarray(dc, np.int64))


class Scene:
    """jobs laid into three planes of odd strides, one 32-row band per job"""
    LS, CS = 37, 41

    def __init__(self, jobs, hbd):
        n = len(jobs)
        dt = _dt(hbd)
        self.jobs, self.hbd = jobs, hbd
        self.luma = np.zeros((n * 32 + 1, self.LS), dt)
        self.src = np.zeros((n * 32 + 1, self.CS), dt)
        self.dc = np.zeros((n * 32 + 1, self.CS), dt)
        self.luma_off, self.c_off = [], []
        for i, j in enumerate(jobs):
            y, xl, xc = i * 32 + 1, 1 + i % 4, 1 + (i * 3) % 8
            lh, lw = j.luma.shape
            self.luma[y:y + lh, xl:xl + lw] = j.luma
            self.src[y:y + j.h, xc:xc + j.w] = j.src
            self.dc[y:y + j.h, xc:xc + j.w] = j.dc
            self.luma_off.append(y * self.LS + xl)
            self.c_off.append(y * self.CS + xc)


def _run_scene(K, sc, sub, bd, alphas):
    """(ac cells [n, 32, 32], costs [n, 33], est [n], predicted plane) on the GPU"""
    import torch
    jobs = sc.jobs
    n = len(jobs)
    aj = K.cfl_ac_jobs(sc.luma_off, [j.luma.shape[1] for j in jobs], [j.luma.shape[0] for j in jobs],
                       [j.tx for j in jobs], sub[0], sub[1], luma_stride=sc.LS,
                       luma_elems=sc.luma.size)
    cells = torch.full((n, 32, 32), GUARD16, dtype=torch.int16, device="cuda")
    K.cfl_ac_batch(_dev(sc.luma), K.cfl_jobs_tensor(aj, "cuda"), sub[0], sub[1], bd, out=cells)
    sj = K.cfl_search_jobs(np.arange(n), sc.c_off, sc.c_off, [j.tx for j in jobs], ncells=n,
                           src_stride=sc.CS, src_elems=sc.src.size, dc_stride=sc.CS,
                           dc_elems=sc.dc.size)
    costs, est = K.cfl_alpha_search_batch(cells, _dev(sc.src), _dev(sc.dc),
                                          K.cfl_jobs_tensor(sj, "cuda"), bd)
    pj = K.cfl_predict_jobs(np.arange(n), sc.c_off, [j.tx for j in jobs], alphas, ncells=n,
                            dst_stride=sc.CS, dst_elems=sc.dc.size)
    dst = _dev(sc.dc)
    K.cfl_predict_batch(cells, dst, K.cfl_jobs_tensor(pj, "cuda"), bd)
    torch.cuda.synchronize()
    return (cells.cpu().numpy(), costs.cpu().numpy(), est.cpu().numpy(),
            _host(dst, sc.hbd).reshape(sc.dc.shape))


def _check_scene(K, sc, sub, bd, alphas):
    cells, costs, est, pred = _run_scene(K, sc, sub, bd, alphas)
    want_pred = sc.dc.astype(np.int64)
    bad = []
    for i, j in enumerate(sc.jobs):
        ac = R.ac_block(j.luma, sub[0], sub[1], j.tx)
        cell = cells[i].astype(np.int64)
        ok_ac = np.array_equal(cell[:j.h, :j.w], ac)
        cell[:j.h, :j.w] = np.int16(GUARD16)
        ok_guard = bool((cell == np.int16(GUARD16)).all())
        c, e = R.search(ac, j.src, j.dc, j.tx, bd)
        ok_cost = np.array_equal(costs[i], c)
        ok_est = int(est[i]) == e
        y, x = divmod(sc.c_off[i], sc.CS)
        want_pred[y:y + j.h, x:x + j.w] = R.predict(ac, j.dc, alphas[i], bd)
        if not (ok_ac and ok_guard and ok_cost and ok_est):
            bad.append((i, j.tx, j.luma.shape, ok_ac, ok_guard, ok_cost, ok_est, int(est[i]), e))
    assert not bad, bad[:8]
    assert np.array_equal(pred.astype(np.int64), want_pred)  # and nothing outside the blocks


# --------------------------------------------------------- seeded batches --
SEEDED_TX = {"4x4": 0, "4x16": 13, "16x4": 14, "8x16": 7, "32x8": 16, "32x32": 3}


@pytest.mark.parametrize("njobs", [1, 17, 65])
@pytest.mark.parametrize("size", list(SEEDED_TX))
def test_seeded_batches_vs_restatement(K, size, njobs):
    tx = SEEDED_TX[size]
    k = list(SEEDED_TX).index(size) + [1, 17, 65].index(njobs)
    bd, hbd = (12, 1) if size == "32x32" else DEPTHS[k % 4]
    sub = SUBS[k % 3]
    rng = np.random.default_rng(4200 + 100 * tx + njobs)
    sc = Scene([_seeded_job(rng, tx, bd, sub, q + k) for q in range(njobs)], hbd)
    _check_scene(K, sc, sub, bd, [int(a) for a in rng.integers(-16, 17, njobs)])


def test_largest_block_at_the_12_bit_maximum(K):
    """32x32, 12 bits: all-maximum luma (the largest q3 and sum, a zero AC), the
    luma split that gives the largest |AC|, and the residuals of largest
    magnitude for the transform."""
    maxv, tx = 4095, 3
    rng = np.random.default_rng(77)
    flat = np.full((32, 32), maxv)
    split = np.where(np.arange(32)[None, :] < 16, maxv, 0) + np.zeros((32, 1), np.int64)
    chk = np.where((np.arange(32)[:, None] // 4 + np.arange(32)[None, :] // 4) % 2 > 0, maxv, 0)
    jobs = [Job(tx, flat, rng.integers(0, maxv + 1, (32, 32)), np.full((32, 32), 2048)),
            Job(tx, split, chk, np.full((32, 32), maxv)),
            Job(tx, split, maxv - chk, np.full((32, 32), 0)),
            Job(tx, chk, chk, np.full((32, 32), 2048)),
            Job(tx, split, np.full((32, 32), maxv), np.full((32, 32), 0))]
    for sub in ((0, 0), (1, 1)):
        _check_scene(K, Scene(jobs, 1), sub, 12, [16, -16, 16, -7, 1])


def test_mixed_sizes_every_depth(K):
    """all 14 sizes in one call, per depth and subsampling"""
    for k, (bd, hbd) in enumerate(DEPTHS):
        sub = SUBS[k % 3]
        rng = np.random.default_rng(900 + k)
        txs = R.CFL_TX * 2
        sc = Scene([_seeded_job(rng, tx, bd, sub, q) for q, tx in enumerate(txs)], hbd)
        _check_scene(K, sc, sub, bd, [int(a) for a in rng.integers(-16, 17, len(txs))])


def test_the_walk_on_tied_costs_and_a_carried_best(K):
    """blocks whose walk does not end on the cheapest alpha, stops on an equal
    cost, or has both neighbours of index 16 cheaper than it, where a walk that
    restarted `best` for the downward leg would answer differently"""
    seeds = R.WALK_SEEDS_TIES + R.WALK_SEEDS_CARRIED_BEST
    blocks = [R.walk_block(s) for s in seeds]
    sc = Scene([Job(tx, luma, src, dc) for tx, luma, src, dc in blocks], 0)
    cells, costs, est, _ = _run_scene(K, sc, (0, 0), 8, [0] * len(seeds))
    n_not_argmin = n_equal = n_carried = 0
    for i, (tx, luma, src, dc) in enumerate(blocks):
        c, e = R.search(R.ac_block(luma, 0, 0, tx), src, dc, tx, 8)
        assert np.array_equal(costs[i], c) and int(est[i]) == e, (seeds[i], int(est[i]), e)
        n_not_argmin += e != int(np.argmin(c))
        seen = R.walk(c)[1]
        ends = [k for k in (max(np.flatnonzero(seen)), min(np.flatnonzero(seen))) if k != e]
        n_equal += any(c[k] == c[e] for k in ends)
        n_carried += c[15] < c[16] and c[17] < c[16] and R.walk(c, restart=True)[0] != e
    assert n_not_argmin >= 20 and n_equal >= 20 and n_carried >= 4


# -------------------------------------------------- sharing, repeat, skip --
def test_jobs_sharing_one_cell_and_a_repeated_call(K):
    import torch
    bd, sub, tx = 10, (1, 1), 2
    rng = np.random.default_rng(5)
    j = _seeded_job(rng, tx, bd, sub, 0)
    ac = R.ac_block(j.luma, 1, 1, tx)
    srcs = [R.planted_chroma(rng, ac, a, bd) for a in (-5, 9)]  # U and V of one block
    both = Scene([Job(tx, j.luma, s, d) for s, d in srcs], 1)
    aj = K.cfl_ac_jobs(both.luma_off[:1], 32, 32, tx, 1, 1)
    cells = K.cfl_ac_batch(_dev(both.luma), K.cfl_jobs_tensor(aj, "cuda"), 1, 1, bd)
    sj = K.cfl_jobs_tensor(K.cfl_search_jobs([0, 0], both.c_off, both.c_off, tx, ncells=1), "cuda")
    src, dc = _dev(both.src), _dev(both.dc)
    runs = [K.cfl_alpha_search_batch(cells, src, dc, sj, bd) for _ in range(2)]
    pj = K.cfl_jobs_tensor(K.cfl_predict_jobs([0, 0], both.c_off, tx, [-5, 9], ncells=1), "cuda")
    outs = []
    for _ in range(2):
        dst = _dev(both.dc)
        K.cfl_predict_batch(cells, dst, pj, bd)
        outs.append(dst)
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(outs[0], outs[1])
    want = both.dc.astype(np.int64)
    for i, (s, d) in enumerate(srcs):
        c, e = R.search(ac, s, d, tx, bd)
        assert np.array_equal(runs[0][0][i].cpu().numpy(), c)
        assert int(runs[0][1][i]) == e
        y, x = divmod(both.c_off[i], both.CS)
        want[y:y + 16, x:x + 16] = R.predict(ac, d, (-5, 9)[i], bd)
    assert np.array_equal(_host(outs[0], 1).reshape(both.dc.shape).astype(np.int64), want)


def test_jobs_a_builder_refuses_are_skipped_on_the_device(K):
    """tables written past the builders: a 64-point size, a cell index and a
    rectangle outside what the call declares, an alpha outside -16 .. 16 and a
    stored extent larger than the transform write nothing; the good job beside
    each runs."""
    import torch
    bd, sub, tx = 8, (0, 0), 1
    rng = np.random.default_rng(6)
    sc = Scene([_seeded_job(rng, tx, bd, sub, 0) for _ in range(6)], 0)
    n = 6
    aj = K.cfl_ac_jobs(sc.luma_off, 8, 8, tx, 0, 0)
    aj[1, 3] = 4                   # TX_64X64
    aj[2, 0] = sc.luma.size - 5    # rectangle past the plane's end
    aj[3, 1] = 16                  # stored 16 wide for an 8-wide transform
    aj[4, 2] = 6                   # not a multiple of 4
    cells = torch.full((n, 32, 32), GUARD16, dtype=torch.int16, device="cuda")
    K.cfl_ac_batch(_dev(sc.luma), K.cfl_jobs_tensor(aj, "cuda"), 0, 0, bd, out=cells)
    torch.cuda.synchronize()
    got = cells.cpu().numpy()
    for i in (1, 2, 3, 4):
        assert (got[i] == np.int16(GUARD16)).all(), i
    for i in (0, 5):
        assert np.array_equal(got[i][:8, :8], R.ac_block(sc.jobs[i].luma, 0, 0, tx)), i
    good = K.cfl_ac_batch(_dev(sc.luma), K.cfl_jobs_tensor(K.cfl_ac_jobs(sc.luma_off, 8, 8, tx, 0, 0),
                                                           "cuda"), 0, 0, bd)
    sj = K.cfl_search_jobs(np.arange(n), sc.c_off, sc.c_off, tx)
    sj[1, 3] = 11                  # TX_32X64
    sj[2, 0] = n                   # cell outside
    sj[3, 1] = sc.src.size - 3     # src rectangle outside
    sj[4, 2] = -1                  # negative dc offset
    costs, est = K.cfl_alpha_search_batch(good, _dev(sc.src), _dev(sc.dc),
                                          K.cfl_jobs_tensor(sj, "cuda"), bd)
    pj = K.cfl_predict_jobs(np.arange(n), sc.c_off, tx, 3)
    pj[1, 3] = 17                  # alpha_q3
    pj[2, 0] = -1
    pj[3, 1] = sc.dc.size
    pj[4, 2] = 18                  # TX_64X16
    dst = _dev(sc.dc)
    K.cfl_predict_batch(good, dst, K.cfl_jobs_tensor(pj, "cuda"), bd)
    torch.cuda.synchronize()
    costs, est = costs.cpu().numpy(), est.cpu().numpy()
    want = sc.dc.astype(np.int64)
    for i in range(n):
        j = sc.jobs[i]
        ac = R.ac_block(j.luma, 0, 0, tx)
        if i in (1, 2, 3, 4):
            assert (costs[i] == 0).all() and est[i] == 0, i   # as allocated
            continue
        c, e = R.search(ac, j.src, j.dc, tx, bd)
        assert np.array_equal(costs[i], c) and est[i] == e, i
        y, x = divmod(sc.c_off[i], sc.CS)
        want[y:y + 8, x:x + 8] = R.predict(ac, j.dc, 3, bd)
    assert np.array_equal(_host(dst, 0).reshape(sc.dc.shape).astype(np.int64), want)
    import lavish_dsp as L
    assert L.status()[0] == 0, L.status()


# ------------------------------------------------------------- the getters --
class Getters:
    """the entries of include/lavish_dsp_cfl.h on a library handle of this
    test's own (the package's handle declares only lavish_* names)"""
    def __init__(self):
        import lavish_dsp as L
        self.lib = ctypes.CDLL(L.LIB_PATH)
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        self.protos = {"subtract_average": ctypes.CFUNCTYPE(None, vp, vp),
                       "subsample": ctypes.CFUNCTYPE(None, vp, i32, vp),
                       "predict_lbd": ctypes.CFUNCTYPE(None, vp, vp, i32, i32),
                       "predict_hbd": ctypes.CFUNCTYPE(None, vp, vp, i32, i32, i32)}

    def get(self, getter, kind, tx):
        g = getattr(self.lib, getter + "_hip")
        g.argtypes, g.restype = [ctypes.c_uint8], ctypes.c_void_p
        p = g(tx)
        return None if not p else self.protos[kind](p)


@pytest.fixture(scope="module")
def G(K):
    return Getters()


def _ptr(a, i=0):
    return ctypes.c_void_p(a.ctypes.data + i * a.itemsize)


GETTER_KINDS = [("cfl_get_subtract_average_fn", "subtract_average")] + \
    [("cfl_get_luma_subsampling_%d_%s" % (s, b), "subsample") for s in (420, 422, 444)
     for b in ("lbd", "hbd")] + \
    [("cfl_get_predict_lbd_fn", "predict_lbd"), ("cfl_get_predict_hbd_fn", "predict_hbd")]


def test_getters_return_null_for_the_64_point_sizes(G):
    for getter, kind in GETTER_KINDS:
        for tx in range(19):
            f = G.get(getter, kind, tx)
            assert (f is None) == (tx not in R.CFL_TX), (getter, tx)


def _getter_case(G, getter, kind, tx, bd, rng, inputs=None):
    """run one getter's function of size tx on guarded host buffers; returns
    what it wrote and whether everything else is intact"""
    w, h = R.TX_W[tx], R.TX_H[tx]
    f = G.get(getter, kind, tx)
    maxv = (1 << bd) - 1
    if kind == "subtract_average":
        q3 = inputs if inputs is not None else rng.integers(0, 8 * maxv + 1, (h, w))
        src = np.full(R.SQUARE + 64, GUARD16, np.uint16)
        dst = np.full(R.SQUARE + 64, GUARD16, np.uint16).view(np.int16)
        sv = src[32:32 + R.SQUARE].reshape(32, 32)
        sv[:h, :w] = q3
        f(_ptr(src, 32), _ptr(dst, 32))
        cell = dst[32:32 + R.SQUARE].reshape(32, 32).astype(np.int64)
        got = cell[:h, :w].copy()
        cell[:h, :w] = np.int16(GUARD16)
        intact = (cell == np.int16(GUARD16)).all() and (dst[:32] == np.int16(GUARD16)).all() and \
            (dst[32 + R.SQUARE:] == np.int16(GUARD16)).all()
        return got, bool(intact), R.subtract_average(q3)
    if kind == "subsample":
        hbd = getter.endswith("hbd")
        sx, sy = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[getter.split("_")[4]]
        luma = inputs if inputs is not None else rng.integers(0, maxv + 1, (h, w))
        stride = w + 5
        inp = np.zeros(h * stride + 8, _dt(hbd))
        inp[3:3 + h * stride].reshape(h, stride)[:, :w] = luma
        out = np.full(R.SQUARE + 64, GUARD16, np.uint16)
        f(_ptr(inp, 3), stride, _ptr(out, 32))
        cell = out[32:32 + R.SQUARE].reshape(32, 32).astype(np.int64)
        got = cell[:h >> sy, :w >> sx].copy()
        cell[:h >> sy, :w >> sx] = GUARD16
        intact = (cell == GUARD16).all() and (out[:32] == GUARD16).all() and \
            (out[32 + R.SQUARE:] == GUARD16).all()
        return got, bool(intact), R.subsample(luma, sx, sy)
    hbd = kind == "predict_hbd"
    ac, dc, alpha = inputs if inputs is not None else (
        rng.integers(-4 * maxv, 4 * maxv + 1, (h, w)), rng.integers(0, maxv + 1, (h, w)),
        int(rng.integers(-16, 17)))
    cell = np.zeros((32, 32), np.int16)
    cell[:h, :w] = ac
    stride = w + 3
    guard = GUARD16 if hbd else 0x5A
    buf = np.full((h + 2) * stride, guard, _dt(hbd))
    rows = buf.reshape(h + 2, stride)
    rows[1:h + 1, 1:w + 1] = dc
    f(*([_ptr(cell), _ptr(buf, stride + 1), stride, alpha] + ([bd] if hbd else [])))
    res = buf.reshape(h + 2, stride).astype(np.int64)
    got = res[1:h + 1, 1:w + 1].copy()
    res[1:h + 1, 1:w + 1] = guard
    return got, bool((res == guard).all()), R.predict(ac, dc, alpha, bd)


def test_every_getter_every_size_vs_restatement(G):
    import lavish_dsp as L
    rng = np.random.default_rng(31)
    bad = []
    for getter, kind in GETTER_KINDS:
        for k, tx in enumerate(R.CFL_TX):
            lbd = getter.endswith("lbd") or kind == "predict_lbd"
            bd = 8 if lbd else (8, 10, 12)[k % 3]
            got, intact, want = _getter_case(G, getter, kind, tx, bd, rng)
            if not intact or not np.array_equal(got, want):
                bad.append((getter, tx, bd, intact))
    assert not bad, bad[:8]
    assert L.status()[0] == 0, L.status()


# ----------------------------------------------------------------- fixture --
def test_every_fixture_getter_row(G, F):
    import lavish_dsp as L
    rng = np.random.default_rng(0)
    bad = []
    for i, row in enumerate(F["getter_rows"]):
        g = R.getter_row(F, row)
        got, intact, _ = _getter_case(G, g.getter, g.kind, g.tx, g.bd, rng, inputs=g.inputs)
        if not intact or not np.array_equal(got, g.out):
            bad.append((i, g.getter, g.tx, g.bd, intact))
    assert not bad, bad[:8]
    assert len(F["getter_rows"]) >= 9 * 14
    assert L.status()[0] == 0, L.status()


@pytest.mark.parametrize("depth", DEPTHS, ids=["8", "8h", "10", "12"])
def test_every_fixture_block_and_search_row_through_the_batches(K, F, depth):
    """cfl_store_block / cfl_store_tx + cfl_predict_block rows and
    cfl_pick_plane_parameter rows: all of a depth and subsampling, every size
    among them, in one call of each kernel"""
    bd, hbd = depth
    nrows = 0
    for sub in SUBS:
        rows = [r for r in (R.block_row(F, row) for row in F["block_rows"])
                if (r.bd, r.hbd, r.sub) == (bd, hbd, sub)]
        srows = [r for r in (R.search_row(F, row) for row in F["search_rows"])
                 if (r.bd, r.hbd, r.sub) == (bd, hbd, sub)]
        if not rows and not srows:
            continue
        nrows += len(rows) + len(srows)
        sc = Scene([Job(r.tx, r.luma, r.src, r.dc) for r in rows + srows], hbd)
        alphas = [r.alpha_q3 for r in rows] + [0] * len(srows)
        cells, costs, est, pred = _run_scene(K, sc, sub, bd, alphas)
        bad = []
        for i, r in enumerate(rows + srows):
            if not np.array_equal(cells[i][:r.h, :r.w], r.ac):
                bad.append((i, "ac", r.tx))
            if i < len(rows):
                y, x = divmod(sc.c_off[i], sc.CS)
                if not np.array_equal(pred[y:y + r.h, x:x + r.w], r.pred):
                    bad.append((i, "pred", r.tx))
            elif int(est[i]) != r.est or not np.array_equal(costs[i][r.mask], r.costs[r.mask]):
                bad.append((i, "search", r.tx, int(est[i]), r.est))
        assert not bad, bad[:8]
    assert nrows > 0
    if depth != (8, 1):
        assert nrows >= 28


# ------------------------------------------------------------- the chain ---
def test_chain_dc_ac_search_joint_predict(K):
    """One 64x64 chroma area, 4:2:0, 10 bits: DC_PRED of every U and V block
    by lavish_intra_pred_batch, the AC of its luma, the alpha search per
    plane, lavish_cfl_joint per block, then the prediction in place on the DC
    blocks; the end result equals the restatement's."""
    import torch
    import _intraref as IR
    import lavish_dsp.intra as I
    bd, S, LS_ = 10, 72, 136
    rng = np.random.default_rng(11)
    maxv = 1023
    y, x = np.mgrid[0:128, 0:128]
    luma = np.clip(500 + 3 * x - 2 * y + 40 * np.sin(x / 5.0) + rng.integers(-6, 7, (128, 128)),
                   0, maxv).astype(np.int64)
    lplane = np.zeros((129, LS_), np.uint16)
    lplane[1:, 1:129] = luma
    # U over V in one tensor, frame origin at (1, 1) of each 66-row band
    recon = rng.integers(300, 700, (132, S)).astype(np.uint16)
    sub2 = (luma[0::2, 0::2] + luma[0::2, 1::2] + luma[1::2, 0::2] + luma[1::2, 1::2]) // 4
    src = np.zeros((132, S), np.uint16)
    for p, (gain, base) in enumerate(((0.6, 420), (-0.9, 610))):
        band = np.clip(base + gain * (sub2 - sub2.mean()) + rng.integers(-2, 3, (64, 64)), 0, maxv)
        src[66 * p + 1:66 * p + 65, 1:65] = band
    blocks = [(2, by * 16, bx * 16) for by in range(2) for bx in range(4)] + \
             [(1, 32 + by * 8, bx * 8) for by in range(2) for bx in range(8)] + \
             [(8, 48 + by * 8, bx * 16) for by in range(2) for bx in range(4)]   # 16x16 8x8 16x8
    nb = len(blocks)
    txs = [b[0] for b in blocks]
    coff = [[(66 * p + 1 + b[1]) * S + 1 + b[2] for b in blocks] for p in range(2)]
    d_recon, d_src = _dev(recon), _dev(src)
    dcp = torch.zeros_like(d_recon)
    ij = I.intra_jobs(coff[0] + coff[1], coff[0] + coff[1], txs * 2, I.DC_PRED)
    I.intra_pred_batch(d_recon, dcp, I.intra_jobs_tensor(ij, "cuda"), bd)
    aj = K.cfl_ac_jobs([(1 + 2 * b[1]) * LS_ + 1 + 2 * b[2] for b in blocks],
                       [2 * R.TX_W[t] for t in txs], [2 * R.TX_H[t] for t in txs], txs, 1, 1,
                       luma_stride=LS_, luma_elems=lplane.size)
    cells = K.cfl_ac_batch(_dev(lplane), K.cfl_jobs_tensor(aj, "cuda"), 1, 1, bd)
    sj = K.cfl_search_jobs(list(range(nb)) * 2, coff[0] + coff[1], coff[0] + coff[1], txs * 2,
                           ncells=nb, src_stride=S, src_elems=src.size, dc_stride=S,
                           dc_elems=src.size)
    costs, est = K.cfl_alpha_search_batch(cells, d_src, dcp, K.cfl_jobs_tensor(sj, "cuda"), bd)
    est = est.cpu().numpy()
    # the host step between the two launches: the joint parameters per block
    pc, po, pt, pa = [], [], [], []
    params = []
    for b in range(nb):
        valid, aidx, js = K.cfl_joint(est[b], est[nb + b])
        params.append((valid, aidx, js))
        if not valid:
            continue
        for p in range(2):
            pc.append(b)
            po.append(coff[p][b])
            pt.append(txs[b])
            pa.append(int(est[p * nb + b]) - 16)
    pj = K.cfl_predict_jobs(pc, po, pt, pa, ncells=nb, dst_stride=S, dst_elems=src.size)
    K.cfl_predict_batch(cells, dcp, K.cfl_jobs_tensor(pj, "cuda"), bd)
    torch.cuda.synchronize()
    got = _host(dcp, 1).reshape(132, S).astype(np.int64)
    # the same on the host
    want = np.zeros((132, S), np.int64)
    flat = recon.reshape(-1).astype(np.int64)
    n_cfl = 0
    for b, (tx, by, bx) in enumerate(blocks):
        w, h = R.TX_W[tx], R.TX_H[tx]
        ac = R.ac_block(luma[2 * by:2 * by + 2 * h, 2 * bx:2 * bx + 2 * w], 1, 1, tx)
        ests = []
        dcs = []
        for p in range(2):
            dc = IR.predict(flat, S, coff[p][b], tx, IR.DC_PRED, 0, 5, 0, 0, w, -1, h, -1, bd)
            yy, xx = divmod(coff[p][b], S)
            _, e = R.search(ac, src[yy:yy + h, xx:xx + w].astype(np.int64), dc, tx, bd)
            ests.append(e)
            dcs.append(dc)
        assert (int(est[b]), int(est[nb + b])) == tuple(ests), b
        assert params[b] == R.joint(*ests), b
        n_cfl += params[b][0]
        for p in range(2):
            yy, xx = divmod(coff[p][b], S)
            want[yy:yy + h, xx:xx + w] = R.predict(ac, dcs[p], ests[p] - 16, bd) if params[b][0] \
                else dcs[p]
    assert np.array_equal(got, want)
    assert n_cfl >= nb // 2   # the planted gains are found: most blocks take CfL
