"""GPU parity of the plain pixel batch calls of csrc/pixel.hip in their packed
form (many jobs per launch), bit-exact against tests/_pixref.py, which
test_pixel_batch_cpu.py pins to tests/golden/fix_pixel.npz and to the oracle:

* lavish_sad_batch / lavish_variance_batch for all 22 block sizes, 8 bits as
  bytes and as 16-bit samples, 10 and 12 bits, on seeded 264x328 planes with
  the edge blocks of _pixref.Planes among ordinary jobs; job counts that end in
  a partial lane group, a partial workgroup and more than one workgroup,
  whatever the lanes per job; every job compared; a sentinel behind every
  output;
* the generic kernels on shapes that are no power of two;
* subtract, sum_squares, sum_sse, Hadamard (+ highbd, lp), SATD (+ lp) and
  block error (+ highbd, lp) with more than one job;
* batch against shim on the same job, and a repeated call."""
import numpy as np
import pytest

import _pixref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NJOBS = [1, 5, 67, 259]  # 259 only where w * h <= 1024
GUARD = 8
FILL = {"int16": 0x5A5A, "int32": 0x5A5A5A5A, "int64": 0x5A5A5A5A5A5A5A5A}
CFG_IDS = ["u8", "hbd8", "hbd10", "hbd12"]


@pytest.fixture(scope="module")
def P():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.pixel as P
    return P


def counts(w, h):
    return [n for n in NJOBS if n <= R.max_jobs(w, h)]


def dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def sentinel(n, dtype="int32"):
    """n output words followed by GUARD sentinel words."""
    import torch
    return torch.full((n + GUARD,), FILL[dtype], dtype=getattr(torch, dtype), device=DEV)


def fetch(out, n, what=""):
    """The first n words of a sentinel buffer; nothing behind them was written."""
    a = out.cpu().numpy()
    assert (a[n:] == FILL[str(a.dtype)]).all(), "words beyond the outputs written: " + what
    return a[:n].astype(np.int64)


def u32(a):
    return a & R.M32


class Dev:
    """A _pixref.Planes on the device."""

    def __init__(self, P, B):
        self.P, self.B = P, B
        self.src, self.ref, self.second = dev(B.src), dev(B.ref), dev(B.second)
        self.jobs = P.jobs_tensor(B.jobs, DEV)

    def sad(self, nj, nrefs, mode):
        P, B = self.P, self.B
        out = sentinel(nj * nrefs)
        rc = P._lib.lavish_sad_batch(P._d(self.src), self.src.stride(0), P._d(self.ref),
                                     self.ref.stride(0), B.w, B.h, P._d(self.jobs), nj, nrefs,
                                     mode, P._d(self.second), int(B.hb), P._d(out),
                                     P._stream_ptr(None))
        assert rc == 0
        return u32(fetch(out, nj * nrefs, "sad mode %d" % mode)).reshape(nj, nrefs)

    def variance(self, nj, kind):
        """(var, sse, sum, sse64) with None for what the kind must leave alone."""
        P, B = self.P, self.B
        var, sse, sm, s64 = sentinel(nj), sentinel(nj), sentinel(nj), sentinel(nj, "int64")
        rc = P._lib.lavish_variance_batch(P._d(self.src), self.src.stride(0), P._d(self.ref),
                                          self.ref.stride(0), B.w, B.h, P._d(self.jobs), nj, kind,
                                          B.bd, int(B.hb), P._d(self.second), P._d(var), P._d(sse),
                                          P._d(sm), P._d(s64), P._stream_ptr(None))
        assert rc == 0
        what = "variance kind %d" % kind
        if kind == 4:
            for o in (var, sse, sm):
                fetch(o, 0, what)
            return None, None, None, fetch(s64, nj, what)
        fetch(s64, 0, what)
        return u32(fetch(var, nj, what)), u32(fetch(sse, nj, what)), fetch(sm, nj, what), None


def planes(P, w, h, bd, hb, njobs=None):
    B = R.Planes(w, h, bd, hb, P.JOB_DTYPE, njobs)
    return B, Dev(P, B)


def eq(got, want, msg):
    np.testing.assert_array_equal(got, want, err_msg=msg)


# ------------------------------------------------------- SAD and variance --
@pytest.mark.parametrize("bd,hb", R.CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("w,h", R.SIZES)
def test_sad_batch(P, w, h, bd, hb):
    B, D = planes(P, w, h, bd, hb)
    S, P2 = B.S(), B.P2()
    refs = [B.R(k=k) for k in range(4)]
    for mode, f in enumerate((R.sad, R.sad_skip, lambda s, r: R.sad_avg(s, r, P2))):
        want = np.stack([f(S, r) for r in refs], 1)
        for nj in counts(w, h):
            for nrefs in (1, 2, 3, 4):
                eq(D.sad(nj, nrefs, mode), want[:nj, :nrefs],
                   "mode %d, %d jobs, %d refs" % (mode, nj, nrefs))


@pytest.mark.parametrize("bd,hb", R.CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("w,h", R.SIZES)
def test_variance_batch(P, w, h, bd, hb):
    """variance, mse, get_var and sse: var, sse and sum of every job."""
    B, D = planes(P, w, h, bd, hb)
    v, s, sm = R.variance(B.S(), B.R(), bd)
    s64 = R.sse(B.S(), B.R())
    for nj in counts(w, h):
        for kind in (0, 1, 2):
            gv, gs, gm, _ = D.variance(nj, kind)
            msg = "kind %d, %d jobs" % (kind, nj)
            eq(gv, (s if kind == 1 else v)[:nj], msg + " var")
            eq(gs, s[:nj], msg + " sse")
            eq(gm, sm[:nj], msg + " sum")
        eq(D.variance(nj, 4)[3], s64[:nj], "sse64, %d jobs" % nj)


@pytest.mark.parametrize("bd,hb", R.CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("w,h", R.SIZES)
def test_sub_pixel_variance_batch(P, w, h, bd, hb):
    """kinds 3 and 5: every (xoff, yoff) of 0..7 x 0..7 over the jobs, second_pred
    blocks at odd offsets of a pool."""
    B, D = planes(P, w, h, bd, hb)
    j = B.jobs
    assert len({(x, y) for x, y in zip(j["xoff"], j["yoff"])}) == 64
    for kind, second in ((3, None), (5, B.P2())):
        v, s, sm = R.sub_pixel_variance(B.S(dw=1), j["xoff"], j["yoff"], B.R(), bd, hb, second)
        for nj in counts(w, h):
            gv, gs, gm, _ = D.variance(nj, kind)
            msg = "kind %d, %d jobs" % (kind, nj)
            eq(gv, v[:nj], msg + " var")
            eq(gs, s[:nj], msg + " sse")
            eq(gm, sm[:nj], msg + " sum")


@pytest.mark.parametrize("bd,hb", R.CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("w,h", [(12, 8), (20, 36)])
def test_shapes_that_are_no_power_of_two(P, w, h, bd, hb):
    """The one-wave-per-job kernels behind the packed ones."""
    B, D = planes(P, w, h, bd, hb, 67)
    S, P2 = B.S(), B.P2()
    refs = [B.R(k=k) for k in range(4)]
    v, s, sm = R.variance(S, refs[0], bd)
    for nj in (5, 67):
        for mode, f in ((0, R.sad), (2, lambda a, r: R.sad_avg(a, r, P2))):
            want = np.stack([f(S, r) for r in refs], 1)
            for nrefs in (1, 4):
                eq(D.sad(nj, nrefs, mode), want[:nj, :nrefs], "mode %d, %d jobs" % (mode, nj))
        gv, gs, gm, _ = D.variance(nj, 0)
        eq(gv, v[:nj], "var"), eq(gs, s[:nj], "sse"), eq(gm, sm[:nj], "sum")
        eq(D.variance(nj, 4)[3], R.sse(S, refs[0])[:nj], "sse64")


# --------------------------------------------------- residuals and sums --
RES_SHAPES = [(4, 4), (16, 8), (7, 5), (64, 64)]


def res_jobs(P, offs, aux=None):
    j = np.zeros(len(offs), P.JOB_DTYPE)
    j["src_off"] = offs
    if aux is not None:
        j["aux_off"] = aux
    return j


@pytest.mark.parametrize("bd,hb", R.CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("w,h", RES_SHAPES)
def test_subtract_batch(P, w, h, bd, hb):
    import torch
    B, D = planes(P, w, h, bd, hb)
    diff = R.subtract(B.S(), B.R())
    ds = w + 3
    for nj in counts(w, h):
        jobs = B.jobs[:nj].copy()
        jobs["aux_off"] = np.arange(nj) * h * ds + 1
        out = torch.full((nj * h + 1, ds), 0x7777, dtype=torch.int16, device=DEV)
        P.subtract_batch(h, w, out, D.src, D.ref, P.jobs_tensor(jobs, DEV))
        want = np.full((nj * h + 1) * ds, 0x7777, np.int16)
        idx = np.arange(h)[:, None] * ds + np.arange(w)[None, :]
        want[jobs["aux_off"][:, None, None] + idx[None]] = diff[:nj]
        eq(out.cpu().numpy().reshape(-1), want, "%d jobs" % nj)


@pytest.mark.parametrize("kind", ["4095", "wrap"])
@pytest.mark.parametrize("w,h", RES_SHAPES)
def test_sum_squares_and_sum_sse_batch(P, w, h, kind):
    plane = R.residual_plane(kind, 5)
    d = dev(plane)
    offs = R.residual_offsets(plane, h, w, R.max_jobs(w, h), w + h)
    assert (offs % w != 0).any() and (offs // plane.shape[1] % h != 0).any()
    X = R.windows(plane, offs, h, w)
    sq, (sm, ss) = R.sum_squares_2d_i16(X), R.get_blk_sse_sum(X)
    tj = P.jobs_tensor(res_jobs(P, offs), DEV)
    for nj in counts(w, h):
        out = sentinel(nj, "int64")
        assert P._lib.lavish_sum_squares_batch(P._d(d), d.stride(0), w, h, P._d(tj), nj,
                                               P._d(out), P._stream_ptr(None)) == 0
        eq(fetch(out, nj, "sum_squares"), sq[:nj], "sum_squares, %d jobs" % nj)
        osm, oss = sentinel(nj), sentinel(nj, "int64")
        assert P._lib.lavish_sum_sse_batch(P._d(d), d.stride(0), w, h, P._d(tj), nj, P._d(osm),
                                           P._d(oss), P._stream_ptr(None)) == 0
        eq(fetch(osm, nj, "sum_sse sum"), sm[:nj], "sum_sse sum, %d jobs" % nj)
        eq(fetch(oss, nj, "sum_sse sse"), ss[:nj], "sum_sse sse, %d jobs" % nj)


# --------------------------------------------------------------- Hadamard --
HEAD = 3  # coefficient words in front of job 0's block
HAD_FORMS = ([("low", n, k) for n in (4, 8, 16, 32) for k in ("255", "wrap")] +
             [("high", n, k) for n in (8, 16, 32) for k in ("4095", "wrap")] +
             [("lp", n, k) for n in (8, 16) for k in ("255", "wrap")])


def run_hadamard(P, form, n, d, tj, nj, total):
    """The raw call on a sentinel buffer of `total` coefficient words: (rc, words)."""
    out = sentinel(total, "int16" if form == "lp" else "int32")
    if form == "lp":
        rc = P._lib.lavish_hadamard_lp_batch(n, P._d(d), d.stride(0), P._d(tj), nj, P._d(out),
                                             P._stream_ptr(None))
    else:
        rc = P._lib.lavish_hadamard_batch(n, int(form == "high"), P._d(d), d.stride(0), P._d(tj),
                                          nj, P._d(out), P._stream_ptr(None))
    return rc, out


@pytest.mark.parametrize("form,n,kind", HAD_FORMS)
def test_hadamard_batch(P, form, n, kind):
    plane = R.residual_plane(kind, 5)
    d = dev(plane)
    offs = R.residual_offsets(plane, n, n, 259, n)
    assert (offs % n != 0).any()
    X = R.windows(plane, offs, n, n)
    want = R.hadamard_lp(X, n) if form == "lp" else R.hadamard(X, n, highbd=form == "high")
    tj = P.jobs_tensor(res_jobs(P, offs, np.arange(259) * n * n + HEAD), DEV)
    for nj in NJOBS:
        total = HEAD + nj * n * n
        rc, out = run_hadamard(P, form, n, d, tj, nj, total)
        assert rc == 0
        got = fetch(out, total, "hadamard")
        assert (got[:HEAD] == FILL["int16" if form == "lp" else "int32"]).all()
        eq(got[HEAD:].reshape(nj, n * n), want[:nj], "%s %d, %d jobs" % (form, n, nj))


@pytest.mark.parametrize("form,n", [("high", 4), ("lp", 32), ("lp", 4), ("low", 12)])
def test_hadamard_forms_the_reference_lacks_are_refused(P, form, n):
    plane = R.residual_plane("255", 5)
    tj = P.jobs_tensor(res_jobs(P, [0, 1, 2, 3, 4]), DEV)
    rc, out = run_hadamard(P, form, n, dev(plane), tj, 5, 64)
    assert rc == -1
    fetch(out, 0, "refused hadamard")


# ------------------------------------------------- SATD and block error --
@pytest.mark.parametrize("length", [16, 64, 256, 1024])
def test_satd_and_block_error_batch(P, length):
    c, q = R.coeff_rows(length, 67, length)
    c16, q16 = R.coeff_rows_lp(length, 67, length)
    dc, dq, dc16, dq16 = dev(c), dev(q), dev(c16), dev(q16)
    L, sp = P._lib, P._stream_ptr(None)
    for nb in (1, 5, 67):
        out = sentinel(nb)
        assert L.lavish_satd_batch(P._d(dc), length, nb, P._d(out), sp) == 0
        eq(fetch(out, nb, "satd"), R.satd(c)[:nb], "satd, %d blocks" % nb)
        out = sentinel(nb)
        assert L.lavish_satd_lp_batch(P._d(dc16), length, nb, P._d(out), sp) == 0
        eq(fetch(out, nb, "satd_lp"), R.satd_lp(c16)[:nb], "satd_lp, %d blocks" % nb)
        for bd in (0, 8, 10, 12):
            err, ssz = sentinel(nb, "int64"), sentinel(nb, "int64")
            assert L.lavish_block_error_batch(P._d(dc), P._d(dq), length, nb, bd, P._d(err),
                                              P._d(ssz), sp) == 0
            we, wz = R.block_error(c, q, bd or None)
            eq(fetch(err, nb, "block_error"), we[:nb], "error, bd %d, %d blocks" % (bd, nb))
            eq(fetch(ssz, nb, "block_error"), wz[:nb], "ssz, bd %d, %d blocks" % (bd, nb))
        err = sentinel(nb, "int64")
        assert L.lavish_block_error_lp_batch(P._d(dc16), P._d(dq16), length, nb, P._d(err),
                                             sp) == 0
        eq(fetch(err, nb, "block_error_lp"), R.block_error_lp(c16, q16)[:nb],
           "block_error_lp, %d blocks" % nb)
    import lavish_dsp
    assert lavish_dsp.status()[0] == 0, lavish_dsp.status()


# ------------------------------------------------------------ batch = shim --
NSHIM = 5


@pytest.mark.parametrize("bd,hb", R.CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("w,h", [(4, 4), (8, 8), (16, 8), (32, 16)])
def test_batch_equals_shim_on_the_same_job(P, w, h, bd, hb):
    """The first jobs of a list (edge blocks among them) through the per-call
    shims, which the fixtures pin, and through the Python batch wrappers."""
    B, D = planes(P, w, h, bd, hb, 67)
    j = B.jobs[:NSHIM]
    tj = P.jobs_tensor(j, DEV)
    fs, fr = B.src.reshape(-1), B.ref.reshape(-1)
    A = [fs[o:] for o in j["src_off"]]
    Bk = [[fr[o:] for o in j["ref_off"][:, k]] for k in range(4)]
    sec = [B.second[o:] for o in j["aux_off"]]
    pw = R.PW
    for mode, kw in ((0, {}), (1, {"skip": True}), (2, None)):
        got = P.sad_batch(D.src, D.ref, w, h, tj, 4, mode, D.second).cpu().numpy()
        for i in range(NSHIM):
            for k in range(4):
                k2 = kw if kw is not None else {"second_pred": sec[i]}
                assert got[i, k] == P.sad(w, h, A[i], pw, Bk[k][i], pw, hb, **k2), (mode, i, k)
    out = {k: {n: t.cpu().numpy() for n, t in
               P.variance_batch(D.src, D.ref, w, h, tj, k, bd, D.second).items()}
           for k in range(6)}
    for i in range(NSHIM):
        a, b = A[i], Bk[0][i]
        xo, yo = int(j["xoff"][i]), int(j["yoff"][i])
        assert (out[0]["var"][i], out[0]["sse"][i]) == P.variance(w, h, a, pw, b, pw, bd, hb)
        assert (out[3]["var"][i], out[3]["sse"][i]) == \
            P.sub_pixel_variance(w, h, a, pw, xo, yo, b, pw, bd, hb)
        assert (out[5]["var"][i], out[5]["sse"][i]) == \
            P.sub_pixel_variance(w, h, a, pw, xo, yo, b, pw, bd, hb, sec[i])
        assert out[4]["sse64"][i] == P.sse(a, pw, b, pw, w, h, hb)
        if (w, h) in ((8, 8), (16, 8)):
            assert (out[1]["var"][i], out[1]["sse"][i]) == P.mse(w, h, a, pw, b, pw, bd, hb)
        if (w, h) == (8, 8):
            assert (out[2]["sse"][i], out[2]["sum"][i]) == P.get_var(8, a, pw, b, pw, bd, hb)


def test_residual_batches_equal_their_shims(P):
    import torch
    plane = R.residual_plane("wrap", 5)
    d, flat, cols = dev(plane), plane.reshape(-1), plane.shape[1]
    for n in (4, 8, 16, 32):
        offs = R.residual_offsets(plane, n, n, NSHIM, n)
        tj = P.jobs_tensor(res_jobs(P, offs, np.arange(NSHIM) * n * n), DEV)
        low = P.hadamard_batch(n, d, tj, NSHIM * n * n).cpu().numpy().reshape(NSHIM, -1)
        sq = P.sum_squares_batch(d, n, n, tj).cpu().numpy()
        sm, ss = (t.cpu().numpy() for t in P.sum_sse_batch(d, n, n, tj))
        for i, o in enumerate(offs):
            eq(low[i], P.hadamard(n, flat[o:], cols), "hadamard %d" % n)
            assert sq[i] == P.sum_squares_2d_i16(flat[o:], cols, n, n)
            assert (ss[i], sm[i]) == P.sum_sse_2d_i16(flat[o:], cols, n, n)
            assert (sm[i], ss[i]) == P.get_blk_sse_sum(flat[o:], cols, n, n)
        if n >= 8:
            high = P.hadamard_batch(n, d, tj, NSHIM * n * n, highbd=True).cpu().numpy()
            for i, o in enumerate(offs):
                eq(high.reshape(NSHIM, -1)[i], P.hadamard(n, flat[o:], cols, highbd=True),
                   "highbd hadamard %d" % n)
        if n in (8, 16):
            lp = P.hadamard_lp_batch(n, d, tj, NSHIM * n * n).cpu().numpy().reshape(NSHIM, -1)
            for i, o in enumerate(offs):
                eq(lp[i], P.hadamard_lp(n, flat[o:], cols), "hadamard_lp %d" % n)
    for length in (16, 1024):
        c, q = R.coeff_rows(length, NSHIM, length)
        c16, q16 = R.coeff_rows_lp(length, NSHIM, length)
        sat = P.satd_batch(dev(c)).cpu().numpy()
        slp = P.satd_lp_batch(dev(c16)).cpu().numpy()
        elp = P.block_error_lp_batch(dev(c16), dev(q16)).cpu().numpy()
        be = {bd: [t.cpu().numpy() for t in P.block_error_batch(dev(c), dev(q), bd)]
              for bd in (0, 8, 10, 12)}
        for i in range(NSHIM):
            assert sat[i] == P.satd(c[i], length)
            assert slp[i] == P.satd_lp(c16[i], length)
            assert elp[i] == P.block_error_lp(c16[i], q16[i], length)
            for bd in (0, 8, 10, 12):
                assert (be[bd][0][i], be[bd][1][i]) == P.block_error(c[i], q[i], length,
                                                                      bd or None), bd
    # subtract: the shim into a strided block, the batch into the same layout
    B, D = planes(P, 16, 8, 10, True, NSHIM)
    out = torch.zeros((NSHIM * 8, 19), dtype=torch.int16, device=DEV)
    jobs = B.jobs.copy()
    jobs["aux_off"] = np.arange(NSHIM) * 8 * 19
    P.subtract_batch(8, 16, out, D.src, D.ref, P.jobs_tensor(jobs, DEV))
    got = out.cpu().numpy()
    for i in range(NSHIM):
        diff = np.zeros((8, 19), np.int16)
        P.subtract_block(8, 16, diff, 19, B.src.reshape(-1)[jobs["src_off"][i]:], R.PW,
                         B.ref.reshape(-1)[jobs["ref_off"][i, 0]:], R.PW, True)
        eq(got[8 * i:8 * i + 8], diff, "subtract job %d" % i)


def test_a_second_identical_call_gives_identical_outputs(P):
    """No state carries over between calls on one stream."""
    B8, D8 = planes(P, 4, 4, 8, False)
    B12, D12 = planes(P, 32, 16, 12, True)
    plane = R.residual_plane("wrap", 5)
    d = dev(plane)
    offs = R.residual_offsets(plane, 32, 32, 67, 32)
    tj = P.jobs_tensor(res_jobs(P, offs, np.arange(67) * 1024), DEV)
    c, q = (dev(a) for a in R.coeff_rows(256, 67, 1))
    c16, q16 = (dev(a) for a in R.coeff_rows_lp(256, 67, 1))

    def once():
        r = []
        for B, D in ((B8, D8), (B12, D12)):
            for mode in (0, 1, 2):
                r.append(D.sad(B.nj, 4, mode))
            for kind in range(6):
                r += [x for x in D.variance(B.nj, kind) if x is not None]
        for n in (4, 8, 16, 32):
            r.append(P.hadamard_batch(n, d, tj, 67 * 1024))
        r += [P.hadamard_batch(32, d, tj, 67 * 1024, highbd=True),
              P.hadamard_lp_batch(16, d, tj, 67 * 1024), P.sum_squares_batch(d, 32, 32, tj)]
        r += list(P.sum_sse_batch(d, 32, 32, tj))
        r += [P.satd_batch(c), P.satd_lp_batch(c16), P.block_error_lp_batch(c16, q16)]
        r += list(P.block_error_batch(c, q, 0)) + list(P.block_error_batch(c, q, 12))
        return [x if isinstance(x, np.ndarray) else x.cpu().numpy().copy() for x in r]

    first, second = once(), once()
    assert len(first) == 2 * (3 + 5 * 3 + 1) + 4 + 3 + 2 + 3 + 4
    for x, y in zip(first, second):
        np.testing.assert_array_equal(x, y)
