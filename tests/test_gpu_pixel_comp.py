"""GPU parity of the masked / OBMC / distance-weighted pixel kernels
(csrc/pixel_comp.hip), bit-exact:

* the per-call RTCD shims against tests/golden/fix_pixel_comp.npz (the
  reference's own outputs), every symbol, bit depth and fixture case;
* the batch calls against tests/_compref.py (pinned to the same fixture by
  test_pixel_comp_cpu.py) on a seeded 256x320 plane;
* batch against shim on the same job, and a repeated call."""
import ctypes
import os

import numpy as np
import pytest

import _compref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(128, 128), (128, 64), (64, 128), (64, 64), (64, 32), (32, 64), (32, 32), (32, 16),
         (16, 32), (16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4), (4, 16), (16, 4),
         (8, 32), (32, 8), (16, 64), (64, 16)]
BATCH_SIZES = [(4, 4), (4, 16), (16, 4), (8, 8), (16, 16), (64, 16), (128, 128)]
SENTINEL = 0x5A5A5A5A
GUARD = 32


@pytest.fixture(scope="module")
def P():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.pixel as P
    return P


@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(GOLD, "fix_pixel_comp.npz")))


def stored(F, c):
    if c.kind == R.MSAD_X4D:
        return [int(v) for v in F["x4d"][c.ret]]
    if c.kind >= R.PRED_AVG:
        return F["pred_out"][c.ret:c.ret + c.w * c.h].astype(np.int64)
    return (c.ret, c.sse)


def call_shim(P, c):
    """A fixture case through its `_hip` symbol: (ret, sse), 4 SADs, or
    (predicted block, guards intact)."""
    hb = bool(c.highbd)
    f = P.rtcd(R.rtcd_name(c))
    pt = lambda a: P._ptr(a, hb)
    sse = np.zeros(1, np.uint32)
    jcp = ctypes.byref(P.DistWtdCompParams(1, c.fwd, c.bck))
    k = c.kind
    if k == R.MSAD:
        return f(pt(c.a), c.a_stride, pt(c.b), c.b_stride, pt(c.second), P._ptr(c.mask),
                 c.mask_stride, c.invert), 0
    if k == R.MSAD_X4D:
        return list(P.masked_sad_x4d(c.w, c.h, c.a, c.a_stride,
                                     [c.b[o:] for o in R.x4d_offsets(c.b_stride)], c.b_stride,
                                     c.second, c.mask, c.mask_stride, c.invert))
    if k == R.MSVAR:
        v = f(pt(c.a), c.a_stride, c.xoff, c.yoff, pt(c.b), c.b_stride, pt(c.second),
              P._ptr(c.mask), c.mask_stride, c.invert, P._ptr(sse))
        return v, int(sse[0])
    if k == R.OSAD:
        return f(pt(c.a), c.a_stride, P._ptr(c.wsrc), P._ptr(c.omask)), 0
    if k == R.OVAR:
        v = f(pt(c.a), c.a_stride, P._ptr(c.wsrc), P._ptr(c.omask), P._ptr(sse))
        return v, int(sse[0])
    if k == R.OSVAR:
        v = f(pt(c.a), c.a_stride, c.xoff, c.yoff, P._ptr(c.wsrc), P._ptr(c.omask), P._ptr(sse))
        return v, int(sse[0])
    if k == R.JSAD:
        return f(pt(c.a), c.a_stride, pt(c.b), c.b_stride, pt(c.second), jcp), 0
    if k == R.JSVAR:
        v = f(pt(c.a), c.a_stride, c.xoff, c.yoff, pt(c.b), c.b_stride, P._ptr(sse),
              pt(c.second), jcp)
        return v, int(sse[0])
    n = c.w * c.h
    fill = 0xA5A5 if hb else 0xA5
    buf = np.full(n + 2 * GUARD, fill, c.dtype)
    out = buf[GUARD:GUARD + n]
    if k == R.PRED_AVG:
        f(pt(out), pt(c.second), c.w, c.h, pt(c.b), c.b_stride)
    elif k == R.PRED_DIST:
        f(pt(out), pt(c.second), c.w, c.h, pt(c.b), c.b_stride, jcp)
    else:
        f(pt(out), pt(c.second), c.w, c.h, pt(c.b), c.b_stride, P._ptr(c.mask), c.mask_stride,
          c.invert)
    return out.astype(np.int64), bool((buf[:GUARD] == fill).all() and
                                      (buf[GUARD + n:] == fill).all())


@pytest.mark.parametrize("w,h", SIZES)
def test_shims_equal_the_fixture(P, F, w, h):
    rows = [r for r in F["cases"] if (r[1], r[2]) == (w, h)]
    assert len(rows) >= 60
    for row in rows:
        c = R.case_inputs(F, row)
        got, want = call_shim(P, c), stored(F, c)
        if c.kind >= R.PRED_AVG:
            np.testing.assert_array_equal(got[0], want, err_msg=R.rtcd_name(c))
            assert got[1], "guard bytes around comp_pred written: " + R.rtcd_name(c)
        else:
            assert list(got) == list(want), (R.rtcd_name(c), row.tolist())
    import lavish_dsp
    assert lavish_dsp.status()[0] == 0, lavish_dsp.status()


# ------------------------------------------------------------------ batch --
PH, PW = 256, 320
POOL = 16  # distinct second_pred / wsrc / OBMC-mask blocks


class Batch:
    """njobs jobs of one size at seeded positions of 256x320 planes, as numpy
    (for _compref) and as device tensors."""

    def __init__(self, P, w, h, bd, njobs, seed):
        import torch
        self.w, self.h, self.bd, self.nj = w, h, bd, njobs
        self.hb = bd > 8
        rng = np.random.default_rng(seed)
        dt = np.uint16 if self.hb else np.uint8
        mx = (1 << bd) - 1
        pix = lambda shape: np.where(rng.integers(0, 8, shape) == 0,
                                     rng.choice([0, 1, mx - 1, mx], shape),
                                     rng.integers(0, mx + 1, shape)).astype(dt)
        self.src, self.ref = pix((PH, PW)), pix((PH, PW))
        self.mask = np.where(rng.integers(0, 4, (PH, PW)) == 0, rng.choice([0, 64], (PH, PW)),
                             rng.integers(0, 65, (PH, PW))).astype(np.uint8)
        n = w * h
        self.second = pix(POOL * n + 1)
        self.wsrc = rng.integers(-mx * 4096, mx * 4096 + 1, POOL * n + 1).astype(np.int32)
        self.omask = np.where(rng.integers(0, 8, POOL * n + 1) == 0, 4096,
                              rng.integers(0, 4097, POOL * n + 1)).astype(np.int32)
        jobs = np.zeros(njobs, P.COMP_JOB_DTYPE)
        pos = lambda: rng.integers(0, PH - h, njobs) * PW + rng.integers(0, PW - w, njobs)
        jobs["src_off"] = pos()
        jobs["src_off"][0] |= 1  # at least one odd element offset, whatever the seed
        for k in range(4):
            jobs["ref_off"][:, k] = pos()
        jobs["ref_off"][-1, 0] |= 1
        jobs["second_off"] = rng.integers(0, POOL, njobs) * n + 1
        jobs["mask_off"] = pos()
        jobs["xoff"] = np.arange(njobs) % 8
        jobs["yoff"] = (np.arange(njobs) // 8 + rng.integers(0, 8)) % 8
        jobs["invert_mask"] = rng.integers(0, 2, njobs) * rng.integers(1, 3, njobs)
        self.jobs = jobs
        self.P = P
        dev = "cuda:0"
        t = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
        self.d = {k: t(getattr(self, k)) for k in ("src", "ref", "mask", "second", "wsrc", "omask")}
        self.djobs = P.comp_jobs_tensor(jobs, dev)

    def win(self, plane, offs, dw=0):
        """[nj, h + dw, w + dw] windows of a plane at element offsets."""
        flat = plane.reshape(-1)
        idx = (np.arange(self.h + dw)[:, None] * plane.shape[1] + np.arange(self.w + dw)[None, :])
        return flat[np.asarray(offs)[:, None, None] + idx[None]]

    def blk(self, pool, offs):
        return pool[np.asarray(offs)[:, None] + np.arange(self.w * self.h)[None]].reshape(
            -1, self.h, self.w)

    def obmc_jobs(self):
        """The same jobs with mask_off addressing the int32 OBMC mask pool."""
        import torch  # noqa: F401
        j = self.jobs.copy()
        j["mask_off"] = (np.arange(self.nj) * 5 % POOL) * self.w * self.h + 1
        return j, self.P.comp_jobs_tensor(j, "cuda:0")


def sentinel_out(n):
    import torch
    t = torch.full((n + 8,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return t


def check_tail(out, n):
    assert (out[n:].cpu().numpy() == SENTINEL).all(), "words beyond njobs * nrefs written"


NJOBS_NREFS = [(1, 3), (37, 4), (300, 1)]


@pytest.mark.parametrize("njobs,nrefs", NJOBS_NREFS)
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("w,h", BATCH_SIZES)
def test_batch_equals_restatement(P, w, h, bd, njobs, nrefs):
    B = Batch(P, w, h, bd, njobs, seed=w * 131 + h * 7 + bd + njobs)
    j, d = B.jobs, B.d
    S = B.blk(B.second, j["second_off"])
    src = B.win(B.src, j["src_off"])
    src_w = B.win(B.src, j["src_off"], 1)
    M = B.win(B.mask, j["mask_off"])
    inv = j["invert_mask"]
    refs = [B.win(B.ref, j["ref_off"][:, k]) for k in range(nrefs)]
    fwd, bck = [(9, 7), (5, 11), (12, 4), (3, 13)][(w + h + bd + njobs) % 4]

    # masked / distance-weighted SAD
    for mode in (0, 1):
        out = sentinel_out(njobs * nrefs)
        got = P.comp_sad_batch(d["src"], d["ref"], w, h, B.djobs, nrefs, mode, d["second"],
                               d["mask"], fwd, bck, out=out).cpu().numpy()
        want = np.stack([R.masked_sad(src, r, S, M, inv) if mode == 0 else
                         R.dist_wtd_sad_avg(src, r, S, fwd, bck) for r in refs], 1)
        np.testing.assert_array_equal(got, want, err_msg="comp_sad mode %d" % mode)
        check_tail(out, njobs * nrefs)

    # masked / distance-weighted sub-pixel variance: src is the filtered operand
    for kind in (0, 1):
        vo, so = sentinel_out(njobs), sentinel_out(njobs)
        var, sse = P.comp_variance_batch(d["src"], d["ref"], w, h, B.djobs, kind, bd, d["second"],
                                         d["mask"], fwd, bck, var_out=vo, sse_out=so)
        if kind == 0:
            wv, ws = R.masked_sub_pixel_variance(src_w, j["xoff"], j["yoff"], refs[0], S, M, inv, bd)
        else:
            wv, ws = R.dist_wtd_sub_pixel_avg_variance(src_w, j["xoff"], j["yoff"], refs[0], S,
                                                       fwd, bck, bd)
        np.testing.assert_array_equal(var.cpu().numpy(), wv, err_msg="comp_variance %d" % kind)
        np.testing.assert_array_equal(sse.cpu().numpy(), ws, err_msg="comp_variance sse %d" % kind)
        check_tail(vo, njobs)
        check_tail(so, njobs)

    # OBMC: the predictors are the ref positions
    oj, doj = B.obmc_jobs()
    W, OM = B.blk(B.wsrc, oj["second_off"]), B.blk(B.omask, oj["mask_off"])
    out = sentinel_out(njobs * nrefs)
    got = P.obmc_batch(d["ref"], w, h, doj, d["wsrc"], d["omask"], nrefs, 0, bd,
                       out=out).cpu().numpy()
    np.testing.assert_array_equal(got, np.stack([R.obmc_sad(r, W, OM) for r in refs], 1),
                                  err_msg="obmc sad")
    check_tail(out, njobs * nrefs)
    ref_w = B.win(B.ref, oj["ref_off"][:, 0], 1)
    for kind in (1, 2):
        vo, so = sentinel_out(njobs), sentinel_out(njobs)
        var, sse = P.obmc_batch(d["ref"], w, h, doj, d["wsrc"], d["omask"], 1, kind, bd, out=vo,
                                sse_out=so)
        wv, ws = R.obmc_variance(refs[0], W, OM, bd) if kind == 1 else \
            R.obmc_sub_pixel_variance(ref_w, oj["xoff"], oj["yoff"], W, OM, bd)
        np.testing.assert_array_equal(var.cpu().numpy(), wv, err_msg="obmc kind %d" % kind)
        np.testing.assert_array_equal(sse.cpu().numpy(), ws, err_msg="obmc sse kind %d" % kind)
        check_tail(vo, njobs)
        check_tail(so, njobs)

    # prediction: job k writes block k of comp_pred (src_off = k * w * h + 3)
    import torch
    n = w * h
    pj = j.copy()
    pj["src_off"] = np.arange(njobs) * n + 3
    dpj = P.comp_jobs_tensor(pj, "cuda:0")
    fill = -23131 if B.hb else 0xA5  # 0xA5A5 as int16
    for mode in (0, 1, 2):
        comp = torch.full((njobs * n + 6,), fill, dtype=d["src"].dtype, device="cuda:0")
        P.comp_pred_batch(comp, d["second"], w, h, d["ref"], dpj, mode, d["mask"], fwd, bck)
        got = comp.cpu().numpy()
        got = got.view(np.uint16) if B.hb else got
        want = (R.avg_pred(refs[0], S), R.dist_wtd_pred(refs[0], S, fwd, bck),
                R.mask_pred(refs[0], S, M, inv))[mode]
        np.testing.assert_array_equal(got[3:3 + njobs * n].astype(np.int64), want.reshape(-1),
                                      err_msg="comp_pred mode %d" % mode)
        g = np.array([fill], np.int16).view(np.uint16)[0] if B.hb else fill
        assert (got[:3] == g).all() and (got[3 + njobs * n:] == g).all()
    assert j["src_off"][0] & 1


def _plane2d(flat, stride, rows):
    out = np.zeros(rows * stride, flat.dtype)
    n = min(out.size, flat.size)
    out[:n] = flat[:n]
    return out.reshape(rows, stride)


@pytest.mark.parametrize("w,h", [(4, 4), (16, 16), (64, 16), (128, 128)])
def test_batch_equals_shim_on_the_same_job(P, F, w, h):
    """Every fixture case of the size through the batch call on one job: the
    same words as the shim (and so as the reference)."""
    import torch
    dev = "cuda:0"
    t = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
    done = set()
    for row in F["cases"]:
        if (row[1], row[2]) != (w, h) or row[0] >= R.PRED_AVG:
            continue
        c = R.case_inputs(F, row)
        shim = call_shim(P, c)
        a = t(_plane2d(c.a, c.a_stride, h + 2))
        b = t(_plane2d(c.b, c.b_stride, h + 2))
        m = t(_plane2d(c.mask, c.mask_stride, h + 1))
        jb = np.zeros(1, P.COMP_JOB_DTYPE)
        jb["xoff"], jb["yoff"], jb["invert_mask"] = c.xoff, c.yoff, c.invert
        jb["ref_off"][0] = R.x4d_offsets(c.b_stride)
        dj = P.comp_jobs_tensor(jb, dev)
        k = c.kind
        if k in (R.MSAD, R.MSAD_X4D, R.JSAD):
            nrefs = 4 if k == R.MSAD_X4D else 1
            got = P.comp_sad_batch(a, b, w, h, dj, nrefs, int(k == R.JSAD), t(c.second), m,
                                   c.fwd, c.bck).cpu().numpy()[0]
            got = list(got) if nrefs == 4 else (int(got[0]), 0)
        elif k in (R.MSVAR, R.JSVAR):
            v, s = P.comp_variance_batch(a, b, w, h, dj, int(k == R.JSVAR), c.bd, t(c.second), m,
                                         c.fwd, c.bck)
            got = (int(v[0]), int(s[0]))
        elif k == R.OSAD:
            got = (int(P.obmc_batch(a, w, h, dj, t(c.wsrc), t(c.omask), 1, 0, c.bd)[0, 0]), 0)
        else:
            v, s = P.obmc_batch(a, w, h, dj, t(c.wsrc), t(c.omask), 1, 1 if k == R.OVAR else 2,
                                c.bd)
            got = (int(v[0]), int(s[0]))
        assert list(got) == list(shim), (R.rtcd_name(c), row.tolist())
        done.add(k)
    assert len(done) == 8


def test_a_second_identical_call_gives_identical_outputs(P):
    """No state carries over between calls on one stream."""
    import torch
    B = Batch(P, 16, 16, 10, 300, seed=99)
    d = B.d
    oj, doj = B.obmc_jobs()
    n = 256
    pj = B.jobs.copy()
    pj["src_off"] = np.arange(B.nj) * n
    dpj = P.comp_jobs_tensor(pj, "cuda:0")

    def once():
        r = [P.comp_sad_batch(d["src"], d["ref"], 16, 16, B.djobs, 4, m, d["second"], d["mask"], 11,
                              5) for m in (0, 1)]
        for k in (0, 1):
            r += list(P.comp_variance_batch(d["src"], d["ref"], 16, 16, B.djobs, k, 10, d["second"],
                                            d["mask"], 11, 5))
        r.append(P.obmc_batch(d["ref"], 16, 16, doj, d["wsrc"], d["omask"], 4, 0, 10))
        for k in (1, 2):
            r += list(P.obmc_batch(d["ref"], 16, 16, doj, d["wsrc"], d["omask"], 1, k, 10))
        for mode in (0, 1, 2):
            comp = torch.zeros(B.nj * n, dtype=torch.int16, device="cuda:0")
            P.comp_pred_batch(comp, d["second"], 16, 16, d["ref"], dpj, mode, d["mask"], 11, 5)
            r.append(comp)
        return [x.cpu().numpy().copy() for x in r]

    first, second = once(), once()
    assert len(first) == 14
    for x, y in zip(first, second):
        np.testing.assert_array_equal(x, y)
