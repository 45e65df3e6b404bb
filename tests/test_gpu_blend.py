"""GPU parity of the mask-building and blending layer (csrc/blend.hip),
bit-exact, no tolerance anywhere:

* the 14 per-call RTCD shims against tests/golden/fix_blend.npz (the
  reference's own outputs), every fixture case;
* the five batch calls against tests/_blendref.py (pinned to the same fixture
  by test_blend_cpu.py) on seeded jobs whose counts end in a partial lane
  group and a partial workgroup, and the OBMC calls on the fixture's scenes;
* batch against shim on the same job, in-place blends, a repeated call;
* chain 1: two first-pass convolves -> d16 diff-weighted mask -> d16 blend,
  against the restatement of av1_make_masked_inter_predictor's arithmetic;
* chain 2: the device-built wsrc / mask through the OBMC full-pel search."""
import os

import numpy as np
import pytest

import _blendref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def B():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.blend as B
    return B


@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(GOLD, "fix_blend.npz")))


def dev(a):
    """numpy -> device tensor (uint16 as its int16 view)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def gather(plane, offs, stride, h, w):
    idx = np.asarray(offs)[:, None, None] + np.arange(h)[None, :, None] * stride + np.arange(w)
    return np.asarray(plane).reshape(-1)[idx].astype(np.int64)


def pdt(highbd):
    return np.uint16 if highbd else np.uint8


# ------------------------------------------------------------------ shims --
def shim_blend(B, c):
    """A fixture blend case through its `_hip` symbol, into a guarded buffer:
    (block, guards intact)."""
    d16 = c.form == R.F_D16
    ds, s0s, s1s = c.w + 5, c.w + 3, c.w + 2
    fill = 0xA5A5 if c.highbd else 0xA5
    dst = np.full((c.h + 2, ds), fill, pdt(c.highbd))
    st = np.uint16 if d16 or c.highbd else np.uint8

    def emb(a, stride, dt):
        b = np.zeros(a.shape[:-1] + (stride,), dt)
        b[..., :a.shape[-1]] = a
        return b
    s0, s1 = emb(c.s0, s0s, st), emb(c.s1, s1s, st)
    out = dst[1:, 1:]
    if c.form in (R.F_HMASK, R.F_VMASK):
        mask = c.mask.astype(np.uint8)
        name = ("aom_highbd_" if c.highbd else "aom_") + \
            ("blend_a64_hmask" if c.form == R.F_HMASK else "blend_a64_vmask")
        args = [out, ds, s0, s0s, s1, s1s, mask, c.w, c.h] + ([c.bd] if c.highbd else [])
    else:
        ms = c.mask.shape[1] + 7
        mask = emb(c.mask, ms, np.uint8)
        args = [out, ds, s0, s0s, s1, s1s, mask, ms, c.w, c.h, c.subw, c.subh]
        if d16:
            name = "aom_highbd_blend_a64_d16_mask" if c.highbd else "aom_lowbd_blend_a64_d16_mask"
            args += [B.conv_params(c.r0, c.r1)] + ([c.bd] if c.highbd else [])
        else:
            name = "aom_highbd_blend_a64_mask" if c.highbd else "aom_blend_a64_mask"
            args += [c.bd] if c.highbd else []
    getattr(B, name)(*args)
    got = dst[1:1 + c.h, 1:1 + c.w].astype(np.int64)
    dst[1:1 + c.h, 1:1 + c.w] = fill
    return got, bool((dst == fill).all())


def test_blend_shims_equal_the_fixture(B, F):
    names = set()
    for row in F["blend_cases"]:
        c = R.blend_case(F, row)
        got, guards = shim_blend(B, c)
        want = F["blend_out"][c.out_off:c.out_off + c.w * c.h].astype(np.int64).reshape(c.h, c.w)
        np.testing.assert_array_equal(got, want, err_msg=str(row.tolist()))
        assert guards, "pixels around dst written: %s" % row.tolist()
        names.add((c.form, c.highbd))
    assert len(names) == 8
    import lavish_dsp
    assert lavish_dsp.status()[0] == 0


def test_diffwtd_shims_equal_the_fixture(B, F):
    for row in F["dw_cases"]:
        c = R.diffwtd_case(F, row)
        st = np.uint8 if c.form == 0 else np.uint16
        s0 = np.zeros((c.h, c.w + 2), st)
        s1 = np.zeros((c.h, c.w + 7), st)
        s0[:, :c.w], s1[:, :c.w] = c.s0, c.s1
        buf = np.full(c.w * c.h + 64, 0xA5, np.uint8)
        mask = buf[32:32 + c.w * c.h]
        if c.form == 0:
            B.av1_build_compound_diffwtd_mask(mask, c.mask_type, s0, c.w + 2, s1, c.w + 7, c.h, c.w)
        elif c.form == 1:
            B.av1_build_compound_diffwtd_mask_highbd(mask, c.mask_type, s0, c.w + 2, s1, c.w + 7,
                                                     c.h, c.w, c.bd)
        else:
            B.av1_build_compound_diffwtd_mask_d16(mask, c.mask_type, s0, c.w + 2, s1, c.w + 7,
                                                  c.h, c.w, B.conv_params(c.r0, c.r1), c.bd)
        np.testing.assert_array_equal(mask, F["dw_out"][c.out_off:c.out_off + c.w * c.h],
                                      err_msg=str(row.tolist()))
        assert (buf[:32] == 0xA5).all() and (buf[32 + c.w * c.h:] == 0xA5).all()


def test_wedge_shims_equal_the_fixture(B, F):
    for row in F["wedge_cases"]:
        c = R.wedge_case(F, row)
        a, b, m = c.a.astype(np.int16), c.b.astype(np.int16), c.m.astype(np.uint8)
        if c.kind == 0:
            d = np.full(c.n + 16, 0x5A5A, np.int16)
            B.av1_wedge_compute_delta_squares(d[8:8 + c.n], a, b, c.n)
            np.testing.assert_array_equal(d[8:8 + c.n], F["wedge_out"][c.ret:c.ret + c.n])
            assert (d[:8] == 0x5A5A).all() and (d[8 + c.n:] == 0x5A5A).all()
        elif c.kind == 1:
            assert B.av1_wedge_sse_from_residuals(a, b, m, c.n) == c.ret, row.tolist()
        else:
            assert B.av1_wedge_sign_from_residuals(a, m, c.n, c.limit) == c.ret, row.tolist()


# ------------------------------------------------------------ batch blend --
class Grid:
    """nj blocks of w x h on a grid with odd gaps, so block offsets take every
    byte alignment; off[j] is block j's first element."""

    def __init__(self, w, h, nj, gx=3, gy=1):
        self.cols = max(1, min(nj, 512 // (w + gx)))
        rows = (nj + self.cols - 1) // self.cols
        self.stride = self.cols * (w + gx) + 5
        self.shape = (rows * (h + gy) + 1, self.stride)
        j = np.arange(nj)
        self.off = ((j // self.cols) * (h + gy) + 1) * self.stride + (j % self.cols) * (w + gx) + 1
        self.w, self.h = w, h

    def inside(self):
        m = np.zeros(self.shape, bool).reshape(-1)
        idx = self.off[:, None, None] + np.arange(self.h)[None, :, None] * self.stride + \
            np.arange(self.w)
        m[idx.reshape(-1)] = True
        return m.reshape(self.shape)


# (w, h, njobs, kind, subw, subh, d16, bd, highbd)
BLEND_CONFIGS = [
    (4, 4, 1, 0, 0, 0, 0, 8, 0), (4, 4, 17, 0, 1, 1, 0, 8, 0), (4, 4, 67, 0, 1, 0, 0, 10, 1),
    (4, 4, 67, 0, 0, 1, 1, 8, 0), (4, 4, 17, 1, 0, 0, 0, 8, 0), (4, 4, 67, 2, 0, 0, 0, 12, 1),
    (64, 64, 5, 0, 0, 0, 0, 8, 0), (64, 64, 5, 0, 1, 1, 1, 12, 1), (64, 64, 5, 1, 0, 0, 0, 10, 1),
    (64, 64, 5, 2, 0, 0, 0, 8, 0), (64, 64, 5, 0, 1, 0, 1, 8, 0), (16, 16, 33, 0, 0, 1, 0, 12, 1),
    (16, 16, 17, 0, 1, 1, 1, 10, 1), (128, 128, 3, 0, 1, 1, 0, 8, 0), (128, 128, 2, 0, 0, 0, 1, 12, 1),
    (4, 16, 19, 0, 1, 0, 0, 8, 0), (16, 4, 19, 0, 0, 1, 0, 8, 1), (32, 8, 9, 0, 0, 0, 1, 10, 1),
    (8, 8, 35, 0, 1, 1, 0, 8, 0), (8, 32, 9, 2, 0, 0, 0, 8, 0), (64, 32, 5, 0, 0, 1, 1, 8, 0),
    # the 2x2 block and the 1- and 2-wide chroma OBMC spans
    (2, 2, 67, 0, 1, 1, 0, 8, 0), (2, 2, 17, 0, 0, 0, 0, 10, 1), (1, 16, 17, 2, 0, 0, 0, 8, 0),
    (1, 4, 67, 0, 1, 0, 0, 8, 0), (1, 4, 17, 1, 0, 0, 0, 12, 1), (2, 8, 17, 1, 0, 0, 0, 10, 1),
    (8, 2, 17, 2, 0, 0, 0, 8, 0), (8, 1, 9, 0, 0, 1, 0, 8, 0), (2, 8, 9, 0, 1, 1, 0, 12, 1)]


def blend_setup(B, rng, cfg):
    w, h, nj, kind, subw, subh, d16, bd, highbd = cfg
    g0, g1, gd = Grid(w, h, nj, 3, 1), Grid(w, h, nj, 5, 2), Grid(w, h, nj, 1, 1)
    st = np.uint16 if d16 or highbd else np.uint8
    if d16:
        r0 = 5 if bd == 12 else 3
        roff, rbits = R.d16_rounding(r0, 7, bd)
        # the first-pass range of CONV_BUF values and a margin that makes the clip work
        lo, hi = roff - (40 << rbits), roff + (((1 << bd) + 40) << rbits)
        cp = B.conv_params(r0, 7)
    else:
        lo, hi, cp, r0 = 0, 1 << bd, None, 0
    s0 = rng.integers(lo, hi, g0.shape).astype(st)
    s1 = rng.integers(lo, hi, g1.shape).astype(st)
    if kind == 0:
        gm = Grid(w << subw, h << subh, nj, 3, 1)
        mask = rng.integers(0, 65, gm.shape).astype(np.uint8)
        mask[rng.integers(0, 4, gm.shape) == 0] = 64
        mask[rng.integers(0, 4, gm.shape) == 0] = 0
        moff, ms = gm.off, gm.stride
        mwin = gather(mask, moff, ms, h << subh, w << subw)
    else:
        n = w if kind == 1 else h
        mask = rng.integers(0, 65, nj * 5 + n + 8).astype(np.uint8)
        moff, ms = np.arange(nj) * 5 + 1, 0
        mwin = gather(mask, moff, 0, 1, n)[:, 0, :]
    a0, a1 = gather(s0, g0.off, g0.stride, h, w), gather(s1, g1.off, g1.stride, h, w)
    if kind == 1:
        exp = R.blend_a64_hmask(a0, a1, mwin)
    elif kind == 2:
        exp = R.blend_a64_vmask(a0, a1, mwin)
    elif d16:
        exp = R.blend_a64_d16_mask(a0, a1, mwin, subw, subh, r0, 7, bd)
    else:
        exp = R.blend_a64_mask(a0, a1, mwin, subw, subh)
    jobs = np.zeros(nj, B.COMP_JOB_DTYPE)
    jobs["ref_off"][:, 0], jobs["ref_off"][:, 1], jobs["mask_off"] = g0.off, g1.off, moff
    return dict(g0=g0, g1=g1, gd=gd, s0=s0, s1=s1, mask=mask, ms=ms, jobs=jobs, exp=exp, cp=cp)


@pytest.mark.parametrize("cfg", BLEND_CONFIGS, ids=lambda c: "x".join(str(v) for v in c))
def test_blend_batch_equals_the_restatement(B, cfg):
    import torch
    w, h, nj, kind, subw, subh, d16, bd, highbd = cfg
    rng = np.random.default_rng(hash(cfg) & 0xFFFF)
    S = blend_setup(B, rng, cfg)
    gd = S["gd"]
    S["jobs"]["src_off"] = gd.off
    fill = 0xA5A5 if highbd else 0xA5
    ts0, ts1, tm, tj = dev(S["s0"]), dev(S["s1"]), dev(S["mask"]), B.comp_jobs_tensor(S["jobs"], "cuda")
    outs = []
    for _ in range(2):     # a second identical call gives identical outputs
        dst = dev(np.full(gd.shape, fill, pdt(highbd)))
        B.blend_a64_batch(dst, ts0, ts1, tm, w, h, tj, kind, subw, subh, bool(d16), bd, S["cp"],
                          mask_stride=S["ms"])
        torch.cuda.synchronize()
        outs.append(host(dst, pdt(highbd)))
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(gather(outs[0], gd.off, gd.stride, h, w), S["exp"])
    assert (outs[0][~gd.inside()] == fill).all(), "pixels outside the dst blocks written"


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("cfg", [(4, 4, 67, 0, 1, 1, 0, 8, 0), (64, 64, 5, 0, 0, 0, 0, 10, 1),
                                 (16, 16, 17, 2, 0, 0, 0, 8, 0), (8, 32, 9, 1, 0, 0, 0, 12, 1),
                                 (2, 2, 17, 0, 0, 1, 0, 8, 0), (128, 128, 2, 0, 1, 0, 0, 8, 0)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_blend_in_place(B, cfg, which):
    """dst = src0 (which 0) or src1 (which 1), equal strides."""
    import torch
    w, h, nj, kind, subw, subh, d16, bd, highbd = cfg
    S = blend_setup(B, np.random.default_rng(99 + which), cfg)
    g = S["g1"] if which else S["g0"]
    S["jobs"]["src_off"] = g.off
    ts = [dev(S["s0"]), dev(S["s1"])]
    B.blend_a64_batch(ts[which], ts[0], ts[1], dev(S["mask"]), w, h,
                      B.comp_jobs_tensor(S["jobs"], "cuda"), kind, subw, subh, False, bd,
                      mask_stride=S["ms"])
    torch.cuda.synchronize()
    got = host(ts[which], pdt(highbd))
    np.testing.assert_array_equal(gather(got, g.off, g.stride, h, w), S["exp"])
    before = S["s1"] if which else S["s0"]
    assert (got[~g.inside()] == before[~g.inside()]).all()
    np.testing.assert_array_equal(host(ts[1 - which], pdt(highbd)), S["s0"] if which else S["s1"])


# (w, h, njobs, form 0 u8 / 1 highbd / 2 d16, bd)
DW_CONFIGS = [(4, 4, 67, 0, 8), (4, 4, 17, 2, 8), (8, 8, 17, 1, 10), (64, 64, 5, 2, 12),
              (16, 4, 19, 2, 10), (4, 16, 19, 1, 12), (128, 128, 2, 1, 8), (32, 32, 1, 0, 8),
              (64, 64, 5, 0, 8)]


@pytest.mark.parametrize("cfg", DW_CONFIGS, ids=lambda c: "x".join(str(v) for v in c))
def test_diffwtd_batch_equals_the_restatement(B, cfg):
    import torch
    w, h, nj, form, bd = cfg
    rng = np.random.default_rng(hash(cfg) & 0xFFFF)
    g0, g1 = Grid(w, h, nj, 3, 1), Grid(w, h, nj, 5, 2)
    r0 = 5 if bd == 12 else 3
    if form == 2:
        roff, rbits = R.d16_rounding(r0, 7, bd)
        lo, hi = roff - (40 << rbits), roff + (((1 << bd) + 40) << rbits)
    else:
        lo, hi = 0, 1 << bd
    st = np.uint8 if form == 0 else np.uint16
    s0 = rng.integers(lo, hi, g0.shape).astype(st)
    s1 = rng.integers(lo, hi, g1.shape).astype(st)
    if form == 2 and nj > 1:
        # job 0: a difference past the pixel range (filter overshoot), which clamps at
        # 64; job 1: equal inputs, which stay at 38 (26 inverted)
        blk = lambda g, j: (slice(g.off[j] // g.stride, g.off[j] // g.stride + h),
                            slice(g.off[j] % g.stride, g.off[j] % g.stride + w))
        s1[blk(g1, 0)] = roff - 3000
        s0[blk(g0, 0)] = roff - 3000 + (416 << (rbits + bd - 8))
        s1[blk(g1, 1)] = s0[blk(g0, 1)]
    a0, a1 = gather(s0, g0.off, g0.stride, h, w), gather(s1, g1.off, g1.stride, h, w)
    mt = np.arange(nj) % 2
    exp = R.diffwtd_mask_d16(a0, a1, mt, r0, 7, bd) if form == 2 else R.diffwtd_mask(a0, a1, mt, bd)
    jobs = np.zeros(nj, B.COMP_JOB_DTYPE)
    jobs["ref_off"][:, 0], jobs["ref_off"][:, 1] = g0.off, g1.off
    jobs["mask_off"] = (nj - 1 - np.arange(nj)) * w * h + 16   # reversed: read per job
    jobs["invert_mask"] = mt
    mask = torch.full((nj * w * h + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    B.diffwtd_mask_batch(mask, dev(s0), dev(s1), w, h, B.comp_jobs_tensor(jobs, "cuda"),
                         d16=form == 2, bit_depth=bd,
                         conv_params=B.conv_params(r0, 7) if form == 2 else None)
    torch.cuda.synchronize()
    got = mask.cpu().numpy()
    np.testing.assert_array_equal(got[16:-16].reshape(nj, h, w)[::-1], exp)
    assert (got[:16] == 0xA5).all() and (got[-16:] == 0xA5).all()
    if form == 2 and nj > 1:
        assert (exp[0] == 64).all() and (exp[1] == 26).all()


# ------------------------------------------------------------------- OBMC --
def obmc_setup(B, rng, bw, bh, nj, bd, ssx=0, ssy=0):
    """nj jobs with seeded bitmaps (all-set, none, and random spans of one or
    more mi) on three planes of the plane's block size."""
    pw, ph = bw >> ssx, bh >> ssy
    gs, ga, gl = Grid(pw, ph, nj, 3, 1), Grid(pw, ph, nj, 5, 2), Grid(pw, ph, nj, 1, 1)
    dt = pdt(bd > 8)
    src, above, left = (rng.integers(0, 1 << bd, g.shape).astype(dt) for g in (gs, ga, gl))
    full_w, full_h = (1 << (bw // 4)) - 1, (1 << (bh // 4)) - 1
    am = rng.integers(0, 1 << 32, nj, dtype=np.uint64) & full_w
    lm = rng.integers(0, 1 << 32, nj, dtype=np.uint64) & full_h
    am[0::5], lm[0::5] = full_w, full_h
    am[1::5] = 0
    lm[2::5] = 0
    jobs = np.zeros(nj, B.OBMC_JOB_DTYPE)
    jobs["src_off"], jobs["above_off"], jobs["left_off"] = gs.off, ga.off, gl.off
    jobs["above_mask"], jobs["left_mask"] = am, lm
    jobs["wsrc_off"] = (nj - 1 - np.arange(nj)) * bw * bh
    jobs["mask_off"] = np.arange(nj) * bw * bh
    return dict(gs=gs, ga=ga, gl=gl, src=src, above=above, left=left, jobs=jobs,
                a=gather(src, gs.off, gs.stride, ph, pw), b=gather(above, ga.off, ga.stride, ph, pw),
                c=gather(left, gl.off, gl.stride, ph, pw))


@pytest.mark.parametrize("bw,bh,nj,bd", [(8, 8, 67, 8), (16, 16, 17, 8), (16, 16, 5, 12),
                                         (64, 16, 5, 8), (64, 64, 5, 10), (128, 128, 2, 8),
                                         (8, 32, 9, 12), (32, 8, 9, 8), (128, 64, 1, 12)])
def test_obmc_wsrc_batch_equals_the_restatement(B, F, bw, bh, nj, bd):
    import torch
    S = obmc_setup(B, np.random.default_rng(bw * 131 + bh + bd), bw, bh, nj, bd)
    tab = dev(F["obmc_masks"])
    n = nj * bw * bh
    outs = []
    for _ in range(2):
        wsrc = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        mask = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        B.obmc_wsrc_batch(dev(S["src"]), dev(S["above"]), dev(S["left"]), bw, bh,
                          B.obmc_jobs_tensor(S["jobs"], "cuda"), tab, wsrc, mask)
        torch.cuda.synchronize()
        outs.append((wsrc.cpu().numpy(), mask.cpu().numpy()))
    for k in (0, 1):
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
        assert (outs[0][k][n:] == 0x5A5A5A5A).all()
    jb = S["jobs"]
    for j in range(nj):
        ws, mk = R.obmc_wsrc(S["a"][j], S["b"][j], S["c"][j], jb["above_mask"][j],
                             jb["left_mask"][j], F["obmc_masks"])
        o = int(jb["wsrc_off"][j])
        np.testing.assert_array_equal(outs[0][0][o:o + bw * bh].reshape(bh, bw), ws, err_msg=str(j))
        o = int(jb["mask_off"][j])
        np.testing.assert_array_equal(outs[0][1][o:o + bw * bh].reshape(bh, bw), mk, err_msg=str(j))


@pytest.mark.parametrize("bw,bh,nj,bd,ss", [(8, 8, 67, 8, 0), (8, 8, 67, 8, 1), (16, 8, 17, 10, 1),
                                            (8, 16, 17, 8, 1), (16, 16, 17, 12, 1),
                                            (16, 16, 33, 8, 0), (64, 64, 5, 8, 1),
                                            (64, 16, 5, 10, 0), (128, 128, 2, 8, 0),
                                            (128, 128, 3, 12, 1), (32, 8, 9, 8, 0)])
def test_obmc_blend_batch_equals_the_restatement(B, F, bw, bh, nj, bd, ss):
    import torch
    S = obmc_setup(B, np.random.default_rng(bw * 17 + bh + bd + ss), bw, bh, nj, bd, ss, ss)
    pw, ph = bw >> ss, bh >> ss
    gs = S["gs"]
    dst = dev(S["src"])
    B.obmc_blend_batch(dst, dev(S["above"]), dev(S["left"]), bw, bh,
                       B.obmc_jobs_tensor(S["jobs"], "cuda"), dev(F["obmc_masks"]), ss, ss)
    torch.cuda.synchronize()
    got = host(dst, pdt(bd > 8))
    jb = S["jobs"]
    for j in range(nj):
        exp = R.obmc_blend(S["a"][j], S["b"][j], S["c"][j], jb["above_mask"][j], jb["left_mask"][j],
                           bw, bh, ss, ss, F["obmc_masks"])
        np.testing.assert_array_equal(gather(got, gs.off[j:j + 1], gs.stride, ph, pw)[0], exp,
                                      err_msg=str(j))
    assert (got[~gs.inside()] == S["src"][~gs.inside()]).all()


def test_obmc_batches_equal_the_fixture_scenes(B, F):
    """The fixture's scenes (the reference's own walk and outputs) through the
    two OBMC calls: every scene and plane one job."""
    import torch
    tab = dev(F["obmc_masks"])
    for row in F["obmc_cases"]:
        c = R.obmc_case(F, row)
        sc, bd = c.sc, c.sc["bd"]
        dt = pdt(bd > 8)
        jobs = np.zeros(1, B.OBMC_JOB_DTYPE)
        jobs["src_off"], jobs["above_off"], jobs["left_off"] = c.src_off, c.above_off, c.left_off
        jobs["above_mask"], jobs["left_mask"] = c.above_mask, c.left_mask
        tj = B.obmc_jobs_tensor(jobs, "cuda")
        pa, pb = F["pa_bd%d" % bd].astype(dt), F["pb_bd%d" % bd].astype(dt)
        n = c.pw * c.ph
        if c.plane == 0:
            wsrc = torch.zeros(n, dtype=torch.int32, device="cuda")
            mask = torch.zeros(n, dtype=torch.int32, device="cuda")
            B.obmc_wsrc_batch(dev(pa), dev(pb), dev(pb), sc["bw"], sc["bh"], tj, tab, wsrc, mask)
            np.testing.assert_array_equal(wsrc.cpu().numpy(),
                                          F["obmc_wsrc"][c.wsrc_off:c.wsrc_off + n], sc["name"])
            np.testing.assert_array_equal(mask.cpu().numpy(),
                                          F["obmc_mask"][c.wsrc_off:c.wsrc_off + n], sc["name"])
        dst = dev(pa)
        B.obmc_blend_batch(dst, dev(pb), dev(pb), sc["bw"], sc["bh"], tj, tab, c.ssx, c.ssy)
        got = R.win(host(dst, dt), c.src_off, R.A_STRIDE, c.ph, c.pw)
        np.testing.assert_array_equal(got.reshape(-1), F["obmc_pred"][c.pred_off:c.pred_off + n],
                                      err_msg="%s plane %d" % (sc["name"], c.plane))


# ------------------------------------------------------------------ wedge --
@pytest.mark.parametrize("nj", [1, 5, 9])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_wedge_batch_equals_the_restatement(B, F, kind, nj):
    """Jobs of different N in one call (4 jobs to a workgroup: 1, 5 and 9 end
    in a partial one); 12-bit-range residuals, so the sse clamp engages."""
    import torch
    rng = np.random.default_rng(kind * 10 + nj)
    ns = np.array([64, 16384, 128, 1024, 64, 4096, 128, 64, 16384])[:nj]
    tot = int(ns.sum()) + 64
    lim = 4095 if kind != 2 else 32767
    a = rng.integers(-lim, lim + 1, tot).astype(np.int16)
    b = rng.integers(-4095, 4096, tot).astype(np.int16)
    a[:64:2] = a[:64:2] // 64            # some small residuals: unclamped terms too
    m = rng.integers(0, 65, tot).astype(np.uint8)
    wm = F["wedge_masks_32x32"][7, 1].reshape(-1)
    m[:1024] = wm[:min(1024, tot)] if tot >= 1024 else m[:1024]
    jobs = np.zeros(nj, B.WEDGE_JOB_DTYPE)
    starts = np.concatenate([[0], np.cumsum(ns)[:-1]])
    jobs["a_off"], jobs["b_off"], jobs["m_off"] = starts + 1, starts + 3, starts + 5
    jobs["out_off"], jobs["n"] = starts + 7, ns
    accs = [R.wedge_sign_acc(a[s + 1:s + 1 + n], m[s + 5:s + 5 + n]) for s, n in zip(starts, ns)]
    jobs["limit"] = [acc - (j % 3 == 1) + (j % 3 == 2) for j, acc in enumerate(accs)]
    tj = B.wedge_jobs_tensor(jobs, "cuda")
    ta, tb, tm = dev(a), dev(b), dev(m)
    if kind == 0:
        out = torch.full((tot + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        B.wedge_batch(ta, tb, None, tj, kind, out=out)
        got = out.cpu().numpy()
        seen = np.zeros(tot + 16, bool)
        for s, n in zip(starts, ns):
            exp = R.wedge_delta_squares(a[s + 1:s + 1 + n], b[s + 3:s + 3 + n])
            np.testing.assert_array_equal(got[s + 7:s + 7 + n], exp)
            seen[s + 7:s + 7 + n] = True
        assert (got[~seen] == 0x5A5A).all()
        return
    out = torch.full((nj + 3,), 0x5A, dtype=torch.int64 if kind == 1 else torch.int8, device="cuda")
    out2 = out.clone()
    B.wedge_batch(ta, tb, tm, tj, kind, out=out)
    B.wedge_batch(ta, tb, tm, tj, kind, out=out2)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, out2.cpu().numpy())
    assert (got[nj:] == 0x5A).all()
    for j, (s, n) in enumerate(zip(starts, ns)):
        if kind == 1:
            exp = R.wedge_sse_from_residuals(a[s + 1:s + 1 + n], b[s + 3:s + 3 + n],
                                             m[s + 5:s + 5 + n])
        else:
            exp = int(accs[j] > int(jobs["limit"][j]))
            assert exp == (j % 3 == 1)        # acc == limit is not greater
        assert int(got[j]) == exp, (j, n)


# -------------------------------------------------------- batch and shim ----
def test_batch_equals_shim_on_the_same_job(B, F):
    import torch
    rng = np.random.default_rng(5)
    w, h = 16, 8
    for bd, hb in ((8, 0), (12, 1)):
        dt = pdt(hb)
        s0 = rng.integers(0, 1 << bd, (h, w + 3)).astype(dt)
        s1 = rng.integers(0, 1 << bd, (h, w + 6)).astype(dt)
        mask = rng.integers(0, 65, (2 * h, 2 * w + 1)).astype(np.uint8)
        jobs = np.zeros(1, B.COMP_JOB_DTYPE)
        for kind, subw, subh in ((0, 1, 1), (0, 0, 0), (1, 0, 0), (2, 0, 0)):
            out = np.zeros((h, w), dt)
            m = mask if kind == 0 else mask[0]
            if kind == 0:
                args = [out, w, s0, w + 3, s1, w + 6, m, 2 * w + 1, w, h, subw, subh]
                name = "blend_a64_mask"
            else:
                args = [out, w, s0, w + 3, s1, w + 6, m, w, h]
                name = "blend_a64_hmask" if kind == 1 else "blend_a64_vmask"
            getattr(B, ("aom_highbd_" if hb else "aom_") + name)(*(args + ([bd] if hb else [])))
            dst = dev(np.zeros((h, w), dt))
            B.blend_a64_batch(dst, dev(s0), dev(s1), dev(mask), w, h,
                              B.comp_jobs_tensor(jobs, "cuda"), kind, subw, subh, False, bd)
            np.testing.assert_array_equal(host(dst, dt), out)
        # diff-weighted mask
        out = np.zeros(w * h, np.uint8)
        if hb:
            B.av1_build_compound_diffwtd_mask_highbd(out, 1, s0, w + 3, s1, w + 6, h, w, bd)
        else:
            B.av1_build_compound_diffwtd_mask(out, 1, s0, w + 3, s1, w + 6, h, w)
        jobs["invert_mask"] = 1
        tmask = torch.zeros(w * h, dtype=torch.uint8, device="cuda")
        B.diffwtd_mask_batch(tmask, dev(s0), dev(s1), w, h, B.comp_jobs_tensor(jobs, "cuda"),
                             bit_depth=bd)
        np.testing.assert_array_equal(tmask.cpu().numpy(), out)
        jobs["invert_mask"] = 0
    # wedge
    n = 128
    a = rng.integers(-4095, 4096, n).astype(np.int16)
    b = rng.integers(-4095, 4096, n).astype(np.int16)
    m = F["wedge_masks_16x8"][2, 0].reshape(-1).copy()
    wj = np.zeros(1, B.WEDGE_JOB_DTYPE)
    wj["n"], wj["limit"] = n, 1000
    tj = B.wedge_jobs_tensor(wj, "cuda")
    assert int(B.wedge_batch(dev(a), dev(b), dev(m), tj, 1).cpu()[0]) == \
        B.av1_wedge_sse_from_residuals(a, b, m, n)
    assert int(B.wedge_batch(dev(a), None, dev(m), tj, 2).cpu()[0]) == \
        B.av1_wedge_sign_from_residuals(a, m, n, 1000)
    d = np.zeros(n, np.int16)
    B.av1_wedge_compute_delta_squares(d, a, b, n)
    td = torch.zeros(n, dtype=torch.int16, device="cuda")
    B.wedge_batch(dev(a), dev(b), None, tj, 0, out=td)
    np.testing.assert_array_equal(td.cpu().numpy(), d)


def test_wrappers_raise_on_a_refusal(B):
    import torch
    z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    jobs = torch.zeros(72, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        B.blend_a64_batch(z, z, z, z, 12, 12, jobs, mask_stride=16)
    with pytest.raises(ValueError):
        B.diffwtd_mask_batch(z, z, z, 16, 16, jobs, d16=True, bit_depth=8, conv_params=None)
    with pytest.raises(ValueError):
        B.wedge_batch(z.view(torch.int16), None, None, jobs[:48], 3, out=z)


# ----------------------------------------------------------------- chains --
@pytest.mark.parametrize("bd,w,h,nj", [(8, 16, 16, 17), (10, 8, 8, 67), (12, 64, 32, 5)])
def test_chain_convolve_mask_blend(B, bd, w, h, nj):
    """Two first passes of lavish_dist_wtd_convolve_batch, the d16
    diff-weighted mask, the d16 blend: the result equals the restatement of
    av1_make_masked_inter_predictor's arithmetic on the same d16 buffers."""
    import torch
    import lavish_dsp.compound as Cm
    import _oracle as O
    from lavish_dsp.inter import ConvolveParams
    rng = np.random.default_rng(bd + w)
    hb = bd > 8
    W, H = 300, 200
    r0 = 5 if bd == 12 else 3
    table = lambda f, size: np.stack([O.interp_kernel(f, size, p) for p in range(16)])
    conv = []
    for k in range(2):
        src = rng.integers(0, 1 << bd, (H, W)).astype(pdt(hb))
        cj = np.zeros(nj, Cm.JOB_DTYPE)
        cj["src_off"] = rng.integers(8, H - h - 8, nj) * W + rng.integers(8, W - w - 8, nj)
        cj["conv_off"] = np.arange(nj) * w * h
        cj["dst_off"] = np.arange(nj) * w * h
        cj["subpel_x_qn"], cj["subpel_y_qn"] = rng.integers(0, 16, nj), rng.integers(0, 16, nj)
        fpx, tx = Cm.filter_params(table(k, w))
        fpy, ty = Cm.filter_params(table(2 - k, h))
        cp = ConvolveParams(0, None, 0, r0, 7, 0, 1, 0, 0, 0)
        tconv = torch.zeros(nj * w * h, dtype=torch.int16, device="cuda")
        tdst = dev(np.zeros(nj * w * h, pdt(hb)))
        Cm.dist_wtd_convolve_batch(dev(src), W, tdst, w, tconv, w, w, h,
                                   torch.from_numpy(cj.view(np.uint8)).cuda(), nj, fpx, fpy, cp, bd)
        conv.append(tconv)
    cp = B.conv_params(r0, 7)
    jobs = np.zeros(nj, B.COMP_JOB_DTYPE)
    off = np.arange(nj) * w * h
    jobs["src_off"], jobs["mask_off"] = off, off
    jobs["ref_off"][:, 0], jobs["ref_off"][:, 1] = off, off
    jobs["invert_mask"] = np.arange(nj) % 2
    tj = B.comp_jobs_tensor(jobs, "cuda")
    mask = torch.zeros(nj * w * h, dtype=torch.uint8, device="cuda")
    B.diffwtd_mask_batch(mask, conv[0], conv[1], w, h, tj, d16=True, bit_depth=bd, conv_params=cp,
                         src0_stride=w, src1_stride=w)
    pred = dev(np.zeros(nj * w * h, pdt(hb)))
    B.blend_a64_batch(pred, conv[0], conv[1], mask, w, h, tj, 0, 0, 0, True, bd, cp, dst_stride=w,
                      src0_stride=w, src1_stride=w, mask_stride=w)
    torch.cuda.synchronize()
    c0 = host(conv[0], np.uint16).reshape(nj, h, w)
    c1 = host(conv[1], np.uint16).reshape(nj, h, w)
    em, ep = R.masked_inter_predictor_d16(c0, c1, np.arange(nj) % 2, r0, 7, bd)
    np.testing.assert_array_equal(mask.cpu().numpy().reshape(nj, h, w), em)
    np.testing.assert_array_equal(host(pred, pdt(hb)).reshape(nj, h, w), ep)
    assert len(np.unique(em)) > 4     # the mask follows the difference of the predictions


def test_chain_obmc_wsrc_into_the_search(B, F):
    """The device-built wsrc / mask feed lavish_obmc_full_pixel_search_batch on
    a handful of 16x16 jobs; the same call on the restatement's arrays returns
    identical results."""
    import torch
    import lavish_dsp.motion as M
    rng = np.random.default_rng(16)
    nj, bw, bh, W, H = 7, 16, 16, 192, 160
    src = rng.integers(0, 256, (H, W)).astype(np.uint8)
    # the reference plane: the source moved by (2, -3) plus noise, so the search moves
    ref = np.roll(src, (2, -3), (0, 1)).astype(np.int64) + rng.integers(-6, 7, (H, W))
    ref = np.clip(ref, 0, 255).astype(np.uint8)
    above = rng.integers(0, 256, (H, W)).astype(np.uint8)
    left = rng.integers(0, 256, (H, W)).astype(np.uint8)
    pos = (48 + 16 * (np.arange(nj) // 4)) * W + 48 + 24 * (np.arange(nj) % 4) + np.arange(nj) % 3
    oj = np.zeros(nj, B.OBMC_JOB_DTYPE)
    oj["src_off"], oj["above_off"], oj["left_off"] = pos, pos, pos
    oj["above_mask"] = [0xF, 0x3, 0xC, 0x0, 0xF, 0x5, 0xA]
    oj["left_mask"] = [0xF, 0xF, 0x0, 0x3, 0xC, 0xA, 0x5]
    oj["wsrc_off"] = np.arange(nj) * bw * bh
    oj["mask_off"] = np.arange(nj) * bw * bh
    wsrc = torch.zeros(nj * bw * bh, dtype=torch.int32, device="cuda")
    mask = torch.zeros(nj * bw * bh, dtype=torch.int32, device="cuda")
    B.obmc_wsrc_batch(dev(src), dev(above), dev(left), bw, bh, B.obmc_jobs_tensor(oj, "cuda"),
                      dev(F["obmc_masks"]), wsrc, mask)
    ews, emk = [], []
    for j in range(nj):
        g = lambda p: gather(p, pos[j:j + 1], W, bh, bw)[0]
        ws, mk = R.obmc_wsrc(g(src), g(above), g(left), oj["above_mask"][j], oj["left_mask"][j],
                             F["obmc_masks"])
        ews.append(ws.reshape(-1))
        emk.append(mk.reshape(-1))
    ews, emk = (np.concatenate(v).astype(np.int32) for v in (ews, emk))
    jobs = np.zeros(nj, M.JOB_DTYPE)
    jobs["ref_off"] = pos
    jobs["col_min"], jobs["col_max"], jobs["row_min"], jobs["row_max"] = -16, 16, -16, 16
    cj = M.to_device(M.comp_jobs(jobs, oj["wsrc_off"], oj["mask_off"]))
    tref = dev(ref)
    cost = M.l1_cost_params()
    got = M.comp_results_numpy(M.obmc_full_pixel_search_batch(tref, W, bw, bh, cj, cost, wsrc, mask,
                                                              step_param=6))
    exp = M.comp_results_numpy(M.obmc_full_pixel_search_batch(tref, W, bw, bh, cj, cost, dev(ews),
                                                              dev(emk), step_param=6))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(wsrc.cpu().numpy(), ews)
    np.testing.assert_array_equal(mask.cpu().numpy(), emk)
    assert got.tobytes() == exp.tobytes()
    assert (got["steps"] > 0).all() and (got["best_row"] != 0).any()
