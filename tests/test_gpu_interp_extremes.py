"""The four predictor units (inter.hip, compound.hip, scale.hip, warp.hip) on
worst-case pixels, bit-exact:
  - every case of tests/golden/fix_interp_extremes.npz (the reference's C
    executed on aligned 0 / max windows, every phase of every kernel kind,
    incl. the MULTITAP_SHARP2 cases whose int16 intermediate wraps) through
    the per-call shims and through the batch calls, no oracle in the loop;
  - lavish_build_inter_pred_batch (the u8 FAST path, the highbd path and the
    12-tap direct path) against O.build_inter_pred on periodic planes of the
    same windows, every kind x phase x polarity;
  - saturation planes (all-max, all-0, checkerboard, stripes) through the
    batch calls of all four units against the oracle.
The oracle is pinned on these patterns by tests/test_oracle_interp_extremes.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import _extfix as E
import _extremes as X
import _oracle as O

pytestmark = pytest.mark.gpu
MIN_JOBS = 40   # more than any unit puts in one workgroup


@pytest.fixture(scope="module")
def F():
    import torch
    assert torch.cuda.is_available()
    return E.load()


def _table(kind):
    return np.stack([X.kernel(kind, p) for p in range(16)]).astype(np.int16)


def _cparams(c, conv=None, stride=0):
    from lavish_dsp.inter import ConvolveParams
    d = conv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)) if conv is not None else None
    return ConvolveParams(int(c.mode >= 2), d, stride, c.round_0, c.round_1, 0, int(c.mode > 0),
                          int(c.mode == 3), c.fwd_offset, c.bck_offset)


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _rows(F, **want):
    R = F["conv_rows"]
    m = np.ones(len(R), bool)
    for n, v in want.items():
        m &= R[:, E.CONV_FIELDS.index(n)] == v
    return np.flatnonzero(m)


# ------------------------------------------------------------ shims, every case --
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_single_shims_vs_reference(F, bd):
    import lavish_dsp.inter as I
    rows = _rows(F, unit=E.SINGLE, bd=bd)
    assert len(rows) > 600
    for k in rows:
        c = E.conv_case(F, k)
        fpx = I.filter_params(_table(c.kind_x), len(X.kernel(c.kind_x, 0)), X.kind_filter(c.kind_x)[0])
        fpy = I.filter_params(_table(c.kind_y), len(X.kernel(c.kind_y, 0)), X.kind_filter(c.kind_y)[0])
        dst = c.dst_in.copy()
        I.convolve(["copy", "x", "y", "2d"][c.path], c.src, c.off, c.src_w, dst, 0, c.w, c.w, c.h,
                   fpx, fpy, c.phase_x, c.phase_y, c.round_0, c.round_1, bd)
        np.testing.assert_array_equal(dst, c.dst, err_msg="row %d %s" % (k, F["conv_rows"][k]))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_compound_shims_vs_reference(F, bd):
    import lavish_dsp.compound as Cm
    rows = _rows(F, unit=E.COMPOUND, bd=bd)
    assert len(rows) > 500
    for k in rows:
        c = E.conv_case(F, k)
        fpx, tx = Cm.filter_params(_table(c.kind_x))
        fpy, ty = Cm.filter_params(_table(c.kind_y))
        dst, buf = c.dst_in.copy(), c.buf_in.copy()
        addr = ctypes.c_void_p(c.src.ctypes.data + c.off * c.src.itemsize)
        Cm.dist_wtd_convolve_shim(c.path, addr, c.src_w, dst, c.w, c.w, c.h, fpx, fpy,
                                  c.subpel_x_qn >> 6, c.subpel_y_qn >> 6, _cparams(c, buf, c.w), bd)
        np.testing.assert_array_equal(buf, c.buf, err_msg="row %d buf" % k)
        np.testing.assert_array_equal(dst, c.dst, err_msg="row %d" % k)


@pytest.mark.parametrize("hb,bd", [(0, 8), (1, 8), (1, 10), (1, 12)])
def test_scale_shims_vs_reference(F, hb, bd):
    import lavish_dsp.compound as Cm
    import lavish_dsp.scale as S
    rows = _rows(F, unit=E.SCALE, highbd=hb, bd=bd)
    assert len(rows) > 150
    for k in rows:
        c = E.conv_case(F, k)
        fpx, tx = Cm.filter_params(_table(c.kind_x))
        fpy, ty = Cm.filter_params(_table(c.kind_y))
        dst, buf = c.dst_in.copy(), c.buf_in.copy()
        addr = ctypes.c_void_p(c.src.ctypes.data + c.off * c.src.itemsize)
        S.convolve_2d_scale_shim(addr, c.src_w, dst, c.w, c.w, c.h, fpx, fpy, c.subpel_x_qn,
                                 c.x_step_qn, c.subpel_y_qn, c.y_step_qn, _cparams(c, buf, c.w), bd)
        np.testing.assert_array_equal(buf, c.buf, err_msg="row %d buf" % k)
        np.testing.assert_array_equal(dst, c.dst, err_msg="row %d" % k)


def _warp_cp(Wp, c, **kw):
    return Wp.conv_params(c.round_0, c.round_1, is_compound=int(c.mode > 0),
                          do_average=int(c.mode >= 2), dist_wtd=int(c.mode == 3),
                          fwd_offset=c.fwd_offset, bck_offset=c.bck_offset, **kw)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_warp_shims_vs_reference(F, bd):
    import lavish_dsp.warp as Wp
    rows = np.flatnonzero(F["warp_rows"][:, 0] == bd)
    assert len(rows) > 400
    for k in rows:
        c = E.warp_case(F, k)
        pred, buf = c.pred_in.copy(), c.buf_in.copy()
        Wp.warp_affine_shim(c.mat, c.ref, c.width, c.height, c.stride, pred, c.p_col, c.p_row,
                            c.p_width, c.p_height, c.p_width, 0, 0,
                            _warp_cp(Wp, c, dst=buf, dst_stride=c.p_width), c.prm, bd)
        np.testing.assert_array_equal(pred, c.pred, err_msg="row %d" % k)
        np.testing.assert_array_equal(buf, c.buf, err_msg="row %d buf" % k)


# ----------------------------------------------- batch calls against the fixture --
def _groups(F, rows, fields):
    """Rows that can share one launch: equal in `fields`."""
    out = {}
    for k in rows:
        key = tuple(int(F["conv_rows"][k][E.CONV_FIELDS.index(n)]) for n in fields)
        out.setdefault(key, []).append(int(k))
    return out


GROUP = ["w", "h", "kind_x", "kind_y", "src_h", "src_w", "mode", "fwd_offset", "bck_offset"]


def _conv_batch(F, ks, jobs_dtype, launch):
    """All cases `ks` (one geometry and conv-param form) in one launch, the
    list repeated to MIN_JOBS jobs; every job's block against the fixture."""
    import torch
    ks = ks * -(-MIN_JOBS // len(ks))
    cs = [E.conv_case(F, k) for k in ks]
    c0 = cs[0]
    n, px = len(cs), c0.w * c0.h
    # (a spare row: the last job's window ends the tensor otherwise)
    src = np.concatenate([c.src for c in cs] + [np.zeros((1, c0.src_w), c0.pdt)])
    dst = np.concatenate([c.dst_in for c in cs])
    buf = np.concatenate([c.buf_in for c in cs])
    jobs = np.zeros(n, jobs_dtype)
    jobs["src_off"] = np.arange(n) * c0.src_h * c0.src_w + c0.off
    jobs["dst_off"] = jobs["conv_off"] = np.arange(n) * px
    tsrc, tdst, tbuf = _dev(src), _dev(dst), _dev(buf)
    launch(cs, jobs, tsrc, tdst, tbuf)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(tbuf, np.uint16), np.concatenate([c.buf for c in cs]),
                                  err_msg="buf, rows %s" % ks[:8])
    np.testing.assert_array_equal(_host(tdst, c0.pdt), np.concatenate([c.dst for c in cs]),
                                  err_msg="dst, rows %s" % ks[:8])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_compound_batch_vs_reference(F, bd):
    import torch
    import lavish_dsp.compound as Cm

    def launch(cs, jobs, tsrc, tdst, tbuf):
        c = cs[0]
        jobs["subpel_x_qn"] = [x.subpel_x_qn >> 6 for x in cs]
        jobs["subpel_y_qn"] = [x.subpel_y_qn >> 6 for x in cs]
        fpx, tx = Cm.filter_params(_table(c.kind_x))
        fpy, ty = Cm.filter_params(_table(c.kind_y))
        Cm.dist_wtd_convolve_batch(tsrc, c.src_w, tdst, c.w, tbuf, c.w, c.w, c.h,
                                   torch.from_numpy(jobs.view(np.uint8)).cuda(), len(jobs), fpx,
                                   fpy, _cparams(c), bd)
    groups = _groups(F, _rows(F, unit=E.COMPOUND, bd=bd), GROUP)
    assert len(groups) > 60
    for ks in groups.values():
        _conv_batch(F, ks, Cm.JOB_DTYPE, launch)


@pytest.mark.parametrize("hb,bd", [(0, 8), (1, 8), (1, 10), (1, 12)])
def test_scale_batch_vs_reference(F, hb, bd):
    import torch
    import lavish_dsp.compound as Cm
    import lavish_dsp.scale as S

    def launch(cs, jobs, tsrc, tdst, tbuf):
        c = cs[0]
        for f in ("subpel_x_qn", "x_step_qn", "subpel_y_qn", "y_step_qn"):
            jobs[f] = [getattr(x, f) for x in cs]
        fpx, tx = Cm.filter_params(_table(c.kind_x))
        fpy, ty = Cm.filter_params(_table(c.kind_y))
        S.convolve_2d_scale_batch(tsrc, c.src_w, tdst, c.w, tbuf, c.w, c.w, c.h,
                                  torch.from_numpy(jobs.view(np.uint8)).cuda(), len(jobs), fpx,
                                  fpy, _cparams(c), bd)
    groups = _groups(F, _rows(F, unit=E.SCALE, highbd=hb, bd=bd), GROUP)
    assert len(groups) > 30
    for ks in groups.values():
        _conv_batch(F, ks, S.JOB_DTYPE, launch)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_warp_batch_vs_reference(F, bd):
    import torch
    import lavish_dsp.warp as Wp
    PS, SLOT = 16, 16 * 16
    J = {n: i for i, n in enumerate(E.WARP_FIELDS)}
    groups = {}
    for k in np.flatnonzero(F["warp_rows"][:, 0] == bd):
        r = F["warp_rows"][k]
        key = tuple(int(r[J[n]]) for n in ("mode", "fwd_offset", "bck_offset", "width", "height",
                                           "stride"))
        groups.setdefault(key, []).append(int(k))
    assert len(groups) >= 8
    for ks in groups.values():
        ks = ks * -(-MIN_JOBS // len(ks))
        cs = [E.warp_case(F, k) for k in ks]
        c0, n = cs[0], len(cs)
        ref = np.concatenate([c.ref for c in cs])
        pred = np.full((n, 16, PS), F["fills"][0], c0.pdt)
        buf = np.full((n, 16, PS), F["fills"][1], np.uint16)
        epred, ebuf = pred.copy(), buf.copy()
        jobs = np.zeros(n, Wp.JOB_DTYPE)
        for i, c in enumerate(cs):
            buf[i, :c.p_height, :c.p_width] = c.buf_in
            epred[i, :c.p_height, :c.p_width] = c.pred
            ebuf[i, :c.p_height, :c.p_width] = c.buf
            jobs[i]["mat"] = c.mat
            for f in ("alpha", "beta", "gamma", "delta", "p_col", "p_row", "p_width", "p_height"):
                jobs[i][f] = getattr(c, f)
        jobs["ref_off"] = np.arange(n) * c0.height * c0.stride
        jobs["pred_off"] = jobs["dst_off"] = np.arange(n) * SLOT
        tref, tpred, tbuf = _dev(ref), _dev(pred), _dev(buf)
        Wp.warp_affine_batch(tref, c0.width, c0.height, c0.stride, tpred, PS,
                             torch.from_numpy(jobs.view(np.uint8)).cuda(), n, _warp_cp(Wp, c0), bd,
                             conv_dst=tbuf, dst_stride=PS)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_host(tpred, c0.pdt).reshape(epred.shape), epred,
                                      err_msg="rows %s" % ks[:8])
        np.testing.assert_array_equal(_host(tbuf, np.uint16).reshape(ebuf.shape), ebuf,
                                      err_msg="buf, rows %s" % ks[:8])


# ------------------------- lavish_build_inter_pred_batch on periodic planes --
W, H, SS = 64, 32, (1, 1)
SIZES = [(8, 16), (16, 16), (8, 8), (8, 4), (4, 8), (4, 2), (2, 8)]
# the table av1_get_interp_filter_params_with_block_size picks (filter.h:253-259)
KIND8 = [X.REGULAR, X.SMOOTH, X.SHARP, X.BILINEAR, X.SHARP2]
KIND4 = [X.REGULAR4, X.SMOOTH4, X.REGULAR4, X.BILINEAR, X.REGULAR4]


def _kind(f, size):
    return KIND4[f] if size <= 4 else KIND8[f]


def _plane(win, dt, anchor):
    """The frame buffer of tests/test_gpu_inter.py::_bordered filled with the
    periodic pattern; frame pixel `anchor` sees the aligned window at mv 0."""
    bx, by = (288 >> SS[0]) + 2, (288 >> SS[1]) + 2
    stride = W + 2 * bx + 24
    plane = X.periodic(win, (H + 2 * by, stride), (by + anchor[0], bx + anchor[1]))
    return np.ascontiguousarray(plane.astype(dt)), by * stride + bx


def _mvs(n, px, py, seed):
    """1/8-pel mvs (1/16 of a chroma sample at ss 1) that share a phase and
    differ by whole pixels."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-5, 6, n) * 16 + py, rng.integers(-5, 6, n) * 16 + px], 1)


def _inter(plane, org, bw, bh, f, px, py, bd, seed, dst_shift=0):
    import torch
    import lavish_dsp.inter as I
    import lavish_dsp.motion as M
    hbd = plane.dtype == np.uint16
    n = (W // bw) * (H // bh)
    jobs = I.plane_jobs(W, H, bw, bh, _mvs(n, px, py, seed), f)
    jobs["dst_off"] += dst_shift
    shape = (H + (1 if dst_shift else 0), W)
    dst = torch.zeros(shape, dtype=torch.int16 if hbd else torch.uint8, device="cuda")
    I.build_inter_pred_batch(_dev(plane), org, W, H, bw, bh, M.to_device(jobs), dst=dst,
                             bit_depth=bd, ss=SS)
    torch.cuda.synchronize()
    exp = O.build_inter_pred(plane, org, W, H, SS[0], SS[1], bw, bh, jobs, shape, bd=bd)
    got = _host(dst, plane.dtype)
    np.testing.assert_array_equal(got, exp, err_msg=str((bw, bh, f, px, py, bd, dst_shift)))
    return got


VARIANTS = [(8, np.uint8), (10, np.uint16), (12, np.uint16)]


@pytest.mark.parametrize("phase", range(1, 16))
@pytest.mark.parametrize("f", [0, 1, 2, 3])
def test_inter_batch_periodic(f, phase):
    """Every 8-tap and 4-tap kind at one phase in both directions, both
    polarities: the u8 FAST path (R 16 / 8 / 4 / 2), the CW 2 path and the
    highbd path."""
    for bd, dt in VARIANTS:
        for bw, bh in SIZES:
            kx, ky = X.kernel(_kind(f, bw), phase), X.kernel(_kind(f, bh), phase)
            for pol in (1, 0):
                seed = ((f * 16 + phase) * 2 + pol) * 7 + bw
                plane, org = _plane(X.window(kx, ky, bd, pol), dt, (seed % 16, seed % 5))
                got = _inter(plane, org, bw, bh, (f, f), phase, phase, bd, seed)
                # the aligned pixel saturates (its value: test_oracle_interp_extremes)
                assert ((1 << bd) - 1 if pol else 0) in got


@pytest.mark.parametrize("which", ["x", "y", "copy"])
@pytest.mark.parametrize("f", [0, 1, 2, 3])
def test_inter_batch_periodic_1d(f, which):
    """Phase 0 in one or both directions: the FAST path runs these through
    its 2-D form with the identity row."""
    for bd, dt in VARIANTS[:2]:
        for bw, bh in SIZES:
            for phase in ([0] if which == "copy" else range(1, 16)):
                px, py = (phase if which == "x" else 0), (phase if which == "y" else 0)
                kx = X.kernel(_kind(f, bw), px) if px else None
                ky = X.kernel(_kind(f, bh), py) if py else None
                pol = phase & 1
                seed = (f * 16 + phase) * 11 + bh
                plane, org = _plane(X.window(kx, ky, bd, pol), dt, (seed % 16, seed % 7))
                _inter(plane, org, bw, bh, (f, f), px, py, bd, seed)


@pytest.mark.parametrize("f", [0, 1, 2, 3])
def test_inter_batch_periodic_unaligned_dst(f):
    """dst one element off: the byte-store branch of the FAST path."""
    for bd, dt in VARIANTS[:2]:
        for bw, bh in SIZES:
            for phase in range(1, 16):
                kx, ky = X.kernel(_kind(f, bw), phase), X.kernel(_kind(f, bh), phase)
                seed = (f * 16 + phase) * 13 + bw
                plane, org = _plane(X.window(kx, ky, bd, phase & 1), dt, (seed % 16, seed % 4))
                _inter(plane, org, bw, bh, (f, f), phase, phase, bd, seed, dst_shift=1)


@pytest.mark.parametrize("phase", range(1, 16))
def test_inter_batch_periodic_12tap(phase):
    """MULTITAP_SHARP2 through the direct per-pixel path, alone and crossed
    with SHARP; at bd 10 / 12 its int16 intermediate wraps."""
    for bd, dt in VARIANTS:
        for bw, bh in [(8, 16), (16, 16), (8, 8), (8, 4), (4, 8)]:
            for fx, fy in ((4, 4), (4, 2), (2, 4)):
                kx, ky = X.kernel(_kind(fx, bw), phase), X.kernel(_kind(fy, bh), phase)
                for pol in (1, 0):
                    seed = (phase * 2 + pol) * 17 + bh + fx
                    plane, org = _plane(X.window(kx, ky, bd, pol), dt, (seed % 12, seed % 5))
                    _inter(plane, org, bw, bh, (fx, fy), phase, phase, bd, seed)


# ------------------------------------------------------------- saturation planes --
PLANES = ["max", "zero", "checker", "vstripes", "hstripes"]


@pytest.mark.parametrize("name", PLANES)
@pytest.mark.parametrize("phase", [1, 8, 15])
def test_inter_saturation(name, phase):
    for bd, dt in VARIANTS:
        bx, by = (288 >> SS[0]) + 2, (288 >> SS[1]) + 2
        stride = W + 2 * bx + 24
        plane = np.ascontiguousarray(
            X.saturation_planes((H + 2 * by, stride), bd)[name].astype(dt))
        for f in range(5):
            for bw, bh in ((8, 8), (4, 4), (16, 16)):
                _inter(plane, by * stride + bx, bw, bh, (f, f), phase, phase, bd, f + phase)


def _sat_jobs(dtype, n, w, h, PW):
    jobs = np.zeros(n, dtype)
    jobs["src_off"] = (8 + np.arange(n) % 5) * PW + 8 + np.arange(n) % 7
    jobs["dst_off"] = jobs["conv_off"] = np.arange(n) * w * h
    return jobs


@pytest.mark.parametrize("name", PLANES)
@pytest.mark.parametrize("phase", [1, 8, 15])
def test_compound_saturation(name, phase):
    import torch
    import lavish_dsp.compound as Cm
    PH, PW, n = 40, 48, MIN_JOBS
    for bd, dt in VARIANTS:
        src = np.ascontiguousarray(X.saturation_planes((PH, PW), bd)[name].astype(dt))
        r0 = X.conv_rounds(bd, True)[0]
        for kind in range(7):
            w, h = (4, 4) if X.kind_filter(kind)[1] == 4 else (8, 8)
            tab = _table(kind)
            fpx, tx = Cm.filter_params(tab)
            fpy, ty = Cm.filter_params(tab)
            jobs = _sat_jobs(Cm.JOB_DTYPE, n, w, h, PW)
            jobs["subpel_x_qn"] = np.where(np.arange(n) % 4 == 1, 0, phase)
            jobs["subpel_y_qn"] = np.where(np.arange(n) % 4 == 2, 0, phase)
            buf0 = np.full((n * h, w), 0x1234, np.uint16)
            for mode, fwd, bck in ((1, 0, 0), (2, 0, 0), (3, 13, 3)):
                cp = dict(do_average=int(mode >= 2), round_0=r0, round_1=7, is_compound=1,
                          use_dist_wtd_comp_avg=int(mode == 3), fwd_offset=fwd, bck_offset=bck)
                c = SimpleNamespace(mode=mode, round_0=r0, round_1=7, fwd_offset=fwd,
                                      bck_offset=bck)
                ed, eb = np.zeros((n * h, w), dt), buf0.copy()
                tdst, tbuf = _dev(ed.copy()), _dev(buf0.copy())
                Cm.dist_wtd_convolve_batch(_dev(src), PW, tdst, w, tbuf, w, w, h,
                                           torch.from_numpy(jobs.view(np.uint8)).cuda(), n, fpx,
                                           fpy, _cparams(c), bd)
                torch.cuda.synchronize()
                O.dist_wtd_batch(src, PW, ed, w, eb, w, w, h, jobs, tx, ty, cp, bd=bd)
                np.testing.assert_array_equal(_host(tbuf, np.uint16), eb,
                                              err_msg=str((bd, kind, mode)))
                np.testing.assert_array_equal(_host(tdst, dt), ed,
                                              err_msg=str((bd, kind, mode)))
                buf0 = eb   # the next mode averages over this first pass


@pytest.mark.parametrize("name", PLANES)
@pytest.mark.parametrize("phase", [1, 8, 15])
def test_scale_saturation(name, phase):
    import torch
    import lavish_dsp.compound as Cm
    import lavish_dsp.scale as S
    PH, PW, n = 48, 56, MIN_JOBS
    for hb, bd in ((0, 8), (1, 8), (1, 10), (1, 12)):
        dt = np.uint16 if hb else np.uint8
        src = np.ascontiguousarray(X.saturation_planes((PH, PW), bd)[name].astype(dt))
        for kind in range(7):
            w, h = (4, 4) if X.kind_filter(kind)[1] == 4 else (8, 8)
            tab = _table(kind)
            fpx, tx = Cm.filter_params(tab)
            fpy, ty = Cm.filter_params(tab)
            jobs = _sat_jobs(S.JOB_DTYPE, n, w, h, PW)
            jobs["subpel_x_qn"] = jobs["subpel_y_qn"] = phase << 6
            steps = np.array([1024, 2048, 512, 1365])[np.arange(n) % 4]
            jobs["x_step_qn"], jobs["y_step_qn"] = steps, steps[::-1]
            buf0 = np.full((n * h, w), 0x1234, np.uint16)
            for mode, fwd, bck in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 4, 12)):
                r0, r1 = X.conv_rounds(bd, mode > 0)
                cp = dict(do_average=int(mode >= 2), round_0=r0, round_1=r1,
                          is_compound=int(mode > 0), use_dist_wtd_comp_avg=int(mode == 3),
                          fwd_offset=fwd, bck_offset=bck)
                c = SimpleNamespace(mode=mode, round_0=r0, round_1=r1, fwd_offset=fwd,
                                      bck_offset=bck)
                ed, eb = np.zeros((n * h, w), dt), buf0.copy()
                tdst, tbuf = _dev(ed.copy()), _dev(buf0.copy())
                S.convolve_2d_scale_batch(_dev(src), PW, tdst, w, tbuf, w, w, h,
                                          torch.from_numpy(jobs.view(np.uint8)).cuda(), n, fpx,
                                          fpy, _cparams(c), bd)
                torch.cuda.synchronize()
                O.convolve_2d_scale_batch(src, PW, ed, w, eb, w, w, h, jobs, tx, ty, cp, bd=bd)
                np.testing.assert_array_equal(_host(tbuf, np.uint16), eb,
                                              err_msg=str((hb, bd, kind, mode)))
                np.testing.assert_array_equal(_host(tdst, dt), ed,
                                              err_msg=str((hb, bd, kind, mode)))
                buf0 = eb


@pytest.mark.parametrize("name", PLANES)
def test_warp_saturation(name):
    """Translations at filter rows 65 / 96 / 127 (phases 1, 8 and 15 of 16 at
    the warp's 1/64 step) and the large shears of the fixture, blocks over
    every edge of the reference."""
    import torch
    import lavish_dsp.warp as Wp
    WW, WH, PS = 48, 40, 16
    F = E.load()
    J = {n: i for i, n in enumerate(E.WARP_FIELDS)}
    sh = F["warp_rows"][F["warp_rows"][:, J["aligned"]] == 0]
    models = sorted({tuple(int(r[J[n]]) for n in ("m0", "m1", "m2", "m3", "m4", "m5", "alpha",
                                                  "beta", "gamma", "delta")) for r in sh})
    models += [((q << 10) + (3 << 16), (q << 10) - (2 << 16), 1 << 16, 0, 0, 1 << 16, 0, 0, 0, 0)
               for q in (1, 32, 63)]
    spots = [(0, 0, 8, 8), (WW - 8, WH - 8, 8, 8), (16, 8, 16, 16), (WW - 16, 0, 16, 8),
             (0, WH - 8, 8, 8)]
    n = len(models) * len(spots)
    assert n >= MIN_JOBS
    jobs = np.zeros(n, Wp.JOB_DTYPE)
    for i in range(n):
        m, (pc, pr, pw, ph) = models[i // len(spots)], spots[i % len(spots)]
        jobs[i]["mat"] = m[:6]
        jobs[i]["alpha"], jobs[i]["beta"], jobs[i]["gamma"], jobs[i]["delta"] = m[6:]
        jobs[i]["p_col"], jobs[i]["p_row"], jobs[i]["p_width"], jobs[i]["p_height"] = pc, pr, pw, ph
    jobs["pred_off"] = jobs["dst_off"] = np.arange(n) * 16 * PS
    tj = torch.from_numpy(jobs.view(np.uint8)).cuda()
    for bd, dt in VARIANTS:
        ref = np.ascontiguousarray(X.saturation_planes((WH, WW), bd)[name].astype(dt))
        buf0 = np.full((n * 16, PS), 0x1234, np.uint16)
        for mode, fwd, bck in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 11, 5)):
            r0, r1 = X.conv_rounds(bd, mode > 0)
            cp = dict(do_average=int(mode >= 2), round_0=r0, round_1=r1, is_compound=int(mode > 0),
                      use_dist_wtd_comp_avg=int(mode == 3), fwd_offset=fwd, bck_offset=bck)
            ep, eb = np.zeros((n * 16, PS), dt), buf0.copy()
            tpred, tbuf = _dev(ep.copy()), _dev(buf0.copy())
            Wp.warp_affine_batch(_dev(ref), WW, WH, WW, tpred, PS, tj, n,
                                 Wp.conv_params(r0, r1, is_compound=int(mode > 0),
                                                do_average=int(mode >= 2),
                                                dist_wtd=int(mode == 3), fwd_offset=fwd,
                                                bck_offset=bck), bd, conv_dst=tbuf, dst_stride=PS)
            torch.cuda.synchronize()
            O.warp_batch(ref, WW, WH, WW, ep, PS, jobs, cp, bd=bd, dst=eb, dst_stride=PS)
            np.testing.assert_array_equal(_host(tpred, dt).reshape(ep.shape), ep,
                                          err_msg=str((bd, mode)))
            np.testing.assert_array_equal(_host(tbuf, np.uint16).reshape(eb.shape), eb,
                                          err_msg=str((bd, mode)))
            buf0 = eb
