"""GPU parity of the intra prediction layer, bit-exact everywhere:
* every case of tests/golden/fix_intra.npz (the reference's own outputs)
  through lavish_intra_pred_batch, all sizes and modes of a bit depth in one
  call, and every shim case through its `_hip` symbol into a guarded buffer;
* seeded batches against tests/_intraref.py with job counts that end in a
  partial lane group, a partial wave and a partial workgroup;
* pixels the counts declare unavailable are never read (two poison values);
* dst inside the plane ref reads; a repeated call; and the TPL chain: 13
  modes predicted into a [13, H, W] tensor and costed by tpl_block_batch."""
import numpy as np
import pytest

import _intraref as R
import _oracle as O

pytestmark = pytest.mark.gpu

import os  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLANE_N = R.PLANE_ROWS * R.PLANE_STRIDE
CELL = 64 * 64  # a job's dst cell: rows at stride 64
GUARD = {1: 0xA5, 2: 0xA5A5}


@pytest.fixture(scope="module")
def I():
    import torch
    assert torch.cuda.is_available()
    import lavish_dsp.intra as I
    return I


@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(GOLD, "fix_intra.npz")))


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host(t, bd):
    a = t.cpu().numpy()
    return a.view(np.uint16) if bd > 8 else a


def _jobs(I, cases, ref_offs, dst_offs):
    g = lambda k: [getattr(c, k) for c in cases]  # noqa: E731
    return I.intra_jobs(ref_offs, dst_offs, g("tx_size"), g("mode"), g("p_angle"), g("fi_mode"),
                        g("disable_edge_filter"), g("filter_type"), g("n_top"), g("n_topright"),
                        g("n_left"), g("n_bottomleft"))


def _run_cells(I, ref, cases, ref_offs, bd):
    """The cases into one 64-stride cell each; returns the host cells [n, 64, 64]."""
    import torch
    n = len(cases)
    dst = _dev(np.full(n * CELL, GUARD[np.dtype(_dt(bd)).itemsize], _dt(bd)))
    jobs = I.intra_jobs_tensor(_jobs(I, cases, ref_offs, np.arange(n) * CELL), "cuda")
    I.intra_pred_batch(ref, dst, jobs, bd, ref_stride=R.PLANE_STRIDE, dst_stride=64)
    torch.cuda.synchronize()
    return _host(dst, bd).reshape(n, 64, 64)


def _check_cells(cells, cases, expected, bd):
    guard = GUARD[np.dtype(_dt(bd)).itemsize]
    bad = []
    for i, (c, e) in enumerate(zip(cases, expected)):
        cell = cells[i].astype(np.int64)
        ok = np.array_equal(cell[:c.h, :c.w], e)
        cell[:c.h, :c.w] = guard
        if not ok or not (cell == guard).all():
            bad.append((i, c.tx_size, c.mode, c.p_angle, c.fi_mode, c.n_top, c.n_topright, c.n_left,
                        c.n_bottomleft, ok))
    assert not bad, bad[:8]


# -------------------------------------------------------------- fixture ----
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_every_fixture_case_through_the_batch(I, F, bd):
    cases = [c for c in (R.intra_case(F, r) for r in F["cases"]) if c.bd == bd]
    assert len(cases) > 500
    # both planes of this depth back to back: plane 1 (all maximum) follows plane 0
    both = np.concatenate([R.plane_of(F, bd, 0), R.plane_of(F, bd, 1)]).astype(_dt(bd))
    offs = [c.ref_off + c.plane * PLANE_N for c in cases]
    cells = _run_cells(I, _dev(both), cases, offs, bd)
    _check_cells(cells, cases, [R.case_out(F, c) for c in cases], bd)


def test_every_fixture_shim_case(I, F):
    import lavish_dsp as L
    bad = []
    for i, row in enumerate(F["shim_cases"]):
        c = R.shim_case(F, row)
        hb = c.bd > 8
        dt = _dt(c.bd)
        pre = "highbd_" if hb else ""
        edge = F["edge_bd%d" % c.bd].astype(dt)
        exp = R.shim_expected(F, c)
        bdarg = [c.bd] if hb else []
        if c.kind in (R.K_FILTER_EDGE, R.K_UPSAMPLE):
            want = edge.copy()
            if c.kind == R.K_FILTER_EDGE:
                want[c.a_off:c.a_off + c.w] = exp
                getattr(I, "av1_filter_intra_edge" + ("_high" if hb else ""))(edge, c.w, c.p0,
                                                                            index=c.a_off)
            else:
                want[c.a_off - 2:c.a_off + 2 * c.w - 1] = exp  # p[-2 .. 2 sz - 2] inclusive
                getattr(I, "av1_upsample_intra_edge" + ("_high" if hb else ""))(
                    *([edge, c.w] + bdarg), index=c.a_off)
            if not np.array_equal(edge, want):  # the rest of the stream is the guard
                bad.append((i, list(map(int, row))))
            continue
        # only the reference's extents are real: everything else in the edge
        # arrays is poisoned, so an over-read shows in the output
        (a_lo, a_hi), (l_lo, l_hi) = R.shim_extents(c)
        above = np.full(R.EDGE_LEN, 0x5A, dt)
        left = np.full(R.EDGE_LEN, 0xC3, dt)
        above[c.a_off + a_lo:c.a_off + a_hi] = edge[c.a_off + a_lo:c.a_off + a_hi]
        left[c.l_off + l_lo:c.l_off + l_hi] = edge[c.l_off + l_lo:c.l_off + l_hi]
        stride = c.w + 7
        guard = GUARD[np.dtype(dt).itemsize]
        buf = np.full((c.h + 2) * stride, guard, dt)
        dst = buf[stride + 3:]
        kw = dict(above_index=c.a_off, left_index=c.l_off)
        if c.kind < 10:
            getattr(I, "aom_%s%s_predictor_%dx%d" % (pre, R.PRED_TYPES[c.kind], c.w, c.h))(
                dst, stride, above, left, *bdarg, **kw)
        elif c.kind == R.K_FILTER_INTRA:
            tx = [t for t in range(19) if (R.TX_W[t], R.TX_H[t]) == (c.w, c.h)][0]
            I.av1_filter_intra_predictor(dst, stride, tx, above, left, c.p0, **kw)
        else:
            dx, dy = R.get_dx_dy(c.p2)
            z = c.kind - R.K_Z1 + 1
            ups = [c.p0] if z == 1 else [c.p1] if z == 3 else [c.p0, c.p1]
            getattr(I, "av1_%sdr_prediction_z%d" % (pre, z))(
                *([dst, stride, c.w, c.h, above, left] + ups + [dx, dy] + bdarg), **kw)
        got = buf.astype(np.int64).reshape(c.h + 2, stride)
        blk = got[1:c.h + 1, 3:3 + c.w].copy()
        got[1:c.h + 1, 3:3 + c.w] = guard
        if not np.array_equal(blk.reshape(-1), exp) or not (got == guard).all():
            bad.append((i, list(map(int, row))))
    assert not bad, bad[:8]
    assert L.status()[0] == 0, L.status()


# --------------------------------------------------------- seeded batches --
MIX = [0, 13, 14, 1, 2, 16, 3, 18, 4]  # 4x4 4x16 16x4 8x8 16x16 32x8 32x32 64x16 64x64


def _random_case(rng, tx, bd):
    w, h = R.TX_W[tx], R.TX_H[tx]
    c = R.Case(R.I_COLS, [0] * len(R.I_COLS))
    c.bd, c.plane, c.tx_size, c.w, c.h = bd, 0, tx, w, h
    c.ref_off = int((1 + rng.integers(3)) * R.PLANE_STRIDE + 1 + rng.integers(7))
    c.mode = int(rng.integers(13))
    c.fi_mode = int(rng.integers(5)) if (w <= 32 and h <= 32 and rng.integers(6) == 0) else 5
    c.p_angle = int(R.T["kModeToAngle"][c.mode]) + 3 * int(rng.integers(-3, 4)) \
        if R.V_PRED <= c.mode <= R.D67_PRED else 0
    c.disable_edge_filter, c.filter_type = int(rng.integers(4) == 0), int(rng.integers(2))
    c.n_top = int(rng.choice([0, w, w, w, max(1, w // 2), max(1, w - 3)]))
    c.n_left = int(rng.choice([0, h, h, h, max(1, h // 2), max(1, h - 1)]))
    c.n_topright = int(rng.choice([-1, 0, max(1, w // 2), w])) if c.n_top == w else \
        int(rng.choice([-1, 0]))
    c.n_bottomleft = int(rng.choice([-1, 0, max(1, h // 2), h])) if c.n_left == h else \
        int(rng.choice([-1, 0]))
    return c


@pytest.mark.parametrize("bd,sizes", [
    (8, [0]), (8, [0] * 17), (10, [0] * (4 * 16 + 3)), (8, [4] * 5), (12, [4] * 5),
    (8, MIX * 9 + [0, 4]), (10, MIX * 8 + [13]), (12, list(range(19)) * 3)],
    ids=["1x4x4", "17x4x4", "67x4x4", "5x64x64-8", "5x64x64-12", "mix8", "mix10", "all12"])
def test_seeded_batches_vs_restatement(I, F, bd, sizes):
    rng = np.random.default_rng(1000 + bd + len(sizes))
    cases = [_random_case(rng, tx, bd) for tx in sizes]
    plane = R.plane_of(F, bd, 0)
    cells = _run_cells(I, _dev(plane.astype(_dt(bd))), cases, [c.ref_off for c in cases], bd)
    _check_cells(cells, cases, [R.run_case(F, c, plane=plane) for c in cases], bd)


def test_a_job_with_an_illegal_angle_is_skipped(I, F):
    """intra_jobs refuses a p_angle that is not base + 3 * delta; a record built
    past it is skipped on the device (nothing written), its neighbour runs."""
    import torch
    cases = [R.intra_case(F, [8, 0, R.PLANE_STRIDE + 1, 2, R.D45_PRED, a, 5, 0, 0, 16, 16, 16, -1, 0])
             for a in (45, 45, 45)]
    jobs = _jobs(I, cases, [c.ref_off for c in cases], np.arange(3) * CELL)
    jobs["p_angle"][1] = 46
    jobs["p_angle"][2] = 67  # a legal angle, of another mode
    plane = R.plane_of(F, 8, 0)
    dst = _dev(np.full(3 * CELL, GUARD[1], np.uint8))
    I.intra_pred_batch(_dev(plane.astype(np.uint8)), dst, I.intra_jobs_tensor(jobs, "cuda"), 8,
                       ref_stride=R.PLANE_STRIDE, dst_stride=64)
    torch.cuda.synchronize()
    cells = _host(dst, 8).reshape(3, 64, 64)
    _check_cells(cells[:1], cases[:1], [R.run_case(F, cases[0], plane=plane)], 8)
    assert (cells[1:] == GUARD[1]).all()


# ------------------------------------------------ unavailable pixels -------
@pytest.fixture(scope="module")
def poison_cases(F):
    """8-bit fixture cases with something excluded, a private plane each."""
    cs = [c for c in (R.intra_case(F, r) for r in F["cases"])
          if c.bd == 8 and c.plane == 0 and c.w * c.h <= 1024]
    short = [c for c in cs if c.n_top < c.w or c.n_left < c.h or c.n_topright >= 0 or
             c.n_bottomleft >= 0 or c.fi_mode != 5]
    return (short[::4] + cs[::29])[:260]


def _private_planes(F, cases, poison):
    plane = R.plane_of(F, 8, 0).astype(np.uint8)
    big = np.tile(plane, len(cases))
    for i, c in enumerate(cases):
        if poison is not None:
            big[i * PLANE_N:(i + 1) * PLANE_N][R.excluded_mask(c)] = poison
    return big


def test_unavailable_pixels_are_not_read(I, F, poison_cases):
    cases = poison_cases
    offs = [i * PLANE_N + c.ref_off for i, c in enumerate(cases)]
    outs = [_run_cells(I, _dev(_private_planes(F, cases, p)), cases, offs, 8) for p in (0x00, 0xFF)]
    assert np.array_equal(outs[0], outs[1])
    _check_cells(outs[0], cases, [R.case_out(F, c) for c in cases], 8)


def test_dst_inside_the_plane_ref_reads_and_repeat(I, F, poison_cases):
    """A block predicted into the position its own edges surround equals the
    out-of-place result and touches nothing else; a repeated out-of-place
    call gives identical output."""
    import torch
    cases = poison_cases[:120]
    offs = np.array([i * PLANE_N + c.ref_off for i, c in enumerate(cases)])
    host = _private_planes(F, cases, None)
    ref = _dev(host)
    a = _run_cells(I, ref, cases, offs, 8)
    b = _run_cells(I, ref, cases, offs, 8)
    assert np.array_equal(a, b)
    jobs = I.intra_jobs_tensor(_jobs(I, cases, offs, offs), "cuda")
    I.intra_pred_batch(ref, ref, jobs, 8, ref_stride=R.PLANE_STRIDE, dst_stride=R.PLANE_STRIDE)
    torch.cuda.synchronize()
    got = ref.cpu().numpy()
    want = host.copy()
    for i, c in enumerate(cases):
        blk = want[i * PLANE_N:(i + 1) * PLANE_N].reshape(R.PLANE_ROWS, R.PLANE_STRIDE)
        y, x = divmod(c.ref_off, R.PLANE_STRIDE)
        blk[y:y + c.h, x:x + c.w] = a[i][:c.h, :c.w]
    assert np.array_equal(got, want)


# ------------------------------------------------------------- the chain ---
def test_chain_13_modes_into_tpl_costs(I, F):
    """The loop body of tpl_model.c:556-572: every intra mode of a 16x16 block
    predicted from the neighbour plane, costed against the source; the
    per-mode costs and the first lowest mode equal the restatement's
    predictions run through the TPL cost oracle."""
    import torch
    import lavish_dsp as L
    import lavish_dsp.tpl as T
    W, H, bs, qindex = 64, 48, 16, 60
    S = R.PLANE_STRIDE
    plane = R.plane_of(F, 8, 0)  # the fixed neighbour plane: frame origin at (1, 1)
    rng = np.random.default_rng(7)
    src = np.clip(plane.reshape(R.PLANE_ROWS, S)[1:1 + H, 1:1 + W] + rng.integers(-9, 10, (H, W)),
                  0, 255).astype(np.uint8)
    cases, dst_offs = [], []
    for m in range(13):
        for by in range(H // bs):
            for bx in range(W // bs):
                ang = int(R.T["kModeToAngle"][m])
                dr = R.V_PRED <= m <= R.D67_PRED
                row = [8, 0, (1 + by * bs) * S + 1 + bx * bs, 2, m, ang, 5, 0, (bx + by) & 1, bs,
                       bs if dr and ang < 90 else -1, bs, bs if dr and ang > 180 else -1, 0]
                cases.append(R.intra_case(F, row))
                dst_offs.append(m * H * W + by * bs * W + bx * bs)
    preds = torch.zeros((13, H, W), dtype=torch.uint8, device="cuda")
    jobs = I.intra_jobs_tensor(_jobs(I, cases, [c.ref_off for c in cases], dst_offs), "cuda")
    I.intra_pred_batch(_dev(plane.astype(np.uint8)), preds.view(-1), jobs, 8, ref_stride=S,
                       dst_stride=W)
    qp = L.build_quant_params(8, qindex, L.QUANT_FP)
    out, recon, costs = T.tpl_block_batch(torch.from_numpy(src).cuda(), preds, bs, 8, qp,
                                          ref_costs=True)
    torch.cuda.synchronize()
    exp_preds = np.zeros((13, H, W), np.uint8)
    for c, off in zip(cases, dst_offs):
        m, rem = divmod(off, H * W)
        y, x = divmod(rem, W)
        exp_preds[m, y:y + bs, x:x + bs] = R.run_case(F, c, plane=plane)
    assert np.array_equal(preds.cpu().numpy(), exp_preds)
    exp, erec, ecost = O.tpl_block_batch(src, exp_preds, bs, 8, qindex)
    gcost = costs.cpu().numpy()
    assert gcost.shape == (12, 13)
    np.testing.assert_array_equal(gcost, ecost)
    np.testing.assert_array_equal(gcost.argmin(axis=1), ecost.argmin(axis=1))
    got = T.records_numpy(out)
    for f in exp.dtype.names:
        np.testing.assert_array_equal(got[f], exp[f], err_msg=f)
    np.testing.assert_array_equal(recon.cpu().numpy(), erec)
