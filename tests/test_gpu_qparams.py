"""Quantizer parameters outside what av1_build_quantizer makes.

The lowbd fast form of quantize_fp (csrc/txq_dev.h) and the CHEAP form
(csrc/rdo_kern.h) are exact for quant >= 0, dequant > 0 and quant * dequant
near 2^16; the batch entry points refuse LAVISH_QUANT_FP rows outside that
(quant_fp_params_ok, csrc/lavish_internal.h) and leave their outputs alone.
Rows inside it that no table holds -- the product anywhere up to 2^17 -- are
computed, and checked here against the oracle.  LAVISH_QUANT_B rows and the
per-call quantizer shims take any int16."""
import numpy as np
import pytest

import _oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

POISON = 0x5A
# (what, field, index, value) on top of the bd-8 / qindex-128 fp row
BAD = [("quant[0] < 0", "quant", 0, -1), ("quant[1] < 0", "quant", 1, -300),
       ("dequant[1] == 0", "dequant", 1, 0), ("dequant[0] < 0", "dequant", 0, -7),
       ("quant * dequant > 2^17", "dequant", 1, 32767)]
BAD_IDS = ["dc_quant_neg", "ac_quant_neg", "ac_dequant_zero", "dc_dequant_neg", "product"]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    import lavish_dsp
    return lavish_dsp


def _bad(L, bd, field, i, v):
    qp = L.build_quant_params(bd, 128, L.QUANT_FP)
    getattr(qp, field)[i] = v
    return qp


def _poison(tensors):
    for t in tensors:
        t.view(torch.uint8).fill_(POISON)


def _untouched(tensors):
    torch.cuda.synchronize()
    return all(bool((t.view(torch.uint8) == POISON).all()) for t in tensors)


def _flat(outs):  # {size: {name: tensor}}
    return [t for o in outs.values() for t in o.values()]


@pytest.mark.parametrize("what,field,i,v", BAD, ids=BAD_IDS)
def test_fp_rows_refused_by_txq(L, what, field, i, v):
    res = torch.randint(-255, 256, (64, 128), dtype=torch.int16, device="cuda")
    qp = _bad(L, 8, field, i, v)
    for s in (2, 3, 4):  # 16x16, 32x32 and a 64-point size (its own kernel)
        out = L.txq_plane_out(res, s, 1)
        _poison(out.values())
        with pytest.raises(ValueError):
            L.txq_plane(res, s, 1, qp, out=out)
        assert _untouched(out.values()), (what, s)
    frame = L.FrameOutputs(res, [0, 2, 3, 4])
    _poison(_flat(frame.outs))
    with pytest.raises(ValueError):
        L.txq_frame(res, frame, qp)
    assert _untouched(_flat(frame.outs)), what
    # lavish_txq_frame_search: neither the transform sizes nor the search run
    import lavish_dsp.motion as M
    import lavish_dsp.synth as synth
    src, refs = synth.motion_planes(64, 64, 1, 160, seed=3)
    jobs = M.frame_jobs(64, 64, src.shape[1], 160, src.size, 16, 16, 1)
    ts, tr = torch.from_numpy(src).cuda(), torch.from_numpy(refs).cuda()
    tiles = M.RefTiles(tr, ts.stride(0)).build()
    sres = torch.empty(len(jobs) * M.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    for sizes in ([0, 2], [2, 3]):  # the <= 16-point class alone / with a 32-point size
        frame = L.FrameOutputs(res, sizes)
        _poison(_flat(frame.outs) + [sres])
        with pytest.raises(ValueError):
            M.txq_frame_search(res, frame, qp, ts, tr, M.to_device(jobs), M.l1_cost_params(),
                               tiles, sres, None, 3)
        assert _untouched(_flat(frame.outs) + [sres]), (what, sizes)
    # the same row is a legitimate LAVISH_QUANT_B row (invert_quant's quant is
    # negative for most qindex) and the transform alone reads none of it
    L.txq_plane(res, 2, 1, qp, quant_kind=L.QUANT_B)
    L.txq_plane(res, 2, 1, qp, quant_kind=L.QUANT_NONE, with_coeff=True)
    torch.cuda.synchronize()
    assert L.status()[0] == 0, L.status()


@pytest.mark.parametrize("what,field,i,v", BAD, ids=BAD_IDS)
def test_fp_rows_refused_by_rdo(L, what, field, i, v):
    src = torch.randint(0, 1024, (64, 128), dtype=torch.int16, device="cuda")
    pred = torch.randint(0, 1024, (64, 128), dtype=torch.int16, device="cuda")
    qp = _bad(L, 10, field, i, v)
    for s, mask in ((2, 0xFFFF), (3, 0x201), (4, 1)):
        for px in (False, True):
            out = L.rdo_out(src, s)
            _poison(out.values())
            with pytest.raises(ValueError):
                L.rdo_plane(src, pred, s, mask, qp, 1000, 10, out=out, px=px)
            assert _untouched(out.values()), (what, s, px)
    out = L.rdo_out(src, 2)
    _poison(out.values())
    with pytest.raises(ValueError):
        L.rdo_plane_masked(src, pred, 2, 0xFFFF, qp, 1000, out=out)
    assert _untouched(out.values()), what
    for px in (False, True):
        fr = L.RdoFrame(src)
        _poison(_flat(fr.outs))
        with pytest.raises(ValueError):
            L.rdo_frame(src, pred, fr, qp, 1000, 10, reconstruct=False, px=px)
        assert _untouched(_flat(fr.outs)), (what, px)
    assert L.status()[0] == 0, L.status()


# fp rows no table holds, inside the accepted range: (quant, dequant) DC / AC
ODD_ROWS = [((16384, 8), (16384, 8)),       # the product at 2^17 exactly
            ((32767, 4), (4, 32767)),       # 2^17 - 4, both ways round
            ((0, 50), (1, 300)),            # quant 0 and 1: everything quantizes to 0
            ((9000, 3), (700, 41)),         # the product well below 2^16
            ((2000, 60), (1900, 66))]       # ~1.9 x 2^16


def _odd(L, bd, qindex, row):
    qp = L.build_quant_params(bd, qindex, L.QUANT_FP)
    q = O.build_quant(bd, qindex)
    for i, (qt, dq) in enumerate(row):
        qp.quant[i], qp.dequant[i] = qt, dq
        q.quant_fp[i], q.dequant[i] = qt, dq
    return qp, q


@pytest.mark.parametrize("row", ODD_ROWS)
@pytest.mark.parametrize("s", [0, 2, 3, 13, 4])
def test_odd_fp_rows_txq_vs_oracle(L, s, row):
    W, H = O.TX_W[s], O.TX_H[s]
    mask = sum(1 << t for t in range(16) if O.type_valid(s, t))
    rng = np.random.default_rng(s)
    for bd in (8, 10, 12):
        m = (1 << bd) - 1
        res = rng.integers(-m, m + 1, (3 * H, 5 * W)).astype(np.int16)
        qp, q = _odd(L, bd, 100, row)
        out = L.txq_plane(torch.from_numpy(res).cuda(), s, mask, qp, bit_depth=bd)
        torch.cuda.synchronize()
        qc, dq, eob = O.txq_plane(res, s, mask, q, bd=bd, threads=8)
        tag = str((O.TX_NAMES[s], bd, row))
        np.testing.assert_array_equal(out["qcoeff"].cpu().numpy(), qc.transpose(1, 0, 2),
                                      err_msg=tag)
        np.testing.assert_array_equal(out["dqcoeff"].cpu().numpy(), dq.transpose(1, 0, 2),
                                      err_msg=tag)
        np.testing.assert_array_equal(out["eob"].cpu().numpy().view(np.uint16), eob.T,
                                      err_msg=tag)


@pytest.mark.parametrize("row", ODD_ROWS)
@pytest.mark.parametrize("s,mask", [(0, 0xFFFF), (2, 0xFFFF), (3, 0x201), (13, 0xFFFF), (4, 1)])
def test_odd_fp_rows_rdo_vs_oracle(L, s, mask, row):
    """The FAST block error narrows to 24 / 32 bits on |dqcoeff| <= |coeff| +
    dequant, which the accepted product bound has to cover."""
    W, H = O.TX_W[s], O.TX_H[s]
    rng = np.random.default_rng(50 + s)
    for bd in (10, 12):
        m = (1 << bd) - 1
        src = rng.integers(0, m + 1, (3 * H, 5 * W)).astype(np.uint16)
        pred = np.clip(src.astype(np.int32) + rng.integers(-1023, 1024, src.shape), 0,
                       m).astype(np.uint16)
        qp, q = _odd(L, bd, 100, row)
        for px in (False, True):
            exp, eq, ed = O.rdo_plane(src, pred, s, mask, bd, q, 1500, threads=8, px=px)
            out = L.rdo_plane(torch.from_numpy(src.view(np.int16)).cuda(),
                              torch.from_numpy(pred.view(np.int16)).cuda(), s, mask, qp, 1500,
                              bd, px=px)
            got = L.rdo_records(out)
            tag = str((O.TX_NAMES[s], bd, px, row))
            for f in ("best_type", "eob", "rate", "satd", "dist", "sse", "rdcost"):
                np.testing.assert_array_equal(got[f], exp[f], err_msg=tag + " " + f)
            np.testing.assert_array_equal(out["qcoeff"].cpu().numpy(), eq, err_msg=tag)
            np.testing.assert_array_equal(out["dqcoeff"].cpu().numpy(), ed, err_msg=tag)


@pytest.mark.parametrize("ls", [0, 1, 2])
@pytest.mark.parametrize("highbd", [False, True])
def test_quantize_fp_shims_take_any_int16(L, highbd, ls):
    """av1_quantize_fp* / av1_highbd_quantize_fp with a negative quant_fp and
    a dequant unrelated to it (av1_quantize.c:174-194 has no such condition):
    the shims run the plain form and agree with the oracle, also where the
    negative quantized magnitude is shifted by log_scale."""
    tx = {0: 2, 1: 3, 2: 3}[ls]
    n = 1024 if ls == 2 else O.max_eob(tx)
    scan, iscan = L.scan_order(tx, 0)
    rng = np.random.default_rng(11 + highbd)
    bd = 10 if highbd else 8
    for quant_fp, dequant in (((-1200, -77), (900, 31)), ((-32768, 5), (3, 32767)),
                              ((700, -1), (-40, 12))):
        q = O.build_quant(bd, 128)
        for i in range(2):
            q.quant_fp[i], q.dequant[i] = quant_fp[i], dequant[i]
        qa = O.quant_arrays(q)
        c = rng.integers(-(1 << (7 + bd)), 1 << (7 + bd), n).astype(np.int32)
        c[rng.random(n) < 0.3] = 0
        qc, dq, eob = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(1, np.uint16)
        a = (c, n, qa["zbin"], qa["round_fp"], qa["quant_fp"], qa["quant_shift"], qc, dq,
             qa["dequant"], eob, scan, iscan)
        if highbd:
            L.av1_highbd_quantize_fp(*a, ls)
        else:
            getattr(L, "av1_quantize_fp" + ("", "_32x32", "_64x64")[ls])(*a)
        rq, rdq, reob = O.quantize("fp", c, n, q, scan, iscan, ls, highbd=highbd)
        tag = str((highbd, ls, quant_fp, dequant))
        np.testing.assert_array_equal(qc, rq, err_msg=tag)
        np.testing.assert_array_equal(dq, rdq, err_msg=tag)
        assert int(eob[0]) == reob, tag
        assert (rq != 0).any(), tag
