"""GPU parity at the edges of the FAST / exact choice of the transform +
quantize kernels (lavish_txq_plane, lavish_rdo_plane / _px) against the
oracle, bit-exact.

Both kernels pick, per wave tile, the certified 24-bit FAST arithmetic when
the tile's residual obeys |x| <= kFastResidualMax (1023) and the exact
64-bit path otherwise, and report neither.  Every case here builds an input
whose tiles land on a stated path and asserts that on the host before the
launch (tests/_fastpath.py restates the tile geometry):
  - the threshold itself: +-1023 in every tile (all FAST), then one sample at
    +-1024 (that tile exact, the other tiles of its workgroup FAST);
  - FAST with the 12-bit quantizer rows (12-bit video with small residuals);
  - the exact path with the lowbd quantizers (int16 residuals past 1023 at
    bit depth 8);
  - +-max sign patterns matched to single basis functions of each transform
    type, which drive the intermediate butterflies near their maxima."""
import numpy as np
import pytest

import _fastpath as FP
import _oracle as O
from test_gpu_rdo import C4_CASES

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES_LE32 = [s for s in range(19) if O.TX_W[s] <= 32 and O.TX_H[s] <= 32]
T = FP.fast_residual_max()
EDGE_TILE = 5  # of ten: second of its workgroup's four (tiles 4 .. 7)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    import lavish_dsp
    return lavish_dsp


def _mask(s):
    return sum(1 << t for t in range(16) if O.type_valid(s, t))


def _types(mask):
    return [t for t in range(16) if (mask >> t) & 1]


def _check_txq(L, res, s, bd, qindex, quant_b, tag):
    mask = _mask(s)
    kind = L.QUANT_B if quant_b else L.QUANT_FP
    qp = L.build_quant_params(bd, qindex, kind)
    out = L.txq_plane(torch.from_numpy(res).cuda(), s, mask, qp, bit_depth=bd, quant_kind=kind)
    torch.cuda.synchronize()
    qc, dq, eob = O.txq_plane(res, s, mask, O.build_quant(bd, qindex), bd=bd, quant_b=quant_b,
                              threads=8)
    tag = str((O.TX_NAMES[s], bd, qindex, "b" if quant_b else "fp") + tuple(tag))
    np.testing.assert_array_equal(out["qcoeff"].cpu().numpy(), qc.transpose(1, 0, 2), err_msg=tag)
    np.testing.assert_array_equal(out["dqcoeff"].cpu().numpy(), dq.transpose(1, 0, 2),
                                  err_msg=tag)
    np.testing.assert_array_equal(out["eob"].cpu().numpy().view(np.uint16), eob.T, err_msg=tag)
    return qc


def _edge_cases(s, seed):
    """(name, plane): the all-FAST edge plane and its two copies with one
    sample one step past the threshold; the paths asserted on the input."""
    base = FP.edge_plane(s, seed)
    P = FP.tile_blocks(s)
    nb = (base.shape[0] // O.TX_H[s]) * (base.shape[1] // O.TX_W[s])
    assert 8 <= len(FP.tile_amax(base, s)) <= 12 and (P == 1 or nb % P)
    assert (FP.tile_amax(base, s) == T).all() and FP.tile_fast(base, s).all()
    for t in range(len(FP.tile_amax(base, s))):
        blks = [FP.block_view(base, s, b) for b in range(t * P, min((t + 1) * P, nb))]
        assert any((b == T).any() for b in blks) and any((b == -T).any() for b in blks)
    cases = [("edge", base)]
    for name, v in (("+1", T + 1), ("-1", -T - 1)):
        p = FP.past_edge(base, s, EDGE_TILE, v, seed + 1)
        fast = FP.tile_fast(p, s)
        assert (p != base).sum() == 1
        assert not fast[EDGE_TILE] and fast.sum() == len(fast) - 1
        assert fast[4] and fast[6] and fast[7]  # the rest of the workgroup
        cases.append((name, p))
    return cases


@pytest.mark.parametrize("s", SIZES_LE32)
def test_txq_threshold_edge(L, s):
    for bd in (10, 12):
        for name, res in _edge_cases(s, 100 + s):
            for quant_b in (False, True):
                _check_txq(L, res, s, bd, 96, quant_b, (name,))


@pytest.mark.parametrize("s", SIZES_LE32)
def test_txq_12bit_fast(L, s):
    """bd 12 rows with |x| <= 1023: every tile FAST."""
    rng = np.random.default_rng(200 + s)
    shape = FP.plane_shape(s)
    planes = {"random": rng.integers(-T, T + 1, shape).astype(np.int16),
              "pm": (T * rng.choice([-1, 1], shape)).astype(np.int16)}
    for name, res in planes.items():
        assert FP.tile_fast(res, s).all()
        for qindex in (0, 1, 128, 255):
            for quant_b in (False, True):
                _check_txq(L, res, s, 12, qindex, quant_b, (name,))


@pytest.mark.parametrize("s", SIZES_LE32)
def test_txq_lowbd_exact(L, s):
    """bd 8 quantizers behind the exact transform path: int16 residuals past
    the threshold in every tile (the quantizers clamp the rounded magnitude
    to int16 as av1_quantize_fp_c / aom_quantize_b_c do)."""
    rng = np.random.default_rng(300 + s)
    shape = FP.plane_shape(s)
    planes = {"extreme16": rng.integers(-32768, 32768, shape).astype(np.int16),
              "pm1024": ((T + 1) * rng.choice([-1, 1], shape)).astype(np.int16)}
    for name, res in planes.items():
        assert not FP.tile_fast(res, s).any()
        for qindex in (0, 128, 255):
            for quant_b in (False, True):
                _check_txq(L, res, s, 8, qindex, quant_b, (name,))


@pytest.mark.parametrize("s", SIZES_LE32)
def test_txq_adversarial_signs(L, s):
    types = _types(_mask(s))
    for bd, amp in ((10, T), (8, 255)):
        res = FP.adversarial_plane(s, types, amp)
        assert FP.tile_fast(res, s).all() and np.abs(res).min() == amp
        for quant_b in (False, True):
            _check_txq(L, res, s, bd, 128, quant_b, ("signs",))


# ---- the C4 decision kernels ----

RDO_FIELDS = ("best_type", "eob", "rate", "satd", "dist", "sse", "rdcost")


def _check_rdo(L, res, s, mask, bd, qindex, px, tag):
    src, pred = FP.src_pred(res, bd, 7)
    q = O.build_quant(bd, qindex)
    qp = L.build_quant_params(bd, qindex, L.QUANT_FP)
    rdmult = 1300 + 11 * s
    exp, eq, ed = O.rdo_plane(src, pred, s, mask, bd, q, rdmult, threads=8, px=px)
    out = L.rdo_plane(torch.from_numpy(src.view(np.int16)).cuda(),
                      torch.from_numpy(pred.view(np.int16)).cuda(), s, mask, qp, rdmult, bd,
                      px=px)
    got = L.rdo_records(out)
    tag = str((O.TX_NAMES[s], bd, qindex, "px" if px else "tx") + tuple(tag))
    for f in RDO_FIELDS:
        np.testing.assert_array_equal(got[f], exp[f], err_msg=tag + " " + f)
    np.testing.assert_array_equal(out["qcoeff"].cpu().numpy(), eq, err_msg=tag)
    np.testing.assert_array_equal(out["dqcoeff"].cpu().numpy(), ed, err_msg=tag)


@pytest.mark.parametrize("px", [False, True])
@pytest.mark.parametrize("s,mask", C4_CASES)
def test_rdo_threshold_edge(L, s, mask, px):
    for bd in (10, 12):
        for name, res in _edge_cases(s, 400 + s):
            _check_rdo(L, res, s, mask, bd, 128, px, (name,))


@pytest.mark.parametrize("s,mask,shape", [(0, 0xFFFF, (520, 1024)), (2, 0xFFFF, (1040, 2048)),
                                          (3, 0x201, (2080, 2048))])
def test_rdo_whole_frame_form_mixed_paths(L, s, mask, shape):
    """Below kRdoSplitTiles wave tiles the TX-domain decision of a size with
    several vertical kinds runs its split form (the cases above); a frame's
    worth of tiles runs the one-wave-per-tile form the benchmark times.  The
    same edge there: everything FAST but two tiles, one sample past the
    threshold each."""
    import re
    src = open(FP.ROOT + "/aom-av1-lavish_amd/csrc/rdo_kern.h").read()
    split_below = int(re.search(r"kRdoSplitTiles\s*=\s*(\d+)", src).group(1))
    rng = np.random.default_rng(600 + s)
    res = rng.integers(-T, T + 1, shape).astype(np.int16)
    ntiles = len(FP.tile_amax(res, s))
    assert ntiles >= split_below
    P = FP.tile_blocks(s)
    for tile, v in ((5, T + 1), (ntiles - 3, -T - 1)):
        FP.block_view(res, s, tile * P + P - 1)[1, 2] = v
    fast = FP.tile_fast(res, s)
    assert not fast[5] and not fast[ntiles - 3] and fast.sum() == ntiles - 2
    _check_rdo(L, res, s, mask, 12, 100, False, ("whole frame",))


@pytest.mark.parametrize("bd", [10, 12])
def test_txq_frame_mixed_paths(L, bd):
    """lavish_txq_frame (the multi-size kernels the benchmark times run the
    same tile body): one plane, every size <= 32x32, one sample past the
    threshold -- per size exactly the tile holding it is exact."""
    rng = np.random.default_rng(700 + bd)
    res = rng.integers(-T, T + 1, (96, 128)).astype(np.int16)
    res[37, 70] = T + 1
    for s in SIZES_LE32:
        fast = FP.tile_fast(res, s)
        assert (~fast).sum() == 1 and len(fast) >= 6
    dres = torch.from_numpy(res).cuda()
    frame = L.FrameOutputs(dres, SIZES_LE32)
    qp = L.build_quant_params(bd, 77, L.QUANT_FP)
    outs = L.txq_frame(dres, frame, qp, bit_depth=bd)
    torch.cuda.synchronize()
    for s in SIZES_LE32:
        qc, dq, eob = O.txq_plane(res, s, _mask(s), O.build_quant(bd, 77), bd=bd, threads=8)
        tag = O.TX_NAMES[s]
        np.testing.assert_array_equal(outs[s]["qcoeff"].cpu().numpy(), qc.transpose(1, 0, 2),
                                      err_msg=tag)
        np.testing.assert_array_equal(outs[s]["dqcoeff"].cpu().numpy(), dq.transpose(1, 0, 2),
                                      err_msg=tag)
        np.testing.assert_array_equal(outs[s]["eob"].cpu().numpy().view(np.uint16), eob.T,
                                      err_msg=tag)


@pytest.mark.parametrize("px", [False, True])
@pytest.mark.parametrize("s,mask", C4_CASES)
def test_rdo_12bit_fast(L, s, mask, px):
    rng = np.random.default_rng(500 + s)
    shape = FP.plane_shape(s)
    planes = {"random": rng.integers(-T, T + 1, shape).astype(np.int16),
              "pm": (T * rng.choice([-1, 1], shape)).astype(np.int16)}
    for name, res in planes.items():
        assert FP.tile_fast(res, s).all()
        for qindex in (0, 255):
            _check_rdo(L, res, s, mask, 12, qindex, px, (name,))


@pytest.mark.parametrize("px", [False, True])
@pytest.mark.parametrize("s,mask", C4_CASES)
def test_rdo_adversarial_signs(L, s, mask, px):
    res = FP.adversarial_plane(s, _types(mask), T)
    assert FP.tile_fast(res, s).all()
    _check_rdo(L, res, s, mask, 10, 128, px, ("signs",))
