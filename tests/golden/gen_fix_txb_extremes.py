#!/usr/bin/env python3
"""fix_txb_extremes.npz: the coefficient rate and the trellis at their
extremes, produced by executing the reference's own C text
(tests/golden/cinterp.py), like gen_fixtures.py and gen_fix_qm.py (whose
reference state, Ref, this generator reuses with the matrices off: level 15).

Executed from the reference:
  av1_cost_coeffs_txb and av1_cost_coeffs_txb_laplacian
    (av1/encoder/txb_rdopt.c:599-660) on the level-map blocks of
    tests/_txbextremes.py (all 127+, all 3 / 2 / 14 / 15 / 16, checkerboards of
    0 and 2^17, the 21-bit Golomb block, eob 0 / 1 / n) for every case of
    LEVEL_CASES, and on a sample of its neighbour probes ("c_rows");
  av1_quant (FP) and av1_optimize_b (encodemb.c:87-103, 308-341) at bd 8, 10
    and 12, qindex 0 / 128 / 255, rdmult 200 / 60000 / 2^20, sharpness 0 / 2,
    luma inter / luma intra / chroma, the three tx classes, sizes up to 64x64,
    on the transform of _txbextremes.residuals() ("t_rows").

The inputs are not stored where _txbextremes.py rebuilds them from the row:
a cost row names its block (set, case, block number) and carries the CRC of
its qcoeff bytes; a trellis row names (kind, seed, magnitude) and stores the
reference quantizer's qcoeff / dqcoeff and what the walk changed in them.
The coefficients themselves come from the CPU oracle's forward transform
(pinned to the reference by fix_txfm.npz): they are inputs, not results.

The generator stops unless the conditions of check_conditions() hold (each
count at least 4).  Run time on one core: about a minute (measured 63 s), of
which 25 s parse the reference.

Usage: python tests/golden/gen_fix_txb_extremes.py
"""
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_fixtures as G  # noqa: E402
import gen_fix_qm as Q  # noqa: E402
import _txbextremes as X  # noqa: E402

_get, _set = G._get, G._set

TABLE_SEED = 4242
C_FIELDS, T_FIELDS = X.C_FIELDS, X.T_FIELDS
# the probe offsets a cost row samples per target: none, the union of the
# three classes' neighbours and three that no class reads
PROBE_SAMPLE = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0), (3, 0), (4, 0), (0, 3), (0, 4),
                (2, 2), (1, 2), (4, 4)]


def crc(q):
    return zlib.crc32(np.ascontiguousarray(q, np.int32).tobytes())


def cost_cases():
    """(set, s, t, plane, block numbers): every level block of every case,
    planes alternating; per probe case the sampled offsets of every target."""
    cases = []
    for k, (s, t) in enumerate(X.LEVEL_CASES):
        nb = len(X.level_blocks(s, t)[2])
        cases.append((0, s, t, k & 1, list(range(nb))))
    for k, (s, t) in enumerate(X.PROBE_CASES):
        _, _, index = X.probe_blocks(s, t)
        blocks = []
        for per in index.values():
            for off in PROBE_SAMPLE:
                if off in per:
                    blocks += list(per[off])
        cases.append((1, s, t, 0, blocks))
    return cases


def cost_rows(ref, cases, log=True):
    """Run the two reference functions on the named blocks -> rows."""
    tu = ref.tu
    rows = []
    for which, s, t, plane, blocks in cases:
        q, eob = (X.level_blocks(s, t) if which == 0 else X.probe_blocks(s, t))[:2]
        n = G.max_eob(s)
        ref.setup_block(8, s, plane, 0, 15, np.zeros(n, np.int64))
        for b in blocks:
            ref.qb.buf[:] = [int(v) for v in q[b]]
            ref.eb.buf[0] = int(eob[b])
            skip_ctx, dc_ctx = (7 * b + s) % 13, (b + t) % 3
            ctx = tu.struct_obj("TXB_CTX")
            _set(ctx.buf[0], txb_skip_ctx=skip_ctx, dc_sign_ctx=dc_ctx)
            rate = tu.func("av1_cost_coeffs_txb")(ref.x, plane, 0, s, t, ctx, 0)
            lap = tu.func("av1_cost_coeffs_txb_laplacian")(ref.x, plane, 0, s, t, ctx, 0, 0)
            ttc = tu.func("get_tx_type_cost")(ref.x, ref.xd_p, plane, s, t, 0)
            rows.append([which, s, t, plane, b, int(eob[b]), skip_ctx, dc_ctx, ttc, rate, lap,
                         crc(q[b])])
        if log:
            print("  cost set %d size %d type %d: %d rows" % (which, s, t, len(rows)), flush=True)
    return np.array(rows, np.int64)


# (tx_size, tx_type): the three classes at 16x16 and 4x4, the 32- and 64-point
# sizes, rectangles of both orientations, IDTX
TR_CASES = [(2, 0), (2, 10), (2, 11), (3, 0), (4, 0), (11, 0), (18, 0), (15, 9), (0, 0), (0, 10),
            (0, 11), (8, 0), (13, 11), (14, 10)]
QINDEX = (0, 128, 255)
RDMULT = (200, 60000, 1 << 20)
PLANES = ((0, 1), (0, 0), (1, 1))  # (plane, is_inter)
# the sparse kind: (qindex, magnitude) per bit depth at which the reference's
# walk ends in update_skip (found on the CPU oracle, asserted below)
SPARSE = X.SPARSE_POINT


def trellis_cases():
    """One dict per row.  The dense kinds cycle through every qindex, rdmult,
    sharpness and plane; the sparse rows run at their tuned point with
    sharpness 0 and a high rdmult, where update_skip decides."""
    rows = []
    k = 0
    for bd in (8, 10, 12):
        for s, t in TR_CASES:
            for kind in (0, 2) if G.max_eob(s) >= 512 else (0, 1, 2):
                rows.append(dict(bd=bd, s=s, t=t, qindex=QINDEX[k % 3], rdmult=RDMULT[(k // 3) % 3],
                                 sharp=(0, 2, 0, 0)[k % 4], plane=PLANES[(k // 2) % 3][0],
                                 inter=PLANES[(k // 2) % 3][1], kind=kind, seed=9000 + k, mag=3))
                k += 1
        # bd 12 at qindex 255 on the largest sizes, whatever the cycle gave
        if bd == 12:
            for s, t in ((4, 0), (3, 0), (2, 11), (11, 0)):
                rows.append(dict(bd=12, s=s, t=t, qindex=255, rdmult=RDMULT[k % 3], sharp=0,
                                 plane=0, inter=1, kind=0, seed=9000 + k, mag=3))
                k += 1
        qi, mag = SPARSE[bd]
        for j, (s, t) in enumerate(((2, 0), (0, 0), (2, 10), (2, 11), (3, 0), (8, 0), (0, 11),
                                    (13, 11))):
            rows.append(dict(bd=bd, s=s, t=t, qindex=qi, rdmult=RDMULT[1 + (j & 1)], sharp=0,
                             plane=PLANES[j % 3][0], inter=PLANES[j % 3][1], kind=3,
                             seed=9500 + k, mag=mag))
            k += 1
    return rows


def trellis_row(ref, r):
    """av1_quant (FP) then av1_optimize_b on one row's coefficients."""
    tu = ref.tu
    s, t, bd, plane = r["s"], r["t"], r["bd"], r["plane"]
    c = X.coeffs(X.KINDS[r["kind"]], s, t, bd, 1, r["seed"], r["mag"])[0]
    ref.setup_block(bd, s, plane, r["qindex"], 15, c, r["inter"])
    _set(ref.X, rdmult=r["rdmult"])
    oxcf = _get(ref.cpi.buf[0], "oxcf")
    _set(_get(oxcf, "algo_cfg"), sharpness=r["sharp"])
    _set(_get(oxcf, "tune_cfg"), dist_metric=ref.E["AOM_DIST_METRIC_PSNR"])
    qp = ref.quant_param(s, t, plane, Q.FP, 1)
    assert _get(qp.buf[0], "qmatrix") is None and _get(qp.buf[0], "iqmatrix") is None
    q_in, dq_in, eob_in = ref.run_quant(bd, s, t, plane, qp)
    skip_ctx, dc_ctx = r["seed"] % 13, r["seed"] % 3
    ctx = tu.struct_obj("TXB_CTX")
    _set(ctx.buf[0], txb_skip_ctx=skip_ctx, dc_sign_ctx=dc_ctx)
    rate = tu.buffer("int", 1)
    ref.ec.buf[0] = 0
    eob = tu.func("av1_optimize_b")(ref.cpi, ref.x, plane, 0, s, t, ctx, rate)
    ttc = tu.func("get_tx_type_cost")(ref.x, ref.xd_p, plane, s, t, 0)
    return dict(q_in=q_in, dq_in=dq_in, eob_in=eob_in, q=np.array(ref.qb.buf, np.int32),
                dq=np.array(ref.db.buf, np.int32), eob=int(eob), rate=int(rate.buf[0]),
                entropy=int(ref.ec.buf[0]), ttc=int(ttc), skip_ctx=skip_ctx, dc_ctx=dc_ctx)


def trellis_rows(ref, cases, log=True):
    rows, arrs = [], {k: [] for k in ("q_in", "dq_in", "q", "dq")}
    off = 0
    for i, r in enumerate(cases):
        o = trellis_row(ref, r)
        n = G.max_eob(r["s"])
        rows.append([r["bd"], r["s"], r["t"], r["qindex"], r["plane"], r["inter"], r["sharp"],
                     r["rdmult"], r["kind"], r["seed"], r["mag"], o["skip_ctx"], o["dc_ctx"],
                     o["ttc"], o["eob_in"], o["eob"], o["rate"], o["entropy"], n, off])
        for k in arrs:
            arrs[k].append(o[k])
        off += n
        if log and i % 20 == 19:
            print("  trellis: %d of %d rows" % (i + 1, len(cases)), flush=True)
    out = {"t_rows": np.array(rows, np.int64)}
    out["t_qcoeff_in"] = np.concatenate(arrs["q_in"])
    out["t_dqcoeff_in"] = np.concatenate(arrs["dq_in"])
    # the walk changes few coefficients: its result is stored as a difference
    out["t_qcoeff_delta"] = np.concatenate(arrs["q"]) - out["t_qcoeff_in"]
    out["t_dqcoeff_delta"] = np.concatenate(arrs["dq"]) - out["t_dqcoeff_in"]
    return out


def check_conditions(F):
    T = F["t_rows"]
    c = X.trellis_conditions(T, F["t_qcoeff_in"], F["t_dqcoeff_in"],
                   F["t_qcoeff_in"] + F["t_qcoeff_delta"], F["t_dqcoeff_in"] + F["t_dqcoeff_delta"])
    fails = []
    for k, v in c.items():
        ok = v == 9 if k == "class_bd_pairs" else v >= 4
        print("  %-4s %s = %d" % ("ok" if ok else "FAIL", k, v))
        if not ok:
            fails.append(k)
    J = {n: i for i, n in enumerate(T_FIELDS)}
    for name, want in (("qindex", set(QINDEX)), ("rdmult", set(RDMULT)), ("sharpness", {0, 2}),
                       ("tx_size", {3, 4, 11, 18})):
        have = set(T[:, J[name]].tolist())
        if not want <= have:
            fails.append("%s %s missing" % (name, sorted(want - have)))
    pi = set(zip(T[:, J["plane"]].tolist(), T[:, J["is_inter"]].tolist()))
    if not set(PLANES) <= pi:
        fails.append("plane / is_inter pairs")
    if fails:
        raise SystemExit("fixture conditions not met:\n  " + "\n  ".join(fails))
    return c


def make_ref():
    ref = Q.Ref()
    blob = X.tables(TABLE_SEED)
    mc = _get(ref.X, "mode_costs")
    rng = np.random.default_rng(TABLE_SEED + 1)
    itx = rng.integers(30, 3000, len(_get(mc, "inter_tx_type_costs")))
    atx = rng.integers(30, 3000, len(_get(mc, "intra_tx_type_costs")))
    ref.set_costs(blob[:10 * G.CC_COEFF_COST], blob[10 * G.CC_COEFF_COST:], itx, atx)
    return ref


def main():
    t0 = time.time()
    ref = make_ref()
    F = {"c_fields": np.array(C_FIELDS), "t_fields": np.array(T_FIELDS),
         "table_seed": np.array([TABLE_SEED], np.int64)}
    F["c_rows"] = cost_rows(ref, cost_cases())
    F.update(trellis_rows(ref, trellis_cases()))
    check_conditions(F)
    path = os.path.join(HERE, "fix_txb_extremes.npz")
    np.savez_compressed(path, **F)
    print("wrote %s (%d bytes) in %.0f s" % (path, os.path.getsize(path), time.time() - t0))


if __name__ == "__main__":
    main()
