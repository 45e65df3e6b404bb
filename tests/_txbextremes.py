"""Worst-case inputs for the coefficient-rate layer: cost_coeffs_txb_batch,
optimize_b_batch (the trellis) and the coefficient-rate ranking of C4
(rdo_plane_rate).  Everything is built deterministically from seeds with
numpy; the forward transform and the scans come from the CPU oracle (pinned
to the reference by fix_txfm.npz), so the CPU test, the GPU test and the
fixture generator (tests/golden/gen_fix_txb_extremes.py) see the same bytes.

  level_blocks()   qcoeff set directly, eob consistent with the scan: all
                   127+, all exactly 3 / 2 / 14 / 15 / 16, checkerboards of 0
                   and 2^17, one block in the 21-bit Golomb range, eob 0 / 1 / n
  probe_blocks()   one target (level 5) and one neighbour (level 9) per
                   candidate offset in {0..4} x {0..4}, each with the target
                   removed beside it, to read off which neighbours a context
                   takes
  residuals()      "sat" +-(2^bd - 1) random sign, "const" +-max per block,
                   "lap" Laplacian of scale max / 6, "sparse" one or two
                   small nonzeros
  coeffs()         the forward transform of residuals()
  plane()          src / pred planes whose difference is residuals()
  tables()         cost tables of the suite's usual magnitude, cells distinct
  stride_blocks()  batches past the cost kernel's grid cap, dense and sparse
                   blocks alternating in each workgroup slot

The second half holds the cases both tests run (trellis_group(),
sparse_group(), rdo_case()) with the oracle's results, and the check_*()
functions that assert each case reaches the regime it is for.
"""
import functools
import os

import numpy as np

import _oracle as O

KINDS = ("sat", "const", "lap", "sparse")

# (tx_size, tx_type) of the level-map and probe sets: per tx class (types
# 0 / 9: 2-D, 11: horizontal, 10: vertical) a square, a wide, a tall and
# -- 2-D only, the 64-point sizes have no other type -- a 64-point-adjusted size
LEVEL_CASES = [(2, 0), (10, 0), (9, 0), (4, 0), (17, 0), (18, 0), (0, 0), (15, 9),
               (2, 11), (14, 11), (13, 11), (0, 11),
               (2, 10), (14, 10), (13, 10), (0, 10)]
PROBE_CASES = [(2, 0), (7, 0), (8, 0), (2, 11), (2, 10)]

GOLOMB21 = (1 << 20) + 14  # get_golomb_cost's r = level - 14 reaches 2^20: length 21


def tx_class(t):
    """tx_type_to_class: 0 2-D, 1 horizontal, 2 vertical."""
    return 0 if t < 10 else (1 if t & 1 else 2)


def dims(s):
    """av1_get_adjusted_tx_size's (w, h): the level map's extent."""
    return min(O.TX_W[s], 32), min(O.TX_H[s], 32)


def tables(seed):
    """The CoeffCosts blob, 30..4000, the cells of each LV_MAP_COEFF_COST and
    each LV_MAP_EOB_COST pairwise distinct (a call reads one of each)."""
    rng = np.random.default_rng(seed)
    parts = [30 + rng.permutation(3971)[:O.CC_COEFF_COST] for _ in range(10)]
    parts += [30 + rng.permutation(3971)[:O.CC_EOB_COST] for _ in range(14)]
    return np.concatenate(parts).astype(np.int32)


def table_cells_distinct(blob, s, plane):
    """The cells one call reads (one LV_MAP_COEFF_COST, one LV_MAP_EOB_COST)
    are pairwise distinct."""
    w, h = O.TX_W[s], O.TX_H[s]
    lg = lambda v: int(v).bit_length() - 1
    txs_ctx = (lg(min(w, h)) - 2 + lg(max(w, h)) - 2 + 1) >> 1
    pt = int(plane > 0)
    a = blob[(txs_ctx * 2 + pt) * O.CC_COEFF_COST:][:O.CC_COEFF_COST]
    return len(np.unique(a)) == len(a)


def _eob_of(q, iscan):
    nz = np.flatnonzero(q)
    return int(iscan[nz].max()) + 1 if len(nz) else 0


def level_blocks(s, t, seed=0):
    """-> (qcoeff int32 [nb, n], eob uint16 [nb], names)."""
    n = O.max_eob(s)
    w, h = dims(s)
    scan, iscan = O.scan(s, t).astype(np.int64), O.iscan(s, t).astype(np.int64)
    rng = np.random.default_rng(1000 * s + t + seed)
    sign = lambda: rng.choice(np.array([-1, 1]), n)
    blocks, names = [], []

    def add(name, q):
        blocks.append(np.asarray(q, np.int64).astype(np.int32))
        names.append(name)

    add("all127+", (127 + np.arange(n) % 5) * sign())
    for v in (3, 2, 14, 15, 16):
        add("all%d" % v, v * sign())
    pos = np.arange(n)
    board = ((pos // h + pos % h) & 1).astype(np.int64)  # raster = col * h + row
    add("checker0", board * (1 << 17) * sign())
    add("checker1", (1 - board) * (1 << 17) * sign())
    add("golomb21", (GOLOMB21 - (np.arange(n) & 1)) * sign())
    add("eob0", np.zeros(n))
    for k, v in enumerate((1, -2, 3, -15, 1 << 17)):
        q = np.zeros(n)
        q[0] = v
        add("eob1_%d" % k, q)
    # dense up to a scan index, nothing after: eob 2, 3 and an interior one
    for e in (2, 3, n // 2 + 1):
        q = np.zeros(n, np.int64)
        q[scan[:e]] = (15 + np.arange(e) % 3) * sign()[:e]
        add("dense_to_%d" % e, q)
    # eob = n reached by a lone last coefficient
    q = np.zeros(n)
    q[scan[n - 1]] = -16
    add("last_only", q)
    q = np.stack(blocks)
    eob = np.array([_eob_of(b, iscan) for b in q], np.uint16)
    return q, eob, names


def nbr_offsets(cls):
    """(dcol, drow) of get_nz_mag's five neighbours (txb_common.h:150-173;
    the first three are get_br_ctx's, :103-135)."""
    if cls == 0:
        return [(0, 1), (1, 0), (1, 1), (0, 2), (2, 0)]
    if cls == 1:
        return [(0, 1), (1, 0), (2, 0), (3, 0), (4, 0)]
    return [(0, 1), (1, 0), (0, 2), (0, 3), (0, 4)]


def probe_targets(s, t):
    """(col, row, zone) of the probe targets of one case: each nz_ctx zone of
    the class and the last rows / columns, where the map's pad is read."""
    w, h = dims(s)
    cls = tx_class(t)
    if cls == 0:
        tg = [(0, 0, "pos0"), (1, 0, "sum<2"), (0, 1, "sum<2"), (1, 2, "sum<4"), (3, 0, "sum<4"),
              (5, 6, "beyond"), (w - 2, h - 2, "edge"), (w - 1, h - 4, "edge"),
              (w - 4, h - 1, "edge"), (w - 1, 3, "edge"), (2, h - 1, "edge")]
        if O.TX_W[s] < O.TX_H[s]:
            tg += [(3, 1, "wlt"), (w - 1, 0, "wlt"), (3, 2, "beyond")]
        if O.TX_W[s] > O.TX_H[s]:
            tg += [(1, 3, "wgt"), (0, h - 1, "wgt"), (2, 3, "beyond")]
        return tg
    if cls == 1:
        return [(0, 5, "idx0"), (1, 5, "idx1"), (7, 5, "idx2+"), (w - 5, 2, "idx2+"),
                (w - 4, 2, "edge"), (w - 2, 5, "edge"), (w - 1, 3, "edge"), (3, h - 1, "edge"),
                (0, 0, "idx0")]
    return [(5, 0, "idx0"), (5, 1, "idx1"), (5, 7, "idx2+"), (2, h - 5, "idx2+"),
            (2, h - 4, "edge"), (5, h - 2, "edge"), (3, h - 1, "edge"), (w - 1, 3, "edge"),
            (0, 0, "idx0")]


def probe_blocks(s, t):
    """-> (qcoeff [nb, n], eob [nb], index) with index[(col, row)][(dc, dr)] =
    (block with target and neighbour, block with the neighbour only);
    (dc, dr) = (0, 0) is the pair without a neighbour.  Every block also
    holds level 1 at the last scan position, so eob = n throughout and the
    target is never the last coefficient.  A neighbour that would fall
    outside the block has no entry."""
    n = O.max_eob(s)
    w, h = dims(s)
    scan = O.scan(s, t)
    anchor = int(scan[n - 1])
    blocks, index = [], {}
    for col, row, _ in probe_targets(s, t):
        tp = col * h + row
        assert tp != anchor
        per = {}
        for dc in range(5):
            for dr in range(5):
                c2, r2 = col + dc, row + dr
                if c2 >= w or r2 >= h:
                    continue
                base = np.zeros(n, np.int32)
                base[anchor] = 1
                if (dc, dr) != (0, 0):
                    base[c2 * h + r2] = 9
                both = base.copy()
                both[tp] = -5 if (col + row) & 1 else 5
                per[(dc, dr)] = (len(blocks), len(blocks) + 1)
                blocks += [both, base]
        index[(col, row)] = per
    q = np.stack(blocks)
    return q, np.full(len(q), n, np.uint16), index


def probe_sets(rates, index):
    """{target: set of offsets whose neighbour changes what the target adds
    to the rate}: rate(target, neighbour) - rate(neighbour) against the same
    difference without a neighbour.  Besides the target's own cost the
    difference holds the target's effect on the contexts of the zeros above
    and left of it; a neighbour interacts with that only at an offset that is
    a difference of two of the class's own offsets, and those with both parts
    >= 0 are themselves among the five, so the set is the set of positions
    the target's contexts read."""
    rates = np.asarray(rates, np.int64)
    out = {}
    for tgt, per in index.items():
        d0 = rates[per[(0, 0)][0]] - rates[per[(0, 0)][1]]
        out[tgt] = {off for off, (a, b) in per.items()
                    if off != (0, 0) and rates[a] - rates[b] != d0}
    return out


def probe_expected(s, t):
    """The sets probe_sets() must give, from the reference's definition: the
    class's five neighbours that lie inside the block; position 0 of the 2-D
    class has the fixed context 0 (get_nz_map_ctx_from_stats) and reads only
    get_br_ctx's three."""
    w, h = dims(s)
    cls = tx_class(t)
    out = {}
    for col, row, _ in probe_targets(s, t):
        offs = nbr_offsets(cls)
        if cls == 0 and col == 0 and row == 0:
            offs = offs[:3]
        out[(col, row)] = {(dc, dr) for dc, dr in offs if col + dc < w and row + dr < h}
    return out


def residuals(kind, w, h, bd, nb, seed, sparse_mag=3):
    """int16 [nb, h, w]."""
    mx = (1 << bd) - 1
    rng = np.random.default_rng(seed)
    if kind == "sat":
        r = rng.choice(np.array([-mx, mx]), (nb, h, w))
    elif kind == "const":
        r = np.where(np.arange(nb) & 1, -mx, mx)[:, None, None] * np.ones((nb, h, w), np.int64)
    elif kind == "lap":
        r = np.clip(np.rint(rng.laplace(0, mx / 6, (nb, h, w))), -mx, mx)
    elif kind == "sparse":
        r = np.zeros((nb, h, w), np.int64)
        for b in range(nb):
            for _ in range(1 + (b & 1)):
                r[b, rng.integers(h), rng.integers(w)] = \
                    (1 + rng.integers(sparse_mag)) * rng.choice(np.array([-1, 1]))
    else:
        raise ValueError(kind)
    return r.astype(np.int16)


def coeffs(kind, s, t, bd, nb, seed, sparse_mag=3):
    """int32 [nb, n]: the oracle's forward transform of residuals()."""
    n = O.max_eob(s)
    res = residuals(kind, O.TX_W[s], O.TX_H[s], bd, nb, seed, sparse_mag)
    return np.stack([O.fwd_txfm2d(r, t, s, bd)[:n] for r in res])


def quantize_fp(c, s, t, bd, qindex):
    """The oracle's av1_quant (FP) per block -> (qcoeff, dqcoeff, eob)."""
    qs, ds, es = [], [], []
    for blk in c:
        _, q, d, e = O.av1_quant_block(blk, s, t, bd, qindex, 0)
        qs.append(q)
        ds.append(d)
        es.append(e)
    return np.stack(qs), np.stack(ds), np.array(es, np.uint16)


def plane(kinds, s, bd, nbx, nby, seed, sparse_mag=3):
    """(src, pred) uint16 [nby * H, nbx * W] with src - pred = residuals() of
    kinds[block % len(kinds)] per block, blocks in raster order."""
    W, H = O.TX_W[s], O.TX_H[s]
    nb = nbx * nby
    per = {k: residuals(k, W, H, bd, nb, seed + 17 * i, sparse_mag) for i, k in enumerate(kinds)}
    res = np.zeros((nby * H, nbx * W), np.int64)
    for b in range(nb):
        by, bx = divmod(b, nbx)
        res[by * H:(by + 1) * H, bx * W:(bx + 1) * W] = per[kinds[b % len(kinds)]][b]
    pred = np.maximum(-res, 0)
    return (pred + res).astype(np.uint16), pred.astype(np.uint16)


def one_type_masks(s, nb, valid, nkinds):
    """Per-block allowed masks with exactly one type each, cycling over the
    valid types; against plane()'s kind cycle (block % nkinds) the type cycle
    advances one extra step per round of kinds, so every type meets every
    kind.  -> (masks uint16 [nb], types [nb])."""
    types = [t for t in range(16) if valid(s, t)]
    tt = np.array([types[(b // nkinds + b) % len(types)] for b in range(nb)])
    return (1 << tt).astype(np.uint16), tt


# row layouts of tests/golden/fix_txb_extremes.npz
C_FIELDS = ["set", "tx_size", "tx_type", "plane", "block", "eob", "txb_skip_ctx", "dc_sign_ctx",
            "tx_type_cost", "rate", "rate_laplacian", "crc"]
T_FIELDS = ["bd", "tx_size", "tx_type", "qindex", "plane", "is_inter", "sharpness", "rdmult",
            "kind", "seed", "sparse_mag", "txb_skip_ctx", "dc_sign_ctx", "tx_type_cost", "eob_in",
            "eob", "rate", "entropy_ctx", "n", "index"]


def trellis_conditions(T, q_in, dq_in, q_out, dq_out):
    """The counts fix_txb_extremes.npz (and any set of trellis results laid
    out like it) is judged by; T: rows of T_FIELDS, the arrays flat with T's
    n / index."""
    J = {n: i for i, n in enumerate(T_FIELDS)}
    c = dict(eob_shrinks=0, update_skip=0, eob_in_1=0, lowered_from_15=0, q255_bd12_nonzero=0)
    pairs = set()
    for r in T:
        n, i = int(r[J["n"]]), int(r[J["index"]])
        a, b = np.abs(q_in[i:i + n].astype(np.int64)), np.abs(q_out[i:i + n].astype(np.int64))
        e_in, e = int(r[J["eob_in"]]), int(r[J["eob"]])
        c["eob_shrinks"] += int(0 < e < e_in)
        # eob 0 from a nonzero eob_in is update_skip's doing alone
        c["update_skip"] += int(e == 0 and e_in > 0)
        c["eob_in_1"] += int(e_in == 1)
        c["lowered_from_15"] += int(((a >= 15) & (b < a)).sum())
        c["q255_bd12_nonzero"] += int(r[J["qindex"]] == 255 and r[J["bd"]] == 12 and
                                      np.any(dq_out[i:i + n]))
        pairs.add((tx_class(int(r[J["tx_type"]])), int(r[J["bd"]])))
    c["class_bd_pairs"] = len(pairs)
    return c


# ---------------------------------------------------------------------------
# the cases of tests/test_txb_extremes_cpu.py and tests/test_gpu_txb_extremes.py
# with their input conditions (asserted on the oracle's outputs in both)
# ---------------------------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "fix_txb_extremes.npz")


def load_fixture():
    return dict(np.load(FIXTURE))


def check_probe_sets(rates, index, s, t):
    got, want = probe_sets(rates, index), probe_expected(s, t)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    five = [k for k, v in want.items() if len(v) == 5]
    assert len(five) >= 3 and all(len(got[k]) == 5 for k in five)
    # the pad is read: some target has a neighbour outside the block
    assert any(len(v) < (3 if k == (0, 0) and tx_class(t) == 0 else 5) for k, v in want.items())
    return len(five)


def check_level_blocks(s, t):
    q, eob, names = level_blocks(s, t)
    n = O.max_eob(s)
    a = np.abs(q.astype(np.int64))
    by = dict(zip(names, range(len(names))))
    assert a[by["all127+"]].min() >= 127 and eob[by["all127+"]] == n
    for v in (3, 2, 14, 15, 16):
        assert (a[by["all%d" % v]] == v).all() and eob[by["all%d" % v]] == n
    for k in ("checker0", "checker1"):
        assert set(np.unique(a[by[k]]).tolist()) == {0, 1 << 17}
    g = a[by["golomb21"]] - 14
    assert g.max() == 1 << 20 and g.min() == (1 << 20) - 1  # Golomb lengths 21 and 20
    assert {0, 1, 2, 3, n} <= set(eob.tolist())
    assert eob[by["last_only"]] == n and (a[by["last_only"]] > 0).sum() == 1
    return q, eob, names


# (tx_size, tx_type) of the trellis runs: 16x16 of each class, 32x32, 64x64,
# 32x64, 64x16, 8x32 IDTX, and the sizes no other trellis test runs
TRELLIS_CASES = [(2, 0), (2, 10), (2, 11), (3, 0), (4, 0), (11, 0), (18, 0), (15, 9), (8, 0),
                 (10, 0), (12, 0), (15, 0)]
TRELLIS_TABLE_SEED = 77


def trellis_batches(s):
    """Batch sizes around the kernel's blocks per wave (64; 32 at n = 1024):
    one block, a partial wave, a wave and one, two waves and two."""
    return (1, 33, 65) if O.max_eob(s) == 1024 else (1, 63, 65, 130)


def _trellis_run(s, t, bd, qindex, rdmult, kind, nb, seed, mag=3, sharp=0, plane=0, inter=1):
    blob = tables(TRELLIS_TABLE_SEED)
    c = coeffs(kind, s, t, bd, nb, seed, mag)
    q_in, dq_in, eob_in = quantize_fp(c, s, t, bd, qindex)
    rng = np.random.default_rng(seed + 1)
    ctx = np.stack([rng.integers(0, 13, nb), rng.integers(0, 3, nb)], 1).astype(np.int32)
    dqv = O.quant_arrays(O.build_quant(bd, qindex))["dequant"]
    ttc = 321
    res = [O.optimize_b(blob, c[b], q_in[b], dq_in[b], int(eob_in[b]), plane, s, t, bd, inter,
                        rdmult, sharp, dqv, int(ctx[b, 0]), int(ctx[b, 1]), ttc) for b in range(nb)]
    return dict(s=s, t=t, bd=bd, qindex=qindex, rdmult=rdmult, kind=kind, nb=nb, sharp=sharp,
                plane=plane, inter=inter, ttc=ttc, dqv=dqv, ctx=ctx, c=c, q_in=q_in, dq_in=dq_in,
                eob_in=eob_in, eob=np.array([r[0] for r in res], np.uint16),
                rate=np.array([r[1] for r in res], np.int32),
                entropy=np.array([r[2] for r in res], np.uint8),
                q=np.stack([r[3] for r in res]), dq=np.stack([r[4] for r in res]))


@functools.lru_cache(maxsize=2)
def trellis_group(s, t):
    """bd 12 x qindex {0, 255} x rdmult {60000, 2^20} x the four kinds, the
    batch sizes of trellis_batches() in turn, with the oracle's results."""
    runs = []
    bs = trellis_batches(s)
    k = 0
    for qindex in (0, 255):
        for rdmult in (60000, 1 << 20):
            for kind in KINDS:
                nb = bs[(k + k // len(bs)) % len(bs)]
                runs.append(_trellis_run(s, t, 12, qindex, rdmult, kind, nb,
                                         500 + 16 * s + t + 7 * k))
                k += 1
    return runs


def check_trellis_group(runs, s, t):
    """At qindex 0, over the group: some block shortens its eob, some
    coefficient that started at level >= 15 is lowered, the densest block has
    at least 0.9 of its coefficients at level >= 15; every batch size ran."""
    short = low15 = changed = blocks = 0
    dens = 0.0
    for r in runs:
        if r["qindex"] != 0:
            continue
        a, b = np.abs(r["q_in"].astype(np.int64)), np.abs(r["q"].astype(np.int64))
        short += int(((r["eob"] > 0) & (r["eob"] < r["eob_in"])).sum())
        low15 += int(((a >= 15) & (b < a)).sum())
        changed += int((a != b).any(1).sum())
        blocks += r["nb"]
        dens = max(dens, float((a >= 15).mean(1).max()))
    assert short > 0 and low15 > 0 and dens >= 0.9, (s, t, short, low15, dens)
    assert {r["nb"] for r in runs} == set(trellis_batches(s))
    assert any(np.any(r["dq"]) for r in runs if r["qindex"] == 255)
    return dict(shortened=short, lowered_from_15=low15, densest=dens, changed=changed,
                blocks=blocks)


SPARSE_POINT = {8: (0, 3), 10: (0, 3), 12: (0, 3)}  # (qindex, magnitude) per bit depth


@functools.lru_cache(maxsize=4)
def sparse_group(bd):
    """The sparse kind where update_skip decides: a low qindex, sharpness 0
    and a high rdmult."""
    qindex, mag = SPARSE_POINT[bd]
    return [_trellis_run(s, t, bd, qindex, 1 << 20, "sparse", 65, 900 + bd + s, mag)
            for s, t in ((2, 0), (0, 11), (3, 0))]


def check_sparse_group(runs):
    skipped = sum(int(((r["eob"] == 0) & (r["eob_in"] > 0)).sum()) for r in runs)
    eob1 = sum(int((r["eob_in"] == 1).sum()) for r in runs)
    assert skipped > 0
    return dict(update_skip=skipped, eob_in_1=eob1)


# C4 with the coefficient rate: 4x4, 16x16, 4x16, 16x4, 8x8, 32x32, 64x64
RDO_SIZES = (0, 2, 13, 14, 1, 3, 4)
RDO_MID_QINDEX = {8: 100, 10: 140, 12: 140}
# 64x64 at 8 bits: about one saturated block in fifty has no level below 3
# (1024 coefficients, levels of a few hundred); this plane seed has one
RDO_SEED_SHIFT = {(4, 8, "q0"): 10000}


def rdo_tile(s):
    """Blocks per wave tile of the C4 decision kernel."""
    return 64 // min(O.TX_W[s], O.TX_H[s])


# planes of at least 2048 wave tiles, where the decision kernel leaves its
# split form (several waves per tile) for one wave per tile: (size, bd) ->
# blocks across, down
RDO_BIG = {(0, 12): (257, 129), (2, 8): (91, 91)}


def rdo_case(s, bd, which, big=False):
    """One plane: "q0" -- the saturated and Laplacian kinds at qindex 0;
    "mid" -- all four kinds at the middle qindex.  9 x 7 blocks (5 x 3 at
    32x32, 3 x 2 at 64x64; big: RDO_BIG): more than one wave tile, the last
    one partial.  Each block is allowed exactly one type."""
    nbx, nby = RDO_BIG[(s, bd)] if big else {3: (5, 3), 4: (3, 2)}.get(s, (9, 7))
    kinds = ("sat", "lap") if which == "q0" else KINDS
    qindex = 0 if which == "q0" else RDO_MID_QINDEX[bd]
    seed = 3000 + 100 * s + bd + (which == "mid") + RDO_SEED_SHIFT.get((s, bd, which), 0)
    src, pred = plane(kinds, s, bd, nbx, nby, seed)
    nb = nbx * nby
    masks, types = one_type_masks(s, nb, O.type_valid, len(kinds))
    rng = np.random.default_rng(seed)
    ctx = np.stack([rng.integers(0, 13, nb), rng.integers(0, 3, nb)], 1).astype(np.int32)
    ttc = rng.integers(0, 3000, 16).astype(np.int32)
    tmask = sum(1 << t for t in range(16) if O.type_valid(s, t))
    assert not big or -(-nb // rdo_tile(s)) >= 2048
    return dict(s=s, bd=bd, which=which, qindex=qindex, src=src, pred=pred, nb=nb, masks=masks,
                types=types, ctx=ctx, ttc=ttc, tmask=tmask, blob=tables(seed), rdmult=1500)


def rdo_oracle(case):
    return O.rdo_plane_rate(case["src"], case["pred"], case["s"], case["tmask"], case["bd"],
                            O.build_quant(case["bd"], case["qindex"]), case["rdmult"], case["blob"],
                            case["ctx"], case["ttc"], case["masks"], None, threads=8)


def check_rdo_case(case, exp, eq):
    s, nb = case["s"], case["nb"]
    a = np.abs(eq.astype(np.int64))
    np.testing.assert_array_equal(exp["best_type"], case["types"])
    P = rdo_tile(s)
    assert nb > P and (P == 1 or nb % P), (nb, P)
    out = dict(share15=float((a >= 15).mean()), max_level=int(a.max()))
    if case["which"] == "q0":
        assert out["share15"] >= 0.9, out
        # every neighbour of every coefficient >= 3: each nibble sum is 15
        out["all_ge3_blocks"] = int((a.min(1) >= 3).sum())
        assert out["all_ge3_blocks"] > 0, out
    else:
        have = set(np.unique(a).tolist())
        assert {1, 2, 3, 4, 14, 15, 16} <= have, sorted(have)[:20]
    return out


# lavish_cost_coeffs_txb_batch caps its grid at 2048 workgroups; a workgroup
# takes 4 waves x (64 / min(n / 4, 64)) blocks per pass, so a second pass
# starts at block 2048 * 64 = 131072 for n = 16 and at 2048 * 4 = 8192 for
# n >= 256.  The counts below end in a partial second pass.
GRID_CAP = 2048
STRIDE_CASES = [(0, 131072 + 70), (2, 8192 + 5), (3, 8192 + 3)]


def stride_blocks(s, nb):
    """-> (qcoeff, eob, txb_ctx) of DCT_DCT blocks laid out so that a
    workgroup slot's first-pass block is dense (all 127, eob n) and its
    second-pass block sparse (eob <= 3), or the reverse: a level-map byte
    left from the pass before would change a rate."""
    n = O.max_eob(s)
    per_pass = GRID_CAP * 4 * (64 // min(n // 4, 64))
    assert per_pass < nb < 2 * per_pass
    scan = O.scan(s, 0)
    rng = np.random.default_rng(s)
    b = np.arange(nb)
    dense = ((b // per_pass + b) & 1) == 0
    q = np.zeros((nb, n), np.int32)
    q[dense] = 127 * rng.choice(np.array([-1, 1], np.int32), (int(dense.sum()), n))
    eob = np.where(dense, n, 1 + b % 3).astype(np.uint16)
    for e in (1, 2, 3):
        m = ~dense & (eob == e)
        q[np.ix_(m, scan[:e])] = (np.array([9, -2, 1], np.int32)[:e])[None, ::-1]
    second = b[b >= per_pass]
    assert (dense[second] != dense[second - per_pass]).all()  # every slot changes kind
    assert (np.abs(q[dense]) == 127).all() and (np.count_nonzero(q[~dense], 1) == eob[~dense]).all()
    return q, eob, np.stack([b % 13, b % 3], 1).astype(np.int32)
