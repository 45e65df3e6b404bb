"""numpy restatement of the chroma-from-luma layer (av1/common/cfl.c and the
fast leg of cfl_pick_plane_parameter, av1/encoder/intra_mode_search.c:569-643)
for the CfL tests.  The per-candidate transform and SATD are the oracle's
(_oracle.fwd_txfm2d, np.abs().sum()).
"""
import numpy as np

TX_W = [4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64]
TX_H = [4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16]
CFL_TX = [t for t in range(19) if TX_W[t] <= 32 and TX_H[t] <= 32]
LINE, SQUARE, MAGS, ZERO = 32, 1024, 33, 16
CFL_SIGN_ZERO, CFL_SIGN_NEG, CFL_SIGN_POS, CFL_SIGNS = 0, 1, 2, 3


def tx_of(w, h):
    return [t for t in range(19) if (TX_W[t], TX_H[t]) == (w, h)][0]


# ----------------------------------------------------------------- cfl.c --
def subsample(luma, sub_x, sub_y):
    """cfl_luma_subsampling_{420,422,444}_*_c on an [h, w] luma block: the q3
    block of (h >> sub_y) x (w >> sub_x)."""
    assert (sub_x, sub_y) != (0, 1)
    a = np.asarray(luma, np.int64)
    if sub_x and sub_y:
        return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) << 1
    if sub_x:
        return (a[:, 0::2] + a[:, 1::2]) << 2
    return a << 3


def pad(q3, w, h):
    """cfl_pad: the stored block to w x h, last column over the stored rows,
    then the last row over the full width."""
    q3 = np.asarray(q3, np.int64)
    sh, sw = q3.shape
    assert sw <= w and sh <= h
    out = np.zeros((h, w), np.int64)
    out[:sh, :sw] = q3
    out[:sh, sw:] = q3[:, sw - 1:sw]
    out[sh:, :] = out[sh - 1:sh, :]
    return out


def subtract_average(q3):
    """subtract_average_c with CFL_SUB_AVG_X's round_offset (half the pixel
    count) and num_pel_log2."""
    q3 = np.asarray(q3, np.int64)
    n = q3.size
    avg = (int(q3.sum()) + (n >> 1)) >> (n.bit_length() - 1)
    return q3 - avg


def ac_block(luma, sub_x, sub_y, tx_size):
    """cfl_store + cfl_compute_parameters: the W x H block of ac_buf_q3."""
    return subtract_average(pad(subsample(luma, sub_x, sub_y), TX_W[tx_size], TX_H[tx_size]))


def scaled_luma_q0(alpha_q3, ac):
    v = alpha_q3 * np.asarray(ac, np.int64)
    return np.where(v < 0, -((-v + 32) >> 6), (v + 32) >> 6)


def predict(ac, dc, alpha_q3, bd):
    """cfl_predict_{lbd,hbd}_c on a W x H block: dc holds the DC prediction."""
    return np.clip(np.asarray(dc, np.int64) + scaled_luma_q0(alpha_q3, ac), 0, (1 << bd) - 1)


# ------------------------------------------------------------- the search --
def idx_to_sign_and_alpha(idx):
    lin = idx - ZERO
    if lin == 0:
        return CFL_SIGN_ZERO, 0
    return (CFL_SIGN_POS if lin > 0 else CFL_SIGN_NEG), abs(lin) - 1


def idx_to_alpha_q3(idx):
    """cfl_idx_to_sign_and_alpha composed with cfl_idx_to_alpha."""
    sign, a = idx_to_sign_and_alpha(idx)
    return 0 if sign == CFL_SIGN_ZERO else a + 1 if sign == CFL_SIGN_POS else -a - 1


def joint(est_u, est_v):
    """(valid, cfl_alpha_idx, cfl_alpha_signs) of intra_mode_search.c:740-752."""
    if est_u == ZERO and est_v == ZERO:
        return 0, 0, 0
    su, au = idx_to_sign_and_alpha(est_u)
    sv, av = idx_to_sign_and_alpha(est_v)
    return 1, (au << 4) + av, su * CFL_SIGNS + sv - 1


def cost(ac, src, dc, idx, tx_size, bd):
    """cfl_compute_rd's fast mode: aom_satd of the DCT_DCT of src - prediction."""
    import _oracle as O
    res = np.asarray(src, np.int64) - predict(ac, dc, idx_to_alpha_q3(idx), bd)
    return int(np.abs(O.fwd_txfm2d(res.astype(np.int16), 0, tx_size, bd).astype(np.int64)).sum())


def all_costs(ac, src, dc, tx_size, bd):
    return np.array([cost(ac, src, dc, i, tx_size, bd) for i in range(MAGS)], np.int64)


def walk(costs, restart=False):
    """cfl_pick_plane_parameter's walk over evaluated costs: (estimate, mask of
    the indices it looked at).  restart: the variant that resets `best` to
    cost[16] for the downward leg (what the reference does not do)."""
    best, est = costs[ZERO], ZERO
    seen = np.zeros(MAGS, bool)
    seen[ZERO] = True
    for d in (1, -1):
        if restart and d == -1:
            best = costs[ZERO]
        for i in range(1, MAGS):
            k = ZERO + d * i
            if k < 0 or k >= MAGS:
                break
            seen[k] = True
            if costs[k] < best:
                best, est = costs[k], k
            else:
                break
    return est, seen


def search(ac, src, dc, tx_size, bd):
    c = all_costs(ac, src, dc, tx_size, bd)
    return c, walk(c)[0]


# ---------------------------------------------------------- seeded inputs --
def smooth_luma(rng, lw, lh, bd):
    """a luma block with a gradient and mild noise, inside the depth's range"""
    maxv = (1 << bd) - 1
    y, x = np.mgrid[0:lh, 0:lw]
    g = rng.integers(-8, 9) * x + rng.integers(-8, 9) * y
    a = maxv // 2 + g * (maxv // 256 + 1) // 2 + rng.integers(-3, 4, (lh, lw))
    return np.clip(a, 0, maxv).astype(np.int64)


def planted_chroma(rng, ac, alpha_q3, bd, noise=1):
    """(src, dc) whose best alpha is near alpha_q3: a flat DC block plus the
    scaled AC plus noise"""
    maxv = (1 << bd) - 1
    dcv = int(rng.integers(maxv // 4, 3 * maxv // 4))
    dc = np.full(ac.shape, dcv, np.int64)
    src = np.clip(dc + scaled_luma_q0(alpha_q3, ac) + rng.integers(-noise, noise + 1, ac.shape),
                  0, maxv)
    return src.astype(np.int64), dc


# Seeds of walk_block() found by a seeded search with all_costs() / walk():
# nearly flat luma makes many alphas predict the same pixels, so costs tie and
# the walk stops short of the minimum; in the last four both neighbours of
# index 16 cost less than it and the downward leg loses only because `best` is
# carried over from the upward one (about 1 in 1500 blocks).
WALK_SEEDS_TIES = [0, 1, 2, 11, 12, 13, 22, 23, 24, 33, 34, 35, 36, 44, 45, 46, 55, 56, 57, 58, 66,
                   67, 68, 77]
WALK_SEEDS_CARRIED_BEST = [3457, 4766, 4997, 5118]


def walk_block(seed):
    """(tx_size, luma, src, dc) of an 8-bit 4:4:4 block of 4x4 .. 8x8: luma 128
    with noise of +-(1 + seed % 11), chroma 100 with noise of +-1"""
    rng = np.random.default_rng(seed)
    tx = (0, 5, 6, 1)[seed % 4]
    w, h = TX_W[tx], TX_H[tx]
    amp = 1 + seed % 11
    luma = 128 + rng.integers(-amp, amp + 1, (h, w))
    dc = np.full((h, w), 100)
    src = np.clip(dc + rng.integers(-1, 2, (h, w)), 0, 255)
    return tx, luma.astype(np.int64), src.astype(np.int64), dc.astype(np.int64)


# ------------------------------------------------- fix_cfl.npz's layout ----
SUBS = [(1, 1), (1, 0), (0, 0)]
GETTERS = ["cfl_get_subtract_average_fn"] + \
    ["cfl_get_luma_subsampling_%d_%s" % (s, b) for s in (420, 422, 444) for b in ("lbd", "hbd")] + \
    ["cfl_get_predict_lbd_fn", "cfl_get_predict_hbd_fn"]
G_COLS = ("getter", "tx_size", "bd", "alpha_q3", "in_pos", "in2_pos", "out_pos")
B_COLS = ("bd", "hbd", "sub_x", "sub_y", "tx_size", "luma_w", "luma_h", "plane", "alpha_q3",
          "luma_pos", "dc_pos", "ac_pos", "pred_pos")
S_COLS = ("bd", "hbd", "sub_x", "sub_y", "tx_size", "luma_w", "luma_h", "plane", "est", "luma_pos",
          "src_pos", "dc_pos", "ac_pos", "cost_pos")


def luma_block_ok(w, h):
    """is w x h a luma block CfL can have (a block size up to 32x32)?"""
    return w <= 32 and h <= 32 and max(w, h) <= 4 * min(w, h)


def getter_kind(g):
    return "subtract_average" if "subtract" in g else "subsample" if "subsampling" in g else \
        "predict_lbd" if "lbd" in g else "predict_hbd"


def getter_sub(g):
    return {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[g.split("_")[4]]


class Row:
    pass


def _take(F, pos, h, w):
    return F["data"][pos:pos + h * w].astype(np.int64).reshape(h, w)


def getter_row(F, row):
    g = Row()
    v = dict(zip(G_COLS, (int(x) for x in row)))
    g.getter, g.tx, g.bd, g.alpha_q3 = GETTERS[v["getter"]], v["tx_size"], v["bd"], v["alpha_q3"]
    g.kind = getter_kind(g.getter)
    w, h = TX_W[g.tx], TX_H[g.tx]
    a = _take(F, v["in_pos"], h, w)
    if g.kind == "subsample":
        sx, sy = getter_sub(g.getter)
        g.inputs, g.out = a, _take(F, v["out_pos"], h >> sy, w >> sx)
    elif g.kind == "subtract_average":
        g.inputs, g.out = a, _take(F, v["out_pos"], h, w)
    else:
        g.inputs, g.out = (a, _take(F, v["in2_pos"], h, w), g.alpha_q3), _take(F, v["out_pos"], h, w)
    return g


def getter_expected(g):
    """the restatement's answer to a getter row"""
    if g.kind == "subsample":
        return subsample(g.inputs, *getter_sub(g.getter))
    if g.kind == "subtract_average":
        return subtract_average(g.inputs)
    return predict(g.inputs[0], g.inputs[1], g.inputs[2], g.bd)


def _xd_row(F, row, cols):
    r = Row()
    v = dict(zip(cols, (int(x) for x in row)))
    r.bd, r.hbd, r.sub, r.tx, r.plane = v["bd"], v["hbd"], (v["sub_x"], v["sub_y"]), v["tx_size"], v["plane"]
    r.w, r.h = TX_W[r.tx], TX_H[r.tx]
    r.luma = _take(F, v["luma_pos"], v["luma_h"], v["luma_w"])
    r.dc = np.repeat(_take(F, v["dc_pos"], 1, r.w), r.h, axis=0)   # cfl_load_dc_pred: one row, every line
    r.ac = _take(F, v["ac_pos"], r.h, r.w)
    return r, v


def block_row(F, row):
    r, v = _xd_row(F, row, B_COLS)
    r.alpha_q3, r.src = v["alpha_q3"], r.dc
    r.pred = _take(F, v["pred_pos"], r.h, r.w)
    return r


def search_row(F, row):
    r, v = _xd_row(F, row, S_COLS)
    r.est = v["est"]
    r.src = _take(F, v["src_pos"], r.h, r.w)
    cm = F["data"][v["cost_pos"]:v["cost_pos"] + 2 * MAGS].astype(np.int64)
    r.costs, r.mask = cm[:MAGS], cm[MAGS:] > 0
    return r


def coverage_problems(F):
    """the conditions the fixture must meet, as a list of what is missing"""
    bad = []
    G = [getter_row(F, r) for r in F["getter_rows"]]
    B = [block_row(F, r) for r in F["block_rows"]]
    S = [search_row(F, r) for r in F["search_rows"]]
    depth = lambda r: (r.bd, getattr(r, "hbd", int(r.bd > 8)))  # noqa: E731
    for fam, rows in (("subtract_average", [g for g in G if g.kind == "subtract_average"]),
                      ("subsample", [g for g in G if g.kind == "subsample"]),
                      ("predict", [g for g in G if g.kind.startswith("predict")]),
                      ("block", B), ("search", S)):
        have = {(r.tx, r.bd) for r in rows}
        miss = [(t, b) for t in CFL_TX for b in (8, 10, 12) if (t, b) not in have]
        if miss:
            bad.append("%s rows lack (tx, bd) %s" % (fam, miss[:6]))
    if not any(g.kind == "subsample" and g.bd == 8 and g.getter.endswith("lbd") for g in G) or \
            not any(depth(r) == (8, 0) for r in B) or not any(depth(r) == (8, 0) for r in S):
        bad.append("no 8-bit u8 rows")
    for fam, rows in (("block", B), ("search", S)):
        if {r.sub for r in rows} != set(SUBS):
            bad.append("%s rows lack a subsampling" % fam)
    if {getter_sub(g.getter) for g in G if g.kind == "subsample"} != set(SUBS):
        bad.append("getter rows lack a subsampling")
    if not any(r.bd == 12 and r.luma.size == 1024 and (r.luma == 4095).all() and r.sub == (0, 0)
               for r in B):
        bad.append("no all-maximum 32x32 luma at 12 bits")
    for bd in (8, 10, 12):
        preds = [r.pred for r in B if r.bd == bd] + [g.out for g in G if g.kind.startswith("predict")
                                                     and g.bd == bd]
        raw = [r.dc + scaled_luma_q0(r.alpha_q3, r.ac) for r in B if r.bd == bd] + \
              [g.inputs[1] + scaled_luma_q0(g.inputs[2], g.inputs[0]) for g in G
               if g.kind.startswith("predict") and g.bd == bd]
        if not any((a < 0).any() for a in raw) or not any((a > (1 << bd) - 1).any() for a in raw):
            bad.append("prediction never clips at both ends at %d bits" % bd)
        assert len(preds) == len(raw)
    ests = {r.est for r in S}
    if not {0, 16, 32} <= ests or not any(0 < e < 16 for e in ests) or not any(16 < e < 32 for e in ests):
        bad.append("estimates %s lack 0 / 16 / 32 or a sign away from the ends" % sorted(ests))
    n_argmin = n_equal = n_carried = 0
    for r in S:
        c = all_costs(r.ac, r.src, r.dc, r.tx, r.bd)
        e, seen = walk(c)
        n_argmin += e != int(np.argmin(c))
        ends = [k for k in (max(np.flatnonzero(seen)), min(np.flatnonzero(seen))) if k != e]
        n_equal += any(c[k] == c[e] for k in ends)
        n_carried += bool(c[15] < c[16] and c[17] < c[16] and walk(c, restart=True)[0] != e)
    if n_argmin < 20:
        bad.append("only %d rows whose walk is not the argmin" % n_argmin)
    if n_equal < 20:
        bad.append("only %d rows that stop on an equal cost" % n_equal)
    if n_carried < 2:
        bad.append("only %d rows where a restarted best would differ" % n_carried)
    return bad
