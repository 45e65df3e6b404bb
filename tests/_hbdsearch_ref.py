"""numpy restatement of the high-bit-depth single-reference motion searches
(av1_full_pixel_search :1755-1873 of DIAMOND / NSTEP / NSTEP_8PT and
av1_find_best_sub_pixel_tree / _pruned / _pruned_more of av1/encoder/mcomp.c
with the members highbd_set_var_fns binds, av1/encoder/encoder_utils.h) -- and
the reader of tests/golden/fix_mcomp_hbd.npz.

The walks are not restated here: the full-pel search is
_compsearch_ref's comp_full_pixel_search (form PLAIN) over an Env whose SAD is
the _bitsN wrapper's -- (aom_highbd_sad or aom_highbd_sad_skip of the whole
block) >> (bd - 8), as MAKE_BFP_SAD_WRAPPER / MAKE_SDSF_SKIP_SAD_WRAPPER
write it -- and whose variance is _pixref.variance at the depth; the sub-pel
search is _compsubpel_ref's search over an Env whose error is
_pixref.sub_pixel_variance(..., highbd=True).  Added here: the
downsampled-SAD recheck (:1840-1873), calc_int_sad_list (:789-841) and the
cost list's first step of the pruned sub-pel methods (:2907-3126), which the
compound searches never take -- with the quarter / eighth-pel levels that
follow it (_finer: _compsubpel_ref.search has no entry after the half-pel
step).

test_mcomp_hbd_cpu.py pins every function here to the fixture (the
reference's own results); the GPU tests then use them at the sizes the
fixture cannot reach.
"""
import collections
import os

import numpy as np

import _compsearch_ref as S
import _compsubpel_ref as P
import _mvextremes as X
import _pixref as PX

INT_MAX = 0x7FFFFFFF
DIAMOND, NSTEP, NSTEP_8PT = S.DIAMOND, S.NSTEP, S.NSTEP_8PT
TREE, PRUNED, PRUNED_MORE = P.TREE, P.PRUNED, P.PRUNED_MORE
FULL_FIELDS = ["best_row", "best_col", "bestsme", "steps", "searches"]
SUB_FIELDS = P.RESULT_FIELDS


# ----------------------------------------------------------------- full pel --
class FullEnv(S.Env):
    """One full-pel job over flat uint16 planes at bit depth bd; skip: the
    search's sdf is the downsampled one (blocks at least 16 high)."""

    def __init__(self, src, ref, stride, bw, bh, job, cost, bd, skip=False):
        S.Env.__init__(self, src, ref, stride, bw, bh, job, cost, S.PLAIN)
        self.bd, self.skip = bd, bool(skip) and bh >= 16
        self.start = (int(job["start_row"]), int(job["start_col"]))
        self.runs = 0

    def raw_sad(self, r, c, skip):
        """(aom_highbd_sad, or aom_highbd_sad_skip: 2 x the even rows')."""
        b = self.block(r, c)
        return int(PX.sad_skip(self.src, b) if skip else PX.sad(self.src, b))

    def wrapped(self, r, c, skip, per_row=False):
        """The _bitsN wrapper: the block's SAD shifted.  per_row: what a
        kernel that shifted each row's SAD before adding them would give
        (only to show that the difference matters)."""
        sh = self.bd - 8
        if per_row:
            d = np.abs(self.src - self.block(r, c)).sum(axis=1)
            return int((2 * (d[::2] >> sh).sum()) if skip else (d >> sh).sum())
        return self.raw_sad(r, c, skip) >> sh

    def sad(self, r, c):
        key = (r, c, self.skip)
        if key not in self.memo:
            self.memo[key] = self.wrapped(r, c, self.skip, getattr(self, "per_row", False))
        return self.memo[key]

    def var(self, r, c):
        return int(PX.variance(self.src, self.block(r, c), self.bd)[0])

    def var_cost(self, r, c):
        self.runs += 1                      # one get_mvpred_var_cost per run
        return S.Env.var_cost(self, r, c)


def int_sad_list(e, br, bc):
    """calc_int_sad_list: centre, left, bottom, right, top."""
    out = []
    for dr, dc in ((0, 0), (0, -1), (1, 0), (0, 1), (-1, 0)):
        r, c = br + dr, bc + dc
        out.append(e.sad(r, c) + e.mvsad(r, c) if e.in_range(r, c) else INT_MAX)
    return out


def recheck(e, br, bc):
    """The quality check of a downsampled search (mcomp.c:1854-1862) on the
    wrapped SADs: True when the search is redone with the full SAD."""
    sad, skip_sad = e.wrapped(br, bc, False), e.wrapped(br, bc, True)
    thresh = (e.bw >> 2) * (e.bh >> 2)
    return sad > thresh and abs(skip_sad - sad) * 10 >= max(sad, 1) * 9


def full_pixel_search(e, method, step_param, trace=None):
    """av1_full_pixel_search of job `e`: (result dict over FULL_FIELDS, cost
    list).  steps / searches accumulate over a redone search, as the device
    counts them.  trace: receives `redo`."""
    res = S.comp_full_pixel_search(e, method, step_param)
    steps = res["steps"]
    redo = e.skip and recheck(e, res["best_row"], res["best_col"])
    if redo:
        e.skip = False
        res = S.comp_full_pixel_search(e, method, step_param)
        steps += res["steps"]
    if trace is not None:
        trace["redo"] = redo
    out = dict(best_row=res["best_row"], best_col=res["best_col"], bestsme=res["bestsme"],
               steps=steps, searches=e.runs)
    return out, int_sad_list(e, res["best_row"], res["best_col"])


def run_fullpel(src, ref, stride, bw, bh, jobs, cost, bd, method=DIAMOND, step_param=0, skip=False):
    """The restatement over JOB_DTYPE records and flat uint16 planes:
    ([n, 5] int64 over FULL_FIELDS, [n, 5] cost lists)."""
    rows, cls = [], []
    for jb in jobs:
        r, cl = full_pixel_search(FullEnv(src, ref, stride, bw, bh, jb, cost, bd, skip), method,
                                  step_param)
        rows.append([r[f] for f in FULL_FIELDS])
        cls.append(cl)
    return np.array(rows, np.int64).reshape(-1, 5), np.array(cls, np.int64).reshape(-1, 5)


# ------------------------------------------------------------------ sub pel --
class SubEnv(P.Env):
    """One sub-pel job over flat uint16 planes at bit depth bd."""

    def __init__(self, src, ref, stride, bw, bh, job, cost, bd):
        P.Env.__init__(self, src, ref, stride, bw, bh, job, cost, P.PLAIN)
        self.bd = bd
        self.win = np.arange(bh + 1)[:, None] * stride + np.arange(bw + 1)[None, :]

    def err(self, r, c, search_type):
        """aom_highbd_{bd}_sub_pixel_variance at the 1/8-pel mv: (var, sse)."""
        off = self.ref_off + (r >> 3) * self.stride + (c >> 3)
        v, sse, _ = PX.sub_pixel_variance(self.ref[off + self.win], c & 7, r & 7, self.src,
                                          self.bd, highbd=True)
        return int(v), int(sse)


def _cdiv(a, b):
    """C's truncating division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _div_round(n, d):
    """divide_and_round (mcomp.c:2853-2855)"""
    return _cdiv(n - _cdiv(d, 2), d) if (n < 0) != (d < 0) else _cdiv(n + _cdiv(d, 2), d)


def search(e, method, forced_stop=P.EIGHTH_PEL, allow_hp=False, iters=1, start=None, cl=None,
           trace=None):
    """One sub-pel search (USE_2_TAPS_ORIG) of job `e` from `start` (default:
    the job's), cl the full-pel cost list or None: a result dict (SUB_FIELDS).
    Without a usable cost list this is _compsubpel_ref.search; with one, the
    pruned methods' first step comes from it."""
    start = e.start if start is None else start
    usable = (cl is not None and method != TREE and forced_stop != P.FULL_PEL and
              all(int(v) != INT_MAX for v in cl))
    if usable and method == PRUNED_MORE:
        usable = all(cl[0] < cl[i] for i in range(1, 5))    # is_cost_list_wellbehaved
    if not usable:
        return P.search(e, method, P.USE_2_TAPS_ORIG, forced_stop, allow_hp, iters, start,
                        trace=trace)
    tr = trace if trace is not None else {}
    tr.update(oob=0, second_level=0)
    var, sse = e.err(start[0], start[1], 0)
    b = dict(best_row=start[0], best_col=start[1], distortion=var, sse=sse,
             besterr=(var + e.mv_err_cost(*start)) & P.M32)

    def check(r, c):
        if not e.in_range(r, c):
            tr["oob"] += 1
            return INT_MAX
        var, sse = e.err(r, c, 0)
        cost = (e.mv_err_cost(r, c) + var) & P.M32
        if cost < b["besterr"]:
            b.update(best_row=r, best_col=c, besterr=cost, distortion=var, sse=sse)
        return cost

    cl = [int(v) for v in cl]
    if method == PRUNED_MORE:       # get_cost_surf_min
        ic = _div_round(cl[1] - cl[3], cl[1] - 2 * cl[0] + cl[3])
        ir = _div_round(cl[4] - cl[2], cl[4] - 2 * cl[0] + cl[2])
        if ir or ic:
            check(start[0] + ir * 4, start[1] + ic * 4)
    else:                           # whichdir: the quadrant of the cheaper sides
        dc = -4 if cl[1] < cl[3] else 4
        dr = 4 if cl[2] < cl[4] else -4
        check(start[0], start[1] + dc)
        check(start[0] + dr, start[1])
        check(start[0] + dr, start[1] + dc)
    # the finer levels from the best so far (_compsubpel_ref.search offers no
    # entry after the half-pel step)
    _finer(e, b, check, forced_stop, allow_hp, iters)
    return b


def _finer(e, b, check, forced_stop, allow_hp, iters):
    """two_level_checks_fast (mcomp.c:2675) at quarter and eighth pel."""
    def level(h):
        tr_, tc = b["best_row"], b["best_col"]
        left, right = check(tr_, tc - h), check(tr_, tc + h)
        up, down = check(tr_ - h, tc), check(tr_ + h, tc)
        dr, dc = (-h if up <= down else h), (-h if left <= right else h)
        check(tr_ + dr, tc + dc)
        if iters <= 1:
            return
        br, bc = b["best_row"], b["best_col"]
        if tr_ != br and tc != bc:
            check(br, bc + dc)
            check(br + dr, bc)
        elif tr_ == br and tc != bc:
            check(br + h, bc + dc)
            check(br - h, bc + dc)
            check(br - dr, bc)
        elif tr_ != br and tc == bc:
            check(br + dr, bc + h)
            check(br + dr, bc - h)
            check(br, bc - dc)
    if forced_stop < P.HALF_PEL:
        level(2)
    if allow_hp and forced_stop == P.EIGHTH_PEL:
        level(1)


def run_subpel(src, ref, stride, bw, bh, jobs, cost, bd, method=PRUNED_MORE,
               forced_stop=P.EIGHTH_PEL, allow_hp=False, iters=1, fullpel=None, cost_lists=None):
    """The restatement over SUBPEL_JOB_DTYPE records: [n, 5] int64
    (SUB_FIELDS).  fullpel: [n, >= 2] best mvs (full pel) to start from."""
    out = []
    for i, jb in enumerate(jobs):
        e = SubEnv(src, ref, stride, bw, bh, jb, cost, bd)
        start = None if fullpel is None else (8 * int(fullpel[i][0]), 8 * int(fullpel[i][1]))
        r = search(e, method, forced_stop, allow_hp, iters, start,
                   None if cost_lists is None else cost_lists[i])
        out.append([r[f] for f in SUB_FIELDS])
    return np.array(out, np.int64).reshape(-1, 5)


# ------------------------------------------------------------------ content --
def _tiled(tile):
    t = tile.shape[0]
    return np.tile(tile, (X.PH // t + 1, X.PW // t + 1))[:X.PH, :X.PW]


def scaled(kind, bd, bw=16, bh=16, seed=5):
    """_mvextremes' planes of a kind scaled to the depth with the low bd - 8
    bits filled from seeded 16 x 16 tiles (one per plane), so that per-row
    partial SADs are no multiples of 4 / 16: (src [PH, PW], refs [NREF, PH,
    PW]) uint16.  Flat 0 / 255 content keeps its extremes: 0 stays 0 and 255
    becomes the depth's maximum."""
    s, r = X.planes(kind, bw, bh)
    sh = bd - 8
    if sh == 0:
        return s.astype(np.uint16), r.astype(np.uint16)
    rng = np.random.default_rng(seed + bd)

    def up(a):
        a = a.astype(np.int64)
        if kind.startswith("flat_") and kind != "flat_128_128":
            return np.where(a == 255, (1 << bd) - 1, 0).astype(np.uint16)
        return ((a << sh) | _tiled(rng.integers(0, 1 << sh, (16, 16)))).astype(np.uint16)
    return up(s), np.stack([up(p) for p in r])


def negclamp(bd, bw, bh, seed=9):
    """References of a seeded 16 x 16 tile repeated and a source that is
    reference 0 plus d, plus one more in the first k pixels (raster order) of
    every bw x bh block of the frame, (d, k) = _pixref.neg_clamp_diffs: at mv
    (0, 0) the 10 / 12-bit variance is negative before its clamp."""
    d, k = PX.neg_clamp_diffs(bw, bh, bd)
    rng = np.random.default_rng(seed + bd)
    ref = _tiled(rng.integers(0, (1 << bd) - 64, (16, 16)))
    y, x = np.mgrid[0:X.PH, 0:X.PW]
    idx = ((y - X.BORDER) % bh) * bw + (x - X.BORDER) % bw
    src = ref + d + (idx < k)
    refs = np.stack([ref, np.roll(ref, (0, -1), (0, 1))][:X.NREF])
    return src.astype(np.uint16), np.ascontiguousarray(refs.astype(np.uint16))


SMOOTH_SHIFTS = [(3, -5), (-10, 13)]     # reference k matches the source at this mv (1/8 pel)


def smooth(bd, seed=991):
    """A seeded 32 x 32 tile low-passed circularly (it repeats seamlessly),
    scaled to the depth; reference k is the tile's bilinear interpolation at
    -SMOOTH_SHIFTS[k] / 8, so the block of reference k at mv SMOOTH_SHIFTS[k]
    is close to the source block: sub-pel searches move."""
    t = np.random.default_rng(seed).integers(0, 256, (32, 32)).astype(np.float64)
    for _ in range(4):
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5
    t = (t - t.min()) / (t.max() - t.min())
    fine = np.rint(t * ((1 << bd) - 1) * 64).astype(np.int64)

    def shifted(dr, dc):       # value at (y - dr / 8, x - dc / 8)
        fr, fc = (-dr) & 7, (-dc) & 7
        a = np.roll(fine, ((dr + fr) // 8, (dc + fc) // 8), (0, 1))
        a = (a * (8 - fr) + np.roll(a, -1, 0) * fr)
        a = (a * (8 - fc) + np.roll(a, -1, 1) * fc)
        return (a + 32 * 64) // (64 * 64)
    src = _tiled((fine + 32) // 64).astype(np.uint16)
    refs = np.stack([_tiled(shifted(*sft)) for sft in SMOOTH_SHIFTS]).astype(np.uint16)
    return src, refs


_planes = {}
SIZED = X.SIZED + ("negclamp",)


def planes(kind, bd, bw=16, bh=16):
    """(src, refs) uint16 of a content kind at a depth; shared, read-only."""
    key = (kind, bd) + ((bw, bh) if kind in SIZED else ())
    if key not in _planes:
        s, r = (negclamp(bd, bw, bh) if kind == "negclamp" else smooth(bd) if kind == "smooth"
                else scaled(kind, bd, bw, bh))
        s.setflags(write=False)
        r.setflags(write=False)
        _planes[key] = (s, r)
    return _planes[key]


def plane_key(kind, bd, bw, bh):
    """The name a fixture stores a plane set under."""
    return "%s_bd%d" % (kind, bd) + ("_%dx%d" % (bw, bh) if kind in SIZED else "")


# ------------------------------------------------------------------ fixture --
CASE_FIELDS = ["bd", "bw", "bh", "method", "step_param", "cost", "error_per_bit", "sad_per_bit",
               "hp_tables", "skip", "use_cl", "sp_method", "sp_forced_stop", "sp_allow_hp",
               "sp_iters", "sp_use_cl", "plane"]
ROW_FIELDS = (["case"] + X.JOB_FIELDS + ["best_row", "best_col", "bestsme", "steps", "searches",
                                          "cl0", "cl1", "cl2", "cl3", "cl4"] +
              ["sp_" + f for f in ("col_min", "col_max", "row_min", "row_max")] +
              ["sp_" + f for f in SUB_FIELDS])
Group = collections.namedtuple("Group", "index prm plane jobs sjobs rows J")


def load_fixture():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "fix_mcomp_hbd.npz")))


def fixture_groups(F):
    """The stored cases: parameters, the plane set's name, the JOB_DTYPE and
    SUBPEL_JOB_DTYPE records (the sub-pel jobs start at the reference's
    full-pel result) and the reference's rows."""
    from lavish_dsp import motion as M
    J = {n: i for i, n in enumerate(ROW_FIELDS)}
    assert [str(s) for s in F["row_fields"]] == ROW_FIELDS
    assert [str(s) for s in F["case_fields"]] == CASE_FIELDS
    for ci, vals in enumerate(F["cases"]):
        prm = dict(zip(CASE_FIELDS, (int(v) for v in vals)))
        rows = F["rows"][F["rows"][:, 0] == ci]
        rec = np.zeros(len(rows), M.JOB_DTYPE)
        for f in X.JOB_FIELDS:
            rec[f] = rows[:, J[f]]
        sj = np.zeros(len(rows), M.SUBPEL_JOB_DTYPE)
        for f in ("src_off", "ref_off", "ref_mv_row", "ref_mv_col"):
            sj[f] = rec[f]
        for f in ("col_min", "col_max", "row_min", "row_max"):
            sj[f] = rows[:, J["sp_" + f]]
        sj["start_row"] = 8 * rows[:, J["best_row"]]
        sj["start_col"] = 8 * rows[:, J["best_col"]]
        yield Group(ci, prm, str(F["planes"][prm["plane"]]), rec, sj, rows, J)


def group_cost(prm, subpel=False):
    return S.cost_of(prm["cost"], prm["error_per_bit"], prm["sad_per_bit"],
                     prm["sp_allow_hp"] if subpel else prm["hp_tables"])


def group_planes(F, g):
    return F["src__" + g.plane].reshape(-1), F["refs__" + g.plane].reshape(-1)


def group_fullpel(F, g):
    """A group's rows through the full-pel restatement."""
    p = g.prm
    src, ref = group_planes(F, g)
    return run_fullpel(src, ref, X.STRIDE, p["bw"], p["bh"], g.jobs, group_cost(p), p["bd"],
                       p["method"], p["step_param"], p["skip"])


def group_subpel(F, g, fullpel=None):
    """A group's rows through the sub-pel restatement, from the fixture's
    full-pel results and cost lists."""
    p = g.prm
    src, ref = group_planes(F, g)
    cl = g.rows[:, g.J["cl0"]:g.J["cl4"] + 1] if p["sp_use_cl"] else None
    return run_subpel(src, ref, X.STRIDE, p["bw"], p["bh"], g.sjobs, group_cost(p, True), p["bd"],
                      p["sp_method"], p["sp_forced_stop"], bool(p["sp_allow_hp"]), p["sp_iters"],
                      cost_lists=cl)


# ----------------------------------------------------------------- coverage --
def check_coverage(F):
    """What a fixture that pins something contains, from the reference's rows
    and the planes alone; returns the counts (the generator stops unless its
    rows meet them; tests/test_mcomp_hbd_cpu.py asserts the same on the
    committed file)."""
    f = collections.Counter()
    combos = set()
    sub = collections.Counter()
    for g in fixture_groups(F):
        p, J = g.prm, g.J
        bd, bw, bh = p["bd"], p["bw"], p["bh"]
        combos.add((bd, "m", p["method"]))
        combos.add((bd, "c", p["cost"]))
        src, ref = group_planes(F, g)
        cost = group_cost(p)
        for jb, sj, row in zip(g.jobs, g.sjobs, g.rows):
            br, bc = int(row[J["best_row"]]), int(row[J["best_col"]])
            e = FullEnv(src, ref, X.STRIDE, bw, bh, jb, cost, bd, p["skip"])
            if bd > 8 and not e.skip:
                # a walk whose winner changes with the shift taken per row
                q = FullEnv(src, ref, X.STRIDE, bw, bh, jb, cost, bd, False)
                q.per_row = True
                alt = S.comp_full_pixel_search(q, p["method"], p["step_param"])
                f["per_row_differs"] += (alt["best_row"], alt["best_col"]) != (br, bc)
            if e.skip:
                # the reference kept the downsampled result iff it is what a
                # downsampled search alone finds and the recheck passes there
                only = S.comp_full_pixel_search(e, p["method"], p["step_param"])
                again = recheck(e, only["best_row"], only["best_col"])
                f["skip_redo" if again else "skip_kept"] += 1
            d = e.src - e.block(br, bc)
            sm, ss = int(d.sum()), int((d * d).sum())
            f["sum_negative"] += sm < 0
            if bd > 8:
                _, sse_r, sum_r = PX.variance_tail(sm, ss, bd, bw * bh)
                f["clamped"] += int(PX.before_clamp(sse_r, sum_r, bw * bh)) < 0
            if bd == 12 and e.src.min() == 4095 and e.block(br, bc).max() == 0:
                f["max_vs_zero"] += 1
            if bd == 12 and e.src.max() == 0 and e.block(br, bc).min() == 4095:
                f["max_vs_zero"] += 1
            # the sub-pel row
            r, c = int(row[J["sp_best_row"]]), int(row[J["sp_best_col"]])
            sub["rows"] += 1
            sub["moved"] += (r, c) != (8 * br, 8 * bc)
            low = (r | c) & 7
            sub["half"] += low == 4
            sub["quarter"] += low in (2, 6)
            sub["eighth"] += bool(low & 1)
            se = SubEnv(src, ref, X.STRIDE, bw, bh, sj, group_cost(p, True), bd)
            tr = {}
            cl = row[J["cl0"]:J["cl4"] + 1] if p["sp_use_cl"] else None
            search(se, p["sp_method"], p["sp_forced_stop"], bool(p["sp_allow_hp"]), p["sp_iters"],
                   cl=cl, trace=tr)
            sub["second_level"] += tr["second_level"] > 0
            sub["oob"] += tr["oob"] > 0
    for bd in (8, 10, 12):
        for m in (DIAMOND, NSTEP, NSTEP_8PT):
            assert (bd, "m", m) in combos, (bd, m)
        for c in (X.ENTROPY, X.L1, X.NONE):
            assert (bd, "c", c) in combos, (bd, c)
    for k in ("per_row_differs", "skip_redo", "skip_kept", "sum_negative", "clamped",
              "max_vs_zero"):
        assert f[k] > 0, (k, dict(f))
    assert 3 * sub["moved"] >= sub["rows"], dict(sub)
    for k in ("half", "quarter", "eighth", "second_level", "oob"):
        assert sub[k] > 0, (k, dict(sub))
    return dict(f), dict(sub)
