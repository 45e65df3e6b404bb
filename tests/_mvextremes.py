"""Worst-case content and jobs for the motion searches: planes on which
candidates tie exactly, difference sums saturate and the mv cost product
rate * error_per_bit passes 2^31 -- what the smooth-gradient-plus-noise planes
of lavish_dsp.synth never produce.  Plain numpy: no GPU and no oracle.

Geometry: the 160x128 frame with a 160-pixel border of fix_mcomp (padded
448 x 480), plane 0 the source, NREF references.

  planes(kind, bw, bh)                      the content kinds (KINDS)
  frame / spread / narrowed / subpel_edge_jobs   job builders over
      motion.frame_jobs / subpel_jobs: whole frames (the GPU tests compare
      these with the oracle), a few of their jobs, point / row / column
      windows, sub-pel starts on the limits
  tie_facts / saturation_facts / limit_facts / mv_rate   the facts that make
      a case non-idle (tests/test_mcomp_extremes_cpu.py asserts them)
  fixture_fullpel() / fixture_subpel(...)   the Cases (kind, block size, jobs
      and parameters of one search call; a sub-pel Case's `facts` holds its
      input cost lists) pinned from the reference in
      tests/golden/fix_mcomp_extremes.npz; fixture_groups() reads them back
"""
import collections

import numpy as np

W, H, BORDER, NREF = 160, 128, 160, 2
PW, PH = W + 2 * BORDER, H + 2 * BORDER
STRIDE, PLANE = PW, PW * PH
ENTROPY, L1, NONE = 0, 3, 4          # MV_COST_ENTROPY, MV_COST_L1_HDRES, MV_COST_NONE
INT_MAX = 0x7FFFFFFF
# the 8 sites of a DIAMOND step at radius 1 (av1_init_dsmotion_compensation)
SITES8 = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]

# (error_per_bit, ref_mv in 1/8 pel, high-precision tables): lambdas at which
# rate * error_per_bit passes 2^31 with the default tables, with sad_per_bit
# 16 (the lut's top: 0.0418 * 334 + 2.41) and a ref_mv that far from the
# block that the mvs around (0, 0) carry the rate the lambda needs.  1023
# full-pel away on both axes the rate is mvjcost[3] + 2 * mvcost = 658 +
# 2 * 17233 = 35124 with the low-precision tables and 658 + 2 * 17745 = 36148
# with the high-precision ones; 2^31 / 59650 = 36001.4, so 59650 passes 2^31
# with the hp tables alone, and only at that distance.  2^31 / 92000 =
# 23342.2 (300 full-pel: 658 + 2 * 11515 = 23688), 2^31 / 131071 = 16384.1
# (60 full-pel: 658 + 2 * 8659 = 17976).
HIGH_LAMBDA = [(59650, (8184, -8184), 1), (92000, (2400, -2400), 0),
               (131071, (484, -492), 0)]
SAD_PER_BIT_TOP = 16

Case = collections.namedtuple("Case", "name kind bw bh jobs params facts")


# ------------------------------------------------------------------ content --
def _both(src, ref=None):
    ref = src if ref is None else ref
    return np.ascontiguousarray(src, np.uint8), np.ascontiguousarray(
        np.stack([ref] * NREF), np.uint8)


def flat(v_src, v_ref):
    """Constant source and references: every site has the same SAD;
    (255, 0) the largest one, with sum^2 / N == sse."""
    return _both(np.full((PH, PW), v_src), np.full((PH, PW), v_ref))


def ramp(transpose=False):
    """v(y, x) = x >> 1 (0..239, no clipping) or its transpose: sites at +d
    and -d along the ramp tie for even d, sites across it tie with the
    centre."""
    if transpose:
        return _both(np.broadcast_to((np.arange(PH) >> 1)[:, None], (PH, PW)))
    return _both(np.broadcast_to((np.arange(PW) >> 1)[None, :], (PH, PW)))


def periodic(p, seed=7):
    """A seeded random p x p tile repeated: an exact match at every offset
    that is a multiple of p."""
    tile = np.random.default_rng(seed + p).integers(0, 256, (p, p))
    return _both(np.tile(tile, (PH // p + 1, PW // p + 1))[:PH, :PW])


def checker():
    """0 / 255 per pixel: odd offsets the largest SAD, even ones 0; every
    half-pel position averages to 127.5."""
    return _both((((np.arange(PH)[:, None] + np.arange(PW)[None, :]) & 1) * 255))


def split(bw):
    """Block columns half 255 | 0 in the source against 0 | 255 in the
    references: at mv (0, 0) the difference sum is 0 and the sse maximal."""
    x = (np.arange(PW) - BORDER) % bw < bw // 2
    s = np.broadcast_to(np.where(x, 255, 0)[None, :], (PH, PW))
    return _both(s, 255 - s)


ONE_SIDED_AT = [(5, -3), (-6, 9)]    # the exact match's mv per reference


def one_sided(bw, bh):
    """Source 255, references 0 but for one exact-match block for every other
    block of every other block row, at ONE_SIDED_AT -- off the sites of the
    first steps."""
    src = np.full((PH, PW), 255, np.uint8)
    refs = np.zeros((NREF, PH, PW), np.uint8)
    for k in range(NREF):
        dy, dx = ONE_SIDED_AT[k % len(ONE_SIDED_AT)]
        for y in range(0, H - bh + 1, 2 * bh):
            for x in range(0, W - bw + 1, 2 * bw):
                refs[k, BORDER + y + dy:BORDER + y + dy + bh,
                     BORDER + x + dx:BORDER + x + dx + bw] = 255
    return src, refs


def stripes():
    """The checker source against column stripes ((x & 1) * 255): at every mv
    the rows of one parity match and the others differ everywhere, so the full
    SAD is half the largest at every site (all tie) while the even rows' is 0
    at even columns -- the downsampled-SAD search's quality recheck fails for
    every job."""
    ref = np.broadcast_to(((np.arange(PW) & 1) * 255)[None, :], (PH, PW))
    return checker()[0], _both(ref)[1]


NOISE_AT = [(0, 0), (0, -1)]         # (one step of every method from mv (0, 0))


def noise(seed=11):
    """Seeded 0 / 255 noise, reference k the source moved by NOISE_AT[k]: one
    exact match far better than anything around it (the high-lambda content:
    the search stays where the rate is the one the parameters were set for)."""
    src = (np.random.default_rng(seed).integers(0, 2, (PH, PW)) * 255).astype(np.uint8)
    refs = np.stack([np.roll(src, NOISE_AT[k % 2], (0, 1)) for k in range(NREF)])
    return src, np.ascontiguousarray(refs)


KINDS = {
    "flat_128_128": lambda bw, bh: flat(128, 128),
    "flat_255_0": lambda bw, bh: flat(255, 0),
    "flat_0_255": lambda bw, bh: flat(0, 255),
    "ramp_x": lambda bw, bh: ramp(False),
    "ramp_y": lambda bw, bh: ramp(True),
    "periodic_2": lambda bw, bh: periodic(2),
    "periodic_8": lambda bw, bh: periodic(8),
    "periodic_16": lambda bw, bh: periodic(16),
    "checker": lambda bw, bh: checker(),
    "split": lambda bw, bh: split(bw),
    "one_sided": one_sided,
    "noise": lambda bw, bh: noise(),
    "stripes": lambda bw, bh: stripes(),
}
SIZED = ("split", "one_sided")       # kinds whose planes depend on the block size
_cache = {}


def planes(kind, bw=16, bh=16):
    """(src [PH, PW], refs [NREF, PH, PW]) of a content kind; shared, read-only."""
    key = (kind, bw, bh) if kind in SIZED else kind
    if key not in _cache:
        s, r = KINDS[kind](bw, bh)
        s.setflags(write=False)
        r.setflags(write=False)
        _cache[key] = (s, r)
    return _cache[key]


def plane_key(kind, bw, bh):
    """The name a fixture stores a kind's planes under."""
    return "%s_%dx%d" % (kind, bw, bh) if kind in SIZED else kind


# --------------------------------------------------------------------- jobs --
def frame(bw, bh, ref_mv=(0, 0), start=(0, 0)):
    """motion.frame_jobs over the frame: every block x every reference."""
    from lavish_dsp import motion as M
    return M.frame_jobs(W, H, STRIDE, BORDER, PLANE, bw, bh, NREF, ref_mv, start)


def spread(jobs, n, salt=0):
    """n jobs of a frame's: the first (a corner block), the last (the other
    corner, last reference) and a stride through the rest."""
    idx = [0, len(jobs) - 1] + [(3 + salt + 7 * i) % len(jobs) for i in range(n)]
    return jobs[sorted(set(idx[:n]))].copy()


def narrowed(jobs, mode, at=(3, -2)):
    """The jobs with a hand-set window inside their own: a single point
    ("point"), a single row ("row") or a single column ("col") through `at`
    (clamped into the window) -- mv_limits returns such windows (min == max)
    far from ref_mv."""
    j = jobs.copy()
    r = np.clip(at[0], j["row_min"], j["row_max"])
    c = np.clip(at[1], j["col_min"], j["col_max"])
    if mode in ("point", "row"):
        j["row_min"] = j["row_max"] = r
    if mode in ("point", "col"):
        j["col_min"] = j["col_max"] = c
    return j


def clamped_start(jobs):
    """(row, col) the searches start from: the start mv clamped to the window."""
    return (np.clip(jobs["start_row"], jobs["row_min"], jobs["row_max"]).astype(np.int64),
            np.clip(jobs["start_col"], jobs["col_min"], jobs["col_max"]).astype(np.int64))


SUBPEL_EDGES = ["top", "bottom", "left", "right", "top_left", "top_right", "bottom_left",
                "bottom_right"]


def subpel_edge_jobs(bw, bh, ref_mv=(0, 0)):
    """Sub-pel jobs of the frame's blocks starting on an edge or a corner of
    their SubpelMvLimits, job i on SUBPEL_EDGES[i % 8] (the other coordinate
    of an edge start is ref_mv's full-pel position)."""
    from lavish_dsp import motion as M
    fp = frame(bw, bh, ref_mv)
    zero = np.zeros(len(fp), M.RESULT_DTYPE)
    sj = M.subpel_jobs(W, H, BORDER, bw, bh, fp, zero, ref_mv)
    mid = (((ref_mv[0] + 4) >> 3) * 8, ((ref_mv[1] + 4) >> 3) * 8)
    for i in range(len(sj)):
        e = SUBPEL_EDGES[i % 8]
        sj["start_row"][i] = (sj["row_min"][i] if "top" in e else
                              sj["row_max"][i] if "bottom" in e else mid[0])
        sj["start_col"][i] = (sj["col_min"][i] if "left" in e else
                              sj["col_max"][i] if "right" in e else mid[1])
    return sj


# -------------------------------------------------------------------- facts --
def block_stats(src, refs, job, row, col, bw, bh):
    """(sad, difference sum, sse) of a job's block against its reference at a
    full-pel mv."""
    s, r = src.reshape(-1), refs.reshape(-1)
    rows = np.arange(bh)[:, None] * STRIDE + np.arange(bw)[None, :]
    so, ro = int(job["src_off"]), int(job["ref_off"]) + int(row) * STRIDE + int(col)
    assert ro >= 0 and ro + rows[-1, -1] < r.size, "mv outside the planes"
    d = s[so + rows].astype(np.int64) - r[ro + rows].astype(np.int64)
    return int(np.abs(d).sum()), int(d.sum()), int((d * d).sum())


def in_window(job, row, col):
    return (job["row_min"] <= row <= job["row_max"]) and (job["col_min"] <= col <= job["col_max"])


def mv_rate(mvjcost, mvcost, row, col, ref_mv):
    """mv_cost (mcomp.c:269-273) of a 1/8-pel mv, int64."""
    mid = (mvcost.shape[1] - 1) // 2
    dr = np.asarray(row, np.int64) - ref_mv[0]
    dc = np.asarray(col, np.int64) - ref_mv[1]
    joint = (dc != 0).astype(np.int64) | ((dr != 0).astype(np.int64) << 1)
    return (np.asarray(mvjcost, np.int64)[joint] + np.asarray(mvcost[0], np.int64)[mid + dr] +
            np.asarray(mvcost[1], np.int64)[mid + dc])


def tie_facts(kind, bw, bh, jobs):
    """The conditions of a tie kind over `jobs` (full-pel), as counts of
    (checked, violated) per fact."""
    src, refs = planes(kind, bw, bh)
    r0, c0 = clamped_start(jobs)
    facts = {}

    def note(name, ok):
        n, bad = facts.get(name, (0, 0))
        facts[name] = (n + 1, bad + (not ok))

    for jb, r, c in zip(jobs, r0, c0):
        centre = block_stats(src, refs, jb, r, c, bw, bh)[0]
        if kind.startswith("flat"):
            for d in (1, 8):
                sads = [block_stats(src, refs, jb, r + d * y, c + d * x, bw, bh)[0]
                        for y, x in SITES8]
                note("flat_sites_equal", len(set(sads)) == 1 and sads[0] == centre)
        if kind.startswith("ramp"):
            along = (1, 0) if kind == "ramp_y" else (0, 1)
            for d in range(2, 66, 2):
                p = (r + d * along[0], c + d * along[1])
                m = (r - d * along[0], c - d * along[1])
                if in_window(jb, *p) and in_window(jb, *m):
                    note("ramp_along_pairs_equal",
                         block_stats(src, refs, jb, *p, bw, bh)[0] ==
                         block_stats(src, refs, jb, *m, bw, bh)[0] > 0)
                for q in ((r + d * along[1], c + d * along[0]),
                          (r - d * along[1], c - d * along[0])):
                    if in_window(jb, *q):
                        note("ramp_across_equals_centre",
                             block_stats(src, refs, jb, *q, bw, bh)[0] == centre)
        if kind.startswith("periodic"):
            p = int(kind.split("_")[1])
            for y in range(-32, 33, p):
                for x in range(-32, 33, p):
                    if in_window(jb, y, x):
                        note("periodic_multiples_match",
                             block_stats(src, refs, jb, y, x, bw, bh)[0] == 0)
        if kind == "checker":
            for y, x in ((0, 0), (0, 1), (1, 1), (2, -1), (-3, 0), (4, 2)):
                if in_window(jb, y, x):
                    note("checker_parity",
                         block_stats(src, refs, jb, y, x, bw, bh)[0] ==
                         ((y + x) & 1) * 255 * bw * bh)
    return facts


def saturation_facts(kind, bw, bh, jobs):
    """Per job at its (clamped) start: |difference sum|^2 and the sse."""
    src, refs = planes(kind, bw, bh)
    r0, c0 = clamped_start(jobs)
    st = [block_stats(src, refs, jb, r, c, bw, bh) for jb, r, c in zip(jobs, r0, c0)]
    return {"sum_sq": [s[1] * s[1] for s in st], "sse": [s[2] for s in st]}


def limit_facts(sj):
    """Per sub-pel job: how many of the first level's four candidates (start
    +- 4 on either axis, the half-pel step) lie outside its limits."""
    out = []
    for j in sj:
        r, c = int(j["start_row"]), int(j["start_col"])
        cand = [(r, c - 4), (r, c + 4), (r - 4, c), (r + 4, c)]
        out.append(sum(not (j["row_min"] <= y <= j["row_max"] and
                            j["col_min"] <= x <= j["col_max"]) for y, x in cand))
    return out


# --------------------------------------------------- the fixture's job sets --
FP_METHODS = ["diamond", "bigdia", "fast_bigdia", "hex", "square"]
TIE_KINDS = ["flat_128_128", "flat_255_0", "flat_0_255", "ramp_x", "ramp_y", "periodic_2",
             "periodic_8", "periodic_16", "checker", "split", "one_sided"]
SMALL = [(4, 4), (8, 8), (16, 16)]
LOW_LAMBDA = (37, 4)                 # (error_per_bit, sad_per_bit) of the tie groups
P = collections.namedtuple("FullpelParams",
                           "method use_cl cost skip step_param epb spb ref_mv hp")
SP = collections.namedtuple("SubpelParams",
                            "method hp forced_stop iters cost use_cl epb ref_mv search_type")


def fixture_fullpel():
    """The full-pel groups of fix_mcomp_extremes.npz, about 300 jobs: every
    tie kind under every method (sizes, costs, the downsampled SAD, cost
    lists and step_param rotating), starts at and away from ref_mv;
    single-point / -row / -column windows; the saturated 64x64 / 128x128
    jobs; the high-lambda set."""
    cases = []
    k = 0
    for kind in TIE_KINDS:
        for mi, meth in enumerate(FP_METHODS):
            bw, bh = SMALL[k % 3]
            cost = (ENTROPY, L1, NONE, ENTROPY)[k % 4]
            ref_mv = [(0, 0), (13, -21), (-40, 33)][k % 3]
            at_ref = ((ref_mv[0] + 4) >> 3, (ref_mv[1] + 4) >> 3)
            start = at_ref if k % 2 else (at_ref[0] + 5 - k % 7, at_ref[1] - 4 + k % 5)
            if kind.startswith("ramp"):   # (the +d / -d ties are around the exact match)
                start = (0, 0)
            p = P(meth, (k >> 1) & 1, cost, int(k % 5 < 2), (0, 3, 1, 6)[(k // 3) % 4],
                  LOW_LAMBDA[0] + k % 9, LOW_LAMBDA[1], ref_mv, 0)
            jobs = spread(frame(bw, bh, ref_mv, start), 4, k)
            cases.append(Case("tie%d" % k, kind, bw, bh, jobs, p, None))
            k += 1
    for kind in ("flat_128_128", "periodic_8", "ramp_x"):
        for mode in ("point", "row", "col"):
            bw, bh = SMALL[k % 3]
            p = P(FP_METHODS[k % 5], 1, (ENTROPY, L1)[k % 2], k % 2, 0, LOW_LAMBDA[0],
                  LOW_LAMBDA[1], (13, -21), 0)
            # (a ramp's +d / -d ties are around the exact match)
            st, at = ((0, 0), (0, 0)) if kind.startswith("ramp") else ((2, -3), (3, -2))
            jobs = narrowed(spread(frame(bw, bh, (13, -21), st), 3, k), mode, at)
            cases.append(Case("%s%d" % (mode, k), kind, bw, bh, jobs, p, None))
            k += 1
    # saturated: the difference sum (flat, one-sided) or the sse (split, held
    # at mv (0, 0) by a single-point window) at its largest
    for (bw, bh), kind, mode, n in [((64, 64), "flat_255_0", None, 2),
                                    ((64, 64), "split", "point", 1),
                                    ((64, 64), "one_sided", None, 1),
                                    ((128, 128), "flat_255_0", "row", 1),
                                    ((128, 128), "split", "point", 1),
                                    ((16, 16), "split", "point", 2),
                                    ((16, 16), "flat_0_255", None, 2)]:
        p = P(FP_METHODS[k % 2], 1, ENTROPY, 0, 7 if bw > 16 else 0, LOW_LAMBDA[0],
              LOW_LAMBDA[1], (0, 0), 0)
        jobs = frame(bw, bh)[:n].copy()
        if mode:
            jobs = narrowed(jobs, mode, (0, 0))
        cases.append(Case("sat%d" % k, kind, bw, bh, jobs, p, None))
        k += 1
    for epb, ref_mv, hp in HIGH_LAMBDA:
        for bw, bh in SMALL:
            p = P(FP_METHODS[k % 5], 1, ENTROPY, k % 2, (0, 2)[k % 2], epb, SAD_PER_BIT_TOP,
                  ref_mv, hp)
            jobs = spread(frame(bw, bh, ref_mv, (0, 0)), 4, k)
            if epb == HIGH_LAMBDA[0][0]:      # the rate it needs is (0, 0)'s alone
                jobs["ref_off"] = jobs["src_off"]      # (reference 0)
            cases.append(Case("lambda%d" % k, "noise", bw, bh, jobs, p, None))
            k += 1
    return cases


SUBPEL_METHODS = ["tree", "pruned", "pruned_more"]


def fixture_subpel(fullpel_results):
    """The sub-pel groups of the fixture, about 150 jobs.  fullpel_results:
    {case name: (results, cost lists)} of fixture_fullpel()'s cases with a
    cost list -- their best mvs are the starts and their cost lists the
    input; the edge / corner starts take no cost list."""
    by_name = {c.name: c for c in fixture_fullpel()}
    cases = []
    k = 0
    for name in sorted(fullpel_results, key=lambda s: (len(s), s)):
        c = by_name[name]
        if not c.params.use_cl or c.name.startswith(("row", "col")):
            continue
        res, cl = fullpel_results[name]
        sj = subpel_from_fullpel(c, res)
        hp = 1 if c.params.hp else k % 2
        p = SP(SUBPEL_METHODS[k % 3], hp, (0, 1, 2, 0)[k % 4], 1 + (k // 2) % 2, c.params.cost,
               int(k % 4 != 3), c.params.epb, c.params.ref_mv, 0)
        cases.append(Case("sub_" + name, c.kind, c.bw, c.bh, sj, p,
                          np.ascontiguousarray(cl, np.int32)))
        k += 1
    for kind in ("flat_128_128", "checker", "ramp_x"):
        for bw, bh in ((8, 8), (16, 16)):
            sj = subpel_edge_jobs(bw, bh, (13, -21))
            sj = sj[[i * 9 % len(sj) for i in range(8)]]     # one of each edge / corner
            p = SP(SUBPEL_METHODS[k % 3], k % 2, 0, 1 + k % 2, (ENTROPY, L1)[k % 2], 0,
                   LOW_LAMBDA[0], (13, -21), 0)
            cases.append(Case("edge%d" % k, kind, bw, bh, sj, p, None))
            k += 1
    return cases


def subpel_from_fullpel(case, results):
    """Sub-pel jobs continuing a full-pel case's jobs from `results`: the
    block's own SubpelMvLimits (whatever window the full-pel job was given)."""
    from lavish_dsp import motion as M
    sj = np.zeros(len(case.jobs), M.SUBPEL_JOB_DTYPE)
    mi_rows, mi_cols = ((H + 7) & ~7) // 4, ((W + 7) & ~7) // 4
    for i, jb in enumerate(case.jobs):
        org = int(jb["src_off"]) - BORDER * STRIDE - BORDER
        y, x = org // STRIDE, org % STRIDE
        lim = M.subpel_limits(M.block_mv_limits(mi_rows, mi_cols, y // 4, x // 4, case.bh // 4,
                                                case.bw // 4, BORDER), case.params.ref_mv)
        sj["col_min"][i], sj["col_max"][i], sj["row_min"][i], sj["row_max"][i] = lim
    sj["src_off"], sj["ref_off"] = case.jobs["src_off"], case.jobs["ref_off"]
    sj["start_row"] = results["best_row"].astype(np.int32) * 8
    sj["start_col"] = results["best_col"].astype(np.int32) * 8
    sj["ref_mv_row"], sj["ref_mv_col"] = case.params.ref_mv
    return sj


# ------------------------------------------------------ the stored fixture --
JOB_FIELDS = ["src_off", "ref_off", "start_row", "start_col", "ref_mv_row", "ref_mv_col",
              "col_min", "col_max", "row_min", "row_max"]
Group = collections.namedtuple("Group", "name kind bw bh jobs params rows J src refs")


def load_fixture():
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                     "fix_mcomp_extremes.npz")))


def fixture_groups(F, which):
    """The stored cases of fix_mcomp_extremes.npz, which = "fp" or "sp": the
    JOB records, the parameters (a dict by the stored field names), the
    reference's rows with their field index, and the stored planes."""
    from lavish_dsp import motion as M
    J = {n: i for i, n in enumerate(F[which + "_row_fields"])}
    rows_all = F[which + "_rows"]
    for ci, (name, kind) in enumerate(zip(F[which + "_names"], F[which + "_kinds"])):
        prm = dict(zip((str(n) for n in F[which + "_param_fields"]),
                       (int(v) for v in F[which + "_params"][ci])))
        rows = rows_all[rows_all[:, J["case"]] == ci]
        rec = np.zeros(len(rows), M.JOB_DTYPE)
        for f in JOB_FIELDS:
            rec[f] = rows[:, J[f]]
        key = plane_key(str(kind), prm["bw"], prm["bh"])
        yield Group(str(name), str(kind), prm["bw"], prm["bh"], rec, prm, rows, J,
                    F["src__" + key], F["refs__" + key])
