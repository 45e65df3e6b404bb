"""numpy restatement of the high-bit-depth sub-pel searches that rank by the
upsampled prediction -- av1_find_best_sub_pixel_tree (plain, with second_pred,
with second_pred and a mask) and av1_find_best_obmc_sub_pixel_tree_up of
av1/encoder/mcomp.c with subpel_search_type USE_2_TAPS / USE_4_TAPS /
USE_8_TAPS over uint16 planes: upsampled_pref_error's is_cur_buf_hbd branch
(:2428-2448), aom_highbd_upsampled_pred_c and its comp_avg / comp_mask forms
(av1/encoder/reconinter_enc.c:562-720, unscaled), then the depth's vf / ovf --
and the reader of tests/golden/fix_subpel_up_hbd.npz.

Nothing is walked here: the search is _compsubpel_ref.search over an Env whose
error is upsampled_pred below, _compsubpel_ref.upsampled_pred at u16 with the
depth's clip.  The 8-tap-layout kernels of av1_get_filter come from the
library's own table (lavish_dsp.inter.interp_kernels).

test_subpel_up_hbd_cpu.py pins run_batch to the fixture (the reference's own
results); the GPU tests then use it at the sizes the fixture cannot reach.
"""
import collections
import os

import numpy as np

import _compref as R
import _compsearch_ref as S
import _compsubpel_ref as P
import _hbdsearch_ref as H
import _mvextremes as X
import _pixref as PX

PLAIN, AVG, MASK, OBMC = P.PLAIN, P.AVG, P.MASK, P.OBMC
USE_2_TAPS_ORIG, USE_2_TAPS, USE_4_TAPS, USE_8_TAPS = range(4)
TREE = P.TREE
RESULT_FIELDS = P.RESULT_FIELDS
FORM_NAMES = {PLAIN: "plain", AVG: "avg", MASK: "mask", OBMC: "obmc"}

_kernels = {}


def up_kernels(search_type):
    """av1_get_filter(search_type)'s kernels in the 8-tap layout: [16, 8]
    (USE_2_TAPS: av1_bilinear_filters, 128 - 8 * phase and 8 * phase in the
    middle)."""
    if search_type not in _kernels:
        if search_type == USE_2_TAPS:
            k = np.zeros((16, 8), np.int64)
            k[:, 3], k[:, 4] = 128 - 8 * np.arange(16), 8 * np.arange(16)
        else:
            k = P.up_kernels(search_type)
        _kernels[search_type] = k
    return _kernels[search_type]


def upsampled_pred(ref, off, stride, w, h, sx, sy, search_type, bd, top=None, clip_mid=True,
                   facts=None):
    """aom_highbd_upsampled_pred_c for an unscaled reference: the block at
    flat offset `off`, sub-pel (sx, sy) in 1/8 pel; every pass is
    clip_pixel_highbd(ROUND_POWER_OF_TWO(sum, 7), bd).  top: clip there
    instead of at (1 << bd) - 1; clip_mid False: leave the 2-D case's
    intermediate rows unclipped (neither is the reference: only to show that
    the difference matters).  facts: a dict that counts horizontal passes
    that clipped at 0 (`low`) and at the top (`high`), and 2-D predictions in
    which the intermediate's clip changed a final pixel (`mid`)."""
    top = (1 << bd) - 1 if top is None else top

    def win(y0, nrows, x0, ncols):
        idx = (np.arange(nrows)[:, None] + y0) * stride + np.arange(ncols)[None, :] + x0
        return ref[off + idx].astype(np.int64)
    if not sx and not sy:
        return win(0, h, 0, w)
    K = up_kernels(search_type)

    def horiz(a, k, clip=True):     # a: [rows, w + 7] from column -3
        v = (sum(a[:, t:t + w] * k[t] for t in range(8)) + 64) >> 7
        if facts is not None:
            facts["low"] = facts.get("low", 0) + int((v < 0).any())
            facts["high"] = facts.get("high", 0) + int((v > top).any())
        return np.clip(v, 0, top) if clip else v

    def vert(a, k):                 # a: [h + 7, w] from row -3
        return np.clip((sum(a[t:t + h, :] * k[t] for t in range(8)) + 64) >> 7, 0, top)
    if not sy:
        return horiz(win(0, h, -3, w + 7), K[2 * sx])
    if not sx:
        return vert(win(-3, h + 7, 0, w), K[2 * sy])
    a = win(-3, h + 7, -3, w + 7)
    out = vert(horiz(a, K[2 * sx], clip_mid), K[2 * sy])
    if facts is not None and clip_mid:
        saved, facts = facts, None      # (the second evaluation counts nothing)
        other = vert(horiz(a, K[2 * sx], False), K[2 * sy])
        facts = saved
        facts["mid"] = facts.get("mid", 0) + int((other != out).any())
    return out


class Env(P.Env):
    """One sub-pel job over flat uint16 planes at bit depth bd, any form.
    top / clip_mid: as upsampled_pred (the variants that are not the
    reference)."""

    def __init__(self, src, ref, stride, bw, bh, job, cost, bd, form, second=None, mask=None,
                 invert=0, wsrc=None, omask=None):
        P.Env.__init__(self, src, ref, stride, bw, bh, job, cost, form, second, mask, invert,
                       wsrc, omask)
        self.bd, self.top, self.clip_mid, self.facts = bd, None, True, None
        self.win = np.arange(bh + 1)[:, None] * stride + np.arange(bw + 1)[None, :]

    def pred(self, r, c, search_type):
        off = self.ref_off + (r >> 3) * self.stride + (c >> 3)
        if search_type == USE_2_TAPS_ORIG:      # the two u16 bilinear passes
            return PX.bilinear(self.ref[off + self.win], c & 7, r & 7, highbd=True)
        return upsampled_pred(self.ref, off, self.stride, self.bw, self.bh, c & 7, r & 7,
                              search_type, self.bd, self.top, self.clip_mid, self.facts)

    def err(self, r, c, search_type):
        """(variance, sse) of the form's prediction at the 1/8-pel mv."""
        p = self.pred(r, c, search_type)
        if self.form == OBMC:
            v, sse = R.obmc_variance(p, self.wsrc, self.omask, self.bd)
        else:
            if self.form == AVG:
                p = R.avg_pred(p, self.second)
            elif self.form == MASK:
                p = R.mask_pred(p, self.second, self.mask, self.invert)
            v, sse = R.variance(p, self.src, self.bd)
        return int(v), int(sse)


def make_env(form, src, ref, stride, bw, bh, cj, cost, bd, second=None, mask=None, mask_stride=0,
             wsrc=None, omask=None):
    """The Env of one COMP_SUBPEL_JOB_DTYPE record over flat planes and pools
    (form PLAIN reads only the record's base)."""
    n = bw * bh
    so, mo = int(cj["second_off"]), int(cj["mask_off"])
    jb = cj["base"]
    if form == OBMC:
        return Env(None, ref, stride, bw, bh, jb, cost, bd, OBMC,
                   wsrc=wsrc[so:so + n].astype(np.int64).reshape(bh, bw),
                   omask=omask[mo:mo + n].astype(np.int64).reshape(bh, bw))
    sec = msk = None
    if form != PLAIN:
        sec = second[so:so + n].astype(np.int64).reshape(bh, bw)
    if form == MASK:
        msk = R.window(mask[mo:], mask_stride, bw, bh).astype(np.int64)
    return Env(src, ref, stride, bw, bh, jb, cost, bd, form, sec, msk, int(cj["invert_mask"]))


def run_batch(form, src, ref, stride, bw, bh, cjobs, cost, bd, search_type=USE_8_TAPS,
              forced_stop=P.EIGHTH_PEL, allow_hp=False, iters=1, second=None, mask=None,
              mask_stride=0, wsrc=None, omask=None, fullpel=None, start_from=0, method=TREE):
    """The restatement over COMP_SUBPEL_JOB_DTYPE records: [n, 5] int64
    (RESULT_FIELDS).  fullpel: [n, >= 2] (best row, best col[, second row,
    second col]) full-pel mvs to start from, as the device call chains
    (start_from 1: the second-best mv; a job without a usable one gives
    P.NO_SEARCH)."""
    out = []
    for i, cj in enumerate(cjobs):
        e = make_env(form, src, ref, stride, bw, bh, cj, cost, bd, second, mask, mask_stride, wsrc,
                     omask)
        start = None
        if fullpel is not None:
            fr, fc = (int(v) for v in fullpel[i][2 * start_from:2 * start_from + 2])
            start = (8 * fr, 8 * fc)
            if start_from and (P.INVALID in (fr, fc) or not e.in_range(*start)):
                out.append([P.NO_SEARCH[f] for f in RESULT_FIELDS])
                continue
        r = P.search(e, method, search_type, forced_stop, allow_hp, iters, start)
        out.append([r[f] for f in RESULT_FIELDS])
    return np.array(out, np.int64).reshape(-1, 5)


# ------------------------------------------------------------------ content --
def step_edges(bd, seed=23):
    """Step-edge planes between 0 and the depth's maximum: a seeded pattern of
    4 x 4 cells that are 0 or the maximum, repeating every 32 pixels (the
    8-tap kernels' negative lobes over- and undershoot at every edge, so
    horizontal passes clip at both ends and clipped intermediates feed the
    vertical pass), the references the source moved by (1, 2) and (-2, 1) full
    pel with the low bits of a few pixels changed (a 16 x 16 tile) so that no
    candidate matches exactly."""
    rng = np.random.default_rng(seed + bd)
    top = (1 << bd) - 1
    cells = rng.integers(0, 2, (8, 8))
    src = H._tiled(np.kron(cells, np.ones((4, 4), np.int64))) * top
    refs = []
    for k, sft in enumerate(((1, 2), (-2, 1))):
        r = np.roll(src, sft, (0, 1))
        noise = H._tiled(rng.integers(0, 8, (16, 16)) * (rng.integers(0, 4, (16, 16)) == 0))
        refs.append(np.where(r > 0, r - noise, r + noise))
    return src.astype(np.uint16), np.stack(refs[:X.NREF]).astype(np.uint16)


OWN_KINDS = ("edges",)
_planes = {}


def planes(kind, bd, bw=16, bh=16):
    """(src, refs) uint16 of a content kind at a depth: _hbdsearch_ref's, or
    the step edges; shared, read-only."""
    if kind not in OWN_KINDS:
        return H.planes(kind, bd, bw, bh)
    if (kind, bd) not in _planes:
        s, r = step_edges(bd)
        s.setflags(write=False)
        r.setflags(write=False)
        _planes[(kind, bd)] = (s, r)
    return _planes[(kind, bd)]


def plane_key(kind, bd, bw, bh):
    return "%s_bd%d" % (kind, bd) if kind in OWN_KINDS else H.plane_key(kind, bd, bw, bh)


# ------------------------------------------------------------------ fixture --
CASE_FIELDS = ["form", "bd", "bw", "bh", "search_type", "allow_hp", "forced_stop", "iters", "cost",
               "error_per_bit", "mask_stride", "plane"]
ROW_FIELDS = (["case"] + X.JOB_FIELDS + ["second_off", "mask_off", "invert_mask"] + RESULT_FIELDS)
Group = collections.namedtuple("Group", "index prm plane cjobs rows J")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    """fix_subpel_up_hbd.npz joined with the plane sets it shares with
    fix_mcomp_hbd.npz (the fixture stores only its own)."""
    F = dict(np.load(os.path.join(GOLDEN, "fix_subpel_up_hbd.npz")))
    MH = H.load_fixture()
    for name in (str(s) for s in F["planes"]):
        if "src__" + name not in F:
            F["src__" + name], F["refs__" + name] = MH["src__" + name], MH["refs__" + name]
    return F


def job_records(rows, J):
    from lavish_dsp import motion as M
    rec = np.zeros(len(rows), M.SUBPEL_JOB_DTYPE)
    for f in X.JOB_FIELDS:
        rec[f] = rows[:, J[f]]
    return M.comp_subpel_jobs(rec, rows[:, J["second_off"]], rows[:, J["mask_off"]],
                              rows[:, J["invert_mask"]])


def fixture_groups(F):
    """The stored cases: parameters (a dict), the plane set's name, the
    COMP_SUBPEL_JOB_DTYPE records and the reference's rows."""
    J = {n: i for i, n in enumerate(ROW_FIELDS)}
    assert [str(s) for s in F["row_fields"]] == ROW_FIELDS
    assert [str(s) for s in F["case_fields"]] == CASE_FIELDS
    for ci, vals in enumerate(F["cases"]):
        prm = dict(zip(CASE_FIELDS, (int(v) for v in vals)))
        rows = F["rows"][F["rows"][:, 0] == ci]
        yield Group(ci, prm, str(F["planes"][prm["plane"]]), job_records(rows, J), rows, J)


def group_cost(prm):
    return S.cost_of(prm["cost"], prm["error_per_bit"], 0, prm["allow_hp"])


def group_planes(F, g):
    return F["src__" + g.plane].reshape(-1), F["refs__" + g.plane].reshape(-1)


def group_env(F, g, cj):
    p = g.prm
    src, ref = group_planes(F, g)
    return make_env(p["form"], src, ref, X.STRIDE, p["bw"], p["bh"], cj, group_cost(p), p["bd"],
                    F["second"], F["mask"], p["mask_stride"], F["wsrc"], F["omask"])


def group_expected(F, g):
    """A group's rows through the restatement: [n, 5] (RESULT_FIELDS)."""
    p = g.prm
    src, ref = group_planes(F, g)
    return run_batch(p["form"], src, ref, X.STRIDE, p["bw"], p["bh"], g.cjobs, group_cost(p),
                     p["bd"], p["search_type"], p["forced_stop"], bool(p["allow_hp"]), p["iters"],
                     F["second"], F["mask"], p["mask_stride"], F["wsrc"], F["omask"])


# ----------------------------------------------------------------- coverage --
def check_coverage(F):
    """What a fixture that pins something contains, from the reference's rows
    and the inputs alone; returns the counts (the generator stops unless its
    rows meet them; tests/test_subpel_up_hbd_cpu.py asserts the same on the
    committed file)."""
    f = collections.Counter()
    combos = set()
    forms = {k: collections.Counter() for k in (PLAIN, AVG, MASK, OBMC)}
    for g in fixture_groups(F):
        p, J = g.prm, g.J
        bd, st, form = p["bd"], p["search_type"], p["form"]
        combos.add((bd, st, form))
        args = (TREE, st, p["forced_stop"], bool(p["allow_hp"]), p["iters"])
        for cj, row in zip(g.cjobs, g.rows):
            if form == MASK:
                combos.add((bd, "inv", int(cj["invert_mask"])))
            r, c = int(row[J["best_row"]]), int(row[J["best_col"]])
            start = (int(row[J["start_row"]]), int(row[J["start_col"]]))
            fm = forms[form]
            fm["rows"] += 1
            fm["moved"] += (r, c) != start
            low = (r | c) & 7
            f["half"] += low == 4
            f["quarter"] += low in (2, 6)
            f["eighth"] += bool(low & 1)
            e = group_env(F, g, cj)
            e.facts = {}
            tr = {}
            got = P.search(e, *args, trace=tr)
            assert [got[k] for k in RESULT_FIELDS] == [int(v) for v in row[J["best_row"]:]], \
                (g.index, p)
            f["second_level"] += tr["second_level"] > 0
            f["oob"] += tr["oob"] > 0
            f["clip_low_%d" % bd] += e.facts.get("low", 0) > 0
            f["clip_high_%d" % bd] += e.facts.get("high", 0) > 0
            if form == OBMC and st >= USE_2_TAPS and p["cost"] == X.L1:
                f["obmc_l1"] += 1
            if (start[0] | start[1]) & 7:
                f["subpel_start"] += 1
                f["centre_differs"] += e.err(start[0], start[1], st) != \
                    e.err(start[0] & ~7, start[1] & ~7, st)

            # a candidate whose clipped intermediate changes the final pixel
            f["mid_clip_%d" % bd] += e.facts.get("mid", 0) > 0
            e.facts = None
            if st >= USE_4_TAPS and bd > 8:     # the same search clipped at 255
                e.top = 255
                alt = P.search(e, *args)
                f["clip255_differs"] += any(alt[k] != got[k] for k in RESULT_FIELDS)
                e.top = None
            if st == USE_8_TAPS:
                alt = P.search(e, TREE, USE_2_TAPS, *args[2:])
                f["taps8_vs_bilinear"] += (alt["best_row"], alt["best_col"]) != (r, c)
            if bd == 12:                    # the variance negative before its clamp
                pr = e.pred(r, c, st)
                if form == OBMC:
                    v = e.wsrc - pr * e.omask
                    rr = (np.abs(v) + 2048) >> 12
                    d = np.where(v < 0, -rr, rr)
                else:
                    if form == AVG:
                        pr = R.avg_pred(pr, e.second)
                    elif form == MASK:
                        pr = R.mask_pred(pr, e.second, e.mask, e.invert)
                    d = pr - e.src
                _, sse_r, sum_r = PX.variance_tail(int(d.sum()), int((d * d).sum()), 12,
                                                   p["bw"] * p["bh"])
                f["clamped_12"] += int(PX.before_clamp(sse_r, sum_r, p["bw"] * p["bh"])) < 0
    for bd in (8, 10, 12):
        for st in (USE_2_TAPS, USE_4_TAPS, USE_8_TAPS):
            for form in (PLAIN, AVG, MASK, OBMC):
                assert (bd, st, form) in combos, (bd, st, form)
        for inv in (0, 1):
            assert (bd, "inv", inv) in combos, (bd, inv)
    need = ["half", "quarter", "eighth", "second_level", "oob", "obmc_l1", "subpel_start",
            "centre_differs", "clip255_differs", "taps8_vs_bilinear", "clamped_12"]
    need += ["%s_%d" % (k, bd) for k in ("clip_low", "clip_high", "mid_clip") for bd in (8, 10, 12)]
    for k in need:
        assert f[k] > 0, (k, dict(f))
    for form, fm in forms.items():
        assert 3 * fm["moved"] >= fm["rows"] > 0, (form, dict(fm))
    sizes = {(g.prm["form"], g.prm["bw"], g.prm["bh"]) for g in fixture_groups(F)}
    for form in forms:
        assert (form, 32, 32) in sizes, form
    return dict(f), {FORM_NAMES[k]: dict(v) for k, v in forms.items()}
