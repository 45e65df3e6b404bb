"""Golden fixture of the chroma-from-luma layer, from the reference's own C
text executed by cinterp.py (as gen_fix_intra.py / gen_fix_blend.py do).

  fix_cfl.npz
    data          one flat int32 pool; the row tables hold positions into it
    getter_rows   tests/_cflref.py G_COLS: every cfl_get_*_c getter at the 14
                  sizes, the function it returns executed directly
    block_rows    B_COLS: cfl_store_block (frame-edge extents cut in width,
                  in height and in both through mb_to_right_edge /
                  mb_to_bottom_edge) or cfl_store_tx (the sub-8x8 stores of
                  BLOCK_4X4 / 4X8 / 8X4 luma blocks at even and odd mi_row /
                  mi_col; u8 planes) on an xd, then cfl_load_dc_pred +
                  cfl_predict_block; records ac_buf_q3 and the prediction
    search_rows   S_COLS: cfl_pick_plane_parameter executed whole
                  (cfl_search_range 1) on an AV1_COMP / MACROBLOCK, records
                  the estimate, the costs it evaluated and which they were
    joint_map     [33, 33, 3]: (valid, cfl_alpha_idx, cfl_alpha_signs) as
                  cfl_rd_pick_alpha forms them from two estimates

Form of the search rows: intra_mode_search.c from PLANE_SIGN_TO_JOINT_SIGN to
the end of cfl_pick_plane_parameter is read from the reference at run time
(cfl_idx_to_sign_and_alpha, cfl_compute_rd, cfl_pick_plane_parameter as
written), with two edits to cfl_compute_rd: its intra_model_rd call becomes a
call of lavish_model_rd below, and its full-RD branch is emptied.
lavish_model_rd is intra_model_rd's loop body for the one transform block of
a CfL plane, made only of reference functions: cfl_load_dc_pred +
cfl_predict_block (the path av1_predict_intra_block_facade takes with
dc_pred_is_cached set; the cache is filled by cfl_store_dc_pred),
av1_subtract_block, av1_quick_txfm (use_hadamard 0) and aom_satd.  On uint8_t
planes the DC cache pair is replaced by a copy loop of the generator's
(lavish_load_dc): there cfl_store_dc_pred / cfl_load_dc_pred memcpy bytes
between the int16_t cache and the uint8_t rows, which cinterp.py does not do
between element sizes; the uint16_t rows run the reference's pair.  The joint
parameters come from cfl_idx_to_sign_and_alpha through a three-line caller.

The generator stops unless _cflref.coverage_problems() is empty.

Usage: python tests/golden/gen_fix_cfl.py
"""
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cinterp as C  # noqa: E402
import _cflref as R  # noqa: E402
from gen_fixtures import REF, _get, _set, check_errors  # noqa: E402

YV12_FLAG_HIGHBITDEPTH = 8  # aom_scale/yv12config.h
TX_W, TX_H = R.TX_W, R.TX_H

GLUE = """
int64_t lavish_seen_cost[33];
int lavish_seen_mask[33];
uint8_t lavish_dc_row[32];
/* cfl_load_dc_pred; for uint8_t planes a copy loop of the generator's own (below) */
void lavish_load_dc(MACROBLOCK *x, int plane, TX_SIZE tx_size) {
  MACROBLOCKD *xd = &x->e_mbd;
  struct macroblockd_plane *pd = &xd->plane[plane];
  if (is_cur_buf_hbd(xd)) {
    cfl_load_dc_pred(xd, pd->dst.buf, pd->dst.stride, tx_size, plane - 1);
    return;
  }
  for (int j = 0; j < tx_size_high[tx_size]; ++j)
    for (int i = 0; i < tx_size_wide[tx_size]; ++i) pd->dst.buf[j * pd->dst.stride + i] = lavish_dc_row[i];
}
int64_t lavish_model_rd(MACROBLOCK *x, int plane, TX_SIZE tx_size, int cfl_idx) {
  MACROBLOCKD *xd = &x->e_mbd;
  struct macroblock_plane *p = &x->plane[plane];
  struct macroblockd_plane *pd = &xd->plane[plane];
  const BitDepthInfo bd_info = get_bit_depth_info(xd);
  const int w = tx_size_wide[tx_size], h = tx_size_high[tx_size];
  lavish_load_dc(x, plane, tx_size);
  cfl_predict_block(xd, pd->dst.buf, pd->dst.stride, tx_size, plane);
  av1_subtract_block(bd_info, h, w, p->src_diff, w, p->src.buf, p->src.stride, pd->dst.buf,
                     pd->dst.stride);
  av1_quick_txfm(0, tx_size, bd_info, p->src_diff, w, p->coeff);
  const int64_t c = aom_satd(p->coeff, tx_size_2d[tx_size]);
  lavish_seen_cost[cfl_idx] = c;
  lavish_seen_mask[cfl_idx] = 1;
  return c;
}
"""

GLUE2 = """
void lavish_seen_reset(void) {
  for (int i = 0; i < 33; ++i) { lavish_seen_cost[i] = 0; lavish_seen_mask[i] = 0; }
}
int lavish_pick(const AV1_COMP *cpi, MACROBLOCK *x, int plane, TX_SIZE tx_size) {
  return cfl_pick_plane_parameter(cpi, x, plane, tx_size, 1);
}
void lavish_sign_alpha(int cfl_idx, int *out) {
  CFL_SIGN_TYPE s;
  int a;
  cfl_idx_to_sign_and_alpha(cfl_idx, &s, &a);
  out[0] = s;
  out[1] = a;
}
void lavish_consts(int *out) {
  out[0] = CFL_INDEX_ZERO;
  out[1] = CFL_ALPHABET_SIZE_LOG2;
  out[2] = CFL_SIGNS;
  out[3] = CFL_MAGS_SIZE;
}
void lavish_store_tx(MACROBLOCK *x, int row, int col, TX_SIZE tx_size, BLOCK_SIZE bsize) {
  cfl_store_tx(&x->e_mbd, row, col, tx_size, bsize);
}
void lavish_store_block(MACROBLOCK *x, BLOCK_SIZE bsize, TX_SIZE tx_size) {
  cfl_store_block(&x->e_mbd, bsize, tx_size);
}
void lavish_store_dc(MACROBLOCK *x, const uint8_t *input, int plane, int width) {
  cfl_store_dc_pred(&x->e_mbd, input, plane - 1, width);
}
void lavish_predict(MACROBLOCK *x, int plane, TX_SIZE tx_size) {
  MACROBLOCKD *xd = &x->e_mbd;
  struct macroblockd_plane *pd = &xd->plane[plane];
  lavish_load_dc(x, plane, tx_size);
  cfl_predict_block(xd, pd->dst.buf, pd->dst.stride, tx_size, plane);
}
"""


def search_text():
    with open(os.path.join(REF, "av1/encoder/intra_mode_search.c")) as fh:
        lines = fh.read().split("\n")
    a = next(i for i, l in enumerate(lines) if l.startswith("#define PLANE_SIGN_TO_JOINT_SIGN"))
    b = next(i for i, l in enumerate(lines)
             if "static AOM_INLINE void set_invalid_cfl_parameters" in l)
    text = "\n".join(lines[a:b])
    text, n = re.subn(r"intra_model_rd\(cm, x, plane, plane_bsize, tx_size,\s*/\*use_hadamard=\*/0\)",
                      "lavish_model_rd(x, plane, tx_size, cfl_idx)", text)
    assert n == 1, n
    text, n = re.subn(r"\} else \{\s*av1_init_rd_stats\(rd_stats\);.*?cfl_cost = rd_stats->rdcost;\s*\}",
                      "} else {\n    cfl_cost = 0;\n  }", text, flags=re.S)
    assert n == 1, n
    return text, "<intra_mode_search.c:%d-%d>" % (a + 1, b)


def tu_cfl():
    tu = C.TU(REF, ["aom/aom_integer.h", "aom_ports/mem.h", "aom_dsp/aom_dsp_common.h",
                    "aom_dsp/txfm_common.h", "av1/common/enums.h", "av1/common/common.h",
                    "av1/common/common_data.h", "av1/common/common_data.c", "av1/common/av1_txfm.h",
                    "av1/common/av1_txfm.c", "av1/encoder/av1_fwd_txfm1d.h",
                    "av1/encoder/av1_fwd_txfm1d_cfg.h", "av1/encoder/av1_fwd_txfm1d.c",
                    "av1/encoder/av1_fwd_txfm2d.c", "av1/encoder/hybrid_fwd_txfm.c",
                    "aom_dsp/subtract.c", "aom_dsp/avg.c", "av1/common/cfl.h", "av1/common/cfl.c",
                    "av1/encoder/encoder.h", "av1/encoder/encodemb.c"], C.reference_defines(REF))
    tu.add_source(GLUE, "<gen_fix_cfl.py glue>")
    tu.add_source(*search_text())
    tu.add_source(GLUE2, "<gen_fix_cfl.py callers>")
    need = ["cfl_store_tx", "cfl_store_block", "cfl_predict_block", "cfl_load_dc_pred",
            "cfl_store_dc_pred", "av1_subtract_block", "av1_quick_txfm", "aom_satd_c",
            "cfl_pick_plane_parameter", "cfl_compute_rd", "cfl_idx_to_sign_and_alpha",
            "lavish_model_rd", "lavish_pick", "lavish_predict"]
    need += [g + "_c" for g in R.GETTERS]
    check_errors(tu, need)
    return tu


class Pool:
    def __init__(self):
        self.chunks, self.pos = [], 0

    def add(self, a):
        a = np.asarray(a, np.int64).reshape(-1)
        p = self.pos
        self.chunks.append(a)
        self.pos += a.size
        return p


# ---------------------------------------------------------------- getters --
def gen_getters(tu, pool, rng):
    rows = []
    for gi, g in enumerate(R.GETTERS):
        kind = R.getter_kind(g)
        for k, tx in enumerate(R.CFL_TX):
            w, h = TX_W[tx], TX_H[tx]
            fn = tu.func(g + "_c")(tx)
            lbd = g.endswith("lbd") or kind == "predict_lbd"
            for bd in ((8,) if lbd else (8, 10, 12)):
                if kind == "subsample" and not lbd and bd == 8 and k % 3:
                    continue
                maxv = (1 << bd) - 1
                ext = (k + bd) % 4 == 0   # extremes
                if kind == "subtract_average":
                    q3 = np.full((h, w), 8 * maxv) if ext else rng.integers(0, 8 * maxv + 1, (h, w))
                    src = tu.buffer("uint16_t", [0] * R.SQUARE)
                    dst = tu.buffer("int16_t", [0] * R.SQUARE)
                    for y in range(h):
                        src.buf[y * 32:y * 32 + w] = [int(v) for v in q3[y]]
                    fn(src, dst)
                    out = np.array(dst.buf, np.int64).reshape(32, 32)[:h, :w]
                    rows.append([gi, tx, bd, 0, pool.add(q3), 0, pool.add(out)])
                elif kind == "subsample":
                    sx, sy = R.getter_sub(g)
                    luma = np.full((h, w), maxv) if ext else rng.integers(0, maxv + 1, (h, w))
                    stride = w + 3
                    buf = np.zeros((h, stride), np.int64)
                    buf[:, :w] = luma
                    inp = tu.buffer("uint8_t" if lbd else "uint16_t", buf.reshape(-1).tolist())
                    o = tu.buffer("uint16_t", [0] * R.SQUARE)
                    fn(inp, stride, o)
                    out = np.array(o.buf, np.int64).reshape(32, 32)[:h >> sy, :w >> sx]
                    rows.append([gi, tx, bd, 0, pool.add(luma), 0, pool.add(out)])
                else:
                    alpha = (16, -16, 5, -9)[(k + bd) % 4]
                    ac = rng.integers(-4 * maxv, 4 * maxv + 1, (h, w))
                    dc = rng.integers(0, maxv + 1, (h, w))
                    if ext:   # clips at 0 and at the maximum
                        dc = np.where(rng.integers(0, 2, (h, w)) > 0, maxv - 2, 2)
                    cell = np.zeros((32, 32), np.int64)
                    cell[:h, :w] = ac
                    a = tu.buffer("int16_t", cell.reshape(-1).tolist())
                    stride = w + 5
                    buf = np.zeros((h, stride), np.int64)
                    buf[:, :w] = dc
                    d = tu.buffer("uint8_t" if lbd else "uint16_t", buf.reshape(-1).tolist())
                    fn(*([a, d, stride, alpha] + ([] if lbd else [bd])))
                    out = np.array(d.buf, np.int64).reshape(h, stride)[:, :w]
                    rows.append([gi, tx, bd, alpha, pool.add(ac), pool.add(dc), pool.add(out)])
    return rows


# --------------------------------------------------------- xd based rows --
class Scene:
    """a MACROBLOCK whose xd holds a CfL context, one luma and one chroma plane"""
    def __init__(self, tu, bd, hbd, sub, bsize_name, plane):
        self.tu, self.bd, self.hbd, self.sub, self.plane = tu, bd, hbd, sub, plane
        E = tu.enums
        self.et = "uint16_t" if hbd else "uint8_t"
        self.x = tu.struct_obj("MACROBLOCK")
        X = self.x.buf[0]
        self.X, self.XD = X, _get(X, "e_mbd")
        self.mbmi = tu.struct_obj("MB_MODE_INFO")
        _set(self.mbmi.buf[0], bsize=E[bsize_name], uv_mode=E["UV_CFL_PRED"])
        ybuf = tu.struct_obj("YV12_BUFFER_CONFIG")
        _set(ybuf.buf[0], flags=YV12_FLAG_HIGHBITDEPTH if hbd else 0)
        _set(self.XD, mi=C.Pointer([self.mbmi], 0, C.Ptr(tu.ctype("MB_MODE_INFO"))), cur_buf=ybuf,
             bd=bd, mi_row=0, mi_col=0, mb_to_right_edge=0, mb_to_bottom_edge=0)
        cfl = _get(self.XD, "cfl")
        _set(cfl, subsampling_x=sub[0], subsampling_y=sub[1], are_parameters_computed=0, store_y=1)
        self.cfl = cfl
        planes = _get(self.XD, "plane")
        _set(planes[0], subsampling_x=0, subsampling_y=0)
        for p in (1, 2):
            _set(planes[p], subsampling_x=sub[0], subsampling_y=sub[1])
        self.planes = planes

    def tag(self, p):
        return self.tu.tagged(p) if self.hbd else p

    def luma_plane(self, luma, stride):
        lh, lw = luma.shape
        buf = np.zeros((lh, stride), np.int64)
        buf[:, :lw] = luma
        self.ybuf = self.tu.buffer(self.et, buf.reshape(-1).tolist())
        self.ystride = stride
        _set(_get(self.planes[0], "dst"), buf=self.tag(self.ybuf), stride=stride)

    def chroma(self, tx, dc_row, src=None):
        """the chroma plane's dst (DC cache filled from dc_row) and source"""
        tu = self.tu
        w, h = TX_W[tx], TX_H[tx]
        self.cs = w + 3
        self.cbuf = tu.buffer(self.et, [0] * (h * self.cs))
        _set(_get(self.planes[self.plane], "dst"), buf=self.tag(self.cbuf), stride=self.cs)
        if self.hbd:
            row = tu.buffer(self.et, [int(v) for v in dc_row])
            tu.func("lavish_store_dc")(self.x, self.tag(row), self.plane, w)
        else:
            tu.global_value("lavish_dc_row")[:w] = [int(v) for v in dc_row]
        _get(self.cfl, "dc_pred_is_cached")[self.plane - 1] = 1
        _set(self.cfl, use_dc_pred_cache=1)
        if src is not None:
            ss = w + 7
            buf = np.zeros((h, ss), np.int64)
            buf[:, :w] = src
            self.sbuf = tu.buffer(self.et, buf.reshape(-1).tolist())
            mp = _get(self.X, "plane")[self.plane]
            _set(_get(mp, "src"), buf=self.tag(self.sbuf), stride=ss)
            _set(mp, src_diff=tu.buffer("int16_t", [0] * (w * h)),
                 coeff=tu.buffer("tran_low_t", [0] * (w * h)))

    def ac(self, tx):
        return np.array(_get(self.cfl, "ac_buf_q3"), np.int64).reshape(32, 32)[:TX_H[tx], :TX_W[tx]]

    def pred(self, tx):
        return np.array(self.cbuf.buf, np.int64).reshape(TX_H[tx], self.cs)[:, :TX_W[tx]]


def bsize_of(w, h):
    return "BLOCK_%dX%d" % (w, h)


def store(sc, luma, how, chroma_tx):
    """cfl_store_block of the luma block (its extent cut at the frame edge down
    to luma's shape), or the sub-8x8 cfl_store_tx calls that tile luma"""
    tu, E = sc.tu, sc.tu.enums
    lh, lw = luma.shape
    if how == "block":
        bw, bh = TX_W[chroma_tx] << sc.sub[0], TX_H[chroma_tx] << sc.sub[1]
        sc.luma_plane(luma, lw + 5)
        _set(sc.XD, mb_to_right_edge=-8 * (bw - lw), mb_to_bottom_edge=-8 * (bh - lh))
        _set(sc.mbmi.buf[0], bsize=E[bsize_of(bw, bh)])
        # mbmi->tx_size TX_4X4: max_intra_block_width aligns the cut extent to it
        tu.func("lavish_store_block")(sc.x, E[bsize_of(bw, bh)], E["TX_4X4"])
        return
    # sub-8x8: luma blocks of pw x ph (one side 4) at consecutive mi positions, the
    # first at even mi_row / mi_col; each call sees its own block as pd->dst.buf
    pw, ph = how
    stride = lw + 5
    sc.luma_plane(luma, stride)
    for y in range(0, lh, ph):
        for x in range(0, lw, pw):
            _set(sc.XD, mi_row=6 + y // 4, mi_col=10 + x // 4)
            _set(_get(sc.planes[0], "dst"),
                 buf=C.Pointer(sc.ybuf.buf, y * stride + x, sc.ybuf.ty), stride=stride)
            tu.func("lavish_store_tx")(sc.x, 0, 0, E["TX_%dX%d" % (pw, ph)], E[bsize_of(pw, ph)])


def set_alpha(sc, alpha_q3):
    """the block's parameters with this plane's alpha and a dummy other plane"""
    idx = alpha_q3 + 16
    other = 15   # alpha -1
    u, v = (idx, other) if sc.plane == 1 else (other, idx)
    valid, aidx, signs = R.joint(u, v)
    assert valid
    _set(sc.mbmi.buf[0], cfl_alpha_idx=aidx, cfl_alpha_signs=signs)


def cut(full, k):
    return full if k == 0 else max(4, (full // 2) & ~3)


def gen_blocks(tu, pool, rng):
    rows = []
    n = 0
    for tx in R.CFL_TX:
        w, h = TX_W[tx], TX_H[tx]
        for bd, hbd in ((8, 0), (10, 1), (12, 1), (8, 1)):
            if (bd, hbd) == (8, 1) and tx % 3:
                continue
            n += 1
            sub = R.SUBS[n % 3]
            if not R.luma_block_ok(w << sub[0], h << sub[1]):
                sub = (0, 0)
            fw, fh = w << sub[0], h << sub[1]
            lw, lh = cut(fw, n % 4 in (1, 3)), cut(fh, n % 4 in (2, 3))
            # get_tx_size takes the cut extent: keep it a transform size
            if max(lw, lh) > 4 * min(lw, lh):
                lw, lh = fw, fh
            maxv = (1 << bd) - 1
            ext = n % 5 == 0
            luma = np.where(rng.integers(0, 2, (lh, lw)) > 0, maxv, 0) if ext else \
                R.smooth_luma(rng, lw, lh, bd)
            plane = 1 + n % 2
            alpha = (16, -16, 3, -7, 1)[n % 5]
            dc_row = np.where(rng.integers(0, 2, w) > 0, maxv - 1, 1) if ext else \
                rng.integers(maxv // 4, 3 * maxv // 4, w)
            sc = Scene(tu, bd, hbd, sub, bsize_of(fw, fh), plane)
            store(sc, luma, "block", tx)
            sc.chroma(tx, dc_row)
            set_alpha(sc, alpha)
            tu.func("lavish_predict")(sc.x, plane, tu.enums["TX_%dX%d" % (w, h)])
            rows.append([bd, hbd, sub[0], sub[1], tx, lw, lh, plane, alpha, pool.add(luma),
                         pool.add(dc_row), pool.add(sc.ac(tx)), pool.add(sc.pred(tx))])
    # all-maximum luma at 12 bits: the largest q3 and sum
    sc = Scene(tu, 12, 1, (0, 0), "BLOCK_32X32", 1)
    luma = np.full((32, 32), 4095)
    store(sc, luma, "block", 3)
    dc_row = rng.integers(0, 4096, 32)
    sc.chroma(3, dc_row)
    set_alpha(sc, 16)
    tu.func("lavish_predict")(sc.x, 1, tu.enums["TX_32X32"])
    rows.append([12, 1, 0, 0, 3, 32, 32, 1, 16, pool.add(luma), pool.add(dc_row),
                 pool.add(sc.ac(3)), pool.add(sc.pred(3))])
    # sub-8x8 stores (u8): 4:2:0 and 4:2:2, luma blocks 4x4 / 4x8 / 8x4 / 4x16 / 16x4
    for k, (sub, piece, lw, lh) in enumerate((((1, 1), (4, 4), 8, 8), ((1, 1), (4, 8), 8, 8),
                                             ((1, 1), (8, 4), 8, 8), ((1, 1), (4, 16), 8, 16),
                                             ((1, 1), (16, 4), 16, 8), ((1, 0), (4, 4), 8, 4),
                                             ((1, 0), (4, 8), 8, 8), ((1, 0), (4, 16), 8, 16))):
        tx = R.tx_of(lw >> sub[0], lh >> sub[1])
        luma = R.smooth_luma(rng, lw, lh, 8) + rng.integers(-20, 21, (lh, lw))
        luma = np.clip(luma, 0, 255)
        plane = 1 + k % 2
        sc = Scene(tu, 8, 0, sub, bsize_of(*piece), plane)
        store(sc, luma, piece, tx)
        dc_row = rng.integers(60, 200, TX_W[tx])
        sc.chroma(tx, dc_row)
        alpha = (-11, 6, 14, -2)[k % 4]
        set_alpha(sc, alpha)
        tu.func("lavish_predict")(sc.x, plane, tu.enums["TX_%dX%d" % (TX_W[tx], TX_H[tx])])
        rows.append([8, 0, sub[0], sub[1], tx, lw, lh, plane, alpha, pool.add(luma),
                     pool.add(dc_row), pool.add(sc.ac(tx)), pool.add(sc.pred(tx))])
    return rows


def run_search(tu, cpi, pool, bd, hbd, sub, tx, luma, src, dc_row, plane):
    w, h = TX_W[tx], TX_H[tx]
    fw, fh = w << sub[0], h << sub[1]
    sc = Scene(tu, bd, hbd, sub, bsize_of(fw, fh), plane)
    store(sc, luma, "block", tx)
    sc.chroma(tx, dc_row, src)
    tu.func("lavish_seen_reset")()
    est = int(tu.func("lavish_pick")(cpi, sc.x, plane, tu.enums["TX_%dX%d" % (w, h)]))
    costs = np.array(tu.global_value("lavish_seen_cost"), np.int64)
    mask = np.array(tu.global_value("lavish_seen_mask"), np.int64)
    lh, lw = luma.shape
    return [bd, hbd, sub[0], sub[1], tx, lw, lh, plane, est, pool.add(luma), pool.add(src),
            pool.add(dc_row), pool.add(sc.ac(tx)), pool.add(np.concatenate([costs, mask]))]


def gen_searches(tu, pool, rng, t0):
    cpi = tu.struct_obj("AV1_COMP")
    rows = []
    n = 0
    for tx in R.CFL_TX:
        w, h = TX_W[tx], TX_H[tx]
        for bd, hbd in ((8, 0), (10, 1), (12, 1)):
            n += 1
            sub = R.SUBS[n % 3]
            if not R.luma_block_ok(w << sub[0], h << sub[1]):
                sub = (0, 0)
            luma = R.smooth_luma(rng, w << sub[0], h << sub[1], bd)
            ac = R.ac_block(luma, sub[0], sub[1], tx)
            alpha = (16, -16, 0, 7, -9, 12, -4)[n % 7]
            src, dc = R.planted_chroma(rng, ac, alpha, bd, noise=1)
            rows.append(run_search(tu, cpi, pool, bd, hbd, sub, tx, luma, src, dc[0], 1 + n % 2))
        print("  search size %dx%d  %.0fs" % (w, h, time.time() - t0), flush=True)
    # the ends and both signs on 8x8 at 12 bits (the planted alpha is recovered there)
    for k, alpha in enumerate((16, -16, 0, 9, -6)):
        luma = R.smooth_luma(rng, 8, 8, 12)
        ac = R.ac_block(luma, 0, 0, 1)
        src, dc = R.planted_chroma(rng, ac, alpha, 12, noise=0)
        rows.append(run_search(tu, cpi, pool, 12, 1, (0, 0), 1, luma, src, dc[0], 1 + k % 2))
    # ties and the carried best: the seeds the restatement found
    for k, seed in enumerate(R.WALK_SEEDS_TIES + R.WALK_SEEDS_CARRIED_BEST):
        tx, luma, src, dc = R.walk_block(seed)
        rows.append(run_search(tu, cpi, pool, 8, 0, (0, 0), tx, luma, src, dc[0], 1 + k % 2))
    print("  %d search rows  %.0fs" % (len(rows), time.time() - t0), flush=True)
    return rows


def gen_joint(tu):
    out = np.zeros((33, 33, 3), np.int64)
    sa = []
    for i in range(33):
        o = tu.buffer("int", [0, 0])
        tu.func("lavish_sign_alpha")(i, o)
        sa.append((int(o.buf[0]), int(o.buf[1])))
    k = tu.buffer("int", [0] * 4)
    tu.func("lavish_consts")(k)
    zero, log2, signs, mags = (int(v) for v in k.buf)
    assert mags == 33
    for u in range(33):
        for v in range(33):
            if u == zero and v == zero:
                continue
            (su, au), (sv, av) = sa[u], sa[v]
            out[u, v] = (1, (au << log2) + av, su * signs + sv - 1)
    return out


def main():
    t0 = time.time()
    tu = tu_cfl()
    rng = np.random.default_rng(0xCF1)
    pool = Pool()
    F = {"getter_rows": np.array(gen_getters(tu, pool, rng), np.int64)}
    print("  %d getter rows  %.0fs" % (len(F["getter_rows"]), time.time() - t0), flush=True)
    F["block_rows"] = np.array(gen_blocks(tu, pool, rng), np.int64)
    print("  %d block rows  %.0fs" % (len(F["block_rows"]), time.time() - t0), flush=True)
    F["search_rows"] = np.array(gen_searches(tu, pool, rng, t0), np.int64)
    F["joint_map"] = gen_joint(tu)
    F["data"] = np.concatenate(pool.chunks).astype(np.int32)
    bad = R.coverage_problems(F)
    if bad:
        raise SystemExit("fixture incomplete: %s" % bad)
    path = os.path.join(HERE, "fix_cfl.npz")
    np.savez_compressed(path, **F)
    size = os.path.getsize(path)
    print("wrote %s: %d bytes" % (path, size))
    if size >= 1 << 20:
        raise SystemExit("fixture too large")


if __name__ == "__main__":
    main()
