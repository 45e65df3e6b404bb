"""numpy restatement of the mask-building and blending layer
(aom_dsp/blend_a64_{mask,hmask,vmask}.c, av1/common/reconinter.c:296-439 and
:844-945, av1/encoder/rdopt.c:6362-6580, av1/common/obmc.h,
av1/encoder/wedge_utils.c:52-125) and the reader of tests/golden/fix_blend.npz.

Blocks are 2-D integer arrays; everything is computed in int64 (Python ints
for the 64-bit sums), so nothing depends on an unsigned wrap.  A leading batch
axis broadcasts.  test_blend_cpu.py pins every function here to the fixture
(the reference's own outputs); the GPU tests then use them on their own jobs.

The fixture generator (tests/golden/gen_fix_blend.py) builds its inputs
through blend_case() / diffwtd_case() / wedge_case() / obmc_case() too, so
generator and tests read a case the same way.
"""
import numpy as np


def _i(a):
    return np.asarray(a).astype(np.int64)


def rpot(v, n):
    """ROUND_POWER_OF_TWO: an arithmetic shift of a possibly negative value."""
    return (v + ((1 << n) >> 1)) >> n


# ------------------------------------------------------------------ blend --
def blend_a64(m, a, b):
    return (_i(m) * _i(a) + (64 - _i(m)) * _i(b) + 32) >> 6


def mask_2d(mask, subw, subh):
    """The h x w mask of a (h << subh) x (w << subw) window: the rounded mean of
    2x2, AOM_BLEND_AVG of a pair, or the window itself."""
    m = _i(mask)
    if subw and subh:
        return (m[..., 0::2, 0::2] + m[..., 1::2, 0::2] + m[..., 0::2, 1::2] +
                m[..., 1::2, 1::2] + 2) >> 2
    if subw:
        return (m[..., :, 0::2] + m[..., :, 1::2] + 1) >> 1
    if subh:
        return (m[..., 0::2, :] + m[..., 1::2, :] + 1) >> 1
    return m


def blend_a64_mask(src0, src1, mask, subw=0, subh=0):
    return blend_a64(mask_2d(mask, subw, subh), src0, src1)


def blend_a64_hmask(src0, src1, mask):
    """mask: [w] (or [n, w])."""
    return blend_a64(_i(mask)[..., None, :], src0, src1)


def blend_a64_vmask(src0, src1, mask):
    """mask: [h] (or [n, h])."""
    return blend_a64(_i(mask)[..., :, None], src0, src1)


def d16_rounding(round_0, round_1, bd):
    """(round_offset, round_bits) of the d16 forms (blend_a64_mask.c:43-47)."""
    ob = bd + 14 - round_0
    return (1 << (ob - round_1)) + (1 << (ob - round_1 - 1)), 14 - round_0 - round_1


def blend_a64_d16_mask(src0, src1, mask, subw, subh, round_0, round_1, bd):
    """A plain >> 6 in the blend, one rounding at the end, clip to bd bits."""
    m = mask_2d(mask, subw, subh)
    roff, rbits = d16_rounding(round_0, round_1, bd)
    res = ((m * _i(src0) + (64 - m) * _i(src1)) >> 6) - roff
    return np.clip(rpot(res, rbits), 0, (1 << bd) - 1)


# ---------------------------------------------------------------- diffwtd --
DIFFWTD_38, DIFFWTD_38_INV = 0, 1


def _diffwtd(diff, mask_type):
    m = np.minimum(38 + diff // 16, 64)
    inv = _i(mask_type)
    if inv.ndim:
        inv = inv[..., None, None]
    return np.where(inv != 0, 64 - m, m)


def diffwtd_mask(src0, src1, mask_type, bd=8):
    """av1_build_compound_diffwtd_mask (bd 8) / _highbd: >> (bd - 8) first."""
    return _diffwtd(np.abs(_i(src0) - _i(src1)) >> (bd - 8), mask_type)


def diffwtd_mask_d16(src0, src1, mask_type, round_0, round_1, bd):
    return _diffwtd(rpot(np.abs(_i(src0) - _i(src1)), 14 - round_0 - round_1 + bd - 8), mask_type)


def masked_inter_predictor_d16(src0, src1, mask_type, round_0, round_1, bd):
    """The arithmetic of av1_make_masked_inter_predictor for COMPOUND_DIFFWTD on
    two first-pass CONV_BUF blocks: (mask, prediction)."""
    m = diffwtd_mask_d16(src0, src1, mask_type, round_0, round_1, bd)
    return m, blend_a64_d16_mask(src0, src1, m, 0, 0, round_0, round_1, bd)


# ------------------------------------------------------------------- OBMC --
OBMC_LENGTHS = (1, 2, 4, 8, 16, 32, 64)


def obmc_mask(table, n):
    """av1_get_obmc_mask(n) out of the 127-byte table (length n at n - 1)."""
    return _i(table)[n - 1:2 * n - 1]


def _bits(mask, n):
    return np.array([(int(mask) >> k) & 1 for k in range(n)], bool)


def obmc_wsrc(src, above, left, above_mask, left_mask, table):
    """calc_target_weighted_pred: (wsrc, mask) of a bw x bh block.  above /
    left: the neighbours' predictions as bh x bw arrays at the block's own
    position (only the selected pixels matter)."""
    src, above, left = _i(src), _i(above), _i(left)
    bh, bw = src.shape
    ovh, ovw = min(bh, 64) // 2, min(bw, 64) // 2
    y, x = np.indices((bh, bw))
    a = _bits(above_mask, 32)[x >> 2] & (y < ovh)
    lf = _bits(left_mask, 32)[y >> 2] & (x < ovw)
    mv = np.zeros(bh, np.int64)
    mv[:ovh] = obmc_mask(table, ovh)
    mh = np.zeros(bw, np.int64)
    mh[:ovw] = obmc_mask(table, ovw)
    wsrc = np.where(a, (64 - mv[y]) * above, 0) * 64
    mask = np.where(a, mv[y], 64) * 64
    wsrc = np.where(lf, (wsrc >> 6) * mh[x] + (left << 6) * (64 - mh[x]), wsrc)
    mask = np.where(lf, (mask >> 6) * mh[x], mask)
    return src * 4096 - wsrc, mask


def skip_u4x4_above(pw, ph):
    """av1_skip_u4x4_pred_in_obmc(., ., 0): BLOCK_4X4 / 8X4 / 4X8 planes."""
    return (pw, ph) in ((4, 4), (8, 4), (4, 8))


def obmc_blend(dst, above, left, above_mask, left_mask, bw, bh, ssx, ssy, table):
    """av1_build_obmc_inter_prediction on one plane: dst, above, left are the
    plane's (bh >> ssy) x (bw >> ssx) arrays; vmask first, then hmask on it."""
    d, above, left = _i(dst).copy(), _i(above), _i(left)
    ph, pw = d.shape
    assert (pw, ph) == (bw >> ssx, bh >> ssy)
    ovh, ovw = (min(bh, 64) // 2) >> ssy, (min(bw, 64) // 2) >> ssx
    y, x = np.indices((ph, pw))
    a = _bits(above_mask, 32)[(x << ssx) >> 2] & (y < ovh) & (not skip_u4x4_above(pw, ph))
    lf = _bits(left_mask, 32)[(y << ssy) >> 2] & (x < ovw)
    mv = np.zeros(ph, np.int64)
    mv[:ovh] = obmc_mask(table, ovh)
    mh = np.zeros(pw, np.int64)
    mh[:ovw] = obmc_mask(table, ovw)
    d = np.where(a, blend_a64(mv[y], d, above), d)
    return np.where(lf, blend_a64(mh[x], d, left), d)


# The scenes of the fixture's OBMC cases: the current block (bw x bh at mi
# position (mi_row, mi_col)) in a frame of mi_rows x mi_cols, and the blocks
# in the mi row above / mi column left of it, in order from the block's own
# first column / row: (width, height, is_inter).  nplanes 3: 4:2:0 chroma too.
def _scene(name, bw, bh, above, left, up=1, lf=1, mi_row=32, mi_col=32, mi_rows=96, mi_cols=96,
           bd=8, nplanes=1):
    return dict(name=name, bw=bw, bh=bh, above=above, left=left, up=up, lf=lf, mi_row=mi_row,
                mi_col=mi_col, mi_rows=mi_rows, mi_cols=mi_cols, bd=bd, nplanes=nplanes)


OBMC_SCENES = [
    _scene("8x8", 8, 8, [(8, 8, 1)], [(8, 8, 1)], nplanes=3),
    _scene("8x32", 8, 32, [(16, 16, 1)], [(8, 8, 1), (8, 16, 0), (8, 8, 1)]),
    _scene("32x8", 32, 8, [(8, 8, 1), (16, 8, 1), (8, 8, 0)], [(32, 32, 1)]),
    _scene("16x16", 16, 16, [(8, 8, 1), (8, 8, 1)], [(8, 8, 0), (8, 8, 1)], nplanes=3),
    _scene("64x16", 64, 16, [(16, 16, 1), (32, 16, 0), (16, 16, 1)], [(64, 64, 1)]),
    _scene("128x128", 128, 128, [(64, 64, 1), (32, 32, 1), (32, 32, 0)],
           [(64, 64, 0), (32, 32, 1), (16, 16, 1), (16, 16, 1)]),
    # 4-wide neighbours: the mi_step == 1 pair path (the second of a pair decides)
    _scene("16x16_4wide", 16, 16, [(4, 8, 0), (4, 8, 1), (4, 16, 1), (4, 16, 0)],
           [(8, 4, 1), (8, 4, 0), (16, 4, 0), (16, 4, 1)]),
    # eight 8-wide neighbours above a 64-wide block: max_neighbor_obmc cuts the walk at 4
    _scene("64x64_8wide", 64, 64, [(8, 8, 1)] * 8, [(8, 8, 1)] * 3 + [(8, 8, 0)] + [(8, 8, 1)] * 4),
    # cut by the frame's right and bottom edge: 8 of 16 mi columns / rows inside
    _scene("64x64_edge", 64, 64, [(16, 16, 1)] * 4, [(16, 16, 1)] * 4, mi_row=88, mi_col=88),
    # an intra neighbour between two inter ones
    _scene("32x32_intra_mid", 32, 32, [(8, 8, 1), (16, 16, 0), (8, 8, 1)],
           [(8, 8, 1), (8, 16, 0), (8, 8, 1)], nplanes=3),
    _scene("16x16_no_up", 16, 16, [(16, 16, 1)], [(16, 16, 1)], up=0),
    _scene("16x16_no_left", 16, 16, [(16, 16, 1)], [(16, 16, 1)], lf=0),
    _scene("16x16_bd10", 16, 16, [(8, 8, 1), (8, 8, 0)], [(16, 16, 1)], bd=10, nplanes=3),
    _scene("32x16_bd12", 32, 16, [(32, 32, 1)], [(8, 8, 1), (8, 8, 1)], bd=12),
    _scene("8x8_bd12", 8, 8, [(8, 8, 1)], [(8, 8, 1)], bd=12, nplanes=3),
    # 16x8 / 8x16: 8x4 and 4x8 chroma blocks take the av1_skip_u4x4_pred_in_obmc skip
    _scene("16x8", 16, 8, [(8, 8, 1), (8, 8, 1)], [(8, 8, 1)], nplanes=3),
    _scene("8x16", 8, 16, [(8, 8, 1)], [(8, 8, 1), (8, 8, 0)], nplanes=3),
]
# max_neighbor_obmc (av1/common/blockd.h), by log2 of the block's mi width / height
MAX_NEIGHBOR_OBMC = [0, 1, 2, 3, 4, 4]


def _walk(n_mi, pos, end_frame, nbrs, dim):
    """foreach_overlappable_nb_above / _left along one side: the bitmap of the
    block's mi columns (rows) under a visited neighbour.  nbrs: the blocks
    along the side from the block's first mi, (w, h, inter); dim 0: widths."""
    cells = []
    for nb in nbrs:
        cells += [nb] * (nb[dim] // 4)
    cells += [(64, 64, 0)] * 32
    nb_max = MAX_NEIGHBOR_OBMC[n_mi.bit_length() - 1]
    end = min(pos + n_mi, end_frame)
    bits, count, k = 0, 0, pos
    while k < end and count < nb_max:
        cell = cells[k - pos]
        step = min(cell[dim] // 4, 16)
        if step == 1:
            k &= ~1
            cell = cells[k + 1 - pos]
            step = 2
        if cell[2]:
            count += 1
            for q in range(min(n_mi, step)):
                bits |= 1 << (k - pos + q)
        k += step
    return bits


def scene_bitmaps(sc):
    """(above_mask, left_mask) of a scene: what a caller's visitor records."""
    above = _walk(sc["bw"] // 4, sc["mi_col"], sc["mi_cols"], sc["above"], 0) if sc["up"] else 0
    left = _walk(sc["bh"] // 4, sc["mi_row"], sc["mi_rows"], sc["left"], 1) if sc["lf"] else 0
    return above, left


# ------------------------------------------------------------------ wedge --
def wedge_delta_squares(a, b):
    return np.clip(_i(a) * _i(a) - _i(b) * _i(b), -32768, 32767)


def wedge_sse_terms(r1, d, m):
    return np.clip(64 * _i(r1) + _i(m) * _i(d), -32768, 32767)


def wedge_sse_from_residuals(r1, d, m):
    t = wedge_sse_terms(r1, d, m)
    return (int((t * t).sum()) + 2048) >> 12


def wedge_sign_acc(ds, m):
    return int((_i(ds) * _i(m)).sum())


def wedge_sign_from_residuals(ds, m, limit):
    return int(wedge_sign_acc(ds, m) > int(limit))


# ---------------------------------------------------------------- fixture --
A_STRIDE, B_STRIDE, MASK_STRIDE = 141, 152, 273
PLANE_ROWS, MASK_ROWS = 131, 258
F_MASK, F_HMASK, F_VMASK, F_D16 = range(4)
# variant: 0 the stored planes; 1 / 2 mask all 0 / all 64; 3 every input at the
# maximum (pixels 2^bd - 1, d16 the top of the first-pass range); 4 d16 inputs
# at the bottom of that range; 5 src0 at the top and src1 at the bottom; 6
# src1 equal to src0
B_COLS = ["form", "w", "h", "subw", "subh", "bd", "highbd", "variant", "s0_off", "s1_off", "m_off",
          "r0", "r1", "out_off"]
D_COLS = ["form", "w", "h", "bd", "mask_type", "variant", "s0_off", "s1_off", "r0", "r1",
          "out_off"]  # form 0 u8, 1 highbd, 2 d16
W_COLS = ["kind", "n", "a_off", "b_off", "m_off", "variant", "limit", "ret"]
O_COLS = ["scene", "plane", "ssx", "ssy", "above_mask", "left_mask", "src_off", "above_off",
          "left_off", "wsrc_off", "pred_off"]


class Case:
    def __init__(self, cols, row):
        for k, v in zip(cols, row):
            setattr(self, k, int(v))


def win(plane, off, stride, h, w):
    idx = off + np.arange(h)[:, None] * stride + np.arange(w)[None, :]
    return _i(np.asarray(plane).reshape(-1)[idx])


def _sources(F, c, d16):
    pre = "d" if d16 else "p"
    mx = (1 << c.bd) - 1
    lo, hi = (int(v) for v in F["d16_range"][(c.bd - 8) // 2]) if d16 else (0, mx)
    s0 = win(F["%sa_bd%d" % (pre, c.bd)], c.s0_off, A_STRIDE, c.h, c.w)
    s1 = win(F["%sb_bd%d" % (pre, c.bd)], c.s1_off, B_STRIDE, c.h, c.w)
    if c.variant == 3:
        s0, s1 = np.full_like(s0, hi), np.full_like(s1, hi)
    elif c.variant == 4:
        s0, s1 = np.full_like(s0, lo), np.full_like(s1, lo)
    elif c.variant == 5:
        s0, s1 = np.full_like(s0, hi), np.full_like(s1, lo)
    elif c.variant == 6:
        s1 = s0.copy()
    return s0, s1


def blend_case(F, row):
    """Inputs of one blend case: c.s0, c.s1 (h x w), c.mask (the 2-D window or
    the 1-D mask)."""
    c = Case(B_COLS, row)
    c.s0, c.s1 = _sources(F, c, c.form == F_D16)
    if c.form == F_HMASK:
        c.mask = _i(F["mask1d"][c.m_off:c.m_off + c.w])
    elif c.form == F_VMASK:
        c.mask = _i(F["mask1d"][c.m_off:c.m_off + c.h])
    else:
        c.mask = win(F["mask2d"], c.m_off, MASK_STRIDE, c.h << c.subh, c.w << c.subw)
    if c.variant in (1, 2):
        c.mask = np.full_like(c.mask, 0 if c.variant == 1 else 64)
    return c


def blend_expected(c):
    if c.form == F_HMASK:
        return blend_a64_hmask(c.s0, c.s1, c.mask)
    if c.form == F_VMASK:
        return blend_a64_vmask(c.s0, c.s1, c.mask)
    if c.form == F_D16:
        return blend_a64_d16_mask(c.s0, c.s1, c.mask, c.subw, c.subh, c.r0, c.r1, c.bd)
    return blend_a64_mask(c.s0, c.s1, c.mask, c.subw, c.subh)


def diffwtd_case(F, row):
    c = Case(D_COLS, row)
    c.s0, c.s1 = _sources(F, c, c.form == 2)
    return c


def diffwtd_expected(c):
    if c.form == 2:
        return diffwtd_mask_d16(c.s0, c.s1, c.mask_type, c.r0, c.r1, c.bd)
    return diffwtd_mask(c.s0, c.s1, c.mask_type, c.bd)


def wedge_case(F, row):
    """c.a, c.b (int16 streams), c.m (u8 mask), each of n elements.
    variant 0: 8-bit-range residuals (res8_*), 1: 12-bit-range (res12_*),
    2: residuals at +-4095 with masks that clamp most terms."""
    c = Case(W_COLS, row)
    pre = "res8" if c.variant == 0 else "res12"
    c.a = _i(F[pre + "_a"][c.a_off:c.a_off + c.n])
    c.b = _i(F[pre + "_b"][c.b_off:c.b_off + c.n])
    c.m = _i(F["wedge_m"][c.m_off:c.m_off + c.n])
    if c.variant == 2:
        sgn = np.where(np.arange(c.n) & 1, -1, 1)
        c.a, c.b = 4095 * sgn, -4095 * sgn * np.where(np.arange(c.n) & 2, 1, -1)
    return c


def wedge_expected(c):
    if c.kind == 0:
        return wedge_delta_squares(c.a, c.b)
    if c.kind == 1:
        return wedge_sse_from_residuals(c.a, c.b, c.m)
    return wedge_sign_from_residuals(c.a, c.m, c.limit)


def obmc_case(F, row):
    """Inputs of one OBMC case row: the plane's src / dst, above and left
    blocks and the scene."""
    c = Case(O_COLS, row)
    c.sc = OBMC_SCENES[c.scene]
    bd = c.sc["bd"]
    c.pw, c.ph = c.sc["bw"] >> c.ssx, c.sc["bh"] >> c.ssy
    c.src = win(F["pa_bd%d" % bd], c.src_off, A_STRIDE, c.ph, c.pw)
    c.above = win(F["pb_bd%d" % bd], c.above_off, B_STRIDE, c.ph, c.pw)
    c.left = win(F["pb_bd%d" % bd], c.left_off, B_STRIDE, c.ph, c.pw)
    return c


SIZES = [(4, 4), (4, 16), (16, 4), (8, 8), (64, 32), (128, 128)]
SMALL = [(2, 2), (1, 4), (1, 16), (2, 8), (8, 2)]  # the chroma OBMC spans and 2x2
SUBS = [(0, 0), (1, 1), (1, 0), (0, 1)]
WEDGE_SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (8, 32), (32, 8)]


# --------------------------------------------------------------- coverage --
def coverage_problems(F):
    """What the fixture must contain (an empty list: all there)."""
    bad = []

    def need(ok, what):
        if not ok:
            bad.append(what)
    B = F["blend_cases"]
    col = {k: B[:, i] for i, k in enumerate(B_COLS)}
    sizes = {(w, h) for w, h in B[:, 1:3]}
    need(sizes >= set(SIZES) | set(SMALL), "blend sizes")
    for form in (F_MASK, F_D16):
        need({(a, b) for a, b in B[col["form"] == form][:, 3:5]} == set(SUBS),
             "blend sub forms of form %d" % form)
    need({1, 2} <= set(col["variant"]), "blend masks all 0 / all 64")
    need((F["mask2d"] == 0).any() and (F["mask2d"] == 64).any(), "mask plane ends")
    pix = col["form"] != F_D16
    need({8, 10, 12} <= set(col["bd"][pix & (col["variant"] == 3)]), "all-maximum pixel inputs")
    for r0, bd in ((3, 8), (3, 10), (5, 12)):
        got = set(col["variant"][(col["form"] == F_D16) & (col["bd"] == bd) & (col["r0"] == r0)])
        need({3, 4, 5} <= got, "d16 range ends at bd %d round_0 %d" % (bd, r0))
    D = F["dw_cases"]
    dcol = {k: D[:, i] for i, k in enumerate(D_COLS)}
    need({(f, bd, mt) for f, bd, mt in D[:, [0, 3, 4]]} >=
         {(f, bd, mt) for mt in (0, 1) for f, bd in ((0, 8), (1, 8), (1, 10), (1, 12), (2, 8),
                                                     (2, 10), (2, 12))}, "diffwtd forms")
    outs = {}
    for row in D:
        c = Case(D_COLS, row)
        o = F["dw_out"][c.out_off:c.out_off + c.w * c.h]
        outs.setdefault((c.form, c.variant, c.mask_type), set()).update(np.unique(o).tolist())
    need(outs.get((2, 5, 0)) == {64} and outs.get((2, 5, 1)) == {0}, "diffwtd clamps at 64")
    need(outs.get((2, 6, 0)) == {38} and outs.get((1, 6, 1)) == {26}, "diffwtd stays at 38")
    need({int(v) for v in dcol["bd"][dcol["form"] == 2]} == {8, 10, 12}, "diffwtd d16 bit depths")
    O = F["obmc_cases"]
    names = {OBMC_SCENES[int(s)]["name"] for s in O[:, 0]}
    need(names == {sc["name"] for sc in OBMC_SCENES}, "OBMC scenes")
    blocks = {(sc["bw"], sc["bh"]) for sc in OBMC_SCENES}
    need(blocks >= {(8, 8), (8, 32), (32, 8), (16, 16), (64, 16), (128, 128)}, "OBMC blocks")
    by = {OBMC_SCENES[int(r[0])]["name"]: r for r in O if r[1] == 0}
    am = lambda nm: int(by[nm][4])
    lm = lambda nm: int(by[nm][5])
    need(am("16x16_4wide") == 0b0011 and lm("16x16_4wide") == 0b1100, "pair path bitmaps")
    need(am("64x64_8wide") == 0x00FF and lm("64x64_8wide") == 0x033F, "max_neighbor_obmc cut")
    need(am("64x64_edge") == 0x00FF and lm("64x64_edge") == 0x00FF, "frame edge cut")
    need(am("32x32_intra_mid") == 0b11000011, "intra neighbour between two inter ones")
    need(am("16x16_no_up") == 0 and lm("16x16_no_up") == 0xF, "up_available off")
    need(lm("16x16_no_left") == 0 and am("16x16_no_left") == 0xF, "left_available off")
    need({sc["bd"] for sc in OBMC_SCENES} == {8, 10, 12}, "OBMC bit depths")
    need(all((int(r[4]), int(r[5])) == scene_bitmaps(OBMC_SCENES[int(r[0])]) for r in O),
         "recorded bitmaps equal the restated walk")
    chroma = {OBMC_SCENES[int(r[0])]["name"] for r in O if r[1] == 1}
    need(chroma >= {"8x8", "16x8", "8x16", "16x16", "32x32_intra_mid"}, "OBMC chroma planes")
    W = F["wedge_cases"]
    need({int(v) for v in W[:, 1]} == {64, 128, 1024, 16384}, "wedge N")
    frac = {}
    for row in W:
        c = wedge_case(F, row)
        if c.kind == 1:
            t = 64 * c.a + c.m * c.b
            frac.setdefault(c.variant, []).append(float((np.abs(t) > 32767).mean()))
        if c.kind == 0 and c.variant == 1:
            d = wedge_delta_squares(c.a, c.b)
            need((d == 32767).any() and (d == -32768).any(), "delta squares saturate on both sides")
    need(max(frac[1]) >= 0.1 and max(frac[0]) == 0.0, "sse clamp engaged / never engaged")
    eq = [r for r in W if r[0] == 2 and wedge_sign_acc(wedge_case(F, r).a,
                                                          wedge_case(F, r).m) == r[6]]
    need(eq and all(r[7] == 0 for r in eq), "sign with acc == limit")
    need(len(F["obmc_masks"]) == 127, "obmc mask table")
    need(all("wedge_masks_%dx%d" % s in F for s in WEDGE_SIZES), "wedge masks")
    return bad
