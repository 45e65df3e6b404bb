"""numpy restatement of the plain pixel kinds of csrc/pixel.hip (aom_dsp/sad.c,
variance.c:38-55,123-298,321-560, sse.c, subtract.c, sum_squares.c,
blk_sse_sum.c, avg.c:102-524, av1/encoder/rdopt.c:635-682) in int64, and the
seeded planes / job lists the packed-kernel tests run on.

Blocks are 2-D integer arrays; a "filtered" operand is the (h + 1) x (w + 1)
window the bilinear filter reads.  Every function also takes a stack of blocks
([n, h, w], per-block parameters as [n] arrays) and then returns [n] results.
Nothing here comes from oracle/: test_pixel_batch_cpu.py pins every function
to tests/golden/fix_pixel.npz (the reference's own outputs) and to the C
oracle, and test_gpu_pixel_batch.py then uses them as the expected values.
"""
import numpy as np

M32 = 0xFFFFFFFF

SIZES = [(128, 128), (128, 64), (64, 128), (64, 64), (64, 32), (32, 64), (32, 32), (32, 16),
         (16, 32), (16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4), (4, 16), (16, 4),
         (8, 32), (32, 8), (16, 64), (64, 16)]
# (bit depth, highbd): 8 bits both as bytes and as 16-bit samples
CONFIGS = [(8, False), (8, True), (10, True), (12, True)]


def _i(a):
    return np.asarray(a).astype(np.int64)


def _b(v):
    """A per-block parameter (scalar or [n]) shaped to broadcast over h x w."""
    return _i(v)[..., None, None]


def _sum(a):
    return a.sum(axis=(-2, -1))


def s32(v):
    """An int64 value wrapped to C's int."""
    return ((_i(v) + (1 << 31)) & M32) - (1 << 31)


def s16(v):
    return ((_i(v) + 0x8000) & 0xFFFF) - 0x8000


# -------------------------------------------------------------------- SAD --
def sad(src, ref):
    return _sum(np.abs(_i(src) - _i(ref))) & M32


def sad_skip(src, ref):
    """2 x the SAD of the even rows (sad.c:73-78, 118-123)."""
    return (2 * sad(_i(src)[..., ::2, :], _i(ref)[..., ::2, :])) & M32


def avg_pred(ref, pred):
    return (_i(pred) + _i(ref) + 1) >> 1


def sad_avg(src, ref, second):
    return sad(src, avg_pred(ref, second))


# --------------------------------------------------------------- variance --
def variance_tail(sum64, sse64, bd, n):
    """(var, sse, sum) as the callers see them, from the exact sums.  8 bits
    (lowbd and highbd_8): sse and sum truncate to 32 bits and var wraps as
    uint32.  10 / 12 bits: highbd_variance64's sums are rounded, (x + half) >>
    2 / 4 for the signed sum (an arithmetic shift), >> 4 / 8 for sse, and the
    variance is clamped at 0 (variance.c:361-408)."""
    sum64, sse64 = _i(sum64), _i(sse64)
    if bd == 8:
        sse, sm = sse64 & M32, s32(sum64)
        return (sse - (((sm * sm) // n) & M32)) & M32, sse, sm
    sh, ss = (2, 4) if bd == 10 else (4, 8)
    sse = ((sse64 + (1 << (ss - 1))) >> ss) & M32
    sm = s32((sum64 + (1 << (sh - 1))) >> sh)
    return np.maximum(0, before_clamp(sse, sm, n)), sse, sm


def before_clamp(sse, sm, n):
    """sse_rounded - sum_rounded^2 / N, the int64 the 10 / 12-bit forms clamp."""
    return _i(sse) - (_i(sm) * _i(sm)) // n


def sums(a, b):
    """(sum, sse) of a - b, exact."""
    d = _i(a) - _i(b)
    return _sum(d), _sum(d * d)


def variance(a, b, bd=8):
    """(var, sse, sum) of aom[_highbd_bd]_variance / mse (returns sse) /
    get_var (sse, sum)."""
    sm, ss = sums(a, b)
    return variance_tail(sm, ss, bd, np.shape(a)[-2] * np.shape(a)[-1])


def sse(a, b):
    """aom_sse / aom_highbd_sse: the exact int64 sum."""
    return sums(a, b)[1]


def bilinear(win, xoff, yoff, highbd=False):
    """(h+1) x (w+1) window -> h x w: the rounded first pass (uint16) and the
    second pass stored as uint8 / uint16 (variance.c:73-121, 454-494)."""
    win = _i(win)
    h, w = win.shape[-2] - 1, win.shape[-1] - 1
    f1, g1 = 16 * _b(xoff), 16 * _b(yoff)
    f0, g0 = 128 - f1, 128 - g1
    hp = ((win[..., :, :w] * f0 + win[..., :, 1:w + 1] * f1 + 64) >> 7) & 0xFFFF
    return ((hp[..., :h, :] * g0 + hp[..., 1:h + 1, :] * g1 + 64) >> 7) & (0xFFFF if highbd
                                                                           else 0xFF)


def sub_pixel_variance(win, xoff, yoff, b, bd=8, highbd=False, second=None):
    """(var, sse, sum) of the filtered window against b; with `second` the
    filtered block is first averaged with it (sub_pixel_avg_variance)."""
    a = bilinear(win, xoff, yoff, highbd)
    if second is not None:
        a = avg_pred(a, second)
    return variance(a, b, bd)


# ------------------------------------------------- residuals and their sums --
def subtract(src, pred):
    return (_i(src) - _i(pred)).astype(np.int16)


def sum_squares_2d_i16(x):
    x = _i(x)
    return _sum(x * x)


def sum_sse_2d_i16(x, sum_in=0):
    """(sse, *sum after the call): the sum is added into an int."""
    x = _i(x)
    return _sum(x * x), s32(_i(sum_in) + _sum(x))


def get_blk_sse_sum(x):
    """(x_sum as int, x2_sum as int64)."""
    x = _i(x)
    return s32(_sum(x)), _sum(x * x)


# --------------------------------------------------------------- Hadamard --
def _col4(x, t):
    """hadamard_col4 down axis -2 of [..., 4, c]."""
    s = [x[..., k, :] for k in range(4)]
    b0, b1 = t((s[0] + s[1]) >> 1), t((s[0] - s[1]) >> 1)
    b2, b3 = t((s[2] + s[3]) >> 1), t((s[2] - s[3]) >> 1)
    return np.stack([t(b0 + b2), t(b1 + b3), t(b0 - b2), t(b1 - b3)], -2)


def _col8(x, t):
    """hadamard_col8 down axis -2 of [..., 8, c], outputs in the reference's
    order (avg.c:147-175)."""
    s = [x[..., k, :] for k in range(8)]
    b = []
    for k in range(4):
        b += [t(s[2 * k] + s[2 * k + 1]), t(s[2 * k] - s[2 * k + 1])]
    c = [t(b[0] + b[2]), t(b[1] + b[3]), t(b[0] - b[2]), t(b[1] - b[3]),
         t(b[4] + b[6]), t(b[5] + b[7]), t(b[4] - b[6]), t(b[5] - b[7])]
    o = [None] * 8
    o[0], o[7], o[3], o[4] = t(c[0] + c[4]), t(c[1] + c[5]), t(c[2] + c[6]), t(c[3] + c[7])
    o[2], o[6], o[1], o[5] = t(c[0] - c[4]), t(c[1] - c[5]), t(c[2] - c[6]), t(c[3] - c[7])
    return np.stack(o, -2)


def _wide(v):
    return v


def _small(x, n, highbd, t):
    """[..., n, n] -> [..., n * n].  Pass 1 transforms the columns of the block
    into the rows of `buffer`; pass 2 transforms buffer's columns into the rows
    of buffer2.  lowbd: int16 throughout, and the "extra transpose" on the way
    out; highbd 8x8: an int32 second pass and no transpose."""
    col = _col4 if n == 4 else _col8
    buf = np.swapaxes(col(x, t), -1, -2)
    b2 = col(buf, _wide if highbd else t)
    out = np.swapaxes(b2, -1, -2) if highbd else b2
    return out.reshape(out.shape[:-2] + (n * n,))


def _quads(x, m):
    """The four m x m quadrants of [..., 2m, 2m] in the reference's idx order."""
    return [x[..., (i >> 1) * m:(i >> 1) * m + m, (i & 1) * m:(i & 1) * m + m] for i in range(4)]


def _combine(a, shift, t):
    """The 16x16 / 32x32 stage over [..., 4, len] (avg.c:258-275, 329-346)."""
    b0, b1 = t((a[..., 0, :] + a[..., 1, :]) >> shift), t((a[..., 0, :] - a[..., 1, :]) >> shift)
    b2, b3 = t((a[..., 2, :] + a[..., 3, :]) >> shift), t((a[..., 2, :] - a[..., 3, :]) >> shift)
    out = np.stack([t(b0 + b2), t(b1 + b3), t(b0 - b2), t(b1 - b3)], -2)
    return out.reshape(out.shape[:-2] + (-1,))


def _had(x, n, highbd, lp, wide):
    t = _wide if wide else s16
    if n <= 8:
        return _small(x, n, highbd, t)
    if n == 16:
        a = np.stack([_small(q, 8, highbd, t) for q in _quads(x, 8)], -2)
        # the lp form keeps int16 in the combine; the others use tran_low_t
        c = _combine(a, 1, t if lp else _wide)
        if not highbd and not lp:  # the 4-wide group swap of the lowbd form (avg.c:278-286)
            c = c.reshape(c.shape[:-1] + (16, 16)).copy()
            c[..., 4:8], c[..., 8:12] = c[..., 8:12].copy(), c[..., 4:8].copy()
            c = c.reshape(c.shape[:-2] + (256,))
        return c
    a = np.stack([_had(q, 16, highbd, lp, wide) for q in _quads(x, 16)], -2)
    return _combine(a, 2, _wide)


def hadamard(x, n, highbd=False, wide=False):
    """aom[_highbd]_hadamard_{n}x{n} of [..., n, n] residuals -> [..., n * n]
    int32 coefficients.  wide: the same butterflies without the int16 wrap of
    the intermediates (what the reference would give were they wider)."""
    assert n in (4, 8, 16, 32) and not (highbd and n == 4)
    return _had(_i(x), n, highbd, False, wide)


def hadamard_lp(x, n, wide=False):
    """aom_hadamard_lp_{8x8,16x16}: int16 coefficients."""
    assert n in (8, 16)
    return _had(_i(x), n, False, True, wide)


def satd(coeff):
    """aom_satd / aom_satd_lp over the last axis: an int sum."""
    return s32(np.abs(_i(coeff)).sum(-1))


satd_lp = satd


def block_error(coeff, dqcoeff, bd=None):
    """(error, ssz) over the last axis.  bd None: av1_block_error, whose
    squares are int products (wrapping) added to int64 sums; 8 / 10 / 12:
    av1_highbd_block_error, exact, rounded down by 2 * (bd - 8) bits."""
    c, d = _i(coeff), _i(dqcoeff)
    if bd is None:
        df = s32(c - d)
        return s32(df * df).sum(-1), s32(c * c).sum(-1)
    shift = 2 * (bd - 8)
    rnd = (1 << (shift - 1)) if shift else 0
    df = c - d
    return ((df * df).sum(-1) + rnd) >> shift, ((c * c).sum(-1) + rnd) >> shift


def block_error_lp(coeff, dqcoeff):
    df = _i(coeff) - _i(dqcoeff)
    return s32(df * df).sum(-1)


# ------------------------------------------------------ planes and job lists --
PH, PW = 264, 328
POOL = 16  # distinct second_pred blocks
# job indices that address the built-in edge blocks (cells of a 2 x 2 grid of
# (h + 1) x (w + 1) areas at row 1, column 1 of both planes)
J_MAX0, J_0MAX, J_NEG, J_CHECK = 0, 2, 3, 4
J_MAX0_B, J_NEG_B = 66, 258


def windows(plane, offs, h, w):
    """[n, h, w] windows of a 2-D plane at element offsets."""
    idx = np.arange(h)[:, None] * plane.shape[1] + np.arange(w)[None, :]
    return plane.reshape(-1)[np.asarray(offs)[:, None, None] + idx[None]]


def blocks(pool, offs, h, w):
    """[n, h, w] contiguous blocks of a 1-D pool at element offsets."""
    return pool[np.asarray(offs)[:, None] + np.arange(w * h)[None]].reshape(-1, h, w)


def neg_clamp_diffs(w, h, bd):
    """(d, k): a block whose differences are d + 1 in k pixels and d in the
    other w * h - k has a negative 10 / 12-bit variance before the clamp: the
    true variance is below one rounding step of sse, and the rounded sum comes
    out larger than the exact one.  The smallest d, then k, that does it."""
    n = w * h
    for d in range(1, 64):
        for k in range(0, min(n, 64) + 1):
            sm, ss = n * d + k, (n - k) * d * d + k * (d + 1) * (d + 1)
            _, sse_r, sum_r = variance_tail(sm, ss, bd, n)
            if before_clamp(sse_r, sum_r, n) < 0:
                return d, k
    return None


def max_jobs(w, h):
    return 259 if w * h <= 1024 else 67


class Planes:
    """Seeded src / ref planes, a second_pred pool and one job list for a block
    size and bit depth; a test with fewer jobs takes a prefix of the list.
    One pixel in eight is one of {0, 1, max-1, max}; the edge blocks (all-max
    against all-0 and the reverse, the negative-before-clamp block, a 0 / max
    checkerboard against all-0) are pasted into the planes and addressed by
    the J_* jobs, beside ordinary jobs at seeded positions."""

    def __init__(self, w, h, bd, highbd, job_dtype, njobs=None, seed=None):
        self.w, self.h, self.bd, self.hb = w, h, bd, highbd
        self.nj = nj = max_jobs(w, h) if njobs is None else njobs
        rng = np.random.default_rng(w * 131 + h * 7 + bd + 1000 * highbd if seed is None else seed)
        self.dtype = dt = np.uint16 if highbd else np.uint8
        mx = self.mx = (1 << bd) - 1
        pix = lambda shape: np.where(rng.integers(0, 8, shape) == 0,
                                     rng.choice([0, 1, mx - 1, mx], shape),
                                     rng.integers(0, mx + 1, shape)).astype(dt)
        self.src, self.ref = pix((PH, PW)), pix((PH, PW))
        n = w * h
        self.second = pix(POOL * n + 1)
        ch, cw = h + 1, w + 1
        cell = lambda i: (1 + (i >> 1) * ch, 1 + (i & 1) * cw)
        assert 1 + 2 * ch <= PH and 1 + 2 * cw <= PW

        def paste(plane, i, block):
            r, c = cell(i)
            plane[r:r + ch, c:c + cw] = block

        paste(self.src, 0, mx), paste(self.ref, 0, 0)
        paste(self.src, 1, 0), paste(self.ref, 1, mx)
        yy, xx = np.mgrid[0:ch, 0:cw]
        paste(self.src, 3, np.where((yy + xx) & 1, mx, 0)), paste(self.ref, 3, 0)
        self.neg = neg_clamp_diffs(w, h, bd) if bd > 8 else None
        if self.neg:
            d, k = self.neg
            base = rng.integers(0, mx - d, (ch, cw))
            up = np.full((ch, cw), d)
            blk = np.full(n, d)
            blk[:k] += 1  # the first k pixels of the w x h block
            up[:h, :w] = blk.reshape(h, w)
            paste(self.ref, 2, base), paste(self.src, 2, base + up)
        off = lambda i: cell(i)[0] * PW + cell(i)[1]
        jobs = np.zeros(nj, job_dtype)
        # the column leaves room for the forced odd offset and the filter's extra column
        pos = lambda: rng.integers(0, PH - h, nj) * PW + rng.integers(0, PW - w - 1, nj)
        jobs["src_off"] = pos()
        for k in range(4):
            jobs["ref_off"][:, k] = pos()
        special = {J_MAX0: 0, J_0MAX: 1, J_CHECK: 3, J_MAX0_B: 0}
        if self.neg:
            special.update({J_NEG: 2, J_NEG_B: 2})
        for j, i in special.items():
            if j < nj:
                jobs["src_off"][j] = jobs["ref_off"][j, 0] = off(i)
        if nj > 1:
            jobs["src_off"][1] |= 1  # odd element offsets, whatever the seed
            jobs["ref_off"][1] |= 1
        jobs["aux_off"] = rng.integers(0, POOL, nj) * n + 1
        jobs["xoff"] = np.arange(nj) % 8
        jobs["yoff"] = (np.arange(nj) // 8) % 8
        self.jobs = jobs

    # the operands of the first `nj` jobs as [nj, h, w] stacks
    def S(self, nj=None, dw=0):
        return windows(self.src, self.jobs["src_off"][:nj], self.h + dw, self.w + dw)

    def R(self, nj=None, k=0):
        return windows(self.ref, self.jobs["ref_off"][:nj, k], self.h, self.w)

    def P2(self, nj=None):
        return blocks(self.second, self.jobs["aux_off"][:nj], self.h, self.w)


def residual_plane(kind, seed, rows=80, cols=208):
    """int16 residual planes for the Hadamard / sum kernels.  kind "255": the
    lowbd range; "4095": the highbd range; "wrap": the whole int16 range, one
    value in eight an extreme, with a constant 32767 area at (1, 1), a constant
    -32768 area at (1, 40) and a +-32767 checkerboard at (40, 1) (each 33 x 33):
    blocks there wrap the int16 intermediates of the lowbd butterflies."""
    rng = np.random.default_rng(seed)
    if kind != "wrap":
        lim = int(kind)
        return rng.integers(-lim, lim + 1, (rows, cols)).astype(np.int16)
    p = np.where(rng.integers(0, 8, (rows, cols)) == 0,
                 rng.choice([-32768, -32767, 32766, 32767], (rows, cols)),
                 rng.integers(-32768, 32768, (rows, cols))).astype(np.int16)
    p[1:34, 1:34] = 32767
    p[1:34, 40:73] = -32768
    yy, xx = np.mgrid[0:33, 0:33]
    p[40:73, 1:34] = np.where((yy + xx) & 1, 32767, -32767)
    return p


def coeff_rows(length, nblocks, seed):
    """int32 (coeff, dqcoeff) [nblocks, length] within +-2^20; one coefficient
    in eight is +-2^16, +-(2^16 + 1) or +-2^20, whose int square wraps, and
    every fourth row is dequantised to zero (the difference is the coefficient)."""
    rng = np.random.default_rng(seed)
    shape = (nblocks, length)
    big = [-(1 << 20), -65537, -65536, 65536, 65537, 1 << 20]
    c = np.where(rng.integers(0, 8, shape) == 0, rng.choice(big, shape),
                 rng.integers(-(1 << 20), (1 << 20) + 1, shape)).astype(np.int32)
    d = (c + rng.integers(-1000, 1001, shape)).astype(np.int32)
    d[::4] = 0
    return c, d


def coeff_rows_lp(length, nblocks, seed):
    """int16 (coeff, dqcoeff) over the whole range, one in eight an extreme:
    differences reach 65535, whose int square wraps."""
    rng = np.random.default_rng(seed)
    shape = (nblocks, length)
    one = lambda: np.where(rng.integers(0, 8, shape) == 0,
                           rng.choice([-32768, -32767, 32766, 32767], shape),
                           rng.integers(-32768, 32768, shape)).astype(np.int16)
    c, d = one(), one()
    c[0, :2], d[0, :2] = (32767, -32768), (-32768, 32767)
    return c, d


def residual_offsets(plane, h, w, njobs, seed):
    """Element offsets of njobs w x h blocks of a residual plane: the three
    built-in areas first (at odd rows and columns, so no multiple of the block
    size), then seeded positions."""
    rows, cols = plane.shape
    rng = np.random.default_rng(seed)
    offs = rng.integers(0, rows - h, njobs) * cols + rng.integers(0, cols - w, njobs)
    fixed = [1 * cols + 1, 1 * cols + 40, 40 * cols + 1]
    if h <= 33 and w <= 33:
        offs[:min(3, njobs)] = fixed[:njobs]
    return offs
