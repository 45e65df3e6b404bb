"""Inputs that steer the transform kernels between their two arithmetic
paths (test infrastructure, numpy only).

txq_plane_body (csrc/txq_dev.h) and rdo_tile (csrc/rdo_kern.h) run the
certified 24-bit FAST arithmetic for a wave tile whose residual obeys
|x| <= kFastResidualMax (csrc/quant_dev.h), the exact 64-bit path otherwise.
A wave tile is P = 64 / min(W, H) consecutive blocks in raster order; a
txq_plane workgroup holds four consecutive tiles.  The kernels do not report
the path they took, so the tests assert it on their inputs with tile_amax."""
import os
import re

import numpy as np

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTX = [0, 1, 0, 1, 2, 0, 2, 1, 2, 3, 0, 3, 1, 3, 2, 3]  # 0 DCT 1 ADST 2 FLIPADST 3 IDTX
HTX = [0, 0, 1, 1, 0, 2, 2, 2, 1, 3, 3, 0, 3, 1, 3, 2]


def fast_residual_max():
    src = open(os.path.join(ROOT, "aom-av1-lavish_amd", "csrc", "quant_dev.h")).read()
    return int(re.search(r"constexpr\s+int\s+kFastResidualMax\s*=\s*(\d+)\s*;", src).group(1))


def tile_blocks(s):
    return 64 // min(O.TX_W[s], O.TX_H[s])


def tile_amax(res, s):
    """max |residual| of each wave tile of a plane (int array [H, W])."""
    W, H, P = O.TX_W[s], O.TX_H[s], tile_blocks(s)
    bh, bw = res.shape[0] // H, res.shape[1] // W
    a = np.abs(res[:bh * H, :bw * W].astype(np.int64)).reshape(bh, H, bw, W).max(axis=(1, 3))
    a = a.reshape(-1)
    a = np.concatenate([a, np.zeros(-len(a) % P, np.int64)])  # the last tile's missing blocks
    return a.reshape(-1, P).max(axis=1)


def tile_fast(res, s):
    return tile_amax(res, s) <= fast_residual_max()


def plane_shape(s):
    """A plane of ten wave tiles, the last one partial (9 P + max(P / 2, 1)
    blocks), in more than one row of blocks where that divides."""
    P = tile_blocks(s)
    nb = 9 * P + max(P // 2, 1)
    bw = 19 if nb % 19 == 0 else 5
    assert nb % bw == 0 and (P == 1 or nb % P)
    return (nb // bw) * O.TX_H[s], bw * O.TX_W[s]


def block_view(res, s, blk):
    W, H = O.TX_W[s], O.TX_H[s]
    by, bx = divmod(blk, res.shape[1] // W)
    return res[by * H:(by + 1) * H, bx * W:(bx + 1) * W]


def edge_plane(s, seed, T=None):
    """|x| <= T everywhere, and in every tile one sample at +T and one at -T."""
    T = fast_residual_max() if T is None else T
    rng = np.random.default_rng(seed)
    h, w = plane_shape(s)
    res = rng.integers(-T, T + 1, (h, w)).astype(np.int16)
    P = tile_blocks(s)
    nb = (h // O.TX_H[s]) * (w // O.TX_W[s])
    for t in range((nb + P - 1) // P):
        n = min(P, nb - t * P)
        for v in (T, -T):
            b = block_view(res, s, t * P + int(rng.integers(0, n)))
            b[int(rng.integers(0, b.shape[0])), int(rng.integers(0, b.shape[1]))] = v
        blocks = [block_view(res, s, t * P + i) for i in range(n)]
        if not (any((b == T).any() for b in blocks) and any((b == -T).any() for b in blocks)):
            b = blocks[0]
            b[0, 0], b[-1, -1] = T, -T
    return res


def past_edge(res, s, tile, value, seed):
    """A copy of `res` with one sample of one block of wave tile `tile` set
    to `value` (a sample that is not one of the tile's +-T marks)."""
    rng = np.random.default_rng(seed)
    out = res.copy()
    P = tile_blocks(s)
    T = int(np.abs(res.astype(np.int32)).max())
    b = block_view(out, s, tile * P + int(rng.integers(0, P)))
    ys, xs = np.nonzero(np.abs(b.astype(np.int32)) < T)
    k = int(rng.integers(0, len(ys)))
    b[ys[k], xs[k]] = value
    return out


def _basis_signs(kind, n, cos_bit=13):
    """S[u] = the +-1 input pattern that drives output u of the forward 1-D
    transform of `kind` to its largest magnitude: the signs of row u of the
    transform's matrix, read off impulse responses (zero -> +1; FLIPADST is
    ADST of the reversed input)."""
    k = {0: 0, 1: 1, 2: 1, 3: 2}[kind]
    M = np.stack([O.fwd_txfm1d(k, np.eye(n, dtype=np.int32)[i] << 12, cos_bit)
                  for i in range(n)], axis=1)
    S = np.where(M < 0, -1, 1).astype(np.int32)
    return S[:, ::-1] if kind == 2 else S


def adversarial_blocks(s, t, amp, seed=0, nrandom=8):
    """[k, H, W] int16 blocks +-amp * outer(col pattern of output u, row
    pattern of output v) for tx type t of size s: (u, v) the four corners of
    the coefficient block plus `nrandom` seeded outputs, both signs."""
    W, H = O.TX_W[s], O.TX_H[s]
    Sc, Sr = _basis_signs(VTX[t], H), _basis_signs(HTX[t], W)
    rng = np.random.default_rng(seed * 1000 + s * 16 + t)
    uv = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    uv += [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(nrandom)]
    out = []
    for u, v in uv:
        b = amp * np.outer(Sc[u], Sr[v])
        out += [b, -b]
    return np.stack(out).astype(np.int16)


def adversarial_plane(s, types, amp, seed=0, nrandom=8):
    """The adversarial blocks of every type in `types`, laid out as a plane
    of 8 blocks per row (24 per type: whole rows)."""
    W, H = O.TX_W[s], O.TX_H[s]
    blocks = np.concatenate([adversarial_blocks(s, t, amp, seed, nrandom) for t in types])
    n = len(blocks)
    assert n % 8 == 0
    return np.ascontiguousarray(
        blocks.reshape(n // 8, 8, H, W).transpose(0, 2, 1, 3).reshape(n // 8 * H, 8 * W))


def src_pred(res, bd, seed):
    """u16 planes with src - pred == res: pred drawn over the pixel range
    where the range allows the difference (at bd 10 a difference of +-1024
    puts one of the two samples at 1024, one past the range)."""
    rng = np.random.default_rng(seed)
    r = res.astype(np.int64)
    M = (1 << bd) - 1
    lo = np.maximum(0, -r)
    hi = np.maximum(lo, M - np.maximum(r, 0))
    pred = lo + rng.integers(0, 1 << 30, r.shape) % (hi - lo + 1)
    src = pred + r
    assert src.min() >= 0 and ((src - pred) == r).all()
    return src.astype(np.uint16), pred.astype(np.uint16)
