"""numpy float32 restatement of the order-fixed column sums (uniter_colsum_x3_add_det / uniter_colsum_bf16_add_det; the order is
stated in include/uniter_hip.h).  The library is built with -ffp-contract=off and every step below is one IEEE float32 add, so the
GPU result is these bits:

  1. rows are cut into blocks of ROWS = 64 consecutive rows (the last one may be ragged);
  2. inside a block, row-lane w = 0..3 adds rows r0 + w, r0 + w + 4, ... in ascending order, starting from 0;
     an x3 element is (p2 + p1) + p0, a bf16 element is widened;
  3. the block's partial is P = (s0 + s1) + (s2 + s3);
  4. out[c] = out[c] + (((P0 + P1) + P2) + ...), the blocks in ascending index."""
import numpy as np

ROWS = 64      # UNITER_COLSUM_DET_ROWS
F = np.float32


def to_bf16(x):
    """float32 -> the nearest bf16 value (ties to even), returned as float32"""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(F)


def split3(x):
    """float32 [rows, cols] -> three bf16 pieces per value [rows, 3, cols] (as float32): x ~ p0 + p1 + p2, largest first"""
    x = np.asarray(x, dtype=F)
    p0 = to_bf16(x)
    p1 = to_bf16(x - p0)
    p2 = to_bf16((x - p0) - p1)
    return np.stack([p0, p1, p2], axis=1)


def x3_elements(pieces):
    pieces = np.asarray(pieces, dtype=F)
    return (pieces[:, 2] + pieces[:, 1]) + pieces[:, 0]


def block_partials(elems):
    """steps 1-3: [rows, cols] float32 -> [ceil(rows / 64), cols]"""
    elems = np.asarray(elems, dtype=F)
    rows, cols = elems.shape
    nb = (rows + ROWS - 1) // ROWS
    P = np.zeros((nb, cols), dtype=F)
    for k in range(nb):
        blk = elems[ROWS * k:min(rows, ROWS * (k + 1))]
        s = np.zeros((4, cols), dtype=F)
        for w in range(4):
            for r in range(w, blk.shape[0], 4):
                s[w] = s[w] + blk[r]
        P[k] = (s[0] + s[1]) + (s[2] + s[3])
    return P


def finish(P, out, order=None):
    """step 4; `order`: another order of the blocks (the tests' order-sensitivity check), None = ascending"""
    idx = list(range(P.shape[0])) if order is None else list(order)
    t = P[idx[0]].copy()
    for k in idx[1:]:
        t = t + P[k]
    return np.asarray(out, dtype=F) + t


def colsum_bf16_add_det(x, out, order=None):
    """x: [rows, cols] bf16 values held as float32"""
    return finish(block_partials(x), out, order)


def colsum_x3_add_det(pieces, out, order=None):
    """pieces: [rows, 3, cols] bf16 values held as float32"""
    return finish(block_partials(x3_elements(pieces)), out, order)


def constructed(cols=8, col=3):
    """the order-sensitivity input: 256 rows, x[0] = 2^24, x[64] = 1, x[128] = -2^24, x[192] = 1 in one column, zeros elsewhere (all
    exact in bf16 and as x3 pieces), prior out = 0.5.  The stated order gives exactly 1.5 in that column; the exact sum is 2.5"""
    x = np.zeros((256, cols), dtype=F)
    x[0, col], x[64, col], x[128, col], x[192, col] = 2.0 ** 24, 1.0, -2.0 ** 24, 1.0
    out = np.full(cols, 0.5, dtype=F)
    return x, out
