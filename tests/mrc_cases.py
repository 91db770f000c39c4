"""The resident dataset and the batches of tests/test_mrc_collate_gpu.py, in numpy alone, so that tests/test_mrc_collate_cpu.py can
check without a GPU that the cases contain what the GPU test says they do (test infrastructure)."""
import numpy as np

CLS, SEP = 101, 102
N, T, D, R_MAX = 9, 8, 64, 11
ARRAY_KEYS = ('feat', 'pos', 'soft', 'row_start', 'row_cnt', 'input_ids', 'token_type_ids', 'txt_len', 'labels', 'ids')
CFG = dict(seed=(5 << 32) + 17, draw=3)
# region counts: ragged 3 .. 11; sample 3 has none; sample 7 shares rows 1 .. 9 of sample 0; sample 8 (batches OUTSIDE only)
# starts two rows before the end of the pool
COUNTS = np.array([11, 3, 7, 0, 5, 11, 4, 9, 6], np.int32)
CRAFTED = 4                        # the sample whose five soft rows are the argmax edge cases of crafted_rows()
MAIN = [0, 1, 2, 4, 5]             # B = 5, R = 11
BATCHES = {'main': MAIN, 'one': [2], 'no regions at all': [3, 3], 'a sample without regions': [3, 1, 3, 6],
           'shared rows': [0, 7, 0], 'outside the pool': [8, 1, 8]}


def leading_dimensions(C):
    """ld_soft == C; C rounded up to 4 and one item more (rows start 16-byte aligned); an odd one beyond C"""
    return {'C': C, 'aligned': (C + 3) // 4 * 4 + 4, 'odd': C + 3 + (C % 2)}


def crafted_rows(C):
    """five rows [C] and the label each must give: a tie between two maxima (the first wins), an all-equal row (1), the maximum
    in column 0 (ignored), the maximum in column C-1, and a tie whose columns fall to one lane of the wave in both row layouts"""
    rng = np.random.default_rng(C)
    base = lambda: (rng.random(C) * 0.5).astype(np.float32)
    hi = np.float32(0.75)
    tie = base(); tie[[2, C - 1]] = hi
    equal = np.full(C, 1.0 / C, np.float32)
    col0 = base(); col0[0] = 10.0
    want0 = 1 + int(np.argmax(col0[1:]))
    last = base(); last[C - 1] = hi
    lane = base()
    a, b = (70, 326) if C > 326 else (1, 3)
    lane[[a, b]] = hi
    return np.stack([tie, equal, col0, last, lane]), [2, 1, want0, C - 1, a]


def synth(C, ld_soft, seed=0):
    """Nine samples over a pool whose rows lie out of order with rows nobody owns between them.  soft[:, :C] is a softmax of
    normals; the columns [C, ld_soft) hold NaN: they belong to the row and must not reach any output."""
    rng = np.random.default_rng(seed)
    cnt = COUNTS.copy()
    place = [5, 2, 0, 4, 1, 6, 3]                    # samples 7 and 8 own no rows of their own
    row_start, at = np.zeros(N, np.int64), 2
    for s in place:
        row_start[s] = at
        at += int(cnt[s]) + 3
    row_start[7] = row_start[0] + 1
    rows = at
    row_start[8] = rows - 2                           # regions 2 .. 5 of sample 8 lie outside the pool
    txt = np.array([T, 2, 5, 3, 7, 4, 6, 2, 5], np.int32)
    input_ids = np.zeros((N, T), np.int64)
    for i, tl in enumerate(txt):
        input_ids[i, :tl] = [CLS] + list(rng.integers(1000, 28996, tl - 2)) + [SEP]
    z = rng.standard_normal((rows, C))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    soft = np.full((rows, ld_soft), np.nan, np.float32)
    soft[:, :C] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    crafted, _ = crafted_rows(C)
    soft[row_start[CRAFTED]:row_start[CRAFTED] + 5, :C] = crafted
    return {'feat': rng.standard_normal((rows, D)).astype(np.float32), 'pos': rng.random((rows, 7)).astype(np.float32), 'soft': soft,
            'row_start': row_start, 'row_cnt': cnt, 'input_ids': input_ids,
            'token_type_ids': rng.integers(0, 2, (N, T)).astype(np.int64), 'txt_len': txt,
            'labels': rng.integers(0, 2, N).astype(np.int64), 'ids': rng.integers(0, 99999, N).astype(np.int64)}


def shape_of(a, sel, ragged):
    """(R, L_out) as the host derives them"""
    sel = np.asarray(sel)
    R = int(a['row_cnt'][sel].max())
    return R, int((a['txt_len'][sel] + (a['row_cnt'][sel] if ragged else R)).max())
