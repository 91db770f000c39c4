"""float64 numpy restatement of the scoring contract of uniter_ensemble_auc_counts, written from the words of include/uniter_hip.h
(test infrastructure; it imports nothing of the package's search code).

    Inputs: a plane x[M][N] of doubles (probabilities or their logits), an optional plane present[M][N] of 0.0 / 1.0 (None = all
    present), columns permuted so that the first n_pos are the positive samples, weights w[C][M].
    Per candidate c and sample i, all in IEEE double and in this order:
      1. num = 0; ws = 0.
      2. for m = 0..M-1: num = num + (w[c][m]*x[m][i])*present[m][i]; ws = ws + w[c][m]*present[m][i].
      3. s_i = num / min(max(ws,1e-4),1e5).
      4. s_i = 0.5 where ws == 0.
    counts[c] = 2 * #{(p,n): s_p > s_n} + #{(p,n): s_p == s_n} over positive p and negative n, int64; 0 with one class only.

One candidate after the other; the pair counts by comparison of every positive with every negative."""
import numpy as np


def mixed_scores(x, present, w_c):
    """s[N] of one candidate"""
    M, N = x.shape
    num = np.zeros(N, dtype=np.float64)
    ws = np.zeros(N, dtype=np.float64)
    for m in range(M):
        wm = np.float64(w_c[m])
        if present is None:
            num = num + (wm * x[m]) * np.float64(1.0)
            ws = ws + wm * np.float64(1.0)
        else:
            num = num + (wm * x[m]) * present[m]
            ws = ws + wm * present[m]
    with np.errstate(invalid='ignore', divide='ignore'):
        s = num / np.minimum(np.maximum(ws, 1e-4), 1e5)
    s[ws == 0.0] = 0.5
    return s


def auc_counts(x, present, w, n_pos):
    """int64 [C]"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    assert x.ndim == 2 and w.ndim == 2 and w.shape[1] == x.shape[0] and 0 <= n_pos <= x.shape[1]
    out = np.zeros(w.shape[0], dtype=np.int64)
    for c in range(w.shape[0]):
        s = mixed_scores(x, present, w[c])
        pos, neg = s[:n_pos], s[n_pos:]
        if pos.size and neg.size:
            out[c] = 2 * int((pos[:, None] > neg[None, :]).sum()) + int((pos[:, None] == neg[None, :]).sum())
    return out


def make_predictions(M, N, n_pos, missing=0, seed=0, grid=None):
    """([M, N] predictions, [N] labels): probabilities of 6 decimals, as a CSV export holds them (or on a 1/grid lattice: heavy
    ties), a little higher for the n_pos positive samples, `missing` entries per model set to -1; labels in a shuffled order"""
    rng = np.random.default_rng(seed)
    gt = np.zeros(N, dtype=np.int64)
    gt[rng.permutation(N)[:n_pos]] = 1
    p = np.clip(rng.normal(0.4 + 0.2 * gt[None, :], 0.25, size=(M, N)), 0.0, 1.0)
    p = np.round(p * grid) / grid if grid else np.round(p, 6)
    for m in range(M):
        p[m, rng.permutation(N)[:min(missing, N)]] = -1.0
    return p, gt


def make_weights(C, M, seed=0, grid_only=False):
    """[C, M]: even rows from the brute-force grid {0, 0.5, 1, 2}, odd rows continuous in [0, 4] with genes at 0, as the
    evolutionary search makes them (grid_only: every row from the grid)"""
    rng = np.random.default_rng(1000 + seed)
    w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0]), size=(C, M))
    if not grid_only:
        cont = rng.uniform(0.0, 4.0, size=(C, M)) * (rng.random((C, M)) < 0.8)
        w[1::2] = cont[1::2]
    return w


SIZES_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
SIZES_M = (1, 2, 3, 15, 64)
SIZES_C = (1, 2, 255, 256, 257)


def positives_of(N):
    """n_pos in {0, 1, about N / 2, N - 1, N}, without repeats"""
    return sorted({0, 1, N // 2, N - 1, N} & set(range(N + 1)))


def shape_matrix():
    """(N, n_pos, M, C): every N with every n_pos while M and C cycle through their values (each pair of M and C comes up), then
    every M with every C at N = 65, and the two N on either side of the kernel's threshold between its two workgroup sizes"""
    cases, k = [], 0
    for N in SIZES_N:
        for n_pos in positives_of(N):
            cases.append((N, n_pos, SIZES_M[k % 5], SIZES_C[(k // 5 + k) % 5]))
            k += 1
    cases += [(65, 32, M, C) for M in SIZES_M for C in SIZES_C]
    cases += [(2048, 1024, 3, 2), (2049, 1024, 3, 2)]
    return cases


def logits_of(p):
    """the wrapper's logits (include/uniter_hip.h): log(clip(p,1e-8,1)) - log(clip(1-p,1e-8,1))"""
    p = np.asarray(p, dtype=np.float64)
    return np.log(np.clip(p, 1e-8, 1.0)) - np.log(np.clip(1 - p, 1e-8, 1.0))


def planes_of(predictions, gt):
    """(probability plane, logit plane, present plane, n_pos) of [M, N] predictions with -1 = missing and labels gt, as the
    wrapper is to prepare them: missing entries 0.5 (logit 0), positives first"""
    p = np.array(predictions, dtype=np.float64)
    gt = np.asarray(gt)
    missing = p == -1
    p[missing] = 0.5
    order = np.concatenate([np.flatnonzero(gt == 1), np.flatnonzero(gt == 0)])
    return p[:, order], logits_of(p)[:, order], (1.0 - missing)[:, order], int((gt == 1).sum())
