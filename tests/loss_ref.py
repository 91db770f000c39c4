"""Float64 references of the loss and pretraining-head kernels (uniter_bce_logits in csrc/head.hip, everything in csrc/heads.hip), the
case lists their tests share, and per-element error bounds for an fp32 evaluation.  Plain numpy / torch on the CPU: no GPU, no library.

Every reference takes the fp32 INPUT VALUES the kernel gets, widened to float64, restates the formula of include/uniter_hip.h and
returns its value next to the bound on |fp32 result - value|.  The backward passes of cross-entropy and KL take the log-sum-exp as
an INPUT, as the C ABI does: the reference is the exact function of that fp32 value, whoever computed it.

Bounds.  U = 2^-24 (half an ulp, relative); each bound is a small constant times U times the quantity the rounding scales with:

    lse, CE loss    A_LSE U max(1, |lse|, |x_target|) + B_LSE U sqrt(C)
                    first term: the roundings of mx + log(sum) and of lse - x_target, relative to the larger operand; second:
                    the relative error of the sum (each expf term, and the summation order) seen through the log, where a relative
                    error becomes an absolute one.  It is stated per sqrt(C) because the order a kernel may choose includes the
                    serial one, whose error grows with the number of terms (measured: 12 U at C = 64, 127 U at 1601, 522 U at
                    28996; a pairwise tree stays at 10 U); one constant for every C would be 60 times too wide at C = 64.
    CE dlogits      A_CE_D U |dloss_r| (max(p, 2^-10) + [c == target])
                    p = exp(x - lse) carries the rounding of x - lse times |x - lse| <= 7 down to p = 2^-10 and an ulp of expf;
                    below that the absolute error only shrinks (d exp(-d) falls); the target column adds the rounding of p - 1.
    KL loss         A_KL U t (|log t| + |x| + |lse|) + t E_lse,  exactly 0 where t == 0
                    the three terms of log t - (x - lse) are rounded relative to their own sizes; E_lse is the bound of the lse
                    the forward kernel computes for itself, which enters as t * lse.
    KL dlogits      A_KL_D U (max(p, 2^-10) S + |dloss_j t_j|),  S = sum_c |dloss_c t_c|
                    the fp32 sum errs relative to S (absolute terms: the bound survives its cancellation), p as above.
    BCE loss        A_BCE_L U (sum_b (|(1 - y) x| + lw softplus(-x))) / B
                    the two parts of a term cancel (x = -30, y = 0: -30 + 30.0000000000001), so the bound is stated on their
                    absolute values, not on |term|, as optim_ref does for g coef + wd p.
    BCE probs       A_BCE_P U                          (absolute: sigmoid lies in [0, 1])
    BCE dlogits     A_BCE_D U lw |grad_scale| / B      (absolute at the scale of the term: at x = +20, y = 1 fp32 1 - sigmoid is 0
                    against a true 2e-9, which no relative bound admits)
    dgelu_mul       A_DGELU U |dy|                     (absolute: Phi + u phi lies in [-0.13, 1.13]; fp32 erff cancels near u = -6)
    MSE             3 ulp of the result (3 * 2^-23 relative): p - t, the square (which doubles it) / the two products; exactly 0
                    where pred == target
    argmax, gather, scatter-add: exact.

The constants are not tuned to the kernels: tests/test_loss_bounds_cpu.py evaluates the same formulas in numpy fp32, independently
written, with a serial sum in column order and again with a pairwise tree, over every case of the lists below; each constant is
at least twice the worst share the worse of the two reaches (the shares are recorded there).  Inputs hold no fp32 subnormals."""
import itertools
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
ULP = 2.0 ** -23
A_LSE, B_LSE = 4.0, 8.0
A_CE_D = 16.0
A_KL = 4.0
A_KL_D = 16.0
A_BCE_L = 40.0
A_BCE_P = 4.0
A_BCE_D = 8.0
A_DGELU = 8.0
MSE_ULPS = 3.0
P_FLOOR = 2.0 ** -10

F = np.float32
D = np.float64


def f32(x):
    """the fp32 value of a scalar argument, as a Python float"""
    return float(np.float32(x))


def worst_ratio(got, ref, bound):
    """max of |got - ref| / bound over the elements; an element with bound 0 must be exact; a NaN or an infinity counts as inf"""
    got, ref, bound = np.asarray(got, dtype=D), np.asarray(ref, dtype=D), np.asarray(bound, dtype=D)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    if not np.all(np.isfinite(r)):
        return math.inf
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def _lse64(x):
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def clamp_targets(t, C):
    """targets outside [0, C) are clamped (memory safety only, see include/uniter_hip.h), the int64 before any narrowing"""
    return np.clip(np.asarray(t, dtype=np.int64), 0, C - 1)


def lse_bound(lse, C, xt=None):
    scale = np.maximum(1.0, np.abs(lse))
    if xt is not None:
        scale = np.maximum(scale, np.abs(xt))
    return A_LSE * U * scale + B_LSE * U * math.sqrt(C)


def ref_bce(x, y, pos_weight, grad_scale):
    """nn.BCEWithLogitsLoss(pos_weight) (train_template.py:65,98-99): loss = mean_b[(1 - y) x + (1 + (pw - 1) y) softplus(-x)],
    probs = sigmoid(x), dlogits = dloss/dx * grad_scale = ((1 - y) - lw (1 - sigmoid(x))) * grad_scale / B
    -> dict loss, probs, dlogits and E_loss, E_probs, E_dlogits"""
    x, y = np.asarray(x, dtype=D), np.asarray(y, dtype=D)
    B = x.size
    pw, gs = f32(pos_weight), f32(grad_scale)
    lw = 1.0 + (pw - 1.0) * y
    sp = np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0)
    with np.errstate(over='ignore'):
        one_minus_sg = np.where(x >= 0, np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))), 1.0 / (1.0 + np.exp(-np.abs(x))))
    sg = np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
    loss = math.fsum((1.0 - y) * x + lw * sp) / B
    mag = math.fsum(np.abs((1.0 - y) * x) + lw * sp) / B
    dl = ((1.0 - y) - lw * one_minus_sg) * gs / B
    return dict(loss=loss, probs=sg, dlogits=dl, E_loss=A_BCE_L * U * mag, E_probs=np.full(B, A_BCE_P * U),
                E_dlogits=A_BCE_D * U * lw * abs(gs) / B)


def ref_ce_fwd(x, t):
    """F.cross_entropy(x, t, reduction='none') (model/pretrain.py:122-124): lse[r] = log sum_c exp(x[r, c]), loss[r] = lse[r] - x[r, t[r]]
    -> dict loss, lse, E_loss, E_lse"""
    x = np.asarray(x, dtype=D)
    n, C = x.shape
    lse = _lse64(x)
    xt = x[np.arange(n), clamp_targets(t, C)]
    return dict(loss=lse - xt, lse=lse, E_loss=lse_bound(lse, C, xt), E_lse=lse_bound(lse, C, xt))


def ref_ce_bwd(x, t, lse, dloss):
    """dlogits[r, c] = (exp(x[r, c] - lse[r]) - [c == t[r]]) * dloss[r], lse the fp32 values the launch is given -> dlogits, E"""
    x, lse, g = np.asarray(x, dtype=D), np.asarray(lse, dtype=D), np.asarray(dloss, dtype=D)
    n, C = x.shape
    p = np.exp(x - lse[:, None])
    hot = np.zeros((n, C))
    hot[np.arange(n), clamp_targets(t, C)] = 1.0
    return (p - hot) * g[:, None], A_CE_D * U * np.abs(g)[:, None] * (np.maximum(p, P_FLOOR) + hot)


def ref_kl_fwd(x, t):
    """F.kl_div(F.log_softmax(x, -1), t, reduction='none') (model/pretrain.py:222-226): t (log t - (x - lse)), 0 where t == 0 (xlogy)
    -> dict loss, lse, E_loss, E_lse"""
    x, t = np.asarray(x, dtype=D), np.asarray(t, dtype=D)
    lse = _lse64(x)
    E_lse = lse_bound(lse, x.shape[1])
    with np.errstate(divide='ignore', invalid='ignore'):
        logt = np.where(t > 0, np.log(np.where(t > 0, t, 1.0)), 0.0)
    loss = np.where(t > 0, t * (logt - (x - lse[:, None])), 0.0)
    E = np.where(t > 0, A_KL * U * t * (np.abs(logt) + np.abs(x) + np.abs(lse)[:, None]) + t * E_lse[:, None], 0.0)
    return dict(loss=loss, lse=lse, E_loss=E, E_lse=E_lse)


def ref_kl_bwd(x, t, lse, dloss):
    """dx[r, j] = exp(x[r, j] - lse[r]) * sum_c(dloss[r, c] t[r, c]) - dloss[r, j] t[r, j], lse the fp32 values given -> dlogits, E"""
    x, t, lse, dl = (np.asarray(a, dtype=D) for a in (x, t, lse, dloss))
    p = np.exp(x - lse[:, None])
    dt = dl * t
    s = dt.sum(axis=-1, keepdims=True)
    S = np.abs(dt).sum(axis=-1, keepdims=True)
    return p * s - dt, A_KL_D * U * (np.maximum(p, P_FLOOR) * S + np.abs(dt))


def ref_argmax(x, c0):
    """torch.max(x[:, c0:], -1)[1] + c0 (model/pretrain.py:227-228): the FIRST maximum, as an absolute column; c0 for a row of -inf"""
    return np.argmax(np.asarray(x)[:, c0:], axis=-1).astype(np.int64) + c0


def ref_mse_fwd(p, t):
    """F.mse_loss(p, t, reduction='none') (model/pretrain.py:150-151) -> loss, E"""
    d = np.asarray(p, dtype=D) - np.asarray(t, dtype=D)
    return d * d, MSE_ULPS * ULP * d * d


def ref_mse_bwd(p, t, dloss):
    """dpred = 2 (pred - target) dloss -> dpred, E"""
    r = 2.0 * (np.asarray(p, dtype=D) - np.asarray(t, dtype=D)) * np.asarray(dloss, dtype=D)
    return r, MSE_ULPS * ULP * np.abs(r)


def dgelu64(u):
    """gelu_erf'(u) = Phi(u) + u phi(u) (the heads' GELU, model/layer.py:31-37), float64"""
    u = np.asarray(u, dtype=D)
    Phi = 0.5 * torch.erfc(torch.from_numpy(-u / math.sqrt(2.0))).numpy()
    return Phi + u * np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def ref_dgelu_mul(dy, u):
    """dy * gelu_erf'(u) -> out, E"""
    dy = np.asarray(dy, dtype=D)
    return dy * dgelu64(u), A_DGELU * U * np.abs(dy)


def ref_gather(src, idx):
    """dst[r] = src[idx[r]] (_compute_masked_hidden, model/pretrain.py:129-133); an index outside [0, nsrc) is clamped"""
    src = np.asarray(src)
    return src[np.clip(np.asarray(idx, dtype=np.int64), 0, src.shape[0] - 1)]


def ref_scatter_add(src, idx, dst):
    """dst[idx[r]] += src[r] in fp32 (one addition per element: exact against the kernel); unique indices; a row whose index
    lies outside [0, ndst) is skipped"""
    out = np.array(dst, dtype=F, copy=True)
    for r, i in enumerate(np.asarray(idx, dtype=np.int64)):
        if 0 <= i < out.shape[0]:
            out[i] = out[i] + np.asarray(src, dtype=F)[r]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------------------
ROW_CS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1601)
VOCAB = 28996                                      # one cross-entropy case at the vocabulary's size, n = 3
ROW_NS = (1, 5, 'planted')                         # random rows in a launch of their own, the planted rows in another
EDGE_COLS = (0, 63, 64, 255, 256, -1)              # -1: column C - 1
OOB = (-1, 'C', 2 ** 33 + 1)                       # targets / indices outside the range: below, one past, beyond int32 (2^33 + 1
                                                   # narrows to 1: a clamp after the narrowing lands on another column)


def row_lds(C):
    return (C, C + 3, (C + 3) // 4 * 4 + 4)


def _rng(*key):
    return np.random.default_rng([k if isinstance(k, int) and k >= 0 else zlib.crc32(str(k).encode()) for k in key])


def _randn3(r, n, C):
    return (3.0 * r.standard_normal((n, C))).astype(F)


def planted_logits(C, seed):
    """rows beside the randn * 3 ones -> (x [P, C] float32, names): for every edge column that exists a row whose maximum sits
    there with a margin of 5 over the rest (a dropped column moves lse by about 5), a row shifted by +1e4 and one by -1e4, and a
    row with two equal maxima (first and last column)"""
    r = _rng(seed, C, 1)
    rows, names = [], []
    for e in sorted({e % C for e in EDGE_COLS if e < C}):
        x = _randn3(r, 1, C)[0]
        x[e] = F(np.delete(x, e).max() + 5.0) if C > 1 else x[e]
        rows.append(x), names.append('max@%d' % e)
    for shift in (1e4, -1e4):
        rows.append(_randn3(r, 1, C)[0] + F(shift)), names.append('shift%+g' % shift)
    if C > 1:
        x = _randn3(r, 1, C)[0]
        x[0] = x[C - 1] = x.max() + F(1.0)
        rows.append(x), names.append('tie')
    return np.stack(rows).astype(F), names


def ce_case(C, n, seed=0):
    """-> dict x [rows, C] float32, t int64, dloss float32, names.  n: the number of randn * 3 rows, or 'planted': the rows of
    planted_logits with random targets, a row whose target is its maximum, one whose target is 40 below it, and three rows with
    the targets of OOB"""
    r = _rng(seed, C, str(n), 2)
    if n == 'planted':
        x, names = planted_logits(C, seed)
        t = r.integers(0, C, x.shape[0])
        extra, et = _randn3(r, 2 + len(OOB), C), []
        et.append(int(np.argmax(extra[0]))), names.append('target=max')
        k = (int(np.argmax(extra[1])) + 1) % C
        if C > 1:
            extra[1, k] = extra[1].max() - F(40.0)
        et.append(k), names.append('target=max-40')
        for o in OOB:
            et.append(C if o == 'C' else o), names.append('target=%s' % o)
        x, t = np.concatenate([x, extra]), np.concatenate([t, np.array(et, dtype=np.int64)])
    else:
        x, t, names = _randn3(r, n, C), r.integers(0, C, n), ['randn'] * n
    g = r.standard_normal(x.shape[0])
    g = np.where(np.abs(g) < 0.1, 0.1, g)
    return dict(x=x.astype(F), t=t.astype(np.int64), dloss=g.astype(F), names=names)


def kl_case(C, n, seed=0):
    """-> dict x, t (targets: softmax(randn * 2), a tenth of the entries exactly 0), dloss [rows, C] float32, names.  'planted': the
    rows of planted_logits, and two more whose target row is all zeros / one-hot"""
    r = _rng(seed, C, str(n), 3)
    if n == 'planted':
        x, names = planted_logits(C, seed)
        x = np.concatenate([x, _randn3(r, 2, C)])
        names = names + ['t=0', 't=onehot']
    else:
        x, names = _randn3(r, n, C), ['randn'] * n
    rows = x.shape[0]
    z = 2.0 * r.standard_normal((rows, C))
    t = np.exp(z - z.max(-1, keepdims=True))
    t = t / t.sum(-1, keepdims=True)
    t = np.where(t < 1e-30, 1e-30, t)
    t[r.random((rows, C)) < 0.1] = 0.0
    if n == 'planted':
        t[-2] = 0.0
        t[-1] = 0.0
        t[-1, C // 2] = 1.0
    dl = r.standard_normal((rows, C))
    dl = np.where(np.abs(dl) < 1e-3, 1e-3, dl)
    return dict(x=x.astype(F), t=t.astype(F), dloss=dl.astype(F), names=names)


def row_cases(vocab=False):
    """(C, n) of the cross-entropy / KL lists"""
    out = list(itertools.product(ROW_CS, ROW_NS))
    return out + [(VOCAB, 3)] if vocab else out


ARGMAX_CS = (2, 64, 65, 129, 1601)
ARGMAX_NS = (1, 3, 4, 5, 'planted')


def argmax_c0s(C):
    return sorted({0, 1, C - 1})


def argmax_lds(C):
    return (C, C + 5)


def argmax_case(C, n, c0, seed=0):
    """-> x [rows, C] float32, names.  n random rows (distinct values), or 'planted': ties at (c, c + 64), at (c0, c0 + 1) and
    across the lane wrap at (c0 + 63, c0 + 64) where these columns exist, the maximum at c0, a value in [0, c0) larger than
    everything (c0 > 0), and a row of -inf"""
    r = _rng(seed, C, str(n), c0, 4)
    if n != 'planted':
        return r.permutation(n * C).reshape(n, C).astype(F) / F(8.0) - F(3.0), ['random'] * n
    rows, names = [], []

    def base():
        return (r.random(C) * 2.0 - 1.0).astype(F)
    for a, b in ((c0, c0 + 64), (c0 + 1, c0 + 65), (c0, c0 + 1), (c0 + 63, c0 + 64), (C - 2, C - 1)):
        if c0 <= a and b < C:
            x = base()
            x[a] = x[b] = F(7.0)
            rows.append(x), names.append('tie@%d,%d' % (a, b))
    x = base()
    x[c0] = F(7.0)
    rows.append(x), names.append('max@c0')
    if c0 > 0:
        x = base()
        x[:c0] = F(100.0)
        rows.append(x), names.append('prefix')
        x = base()
        x[c0 - 1] = F(100.0)
        x[C - 1] = F(7.0)
        rows.append(x), names.append('prefix1')
    rows.append(np.full(C, -np.inf, dtype=F)), names.append('-inf')
    return np.stack(rows), names


BCE_BS = (1, 3, 64, 255, 256, 257, 1000)
BCE_PWS = (1.0, 1.8, 0.25)
BCE_GSS = (1.0, 0.5, 0.125)
BCE_LABELS = ('zeros', 'ones', 'mixed')
BCE_PLANTED = (0.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)


def bce_case(B, labels, seed=0):
    """-> x float32 [B], y int64 [B].  randn * 3 logits; the leading entries hold BCE_PLANTED, with both labels in turn where
    the labels are mixed (as many as fit into B; bce_planted_case holds them all)"""
    r = _rng(seed, B, labels, 5)
    x = (3.0 * r.standard_normal(B)).astype(F)
    y = {'zeros': np.zeros(B), 'ones': np.ones(B), 'mixed': r.integers(0, 2, B)}[labels].astype(np.int64)
    if B == 3 and labels == 'mixed':
        y[:] = (0, 1, 0)
    px = np.repeat(np.array(BCE_PLANTED, dtype=F), 2) if labels == 'mixed' else np.array(BCE_PLANTED, dtype=F)
    k = min(B, px.size) if B >= 64 else 0
    x[:k] = px[:k]
    if labels == 'mixed':
        y[:k] = (np.arange(k) % 2)
    return x, y


def bce_planted_case():
    """the planted logits with both labels, nothing else: B = 14"""
    return np.repeat(np.array(BCE_PLANTED, dtype=F), 2), (np.arange(2 * len(BCE_PLANTED)) % 2).astype(np.int64)


def bce_cases():
    """(B, pos_weight, grad_scale, labels): the whole product"""
    return list(itertools.product(BCE_BS, BCE_PWS, BCE_GSS, BCE_LABELS))


ELEM_NS = (1, 255, 256, 257, 1000)
DGELU_PLANTED = (0.0, 1e-4, -1e-4, 1.0, -1.0, 5.0, -5.0, 6.0, -6.0, 10.0, -10.0, 40.0, -40.0)


def mse_case(n, seed=0):
    """-> pred, target, dloss float32 [n]; an eighth of the targets equal their prediction; no difference below 1e-3"""
    r = _rng(seed, n, 6)
    p = r.standard_normal(n).astype(F)
    d = r.standard_normal(n)
    d = np.where(np.abs(d) < 1e-3, 1e-3, d)
    t = (p + d).astype(F)
    t = np.where(r.integers(0, 8, n) == 0, p, t)
    if n > 1:
        t[-1] = p[-1]
    dl = r.standard_normal(n)
    return p, t.astype(F), np.where(np.abs(dl) < 1e-3, 1e-3, dl).astype(F)


def dgelu_case(n, seed=0):
    """-> dy, u float32 [n]: u ~ 2 randn, the trailing entries DGELU_PLANTED (as many as fit)"""
    r = _rng(seed, n, 7)
    dy = r.standard_normal(n)
    dy = np.where(np.abs(dy) < 1e-3, 1e-3, dy).astype(F)
    u = (2.0 * r.standard_normal(n)).astype(F)
    k = min(n, len(DGELU_PLANTED)) if n >= 255 else 0
    if k:
        u[n - k:] = np.array(DGELU_PLANTED[:k], dtype=F)
    return dy, u


GATHER_HS = (4, 8, 252, 256, 260, 768)
GATHER_NS = (1, 3, 4, 5, 9)
NSRC = 11


def gather_case(n, H, seed=0, oob=False):
    """-> src [NSRC, H], rows [n, H] float32, idx int64 [n]: unique indices that include 0 and NSRC - 1 (n = 1: one of the two);
    oob: the indices of OOB in place of the first three that are neither"""
    r = _rng(seed, n, H, 8)
    src = r.standard_normal((NSRC, H)).astype(F)
    rows = r.standard_normal((n, H)).astype(F)
    mid = list(r.permutation(np.arange(1, NSRC - 1)))
    idx = [0, NSRC - 1][seed % 2:seed % 2 + 1] if n == 1 else [NSRC - 1, 0] + mid[:n - 2]
    idx = np.array(idx, dtype=np.int64)[r.permutation(n)] if n > 1 else np.array(idx, dtype=np.int64)
    if oob:
        free = [k for k in range(n) if idx[k] not in (0, NSRC - 1)][:len(OOB)]
        for k, o in zip(free, OOB):
            idx[k] = NSRC if o == 'C' else o
    return src, rows, idx
