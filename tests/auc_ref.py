"""Float64 reference of uniter_bce_auc_logits (csrc/head.hip) -- BCE plus a pairwise AUROC surrogate over (batch) x (batch U a bank
of recent scores), and the bank's push -- with the case list its tests share and error bounds for an fp32 evaluation.  Plain numpy on
the CPU: no GPU, no library.  Written from the words of include/uniter_hip.h, after tests/adv_ref.py; the BCE part is
tests/loss_ref.py's reference, constants and helpers as they are.

The reference takes the fp32 INPUT VALUES the kernel gets, widened to float64.  With S+ / S- the batch rows labelled 1 / 0, K+ / K-
the bank's `fill` most recently pushed slots labelled 1 / 0 (as they are BEFORE the call's push), s a row's logit or a slot's score:

    P       = S+ x S-  U  S+ x K-  U  K+ x S-,   n = |P|                (no bank-bank pairs)
    auc     = (1 / n) sum_{(i, j) in P} l(s_i - s_j),   0 where n = 0
    l(d)    = softplus(-d) (kind 0)   |   max(0, margin - d)^2 (kind 1)
    total   = bce + auc_weight auc
    g_b     = (1 / n) sum_{j in S- U K-} l'(z_b - s_j)  (b in S+),   -(1 / n) sum_{i in S+ U K+} l'(s_i - z_b)  (b in S-),   else 0
    dlogits = grad_scale (bce'_b / B + auc_weight g_b)

Bounds.  U = 2^-24.  With M = B + N the number of scores a row can be paired with:

    one pair    A_PAIR U |l(d)| + [l(d - delta) - l(d)],   delta = 2 U |d|                                     (value)
                A_PAIR U |l'(d)| + max |l'(d +- delta) - l'(d)|                                                 (slope)
                The first term is the arithmetic on a given d: kind 0 takes an expf and a log1pf (2 ulp = 4 U each, the allowance
                loss_ref gives them: a relative error of e moves log1p(e) by no more relatively, since e / (1 + e) <= log1p(e)),
                an addition, and for the slope a division in place of the logarithm; kind 1 a subtraction, and a square that
                doubles its error, or a doubling.  That is 9 U at most; A_PAIR = 16.  The second term is the conditioning: d is
                the ROUNDED difference of two fp32 scores, off by U |d|, and l is evaluated there -- taken on the function itself
                (l falls and is convex, so the left side is the larger one) and not as |l'| delta, which is 0 at the hinge's kink
                where a rounded d just inside the margin still gives (delta)^2.  At d = +-160 (logits +-80) it is what matters:
                softplus(-160) = 160 (1 + U) is off by 160 U.
    auc         the mean of the pair bounds + (M + B + 8) U auc
                all terms are non-negative, so any order's rounding is relative to the sum, at most U per addition a term passes
                through.  A kernel may sum a row's up to M terms serially and then the B rows serially: M + B, and 8 for
                1 / n, float(n) and the product.  This is the worst case of that order, not an estimate: 1.5e-4 relative at the
                largest case (B = 257, N = 1000); a tree does far better.
    g_b         the mean of the slope bounds over the row's pairs, over n, + (M + 8) U |g_b|            (l' <= 0: one sign, as above)
    bce, probs  loss_ref's E_loss, E_probs
    total       E_bce + auc_weight E_auc + 2 U (|bce| + auc_weight auc)                                   (the product and the addition)
    dlogits     loss_ref's E_dlogits + |grad_scale| auc_weight E_g + 4 U (|bce' share| + |grad_scale| auc_weight |g_b|)
    n_pairs, the pushed bank, head, fill: exact.

The constants are not tuned to the kernel: tests/test_auc_bounds_cpu.py evaluates the same formulas in numpy fp32, independently
written, with serial sums and with pairwise trees, over every case below, and stays within half of every bound.  Inputs hold no fp32
subnormals; the slots of a bank outside its `fill` hold garbage (NaN in two cases) that no result may depend on."""
import math

import numpy as np

import loss_ref as R

U = R.U
F = np.float32
D = np.float64
A_PAIR = 16.0
KINDS = {'logistic': 0, 'hinge2': 1}

worst_ratio = R.worst_ratio
f32 = R.f32


# ---------------------------------------------------------------------------------------------------------------------------
# the bank
# ---------------------------------------------------------------------------------------------------------------------------
class Bank(object):
    """scores float32 [N], labels int32 [N], head, fill -- the three arrays of the C ABI on the host"""

    def __init__(self, scores, labels, head, fill):
        self.scores, self.labels = np.asarray(scores, dtype=F).copy(), np.asarray(labels, dtype=np.int32).copy()
        self.head, self.fill = int(head), int(fill)
        self.N = self.scores.size
        assert self.labels.size == self.N and 0 <= self.head < self.N and 0 <= self.fill <= self.N

    def valid(self):
        """mask [N]: the `fill` slots pushed most recently, i.e. the ones that precede head on the ring"""
        age = (self.head - 1 - np.arange(self.N)) % self.N
        return age < self.fill

    def state(self):
        return np.array([self.head, self.fill], dtype=np.int32)

    def pushed(self, z, y):
        """the bank after the push of the batch (z, y): slot (head + r) mod N <- (z[r], (int32) y[r])"""
        B = len(z)
        assert B <= self.N
        out = Bank(self.scores, self.labels, self.head, self.fill)
        slots = (self.head + np.arange(B)) % self.N
        out.scores[slots] = np.asarray(z, dtype=F)
        out.labels[slots] = np.asarray(y, dtype=np.int64).astype(np.int32)
        out.head, out.fill = (self.head + B) % self.N, min(self.fill + B, self.N)
        return out

    def oldest_first(self):
        idx = (self.head - self.fill + np.arange(self.fill)) % self.N
        return self.scores[idx], self.labels[idx]


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def surrogate(d, kind, margin):
    """-> l(d), l'(d) in float64"""
    d = np.asarray(d, dtype=D)
    if kind == 0:
        e = np.exp(-np.abs(d))
        return np.maximum(-d, 0.0) + np.log1p(e), -np.where(d >= 0, e, 1.0) / (1.0 + e)
    h = np.maximum(margin - d, 0.0)
    return h * h, -2.0 * h


def pair_bounds(d, kind, margin):
    """-> the bound of one pair's value and of its slope, for the fp32 evaluation at the rounded difference (module docstring)"""
    d = np.asarray(d, dtype=D)
    delta = 2.0 * U * np.abs(d)
    l, dl = surrogate(d, kind, margin)
    l_lo, dl_lo = surrogate(d - delta, kind, margin)
    _, dl_hi = surrogate(d + delta, kind, margin)
    return A_PAIR * U * l + (l_lo - l), A_PAIR * U * np.abs(dl) + np.maximum(np.abs(dl_lo - dl), np.abs(dl_hi - dl))


def ref_bce_auc(z, y, pos_weight, auc_weight, kind, margin, grad_scale, bank=None):
    """-> dict total, bce, auc, n, probs, dlogits, g (the surrogate's share of the gradient, unscaled) and E_total, E_bce, E_auc,
    E_probs, E_dlogits.  z may hold float64 values that are no fp32 numbers (the central differences of the CPU test)"""
    z, yi = np.asarray(z, dtype=D), np.asarray(y, dtype=np.int64)
    B = z.size
    base = R.ref_bce(z, yi, pos_weight, grad_scale)
    aw, m, gs = f32(auc_weight), f32(margin), f32(grad_scale)
    if bank is None:
        ks, kpos, kneg = np.zeros(0), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)
    else:
        ok = bank.valid()
        ks = np.where(ok, bank.scores.astype(D), 0.0)          # (what an invalid slot holds is never looked at)
        kpos, kneg = ok & (bank.labels == 1), ok & (bank.labels == 0)
    M = B + ks.size
    s = np.concatenate([z, ks])
    pos = np.concatenate([yi == 1, kpos])
    neg = np.concatenate([yi == 0, kneg])
    in_batch = np.arange(M) < B
    # pair (i, j): i a positive, j a negative, at least one of them a batch row
    pair = pos[:, None] & neg[None, :] & (in_batch[:, None] | in_batch[None, :])
    n = int(pair.sum())
    d = s[:, None] - s[None, :]
    l, dl = surrogate(d, kind, m)
    e_l, e_dl = pair_bounds(d, kind, m)
    g, E_g = np.zeros(B), np.zeros(B)
    auc = E_auc = 0.0
    if n:
        auc = math.fsum(l[pair]) / n
        E_auc = math.fsum(e_l[pair]) / n + (M + B + 8) * U * auc
        gp = np.where(pair, dl, 0.0)
        ep = np.where(pair, e_dl, 0.0)
        g = (gp.sum(axis=1) - gp.sum(axis=0))[:B] / n            # a row is positive or negative, never both: one of the two is 0
        E_g = (ep.sum(axis=1) + ep.sum(axis=0))[:B] / n + (M + 8) * U * np.abs(g)
    total = base['loss'] + aw * auc
    dlog = base['dlogits'] + gs * aw * g
    return dict(total=total, bce=base['loss'], auc=auc, n=n, probs=base['probs'], dlogits=dlog, g=g,
                E_total=base['E_loss'] + aw * E_auc + 2.0 * U * (abs(base['loss']) + aw * auc), E_bce=base['E_loss'], E_auc=E_auc,
                E_probs=base['E_probs'],
                E_dlogits=base['E_dlogits'] + abs(gs) * aw * E_g + 4.0 * U * (np.abs(base['dlogits']) + abs(gs) * aw * np.abs(g)))


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _bank(r, N, head, fill, garbage='finite', labels=None, scores=None):
    """N slots, the valid ones 2 randn scores with random 0 / 1 labels (or the given ones, oldest first), the others garbage: a
    large score with a label that would count ('finite'), or NaN with label 1 ('nan')"""
    sc = np.where(np.arange(N) % 2 == 0, 9.0, -9.0).astype(F) if garbage == 'finite' else np.full(N, np.nan, dtype=F)
    lb = (np.arange(N) % 2 == 0).astype(np.int32) if garbage == 'finite' else np.ones(N, dtype=np.int32)
    idx = (head - fill + np.arange(fill)) % N
    sc[idx] = (2.0 * r.standard_normal(fill)).astype(F) if scores is None else np.asarray(scores, dtype=F)
    lb[idx] = r.integers(0, 2, fill).astype(np.int32) if labels is None else np.asarray(labels, dtype=np.int32)
    return Bank(sc, lb, head, fill)


def _mixed(r, B):
    z = (2.0 * r.standard_normal(B)).astype(F)
    y = r.integers(0, 2, B).astype(np.int64)
    if B > 1:
        y[0], y[1] = 1, 0
    return z, y


def base_cases():
    """name -> (z float32 [B], y int64 [B], bank or None, margin, grad_scale): the shapes and values of the issue's list"""
    out = {}
    r = R._rng('auc', 1)
    out['B1_no_bank'] = (np.array([0.3], dtype=F), np.array([1], dtype=np.int64), None, 1.0, 1.0)                 # n = 0
    out['B2_one_of_each'] = (np.array([0.5, -0.25], dtype=F), np.array([1, 0], dtype=np.int64), None, 1.0, 1.0)
    zp = (2.0 * r.standard_normal(4)).astype(F)
    out['all_positive_empty_bank'] = (zp, np.ones(4, dtype=np.int64), _bank(r, 8, 0, 0, 'nan'), 1.0, 1.0)        # n = 0
    out['all_positive_bank_of_negatives'] = (zp, np.ones(4, dtype=np.int64), _bank(r, 8, 5, 5, labels=np.zeros(5)), 1.0, 1.0)
    for fill, head, garbage in ((0, 0, 'finite'), (3, 3, 'nan'), (8, 5, 'finite')):
        out['B5_N8_fill%d' % fill] = _mixed(r, 5) + (_bank(r, 8, head, fill, garbage), 1.0, 1.0)
    out['push_wraps'] = _mixed(r, 5) + (_bank(r, 8, 6, 6), 1.0, 0.5)                                              # head + B = 11 > 8
    out['B_equals_N'] = _mixed(r, 8) + (_bank(r, 8, 3, 8), 1.0, 1.0)
    out['B257_N1000'] = _mixed(r, 257) + (_bank(r, 1000, 123, 1000), 0.5, 1.0 / 3.0)       # rows beyond one per lane, N % 64 != 0
    out['B257_N1000_fill700'] = _mixed(r, 257) + (_bank(r, 1000, 900, 700), 1.0, 1.0)      # the valid stretch wraps: 200 .. 899
    out['logits_pm80'] = (np.array([80, -80, 80, -80, 0, 0], dtype=F), np.array([1, 1, 0, 0, 1, 0], dtype=np.int64),
                          _bank(r, 8, 4, 4, scores=[80, -80, 80, -80], labels=[1, 1, 0, 0]), 1.0, 1.0)
    out['ties'] = (np.full(4, 0.5, dtype=F), np.array([1, 0, 1, 0], dtype=np.int64),
                   _bank(r, 6, 2, 2, scores=[0.5, 0.5], labels=[1, 0]), 1.0, 1.0)                                 # every d = 0
    # d == margin exactly (1.5 - 0.5, 2.25 - 1.25 and both against the bank), beside pairs inside (1.5 - 1.25) and outside it
    out['d_equals_margin'] = (np.array([1.5, 0.5, 2.25, 1.25], dtype=F), np.array([1, 0, 1, 0], dtype=np.int64),
                              _bank(r, 4, 2, 2, scores=[0.5, 2.25], labels=[0, 1]), 1.0, 1.0)
    out['label_2'] = (_mixed(r, 6)[0], np.array([1, 0, 2, 1, 0, 2], dtype=np.int64),
                      _bank(r, 8, 4, 4, labels=[1, 2, 0, 0]), 1.0, 2.0)              # in the batch and in a valid slot of the bank
    return out


def cases():
    """[(id, dict z, y, bank, pos_weight, auc_weight, kind, margin, grad_scale)]: every base case with both surrogates at
    auc_weight 0.7, pos_weight 1.8"""
    out = []
    for name, (z, y, bank, margin, gs) in base_cases().items():
        for kname, kind in KINDS.items():
            out.append(('%s-%s' % (name, kname), dict(z=z, y=y, bank=bank, pos_weight=1.8, auc_weight=0.7, kind=kind, margin=margin,
                                                      grad_scale=gs)))
    return out


def ref_of(case):
    return ref_bce_auc(case['z'], case['y'], case['pos_weight'], case['auc_weight'], case['kind'], case['margin'], case['grad_scale'],
                       case['bank'])
