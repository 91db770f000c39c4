"""Float64 references of the VILLA kernels (uniter_bce_kl_logits in csrc/head.hip, uniter_adv_delta_step_linf in csrc/adv.hip), the case lists their
tests share, and per-element error bounds for an fp32 evaluation.  Plain numpy on the CPU: no GPU, no library.  Written after
tests/loss_ref.py, whose BCE reference, constants and helpers are used as they are.

Every reference takes the fp32 INPUT VALUES the kernel gets, widened to float64, and restates the formula of include/uniter_hip.h.
With z the perturbed logit, c the clean one, q = sigmoid(z), p = sigmoid(c), lw = 1 + (pos_weight - 1) y:

    kl      = mean_b (p - q)(c - z)            [= mean_b KL(p||q) + KL(q||p); ref_kl_four_logs is the four-logarithm form]
    total   = bce + kl_weight kl
    dlogits = grad_scale / B (bce' + kl_weight ((q - p) + q (1 - q)(z - c)))

Bounds.  U = 2^-24; each is a small constant times U times the quantity the rounding scales with:

    kl term     A_KL_T U mean_b |c - z|
                p and q are sigmoids in [0, 1] with an absolute error of an ulp or two each, so p - q errs by a few U ABSOLUTELY
                (it cancels where c is near z: no relative bound holds) and the product by a few U |c - z|; the terms are
                non-negative, so the sum's own rounding is relative to the sum, which is at most mean |c - z|.  The constant
                is sized by the order a kernel may choose, the serial one included, as A_BCE_L is: a serial fp32 sum of 1000
                terms reaches 12.9, a pairwise tree 1.1.
    bce term    loss_ref's E_loss (A_BCE_L), probs loss_ref's E_probs (A_BCE_P)
    total       E_bce + kl_weight E_kl + 2 U (|bce| + kl_weight kl)        (the product and the addition)
    dlogits     A_KL_D U |grad_scale| / B (lw + kl_weight (1 + |c - z| / 4))
                bce' is bounded by lw; q - p by 1, absolute error a few U; q (1 - q) <= 1/4 with a relative error of a few U,
                times |z - c|; the roundings of the weighted sum and of the scaling are relative to the same quantities.  With
                kl_weight = 0 this is loss_ref's BCE bound (A_KL_D = A_BCE_D).
    Linf step   A_LINF U (|delta| + |step_size|), against the reference that uses the fp32-rounded factor step_size / max|g|
                |a g| <= |step_size| (1 + U): the product's rounding is U |step_size|, the addition's U (|delta| + |step_size|);
                the clamp is exact.

The constants are not tuned to the kernels: tests/test_adv_bounds_cpu.py evaluates the same formulas in numpy fp32, independently
written, with a serial and with a pairwise sum, over every case of the lists below; each constant is at least twice the worst share
the worse of the two reaches (recorded there).  Inputs hold no fp32 subnormals."""
import itertools
import math

import numpy as np

import loss_ref as R

U = R.U
F = np.float32
D = np.float64
A_KL_T = 32.0
A_KL_D = 8.0
A_LINF = 4.0

worst_ratio = R.worst_ratio
f32 = R.f32


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def _sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def ref_bce_kl(z, c, y, pos_weight, kl_weight, grad_scale):
    """-> dict total, bce, kl, probs, dlogits and E_total, E_bce, E_kl, E_probs, E_dlogits; kl_el, the per-element KL terms"""
    z, c, yd = np.asarray(z, dtype=D), np.asarray(c, dtype=D), np.asarray(y, dtype=D)
    B = z.size
    base = R.ref_bce(z, y, pos_weight, grad_scale)
    pw, klw, gs = f32(pos_weight), f32(kl_weight), f32(grad_scale)
    lw = 1.0 + (pw - 1.0) * yd
    q, p = _sigmoid64(z), _sigmoid64(c)
    kl_el = (p - q) * (c - z)
    kl = math.fsum(kl_el) / B
    dist = np.abs(c - z)
    E_kl = A_KL_T * U * math.fsum(dist) / B
    e = np.exp(-np.abs(z))
    qq = e / ((1.0 + e) * (1.0 + e))
    dl = base['dlogits'] + klw * ((q - p) + qq * (z - c)) * gs / B
    total = base['loss'] + klw * kl
    return dict(total=total, bce=base['loss'], kl=kl, probs=base['probs'], dlogits=dl, kl_el=kl_el,
                E_total=base['E_loss'] + klw * E_kl + 2.0 * U * (abs(base['loss']) + klw * kl), E_bce=base['E_loss'], E_kl=E_kl,
                E_probs=base['E_probs'], E_dlogits=A_KL_D * U * abs(gs) / B * (lw + klw * (1.0 + dist / 4.0)))


def ref_kl_four_logs(z, c):
    """mean_b [p log(p / q) + (1 - p) log((1 - p) / (1 - q)) + q log(q / p) + (1 - q) log((1 - q) / (1 - p))], the logarithms
    of the sigmoids taken as -softplus so that they stay finite; float64"""
    z, c = np.asarray(z, dtype=D), np.asarray(c, dtype=D)

    def logsig(x):
        return -(np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0))
    q, p = _sigmoid64(z), _sigmoid64(c)
    q1, p1 = _sigmoid64(-z), _sigmoid64(-c)
    el = p * (logsig(c) - logsig(z)) + p1 * (logsig(-c) - logsig(-z)) + q * (logsig(z) - logsig(c)) + q1 * (logsig(-z) - logsig(-c))
    return math.fsum(el) / z.size


def linf_factor(grad, step_size):
    """the fp32 factor step_size / max|g| per sample [B, 1] as float64 values, 0 where the gradient vanishes"""
    gm = np.abs(np.asarray(grad, dtype=F)).max(axis=1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.where(gm > 0, F(step_size) / gm, F(0)).astype(F)
    return a.astype(D)


def ref_linf(delta, grad, step_size, max_norm):
    """delta <- clamp(delta + a g, -max_norm, max_norm) (max_norm <= 0: no clamp), a = linf_factor -> new delta, E"""
    d, g = np.asarray(delta, dtype=D), np.asarray(grad, dtype=D)
    out = d + linf_factor(grad, step_size) * g
    mn = f32(max_norm)
    if mn > 0:
        out = np.clip(out, -mn, mn)
    return out, A_LINF * U * (np.abs(d) + abs(f32(step_size)))


# ---------------------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------------------
BS = R.BCE_BS
PWS = R.BCE_PWS
KLWS = (0.0, 1.0, 0.3)
GSS = (1.0, 0.5, 1.0 / 3.0)
LABELS = R.BCE_LABELS
PLANTED_PAIRS = tuple(itertools.product(R.BCE_PLANTED, R.BCE_PLANTED))        # (z, c): 49 pairs, 7 of them z == c


def bce_kl_case(B, labels, seed=0):
    """-> z, c float32 [B], y int64 [B].  z ~ 3 randn, c = z + 0.7 randn with every eighth entry c == z; from B = 64 on the
    leading entries hold PLANTED_PAIRS (as many as fit; bce_kl_planted_case holds them all with both labels)"""
    r = R._rng(seed, B, labels, 11)
    z = (3.0 * r.standard_normal(B)).astype(F)
    c = (z + 0.7 * r.standard_normal(B)).astype(F)
    c[::8] = z[::8]
    y = {'zeros': np.zeros(B), 'ones': np.ones(B), 'mixed': r.integers(0, 2, B)}[labels].astype(np.int64)
    if B == 3 and labels == 'mixed':
        y[:] = (0, 1, 0)
    k = min(B, len(PLANTED_PAIRS)) if B >= 64 else 0
    pp = np.array(PLANTED_PAIRS, dtype=F)
    z[:k], c[:k] = pp[:k, 0], pp[:k, 1]
    return z, c, y


def bce_kl_planted_case():
    """the planted pairs with both labels, nothing else: B = 98"""
    pp = np.repeat(np.array(PLANTED_PAIRS, dtype=F), 2, axis=0)
    return pp[:, 0].copy(), pp[:, 1].copy(), (np.arange(pp.shape[0]) % 2).astype(np.int64)


def bce_kl_equal_case(B, seed=0):
    """z == c everywhere (the planted values in front): the KL term and its share of the gradient are exactly 0"""
    z, _, y = bce_kl_case(B, 'mixed', seed)
    k = min(B, len(R.BCE_PLANTED))
    z[:k] = np.array(R.BCE_PLANTED[:k], dtype=F)
    return z, z.copy(), y


def bce_kl_cases():
    """(B, pos_weight, kl_weight, grad_scale, labels): the whole product"""
    return list(itertools.product(BS, PWS, KLWS, GSS, LABELS))


LINF_BS = (1, 3)
LINF_NS = (4, 4092, 4096, 4100, 12292)            # the 4096-float chunk's edge from both sides, and a fourth chunk of 4 floats
LINF_KINDS = ('first', 'last', 'negative', 'tie', 'zero')
LINF_STEP, LINF_MAX_NORM = 0.3, 0.4
LINF_PLANT = 0.0125                               # the planted max|g|: 5 times what the other elements reach


def linf_case(B, n, kind, seed=0):
    """-> delta, grad float32 [B, n].  delta uniform in [-0.5, 0.5] (a part of it lies outside the ball of LINF_MAX_NORM),
    the gradient uniform in [-0.0025, 0.0025] with the maximum planted per sample: 'first' at element 0, 'last' at element n - 1
    (the last of the last chunk), 'negative' a negative value in the middle, 'tie' +max at element 0 and -max at n - 1, 'zero' as
    'last' with the gradient of sample B // 2 all zero"""
    r = R._rng(seed, B, n, kind, 12)
    delta = (r.random((B, n)) - 0.5).astype(F)
    grad = ((r.random((B, n)) - 0.5) * 0.005).astype(F)
    m = F(LINF_PLANT)
    if kind == 'first':
        grad[:, 0] = m
    elif kind in ('last', 'zero'):
        grad[:, n - 1] = m
    elif kind == 'negative':
        grad[:, n // 2] = -m
    elif kind == 'tie':
        grad[:, 0], grad[:, n - 1] = m, -m
    if kind == 'zero':
        grad[B // 2] = 0
    return delta, grad


def linf_cases():
    return list(itertools.product(LINF_BS, LINF_NS, LINF_KINDS))
