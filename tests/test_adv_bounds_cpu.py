"""tests/adv_ref.py checks itself: a numpy-fp32 restatement of uniter_bce_kl_logits and uniter_adv_delta_step_linf as
include/uniter_hip.h states them, written independently of the references, stays within HALF of every bound over every case of the
shared lists, with the batch sums taken serially and again as a pairwise tree (the worse of the two counts); wrong formulas leave
the bounds; and the closed form of the symmetric KL divergence is the four-logarithm form.  No GPU, no library.

Recorded over the lists (loss: 7 batch sizes x 3 pos_weight x 3 kl_weight x 3 grad_scale x 3 label patterns, the 49 planted pairs
with both labels, z == c everywhere; Linf: 2 batch sizes x 5 sizes x 5 placements of the maximum x max_norm 0.4 / 0), worst
|fp32 - float64| as a share of the bound, the worse of the two summation orders: total 0.335, bce 0.352, kl 0.404, probs 0.362,
dlogits 0.353, Linf 0.304.  In units of 2^-24 times each bound's scale that is A_KL_T 32 (12.9 reached: the serial sum of 1000
terms; 11.3 at 256, and 1.1 with the pairwise tree), A_KL_D 8 (2.8), A_LINF 4 (1.2).
Wrong formulas, times over the bound: KL in one direction only 2.0e5 on the kl term and 1.7e5 on the total; the gradient without its
q (1 - q)(z - c) term 2.0e6; grad_scale applied twice 1.4e6; the Linf maximum taken without the sample's last element 3.7e7, taken
of g instead of |g| 3.7e7."""
import numpy as np
import pytest

import adv_ref as A
import loss_ref as R

F = np.float32
ONE, ZERO = F(1), F(0)
MODES = ('serial', 'tree')


def sum32(a, mode):
    """fp32 sum of a vector: 'serial' in index order, 'tree' pairwise over the zero-padded power of two"""
    a = np.asarray(a, dtype=F)
    if mode == 'serial':
        return np.cumsum(a, dtype=F)[-1]
    m = 1 << max(0, (a.size - 1).bit_length())
    a = np.concatenate([a, np.zeros(m - a.size, dtype=F)])
    while a.size > 1:
        a = a[::2] + a[1::2]
    return a[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 restatements; bug = None or the name of a wrong formula
# ---------------------------------------------------------------------------------------------------------------------------
def bce_kl32(z, c, y, pw, klw, gs, mode, bug=None):
    z, c, yf = np.asarray(z, dtype=F), np.asarray(c, dtype=F), np.asarray(y).astype(F)
    pw, klw, gs = F(pw), F(klw), F(gs)
    Bf = F(z.size)
    lw = ONE + (pw - ONE) * yf
    with np.errstate(all='ignore'):
        sp = np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, ZERO)
        q = ONE / (ONE + np.exp(-z))
        p = ONE / (ONE + np.exp(-c))
        if bug == 'one_direction':                       # KL(p||q) alone: p (log p - log q) + (1 - p)(log(1 - p) - log(1 - q))
            spc = np.log1p(np.exp(-np.abs(c))) + np.maximum(-c, ZERO)
            kl_el = p * (sp - spc) + (ONE - p) * ((z + sp) - (c + spc))
        else:
            kl_el = (p - q) * (c - z)
    bce = sum32((ONE - yf) * z + lw * sp, mode) / Bf
    kl = sum32(kl_el, mode) / Bf
    total = bce + klw * kl
    slope = ZERO if bug == 'no_slope' else q * (ONE - q) * (z - c)
    kg = (q - p) + slope
    scale = gs / Bf
    dlog = (((ONE - yf) - lw * (ONE - q)) + klw * kg) * scale
    if bug == 'scale_twice':
        dlog = dlog * gs
    assert q.dtype == dlog.dtype == F and all(np.asarray(v).dtype == F for v in (total, bce, kl))
    return dict(total=total, bce=bce, kl=kl, probs=q, dlogits=dlog)


def linf32(delta, grad, step, max_norm, bug=None):
    d, g = np.asarray(delta, dtype=F), np.asarray(grad, dtype=F)
    out = d.copy()
    for b in range(d.shape[0]):
        src = g[b, :-1] if bug == 'skip_last' else g[b]
        gm = np.abs(src).max() if src.size else ZERO
        if bug == 'signed_max':
            gm = src.max()
        if gm > 0:
            out[b] = d[b] + (F(step) / gm) * g[b]
    if max_norm > 0:
        out = np.minimum(np.maximum(out, F(-max_norm)), F(max_norm))
    assert out.dtype == F
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# ratios over the case lists
# ---------------------------------------------------------------------------------------------------------------------------
def _loss_inputs():
    for B, pw, klw, gs, labels in A.bce_kl_cases():
        yield A.bce_kl_case(B, labels) + (pw, klw, gs)
    for pw, klw in zip(A.PWS, A.KLWS):
        yield A.bce_kl_planted_case() + (pw, klw, 0.5)
        yield A.bce_kl_planted_case() + (pw, 1.0, 1.0 / 3.0)
    for B in A.BS:
        yield A.bce_kl_equal_case(B) + (1.8, 1.0, 0.5)


KEYS = ('total', 'bce', 'kl', 'probs', 'dlogits')


def loss_ratios(bug=None):
    out = {}
    for z, c, y, pw, klw, gs in _loss_inputs():
        ref = A.ref_bce_kl(z, c, y, pw, klw, gs)
        for mode in MODES:
            got = bce_kl32(z, c, y, pw, klw, gs, mode, bug)
            for k in KEYS:
                out[k] = max(out.get(k, 0.0), A.worst_ratio(got[k], ref[k], ref['E_' + k]))
    return out


def linf_ratio(bug=None):
    worst = 0.0
    for B, n, kind in A.linf_cases():
        delta, grad = A.linf_case(B, n, kind)
        for mn in (A.LINF_MAX_NORM, 0.0):
            worst = max(worst, A.worst_ratio(linf32(delta, grad, A.LINF_STEP, mn, bug), *A.ref_linf(delta, grad, A.LINF_STEP, mn)))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_case_lists_hold_what_they_promise():
    z, c, y = A.bce_kl_planted_case()
    assert z.size == 98 and (y[::2] == 0).all() and (y[1::2] == 1).all()
    assert {(float(a), float(b)) for a, b in zip(z, c)} == set(A.PLANTED_PAIRS) and int((z == c).sum()) == 14
    for B in A.BS:
        z, c, y = A.bce_kl_case(B, 'mixed')
        idx = np.arange(0, B, 8)
        idx = idx[idx >= (len(A.PLANTED_PAIRS) if B >= 64 else 0)]
        assert z.dtype == c.dtype == F and y.dtype == np.int64 and (z[idx] == c[idx]).all()
        assert B < 64 or [(float(a), float(b)) for a, b in zip(z[:49], c[:49])] == list(A.PLANTED_PAIRS)
        assert B == 1 or set(y) == {0, 1}
        z, c, y = A.bce_kl_equal_case(B)
        assert np.array_equal(z, c) and (B < 7 or set(R.BCE_PLANTED) <= set(z.astype(np.float64).tolist()))
    assert A.GSS == (1.0, 0.5, 1.0 / 3.0) and A.KLWS == (0.0, 1.0, 0.3) and A.PWS == (1.0, 1.8, 0.25) and A.BS == (1, 3, 64, 255, 256, 257, 1000)
    for B, n, kind in A.linf_cases():
        d, g = A.linf_case(B, n, kind)
        assert d.shape == g.shape == (B, n) and np.abs(d).max() <= 0.5
        a = np.abs(g)
        for b in range(B):
            if kind == 'zero' and b == B // 2:
                assert not g[b].any()
                continue
            top = np.flatnonzero(a[b] == a[b].max())
            want = {'first': [0], 'last': [n - 1], 'zero': [n - 1], 'negative': [n // 2], 'tie': [0, n - 1]}[kind]
            assert list(top) == want and a[b].max() == F(A.LINF_PLANT)
            assert n == 4 and kind == 'tie' or np.delete(a[b], want).max() <= A.LINF_PLANT / 4.9
            assert kind != 'negative' or g[b, n // 2] < 0
            assert kind != 'tie' or (g[b, 0] > 0 > g[b, n - 1])


def test_closed_form_is_the_four_logarithm_form():
    worst = 0.0
    for B in A.BS:
        for labels in A.LABELS:
            z, c, y = A.bce_kl_case(B, labels)
            worst = max(worst, abs(A.ref_bce_kl(z, c, y, 1.0, 1.0, 1.0)['kl'] - A.ref_kl_four_logs(z, c)))
    z, c, y = A.bce_kl_planted_case()
    ref = A.ref_bce_kl(z, c, y, 1.0, 1.0, 1.0)
    four = A.ref_kl_four_logs(z, c)
    print('closed form against four logarithms: random cases %.3e absolute, planted pairs %.3e relative' % (worst, abs(ref['kl'] - four) / four))
    assert worst <= 1e-14 and abs(ref['kl'] - four) <= 1e-14 * four
    assert (ref['kl_el'] >= 0).all() and (ref['kl_el'][z == c] == 0).all()


def test_fp32_restatement_stays_within_half_of_every_bound():
    shares = loss_ratios()
    shares['linf'] = linf_ratio()
    print('worst |fp32 - float64| / bound: ' + ', '.join('%s %.3f' % kv for kv in shares.items()))
    print('in units of 2^-24 x scale: kl %.2f, dlogits %.2f, linf %.2f' % (shares['kl'] * A.A_KL_T, shares['dlogits'] * A.A_KL_D,
                                                                        shares['linf'] * A.A_LINF))
    for k, v in shares.items():
        assert v <= 0.5, (k, v)


def test_equal_logits_give_an_exact_zero():
    for B in A.BS:
        z, c, y = A.bce_kl_equal_case(B)
        for mode in MODES:
            with_kl, without = bce_kl32(z, c, y, 1.8, 1.0, 0.5, mode), bce_kl32(z, c, y, 1.8, 0.0, 0.5, mode)
            assert with_kl['kl'] == 0 and np.array_equal(with_kl['dlogits'], without['dlogits']) and with_kl['total'] == without['total']


WRONG = {
    'one_direction': (loss_ratios, ('kl', 'total')),
    'no_slope': (loss_ratios, ('dlogits',)),
    'scale_twice': (loss_ratios, ('dlogits',)),
    'skip_last': (linf_ratio, None),
    'signed_max': (linf_ratio, None),
}


@pytest.mark.parametrize('bug', list(WRONG))
def test_a_wrong_formula_leaves_the_bound(bug):
    fn, need = WRONG[bug]
    r = fn(bug)
    if need is None:
        print('%s: times over the bound: %.3g' % (bug, r))
        assert r > 1.0
        return
    print('%s: times over the bound: ' % bug + ', '.join('%s %.3g' % (k, r[k]) for k in need))
    for k in need:
        assert r[k] > 1.0, (bug, k, r)
