"""tests/loss_ref.py checks itself: a numpy-fp32 restatement of the loss and head formulas of include/uniter_hip.h, written
independently of the references, stays within HALF of every bound over every case of the shared lists, with its sums taken serially
in column order and again as a pairwise tree (the worse of the two counts); and wrong formulas leave the bounds.  No GPU, no library.

Recorded over the lists (cross-entropy and KL: C = 1 .. 1601 x (1, 5 random rows, the planted rows), and 3 rows of 28996 for
cross-entropy; BCE: 7 batch sizes x 3 pos_weight x 3 grad_scale x 3 label patterns and the planted logits; MSE / dgelu: 5 sizes),
worst |fp32 - float64| as a share of the bound, the worse of the two summation orders: CE lse 0.367, loss 0.368, dlogits 0.462; KL
lse 0.331, loss 0.327, dlogits 0.401; BCE loss 0.448, probs 0.361, dlogits 0.345; MSE 0.474, its backward 0.271; dgelu_mul 0.268.
With the constants of loss_ref.py that is, in units of 2^-24 times each bound's scale: A_CE_D 16 (7.4 reached), A_KL_D 16 (6.4),
A_BCE_L 40 (17.9: the serial sum of 1000 terms), A_BCE_P 4 (1.4), A_BCE_D 8 (2.8), A_DGELU 8 (2.1), and A_LSE 4 with B_LSE 8 sqrt(C).
The second lse term grows with sqrt(C) because the serial fp32 sum does: its absolute error is 12 x 2^-24 at C = 64, 23 at 513, 127
at 1601 (the planted row whose maximum sits on column 256: every later term is added to a sum 150 times its size) and 522 at 28996,
where the pairwise tree stays at 10 for every C; 8 sqrt(C) is 320 and 1362 at the last two, the constant 8 itself well below 64.
Wrong formulas, times over the bound: lse with column 63 / 64 / 255 / 256 dropped 6.8e5 / 5.8e5 / 4.1e5 / 3.0e5, with column 0 or
C - 1 dropped infinite (C = 1 leaves no column; 1.6e5 and more at every larger C); lse without the max subtraction infinite (the
shifted rows overflow); CE one-hot on the narrowed, unclamped target 1.1e9; BCE without pos_weight on the gradient 6.3e6, with
pos_weight on the (1 - y) term 1.3e6, the sum divided by 256 1.2e6, log(1 + exp(-x)) infinite (x = -88, -100); the tanh GELU
derivative 1.8e3, phi(u) without its factor u 1.1e6; KL with log t unmasked at t = 0 infinite (NaN), KL backward without the
softmax * sum term 1.1e6; argmax taking the last maximum wrong on 32 rows of the list, the lowest lane in place of the lowest column
on 8, c0 ignored on 41."""
import math

import numpy as np
import pytest
import torch

import loss_ref as R

F = np.float32
ONE, ZERO, HALF = F(1), F(0), F(0.5)
MODES = ('serial', 'tree')


def sum32(a, mode):
    """fp32 sum over the last axis: 'serial' in index order, 'tree' pairwise over the zero-padded power of two"""
    a = np.asarray(a, dtype=F)
    if mode == 'serial':
        return np.cumsum(a, axis=-1, dtype=F)[..., -1]
    n = a.shape[-1]
    m = 1 << max(0, (n - 1).bit_length())
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (m - n,), dtype=F)], axis=-1)
    while a.shape[-1] > 1:
        a = a[..., ::2] + a[..., 1::2]
    return a[..., 0]


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 restatements; bug = None or the name of a wrong formula
# ---------------------------------------------------------------------------------------------------------------------------
def lse32(x, mode, bug=None, drop=None):
    x = np.asarray(x, dtype=F)
    with np.errstate(all='ignore'):
        if drop is not None and drop < x.shape[1]:           # (-1: the last column)
            x = np.delete(x, drop % x.shape[1], axis=1)
            if x.shape[1] == 0:
                return np.full(x.shape[0], -np.inf, dtype=F)
        if bug == 'no_max':
            return np.log(sum32(np.exp(x), mode))
        mx = x.max(axis=1)
        return mx + np.log(sum32(np.exp(x - mx[:, None]), mode))


def ce32(x, t, lse_in, g, mode, bug=None, drop=None):
    x, g, lse_in = np.asarray(x, dtype=F), np.asarray(g, dtype=F), np.asarray(lse_in, dtype=F)
    n, C = x.shape
    lse = lse32(x, mode, bug, drop)
    tc = np.where(t < 0, 0, np.where(t >= C, C - 1, t))
    loss = lse - x[np.arange(n), tc]
    hot = np.zeros((n, C), dtype=F)
    if bug == 'unclamped':                      # the column compared with (int)target: narrowed, not clamped
        tn = t.astype(np.int32)
        ok = (tn >= 0) & (tn < C)
        hot[np.arange(n)[ok], tn[ok]] = ONE
    else:
        hot[np.arange(n), tc] = ONE
    dlog = (np.exp(x - lse_in[:, None]) - hot) * g[:, None]
    assert loss.dtype == lse.dtype == dlog.dtype == F
    return loss, lse, dlog


def kl32(x, t, lse_in, dl, mode, bug=None):
    x, t, dl, lse_in = (np.asarray(a, dtype=F) for a in (x, t, dl, lse_in))
    lse = lse32(x, mode)
    with np.errstate(all='ignore'):
        full = t * (np.log(t) - (x - lse[:, None]))
    loss = full if bug == 'log0' else np.where(t > 0, full, ZERO)
    dt = dl * t
    s = ZERO if bug == 'no_sum' else sum32(dt, mode)[:, None]
    dlog = np.exp(x - lse_in[:, None]) * s - dt
    assert loss.dtype == lse.dtype == dlog.dtype == F
    return loss, lse, dlog


def bce32(x, y, pw, gs, mode, bug=None):
    x, yf, pw, gs = np.asarray(x, dtype=F), np.asarray(y).astype(F), F(pw), F(gs)
    B = x.size
    lw = ONE + (pw - ONE) * yf
    with np.errstate(all='ignore'):
        sp = np.log(ONE + np.exp(-x)) if bug == 'naive' else np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, ZERO)
        sg = ONE / (ONE + np.exp(-x))
    if bug == 'pw_on_neg':
        terms = lw * (ONE - yf) * x + sp
    else:
        terms = (ONE - yf) * x + lw * sp
    loss = sum32(terms, mode) / F(256 if bug == 'div256' else B)
    lwg = ONE if bug == 'no_pw_grad' else lw
    dlog = ((ONE - yf) - lwg * (ONE - sg)) * (gs / F(B))
    assert sg.dtype == dlog.dtype == F and np.asarray(loss).dtype == F
    return loss, sg, dlog


def dgelu32(dy, u, bug=None):
    dy, u = np.asarray(dy, dtype=F), np.asarray(u, dtype=F)
    if bug == 'tanh':
        k, c = F(math.sqrt(2.0 / math.pi)), F(0.044715)
        th = np.tanh(k * (u + c * u * u * u))
        return dy * (HALF * (ONE + th) + HALF * u * (ONE - th * th) * k * (ONE + F(3) * c * u * u))
    cdf = HALF * (ONE + torch.erf(torch.from_numpy(u * F(0.70710678118654752440))).numpy())
    pdf = F(0.39894228040143267794) * np.exp(-HALF * u * u)
    out = dy * (cdf + (pdf if bug == 'no_u' else u * pdf))
    assert out.dtype == F
    return out


def argmax32(x, c0, bug=None):
    """the kernel's shape of the search: lane l of 64 walks the columns c0 + l, c0 + l + 64, ..., then the lanes are joined"""
    x = np.asarray(x, dtype=F)
    n, C = x.shape
    if bug == 'no_c0':
        c0 = 0
    out = np.empty(n, dtype=np.int64)
    for r in range(n):
        cand = []                                # (value, column) of every lane that saw something above -inf, in lane order
        for lane in range(64):
            cols = np.arange(c0 + lane, C, 64)
            if cols.size:
                v = x[r, cols]
                k = v.size - 1 - int(np.argmax(v[::-1])) if bug == 'last' else int(np.argmax(v))
                if v[k] > -np.inf:
                    cand.append((float(v[k]), int(cols[k])))
        if not cand:
            out[r] = c0
            continue
        top = max(v for v, _ in cand)
        tied = [c for v, c in cand if v == top]
        out[r] = max(tied) if bug == 'last' else tied[0] if bug == 'lane_first' else min(tied)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# ratios over the case lists
# ---------------------------------------------------------------------------------------------------------------------------
def _upd(d, **kv):
    for k, v in kv.items():
        d[k] = max(d.get(k, 0.0), v)


def ce_ratios(bug=None, drop=None, cases=None):
    out = {}
    for C, n in cases or R.row_cases(vocab=True):
        c = R.ce_case(C, n)
        fwd = R.ref_ce_fwd(c['x'], c['t'])
        lse_in = fwd['lse'].astype(F)
        ref_d, E_d = R.ref_ce_bwd(c['x'], c['t'], lse_in, c['dloss'])
        for mode in MODES:
            loss, lse, dlog = ce32(c['x'], c['t'], lse_in, c['dloss'], mode, bug, drop)
            _upd(out, lse=R.worst_ratio(lse, fwd['lse'], fwd['E_lse']), loss=R.worst_ratio(loss, fwd['loss'], fwd['E_loss']),
                 dlogits=R.worst_ratio(dlog, ref_d, E_d))
    return out


def kl_ratios(bug=None):
    out = {}
    for C, n in R.row_cases():
        c = R.kl_case(C, n)
        fwd = R.ref_kl_fwd(c['x'], c['t'])
        lse_in = fwd['lse'].astype(F)
        ref_d, E_d = R.ref_kl_bwd(c['x'], c['t'], lse_in, c['dloss'])
        for mode in MODES:
            loss, lse, dlog = kl32(c['x'], c['t'], lse_in, c['dloss'], mode, bug)
            _upd(out, kl_lse=R.worst_ratio(lse, fwd['lse'], fwd['E_lse']), kl_loss=R.worst_ratio(loss, fwd['loss'], fwd['E_loss']),
                 kl_dlogits=R.worst_ratio(dlog, ref_d, E_d))
    return out


def _bce_inputs():
    for B, pw, gs, labels in R.bce_cases():
        yield R.bce_case(B, labels) + (pw, gs)
    for pw in R.BCE_PWS:
        yield R.bce_planted_case() + (pw, 0.5)


def bce_ratios(bug=None):
    out = {}
    for x, y, pw, gs in _bce_inputs():
        ref = R.ref_bce(x, y, pw, gs)
        for mode in MODES:
            loss, sg, dlog = bce32(x, y, pw, gs, mode, bug)
            _upd(out, bce_loss=R.worst_ratio(loss, ref['loss'], ref['E_loss']), bce_probs=R.worst_ratio(sg, ref['probs'], ref['E_probs']),
                 bce_dlogits=R.worst_ratio(dlog, ref['dlogits'], ref['E_dlogits']))
    return out


def elem_ratios(bug=None):
    out = {}
    for n in R.ELEM_NS:
        p, t, dl = R.mse_case(n)
        d = p - t
        _upd(out, mse=R.worst_ratio(d * d, *R.ref_mse_fwd(p, t)), mse_bwd=R.worst_ratio(F(2) * d * dl, *R.ref_mse_bwd(p, t, dl)))
        dy, u = R.dgelu_case(n)
        _upd(out, dgelu=R.worst_ratio(dgelu32(dy, u, bug), *R.ref_dgelu_mul(dy, u)))
    return out


def argmax_wrong(bug=None):
    """number of rows of the case list on which the search differs from the reference"""
    bad = 0
    for C in R.ARGMAX_CS:
        for c0 in R.argmax_c0s(C):
            for n in R.ARGMAX_NS:
                if bug is None or n in ('planted', 3):
                    x, _ = R.argmax_case(C, n, c0)
                    bad += int((argmax32(x, c0, bug) != R.ref_argmax(x, c0)).sum())
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_case_lists_hold_what_they_promise():
    tiny = float(np.finfo(F).tiny)
    for C, n in R.row_cases(vocab=True):
        c = R.ce_case(C, n)
        assert c['x'].dtype == F and c['t'].dtype == np.int64 and c['x'].shape[1] == C
        if n == 'planted':
            x, names = c['x'].astype(np.float64), c['names']
            for e in sorted({e % C for e in R.EDGE_COLS if e < C}):
                r = names.index('max@%d' % e)
                assert C == 1 or x[r, e] - np.delete(x[r], e).max() >= 4.99
            assert x[names.index('shift+10000')].min() > 9900 and x[names.index('shift-10000')].max() < -9900
            if C > 1:
                r = names.index('tie')
                assert x[r, 0] == x[r, C - 1] == x[r].max()
                r = names.index('target=max-40')
                assert x[r].max() - x[r, c['t'][r]] >= 39.9
            assert x[names.index('target=max'), c['t'][names.index('target=max')]] == x[names.index('target=max')].max()
            assert list(c['t'][-3:]) == [-1, C, 2 ** 33 + 1]
        k = R.kl_case(C, n) if C != R.VOCAB else None
        if k is not None:
            t = k['t']
            assert ((t == 0) | (t >= 1e3 * tiny)).all() and (t >= 0).all() and (C < 64 or (t == 0).any())
            if n == 'planted':
                assert not t[-2].any() and t[-1].sum() == 1.0 and (t[-1] == 1.0).sum() == 1
    x, y = R.bce_planted_case()
    assert sorted(set(np.abs(x).tolist())) == [0.0, 30.0, 88.0, 100.0] and x.size == 14 and (y[::2] == 0).all() and (y[1::2] == 1).all()
    for B in R.BCE_BS:
        x, y = R.bce_case(B, 'mixed')
        assert B < 64 or (np.array_equal(x[:14], R.bce_planted_case()[0]) and np.array_equal(y[:14], R.bce_planted_case()[1]))
        assert B == 1 or set(y) == {0, 1}
    for n in R.ELEM_NS:
        dy, u = R.dgelu_case(n)
        assert n < 255 or set(R.DGELU_PLANTED) <= set(u.astype(np.float64).tolist()) | {1e-4, -1e-4}
        p, t, dl = R.mse_case(n)
        assert n == 1 or (p == t).any()
        d = np.abs(p.astype(np.float64) - t)
        assert ((d == 0) | (d > 1e-4)).all()
    for H in R.GATHER_HS:
        for n in R.GATHER_NS:
            src, rows, idx = R.gather_case(n, H, seed=n)
            assert len(set(idx)) == n and (n == 1 or {0, R.NSRC - 1} <= set(idx)) and idx.min() >= 0 and idx.max() < R.NSRC
    assert set(R.gather_case(9, 8, oob=True)[2]) >= {-1, R.NSRC, 2 ** 33 + 1, 0, R.NSRC - 1}


def test_fp32_restatement_stays_within_half_of_every_bound():
    shares = {}
    for part in (ce_ratios(), kl_ratios(), bce_ratios(), elem_ratios()):
        shares.update(part)
    print('worst |fp32 - float64| / bound: ' + ', '.join('%s %.3f' % kv for kv in shares.items()))
    for k, v in shares.items():
        assert v <= 0.5, (k, v)
    assert argmax_wrong() == 0


@pytest.mark.parametrize('col', R.EDGE_COLS)
def test_lse_with_an_edge_column_dropped_leaves_the_bound(col):
    cases = [(C, 'planted') for C in R.ROW_CS if col < C]
    r = ce_ratios(drop=col, cases=cases)
    print('column %d dropped: times over the bound: lse %.3g, loss %.3g' % (col, r['lse'], r['loss']))
    assert r['lse'] > 1.0 and r['loss'] > 1.0
    for C, n in cases:                                         # every C that has the column catches it on its own
        assert ce_ratios(drop=col, cases=[(C, n)])['lse'] > 1.0, C


WRONG = {
    'no_max': (ce_ratios, ('lse', 'loss')),
    'unclamped': (ce_ratios, ('dlogits',)),
    'no_pw_grad': (bce_ratios, ('bce_dlogits',)),
    'pw_on_neg': (bce_ratios, ('bce_loss',)),
    'div256': (bce_ratios, ('bce_loss',)),
    'naive': (bce_ratios, ('bce_loss',)),
    'tanh': (elem_ratios, ('dgelu',)),
    'no_u': (elem_ratios, ('dgelu',)),
    'log0': (kl_ratios, ('kl_loss',)),
    'no_sum': (kl_ratios, ('kl_dlogits',)),
}


@pytest.mark.parametrize('bug', list(WRONG))
def test_a_wrong_formula_leaves_the_bound(bug):
    fn, need = WRONG[bug]
    r = fn(bug)
    print('%s: times over the bound: ' % bug + ', '.join('%s %.3g' % (k, r[k]) for k in need))
    for k in need:
        assert r[k] > 1.0, (bug, k, r)


def test_naive_softplus_fails_at_minus_100():
    x, y = np.array([-100.0], dtype=F), np.array([1])
    ref = R.ref_bce(x, y, 1.8, 1.0)
    assert R.worst_ratio(bce32(x, y, 1.8, 1.0, 'serial', 'naive')[0], ref['loss'], ref['E_loss']) > 1.0
    assert R.worst_ratio(bce32(x, y, 1.8, 1.0, 'serial')[0], ref['loss'], ref['E_loss']) <= 0.5


@pytest.mark.parametrize('bug', ['last', 'lane_first', 'no_c0'])
def test_a_wrong_argmax_differs(bug):
    bad = argmax_wrong(bug)
    print('%s: wrong on %d rows' % (bug, bad))
    assert bad > 0
