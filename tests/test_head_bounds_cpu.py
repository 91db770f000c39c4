"""tests/head_ref.py checks itself: a numpy-fp32 restatement of the pooler and classifier formulas of include/uniter_hip.h, written
independently of the references, stays within HALF of every bound over every case of the shared lists, with its sums taken serially
in index order and again as a pairwise tree (the worse of the two counts); the case lists hold what they promise; and wrong formulas
leave the bounds on the cases named for them.  No GPU, no library.

Recorded over the list (15 shapes with the randn pattern, 6 shapes x 5 further value patterns), worst |fp32 - float64| as a share
of the bound, the worse of the two summation orders:
pooled 0.270, logits 0.142, dpooled 0.428, dpre 0.179, dWp 0.498, dbp 0.485, dWl 0.470, dbl 0.215, dh0 0.138, dh0_add 0.484.
The constants of head_ref.py behind them: A_DOT 16 (pooled, logits, dhidden), A_CN 8 (dpooled), A_DPRE 8 (dpre), and A_SUM 8 with
A_ADD 2 together (dWp, dbp, dWl, dbl and the beta = 1 dhidden).  In the last group the final add's one rounding reaches U |g0 + s|
wherever the sum is small beside the value already there, which is why those shares sit just below one half of a bound whose last
term is 2 U |g0 + s|.  With A_DOT 8 and A_CN 4 the same run gave pooled 0.525 and dpooled 0.856, over the half: both were doubled.
Wrong formulas, times over the bound, the least over the cases each must fail at (every case fails on its own): row 1 of hidden
for row 0 1.8e6 (the 10 shapes with L > 1); the last H % 64 columns dropped 6.1e3 (the 12 shapes with H % 64 != 0); the logits'
columns >= 1024 dropped 1.6e3 (the 4 shapes with H > 1024); 1 - p for 1 - p^2 dpre 3.0e5, dWp 6.3e4, dbp 4.3e4, dhidden 9.8e4;
batch rows >= 64 skipped dWp 5.7e4, dbp 1.4e4 (B = 65, 129); assigned for accumulated dWp 2.6e6, dbp 6.6e5, dWl 8.1e4, dbl 1.8e4;
bp omitted 1.8e4; Wl read as [k][c] 5.0e4 (the 9 shapes with Cn > 1).  The formulas that touch every shape are run below H = 4096
(14 shapes) to keep this file at seconds."""
import numpy as np
import pytest

import head_ref as R

F = np.float32
ONE = F(1)
MODES = ('serial', 'tree')
TINY = float(np.finfo(F).tiny)


def sum32(a, mode):
    """fp32 sum over the last axis: 'serial' in index order, 'tree' pairwise over the zero-padded power of two"""
    a = np.asarray(a, dtype=F)
    if a.shape[-1] == 0:
        return np.zeros(a.shape[:-1], dtype=F)
    if mode == 'serial':
        return np.cumsum(a, axis=-1, dtype=F)[..., -1]
    n = a.shape[-1]
    m = 1 << max(0, (n - 1).bit_length())
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (m - n,), dtype=F)], axis=-1)
    while a.shape[-1] > 1:
        a = a[..., ::2] + a[..., 1::2]
    return a[..., 0]


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 restatement of forward and backward; bug = None or the name of a wrong formula
# ---------------------------------------------------------------------------------------------------------------------------
def head32(c, mode, bug=None, backward=True):
    hidden, Wp, bp, Wl, bl, dy = (c[k] for k in ('hidden', 'Wp', 'bp', 'Wl', 'bl', 'dlog'))
    B, L, H = hidden.shape
    Cn = Wl.shape[0]
    h0 = hidden[:, 1 if bug == 'row1' else 0, :]
    kp = H - H % 64 if bug == 'drop_tail' else H
    pre = sum32(h0[:, None, :kp] * Wp[None, :, :kp], mode)                     # [B, n, k] over k
    if bug != 'no_bp':
        pre = pre + bp
    pooled = np.tanh(pre)
    wl = np.ascontiguousarray(Wl.reshape(H, Cn).T) if bug == 'wl_swapped' else Wl
    kl = min(H, 1024) if bug == 'logits_1024' else H
    logits = sum32(pooled[:, None, :kl] * wl[None, :, :kl], mode) + bl          # [B, c, k] over k
    if not backward:
        return dict(pooled=pooled, logits=logits)
    dpooled = sum32(dy[:, None, :] * Wl.T[None, :, :], mode)                    # [B, k, c] over c
    dpre = dpooled * ((ONE - pooled) if bug == 'one_minus_p' else (ONE - pooled * pooled))
    bw = min(B, 64) if bug == 'batch_64' else B
    sW = sum32(dpre.T[:, None, :bw] * h0.T[None, :, :bw], mode)                 # [n, k, b] over b
    sb = sum32(dpre.T[:, :bw], mode)
    sL = sum32(dy.T[:, None, :] * pooled.T[None, :, :], mode)                   # [c, k, b] over b
    sl = sum32(dy.T, mode)
    if bug == 'assign':
        dWp, dbp, dWl, dbl = sW, sb, sL, sl
    else:
        dWp, dbp, dWl, dbl = c['dWp0'] + sW, c['dbp0'] + sb, c['dWl0'] + sL, c['dbl0'] + sl
    dh0 = sum32(dpre[:, None, :] * Wp.T[None, :, :], mode)                      # [B, k, n] over n
    out = dict(pooled=pooled, logits=logits, dpooled=dpooled, dpre=dpre, dWp=dWp, dbp=dbp, dWl=dWl, dbl=dbl, dh0=dh0,
               dh0_add=c['dh_prev'][:, 0] + dh0)
    assert all(v.dtype == F for v in out.values())
    return out


QUANTITIES = ('pooled', 'logits', 'dpooled', 'dpre', 'dWp', 'dbp', 'dWl', 'dbl', 'dh0', 'dh0_add')


def ratios(c, mode, bug=None, backward=True):
    """|restatement - reference| / bound per quantity; the backward's reference is the function of the restatement's own pooled"""
    got = head32(c, mode, bug, backward)
    fwd = R.ref_pooler_fwd(c['hidden'], c['Wp'], c['bp'])
    lg, E_lg = R.ref_linear_fwd(got['pooled'], c['Wl'], c['bl'])
    if not backward:
        return dict(pooled=R.worst_ratio(got['pooled'], fwd['pooled'], fwd['E_pooled']), logits=R.worst_ratio(got['logits'], lg, E_lg))
    bw = R.ref_head_bwd(c, got['pooled'])
    out = dict(pooled=R.worst_ratio(got['pooled'], fwd['pooled'], fwd['E_pooled']), logits=R.worst_ratio(got['logits'], lg, E_lg))
    for k in ('dpooled', 'dpre', 'dWp', 'dbp', 'dWl', 'dbl', 'dh0', 'dh0_add'):
        out[k] = R.worst_ratio(got[k], bw[k], bw['E_' + k])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_case_lists_hold_what_they_promise():
    shapes = R.SHAPES
    # conditions on the list, not measurements
    assert any(H % 4 for _, _, H, _ in shapes) and any(H > 1024 for _, _, H, _ in shapes) and any(H > 1024 and H % 4 for _, _, H, _ in shapes)
    assert any(R.workgroups(s) < 16 for s in shapes) and any(R.workgroups(s) == 1 for s in shapes)
    assert any(B > 64 for B, _, _, _ in shapes) and any(B % 4 for B, _, _, _ in shapes) and any(L == 1 for _, L, _, _ in shapes)
    assert any(Cn == H for _, _, H, Cn in shapes) and any(H == 4096 for _, _, H, _ in shapes) and all(Cn <= 16 for _, _, _, Cn in shapes)
    assert {B for B, _, _, _ in shapes} >= {64, 65, 129} and set(R.PATTERN_SHAPES) <= set(shapes) and len(set(shapes)) == len(shapes)
    assert sorted(set(R.cases())) == sorted(R.cases()) and {p for _, p in R.cases()} == set(R.PATTERNS)
    for shape, pattern in R.cases():
        c = R.head_case(shape, pattern)
        B, L, H, Cn = shape
        assert c['hidden'].shape == (B, L, H) and c['Wp'].shape == (H, H) and c['Wl'].shape == (Cn, H) and c['dlog'].shape == (B, Cn)
        for k in ('hidden', 'Wp', 'bp', 'Wl', 'bl', 'dlog', 'dWp0', 'dbp0', 'dWl0', 'dbl0', 'dh_prev'):
            a = c[k]
            assert a.dtype == F and np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= TINY)).all(), (shape, pattern, k)
        for k in ('dWp0', 'dbp0', 'dWl0', 'dbl0', 'dh_prev'):                  # the accumulators never start from zeros
            assert (c[k] != 0).all(), (shape, pattern, k)
        fwd = R.ref_pooler_fwd(c['hidden'], c['Wp'], c['bp'])
        with np.errstate(over='ignore'):
            p32 = np.tanh((fwd['pre']).astype(F))
        h0 = c['hidden'][:, 0].astype(np.float64)
        if pattern == 'saturated':
            rows = c['sat_rows']
            assert rows and rows[0] == 0 and (B == 1 or len(rows) < B)
            assert fwd['saturated'][rows].all() and (np.abs(fwd['pre'][rows]) - fwd['E_pre'][rows] >= R.T_SAT).all()
            assert (np.abs(p32[rows]) == 1.0).all()                            # really +-1 in fp32 ...
            for b in rows:
                assert {-1.0, 1.0} <= set(p32[b].tolist())                     # ... with both signs in every sample
            # (at the threshold float64 tanh is 1 and fp32 tanh with it; at 8 neither is)
            assert np.tanh(R.T_SAT) == 1.0 and np.tanh(F(R.T_SAT)) == ONE and np.tanh(F(8.0)) < ONE and np.tanh(R.T_SAT - 0.5) < 1.0
        elif pattern == 'near_sat':
            assert (np.abs(fwd['pre']) > 6.0).all() and (np.abs(fwd['pre']) < 8.0).all()
            assert (np.abs(p32) < 1.0).all() and not fwd['saturated'].any()
            assert (1.0 - p32.astype(np.float64) ** 2 < 2.0 ** -15).all()
        elif pattern == 'zero_pre':
            assert not c['hidden'][:, 0].any() and not c['bp'].any() and (L == 1 or c['hidden'][:, 1:].all())
        elif pattern == 'zero_dlog':
            assert not c['dlog'].any()
        elif pattern == 'cancel':
            rows = c['cancel_rows']
            assert rows == sorted({0, B - 1})
            W = c['Wp'].astype(np.float64)
            for b in rows:
                s = np.abs(h0[b]) @ np.abs(W).T + np.abs(c['bp'])
                assert (s / np.abs(fwd['pre'][b]) > R.CANCEL_FACTOR).all(), (shape, b)
                assert np.abs(h0[b]).max() > 1e4
            lg = fwd['pooled'] @ c['Wl'].astype(np.float64).T + c['bl']
            s = np.abs(fwd['pooled']) @ np.abs(c['Wl'].astype(np.float64)).T + np.abs(c['bl'])
            assert (s / np.abs(lg) > R.CANCEL_FACTOR).all(), shape
        else:
            assert (np.abs(fwd['pre']) < 6.0).all() and not fwd['saturated'].any()


def test_fp32_restatement_stays_within_half_of_every_bound():
    shares = {}
    for shape, pattern in R.cases():
        c = R.head_case(shape, pattern)
        for mode in MODES:
            for k, v in ratios(c, mode).items():
                shares[k] = max(shares.get(k, 0.0), v)
    print('worst |fp32 - float64| / bound: ' + ', '.join('%s %.3f' % (k, shares[k]) for k in QUANTITIES))
    for k in QUANTITIES:
        assert shares[k] <= 0.5, (k, shares[k])


def test_exact_patterns_are_exact_in_the_restatement():
    """the equalities the GPU test asserts hold for any evaluation order of the formulas"""
    for shape in R.PATTERN_SHAPES:
        for mode in MODES:
            c = R.head_case(shape, 'zero_pre')
            g = head32(c, mode)
            assert not g['pooled'].any() and np.array_equal(g['logits'], np.broadcast_to(c['bl'], g['logits'].shape))
            c = R.head_case(shape, 'saturated')
            g = head32(c, mode)
            rows = c['sat_rows']
            assert (np.abs(g['pooled'][rows]) == 1.0).all() and not g['dpre'][rows].any() and not g['dh0'][rows].any()
            c = R.head_case(shape, 'zero_dlog')
            g = head32(c, mode)
            assert not g['dh0'].any() and all(np.array_equal(g[k], c[k + '0']) for k in ('dWp', 'dbp', 'dWl', 'dbl'))


# bug -> (the cases at which it must fail: a predicate on the shape, all with the randn pattern; the quantities that must leave)
WRONG = {
    'row1': (lambda B, L, H, Cn: L > 1, ('pooled',)),                         # row 1 of hidden where row 0 belongs
    'drop_tail': (lambda B, L, H, Cn: H % 64 != 0, ('pooled',)),              # the last H % 64 columns dropped
    'logits_1024': (lambda B, L, H, Cn: H > 1024, ('logits',)),               # columns >= 1024 of the logits dropped
    'one_minus_p': (lambda B, L, H, Cn: H < 4096, ('dpre', 'dWp', 'dbp', 'dh0')),  # 1 - p where 1 - p^2 belongs
    'batch_64': (lambda B, L, H, Cn: B > 64, ('dWp', 'dbp')),                 # batch rows >= 64 skipped in dWp
    'assign': (lambda B, L, H, Cn: H < 4096, ('dWp', 'dbp', 'dWl', 'dbl')),       # assigned where the weight gradients accumulate
    'no_bp': (lambda B, L, H, Cn: H < 4096, ('pooled',)),                         # bp omitted
    'wl_swapped': (lambda B, L, H, Cn: Cn > 1, ('logits',)),                  # Wl read as [k][c]
}


@pytest.mark.parametrize('bug', list(WRONG))
def test_a_wrong_formula_leaves_the_bound(bug):
    where, need = WRONG[bug]
    shapes = [s for s in R.SHAPES if where(*s)]
    assert shapes
    least = {k: float('inf') for k in need}
    for shape in shapes:
        r = ratios(R.head_case(shape, 'randn'), 'tree', bug, backward=not set(need) <= {'pooled', 'logits'})
        for k in need:                                                        # every named case catches it on its own
            assert r[k] > 1.0, (bug, shape, k, r[k])
            least[k] = min(least[k], r[k])
    print('%s: times over the bound, the least over %d cases: ' % (bug, len(shapes)) + ', '.join('%s %.3g' % kv for kv in least.items()))
