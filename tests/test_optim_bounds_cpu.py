"""tests/optim_ref.py checks itself: a numpy-fp32 evaluation of the optimizer step's contract stays within HALF of every bound of
ref_step over the grid Adam / AdamW x step x gradient size x (lr, wd) x moment state x clip mode, and four wrong formulas each
leave the bound.  No GPU, no library, no torch.

Recorded on the grid below (480 cases of 2^14 elements, clip off and clip at coef ~ 0.1 in turn), worst |fp32 - float64| as a
share of the C = 16 bound: v 0.414, m 0.233, p 0.156; the clip norm (fp32 squares and pair sums, double accumulation) 0.014 of its
3 * 2^-24 bound.  With the norm at 1e-3 against max_norm 1e-4 the coefficient's own roundings show: v 0.505, m 0.252, p 0.156 (held
to the bound itself, see the test).  Wrong formulas, times over the bound: eps inside the bias correction 1.6e5 (p), bc2 dropped
6.4e6 (p), v fed the unclipped gradient 8e9 (v), coefficient off by 1e-5: 4.2 (p) / 10.7 (m) / 21.4 (v)."""
import itertools
import math

import numpy as np
import pytest

import optim_ref as R

N = 2 ** 14
F = np.float32
STEPS = (1, 2, 10, 1000, 100000)
GMAGS = (1e-8, 1e-3, 1.0, 1e4)
LRWD = ((3e-5, 1e-3), (1e-3, 1e-2), (1e-3, 0.0))
BUGS = ('eps_in_bc', 'no_bc2', 'v_unclipped', 'coef_1e-5')


def _grid(clips=('off', 'active')):
    for i, (adamw, step, gmag, (lr, wd), mom) in enumerate(itertools.product((0, 1), STEPS, GMAGS, LRWD, R.MOMENTS)):
        yield i, dict(adamw=adamw, step=step, gmag=gmag, lr=lr, wd=wd, moments=mom, clip=clips[(i + i // 4) % len(clips)])


def fp32_step(p, g, m, v, flags, h, sumsq, bug=None):
    """the contract, every operation rounded to fp32 (numpy float32 arrays and scalars), in the order the text gives them"""
    lr, b1, b2, eps, gscale, max_norm = F(h.lr), F(h.b1), F(h.b2), F(h.eps), F(h.gscale), F(h.max_norm)
    wd = np.where((R.expand_flags(flags, p.size) & 3) == 2, F(h.wd), F(0))
    coef = gscale
    if h.max_norm > 0 and sumsq is not None:
        total = F(math.sqrt(sumsq)) * gscale
        c = max_norm / (total + F(1e-6))
        coef = gscale * min(c, F(1))
    if bug == 'coef_1e-5':
        coef = F(float(coef) * (1.0 + 1e-5))
    bc1, bc2 = 1.0 - h.b1 ** h.step, 1.0 - h.b2 ** h.step
    step_size, rt_bc2 = F(h.lr / bc1), F(math.sqrt(bc2))
    one = F(1)
    gg = g * coef
    graw = g * gscale
    if h.adamw:
        p0 = p * (one - lr * wd)
    else:
        p0, gg, graw = p, gg + wd * p, graw + wd * p
    gv = graw if bug == 'v_unclipped' else gg
    m1 = b1 * m + (one - b1) * gg
    v1 = b2 * v + (one - b2) * (gv * gv)
    if bug == 'eps_in_bc':
        den = (np.sqrt(v1) + eps) / rt_bc2
    elif bug == 'no_bc2':
        den = np.sqrt(v1) + eps
    else:
        den = np.sqrt(v1) / rt_bc2 + eps
    p1 = p0 - step_size * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def fp32_sumsq(g, flags):
    """squares and pair sums in fp32, accumulation in double"""
    x = g[R.expand_flags(flags, g.size) != 0].astype(F)
    s = (x * x).reshape(-1, 2)
    return float(np.sum((s[:, 0] + s[:, 1]).astype(np.float64)))


def _ratios(case, seed, bug=None):
    p, g, m, v, flags, h, sumsq = R.build_case(N, seed, **case)
    ref = R.ref_step(p, g, m, v, flags, h, sumsq)
    p1, m1, v1 = fp32_step(p, g, m, v, flags, h, sumsq, bug)
    out = {k: R.worst_ratio(got, ref[k], ref['E_' + k]) for k, got in (('p', p1), ('m', m1), ('v', v1))}
    if bug is None and sumsq:
        out['sumsq'] = abs(fp32_sumsq(g, flags) - sumsq) / (R.SUMSQ_REL * sumsq)
    return out


def test_inputs_are_free_of_subnormals_and_hold_the_planted_values():
    tiny = float(np.finfo(np.float32).tiny)
    for i, case in list(_grid()) + list(_grid(('tiny',))):
        p, g, m, v, flags, h, sumsq = R.build_case(N, i, **case)
        coef = R.clip_coef(sumsq, h)
        gc = np.abs(g.astype(np.float64) * coef)
        assert ((gc == 0) | (gc >= 1e-12)).all(), case
        assert 0.1 < (g == 0).mean() < 0.2
        assert 0.08 < (np.abs(p - 1) < 0.01).mean() < 0.2
        for a in (p, m, v):
            assert ((a == 0) | (np.abs(a) >= 1e3 * tiny)).all(), case
        assert (np.diff(flags.astype(int)) != 0).all() and set(flags) == {0, 1, 2, 5, 6}
        if case['clip'] == 'tiny':
            assert 0.5e-3 < math.sqrt(sumsq) * h.gscale < 2e-3 and 0.05 < coef / h.gscale < 0.2
        if case['wd'] > 0 and not case['adamw'] and case['clip'] == 'off' and case['gmag'] == 1e-3:
            decay = (R.expand_flags(flags, N) & 3) == 2
            s = g.astype(np.float64) * coef + h.wd * p
            rel = np.abs(s) / (np.abs(h.wd * p) + 1e-300)
            assert (rel[decay] < 3e-6).mean() > 0.05, case      # the planted cancellations (a fifth, less the zeroed gradients and
                                                                    # those that would be far larger than the gradients)


def test_fp32_evaluation_of_the_contract_stays_within_half_of_every_bound():
    worst = dict(p=0.0, m=0.0, v=0.0, sumsq=0.0)
    for i, case in _grid():
        r = _ratios(case, i)
        for k in worst:
            assert r[k] <= 0.5, (k, r[k], case)
            worst[k] = max(worst[k], r[k])
    print('worst error / bound on %d elements per case: ' % N + ', '.join('%s %.3f' % kv for kv in worst.items()))


def test_fp32_evaluation_with_the_clip_at_a_norm_of_1e_3_stays_within_the_bound():
    """total * gscale about 1e-3 against max_norm 1e-4: the coefficient's own chain (the root rounded to fp32, x gscale, + 1e-6, the
    quotient, x gscale) adds five roundings to every g coef, ten to v, which the half-margin of the grid above does not count"""
    worst = dict(p=0.0, m=0.0, v=0.0)
    for i, case in _grid(('tiny',)):
        if i % 3 == 0:
            r = _ratios(case, i)
            for k in worst:
                assert r[k] <= 1.0, (k, r[k], case)
                worst[k] = max(worst[k], r[k])
    print('clip at 1e-3: worst error / bound: ' + ', '.join('%s %.3f' % kv for kv in worst.items()))


def test_b1_zero_and_the_other_clip_modes_stay_within_half_of_every_bound():
    cases = [dict(b1=0.0, step=1, moments='zero'), dict(b1=0.0, step=10, adamw=1), dict(clip='null'), dict(clip='zero'),
             dict(clip='zero', adamw=1, moments='zero'), dict(clip='null', wd=0.0, moments='zero')]
    for i, case in enumerate(cases):
        r = _ratios(case, 1000 + i)
        assert max(r['p'], r['m'], r['v']) <= 0.5, (r, case)


@pytest.mark.parametrize('bug', BUGS)
def test_a_wrong_formula_leaves_the_bound(bug):
    over = dict(p=0.0, m=0.0, v=0.0)
    for i, case in _grid(('off', 'active', 'tiny')):
        if i % 4 and not (bug == 'v_unclipped' and case['clip'] != 'off' and i % 2):
            continue
        r = _ratios(case, i, bug)
        for k in over:
            over[k] = max(over[k], r[k])
    print('%s: times over the bound: ' % bug + ', '.join('%s %.3g' % kv for kv in over.items()))
    need = {'eps_in_bc': ('p',), 'no_bc2': ('p',), 'v_unclipped': ('v',), 'coef_1e-5': ('p', 'm', 'v')}[bug]
    for k in need:
        assert over[k] > 1.0, (bug, k, over)
