"""tests/optim_kinds_ref.py checks itself: a numpy-fp32 evaluation of the Adamax and SGD-momentum contracts stays within HALF of
every bound of ref_step_adamax / ref_step_sgd over the grid step x gradient size x (lr, wd) x state x clip mode of
tests/test_optim_bounds_cpu.py; wrong formulas each leave the bound; and the contract IS torch's: torch.optim.Adamax and
torch.optim.SGD in float64 on the CPU, with the decay / no-decay groups, clip_grad_norm_ and several steps, agree with
ref_step_* to 1e-12 (float64 against float64: an identity up to the order of a few additions, not a measured tolerance).
No GPU, no library.

Recorded on the grid below (240 cases of 2^14 elements per rule), worst |fp32 - float64| as a share of the C = 16 bound:
Adamax p 0.083, m 0.233, u 0.216; SGD p 0.102, b 0.235.  With the norm at 1e-3 against max_norm 1e-4 (the coefficient's own
roundings; held to the bound itself): Adamax p 0.096, m 0.252, u 0.233; SGD p 0.062, b 0.230.  Wrong formulas, times over the
bound: Adamax with eps outside the max 5.2e5 (u), without bias correction 3.2e5 (p), without b2 1.0e3 (u), with decoupled decay
1.0e6 (m); SGD with dampening 9.4e5 (b), Nesterov 5.2e5 (p), decoupled decay 1.0e6 (b)."""
import itertools
import math

import numpy as np
import pytest
import torch

import optim_kinds_ref as K
import optim_ref as R

N = 2 ** 14
F = np.float32
STEPS = (1, 2, 10, 1000, 100000)
GMAGS = (1e-8, 1e-3, 1.0, 1e4)
LRWD = ((3e-5, 1e-3), (1e-3, 1e-2), (1e-3, 0.0))
KINDS = {'adamax': K.KIND_ADAMAX, 'sgd': K.KIND_SGD}
BUGS = {'adamax': ('eps_outside_max', 'no_bias_correction', 'no_b2', 'decoupled_decay'),
        'sgd': ('dampening', 'nesterov', 'decoupled_decay')}
# the quantity in which each wrong formula must leave the bound somewhere on the grid
NEED = {'eps_outside_max': ('v', 'p'), 'no_bias_correction': ('p',), 'no_b2': ('v', 'p'), 'dampening': ('m', 'p'),
        'nesterov': ('p',), 'decoupled_decay': ('m',)}


def _grid(clips=('off', 'active')):
    for i, (step, gmag, (lr, wd), mom) in enumerate(itertools.product(STEPS, GMAGS, LRWD, R.MOMENTS)):
        yield i, dict(step=step, gmag=gmag, lr=lr, wd=wd, moments=mom, clip=clips[(i + i // 4) % len(clips)])


def _coef32(h, sumsq):
    gscale, max_norm = F(h.gscale), F(h.max_norm)
    coef = gscale
    if h.max_norm > 0 and sumsq is not None:
        total = F(math.sqrt(sumsq)) * gscale
        c = max_norm / (total + F(1e-6))
        coef = gscale * min(c, F(1))
    return coef


def fp32_adamax(p, g, m, u, flags, h, sumsq, bug=None):
    """the contract, every operation rounded to fp32, in the order the text gives them"""
    lr, b1, b2, eps, one = F(h.lr), F(h.b1), F(h.b2), F(h.eps), F(1)
    wd = np.where((R.expand_flags(flags, p.size) & 3) == 2, F(h.wd), F(0))
    bc1 = 1.0 - h.b1 ** h.step
    step_size = F(h.lr) if bug == 'no_bias_correction' else F(h.lr / bc1)
    gg, p0 = g * _coef32(h, sumsq), p
    if bug == 'decoupled_decay':
        p0 = p * (one - lr * wd)
    else:
        gg = gg + wd * p
    m1 = b1 * m + (one - b1) * gg
    if bug == 'eps_outside_max':
        u1 = np.maximum(b2 * u, np.abs(gg)) + eps
    elif bug == 'no_b2':
        u1 = np.maximum(u, np.abs(gg) + eps)
    else:
        u1 = np.maximum(b2 * u, np.abs(gg) + eps)
    p1 = p0 - step_size * (m1 / u1)
    assert p1.dtype == m1.dtype == u1.dtype == np.float32
    return dict(p=p1, m=m1, v=u1)


def fp32_sgd(p, g, b, flags, h, sumsq, bug=None):
    lr, mu, one = F(h.lr), F(h.b1), F(1)
    wd = np.where((R.expand_flags(flags, p.size) & 3) == 2, F(h.wd), F(0))
    gg, p0 = g * _coef32(h, sumsq), p
    if bug == 'decoupled_decay':
        p0 = p * (one - lr * wd)
    else:
        gg = gg + wd * p
    b1 = mu * b + ((one - mu) * gg if bug == 'dampening' else gg)
    p1 = p0 - lr * ((gg + mu * b1) if bug == 'nesterov' else b1)
    assert p1.dtype == b1.dtype == np.float32
    return dict(p=p1, m=b1)


def _ratios(rule, case, seed, bug=None):
    kind = KINDS[rule]
    p, g, m, v, flags, h, sumsq = K.build_kind_case(kind, N, seed, **case)
    ref = K.ref_step_kind(kind, p, g, m, v, flags, h, sumsq)
    with np.errstate(all='ignore'):
        got = fp32_adamax(p, g, m, v, flags, h, sumsq, bug) if kind == K.KIND_ADAMAX else fp32_sgd(p, g, m, flags, h, sumsq, bug)
    return {k: R.worst_ratio(got[k], ref[k], ref['E_' + k]) for k in got}


def test_the_adamax_state_is_free_of_subnormals_and_of_the_gradients_size():
    tiny = float(np.finfo(np.float32).tiny)
    for i, case in _grid():
        p, g, m, u, flags, h, sumsq = K.build_kind_case(K.KIND_ADAMAX, N, i, **case)
        assert u.dtype == np.float32 and ((u == 0) | (u >= 1e3 * tiny)).all(), case
        ge = case['gmag'] * R.clip_coef(sumsq, h)
        if case['moments'] == 'warm' and case['gmag'] >= 1e-3:      # (at 1e-8 the + 1e-6 of the clip decides the coefficient)
            assert 0.2 * ge < np.median(u) < 5 * ge, case
        assert K.build_kind_case(K.KIND_SGD, 64, i, **case)[3] is None


@pytest.mark.parametrize('rule', list(KINDS))
def test_fp32_evaluation_of_the_contract_stays_within_half_of_every_bound(rule):
    worst = {}
    for i, case in _grid():
        r = _ratios(rule, case, i)
        for k in r:
            assert r[k] <= 0.5, (rule, k, r[k], case)
            worst[k] = max(worst.get(k, 0.0), r[k])
    print('%s: worst error / bound on %d elements per case: ' % (rule, N) + ', '.join('%s %.3f' % kv for kv in worst.items()))


@pytest.mark.parametrize('rule', list(KINDS))
def test_fp32_evaluation_with_the_clip_at_a_norm_of_1e_3_stays_within_the_bound(rule):
    """(as in test_optim_bounds_cpu.py: the coefficient's own chain adds five roundings to every g coef, which the half-margin of
    the grid above does not count)"""
    worst = {}
    for i, case in _grid(('tiny',)):
        if i % 3 == 0:
            r = _ratios(rule, case, i)
            for k in r:
                assert r[k] <= 1.0, (rule, k, r[k], case)
                worst[k] = max(worst.get(k, 0.0), r[k])
    print('%s, clip at 1e-3: worst error / bound: ' % rule + ', '.join('%s %.3f' % kv for kv in worst.items()))


@pytest.mark.parametrize('rule', list(KINDS))
def test_zero_momentum_and_the_other_clip_modes_stay_within_half_of_every_bound(rule):
    cases = [dict(b1=0.0, step=1, moments='zero'), dict(b1=0.0, step=10), dict(clip='null'), dict(clip='zero'),
             dict(clip='zero', moments='zero'), dict(clip='null', wd=0.0, moments='zero')]
    for i, case in enumerate(cases):
        r = _ratios(rule, case, 1000 + i)
        assert max(r.values()) <= 0.5, (rule, r, case)


@pytest.mark.parametrize('rule,bug', [(r, b) for r in BUGS for b in BUGS[r]])
def test_a_wrong_formula_leaves_the_bound(rule, bug):
    over = {}
    for i, case in _grid(('off', 'active', 'tiny')):
        if i % 5:             # (a fifth of the grid; 5 is prime to every axis length but the steps', which i // 48 walks anyway)
            continue
        r = _ratios(rule, case, i, bug)
        for k in r:
            over[k] = max(over.get(k, 0.0), r[k])
    print('%s, %s: times over the bound: ' % (rule, bug) + ', '.join('%s %.3g' % kv for kv in over.items()))
    assert any(over[k] > 1.0 for k in NEED[bug]), (rule, bug, over)


# ---------------------------------------------------------------------------------------------------------------------------
# the contract is torch's
# ---------------------------------------------------------------------------------------------------------------------------
def _torch_steps(rule, steps, max_norm_factor, seed):
    """`steps` steps of torch.optim.<rule> in float64 on one parameter per 64-element chunk (flag 0: no gradient, flag & 3 == 2: the
    weight-decay group) with clip_grad_norm_ in front; every step against ONE float64 reference step from torch's own state before it"""
    kind = KINDS[rule]
    n = 64 * 40
    flags = R.make_flags(n // 64, seed)
    h = R.Hyper(lr=1e-3, b1=0.9, wd=1e-2, gscale=0.125)
    # (no planted cancellations, coef_hint = 0: torch scales the gradient in two roundings where the contract has one, which a
    # cancellation to 1e-6 would magnify to 1e-10 -- of the sum, not of its terms; the bound's own terms are what 1e-12 is held against)
    p, _, m, v = R.make_case(n, seed, 1.0, 'zero', h.wd, coef_hint=0.0)
    p, m = p.astype(np.float64), np.zeros(n)
    u = np.zeros(n)
    live = R.expand_flags(flags, n) != 0
    params = [torch.nn.Parameter(torch.tensor(p[c * 64:(c + 1) * 64])) for c in range(n // 64)]
    groups = [{'params': [q for q, f in zip(params, flags) if f & 3 == 2], 'weight_decay': h.wd},
              {'params': [q for q, f in zip(params, flags) if f & 3 != 2], 'weight_decay': 0.0}]
    if rule == 'adamax':
        opt = torch.optim.Adamax(groups, lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, foreach=False)
    else:
        opt = torch.optim.SGD(groups, lr=h.lr, momentum=h.b1, foreach=False)
    for k in range(1, steps + 1):
        g = R.make_case(n, seed + k, 1.0, 'zero', h.wd, coef_hint=0.0)[1].astype(np.float64)
        sumsq = R.ref_sumsq(g, flags)
        hk = h.replace(step=k, max_norm=max_norm_factor * math.sqrt(sumsq) * h.gscale)
        for c, q in enumerate(params):
            q.grad = torch.tensor(g[c * 64:(c + 1) * 64]) * h.gscale if flags[c] else None      # average_gradients
        if hk.max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, hk.max_norm)
        opt.step()
        ref = K.ref_step_kind(kind, p, g, m, u, flags, hk, sumsq if hk.max_norm > 0 else None)
        got = dict(p=torch.cat([q.detach() for q in params]).numpy())
        st = [opt.state[q] for q in params]
        zero = torch.zeros(64, dtype=torch.float64)
        if rule == 'adamax':
            got['m'] = torch.cat([s.get('exp_avg', zero) for s in st]).numpy()
            got['v'] = torch.cat([s.get('exp_inf', zero) for s in st]).numpy()
        else:
            got['m'] = torch.cat([zero if s.get('momentum_buffer') is None else s['momentum_buffer'] for s in st]).numpy()
        for key in got:
            tol = 1e-12 * ref['E_' + key] / (R.C * R.U)          # 1e-12 of the terms the bound is relative to
            err = np.abs(got[key] - ref[key])
            assert (err[live] <= tol[live]).all(), (rule, k, key, float((err[live] / tol[live]).max()))
        assert np.array_equal(got['p'][~live], p[~live])          # no gradient: torch skips the parameter, decay included
        p, m = got['p'], got['m']
        if rule == 'adamax':
            u = got['v']
    assert set(flags) == {0, 1, 2, 5, 6}


@pytest.mark.parametrize('clip', ['off', 'inactive', 'active'])
@pytest.mark.parametrize('rule', list(KINDS))
def test_the_reference_is_torchs_optimizer_in_float64(rule, clip):
    _torch_steps(rule, 5, {'off': 0.0, 'inactive': 10.0, 'active': 0.1}[clip], 7)
