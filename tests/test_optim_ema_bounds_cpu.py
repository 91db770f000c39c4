"""tests/optim_ema_ref.py checks itself: a numpy-fp32 evaluation of the averaged weights' contract, in the stated order, stays within
HALF of the bound of ref_avg over rule x step x weight; the host's weight sequence (trainer.ema_weight) is the stated formula for
t = 0 .. 200 with and without warm-up; and four wrong forms each leave the bound by a large factor on the same inputs, on which the
correct form alone stays inside.  No GPU, no library.

p' is what an fp32 evaluation of the step's own contract gives (test_optim_bounds_cpu.fp32_step) on optim_ref's cases, so
|p' - p| is an optimizer step's (about lr), and a comes from optim_ema_ref.make_avg (|p' - a| of the order of |a|).

Recorded: worst |fp32 - float64| as a share of the C = 16 bound 0.114; wrong forms, times over the bound (the least over the three
weights): w and 1 - w exchanged 7.7e5, the average of the old p 6.7e3, warm-up off by one step 9.8e3, skipped chunks averaged:
infinite (their bound is 0)."""
import itertools
import math

import numpy as np
import pytest

import optim_ema_ref as E
import optim_ref as R
import test_optim_bounds_cpu as B

N = 2 ** 13
F = np.float32
BUGS = ('w_exchanged', 'old_p', 'warmup_off_by_one', 'skipped_averaged')
DECAY = 0.999


def fp32_avg(a, p_new, w, upd):
    """the contract, every operation rounded to fp32, in the order the text gives: the difference, the product, the sum"""
    w = F(w)
    with np.errstate(all='ignore'):
        d = (p_new - a).astype(F)
        inc = (w * d).astype(F)
        out = (a + inc).astype(F)
    assert out.dtype == np.float32
    return np.where(upd, out, a)


def _case(seed, w, adamw=0, step=3, lr=1e-3):
    p, g, m, v, flags, h, sumsq = R.build_case(N, seed, adamw=adamw, step=step, lr=lr, clip='active')
    p1 = B.fp32_step(p, g, m, v, flags, h, sumsq)[0]
    upd = (R.expand_flags(flags, N) & 3) != 0
    a = E.make_avg(p, seed + 7)
    return p, p1, a, upd, R.f32(w)


def _ratio(seed, w, bug=None, t=None, **kw):
    p, p1, a, upd, w = _case(seed, w, **kw)
    if t is not None:            # the weight of averaging step t of a run with warm-up
        w = E.ref_weight(DECAY, t)
    ref = E.ref_avg(a, p1, w, upd)
    if bug == 'w_exchanged':
        got = fp32_avg(a, p1, 1.0 - w, upd)
    elif bug == 'old_p':
        got = fp32_avg(a, p, w, upd)
    elif bug == 'warmup_off_by_one':
        got = fp32_avg(a, p1, E.ref_weight(DECAY, t + 1), upd)
    elif bug == 'skipped_averaged':
        got = fp32_avg(a, p1, w, np.ones_like(upd))
    else:
        got = fp32_avg(a, p1, w, upd)
    return R.worst_ratio(got, ref['a'], ref['E_a'])


def test_inputs_put_the_difference_at_the_size_of_the_average():
    for seed, w in enumerate(E.WEIGHTS):
        p, p1, a, upd, _ = _case(seed, w)
        rel = np.abs(p1.astype(np.float64) - a) / np.abs(a)
        assert np.quantile(rel, 0.01) > 0.02 and 0.2 < np.median(rel) < 2.0      # (a is placed around the OLD p: a few p' land near it)
        assert (~upd).sum() >= 64 and upd.sum() >= 64
        moved = np.abs(p1.astype(np.float64) - p)[upd]
        assert np.median(moved) > 1e-5                    # an optimizer step's worth between the old and the new p
        tiny = float(np.finfo(np.float32).tiny)
        assert (np.abs(R.f32(w) * (p1.astype(np.float64) - a)) >= 1e3 * tiny).all()


def test_fp32_evaluation_in_the_stated_order_stays_within_half_of_the_bound():
    worst = 0.0
    for i, (w, adamw, step, lr) in enumerate(itertools.product(E.WEIGHTS + (0.0, 1.0), (0, 1), (1, 10, 1000), (3e-5, 1e-3))):
        r = _ratio(i, w, adamw=adamw, step=step, lr=lr)
        assert r <= 0.5, (r, w, adamw, step, lr)
        worst = max(worst, r)
    print('averaged weights: worst error / bound on %d elements per case: %.3f' % (N, worst))


def test_weights_zero_and_one_are_exact():
    p, p1, a, upd, _ = _case(5, 0.5)
    assert np.array_equal(fp32_avg(a, p1, 0.0, upd), a)
    ref = E.ref_avg(a, p1, 1.0, upd)
    assert R.worst_ratio(fp32_avg(a, p1, 1.0, upd), ref['a'], ref['E_a']) <= 0.5
    assert np.allclose(ref['a'][upd], p1[upd].astype(np.float64), rtol=0, atol=0)


@pytest.mark.parametrize('warmup', [True, False])
def test_host_weight_sequence_is_the_formula(warmup):
    from meme_challenge_amd import trainer
    for D in (0.9, 0.999, 0.9999):
        for t in range(201):
            d = min(D, (1 + t) / (10 + t)) if warmup else D
            w = trainer.ema_weight(D, t, warmup)
            assert w == 1.0 - d and isinstance(w, float)
            assert R.f32(w) == E.ref_weight(D, t, warmup)
            assert 0.0 < w < 1.0
    assert trainer.ema_weight(0.999, 0) == pytest.approx(0.9) and trainer.ema_weight(0.999, 1) == pytest.approx(1 - 2 / 11)
    assert trainer.ema_weight(0.999, 10 ** 6) == 1.0 - 0.999


@pytest.mark.parametrize('bug', BUGS)
def test_a_wrong_form_leaves_the_bound_and_the_right_one_does_not(bug):
    over = math.inf
    for seed, w in enumerate(E.WEIGHTS):
        t = (0, 3, 40)[seed] if bug == 'warmup_off_by_one' else None
        good, bad = _ratio(20 + seed, w, t=t), _ratio(20 + seed, w, bug=bug, t=t)
        assert good <= 0.5, (bug, w, good)
        over = min(over, bad)
    print('%s: at least %.3g times over the bound' % (bug, over))
    assert over > 100.0, (bug, over)
