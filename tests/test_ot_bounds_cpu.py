"""tests/ot_ref.py checks itself.  No GPU, no library.

1. The case list is what it claims: every shape passes the entry points' own checks, the list covers the sizes, paddings, input kinds,
   beta and iteration values the kernels branch on, no unpadded row has a norm near the clamp, and the fp32 yardstick of EVERY case
   is finite in all four quantities -- tests/test_ot_f64_gpu.py runs every case, none is skipped or waived.
2. reference() is oracle/ot_oracle.py: called directly on the widened inputs the oracle returns the same numbers.
3. MARGIN[q] e_ref(q) never exceeds the tolerance tests/test_ot_gpu.py applies to the same quantity, and it rejects every formula of
   ot_ref.MUTANTS on at least one case and quantity -- the standing proof that the measured margins are still tight enough to matter.
   The two EQUIVALENT mutants (derivation in ot_ref.py) leave all four quantities where they were, to a millionth of e_ref.

Recorded with the margins of ot_ref.py (dist 3, T 8, dx 4, dy 5), the number of the 52 cases that reject a mutant and the most it
exceeds a bound by, in bounds (test_every_mutant_is_rejected prints them, -s): bwd_no_projection 50, 1.6e6 and more (and any
difference at all on D1, whose dy bound is 0); bwd_no_clamp_branch 2 (the tiny_rows cases), 2.9e3; pad_1e4_dropped 44 (every padded
case: NaN); y_len_for_x_len 48, 1.9e8; plan_untransposed 49, 1.5e6; beta_doubled 44, 4.3e5; g_of_sample_0 49, 3.4e6;
plan_padding_never_zeroed 2 (it0, it0_65x3), 1.0e6; one_step_fewer 44, 2.8e8 (it1; 4.1e5 at it2).  The whole file takes 9 s."""
import math

import pytest
import torch

import ot_ref as R
from oracle import ot_oracle as OT


def _unpadded_norms(d):
    return torch.cat([d['x'].double().norm(dim=-1)[~d['x_pad']], d['y'].double().norm(dim=-1)[~d['y_pad']]])


def test_case_list_covers_what_the_kernels_branch_on():
    C = R.CASES
    assert {c['D'] for c in C} >= {1, 7, 31, 32, 33, 63, 64, 65, 255, 256, 257, 768}
    assert {(c['M'], c['N']) for c in C} >= {(1, 1), (5, 3), (64, 64), (65, 3), (3, 65), (63, 36), (60, 36), (128, 64), (100, 100),
                                             (300, 1), (1, 300), (257, 30)}
    assert {c['beta'] for c in C} == {0.05, 0.1, 0.5, 1.0, 2.0} and {c['iteration'] for c in C} == {0, 1, 2, 50, 200}
    assert {c['pad'] for c in C} == {'none', 'suffix', 'middle', 'one_txt', 'one_img', 'one_each'}
    assert {c['kind'] for c in C} == {'randn', 'aligned', 'anti', 'scaled', 'zero_rows', 'tiny_rows'}
    assert {c['g'] for c in C} == {'ones', 'rand', 'zero', 'big'}
    assert {c['B'] for c in C} >= {1, 2, 3, 4, 70}
    assert any((c['M'], c['N'], c['D'], c['beta'], c['iteration']) == (60, 36, 768, 0.5, 50) for c in C)      # the model's own
    for c in C:
        assert c['M'] * c['N'] <= 12288 and R.lds_bytes(c['M'], c['N']) <= 160 * 1024, c['id']
        assert c['B'] in (1, 70) or 2 <= c['B'] <= 4, c['id']


@pytest.mark.parametrize('case_id', R.CASE_IDS)
def test_case_is_well_posed_and_its_yardstick_finite(case_id):
    c = R.BY_ID[case_id]
    d, ref, e, finite = R.solved(case_id)
    assert finite, 'the fp32 evaluation is not finite: the case does not belong in CASES'
    assert all(math.isfinite(e[q]) for q in R.QUANTITIES)
    x_pad, y_pad = d['x_pad'], d['y_pad']
    assert (~x_pad).sum(1).min() >= 1 and (~y_pad).sum(1).min() >= 1, 'a side padded entirely is out of scope'
    n = _unpadded_norms(d)
    assert ((n < 0.5 * R.EPS) | (n > 2 * R.EPS)).all(), 'a norm near the clamp'
    # the patterns do what their names say
    if c['pad'] == 'middle':
        for p in ((x_pad, y_pad) if min(c['M'], c['N']) >= 3 else (x_pad,) if c['M'] >= 3 else (y_pad,)):
            assert (p[:, :-1] & ~p[:, 1:]).any(), 'no flag in the middle'
        assert c['B'] == 1 or not all(torch.equal(x_pad[0], x_pad[b]) and torch.equal(y_pad[0], y_pad[b]) for b in range(1, c['B']))
    if c['pad'] in ('one_txt', 'one_each'):
        assert ((~x_pad).sum(1) == 1).all() and len({int((~x_pad[b]).nonzero()) for b in range(c['B'])}) == c['B']
    if c['pad'] in ('one_img', 'one_each'):
        assert ((~y_pad).sum(1) == 1).all() and len({int((~y_pad[b]).nonzero()) for b in range(c['B'])}) == c['B']
    if c['kind'] == 'zero_rows':
        assert (n == 0).sum() == 4
    if c['kind'] == 'tiny_rows':
        assert ((n > 0) & (n < 0.5 * R.EPS)).sum() == 4
    if c['kind'] == 'aligned':
        assert ref['T'].max() > 3 * ref['T'][ref['T'] > 0].median()                  # a peaked plan
    if c['g'] == 'zero':
        assert (d['g'] == 0).sum() == 1 and (ref['dx'][d['g'] == 0] == 0).all()
    if c['g'] == 'big':
        assert d['g'].abs().max() == 1e3
    # the bound is never wider than what tests/test_ot_gpu.py allows the same quantity
    for q in R.QUANTITIES:
        assert R.MARGIN[q] * e[q] <= R.OLD_TOL[q] * max(1.0, ref[q].abs().max().item()), (q, e[q])


@pytest.mark.parametrize('case_id', R.CASE_IDS)
def test_reference_is_the_oracle(case_id):
    d, ref, _, _ = R.solved(case_id)
    x, y = d['x'].double().requires_grad_(True), d['y'].double().requires_grad_(True)
    assert torch.equal(x.detach().float(), d['x']) and torch.equal(y.detach().float(), d['y'])      # widened exactly
    dist, T, _ = OT.optimal_transport_dist(x, y, d['x_pad'], d['y_pad'], float(torch.tensor(d['beta'], dtype=torch.float32)),
                                           d['iteration'])
    dx, dy = torch.autograd.grad((dist * d['g'].double()).sum(), (x, y))
    for q, v in zip(R.QUANTITIES, (dist.detach(), T, dx, dy)):
        assert v.dtype == ref[q].dtype == torch.float64 and v.shape == ref[q].shape
        assert (v - ref[q]).abs().max().item() <= 1e-12 * max(ref[q].abs().max().item(), 1e-300), q
    B, M, N, D = (R.BY_ID[case_id][k] for k in 'BMND')
    assert ref['dist'].shape == (B,) and ref['T'].shape == (B, N, M) and ref['dx'].shape == (B, M, D) and ref['dy'].shape == (B, N, D)


def _rejections(name):
    """{case id: the most a quantity of mutant `name` exceeds its bound by, in bounds} over the cases that reject it"""
    out = {}
    for case_id in R.CASE_IDS:
        d, ref, e, _ = R.solved(case_id)
        m = R.mutant(name, *R.args(d))
        w = max(R.ratio(m[q], ref[q], R.MARGIN[q] * e[q]) for q in R.QUANTITIES)
        if w > 1.0:
            out[case_id] = w
    return out


@pytest.mark.parametrize('name', R.MUTANTS)
def test_every_mutant_is_rejected(name):
    caught = _rejections(name)
    print('%s: rejected by %d of %d cases, by up to %.3g bounds (%s)' % ((name, len(caught), len(R.CASES)) + max(
        ((w, c) for c, w in caught.items()), default=(0.0, '-'))))
    assert caught, 'no case rejects %s: the margins are too loose' % name
    if name == 'one_step_fewer':                 # the unconverged cases; with no iteration there is no step to lose
        assert set(caught) >= {c['id'] for c in R.CASES if c['iteration'] in (1, 2)}
        assert not set(caught) & {c['id'] for c in R.CASES if c['iteration'] == 0}
    if name == 'plan_padding_never_zeroed':      # A is zero at the padding: only a plan that is never multiplied by it shows
        assert set(caught) == {c['id'] for c in R.CASES if c['iteration'] == 0 and c['pad'] != 'none'} != set()
    if name == 'bwd_no_clamp_branch':            # an exactly zero row has no projection to lose
        assert set(caught) == {c['id'] for c in R.CASES if c['kind'] == 'tiny_rows'} != set()
    if name == 'plan_untransposed':              # the flat [N][M] plan read as [M][N]: for M != N no transposition of anything
        assert any(R.BY_ID[c]['M'] != R.BY_ID[c]['N'] for c in caught)
    if name == 'g_of_sample_0':
        assert 'B1' not in caught and 'g_ones' not in caught


@pytest.mark.parametrize('name', R.EQUIVALENT)
def test_equivalent_mutants_change_nothing(name):
    for case_id in R.CASE_IDS:
        d, ref, e, _ = R.solved(case_id)
        m = R.mutant(name, *R.args(d))
        for q in R.QUANTITIES:
            assert (m[q] - ref[q]).abs().max().item() <= 1e-6 * e[q], (name, case_id, q)
