"""uniter_bce_auc_logits (csrc/head.hip) through the C ABI, against the float64 reference, the case list and the bounds of
tests/auc_ref.py (derivation there; tests/test_auc_bounds_cpu.py is the standing proof that an fp32 evaluation of the formulas keeps
them and that wrong formulas do not).

Every output is prefilled with a recognisable NaN and carries GUARD elements behind its last one that must still hold the prefill
(the Vec of tests/test_adv_kernels_gpu.py); logits and labels must come back bit-identical; the bank's three arrays are compared
bit for bit with the reference's push, or with what they were.  The worst error / bound ratios per quantity are collected in WORST
and printed at the end of the module (-s shows them).
Recorded on an MI355X: total 0.029, bce 0.031, auc 0.044, probs 0.321, dlogits 0.104; 69 tests in 2 s."""
import itertools

import numpy as np
import pytest
import torch

import auc_ref as A
from test_adv_kernels_gpu import Vec as _Vec, _bits, _call

pytestmark = pytest.mark.gpu


class Vec(_Vec):
    """(with int32 vectors beside the float32 and int64 ones: bit patterns element by element, by the element's size)"""

    def _bits(self, a):
        return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


F = np.float32
WORST = {}
CASES = A.cases()
IDS = [n for n, _ in CASES]
BY_NAME = dict(CASES)
_REFS = {}


def _ref(name):
    if name not in _REFS:
        _REFS[name] = A.ref_of(BY_NAME[name])
    return _REFS[name]


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nuniter_bce_auc_logits, worst |got - float64| / bound: ' + ', '.join('%s %.3f' % kv for kv in WORST.items()))


def _hold(key, got, ref, bound, what=''):
    r = A.worst_ratio(got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, (key, what, r)


class DevBank(object):
    """the three arrays of an auc_ref.Bank on the device, each a Vec with its guard"""

    def __init__(self, bank):
        self.N = bank.N
        self.scores = Vec(bank.N, bank.scores)
        self.labels = Vec(bank.N, bank.labels, fill=-7, dtype=np.int32)
        self.state = Vec(2, bank.state(), fill=-7, dtype=np.int32)

    def ptrs(self):
        return self.scores.ptr(), self.labels.ptr(), self.state.ptr()

    def unchanged(self):
        return self.scores.unchanged() and self.labels.unchanged() and self.state.unchanged()

    def equals(self, bank):
        """bit for bit, NaN garbage included"""
        return (np.array_equal(_bits(self.scores.got()), _bits(bank.scores)) and np.array_equal(self.labels.got(), bank.labels) and
                self.state.got().tolist() == [bank.head, bank.fill] and self.scores.intact() and self.labels.intact() and self.state.intact())


def _launch(case, push, want=(1, 1, 1, 1), auc_weight=None):
    """-> (terms [3], n_pairs, probs [B], dlogits [B]), None for an output left out; inputs, the outputs left out and every guard
    are checked, and the bank against the reference's push (or for being untouched)"""
    z, y, bank = case['z'], case['y'], case['bank']
    B = z.size
    Z, Y = Vec(B, z), Vec(B, y, dtype=np.int64, fill=-7)
    outs = (Vec(3), Vec(1, fill=-7, dtype=np.int32), Vec(B), Vec(B))
    ptrs = [o.ptr() if w else None for o, w in zip(outs, want)]
    dev = DevBank(bank) if bank is not None else None
    bp, N = (dev.ptrs(), bank.N) if bank is not None else ((None, None, None), 0)
    aw = case['auc_weight'] if auc_weight is None else auc_weight
    _call('uniter_bce_auc_logits', Z.ptr(), Y.ptr(), case['pos_weight'], aw, case['kind'], case['margin'], *bp, N, int(push),
          *ptrs, case['grad_scale'], B)
    assert Z.unchanged() and Y.unchanged()
    if dev is not None:
        assert dev.equals(bank.pushed(z, y)) if push else dev.unchanged()
    res = []
    for o, w in zip(outs, want):
        assert o.intact() if w else o.unchanged()
        res.append(o.got() if w else None)
    return res


def _check(name, res):
    terms, n, probs, dlog = res
    ref = _ref(name)
    if terms is not None:
        for i, key in enumerate(('total', 'bce', 'auc')):
            _hold(key, terms[i], ref[key], ref['E_' + key], name)
        assert terms[2] >= 0 and (ref['n'] > 0 or terms[2] == 0)
    if n is not None:
        assert int(n[0]) == ref['n']
    if probs is not None:
        _hold('probs', probs, ref['probs'], ref['E_probs'], name)
    if dlog is not None:
        _hold('dlogits', dlog, ref['dlogits'], ref['E_dlogits'], name)


@pytest.mark.parametrize('name', IDS)
def test_matches_float64_and_pushes(name):
    """every case with a push (the bank afterwards is the reference's, bit for bit) and without one (the bank as it was); the
    two launches read the same bank, so their outputs are the same bits"""
    a, b = _launch(BY_NAME[name], push=1), _launch(BY_NAME[name], push=0)
    _check(name, a)
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


@pytest.mark.parametrize('name', ['B5_N8_fill3-logistic', 'B257_N1000-hinge2', 'B2_one_of_each-hinge2'])
def test_outputs_left_out_are_not_touched(name):
    """every combination of terms, n_pairs, probs and dlogits NULL or given: the given ones are right, the others untouched, the
    push happens all the same"""
    for want in itertools.product((0, 1), repeat=4):
        _check(name, _launch(BY_NAME[name], push=1, want=want))


@pytest.mark.parametrize('name', IDS)
def test_auc_weight_zero_is_bce_logits_bit_for_bit(name):
    """terms[0], terms[1], probs and dlogits; terms[2] and n_pairs still describe the pairs; the push still happens"""
    case = BY_NAME[name]
    terms, n, probs, dlog = _launch(case, push=1, auc_weight=0.0)
    B = case['z'].size
    Z, Y = Vec(B, case['z']), Vec(B, case['y'], dtype=np.int64, fill=-7)
    loss, p0, d0 = Vec(1), Vec(B), Vec(B)
    _call('uniter_bce_logits', Z.ptr(), Y.ptr(), case['pos_weight'], loss.ptr(), p0.ptr(), d0.ptr(), case['grad_scale'], B)
    assert _bits(terms[0]).tolist() == _bits(loss.got()[0]).tolist() == _bits(terms[1]).tolist()
    assert np.array_equal(_bits(probs), _bits(p0.got())) and np.array_equal(_bits(dlog), _bits(d0.got()))
    ref = _ref(name)
    assert int(n[0]) == ref['n']
    _hold('auc', terms[2], ref['auc'], ref['E_auc'], name)


@pytest.mark.parametrize('name', ['B257_N1000-logistic', 'B257_N1000_fill700-hinge2', 'label_2-logistic'])
def test_two_identical_launches_are_bit_equal(name):
    a, b = _launch(BY_NAME[name], push=1), _launch(BY_NAME[name], push=1)
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def test_the_hinge_is_exactly_zero_at_the_margin():
    """one positive, one negative, d == margin: auc 0, and the gradient is BCE's bits"""
    case = dict(BY_NAME['B2_one_of_each-hinge2'], z=np.array([1.5, 0.5], dtype=F))
    terms, n, probs, dlog = _launch(case, push=0)
    t0, _, _, d0 = _launch(case, push=0, auc_weight=0.0)
    assert int(n[0]) == 1 and terms[2] == 0.0 and _bits(terms[0]).tolist() == _bits(t0[0]).tolist()
    assert np.array_equal(np.abs(dlog), np.abs(d0))            # (a zero share may flip the sign of a zero, nothing else)


def test_successive_pushes_fill_the_ring_oldest_first():
    """three launches of B = 5 on ONE bank of 8 (the state stays on the device in between): the pairs of each launch are those
    with the bank as the launches before left it, and the bank ends with the last eight scores"""
    r = np.random.default_rng(7)
    bank = A.Bank(np.full(8, np.nan), np.ones(8), 0, 0)
    dev = DevBank(bank)
    for k in range(3):
        z, y = (2.0 * r.standard_normal(5)).astype(F), r.integers(0, 2, 5).astype(np.int64)
        Z, Y, T, Np = Vec(5, z), Vec(5, y, dtype=np.int64, fill=-7), Vec(3), Vec(1, fill=-7, dtype=np.int32)
        _call('uniter_bce_auc_logits', Z.ptr(), Y.ptr(), 1.8, 0.7, 0, 1.0, *dev.ptrs(), 8, 1, T.ptr(), Np.ptr(), None, None, 1.0, 5)
        ref = A.ref_bce_auc(z, y, 1.8, 0.7, 0, 1.0, 1.0, bank)
        assert int(Np.got()[0]) == ref['n']
        _hold('auc', T.got()[2], ref['auc'], ref['E_auc'], 'launch %d' % k)
        bank = bank.pushed(z, y)
        assert dev.equals(bank)
    assert (bank.head, bank.fill) == (7, 8)


def test_refusals_touch_nothing():
    from meme_challenge_amd import _lib as L
    case = BY_NAME['B5_N8_fill3-logistic']
    z, y, bank = case['z'], case['y'], case['bank']
    Z, Y, dev = Vec(5, z), Vec(5, y, dtype=np.int64, fill=-7), DevBank(bank)
    T, Np, P, Dl = Vec(3), Vec(1, fill=-7, dtype=np.int32), Vec(5), Vec(5)
    ok = [Z.ptr(), Y.ptr(), 1.8, 0.7, 0, 1.0, *dev.ptrs(), 8, 1, T.ptr(), Np.ptr(), P.ptr(), Dl.ptr(), 1.0, 5]
    for i, v in ((0, None), (1, None), (16, 0), (16, 4097), (9, 4), (9, 8193), (7, None), (8, None), (3, -1.0), (3, float('nan')),
                 (4, 2), (5, float('nan'))):
        args = list(ok)
        args[i] = v
        rc = L.lib().uniter_bce_auc_logits(*args, L.cur_stream())
        assert rc == -1 and L.lib().uniter_last_error(), (i, v, rc)
    torch.cuda.synchronize()
    assert all(v.unchanged() for v in (Z, Y, T, Np, P, Dl)) and dev.unchanged()
    _check('B5_N8_fill3-logistic', _launch(case, push=1))          # and the library is left in working order
