"""tests/auc_ref.py checks itself.  A numpy-fp32 restatement of uniter_bce_auc_logits as include/uniter_hip.h states it, written
independently of the reference (row by row over index lists, where the reference masks a matrix), stays within HALF of every bound
over every case of the shared list, with every sum taken serially and again as a pairwise tree (the worse of the two counts); the
reference's gradient is the central difference of its own loss; four wrong formulas leave the bounds; and the case list holds what
it promises.  No GPU, no library.

Recorded over the list (15 base cases x 2 surrogates), worst |fp32 - float64| as a share of the bound, the worse of the two orders:
total 0.052, bce 0.044, auc 0.064, probs 0.336, dlogits 0.104.
Wrong formulas, times over the bound on the worst case: normalising by B (B + N) 4.3e5 (auc) and 3.2e5 (dlogits); bank-bank pairs
counted 1.4e6 (auc); slots beyond `fill` counted inf (the NaN garbage reaches the sum); the negatives' gradient with the positives'
sign 7.8e5 (dlogits)."""
import numpy as np
import pytest

import auc_ref as A
from test_adv_bounds_cpu import sum32

F = np.float32
ONE, ZERO = F(1), F(0)
MODES = ('serial', 'tree')
KEYS = ('total', 'bce', 'auc', 'probs', 'dlogits')
BUGS = ('norm_all', 'bank_bank', 'beyond_fill', 'neg_sign')


def pair32(d, kind, margin):
    d = np.asarray(d, dtype=F)
    with np.errstate(all='ignore'):
        if kind == 0:
            e = np.exp(-np.abs(d))
            return np.maximum(-d, ZERO) + np.log1p(e), -(np.where(d >= 0, e, ONE) / (ONE + e))
        h = np.maximum(F(margin) - d, ZERO)
        return h * h, F(-2) * h


def bce_auc32(case, mode, bug=None):
    """fp32 throughout; index lists of the four sets, one row at a time"""
    z, y, bank = np.asarray(case['z'], dtype=F), np.asarray(case['y'], dtype=np.int64), case['bank']
    pw, aw, gs, kind, margin = F(case['pos_weight']), F(case['auc_weight']), F(case['grad_scale']), case['kind'], case['margin']
    B = z.size
    yf = y.astype(F)
    lw = ONE + (pw - ONE) * yf
    with np.errstate(all='ignore'):
        sp = np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, ZERO)
        q = ONE / (ONE + np.exp(-z))
    bce = sum32((ONE - yf) * z + lw * sp, mode) / F(B)
    sp_rows, sn_rows = np.flatnonzero(y == 1), np.flatnonzero(y == 0)
    N = 0
    kp = kn = np.zeros(0, dtype=F)
    if bank is not None:
        N = bank.N
        slots = np.arange(N) if bug == 'beyond_fill' else np.sort((bank.head - 1 - np.arange(bank.fill)) % N)
        kp, kn = bank.scores[slots[bank.labels[slots] == 1]], bank.scores[slots[bank.labels[slots] == 0]]
    negs, poss = np.concatenate([z[sn_rows], kn]), np.concatenate([z[sp_rows], kp])
    n = sp_rows.size * negs.size + kp.size * sn_rows.size
    denom = B * (B + N) if bug == 'norm_all' else n
    inv = ONE / F(denom) if n > 0 else ZERO
    g = np.zeros(B, dtype=F)
    rows = []
    if n > 0:
        for b in sp_rows:
            l, dl = pair32(z[b] - negs, kind, margin)
            rows.append(sum32(l, mode) if l.size else ZERO)
            g[b] = (sum32(dl, mode) if dl.size else ZERO) * inv
        for b in sn_rows:
            l, dl = pair32(poss - z[b], kind, margin)
            lk = l[sp_rows.size:]                                   # the bank's positives: the batch's were counted above
            rows.append(sum32(lk, mode) if lk.size else ZERO)
            s = (sum32(dl, mode) if dl.size else ZERO) * inv
            g[b] = s if bug == 'neg_sign' else -s
        if bug == 'bank_bank':
            for s in kp:
                rows.append(sum32(pair32(s - kn, kind, margin)[0], mode) if kn.size else ZERO)
            inv = ONE / F(n + kp.size * kn.size)
    auc = (sum32(np.array(rows, dtype=F), mode) if rows else ZERO) * inv
    total = bce + aw * auc
    dlog = ((ONE - yf) - lw * (ONE - q)) * (gs / F(B)) + (gs * aw) * g
    assert dlog.dtype == q.dtype == F and all(np.asarray(v).dtype == F for v in (total, bce, auc))
    return dict(total=total, bce=bce, auc=auc, probs=q, dlogits=dlog, n=n)


_REFS = {}


def _ref(name, case):
    if name not in _REFS:
        _REFS[name] = A.ref_of(case)
    return _REFS[name]


def ratios(bug=None):
    """key -> (worst ratio, the case it is reached on)"""
    out = {}
    for name, case in A.cases():
        ref = _ref(name, case)
        for mode in MODES:
            got = bce_auc32(case, mode, bug)
            assert bug is not None or got['n'] == ref['n']
            for k in KEYS:
                r = A.worst_ratio(got[k], ref[k], ref['E_' + k])
                if r >= out.get(k, (-1.0, ''))[0]:
                    out[k] = (r, name)
    return out


def test_the_case_list_holds_what_it_promises():
    base = A.base_cases()
    n = {name: A.ref_bce_auc(z, y, 1.8, 0.7, 0, m, gs, bank)['n'] for name, (z, y, bank, m, gs) in base.items()}
    assert n['B1_no_bank'] == 0 and n['all_positive_empty_bank'] == 0 and n['B2_one_of_each'] == 1
    assert n['all_positive_bank_of_negatives'] == 4 * 5                              # S+ x K- alone
    z, y, bank, _, _ = base['all_positive_bank_of_negatives']
    assert (y == 1).all() and (bank.labels[bank.valid()] == 0).all()
    for fill in (0, 3, 8):
        z, y, bank, _, _ = base['B5_N8_fill%d' % fill]
        assert z.size == 5 and bank.N == 8 and bank.fill == fill and int(bank.valid().sum()) == fill
    z, y, bank, _, gs = base['push_wraps']
    assert bank.head + z.size > bank.N and gs != 1.0
    after = bank.pushed(z, y)
    assert (after.head, after.fill) == (3, 8) and np.array_equal(after.scores[[6, 7, 0, 1, 2]], z)
    z, y, bank, _, _ = base['B_equals_N']
    assert z.size == bank.N
    z, y, bank, _, gs = base['B257_N1000']
    assert z.size == 257 and bank.N == 1000 and bank.N % 64 and gs != 1.0
    z, y, bank, _, _ = base['logits_pm80']
    assert set(np.abs(z).tolist()) == {80.0, 0.0}
    z, y, bank, _, _ = base['ties']
    assert np.unique(np.concatenate([z, bank.scores[bank.valid()]])).size == 1
    z, y, bank, m, _ = base['d_equals_margin']
    d = z[y == 1][:, None].astype(np.float64) - np.concatenate([z[y == 0], bank.scores[bank.valid() & (bank.labels == 0)]])[None, :]
    assert (d == m).sum() >= 2 and (d < m).any() and (d > m).any()
    l, dl = A.surrogate(np.array([m]), 1, m)
    assert l[0] == 0.0 and dl[0] == 0.0
    z, y, bank, _, _ = base['label_2']
    assert (y == 2).sum() == 2 and (bank.labels[bank.valid()] == 2).sum() == 1
    assert len(A.cases()) == 2 * len(base) and {c['kind'] for _, c in A.cases()} == {0, 1}
    # the garbage outside `fill` is there, and NaN in two cases
    assert sum(bool(np.isnan(b.scores).any()) for _, _, b, _, _ in base.values() if b is not None) == 2


def test_the_push_is_a_ring():
    b = A.Bank(np.zeros(8), np.zeros(8), 0, 0)
    seen = []
    for k in range(4):
        z = np.arange(3, dtype=F) + F(10 * k)
        b = b.pushed(z, np.array([1, 0, 2]))
        seen += z.tolist()
        sc, lb = b.oldest_first()
        assert sc.tolist() == seen[-8:] and b.fill == min(3 * (k + 1), 8) and b.head == (3 * (k + 1)) % 8
    assert lb.tolist() == [2, 1, 0, 2, 1, 0, 2, 1, 0, 2][-8:]


def test_fp32_restatement_stays_within_half_of_every_bound():
    shares = ratios()
    print('worst |fp32 - float64| / bound: ' + ', '.join('%s %.3f (%s)' % ((k,) + v) for k, v in shares.items()))
    for k, (v, name) in shares.items():
        assert v <= 0.5, (k, v, name)


@pytest.mark.parametrize('name', [n for n, _ in A.cases()])
def test_the_gradient_is_the_central_difference_of_the_loss(name):
    case = dict(A.cases())[name]
    z = case['z'].astype(np.float64)
    ref = _ref(name, case)
    h = 1e-6
    args = (case['y'], case['pos_weight'], case['auc_weight'], case['kind'], case['margin'], case['grad_scale'], case['bank'])
    rows = range(z.size) if z.size <= 16 else (0, 1, z.size - 1)            # (a positive row, a negative one, the last)
    for b in rows:
        zp, zm = z.copy(), z.copy()
        zp[b] += h
        zm[b] -= h
        fd = (A.ref_bce_auc(zp, *args)['total'] - A.ref_bce_auc(zm, *args)['total']) / (2 * h) * A.f32(case['grad_scale'])
        # the loss is smooth but for the hinge's second derivative, which jumps at the margin: there the difference is off by O(h)
        assert abs(fd - ref['dlogits'][b]) <= 1e-8 + 4.0 * h * A.f32(case['grad_scale']), (name, b, fd, ref['dlogits'][b])


NEED = {'norm_all': ('auc', 'dlogits'), 'bank_bank': ('auc',), 'beyond_fill': ('auc',), 'neg_sign': ('dlogits',)}


@pytest.mark.parametrize('bug', BUGS)
def test_a_wrong_formula_leaves_the_bound(bug):
    r = ratios(bug)
    print('%s: times over the bound: ' % bug + ', '.join('%s %.3g (%s)' % ((k,) + r[k]) for k in NEED[bug]))
    for k in NEED[bug]:
        assert r[k][0] > 1.0, (bug, k, r[k])
