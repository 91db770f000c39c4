"""CPU: the error bounds of tests/attn_grad_ref.py are honest -- two independently written numpy-fp32 evaluations of g = p dP, of the
head mean of max(g, 0), of the head sums and of the relevance recurrence stay at or below HALF of them on every case -- and sharp: seven
wrong formulas, and the recurrence multiplied from the wrong side, each exceed them tenfold.

The two evaluations:
  serial    the two-pass probabilities of tests/test_attn_probs_bounds_cpu.py (serial dot products and sums); the slabs added one after
            the other; dP by a serial 64-term dot product; the heads added one after the other, then divided; the head sum row by row,
            each row key by key; relevance with the L terms added one after the other
  blocked   that file's online softmax over 32-key chunks; the slabs added by numpy's pairwise sum; dP by a BLAS product; numpy's mean
            over the heads; numpy's pairwise sum over the map; relevance by BLAS products

Worst shares (serial | blocked): the table in tests/attn_grad_ref.py, printed by test_bounds_are_honest."""
import numpy as np
import pytest

import attn_ref as R
import attn_probs_ref as PR
import attn_grad_ref as GR
from test_attn_probs_bounds_cpu import twopass_probs, blocked_probs, _serial_dot, _serial_last

F = np.float32


def serial_eval(q, k, v, bias, slabs, lse_shift=0):
    p = twopass_probs(q, k, bias)
    if lse_shift:      # the mutation: each head normalised by the next head's lse, i.e. p_h scaled by exp(lse_h - lse_(h+1))
        p = head_shifted(q, k, bias, p)
    dO = slabs[0]
    for s in slabs[1:]:
        dO = dO + s
    dP = _serial_dot(dO, v)
    g = p * dP
    sums = _serial_last(_serial_last(g))
    return p, dP, g, sums


def blocked_eval(q, k, v, bias, slabs, lse_shift=0):
    p = blocked_probs(q, k, bias)
    if lse_shift:
        p = head_shifted(q, k, bias, p)
    dO = np.sum(np.stack(slabs), axis=0, dtype=F)
    dP = np.matmul(dO, v.transpose(0, 2, 1))
    g = p * dP
    return p, dP, g, g.sum((1, 2), dtype=F)


def head_shifted(q, k, bias, p):
    s = (np.einsum('hid,hjd->hij', q.astype(np.float64), k.astype(np.float64)) / 8.0 + bias[None, None, :])
    mx = s.max(-1)
    lse = mx + np.log(np.exp(s - mx[..., None]).sum(-1))
    return (p * np.exp(lse - np.roll(lse, -1, axis=0))[..., None]).astype(F)


def serial_mean(x, relu=True):
    acc = np.zeros(x.shape[1:], dtype=F)
    for h in range(x.shape[0]):
        acc = acc + (np.maximum(x[h], F(0)) if relu else x[h])
    return acc / F(x.shape[0])


def blocked_mean(x, relu=True):
    return (np.maximum(x, F(0)) if relu else x).mean(0, dtype=F)


def serial_relevance(maps, reverse=False):
    B, L = maps.shape[1], maps.shape[2]
    out, Rl = [], np.broadcast_to(np.eye(L, dtype=F), (B, L, L))
    for l in range(maps.shape[0]):
        x, y = (Rl, maps[l]) if reverse else (maps[l], Rl)
        acc = np.zeros((B, L, L), dtype=F)
        for kk in range(L):
            acc = acc + x[:, :, kk, None] * y[:, kk, None, :]
        Rl = Rl + acc
        out.append(Rl)
    return out


def blocked_relevance(maps, reverse=False):
    B, L = maps.shape[1], maps.shape[2]
    out, Rl = [], np.broadcast_to(np.eye(L, dtype=F), (B, L, L))
    for l in range(maps.shape[0]):
        Rl = Rl + (np.matmul(Rl, maps[l]) if reverse else np.matmul(maps[l], Rl))
        out.append(Rl)
    return out


EVALS = {'serial': (serial_eval, serial_mean, serial_relevance), 'blocked': (blocked_eval, blocked_mean, blocked_relevance)}


def evaluate(call, which, n_slabs=1, mut=None):
    """(g [B, nh, L, L], mean [B, L, L], sums [B, nh]) of `call` as evaluation `which` computes them"""
    ev, mean, _ = EVALS[which]
    g = np.zeros((call.B, call.nh, call.L, call.L), dtype=F)
    mn = np.zeros((call.B, call.L, call.L), dtype=F)
    sums = np.zeros((call.B, call.nh), dtype=F)
    slabs_all = GR.split_slabs(call.dO) if n_slabs == 2 else call.dO[None]
    if mut == 'slab-dropped':
        slabs_all = slabs_all[:1]
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for b, r0, n, q, k, v, dO, bias, m in R.samples(call):
            if mut == 'mask-dropped':
                bias = np.zeros_like(bias)
            slabs = [R.heads(s[r0:r0 + n], call.nh) for s in slabs_all]
            p, dP, x, sm = ev(q, k, v, bias, slabs, lse_shift=mut == 'lse-of-another-head')
            if mut == 'transposed':
                x = np.ascontiguousarray(x.transpose(0, 2, 1))
            if mut == 'dS':
                x = p * (dP - (p * dP).sum(-1, dtype=F)[..., None])
            g[b, :, :n, :n] = x
            if mut == 'relu-after-mean':
                mn[b, :n, :n] = np.maximum(mean(x, relu=False), F(0))
            else:
                mn[b, :n, :n] = mean(x, relu=mut != 'no-relu')
            sums[b] = sm
    return g, mn, sums


def shares(call, got, n_slabs=1):
    ref = GR.reference(call, n_slabs)
    return dict(g=GR.share(got[0], ref['g'], ref['E_g']), mean=GR.share(got[1], ref['mean'], ref['E_mean']),
                sums=GR.share(got[2], ref['sums'], ref['E_sums']))


def relevance_share(got, ref):
    return max(GR.share(g, r, e) for g, (r, e) in zip(got, ref))


@pytest.mark.parametrize('which', list(EVALS))
def test_bounds_are_honest(which):
    """every share of every output on every case is <= 0.5: each constant is at least twice what an fp32 evaluation needs; with one
    slab and with two, and on the bf16-rounded inputs of two calls"""
    top = dict(g=(0.0, None), mean=(0.0, None), sums=(0.0, None), relevance=(0.0, None))
    calls = [(c, 1 + i % 2) for i, c in enumerate(GR.grad_calls())]
    calls += [(R.scores_call(0.0), 2), (R.length_call(17, 0.0), 1), (PR.as_bf16(R.scores_call(0.0)), 1), (PR.as_bf16(R.length_call(65, 0.0)), 2)]
    for call, ns in calls:
        for name, sh in shares(call, evaluate(call, which, ns), ns).items():
            if sh > top[name][0]:
                top[name] = (sh, '%s, %d slab(s)' % (call.name, ns))
    for L in GR.REL_L:
        maps = GR.relevance_maps(L)
        sh = relevance_share(EVALS[which][2](maps), GR.relevance_reference(maps))
        if sh > top['relevance'][0]:
            top['relevance'] = (sh, 'L %d nl %d' % (L, maps.shape[0]))
    print('\n%s: worst shares %s' % (which, ', '.join('%s %.3f (%s)' % (n, s, c) for n, (s, c) in top.items())))
    for name, (sh, where) in top.items():
        assert sh <= 0.5, (which, name, sh, where)


def test_packed_padding_and_masked_keys_have_a_zero_reference():
    ref = GR.reference(R.packed_call(0.0))
    n = R.PACKED_LENS[1]
    for key in ('g', 'E_g'):
        assert not ref[key][1, :, n:, :].any() and not ref[key][1, :, :, n:].any()
    assert not ref['E_mean'][1, n:, :].any() and not ref['E_mean'][1, :, n:].any()
    assert (ref['E_g'][1, :, :n, :n] > 0).all()
    call = R.masks_call(0.0)
    ref = GR.reference(call)
    for b in range(call.B - 1):      # (the all-masked pattern is the last one: there every key is an ordinary key)
        assert not ref['g'][b][:, :, call.mask[b] == 0].any()


# mutation -> (call, slabs, output that must exceed its bound tenfold)
MUTATIONS = {
    'transposed': (lambda: R.length_call(17, 0.0), 1, 'g'),
    'dS': (lambda: R.length_call(17, 0.0), 1, 'g'),
    'relu-after-mean': (lambda: R.length_call(17, 0.0), 1, 'mean'),
    'no-relu': (lambda: R.length_call(17, 0.0), 1, 'mean'),
    'slab-dropped': (lambda: R.length_call(17, 0.0), 2, 'g'),
    'mask-dropped': (lambda: R.masks_call(0.0), 1, 'g'),
    'lse-of-another-head': (lambda: R.length_call(17, 0.0), 1, 'g'),
}


@pytest.mark.parametrize('which', list(EVALS))
@pytest.mark.parametrize('name', list(MUTATIONS))
def test_wrong_formulas_exceed_the_bounds(name, which):
    make, ns, out = MUTATIONS[name]
    call = make()
    sh = shares(call, evaluate(call, which, ns, mut=name), ns)[out]
    print('\n%s (%s) on %s: %s share %.3g' % (name, which, call.name, out, sh))
    assert sh >= 10.0, (name, which, sh)
    assert shares(call, evaluate(call, which, ns), ns)[out] <= 0.5


@pytest.mark.parametrize('which', list(EVALS))
def test_relevance_from_the_wrong_side_exceeds_the_bound(which):
    maps = GR.relevance_maps(17)[:2]
    ref = GR.relevance_reference(maps)
    sh = relevance_share(EVALS[which][2](maps, reverse=True), ref)
    print('\nrelevance reversed (%s): share %.3g' % (which, sh))
    assert sh >= 10.0
    assert relevance_share(EVALS[which][2](maps), ref) <= 0.5
    rev = GR.relevance_reference(maps, reverse=True)
    assert GR.share(rev[1][0], ref[1][0], ref[1][1]) >= 10.0


def test_relevance_exact_cases_in_the_reference():
    L = 17
    zero = np.zeros((3, 2, L, L), dtype=F)
    assert np.array_equal(GR.relevance_reference(zero)[-1][0], np.eye(L)[None].repeat(2, 0))
    maps = GR.upper_triangular_maps(L, 3)
    want = GR.relevance_reference(maps)[-1][0]
    assert np.array_equal(want, np.round(want)) and want.max() < 2 ** 24 and want.max() > 1
    for which in EVALS:
        assert np.array_equal(EVALS[which][2](maps)[-1].astype(np.float64), want)


def test_slabs_sum_exactly():
    call = R.scores_call(0.0)
    s = GR.split_slabs(call.dO)
    assert np.array_equal(s[0].astype(np.float64) + s[1].astype(np.float64), call.dO.astype(np.float64))
    assert np.abs(s[1]).max() > 0
