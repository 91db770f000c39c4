"""CPU: the error bounds of tests/attn_ref.py are honest -- two independently written numpy-fp32 evaluations of the attention forward and
backward passes stay at or below HALF of them on every case list -- and sharp: eleven wrong formulas each exceed them on a named case.

The two evaluations:
  two-pass   scores by a serial 64-term dot product, row maximum, exp, a serial sum over the keys, p = e / l, serial P.V; backward
             with serial sums throughout
  blocked    the kernels' scheme: online softmax over 32-key chunks (running maximum, alpha = exp(m_run - m_new) rescaling of l and O),
             every product as six of the nine bf16-piece products (gemm_ref.split3_host) accumulated in fp32, unnormalised probabilities
             into P.V and one division at the end; backward with p = exp(s - lse_in) chunk by chunk
Both read the dropout multipliers, the bias and the case lists from attn_ref (there is one specification of those), nothing else."""
import numpy as np
import pytest
import torch

import attn_ref as R
from gemm_ref import split3_host

F = np.float32
SCALE = F(0.125)

# worst share of its bound that each evaluation reaches over all case lists (printed by test_bounds_are_honest; asserted <= 0.5)
RECORDED = {}


# ---------------------------------------------------------------------------------------------------------------------------
# evaluation 1: two passes, serial sums
# ---------------------------------------------------------------------------------------------------------------------------
def _serial_dot(a, b):
    """[h, n, 64] x [h, m, 64] -> [h, n, m], the 64 terms added one after the other in fp32"""
    acc = np.zeros((a.shape[0], a.shape[1], b.shape[1]), dtype=F)
    for d in range(a.shape[2]):
        acc = acc + a[:, :, None, d] * b[:, None, :, d]
    return acc


def _serial_pv(w, x):
    """[h, n, m] x [h, m, 64] -> [h, n, 64], the m terms added one after the other"""
    acc = np.zeros((w.shape[0], w.shape[1], x.shape[2]), dtype=F)
    for j in range(w.shape[2]):
        acc = acc + w[:, :, j, None] * x[:, None, j, :]
    return acc


def _serial_last(x):
    acc = np.zeros(x.shape[:-1], dtype=F)
    for j in range(x.shape[-1]):
        acc = acc + x[..., j]
    return acc


def twopass_fwd(q, k, v, bias, m, mut=None):
    m = m.astype(F)
    if mut == 'mask-inf':
        bias = np.where(bias < 0, F(-np.inf), bias).astype(F)
    s = _serial_dot(q, k) * SCALE + bias[None, None, :]
    mx = np.zeros(s.shape[:-1], dtype=F) if mut == 'no-max' else s.max(-1)
    e = np.exp(s - mx[..., None])
    l = _serial_last(e)
    lse = mx + np.log(l)
    p = e / l[..., None]
    return dict(ctx=_serial_pv(p * m, v), lse=lse.astype(F))


def twopass_bwd(q, k, v, bias, m, dO, ctx_in, lse_in, mut=None):
    m = m.astype(F)
    s = _serial_dot(q, k) * SCALE + bias[None, None, :]
    p = np.exp(s - lse_in[..., None])
    dP = _serial_dot(dO, v)
    delta = _serial_last(ctx_in * dO)
    g = dP * m - (_serial_last(p * dP) if mut == 'delta-undropped' else delta)[..., None]
    dS = p * g
    dq = _serial_pv(dS, k) * SCALE
    dk = _serial_pv(dS.transpose(0, 2, 1), q) * SCALE
    if mut == 'dq-scaled-twice':
        dq = dq * SCALE
    if mut == 'dk-unscaled':
        dk = dk / SCALE
    return dict(dq=dq, dk=dk, dv=_serial_pv((p * m).transpose(0, 2, 1), dO), delta=delta)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluation 2: online softmax over 32-key chunks, bf16-piece products
# ---------------------------------------------------------------------------------------------------------------------------
SIX = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))


def _pieces(x, npieces):
    p3 = split3_host(torch.from_numpy(np.ascontiguousarray(x, dtype=F)).reshape(-1, x.shape[-1])).float().numpy()
    return [p3[:, t].reshape(x.shape) for t in range(npieces)]


def prod6(a, b, npieces=3):
    """a [h, n, K] @ b [h, K, m] as the bf16-piece products a1 b1, a1 b2, a2 b1, a1 b3, a2 b2, a3 b1 (those with both pieces present),
    accumulated in fp32 in that order"""
    ap, bp = _pieces(a, npieces), _pieces(b, npieces)
    acc = np.zeros((a.shape[0], a.shape[1], b.shape[2]), dtype=F)
    for x, y in SIX:
        if x < npieces and y < npieces:
            acc = acc + np.matmul(ap[x], bp[y])
    return acc


def blocked_fwd(q, k, v, bias, m, mut=None):
    np_ = 2 if mut == 'two-pieces' else 3
    m = m.astype(F)
    h, n = q.shape[0], q.shape[1]
    m_run = np.full((h, n), -np.inf, dtype=F)
    l = np.zeros((h, n), dtype=F)
    o = np.zeros((h, n, R.HD), dtype=F)
    with np.errstate(invalid='ignore'):
        for c, k0 in enumerate(range(0, n, 32)):
            ks = slice(k0, min(k0 + 32, n))
            s = prod6(q, k[:, ks].transpose(0, 2, 1), np_) * SCALE + bias[None, None, ks]
            m_new = np.maximum(m_run, s.max(-1))
            alpha = np.exp(m_run - m_new)
            e = np.exp(s - m_new[..., None])
            l = l * alpha + e.sum(-1, dtype=F)
            if mut == 'alpha-skipped' and c == 1:
                alpha = np.ones_like(alpha)
            o = o * alpha[..., None] + prod6(e * m[:, :, ks], v[:, ks], np_)
            m_run = m_new
    return dict(ctx=o * (F(1.0) / l)[..., None], lse=(m_run + np.log(l)).astype(F))


def blocked_bwd(q, k, v, bias, m, dO, ctx_in, lse_in, mut=None):
    np_ = 2 if mut == 'two-pieces' else 3
    m = m.astype(F)
    h, n = q.shape[0], q.shape[1]
    delta = (ctx_in * dO).sum(-1, dtype=F)
    dq = np.zeros((h, n, R.HD), dtype=F)
    dk, dv = np.zeros_like(dq), np.zeros_like(dq)
    for k0 in range(0, n, 32):
        ks = slice(k0, min(k0 + 32, n))
        s = prod6(q, k[:, ks].transpose(0, 2, 1), np_) * SCALE + bias[None, None, ks]
        p = np.exp(s - lse_in[..., None])
        dP = prod6(dO, v[:, ks].transpose(0, 2, 1), np_)
        mk = m[:, :, ks]
        dS = p * (dP * mk - delta[..., None]) * SCALE
        dq = dq + prod6(dS, k[:, ks], np_)
        dk[:, ks] = prod6(dS.transpose(0, 2, 1), q, np_)
        dv[:, ks] = prod6((p * mk).transpose(0, 2, 1), dO, np_)
    return dict(dq=dq, dk=dk, dv=dv, delta=delta)


EVALS = {'two-pass': (twopass_fwd, twopass_bwd), 'blocked': (blocked_fwd, blocked_bwd)}


def evaluate(call, which, mut=None, keep_args=None, bias_rows='all', short_by_one=False):
    """the library's outputs of `call` as evaluation `which` computes them: forward, then backward on fp32(reference ctx, lse)"""
    ref = R.reference(call)
    fwd, bwd = EVALS[which]
    fw, bw = [], []
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for b, r0, n, q, k, v, dO, bias, m in R.samples(call, **(keep_args or {})):
            if short_by_one and n > 1:
                bias = bias.copy()
                bias[n - 1] = F(-10000.0)          # the last key of the sample is not seen
            ctx_in = R.heads(ref['ctx_in'][r0:r0 + n], call.nh)
            lse_in = ref['lse_in'][b, :, :n]
            fw.append(fwd(q, k, v, bias, m, mut))
            bw.append(bwd(q, k, v, bias, m, dO, ctx_in, lse_in, mut))
    return dict(R.assemble(call, fw), **R.assemble(call, bw, bias_rows=bias_rows))


ALL = R.OUTPUTS_FWD + R.OUTPUTS_BWD


def worst(call, got, names=ALL):
    return R.shares(call, R.reference(call), got, names=names)


def all_calls():
    return (R.masks_calls() + R.scores_calls() + R.lengths_calls() + R.long_calls(thin=True) + R.packed_calls() + R.dropout_calls())


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', list(EVALS))
def test_bounds_are_honest(which):
    """every share of every output on every case list is <= 0.5: each constant is at least twice what an fp32 evaluation needs"""
    top = {name: (0.0, None) for name in ALL}
    for call in all_calls():
        for name, share in worst(call, evaluate(call, which)).items():
            if share > top[name][0]:
                top[name] = (share, call.name)
    RECORDED[which] = top
    print('\n%s: worst shares %s' % (which, ', '.join('%s %.3f (%s)' % (n, s, c) for n, (s, c) in top.items())))
    for name, (share, where) in top.items():
        assert share <= 0.5, (which, name, share, where)


def test_a_zero_bound_means_exact():
    """q = 0 without padding: s = 0 exactly and E_s = 0; lse = log L keeps only the rounding terms"""
    call = R.dropout_call(33, 0.5)
    for b, r0, n, q, k, v, dO, bias, m in R.samples(call):
        s, E_s = R._scores(q.astype(np.float64), k.astype(np.float64), bias.astype(np.float64))
        assert not s.any() and not E_s.any()


def _sample_shares(call, got, b, names):
    """shares restricted to sample b of a call (MASKS and SCORES hold one pattern per sample)"""
    from gemm_ref import worst_ratio
    ref = R.reference(call)
    out = {}
    for name in names:
        if name in ('dq', 'dk', 'dv'):
            t = ('dq', 'dk', 'dv').index(name)
            cols = slice(t * call.H, (t + 1) * call.H)
            rows = slice(int(call.cu[b]), int(call.cu[b + 1]))
            out[name] = worst_ratio(got['dqkv'][rows, cols], ref['dqkv'][rows, cols], ref['E_dqkv'][rows, cols])
        elif name == 'ctx':
            rows = slice(int(call.cu[b]), int(call.cu[b + 1]))
            out[name] = worst_ratio(got['ctx'][rows], ref['ctx'][rows], ref['E_ctx'][rows])
        elif name == 'bias_part':
            out[name] = worst_ratio(got[name][b], ref[name][b], ref['E_bias_part'][b])
        else:
            n = call.lens[b]
            out[name] = worst_ratio(got[name][b, :, :n], ref[name][b, :, :n], ref['E_' + name][b, :, :n])
    return out


# mutation -> (evaluation, call, sample of the call or None, outputs that must exceed their bound, arguments of evaluate)
MUTATIONS = {
    'mask as -inf instead of -10000': ('two-pass', lambda: R.masks_call(0.0), R.MASK_NAMES.index('zeros'), ('ctx', 'lse'), dict(mut='mask-inf')),
    'no 1 / (1 - p)': ('two-pass', lambda: R.dropout_call(33, 0.5), None, ('ctx', 'dv'), dict(keep_args=dict(scaled=False))),
    'keep mask indexed with L instead of Lp': ('two-pass', lambda: R.dropout_call(33, 0.5), None, ('ctx', 'dv'), dict(keep_args=dict(lp=33))),
    'keep mask transposed': ('two-pass', lambda: R.dropout_call(164, 0.5), None, ('ctx', 'dv'), dict(keep_args=dict(transposed=True))),
    'delta from the undropped probabilities': ('two-pass', lambda: R.scores_call(0.1), R.SCORE_NAMES.index('randn'), ('dq', 'dk'),
                                               dict(mut='delta-undropped')),
    'score scale applied twice on dQ': ('two-pass', lambda: R.length_call(17, 0.1), None, ('dq',), dict(mut='dq-scaled-twice')),
    'score scale missing on dK': ('two-pass', lambda: R.length_call(17, 0.1), None, ('dk',), dict(mut='dk-unscaled')),
    'no maximum subtraction': ('two-pass', lambda: R.scores_call(0.0), R.SCORE_NAMES.index('x10'), ('ctx', 'lse'), dict(mut='no-max')),
    "one chunk's alpha rescale skipped": ('blocked', lambda: R.masks_call(0.0), R.MASK_NAMES.index('chunk0-masked'), ('ctx',),
                                          dict(mut='alpha-skipped')),
    'sample length off by one in the packed form': ('two-pass', lambda: R.packed_call(0.0), None, ('ctx', 'lse', 'dv'), dict(short_by_one=True)),
    'bias_part over valid rows only in the mask form': ('two-pass', lambda: R.masks_call(0.0), R.MASK_NAMES.index('right-pad-40'), ('bias_part',),
                                                        dict(bias_rows='valid')),
    'operands cut to two bf16 pieces': ('blocked', lambda: R.scores_call(0.0), R.SCORE_NAMES.index('x4'), ('lse', 'dq', 'dk', 'dv'),
                                        dict(mut='two-pieces')),
}


@pytest.mark.parametrize('name', list(MUTATIONS))
def test_wrong_formulas_exceed_the_bounds(name):
    which, make, b, outputs, args = MUTATIONS[name]
    call = make()
    got = evaluate(call, which, **args)
    sh = worst(call, got, outputs) if b is None else _sample_shares(call, got, b, outputs)
    print('\n%s on %s%s: %s' % (name, call.name, '' if b is None else ' sample %d' % b, ', '.join('%s %.3g' % kv for kv in sh.items())))
    for out in outputs:
        assert sh[out] > 1.0, (name, out, sh[out])
    clean = evaluate(call, which)
    sh0 = worst(call, clean, outputs) if b is None else _sample_shares(call, clean, b, outputs)
    assert all(v <= 0.5 for v in sh0.values()), (name, sh0)
