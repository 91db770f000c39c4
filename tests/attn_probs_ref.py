"""Float64 reference of csrc/attn_probs.hip -- the attention probabilities as an output (uniter_attn_probs) and attention rollout on their
head means (uniter_attn_rollout) -- with per-element error bounds for an fp32 evaluation, and the case lists
tests/test_attn_probs_bounds_cpu.py (CPU) and tests/test_attn_probs_gpu.py (GPU) share.  Plain numpy on the CPU.

The probabilities and their bound are those of tests/attn_ref.py, one (sample, head) at a time, from the INPUT VALUES the kernel gets
widened to float64 (inputs given as bf16: the bf16 values widened): s and E_s from attn_ref._scores, then the E_lse and E_p formulas
of attn_ref.forward_sample with its constants unchanged.  On top of them, U = 2^-24, T = 2^-126:

    probs [B, nh, L, L]     E_p
    head mean [B, L, L]     mean_h E_p + (nh + 2) U mean_h p + T      nh - 1 additions and one division, each relative to a partial sum
                                                                    that is at most the whole (the terms are nonnegative); T: the
                                                                    quotient may leave the normal range
    rollout, after the product of layer l
                            R expm1((l + 1) (L + 4) U) + (l + 1) L T  A~ = residual I + (1 - residual) A costs two roundings, a product
                                                                    and L - 1 additions of nonnegative terms L more, so one layer's
                                                                    product is off by at most (L + 4) U RELATIVE to the value, and the
                                                                    factors (1 + e) compound over the layers; T per term of each sum

In the packed form rows and columns at or beyond a sample's length are 0 with bound 0: they must come out exactly 0.

Worst shares of these bounds that two numpy-fp32 evaluations reach (tests/test_attn_probs_bounds_cpu.py; the rule there, as in
tests/test_attn_bounds_cpu.py, is <= 0.5), two-pass | blocked: probs 0.309 | 0.276 (SCORES), head mean the same (one head), rollout
0.116 | 0.130 (L = 17, 12 layers, residual 0.5)."""
import functools

import numpy as np

import attn_ref as R

F, D, U, TINY = R.F, R.D, R.U, R.TINY


def rne_bf16(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F)).bfloat16().float().numpy()


@functools.lru_cache(maxsize=None)
def as_bf16(call):
    """the call whose qkv holds the bf16-rounded values (what a bf16 qkv buffer widened gives)"""
    kw = dict(lens=call.lens) if call.packed else dict(mask=call.mask)
    return R.Call(call.name + '-b16', call.nh, 0.0, rne_bf16(call.qkv), call.dO, **kw)


def probs_sample(q, k, bias):
    """p and E_p [nh, n, n] of one sample in float64"""
    q, k, bias = (np.asarray(t, dtype=D) for t in (q, k, bias))
    s, E_s = R._scores(q, k, bias)
    mx = s.max(-1)
    lse = mx + np.log(np.exp(s - mx[..., None]).sum(-1))
    p = np.exp(s - lse[..., None])
    E_lse = (p * E_s).sum(-1) + U * (R.A_L * np.maximum(1.0, np.maximum(np.abs(lse), np.abs(mx))) + R.B_L)
    E_p = p * np.expm1(E_s + E_lse[..., None] + R.A_P * U * (1.0 + np.abs(s - lse[..., None]))) + TINY
    return p, E_p


_CACHE = {}


def reference(call):
    """dict(p, E_p [B, nh, L, L]; mean, E_mean [B, L, L]) in float64, computed once per call and not to be modified; a packed sample's
    rows and columns beyond its length hold 0 with bound 0"""
    if call.name in _CACHE:
        return _CACHE[call.name]
    B, nh, L = call.B, call.nh, call.L
    p, E = np.zeros((B, nh, L, L), dtype=D), np.zeros((B, nh, L, L), dtype=D)
    for b, r0, n, q, k, v, dO, bias, m in R.samples(call):
        p[b, :, :n, :n], E[b, :, :n, :n] = probs_sample(q, k, bias)
    mean = p.mean(1)
    E_mean = E.mean(1) + (nh + 2) * U * mean + TINY * (E.max(1) > 0)
    out = dict(p=p, E_p=E, mean=mean, E_mean=E_mean)
    _CACHE[call.name] = out
    return out


def share(got, ref, bound):
    from gemm_ref import worst_ratio
    return worst_ratio(got, ref, bound)


def probs_calls():
    """the calls the probabilities are checked on, all without dropout (the kernel has none)"""
    return ([R.masks_call(0.0), R.scores_call(0.0)] + [R.length_call(L, 0.0) for L in R.LENGTHS]
            + [R.length_call(L, 0.0, nh=3) for L in (193, 256, 321)] + [R.packed_call(0.0)])


# ---------------------------------------------------------------------------------------------------------------------------
# rollout
# ---------------------------------------------------------------------------------------------------------------------------
ROLLOUT_L = (1, 17, 64, 164, 193)
ROLLOUT_NL = (1, 2, 12)
ROLLOUT_RES = (0.5, 0.0)


@functools.lru_cache(maxsize=None)
def rollout_maps(L, nl=max(ROLLOUT_NL)):
    """[nl, 2, L, L] fp32: the fp32-rounded head-mean reference maps of nl seeded calls (B = 2, nh = 2, sample 1 right-padded by 7 % L
    as in attn_ref.length_call); a shorter stack is a prefix of it"""
    out = np.zeros((nl, 2, L, L), dtype=F)
    for l in range(nl):
        x, d = R._operands(700 + 13 * l + L, 2, L, 2)
        m = np.ones((2, L), dtype=F)
        if 7 % L:
            m[1, L - 7 % L:] = 0
        qkv, dO = R._flat(x, d)
        out[l] = reference(R.Call('rollout-L%d-l%d' % (L, l), 2, 0.0, qkv, dO, mask=m))['mean'].astype(F)
    out.setflags(write=False)
    return out


def rollout_reference(attn, residual, reverse=False):
    """[(R_l, bound_l)] for l = 0 .. nl - 1 in float64 from the fp32 maps attn [nl, B, L, L]; reverse: the handle of the CPU test's
    mutation (R_l = R_{l-1} A~_l)"""
    attn = np.asarray(attn, dtype=D)
    nl, B, L = attn.shape[:3]
    res = float(F(residual))
    eye = np.eye(L, dtype=D)[None]
    out, Rl = [], None
    for l in range(nl):
        At = res * eye + (1.0 - res) * attn[l]
        Rl = At if l == 0 else (np.matmul(Rl, At) if reverse else np.matmul(At, Rl))
        out.append((Rl, Rl * np.expm1((l + 1) * (L + 4) * U) + (l + 1) * L * TINY))
    return out
