"""Float64 reference of csrc/attn_grad.hip -- gradient-weighted attention g = p dP per head, its head mean after a ReLU, the per-head sums
(uniter_attn_grad) and the relevance recurrence on the head means (uniter_attn_relevance) -- with per-element error bounds for an
fp32 evaluation, and the case lists tests/test_attn_grad_bounds_cpu.py (CPU) and tests/test_attn_grad_gpu.py (GPU) share.  Plain numpy
on the CPU.

The reference takes the INPUT VALUES the kernel gets widened to float64, one (sample, head) at a time, on the calls of tests/attn_ref.py
(`Call.dO` is the gradient of the context, dctx; given as slabs, their float64 sum):

    p_ij, E_p         attn_probs_ref.probs_sample: s_ij = q_i . k_j / 8 + bias_j, lse recomputed, p = exp(s - lse)
    dP_ij = dO_i . v_j
    g_ij  = p_ij dP_ij

Bounds.  U = 2^-24, T = 2^-126, d_ij = sum_d |dO_id v_jd|, ns the number of slabs:

    E_dP   = (A_S + ns - 1) U d_ij                 the dot product relative to its absolute terms, as E_s in attn_ref (A_S = 16); each
                                                   of the ns - 1 additions that form dO_id is one rounding relative to a partial sum
                                                   that |dO_id| bounds only when the slabs share a sign -- the tests' slabs do (below)
    E_g    = E_p |dP| + p E_dP + U |g| + T         the product's own rounding; T: a product below the normal range
    head mean  A = (1 / nh) sum_h max(g, 0)
    E_A    = mean_h E_g + (nh + 2) U A + T         max(., 0) is 1-Lipschitz; nh - 1 additions of nonnegative terms and one division,
                                                   as E_mean in attn_probs_ref
    head_sums  S = sum_ij g_ij
    E_S    = sum_ij E_g + A_H U sum_ij |g_ij|      a signed sum: every addition rounds relative to a partial sum that sum |g| bounds.
                                                   A_H = 8 (A_B of attn_ref, the same kind of sum): a workgroup's lanes add their keys'
                                                   terms chunk after chunk, a shuffle tree joins the lanes, then waves and tiles
    relevance, after layer l (R_0 = I + A_0, R_l = R_{l-1} + A_l R_{l-1}; maps nonnegative)
    E_R    = R expm1((l + 1) (L + 4) U) + (l + 1) L T
                                                   L fused multiply-adds of nonnegative terms and the addition of R_{l-1}: one layer is
                                                   off by at most (L + 1) U relative to the value, the factors compound; as the rollout
                                                   bound of attn_probs_ref
    In the packed form rows and columns at or beyond a sample's length are 0 with bound 0; so is every masked key's column wherever
    p underflows to 0 in float64 too (bias -10000 against finite scores: always) -- there the bound is T alone, and the GPU test
    asserts the exact 0 separately.

Slabs.  The tests split dO into two slabs that sum to it EXACTLY in fp32: slab 0 = dO rounded to bf16, slab 1 = dO - slab 0 (exact:
the difference of an fp32 number and its 8-bit-mantissa rounding has at most 16 significant bits).  slab 1 is 2^-9 of dO, so dropping it
moves dP by ~2^-9 d / sqrt(64), three orders of magnitude above E_dP.

Constants.  None is fitted to the kernel.  tests/test_attn_grad_bounds_cpu.py evaluates the formulas in numpy fp32 twice, independently
written (serial sums | BLAS products with pairwise sums), over every case below; each constant is at least twice the worst share
either reaches.  Worst shares (serial | blocked), each on the case named:

    g          0.307 | 0.274   SCORES, two slabs (the probabilities' share: E_p |dP| dominates)
    head mean  0.307 | 0.274   SCORES, two slabs (one head: the mean is the head)
    head_sums  0.011 | 0.006   L = 1 | PACKED (sum E_g dominates: the elements' errors do not line up)
    relevance  0.175 | 0.175   L = 1, 12 layers (R = prod (1 + a_l): twelve products and additions of one number)"""
import functools

import numpy as np

import attn_ref as R
import attn_probs_ref as PR

F, D, U, TINY = R.F, R.D, R.U, R.TINY
A_H = 8.0


def split_slabs(dO):
    """[2, rows, H] fp32 that sum to dO exactly in fp32"""
    s0 = PR.rne_bf16(dO)
    s1 = (np.asarray(dO, dtype=F) - s0).astype(F)
    assert np.array_equal((s0 + s1).astype(F), np.asarray(dO, dtype=F))
    return np.stack([s0, s1])


_PARTS = {}


def _parts(call):
    """p, E_p, dP, d [B, nh, L, L] float64 of a call (dO as one array), computed once"""
    if call.name in _PARTS:
        return _PARTS[call.name]
    B, nh, L = call.B, call.nh, call.L
    p, E_p, dP, d = (np.zeros((B, nh, L, L), dtype=D) for _ in range(4))
    for b, r0, n, q, k, v, dO, bias, m in R.samples(call):
        p[b, :, :n, :n], E_p[b, :, :n, :n] = PR.probs_sample(q, k, bias)
        dO64, v64 = dO.astype(D), v.astype(D)
        dP[b, :, :n, :n] = dO64 @ v64.transpose(0, 2, 1)
        d[b, :, :n, :n] = np.abs(dO64) @ np.abs(v64).transpose(0, 2, 1)
    out = (p, E_p, dP, d)
    _PARTS[call.name] = out
    return out


_CACHE = {}


def reference(call, n_slabs=1):
    """dict(g, E_g [B, nh, L, L]; mean, E_mean [B, L, L]; sums, E_sums [B, nh]) in float64 for dO given as n_slabs slabs that sum to
    call.dO exactly; computed once and not to be modified"""
    key = (call.name, n_slabs)
    if key in _CACHE:
        return _CACHE[key]
    p, E_p, dP, d = _parts(call)
    nh = call.nh
    valid = E_p > 0
    g = p * dP
    E_dP = (R.A_S + n_slabs - 1) * U * d
    E_g = (E_p * np.abs(dP) + p * E_dP + U * np.abs(g) + TINY) * valid
    mean = np.maximum(g, 0.0).mean(1)
    E_mean = E_g.mean(1) + (nh + 2) * U * mean + TINY * valid.any(1)
    sums = g.sum((2, 3))
    E_sums = E_g.sum((2, 3)) + A_H * U * np.abs(g).sum((2, 3))
    out = dict(g=g, E_g=E_g, mean=mean, E_mean=E_mean, sums=sums, E_sums=E_sums)
    _CACHE[key] = out
    return out


share = PR.share

GRAD_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 164, 192)
GRAD_LONG = (193, 257)


def grad_calls():
    """the calls uniter_attn_grad is checked on, all without dropout (the kernel has none)"""
    return ([R.masks_call(0.0), R.scores_call(0.0)] + [R.length_call(L, 0.0) for L in GRAD_LENGTHS]
            + [R.length_call(L, 0.0, nh=3) for L in GRAD_LONG] + [R.packed_call(0.0)])


# ---------------------------------------------------------------------------------------------------------------------------
# relevance
# ---------------------------------------------------------------------------------------------------------------------------
REL_L = (1, 17, 64, 164, 193)
REL_NL = (1, 2, 12)


@functools.lru_cache(maxsize=None)
def relevance_maps(L, nl=max(REL_NL)):
    """[nl, 2, L, L] fp32, nonnegative: the fp32-rounded head-mean reference maps of nl seeded calls (B = 2, nh = 2, sample 1
    right-padded by 7 % L as in attn_ref.length_call); a shorter stack is a prefix of it"""
    out = np.zeros((nl, 2, L, L), dtype=F)
    for l in range(nl):
        x, dd = R._operands(900 + 13 * l + L, 2, L, 2)
        m = np.ones((2, L), dtype=F)
        if 7 % L:
            m[1, L - 7 % L:] = 0
        qkv, dO = R._flat(x, dd)
        out[l] = reference(R.Call('relevance-L%d-l%d' % (L, l), 2, 0.0, qkv, dO, mask=m))['mean'].astype(F)
    out.setflags(write=False)
    return out


def relevance_reference(maps, reverse=False):
    """[(R_l, bound_l)] for l = 0 .. nl - 1 in float64 from the fp32 maps [nl, B, L, L]; reverse: the handle of the CPU test's
    mutation (R_l = R_{l-1} + R_{l-1} A_l)"""
    maps = np.asarray(maps, dtype=D)
    nl, B, L = maps.shape[:3]
    out, Rl = [], np.broadcast_to(np.eye(L, dtype=D), (B, L, L))
    for l in range(nl):
        Rl = Rl + (np.matmul(Rl, maps[l]) if reverse else np.matmul(maps[l], Rl))
        out.append((Rl, np.abs(Rl) * np.expm1((l + 1) * (L + 4) * U) + (l + 1) * L * TINY))
    return out


def upper_triangular_maps(L, nl, B=2):
    """[nl, B, L, L] fp32 of zeros and ones, strictly upper triangular (seeded): every R_l is a matrix of small integers"""
    rs = np.random.RandomState(1000 + L)
    return np.ascontiguousarray(np.triu((rs.rand(nl, B, L, L) < 0.3).astype(F), 1))
