"""Float64 references of the pooler and classifier head (csrc/head.hip: uniter_pooler_fwd / _bwd, uniter_linear_small_fwd / _bwd and
the one-launch forms uniter_pool_head_fwd / _bwd), the case lists their tests share, and per-element error bounds for an fp32
evaluation.  Plain numpy on the CPU: no GPU, no library.

Every reference takes the fp32 INPUT VALUES the launch gets, widened to float64, restates the formula of include/uniter_hip.h and
returns its value next to the bound on |fp32 result - value|.  The backward passes take `pooled` as an INPUT, as the C ABI does: the
reference is the exact function of that fp32 array, whoever produced it (the GPU test feeds the kernel's own pooled rows), so the
cancellation in 1 - p^2 is bounded absolutely and is not amplified by an error of the forward pass.

Bounds.  U = 2^-24 (half an ulp, relative); each bound is a constant times U times the quantity the rounding scales with.  h0 is
hidden[:, 0, :], sums run over k (columns), n (pooler outputs), c (classes) or b (batch rows).

    pre[b, n]       E_pre = A_DOT U (sum_k |h0_bk| |Wp_nk| + |bp_n|)
                    the dot product relative to its ABSOLUTE terms, as E_s in attn_ref: the bound survives a sum that cancels.
    pooled          E_pre * max slope + TANH_ULPS 2^-23 |tanh(pre)|
                    the slope 1 - tanh^2 <= 1 is taken at the point of [|pre| - E_pre, |pre| + E_pre] nearest zero; TANH_ULPS = 5 is
                    OpenCL's limit for tanh.  Where |pre| - E_pre >= T_SAT the value is EXACTLY +-1 and the bound 0.  T_SAT: the
                    complement 1 - |tanh x| = 2 / (exp(2 x) + 1) < 2 exp(-2 x).  The correctly rounded fp32 result is 1 once that
                    lies below 2^-25 (x > 13 ln 2 = 9.01), but an ulp bound alone lets a tanhf miss 1 by whole ulps there (numpy's
                    fp32 tanh returns 1 - 2^-24 at 9.36).  The promise starts where float64 itself has saturated,
                    2 exp(-2 x) < 2^-54, T_SAT = 27.5 ln 2 = 19.06: the complement is 2^-30 of an fp32 ulp, and no evaluation that
                    is accurate in any sense a library documents keeps a bit of it.
    logits[b, c]    A_DOT U (sum_k |pooled_bk| |Wl_ck| + |bl_c|), on the fp32 pooled rows given (the fused forward: the kernel's own)
    dpooled[b, k]   E_dp = A_CN U sum_c |dlogits_bc| |Wl_ck|                     (Cn terms)
    dpre[b, n]      E_dpre = (1 - p^2) E_dp + A_DPRE U |dpooled| ;  exactly 0 where |p| == 1
                    p p is rounded once (absolute U, p^2 <= 1), 1 - p p once more at most (exact from p^2 >= 0.5 on), the product
                    with dpooled once: about 2 U |dpooled| + U |dpre|.  E_dp is 0 where dpooled is an fp32 input (uniter_pooler_bwd).
    dWp, dbp        A_SUM U sum_b |dpre_bn| |h0_bk| + sum_b E_dpre_bn |h0_bk| + A_ADD U |g0 + s|      (dbp: h0 = 1)
    dWl, dbl        A_SUM U sum_b |dlogits_bc| |pooled_bk|                   + A_ADD U |g0 + s|      (dbl: pooled = 1)
                    the rounding of the batch sum, what the terms' own error adds, and the rounding of the final add into the
                    value g0 already there.  That add alone reaches U |g0 + s| (a sum s far below g0), so A_ADD is 2: a constant
                    of 1 could not stand at twice its share.
    dhidden[b,0,k]  A_DOT U sum_n |dpre_bn| |Wp_nk| + sum_n E_dpre_bn |Wp_nk|  (+ A_ADD U |prev + s| with beta != 0)

The constants are not tuned to the kernels: tests/test_head_bounds_cpu.py evaluates the same formulas in numpy fp32, independently
written, with serial sums in index order and again with pairwise trees, over every case of the lists below; each constant is at
least twice the worst share the worse of the two reaches (the shares are recorded there).  Inputs hold no fp32 subnormals.

Cases.  SHAPES are (B, L, H, Cn), the smallest at which each branch of the kernels can still go wrong (the comment beside each).
Every shape runs the 'randn' pattern; the other value patterns run at PATTERN_SHAPES.  Accumulators (dWp, dbp, dWl, dbl and the
dhidden a beta = 1 launch adds to) start from randn, never from zeros.
    randn       hidden ~ randn, Wp, Wl ~ randn / sqrt(H), biases ~ 0.1 randn: |pre| near 1
    cancel      everything at scale 1 (|pre| ~ sqrt(H): a natural mix of saturated and live units).  Paired signs: the odd columns of
                Wp are the even ones times (1 + 2^-10 r), the odd rows of Wp and bp repeat the even ones, the odd columns of Wl are
                MINUS the even ones times (1 + 2^-10 r) and Wl is scaled to 1e4; the samples in `cancel_rows` have h0 = 1e4 v with
                v_odd = -v_even.  Their pre, and every logit, is a sum with |sum a b| below sum |a| |b| / CANCEL_FACTOR.
    zero_pre    h0 == 0 and bp == 0: pooled == 0 and logits == bl exactly
    saturated   column 0 of Wp is 3 (-1)^n and the samples in `sat_rows` (every other one) have h0[0] = +-10: |pre| >= T_SAT on
                every unit with both signs, pooled exactly +-1, dpre exactly 0, the sample's dhidden row 0 and its share of dWp, dbp
    near_sat    bp = +-(6.3 .. 7.7), h0 ~ 0.05 randn: 6 < |pre| < 8, |p| < 1 and 1 - p^2 a few ulps of 1
    zero_dlog   the randn pattern with dlogits == 0: every accumulator keeps its bits, dhidden[:, 0] == 0"""
import math
import zlib

import numpy as np

U = 2.0 ** -24
ULP = 2.0 ** -23
A_DOT = 16.0
A_CN = 8.0
A_DPRE = 8.0
A_SUM = 8.0
A_ADD = 2.0
TANH_ULPS = 5.0
T_SAT = 27.5 * math.log(2.0)
CANCEL_FACTOR = 100.0

F = np.float32
D = np.float64


def worst_ratio(got, ref, bound):
    """max of |got - ref| / bound over the elements; an element with bound 0 must be exact; a NaN or an infinity counts as inf"""
    got, ref, bound = np.asarray(got, dtype=D), np.asarray(ref, dtype=D), np.asarray(bound, dtype=D)
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    if not np.all(np.isfinite(r)):
        return math.inf
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------
def _d(*xs):
    return [np.asarray(x, dtype=D) for x in xs]


def ref_pooler_fwd(hidden, Wp, bp):
    """pooled[b, :] = tanh(hidden[b, 0, :] @ Wp^T + bp) -> dict pre, E_pre, pooled, E_pooled, saturated (bool: exactly +-1)"""
    hidden, Wp, bp = _d(hidden, Wp, bp)
    h0 = hidden[:, 0, :]
    pre = h0 @ Wp.T + bp
    E_pre = A_DOT * U * (np.abs(h0) @ np.abs(Wp).T + np.abs(bp))
    lo = np.maximum(np.abs(pre) - E_pre, 0.0)
    sat = lo >= T_SAT
    pooled = np.where(sat, np.sign(pre), np.tanh(pre))
    E = np.where(sat, 0.0, E_pre * (1.0 - np.tanh(lo) ** 2) + TANH_ULPS * ULP * np.abs(pooled))
    return dict(pre=pre, E_pre=E_pre, pooled=pooled, E_pooled=E, saturated=sat)


def ref_linear_fwd(x, W, b):
    """y[b, c] = x[b, :] . W[c, :] + b[c] -> y, E"""
    x, W, b = _d(x, W, b)
    return x @ W.T + b, A_DOT * U * (np.abs(x) @ np.abs(W).T + np.abs(b))


def ref_linear_bwd(dy, x, W, dW0, db0):
    """dx = dy @ W;  dW = dW0 + dy^T x;  db = db0 + colsum(dy) -> dict dx, dW, db, E_dx, E_dW, E_db"""
    dy, x, W, dW0, db0 = _d(dy, x, W, dW0, db0)
    dW, db = dW0 + dy.T @ x, db0 + dy.sum(0)
    return dict(dx=dy @ W, E_dx=A_CN * U * (np.abs(dy) @ np.abs(W)),
                dW=dW, E_dW=A_SUM * U * (np.abs(dy).T @ np.abs(x)) + A_ADD * U * np.abs(dW),
                db=db, E_db=A_SUM * U * np.abs(dy).sum(0) + A_ADD * U * np.abs(db))


def ref_pooler_bwd(dpooled, pooled, hidden, Wp, dWp0, dbp0, dh_prev=None, E_dpooled=None):
    """dpre = dpooled (1 - pooled^2);  dWp = dWp0 + dpre^T h0;  dbp = dbp0 + colsum(dpre);  dh0 = dpre @ Wp (what a
    beta_dhidden = 0 launch assigns to row 0);  with dh_prev also dh0_add = dh_prev[:, 0] + dh0 (beta_dhidden != 0)
    -> dict dpre, dWp, dbp, dh0 (, dh0_add) and their E_...  E_dpooled: the bound of a dpooled the launch computes for itself (the fused
    backward); None where dpooled is the fp32 array the launch reads"""
    dpooled, pooled, hidden, Wp, dWp0, dbp0 = _d(dpooled, pooled, hidden, Wp, dWp0, dbp0)
    h0 = hidden[:, 0, :]
    one_m = 1.0 - pooled * pooled
    dpre = dpooled * one_m
    E_dpre = np.where(np.abs(pooled) == 1.0, 0.0, A_DPRE * U * np.abs(dpooled) + (0.0 if E_dpooled is None else E_dpooled * one_m))
    dWp, dbp = dWp0 + dpre.T @ h0, dbp0 + dpre.sum(0)
    E_dWp = A_SUM * U * (np.abs(dpre).T @ np.abs(h0)) + E_dpre.T @ np.abs(h0) + A_ADD * U * np.abs(dWp)
    E_dbp = A_SUM * U * np.abs(dpre).sum(0) + E_dpre.sum(0) + A_ADD * U * np.abs(dbp)
    dh0 = dpre @ Wp
    E_dh0 = A_DOT * U * (np.abs(dpre) @ np.abs(Wp)) + E_dpre @ np.abs(Wp)
    out = dict(dpre=dpre, E_dpre=E_dpre, dWp=dWp, E_dWp=E_dWp, dbp=dbp, E_dbp=E_dbp, dh0=dh0, E_dh0=E_dh0)
    if dh_prev is not None:
        out['dh0_add'] = np.asarray(dh_prev, dtype=D)[:, 0, :] + dh0
        out['E_dh0_add'] = E_dh0 + A_ADD * U * np.abs(out['dh0_add'])
    return out


def ref_head_bwd(c, pooled):
    """the fused backward (uniter_pool_head_bwd) of case c from the fp32 pooled rows given: dWl, dbl as ref_linear_bwd, then
    ref_pooler_bwd on the float64 dpooled with its bound -> dict dWp, dbp, dWl, dbl, dh0, dh0_add and their E_..."""
    lb = ref_linear_bwd(c['dlog'], pooled, c['Wl'], c['dWl0'], c['dbl0'])
    pb = ref_pooler_bwd(lb['dx'], pooled, c['hidden'], c['Wp'], c['dWp0'], c['dbp0'], c['dh_prev'], E_dpooled=lb['E_dx'])
    return dict(pb, dWl=lb['dW'], E_dWl=lb['E_dW'], dbl=lb['db'], E_dbl=lb['E_db'], dpooled=lb['dx'], E_dpooled=lb['E_dx'])


# ---------------------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = (
    (1, 1, 4, 1),          # one workgroup, L = 1, the ticket with total = 1
    (3, 2, 8, 2),          # two workgroups
    (4, 3, 60, 3),         # 15 workgroups: fewer than the 16 counter groups; H % 64 != 0
    (5, 2, 64, 1),         # B % 4 != 0: the second batch group has one live row
    (2, 3, 66, 2),         # scalar path (H % 4 != 0), two columns past a wave
    (7, 2, 70, 16),        # scalar path, Cn = 16 (the most pool_head sends to the fused form): 112 tasks over 8 task slots
    (2, 1, 4, 4),          # Cn == H, the backward's limit
    (64, 1, 68, 1),        # the W role's 64-row batch chunks: exactly one ...
    (65, 2, 68, 2),        # ... one row into the second ...
    (129, 2, 36, 1),       # ... one row into the third; H / 4 < 64 with more batch rows than that
    (2, 2, 1028, 2),       # the second 1024-column pass of the fused logits: one 16-byte group of columns into it
    (1, 2, 1092, 3),       # ... 68 columns into it: two loads per lane
    (1, 1, 1027, 1),       # ... with the scalar path
    (2, 1, 4096, 2),       # PHB_MAX_H
    (16, 3, 768, 1),       # the model's H, short L
)
PATTERNS = ('randn', 'cancel', 'zero_pre', 'saturated', 'near_sat', 'zero_dlog')
PATTERN_SHAPES = ((1, 1, 4, 1), (4, 3, 60, 3), (7, 2, 70, 16), (65, 2, 68, 2), (1, 2, 1092, 3), (16, 3, 768, 1))


def workgroups(shape):
    """the forward grid: ceil(H / 4) x ceil(B / 4)"""
    B, _, H, _ = shape
    return ((H + 3) // 4) * ((B + 3) // 4)


def cases():
    """(shape, pattern) of every case"""
    return [(s, 'randn') for s in SHAPES] + [(s, p) for p in PATTERNS[1:] for s in PATTERN_SHAPES]


def case_id(shape, pattern):
    return '%s-%s' % ('x'.join(str(v) for v in shape), pattern)


def _rng(*key):
    return np.random.default_rng([k if isinstance(k, int) and k >= 0 else zlib.crc32(str(k).encode()) for k in key])


def head_case(shape, pattern='randn', seed=0):
    """-> dict of float32 arrays hidden [B, L, H], Wp [H, H], bp [H], Wl [Cn, H], bl [Cn], dlog [B, Cn], the accumulators' prior
    values dWp0, dbp0, dWl0, dbl0 and dh_prev [B, L, H], and the lists sat_rows, cancel_rows"""
    assert pattern in PATTERNS, pattern
    B, L, H, Cn = shape
    r = _rng(seed, B, L, H, Cn, pattern)
    n = r.standard_normal
    hidden, Wp, bp = n((B, L, H)), n((H, H)) / math.sqrt(H), 0.1 * n(H)
    Wl, bl, dlog = n((Cn, H)) / math.sqrt(H), 0.1 * n(Cn), n((B, Cn))
    sat_rows, cancel_rows = [], []
    if pattern == 'cancel':
        assert H % 2 == 0, 'the cancel pattern pairs columns'
        Wp, bp, Wl = n((H, H)), n(H), n((Cn, H))
        Wp[:, 1::2] = Wp[:, 0::2] * (1.0 + 2.0 ** -10 * n((H, H // 2)))
        Wp[1::2] = Wp[0::2]
        bp[1::2] = bp[0::2]
        Wl[:, 1::2] = -Wl[:, 0::2] * (1.0 + 2.0 ** -10 * n((Cn, H // 2)))
        Wl *= 1e4
        cancel_rows = sorted({0, B - 1})
        for b in cancel_rows:
            hidden[b, 0] = 1e4 * n(H)
            hidden[b, 0, 1::2] = -hidden[b, 0, 0::2]
    elif pattern == 'zero_pre':
        hidden[:, 0] = 0.0
        bp[:] = 0.0
    elif pattern == 'saturated':
        Wp[:, 0] = 3.0 * (-1.0) ** np.arange(H)
        sat_rows = list(range(0, B, 2))
        for i, b in enumerate(sat_rows):
            hidden[b, 0, 0] = 10.0 * (-1.0) ** i
    elif pattern == 'near_sat':
        hidden[:, 0] *= 0.05
        bp = r.uniform(6.3, 7.7, H) * (-1.0) ** np.arange(H)
    elif pattern == 'zero_dlog':
        dlog[:] = 0.0
    out = dict(hidden=hidden, Wp=Wp, bp=bp, Wl=Wl, bl=bl, dlog=dlog, dWp0=n((H, H)), dbp0=n(H), dWl0=n((Cn, H)), dbl0=n(Cn),
               dh_prev=n((B, L, H)))
    out = {k: np.ascontiguousarray(v, dtype=F) for k, v in out.items()}
    out.update(sat_rows=sat_rows, cancel_rows=cancel_rows, shape=shape, pattern=pattern)
    return out
