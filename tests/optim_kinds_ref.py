"""Float64 references of the Adamax and SGD-momentum rules of the fused optimizer step (uniter_optim_step, kinds 2 and 3;
csrc/optim.hip) with per-element error bounds for an fp32 evaluation.  Plain numpy: no GPU, no library.  Inputs, flags, the clip
coefficient and the constants U = 2^-24, C = 16 are those of tests/optim_ref.py.

The contracts (include/uniter_hip.h, uniter_optim_step), with coef as in optim_ref and wd only where the chunk flag & 3 == 2:

    Adamax (torch.optim.Adamax):   g' = g coef + wd p,  m' = b1 m + (1 - b1) g',  u' = max(b2 u, |g'| + eps),
                                   p' = p - lr / bc1 * m' / u',   bc1 = 1 - b1^step        (u: the second state buffer)
    SGD    (torch.optim.SGD, dampening 0, no Nesterov; mu = the b1 slot of the hyper-parameters):
                                   g' = g coef + wd p,  b' = mu b + g',  p' = p - lr b'    (no second state)

ref_step_* take the fp32 INPUT VALUES widened to float64 and the fp32 values of the hyper-parameters (optim_ref.Hyper).

The bounds are the first-order propagation of fp32 rounding that optim_ref.py uses, with the same U and the same C:

    Sg   = |g coef| + |wd p|                 absolute terms: the bound survives the cancellation of g coef + wd p
    E_m  = C U (|b1 m| + (1 - b1) Sg)        as in optim_ref: g' carries three roundings against Sg, the two products and the sum
                                             of m' three more, coef a few of its own
    E_u  = C U (b2 u + Sg + eps)             max is 1-Lipschitz in each argument: |max(a, b) - max(a', b')| <= max(|a - a'|,
                                             |b - b'|); a = b2 u carries one rounding, b = |g'| + eps those of g' plus one
    u_lo = max(u' - E_u, eps / 2)            the smallest denominator an fp32 evaluation can see (u' >= eps always)
    E_p  = C U (|p'| + |upd|) + (lr / bc1) (E_m / u_lo + |m'| E_u / (u' u_lo)),   upd = lr / bc1 * m' / u'
                                             the quotient's error from its numerator and its denominator, then the roundings of
                                             the quotient, of step_size (a double rounded once), of the product and of the
                                             difference, which are relative to |upd| and |p'|
    SGD:
    E_b  = C U (|mu b| + Sg)                 g' as above, one product, one sum
    E_p  = C U (|p'| + |lr b'|) + lr E_b     the error of b' carried through lr, then the product and the difference

C = 16 is NOT re-tuned for these rules: their chains are shorter than Adam's v (no square, no root), so the same constant holds
with more room.  Division is correctly rounded and nothing is contracted (the library is built without fast-math and with
-ffp-contract=off).  tests/test_optim_kinds_bounds_cpu.py holds a numpy-fp32 evaluation of both contracts to HALF of every bound,
shows wrong formulas leaving it, and checks ref_step_* against torch.optim.Adamax / torch.optim.SGD in float64.

Like optim_ref, the bounds assume that no intermediate is an fp32 subnormal (make_case / adamax_state see to that)."""
import numpy as np

from optim_ref import U, C, f32, Hyper, clip_coef, expand_flags, make_case, make_flags, worst_ratio, build_case  # noqa: F401

KIND_ADAM, KIND_ADAMW, KIND_ADAMAX, KIND_SGD = 0, 1, 2, 3
# torch.optim.Adamax's defaults: what the reference's get_optimizer runs with (utils/optim_utils.py:36-37 passes lr only)
ADAMAX_BETAS, ADAMAX_EPS = (0.9, 0.999), 1e-8


def _common(p, g, flags, h, sumsq):
    n = p.size
    decay = (expand_flags(flags, n) & 3) == 2
    wd = np.where(decay, h.wd, 0.0)
    gc = g * clip_coef(sumsq, h)
    return gc + wd * p, np.abs(gc) + np.abs(wd * p)


def ref_step_adamax(p, g, m, u, flags, h, sumsq=None):
    """One Adamax step in float64 on the fp32 input values, every element treated as updated (the caller masks the chunks whose
    flag & 3 is 0).  -> dict of float64 arrays p, m, v (new values; v is the infinity norm u) and E_p, E_m, E_v."""
    p, g, m, u = (np.asarray(a, dtype=np.float64) for a in (p, g, m, u))
    gg, Sg = _common(p, g, flags, h, sumsq)
    bc1 = 1.0 - h.b1 ** h.step
    step_size = h.lr / bc1
    m1 = h.b1 * m + (1.0 - h.b1) * gg
    u1 = np.maximum(h.b2 * u, np.abs(gg) + h.eps)
    upd = step_size * m1 / u1
    p1 = p - upd
    E_m = C * U * (np.abs(h.b1 * m) + (1.0 - h.b1) * Sg)
    E_u = C * U * (h.b2 * u + Sg + h.eps)
    u_lo = np.maximum(u1 - E_u, h.eps / 2.0)
    E_p = C * U * (np.abs(p1) + np.abs(upd)) + step_size * (E_m / u_lo + np.abs(m1) * E_u / (u1 * u_lo))
    return dict(p=p1, m=m1, v=u1, E_p=E_p, E_m=E_m, E_v=E_u)


def ref_step_sgd(p, g, b, flags, h, sumsq=None):
    """One SGD-momentum step in float64 (mu = h.b1).  -> dict of float64 arrays p, m (the momentum buffer) and E_p, E_m."""
    p, g, b = (np.asarray(a, dtype=np.float64) for a in (p, g, b))
    gg, Sg = _common(p, g, flags, h, sumsq)
    b1 = h.b1 * b + gg
    upd = h.lr * b1
    p1 = p - upd
    E_b = C * U * (np.abs(h.b1 * b) + Sg)
    E_p = C * U * (np.abs(p1) + np.abs(upd)) + h.lr * E_b
    return dict(p=p1, m=b1, E_p=E_p, E_m=E_b)


def ref_step_kind(kind, p, g, m, v, flags, h, sumsq=None):
    """the reference of `kind` (2 or 3) with the key set of ref_step_adamax (SGD: no v)"""
    if kind == KIND_ADAMAX:
        return ref_step_adamax(p, g, m, v, flags, h, sumsq)
    if kind == KIND_SGD:
        return ref_step_sgd(p, g, m, flags, h, sumsq)
    raise ValueError(kind)


def adamax_state(v):
    """the infinity-norm state that goes with optim_ref's second moment v ~ g^2: its root (|g|-sized, fp32).  The states of
    optim_ref.MOMENTS become zero | warm | stale_hi (u ten times larger) | stale_lo (u 1e-6 of |g|: the gradient decides the max)."""
    return np.sqrt(np.asarray(v, dtype=np.float64)).astype(np.float32)


def build_kind_case(kind, n, seed, **case):
    """optim_ref.build_case for kind 2 / 3: -> p, g, m, v, flags, Hyper, sumsq with v = the Adamax state (kind 2) or None (kind 3).
    `mu` (kind 3) names the momentum, default 0.9; the Adamax betas are optim_ref's b1 = 0.9, b2 = 0.999 unless `b1` is given."""
    case = dict(case)
    case.pop('adamw', None)
    if kind == KIND_SGD and 'mu' in case:
        case['b1'] = case.pop('mu')
    p, g, m, v, flags, h, sumsq = build_case(n, seed, adamw=0, **case)
    return p, g, m, (adamax_state(v) if kind == KIND_ADAMAX else None), flags, h, sumsq
