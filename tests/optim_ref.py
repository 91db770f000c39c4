"""Float64 reference of the fused optimizer step and of the clip norm (csrc/optim.hip), with per-element error bounds for an
fp32 evaluation.  Plain numpy: no GPU, no library.

The contract is that of include/uniter_hip.h, "Optimizer step over FLAT fp32 buffers":

    coef = gscale * min(1, max_norm / (sqrt(sumsq) * gscale + 1e-6))        (max_norm <= 0: coef = gscale)
    Adam  (adamw = 0):  g' = g * coef + wd * p,  p0 = p
    AdamW (adamw = 1):  g' = g * coef,           p0 = p * (1 - lr * wd)     wd only where chunk flag & 3 == 2
    m' = b1 m + (1 - b1) g',   v' = b2 v + (1 - b2) g'^2
    p' = p0 - lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps),   bc1 = 1 - b1^step, bc2 = 1 - b2^step

ref_step takes the fp32 INPUT VALUES (p, g, m, v) widened to float64 and the fp32 VALUES of the hyper-parameters, as the C ABI
receives them (f32(lr) and so on: lr = 3e-5 is not an fp32 number, and the difference is 3e-8 relative, half a rounding).

The bound is a first-order propagation of fp32 rounding, U = 2^-24, with ONE constant C = 16:

    Sg    = |g coef| (+ |wd p| for Adam)            absolute terms: the bound survives the cancellation of g coef + wd p
    E_m   = C U (|b1 m| + (1 - b1) Sg)
    E_v   = C U (b2 v + (1 - b2) Sg^2)
    E_rt  = min(E_v / sqrt(v'), sqrt(E_v))          error of sqrt(v'); the second form where v' ~ 0
    E_den = E_rt / sqrt(bc2) + C U den
    den_lo = max(den - E_den, eps / 2)
    E_p   = C U (|p'| + |upd|) + (lr / bc1) (E_m / den_lo + |m'| E_den / (den den_lo)) + C U |upd|

C is derived, not tuned: the longest chain (v) carries about ten roundings relative to its absolute terms -- g coef, wd p, their
sum, the square (which doubles the three before it), two products and one sum -- and the few roundings of coef itself; division
and square root are correctly rounded (the library is built without fast-math and with -ffp-contract=off).
tests/test_optim_bounds_cpu.py holds a numpy-fp32 evaluation of the contract to HALF of every bound and shows that wrong
formulas miss it by large factors.

The bound assumes that no intermediate is an fp32 subnormal: inputs are to be generated so that |g coef| is exactly 0 or
>= 1e-12 (make_case does), and the moments likewise.

ref_sumsq: the float64 sum of squares over flagged chunks; an fp32 kernel that squares and pair-sums in fp32 (two roundings on
non-negative terms) and accumulates in double (n 2^-53: nothing below 2^27 terms) is held to 3 * 2^-24 * ref."""
import math

import numpy as np

U = 2.0 ** -24
C = 16.0
CHUNK = 64
SUMSQ_REL = 3.0 * U
COMBINE_REL = 2.0 ** -45          # uniter_sumsq_combine: a double tree over at most 2^16 parts, against sum |parts|


def f32(x):
    """the fp32 value of a hyper-parameter, as a Python float"""
    return float(np.float32(x))


class Hyper:
    """hyper-parameters of one step; every float attribute holds the fp32 value the C ABI receives"""

    def __init__(self, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=1, adamw=0, gscale=1.0, max_norm=0.0):
        self.lr, self.b1, self.b2, self.eps, self.wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
        self.gscale, self.max_norm = f32(gscale), f32(max_norm)
        self.step, self.adamw = int(step), int(adamw)

    def c_args(self):
        """grad_scale .. adamw in the order of uniter_adam_step*"""
        return (self.gscale, self.max_norm, self.lr, self.b1, self.b2, self.eps, self.wd, self.step, self.adamw)

    def replace(self, **kw):
        h = Hyper.__new__(Hyper)
        h.__dict__.update(self.__dict__)
        for k, val in kw.items():
            setattr(h, k, val if k in ('step', 'adamw') else f32(val))
        return h


def clip_coef(sumsq, h):
    """coef of the contract; sumsq: float (the float64 sum of squares) or None"""
    if h.max_norm > 0.0 and sumsq is not None:
        return h.gscale * min(1.0, h.max_norm / (math.sqrt(sumsq) * h.gscale + 1e-6))
    return h.gscale


def expand_flags(flags, n):
    """per-chunk flags -> per-element"""
    return np.repeat(np.asarray(flags, dtype=np.uint8), CHUNK)[:n]


def ref_step(p, g, m, v, flags, h, sumsq=None):
    """One step in float64 on the fp32 input values, every element treated as updated (the caller masks the chunks whose
    flag & 3 is 0: those are not touched at all).  flags: per 64-element chunk.  -> dict of float64 arrays p, m, v (new values)
    and E_p, E_m, E_v (bounds on |fp32 result - new value|)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    n = p.size
    decay = (expand_flags(flags, n) & 3) == 2
    wd = np.where(decay, h.wd, 0.0)
    coef = clip_coef(sumsq, h)
    bc1 = 1.0 - h.b1 ** h.step
    bc2 = 1.0 - h.b2 ** h.step
    gc = g * coef
    if h.adamw:
        gg, p0, Sg = gc, p * (1.0 - h.lr * wd), np.abs(gc)
    else:
        gg, p0, Sg = gc + wd * p, p, np.abs(gc) + np.abs(wd * p)
    m1 = h.b1 * m + (1.0 - h.b1) * gg
    v1 = h.b2 * v + (1.0 - h.b2) * gg * gg
    rt = np.sqrt(v1)
    den = rt / math.sqrt(bc2) + h.eps
    step_size = h.lr / bc1
    upd = step_size * m1 / den
    p1 = p0 - upd
    E_m = C * U * (np.abs(h.b1 * m) + (1.0 - h.b1) * Sg)
    E_v = C * U * (h.b2 * v + (1.0 - h.b2) * Sg * Sg)
    with np.errstate(divide='ignore', invalid='ignore'):
        E_rt = np.where(rt > 0.0, np.minimum(E_v / rt, np.sqrt(E_v)), np.sqrt(E_v))
    E_den = E_rt / math.sqrt(bc2) + C * U * den
    den_lo = np.maximum(den - E_den, h.eps / 2.0)
    E_p = C * U * (np.abs(p1) + np.abs(upd)) + step_size * (E_m / den_lo + np.abs(m1) * E_den / (den * den_lo)) + C * U * np.abs(upd)
    return dict(p=p1, m=m1, v=v1, E_p=E_p, E_m=E_m, E_v=E_v)


def ref_sumsq(values, flags=None):
    """float64 sum of squares of `values` over the chunks whose flag is non-zero (flags None: all of them); values in other
    chunks are not looked at (they may be NaN)"""
    x = np.asarray(values, dtype=np.float64)
    if flags is not None:
        x = x[expand_flags(flags, x.size) != 0]
    return float(np.sum(x * x))          # numpy float64 pairwise summation: n 2^-53 log n


def worst_ratio(got, ref, bound):
    """max of |got - ref| / bound over the elements; an element with bound 0 must be exact (ratio 0, else inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    if not np.all(np.isfinite(r)):
        return math.inf
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
MOMENTS = ('zero', 'warm', 'stale_hi', 'stale_lo')


def make_case(n, seed, gmag=1.0, moments='warm', wd=1e-2, coef_hint=1.0):
    """fp32 inputs p, g, m, v of n elements (float32 arrays), free of fp32 subnormals in every intermediate:
    - g ~ gmag * N(0, 1) with |N| clamped to >= 0.1, a seventh of them exactly zero (|g coef| is 0 or >= 1e-12 for
      gmag >= 1e-8 and coef >= 1e-3);
    - a fifth planted so that g coef + wd p cancels to about 1e-6 relative (coef_hint = the coef the step will use; only where
      that g is within 1e-3 .. 3 of gmag: a cancellation needs terms of like size);
    - p ~ 0.05 N(0, 1), an eighth of them near 1;
    - moments: zero | warm (m ~ 0.3 gmag N, v ~ gmag^2 (0.1 + N^2)) | stale_hi (v 1e2 times larger) | stale_lo (v 1e-12 times
      smaller than g^2)."""
    r = np.random.default_rng(seed)
    z = r.standard_normal(n)
    z = np.where(np.abs(z) < 0.1, np.copysign(0.1, z), z)
    g = gmag * z
    p = 0.05 * r.standard_normal(n)
    p = np.where(np.abs(p) < 1e-4, 1e-4, p)
    k = r.integers(0, 8, n)
    p = np.where(k == 0, 1.0 + 1e-3 * r.standard_normal(n), p)
    p = p.astype(np.float32)
    if wd > 0 and coef_hint > 0:
        cancel = -f32(wd) * p.astype(np.float64) / coef_hint * (1.0 + 1e-6 * np.sign(r.standard_normal(n)))
        ok = (np.abs(cancel) >= 1e-3 * gmag) & (np.abs(cancel) <= 3.0 * gmag)       # (the norm stays about that of the random part)
        g = np.where((r.integers(0, 5, n) == 0) & ok, cancel, g)
    g = np.where(r.integers(0, 7, n) == 0, 0.0, g).astype(np.float32)
    if moments == 'zero':
        m, v = np.zeros(n), np.zeros(n)
    else:
        ge = gmag * coef_hint if coef_hint > 0 else gmag
        m = 0.3 * ge * r.standard_normal(n)
        m = np.where(np.abs(m) < 1e-3 * ge, 1e-3 * ge, m)
        v = ge * ge * (0.1 + r.standard_normal(n) ** 2)
        if moments == 'stale_hi':
            v = v * 1e2
        elif moments == 'stale_lo':
            v = v * 1e-12
        elif moments != 'warm':
            raise ValueError(moments)
    return p, g, m.astype(np.float32), v.astype(np.float32)


def make_flags(nchunks, seed, choices=(0, 1, 2, 5, 6)):
    """per-chunk flags drawn from `choices` in runs of length 1 (neighbours always differ), every choice present where there is room"""
    r = np.random.default_rng(seed)
    c = np.asarray(choices, dtype=np.uint8)
    idx = np.empty(nchunks, dtype=np.int64)
    prev = -1
    draws = r.integers(0, len(c) - 1, nchunks) if len(c) > 1 else np.zeros(nchunks, dtype=np.int64)
    for i in range(nchunks):
        if i < len(c):
            k = (i + 1 + seed % (len(c) - 1)) % len(c) if len(c) > 1 else 0      # the first chunks walk through every choice,
                                                                                  # beginning behind the first of them (0 = skip)
        else:
            k = draws[i] + (draws[i] >= prev)
        idx[i] = prev = k
    return c[idx]


CLIPS = ('off', 'active', 'tiny', 'null', 'zero')


def build_case(n, seed, adamw=0, step=1, gmag=1.0, lr=1e-3, wd=1e-2, moments='warm', clip='off', b1=0.9, gscale=0.125,
               flag_choices=(0, 1, 2, 5, 6)):
    """-> p, g, m, v (float32 arrays), flags (uint8 per chunk), Hyper, sumsq (float64 sum of squares over the flagged chunks, or
    None).  clip: 'off' = max_norm far above the norm (min(1, .) = 1); 'active' = coef about 0.1 gscale; 'tiny' = total * gscale
    about 1e-3 against max_norm 1e-4, where the + 1e-6 of the contract is worth 1e-3; 'null' = max_norm 0, no sumsq; 'zero' =
    max_norm > 0 with all-zero gradients and sumsq 0."""
    flags = make_flags((n + CHUNK - 1) // CHUNK, seed + 1, flag_choices)
    h = Hyper(lr=lr, b1=b1, wd=wd, step=step, adamw=adamw, gscale=gscale)
    factor = 0.1 if clip in ('active', 'tiny') else 1.0
    p, g, m, v = make_case(n, seed, gmag, moments, wd, coef_hint=h.gscale * factor)
    if clip == 'tiny':
        h = h.replace(gscale=1e-3 / math.sqrt(ref_sumsq(g, flags)))
        p, g, m, v = make_case(n, seed, gmag, moments, wd, coef_hint=h.gscale * factor)
    if clip == 'zero':
        g = np.zeros_like(g)
    sumsq = ref_sumsq(g, flags)
    total = math.sqrt(sumsq) * h.gscale
    if clip == 'off':
        h = h.replace(max_norm=1e3 * total)
    elif clip == 'active':
        h = h.replace(max_norm=0.1 * total)
    elif clip == 'tiny':
        h = h.replace(max_norm=1e-4)
    elif clip == 'zero':
        h = h.replace(max_norm=1.0)
    elif clip == 'null':
        sumsq = None
    else:
        raise ValueError(clip)
    return p, g, m, v, flags, h, sumsq
