"""Float64 reference of the averaged weights the fused optimizer step keeps (uniter_optim_step_avg / uniter_optim_step_groups_avg;
csrc/optim.hip, AVG) with a per-element error bound for an fp32 evaluation.  Plain numpy: no GPU, no library.  The constants
U = 2^-24 and C = 16, the flags and the case generators are those of tests/optim_ref.py.

The contract (include/uniter_hip.h, uniter_optim_step_avg): on every element the launch updates

    a' = fl(a + fl(w * fl(p' - a)))          p' = the fp32 parameter the launch has just computed, w = avg_weight in [0, 1]

and elsewhere (chunk flag & 3 == 0, or a group outside the table) a is neither read nor written.  ref_avg takes the fp32 VALUES
a, p' and w widened to float64 -- p' is the kernel's OWN fp32 result, so the parameter's error (bounded by optim_ref) does not enter
the average's bound a second time.

The bound is the first-order propagation of fp32 rounding that optim_ref.py uses, with the same U and the same C, on the absolute
terms of the sum:

    E_a = C U (|a| + |w (p' - a)|)

Three roundings in all: the difference and the product are each relative to |w (p' - a)|, the sum to |a'| <= |a| + |w (p' - a)|;
nothing is contracted (-ffp-contract=off).  C = 16 is NOT re-tuned: the chain is shorter than any of optim_ref's.  Like optim_ref,
the bound assumes no fp32 subnormal among the intermediates (make_avg sees to that).  A skipped element's bound is 0: bit-exact.

The weight per step is formed in double on the host and handed over as fp32 (trainer.ema_weight):

    w_t = 1 - d_t,   d_t = min(D, (1 + t) / (10 + t)) with warm-up, D without;   t = averaging steps before this one"""
import numpy as np

from optim_ref import U, C, f32, expand_flags, worst_ratio  # noqa: F401

WEIGHTS = (0.9, 0.1, 1e-3)


def ref_weight(decay, t, warmup=True):
    """the weight of the step that follows t earlier ones, as the fp32 value the launch receives (a Python float)"""
    d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return f32(1.0 - d)


def ref_avg(a, p_new, w, upd):
    """a' in float64 from the fp32 values (a, p') and the fp32 weight w; upd: per-element mask of the update path.
    -> dict a (float64; the input where upd is False) and E_a (0 there)."""
    a, p_new = np.asarray(a, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    with np.errstate(all='ignore'):         # (skipped chunks may hold NaN / Inf patterns: masked out below)
        inc = float(w) * (p_new - a)
        out = np.where(upd, a + inc, a)
        E = np.where(upd, C * U * (np.abs(a) + np.abs(inc)), 0.0)
    return dict(a=out, E_a=E)


def make_avg(p_like, seed):
    """an average to go with parameters of the size of `p_like` (fp32): |p - a| of the order of |a| -- a = p x (a factor in
    0.25 .. 1.75 away from 1 by at least 0.05, a tenth of them with the other sign) -- so that a wrong weight, a wrong p or a
    missed skip moves a' by far more than the bound; free of subnormals where p_like is."""
    r = np.random.default_rng(seed)
    n = p_like.size
    f = 0.25 + 1.5 * r.random(n)
    f = np.where(np.abs(f - 1.0) < 0.05, 1.05, f)
    f = np.where(r.integers(0, 10, n) == 0, -f, f)
    return (np.asarray(p_like, dtype=np.float64) * f).astype(np.float32)
