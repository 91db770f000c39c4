"""Float64 reference of the optimal-transport distance kernels (csrc/ot.hip: uniter_ot_dist_fwd, uniter_ot_dist_bwd), the yardstick
their error is measured with, the case list their tests share, and wrong versions of the formulas.  Plain torch on the CPU: no GPU,
no library.

Reference.  reference() IS oracle/ot_oracle.py, called on the fp32 input values widened to float64 (beta at its fp32 value, which is
what the C ABI receives); the gradients come from autograd with g as the upstream gradient of the distances.  Nothing is restated here.

Yardstick.  The same evaluation in torch.float32 on the CPU.  For each quantity q of dist [B], T [B, N, M], dx, dy and a case,
    e_ref(q) = max(max|fp32 - float64|, 2^-23 max|float64|)
(the second term, one fp32 unit of the largest value, because 1 x 1 and 0-iteration cases give an fp32 error of exactly 0), a kernel's
error is reported as max|got - float64| / e_ref(q), and the bound is MARGIN[q] e_ref(q).  MARGIN is measured, not derived: about twice
the worst ratio the kernels reach over CASES on an MI355X (recorded in tests/test_ot_f64_gpu.py), rounded up.
tests/test_ot_bounds_cpu.py is the standing proof that the margins still reject every formula of MUTANTS, and that the bound never
exceeds the tolerance tests/test_ot_gpu.py applies to the same quantity (OLD_TOL).

Cases.  Every (M, N) passes the entry point's checks (M N <= 12288, LDS bytes 4 (3 M N + 35 (M + N) + 4) <= 160 KB).  A sample with a
side padded entirely is out of scope: x_len = 0 divides by zero in the reference as well.  No unpadded row has a norm in
[eps / 2, 2 eps] (eps = 1e-5, the clamp of F.normalize): the fp32 and the float64 evaluation must fall on the same side of the clamp.

Mutants.  Each is a textual patch of the oracle's source (the patched module is executed in float64) or a change of what reference()
hands the oracle, never a second implementation.  Two mutants the formulas invite are EQUIVALENT: the plan does not change, in exact
arithmetic, so no test can reject them and a kernel may legitimately be built either way; test_ot_bounds_cpu.py asserts the
equivalence instead:
    x_len_for_y_len     delta scales by y_len / x_len, the sigma computed from it by the inverse, and T = delta Q sigma is unchanged
                        (so is the start value of sigma: only the x_len of the sigma UPDATE shows, mutant y_len_for_x_len)
    plan_not_rezeroed   A is zero at the padded entries, so Q = A T and every later T are zero there; with no iteration T is the
                        masked start value.  Only a plan that is ALSO not masked at the start shows (plan_padding_never_zeroed,
                        on the padded cases with iteration == 0)
one_step_fewer: expected on the cases with iteration in {1, 2}, where it exceeds the bounds 1e8- and 4e5-fold; in fact the proximal
iteration is nowhere near a fixed point after 50 or even 200 steps (13 bounds off at aligned_it200, 135 at it200, 1900 at the model's
shape), so every case rejects it but those with no iteration (it0, it0_65x3) and those with one valid row on a side (1x1, 300x1,
1x300, pad_one_txt, pad_one_img, pad_one_each), whose plan is fixed after the first step."""
import functools
import inspect
import math
import types

import numpy as np
import torch

from oracle import ot_oracle as OT

EPS = 1e-5                                         # the clamp of cost_matrix_cosine
QUANTITIES = ('dist', 'T', 'dx', 'dy')
MARGIN = dict(dist=3.0, T=8.0, dx=4.0, dy=5.0)              # measured worst ratios 1.48, 3.65, 1.60, 2.21 (test_ot_f64_gpu.py)
OLD_TOL = dict(dist=5e-5, T=1e-4, dx=1e-4, dy=1e-4)     # tests/test_ot_gpu.py: tol * max(1, max|ref|), the tighter of its two uses


def f32(v):
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------------------
# reference and yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def evaluate(x, y, x_pad, y_pad, g, beta, iteration, dtype=torch.float64, oracle=OT):
    """oracle.optimal_transport_dist on the values of x, y (fp32 tensors) in `dtype` -> dict dist [B], T [B, N, M], dx, dy"""
    xo, yo = x.detach().to(dtype).clone().requires_grad_(True), y.detach().to(dtype).clone().requires_grad_(True)
    dist, T, _ = oracle.optimal_transport_dist(xo, yo, x_pad.bool(), y_pad.bool(), f32(beta), int(iteration))
    dist.backward(g.to(dtype))
    return dict(dist=dist.detach(), T=T.detach(), dx=xo.grad, dy=yo.grad)


def reference(x, y, x_pad, y_pad, g, beta, iteration):
    """float64: dist [B], T [B, N, M], dx [B, M, D], dy [B, N, D]"""
    r = evaluate(x, y, x_pad, y_pad, g, beta, iteration, torch.float64)
    return r['dist'], r['T'], r['dx'], r['dy']


def yardstick(x, y, x_pad, y_pad, g, beta, iteration, ref=None):
    """-> (e_ref, finite): e_ref[q] as above; finite: the fp32 evaluation holds no NaN and no infinity in any quantity"""
    ref = ref or dict(zip(QUANTITIES, reference(x, y, x_pad, y_pad, g, beta, iteration)))
    lo = evaluate(x, y, x_pad, y_pad, g, beta, iteration, torch.float32)
    e, finite = {}, True
    for q in QUANTITIES:
        finite = finite and bool(torch.isfinite(lo[q]).all()) and bool(torch.isfinite(ref[q]).all())
        e[q] = max((lo[q].double() - ref[q]).abs().max().item(), 2.0 ** -23 * ref[q].abs().max().item())
    return e, finite


def ratio(got, ref, e):
    """max|got - ref| / e; a NaN or an infinity counts as inf; e == 0 asks for the exact value"""
    got = torch.as_tensor(got).detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    if e > 0.0:
        return err / e
    return 0.0 if err == 0.0 else math.inf


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def _case(name, B, M, N, D, beta=0.5, it=50, pad='none', kind='randn', g='rand'):
    return dict(id=name, B=B, M=M, N=N, D=D, beta=beta, iteration=it, pad=pad, kind=kind, g=g, seed=len(_LIST) + 1)


_LIST = []


def _add(*a, **k):
    _LIST.append(_case(*a, **k))


# D: the 32-column staging tail, the 64-lane stride, the backward's 256-column chunk and its second chunk
for _D, _pad in ((1, 'none'), (7, 'suffix'), (31, 'middle'), (32, 'suffix'), (33, 'middle'), (63, 'suffix'), (64, 'none'),
                 (65, 'middle'), (255, 'suffix'), (256, 'middle'), (257, 'suffix')):
    _add('D%d' % _D, 2, 5, 3, _D, pad=_pad)
_add('D768_model_shape', 2, 60, 36, 768, pad='suffix')                    # the model's own shape, the defaults (0.5, 50)
# M, N: a single row / column, 63 / 64 / 65 for the wave-strided sums, more rows than threads, the largest that fit
_add('1x1', 3, 1, 1, 8)
_add('64x64', 2, 64, 64, 33, pad='middle')
_add('65x3', 2, 65, 3, 31, pad='suffix')
_add('3x65', 2, 3, 65, 31, pad='suffix')
_add('63x36', 2, 63, 36, 65, pad='middle')
_add('128x64', 2, 128, 64, 64, pad='suffix')
_add('100x100', 2, 100, 100, 40, pad='middle')
_add('300x1', 2, 300, 1, 7, pad='middle')
_add('1x300', 2, 1, 300, 7, pad='suffix')
_add('257x30', 2, 257, 30, 33, pad='suffix')
_add('B1', 1, 5, 3, 33, pad='middle')
_add('B70', 70, 5, 3, 7, pad='middle')
# padding
_add('pad_one_txt', 3, 9, 6, 33, pad='one_txt')
_add('pad_one_img', 3, 9, 6, 33, pad='one_img')
_add('pad_one_each', 3, 9, 6, 33, pad='one_each')
_add('pad_middle_65', 4, 65, 7, 33, pad='middle')
# input kinds
_add('aligned', 3, 12, 9, 64, kind='aligned', pad='suffix')
_add('aligned_beta0.05', 2, 12, 9, 64, kind='aligned', beta=0.05)
_add('aligned_it200', 2, 12, 9, 64, kind='aligned', it=200, pad='middle')
_add('aligned_beta0.1_it200', 2, 12, 9, 64, kind='aligned', beta=0.1, it=200, pad='middle')
_add('anti', 3, 12, 9, 64, kind='anti', pad='suffix')
_add('anti_beta0.1', 2, 12, 9, 64, kind='anti', beta=0.1, pad='middle')
_add('scaled', 3, 12, 9, 65, kind='scaled', pad='middle')
_add('zero_rows', 3, 12, 9, 65, kind='zero_rows', pad='suffix')
_add('tiny_rows', 3, 12, 9, 64, kind='tiny_rows', pad='suffix')
_add('tiny_rows_D257', 2, 5, 3, 257, kind='tiny_rows')
# beta, iteration
for _beta in (0.05, 0.1, 1.0, 2.0):
    _add('beta%g' % _beta, 2, 20, 12, 33, beta=_beta, pad='suffix')
for _it in (0, 1, 2, 200):
    _add('it%d' % _it, 2, 20, 12, 33, it=_it, pad='middle')
_add('it0_65x3', 2, 65, 3, 7, it=0, pad='suffix')
_add('it1_beta0.1', 2, 7, 11, 31, it=1, beta=0.1)
_add('it200_beta2', 2, 7, 11, 31, it=200, beta=2.0, pad='suffix')
# g
_add('g_ones', 3, 7, 11, 33, g='ones', pad='suffix')
_add('g_zero', 3, 7, 11, 33, g='zero', pad='middle')
_add('g_big', 3, 7, 11, 33, g='big', pad='suffix')

CASES = tuple(_LIST)
CASE_IDS = tuple(c['id'] for c in CASES)
BY_ID = {c['id']: c for c in CASES}
assert len(BY_ID) == len(CASES)


def lds_bytes(M, N):
    return 4 * (3 * M * N + 2 * (M + N) + 33 * (M + N) + 4)


def _pads(c, r):
    """-> x_pad [B, M], y_pad [B, N] bool.  Every pattern but 'none' differs from sample to sample, and leaves a valid row a side."""
    B, M, N = c['B'], c['M'], c['N']
    xp, yp = torch.zeros(B, M, dtype=torch.bool), torch.zeros(B, N, dtype=torch.bool)
    kind = c['pad']
    for b in range(B):
        if kind == 'suffix' and b > 0:                     # as tests/test_ot_gpu.py: sample 0 whole
            xp[b, max(1, M - (3 * b) % M):] = True
            yp[b, max(1, N - (5 * b) % N):] = True
        elif kind == 'middle':                             # flags that are no suffix: the first and the last row stay valid
            for p, L in ((xp, M), (yp, N)):
                if L >= 3:
                    p[b, 1:L - 1] = torch.from_numpy(r.random(L - 2) < 0.4)
                    p[b, 1 + (b % (L - 2))] = True
        if kind in ('one_txt', 'one_each'):                # one valid text row, at another place in every sample
            xp[b] = True
            xp[b, (4 * b + 1) % M] = False
        if kind in ('one_img', 'one_each'):
            yp[b] = True
            yp[b, (2 * b + 2) % N] = False
        if kind == 'one_txt':
            yp[b, N - 1 - b:] = True
        if kind == 'one_img':
            xp[b, :b] = True
    return xp, yp


def make(c):
    """-> dict x [B, M, D], y [B, N, D] float32, x_pad, y_pad bool, g [B] float32, beta, iteration (tensors on the CPU)"""
    c = BY_ID[c] if isinstance(c, str) else c
    B, M, N, D = c['B'], c['M'], c['N'], c['D']
    r = np.random.default_rng([c['seed'], B, M, N, D])

    def randn(*s):
        return torch.from_numpy(r.standard_normal(s).astype(np.float32))
    x = randn(B, M, D)
    idx = torch.arange(N) % M
    kind = c['kind']
    if kind in ('randn', 'zero_rows', 'tiny_rows', 'scaled'):
        y = randn(B, N, D) + 0.2 * x[:, :1, :]
    elif kind == 'aligned':                                # every image row a text row plus small noise: costs near 0, a peaked plan
        y = x[:, idx, :] + 0.01 * randn(B, N, D)
    elif kind == 'anti':                                   # every pair nearly opposite: costs near 2
        v = randn(B, 1, D)
        x = v + 0.05 * x
        y = -v + 0.05 * randn(B, N, D)
    else:
        raise ValueError(kind)
    xp, yp = _pads(c, r)
    if kind == 'scaled':                                   # the cost is scale-free; the backward divides by the norm
        x[:, 0::2] *= 1e3
        x[:, 1::2] *= 1e-3
        y[:, 0::2] *= 1e-3
        y[:, 1::2] *= 1e3
    if kind in ('zero_rows', 'tiny_rows'):                 # the clamp, on the first unpadded row of each side in samples 0 and 1
        for b in range(min(B, 2)):
            i, j = int((~xp[b]).nonzero()[-b]), int((~yp[b]).nonzero()[0])    # (sample 1: its last valid text row)
            x[b, i] = 0.0 if kind == 'zero_rows' else 1e-7 * randn(D)         # 0 < |x| < eps: the clamped branch with own != 0
            y[b, j] = 0.0 if kind == 'zero_rows' else 1e-7 * randn(D)
    gk = c['g']
    g = torch.ones(B) if gk == 'ones' else randn(B) * torch.exp(randn(B))
    if gk == 'zero':
        g[1] = 0.0
    if gk == 'big':
        g[B - 1] = -1e3
    return dict(x=x.contiguous(), y=y.contiguous(), x_pad=xp, y_pad=yp, g=g.float(), beta=c['beta'], iteration=c['iteration'])


def args(d):
    return d['x'], d['y'], d['x_pad'], d['y_pad'], d['g'], d['beta'], d['iteration']


@functools.lru_cache(maxsize=None)
def solved(case_id):
    """(inputs, float64 reference as a dict, e_ref, finite) of a case: computed once, shared by the tests, not to be written to"""
    d = make(case_id)
    ref = dict(zip(QUANTITIES, reference(*args(d))))
    e, finite = yardstick(*args(d), ref=ref)
    return d, ref, e, finite


# ---------------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------------
def _soft_norm(v, eps):
    """max(|v|, eps) in value, v / max(|v|, eps) in gradient on BOTH sides of the clamp: what a backward without the clamp branch
    differentiates"""
    s = (v * v).sum(-1, keepdim=True)
    return (s + (eps * eps - s).clamp_min(0).detach()).sqrt()


_NORM = "%s.norm(dim=-1, keepdim=True).clamp_min(eps)"
# name -> [(text of oracle/ot_oracle.py, its replacement, occurrences)]
_PATCHES = {
    'bwd_no_projection': [('.clamp_min(eps)', '.clamp_min(eps).detach()', 2)],
    'bwd_no_clamp_branch': [(_NORM % 'x', '_soft_norm(x, eps)', 1), (_NORM % 'y', '_soft_norm(y, eps)', 1)],
    'pad_1e4_dropped': [('* 1e4)', '* 0.0)', 2)],
    'y_len_for_x_len': [('1 / (xl * delta.matmul(Q)', '1 / (yl * delta.matmul(Q)', 1)],
    'plan_untransposed': [('cost.matmul(T)', 'cost.matmul(T.reshape(cost.shape).transpose(1, 2))', 1)],
    'beta_doubled': [('/ beta)', '/ (2 * beta))', 1)],
    'plan_padding_never_zeroed': [('    T = T.masked_fill(jp, 0)\n', '', 1), ('return T.masked_fill(jp, 0)', 'return T', 1)],
    'one_step_fewer': [('range(iteration)', 'range(max(iteration - 1, 0))', 1)],
    # equivalent (see the module docstring)
    'x_len_for_y_len': [('1 / (yl * Q.matmul(sigma)', '1 / (xl * Q.matmul(sigma)', 1)],
    'plan_not_rezeroed': [('return T.masked_fill(jp, 0)', 'return T', 1)],
}
MUTANTS = ('bwd_no_projection', 'bwd_no_clamp_branch', 'pad_1e4_dropped', 'y_len_for_x_len', 'plan_untransposed', 'beta_doubled',
           'g_of_sample_0', 'plan_padding_never_zeroed', 'one_step_fewer')
EQUIVALENT = ('x_len_for_y_len', 'plan_not_rezeroed')


@functools.lru_cache(maxsize=None)
def _patched_oracle(name):
    src = inspect.getsource(OT)
    for old, new, count in _PATCHES[name]:
        assert src.count(old) == count, 'oracle/ot_oracle.py changed: %r occurs %d times, not %d' % (old, src.count(old), count)
        src = src.replace(old, new)
    m = types.ModuleType('ot_oracle_' + name)
    m._soft_norm = _soft_norm
    exec(compile(src, 'ot_oracle[%s]' % name, 'exec'), m.__dict__)
    return m


def mutant(name, x, y, x_pad, y_pad, g, beta, iteration):
    """the wrong formula `name` in float64 -> dict dist, T, dx, dy"""
    if name == 'g_of_sample_0':
        return evaluate(x, y, x_pad, y_pad, g[:1].expand_as(g), beta, iteration)
    return evaluate(x, y, x_pad, y_pad, g, beta, iteration, oracle=_patched_oracle(name))
