"""uniter_ot_dist_fwd and uniter_ot_dist_bwd (csrc/ot.hip) through the C ABI, and meme_challenge_amd.ot.optimal_transport_dist on
top of them, against the float64 reference, the fp32 yardstick and the case list of tests/ot_ref.py (tests/test_ot_bounds_cpu.py is
the standing proof that the bounds used here reject wrong formulas and never exceed the tolerances of tests/test_ot_gpu.py).

Every output (dist, T, dx, dy) is prefilled with a recognisable NaN and carries GUARD rows of the same pattern behind it; after the
launches every element inside the logical shape is finite, padded plan entries and the gradient rows of padded positions are exact
zeros, every guard still holds its prefill and every input, pad flags included, comes back bit for bit.  The backward launch gets
the float64 plan rounded to fp32, so an error of the forward kernel can neither mask nor fake one of the backward; one test chains
the two launches as ot.py does.  No case is skipped or waived; nothing here reads or writes outside its buffers or expects a launch
to fail (rejections: tests/test_ot_gpu.py).  Samples with a side padded entirely are out of scope (ot_ref.py).

The worst |got - float64| / e_ref per quantity is collected in WORST and printed at the end of the module (-s shows it).
Recorded on an MI355X over the 52 cases and the wrapper tests, worst ratio (case) -> ot_ref.MARGIN, about twice it rounded up:
    dist 1.483 (aligned_beta0.05) -> 3     T 3.648 (beta0.05) -> 8     dx 1.602 (it0_65x3) -> 4     dy 2.206 (300x1) -> 5
73 tests in 3.3 s.  The same module on the kernels as they were before it:
    dist 1.000 (aligned_beta0.05), T 4.679 (aligned_beta0.1_it200), dx 1.180 (pad_one_each), dy INFINITE (D1)
 -  dy at D = 1: the gradient of a cosine cost of scalars is identically zero, and the fp32 yardstick is exactly 0 there; the
    backward's x (x . dn) / |x|^2 left a rounding residue of dn / |x| against values of 0.  The projection is now taken with the
    normalised row x / |x|, which is exactly +-1 at D = 1: dx, dy are exact zeros there (both ratios 0.000); the other cases
    moved by at most 0.7 either way, in units that are one fp32 ulp of the largest gradient on most of them (worst dx 1.180 ->
    1.602, worst finite dy 2.206 before and after, dist and T bit for bit the same).
 -  the worst T ratios sat on the small-beta cases (aligned_beta0.1_it200 4.68, beta0.05 3.07, anti 3.00, the next 2.50), where
    __expf(-c / beta) errs by |c / beta| 2^-24 against libm's ulp.  With expf: aligned_beta0.1_it200 0.99, anti 2.08, beta0.05
    3.65, worst T 4.68 -> 3.65 (dist 1.00 -> 1.48 on aligned_beta0.05).  What is left at beta 0.05 is the rounding of c / beta
    itself, which the yardstick shares, carried through fifty steps."""
import numpy as np
import pytest
import torch

import ot_ref as R

pytestmark = pytest.mark.gpu

GUARD = 2
NANBITS = 0x7fc0beef
WORST = {}


def _L():
    from meme_challenge_amd import _lib
    return _lib


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\not kernels, worst |got - float64| / e_ref: ' + ', '.join('%s %.3f (%s)' % (q, r, c) for q, (r, c) in WORST.items()))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.uint8)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Out:
    """an output of `rows` rows of `width` floats on the device with GUARD more rows behind it, all of it the NaN pattern"""

    def __init__(self, rows, width, shape):
        self.n, self.shape = rows * width, shape
        host = np.full((rows + GUARD) * width, NANBITS, dtype=np.uint32).view(np.float32)
        self.init = torch.from_numpy(host)
        self.dev = self.init.clone().cuda()

    def ptr(self):
        return self.dev.data_ptr()

    def got(self):
        return self.dev[:self.n].cpu().view(self.shape)

    def intact(self):
        return _same(self.dev[self.n:].cpu(), self.init[self.n:])


class In:
    def __init__(self, t):
        self.init = t.contiguous().clone()
        self.dev = self.init.clone().cuda()

    def ptr(self):
        return self.dev.data_ptr()

    def unchanged(self):
        return _same(self.dev.cpu(), self.init)


def _launch(d, plan=None, with_T=True, backward=True):
    """forward, then backward on `plan` (fp32 [B, N, M]; None: on the plan the forward left on the device, as ot.py does)
    -> dict dist, T, dx, dy on the CPU.  Checks finiteness, exact zeros at padding, guards and inputs."""
    L = _L()
    x, y, xp, yp, g = d['x'], d['y'], d['x_pad'], d['y_pad'], d['g']
    B, M, D = x.shape
    N = y.shape[1]
    X, Y, XP, YP, G = In(x), In(y), In(xp.to(torch.uint8)), In(yp.to(torch.uint8)), In(g)
    dist, T = Out(B, 1, (B,)), Out(B * N, M, (B, N, M))
    L.check(L.lib().uniter_ot_dist_fwd(X.ptr(), Y.ptr(), XP.ptr(), YP.ptr(), dist.ptr(), T.ptr() if with_T else None, B, M, N, D,
                                       float(d['beta']), int(d['iteration']), L.cur_stream()), 'uniter_ot_dist_fwd')
    torch.cuda.synchronize()
    out = dict(dist=dist.got())
    assert torch.isfinite(out['dist']).all(), 'dist'
    assert dist.intact() and T.intact(), 'a guard behind dist / T was written'
    if with_T:
        out['T'] = T.got()
        assert torch.isfinite(out['T']).all(), 'T'
        jp = (xp.unsqueeze(1) | yp.unsqueeze(2))                                   # [B, N, M]
        assert (out['T'][jp] == 0).all(), 'plan entries at padded positions'
    else:
        assert _same(T.dev.cpu(), T.init), 'T == NULL, and the buffer next to dist was written'
    assert all(i.unchanged() for i in (X, Y, XP, YP)), 'the forward changed an input'
    if not backward:
        return out
    P = In(plan.float()) if plan is not None else None
    dx, dy = Out(B * M, D, (B, M, D)), Out(B * N, D, (B, N, D))
    L.check(L.lib().uniter_ot_dist_bwd(X.ptr(), Y.ptr(), P.ptr() if P else T.ptr(), G.ptr(), dx.ptr(), dy.ptr(), B, M, N, D,
                                       L.cur_stream()), 'uniter_ot_dist_bwd')
    torch.cuda.synchronize()
    out['dx'], out['dy'] = dx.got(), dy.got()
    assert torch.isfinite(out['dx']).all() and torch.isfinite(out['dy']).all(), 'dx / dy'
    assert (out['dx'][xp] == 0).all() and (out['dy'][yp] == 0).all(), 'gradient rows of padded positions'
    assert dx.intact() and dy.intact() and T.intact() and dist.intact(), 'a guard behind dx / dy was written'
    assert all(i.unchanged() for i in (X, Y, XP, YP, G)) and (P is None or P.unchanged()), 'the backward changed an input'
    if P is None:
        assert _same(T.got(), out['T']), 'the backward changed the plan'
    return out


def _hold(case_id, out, ref, e, quantities=R.QUANTITIES):
    """every ratio is recorded and printed before any is asserted"""
    r = {q: R.ratio(out[q], ref[q], e[q]) for q in quantities}
    for q in quantities:
        if r[q] >= WORST.get(q, (-1.0, ''))[0]:
            WORST[q] = (r[q], case_id)
    print('%s: ' % case_id + ', '.join('%s %.3f' % kv for kv in r.items()) + ' of e_ref')
    for q in quantities:
        assert r[q] <= R.MARGIN[q], (case_id, q, r[q], R.MARGIN[q])


def _identical(a, b, what):
    for q in a:
        assert _same(a[q], b[q]), (what, q)


@pytest.mark.parametrize('case_id', R.CASE_IDS)
def test_ot_kernels_match_float64(case_id):
    d, ref, e, finite = R.solved(case_id)
    assert finite
    _hold(case_id, _launch(d, plan=ref['T']), ref, e)


@pytest.mark.parametrize('case_id', ['D768_model_shape', 'pad_middle_65', 'tiny_rows', 'it1'])
def test_ot_forward_chained_into_backward(case_id):
    """the way ot.py does it: the backward reads the plan the forward left on the device.  Distance and plan are held against the
    reference; the gradients equal, bit for bit, those of a backward launch that is handed that plan as an input."""
    d, ref, e, _ = R.solved(case_id)
    out = _launch(d)
    _hold(case_id + '/chained', out, ref, e, ('dist', 'T'))
    alone = _launch(d, plan=out['T'])
    _identical({q: out[q] for q in ('dx', 'dy')}, {q: alone[q] for q in ('dx', 'dy')}, 'chained against the same plan as an input')


@pytest.mark.parametrize('case_id', ['D33', '257x30', 'pad_one_each', 'it0'])
def test_ot_forward_without_a_plan_gives_the_same_distances(case_id):
    d = R.solved(case_id)[0]
    _identical(dict(dist=_launch(d, with_T=False, backward=False)['dist']), dict(dist=_launch(d, backward=False)['dist']), 'T = NULL')


@pytest.mark.parametrize('case_id', ['D768_model_shape', '100x100', '300x1', 'B70', 'tiny_rows'])
def test_ot_kernels_are_reproducible(case_id):
    """no atomics, a fixed reduction order: two launches agree bit for bit"""
    d = R.solved(case_id)[0]
    _identical(_launch(d), _launch(d), 'second launch')


@pytest.mark.parametrize('case_id', ['pad_one_each', 'scaled', 'g_zero', 'anti'])
def test_ot_samples_are_independent_of_their_batch(case_id):
    """sample b of a B = 3 launch, run alone as B = 1, gives the same bits: a stray batch stride would not"""
    d = R.solved(case_id)[0]
    assert d['x'].shape[0] == 3
    whole = _launch(d)
    for b in range(3):
        one = dict(d, **{k: d[k][b:b + 1] for k in ('x', 'y', 'x_pad', 'y_pad', 'g')})
        _identical(_launch(one), {q: v[b:b + 1] for q, v in whole.items()}, 'sample %d alone' % b)


# ---------------------------------------------------------------------------------------------------------------------------
# through meme_challenge_amd.ot.optimal_transport_dist
# ---------------------------------------------------------------------------------------------------------------------------
WRAPPED = 'g_zero'


def _wrapped(x, y, d, g=None):
    from meme_challenge_amd.ot import optimal_transport_dist
    dist = optimal_transport_dist(x, y, d['x_pad'].cuda(), d['y_pad'].cuda(), d['beta'], d['iteration'])
    dist.backward(d['g'].cuda() if g is None else g)
    torch.cuda.synchronize()
    return dist.detach()


@pytest.mark.parametrize('side', ['txt', 'img'])
def test_ot_wrapper_with_one_side_requiring_grad(side):
    d, ref, e, _ = R.solved(WRAPPED)
    x, y = d['x'].cuda().requires_grad_(side == 'txt'), d['y'].cuda().requires_grad_(side == 'img')
    dist = _wrapped(x, y, d)
    has, hasnot, q = (x, y, 'dx') if side == 'txt' else (y, x, 'dy')
    assert hasnot.grad is None
    _hold(WRAPPED + '/' + side, {'dist': dist, q: has.grad}, ref, e, ('dist', q))


def test_ot_wrapper_casts_bf16_inputs_as_a_cast_by_hand_does():
    d = R.solved(WRAPPED)[0]
    xb, yb = d['x'].cuda().bfloat16().requires_grad_(True), d['y'].cuda().bfloat16().requires_grad_(True)
    xf, yf = xb.detach().float().requires_grad_(True), yb.detach().float().requires_grad_(True)
    db, df = _wrapped(xb, yb, d), _wrapped(xf, yf, d)
    assert db.dtype == torch.float32 and _same(db.cpu(), df.cpu())
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad, xf.grad.bfloat16()) and torch.equal(yb.grad, yf.grad.bfloat16())


def test_ot_wrapper_takes_a_non_contiguous_upstream_gradient():
    d, ref, e, _ = R.solved(WRAPPED)
    g2 = torch.stack([d['g'], torch.full_like(d['g'], 7.0)], dim=1).cuda()[:, 0]
    assert not g2.is_contiguous()
    x, y = d['x'].cuda().requires_grad_(True), d['y'].cuda().requires_grad_(True)
    dist = _wrapped(x, y, d, g=g2)
    _hold(WRAPPED + '/strided g', dict(dist=dist, dx=x.grad, dy=y.grad), ref, e, ('dist', 'dx', 'dy'))
