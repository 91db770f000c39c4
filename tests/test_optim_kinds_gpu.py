"""uniter_optim_step (csrc/optim.hip) through the C ABI: the Adamax and SGD-momentum rules (kinds 2 and 3) against the float64
references and the per-element bounds of tests/optim_kinds_ref.py (derivation there; tests/test_optim_kinds_bounds_cpu.py is the
standing proof that an fp32 evaluation of the contracts keeps them and that the contracts are torch's), bit for bit where the
contract is exact, and kinds 0 / 1 bit for bit against uniter_adam_step_x3p.

The harness is that of tests/test_optim_f64_gpu.py (its Buf, guards and poison patterns are imported): every buffer sits between
guard chunks of NaN patterns, chunks whose flag is 0 hold NaN / Inf in every buffer and must come back bit-identical, and the sum
of squares the step consumes is the float64 reference written to the device.  Kind 3 has no second state: it runs with
exp_avg_sq = NULL or with a buffer of NaN patterns that must come back untouched.

The worst error / bound ratios per kind and quantity are collected in WORST and printed at the end of the module (-s shows them).
Recorded on an MI355X: Adamax p 0.093, m 0.244, u 0.202; SGD p 0.088, b 0.243; 135 tests in 15 s."""
import numpy as np
import pytest
import torch

import optim_kinds_ref as K
import optim_ref as R
import test_optim_f64_gpu as A

pytestmark = pytest.mark.gpu

Buf, FILL, GUARD, SIZES, GRIDS = A.Buf, A.FILL, A.GUARD, A.SIZES, A.GRIDS
KINDS = {'adamax': K.KIND_ADAMAX, 'sgd': K.KIND_SGD}
WORST = {'adamax p': 0.0, 'adamax m': 0.0, 'adamax u': 0.0, 'sgd p': 0.0, 'sgd b': 0.0}
NAME = {(2, 'p'): 'adamax p', (2, 'm'): 'adamax m', (2, 'v'): 'adamax u', (3, 'p'): 'sgd p', (3, 'm'): 'sgd b'}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nuniter_optim_step, worst |got - float64| / bound: ' + ', '.join('%s %.3f' % kv for kv in WORST.items()))


def _optim_step(kind, p, g, g16, m, v, flags, n, sumsq, h, zero, mirror, ps, tab, first, wgs):
    L = A._L()
    return L.lib().uniter_optim_step(kind, p, g, g16, m, v, flags, n, sumsq, *h.c_args(), zero, mirror, ps, tab, first, wgs,
                                     L.cur_stream())


class KRun:
    """One uniter_optim_step launch of kind 2 / 3 on fresh device copies of the inputs with every check that holds for every
    launch: the guards, the untouched chunks, the cleared gradients, the mirror, the second buffer of kind 3, and p / m / u against
    float64.  v: the Adamax state; kind 3: None = exp_avg_sq NULL, 'poison' = a buffer of NaN patterns."""

    def __init__(self, kind, p, g, m, v, flags, h, sumsq, wgs=0, zero=1, mirror=None, g16=False, check=True, launch=True):
        self.kind, self.n, self.h, self.flags_h, self.sumsq_h, self.zero, self.mirror_kind = kind, p.size, h, flags, sumsq, zero, mirror
        self.inp = dict(p=p, g=g, m=m, v=v if kind == K.KIND_ADAMAX else None)
        self.p, self.m = Buf(p), Buf(m)
        if kind == K.KIND_ADAMAX:
            self.v = Buf(v)
        else:
            self.v = None if v is None else Buf(A.POISON[np.arange(p.size) % 4].view(np.float32))
        self.g16 = None
        if g16:         # the payload holds g (rounded to bf16); the fp32 buffer holds something else
            gb = torch.as_tensor(g).to(torch.bfloat16)
            bits = gb.view(torch.int16).numpy().copy().view(np.uint16)
            skip = R.expand_flags(flags, p.size) == 0
            bits[skip] = A.POISON16[np.arange(p.size) % 4][skip]
            gb = torch.as_tensor(bits.view(np.int16)).view(torch.bfloat16)
            self.g16 = Buf(gb)
            self.inp['g'] = gb.float().numpy()
            self.g = Buf(np.where(np.arange(p.size) % 3 == 0, 0.0, 7.5).astype(np.float32))
        else:
            self.g = Buf(g)
        self.flags = Buf(flags)
        self.sumsq = None if sumsq is None else Buf(torch.tensor([sumsq], dtype=torch.float64), lead=1, tail=1)
        self.stride, self.mirror = 0, None
        if mirror == 'bf16':
            self.mirror = Buf(torch.full((self.n,), FILL[2], dtype=torch.int16))
        elif mirror == 'x3':
            self.stride = self.n + 192
            self.mirror = Buf(torch.full((2 * self.stride + self.n,), FILL[2], dtype=torch.int16))
        self.wgs = wgs
        if launch:
            A._L().check(self.launch(), 'uniter_optim_step (%d)' % kind)
            torch.cuda.synchronize()
            if check:
                self.check()
            else:
                assert all(b.guards_ok() for b in self.bufs()), 'guard region written'

    def launch(self, off=0, n=None, tab=None, first=0, wgs=None, **over):
        n = self.n - off if n is None else n
        a = dict(kind=self.kind, p=self.p.ptr(off), g=self.g.ptr(off), m=self.m.ptr(off), v=None if self.v is None else self.v.ptr(off),
                 flags=self.flags.ptr(off // 64), sumsq=None if self.sumsq is None else self.sumsq.ptr(),
                 g16=None if self.g16 is None else self.g16.ptr(off), mirror=None if self.mirror is None else self.mirror.ptr(),
                 ps=self.stride, h=self.h)
        a.update(over)
        return _optim_step(a['kind'], a['p'], a['g'], a['g16'], a['m'], a['v'], a['flags'], n, a['sumsq'], a['h'], self.zero,
                           a['mirror'], a['ps'], tab, first, self.wgs if wgs is None else wgs)

    def bufs(self):
        return [b for b in (self.p, self.g, self.m, self.v, self.flags, self.sumsq, self.g16, self.mirror) if b is not None]

    def out(self):
        return dict(p=self.p.bits(), g=self.g.bits(), m=self.m.bits(), v=None if self.v is None else self.v.bits(),
                    mirror=None if self.mirror is None else self.mirror.bits())

    def check(self, upd=None, perm=None):
        n, fl = self.n, R.expand_flags(self.flags_h, self.n)
        upd = (fl & 3) != 0 if upd is None else upd
        for b in self.bufs():
            assert b.guards_ok(), 'guard region written'
        assert self.flags.unchanged() and (self.sumsq is None or self.sumsq.unchanged()) and (self.g16 is None or self.g16.unchanged())
        keys = 'pmv' if self.kind == K.KIND_ADAMAX else 'pm'
        if self.kind == K.KIND_SGD and self.v is not None:
            assert self.v.unchanged(), 'kind 3 wrote the second state buffer'
        got = {k: getattr(self, k).np() for k in keys + 'g'}
        for k in keys:
            assert np.array_equal(A._u32(got[k])[~upd], A._u32(self.inp[k])[~upd]), k + ': a skipped chunk was written'
        g0 = A._u32(self.g.init[GUARD:GUARD + n].view(torch.float32).cpu().numpy())
        clear = upd & (self.zero != 0) & ((fl & 4) == 0)
        assert np.array_equal(A._u32(got['g'])[~clear], g0[~clear]), 'a gradient was changed that had to be left alone'
        assert not A._u32(got['g'])[clear].any(), 'a gradient was not cleared'
        with np.errstate(all='ignore'):
            ref = K.ref_step_kind(self.kind, self.inp['p'], self.inp['g'], self.inp['m'], self.inp['v'], self.flags_h, self.h, self.sumsq_h)
        self.ratio = {}
        for k in keys:
            assert np.isfinite(got[k][upd]).all(), k
            self.ratio[k] = R.worst_ratio(got[k][upd], ref[k][upd], ref['E_' + k][upd])
            WORST[NAME[self.kind, k]] = max(WORST[NAME[self.kind, k]], self.ratio[k])
        assert max(self.ratio.values()) <= 1.0, self.ratio
        if self.mirror is not None and perm is None:
            mb = self.mirror.bits()
            first = mb[:n]
            assert np.array_equal(first[upd], A._bf16_bits(got['p'])[upd]), 'mirror is not bf16(p)'
            assert (first[~upd] == FILL[2]).all(), 'mirror of a skipped chunk written'
            if self.mirror_kind == 'x3':
                s = self.stride
                assert (mb[n:s] == FILL[2]).all() and (mb[s + n:2 * s] == FILL[2]).all(), 'between the pieces'
                pieces = [torch.as_tensor(mb[k * s:k * s + n].copy()).view(torch.bfloat16).double().numpy() for k in range(3)]
                assert np.array_equal((pieces[0] + pieces[1] + pieces[2])[upd], got['p'].astype(np.float64)[upd]), 'x1 + x2 + x3 != p'
                for k in (1, 2):
                    assert (mb[k * s:k * s + n][~upd] == FILL[2]).all()
        return self


def _same(a, b, keys=('p', 'g', 'm', 'v', 'mirror')):
    oa, ob = a.out(), b.out()
    for k in keys:
        if oa[k] is None and ob[k] is None:
            continue
        assert np.array_equal(oa[k], ob[k]), k + ' differs'


def _inputs(kind, n, seed, **case):
    p, g, m, v, flags, h, sumsq = K.build_kind_case(kind, n, seed, **case)
    if kind == K.KIND_ADAMAX:
        p, g, m, v = A._poison(flags, p, g, m, v)
    else:
        p, g, m = A._poison(flags, p, g, m)
        v = 'poison' if seed % 2 else None            # every second case hands kind 3 a second buffer it must not touch
    return p, g, m, v, flags, h, sumsq


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rules against float64
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = (1, 2, 10, 1000, 100000)
GMAGS = (1e-8, 1e-3, 1.0, 1e4)
LRWD = ((3e-5, 1e-3), (1e-3, 1e-2), (1e-3, 0.0))


def _step_cases():
    """32 combinations per kind: every axis walks through all its values with its own period (every size of SIZES four times)"""
    out = []
    for i in range(32):
        lr, wd = LRWD[i % 3]
        c = dict(i=i, step=STEPS[i % 5], moments=R.MOMENTS[(i // 3) % 4], gmag=GMAGS[(i // 2) % 4], lr=lr, wd=wd,
                 clip=('off', 'active', 'tiny')[(i // 5) % 3], n=SIZES[(i * 3) % 8], grid=GRIDS[(i // 2) % 5])
        if i in (7, 30):
            c['b1'] = 0.0              # Adamax without a first moment; plain SGD
        out.append(c)
    return out


@pytest.mark.parametrize('case', A._ids(_step_cases()))
@pytest.mark.parametrize('rule', list(KINDS))
def test_step_matches_float64(rule, case):
    case = dict(case)
    n, grid, seed = case.pop('n'), case.pop('grid'), 100 + case.pop('i')
    inp = _inputs(KINDS[rule], n, seed, **case)
    KRun(KINDS[rule], *inp, wgs=A._wgs(grid, n), mirror=(None, 'bf16', 'x3')[seed % 3])


@pytest.mark.parametrize('clip', R.CLIPS)
@pytest.mark.parametrize('rule', list(KINDS))
def test_step_clip_modes_match_float64(rule, clip):
    """no clip at a norm far below max_norm, coef about 0.1, a norm of 1e-3 against max_norm 1e-4, max_norm = 0 with sumsq = NULL,
    and max_norm > 0 with all-zero gradients and sumsq = 0"""
    for n in (64 * 17, SIZES[6]):
        inp = _inputs(KINDS[rule], n, 7, step=3, clip=clip)
        r = KRun(KINDS[rule], *inp, wgs=3)
        assert (r.sumsq is None) == (clip == 'null')


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('rule', list(KINDS))
def test_step_does_not_depend_on_the_grid(rule, n):
    inp = _inputs(KINDS[rule], n, n % 977, step=2, clip='active')
    base = KRun(KINDS[rule], *inp, wgs=0, mirror='x3')
    for grid in GRIDS[1:]:
        _same(KRun(KINDS[rule], *inp, wgs=A._wgs(grid, n), mirror='x3', check=False), base)


@pytest.mark.parametrize('rule', list(KINDS))
def test_eight_steps_each_against_float64_from_the_previous_fp32_state(rule):
    """the kernel feeds its own state (SGD from a zero buffer: torch's first step, buf = g'); step k is checked against ONE
    float64 step from the kernel's fp32 state after step k - 1"""
    kind, n = KINDS[rule], 64 * 17 * 8
    p, g, m, v, flags, h, sumsq = _inputs(kind, n, 21, moments='zero', clip='active')
    for k in range(1, 9):
        r = KRun(kind, p, g, m, v, flags, h.replace(step=k), sumsq, wgs=(0, 1, 3)[k % 3])
        p, m = r.p.np(), r.m.np()
        if kind == K.KIND_ADAMAX:
            v = r.v.np()
        g = R.make_case(n, 21 + k, wd=h.wd, coef_hint=R.clip_coef(sumsq, h))[1]
        (g,) = A._poison(flags, g)
        sumsq = R.ref_sumsq(g, flags)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the exact contracts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g16', [False, True], ids=['g32', 'g16'])
@pytest.mark.parametrize('zero', [0, 1])
@pytest.mark.parametrize('n', [64, 64 * 17, SIZES[6]])
@pytest.mark.parametrize('rule', list(KINDS))
def test_skipped_chunks_and_gradient_clearing(rule, n, zero, g16):
    inp = _inputs(KINDS[rule], n, 31 + zero, step=2)
    r = KRun(KINDS[rule], *inp, g16=g16, zero=zero, wgs=1, mirror='bf16')
    fl = R.expand_flags(inp[4], n)
    assert set(inp[4][:5]) == {0, 1, 2, 5, 6} or n == 64
    if zero and g16:
        assert not r.g.np()[((fl & 3) != 0) & ((fl & 4) == 0)].any()
    if not zero:
        assert r.g.unchanged()


@pytest.mark.parametrize('n', [64 * 17, SIZES[6]])
@pytest.mark.parametrize('rule', list(KINDS))
def test_bf16_payload_equals_the_fp32_path_on_the_widened_values(rule, n):
    inp = list(_inputs(KINDS[rule], n, 51, clip='active'))
    r16 = KRun(KINDS[rule], *inp, g16=True, mirror='bf16', wgs=3)
    inp[1] = r16.inp['g']
    r32 = KRun(KINDS[rule], *inp, mirror='bf16', wgs=3)
    _same(r16, r32, keys=('p', 'm', 'v', 'mirror'))


def test_sgd_never_touches_a_second_buffer():
    """exp_avg_sq NULL and a poisoned buffer give the same bits; the buffer comes back as it went in (KRun.check)"""
    n = 64 * 17 * 8
    p, g, m, _, flags, h, sumsq = _inputs(K.KIND_SGD, n, 60, clip='active', step=4)
    null = KRun(K.KIND_SGD, p, g, m, None, flags, h, sumsq, mirror='x3')
    pois = KRun(K.KIND_SGD, p, g, m, 'poison', flags, h, sumsq, mirror='x3')
    assert null.v is None and pois.v is not None and pois.v.unchanged()
    _same(null, pois, keys=('p', 'g', 'm', 'mirror'))
    # beta2 and eps are ignored
    odd = KRun(K.KIND_SGD, p, g, m, None, flags, h, sumsq, mirror='x3', launch=False)
    A._L().check(odd.launch(h=h.replace(b2=0.5, eps=3.0)), 'uniter_optim_step')
    torch.cuda.synchronize()
    _same(null, odd, keys=('p', 'g', 'm', 'mirror'))


@pytest.mark.parametrize('rule', list(KINDS))
def test_zero_gradient_and_zero_state_leave_the_parameters_alone(rule):
    n = 64 * 17
    p, g, m, v, flags, h, sumsq = _inputs(KINDS[rule], n, 61, wd=0.0, moments='zero', clip='zero')
    r = KRun(KINDS[rule], p, g, m, v, flags, h, sumsq, mirror='bf16')
    assert r.p.unchanged() and r.g.unchanged()
    upd = R.expand_flags(flags, n) != 0
    assert not r.m.np()[upd].any()
    if rule == 'adamax':
        assert (r.v.np()[upd] == np.float32(h.eps)).all()        # u' = max(0, 0 + eps)


@pytest.mark.parametrize('wgs', [0, 1, 2])
@pytest.mark.parametrize('rule', list(KINDS))
def test_pair_table_permutes_the_mirror_and_nothing_else(rule, wgs):
    """the launch that walks the mirror's order (pair_src, first_element > 0) against the flat launch over the same range: p, g and the
    state bit-identical, the mirror the permutation the table describes"""
    kind = KINDS[rule]
    first, n, inp, tab, src = A._pair_case(wgs)
    p, g, m, v, flags, h, sumsq = inp
    v = K.adamax_state(np.where(np.isfinite(v), v, 1.0)) if kind == K.KIND_ADAMAX else None
    if kind == K.KIND_ADAMAX:
        (v,) = A._poison(flags, v)
    plain = KRun(kind, p, g, m, v, flags, h, sumsq, launch=False, mirror='x3', wgs=wgs)
    pair = KRun(kind, p, g, m, v, flags, h, sumsq, launch=False, mirror='x3', wgs=wgs)
    for r in (plain, pair):
        r.stride = n + 192
        r.mirror = Buf(torch.full((2 * r.stride + n,), FILL[2], dtype=torch.int16))
    t = Buf(torch.as_tensor(tab.reshape(-1)))
    A._L().check(plain.launch(off=first), 'optim_step')
    A._L().check(pair.launch(off=first, tab=t.ptr(), first=first), 'optim_step, paired')
    torch.cuda.synchronize()
    upd = (R.expand_flags(flags, first + n) & 3) != 0
    upd[:first] = False
    plain.check(upd=upd, perm=True)
    pair.check(upd=upd, perm=True)
    assert t.unchanged()
    _same(pair, plain, keys='pgmv')
    a, b, s = plain.mirror.bits(), pair.mirror.bits(), plain.stride
    for k in range(3):
        pk = a[k * s:k * s + n]
        assert np.array_equal(pk[upd[first:]], A._bf16_bits(plain.p.np()[first:])[upd[first:]]) or k
        assert np.array_equal(b[k * s:k * s + n], pk[src]), 'piece %d' % k
        assert (b[k * s + n:(k + 1) * s] == FILL[2]).all() or k == 2
    pieces = sum(torch.as_tensor(a[k * s:k * s + n].copy()).view(torch.bfloat16).double().numpy() for k in range(3))
    assert np.array_equal(pieces[upd[first:]], plain.p.np()[first:].astype(np.float64)[upd[first:]])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. kinds 0 / 1 and refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g16', [False, True], ids=['g32', 'g16'])
@pytest.mark.parametrize('kind', [0, 1])
def test_adam_kinds_are_uniter_adam_step_x3p_bit_for_bit(kind, g16):
    """kind decides; the adamw argument of uniter_optim_step is ignored for kinds 0 / 1 (passed as the opposite here)"""
    n = SIZES[6]
    inp = A._inputs(n, 41 + kind, adamw=kind, clip='active', step=4)
    ref = A.Run(*inp, entry='x3p', mirror='x3', g16=g16, wgs=3)
    new = A.Run(*inp, entry='x3p', mirror='x3', g16=g16, wgs=3, launch=False)
    h = new.h.replace(adamw=1 - kind)
    A._L().check(_optim_step(kind, new.p.ptr(), new.g.ptr(), None if new.g16 is None else new.g16.ptr(), new.m.ptr(), new.v.ptr(),
                             new.flags.ptr(), n, new.sumsq.ptr(), h, 1, new.mirror.ptr(), new.stride, None, 0, 3), 'uniter_optim_step')
    torch.cuda.synchronize()
    new.check()
    A._same(new, ref)


def test_refused_calls_touch_nothing():
    L = A._L()
    lib = L.lib()
    n = 64 * 6
    inp = _inputs(K.KIND_ADAMAX, n, 91, clip='active')
    r = KRun(K.KIND_ADAMAX, *inp, launch=False, g16=True, mirror='x3')
    tab = Buf(torch.full((2 * n // 64,), -1, dtype=torch.int32))
    refused = [
        ('kind -1', lambda: r.launch(kind=-1)),
        ('kind 4', lambda: r.launch(kind=4)),
        ('kind 1000', lambda: r.launch(kind=1000)),
        ('adamax without its second state', lambda: r.launch(v=None)),
        ('adam through kind 0 without its second state', lambda: r.launch(kind=0, v=None)),
        ('n % 64', lambda: r.launch(n=n - 4)),
        ('step 0', lambda: r.launch(h=r.h.replace(step=0))),
        ('clip without sumsq', lambda: r.launch(sumsq=None)),
        ('null p', lambda: r.launch(p=None)),
        ('null m, sgd', lambda: r.launch(kind=3, m=None)),
        ('null flags', lambda: r.launch(flags=None)),
        ('g16 alignment', lambda: r.launch(g16=r.g16.ptr(2))),
        ('piece stride % 4', lambda: r.launch(ps=r.stride + 2)),
        ('pair table with one bf16 copy', lambda: r.launch(tab=tab.ptr(), ps=0)),
        ('pair table, first % 64', lambda: r.launch(kind=3, tab=tab.ptr(), first=32)),
    ]
    for what, call in refused:
        rc = call()
        assert rc != 0, what
        with pytest.raises(L.UniterHipError):
            L.check(rc, what)
        assert lib.uniter_last_error(), what
    assert r.launch(kind=7) < 0 and b'kind' in bytes(lib.uniter_last_error())
    torch.cuda.synchronize()
    for b in r.bufs() + [tab]:
        assert b.unchanged()
    # the library is left in working order
    L.check(r.launch(), 'uniter_optim_step')
    torch.cuda.synchronize()
    r.check()
