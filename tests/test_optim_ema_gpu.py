"""uniter_optim_step_avg / uniter_optim_step_groups_avg (csrc/optim.hip, adam_kernel<RULE, GROUPED, AVG>) through the C ABI: the
fused step that also keeps an exponential moving average of the parameters, against the entry points without the average and
against the float64 reference and bound of tests/optim_ema_ref.py (derivation there; tests/test_optim_ema_bounds_cpu.py is the
standing proof that an fp32 evaluation of the contract keeps it to half and that wrong forms leave it).

The harness is that of tests/test_optim_groups_gpu.py (its Case: every buffer between guard chunks of NaN patterns, NaN / Inf in
every chunk off the update path) with one more buffer, the average, built by optim_ema_ref.make_avg around the parameters.
Sizes 64, 64 x 17 and 64 x 37 elements (592 items: on one workgroup the second round, on two the first, leaves threads with a
single item); grids 0 (default), 1 and 2 workgroups; kinds 0 - 3; the grouped form with three groups and one chunk that names a
fourth; flag bytes 0, 1, 2, 5, 6; fp32 gradients and the bf16 payload; no mirror, one bf16 copy, the three pieces; a pair table
over the [4][64] tensor at chunk 9 next to unpaired neighbours.

Asserted per case: p, g, m, v and the mirror bit-identical (guards included) to the entry point without the average on the same
inputs; a' within the bound of the float64 reference taken from the kernel's OWN fp32 p' on the update path; the average
elsewhere -- skipped chunks, the out-of-table group, the guards -- untouched bit for bit; the same bits on every grid.  Then eight
steps with the warm-up sequence, each against the reference from the previous fp32 state, and refused calls that write nothing.

The worst error / bound ratio is printed at the end of the module (-s shows it).  Recorded on an MI355X: 0.126; 41 tests in 3 s."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import optim_ema_ref as E
import optim_ref as R
import test_optim_f64_gpu as A
import test_optim_groups_gpu as G

pytestmark = pytest.mark.gpu

Buf = A.Buf
GRIDS = (0, 1, 2)
WORST = {'a': 0.0}
H0 = G.GROUPS[0]


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nuniter_optim_step_avg, worst |a\' - float64| / bound: %.3f' % WORST['a'])


def _plain_flags(nchunks):
    """0, 1, 2, 5, 6 in runs of one (the grouped test's bytes without their group bits)"""
    return (np.array([2, 1, 6, 0, 5], dtype=np.uint8)[(np.arange(nchunks) * 3) % 5]).astype(np.uint8)


class ECase(G.Case):
    """test_optim_groups_gpu.Case with the average; launch() is any of the four entry points on the case's buffers"""

    def __init__(self, kind, nchunks, flags, seed=11, **kw):
        super().__init__(kind, nchunks, flags, seed=seed, **kw)
        p = self.p.np()
        a = E.make_avg(np.where(np.isfinite(p), p, 1.0), seed + 5)
        (a,) = A._poison(self.eff, a)
        self.a_h, self.a = a, Buf(a)
        self.upd = (R.expand_flags(self.eff, self.n) & 3) != 0
        self.flags = Buf(self.flags_h)

    def launch(self, grouped, avg, wgs, w=0.1, step=G.STEP, zero=1, **over):
        L = A._L()
        lib = L.lib()
        a = dict(kind=self.kind, avg_ptr=self.a.ptr(), n_groups=self.n_groups)
        a.update(over)
        tail = self._tail(wgs)
        more = (a['avg_ptr'], w) if avg else ()
        common = (a['kind'],) + self._common(self.flags)
        if grouped:
            table = G._table(G.GROUPS)
            fn = lib.uniter_optim_step_groups_avg if avg else lib.uniter_optim_step_groups
            return fn(*common, C.cast(table, C.c_void_p), a['n_groups'], step, zero, *tail[:-2], *more, *tail[-2:])
        h = R.Hyper(lr=H0['lr'], b1=H0['b1'], b2=H0['b2'], eps=H0['eps'], wd=H0['wd'])
        fn = lib.uniter_optim_step_avg if avg else lib.uniter_optim_step
        return fn(*common, h.lr, h.b1, h.b2, h.eps, h.wd, step, 0, zero, *tail[:-2], *more, *tail[-2:])

    def bufs(self):
        return dict(super().bufs(), a=self.a, flags=self.flags)

    def check_avg(self, w, a_before=None):
        """a' against float64 from the kernel's own p' on the update path; everything else of the buffer as it went in"""
        a0 = self.a_h if a_before is None else a_before
        got, p1 = self.a.np(), self.p.np()
        assert self.a.guards_ok(), 'guard region of avg written'
        assert np.array_equal(A._u32(got)[~self.upd], A._u32(a0)[~self.upd]), 'avg of a skipped chunk written'
        assert np.isfinite(got[self.upd]).all() and np.isfinite(p1[self.upd]).all()
        ref = E.ref_avg(a0, p1, R.f32(w), self.upd)
        ratio = R.worst_ratio(got[self.upd], ref['a'][self.upd], ref['E_a'][self.upd])
        WORST['a'] = max(WORST['a'], ratio)
        assert ratio <= 1.0, ratio
        return ratio


def _same_but_avg(a, b):
    oa, ob = a.out(), b.out()
    for k in ('p', 'g', 'm', 'v', 'mirror', 'g16', 'sumsq', 'tab', 'flags'):
        assert (oa[k] is None) == (ob[k] is None), k
        if oa[k] is not None:
            assert np.array_equal(oa[k], ob[k]), k + ' differs from the entry point without the average (guards included)'


# (chunks, grouped, mirror, bf16 payload, pair table): every kind runs every row on every grid
SHAPES = [(1, False, None, False, False), (17, False, 'bf16', True, False), (17, False, 'x3', False, False),
          (37, False, None, True, False), (37, False, 'x3', False, True), (37, True, 'x3', True, True), (37, True, 'bf16', False, False),
          (37, True, None, False, False)]
WEIGHTS = (0.9, 0.1, 1e-3)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dchunks-%s-%s-%s%s' % (s[0], 'grouped' if s[1] else 'flat', s[2] or 'nomirror',
                                                                                   'g16' if s[3] else 'g32', '-pair' if s[4] else ''))
@pytest.mark.parametrize('kind', [0, 1, 2, 3], ids=['adam', 'adamw', 'adamax', 'sgd'])
def test_avg_entry_point(kind, shape):
    nchunks, grouped, mirror, g16, pair = shape
    flags = G._flags(nchunks) if grouped else _plain_flags(nchunks)
    if pair and not grouped:
        flags[G.PAIR0:G.PAIR0 + 4] = 6              # one tensor, one byte
    if nchunks >= 5:
        assert set(flags[:5] & 7) == {0, 1, 2, 5, 6}
    w = WEIGHTS[(kind + nchunks) % 3]
    kw = dict(seed=11 + kind + nchunks, mirror=mirror, g16=g16, pair=pair)
    first = None
    for wgs in GRIDS:
        base, avg = ECase(kind, nchunks, flags, **kw), ECase(kind, nchunks, flags, **kw)
        A._L().check(base.launch(grouped, False, wgs), 'the entry point without the average')
        A._L().check(avg.launch(grouped, True, wgs, w=w), 'the _avg entry point')
        torch.cuda.synchronize()
        _same_but_avg(avg, base)                    # 1. everything but the average: bit-identical
        assert base.a.unchanged()
        avg.check_avg(w)                            # 2. + 3. the average: the bound on the update path, untouched elsewhere
        if grouped:
            skip = R.expand_flags(avg.eff, avg.n) == 0
            assert skip[G.OUT_OF_RANGE * 64] and np.array_equal(A._u32(avg.a.np())[skip], A._u32(avg.a_h)[skip])
        out = avg.out()
        if first is None:
            first = out
        else:                                       # 4. the grid changes nothing
            for k, v in out.items():
                assert v is None or np.array_equal(v, first[k]), '%s depends on the grid (%d workgroups)' % (k, wgs)
    if pair:        # the average is indexed like p, whatever order the mirror is walked in
        flat = ECase(kind, nchunks, flags, **dict(kw, pair=False))
        A._L().check(flat.launch(grouped, True, 1, w=w), 'the _avg entry point, no pair table')
        torch.cuda.synchronize()
        assert np.array_equal(flat.out()['a'], first['a']) and np.array_equal(flat.out()['p'], first['p'])
        assert not np.array_equal(flat.out()['mirror'], first['mirror'])


@pytest.mark.parametrize('kind', [0, 3])
def test_weight_zero_leaves_the_average_and_one_copies_the_parameters_within_the_bound(kind):
    flags = _plain_flags(17)
    c = ECase(kind, 17, flags)
    A._L().check(c.launch(False, True, 0, w=0.0), 'w = 0')
    torch.cuda.synchronize()
    assert c.a.unchanged()
    A._L().check(c.launch(False, True, 0, w=1.0), 'w = 1')
    torch.cuda.synchronize()
    c.check_avg(1.0)


@pytest.mark.parametrize('grouped', [False, True], ids=['flat', 'grouped'])
@pytest.mark.parametrize('kind', [1, 2, 3], ids=['adamw', 'adamax', 'sgd'])
def test_eight_steps_with_the_warmup_sequence_each_against_the_previous_fp32_state(kind, grouped):
    """the kernel feeds its own p, moments and average (gradients kept: zero_grads = 0); step k is checked against ONE float64
    averaging step from the kernel's fp32 average after step k - 1 and its fp32 p' of step k"""
    flags = G._flags(37) if grouped else _plain_flags(37)
    c = ECase(kind, 37, flags, seed=23, mirror='x3')
    g0 = c.g.bits()
    before = c.a_h
    for k in range(1, 9):
        w = E.ref_weight(0.999, k - 1)
        assert w == R.f32(1.0 - min(0.999, k / (9.0 + k)))
        A._L().check(c.launch(grouped, True, GRIDS[k % 3], w=w, step=k, zero=0), 'step %d' % k)
        torch.cuda.synchronize()
        c.check_avg(w, a_before=before)
        before = c.a.np()
        assert np.array_equal(c.g.bits(), g0)
    moved = np.abs(before[c.upd].astype(np.float64) - c.a_h[c.upd])
    assert np.median(moved / np.abs(c.a_h[c.upd])) > 0.1             # eight warm-up steps carry the average most of the way to p


def test_refused_calls_write_nothing():
    L = A._L()
    lib = L.lib()
    flags = G._flags(37)
    c = ECase(1, 37, flags, mirror='x3', g16=True, pair=True)
    refused = [
        ('avg NULL', lambda g: c.launch(g, True, 0, avg_ptr=None)),
        ('weight below 0', lambda g: c.launch(g, True, 0, w=-1e-3)),
        ('weight above 1', lambda g: c.launch(g, True, 0, w=1.0 + 1e-6)),
        ('weight NaN', lambda g: c.launch(g, True, 0, w=math.nan)),
        ('weight Inf', lambda g: c.launch(g, True, 0, w=math.inf)),
        ('kind -1', lambda g: c.launch(g, True, 0, kind=-1)),
        ('kind 4', lambda g: c.launch(g, True, 0, kind=4)),
    ]
    for grouped in (False, True):
        for what, call in refused:
            rc = call(grouped)
            assert rc == -1, (what, grouped, rc)                      # UNITER_E_ARG
            with pytest.raises(L.UniterHipError):
                L.check(rc, what)
            assert lib.uniter_last_error(), what
    assert c.launch(True, True, 0, n_groups=0) == -1 and c.launch(True, True, 0, n_groups=33) == -1
    assert c.launch(False, True, 0, step=0) != 0 and c.launch(True, True, 0, step=0) != 0
    assert c.launch(False, True, 0, avg_ptr=c.a.ptr(1)) != 0            # not 16-byte aligned
    torch.cuda.synchronize()
    for k, b in c.bufs().items():
        assert b is None or b.unchanged(), k
    # the library is left in working order
    L.check(c.launch(True, True, 0, w=0.5), 'uniter_optim_step_groups_avg')
    torch.cuda.synchronize()
    c.check_avg(0.5)
