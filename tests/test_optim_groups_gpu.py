"""uniter_optim_step_groups (csrc/optim.hip) through the C ABI, all four kinds: one launch whose chunks carry their parameter
group in bits 3-7 of the flag byte against ONE uniter_optim_step LAUNCH PER GROUP -- that group's scalars, the other groups' chunks
zeroed in the flags -- on the same inputs, bit for bit.  The per-group entry point is held to float64 bounds by
tests/test_optim_f64_gpu.py and tests/test_optim_kinds_gpu.py, so bit-identity needs no tolerance of its own.

37 chunks (2368 elements: an odd chunk count, the last thread iteration without a second item) on the default grid and on one
workgroup, and 165 chunks on one workgroup (every thread walks its loop more than once).  Three groups that differ in lr,
weight_decay, beta1, beta2 and eps, with boundaries every 9 chunks (a wave covers 4: the boundaries fall inside waves); skipped
chunks, the keep bit, and one chunk whose group index is >= n_groups.  Skipped chunks hold NaN / Inf patterns in every buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_kinds_ref as K
import optim_ref as R
import test_optim_f64_gpu as A

pytestmark = pytest.mark.gpu

Buf, FILL = A.Buf, A.FILL
GROUPS = (dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2), dict(lr=1e-2, b1=0.8, b2=0.95, eps=1e-6, wd=0.0),
          dict(lr=3e-5, b1=0.5, b2=0.9, eps=1e-7, wd=0.1))
OUT_OF_RANGE, PAIR0 = 20, 9          # the chunk that names group 3 of 3; the first chunk of the [4][64] paired tensor
SHAPES = [(37, 0), (37, 1), (165, 1)]          # (chunks, max_workgroups)
GSCALE, STEP = 0.125, 3


def _flags(nchunks):
    c = np.arange(nchunks)
    low = np.array([2, 1, 6, 0, 5], dtype=np.uint8)[(c * 3) % 5]
    group = ((c // 9) % 3).astype(np.uint8)
    low[PAIR0:PAIR0 + 4] = 6                     # one tensor: one group (chunks 9 .. 17 are group 1), one byte
    f = np.where(low == 0, 0, (group << 3) | low).astype(np.uint8)
    f[OUT_OF_RANGE] = (3 << 3) | 2
    return f


def _table(groups):
    L = A._L()
    return (L.OptimGroupC * len(groups))(*[L.OptimGroupC(g['lr'], g['b1'], g['b2'], g['eps'], g['wd']) for g in groups])


class Case:
    """fresh device copies of one set of inputs; launch_groups / launch_per_group run on them"""

    def __init__(self, kind, nchunks, flags, seed=11, mirror=None, g16=False, pair=False, n_groups=3):
        self.kind, self.n, self.flags_h, self.n_groups = kind, nchunks * 64, flags, n_groups
        n = self.n
        live = ((flags & 3) != 0) & ((flags >> 3) < n_groups)
        self.eff = np.where(live, flags, 0).astype(np.uint8)            # what the grouped launch may touch
        p, g, m, v = R.make_case(n, seed, coef_hint=GSCALE * 0.1)
        if kind == K.KIND_ADAMAX:
            v = K.adamax_state(v)
        p, g, m, v = A._poison(self.eff, p, g, m, v)
        self.sumsq_h = R.ref_sumsq(g, self.eff)
        self.max_norm = 0.1 * np.sqrt(self.sumsq_h) * GSCALE            # the clip coefficient is about 0.1
        self.p, self.m, self.v = Buf(p), Buf(m), (None if kind == K.KIND_SGD else Buf(v))
        self.g16 = None
        if g16:
            bits = torch.as_tensor(g).to(torch.bfloat16).view(torch.int16).numpy().copy().view(np.uint16)
            skip = R.expand_flags(self.eff, n) == 0
            bits[skip] = A.POISON16[np.arange(n) % 4][skip]
            self.g16 = Buf(torch.as_tensor(bits.view(np.int16)).view(torch.bfloat16))
            self.g = Buf(np.where(np.arange(n) % 3 == 0, 0.0, 7.5).astype(np.float32))
        else:
            self.g = Buf(g)
        self.sumsq = Buf(torch.tensor([self.sumsq_h], dtype=torch.float64), lead=1, tail=1)
        self.stride, self.mirror = 0, None
        if mirror == 'bf16':
            self.mirror = Buf(torch.full((n,), FILL[2], dtype=torch.int16))
        elif mirror == 'x3':
            self.stride = n + 192
            self.mirror = Buf(torch.full((2 * self.stride + n,), FILL[2], dtype=torch.int16))
        self.tab = None
        if pair:        # a [4][64] tensor at chunk PAIR0: mirror chunk d holds unit d % 2 of rows 2 (d // 2) and 2 (d // 2) + 1
            tab = np.full((nchunks, 2), -1, dtype=np.int32)
            d = np.arange(4)
            tab[PAIR0:PAIR0 + 4, 0] = PAIR0 * 64 + 2 * (d // 2) * 64 + 32 * (d % 2)
            tab[PAIR0:PAIR0 + 4, 1] = tab[PAIR0:PAIR0 + 4, 0] + 64
            self.tab = Buf(torch.as_tensor(tab.reshape(-1)))

    def _common(self, flags_buf):
        return (self.p.ptr(), self.g.ptr(), None if self.g16 is None else self.g16.ptr(), self.m.ptr(),
                None if self.v is None else self.v.ptr(), flags_buf.ptr(), self.n, self.sumsq.ptr(), GSCALE, float(self.max_norm))

    def _tail(self, wgs):
        return (None if self.mirror is None else self.mirror.ptr(), self.stride, None if self.tab is None else self.tab.ptr(), 0, wgs,
                A._L().cur_stream())

    def launch_groups(self, wgs, groups=GROUPS, n_groups=None):
        self.flags = Buf(self.flags_h)
        table = _table(groups)
        return A._L().lib().uniter_optim_step_groups(self.kind, *self._common(self.flags), C.cast(table, C.c_void_p),
                                                     self.n_groups if n_groups is None else n_groups, STEP, 1, *self._tail(wgs))

    def launch_per_group(self, wgs, groups=GROUPS):
        L = A._L()
        self.flag_bufs = []
        for k, gr in enumerate(groups[:self.n_groups]):
            own = np.where((self.eff >> 3) == k, self.eff & 7, 0).astype(np.uint8)
            fb = Buf(own)
            self.flag_bufs.append(fb)
            h = R.Hyper(lr=gr['lr'], b1=gr['b1'], b2=gr['b2'], eps=gr['eps'], wd=gr['wd'], step=STEP, adamw=0)
            L.check(L.lib().uniter_optim_step(self.kind, *self._common(fb), h.lr, h.b1, h.b2, h.eps, h.wd, STEP, 0, 1,
                                              *self._tail(wgs)), 'uniter_optim_step, group %d' % k)

    def bufs(self):
        return dict(p=self.p, g=self.g, m=self.m, v=self.v, mirror=self.mirror, g16=self.g16, sumsq=self.sumsq, tab=self.tab)

    def out(self):
        return {k: None if b is None else b.full.cpu().numpy() for k, b in self.bufs().items()}


def _pair(kind, nchunks, flags, wgs, **kw):
    a, b = Case(kind, nchunks, flags, **kw), Case(kind, nchunks, flags, **kw)
    A._L().check(a.launch_groups(wgs), 'uniter_optim_step_groups')
    b.launch_per_group(wgs)
    torch.cuda.synchronize()
    return a, b


def _assert_same(a, b):
    oa, ob = a.out(), b.out()
    for k in oa:
        assert (oa[k] is None) == (ob[k] is None)
        if oa[k] is not None:
            assert np.array_equal(oa[k], ob[k]), k + ' differs (guards included)'


def _assert_skipped_untouched(c):
    """(c) the 0 chunks and the out-of-range chunk: every buffer as it went in"""
    skip = R.expand_flags(c.eff, c.n) == 0
    assert skip[OUT_OF_RANGE * 64] and skip.sum() > 64
    for k in ('p', 'g', 'm', 'v'):
        b = getattr(c, k)
        if b is not None:
            assert np.array_equal(b.bits()[skip], b.init[b.lead:b.lead + b.n].cpu().numpy()[skip]), k
            assert b.guards_ok()
    if c.mirror is not None:
        mb = c.mirror.bits()
        for piece in range(3 if c.stride else 1):
            assert (mb[piece * c.stride:piece * c.stride + c.n][skip] == FILL[2]).all()
        assert c.mirror.guards_ok()
    assert c.flags.unchanged() and c.sumsq.unchanged() and (c.g16 is None or c.g16.unchanged())


VARIANTS = {'plain': dict(), 'mirror1': dict(mirror='bf16'), 'mirror3': dict(mirror='x3'), 'paired': dict(mirror='x3', pair=True),
            'g16': dict(g16=True, mirror='bf16')}


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('nchunks, wgs', SHAPES)
@pytest.mark.parametrize('kind', [0, 1, 2, 3])
def test_grouped_launch_is_one_launch_per_group_bit_for_bit(kind, nchunks, wgs, variant):
    """(a), (c), (d)"""
    flags = _flags(nchunks)
    lows, groups = set((flags & 7).tolist()), set((flags >> 3).tolist())
    assert lows == {0, 1, 2, 5, 6} and groups == {0, 1, 2, 3}
    a, b = _pair(kind, nchunks, flags, wgs, **VARIANTS[variant])
    _assert_same(a, b)
    _assert_skipped_untouched(a)
    upd = R.expand_flags(a.eff, a.n) != 0
    assert (a.p.bits()[upd] != a.p.init[a.p.lead:a.p.lead + a.n].cpu().numpy()[upd]).mean() > 0.9          # and the step did step
    assert np.isfinite(a.p.np()[upd]).all()
    clear = upd & ((R.expand_flags(a.eff, a.n) & 4) == 0)
    assert not a.g.bits()[clear].any() and a.g.bits()[upd & ~clear].any()


@pytest.mark.parametrize('nchunks, wgs', SHAPES)
@pytest.mark.parametrize('kind', [0, 1, 2, 3])
def test_one_group_with_todays_bytes_is_uniter_optim_step(kind, nchunks, wgs):
    """(b)"""
    flags = R.make_flags(nchunks, 5)
    flags[OUT_OF_RANGE] = 0
    assert set(flags.tolist()) == {0, 1, 2, 5, 6}
    a, b = _pair(kind, nchunks, flags, wgs, mirror='x3', n_groups=1)
    _assert_same(a, b)
    _assert_skipped_untouched(a)


def test_the_groups_really_differ():
    """the same launch with the groups' rows swapped gives other parameters: the table is read per chunk"""
    flags = _flags(37)
    a, b = Case(0, 37, flags), Case(0, 37, flags)
    A._L().check(a.launch_groups(0), 'groups')
    A._L().check(b.launch_groups(0, groups=GROUPS[::-1]), 'groups')
    torch.cuda.synchronize()
    for k in range(3):
        own = R.expand_flags(np.where((a.eff >> 3) == k, a.eff, 0), a.n) != 0
        assert (a.p.bits()[own] != b.p.bits()[own]).any() == (k != 1)


@pytest.mark.parametrize('n_groups', [0, 33, -1])
def test_group_counts_outside_1_to_32_are_refused(n_groups):
    """(e)"""
    L = A._L()
    c = Case(1, 37, _flags(37), mirror='x3')
    rc = c.launch_groups(0, n_groups=n_groups)
    assert rc != 0 and b'n_groups' in bytes(L.lib().uniter_last_error())
    with pytest.raises(L.UniterHipError):
        L.check(rc, 'uniter_optim_step_groups')
    c.kind = 4
    assert c.launch_groups(0) != 0 and b'kind' in bytes(L.lib().uniter_last_error())
    torch.cuda.synchronize()
    for b in list(c.bufs().values()) + [c.flags]:
        assert b is None or b.unchanged()
    c.kind = 1                                   # the library is left in working order, and 32 groups are accepted
    L.check(c.launch_groups(0, groups=GROUPS + (GROUPS[0],) * 29, n_groups=32), 'uniter_optim_step_groups')
    torch.cuda.synchronize()
    assert not c.p.unchanged() and c.p.guards_ok()
