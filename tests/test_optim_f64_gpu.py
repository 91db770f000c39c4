"""The clip-norm and optimizer-step kernels of csrc/optim.hip through the C ABI, against the float64 reference and the per-element
bounds of tests/optim_ref.py (derivation there; tests/test_optim_bounds_cpu.py is the standing proof that an fp32 evaluation of the
contract keeps them), and against each other bit for bit where the contract is exact.

Every buffer handed to a call sits between guard chunks of 64 elements that hold a recognisable NaN pattern; chunks whose flag is
0 hold NaN / Inf patterns in every buffer and must come back bit-identical.  The sum of squares the step consumes is the float64
reference written to the device (one case chains the norm kernel into the step instead), so an error of the norm kernels can
neither mask nor fake one of the step.  The inputs hold no fp32 subnormals (optim_ref.make_case).

The worst error / bound ratios per quantity are collected in WORST and printed at the end of the module (-s shows them).
Recorded on an MI355X: p 0.156, m 0.245, v 0.442, the norm 0.004, the combine 0.005; 160 tests in 18 s."""
import math

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = {1: 0xA5, 2: 0x7fc1, 4: 0x7fc0beef, 8: 0x7ff8dead0000beef}          # guard patterns (NaN as bf16 / fp32 / double)
INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
POISON = np.array([0x7fc00123, 0x7f800000, 0xff800000, 0xffc0abcd], dtype=np.uint32)      # NaN, +Inf, -Inf, NaN
POISON16 = np.array([0x7fc1, 0x7f80, 0xff80, 0xffc3], dtype=np.uint16)
SIZES = (64, 128, 64 * 15, 64 * 16, 64 * 17, 256 * 4 * 2, 2048 * 256 * 4 + 64 * 3, 2 * 2048 * 256 * 4 + 64 * 5)
WORST = dict(p=0.0, m=0.0, v=0.0, sumsq=0.0, combine=0.0)


def _L():
    from meme_challenge_amd import _lib
    return _lib


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\noptimizer kernels, worst |got - float64| / bound: ' + ', '.join('%s %.3f' % kv for kv in WORST.items()))


def _ids(cases):
    return [pytest.param(c, id='-'.join('%s=%s' % kv for kv in c.items())) for c in cases]


class Buf:
    """a device buffer between two guard regions; compared as bit patterns (integer views)"""

    def __init__(self, host, lead=GUARD, tail=GUARD):
        host = torch.as_tensor(host)
        self.es, self.dtype, self.n, self.lead = host.element_size(), host.dtype, host.numel(), lead
        it = INT[self.es]
        full = torch.full((lead + self.n + tail,), FILL[self.es], dtype=it)
        full[lead:lead + self.n] = host.contiguous().view(it)
        self.full = full.cuda()
        self.init = self.full.clone()

    def ptr(self, off=0):
        return self.full.data_ptr() + (self.lead + off) * self.es

    def bits(self):
        return self.full[self.lead:self.lead + self.n].cpu().numpy()

    def np(self):
        return self.full[self.lead:self.lead + self.n].view(self.dtype).cpu().numpy() if self.dtype != torch.bfloat16 else None

    def torch(self):
        return self.full[self.lead:self.lead + self.n].view(self.dtype).cpu()

    def set(self, host):
        self.full[self.lead:self.lead + self.n] = torch.as_tensor(host).contiguous().view(INT[self.es]).cuda()

    def guards_ok(self):
        e = self.lead + self.n
        return torch.equal(self.full[:self.lead], self.init[:self.lead]) and torch.equal(self.full[e:], self.init[e:])

    def unchanged(self):
        return torch.equal(self.full, self.init)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _poison(flags, *arrays):
    """copies of the fp32 arrays with NaN / Inf patterns in every chunk whose flag is 0"""
    skip = R.expand_flags(flags, arrays[0].size) == 0
    out = []
    for k, a in enumerate(arrays):
        b = _u32(a).copy()
        b[skip] = POISON[(np.arange(b.size) + k) % 4][skip]
        out.append(b.view(np.float32))
    return out


def _bf16_bits(x):
    """round-to-nearest-even bf16 of fp32 values (torch on the host), as int16 bit patterns"""
    return torch.as_tensor(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy()


class Run:
    """One launch of a step entry point on fresh device copies of the inputs, with every check that holds for every launch: the
    guards, the untouched chunks, the cleared gradients, the mirror, and p / m / v against float64.  The results stay on the object
    for bit-for-bit comparisons between launches."""

    def __init__(self, p, g, m, v, flags, h, sumsq, entry='ex', wgs=0, zero=1, mirror=None, g16=False, check=True, launch=True,
                 gjunk=None):
        self.n, self.h, self.flags_h, self.sumsq_h, self.zero, self.mirror_kind = p.size, h, flags, sumsq, zero, mirror
        self.inp = dict(p=p, g=g, m=m, v=v)
        self.p, self.m, self.v = Buf(p), Buf(m), Buf(v)
        self.g16 = None
        if g16:         # the payload holds g (rounded to bf16); the fp32 buffer holds something else
            gb = torch.as_tensor(g).to(torch.bfloat16)
            bits = gb.view(torch.int16).numpy().copy().view(np.uint16)
            skip = R.expand_flags(flags, p.size) == 0
            bits[skip] = POISON16[np.arange(p.size) % 4][skip]
            gb = torch.as_tensor(bits.view(np.int16)).view(torch.bfloat16)
            self.g16 = Buf(gb)
            self.inp['g'] = gb.float().numpy()
            self.g = Buf(gjunk if gjunk is not None else np.where(np.arange(p.size) % 3 == 0, 0.0, 7.5).astype(np.float32))
        else:
            self.g = Buf(g)
        self.flags = Buf(flags)
        self.sumsq = None if sumsq is None else Buf(torch.tensor([sumsq], dtype=torch.float64), lead=1, tail=1)
        self.stride = 0
        self.mirror = None
        if mirror == 'bf16':
            self.mirror = Buf(torch.full((self.n,), FILL[2], dtype=torch.int16))
        elif mirror == 'x3':
            self.stride = self.n + 192                  # pieces further apart than n: a guard between them
            self.mirror = Buf(torch.full((2 * self.stride + self.n,), FILL[2], dtype=torch.int16))
        self.entry, self.wgs = entry, wgs
        if launch:
            _L().check(self.launch(), 'uniter_adam_step (%s)' % entry)
            torch.cuda.synchronize()
            if check:
                self.check()
            else:
                assert all(b.guards_ok() for b in self.bufs()), 'guard region written'

    def launch(self, entry=None, off=0, n=None, tab=None, first=0, rowmask=None, row_len=0, touched=0, wgs=None, **over):
        """off: the launch starts `off` elements into the buffers.  over: arguments replaced for the refusal tests."""
        L = _L()
        lib, cs = L.lib(), L.cur_stream()
        entry, wgs = entry or self.entry, self.wgs if wgs is None else wgs
        n = self.n - off if n is None else n
        a = dict(p=self.p.ptr(off), g=self.g.ptr(off), m=self.m.ptr(off), v=self.v.ptr(off), flags=self.flags.ptr(off // 64),
                 sumsq=None if self.sumsq is None else self.sumsq.ptr(), g16=None if self.g16 is None else self.g16.ptr(off),
                 mirror=None if self.mirror is None else self.mirror.ptr(), ps=self.stride, h=self.h)
        a.update(over)
        common = (a['flags'], n, a['sumsq']) + a['h'].c_args() + (self.zero,)
        pgmv = (a['p'], a['g'], a['m'], a['v'])
        pg16 = (a['p'], a['g'], a['g16'], a['m'], a['v'])
        if entry == 'step':
            return lib.uniter_adam_step(*pgmv, *common, cs)
        if entry == 'mirror':
            return lib.uniter_adam_step_mirror(*pgmv, *common, a['mirror'], cs)
        if entry == 'ex':
            return lib.uniter_adam_step_ex(*pgmv, *common, a['mirror'], wgs, cs)
        if entry == 'g16':
            return lib.uniter_adam_step_g16(*pg16, *common, a['mirror'], wgs, cs)
        if entry == 'x3':
            return lib.uniter_adam_step_x3(*pg16, *common, a['mirror'], a['ps'], wgs, cs)
        if entry == 'x3p':
            return lib.uniter_adam_step_x3p(*pg16, *common, a['mirror'], a['ps'], tab, first, wgs, cs)
        if entry == 'rows':
            return lib.uniter_adam_step_rows(*pgmv, *common, rowmask, row_len, touched, wgs, cs)
        raise ValueError(entry)

    def bufs(self):
        return [b for b in (self.p, self.g, self.m, self.v, self.flags, self.sumsq, self.g16, self.mirror) if b is not None]

    def out(self):
        return dict(p=self.p.bits(), g=self.g.bits(), m=self.m.bits(), v=self.v.bits(),
                    mirror=None if self.mirror is None else self.mirror.bits())

    def check(self, upd=None, g_read=True, perm=None):
        """upd: per-element mask of what this launch had to update (default: every chunk whose flag & 3 is not 0)"""
        n, fl = self.n, R.expand_flags(self.flags_h, self.n)
        upd = (fl & 3) != 0 if upd is None else upd
        for b in self.bufs():
            assert b.guards_ok(), 'guard region written'
        assert self.flags.unchanged() and (self.sumsq is None or self.sumsq.unchanged()) and (self.g16 is None or self.g16.unchanged())
        got = {k: getattr(self, k).np() for k in 'pgmv'}
        # chunks that are not this launch's: bit-identical in every buffer
        for k in 'pmv':
            assert np.array_equal(_u32(got[k])[~upd], _u32(self.inp[k])[~upd]), k + ': a skipped chunk was written'
        g0 = _u32(self.g.init[GUARD:GUARD + n].view(torch.float32).cpu().numpy())
        clear = upd & (self.zero != 0) & ((fl & 4) == 0) & g_read
        assert np.array_equal(_u32(got['g'])[~clear], g0[~clear]), 'a gradient was changed that had to be left alone'
        assert not _u32(got['g'])[clear].any(), 'a gradient was not cleared'
        # p, m, v against float64
        with np.errstate(all='ignore'):
            ref = R.ref_step(self.inp['p'], self.inp['g'] if g_read else np.zeros(n, np.float32), self.inp['m'], self.inp['v'],
                             self.flags_h, self.h, self.sumsq_h if g_read else None)
        self.ratio = {}
        for k in 'pmv':
            assert np.isfinite(got[k][upd]).all(), k
            self.ratio[k] = R.worst_ratio(got[k][upd], ref[k][upd], ref['E_' + k][upd])
            WORST[k] = max(WORST[k], self.ratio[k])
        assert max(self.ratio.values()) <= 1.0, self.ratio
        # the mirror: bf16 (round to nearest even) of the new p, or its exact three-piece split; untouched where p is
        if self.mirror is not None and perm is None:
            mb = self.mirror.bits()
            first = mb[:n]
            assert np.array_equal(first[upd], _bf16_bits(got['p'])[upd]), 'mirror is not bf16(p)'
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


def _full_grid(n):
    return (n // 4 + 511) // 512


def _wgs(kind, n):
    return {'default': 0, 'one': 1, 'three': 3, 'full': _full_grid(n), 'over': _full_grid(n) + 5}[kind]


def _inputs(n, seed, **case):
    p, g, m, v, flags, h, sumsq = R.build_case(n, seed, **case)
    p, g, m, v = _poison(flags, p, g, m, v)
    return p, g, m, v, flags, h, sumsq


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the clip norm
# ---------------------------------------------------------------------------------------------------------------------------
def _spiked(n, stride_items, seed, flags_wanted=True, bf16=False):
    """n values (|x| in 0.01 .. 4, variance about 1) with spikes of 100 .. 137.5 on the first and last 16-byte item, the items on either side
    of every multiple of the launched grid's stride, and one in the middle; flags in runs of 1 (non-zero where a spike sits), NaN /
    Inf in the chunks whose flag is 0.  -> values (float32, or bf16 tensor), flags or None, float64 reference"""
    r = np.random.default_rng(seed)
    x = r.standard_normal(n)
    x = np.clip(np.where(np.abs(x) < 0.01, 0.01, x), -4, 4).astype(np.float32)
    n4 = n // 4
    items = {0, n4 - 1, n4 // 2}
    for b in range(stride_items, n4, stride_items):
        items |= {b - 1, b}
    items = np.array(sorted(items))
    for e in range(4):
        x[items * 4 + e] = np.copysign(100.0 + 12.5 * e, x[items * 4 + e])
    if bf16:
        x = torch.as_tensor(x).to(torch.bfloat16).float().numpy()
    flags = None
    if flags_wanted:
        flags = R.make_flags((n + 63) // 64, seed)
        hit = np.unique(items * 4 // 64)
        flags[hit] = np.where(flags[hit] == 0, 6, flags[hit])
        (x,) = _poison(flags, x)
    ref = R.ref_sumsq(x, flags)
    share = min(float(np.sum(x[i * 4:i * 4 + 4].astype(np.float64) ** 2)) for i in items) / ref
    assert share >= 1e-3 or n4 <= 3, share              # one dropped or doubled spike moves the sum by 5000 bounds
    if bf16:
        bits = (_u32(x) >> 16).astype(np.uint16)        # (exact: the values are bf16 numbers, the poison patterns keep their class)
        x = torch.as_tensor(bits.view(np.int16)).view(torch.bfloat16)
    return x, flags, ref


def _sumsq_close(got, ref, what):
    assert math.isfinite(got), what
    ratio = abs(got - ref) / (R.SUMSQ_REL * ref)
    WORST['sumsq'] = max(WORST['sumsq'], ratio)
    assert ratio <= 1.0, (what, got, ref, ratio)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('n', SIZES)
def test_grad_sumsq_matches_float64(n, bf16):
    L = _L()
    lib, cs = L.lib(), L.cur_stream()
    nb = min(2048, max(1, (n // 4 + 255) // 256))
    x, flags, ref = _spiked(n, nb * 256, n % 1000 + bf16, bf16=bf16)
    nws = lib.uniter_grad_sumsq_ws_bytes(n)
    assert nws % 8 == 0 and nws >= 8
    bx, bf = Buf(x), Buf(flags)
    ws = Buf(torch.full((nws // 8,), FILL[8], dtype=torch.int64), lead=8, tail=8)
    out = Buf(torch.full((1,), FILL[8], dtype=torch.int64), lead=1, tail=1)
    fn = lib.uniter_grad_sumsq_bf16 if bf16 else lib.uniter_grad_sumsq
    L.check(fn(bx.ptr(), bf.ptr(), n, out.ptr(), ws.ptr(), nws, cs), 'grad_sumsq')
    torch.cuda.synchronize()
    assert ws.guards_ok() and out.guards_ok() and bx.unchanged() and bf.unchanged()
    _sumsq_close(float(out.bits().view(np.float64)[0]), ref, 'sumsq')


PART_CASES = [(4, 1), (4, 7), (12, 2), (1028, 1), (1028, 7), (64, 256), (128, 1), (64 * 15, 2), (64 * 16, 1), (64 * 17, 2048),
              (256 * 4 * 2, 1), (256 * 4 * 2, 2), (64 * 17 * 8, 7), (SIZES[6], 256), (SIZES[6], 2048), (SIZES[7], 256), (SIZES[7], 2048)]


@pytest.mark.parametrize('with_flags', [False, True], ids=['noflags', 'flags'])
@pytest.mark.parametrize('n,nblocks', PART_CASES)
def test_grad_sumsq_part_matches_float64(n, nblocks, with_flags):
    """`nblocks` unreduced partial sums (blocks without an item leave 0), joined in float64 on the host and by
    uniter_sumsq_combine; every second case starts 16 bytes x an odd number into its buffer"""
    L = _L()
    lib, cs = L.lib(), L.cur_stream()
    x, flags, ref = _spiked(n, nblocks * 256, n % 1000 + nblocks, flags_wanted=with_flags)
    sliced = (n // 4 + nblocks) % 2 == 1
    bx = Buf(x, lead=GUARD + (12 if sliced else 0))
    assert bx.ptr() % 16 == 0 and (not sliced or (bx.ptr() - bx.full.data_ptr()) // 16 % 2 == 1)
    bf = Buf(flags) if with_flags else None
    parts = Buf(torch.full((nblocks,), FILL[8], dtype=torch.int64), lead=4, tail=4)
    L.check(lib.uniter_grad_sumsq_part(bx.ptr(), None if bf is None else bf.ptr(), n, parts.ptr(), nblocks, cs), 'grad_sumsq_part')
    out = Buf(torch.full((1,), FILL[8], dtype=torch.int64), lead=1, tail=1)
    L.check(lib.uniter_sumsq_combine(parts.ptr(), nblocks, out.ptr(), cs), 'sumsq_combine')
    torch.cuda.synchronize()
    assert parts.guards_ok() and out.guards_ok() and bx.unchanged()
    pv = parts.bits().view(np.float64)
    assert np.isfinite(pv).all() and (pv >= 0).all()
    assert (pv[(n // 4 + 255) // 256:] == 0).all()           # workgroups behind the last item
    _sumsq_close(math.fsum(pv), ref, 'sum of the parts')
    _sumsq_close(float(out.bits().view(np.float64)[0]), ref, 'combined')


@pytest.mark.parametrize('n', [1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 20000])
def test_sumsq_combine_matches_float64_and_reads_no_further(n):
    L = _L()
    lib, cs = L.lib(), L.cur_stream()
    r = np.random.default_rng(n)
    parts = 10.0 ** r.uniform(-12, 6, n)
    bp = Buf(torch.as_tensor(parts), lead=4, tail=4096)        # NaN behind the parts: a slot not asked for must not be read
    outs = []
    for _ in range(2):
        out = Buf(torch.full((1,), FILL[8], dtype=torch.int64), lead=1, tail=1)
        L.check(lib.uniter_sumsq_combine(bp.ptr(), n, out.ptr(), cs), 'sumsq_combine')
        torch.cuda.synchronize()
        assert out.guards_ok() and bp.unchanged()
        outs.append(out.bits().copy())
    assert np.array_equal(outs[0], outs[1])
    got, ref = float(outs[0].view(np.float64)[0]), math.fsum(parts)
    ratio = abs(got - ref) / (R.COMBINE_REL * math.fsum(np.abs(parts)))
    WORST['combine'] = max(WORST['combine'], ratio)
    assert math.isfinite(got) and ratio <= 1.0, (got, ref, ratio)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the step against float64
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = (1, 2, 10, 1000, 100000)
GMAGS = (1e-8, 1e-3, 1.0, 1e4)
LRWD = ((3e-5, 1e-3), (1e-3, 1e-2), (1e-3, 0.0))
GRIDS = ('default', 'one', 'three', 'full', 'over')


def _step_cases():
    """48 of the 2 x 5 x 4 x 4 x 3 x 3 x 8 x 5 combinations: every axis walks through all its values with its own period"""
    out = []
    for i in range(48):
        lr, wd = LRWD[i % 3]
        c = dict(i=i, adamw=i % 2, step=STEPS[i % 5], moments=R.MOMENTS[(i // 3) % 4], gmag=GMAGS[(i // 2) % 4], lr=lr, wd=wd,
                 clip=('off', 'active', 'tiny')[(i // 5) % 3], n=SIZES[(i * 3) % 8], grid=GRIDS[(i // 2) % 5])
        if i in (7, 30):
            c['b1'] = 0.0
        out.append(c)
    return out


def _split(case):
    case = dict(case)
    n, grid, seed = case.pop('n'), case.pop('grid', 'default'), case.pop('i', 0)
    return n, grid, 100 + seed, case


@pytest.mark.parametrize('case', _ids(_step_cases()))
def test_step_matches_float64(case):
    n, grid, seed, kw = _split(case)
    inp = _inputs(n, seed, **kw)
    Run(*inp, entry='ex', wgs=_wgs(grid, n), mirror='bf16' if seed % 2 else None)


@pytest.mark.parametrize('adamw', [0, 1])
@pytest.mark.parametrize('clip', R.CLIPS)
def test_step_clip_modes_match_float64(clip, adamw):
    """no clip at a norm far below max_norm, coef about 0.1, a norm of 1e-3 against max_norm 1e-4 (where the + 1e-6 is worth 1e-3),
    max_norm = 0 with sumsq = NULL, and max_norm > 0 with all-zero gradients and sumsq = 0"""
    for n in (64 * 17, SIZES[6]):
        inp = _inputs(n, 7 + adamw, adamw=adamw, step=3, clip=clip, wd=1e-2 if adamw == 0 else 1e-3)
        r = Run(*inp, wgs=3)
        assert (r.sumsq is None) == (clip == 'null')
        if clip == 'zero':
            assert inp[6] == 0.0 and r.h.max_norm > 0


def test_norm_kernel_chained_into_the_step():
    """the way the trainer does it: uniter_grad_sumsq leaves the double on the device, the step reads it from there"""
    L = _L()
    lib, cs = L.lib(), L.cur_stream()
    n = SIZES[6]
    inp = _inputs(n, 11, clip='active', step=5)
    r = Run(*inp, launch=False)
    r.sumsq = Buf(torch.full((1,), FILL[8], dtype=torch.int64), lead=1, tail=1)
    nws = lib.uniter_grad_sumsq_ws_bytes(n)
    ws = Buf(torch.full((nws // 8,), FILL[8], dtype=torch.int64), lead=8, tail=8)
    L.check(lib.uniter_grad_sumsq(r.g.ptr(), r.flags.ptr(), n, r.sumsq.ptr(), ws.ptr(), nws, cs), 'grad_sumsq')
    L.check(r.launch(), 'adam_step_ex')
    torch.cuda.synchronize()
    _sumsq_close(float(r.sumsq.bits().view(np.float64)[0]), inp[6], 'sumsq')
    r.sumsq.init = r.sumsq.full.clone()
    r.check()
    assert ws.guards_ok()


@pytest.mark.parametrize('n', SIZES)
def test_step_does_not_depend_on_the_grid(n):
    """max_workgroups 0, 1, 3, the grid in which every thread takes its two items once, and more than that: against float64 each,
    and bit-identical p, m, v, g and mirror"""
    inp = _inputs(n, n % 977, adamw=1, step=2, clip='active')
    base = Run(*inp, wgs=0, mirror='x3', entry='x3')
    for grid in GRIDS[1:]:
        _same(Run(*inp, wgs=_wgs(grid, n), mirror='x3', entry='x3', check=False), base)


@pytest.mark.parametrize('adamw', [0, 1])
def test_eight_steps_each_against_float64_from_the_previous_fp32_state(adamw):
    """the kernel feeds its own state; step k is checked against ONE float64 step from the kernel's fp32 state after step k - 1, so
    no error is carried into a bound"""
    n = 64 * 17 * 8
    p, g, m, v, flags, h, sumsq = _inputs(n, 21, adamw=adamw, moments='zero', clip='active')
    for k in range(1, 9):
        r = Run(p, g, m, v, flags, h.replace(step=k), sumsq, wgs=(0, 1, 3)[k % 3])
        p, m, v = r.p.np(), r.m.np(), r.v.np()
        g = R.make_case(n, 21 + k, wd=h.wd, coef_hint=R.clip_coef(sumsq, h))[1]
        (g,) = _poison(flags, g)
        sumsq = R.ref_sumsq(g, flags)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the step's exact contracts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g16', [False, True], ids=['g32', 'g16'])
@pytest.mark.parametrize('zero', [0, 1])
@pytest.mark.parametrize('n', [64, 64 * 17, SIZES[6]])
def test_skipped_chunks_and_gradient_clearing(n, zero, g16):
    """(Run.check holds every launch to these; here with zero_grads 0 and 1, and with the bf16 payload, whose fp32 buffer is
    cleared in every updated chunk without + 4 whatever it held -- zeros included -- while the payload stays as it is)"""
    inp = _inputs(n, 31 + zero, step=2)
    r = Run(*inp, entry='g16' if g16 else 'ex', g16=g16, zero=zero, wgs=1, mirror='bf16')
    fl = R.expand_flags(inp[4], n)
    assert set(inp[4][:5]) == {0, 1, 2, 5, 6} or n == 64
    if zero and g16:
        assert not r.g.np()[((fl & 3) != 0) & ((fl & 4) == 0)].any()
    if not zero:
        assert r.g.unchanged()


def test_entry_points_agree_bit_for_bit():
    """uniter_adam_step, _mirror, _ex, _g16 with a NULL payload and _x3 with stride 0 on the same inputs"""
    n = 64 * 17 * 8
    inp = _inputs(n, 41, clip='active', step=4)
    base = Run(*inp, entry='step')
    for entry in ('mirror', 'ex', 'g16', 'x3'):
        _same(Run(*inp, entry=entry), base)
    mir = Run(*inp, entry='mirror', mirror='bf16')
    _same(mir, base, keys='pgmv')
    for entry in ('ex', 'g16', 'x3'):
        _same(Run(*inp, entry=entry, mirror='bf16'), mir)


@pytest.mark.parametrize('n', [64 * 17, SIZES[6]])
def test_bf16_payload_equals_the_fp32_path_on_the_widened_values(n):
    inp = list(_inputs(n, 51, clip='active', adamw=1))
    r16 = Run(*inp, entry='g16', g16=True, mirror='bf16', wgs=3)
    inp[1] = r16.inp['g']                                       # the payload widened to fp32 (poisoned chunks included)
    r32 = Run(*inp, entry='ex', mirror='bf16', wgs=3)
    _same(r16, r32, keys=('p', 'm', 'v', 'mirror'))


def test_zero_gradient_and_zero_moments_leave_the_parameters_alone():
    n = 64 * 17
    p, g, m, v, flags, h, sumsq = _inputs(n, 61, wd=0.0, moments='zero', clip='zero')
    r = Run(p, g, m, v, flags, h, sumsq, mirror='bf16')
    assert r.p.unchanged() and r.g.unchanged()
    upd = R.expand_flags(flags, n) != 0
    assert not r.m.np()[upd].any() and not r.v.np()[upd].any()


def _pair_case(wgs):
    """[first | 64 plain | a 6 x 128 tensor whose rows are paired in the mirror | plain] with the launch starting at `first`"""
    first, pre, N, K, n = 128, 64, 6, 128, 64 * 33
    pc = (first + pre) // 64 + np.arange(N * K // 64)           # the paired tensor's chunks; a row is K / 64 of them
    seed = next(s for s in range(71, 200) for f in [R.make_flags((first + n) // 64, s + 1)]
                for ev in [pc[(np.arange(pc.size) // (K // 64)) % 2 == 0]] if ((f[ev] == 0) != (f[ev + K // 64] == 0)).any())        # (one unit skipped, its partner updated)
    p, g, m, v, flags, h, sumsq = _inputs(first + n, seed, clip='active', step=2)
    tab = np.full((n // 64, 2), -1, dtype=np.int32)
    d = np.arange(N * K // 64) * 64
    q, u = d // (2 * K), (d % (2 * K)) // 64
    tab[pre // 64:pre // 64 + d.size, 0] = first + pre + (2 * q) * K + 32 * u
    tab[pre // 64:pre // 64 + d.size, 1] = first + pre + (2 * q + 1) * K + 32 * u
    src = np.arange(n)                                          # mirror position -> parameter, both from the launch's start
    for c in np.nonzero(tab[:, 0] >= 0)[0]:
        for unit in (0, 1):
            src[c * 64 + unit * 32:c * 64 + unit * 32 + 32] = tab[c, unit] - first + np.arange(32)
    assert np.array_equal(np.sort(src), np.arange(n))
    f0, f1 = flags[tab[tab[:, 0] >= 0, 0] // 64], flags[tab[tab[:, 0] >= 0, 1] // 64]
    assert (f0 != f1).any() and ((f0 == 0) != (f1 == 0)).any()      # the two units of one mirror chunk under different flags
    return first, n, (p, g, m, v, flags, h, sumsq), tab, src


@pytest.mark.parametrize('wgs', [0, 1, 2])
def test_pair_table_permutes_the_mirror_and_nothing_else(wgs):
    """uniter_adam_step_x3p over a range that starts inside the buffers (first_element > 0) against uniter_adam_step_x3 over the
    same range: p, m, v, g bit-identical, the mirror the permutation the table describes.  64 * 33 elements: with one workgroup the
    last 16 items are a third round without a partner, with two the first 16 items alone have one."""
    first, n, inp, tab, src = _pair_case(wgs)
    plain, pair = Run(*inp, launch=False, mirror='x3', entry='x3', wgs=wgs), Run(*inp, launch=False, mirror='x3', entry='x3p', wgs=wgs)
    for r in (plain, pair):
        r.stride = n + 192
        r.mirror = Buf(torch.full((2 * r.stride + n,), FILL[2], dtype=torch.int16))
    t = Buf(torch.as_tensor(tab.reshape(-1)))
    _L().check(plain.launch(off=first), 'adam_step_x3')
    _L().check(pair.launch(off=first, tab=t.ptr(), first=first), 'adam_step_x3p')
    torch.cuda.synchronize()
    upd = (R.expand_flags(inp[4], first + n) & 3) != 0
    upd[:first] = False
    plain.check(upd=upd, perm=True)
    pair.check(upd=upd, perm=True)
    assert t.unchanged()
    _same(pair, plain, keys='pgmv')
    a, b, s = plain.mirror.bits(), pair.mirror.bits(), plain.stride
    for k in range(3):
        pk = a[k * s:k * s + n]
        assert np.array_equal(pk[upd[first:]], _bf16_bits(plain.p.np()[first:])[upd[first:]]) or k
        assert np.array_equal(b[k * s:k * s + n], pk[src]), 'piece %d' % k
        assert (b[k * s + n:(k + 1) * s] == FILL[2]).all() or k == 2
    pieces = sum(torch.as_tensor(a[k * s:k * s + n].copy()).view(torch.bfloat16).double().numpy() for k in range(3))
    assert np.array_equal(pieces[upd[first:]], plain.p.np()[first:].astype(np.float64)[upd[first:]])


MASKS = {'empty': lambda r: np.zeros(r, np.uint8), 'full': lambda r: np.ones(r, np.uint8),
         'alternating': lambda r: (np.arange(r) % 2).astype(np.uint8) * 3, 'last': lambda r: (np.arange(r) == r - 1).astype(np.uint8)}


@pytest.mark.parametrize('mask', list(MASKS))
@pytest.mark.parametrize('row_len', [64, 128, 768])
def test_row_split_equals_one_launch(row_len, mask):
    """uniter_adam_step_rows: rows_touched = 0 (the rows whose mask byte is 0, g taken as zero: it holds NaN there, is not read and
    not cleared) then rows_touched = 1 (the masked rows, clipped) against one uniter_adam_step_ex launch over the table whose
    gradient is zero in the unmasked rows"""
    rows = 9
    n = rows * row_len
    p, g, m, v, flags, h, sumsq = _inputs(n, 81 + row_len, clip='active', step=3)
    rm = MASKS[mask](rows)
    masked = np.repeat(rm != 0, row_len)
    upd = (R.expand_flags(flags, n) & 3) != 0
    g_one = np.where(masked, g, np.float32(0)).astype(np.float32)       # (the masked rows keep their NaN / Inf in skipped chunks)
    g_split = _u32(g).copy()
    g_split[~masked] = POISON[0]
    g_split = g_split.view(np.float32)
    sumsq = R.ref_sumsq(g_one, flags)
    one = Run(p, g_one, m, v, flags, h, sumsq)
    two = Run(p, g_split, m, v, flags, h, sumsq, launch=False)
    two.inp['g'] = g_one
    bm = Buf(torch.as_tensor(rm))
    _L().check(two.launch('rows', rowmask=bm.ptr(), row_len=row_len, touched=0, wgs=1), 'adam_step_rows 0')
    torch.cuda.synchronize()
    assert two.g.unchanged()
    two.check(upd=upd & ~masked, g_read=False)                  # the g = 0 reference; everything else bit-identical to its prefill
    mid = {k: getattr(two, k).np() for k in 'pmv'}
    _L().check(two.launch('rows', rowmask=bm.ptr(), row_len=row_len, touched=1, wgs=0), 'adam_step_rows 1')
    torch.cuda.synchronize()
    assert bm.unchanged()
    for b in two.bufs():
        assert b.guards_ok()
    _same(two, one, keys='pmv')
    for k in 'pmv':                                             # the second launch left the first one's rows alone
        assert np.array_equal(_u32(getattr(two, k).np())[~masked], _u32(mid[k])[~masked])
    g2, g1 = two.g.bits(), one.g.bits()
    assert np.array_equal(g2[masked], g1[masked]) and np.array_equal(g2[~masked], _u32(g_split).view(np.int32)[~masked])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_touch_nothing():
    L = _L()
    lib, cs = L.lib(), L.cur_stream()
    n = 64 * 6
    inp = _inputs(n, 91, clip='active')
    r = Run(*inp, launch=False, g16=True, mirror='x3')
    tab = Buf(torch.full((2 * n // 64,), -1, dtype=torch.int32))
    rm = Buf(torch.ones(6, dtype=torch.uint8))
    nws = lib.uniter_grad_sumsq_ws_bytes(n)
    ws = Buf(torch.full((nws // 8,), FILL[8], dtype=torch.int64), lead=8, tail=8)
    parts = Buf(torch.full((2049,), FILL[8], dtype=torch.int64), lead=4, tail=4)
    out = Buf(torch.full((1,), FILL[8], dtype=torch.int64), lead=1, tail=1)
    nomax = r.h.replace(max_norm=0.0)
    refused = [
        ('n % 64', lambda: r.launch('x3', n=n - 4)),
        ('n % 64, rows', lambda: r.launch('rows', n=n - 32, rowmask=rm.ptr(), row_len=32, touched=1)),
        ('step 0', lambda: r.launch('x3', h=r.h.replace(step=0))),
        ('clip without sumsq', lambda: r.launch('x3', sumsq=None)),
        ('null p', lambda: r.launch('x3', p=None)),
        ('null g', lambda: r.launch('ex', g=None)),
        ('null m', lambda: r.launch('step', m=None)),
        ('null v', lambda: r.launch('g16', v=None)),
        ('null flags', lambda: r.launch('mirror', flags=None)),
        ('g16 alignment', lambda: r.launch('g16', g16=r.g16.ptr(2))),
        ('piece stride % 4', lambda: r.launch('x3', ps=r.stride + 2)),
        ('piece stride without a mirror', lambda: r.launch('x3', mirror=None)),
        ('pair table without a mirror', lambda: r.launch('x3p', tab=tab.ptr(), mirror=None, ps=0)),
        ('pair table with one bf16 copy', lambda: r.launch('x3p', tab=tab.ptr(), ps=0)),
        ('pair table, first % 64', lambda: r.launch('x3p', tab=tab.ptr(), first=32)),
        ('row_len does not divide n', lambda: r.launch('rows', rowmask=rm.ptr(), row_len=256, touched=1)),
        ('row_len % 64', lambda: r.launch('rows', rowmask=rm.ptr(), row_len=96, touched=1)),
        ('row mask null', lambda: r.launch('rows', rowmask=None, row_len=64, touched=1)),
        ('workspace too small', lambda: lib.uniter_grad_sumsq(r.g.ptr(), r.flags.ptr(), n, out.ptr(), ws.ptr(), nws - 1, cs)),
        ('workspace too small, bf16', lambda: lib.uniter_grad_sumsq_bf16(r.g16.ptr(), r.flags.ptr(), n, out.ptr(), ws.ptr(), nws - 1, cs)),
        ('sumsq n % 64', lambda: lib.uniter_grad_sumsq(r.g.ptr(), r.flags.ptr(), n - 4, out.ptr(), ws.ptr(), nws, cs)),
        ('sumsq null flags', lambda: lib.uniter_grad_sumsq(r.g.ptr(), None, n, out.ptr(), ws.ptr(), nws, cs)),
        ('part, 0 blocks', lambda: lib.uniter_grad_sumsq_part(r.g.ptr(), None, n, parts.ptr(), 0, cs)),
        ('part, 2049 blocks', lambda: lib.uniter_grad_sumsq_part(r.g.ptr(), None, n, parts.ptr(), 2049, cs)),
        ('part, n % 4', lambda: lib.uniter_grad_sumsq_part(r.g.ptr(), None, n - 2, parts.ptr(), 2, cs)),
        ('part, alignment', lambda: lib.uniter_grad_sumsq_part(r.g.ptr(1), None, n - 4, parts.ptr(), 2, cs)),
        ('combine, n 0', lambda: lib.uniter_sumsq_combine(parts.ptr(), 0, out.ptr(), cs)),
    ]
    for what, call in refused:
        rc = call()
        assert rc != 0, what
        with pytest.raises(L.UniterHipError):
            L.check(rc, what)
        assert lib.uniter_last_error(), what
    torch.cuda.synchronize()
    for b in r.bufs() + [tab, rm, ws, parts, out]:
        assert b.unchanged()
    # max_norm <= 0 needs no sumsq, and the library is left in working order
    L.check(r.launch('x3', sumsq=None, h=nomax), 'adam_step_x3')
    torch.cuda.synchronize()
    r.h, r.sumsq_h = nomax, None
    r.check()
