"""The LayerNorm row passes, their column reductions, the column sums and the slab fold of csrc/layernorm.hip (with csrc/rowops.h)
through the C ABI, against float64 torch references built here from the same fp32 input values; dropout is replayed from
oracle/philox.keep_mask.  Outputs are prefilled with NaN (with known values where the call accumulates) and carry guard regions.

Bounds.  Rows, as in tests/test_embeddings_gpu.py and for its reasons: fp32 arithmetic against float64 gives about 4e-6 x max |ref| for
forward rows (z, y; the mean to 4e-6 x max |z| of its row, rstd to 1e-5 relative) and 1e-5 x max |ref| for dz / dx.  Rows whose
LayerNorm input is nearly constant (mean ~1, spread ~1e-3) lose about mean / spread times more of their digits in any fp32
LayerNorm -- already the fp32 rounding of z moves xhat by 2^-24 / 1e-3 = 6e-5 -- and are held to 2e-3 relative, which a two-pass
variance with eps = 1e-12 meets by a wide margin and a one-pass variance or eps = 1e-5 misses by percent to tens of percent.
LayerNorm's output does not depend on the scale of its input, so rows rescaled by 1e3 and 1e-4 keep the well-conditioned bounds.

Column outputs (dgamma, dbeta, dbias, colsum), per column c:   |got - ref| <= 64 * 2^-24 * S_c + 2^-22 * |prefill + ref|,
S_c the float64 sum over rows of the absolute values of the summed terms (|dy| for dbeta, |dy * xhat| for dgamma, |dx| for dbias,
|X| for a column sum).  An fp32 sum evaluated as a tree of depth d errs by at most about d * 2^-24 * S_c; 64 covers the depth of a
sensible two-stage reduction of up to 16384 rows plus the few ulp each term carries itself, while one dropped or doubled row at
M = 10496 moves a column by about S_c / M ~ 1e-4 * S_c, 25 times the bound.  The second term is the rounding of the accumulated
value.  On the ill-conditioned rows the terms themselves carry the 2e-3 of xhat: there dgamma (terms dy * xhat) and dbias (terms
dx = rstd * (gamma dy - c1 - xhat c2), which carry xhat in the same way) are held to 2e-3 * S_c; dbeta keeps the bound above.  (fp32 torch on the CPU, two-pass, reaches
3.5e-4 * S_c for dgamma and 1.0e-4 * S_c for dbias on these rows, given its own statistics or the float64 ones rounded to fp32.)
The same formulas evaluated in fp32 torch on the CPU stay inside every one of these bounds for every case of the lists below."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import philox

pytestmark = pytest.mark.gpu

SEED, OFFSET, SITE = 0x1234ABCD5678, 11, 7
FWD, BWD, ILL, RSTD = 4e-6, 1e-5, 2e-3, 1e-5
U = 2.0 ** -24
COL = 64 * U
NAN = float('nan')
GUARD = 2                                        # guard rows behind row M - 1 of every row output
HS = (4, 8, 64, 128, 256, 260, 516, 768, 1020, 1024)      # NV = 1 (4 .. 256), 2 (260, 516), 3 (768), 4 (1020, 1024)
# a constant row whose every partial sum is exact in fp32 (4 mantissa bits, up to 1024 terms): its fp32 mean is c itself, in any
# summation order.  For a general c the fp32 mean is off by an ulp of c, which rstd = 1 / sqrt(eps) = 1e6 turns into a y far from
# beta in any fp32 LayerNorm; that is the input's doing, not the kernel's.
CONST = 3.75


def _L():
    from meme_challenge_amd import _lib
    return _lib


def _ids(cases):
    return [pytest.param(c, id='-'.join('%s=%s' % kv for kv in c.items())) for c in cases]


def _scale(p):
    """the fp32 value 1 / (1 - p) of make_drop (csrc/philox.h)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def _keep(M, H, p, site=SITE):
    return torch.from_numpy(philox.keep_mask(M * H, p, SEED, OFFSET, site)).view(M, H)


def _padded(t, pad=64):
    """[nslab, M, H] -> a flat device buffer of nslab slabs `stride` floats apart, NaN in the padding; (buffer, stride)"""
    nslab, n = t.shape[0], t[0].numel()
    stride = n + pad
    flat = torch.full((nslab * stride,), NAN)
    flat.view(nslab, stride)[:, :n] = t.reshape(nslab, n)
    return flat.cuda(), stride


class _Inputs:
    """fp32 inputs of one case on the host, and on the device (slabs with a padded stride)"""

    def __init__(self, case):
        self.case = case
        H, M = case['H'], case.get('M', 5)
        self.H, self.M = H, M
        self.cond = case.get('cond')
        self.p = 0.0 if self.cond == 'const' else case.get('p', 0.1)
        self.nslab, self.dyslab = case.get('nslab', 1), case.get('dyslab', 1)
        g = torch.Generator().manual_seed(H * 131 + M * 17 + self.nslab * 5 + self.dyslab * 3 + int(self.p * 10) + len(str(self.cond)))
        rn = lambda *s: torch.randn(*s, generator=g)
        if self.cond == 'ill':                   # z: mean ~1, spread ~1e-3
            xs, res = 1e-3 * rn(self.nslab, M, H), 1.0 + 1e-3 * rn(M, H)
        elif self.cond == 'const':               # z identically CONST
            xs, res = torch.full((self.nslab, M, H), CONST / self.nslab), None
        else:
            s = {'x1e3': 1e3, 'x1e-4': 1e-4}.get(self.cond, 1.0)
            rows = 1.0 + torch.rand(M, 1, generator=g)
            xs, res = s * rn(self.nslab, M, H) * rows, s * rn(M, H)
        if case.get('res') is False:
            res = None
        self.xs, self.res = xs.float(), None if res is None else res.float()
        self.gamma, self.beta = (1.0 + 0.1 * rn(H)).float(), (0.1 * rn(H)).float()
        self.dys = rn(self.dyslab, M, H).float()
        self.keep = _keep(M, H, self.p) if self.p > 0 else None
        self.ill = self.cond == 'ill'

    def to_device(self):
        self.d_x, self.x_stride = _padded(self.xs)
        self.d_dy, self.dy_stride = _padded(self.dys)
        self.d_res = None if self.res is None else self.res.cuda()
        self.d_gamma, self.d_beta = self.gamma.cuda(), self.beta.cuda()
        return self


class _Ref:
    """float64 forward and autograd backward of z = dropout(sum of slabs) + res, y = LayerNorm(z) (biased variance, eps = 1e-12
    inside the root), on the fp32 input values"""

    def __init__(self, inp, backward=True):
        xs = inp.xs.double().requires_grad_(True)
        res = None if inp.res is None else inp.res.double().requires_grad_(True)
        gamma, beta = inp.gamma.double().requires_grad_(True), inp.beta.double().requires_grad_(True)
        x = xs.sum(0)
        if inp.p > 0:
            x = x * inp.keep.double() * _scale(inp.p)
        z = x if res is None else x + res
        z.retain_grad()
        mu = z.mean(-1, keepdim=True)
        var = ((z - mu) ** 2).mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + 1e-12)
        xhat = (z - mu) * rstd
        y = xhat * gamma + beta
        self.z, self.y, self.mean, self.rstd = z.detach(), y.detach(), mu.detach().squeeze(-1), rstd.detach().squeeze(-1)
        if backward:
            dy = inp.dys.double().sum(0)
            y.backward(dy)
            self.dz, self.dx = z.grad, xs.grad[0]                     # (every slab gets the same gradient)
            self.dgamma, self.dbeta, self.dbias = gamma.grad, beta.grad, self.dx.sum(0)
            if res is not None:
                assert torch.equal(res.grad, self.dz)
            xhat = xhat.detach()
            self.S = dict(dgamma=(dy * xhat).abs().sum(0), dbeta=dy.abs().sum(0), dbias=self.dx.abs().sum(0))


# ---------------------------------------------------------------------------------------------------------------------------
# checks (host tensors; also what the fp32-torch evaluation of the same formulas was held to on the CPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _rows_close(got, ref, rel, what):
    err, tol = (got.double() - ref).abs().max().item(), rel * ref.abs().max().item()
    assert err <= tol, (what, err, tol)


def _cols_close(got, ref, S, what, pre=None, rel=COL):
    exp = ref if pre is None else pre.double() + ref
    err, tol = (got.double() - exp).abs(), rel * S + 2.0 ** -22 * exp.abs()
    c = int((err - tol).argmax())
    assert (err <= tol).all(), (what, 'column', c, err[c].item(), tol[c].item())


def _check_fwd(inp, ref, z, y, mean, rstd):
    if z is not None:
        _rows_close(z, ref.z, FWD, 'z')
    if inp.cond == 'const':      # xhat is exactly zero: y is beta
        _rows_close(y, ref.y, FWD, 'y')
        assert torch.isfinite(y).all()
    else:
        _rows_close(y, ref.y, ILL if inp.ill else FWD, 'y')
    if mean is not None:
        assert torch.isfinite(rstd).all()
        assert ((mean.double() - ref.mean).abs() <= 4e-6 * ref.z.abs().amax(-1)).all(), 'mean'
        rerr = ((rstd.double() - ref.rstd).abs() / ref.rstd).max().item()
        assert rerr <= (ILL if inp.ill else RSTD), ('rstd', rerr)


def _check_bwd(inp, ref, got, pre):
    rel = ILL if inp.ill else BWD
    if got.get('dz') is not None:
        _rows_close(got['dz'], ref.dz, rel, 'dz')
    if got.get('dx') is not None:
        _rows_close(got['dx'], ref.dx, rel, 'dx')
    _cols_close(got['dbeta'], ref.dbeta, ref.S['dbeta'], 'dbeta', pre['dbeta'])
    _cols_close(got['dgamma'], ref.dgamma, ref.S['dgamma'], 'dgamma', pre['dgamma'], ILL if inp.ill else COL)
    if got.get('dbias') is not None:
        _cols_close(got['dbias'], ref.dbias, ref.S['dbias'], 'dbias', pre['dbias'], ILL if inp.ill else COL)


# ---------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------
def _rows_out(M, H, dtype=torch.float32):
    return torch.full((M + GUARD, H), NAN, dtype=dtype, device='cuda')


def _guards_untouched(M, *outs):
    for t in outs:
        if t is not None:
            assert torch.isnan(t[M:]).all(), 'guard region written'


def _run_fwd(inp, out='all', b16=False, site=SITE, entry=None):
    """-> device tensors z, y, mean, rstd, y_bf16 (None where not asked for), guard rows checked and cut off"""
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    M, H = inp.M, inp.H
    y = _rows_out(M, H)
    z = _rows_out(M, H) if out == 'all' else None
    mean, rstd = ((torch.full((M + 8,), NAN, device='cuda') for _ in range(2)) if out == 'all' else (None, None))
    yb = _rows_out(M, H, torch.bfloat16) if b16 else None
    tail = (M, H, inp.p, SEED, OFFSET, site, cs)
    if inp.nslab > 1 or entry == 'slabs':
        rc = lib.uniter_ln_fwd_slabs(ptr(inp.d_x), inp.nslab, inp.x_stride, ptr(inp.d_res), ptr(inp.d_gamma), ptr(inp.d_beta),
                                     ptr(z), ptr(y), ptr(yb), ptr(mean), ptr(rstd), *tail)
    elif b16:
        rc = lib.uniter_ln_fwd_b16(ptr(inp.d_x), ptr(inp.d_res), ptr(inp.d_gamma), ptr(inp.d_beta), ptr(z), ptr(y), ptr(yb),
                                   ptr(mean), ptr(rstd), *tail)
    else:
        rc = lib.uniter_ln_fwd(ptr(inp.d_x), ptr(inp.d_res), ptr(inp.d_gamma), ptr(inp.d_beta), ptr(z), ptr(y), ptr(mean),
                               ptr(rstd), *tail)
    L.check(rc, 'ln_fwd')
    torch.cuda.synchronize()
    _guards_untouched(M, z, y, yb, mean, rstd)
    cut = lambda t: None if t is None else t[:M]
    return cut(z), cut(y), cut(mean), cut(rstd), cut(yb)


def _prefills(H, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: (c + 0.1 * torch.randn(H, generator=g)).float() for k, c in (('dgamma', 0.5), ('dbeta', -0.25), ('dbias', 0.125))}


def _run_bwd(inp, z, mean, rstd, pre, form='dz+dx', call='one', want_dbias=True, site=SITE):
    """One backward pass.  form: which of dz / dx / the bf16 copy are asked for ('alias': dx == dz); call: 'one' = uniter_ln_bwd
    (_b16), 'two' = uniter_ln_bwd_rows (_slabs) then uniter_ln_bwd_finalize.  -> host tensors"""
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    M, H = inp.M, inp.H
    dz = _rows_out(M, H) if form in ('dz+dx', 'dz', 'alias') else None
    dx = dz if form == 'alias' else (_rows_out(M, H) if form in ('dz+dx', 'dx') else None)
    dxb = _rows_out(M, H, torch.bfloat16) if form == 'b16' else None
    acc = {k: t.cuda() for k, t in pre.items()}
    dbias = acc['dbias'] if want_dbias else None
    nws = lib.uniter_ln_bwd_ws_bytes(M, H)
    ws = torch.full((nws // 4 + 16,), NAN, device='cuda')         # NaN: a partial row that is read without having been written shows
    tail = (M, H, inp.p, SEED, OFFSET, site, ptr(ws), nws, cs)
    if inp.dyslab > 1:
        call = 'two'
    if call == 'one' and form == 'b16':
        rc = lib.uniter_ln_bwd_b16(ptr(inp.d_dy), ptr(z), ptr(mean), ptr(rstd), ptr(inp.d_gamma), ptr(dz), ptr(dx), ptr(dxb),
                                   ptr(acc['dgamma']), ptr(acc['dbeta']), ptr(dbias), *tail)
    elif call == 'one':
        rc = lib.uniter_ln_bwd(ptr(inp.d_dy), ptr(z), ptr(mean), ptr(rstd), ptr(inp.d_gamma), ptr(dz), ptr(dx),
                               ptr(acc['dgamma']), ptr(acc['dbeta']), ptr(dbias), *tail)
    else:
        if inp.dyslab > 1:
            rc = lib.uniter_ln_bwd_rows_slabs(ptr(inp.d_dy), inp.dyslab, inp.dy_stride, ptr(z), ptr(mean), ptr(rstd),
                                              ptr(inp.d_gamma), ptr(dz), ptr(dx), ptr(dxb), int(want_dbias), *tail)
        else:
            rc = lib.uniter_ln_bwd_rows(ptr(inp.d_dy), ptr(z), ptr(mean), ptr(rstd), ptr(inp.d_gamma), ptr(dz), ptr(dx), ptr(dxb),
                                        int(want_dbias), *tail)
        L.check(rc, 'ln_bwd_rows')
        rc = lib.uniter_ln_bwd_finalize(ptr(ws), nws, M, H, ptr(acc['dgamma']), ptr(acc['dbeta']), ptr(dbias), cs)
    L.check(rc, 'ln_bwd')
    torch.cuda.synchronize()
    _guards_untouched(M, dz, dx, dxb)
    assert torch.isnan(ws[nws // 4:]).all(), 'workspace overrun'
    got = dict(dz=dz, dx=dx, dxb=dxb, dgamma=acc['dgamma'], dbeta=acc['dbeta'], dbias=dbias)
    return {k: None if t is None else t[:M].cpu() if t.dim() == 2 else t.cpu() for k, t in got.items()}


def _expected_ws_bytes(M, H):
    """the backward pass's partial rows under the process's switches: one per workgroup of UNITER_LNB_WAVES (4 | 8) waves of
    UNITER_LNB_ROWS (2) rows, 1024 workgroups at the most"""
    waves = 8 if os.environ.get('UNITER_LNB_WAVES') == '8' else 4
    rows = max(1, int(os.environ.get('UNITER_LNB_ROWS', '2')))
    return min(1024, max(1, -(-M // (waves * rows)))) * 3 * H * 4


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------------------------------
def _fwd_cases():
    c = [dict(H=H) for H in HS]                                                   # M = 5: a partial last workgroup of 4 rows
    for H in (260, 768):
        c += [dict(H=H, M=m) for m in (1, 3, 4, 37)]
        c += [dict(H=H, p=0.0), dict(H=H, p=0.5), dict(H=H, res=False), dict(H=H, p=0.0, res=False), dict(H=H, nslab=2),
              dict(H=H, nslab=3, p=0.5), dict(H=H, nslab=2, p=0.0, res=False), dict(H=H, out='y'), dict(H=H, out='y', nslab=2)]
    for H in (4, 260, 516, 768, 1020, 1024):
        c += [dict(H=H, cond=k) for k in ('ill', 'x1e3', 'x1e-4', 'const')]
    c += [dict(H=1020, M=37, nslab=3), dict(H=1024, M=3, out='y', p=0.0), dict(H=516, M=4, res=False, p=0.5),
          dict(H=768, M=10496), dict(H=768, M=37, cond='ill', p=0.0)]
    return _ids(c)


@pytest.mark.parametrize('case', _fwd_cases())
def test_forward_rows_match_float64(case):
    inp = _Inputs(case).to_device()
    ref = _Ref(inp, backward=False)
    z, y, mean, rstd, _ = _run_fwd(inp, out=case.get('out', 'all'))
    cpu = lambda t: None if t is None else t.cpu()
    _check_fwd(inp, ref, cpu(z), cpu(y), cpu(mean), cpu(rstd))
    if inp.cond == 'const':
        assert (rstd.cpu().double() - 1e6).abs().max().item() <= 10.0              # 1 / sqrt(0 + 1e-12)


@pytest.mark.parametrize('case', _ids([dict(H=H) for H in HS] + [dict(H=260, M=37, p=0.5), dict(H=768, M=3, nslab=2),
                                                                   dict(H=1020, M=4, res=False, p=0.0), dict(H=516, M=1),
                                                                   dict(H=768, M=2624)]))
def test_forward_bf16_copy_is_the_rounded_fp32_output(case):
    """uniter_ln_fwd_b16 (uniter_ln_fwd_slabs for several slabs): the bf16 operand copy is y rounded to nearest even, and the
    fp32 outputs are those of the call without the copy, bit for bit"""
    inp = _Inputs(case).to_device()
    z0, y0, mean0, rstd0, _ = _run_fwd(inp)
    z, y, mean, rstd, yb = _run_fwd(inp, b16=True)
    _check_fwd(inp, _Ref(inp, backward=False), z.cpu(), y.cpu(), mean.cpu(), rstd.cpu())
    assert torch.equal(z, z0) and torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    assert torch.equal(yb.view(torch.int16), y.to(torch.bfloat16).view(torch.int16))
    _, y1, _, _, yb1 = _run_fwd(inp, out='y', b16=True)                             # the copy without z and the statistics
    assert torch.equal(y1, y0) and torch.equal(yb1.view(torch.int16), yb.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. backward: rows, and dgamma / dbeta / dbias through the two-stage column reduction
# ---------------------------------------------------------------------------------------------------------------------------
def _bwd_cases():
    sched = (64, 260, 516, 768, 1020, 1024)       # tag=sched: the list that runs again with 8-wave workgroups
    c = [dict(H=H, tag='sched') if H in sched else dict(H=H) for H in HS]
    for H in (260, 768):
        c += [dict(H=H, M=m) for m in (1, 3, 4, 37)]
        c += [dict(H=H, p=0.0), dict(H=H, p=0.5), dict(H=H, res=False), dict(H=H, dyslab=2), dict(H=H, dyslab=2, p=0.0, M=37),
              dict(H=H, cond='ill'), dict(H=H, cond='x1e3'), dict(H=H, cond='x1e-4'), dict(H=H, cond='ill', p=0.0, M=37)]
    c += [dict(H=4, cond='ill'), dict(H=516, cond='ill'), dict(H=1020, cond='ill'), dict(H=1024, cond='ill', M=37),
          dict(H=1020, M=37, dyslab=2, nslab=2)]
    c += [
        # 328 workgroups of 4 waves x 2 rows (164 of 8 waves): below the grid cap, one row per wave, but more than 48 partial rows:
        # the finalize kernel's four-way unrolled loop and its tail
        dict(H=768, M=2624, tag='sched'),
        # 8193 rows: the first M whose 1025 workgroups are capped at 1024; every wave walks two rows, wave 0 of workgroup 0 a
        # third one (row 8192)
        dict(H=1020, M=8193, tag='sched'),
        dict(H=768, M=8193, dyslab=2),
        # B = 64 at L = 164: every wave accumulates dg / db / dbx over two or three rows; 1024 partial rows, 64 per finalize slice
        dict(H=768, M=10496, tag='sched'),
    ]
    return _ids(c)


@pytest.mark.parametrize('case', _bwd_cases())
def test_backward_rows_and_column_sums_match_float64(case):
    """The backward row pass fed (a) the forward kernel's own z, mean, rstd and (b) the float64 ones rounded to fp32, so that a
    forward error cannot mask a backward one or the reverse; dgamma / dbeta / dbias accumulate onto distinct prefills; the single
    call and the rows + finalize pair give the same column outputs bit for bit."""
    inp = _Inputs(case).to_device()
    ref = _Ref(inp)
    M, H = inp.M, inp.H
    assert _L().lib().uniter_ln_bwd_ws_bytes(M, H) == _expected_ws_bytes(M, H)     # (the schedule the environment asks for)
    pre = _prefills(H, M + H)
    z, _, mean, rstd, _ = _run_fwd(inp)
    stats = dict(kernel=(z.contiguous(), mean.contiguous(), rstd.contiguous()),
                 f64=(ref.z.float().cuda(), ref.mean.float().cuda(), ref.rstd.float().cuda()))
    for name, (sz, sm, sr) in stats.items():
        got = _run_bwd(inp, sz, sm, sr, pre)
        _check_bwd(inp, ref, got, pre)
        if inp.p == 0:
            assert torch.equal(got['dx'], got['dz']), name
        else:       # a product by 0 or by one fp32 constant
            assert torch.equal(got['dx'], got['dz'] * (inp.keep.float() * torch.tensor(_scale(inp.p), dtype=torch.float32))), name
        two = _run_bwd(inp, sz, sm, sr, pre, call='two')
        for k in ('dz', 'dx', 'dgamma', 'dbeta', 'dbias'):
            assert torch.equal(two[k], got[k]), (name, k)


@pytest.mark.parametrize('form', ['dz', 'dx', 'alias', 'b16'])
@pytest.mark.parametrize('case', _ids([dict(H=260, p=0.0), dict(H=260, p=0.1), dict(H=768, M=37, p=0.0), dict(H=768, M=37, p=0.5),
                                        dict(H=1020, M=3, p=0.0), dict(H=1020, M=3, p=0.1), dict(H=64, M=1, p=0.1),
                                        dict(H=516, M=4, p=0.1, dyslab=2)]))
def test_backward_output_forms(case, form):
    """dz only, dx only, dx == dz (one buffer: it ends up holding dx) and the bf16 copy alone give what the pass with dz and dx
    gives, bit for bit (the copy: dx rounded to nearest even), and the same column outputs"""
    inp = _Inputs(case).to_device()
    ref = _Ref(inp)
    pre = _prefills(inp.H, 3)
    z, _, mean, rstd, _ = _run_fwd(inp)
    z, mean, rstd = z.contiguous(), mean.contiguous(), rstd.contiguous()
    base = _run_bwd(inp, z, mean, rstd, pre)
    _check_bwd(inp, ref, base, pre)
    for call in ('one', 'two'):
        got = _run_bwd(inp, z, mean, rstd, pre, form=form, call=call)
        if form == 'dz':
            assert torch.equal(got['dz'], base['dz']) and got['dx'] is None
        elif form == 'dx':
            assert torch.equal(got['dx'], base['dx']) and got['dz'] is None
        elif form == 'alias':
            assert torch.equal(got['dx'], base['dx'])
        else:
            assert torch.equal(got['dxb'].view(torch.int16), base['dx'].to(torch.bfloat16).view(torch.int16))
        for k in ('dgamma', 'dbeta', 'dbias'):
            assert torch.equal(got[k], base[k]), k


@pytest.mark.parametrize('case', _ids([dict(H=260), dict(H=768, M=37, p=0.0), dict(H=1020, M=2624), dict(H=8, M=3)]))
def test_backward_without_dbias_never_touches_the_third_partial_row(case):
    """want_dbias = 0 / dbias = NULL: the workspace is NaN beforehand and its third partial row stays unwritten; dgamma and dbeta
    are finite and those of the pass with dbias"""
    inp = _Inputs(case).to_device()
    ref = _Ref(inp)
    pre = _prefills(inp.H, 5)
    z, _, mean, rstd, _ = _run_fwd(inp)
    z, mean, rstd = z.contiguous(), mean.contiguous(), rstd.contiguous()
    base = _run_bwd(inp, z, mean, rstd, pre)
    for call in ('one', 'two'):
        got = _run_bwd(inp, z, mean, rstd, pre, call=call, want_dbias=False)
        assert got['dbias'] is None
        assert torch.isfinite(got['dgamma']).all() and torch.isfinite(got['dbeta']).all()
        _check_bwd(inp, ref, got, pre)
        for k in ('dz', 'dx', 'dgamma', 'dbeta'):
            assert torch.equal(got[k], base[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 3. column sums and the slab fold
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4, 260, 768, 3072])
@pytest.mark.parametrize('M', [1, 3, 33, 2049, 10496])
def test_colsum_f32_matches_float64(M, N):
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    g = torch.Generator().manual_seed(M * 7 + N)
    ld = N + 8
    X = torch.full((M, ld), NAN)
    X[:, :N] = torch.randn(M, N, generator=g) * (1.0 + torch.rand(1, N, generator=g))
    ref, S = X[:, :N].double().sum(0), X[:, :N].double().abs().sum(0)
    pre = (0.5 + torch.randn(N, generator=g)).float()
    dX = X.cuda()
    nws = lib.uniter_colsum_ws_bytes(M, N)
    ws = torch.full((nws // 4 + 16,), NAN, device='cuda')
    for beta in (1, 0):
        out = torch.full((N + 8,), NAN, device='cuda')
        out[:N] = pre.cuda()
        L.check(lib.uniter_colsum_f32(ptr(dX), M, N, ld, ptr(out), beta, ptr(ws), nws, cs))
        torch.cuda.synchronize()
        _cols_close(out[:N].cpu(), ref, S, 'colsum beta=%d' % beta, pre if beta else None)
        assert torch.isnan(out[N:]).all() and torch.isnan(ws[nws // 4:]).all()


@pytest.mark.parametrize('N', [8, 520, 3072])
@pytest.mark.parametrize('M', [1, 63, 64, 65, 2624])
def test_colsum_bf16_add_matches_float64(M, N):
    """float atomics: the sum differs from run to run, so two runs are held to the bound"""
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    g = torch.Generator().manual_seed(M * 11 + N)
    ld = N + 8
    X = torch.full((M, ld), NAN, dtype=torch.bfloat16)
    X[:, :N] = (torch.randn(M, N, generator=g) * (1.0 + torch.rand(1, N, generator=g))).to(torch.bfloat16)
    ref, S = X[:, :N].double().sum(0), X[:, :N].double().abs().sum(0)           # of the bf16 values
    pre = (0.5 + torch.randn(N, generator=g)).float()
    dX = X.cuda()
    for run in range(2):
        out = torch.full((N + 8,), NAN, device='cuda')
        out[:N] = pre.cuda()
        L.check(lib.uniter_colsum_bf16_add(ptr(dX), M, N, ld, ptr(out), cs))
        torch.cuda.synchronize()
        _cols_close(out[:N].cpu(), ref, S, 'colsum_bf16 run %d' % run, pre)
        assert torch.isnan(out[N:]).all()


@pytest.mark.parametrize('nslab', [1, 2, 5])
@pytest.mark.parametrize('n', [4, 1028, 2 ** 21 + 4])          # the last: more 16-byte groups than 2048 workgroups x 256 threads
def test_slab_reduce_add_matches_float64(n, nslab):
    L = _L()
    g = torch.Generator().manual_seed(n % 1000 + nslab)
    slabs = torch.randn(nslab, n, generator=g)
    pre = torch.randn(n, generator=g)
    d_slabs, stride = _padded(slabs)
    out = torch.full((n + 8,), NAN, device='cuda')
    out[:n] = pre.cuda()
    L.check(L.lib().uniter_slab_reduce_add(L.ptr(d_slabs), nslab, stride, L.ptr(out), n, L.cur_stream()))
    torch.cuda.synchronize()
    ref = pre.double() + slabs.double().sum(0)
    tol = (nslab + 1) * U * (pre.double().abs() + slabs.double().abs().sum(0))
    err = (out[:n].cpu().double() - ref).abs()
    assert (err <= tol).all(), (int((err - tol).argmax()), err.max().item())
    assert torch.isnan(out[n:]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. keep flags drawn ahead: the hand-over is consumed by a refused call
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_consumes_the_keep_flags_handed_over():
    """uniter_ln_set_next_keep_bits, then a call that is refused: the next valid call draws its own flags.  The flags handed over
    are ANOTHER site's, so a hand-over that survived the refusal would show in the outputs."""
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    inp = _Inputs(dict(H=264, M=5, p=0.3)).to_device()
    M, H = inp.M, inp.H
    other = SITE + 4
    nb = lib.uniter_hidden_keep_bits_bytes(M * H)
    bits = torch.zeros(nb, dtype=torch.uint8, device='cuda')
    L.check(lib.uniter_hidden_keep_bits_gen(ptr(bits), nb, 1, other, other, 0, M * H, inp.p, SEED, OFFSET, cs))
    z, y, mean, rstd, _ = _run_fwd(inp)
    assert not torch.equal(_keep(M, H, inp.p), _keep(M, H, inp.p, other))
    pre = _prefills(H, 9)
    base = _run_bwd(inp, z.contiguous(), mean.contiguous(), rstd.contiguous(), pre)
    nan_out = torch.full((M * 3 * H + 64,), NAN, device='cuda')
    x3 = torch.full((M * 3 * H + 64,), NAN, dtype=torch.bfloat16, device='cuda')
    nws = lib.uniter_ln_bwd_ws_bytes(M, H)
    ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    P = ptr(nan_out)

    def refused_fwd():       # H = 6
        return lib.uniter_ln_fwd(ptr(inp.d_x), None, ptr(inp.d_gamma), ptr(inp.d_beta), None, P, None, None, M, 6, inp.p, SEED,
                                 OFFSET, SITE, cs)

    def refused_fwd_x3():    # the three-piece copy at H % 8 != 0
        return lib.uniter_ln_fwd_slabs_x3(ptr(inp.d_x), 1, 0, None, ptr(inp.d_gamma), ptr(inp.d_beta), None, P, ptr(x3), None, None,
                                          M, 260, inp.p, SEED, OFFSET, SITE, cs)

    def refused_bwd():
        return lib.uniter_ln_bwd_rows(ptr(inp.d_dy), ptr(z.contiguous()), ptr(mean.contiguous()), ptr(rstd.contiguous()),
                                      ptr(inp.d_gamma), P, None, None, 1, M, 6, inp.p, SEED, OFFSET, SITE, ptr(ws), nws, cs)

    def refused_bwd_x3():
        return lib.uniter_ln_bwd_rows_slabs_x3(ptr(inp.d_dy), 1, 0, ptr(z.contiguous()), ptr(mean.contiguous()),
                                               ptr(rstd.contiguous()), ptr(inp.d_gamma), P, None, ptr(x3), 1, M, 260, inp.p, SEED,
                                               OFFSET, SITE, ptr(ws), nws, cs)

    for refused in (refused_fwd, refused_fwd_x3, refused_bwd, refused_bwd_x3):
        L.check(lib.uniter_ln_set_next_keep_bits(ptr(bits)))
        assert refused() != 0, refused.__name__
        z1, y1, _, _, _ = _run_fwd(inp)
        assert torch.equal(z1, z) and torch.equal(y1, y), refused.__name__
        L.check(lib.uniter_ln_set_next_keep_bits(ptr(bits)))
        assert refused() != 0, refused.__name__
        got = _run_bwd(inp, z.contiguous(), mean.contiguous(), rstd.contiguous(), pre)
        assert torch.equal(got['dx'], base['dx']) and torch.equal(got['dbias'], base['dbias']), refused.__name__
    assert torch.isnan(nan_out).all() and torch.isnan(x3).all()
    # and handed over to a valid call, the other site's flags do show (the check above can see a leak)
    L.check(lib.uniter_ln_set_next_keep_bits(ptr(bits)))
    z2, _, _, _, _ = _run_fwd(inp)
    assert not torch.equal(z2, z)
    x64 = inp.xs[0].double() * _keep(M, H, inp.p, other).double() * _scale(inp.p) + inp.res.double()
    _rows_close(z2.cpu(), x64, FWD, 'z with the flags handed over')


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the 8-wave backward: the switch is read once per process, so the tagged cases run again in a child process
# ---------------------------------------------------------------------------------------------------------------------------
def test_backward_with_eight_wave_workgroups():
    """UNITER_LNB_WAVES=8 (ln_bwd_kernel<NV, 8>: its own LDS reduction, half as many partial rows): one H per NV with full and
    partial last chunks at a small M, and the large M; the child asserts that the switch took effect (through the workspace size
    it implies)."""
    env = {'UNITER_LNB_WAVES': '8'}
    if any(k in os.environ for k in env):
        pytest.fail('run this test without %s set' % ', '.join(env))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider',
                        'tests/test_layernorm_f64_gpu.py::test_backward_rows_and_column_sums_match_float64', '-k', 'sched'],
                       cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '9 passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]


# ---------------------------------------------------------------------------------------------------------------------------
# 6. refusals: host-side checks that return before a launch (every buffer is sized so that even a launch would stay in bounds)
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_do_not_cover():
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    E_ARG, E_SHAPE = -1, -2
    M, H, Hmax = 2, 128, 1028
    n = 8 * Hmax * 8
    src = torch.zeros(n, device='cuda')                      # every input
    ones = torch.ones(n, device='cuda')                      # rstd
    out = torch.full((n,), NAN, device='cuda')               # every fp32 output
    out16 = torch.full((n,), NAN, dtype=torch.bfloat16, device='cuda')
    src16 = torch.zeros(n, dtype=torch.bfloat16, device='cuda')
    ok = torch.full((n,), NAN, device='cuda')                # outputs of the legal calls
    ok16 = torch.full((n,), NAN, dtype=torch.bfloat16, device='cuda')
    S, O, O16 = ptr(src), ptr(out), ptr(out16)
    ws_ln = lambda M, H: lib.uniter_ln_bwd_ws_bytes(M, H)

    def fwd(H=H, M=M, p=0.1, nslab=1, stride=0, gamma=S, y=O, mean=O, rstd=O):
        return lib.uniter_ln_fwd_slabs(S, nslab, stride, S, gamma, S, O if y is O else ptr(ok), y, None, mean, rstd, M, H, p, 1, 0,
                                       0, cs)

    def fwd_x3(H=H, y3=O16, y=O):
        return lib.uniter_ln_fwd_slabs_x3(S, 1, 0, S, S, S, None, y, y3, None, None, M, H, 0.1, 1, 0, 0, cs)

    def bwd(H=H, M=M, nslab=1, stride=0, dz=O, dx=O, dxb=None, short=0, ws=O):
        return lib.uniter_ln_bwd_rows_slabs(S, nslab, stride, S, S, ptr(ones), S, dz, dx, dxb, 1, M, H, 0.1, 1, 0, 0, ws,
                                            ws_ln(M, H) - short, cs)

    def bwd_x3(H=H, dx3=O16, dz=O, ws=O):
        return lib.uniter_ln_bwd_rows_slabs_x3(S, 1, 0, S, S, ptr(ones), S, dz, None, dx3, 1, M, H, 0.1, 1, 0, 0, ws, ws_ln(M, H),
                                               cs)

    def colsum(N=H, short=0, o=O, ws=O):
        return lib.uniter_colsum_f32(S, M, N, N, o, 0, ws, lib.uniter_colsum_ws_bytes(M, N) - short, cs)

    def colsum16(N=H, X=ptr(src16), o=O):
        return lib.uniter_colsum_bf16_add(X, M, N, N, o, cs)

    def fold(n=H, o=O):
        return lib.uniter_slab_reduce_add(S, 1, 0, o, n, cs)

    K, K16 = ptr(ok), ptr(ok16)
    # the legal calls these vary
    assert fwd(y=K, mean=K, rstd=K) == 0 and fwd_x3(y3=K16, y=K) == 0 and bwd(dz=K, dx=K, ws=K) == 0
    assert bwd_x3(dx3=K16, dz=K, ws=K) == 0 and colsum(o=K, ws=K) == 0 and fold(o=K) == 0
    ok[:H] = 0
    assert colsum16(o=K) == 0
    torch.cuda.synchronize()

    def refused(rc, code, word):
        assert rc == code, (word, rc)
        assert word.encode() in lib.uniter_last_error(), (word, lib.uniter_last_error())

    refused(fwd(H=6), E_SHAPE, 'multiple of 4')
    refused(fwd(H=0), E_SHAPE, 'multiple of 4')
    refused(fwd(H=Hmax), E_SHAPE, 'unsupported')
    refused(fwd(p=-0.1), E_ARG, 'dropout')
    refused(fwd(p=1.0), E_ARG, 'dropout')
    refused(fwd(nslab=0), E_ARG, 'slab')
    refused(fwd(nslab=2, stride=M * H - 4), E_ARG, 'slab')
    refused(fwd(gamma=None), E_ARG, 'null')
    refused(fwd(rstd=None), E_ARG, 'mean/rstd')
    refused(fwd_x3(H=260), E_SHAPE, 'x3')
    refused(fwd_x3(y3=ptr(out16[4:])), E_SHAPE, 'x3')                  # 8-byte aligned
    refused(bwd(H=6), E_SHAPE, 'multiple of 4')
    refused(bwd(H=0), E_SHAPE, 'multiple of 4')
    refused(bwd(H=Hmax), E_SHAPE, 'unsupported')
    refused(bwd(nslab=0), E_ARG, 'slab')
    refused(bwd(nslab=2, stride=M * H - 4), E_ARG, 'slab')
    refused(bwd(dz=None, dx=None), E_ARG, 'need dz or dx')
    refused(bwd(short=1), E_ARG, 'workspace')
    refused(bwd_x3(H=260), E_SHAPE, 'x3')
    refused(bwd_x3(dx3=ptr(out16[4:])), E_SHAPE, 'x3')
    refused(lib.uniter_ln_bwd(S, S, S, ptr(ones), S, O, O, None, O, O, M, H, 0.1, 1, 0, 0, O, ws_ln(M, H), cs), E_ARG, 'null')
    refused(lib.uniter_ln_bwd_finalize(O, ws_ln(M, H) - 1, M, H, O, O, O, cs), E_ARG, 'finalize')
    refused(colsum(N=6), E_SHAPE, 'multiples of 4')
    refused(colsum(short=1), E_ARG, 'workspace')
    refused(colsum16(N=12), E_SHAPE, 'multiples of 8')
    refused(colsum16(X=ptr(src16[4:])), E_SHAPE, '16-byte')
    refused(fold(n=6), E_SHAPE, 'multiples of 4')
    # M = 0: nothing to do, nothing launched
    assert fwd(M=0) == 0 and bwd(M=0) == 0
    assert lib.uniter_ln_bwd_finalize(O, ws_ln(0, H), 0, H, O, O, O, cs) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(out16).all()
