"""GPU: the dense products against float64 where the other GEMM tests do not look (tests/gemm_ref.py has the references, the bounds
and the arena; tests/test_gemm_bounds_cpu.py checks those on the CPU).

A. Activation sweep: each epilogue function alone at exactly known fp32 arguments (the accumulator is 0, 1, -2 or 0.5 exactly in every
   family), a few thousand points over [-12, 12] and the planted ones, against float64 at the bounds of gemm_ref.py.
B. Contract cases: every operand at a leading dimension larger than its width (pad 8 and 24 elements), at a base that is 16-byte
   and not 32-byte aligned, inputs surrounded by NaN, outputs surrounded by a sentinel that must survive bit for bit; results at the
   tolerance of the family's own test file, and bit-identical to the dense call where the path has no atomics.

Measured on an MI355X, the worst error of the sweep as a share of its bound -- the same in every family and configuration, the
epilogue functions being shared code: gelu_pair_fast (epilogue 5) gelu 0.388, gelu' 0.470, with a bf16 aux_out 0.994 and with only the
bf16 output 0.976 (the 2^-8 |ref| term: bf16 rounding itself); gelu_erf (2) 0.177; acc * dgelu_erf (3) 0.231, bf16 output only 0.995;
x aux (6) exact; the x3 output carries the fp32 output's error, 0.388.  Absolute, over |u| <= 12 at the sweep's points: gelu 3.92e-7,
gelu' 2.42e-7; a dense search of 400 000 points per window through epilogue 5 (f32 cfg 0 and 4, bf16 cfg 1, bf16v2 cfg 1 and 6, x3
cfg 3, all alike) gives the device maxima gelu 4.22e-7 at x = 3.108 and gelu' 3.20e-7 at x = 0.0751 -- what csrc/common.h states.
The contract cases found no violation: no store outside a window, no finite result that depends on padding, and every path
without atomics bit-identical to the dense call."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF, F32 = torch.bfloat16, torch.float32
D = np.float64


def _vp(a):
    return None if a is None else ctypes.c_void_p(a.ptr)


def _gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _dgelu(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


# ---------------------------------------------------------------------------------------------------------------------------
# one launch of any family on arenas
# ---------------------------------------------------------------------------------------------------------------------------
def _gemm(family, cfg, akm, bkm, M, N, K, epi, d, pad, dense=False, nsplit=1, beta=0, out='both', aux_bf16=False, b_pm=False):
    """d: CPU tensors A, B (fp32, as stored: [K, M] if akm, [K, N] if bkm), bias [N], aux [M, N], C0 [M, N].  Every operand goes into
    an arena at leading dimension width + pad (dense: plain tensors, ld = width).  Returns the output arenas."""
    from meme_challenge_amd import _lib as L
    lib = L.lib()
    p = 0 if dense else pad
    x8, x64 = (8 if p else 0), (64 if p else 0)
    A, B = d['A'], d['B']
    psa = psb = 0
    if family == 'x3':
        ald, bld = A.shape[1] + p, B.shape[1] + p
        lda, psa = 3 * ald + x8, ald
        ldb, psb = (bld, B.shape[0] * bld + x64) if b_pm else (3 * bld + x8, bld)
        a = R.in_arena(R.split3_host(A), 0, DEV, dense, index=R.x3_index(A.shape[0], A.shape[1], lda, psa), stride=lda)
        b = R.in_arena(R.split3_host(B), 0, DEV, dense, index=R.x3_index(B.shape[0], B.shape[1], ldb, psb), stride=ldb)
    else:
        if family in ('res', 'v2'):
            A, B = A.bfloat16(), B.bfloat16()
        a, b = R.in_arena(A, p, DEV, dense), R.in_arena(B, p, DEV, dense)
        lda, ldb = A.shape[1] + p, B.shape[1] + p
    bias = R.in_arena(d['bias'].view(1, N), p, DEV, dense) if epi in (1, 2, 5) else None
    aux_in = None
    if epi in (3, 4, 6):
        aux_in = R.in_arena(d['aux'].bfloat16() if aux_bf16 else d['aux'], p, DEV, dense)
    aux_out = R.out_arena(M, N, p, BF if aux_bf16 else F32, DEV, dense) if epi in (2, 5) else None
    ldc = ld_aux = N + p
    css = M * ldc + x64
    want_c = out in ('both', 'f32') or nsplit > 1 or beta or family in ('f32', 'bf16')
    want_2 = out in ('both', 'bf16', 'x3') and nsplit == 1 and not beta and family in ('res', 'v2', 'x3')
    C = Cb = Cx = None
    if want_c:
        C = R.out_arena(M, N, p, F32, DEV, dense, index=R.slab_index(nsplit, M, N, ldc, css) if nsplit > 1 else None,
                        init=d['C0'] if beta else None, stride=ldc)
    ldcb = N + p
    ldcx, pscx = 3 * (N + p) + x8, N + p
    if want_2 and family == 'x3':
        Cx = R.out_arena(M, N, 0, BF, DEV, dense, index=R.x3_index(M, N, ldcx, pscx), stride=ldcx)
    elif want_2:
        Cb = R.out_arena(M, N, p, BF, DEV, dense)
    st = L.cur_stream()
    if family in ('f32', 'bf16'):
        fn = lib.uniter_gemm_f32_cfg if family == 'f32' else lib.uniter_gemm_bf16_cfg
        rc = fn(cfg, akm, bkm, M, N, K, _vp(a), lda, _vp(b), ldb, _vp(C), ldc, epi, _vp(bias), _vp(aux_in), _vp(aux_out), ld_aux, beta, st)
    elif family == 'res':
        rc = lib.uniter_gemm_bf16res_cfg(cfg, akm, bkm, M, N, K, _vp(a), lda, _vp(b), ldb, _vp(C), ldc, _vp(Cb), ldcb, epi, _vp(bias),
                                         _vp(aux_in), _vp(aux_out), ld_aux, beta, st)
    elif family == 'v2':
        rc = lib.uniter_gemm_bf16v2_cfg(cfg, nsplit, akm, bkm, M, N, K, _vp(a), lda, _vp(b), ldb, _vp(C), ldc, css, _vp(Cb), ldcb, epi,
                                        _vp(bias), _vp(aux_in), int(aux_bf16), _vp(aux_out), int(aux_bf16), ld_aux, beta, st)
    else:
        rc = lib.uniter_gemm_x3_cfg(cfg, nsplit, akm, bkm, M, N, K, _vp(a), lda, psa, _vp(b), ldb, psb, _vp(C), ldc, css, _vp(Cx), ldcx,
                                    pscx, epi, _vp(bias), _vp(aux_in), _vp(aux_out), ld_aux, st)
    L.check(rc, 'gemm %s' % family)
    torch.cuda.synchronize()
    return dict(C=C, Cb=Cb, Cx=Cx, aux_out=aux_out)


def _np(arena):
    return arena.get().float().cpu().numpy() if arena.dtype == BF else arena.get().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# A. the activation sweep
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_case():
    return R.forward_case()


@functools.lru_cache(maxsize=None)
def _dgrad_case(bf16):
    return R.dgrad_case(bf16=bf16)


SHARES = {}


def _share(key, got, ref, bound):
    r = R.worst_ratio(got, ref, bound)
    SHARES[key] = max(SHARES.get(key, 0.0), r)
    return r


def _abs(key, got, ref, where):
    SHARES[key] = max(SHARES.get(key, 0.0), float(np.abs(got.astype(D) - ref)[where].max()))


def _report(family):
    print('sweep shares %s: ' % family + ', '.join('%s %.3g' % (k[1], v) for k, v in sorted(SHARES.items()) if k[0] == family))


def _pieces_are_the_fp32_output(joined, c32, tag):
    """the x3 output is the exact three-piece split of the fp32 output -- for |x| >= 2^-108; below, the third piece falls under bf16's
    subnormals: an absolute error <= 2^-133 (tests/test_gemm_x3_gpu.py, the extreme-operand cases, state the same range)"""
    c = c32.astype(D)
    small = np.abs(c) < 2.0 ** -108
    assert np.array_equal(joined[~small], c[~small]), tag
    assert small.sum() == 0 or np.abs(joined[small] - c[small]).max() <= 2.0 ** -133, tag


def _sweep_forward(family, cfg, epi, K=R.SWEEP_K, out='both', aux_bf16=False):
    """C = gelu(u), aux_out = u (epilogue 2) or gelu'(u) (epilogue 5) at u = s_m + bias[n]"""
    c = _fwd_case()
    M, N = R.SWEEP_M, R.SWEEP_N
    d = dict(A=torch.from_numpy(R.sweep_A(M, K)), B=torch.ones(N, K), bias=torch.from_numpy(c['bias']))
    o = _gemm(family, cfg, 0, 0, M, N, K, epi, d, 0, dense=True, out=out, aux_bf16=aux_bf16)
    tag = (family, cfg, epi, K, out, aux_bf16)
    name = 'pair' if epi == 5 else 'erf'
    bg = R.B_PAIR_GELU if epi == 5 else R.bound_erf(c['u'])
    inner = np.abs(c['u']) <= 12
    second = o['Cb'] if o['Cb'] is not None else o['Cx']
    if o['C'] is not None:
        got = _np(o['C'])
        assert not np.isnan(got).any(), tag
        r = _share((family, 'gelu_%s' % name), got, c['gelu'], R.sweep_bound(bg, c['scale'], c['gelu']))
        _abs((family, 'abs_gelu_%s' % name), got, c['gelu'], inner)
        assert r <= 1.0, tag + ('gelu', r)
    if second is not None:
        g2 = second.get()
        if o['Cx'] is not None:
            v = g2.double().sum(1).cpu().numpy()             # the exact sum of the three pieces
        else:
            v = g2.float().cpu().numpy()
        assert not np.isnan(v).any(), tag
        if o['C'] is not None and o['Cx'] is not None:
            _pieces_are_the_fp32_output(v, _np(o['C']), tag)
        elif o['C'] is not None:
            assert torch.equal(g2, o['C'].get().bfloat16()), tag                # the bf16 copy is the RNE rounding of the fp32 output
        else:
            r = _share((family, 'gelu_%s_second_only' % name), v, c['gelu'], R.sweep_bound(bg, c['scale'], c['gelu'], bf16_only=o['Cb'] is not None))
            assert r <= 1.0, tag + ('gelu, second output only', r)
    ga = _np(o['aux_out'])
    assert not np.isnan(ga).any(), tag
    if epi == 2 and not aux_bf16:
        assert np.array_equal(ga.view(np.int32), c['u'].view(np.int32)), tag   # u itself: the one fp32 addition, bit for bit
    elif epi == 2:
        assert R.worst_ratio(ga, c['u'].astype(D), R.sweep_bound(0.0, c['scale'], c['u'], bf16_only=True)) <= 1.0, tag
    else:
        r = _share((family, 'dgelu_pair' + ('_bf16' if aux_bf16 else '')), ga, c['dgelu'],
                   R.sweep_bound(R.B_PAIR_DGELU, c['scale'], c['dgelu'], bf16_only=aux_bf16))
        if not aux_bf16:
            _abs((family, 'abs_dgelu_pair'), ga, c['dgelu'], inner)
        assert r <= 1.0, tag + ('gelu\'', r)


def _sweep_dgrad(family, cfg, epi, K=R.SWEEP_K, out='both', aux_bf16=False):
    """C = s_m * gelu'(aux_in[m, n]) (epilogue 3) or s_m * aux_in[m, n] (epilogue 6)"""
    c = _dgrad_case(aux_bf16)
    M, N = R.SWEEP_M, R.SWEEP_N
    d = dict(A=torch.from_numpy(R.sweep_A(M, K)), B=torch.ones(K, N), aux=torch.from_numpy(c['aux']))
    o = _gemm(family, cfg, 0, 1, M, N, K, epi, d, 0, dense=True, out=out, aux_bf16=aux_bf16)
    tag = (family, cfg, epi, K, out, aux_bf16)
    ref = c['dgelu_mul'] if epi == 3 else c['mul']
    b = R.bound_erf(c['aux']) if epi == 3 else 0.0
    key = 'dgelu_erf_mul' if epi == 3 else 'mul'
    if o['C'] is not None:
        got = _np(o['C'])
        assert not np.isnan(got).any(), tag
        r = _share((family, key), got, ref, R.sweep_bound(b, c['scale'], ref))
        assert r <= 1.0, tag + (r,)
    second = o['Cb'] if o['Cb'] is not None else o['Cx']
    if second is not None:
        g2 = second.get()
        v = g2.double().sum(1).cpu().numpy() if o['Cx'] is not None else g2.float().cpu().numpy()
        assert not np.isnan(v).any(), tag
        if o['C'] is not None and o['Cx'] is not None:
            _pieces_are_the_fp32_output(v, _np(o['C']), tag)
        elif o['C'] is not None:
            assert torch.equal(g2, o['C'].get().bfloat16()), tag
        else:
            r = _share((family, key + '_second_only'), v, ref, R.sweep_bound(b, c['scale'], ref, bf16_only=o['Cb'] is not None))
            assert r <= 1.0, tag + ('second output only', r)


@pytest.mark.parametrize('cfg,K', [(0, 64), (1, 64), (21, 64), (24, 64), (4, 64), (0, 40)])
def test_sweep_f32(cfg, K):
    """uniter_gemm_f32_cfg: the buffer-path kernels (cfg 0, 1, 21, 24) and the v1 fallback (cfg 4; K = 40, no multiple of the k-tile)"""
    for epi in (2, 5):
        _sweep_forward('f32', cfg, epi, K)
    for epi in (3, 6):
        _sweep_dgrad('f32', cfg, epi, K)
    _report('f32')


@pytest.mark.parametrize('cfg', [0, 1, 4])
@pytest.mark.parametrize('family', ['bf16', 'res'])
def test_sweep_bf16_and_bf16res(family, cfg):
    for epi in (2, 5):
        _sweep_forward(family, cfg, epi)
    for epi in (3, 6):
        _sweep_dgrad(family, cfg, epi)
    if family == 'res':
        _sweep_forward(family, cfg, 5, out='bf16')
        _sweep_dgrad(family, cfg, 3, out='bf16')
    _report(family)


@pytest.mark.parametrize('cfg', [1, 2, 3, 4, 5, 6, 7, 8])
def test_sweep_bf16v2(cfg):
    """cfg 1-5: epilogues 2, 3, 5 (and 6); the persistent kernels 6-8: epilogue 5 (6 and 7 also x aux); fp32 and bf16 aux"""
    for out, aux_bf16 in (('both', False), ('bf16', True)):
        for epi in ((2, 5) if cfg <= 5 else (5,)):
            _sweep_forward('v2', cfg, epi, out=out, aux_bf16=aux_bf16)
        for epi in ((3, 6) if cfg <= 5 else (6,) if cfg <= 7 else ()):
            _sweep_dgrad('v2', cfg, epi, out=out, aux_bf16=aux_bf16)
    _report('v2')


@pytest.mark.parametrize('cfg', [1, 2, 3, 4, 5])
def test_sweep_x3(cfg):
    """epilogue 5 with the fp32 output, the x3 output and both (cfg 5: fp32 only); x aux on the input-gradient layout"""
    for out in (('both', 'f32', 'x3') if cfg != 5 else ('f32',)):
        _sweep_forward('x3', cfg, 5, out=out)
        if cfg != 5:
            _sweep_dgrad('x3', cfg, 6, out=out)
    _report('x3')


# ---------------------------------------------------------------------------------------------------------------------------
# B. leading dimensions, poisoned surroundings, guard bands, 16-byte alignment
# ---------------------------------------------------------------------------------------------------------------------------
def _data(family, akm, bkm, M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((K, M) if akm else (M, K), generator=g)
    B = torch.randn((K, N) if bkm else (N, K), generator=g) * (0.05 if family == 'x3' else 1.0)
    d = dict(A=A, B=B, bias=torch.randn(N, generator=g), aux=torch.randn(M, N, generator=g), C0=torch.randn(M, N, generator=g))
    return d


def _contract(family, cfg, akm, bkm, M, N, K, epi, pad, nsplit=1, beta=0, out='both', aux_bf16=False, b_pm=False):
    d = _data(family, akm, bkm, M, N, K)
    if aux_bf16:
        d['aux'] = d['aux'].bfloat16().float()
    Ar, Br = (d['A'].double(), d['B'].double()) if family in ('f32', 'x3') else (d['A'].bfloat16().double(), d['B'].bfloat16().double())
    ref = (Ar.t() if akm else Ar) @ (Br if bkm else Br.t())
    pre = None
    if epi in (1, 2, 5):
        ref = ref + d['bias'].double()
    if epi == 2:
        pre, ref = ref, _gelu(ref)
    if epi == 5:
        pre, ref = _dgelu(ref), _gelu(ref)
    if epi == 3:
        ref = ref * _dgelu(d['aux'].double())
    if epi == 4:
        ref = ref + d['aux'].double()
    if epi == 6:
        ref = ref * d['aux'].double()
    if beta:
        ref = ref + d['C0'].double()
    tol = {'f32': 2e-5 * math.sqrt(K) * 4, 'bf16': 1e-4 * math.sqrt(K), 'res': 1e-4 * math.sqrt(K),
           'v2': 1e-4 * math.sqrt(K) * (1 + 0.1 * nsplit), 'x3': 3e-6 * math.sqrt(K) * (1.0 + ref.abs().max().item() * 0.05)}[family]
    kw = dict(nsplit=nsplit, beta=beta, out=out, aux_bf16=aux_bf16, b_pm=b_pm)
    o = _gemm(family, cfg, akm, bkm, M, N, K, epi, d, pad, **kw)
    tag = (family, cfg, akm, bkm, M, N, K, epi, pad, nsplit, beta, out, aux_bf16, b_pm)
    bad = []
    if o['C'] is not None:
        bad += o['C'].problems(what='C')                          # (every slab's window written, the gaps between slabs untouched)
        got = o['C'].get().double().cpu()
        got = got.sum(0) if got.dim() == 3 else got
        if not (got - ref).abs().max().item() < tol:
            bad.append('C: max error %.3g >= %.3g' % ((got - ref).abs().max().item(), tol))
    if o['Cb'] is not None:
        bad += o['Cb'].problems(what='C_bf16')
        gb = o['Cb'].get().double().cpu()
        rel = ((gb - ref).abs() / (ref.abs() + 1.0)).max().item()
        if not rel < 2.0 ** -8:
            bad.append('C_bf16: relative error %.3g' % rel)
        if o['C'] is not None and not torch.equal(o['Cb'].get(), o['C'].get().reshape(M, N).bfloat16()):
            bad.append('C_bf16 is not the rounded fp32 output')
    if o['Cx'] is not None:
        bad += o['Cx'].problems(what='C_x3')
        gx = o['Cx'].get().double().sum(1).cpu()
        if not (gx - ref).abs().max().item() < tol:
            bad.append('C_x3: max error %.3g >= %.3g' % ((gx - ref).abs().max().item(), tol))
        if o['C'] is not None and not torch.equal(gx, o['C'].get().reshape(M, N).double().cpu()):
            bad.append('C_x3 is not the exact split of the fp32 output')
    if o['aux_out'] is not None:
        bad += o['aux_out'].problems(what='aux_out')
        ga = o['aux_out'].get().double().cpu()
        e = ((ga - pre).abs() / (pre.abs() + 1.0)).max().item() if aux_bf16 else (ga - pre).abs().max().item()
        if not e < (2.0 ** -8 if aux_bf16 else tol):
            bad.append('aux_out: error %.3g' % e)
    if not beta:            # no atomics: a leading dimension must not change the arithmetic
        od = _gemm(family, cfg, akm, bkm, M, N, K, epi, d, pad, dense=True, **kw)
        for k, v in o.items():
            if v is not None and not torch.equal(v.get().view(R.INT_VIEW[v.dtype]), od[k].get().view(R.INT_VIEW[v.dtype])):
                bad.append('%s: not bit-identical to the call with dense leading dimensions' % k)
    assert not bad, tag + tuple(bad)


PADS = [8, 24]


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('cfg', [0, 1, 2, 3, 4, 21, 24])
def test_contract_f32(cfg, pad):
    M, N, K = 164, 136, 96
    _contract('f32', cfg, 0, 0, M, N, K, 5, pad)
    _contract('f32', cfg, 0, 1, M, N, K, 4, pad)
    _contract('f32', cfg, 1, 0, M, N, K, 0, pad)
    _contract('f32', cfg, 1, 1, M, N, K, 0, pad)
    _contract('f32', cfg, 1, 1, M, N, 100, 0, pad, beta=1)          # weight gradient: ragged K (rows beyond K read as zero), accumulate
    _contract('f32', cfg, 0, 0, M, N, 72, 5, pad)                   # K % 32 != 0: the fallback kernel
    _contract('f32', cfg, 0, 1, M, N, 72, 4, pad)


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('cfg', [0, 1, 2, 3, 4])
def test_contract_bf16(cfg, pad):
    M, N, K = 168, 136, 128
    _contract('bf16', cfg, 0, 0, M, N, K, 5, pad)
    _contract('bf16', cfg, 0, 1, M, N, K, 4, pad)
    _contract('bf16', cfg, 1, 0, M, N, K, 0, pad)
    _contract('bf16', cfg, 1, 1, M, N, 200, 0, pad)
    _contract('bf16', cfg, 1, 1, M, N, 200, 0, pad, beta=1)


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('cfg', [0, 1, 4])
def test_contract_bf16res(cfg, pad):
    M, N, K = 168, 136, 128
    _contract('res', cfg, 0, 0, M, N, K, 5, pad)                   # fp32 and bf16 output: ldcb padded too
    _contract('res', cfg, 0, 0, M, N, K, 5, pad, out='bf16')
    _contract('res', cfg, 0, 1, M, N, K, 4, pad)
    _contract('res', cfg, 1, 1, M, N, 200, 0, pad)
    _contract('res', cfg, 1, 1, M, N, 200, 0, pad, beta=1)


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('cfg', [1, 2, 3, 4, 5, 6, 7, 8])
def test_contract_bf16v2(cfg, pad):
    M, N, K = 257, 264, 192
    for out, aux_bf16 in (('both', False), ('bf16', True)):
        for epi in ((2, 5) if cfg <= 5 else (5,)):
            _contract('v2', cfg, 0, 0, M, N, K, epi, pad, out=out, aux_bf16=aux_bf16)
        for epi in ((3, 6) if cfg <= 5 else (6,) if cfg <= 7 else ()):
            _contract('v2', cfg, 0, 1, M, N, K, epi, pad, out=out, aux_bf16=aux_bf16)


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('cfg', [1, 2, 3, 4, 5, 6, 7, 8])
def test_contract_bf16v2_slabs(cfg, pad):
    """nsplit = 3 with c_split_stride = M * ldc + 64: each slab's window is checked, the gaps between the slabs stay untouched"""
    M, N, K = 257, 264, 192
    _contract('v2', cfg, 0, 0, M, N, K, 1, pad, nsplit=3)
    if cfg != 8:
        _contract('v2', cfg, 0, 1, M, N, K, 4, pad, nsplit=3)
    if cfg in (1, 4):       # the weight-gradient layout of these two: ragged K, slabs and accumulate
        _contract('v2', cfg, 1, 1, 136, N, 200, 0, pad, nsplit=3)
        _contract('v2', cfg, 1, 1, 136, N, 200, 0, pad, beta=1)


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('cfg', [1, 2, 3, 4, 5])
def test_contract_x3(cfg, pad):
    """A as [rows][3][ld] with ld > cols and a padded row stride; B once in that form and once piece-major with a piece stride
    beyond rows * ldb; ldcx and pscx padded"""
    M, N, K = 257, 264, 192
    for b_pm in (False, True):
        for out in (('both', 'x3') if cfg != 5 else ('f32',)):
            _contract('x3', cfg, 0, 0, M, N, K, 5, pad, out=out, b_pm=b_pm)
            if cfg != 5:
                _contract('x3', cfg, 0, 1, M, N, K, 6, pad, out=out, b_pm=b_pm)
    _contract('x3', cfg, 0, 0, M, N, K, 1, pad, nsplit=3)
    if cfg != 5:
        _contract('x3', cfg, 0, 1, M, N, K, 4, pad, nsplit=3, b_pm=True)
    if cfg <= 3:            # weight gradient (whole-K 128 x 128 tiles): ragged K, rows beyond K read as zeros
        _contract('x3', cfg, 1, 1, 136, N, 200, 0, pad, out='f32')
        _contract('x3', cfg, 1, 1, 136, N, 200, 4, pad, out='f32')


# ---------------------------------------------------------------------------------------------------------------------------
# the helpers around the products
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', PADS)
def test_contract_split3_join3(pad):
    """padded source ld and destination strides, both forms of the x3 tensor; exactness as in test_pieces_are_exact"""
    from meme_challenge_amd import _lib as L
    lib = L.lib()
    rows, cols = 257, 264
    g = torch.Generator().manual_seed(1)
    x = torch.randn(rows, cols, generator=g) * torch.exp(torch.randn(rows, cols, generator=g) * 6)
    x[0, :8] = 0.0
    x[1, :4] = torch.tensor([1.0, -1.0, 2.0 ** -100, -(2.0 ** 100)])
    want = R.split3_host(x)
    ld = cols + pad
    for pm in (False, True):
        rs, ps = (ld, rows * ld + 64) if pm else (3 * ld + 8, ld)
        src = R.in_arena(x, pad, DEV)
        dst = R.Arena(R.x3_index(rows, cols, rs, ps), BF, DEV, 257 * rs, 'sentinel')
        L.check(lib.uniter_split3(_vp(src), rows, cols, ld, _vp(dst), rs, ps, L.cur_stream()), 'split3')
        torch.cuda.synchronize()
        assert dst.problems(what='x3') == [], (pm, dst.problems())
        got = dst.get().cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), pm
        assert torch.equal(got.double().sum(1), x.double())
        # join3 of the same pieces, their surroundings NaN, into a padded fp32 window
        src3 = R.Arena(R.x3_index(rows, cols, rs, ps), BF, DEV, 257 * rs, 'nan').put(want)
        back = R.out_arena(rows, cols, pad, F32, DEV)
        L.check(lib.uniter_join3(_vp(src3), rows, cols, rs, ps, _vp(back), ld, L.cur_stream()), 'join3')
        torch.cuda.synchronize()
        assert back.problems(what='x') == [], (pm, back.problems())
        assert torch.equal(back.get().cpu(), x), pm


def test_contract_cast_bf16_and_slab_reduce_add():
    from meme_challenge_amd import _lib as L
    lib = L.lib()
    rows, cols = 257, 264
    n = rows * cols
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, n, generator=g)
    flat = torch.arange(n)[None, :]
    src = R.Arena(flat, F32, DEV, 4096, 'nan').put(x)
    dst = R.Arena(flat, BF, DEV, 4096, 'sentinel')
    L.check(lib.uniter_cast_bf16(_vp(src), _vp(dst), n, L.cur_stream()), 'cast_bf16')
    torch.cuda.synchronize()
    assert dst.problems(what='bf16') == []
    assert torch.equal(dst.get().cpu(), x.bfloat16())                      # round to nearest even
    # three slabs at a stride beyond their length (NaN in the gaps), added into a guarded output
    nslab, stride = 3, n + 64
    s = torch.randn(nslab, n, generator=g)
    out0 = torch.randn(1, n, generator=g)
    slabs = R.Arena(torch.arange(nslab)[:, None] * stride + torch.arange(n)[None, :], F32, DEV, 4096, 'nan').put(s)
    out = R.Arena(flat, F32, DEV, 4096, 'sentinel').put(out0)
    L.check(lib.uniter_slab_reduce_add(_vp(slabs), nslab, stride, _vp(out), n, L.cur_stream()), 'slab_reduce_add')
    torch.cuda.synchronize()
    assert out.problems(what='out') == []
    ref = out0.double() + s.double().sum(0, keepdim=True)
    # four fp32 terms in some order: three additions, each rounding a partial sum that is at most the sum of the magnitudes
    bound = 3 * 2.0 ** -24 * (out0.double().abs() + s.double().abs().sum(0, keepdim=True))
    assert bool(((out.get().double().cpu() - ref).abs() <= bound).all())


GROUP_SHAPES, GROUP_K = [(136, 200), (256, 128), (8, 8)], 200


def _group(family, cfg, overwrite):
    """the grouped weight-gradient launches: operands dense by contract ([K, M], [K, N], dW [M, N]), so guards only -- NaN right
    behind row K - 1 of each k-major operand (rows beyond K must read as zero), the sentinel all around each dW"""
    from meme_challenge_amd import _lib as L
    lib = L.lib()
    K = GROUP_K
    g = torch.Generator().manual_seed(len(GROUP_SHAPES) * 1000 + K)
    Af = [torch.randn(K, M, generator=g) for M, N in GROUP_SHAPES]
    Bf = [torch.randn(K, N, generator=g) * (0.05 if family == 'x3' else 1.0) for M, N in GROUP_SHAPES]
    C0 = [torch.randn(M, N, generator=g) for M, N in GROUP_SHAPES]
    if family == 'x3':
        mk = lambda t: R.Arena(R.x3_index(t.shape[0], t.shape[1], 3 * t.shape[1], t.shape[1]), BF, DEV, 257 * 3 * t.shape[1], 'nan').put(R.split3_host(t))
    elif family == 'bf16':
        Af, Bf = [a.bfloat16() for a in Af], [b.bfloat16() for b in Bf]
        mk = lambda t: R.in_arena(t, 0, DEV)
    else:
        mk = lambda t: R.in_arena(t, 0, DEV)
    As, Bs = [mk(a) for a in Af], [mk(b) for b in Bf]
    Cs = [R.out_arena(M, N, 0, F32, DEV, init=c) for (M, N), c in zip(GROUP_SHAPES, C0)]
    n = len(GROUP_SHAPES)
    IA, PA = ctypes.c_int * n, ctypes.c_void_p * n
    Ms, Ns = IA(*[m for m, _ in GROUP_SHAPES]), IA(*[nn for _, nn in GROUP_SHAPES])
    pa, pb, pc = PA(*[a.ptr for a in As]), PA(*[b.ptr for b in Bs]), PA(*[c.ptr for c in Cs])
    st = L.cur_stream()
    if family == 'f32':
        rc = lib.uniter_wgrad_f32_group(n, Ms, Ns, K, pa, pb, pc, overwrite, st)
    elif family == 'bf16' and not overwrite:
        rc = lib.uniter_wgrad_bf16_group(cfg, n, Ms, Ns, K, pa, pb, pc, st)
    elif family == 'bf16':
        rc = lib.uniter_wgrad_bf16_group_riders(cfg, n, Ms, Ns, K, pa, pb, pc, 1, 0, None, st)
    else:
        rc = lib.uniter_wgrad_x3_group(cfg, n, Ms, Ns, K, pa, pb, pc, overwrite, 0, st)
    L.check(rc, 'wgrad group %s' % family)
    torch.cuda.synchronize()
    for (M, N), a, b, c0, c in zip(GROUP_SHAPES, Af, Bf, C0, Cs):
        ref = a.double().t() @ b.double() + (0 if overwrite else c0.double())
        tol = {'f32': 2e-6 * K ** 0.5 * max(1.0, ref.abs().max().item()) / 10 + 1e-5, 'bf16': 1e-4 * math.sqrt(K),
               'x3': 3e-6 * math.sqrt(K) * (1 + 0.05 * ref.abs().max().item())}[family]
        p = c.problems(ref, tol, 'dW %d x %d' % (M, N))
        assert p == [], (family, cfg, overwrite, p)


@pytest.mark.parametrize('overwrite', [0, 1])
@pytest.mark.parametrize('family,cfg', [('f32', 0), ('bf16', 1), ('bf16', 4), ('bf16', 7), ('x3', 3), ('x3', 4)])
def test_contract_weight_gradient_groups(family, cfg, overwrite):
    _group(family, cfg, overwrite)
