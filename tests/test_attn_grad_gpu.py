"""GPU: uniter_attn_grad and uniter_attn_relevance (csrc/attn_grad.hip) through the C ABI against the float64 reference and the derived
per-element bounds of tests/attn_grad_ref.py: per head and as the head mean of max(g, 0), with the head sums, qkv as fp32 and as bf16,
the context's gradient as one slab and as two, on the mask layouts, score regimes, the lengths where tile and chunk edges sit (to
L = 257) and the packed batch of tests/attn_ref.py.

Every operand sits in an arena (gemm_ref.Arena): inputs are NaN outside their windows (also between the slabs), every output holds a NaN
sentinel all around its window that is compared bit for bit afterwards, and no element inside may be left unwritten.  Every share
|got - ref| / bound must be <= 1; a packed sample's padding and every masked key's column must hold exact zeros; a second run must give
the same bits.

Worst shares measured on an MI355X (the module in 4 s; profiles/attn_grad_parity.txt): per head 0.308 (fp32 qkv) and 0.215 (bf16 qkv),
head mean 0.308 and 0.205, head_sums 0.011 and 0.022, relevance 0.175."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_probs_ref as PR
import attn_grad_ref as GR
from gemm_ref import in_arena, out_arena, slab_index

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32 = torch.float32
WORST = {}


def _libs():
    from meme_challenge_amd import _lib as Lb
    return Lb, Lb.lib()


def P(a):
    if a is None:
        return None
    return C.c_void_p(a.ptr if hasattr(a, 'flat') else a.data_ptr())


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _note(key, share):
    WORST[key] = max(WORST.get(key, 0.0), share)


def run_grad(call, reduce, b16, n_slabs):
    """one launch into fresh arenas -> (out [B, (nh,) L, L], head_sums [B, nh]) on the host"""
    Lb, lib = _libs()
    qkv = _t(call.qkv)
    qkv = in_arena(qkv.bfloat16() if b16 else qkv, 0, DEV)
    mask = None if call.packed else in_arena(_t(call.mask), 0, DEV)
    cu = _t(call.cu).to(DEV) if call.packed else None
    H = call.H
    if n_slabs == 1:
        dctx, stride = in_arena(_t(call.dO), 0, DEV), 0
    else:
        stride = call.rows * H + 64      # (a gap of NaN between the slabs)
        dctx = in_arena(_t(GR.split_slabs(call.dO)), 0, DEV, index=slab_index(2, call.rows, H, H, stride), stride=H)
    planes = call.B * (1 if reduce else call.nh)
    out = out_arena(planes * call.L, call.L, 0, F32, DEV)
    sums = out_arena(call.B, call.nh, 0, F32, DEV)
    nws = lib.uniter_attn_grad_ws_bytes(call.B, call.L, call.nh)
    assert nws >= 4 * call.B * call.nh and nws % 4 == 0
    ws = out_arena(1, nws // 4, 0, F32, DEV)      # (exactly what the library asks for: a partial beyond it would hit the canary)
    Lb.check(lib.uniter_attn_grad(P(qkv), int(b16), P(mask), P(cu), P(dctx), n_slabs, stride, P(out), P(sums), P(ws), nws, call.B, call.L,
                                  call.nh, int(reduce), Lb.cur_stream()), 'uniter_attn_grad')
    torch.cuda.synchronize()
    bad = out.problems(what='out') + sums.problems(what='head_sums')
    assert not bad, (call.name, bad)                # the NaN canaries are untouched, the windows are written
    assert ws.touched_outside()[0] == 0, (call.name, 'the workspace was overrun')
    shape = (call.B, call.L, call.L) if reduce else (call.B, call.nh, call.L, call.L)
    return out.get().cpu().reshape(shape), sums.get().cpu()


CALLS = {c.name: c for c in GR.grad_calls()}


@pytest.mark.parametrize('n_slabs', [1, 2], ids=['slab1', 'slab2'])
@pytest.mark.parametrize('b16', [False, True], ids=['f32', 'b16'])
@pytest.mark.parametrize('reduce', [0, 1], ids=['all', 'relu_mean'])
@pytest.mark.parametrize('name', list(CALLS))
def test_grad_within_the_derived_bounds(name, reduce, b16, n_slabs):
    call = PR.as_bf16(CALLS[name]) if b16 else CALLS[name]       # (bf16 inputs: the reference takes the bf16 values widened)
    ref = GR.reference(call, n_slabs)
    got, sums = run_grad(call, reduce, b16, n_slabs)
    want, bound = (ref['mean'], ref['E_mean']) if reduce else (ref['g'], ref['E_g'])
    sh = GR.share(got.double().numpy(), want, bound)
    sh_s = GR.share(sums.double().numpy(), ref['sums'], ref['E_sums'])
    tag = ('relu_mean' if reduce else 'all', 'b16' if b16 else 'f32')
    _note(tag, sh)
    _note(('head_sums',) + tag, sh_s)
    print('%s %s %s %d slab(s): share %.3f, head_sums %.3f' % ((name,) + tag + (n_slabs, sh, sh_s)))
    assert sh <= 1.0, (name, reduce, b16, n_slabs, sh)
    assert sh_s <= 1.0, (name, reduce, b16, n_slabs, 'head_sums', sh_s)
    if call.packed:
        for b, n in enumerate(call.lens):
            assert not got[b, ..., n:, :].any() and not got[b, ..., :, n:].any(), (name, b, 'padding of a packed sample must be exact zeros')
    else:
        for b in range(call.B):
            masked = torch.from_numpy(call.mask[b] == 0)
            if not masked.all():      # (every key masked: the bias shifts all scores alike and every key is an ordinary key)
                assert not got[b][..., masked].any(), (name, b, 'a masked key has p = 0, hence g = 0 exactly')
    again, sums2 = run_grad(call, reduce, b16, n_slabs)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (name, 'two runs differ')
    assert torch.equal(sums.view(torch.int32), sums2.view(torch.int32)), (name, 'two runs differ in head_sums')


def test_head_sums_are_optional():
    Lb, lib = _libs()
    call = CALLS['len17-nh2-p0']
    qkv, mask, dctx = (in_arena(_t(x), 0, DEV) for x in (call.qkv, call.mask, call.dO))
    out = out_arena(call.B * call.nh * call.L, call.L, 0, F32, DEV)
    Lb.check(lib.uniter_attn_grad(P(qkv), 0, P(mask), None, P(dctx), 1, 0, P(out), None, None, 0, call.B, call.L, call.nh, 0,
                                  Lb.cur_stream()), 'uniter_attn_grad')
    torch.cuda.synchronize()
    assert not out.problems(what='out')
    full, _ = run_grad(call, 0, False, 1)
    assert torch.equal(out.get().cpu().reshape(full.shape), full)


def run_relevance(maps):
    Lb, lib = _libs()
    nl, B, L = maps.shape[:3]
    a = in_arena(_t(maps).reshape(nl * B * L, L), 0, DEV)
    out, tmp = out_arena(B * L, L, 0, F32, DEV), out_arena(B * L, L, 0, F32, DEV)
    Lb.check(lib.uniter_attn_relevance(P(a), P(out), P(tmp), nl, B, L, Lb.cur_stream()), 'uniter_attn_relevance')
    torch.cuda.synchronize()
    assert out.touched_outside()[0] == 0 and tmp.touched_outside()[0] == 0
    assert not out.problems(what='relevance')
    return out.get().cpu().reshape(B, L, L), tmp.get().cpu().reshape(B, L, L)


@pytest.mark.parametrize('nl', GR.REL_NL)
@pytest.mark.parametrize('L', GR.REL_L)
def test_relevance_within_the_derived_bound(L, nl):
    maps = GR.relevance_maps(L)[:nl]
    ref = GR.relevance_reference(maps)
    got, tmp = run_relevance(maps)
    sh = GR.share(got.double().numpy(), *ref[-1])
    if nl >= 2:      # the product before the last one is what the ping-pong space holds
        sh = max(sh, GR.share(tmp.double().numpy(), *ref[-2]))
    _note(('relevance',), sh)
    print('relevance L %d nl %d: share %.3f' % (L, nl, sh))
    assert sh <= 1.0, (L, nl, sh)
    again, _ = run_relevance(maps)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize('L', [1, 17, 64, 193])
def test_relevance_exact_cases(L):
    eye = np.eye(L, dtype=np.float32)
    got, _ = run_relevance(np.zeros((3, 2, L, L), dtype=np.float32))
    assert torch.equal(got, _t(eye).expand(2, L, L)), L            # all-zero maps: R = I
    maps = GR.upper_triangular_maps(L, 3)
    want = GR.relevance_reference(maps)[-1][0]
    assert want.max() < 2 ** 24
    got, _ = run_relevance(maps)
    assert np.array_equal(got.double().numpy(), want), L            # 0 / 1 strictly upper triangular: exact integers


def test_the_calls_refuse_what_they_cannot_do():
    Lb, lib = _libs()
    st = Lb.cur_stream()
    x = torch.zeros(1 << 16, device=DEV)
    base = x.data_ptr()

    def at(off):
        return C.c_void_p(base + off)
    qkv, dctx, mask, out, hs, ws = at(0), at(16384), at(32768), at(49152), at(65536), at(81920)      # B 1, L 4, nh 1: 3 KB, 1 KB, ..
    ok = dict(qkv=qkv, b16=0, mask=mask, cu=None, dctx=dctx, ns=1, stride=0, out=out, hs=hs, ws=ws, nws=4096, B=1, L=4, nh=1, red=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.uniter_attn_grad(a['qkv'], a['b16'], a['mask'], a['cu'], a['dctx'], a['ns'], a['stride'], a['out'], a['hs'], a['ws'],
                                    a['nws'], a['B'], a['L'], a['nh'], a['red'], st)
    assert call() == 0
    assert call(hs=None, ws=None, nws=0) == 0
    for key in ('qkv', 'dctx', 'out'):
        assert call(**{key: None}) == -1, key                               # null pointers
    assert call(ws=None) == -1 and call(nws=0) == -1                        # head_sums without (enough) workspace
    assert call(cu=mask) == -1 and call(mask=None) == -1                    # both / neither of mask and cu_seqlens
    assert call(qkv=at(8)) == -1 and call(dctx=at(16384 + 8)) == -1         # alignment
    assert call(out=at(49152 + 2)) == -1 and call(ns=2, stride=1026) == -1
    assert call(ns=0) == -1 and call(ns=-1) == -1                           # n_slabs >= 1
    assert call(B=0) == -2 and call(L=0) == -2 and call(nh=0) == -2         # shapes
    assert call(B=65536) == -2 and call(nh=65536) == -2
    assert call(nh=65, red=1, hs=None, ws=None) == -2                       # the reduction walks at most 64 heads
    assert call(out=qkv) == -1 and call(out=at(16384 + 64)) == -1           # outputs overlapping inputs
    assert call(out=mask) == -1 and call(hs=qkv) == -1 and call(ws=dctx) == -1
    assert call(ns=2, stride=8192, out=at(16384 + 4 * 8192)) == -1          # ... also the second slab
    assert call(hs=out) == -1 and call(ws=out) == -1                        # outputs overlapping each other
    rel = lib.uniter_attn_relevance
    assert rel(qkv, out, hs, 2, 1, 4, st) == 0
    assert rel(qkv, out, None, 1, 1, 4, st) == 0
    assert rel(None, out, hs, 2, 1, 4, st) == -1 and rel(qkv, None, hs, 2, 1, 4, st) == -1 and rel(qkv, out, None, 2, 1, 4, st) == -1
    assert rel(qkv, at(64), hs, 2, 1, 4, st) == -1                          # maps alias out (layer 1's map)
    assert rel(qkv, out, at(64), 2, 1, 4, st) == -1                         # maps alias tmp
    assert rel(qkv, out, at(49152 + 32), 2, 1, 4, st) == -1                 # out aliases tmp
    assert rel(qkv, out, hs, 0, 1, 4, st) == -2 and rel(qkv, out, hs, 2, 0, 4, st) == -2 and rel(qkv, out, hs, 2, 1, 0, st) == -2
    assert rel(qkv, out, hs, 2, 65536, 4, st) == -2
    torch.cuda.synchronize()


def test_report_worst_shares():
    print('\nworst shares: ' + ', '.join('%s %.3f' % (' '.join(k), v) for k, v in sorted(WORST.items())))
