"""GPU: uniter_attn_probs and uniter_attn_rollout (csrc/attn_probs.hip) through the C ABI against the float64 reference and the derived
per-element bounds of tests/attn_probs_ref.py: per head and as the mean over heads, qkv as fp32 and as bf16, on the mask layouts, score
regimes, lengths (to L = 321, beyond every other attention kernel's limit) and the packed batch of tests/attn_ref.py.

Every operand sits in an arena (gemm_ref.Arena): inputs are NaN outside their windows, the output holds a NaN sentinel all around its
window that is compared bit for bit afterwards, and no element inside may be left unwritten.  Every share |got - ref| / bound must be
<= 1; a packed sample's padding has bound 0 and must hold exact zeros; a second run must give the same bits.

Worst shares measured on an MI355X (the module in 4 s): probs 0.309 (fp32 qkv) and 0.215 (bf16 qkv), head mean 0.309 and 0.204, rollout
0.116."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_ref as R
import attn_probs_ref as PR
from gemm_ref import in_arena, out_arena

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


def run_probs(call, head_mean, b16):
    """one launch into a fresh arena -> (the arena, its window as [B, (nh,) L, L] float64 on the host)"""
    Lb, lib = _libs()
    qkv = _t(call.qkv)
    qkv = in_arena(qkv.bfloat16() if b16 else qkv, 0, DEV)
    mask = None if call.packed else in_arena(_t(call.mask), 0, DEV)
    cu = _t(call.cu).to(DEV) if call.packed else None
    planes = call.B * (1 if head_mean else call.nh)
    out = out_arena(planes * call.L, call.L, 0, F32, DEV)
    Lb.check(lib.uniter_attn_probs(P(qkv), int(b16), P(mask), P(cu), P(out), call.B, call.L, call.nh, int(head_mean), Lb.cur_stream()),
             'uniter_attn_probs')
    torch.cuda.synchronize()
    shape = (call.B, call.L, call.L) if head_mean else (call.B, call.nh, call.L, call.L)
    return out, out.get().cpu().reshape(shape)


CALLS = {c.name: c for c in PR.probs_calls()}


@pytest.mark.parametrize('b16', [False, True], ids=['f32', 'b16'])
@pytest.mark.parametrize('head_mean', [0, 1], ids=['all', 'mean'])
@pytest.mark.parametrize('name', list(CALLS))
def test_probs_within_the_derived_bounds(name, head_mean, b16):
    call = PR.as_bf16(CALLS[name]) if b16 else CALLS[name]       # (bf16 inputs: the reference takes the bf16 values widened)
    ref = PR.reference(call)
    arena, got = run_probs(call, head_mean, b16)
    bad = arena.problems(what='probs')
    assert not bad, (name, bad)                                  # the NaN canary around the window is untouched, the window is written
    want, bound = (ref['mean'], ref['E_mean']) if head_mean else (ref['p'], ref['E_p'])
    sh = PR.share(got.double().numpy(), want, bound)
    _note(('mean' if head_mean else 'probs', 'b16' if b16 else 'f32'), sh)
    print('%s %s %s: share %.3f' % (name, 'mean' if head_mean else 'all', 'b16' if b16 else 'f32', sh))
    assert sh <= 1.0, (name, head_mean, b16, sh)
    if call.packed:
        for b, n in enumerate(call.lens):
            assert not got[b, ..., n:, :].any() and not got[b, ..., :, n:].any(), (name, b, 'padding of a packed sample must be exact zeros')
    _, again = run_probs(call, head_mean, b16)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (name, 'two runs differ')


def run_rollout(attn, res):
    Lb, lib = _libs()
    nl, B, L = attn.shape[:3]
    a = in_arena(_t(attn).reshape(nl * B * L, L), 0, DEV)
    out, tmp = out_arena(B * L, L, 0, F32, DEV), out_arena(B * L, L, 0, F32, DEV)
    Lb.check(lib.uniter_attn_rollout(P(a), P(out), P(tmp), nl, B, L, res, Lb.cur_stream()), 'uniter_attn_rollout')
    torch.cuda.synchronize()
    assert out.touched_outside()[0] == 0 and tmp.touched_outside()[0] == 0
    assert not out.problems(what='rollout')
    return out.get().cpu().reshape(B, L, L), tmp.get().cpu().reshape(B, L, L)


@pytest.mark.parametrize('res', PR.ROLLOUT_RES)
@pytest.mark.parametrize('nl', PR.ROLLOUT_NL)
@pytest.mark.parametrize('L', PR.ROLLOUT_L)
def test_rollout_within_the_derived_bound(L, nl, res):
    attn = PR.rollout_maps(L)[:nl]
    ref = PR.rollout_reference(attn, res)
    got, tmp = run_rollout(attn, res)
    sh = PR.share(got.double().numpy(), *ref[-1])
    if nl >= 2:      # the product before the last one is what the ping-pong space holds
        sh = max(sh, PR.share(tmp.double().numpy(), *ref[-2]))
    _note(('rollout',), sh)
    print('rollout L %d nl %d residual %g: share %.3f' % (L, nl, res, sh))
    assert sh <= 1.0, (L, nl, res, sh)
    again, _ = run_rollout(attn, res)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize('L', [1, 17, 64, 193])
def test_rollout_of_identities_and_permutations_is_exact(L):
    eye = np.eye(L, dtype=np.float32)
    for res in PR.ROLLOUT_RES:
        got, _ = run_rollout(np.ascontiguousarray(np.broadcast_to(eye, (3, 2, L, L))), res)
        assert torch.equal(got, _t(eye).expand(2, L, L)), (L, res)
    rs = np.random.RandomState(L)
    perms = np.stack([np.stack([eye[rs.permutation(L)] for _ in range(2)]) for _ in range(3)])      # [3, 2, L, L]
    want = perms[0].astype(np.float64)
    for l in (1, 2):
        want = np.matmul(perms[l].astype(np.float64), want)
    got, _ = run_rollout(perms, 0.0)
    assert np.array_equal(got.double().numpy(), want), L


def test_the_calls_refuse_what_they_cannot_do():
    Lb, lib = _libs()
    st = Lb.cur_stream()
    x = torch.zeros(4096, device=DEV)
    p = P(x)
    assert lib.uniter_attn_probs(p, 0, p, None, p, 0, 4, 1, 0, st) == -2
    assert lib.uniter_attn_probs(p, 0, p, None, p, 1, 0, 1, 0, st) == -2
    assert lib.uniter_attn_probs(p, 0, p, None, p, 1, 4, 0, 0, st) == -2
    assert lib.uniter_attn_probs(p, 0, p, None, p, 1, 4, 65, 1, st) == -2
    assert lib.uniter_attn_probs(p, 0, p, p, p, 1, 4, 1, 0, st) == -1
    assert lib.uniter_attn_probs(p, 0, None, None, p, 1, 4, 1, 0, st) == -1
    assert lib.uniter_attn_probs(None, 0, p, None, p, 1, 4, 1, 0, st) == -1
    assert lib.uniter_attn_rollout(p, p, C.c_void_p(x.data_ptr() + 8192), 2, 1, 4, 0.5, st) == -1       # attn aliases rollout
    assert lib.uniter_attn_rollout(p, C.c_void_p(x.data_ptr() + 8192), p, 2, 1, 4, 0.5, st) == -1       # attn aliases tmp
    assert lib.uniter_attn_rollout(p, C.c_void_p(x.data_ptr() + 8192), None, 2, 1, 4, 0.5, st) == -1
    assert lib.uniter_attn_rollout(p, C.c_void_p(x.data_ptr() + 8192), None, 1, 1, 0, 0.5, st) == -2
    assert lib.uniter_attn_rollout(p, C.c_void_p(x.data_ptr() + 8192), None, 1, 1, 4, 1.5, st) == -1
    torch.cuda.synchronize()


def test_report_worst_shares():
    print('\nworst shares: ' + ', '.join('%s %.3f' % (' '.join(k), v) for k, v in sorted(WORST.items())))
