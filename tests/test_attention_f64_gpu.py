"""GPU: every attention kernel family (csrc/attention_f32.hip, attention_x3.hip, attention_bf16.hip) against the float64 reference and
the derived per-element bounds of tests/attn_ref.py, on its case lists: mask layouts with holes, whole masked chunks and single valid
keys; peaked softmax, common offsets of +-300 and probabilities that underflow; every length at which the chunk count, the two key
halves or the last partial wave change; packed batches; dropout with every keep flag visible.

Every operand sits in an arena (gemm_ref.Arena): the base is 16-byte and not 32-byte aligned, inputs are NaN outside their windows,
outputs hold a sentinel outside their windows that is compared bit for bit afterwards, workspaces are NaN-filled.  The windows of lse
and delta are the positions that belong to a sample: in a packed batch the positions at or beyond a sample's length are outside and
must be left untouched (include/uniter_hip.h).

The backward pass runs twice: on ctx_in = fp32(reference ctx), lse_in = fp32(reference lse) -- a forward error cannot hide a backward
one -- and chained to the device's own forward, with the bounds widened by E_ctx and E_lse.  Every share |got - ref| / bound must be
<= 1; the worst per family and output is printed.  The bf16 families are judged by the bf16-rounding reference and the bars of
tests/test_attention_bf16_gpu.py.

Worst shares measured on an MI355X (forward | backward on the reference's ctx, lse | chained), the whole module in 16 s:
    fwd_pre / bwd_ex (keep flags drawn or read)   ctx 0.15 lse 0.30 | dq 0.28 dk 0.18 dv 0.18 delta 0.25 bias_part 0.07 | all <= 0.11
    fwd_pre_x3 / bwd_ex_x3 (MASKS)                ctx 0.04 lse 0.16 | dq 0.13 dk 0.14 dv 0.10 delta 0.24 bias_part 0.02 | all <= 0.05
    attn_fwd / attn_bwd (to L = 321)              ctx 0.05 lse 0.16 | dq 0.13 dk 0.14 dv 0.10 delta 0.28                | all <= 0.06
    fwd_varlen / bwd_varlen                       ctx 0.04 lse 0.11 | dq 0.08 dk 0.07 dv 0.09 delta 0.21                | all <= 0.05
    attn_x3_fwd / attn_x3_bwd                     ctx 0.19 lse 0.30 | dq 0.39 dk 0.14 dv 0.31 delta 0.19 bias_part 0.07 | all <= 0.17
    bf16 and b16x (shares of the existing bars)   ctx max 0.27, mean 0.30, lse 0.004, dq 0.24, dk 0.33, dv 0.02
The first run found one thing: at SCORES (|s| up to 400) some gradients are below 2^-102, where a three-piece copy cannot be exact
(see _check_copy and include/uniter_hip.h)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_ref as R
from gemm_ref import in_arena, out_arena, x3_index, slab_index

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32, B16 = torch.float32, torch.bfloat16
WORST = {}


def _libs():
    from meme_challenge_amd import _lib as Lb
    return Lb, Lb.lib()


def P(a):
    """the pointer of an arena's window, of a plain tensor, or NULL"""
    if a is None:
        return None
    return C.c_void_p(a.ptr if hasattr(a, 'flat') else a.data_ptr())


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _offset16(n, dtype, fill):
    """a tensor of n elements whose base is 16-byte and not 32-byte aligned"""
    isz = torch.empty(0, dtype=dtype).element_size()
    t = torch.full((n + 16 // isz + 64,), fill, dtype=dtype, device=DEV)[16 // isz:]
    assert t.data_ptr() % 32 == 16
    return t


class Operands:
    """the inputs of one call on the device, each in an arena"""

    def __init__(self, call):
        Lb, lib = _libs()
        self.call = call
        self.qkv = in_arena(_t(call.qkv), 0, DEV)
        self.dO = in_arena(_t(call.dO), 0, DEV)
        self.mask = None if call.packed else in_arena(_t(call.mask), 0, DEV)
        self.cu = _t(call.cu).to(DEV) if call.packed else None
        self.pos = torch.nonzero(_t(call.valid_pos()).reshape(-1))[:, 0]        # positions of lse / delta that belong to a sample
        self.keep = None
        if call.p > 0 and call.L <= 192:
            self.keep = self.new_keep()
            Lb.check(lib.uniter_attn_keep_bits_gen(P(self.keep), 0, 1, call.B, call.L, call.nh, call.p, R.SEED, R.OFFSET, R.SITE, 0,
                                                   Lb.cur_stream()))

    def new_keep(self):
        _, lib = _libs()
        c = self.call
        return _offset16(max(lib.uniter_attn_keep_bits_bytes(c.B, c.L, c.nh), 2) // 2, torch.int16, 0)

    def pos_in(self, x):
        """lse / delta as an input: [B, nh, L] values at the samples' positions, NaN elsewhere"""
        return in_arena(_t(np.asarray(x, dtype=np.float32)).reshape(-1)[self.pos], 0, DEV, index=self.pos, stride=self.call.L)

    def pos_out(self):
        return out_arena(0, 0, 0, F32, DEV, index=self.pos, stride=self.call.L)

    def pos_get(self, arena):
        c = self.call
        out = np.full(c.B * c.nh * c.L, np.nan)
        out[self.pos.numpy()] = arena.get().double().cpu().numpy()
        return out.reshape(c.B, c.nh, c.L)


def _mc(ops):
    return P(ops.mask), P(ops.cu)


def _problems(arenas):
    out = []
    for name, a in arenas.items():
        if a is not None:
            out += a.problems(what=name)
    return out


def _pieces_sum(x3):
    d = x3.double()
    return d[:, 2] + d[:, 1] + d[:, 0]


PIECES_EXACT_FROM = 2.0 ** -102


def _check_copy(kind, copy, full, what):
    """the operand copies of an fp32 output: bf16 = the rounded value, pieces = its exact three-piece split.  The split of an fp32
    value x = m 2^e (24-bit m) consists of multiples of 2^(e - 23); they are normal bf16 numbers, and the split is exact, from
    |x| >= 2^-102.  Below that a piece may be a bf16 subnormal, which the conversion flushes: there the pieces' sum is within 2^-126."""
    full = full.get()
    if kind == 'b16':
        assert torch.equal(copy.get(), full.bfloat16()), what
        return
    c = copy.get()
    s = _pieces_sum(c)
    big = full.abs() >= PIECES_EXACT_FROM
    bad = (s.float() != full) | (c[:, 0] != full.bfloat16())
    off = (s - full.double()).abs()
    report = (what, 'mismatches %d, of them at |x| >= 2^-102: %d' % (int(bad.sum()), int((bad & big).sum())),
              'largest |x| at a mismatch %.3g' % (full.abs()[bad].max().item() if bad.any() else 0.0), 'largest |sum - x| %.3g' % off.max().item())
    assert not (bad & big).any() and off.max().item() <= 2.0 ** -126, report


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32-accurate families
# ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = {      # family -> (forward, backward)
    'pre0': ('uniter_attn_fwd_pre, keep_bits_ready = 0', 'uniter_attn_bwd_ex, Philox drawn again'),
    'pre1': ('uniter_attn_fwd_pre, keep_bits_ready = 1', 'uniter_attn_bwd_ex, keep flags read'),
    'pre_x3': ('uniter_attn_fwd_pre_x3', 'uniter_attn_bwd_ex_x3'),
    'plain': ('uniter_attn_fwd', 'uniter_attn_bwd'),
    'varlen': ('uniter_attn_fwd_varlen', 'uniter_attn_bwd_varlen'),
    'x3': ('uniter_attn_x3_fwd', 'uniter_attn_x3_bwd'),
}


def forward(fam, ops):
    Lb, lib = _libs()
    c = ops.call
    args = (c.B, c.L, c.nh, c.p)
    rnd = (R.SEED, R.OFFSET, R.SITE)
    st = Lb.cur_stream()
    ctx = out_arena(c.rows, c.H, 0, F32, DEV)
    lse = ops.pos_out()
    copy, kind, keep = None, None, None
    m, cu = _mc(ops)
    if fam in ('pre0', 'pre1'):
        copy, kind = out_arena(c.rows, c.H, 0, B16, DEV), 'b16'
        keep = ops.keep if fam == 'pre1' else ops.new_keep()
        ready = 1 if fam == 'pre1' and c.p > 0 else 0
        Lb.check(lib.uniter_attn_fwd_pre(P(ops.qkv), m, cu, P(ctx), P(copy), P(lse), P(keep), ready, *args, *rnd, st))
    elif fam == 'pre_x3':
        copy, kind = out_arena(c.rows, c.H, 0, B16, DEV, index=x3_index(c.rows, c.H, 3 * c.H, c.H), stride=3 * c.H), 'x3'
        Lb.check(lib.uniter_attn_fwd_pre_x3(P(ops.qkv), m, cu, P(ctx), P(copy), P(lse), P(ops.keep), 1 if c.p > 0 else 0, *args, *rnd, st))
    elif fam == 'plain':
        Lb.check(lib.uniter_attn_fwd(P(ops.qkv), m, P(ctx), P(lse), *args, *rnd, st))
    elif fam == 'varlen':
        Lb.check(lib.uniter_attn_fwd_varlen(P(ops.qkv), cu, P(ctx), P(lse), *args, *rnd, st))
    elif fam == 'x3':
        copy, kind = out_arena(c.rows, c.H, 0, B16, DEV, index=x3_index(c.rows, c.H, 3 * c.H, c.H), stride=3 * c.H), 'x3'
        Lb.check(lib.uniter_attn_x3_fwd(P(ops.qkv), m, cu, P(ctx), P(copy), P(lse), P(ops.keep) if c.p > 0 else None, *args, st))
    torch.cuda.synchronize()
    bad = _problems(dict(ctx=ctx, lse=lse, ctx_copy=copy))
    assert not bad, (fam, c.name, bad)
    if copy is not None:
        _check_copy(kind, copy, ctx, (fam, c.name, 'ctx copy'))
    if fam == 'pre0' and c.p > 0 and not c.packed:      # (a packed sample's flags beyond its length are never drawn)
        assert torch.equal(keep, ops.keep), (fam, c.name, 'the keep flags the kernel drew are not those drawn ahead')
    return dict(ctx=ctx.get().double().cpu().numpy(), lse=ops.pos_get(lse))


def backward(fam, ops, ctx_in, lse_in, slabs=None):
    """slabs: dO given as that many k-pieces (x3 only) -> returns the raw dqkv_x3 / delta tensors as well"""
    Lb, lib = _libs()
    c = ops.call
    args = (c.B, c.L, c.nh, c.p)
    rnd = (R.SEED, R.OFFSET, R.SITE)
    st = Lb.cur_stream()
    a_ctx, a_lse = in_arena(_t(np.asarray(ctx_in, dtype=np.float32)), 0, DEV), ops.pos_in(lse_in)
    dqkv = out_arena(c.rows, 3 * c.H, 0, F32, DEV)
    delta = ops.pos_out()
    part, copy, kind = None, None, None
    m, cu = _mc(ops)
    if fam in ('pre0', 'pre1', 'pre_x3', 'plain', 'varlen'):
        wsb = lib.uniter_attn_bwd_ws_bytes(c.B, c.L, c.nh)
        ws = _offset16(max(wsb, 4) // 4, F32, float('nan'))
    if fam in ('pre0', 'pre1'):
        part = out_arena(c.B, 3 * c.H, 0, F32, DEV)
        copy, kind = out_arena(c.rows, 3 * c.H, 0, B16, DEV), 'b16'
        keep = ops.keep if fam == 'pre1' and c.p > 0 else None
        Lb.check(lib.uniter_attn_bwd_ex(P(ops.qkv), m, cu, P(a_ctx), P(a_lse), P(ops.dO), P(dqkv), P(copy), P(part), P(keep), P(delta),
                                        *args, *rnd, P(ws), wsb, st))
    elif fam == 'pre_x3':
        part = out_arena(c.B, 3 * c.H, 0, F32, DEV)
        copy, kind = out_arena(c.rows, 3 * c.H, 0, B16, DEV, index=x3_index(c.rows, 3 * c.H, 9 * c.H, 3 * c.H), stride=9 * c.H), 'x3'
        Lb.check(lib.uniter_attn_bwd_ex_x3(P(ops.qkv), m, cu, P(a_ctx), P(a_lse), P(ops.dO), P(dqkv), P(copy), P(part), P(ops.keep),
                                           P(delta), *args, *rnd, P(ws), wsb, st))
    elif fam == 'plain':
        Lb.check(lib.uniter_attn_bwd(P(ops.qkv), m, P(a_ctx), P(a_lse), P(ops.dO), P(dqkv), P(delta), *args, *rnd,
                                     P(ws) if wsb else None, wsb, st))
    elif fam == 'varlen':
        Lb.check(lib.uniter_attn_bwd_varlen(P(ops.qkv), cu, P(a_ctx), P(a_lse), P(ops.dO), P(dqkv), P(delta), *args, *rnd, P(ws), wsb, st))
    elif fam == 'x3':
        part = out_arena(c.B, 3 * c.H, 0, F32, DEV)
        copy, kind = out_arena(c.rows, 3 * c.H, 0, B16, DEV, index=x3_index(c.rows, 3 * c.H, 9 * c.H, 3 * c.H), stride=9 * c.H), 'x3'
        dO, ns, stride = ops.dO, 1, 0
        if slabs:
            dO, ns, stride = slabs
        Lb.check(lib.uniter_attn_x3_bwd(P(ops.qkv), m, cu, P(a_ctx), P(a_lse), P(dO), ns, stride, P(dqkv), P(copy), P(part),
                                        P(ops.keep) if c.p > 0 else None, P(delta), *args, st))
    torch.cuda.synchronize()
    bad = _problems(dict(dqkv=dqkv, delta=delta, bias_part=part, dqkv_copy=copy))
    assert not bad, (fam, c.name, bad)
    if copy is not None:
        _check_copy(kind, copy, dqkv, (fam, c.name, 'dqkv copy'))
    got = dict(dqkv=dqkv.get().double().cpu().numpy(), delta=ops.pos_get(delta))
    if part is not None:
        got['bias_part'] = part.get().double().cpu().numpy()
    if slabs:
        got['raw'] = (copy.get().clone(), delta.get().clone(), dqkv.get().clone())
    return got


def judge(fam, call, slabs_too=False):
    """forward, backward on the reference's ctx / lse, backward chained to the device forward: every share <= 1"""
    ref = R.reference(call)
    ops = Operands(call)
    fw = forward(fam, ops)
    runs = [('fwd', R.shares(call, ref, fw, names=('ctx', 'lse')))]
    names = ('dq', 'dk', 'dv', 'delta') + (('bias_part',) if fam not in ('plain', 'varlen') else ())
    runs.append(('bwd', R.shares(call, ref, backward(fam, ops, ref['ctx_in'], ref['lse_in']), names=names)))
    lse_dev = np.where(call.valid_pos(), fw['lse'], 0.0)
    runs.append(('chained', R.shares(call, ref, backward(fam, ops, fw['ctx'], lse_dev), chained=True, names=names)))
    for run, sh in runs:
        for name, v in sh.items():
            key = (fam, run, name)
            if v >= WORST.get(key, (0.0, ''))[0]:
                WORST[key] = (v, call.name)
    over = [(run, name, '%.3f' % v) for run, sh in runs for name, v in sh.items() if not v <= 1.0]
    print('%-7s %-22s %s' % (fam, call.name, '  '.join('%s[%s]' % (run, ' '.join('%s %.3f' % kv for kv in sh.items())) for run, sh in runs)))
    assert not over, (fam, call.name, over)
    return ops, ref, fw


def _report(fam):
    print('\nworst shares, %s (%s | %s):' % ((fam,) + FAMILIES[fam]))
    for (f, run, name), (v, where) in sorted(WORST.items()):
        if f == fam:
            print('  %-8s %-10s %.3f  (%s)' % (run, name, v, where))


LISTS = {
    'MASKS': R.masks_calls, 'SCORES': R.scores_calls, 'LENGTHS': R.lengths_calls, 'PACKED': R.packed_calls, 'DROPOUT': R.dropout_calls,
    'LONG': R.long_calls, 'LENGTHS3': lambda: [R.length_call(L, p) for L, p in ((1, 0.0), (33, 0.1), (192, 0.1))],
}


@pytest.mark.parametrize('which', ['MASKS', 'SCORES', 'LENGTHS', 'PACKED', 'DROPOUT'])
@pytest.mark.parametrize('fam', ['pre0', 'pre1'])
def test_fp32_general_forms(fam, which):
    """uniter_attn_fwd_pre (keep flags drawn by the kernel, and read) / uniter_attn_bwd_ex, with their bf16 copies and bias partials"""
    for call in LISTS[which]():
        judge(fam, call)
    _report(fam)


def test_fp32_piece_variants():
    """uniter_attn_fwd_pre_x3 / uniter_attn_bwd_ex_x3: the same kernels with three-piece copies of ctx and dqkv"""
    for call in LISTS['MASKS']():
        judge('pre_x3', call)
    _report('pre_x3')


def test_fp32_piece_variants_on_a_packed_batch():
    """the same pair behind cu_seqlens: the three-piece copies of ctx and dqkv land on a packed batch's rows (lengths 1 .. 192, the
    reference and the bounds of test_fp32_packed_forms)"""
    for call in LISTS['PACKED']():
        judge('pre_x3', call)
    _report('pre_x3')


@pytest.mark.parametrize('which', ['LONG', 'LENGTHS3', 'MASKS'])
def test_fp32_plain_forms(which):
    """uniter_attn_fwd / uniter_attn_bwd: L <= 192 as the general forms, to 256 the resident kernels, beyond the streaming ones (with
    UNITER_ATTN_SPLIT=0 the resident kernels from L = 1)"""
    for call in LISTS[which]():
        judge('plain', call)
    _report('plain')


def test_fp32_packed_forms():
    """uniter_attn_fwd_varlen / uniter_attn_bwd_varlen"""
    for call in LISTS['PACKED']():
        judge('varlen', call)
    _report('varlen')


@pytest.mark.parametrize('which', ['MASKS', 'SCORES', 'LENGTHS', 'PACKED', 'DROPOUT'])
def test_x3_forms(which):
    """uniter_attn_x3_fwd / uniter_attn_x3_bwd: the products on the bf16 matrix pipe, three pieces per operand"""
    for call in LISTS[which]():
        judge('x3', call)
    _report('x3')


@pytest.mark.parametrize('nslab', [3, 4])
def test_x3_dctx_slabs_are_summed_in_slab_order(nslab):
    """dctx as 3 and 4 k-pieces at a padded stride with NaN between them: bit-equal to the call on their fp32 sum taken in slab order"""
    call = R.length_call(97, 0.1)
    ref = R.reference(call)
    ops = Operands(call)
    g = torch.Generator().manual_seed(nslab)
    parts = torch.randn(nslab - 1, call.rows, call.H, generator=g)
    last = _t(call.dO) - parts.sum(0)
    pieces = torch.cat([parts, last[None]]).contiguous()
    summed = pieces[0].clone()
    for s in range(1, nslab):
        summed = summed + pieces[s]                    # fp32, slab order
    stride = call.rows * call.H + 36                   # a multiple of 4 elements, not the dense one
    slab = in_arena(pieces, 0, DEV, index=slab_index(nslab, call.rows, call.H, call.H, stride), stride=stride)
    one = in_arena(summed, 0, DEV)
    a = backward('x3', ops, ref['ctx_in'], ref['lse_in'], slabs=(slab, nslab, stride))['raw']
    b = backward('x3', ops, ref['ctx_in'], ref['lse_in'], slabs=(one, 1, 0))['raw']
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------------
# the bf16 families: the bf16-rounding reference and the bars of tests/test_attention_bf16_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------
def _bf16_run(kind, call):
    import test_attention_bf16_gpu as T
    Lb, lib = _libs()
    c = call
    ops = Operands(c)
    qkv, dO = _t(c.qkv), _t(c.dO)
    if c.packed:          # the reference works on the padded layout
        pad_q, pad_d = torch.zeros(c.B, c.L, 3 * c.H), torch.zeros(c.B, c.L, c.H)
        for b, n in enumerate(c.lens):
            pad_q[b, :n], pad_d[b, :n] = qkv[c.cu[b]:c.cu[b + 1]], dO[c.cu[b]:c.cu[b + 1]]
        ctx_ref, lse_ref, dqkv_ref, valid = T._reference(pad_q.view(-1, 3 * c.H), pad_d.view(-1, c.H), c.lens, c.B, c.L, c.nh, c.p, R.SEED,
                                                         R.OFFSET, R.SITE, emulate=False)
        dO_dev = ops.dO
    else:
        kmask = _t(c.mask)
        ctx_ref, lse_ref, dqkv_ref, valid = T._reference(qkv, dO, c.lens, c.B, c.L, c.nh, c.p, R.SEED, R.OFFSET, R.SITE, emulate=True,
                                                         kmask=kmask)
        dO_dev = in_arena(dO * kmask.view(-1, 1), 0, DEV)          # padded queries carry no gradient
    rows = torch.nonzero(valid).view(-1)
    sel = slice(None) if c.packed else rows
    m, cu = _mc(ops)
    args = (c.B, c.L, c.nh, c.p)
    rnd = (R.SEED, R.OFFSET, R.SITE)
    st = Lb.cur_stream()
    ctx, ctxb = out_arena(c.rows, c.H, 0, F32, DEV), out_arena(c.rows, c.H, 0, B16, DEV)
    lse, delta = ops.pos_out(), ops.pos_out()
    dqkv, dqkvb = out_arena(c.rows, 3 * c.H, 0, F32, DEV), out_arena(c.rows, 3 * c.H, 0, B16, DEV)
    part = out_arena(c.B, 3 * c.H, 0, F32, DEV)
    kp = P(ops.keep) if c.p > 0 else None
    if kind == 'b16x':
        Lb.check(lib.uniter_attn_b16x_fwd(P(ops.qkv), 0, m, cu, P(ctx), P(ctxb), P(lse), kp, *args, st))
    else:
        Lb.check(lib.uniter_attn_bf16_fwd_pre(P(ops.qkv), 0, m, cu, P(ctx), P(ctxb), P(lse), kp, 1 if c.p > 0 else 0, *args, *rnd, st))
    torch.cuda.synchronize()
    bad = _problems(dict(ctx=ctx, ctx_bf16=ctxb, lse=lse))
    assert not bad, (kind, c.name, bad)
    a_ctx, a_lse = in_arena(ctx.get(), 0, DEV), ops.pos_in(np.nan_to_num(ops.pos_get(lse)))
    if kind == 'b16x':
        Lb.check(lib.uniter_attn_b16x_bwd(P(ops.qkv), 0, m, cu, P(a_ctx), P(a_lse), P(dO_dev), P(dqkv), P(dqkvb), P(part), kp, P(delta),
                                          *args, st))
    else:
        wsb = lib.uniter_attn_bf16_bwd_ws_bytes(c.B, c.L, c.nh)
        ws = _offset16(max(wsb, 4) // 2, B16, float('nan'))
        Lb.check(lib.uniter_attn_bf16_bwd(P(ops.qkv), 0, m, cu, P(a_ctx), P(a_lse), P(dO_dev), P(dqkv), P(dqkvb), P(part), kp, P(delta),
                                          *args, *rnd, P(ws), wsb, st))
    torch.cuda.synchronize()
    bad = _problems(dict(dqkv=dqkv, dqkv_bf16=dqkvb, delta=delta, bias_part=part))
    assert not bad, (kind, c.name, bad)
    got_ctx, got_d = ctx.get().double().cpu()[sel], dqkv.get().double().cpu()[sel]
    cmax, cmean = T.CTX_BARS[c.packed]
    e = (got_ctx - ctx_ref[rows]).abs()
    fig = dict(ctx_max=e.max().item() / max(1.0, ctx_ref[rows].abs().max().item()) / cmax, ctx_mean=e.mean().item() / cmean)
    got_lse = ops.pos_get(lse)
    vq = valid.view(c.B, c.L).numpy()
    fig['lse'] = max(float(np.abs(got_lse[b][:, vq[b]] - lse_ref[b].numpy()[:, vq[b]]).max()) for b in range(c.B)) / T.LSE_BAR
    ref_d = dqkv_ref[rows]
    for t, name in enumerate(('dq', 'dk', 'dv')):
        sl = slice(t * c.H, (t + 1) * c.H)
        fig[name] = (got_d[:, sl] - ref_d[:, sl]).abs().max().item() / (T.DQKV_BAR * max(1.0, ref_d[:, sl].abs().max().item()))
    full, bp = dqkv.get().double().cpu(), part.get().double().cpu()
    fig['bias_part'] = max(((bp[b] - full[c.cu[b]:c.cu[b + 1]].sum(0)).abs().max().item()
                            / (T.BIAS_BAR * max(1.0, full[c.cu[b]:c.cu[b + 1]].abs().sum(0).max().item()))) for b in range(c.B))
    print('%-5s %-22s %s' % (kind, c.name, ' '.join('%s %.3f' % kv for kv in fig.items())))
    for name, v in fig.items():
        key = (kind, 'bars', name)
        if v >= WORST.get(key, (0.0, ''))[0]:
            WORST[key] = (v, c.name)
        assert v < 1.0, (kind, c.name, name, v)
    assert torch.equal(ctxb.get().cpu()[sel], ctx.get().cpu()[sel].bfloat16())
    assert torch.equal(dqkvb.get().cpu()[sel], dqkv.get().cpu()[sel].bfloat16())


@pytest.mark.parametrize('which', ['MASKS', 'PACKED'])
@pytest.mark.parametrize('kind', ['bf16', 'b16x'])
def test_bf16_forms(kind, which):
    """uniter_attn_bf16_fwd_pre / uniter_attn_bf16_bwd and uniter_attn_b16x_fwd / uniter_attn_b16x_bwd: shares of the existing bars"""
    if which == 'MASKS':
        calls = [R.masks_call(p, R.MASK_NAMES[:-1]) for p in (0.0, 0.1)]
    else:
        calls = R.packed_calls()
    for call in calls:
        _bf16_run(kind, call)
    print('\nworst shares of the bars, %s:' % kind)
    for (f, run, name), (v, where) in sorted(WORST.items()):
        if f == kind:
            print('  %-10s %.3f  (%s)' % (name, v, where))


# ---------------------------------------------------------------------------------------------------------------------------
# switches: read once per process, so the tests above run again in a child process
# ---------------------------------------------------------------------------------------------------------------------------
def _rerun(env, tests):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider'] + ['tests/test_attention_f64_gpu.py::' + t for t in tests],
                       cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-2000:])
    assert ' passed' in r.stdout and 'failed' not in r.stdout, (env, r.stdout[-500:])


def test_backward_as_two_launches_meets_the_same_bounds():
    """UNITER_ATTN_BWD_FUSED=0: the dQ and dK / dV passes of the L <= 192 backward as two launches"""
    _rerun({'UNITER_ATTN_BWD_FUSED': '0'}, ['test_fp32_general_forms'])


def test_resident_kernels_meet_the_same_bounds_at_every_length():
    """UNITER_ATTN_SPLIT=0: L <= 192 through the one-wave-per-block resident kernels (the other forms are refused under that switch)"""
    _rerun({'UNITER_ATTN_SPLIT': '0'}, ['test_fp32_plain_forms'])
