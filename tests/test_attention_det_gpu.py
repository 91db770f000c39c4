"""GPU: the attention backward kernels' per-sample query|key|value bias partials in a fixed order (uniter_attn_bwd_set_next_det): every
backward family through the C ABI with the flag set gives the same bits call after call, the partials are the column sums of dqkv
at the existing bar, and nothing else the call writes changes by a bit.

(Not asserted: that the default path differs from run to run -- its LDS atomics usually arrive in the same order.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, OFFSET, SITE = 0xABCDEF0123, 5, 2
FAMILIES = ['x3', 'b16x', 'ex', 'bf16']
# (lengths per sample or None, B, L, nh, p): 7 waves of 16 rows contribute at L = 100 (4 merged 32-row blocks in the fp32 / bf16 files),
# 12 at L = 192, 3 at L = 33 in a 48-row workgroup; the packed batch has a full-length sample, a one-row sample and two between
SHAPES = [(None, 2, 100, 2, 0.1), (None, 2, 192, 2, 0.0), (None, 3, 33, 1, 0.1), ([164, 40, 1, 97], 4, 164, 2, 0.1)]


def _run(family, lens, B, L, nh, p, det, calls):
    from meme_challenge_amd import _lib as Lb
    lib = Lb.lib()
    H = nh * 64
    g = torch.Generator().manual_seed(B * 1000 + L)
    if lens is None:
        rows = B * L
        mask = torch.ones(B, L)
        for b in range(1, B):
            mask[b, L - (b * 7) % L:] = 0
        dm, cu = mask.cuda(), None
        spans = [(b * L, L) for b in range(B)]
    else:
        rows = sum(lens)
        offs = [0]
        for n in lens:
            offs.append(offs[-1] + n)
        dm, cu = None, torch.tensor(offs, dtype=torch.int32).cuda()
        spans = [(offs[b], lens[b]) for b in range(B)]
    qkv = torch.randn(rows, 3 * H, generator=g).cuda()
    dctx = torch.randn(rows, H, generator=g).cuda()
    keep = torch.zeros(max(lib.uniter_attn_keep_bits_bytes(B, L, nh), 2) // 2, dtype=torch.int16, device='cuda')
    if p > 0:
        Lb.check(lib.uniter_attn_keep_bits_gen(Lb.ptr(keep), 0, 1, B, L, nh, p, SEED, OFFSET, SITE, 0, Lb.cur_stream()))
    kp = Lb.ptr(keep) if p > 0 else None
    ctx = torch.zeros(rows, H, device='cuda')
    lse = torch.zeros(B, nh, L, device='cuda')
    Lb.check(lib.uniter_attn_x3_fwd(Lb.ptr(qkv), Lb.ptr(dm), Lb.ptr(cu), Lb.ptr(ctx), None, Lb.ptr(lse), kp, B, L, nh, p, Lb.cur_stream()))
    wsb = max(lib.uniter_attn_bwd_ws_bytes(B, L, nh), lib.uniter_attn_bf16_bwd_ws_bytes(B, L, nh))
    ws = torch.zeros(max(wsb, 4) // 4, device='cuda')
    outs = []
    for _ in range(calls):
        nan = float('nan')
        dqkv = torch.full((rows, 3 * H), nan, device='cuda')
        copy = torch.full((rows, 3, 3 * H) if family == 'x3' else (rows, 3 * H), nan, dtype=torch.bfloat16, device='cuda')
        part = torch.full((B, 3 * H), nan, device='cuda')
        delta = torch.zeros(B, nh, L, device='cuda')
        if det:
            Lb.check(lib.uniter_attn_bwd_set_next_det(1))
        a = (Lb.ptr(dm), Lb.ptr(cu), Lb.ptr(ctx), Lb.ptr(lse), Lb.ptr(dctx))
        tail = (B, L, nh, p, SEED, OFFSET, SITE, Lb.ptr(ws), wsb, Lb.cur_stream())
        if family == 'x3':
            rc = lib.uniter_attn_x3_bwd(Lb.ptr(qkv), *a, 1, 0, Lb.ptr(dqkv), Lb.ptr(copy), Lb.ptr(part), kp, Lb.ptr(delta), B, L, nh, p,
                                        Lb.cur_stream())
        elif family == 'b16x':
            rc = lib.uniter_attn_b16x_bwd(Lb.ptr(qkv), 0, *a, Lb.ptr(dqkv), Lb.ptr(copy), Lb.ptr(part), kp, Lb.ptr(delta), B, L, nh, p,
                                          Lb.cur_stream())
        elif family == 'ex':
            rc = lib.uniter_attn_bwd_ex(Lb.ptr(qkv), *a, Lb.ptr(dqkv), Lb.ptr(copy), Lb.ptr(part), Lb.ptr(keep), Lb.ptr(delta), *tail)
        else:
            rc = lib.uniter_attn_bf16_bwd(Lb.ptr(qkv), 0, *a, Lb.ptr(dqkv), Lb.ptr(copy), Lb.ptr(part), Lb.ptr(keep), Lb.ptr(delta), *tail)
        Lb.check(rc, family)
        torch.cuda.synchronize()
        outs.append((dqkv, copy, delta, part))
    return outs, spans


@pytest.mark.parametrize('lens,B,L,nh,p', SHAPES)
@pytest.mark.parametrize('family', FAMILIES)
def test_bias_partials_in_a_fixed_order(family, lens, B, L, nh, p):
    (plain,), spans = _run(family, lens, B, L, nh, p, det=False, calls=1)
    det, _ = _run(family, lens, B, L, nh, p, det=True, calls=5)
    dqkv, copy, delta, part = det[0]
    # 1. everything but the partials: the same bits as the call without the flag
    assert torch.isfinite(dqkv).all() and torch.isfinite(part).all()
    assert torch.equal(dqkv, plain[0]) and torch.equal(copy.view(torch.int16), plain[1].view(torch.int16)) and torch.equal(delta, plain[2])
    # 2. the partials are the per-sample column sums of dqkv: the existing bar, 1e-4 * max(1, |colsum|)
    colsum = torch.stack([dqkv[r0:r0 + n].double().sum(0) for r0, n in spans])
    bar = 1e-4 * max(1.0, colsum.abs().max().item())
    err = (part.double() - colsum).abs().max().item()
    err_plain = (plain[3].double() - colsum).abs().max().item()
    print('%s %s: |partials - colsum| det %.3g, default %.3g, bar %.3g' % (family, (lens, B, L, nh, p), err, err_plain, bar))
    assert err < bar and err_plain < bar
    # 3. the same bits in five calls
    for other in det[1:]:
        assert torch.equal(other[3], part)
        assert torch.equal(other[0], dqkv) and torch.equal(other[2], delta)


def test_the_flag_is_taken_by_one_call():
    """the setter returns 0 and arms ONE call: a second backward call without it runs the default kernel, whose results the first
    checks already bound; here only that setting and clearing it by hand is accepted and leaves a working default call"""
    from meme_challenge_amd import _lib as Lb
    lib = Lb.lib()
    assert lib.uniter_attn_bwd_set_next_det(1) == 0 and lib.uniter_attn_bwd_set_next_det(0) == 0
    (plain,), spans = _run('x3', None, 2, 40, 1, 0.0, det=False, calls=1)
    det, _ = _run('x3', None, 2, 40, 1, 0.0, det=True, calls=1)
    assert torch.equal(plain[0], det[0][0])
    assert (plain[3] - det[0][3]).abs().max().item() < 1e-4 * max(1.0, plain[3].abs().max().item())
