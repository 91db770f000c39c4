"""The order-fixed embedding backward (uniter_txt_embed_bwd_det / uniter_img_embed_bwd_det, csrc/embed.hip) through the C ABI:
against float64 torch references of the same operations, accumulation, exactness for a table row one token reads, bit
reproducibility, the token-type table both branches add to, and the host-side refusals.

Tolerances are those tests/test_embeddings_gpu.py holds the atomic kernels to -- 1e-5 x max |ref| per gradient, plus a few ulp of
the accumulated value where the kernel adds onto prefilled buffers: the order of the sums changes, their error's size does not.

Shapes come from the kernel's constants (tests/embed_det_ref.py repeats them): the BIG cases have 7 x 41 = 287 text rows and
9 x 33 = 297 regions, more than the 256 rows one workgroup ranks (RANK_WG), and every token on one word id / two token types, so one
segment holds far more ranked rows than a chunk of 32 (CHUNK) and spans nine chunks; the regions' 297 rows are ten 32-row partial
sums of the position projection's weight gradient (WG_ROWS).  B * T = 21 and 287 are no multiples of 4."""
import functools

import pytest
import torch

import embed_det_ref as R
from oracle import philox
from oracle import uniter_oracle as O

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x1234ABCD5678, 11
BWD = 1e-5
VOCAB, MAX_POS, TV = 50, 40, 2
BIG_TXT, BIG_IMG = (7, 41), (9, 33)
assert BIG_TXT[0] * BIG_TXT[1] > R.RANK_WG and BIG_IMG[0] * BIG_IMG[1] > R.RANK_WG and BIG_TXT[0] * BIG_TXT[1] > 2 * R.CHUNK
TXT_NAMES = ('word', 'pos', 'type', 'gamma', 'beta')
IMG_NAMES = ('Wp', 'bp', 'type', 'dg_i', 'db_i', 'dg_p', 'db_p', 'dg_f', 'db_f')


def _L():
    from meme_challenge_amd import _lib
    return _lib


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _close(got, ref, rel, what, pre=None, times=1):
    """|got - (pre + times * ref)| <= times * rel * max |ref| (+ a few ulp of the accumulated value when the kernel adds onto pre)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double() * times
    exp = ref if pre is None else pre.double() + ref
    tol = rel * ref.abs().max().item() + (0.0 if pre is None else times * 2.0 ** -20 * exp.abs().max().item())
    err = (got - exp).abs().max().item()
    assert err <= tol, (what, err, tol)


def _drop(p):
    return O.DropSpec(SEED, OFFSET, p, p) if p > 0 else None


def _ws(txt_rows, img_rows, H):
    n = _L().lib().uniter_embed_bwd_det_ws_bytes(txt_rows, img_rows, H)
    return torch.empty(max(n, 1), dtype=torch.uint8, device='cuda'), n


# ---------------------------------------------------------------------------------------------------------------------------
# text
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _txt_problem(H, BT=(3, 7), ids='mixed', pos='own', types=None, pos_bcast=0, p=0.0):
    """inputs (CPU), the float64 gradients of the same math, and prefilled gradient buffers; built once per case and not modified"""
    B, T = BT
    n = B * T
    g = torch.Generator().manual_seed(H * 131 + n * 17 + len(ids) + 7 * len(str(types)) + 3 * pos_bcast + int(p * 10))
    if ids == 'same':                                                              # every token on one table row
        tok = torch.full((B, T), 23, dtype=torch.int64)
    elif ids == 'single':                                                          # id 37 and position 33 are read by row 5 alone
        tok = torch.randint(1, 30, (B, T), generator=g)
        tok.view(-1)[5] = 37
    else:                                                                          # padding, ids below 0 and at / above the vocabulary
        tok = torch.randint(0, VOCAB, (B, T), generator=g)
        tok.view(-1)[:6] = torch.tensor([0, -3, VOCAB, VOCAB + 7, VOCAB - 1, 0])
        tok.view(-1)[-1] = -(1 << 40)
    if pos == 'shared':                                                            # every position is shared by all samples
        pos_ids = (torch.arange(T) % MAX_POS).expand(1 if pos_bcast else B, T).contiguous()
    else:
        pos_ids = torch.randint(0, 30 if ids == 'single' else MAX_POS, (1 if pos_bcast else B, T), generator=g)
        if ids == 'single':
            assert not pos_bcast
            pos_ids.view(-1)[5] = 33
        else:
            pos_ids.view(-1)[:3] = torch.tensor([-2, MAX_POS + 5, MAX_POS - 1])   # clamped as in the forward
    type_ids = None
    if types == 'equal':
        type_ids = torch.ones(B, T, dtype=torch.int64)
    elif types == 'mixed':
        type_ids = torch.randint(0, TV, (B, T), generator=g)
        type_ids.view(-1)[:4] = torch.tensor([0, 1, -1, TV + 2])
    word = torch.randn(VOCAB, H, generator=g)
    posw, typ = 0.5 * torch.randn(MAX_POS, H, generator=g), 0.5 * torch.randn(TV, H, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    par = dict(word=word.float(), pos=posw.float(), type=typ.float(), gamma=gamma.float(), beta=beta.float())
    S = T + 3
    dcat = torch.randn(B, S, H, generator=g)
    leaves = {k: t.double().requires_grad_(True) for k, t in par.items()}
    sd = {'embeddings.word_embeddings.weight': leaves['word'], 'embeddings.position_embeddings.weight': leaves['pos'],
          'embeddings.token_type_embeddings.weight': leaves['type'], 'embeddings.LayerNorm.weight': leaves['gamma'],
          'embeddings.LayerNorm.bias': leaves['beta']}
    ref = O.text_embeddings(sd, '', tok.clamp(0, VOCAB - 1), pos_ids.clamp(0, MAX_POS - 1).expand(B, T),
                            None if type_ids is None else type_ids.clamp(0, TV - 1), {'hidden_dropout_prob': p}, _drop(p))
    ref.backward(dcat[:, :T].double())
    grads = {k: leaves[k].grad.clone() for k in TXT_NAMES}
    grads['word'][0] = 0                                                          # padding_idx = 0
    pre = {k: (torch.randn(*par[k].shape, generator=g) * 0.5).float() for k in TXT_NAMES}
    return dict(B=B, T=T, S=S, H=H, ids=tok, pos_ids=pos_ids, type_ids=type_ids, par=par, dcat=dcat, grads=grads, pre=pre,
                pos_bcast=pos_bcast, p=p)


def _run_txt(q, bufs, ws=None):
    """one backward call on the gradient buffers `bufs` (device tensors by TXT_NAMES); returns the error code"""
    L = _L()
    lib, ptr = L.lib(), L.ptr
    B, T, H = q['B'], q['T'], q['H']
    d = q.setdefault('_dev', {})
    if not d:
        d.update(ids=_dev(q['ids']), pos=_dev(q['pos_ids']), typ=_dev(q['type_ids']), dcat=_dev(q['dcat']),
                 **{'p_' + k: _dev(t) for k, t in q['par'].items()})
    if ws is None:
        ws = _ws(B * T, 0, H)
    rc = lib.uniter_txt_embed_bwd_det(ptr(d['dcat']), ptr(d['ids']), ptr(d['pos']), ptr(d['typ']), ptr(d['p_word']), ptr(d['p_pos']), ptr(d['p_type']),
            ptr(d['p_gamma']), *[ptr(bufs[k]) for k in TXT_NAMES], B, T, q['S'], H, VOCAB, MAX_POS, TV, q['pos_bcast'], q['p'],
            SEED, OFFSET, ptr(ws[0]), ws[1], L.cur_stream())
    return rc


def _txt_cases():
    cases = [dict(H=H) for H in (128, 768, 1024)]
    cases += [dict(H=H, ids='same', pos='shared', pos_bcast=1, types='equal') for H in (128, 768, 1024)]      # heavy collisions
    cases += [dict(H=768, pos_bcast=1), dict(H=768, types='equal'), dict(H=768, types='mixed'), dict(H=128, p=0.1),
              dict(H=1024, types='mixed', pos_bcast=1, p=0.1),
              dict(H=128, BT=BIG_TXT, ids='same', pos='shared', types='mixed'),
              dict(H=128, BT=BIG_TXT, types='mixed', pos_bcast=1, p=0.1),
              dict(H=768, BT=BIG_TXT, ids='same', pos='shared', pos_bcast=1)]
    return [pytest.param(c, id='-'.join('%s=%s' % kv for kv in c.items())) for c in cases]


@pytest.mark.parametrize('case', _txt_cases())
def test_text_table_gradients_match_float64_and_accumulate(case):
    L = _L()
    q = _txt_problem(**case)
    got = {k: _dev(t) for k, t in q['pre'].items()}
    L.check(_run_txt(q, got))
    torch.cuda.synchronize()
    once = {k: t.cpu() for k, t in got.items()}
    for k in TXT_NAMES:
        _close(once[k], q['grads'][k], BWD, 'd' + k, q['pre'][k])
    # rows no token reads are bit-unchanged: the padding row (ids 0 and below), unused words / positions / types
    used = R.keys_of(q['ids'].numpy(), VOCAB)
    untouched = torch.ones(VOCAB, dtype=torch.bool)
    untouched[torch.from_numpy(used)] = False
    untouched[0] = True
    assert torch.equal(once['word'][untouched], q['pre']['word'][untouched])
    unused_pos = torch.ones(MAX_POS, dtype=torch.bool)
    unused_pos[q['pos_ids'].clamp(0, MAX_POS - 1).view(-1)] = False
    assert torch.equal(once['pos'][unused_pos], q['pre']['pos'][unused_pos])
    if q['type_ids'] is None:
        assert torch.equal(once['type'][1], q['pre']['type'][1])
    elif case.get('types') == 'equal':
        assert torch.equal(once['type'][0], q['pre']['type'][0])
    # a second call adds again
    L.check(_run_txt(q, got))
    torch.cuda.synchronize()
    for k in TXT_NAMES:
        _close(got[k], q['grads'][k], BWD, 'd%s twice' % k, q['pre'][k], times=2)
    assert torch.equal(got['word'].cpu()[untouched], q['pre']['word'][untouched])


def test_a_table_row_one_token_reads_receives_that_rows_gradient_exactly():
    """Single owner: word id 37 and position 33 are read by row 5 alone, so their gradient rows are prior + d(row 5) bit for bit;
    d(row 5) comes from a one-row launch of the same row into zeroed buffers (a row's arithmetic does not depend on the others)."""
    L = _L()
    q = _txt_problem(H=768, BT=BIG_TXT, ids='single', types='mixed')
    got = {k: _dev(t) for k, t in q['pre'].items()}
    L.check(_run_txt(q, got))
    B, T, S, H = q['B'], q['T'], q['S'], q['H']
    b, t = divmod(5, T)
    one = dict(q, B=1, T=1, S=1, ids=q['ids'][b:b + 1, t:t + 1], pos_ids=q['pos_ids'][b:b + 1, t:t + 1],
               type_ids=q['type_ids'][b:b + 1, t:t + 1], dcat=q['dcat'][b:b + 1, t:t + 1], _dev={})
    d = {k: torch.zeros_like(v).cuda() for k, v in q['pre'].items()}
    L.check(_run_txt(one, d))
    torch.cuda.synchronize()
    assert d['word'][37].abs().max().item() > 0
    assert torch.equal(d['word'][37], d['pos'][33])
    assert torch.equal(got['word'][37].cpu(), q['pre']['word'][37] + d['word'][37].cpu())
    assert torch.equal(got['pos'][33].cpu(), q['pre']['pos'][33] + d['pos'][33].cpu())


def _busy_copy():
    """a large copy on another stream, in flight while the caller's launches run"""
    side = torch.cuda.Stream()
    src = torch.empty(256 << 20, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    with torch.cuda.stream(side):
        for _ in range(4):
            dst.copy_(src, non_blocking=True)
    return side, (src, dst)


@pytest.mark.parametrize('case', [dict(H=128, BT=BIG_TXT, ids='same', pos='shared', types='mixed'),
                                  dict(H=768, types='mixed', pos_bcast=1, p=0.1)], ids=['big', 'small'])
def test_text_gradients_are_the_same_bits_run_after_run(case):
    L = _L()
    q = _txt_problem(**case)
    runs = []
    for i in range(3):
        got = {k: _dev(t) for k, t in q['pre'].items()}
        torch.cuda.synchronize()
        keep = _busy_copy() if i == 2 else None
        L.check(_run_txt(q, got))
        torch.cuda.synchronize()
        runs.append({k: t.cpu() for k, t in got.items()})
        del keep
    for k in TXT_NAMES:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# image
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _img_problem(H, BR=(3, 7), types=None, p=0.0, T0=3):
    B, Rg = BR
    n = B * Rg
    g = torch.Generator().manual_seed(H * 71 + n * 13 + 5 * len(str(types)) + int(p * 10) + T0)
    imgfc = (torch.randn(n, H, generator=g) * (1.0 + torch.rand(n, 1, generator=g))).float()
    pos7 = torch.rand(n, 7, generator=g).float()
    Wp, bp = (0.5 * torch.randn(H, 7, generator=g)).float(), (0.1 * torch.randn(H, generator=g)).float()
    typ = (0.5 * torch.randn(TV, H, generator=g)).float()
    aff = [(1.0 + 0.1 * torch.randn(H, generator=g) if i % 2 == 0 else 0.1 * torch.randn(H, generator=g)).float() for i in range(6)]
    type_ids = None
    if types == 'mixed':
        type_ids = torch.randint(0, TV, (n,), generator=g)
        type_ids[:4] = torch.tensor([0, 1, -4, TV + 1])                            # clamped as in the forward
    elif types == 'equal':
        type_ids = torch.zeros(n, dtype=torch.int64)
    S = T0 + Rg + 2
    dcat = torch.randn(B, S, H, generator=g)
    x = imgfc.double().requires_grad_(True)
    Wp64, bp64, typ64 = (t.double().requires_grad_(True) for t in (Wp, bp, typ))
    aff64 = [t.double().requires_grad_(True) for t in aff]
    qq = pos7.double() @ Wp64.t() + bp64
    tid = type_ids.clamp(0, TV - 1) if type_ids is not None else torch.ones(n, dtype=torch.int64)
    f = O.layer_norm(x, aff64[0], aff64[1]) + O.layer_norm(qq, aff64[2], aff64[3]) + typ64[tid]
    e = O.layer_norm(f, aff64[4], aff64[5])
    ref = O._apply_dropout(e.view(B, Rg, H), p, _drop(p), philox.SITE_IMG_EMB)
    ref.backward(dcat[:, T0:T0 + Rg].double())

    def stats64(z):
        z = z.detach()
        return z.mean(-1), 1.0 / torch.sqrt(z.var(-1, unbiased=False) + 1e-12)
    stats = torch.stack([*stats64(x), *stats64(qq), *stats64(f)], 1).float()      # what the forward saves (to fp32 round-off)
    grads = dict(Wp=Wp64.grad, bp=bp64.grad, type=typ64.grad,
                 **{k: aff64[i].grad for i, k in enumerate(('dg_i', 'db_i', 'dg_p', 'db_p', 'dg_f', 'db_f'))})
    shapes = dict(Wp=Wp.shape, bp=bp.shape, type=typ.shape, **{k: (H,) for k in IMG_NAMES[3:]})
    pre = {k: (torch.randn(*shapes[k], generator=g) * 0.5).float() for k in IMG_NAMES}
    return dict(B=B, R=Rg, T0=T0, S=S, H=H, imgfc=imgfc, pos7=pos7, type_ids=type_ids, Wp=Wp, bp=bp, typ=typ, aff=aff, stats=stats,
                dcat=dcat, grads=grads, pre=pre, p=p, dx=x.grad)


def _run_img(q, bufs):
    L = _L()
    lib, ptr = L.lib(), L.ptr
    B, Rg, H = q['B'], q['R'], q['H']
    n = B * Rg
    d = q.setdefault('_dev', {})
    if not d:
        d.update({k: _dev(q[k]) for k in ('imgfc', 'pos7', 'type_ids', 'Wp', 'bp', 'typ', 'stats', 'dcat')})
        d['aff'] = [_dev(t) for t in q['aff']]
    d_imgfc = torch.full((n, H), float('nan'), device='cuda')
    d_posfc = torch.full((n, H), float('nan'), device='cuda')
    ws = _ws(0, n, H)
    rc = lib.uniter_img_embed_bwd_det(ptr(d['dcat']), ptr(d['imgfc']), ptr(d['pos7']), ptr(d['type_ids']), ptr(d['Wp']), ptr(d['bp']), ptr(d['typ']),
            *[ptr(t) for t in d['aff'][:5]], ptr(d['stats']), ptr(d_imgfc), ptr(d_posfc), *[ptr(bufs[k]) for k in IMG_NAMES],
            B, Rg, q['T0'], q['S'], H, TV, q['p'], SEED, OFFSET, ptr(ws[0]), ws[1], L.cur_stream())
    return rc, d_imgfc


def _img_cases():
    cases = [dict(H=H) for H in (128, 768, 1024)] + [dict(H=H, types='mixed') for H in (128, 768, 1024)]
    cases += [dict(H=768, types='equal'), dict(H=128, p=0.1), dict(H=768, types='mixed', p=0.1, T0=0),
              dict(H=128, BR=BIG_IMG, types='mixed'), dict(H=768, BR=BIG_IMG), dict(H=1024, BR=BIG_IMG, types='mixed', p=0.1)]
    return [pytest.param(c, id='-'.join('%s=%s' % kv for kv in c.items())) for c in cases]


@pytest.mark.parametrize('case', _img_cases())
def test_image_gradients_match_float64_and_accumulate(case):
    L = _L()
    q = _img_problem(**case)
    got = {k: _dev(t) for k, t in q['pre'].items()}
    rc, d_imgfc = _run_img(q, got)
    L.check(rc)
    torch.cuda.synchronize()
    _close(d_imgfc, q['dx'], BWD, 'd_imgfc')
    once = {k: t.cpu() for k, t in got.items()}
    for k in IMG_NAMES:
        _close(once[k], q['grads'][k], BWD, k, q['pre'][k])
    if q['type_ids'] is None:
        assert torch.equal(once['type'][0], q['pre']['type'][0])
    elif case.get('types') == 'equal':
        assert torch.equal(once['type'][1], q['pre']['type'][1])
    L.check(_run_img(q, got)[0])
    torch.cuda.synchronize()
    for k in IMG_NAMES:
        _close(got[k], q['grads'][k], BWD, k + ' twice', q['pre'][k], times=2)


def test_image_gradients_are_the_same_bits_run_after_run():
    L = _L()
    q = _img_problem(H=1024, BR=BIG_IMG, types='mixed', p=0.1)
    runs = []
    for i in range(3):
        got = {k: _dev(t) for k, t in q['pre'].items()}
        torch.cuda.synchronize()
        keep = _busy_copy() if i == 2 else None
        L.check(_run_img(q, got)[0])
        torch.cuda.synchronize()
        runs.append({k: t.cpu() for k, t in got.items()})
        del keep
    for k in IMG_NAMES:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# the token-type table both branches add to
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('img_types', [None, 'mixed'])
def test_token_type_table_is_text_share_then_image_share(img_types):
    """Both branches add to type row 1 (the text rows with explicit ids, the regions implicitly or with ids of their own): text then
    image on one stream gives (prior + text share) + image share, the shares being what each call adds to a zeroed table."""
    L = _L()
    H = 768
    qt = _txt_problem(H=H, BT=BIG_TXT, ids='same', pos='shared', types='mixed')
    qi = _img_problem(H=H, BR=BIG_IMG, types=img_types)
    g = torch.Generator().manual_seed(4)
    prior = (torch.randn(TV, H, generator=g) * 0.5).float()

    def bufs(q, dtype):
        b = {k: torch.zeros_like(v).cuda() for k, v in q['pre'].items()}
        b['type'] = dtype
        return b

    share_t, share_i = torch.zeros(TV, H, device='cuda'), torch.zeros(TV, H, device='cuda')
    L.check(_run_txt(qt, bufs(qt, share_t)))
    L.check(_run_img(qi, bufs(qi, share_i))[0])
    results = []
    for _ in range(2):
        both = prior.clone().cuda()
        L.check(_run_txt(qt, bufs(qt, both)))
        L.check(_run_img(qi, bufs(qi, both))[0])
        torch.cuda.synchronize()
        results.append(both.cpu())
    assert share_t[1].abs().max().item() > 0 and share_i[1].abs().max().item() > 0
    assert torch.equal(results[0], (prior + share_t.cpu()) + share_i.cpu())
    assert torch.equal(results[0], results[1])


def test_model_backward_embed_with_explicit_type_ids_is_reproducible_with_the_auxiliary_stream():
    """Through uniter_model_backward_embed, side and auxiliary streams on, explicit token-type ids on both sides: the two branches
    run on one stream, text then image, and every embedding gradient is the same bits in three runs (precision fp32x3, whose
    input-gradient chain has no atomics)."""
    from common import TINY, TINY_IMG_DIM, model_kwargs
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.trainer import bce_with_logits_loss
    from meme_challenge_amd.utils import make_synthetic_batch
    torch.manual_seed(0)
    m = MemeUniter(UniterModel(UniterConfig.from_dict(TINY), img_dim=TINY_IMG_DIM), TINY['hidden_size'], 1).cuda().train()
    m.uniter_model.precision, m.uniter_model.deterministic = 'fp32x3', True
    assert m.uniter_model.use_side_stream
    B, T, Rg = 4, 16, 6
    b = make_synthetic_batch(B, T, Rg, seed=3, device='cuda', vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM)
    g = torch.Generator().manual_seed(1)
    kw = dict(model_kwargs(b), txt_type_ids=torch.randint(0, 2, (B, T), generator=g).cuda(),
              img_type_ids=torch.randint(0, 2, (B, Rg), generator=g).cuda())
    runs = []
    for _ in range(3):
        m.uniter_model.set_dropout_seed(11, 0)
        m.zero_grad(set_to_none=False)
        m.param_store().zero_grads()
        bce_with_logits_loss(m(**kw).squeeze(1), b['labels'], 1.8).backward()
        torch.cuda.synchronize()
        runs.append({n: p_.grad.clone() for n, p_ in m.uniter_model.named_parameters()
                     if n.startswith(('embeddings.', 'img_embeddings.')) and p_.grad is not None})
    assert len(runs[0]) >= 14 and runs[0]['embeddings.token_type_embeddings.weight'].abs().amax(1).min().item() > 0
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]) and torch.equal(runs[0][n], runs[2][n]), n


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: host-side checks, nothing launched
# ---------------------------------------------------------------------------------------------------------------------------
def test_det_entry_points_refuse_too_many_rows_and_a_short_workspace():
    L = _L()
    lib = L.lib()
    q = _txt_problem(H=128)
    qi = _img_problem(H=128)
    got = {k: _dev(t) for k, t in q['pre'].items()}
    goti = {k: _dev(t) for k, t in qi['pre'].items()}
    ws, n = _ws(q['B'] * q['T'], 0, 128)
    assert _run_txt(q, got, ws=(ws, n - 1)) == -1 and b'txt_embed_bwd_det: workspace' in lib.uniter_last_error()
    over = dict(q, B=R.MAX_ROWS + 1, T=1, S=1)                                     # refused before anything reads the buffers
    assert _run_txt(over, got, ws=(ws, 1 << 40)) == -2 and b'rows' in lib.uniter_last_error()
    assert lib.uniter_embed_bwd_det_ws_bytes(R.MAX_ROWS, 0, 1024) > 0              # the limit itself is served
    overi = dict(qi, B=R.MAX_ROWS // 4 + 1, R=4, S=qi['T0'] + 4)
    need = lib.uniter_embed_bwd_det_ws_bytes
    assert _run_img(overi, goti)[0] == -2 and b'img_embed_bwd_det' in lib.uniter_last_error()
    P = L.ptr(ws)
    assert lib.uniter_img_embed_bwd_det(P, P, P, None, *[P] * 20, 2, 3, 1, 4, 128, 2, 0.0, 1, 0, P,
                                        need(0, 6, 128) - 1, L.cur_stream()) == -1
    assert b'img_embed_bwd_det: workspace' in lib.uniter_last_error()
    torch.cuda.synchronize()
    for k in TXT_NAMES:
        assert torch.equal(got[k].cpu(), q['pre'][k]), k
    for k in IMG_NAMES:
        assert torch.equal(goti[k].cpu(), qi['pre'][k]), k
