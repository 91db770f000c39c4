"""The input-gradient kernels (csrc/input_grads.hip and the perturbed instantiation of the text row kernel in csrc/embed.hip) through
the C ABI against float64 torch: the text embedding forward with an additive perturbation, the per-token gradient of the sum that
enters its LayerNorm, the 7-column position-feature gradient, the ascent / projection step of an adversarial perturbation (csrc/adv.hip), and the
host-side refusals.

The perturbation is restated for the oracle as a word table of B * T rows, word[ids[b, t]] + delta[b, t], with
input_ids = arange(B * T): that table's gradient is the per-token gradient.

Tolerances are the ones tests/test_embeddings_gpu.py derives for the same fp32 arithmetic against float64: FWD = 4e-6 x max |ref|
for forward rows of unit scale, BWD = 1e-5 x max |ref| for a gradient, ILL = 2e-3 for rows whose LayerNorm input is nearly constant.
The position gradient is a sum of H products per element, the same kind of sum as the gradients BWD was derived for.  The
perturbation's step is elementwise fp32 on top of norms reduced in double: FWD."""
import pytest
import torch

from oracle import uniter_oracle as O

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x1234ABCD5678, 11
FWD, BWD, ILL = 4e-6, 1e-5, 2e-3


def _L():
    from meme_challenge_amd import _lib
    return _lib


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _close(got, ref, rel, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    tol = rel * ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print('%s: err %.3e tol %.3e' % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _drop(p):
    return O.DropSpec(SEED, OFFSET, p, p) if p > 0 else None


# ---------------------------------------------------------------------------------------------------------------------------
# text forward with a perturbation, and the per-token gradient
# ---------------------------------------------------------------------------------------------------------------------------
def _txt_cases():
    cases = []
    for H in (4, 64, 260, 768, 1024):
        for bt in ((1, 1), (5, 1), (4, 33)):
            cases.append(dict(H=H, BT=bt))
        cases += [dict(H=H, BT=(4, 33), types=True), dict(H=H, BT=(4, 33), pos_bcast=1), dict(H=H, BT=(4, 33), p=0.1),
                  dict(H=H, BT=(4, 33), types=True, pos_bcast=1, p=0.1)]
    for H in (260, 768):
        cases += [dict(H=H, BT=(4, 33), ids='same'), dict(H=H, BT=(4, 33), ids='zeros', p=0.1), dict(H=H, BT=(4, 33), ids='distinct', p=0.1),
                  dict(H=H, BT=(4, 33), ids='distinct', types=True), dict(H=H, BT=(4, 33), cond='ill')]
    return [pytest.param(c, id='-'.join('%s=%s' % kv for kv in c.items())) for c in cases]


class _Txt(object):
    """one case's inputs on the host and on the device"""

    def __init__(self, case):
        H, (B, T) = case['H'], case['BT']
        types, pos_bcast, p = case.get('types', False), case.get('pos_bcast', 0), case.get('p', 0.0)
        kind, ill = case.get('ids', 'random'), case.get('cond') == 'ill'
        g = torch.Generator().manual_seed(H * 131 + B * 17 + T + 7 * types + 3 * pos_bcast + int(p * 10) + len(kind) + 50 * ill)
        n = B * T
        vocab, max_pos, tv, S = max(50, n + 1), 96, 2, T + 3
        if kind == 'same':
            ids = torch.full((B, T), 23, dtype=torch.int64)
        elif kind == 'distinct':                                                  # all different, none the padding row
            ids = (torch.randperm(vocab - 1, generator=g)[:n] + 1).view(B, T)
        else:
            ids = torch.randint(0, vocab, (B, T), generator=g)
            if kind == 'zeros':
                ids.view(-1)[::3] = 0
            if n > 1:
                ids.view(-1)[0] = 0                                               # a padding id still gets its row's gradient
                ids.view(-1)[-1] = vocab - 1
        pos_ids = torch.randint(0, max_pos, (T,) if pos_bcast else (B, T), generator=g)
        pos_ids.view(-1)[-1] = max_pos - 1
        type_ids = torch.randint(0, tv, (B, T), generator=g) if types else None
        if ill:
            word = 1.0 + 1e-3 * torch.randn(vocab, H, generator=g)
            pos, typ = 5e-4 * torch.randn(max_pos, H, generator=g), 5e-4 * torch.randn(tv, H, generator=g)
            delta = 5e-4 * torch.randn(B, T, H, generator=g)
        else:
            word = torch.randn(vocab, H, generator=g)
            pos, typ = 0.5 * torch.randn(max_pos, H, generator=g), 0.5 * torch.randn(tv, H, generator=g)
            delta = 0.3 * torch.randn(B, T, H, generator=g)
        gamma, beta = 1.0 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
        self.word, self.pos, self.typ, self.gamma, self.beta, self.delta = (t.float() for t in (word, pos, typ, gamma, beta, delta))
        self.dcat = torch.randn(B, S, H, generator=g)
        self.ids, self.pos_ids, self.type_ids = ids, pos_ids, type_ids
        self.B, self.T, self.S, self.H, self.vocab, self.max_pos, self.tv = B, T, S, H, vocab, max_pos, tv
        self.pos_bcast, self.p, self.ill, self.kind = pos_bcast, p, ill, kind
        self.d = {k: _dev(getattr(self, k)) for k in ('ids', 'pos_ids', 'type_ids', 'word', 'pos', 'typ', 'gamma', 'beta', 'delta', 'dcat')}

    def reference(self, delta):
        """float64 oracle on the per-token table word[ids] + delta: the forward rows and that table's gradient"""
        B, T = self.B, self.T
        rows = (self.word[self.ids.view(-1)].double() + delta.double().view(B * T, -1)).requires_grad_(True)
        sd = {'embeddings.word_embeddings.weight': rows, 'embeddings.position_embeddings.weight': self.pos.double(),
              'embeddings.token_type_embeddings.weight': self.typ.double(), 'embeddings.LayerNorm.weight': self.gamma.double(),
              'embeddings.LayerNorm.bias': self.beta.double()}
        ref = O.text_embeddings(sd, '', torch.arange(B * T).view(B, T), self.pos_ids.expand(B, T) if self.pos_bcast else self.pos_ids,
                                self.type_ids, {'hidden_dropout_prob': self.p}, _drop(self.p))
        ref.backward(self.dcat[:, :T].double())
        return ref.detach(), rows.grad.view(B, T, -1)

    def fwd(self, delta, word=None):
        L = _L()
        lib, ptr, d = L.lib(), L.ptr, self.d
        cat = torch.full((self.B, self.S, self.H), float('nan'), device='cuda')
        common = (self.B, self.T, self.S, self.H, self.vocab, self.max_pos, self.tv, self.pos_bcast, self.p, SEED, OFFSET, L.cur_stream())
        head = (ptr(d['ids']), ptr(d['pos_ids']), ptr(d['type_ids']), ptr(word if word is not None else d['word']), ptr(d['pos']),
                ptr(d['typ']), ptr(d['gamma']), ptr(d['beta']))
        if delta is False:
            L.check(lib.uniter_txt_embed_fwd(*head, ptr(cat), *common), 'uniter_txt_embed_fwd')
        else:
            L.check(lib.uniter_txt_embed_fwd_delta(*head, ptr(delta), ptr(cat), *common), 'uniter_txt_embed_fwd_delta')
        torch.cuda.synchronize()
        return cat.cpu()

    def bwd_rows(self, delta, prefill):
        L = _L()
        lib, ptr, d = L.lib(), L.ptr, self.d
        out = torch.full((self.B, self.T, self.H), prefill, device='cuda')
        L.check(lib.uniter_txt_embed_bwd_rows(ptr(d['dcat']), ptr(d['ids']), ptr(d['pos_ids']), ptr(d['type_ids']), ptr(d['word']),
                                              ptr(d['pos']), ptr(d['typ']), ptr(d['gamma']), ptr(delta), ptr(out), self.B, self.T, self.S,
                                              self.H, self.vocab, self.max_pos, self.tv, self.pos_bcast, self.p, SEED, OFFSET,
                                              L.cur_stream()), 'uniter_txt_embed_bwd_rows')
        torch.cuda.synchronize()
        return out.cpu()


@pytest.mark.parametrize('case', _txt_cases())
def test_text_forward_with_delta_and_per_token_gradient_match_float64(case):
    c = _Txt(case)
    T, rel_f, rel_b = c.T, (ILL if c.ill else FWD), (ILL if c.ill else BWD)
    ref_fwd, ref_rows = c.reference(c.delta)

    cat = c.fwd(c.d['delta'])
    _close(cat[:, :T], ref_fwd, rel_f, 'cat')
    assert torch.isnan(cat[:, T:]).all()

    # delta == 0 and delta == NULL are the plain forward, bit for bit
    plain = c.fwd(False)
    assert torch.equal(c.fwd(torch.zeros_like(c.d['delta']))[:, :T], plain[:, :T])
    assert torch.equal(c.fwd(None)[:, :T], plain[:, :T])
    if c.kind == 'distinct':      # ... and a perturbed row is the plain forward on a table that holds word + delta, bit for bit
        table = c.word.clone()
        table[c.ids.view(-1)] = c.word[c.ids.view(-1)] + c.delta.view(-1, c.H)
        assert torch.equal(cat[:, :T], c.fwd(False, word=_dev(table))[:, :T])

    # the per-token gradient: overwrites whatever the buffer held
    rows = c.bwd_rows(c.d['delta'], float('nan'))
    _close(rows, ref_rows, rel_b, 'd_rows')
    assert torch.equal(rows, c.bwd_rows(c.d['delta'], 7.0))
    _, ref_rows0 = c.reference(torch.zeros_like(c.delta))
    rows0 = c.bwd_rows(None, float('nan'))
    _close(rows0, ref_rows0, rel_b, 'd_rows without delta')

    if c.kind == 'distinct':
        # all ids distinct and non-zero: the order-fixed backward on zeroed tables leaves exactly this row in dword[ids[b, t]]
        L = _L()
        lib, ptr, d = L.lib(), L.ptr, c.d
        n = c.B * c.T
        nws = lib.uniter_embed_bwd_det_ws_bytes(n, 0, c.H)
        ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
        gt = {k: torch.zeros_like(d[k]) for k in ('word', 'pos', 'typ', 'gamma', 'beta')}
        L.check(lib.uniter_txt_embed_bwd_det(ptr(d['dcat']), ptr(d['ids']), ptr(d['pos_ids']), ptr(d['type_ids']), ptr(d['word']),
                                             ptr(d['pos']), ptr(d['typ']), ptr(d['gamma']), ptr(gt['word']), ptr(gt['pos']), ptr(gt['typ']),
                                             ptr(gt['gamma']), ptr(gt['beta']), c.B, c.T, c.S, c.H, c.vocab, c.max_pos, c.tv, c.pos_bcast,
                                             c.p, SEED, OFFSET, ptr(ws), nws, L.cur_stream()), 'uniter_txt_embed_bwd_det')
        torch.cuda.synchronize()
        assert torch.equal(rows0.view(n, c.H), gt['word'].cpu()[c.ids.view(-1)])


# ---------------------------------------------------------------------------------------------------------------------------
# position features: d_pos7 = d_posfc @ Wp
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [4, 128, 260, 768, 1024])
@pytest.mark.parametrize('BR', [1, 5, 70, 576])
def test_pos_feat_dgrad_matches_float64(BR, H):
    L = _L()
    g = torch.Generator().manual_seed(BR * 31 + H)
    d_posfc = torch.randn(BR, H, generator=g).float()
    Wp = (0.5 * torch.randn(H, 7, generator=g)).float()
    ref = d_posfc.double() @ Wp.double()
    outs, d_d, d_w = [], _dev(d_posfc), _dev(Wp)
    for fill in (float('nan'), 3.0):
        out = torch.full((BR + 1, 7), fill, device='cuda')                        # one row beyond: must stay as it is
        L.check(L.lib().uniter_pos_feat_dgrad(L.ptr(d_d), L.ptr(d_w), L.ptr(out), BR, H, L.cur_stream()), 'uniter_pos_feat_dgrad')
        torch.cuda.synchronize()
        outs.append(out.cpu())
    _close(outs[0][:BR], ref, BWD, 'd_pos7')
    assert torch.isnan(outs[0][BR]).all() and torch.equal(outs[1][BR], torch.full((7,), 3.0))
    assert torch.equal(outs[0][:BR], outs[1][:BR])


# ---------------------------------------------------------------------------------------------------------------------------
# the perturbation's ascent step and projection
# ---------------------------------------------------------------------------------------------------------------------------
def _adv_ref(delta, grad, step, max_norm):
    d, g = delta.double(), grad.double()
    gn = g.norm(dim=1, keepdim=True)
    d = d + torch.where(gn > 0, step * g / gn.clamp_min(1e-300), torch.zeros_like(g))
    if max_norm > 0:
        dn = d.norm(dim=1, keepdim=True)
        d = d * torch.where(dn > max_norm, max_norm / dn.clamp_min(1e-300), torch.ones_like(dn))
    return d


def _adv_run(delta, grad, step, max_norm):
    L = _L()
    B, n = delta.shape
    d, g = _dev(delta.clone()), _dev(grad)
    nws = L.lib().uniter_adv_delta_ws_bytes(B, n)
    ws = torch.empty(max(nws, 8), dtype=torch.uint8, device='cuda')
    L.check(L.lib().uniter_adv_delta_step(L.ptr(d), L.ptr(g), B, n, step, max_norm, L.ptr(ws), L.cur_stream()), 'uniter_adv_delta_step')
    torch.cuda.synchronize()
    return d.cpu()


@pytest.mark.parametrize('max_norm', [1.0, 0.0])
@pytest.mark.parametrize('n', [4, 1000, 98304])
@pytest.mark.parametrize('B', [1, 3, 16])
def test_adv_delta_step_matches_float64_and_repeats(B, n, max_norm):
    g_ = torch.Generator().manual_seed(B * 7 + n)
    delta = torch.randn(B, n, generator=g_).double()
    delta = (delta * (0.5 / delta.norm(dim=1, keepdim=True))).float()             # norm 0.5: inside the unit ball
    grad = (torch.randn(B, n, generator=g_) * 1e-3).float()
    grad[0] = 0                                                                   # this sample's gradient vanishes
    if B > 1:
        delta[1] *= 6.0                                                           # already outside the ball
    step = 1.2                                                                    # (0.5^2 + 1.2^2 > 1: the stepped samples leave the unit ball and are projected)
    ref = _adv_ref(delta, grad, step, max_norm)
    got = _adv_run(delta, grad, step, max_norm)
    _close(got, ref, FWD, 'delta')
    assert torch.equal(got[0], delta[0])                                          # g = 0 inside the ball: the same bits
    if max_norm > 0:
        assert (got.double().norm(dim=1) <= max_norm * (1 + 1e-6)).all()
    assert torch.equal(got, _adv_run(delta, grad, step, max_norm))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [6, 1028])
def test_row_kernels_refuse_unsupported_hidden_sizes(H):
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    B, T, S = 1, 2, 2
    i64 = torch.zeros(B, T, dtype=torch.int64, device='cuda')
    tab, vec = torch.zeros(4, H, device='cuda'), torch.zeros(H, device='cuda')
    big = torch.zeros(B, S, H, device='cuda')
    common = (B, T, S, H, 4, 4, 2, 0, 0.0, SEED, OFFSET, cs)
    rc = lib.uniter_txt_embed_fwd_delta(ptr(i64), ptr(i64), None, ptr(tab), ptr(tab), ptr(tab), ptr(vec), ptr(vec), ptr(big), ptr(big), *common)
    assert rc == -2 and lib.uniter_last_error()
    rc = lib.uniter_txt_embed_bwd_rows(ptr(big), ptr(i64), ptr(i64), None, ptr(tab), ptr(tab), ptr(tab), ptr(vec), None, ptr(big), *common)
    assert rc == -2
    w7, o7 = torch.zeros(H, 7, device='cuda'), torch.zeros(2, 7, device='cuda')
    assert lib.uniter_pos_feat_dgrad(ptr(big), ptr(w7), ptr(o7), 2, H, cs) == -2
    assert lib.uniter_txt_embed_bwd_rows(None, ptr(i64), ptr(i64), None, ptr(tab), ptr(tab), ptr(tab), ptr(vec), None, ptr(big), *common) == -1
    assert lib.uniter_adv_delta_step(ptr(big), ptr(big), 1, 6, 1.0, 1.0, ptr(big), cs) == -2
    assert lib.uniter_adv_delta_step(None, ptr(big), 1, 4, 1.0, 1.0, ptr(big), cs) == -1


def _tiny():
    from common import TINY, TINY_IMG_DIM
    from meme_challenge_amd.model import UniterConfig, UniterModel
    torch.manual_seed(0)
    return UniterModel(UniterConfig.from_dict(TINY), TINY_IMG_DIM).cuda(), TINY, TINY_IMG_DIM


def test_model_forward_refuses_input_gradients_that_do_not_fit_the_batch():
    L = _L()
    model, cfg, D = _tiny()
    B, T, R, H = 2, 5, 3, cfg['hidden_size']
    ids = torch.randint(1, cfg['vocab_size'], (B, T), device='cuda')
    pos = torch.arange(T, device='cuda').unsqueeze(0)
    feat, pos7 = torch.randn(B, R, D, device='cuda'), torch.rand(B, R, 7, device='cuda')
    txt = dict(input_ids=ids, position_ids=pos, img_feat=None, img_pos_feat=None, attention_mask=torch.ones(B, T, device='cuda'),
               output_all_encoded_layers=False)
    img = dict(input_ids=None, position_ids=None, img_feat=feat, img_pos_feat=pos7, attention_mask=torch.ones(B, R, device='cuda'),
               output_all_encoded_layers=False)
    buf = torch.zeros(B, max(T, R), max(H, D), device='cuda')
    with torch.no_grad():
        model(**txt)                                                              # (creates the handle)
    setter = L.lib().uniter_model_set_input_grads
    # a perturbation / a per-token gradient on an image-only batch
    for args in ((L.ptr(buf), None, None, None), (None, L.ptr(buf), None, None)):
        L.check(setter(model._handle, *args))
        with pytest.raises(L.UniterHipError, match='without text'):
            model(**img)
    # the image outputs on a text-only batch
    for args in ((None, None, L.ptr(buf), None), (None, None, None, L.ptr(buf))):
        L.check(setter(model._handle, *args))
        with pytest.raises(L.UniterHipError, match='without regions'):
            model(**txt)
    # outputs for an inference forward
    L.check(setter(model._handle, None, L.ptr(buf), None, None))
    with torch.no_grad(), pytest.raises(L.UniterHipError, match='inference'):
        model(**txt)
    # a refused setting is forgotten: the next pass runs, and a perturbation alone is fine without gradients
    with torch.no_grad():
        plain = model(**txt)
        moved = model(txt_embed_delta=torch.full((B, T, H), 0.05, device='cuda'), **txt)
        again = model(**txt)
    assert torch.equal(plain, again) and not torch.equal(plain, moved)
