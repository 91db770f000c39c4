"""The embedding kernels of csrc/embed.hip through the C ABI, against float64 torch references of the same operations:
text and image embeddings forward and backward (LayerNorms, lookups, 7-d position projection, dropout replayed from the shared
Philox masks, atomic scatter into the tables), the joint gather's backward, img_mask_add, bias_rows, and the host-side refusals.

Tolerances follow from fp32 arithmetic against float64: about 4e-6 x max |ref| for forward rows of unit scale, 1e-5 x max |ref|
for each gradient.  Rows whose LayerNorm input is nearly constant (mean ~1, spread ~1e-3) lose about mean / spread times more
of their digits in any fp32 LayerNorm; they are held to 2e-3 relative, which an fp32 two-pass LayerNorm with eps = 1e-12 meets
by a wide margin and a one-pass variance or eps = 1e-5 misses by percent to tens of percent."""
import pytest
import torch

from oracle import philox
from oracle import uniter_oracle as O

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x1234ABCD5678, 11
FWD, BWD, ILL = 4e-6, 1e-5, 2e-3


def _L():
    from meme_challenge_amd import _lib
    return _lib


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _close(got, ref, rel, what, pre=None):
    """|got - (pre + ref)| <= rel * max |ref| (+ a few ulp of the accumulated value when the kernel adds onto pre)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    exp = ref if pre is None else pre.double() + ref
    tol = rel * ref.abs().max().item() + (0.0 if pre is None else 2.0 ** -20 * exp.abs().max().item())
    err = (got - exp).abs().max().item()
    assert err <= tol, (what, err, tol)


def _prefill(shape, g):
    return (torch.randn(*shape, generator=g) * 0.5).float()


def _ws(rows, H):
    L = _L()
    n = L.lib().uniter_embed_bwd_ws_bytes(rows, H)
    return torch.empty(max(n, 1), dtype=torch.uint8, device='cuda'), n


def _drop(p):
    return O.DropSpec(SEED, OFFSET, p, p) if p > 0 else None


# ---------------------------------------------------------------------------------------------------------------------------
# text: word + position + token type, LayerNorm, dropout; backward scatters into the three tables
# ---------------------------------------------------------------------------------------------------------------------------
def _txt_cases():
    cases = [dict(H=H) for H in (4, 64, 128, 260, 516, 768, 1020, 1024)]       # NV = 1..4, full and partial last chunks
    for H in (260, 768):
        cases += [dict(H=H, BT=bt) for bt in ((1, 1), (1, 3), (2, 2), (5, 1), (16, 128))]   # partial workgroup .. grid-stride
        cases += [dict(H=H, types=True), dict(H=H, pos_bcast=1), dict(H=H, p=0.1), dict(H=H, ids='same'),
                  dict(H=H, cond='ill'), dict(H=H, BT=(4, 33), types=True, pos_bcast=1, p=0.1)]
    return [pytest.param(c, id='-'.join('%s=%s' % kv for kv in c.items())) for c in cases]


@pytest.mark.parametrize('case', _txt_cases())
def test_text_embedding_forward_and_backward_match_float64(case):
    H, (B, T) = case['H'], case.get('BT', (3, 7))
    types, pos_bcast, p = case.get('types', False), case.get('pos_bcast', 0), case.get('p', 0.0)
    ill = case.get('cond') == 'ill'
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    g = torch.Generator().manual_seed(H * 131 + B * 17 + T + 7 * types + 3 * pos_bcast + int(p * 10) + 50 * ill)
    vocab, max_pos, tv, S = 50, 96, 2, T + 3
    n = B * T
    if case.get('ids') == 'same':
        ids = torch.full((B, T), 23, dtype=torch.int64)                          # every token on one table row
    else:
        ids = torch.randint(0, vocab, (B, T), generator=g)
        flat = ids.view(-1)
        flat[-1] = vocab - 1
        if n > 1:
            flat[0] = 0                                                           # padding row
    pos_ids = torch.randint(0, max_pos, (T,) if pos_bcast else (B, T), generator=g)
    pos_ids.view(-1)[-1] = max_pos - 1
    type_ids = None
    if types:
        type_ids = torch.randint(0, tv, (B, T), generator=g)
        if n > 1:
            type_ids.view(-1)[:2] = torch.tensor([0, 1])
    if ill:     # row sums: mean ~1, spread ~1e-3
        word = 1.0 + 1e-3 * torch.randn(vocab, H, generator=g)
        pos, typ = 5e-4 * torch.randn(max_pos, H, generator=g), 5e-4 * torch.randn(tv, H, generator=g)
    else:
        word = torch.randn(vocab, H, generator=g)
        pos, typ = 0.5 * torch.randn(max_pos, H, generator=g), 0.5 * torch.randn(tv, H, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    word, pos, typ, gamma, beta = (t.float() for t in (word, pos, typ, gamma, beta))

    # float64 reference: the oracle's UniterTextEmbeddings on the same fp32 values
    leaves = {k: t.double().requires_grad_(True) for k, t in
              dict(word=word, pos=pos, type=typ, gamma=gamma, beta=beta).items()}
    sd = {'embeddings.word_embeddings.weight': leaves['word'], 'embeddings.position_embeddings.weight': leaves['pos'],
          'embeddings.token_type_embeddings.weight': leaves['type'], 'embeddings.LayerNorm.weight': leaves['gamma'],
          'embeddings.LayerNorm.bias': leaves['beta']}
    ref = O.text_embeddings(sd, '', ids, pos_ids.expand(B, T) if pos_bcast else pos_ids, type_ids,
                            {'hidden_dropout_prob': p}, _drop(p))

    # forward: rows [b, 0:T) of a NaN-prefilled cat
    d_ids, d_pos, d_type = _dev(ids), _dev(pos_ids), _dev(type_ids)
    d_word, d_posw, d_typ, d_g, d_b = (_dev(t) for t in (word, pos, typ, gamma, beta))
    cat = torch.full((B, S, H), float('nan'), device='cuda')
    L.check(lib.uniter_txt_embed_fwd(ptr(d_ids), ptr(d_pos), ptr(d_type), ptr(d_word), ptr(d_posw), ptr(d_typ), ptr(d_g),
                                     ptr(d_b), ptr(cat), B, T, S, H, vocab, max_pos, tv, pos_bcast, p, SEED, OFFSET, cs))
    torch.cuda.synchronize()
    _close(cat[:, :T], ref, ILL if ill else FWD, 'cat')
    assert torch.isnan(cat[:, T:]).all()

    # backward: accumulates onto prefilled gradients
    dcat = torch.randn(B, S, H, generator=g)
    ref.backward(dcat[:, :T].double())
    gw = leaves['word'].grad.clone()
    gw[0] = 0                                                                     # padding_idx = 0
    pre = {k: _prefill(t.shape, g) for k, t in dict(word=word, pos=pos, type=typ, gamma=gamma, beta=beta).items()}
    got = {k: _dev(t) for k, t in pre.items()}
    ws, nws = _ws(n, H)
    d_dcat = _dev(dcat)
    L.check(lib.uniter_txt_embed_bwd(ptr(d_dcat), ptr(d_ids), ptr(d_pos), ptr(d_type), ptr(d_word), ptr(d_posw),
                                     ptr(d_typ), ptr(d_g), ptr(got['word']), ptr(got['pos']), ptr(got['type']),
                                     ptr(got['gamma']), ptr(got['beta']), B, T, S, H, vocab, max_pos, tv, pos_bcast, p, SEED,
                                     OFFSET, ptr(ws), nws, cs))
    torch.cuda.synchronize()
    got = {k: t.cpu() for k, t in got.items()}
    rel = ILL if ill else BWD
    _close(got['word'], gw, rel, 'dword', pre['word'])
    _close(got['pos'], leaves['pos'].grad, rel, 'dpos', pre['pos'])
    _close(got['type'], leaves['type'].grad, rel, 'dtype', pre['type'])
    _close(got['gamma'], leaves['gamma'].grad, rel, 'dgamma', pre['gamma'])
    _close(got['beta'], leaves['beta'].grad, rel, 'dbeta', pre['beta'])
    # rows no token reads are bit-unchanged: the padding row, unused words / positions, the unused type row
    untouched = torch.ones(vocab, dtype=torch.bool)
    untouched[ids.view(-1)] = False
    untouched[0] = True
    assert torch.equal(got['word'][untouched], pre['word'][untouched])
    unused_pos = torch.ones(max_pos, dtype=torch.bool)
    unused_pos[pos_ids.view(-1)] = False
    assert torch.equal(got['pos'][unused_pos], pre['pos'][unused_pos])
    if type_ids is None:
        assert torch.equal(got['type'][1], pre['type'][1])


# ---------------------------------------------------------------------------------------------------------------------------
# image: LN(img_linear out) + LN(7-d position projection) + type row, LayerNorm, dropout
# ---------------------------------------------------------------------------------------------------------------------------
def _img_cases():
    cases = [dict(H=H) for H in (4, 64, 128, 260, 516, 768, 1020, 1024)]
    for H in (260, 768):
        cases += [dict(H=H, BR=br) for br in ((1, 1), (3, 1), (4, 1), (5, 1), (1, 36), (2, 100), (21, 100))]
        cases += [dict(H=H, types=True), dict(H=H, p=0.1), dict(H=H, T0=0), dict(H=H, T0=40), dict(H=H, cond='ill'),
                  dict(H=H, BR=(3, 36), types=True, p=0.1)]
    cases += [dict(H=1024, cond='ill', BR=(2, 36))]
    return [pytest.param(c, id='-'.join('%s=%s' % kv for kv in c.items())) for c in cases]


def _stats64(z):
    return z.mean(-1), 1.0 / torch.sqrt(z.var(-1, unbiased=False) + 1e-12)


@pytest.mark.parametrize('case', _img_cases())
def test_image_embedding_forward_and_backward_match_float64(case):
    H, (B, R) = case['H'], case.get('BR', (2, 5))
    types, p, T0 = case.get('types', False), case.get('p', 0.0), case.get('T0', 3)
    ill = case.get('cond') == 'ill'
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    g = torch.Generator().manual_seed(H * 71 + B * 13 + R + 5 * types + int(p * 10) + T0 + 90 * ill)
    tv, S, n = 2, T0 + R + 2, B * R
    if ill:     # near-constant rows: mean ~1, spread ~1e-3 (variance 1e-6)
        imgfc = 1.0 + 1e-3 * torch.randn(n, H, generator=g)
    else:
        imgfc = torch.randn(n, H, generator=g) * (1.0 + torch.rand(n, 1, generator=g))
    pos7 = torch.rand(n, 7, generator=g)
    Wp, bp = 0.5 * torch.randn(H, 7, generator=g), 0.1 * torch.randn(H, generator=g)
    typ = 0.5 * torch.randn(tv, H, generator=g)
    aff = [1.0 + 0.1 * torch.randn(H, generator=g) if i % 2 == 0 else 0.1 * torch.randn(H, generator=g) for i in range(6)]
    type_ids = None
    if types:
        type_ids = torch.randint(0, tv, (n,), generator=g)
        if n > 1:
            type_ids[:2] = torch.tensor([0, 1])
    imgfc, pos7, Wp, bp, typ = (t.float() for t in (imgfc, pos7, Wp, bp, typ))
    aff = [t.float() for t in aff]

    # float64 reference
    x = imgfc.double().requires_grad_(True)
    Wp64, bp64, typ64 = (t.double().requires_grad_(True) for t in (Wp, bp, typ))
    aff64 = [t.double().requires_grad_(True) for t in aff]
    q = pos7.double() @ Wp64.t() + bp64
    q.retain_grad()
    tid = type_ids if types else torch.ones(n, dtype=torch.int64)
    f = O.layer_norm(x, aff64[0], aff64[1]) + O.layer_norm(q, aff64[2], aff64[3]) + typ64[tid]
    e = O.layer_norm(f, aff64[4], aff64[5])
    ref = O._apply_dropout(e.view(B, R, H), p, _drop(p), philox.SITE_IMG_EMB)
    st_ref = torch.stack([*_stats64(x.detach()), *_stats64(q.detach()), *_stats64(f.detach())], 1)

    dev = [_dev(t) for t in (imgfc, pos7, type_ids, Wp, bp, typ)] + [_dev(t) for t in aff]
    d_x, d_p7, d_tid, d_Wp, d_bp, d_typ = dev[:6]
    d_aff = dev[6:]
    cat = torch.full((B, S, H), float('nan'), device='cuda')
    stats = torch.full((n, 6), float('nan'), device='cuda')
    L.check(lib.uniter_img_embed_fwd(ptr(d_x), ptr(d_p7), ptr(d_tid), ptr(d_Wp), ptr(d_bp), ptr(d_typ),
                                     *[ptr(t) for t in d_aff], ptr(cat), ptr(stats), B, R, T0, S, H, tv, p, SEED, OFFSET, cs))
    torch.cuda.synchronize()
    rel = ILL if ill else FWD
    _close(cat[:, T0:T0 + R], ref, rel, 'cat')
    assert torch.isnan(cat[:, :T0]).all() and torch.isnan(cat[:, T0 + R:]).all()
    st = stats.cpu().double()       # (mean, rstd) of the three LayerNorms' inputs, per row
    for i, z in enumerate((x, q, f)):
        scale = z.detach().abs().amax(-1)
        # the third LayerNorm's input carries the first one's output, ill-conditioned in the 'ill' case
        assert ((st[:, 2 * i] - st_ref[:, 2 * i]).abs() <= (ILL if ill and i == 2 else 4e-6) * scale).all(), ('mean', i)
        rerr = ((st[:, 2 * i + 1] - st_ref[:, 2 * i + 1]).abs() / st_ref[:, 2 * i + 1]).max().item()
        assert rerr <= (ILL if ill else 2e-5), ('rstd', i, rerr)

    # backward
    dcat = torch.randn(B, S, H, generator=g)
    ref.backward(dcat[:, T0:T0 + R].double())
    pre = {k: _prefill(t.shape, g) for k, t in dict(Wp=Wp, bp=bp, type=typ).items()}
    pre_aff = [_prefill((H,), g) for _ in range(6)]
    got = {k: _dev(t) for k, t in pre.items()}
    got_aff = [_dev(t) for t in pre_aff]
    d_imgfc = torch.full((n, H), float('nan'), device='cuda')
    d_posfc = torch.full((n, H), float('nan'), device='cuda')
    ws, nws = _ws(n, H)
    d_dcat = _dev(dcat)
    L.check(lib.uniter_img_embed_bwd(ptr(d_dcat), ptr(d_x), ptr(d_p7), ptr(d_tid), ptr(d_Wp), ptr(d_bp), ptr(d_typ),
                                     *[ptr(t) for t in d_aff[:5]], ptr(stats), ptr(d_imgfc), ptr(d_posfc), ptr(got['Wp']),
                                     ptr(got['bp']), ptr(got['type']), *[ptr(t) for t in got_aff], B, R, T0, S, H, tv, p,
                                     SEED, OFFSET, ptr(ws), nws, cs))
    torch.cuda.synchronize()
    rel = ILL if ill else BWD
    _close(d_imgfc, x.grad, rel, 'd_imgfc')
    _close(d_posfc, q.grad, rel, 'd_posfc')
    _close(got['Wp'], Wp64.grad, rel, 'dWp', pre['Wp'])
    _close(got['bp'], bp64.grad, rel, 'dbp', pre['bp'])
    _close(got['type'], typ64.grad, rel, 'dtype', pre['type'])
    for i, name in enumerate(('dg_i', 'db_i', 'dg_p', 'db_p', 'dg_f', 'db_f')):
        _close(got_aff[i], aff64[i].grad, rel, name, pre_aff[i])
    if type_ids is None:
        assert torch.equal(got['type'][0].cpu(), pre['type'][0])


# ---------------------------------------------------------------------------------------------------------------------------
# the joint gather's backward: the adjoint of uniter_gather_rows (which reads row clamp(gi, 0, S-1))
# ---------------------------------------------------------------------------------------------------------------------------
def _gather_bwd(dout, gi, B, S, Lout, H):
    L = _L()
    dcat = torch.full((B, S, H), float('nan'), device='cuda')
    L.check(L.lib().uniter_gather_rows_bwd(L.ptr(dout), L.ptr(gi), L.ptr(dcat), B, S, Lout, H, L.cur_stream()))
    torch.cuda.synchronize()
    return dcat


def _scatter64(dout, gi, S):
    B, Lout, H = dout.shape
    ref = torch.zeros(B, S, H, dtype=torch.float64)
    ref.scatter_add_(1, gi.clamp(0, S - 1)[:, :, None].expand(B, Lout, H), dout.double())
    return ref


@pytest.mark.parametrize('B,S,Lout,H', [(3, 20, 17, 260), (2, 9, 9, 64), (1, 300, 256, 1024), (4, 5, 1, 4)])
def test_gather_backward_without_index_is_the_identity_then_zeros(B, S, Lout, H):
    g = torch.Generator().manual_seed(S * 7 + H)
    dout = torch.randn(B, Lout, H, generator=g).cuda()
    dcat = _gather_bwd(dout, None, B, S, Lout, H)
    assert torch.equal(dcat[:, :Lout], dout)
    assert (dcat[:, Lout:] == 0).all()


@pytest.mark.parametrize('H', [64, 260, 768])
def test_gather_backward_of_a_ragged_batch_sums_duplicate_indices(H):
    """get_gather_index points the padded tail of a short sample at rows other positions also read: their gradients add up"""
    tl, nbb, T, R = [7, 2, 5, 1], [4, 4, 1, 3], 7, 4
    B, Lout = len(tl), max(a + c for a, c in zip(tl, nbb))
    S = T + R
    gi = O.get_gather_index(tl, nbb, B, T, Lout)
    assert any(len(set(r.tolist())) < Lout for r in gi)                          # duplicates present
    g = torch.Generator().manual_seed(H)
    dout = torch.randn(B, Lout, H, generator=g)
    dcat = _gather_bwd(dout.cuda(), gi.cuda(), B, S, Lout, H)
    _close(dcat, _scatter64(dout, gi, S), 1e-6, 'dcat')


@pytest.mark.parametrize('H', [4, 264, 1024])
def test_gather_backward_is_the_adjoint_of_the_clamped_forward(H):
    """<gather(cat), dout> = <cat, gather_bwd(dout)> with out-of-range indices (negative and >= S), which the forward clamps"""
    L = _L()
    B, S, Lout = 3, 10, 14
    g = torch.Generator().manual_seed(H + 1)
    gi = torch.randint(-4, S + 4, (B, Lout), generator=g)
    gi[0, :4] = torch.tensor([-1, S, -(1 << 40), S + 3])
    cat = torch.randn(B, S, H, generator=g)
    dout = torch.randn(B, Lout, H, generator=g)
    out = torch.empty(B, Lout, H, device='cuda')
    d_cat, d_gi = cat.cuda(), gi.cuda()
    L.check(L.lib().uniter_gather_rows(L.ptr(d_cat), L.ptr(d_gi), L.ptr(out), B, S, Lout, H, L.cur_stream()))
    dcat = _gather_bwd(dout.cuda(), d_gi, B, S, Lout, H)
    assert torch.equal(out.cpu(), torch.gather(cat, 1, gi.clamp(0, S - 1)[:, :, None].expand(B, Lout, H)))
    lhs = (out.cpu().double() * dout.double()).sum().item()
    rhs = (cat.double() * dcat.cpu().double()).sum().item()
    assert abs(lhs - rhs) <= 2e-7 * (cat.double().abs() * _scatter64(dout.abs(), gi, S)).sum().item() + 1e-6, (lhs, rhs)
    _close(dcat, _scatter64(dout, gi, S), 1e-6, 'dcat')


# ---------------------------------------------------------------------------------------------------------------------------
# img_mask_add and bias_rows: exact
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,D', [(1, 4), (7, 20), (300, 64), (37, 2048)])
def test_img_mask_add_adds_mask_row_one_where_masked(rows, D):
    L = _L()
    g = torch.Generator().manual_seed(rows * 3 + D)
    feat = torch.randn(rows, D, generator=g)
    masks = torch.tensor([0, 1, 2, -1, 7, -3] * rows, dtype=torch.int64)[:rows]  # every non-zero mask counts as 1
    emb = torch.randn(2, D, generator=g)                                          # row 0 is never added (the reference zeroes it)
    out = torch.full((rows + 1, D), float('nan'), device='cuda')                  # + one guard row
    d_feat, d_masks, d_emb = feat.cuda(), masks.cuda(), emb.cuda()
    L.check(L.lib().uniter_img_mask_add(L.ptr(d_feat), L.ptr(d_masks), L.ptr(d_emb), L.ptr(out), rows, D, L.cur_stream()))
    torch.cuda.synchronize()
    ref = torch.where((masks != 0)[:, None], feat + emb[1], feat)
    assert torch.equal(out[:rows].cpu(), ref)
    assert torch.isnan(out[rows]).all()


@pytest.mark.parametrize('M,N', [(1, 4), (3, 12), (7, 260), (1100, 1024)])    # the last one walks its 1024-workgroup grid twice
def test_bias_rows_broadcasts_the_bias(M, N):
    L = _L()
    bias = torch.randn(N, generator=torch.Generator().manual_seed(M + N)).cuda()
    out = torch.full((M + 1, N), float('nan'), device='cuda')
    L.check(L.lib().uniter_bias_rows(L.ptr(bias), L.ptr(out), M, N, L.cur_stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[:M], bias.expand(M, N))
    assert torch.isnan(out[M]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: host-side checks, nothing launched (every buffer is sized so that even a launch would stay in bounds)
# ---------------------------------------------------------------------------------------------------------------------------
def test_embedding_entry_points_refuse_what_they_do_not_cover():
    L = _L()
    lib, ptr, cs = L.lib(), L.ptr, L.cur_stream()
    B, T, H, Hmax = 2, 4, 128, 1028
    big = torch.zeros(64 * Hmax * 8, device='cuda')          # every float operand
    ids = torch.zeros(64, dtype=torch.int64, device='cuda')
    P, I = ptr(big), ptr(ids)

    def txt_fwd(H, T, S):
        return lib.uniter_txt_embed_fwd(I, I, None, P, P, P, P, P, P, B, T, S, H, 8, 8, 2, 0, 0.0, 1, 0, cs)

    def txt_bwd(H, T, S, ws_bytes):
        return lib.uniter_txt_embed_bwd(P, I, I, None, P, P, P, P, P, P, P, P, P, B, T, S, H, 8, 8, 2, 0, 0.0, 1, 0, P,
                                        ws_bytes, cs)

    def img_fwd(H, R, T0, S, tv):
        return lib.uniter_img_embed_fwd(P, P, None, *[P] * 9, P, P, B, R, T0, S, H, tv, 0.0, 1, 0, cs)

    def img_bwd(H, R, T0, S, tv, ws_bytes):
        return lib.uniter_img_embed_bwd(P, P, P, None, *[P] * 20, B, R, T0, S, H, tv, 0.0, 1, 0, P, ws_bytes, cs)

    ws = lambda rows, H: lib.uniter_embed_bwd_ws_bytes(rows, H)
    assert txt_fwd(H, T, T) == 0 and txt_bwd(H, T, T, ws(B * T, H)) == 0            # the legal calls these vary
    assert img_fwd(H, 3, 1, 4, 2) == 0 and img_bwd(H, 3, 1, 4, 2, ws(B * 3, H)) == 0
    torch.cuda.synchronize()
    assert txt_fwd(Hmax, T, T) != 0 and txt_bwd(Hmax, T, T, ws(B * T, Hmax)) != 0       # H > 1024
    assert txt_fwd(130, T, T) != 0 and txt_bwd(130, T, T, ws(B * T, 130)) != 0          # H % 4
    assert txt_fwd(H, T + 1, T) != 0 and txt_bwd(H, T + 1, T, ws(B * (T + 1), H)) != 0  # T > S
    assert txt_bwd(H, T, T, ws(B * T, H) - 1) != 0                                      # workspace one byte short
    assert img_fwd(Hmax, 3, 1, 4, 2) != 0 and img_bwd(Hmax, 3, 1, 4, 2, ws(B * 3, Hmax)) != 0
    assert img_fwd(130, 3, 1, 4, 2) != 0 and img_bwd(130, 3, 1, 4, 2, ws(B * 3, 130)) != 0
    assert img_fwd(H, 3, 2, 4, 2) != 0 and img_bwd(H, 3, 2, 4, 2, ws(B * 3, H)) != 0    # T0 + R > S
    assert img_fwd(H, 3, 1, 4, 1) != 0 and img_bwd(H, 3, 1, 4, 1, ws(B * 3, H)) != 0    # type_vocab < 2
    assert img_bwd(H, 3, 1, 4, 2, ws(B * 3, H) - 1) != 0
    assert b'embed' in lib.uniter_last_error()
    torch.cuda.synchronize()
