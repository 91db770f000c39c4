"""`UniterModel.output_attention_grads` / `last_attention_grads` / `last_head_grads` and `attribution.attention_gradients`,
`attention_relevance`, `head_importance` on the tiny model of tests/common.py and the golden batch (B = 3, L = 16, two samples with 6
masked positions); target = the sum of the logits.

Reference: a restatement of `oracle.uniter_oracle.bert_layer` (`_layer` below, built from O.linear, O.layer_norm, O.gelu, O.pooler)
that starts from `uniter_forward(..., return_embed=True)`'s embedding and keeps every layer's softmax output with `retain_grad()`:
g_l = P_l * P_l.grad after the backward pass of the logits' sum.  In float64 its logits equal `O.meme_uniter_forward`'s exactly
(test_restatement_equals_the_oracle).  For precision 'bf16' the same restatement runs in fp32 tensors with prec='bf16' linears
(`round_out=True` for q, k, v): the bf16 values the kernels read and the bf16-rounded products of the backward pass; it is 7e-3 from
float64, which is why bf16 is judged against its own restatement.

Cases: 'fp32', 'fp32x3', 'bf16'; 'all' and 'relu_mean'; padded and packed (pack_padded), eval mode; a model with freeze_prefix(1).

Tolerance.  The gradient that reaches each layer carries the model's own error, so no closed form: max |got - ref| / max |ref_l| per
layer was measured per mode on an MI355X over all the cases above (profiles/attn_grad_parity.txt), and the assertion is 4 x that,
capped at 0.015 for the fp32 forms and 0.03 for bf16 (the caps are conditions, not the tolerance):

    mode     measured    asserted
    fp32     7.812e-07   3.125e-06
    fp32x3   8.526e-07   3.410e-06
    bf16     2.160e-03   8.640e-03      (against the bf16-rounding restatement; the maps 2.2e-3, the head sums 1.5e-3)

The caps keep the test sharp: test_mutations_are_far_above_the_caps recomputes, in float64 on this batch and relative to max |g_l|,
what each wrong capture would differ by (ReLU after the mean, no ReLU, dS instead of g, heads swapped, transposed, layers swapped, dP
alone) and asserts the smallest is >= 10 x the fp32 cap and >= 5 x the bf16 cap."""
import pytest
import torch
import torch.nn.functional as Fn

from oracle import uniter_oracle as O
from common import TINY, TINY_IMG_DIM, sd_from_npz, batch_from_npz, model_kwargs
import attn_grad_ref as GR

MODES = ['fp32', 'fp32x3', 'bf16']
CAP = {'fp32': 0.015, 'fp32x3': 0.015, 'bf16': 0.03}
# max |got - ref| / max |ref_l| measured on an MI355X per mode (profiles/attn_grad_parity.txt); asserted: 4 x that, capped
MEASURED = {'fp32': 7.812e-7, 'fp32x3': 8.526e-7, 'bf16': 2.160e-3}
TOL = {m: min(4 * MEASURED[m], CAP[m]) for m in MODES}
WORST = {}
NL, NH = TINY['num_hidden_layers'], TINY['num_attention_heads']
B, L = 3, 16


# ---------------------------------------------------------------------------------------------------------------------------
# the restated oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _layer(sd, lp, x, ext, prec, kept):
    """oracle.uniter_oracle.bert_layer without dropout, the softmax output kept with retain_grad()"""
    Bx, Lx, H = x.shape
    rnd = prec != 'fp32'
    a = lp + 'attention.self.'

    def heads(t):
        return t.view(Bx, Lx, NH, H // NH).permute(0, 2, 1, 3)
    q, k, v = (heads(O.linear(x, sd[a + n + '.weight'], sd[a + n + '.bias'], prec, rnd)) for n in ('query', 'key', 'value'))
    s = torch.matmul(q, k.transpose(-1, -2)) / 8.0
    s = s + ext
    pr = torch.softmax(s, dim=-1)
    pr.retain_grad()
    kept.append((pr, v))
    c = torch.matmul(pr, v).permute(0, 2, 1, 3).contiguous().view(Bx, Lx, H)
    o = lp + 'attention.output.'
    h = O.linear(c, sd[o + 'dense.weight'], sd[o + 'dense.bias'], prec)
    y1 = O.layer_norm(h + x, sd[o + 'LayerNorm.weight'], sd[o + 'LayerNorm.bias'])
    u = O.gelu(O.linear(y1, sd[lp + 'intermediate.dense.weight'], sd[lp + 'intermediate.dense.bias'], prec))
    o = lp + 'output.'
    h = O.linear(u, sd[o + 'dense.weight'], sd[o + 'dense.bias'], prec)
    return O.layer_norm(h + y1, sd[o + 'LayerNorm.weight'], sd[o + 'LayerNorm.bias'])


_RESTATED = {}


def restated(tiny, prec):
    """dict(logits; p, dp, g [nl, B, nh, L, L]; mean [nl, B, L, L]; sums [nl, B, nh]) as float64, computed once per arithmetic"""
    if prec in _RESTATED:
        return _RESTATED[prec]
    dt = torch.float64 if prec == 'fp32' else torch.float32
    sd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd_from_npz(tiny).items()}
    b = batch_from_npz(tiny)
    kw = dict(model_kwargs(b))
    kw['img_feat'], kw['img_pos_feat'] = kw['img_feat'].to(dt), kw['img_pos_feat'].to(dt)
    with torch.no_grad():
        _, emb = O.uniter_forward(sd, TINY, prefix='uniter_model.', return_embed=True, prec=prec, **kw)
    ext = ((1.0 - b['attn_mask'].to(torch.float32).unsqueeze(1).unsqueeze(2)) * -10000.0)
    h = emb.detach().requires_grad_(True)
    kept = []
    for i in range(NL):
        h = _layer(sd, 'uniter_model.encoder.layer.%d.' % i, h, ext, prec, kept)
    logits = Fn.linear(O.pooler(sd, 'uniter_model.', h), sd['linear.weight'], sd['linear.bias'])
    logits.sum().backward()
    p = torch.stack([pr.detach().double() for pr, _ in kept])
    dp = torch.stack([pr.grad.double() for pr, _ in kept])
    g = p * dp
    out = dict(logits=logits.detach().double(), p=p, dp=dp, g=g, mean=g.clamp(min=0).mean(2), sums=g.sum((3, 4)))
    _RESTATED[prec] = out
    return out


def test_restatement_equals_the_oracle(tiny):
    """CPU: the restated layers give the oracle's logits exactly in float64, so P_l.grad is the gradient of the oracle's logits"""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd_from_npz(tiny).items()}
    b = batch_from_npz(tiny)
    kw = dict(model_kwargs(b))
    kw['img_feat'], kw['img_pos_feat'] = kw['img_feat'].double(), kw['img_pos_feat'].double()
    with torch.no_grad():
        want = O.meme_uniter_forward(sd, TINY, **kw)
    got = restated(tiny, 'fp32')['logits']
    print('\nmax |restated - oracle| logits: %.3e' % (got - want).abs().max().item())
    assert torch.equal(got, want)
    # ... and the bf16-rounding restatement is close to it, and far from exact
    d = (restated(tiny, 'bf16')['g'] - restated(tiny, 'fp32')['g']).abs().amax((1, 2, 3, 4)) / restated(tiny, 'fp32')['g'].abs().amax((1, 2, 3, 4))
    print('bf16 restatement against float64, relative to max |g_l|: %s' % ', '.join('%.3e' % x for x in d.tolist()))
    assert 1e-5 < d.max().item() < CAP['bf16']


def _rel(x, ref, over=max):
    """max (or `over`) over the layers of max |x_l - ref_l| / max |ref_l|"""
    dims = tuple(range(1, ref.dim()))
    return over(((x - ref).abs().amax(dims) / ref.abs().amax(dims)).tolist())


def test_mutations_are_far_above_the_caps(tiny):
    """CPU: what each wrong capture would differ by from the reference on this batch, in float64 and relative to max |ref_l| -- in the
    layer where it differs LEAST, although one layer over the tolerance is enough to fail the GPU test"""
    r = restated(tiny, 'fp32')
    p, dp, g, mean = r['p'], r['dp'], r['g'], r['mean']
    muts = {
        'ReLU after the mean': _rel(g.mean(2).clamp(min=0), mean, min),
        'no ReLU': _rel(g.mean(2), mean, min),
        'dS instead of g': _rel(p * (dp - g.sum(-1, keepdim=True)), g, min),
        'heads swapped': _rel(g.flip(2), g, min),
        'transposed': _rel(g.transpose(-1, -2), g, min),
        'layers swapped': _rel(g.flip(0), g, min),
        'dP alone': _rel(dp, g, min),
    }
    print('\n' + '\n'.join('%-22s %.3g' % kv for kv in muts.items()))
    smallest = min(muts.values())
    assert smallest >= 10 * CAP['fp32'] and smallest >= 5 * CAP['bf16'], muts
    for m in MODES:
        assert TOL[m] <= CAP[m]


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
def _model(tiny, precision, train=False, packed=False, deterministic=False):
    from test_model_gpu import build
    m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision)
    m = m.train() if train else m.eval()
    m.uniter_model.pack_padded = packed
    m.uniter_model.deterministic = deterministic
    return m


def _lens(tiny):
    return [int(n) for n in batch_from_npz(tiny)['attn_mask'].sum(1).tolist()]


def _kwargs(tiny, packed=False):
    b = {k: v.cuda() for k, v in batch_from_npz(tiny).items()}
    kw = dict(model_kwargs(b))
    if packed:
        kw['seq_lens'] = _lens(tiny)
    return kw


def _capture(m, tiny, kind, packed=False):
    """one forward and one backward of the logits' sum -> (logits, last_attention_grads, last_head_grads)"""
    u = m.uniter_model
    u.output_attention_grads = kind
    logits = m(**_kwargs(tiny, packed))
    assert u.last_attention_grads is None and u.last_head_grads is None      # None until a backward pass has filled them
    logits.sum().backward()
    torch.cuda.synchronize()
    return logits.detach(), u.last_attention_grads, u.last_head_grads


def _check(got, hg, ref, kind, precision, what, lens=None):
    want = ref['g'] if kind == 'all' else ref['mean']
    got, hg = got.double().cpu(), hg.double().cpu()
    assert tuple(got.shape) == ((NL, B, NH, L, L) if kind == 'all' else (NL, B, L, L)) and tuple(hg.shape) == (NL, B, NH)
    if lens is not None:
        for b, n in enumerate(lens):
            assert not got[:, b, ..., n:, :].any() and not got[:, b, ..., :, n:].any(), 'padding of a packed sample must be exact zeros'
    err, err_h = _rel(got, want), _rel(hg, ref['sums'])
    WORST[precision] = max(WORST.get(precision, 0.0), err, err_h)
    print('%s %s %s: max |got - ref| / max |ref_l| %.3e, head_grads %.3e (asserted %.3e)' % (precision, what, kind, err, err_h, TOL[precision]))
    assert err <= TOL[precision], (precision, what, kind, err)
    assert err_h <= TOL[precision], (precision, what, kind, 'head_grads', err_h)


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [False, True], ids=['padded', 'packed'])
@pytest.mark.parametrize('precision', MODES)
def test_captured_gradients_match_the_restated_oracle(tiny, precision, packed):
    ref = restated(tiny, 'bf16' if precision == 'bf16' else 'fp32')
    m = _model(tiny, precision, packed=packed)
    u = m.uniter_model
    for kind in ('all', 'relu_mean'):
        _, got, hg = _capture(m, tiny, kind, packed)
        assert got.dtype == torch.float32 and not got.requires_grad and hg.dtype == torch.float32 and not hg.requires_grad
        _check(got, hg, ref, kind, precision, 'packed' if packed else 'padded', _lens(tiny) if packed else None)
        if kind == 'all':
            # head_grads is the sum of the 'all' maps: the same fp32 values added in another order (GR's bound without the elements' own error)
            tot, mag = got.double().sum((3, 4)).cpu(), got.double().abs().sum((3, 4)).cpu()
            sh = GR.share(hg.double().cpu().numpy(), tot.numpy(), (GR.A_H * GR.U * mag + GR.TINY).numpy())
            print('%s head_grads against the sum of the maps: share %.3f' % (precision, sh))
            assert sh <= 1.0, sh
    # ... reset by the next forward, and the tensors handed out before keep their bits
    kept, copy = got, got.clone()
    u.output_attention_grads = None
    with torch.no_grad():
        m(**_kwargs(tiny, packed))
    assert u.last_attention_grads is None and u.last_head_grads is None and torch.equal(kept, copy)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', MODES)
def test_a_frozen_prefix_does_not_cut_layers_off(tiny, precision):
    ref = restated(tiny, 'bf16' if precision == 'bf16' else 'fp32')
    m = _model(tiny, precision)
    m.uniter_model.freeze_prefix(1)
    assert m.uniter_model.backward_floor() == 1
    for kind in ('all', 'relu_mean'):
        _, got, hg = _capture(m, tiny, kind)
        _check(got, hg, ref, kind, precision, 'freeze_prefix(1)')


@pytest.mark.gpu
def test_report_measured_errors():
    print('\nmax |got - ref| / max |ref_l| per mode: ' + ', '.join('%s %.3e' % kv for kv in sorted(WORST.items())))


@pytest.mark.gpu
@pytest.mark.parametrize('precision', MODES)
def test_the_capture_changes_no_output(tiny, precision):
    """logits, every parameter gradient (deterministic) and the three input gradients: bit for bit those of a run without it"""
    runs = []
    for kind in (None, 'all', 'relu_mean', None):
        m = _model(tiny, precision, deterministic=True)
        u = m.uniter_model
        m.param_store().zero_grads()
        kw = _kwargs(tiny)
        feat = kw['img_feat'].detach().requires_grad_(True)
        pos7 = kw['img_pos_feat'].detach().requires_grad_(True)
        delta = torch.zeros(B, kw['input_ids'].shape[1], TINY['hidden_size'], device='cuda').requires_grad_(True)
        kw.update(img_feat=feat, img_pos_feat=pos7, txt_embed_delta=delta)
        u.output_attention_grads = kind
        logits = m(**kw)
        logits.sum().backward()
        torch.cuda.synchronize()
        assert (u.last_attention_grads is None) == (kind is None) and (u.last_head_grads is None) == (kind is None)
        runs.append([logits.detach().clone(), m.param_store().flat_grads.clone(), feat.grad.clone(), pos7.grad.clone(), delta.grad.clone()])
    assert all(float(t.abs().max()) > 0 for t in runs[0])
    for other in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(runs[0], other)), precision


@pytest.mark.gpu
def test_what_the_setting_refuses(tiny):
    m = _model(tiny, 'fp32', train=True)
    u = m.uniter_model
    u.output_attention_grads = 'all'
    offset = u._offset
    with pytest.raises(ValueError):
        m(**_kwargs(tiny))                       # train mode with attention dropout: defined on the undropped probabilities
    assert u._offset == offset and u.last_attention_grads is None
    u.output_attention_grads = 'mean'
    with pytest.raises(ValueError):
        m.eval()(**_kwargs(tiny))
    # a forward without gradients captures nothing and raises nothing
    u.output_attention_grads = 'all'
    with torch.no_grad():
        m.eval()(**_kwargs(tiny))
    assert u.last_attention_grads is None and u.last_head_grads is None
    # the C ABI: the forward pass refuses the setting for an inference forward and forgets it
    from meme_challenge_amd import _lib
    lib = _lib.lib()
    x = torch.zeros(NL * B * NH * L * L + NL * B * NH + 64, device='cuda')
    assert lib.uniter_model_set_attn_grads(u._handle, _lib.ptr(x), B * NH * L * L, 0, None, None, 0) == 0
    with pytest.raises(Exception):
        with torch.no_grad():
            m(**_kwargs(tiny))
    with torch.no_grad():
        m(**_kwargs(tiny))                       # forgotten: the next one runs
    assert lib.uniter_model_set_attn_grads(None, _lib.ptr(x), 1, 0, None, None, 0) == -1
    assert lib.uniter_model_set_attn_grads(u._handle, None, 0, 0, _lib.ptr(x), None, 0) == -1


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32x3', 'bf16'])
def test_attribution_functions(tiny, precision):
    from meme_challenge_amd.attribution import attention_gradients, attention_relevance, head_importance, split_joint
    ref = restated(tiny, 'bf16' if precision == 'bf16' else 'fp32')
    m = _model(tiny, precision, train=True, deterministic=True)
    u = m.uniter_model
    store = m.param_store()
    hb = {k: v for k, v in batch_from_npz(tiny).items() if k != 'img_masks'}      # (the restated oracle masks no region)
    b = {k: v.cuda() for k, v in hb.items()}
    T, Rn = hb['input_ids'].shape[1], hb['img_feat'].shape[1]
    # gradients of a training step in the buffer: every function must leave them, and the store's bookkeeping, as they are
    from meme_challenge_amd.trainer import bce_with_logits_loss
    u.set_dropout_seed(1234, 5)
    bce_with_logits_loss(m(**model_kwargs(b)), b['labels'], 1.8).backward()
    torch.cuda.synchronize()
    u.output_attention_grads = None
    u.output_attentions = 'mean'
    before = (store.flat_grads.clone(), set(store.touched), store.wgrad_stale)

    def unchanged():
        return (m.training and u.output_attention_grads is None and u.output_attentions == 'mean' and torch.equal(store.flat_grads, before[0])
                and set(store.touched) == before[1] and store.wgrad_stale == before[2])

    every = attention_gradients(m, b, heads='all')
    assert unchanged()
    _check(every.maps, every.head_grads, ref, 'all', precision, 'attention_gradients')
    mean = attention_gradients(m, b)
    assert unchanged()
    _check(mean.maps, mean.head_grads, ref, 'relu_mean', precision, 'attention_gradients')
    assert torch.equal(mean.logits, every.logits) and tuple(mean.logits.shape) == (B, 1)
    # (the two reductions add the same values over tiles of 16 and of 4 rows: equal within the sum's bound, not bit for bit)
    mag = every.maps.double().abs().sum((3, 4)).cpu()
    assert GR.share(mean.head_grads.double().cpu().numpy(), every.head_grads.double().cpu().numpy(), (2 * GR.A_H * GR.U * mag + GR.TINY).numpy()) <= 1.0
    # another target: its gradient, linear in the target
    twice = attention_gradients(m, b, target=lambda lg: 2.0 * lg.sum(), heads='all')
    assert _rel(twice.maps.double().cpu(), 2.0 * every.maps.double().cpu()) < 1e-5
    for start in (0, 1):
        rel = attention_relevance(m, b, start_layer=start)
        torch.cuda.synchronize()
        assert unchanged()
        want, bound = GR.relevance_reference(mean.maps[start:].cpu().numpy())[-1]
        sh = GR.share(rel.joint.double().cpu().numpy(), want, bound)
        print('%s relevance from layer %d: share %.3f' % (precision, start, sh))
        assert sh <= 1.0, (start, sh)
        tok, reg = split_joint(rel.joint[:, 0].cpu(), hb['gather_index'], hb['attn_mask'], T, Rn)
        assert torch.equal(rel.cls_token.cpu(), tok) and torch.equal(rel.cls_region.cpu(), reg)
        assert tuple(tok.shape) == (B, T) and tuple(reg.shape) == (B, Rn)
        assert (rel.joint[:, 0, 0] >= 1.0).all()                    # the identity's own entry at [CLS] is part of joint
        assert torch.equal(rel.logits, mean.logits)
    with pytest.raises(ValueError):
        attention_relevance(m, b, start_layer=NL)
    with pytest.raises(ValueError):
        attention_gradients(m, b, heads='mean')
    assert unchanged()
    imp = head_importance(m, [b, b], normalize=False)
    assert unchanged()
    want = every.head_grads.double().mean(1).abs()
    assert tuple(imp.shape) == (NL, NH) and _rel(imp.double().cpu(), want.cpu()) < 1e-6
    imp = head_importance(m, [b])
    assert _rel(imp.double().cpu(), (want / want.norm(dim=1, keepdim=True)).cpu()) < 1e-6
    zero = head_importance(m, [b], target=lambda lg: 0.0 * lg.sum())
    assert unchanged() and not zero.any() and not torch.isnan(zero).any()          # a layer of zeros stays zeros
