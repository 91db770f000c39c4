"""Input gradients of the whole model: img_feat.grad, img_pos_feat.grad and txt_embed_delta.grad of `MemeUniter` (tiny model of
tests/common.py, the golden batch's shapes, B = 3) against float64 autograd of the oracle's BCE loss.

The text perturbation is restated for the oracle as a word table of B * T rows, word[ids[b, t]] + delta[b, t], with
input_ids = arange(B * T): that leaf's gradient is the per-token gradient.  The tolerance is the project's tiny-model gradient bound
of tests/test_model_gpu.py, 2e-6 + 2e-4 x max |ref| per tensor."""
import numpy as np
import pytest
import torch

from oracle import uniter_oracle as O
from oracle import step_oracle as S
from common import TINY, TINY_IMG_DIM, sd_from_npz, batch_from_npz, maxdiff
from test_model_gpu import build, to_dev

pytestmark = pytest.mark.gpu

FP32_MODES = ['fp32', 'fp32x3']
SEED, OFFSET = 0x5EED5EED1234, 9
WORD = 'uniter_model.embeddings.word_embeddings.weight'
POS_WT = 1.8


def _bound(ref):
    return 2e-6 + 2e-4 * ref.abs().max().item()


def _check(got, ref, what):
    err, tol = maxdiff(got, ref), _bound(ref)
    print('%s: err %.3e bound %.3e (max |ref| %.3e)' % (what, err, tol, ref.abs().max().item()))
    assert err <= tol, (what, err, tol)


def _delta(kind, B, T, H):
    if kind == 'none':
        return None
    if kind == 'zero':
        return torch.zeros(B, T, H)
    return 0.05 * torch.randn(B, T, H, generator=torch.Generator().manual_seed(5))


def _kwargs(b, layout):
    """model keyword arguments of a layout: joint, masked (joint + img_masks), txt, img"""
    B, T = b['input_ids'].shape
    R = b['img_feat'].shape[1]
    if layout == 'txt':
        return dict(input_ids=b['input_ids'], position_ids=b['position_ids'], img_feat=None, img_pos_feat=None,
                    attention_mask=(b['input_ids'] != 0).float(), output_all_encoded_layers=False)
    if layout == 'img':
        return dict(input_ids=None, position_ids=None, img_feat=b['img_feat'], img_pos_feat=b['img_pos_feat'],
                    attention_mask=torch.ones(B, R), output_all_encoded_layers=False)
    kw = dict(input_ids=b['input_ids'], position_ids=b['position_ids'], img_feat=b['img_feat'], img_pos_feat=b['img_pos_feat'],
              attention_mask=b['attn_mask'], gather_index=b['gather_index'], output_all_encoded_layers=False)
    if layout == 'masked':
        kw['img_masks'] = b['img_masks']
    return kw


_REFS = {}


def _reference(tiny, layout, train, delta_kind):
    """float64 oracle: loss, the three input gradients and every parameter gradient (computed once per case, shared, read only)"""
    key = (layout, train, delta_kind)
    if key in _REFS:
        return _REFS[key]
    sd = {k: v.double().requires_grad_(True) for k, v in sd_from_npz(tiny).items()}
    b = batch_from_npz(tiny)
    kw = _kwargs(b, layout)
    B, T = b['input_ids'].shape
    out = {}
    feat = pos7 = rows = None
    use = dict(sd)
    if kw['img_feat'] is not None:
        feat, pos7 = kw['img_feat'].double().requires_grad_(True), kw['img_pos_feat'].double().requires_grad_(True)
        kw['img_feat'], kw['img_pos_feat'] = feat, pos7
    if kw['input_ids'] is not None:
        d = _delta(delta_kind, B, T, TINY['hidden_size'])
        rows = sd[WORD].detach()[b['input_ids'].view(-1)]
        if d is not None:
            rows = rows + d.double().view(B * T, -1)
        rows = rows.clone().requires_grad_(True)
        use[WORD] = rows
        kw['input_ids'] = torch.arange(B * T).view(B, T)
    drop = O.DropSpec(SEED, OFFSET, TINY['hidden_dropout_prob'], TINY['attention_probs_dropout_prob']) if train else None
    logits = O.meme_uniter_forward(use, TINY, drop=drop, **kw)
    loss = S.bce_with_logits(logits, b['labels'], POS_WT)
    loss.backward()
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach() for n, p in sd.items()}
    if rows is not None:      # the word table's gradient from the per-token rows (row 0 is the padding row)
        gw = torch.zeros_like(sd[WORD]).index_add_(0, b['input_ids'].view(-1), rows.grad)
        gw[0] = 0
        grads[WORD] = gw
    out = dict(logits=logits.detach(), loss=loss.detach(), params=grads,
               feat=None if feat is None else feat.grad, pos7=None if pos7 is None else pos7.grad,
               rows=None if rows is None else rows.grad.view(B, T, -1))
    _REFS[key] = out
    return out


def _run(m, tiny, layout, train, delta_kind, want=True, seq_lens=None):
    """one forward + backward of the HIP model; returns logits and the three input gradients (None where the layout has no such input)"""
    from meme_challenge_amd.trainer import bce_with_logits_loss
    m.train(train)
    m.uniter_model.set_dropout_seed(SEED, OFFSET)
    b = to_dev(batch_from_npz(tiny))
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in _kwargs(batch_from_npz(tiny), layout).items()}
    B, T = b['input_ids'].shape
    leaves = {}
    if kw['img_feat'] is not None and want:
        leaves['feat'] = kw['img_feat'] = kw['img_feat'].clone().requires_grad_(True)
        leaves['pos7'] = kw['img_pos_feat'] = kw['img_pos_feat'].clone().requires_grad_(True)
    if kw['input_ids'] is not None:
        d = _delta(delta_kind if (want or delta_kind == 'rand') else 'none', B, T, TINY['hidden_size'])
        if d is not None:
            d = d.cuda()
            if want:
                leaves['rows'] = d = d.requires_grad_(True)
            kw['txt_embed_delta'] = d
    if seq_lens is not None:
        kw['seq_lens'] = seq_lens
    logits = m(**kw)
    loss = bce_with_logits_loss(logits, b['labels'], POS_WT)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), {k: v.grad for k, v in leaves.items()}


CASES = [('joint', False, 'zero'), ('joint', True, 'zero'), ('txt', False, 'zero'), ('txt', True, 'zero'), ('img', False, 'none'),
         ('img', True, 'none'), ('masked', False, 'zero'), ('masked', True, 'zero'), ('joint', False, 'rand'), ('joint', True, 'rand')]


@pytest.mark.parametrize('precision', FP32_MODES)
@pytest.mark.parametrize('layout,train,delta_kind', CASES)
def test_input_and_parameter_gradients_match_float64_oracle(tiny, precision, layout, train, delta_kind):
    ref = _reference(tiny, layout, train, delta_kind)
    m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision)
    m.param_store().zero_grads()
    logits, g = _run(m, tiny, layout, train, delta_kind)
    assert maxdiff(logits, ref['logits']) < 1e-5
    for k in ('feat', 'pos7', 'rows'):
        if ref[k] is None:
            assert k not in g
            continue
        assert g[k] is not None, '%s.grad is None' % k
        _check(g[k], ref[k], k)
    # the parameter gradients of the same pass still meet their bound
    for n, p in m.named_parameters():
        r = ref['params'][n]
        assert maxdiff(p.grad, r) <= _bound(r), (n, maxdiff(p.grad, r), _bound(r))


@pytest.mark.parametrize('precision', FP32_MODES)
@pytest.mark.parametrize('layout', ['joint', 'masked'])
def test_asking_for_input_gradients_changes_no_parameter_gradient(tiny, precision, layout):
    grads = []
    for want in (False, True):
        m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision)
        m.uniter_model.deterministic = True
        m.param_store().zero_grads()
        _run(m, tiny, layout, True, 'zero', want=want)
        grads.append(m.param_store().flat_grads.clone())
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize('precision', FP32_MODES)
def test_fully_frozen_model_still_returns_input_gradients(tiny, precision):
    ref = _reference(tiny, 'joint', False, 'zero')
    m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision)
    for p in m.parameters():
        p.requires_grad = False
    _, g = _run(m, tiny, 'joint', False, 'zero')
    for k in ('feat', 'pos7', 'rows'):
        assert g[k] is not None
        _check(g[k], ref[k], k)


@pytest.mark.parametrize('precision', FP32_MODES)
def test_frozen_prefix_with_input_gradients_runs_the_full_pass(tiny, precision):
    ref = _reference(tiny, 'joint', True, 'rand')
    m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision)
    assert m.uniter_model.freeze_prefix(1) == 1
    m.param_store().zero_grads()
    _, g = _run(m, tiny, 'joint', True, 'rand')
    for k in ('feat', 'pos7', 'rows'):
        _check(g[k], ref[k], k)
    for n, p in m.named_parameters():
        if p.requires_grad:
            r = ref['params'][n]
            assert maxdiff(p.grad, r) <= _bound(r), n
    # without an input gradient the pass still stops above the frozen prefix: layer 0 and the embeddings receive nothing
    m.param_store().zero_grads()
    _run(m, tiny, 'joint', True, 'rand', want=False)
    assert float(m.uniter_model.encoder.layer[0].output.dense.weight.grad.abs().max()) == 0.0


@pytest.mark.parametrize('precision', FP32_MODES)
def test_packed_input_gradients_match_padded_and_oracle(tiny, precision):
    # eval mode, as tests/test_packed_gpu.py compares the layouts: the packed layout draws the hidden dropout's masks by packed row,
    # so only without dropout is it the padded computation (and the oracle's) element for element
    ref = _reference(tiny, 'joint', False, 'rand')
    lens = [int(x) for x in batch_from_npz(tiny)['attn_mask'].sum(1).tolist()]
    m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision)
    m.uniter_model.pack_padded = True
    _, g = _run(m, tiny, 'joint', False, 'rand', seq_lens=lens)
    for k in ('feat', 'pos7', 'rows'):
        _check(g[k], ref[k], 'packed ' + k)


@pytest.mark.parametrize('precision', ['fp32', 'fp32x3', 'bf16'])
def test_deterministic_input_gradients_repeat_bit_for_bit(tiny, precision):
    runs = []
    for _ in range(3):
        m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision)
        m.uniter_model.deterministic = True
        _, g = _run(m, tiny, 'masked', True, 'rand')
        runs.append(g)
    for k in ('feat', 'pos7', 'rows'):
        assert torch.isfinite(runs[0][k]).all() and float(runs[0][k].abs().max()) > 0
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k


def test_bf16_region_gradient_meets_the_two_sided_criterion():
    """precision 'bf16', B = 8, R = 36, D = 64 (18432 values): rms(kernels - fp32 oracle) <= 1.6 x rms(bf16 oracle - fp32 oracle)
    (DESIGN section 2).  The reference quantity is computed first, on the host, and has to be a usable yardstick at this size."""
    from meme_challenge_amd.trainer import bce_with_logits_loss
    from meme_challenge_amd.utils import make_synthetic_batch
    B, T, R = 8, 12, 36
    sd = O.synth_state_dict(TINY, seed=5, img_dim=TINY_IMG_DIM, ln_jitter=0.05)
    tl = [12, 9, 12, 5, 12, 7, 12, 10]
    nb = [36, 30, 36, 36, 20, 36, 36, 33]
    b = make_synthetic_batch(B, T, R, seed=77, vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM, txt_lens=tl, num_bbs=nb)
    kw = dict(input_ids=b['input_ids'], position_ids=b['position_ids'], img_feat=b['img_feat'], img_pos_feat=b['img_pos_feat'],
              attention_mask=b['attn_mask'], gather_index=b['gather_index'], output_all_encoded_layers=False)

    def oracle(prec):
        feat = b['img_feat'].clone().requires_grad_(True)
        lo = O.meme_uniter_forward({k: v.clone() for k, v in sd.items()}, TINY, prec=prec, **dict(kw, img_feat=feat))
        S.bce_with_logits(lo, b['labels'], POS_WT).backward()
        return feat.grad.double()

    g32, g16 = oracle('fp32'), oracle('bf16')
    own = (g16 - g32).pow(2).mean().sqrt().item()
    scale = g32.pow(2).mean().sqrt().item()
    print('oracle bf16 vs fp32: rms %.3e of rms %.3e' % (own, scale))
    assert own > 1e-4 * scale and np.isfinite(own), 'the bf16 oracle\'s own error is no yardstick at this size: enlarge R'
    m = build(TINY, TINY_IMG_DIM, sd, 'bf16').eval()
    feat = b['img_feat'].cuda().requires_grad_(True)
    dk = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
    logits = m(**dict(dk, img_feat=feat))
    bce_with_logits_loss(logits, b['labels'].cuda(), POS_WT).backward()
    torch.cuda.synchronize()
    err = (feat.grad.cpu().double() - g32).pow(2).mean().sqrt().item()
    print('kernels bf16 vs fp32 oracle: rms %.3e, ratio %.3f' % (err, err / own))
    assert err <= 1.6 * own, (err, own, err / own)


@pytest.mark.parametrize('precision', FP32_MODES)
def test_input_saliency_scores_and_parameter_gradients(tiny, precision):
    from meme_challenge_amd.attribution import input_saliency
    m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision).train()
    st = m.param_store()
    st.zero_grads()
    st.flat_grads.copy_(torch.randn(st.flat_grads.shape, generator=torch.Generator().manual_seed(3)).cuda())
    before = st.flat_grads.clone()
    b = to_dev(batch_from_npz(tiny))
    sal = input_saliency(m, b)
    torch.cuda.synchronize()
    assert m.training                                               # the mode is restored
    assert torch.equal(st.flat_grads, before)                       # ... and so is every parameter gradient, as the docstring says
    # d sum(logits): the oracle's gradients of the same scalar
    sd = {k: v.double() for k, v in sd_from_npz(tiny).items()}
    hb = batch_from_npz(tiny)
    B, T = hb['input_ids'].shape
    feat = hb['img_feat'].double().requires_grad_(True)
    words = sd[WORD][hb['input_ids'].view(-1)]
    rows = words.clone().requires_grad_(True)
    kw = _kwargs(hb, 'joint')
    kw.update(img_feat=feat, img_pos_feat=hb['img_pos_feat'].double(), input_ids=torch.arange(B * T).view(B, T))
    O.meme_uniter_forward(dict(sd, **{WORD: rows}), TINY, **kw).sum().backward()
    gr = rows.grad.view(B, T, -1)
    _check(sal.img_feat_grad, feat.grad, 'img_feat_grad')
    _check(sal.txt_grad, gr, 'txt_grad')
    # the scores are the norms and the gradient x input sums of those gradients
    g, x = sal.img_feat_grad.double(), b['img_feat'].double()
    assert maxdiff(sal.region_norm, g.norm(dim=-1)) <= 1e-6 * float(g.norm(dim=-1).max())
    assert maxdiff(sal.region_gxi, (g * x).sum(-1)) <= 1e-5 * float((g * x).abs().sum(-1).max())
    g, x = sal.txt_grad.double(), words.view(B, T, -1).cuda()
    assert maxdiff(sal.token_norm, g.norm(dim=-1)) <= 1e-6 * float(g.norm(dim=-1).max())
    assert maxdiff(sal.token_gxi, (g * x).sum(-1)) <= 1e-5 * float((g * x).abs().sum(-1).max())
    assert tuple(sal.region_norm.shape) == (B, hb['img_feat'].shape[1]) and tuple(sal.token_gxi.shape) == (B, T)
    assert tuple(sal.img_pos_feat_grad.shape) == (B, hb['img_feat'].shape[1], 7)
