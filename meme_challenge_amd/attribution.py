"""Which regions and which tokens moved the classifier?  Gradient saliency of a `MemeUniter` with respect to its inputs.

The reference inspects its mistakes by listing them (utils/misclassification.py); the step from a wrong prediction to the
regions and words behind it needs the gradient of the logit with respect to the image-region features and the word
embeddings, which `UniterModel.forward` exposes (csrc/input_grads.hip: `img_feat.grad`, and the gradient of a zero
`txt_embed_delta`, which is the per-token gradient of the word rows).

And what does the encoder's attention look like?  `UniterModel.output_attentions` makes a forward pass leave every layer's
probabilities softmax(QK^T / 8 + mask) (model/layer.py:85-95, before the dropout; csrc/attn_probs.hip) in `last_attentions`:
`attention_maps` returns them for a batch, `attention_rollout` multiplies the head-mean maps through the layers (Abnar & Zuidema 2020,
uniter_attn_rollout) and reads off what reaches [CLS], and `split_joint` maps scores over the joint sequence back to tokens and
regions.

And which of that attention moved THIS logit?  `UniterModel.output_attention_grads` makes the backward pass leave every layer's
gradient-weighted attention g = p * d target / d p (csrc/attn_grad.hip) in `last_attention_grads` and every head's sum of g in
`last_head_grads`: `attention_gradients` returns them for a batch, `attention_relevance` propagates the head means of max(g, 0)
through the layers (Chefer, Gur & Wolf 2021, uniter_attn_relevance) and reads off row [CLS], and `head_importance` turns the head sums
of many batches into Michel et al.'s (2019) importance score per head."""
from collections import namedtuple

import torch

Saliency = namedtuple('Saliency', 'region_norm region_gxi token_norm token_gxi img_feat_grad img_pos_feat_grad txt_grad logits')
AttentionMaps = namedtuple('AttentionMaps', 'probs logits')
Rollout = namedtuple('Rollout', 'joint cls_token cls_region logits')
AttentionGrads = namedtuple('AttentionGrads', 'maps head_grads logits')
Relevance = namedtuple('Relevance', 'joint cls_token cls_region logits')

MODEL_KEYS = ('input_ids', 'position_ids', 'img_feat', 'img_pos_feat', 'attention_mask', 'gather_index', 'img_masks',
              'txt_type_ids', 'img_type_ids', 'seq_lens')


def _model_kwargs(batch):
    """the keyword arguments of `MemeUniter.forward` out of a batch (``attn_mask`` is accepted for ``attention_mask``)"""
    kw = {k: batch[k] for k in MODEL_KEYS if k in batch and batch[k] is not None}
    if 'attention_mask' not in kw and batch.get('attn_mask') is not None:
        kw['attention_mask'] = batch['attn_mask']
    for k in ('input_ids', 'position_ids', 'img_feat', 'img_pos_feat'):
        kw.setdefault(k, None)
    kw['output_all_encoded_layers'] = False
    return kw


class _Run:
    feat = pos7 = delta = words = logits = None


def _eval_backward(model, batch, target, attention_grads=None):
    """One eval-mode forward with gradients and one backward of the logits' sum (or of ``target(logits)``) with the batch's inputs
    as differentiable leaves -- what `input_saliency` and `attention_gradients` share.  Returns a `_Run` (the leaves, the word rows,
    the detached logits).  Whatever happens, the flat gradient buffer is restored bit for bit afterwards, with the store's
    bookkeeping (which tensors were touched, the lazy zero_grad's flag), and so are the model's train / eval mode and
    ``output_attention_grads`` (set to ``attention_grads`` for the pass)."""
    from .model import ensure_store
    uniter = model.uniter_model
    kw = _model_kwargs(batch)
    store = ensure_store(model)
    saved = store.flat_grads.clone()
    saved_touched, saved_stale = set(store.touched), store.wgrad_stale
    was_training, was_setting = model.training, uniter.output_attention_grads
    model.eval()
    uniter.output_attention_grads = attention_grads
    run = _Run()
    try:
        with torch.enable_grad():
            if kw['img_feat'] is not None:
                run.feat = kw['img_feat'].detach().float().requires_grad_(True)
                run.pos7 = kw['img_pos_feat'].detach().float().requires_grad_(True)
                kw['img_feat'], kw['img_pos_feat'] = run.feat, run.pos7
            if kw['input_ids'] is not None:
                run.words = uniter.embeddings.word_embeddings.weight.detach()[kw['input_ids']]
                run.delta = torch.zeros_like(run.words).requires_grad_(True)
                kw['txt_embed_delta'] = run.delta
            logits = model(**kw)
            out = logits.sum() if target is None else target(logits)
            out.backward()
            run.logits = logits.detach()
    finally:
        store.flat_grads.copy_(saved)
        store.touched.clear()
        store.touched.update(saved_touched)
        store.wgrad_stale = saved_stale
        uniter.output_attention_grads = was_setting
        model.train(was_training)
    return run


def input_saliency(model, batch, target=None):
    """One eval-mode forward with gradients and one backward of the logits' sum (or of ``target(logits)``, a scalar).

    ``batch``: the keyword arguments of `MemeUniter.forward` (``attn_mask`` is accepted for ``attention_mask``, other keys
    such as ``labels`` are ignored), on the model's device.  Returns a `Saliency`:

    * ``region_norm`` [B, R]: L2 norm of d target / d img_feat per region; ``region_gxi`` [B, R]: gradient x input summed
      over the feature dimension;
    * ``token_norm`` / ``token_gxi`` [B, T]: the same per token, the input being the token's word-embedding row;
    * the raw gradients (``img_feat_grad`` [B, R, D], ``img_pos_feat_grad`` [B, R, 7], ``txt_grad`` [B, T, H]) and the
      detached ``logits``.  A modality the batch lacks gives None.

    Parameter gradients: the backward pass accumulates into the parameters' ``.grad`` (the flat gradient buffer) like any
    other; this function saves that buffer before the pass and RESTORES it afterwards, bit for bit, together with the
    store's bookkeeping (which tensors were touched, the lazy zero_grad's flag).  The model's train / eval mode is restored.
    The library keeps the activations of one forward per model, so this call must not sit between another forward and its
    backward."""
    run = _eval_backward(model, batch, target)
    feat, pos7, delta, words, logits = run.feat, run.pos7, run.delta, run.words, run.logits

    def scores(g, x):
        return (None, None) if g is None else (g.norm(dim=-1), (g * x.detach()).sum(dim=-1))
    rn, rg = scores(feat.grad if feat is not None else None, feat)
    tn, tg = scores(delta.grad if delta is not None else None, words)
    return Saliency(rn, rg, tn, tg, feat.grad if feat is not None else None, pos7.grad if pos7 is not None else None,
                    delta.grad if delta is not None else None, logits)



def attention_maps(model, batch, heads='mean'):
    """Every layer's attention probabilities for ``batch`` (keys as for `input_saliency`): one eval-mode forward under ``no_grad`` with
    ``UniterModel.output_attentions = heads``.  Returns `AttentionMaps`: ``probs`` [nl, B, L, L] (``heads='mean'``, the mean over
    heads) or [nl, B, nh, L, L] (``'all'``), row i = what joint position i attends to, and the detached ``logits``.  The model's
    train / eval mode and ``output_attentions`` are restored.  Like any forward, this call must not sit between another forward and
    its backward."""
    if heads not in ('mean', 'all'):
        raise ValueError("heads must be 'mean' or 'all'")
    uniter = model.uniter_model
    kw = _model_kwargs(batch)
    was_training, was_output = model.training, uniter.output_attentions
    model.eval()
    uniter.output_attentions = heads
    try:
        with torch.no_grad():
            logits = model(**kw)
        probs = uniter.last_attentions
    finally:
        uniter.output_attentions = was_output
        model.train(was_training)
    return AttentionMaps(probs, logits.detach())


def attention_rollout(model, batch, residual=0.5, start_layer=0):
    """Attention rollout of the head-mean maps of layers ``start_layer`` .. nl - 1: R = A~_(nl-1) ... A~_(start_layer) with
    A~_l = residual I + (1 - residual) A_l per sample (uniter_attn_rollout; fp32, no renormalisation: the rows of A_l sum to 1).
    Returns `Rollout`: ``joint`` [B, L, L]; ``cls_token`` [B, T] and ``cls_region`` [B, R], row 0 of ``joint`` -- how much of each
    input position reaches [CLS] -- mapped back to tokens and regions with `split_joint` (None for a modality the batch lacks);
    the detached ``logits``."""
    from . import _lib
    maps = attention_maps(model, batch, 'mean')
    probs = maps.probs
    nl, B, L = probs.shape[0], probs.shape[1], probs.shape[2]
    if not 0 <= int(start_layer) < nl:
        raise ValueError('start_layer must lie in [0, %d)' % nl)
    attn = probs[int(start_layer):].contiguous()
    joint, tmp = torch.empty_like(attn[0]), torch.empty_like(attn[0])
    _lib.check(_lib.lib().uniter_attn_rollout(_lib.ptr(attn), _lib.ptr(joint), _lib.ptr(tmp), attn.shape[0], B, L, float(residual),
                                              _lib.cur_stream()), 'uniter_attn_rollout')
    tok, reg = _split_cls(joint, batch)
    return Rollout(joint, tok, reg, maps.logits)


def _split_cls(joint, batch):
    """row [CLS] of ``joint`` [B, L, L] as ([B, T] or None, [B, R] or None)"""
    kw = _model_kwargs(batch)
    T = kw['input_ids'].shape[1] if kw['input_ids'] is not None else 0
    R = kw['img_feat'].shape[1] if kw['img_feat'] is not None else 0
    tok, reg = split_joint(joint[:, 0], kw.get('gather_index') if T and R else None, kw['attention_mask'], T, R)
    return tok if T else None, reg if R else None


def attention_gradients(model, batch, target=None, heads='relu_mean'):
    """Every layer's gradient-weighted attention for ``batch`` (keys as for `input_saliency`): one eval-mode forward with gradients and
    one backward of the logits' sum (or of ``target(logits)``, a scalar) with ``UniterModel.output_attention_grads = heads``.
    Returns `AttentionGrads`: ``maps`` -- g = p * d target / d p per head [nl, B, nh, L, L] (``heads='all'``, signed), or the mean
    over heads of max(g, 0) [nl, B, L, L] (``'relu_mean'``, the layer maps of Chefer et al. 2021); ``head_grads`` [nl, B, nh], the
    sum of g over each head's map = d target / d (a gate on that head); the detached ``logits``.  The flat gradient buffer and the
    store's bookkeeping are restored bit for bit, and so are the train / eval mode and ``output_attention_grads``.  Like any
    forward, this call must not sit between another forward and its backward."""
    if heads not in ('relu_mean', 'all'):
        raise ValueError("heads must be 'relu_mean' or 'all'")
    uniter = model.uniter_model
    run = _eval_backward(model, batch, target, heads)
    return AttentionGrads(uniter.last_attention_grads, uniter.last_head_grads, run.logits)


def attention_relevance(model, batch, target=None, start_layer=0):
    """Relevance of every joint position for the target (Chefer, Gur & Wolf 2021, the single-stream rule): with A_l the 'relu_mean'
    map of layer l, R = I, then R <- R + A_l R for l = ``start_layer`` .. nl - 1 per sample (uniter_attn_relevance; fp32).
    Returns `Relevance`: ``joint`` [B, L, L]; ``cls_token`` [B, T] and ``cls_region`` [B, R], row 0 of ``joint`` -- the relevance of
    each input position for what [CLS] holds -- mapped back to tokens and regions with `split_joint` (None for a modality the batch
    lacks); the detached ``logits``.  ``joint`` includes the identity R started from: entry [0, 0] of every sample carries [CLS]'s
    own 1, and so does ``cls_token[:, 0]``; subtract it (or drop that position) before ranking the tokens."""
    from . import _lib
    grads = attention_gradients(model, batch, target, 'relu_mean')
    nl, B, L = grads.maps.shape[:3]
    if not 0 <= int(start_layer) < nl:
        raise ValueError('start_layer must lie in [0, %d)' % nl)
    maps = grads.maps[int(start_layer):].contiguous()
    joint, tmp = torch.empty_like(maps[0]), torch.empty_like(maps[0])
    _lib.check(_lib.lib().uniter_attn_relevance(_lib.ptr(maps), _lib.ptr(joint), _lib.ptr(tmp), maps.shape[0], B, L, _lib.cur_stream()),
               'uniter_attn_relevance')
    tok, reg = _split_cls(joint, batch)
    return Relevance(joint, tok, reg, grads.logits)


def head_importance(model, batches, target=None, normalize=True):
    """Michel, Levy & Neubig (2019): the importance of head h of layer l is |E_x d target / d gate_lh|, the expectation over the
    samples of ``batches`` (an iterable of batches) of `attention_gradients`' ``head_grads``.  Returns [nl, nh]; with ``normalize``
    each layer is divided by its L2 norm (their section 4), a layer of zeros staying zeros."""
    total, count = None, 0
    for batch in batches:
        hg = attention_gradients(model, batch, target, 'relu_mean').head_grads.double()
        total = hg.sum(1) if total is None else total + hg.sum(1)
        count += hg.shape[1]
    if total is None:
        raise ValueError('head_importance needs at least one batch')
    imp = (total / count).abs()
    if normalize:
        norm = imp.norm(dim=1, keepdim=True)
        imp = imp / torch.where(norm > 0, norm, torch.ones_like(norm))
    return imp.float()


def split_joint(scores, gather_index, attention_mask, T, R):
    """Scores over the joint sequence ``scores`` [B, L] back to the inputs: ([B, T], [B, R]).  Joint position l of sample b is token
    ``gather_index[b, l]`` when that is < T, else region ``gather_index[b, l] - T`` (model/model.py:327-333); positions whose
    ``attention_mask`` is 0 are dropped, and a token or region no position maps to gets 0.  ``gather_index=None`` (text only or
    regions only) is the identity: position l is token l, or region l - T.  Pure torch, any device."""
    B, L = scores.shape
    gi = gather_index if gather_index is not None else torch.arange(L, device=scores.device).unsqueeze(0).expand(B, L)
    gi = gi.to(torch.int64)
    valid = (attention_mask != 0) & (gi >= 0) & (gi < T + R)
    out = torch.zeros(B, T + R + 1, dtype=scores.dtype, device=scores.device)
    out.scatter_(1, torch.where(valid, gi, torch.full_like(gi, T + R)), torch.where(valid, scores, torch.zeros_like(scores)))
    return out[:, :T], out[:, T:T + R]
