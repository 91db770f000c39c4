"""Which regions and which tokens moved the classifier?  Gradient saliency of a `MemeUniter` with respect to its inputs.

The reference inspects its mistakes by listing them (utils/misclassification.py); the step from a wrong prediction to the
regions and words behind it needs the gradient of the logit with respect to the image-region features and the word
embeddings, which `UniterModel.forward` exposes (csrc/input_grads.hip: `img_feat.grad`, and the gradient of a zero
`txt_embed_delta`, which is the per-token gradient of the word rows)."""
from collections import namedtuple

import torch

Saliency = namedtuple('Saliency', 'region_norm region_gxi token_norm token_gxi img_feat_grad img_pos_feat_grad txt_grad logits')

MODEL_KEYS = ('input_ids', 'position_ids', 'img_feat', 'img_pos_feat', 'attention_mask', 'gather_index', 'img_masks',
              'txt_type_ids', 'img_type_ids', 'seq_lens')


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
    from .model import ensure_store
    uniter = model.uniter_model
    kw = {k: batch[k] for k in MODEL_KEYS if k in batch and batch[k] is not None}
    if 'attention_mask' not in kw and batch.get('attn_mask') is not None:
        kw['attention_mask'] = batch['attn_mask']
    for k in ('input_ids', 'position_ids', 'img_feat', 'img_pos_feat'):
        kw.setdefault(k, None)
    kw['output_all_encoded_layers'] = False
    store = ensure_store(model)
    saved = store.flat_grads.clone()
    saved_touched, saved_stale = set(store.touched), store.wgrad_stale
    was_training = model.training
    model.eval()
    try:
        with torch.enable_grad():
            feat = pos7 = delta = words = None
            if kw['img_feat'] is not None:
                feat = kw['img_feat'].detach().float().requires_grad_(True)
                pos7 = kw['img_pos_feat'].detach().float().requires_grad_(True)
                kw['img_feat'], kw['img_pos_feat'] = feat, pos7
            if kw['input_ids'] is not None:
                words = uniter.embeddings.word_embeddings.weight.detach()[kw['input_ids']]
                delta = torch.zeros_like(words).requires_grad_(True)
                kw['txt_embed_delta'] = delta
            logits = model(**kw)
            out = logits.sum() if target is None else target(logits)
            out.backward()
    finally:
        store.flat_grads.copy_(saved)
        store.touched.clear()
        store.touched.update(saved_touched)
        store.wgrad_stale = saved_stale
        model.train(was_training)

    def scores(g, x):
        return (None, None) if g is None else (g.norm(dim=-1), (g * x.detach()).sum(dim=-1))
    rn, rg = scores(feat.grad if feat is not None else None, feat)
    tn, tg = scores(delta.grad if delta is not None else None, words)
    return Saliency(rn, rg, tn, tg, feat.grad if feat is not None else None, pos7.grad if pos7 is not None else None,
                    delta.grad if delta is not None else None, logits.detach())

