"""The call forms of UniterModel.forward and their CPU reference (test infrastructure; tests/test_call_forms_cpu.py and
tests/test_call_forms_gpu.py share it).

A call form is (layout, mode, modality, which layers are returned, which of them the loss reads).  reference_step runs one
oracle step of a form -- oracle.uniter_oracle's forward in 'fp32' or 'bf16' arithmetic, in float32 or float64 storage, torch
autograd behind it -- and returns the per-layer outputs, logits, loss and every parameter gradient as float64 arrays.

Dropout of the packed layout.  UniterModel.pack_padded hands the library the Mp = sum(seq_lens) valid rows only
(model.py: _pack; csrc/model.cpp: make_plan with Mrows = Mp).  What the three kinds of dropout site index by then, as read
from csrc/model.cpp and the kernels:
  * hidden dropout behind the attention output and behind the FFN output of every layer (ln_fwd / ln_bwd: the row passes get
    pl.M = Mp rows): element r * H + c with r(b, l) = sum(seq_lens[:b]) + l the PACKED row -- oracle.uniter_oracle.packed_hidden_index;
  * attention probabilities: ((b * nh + h) * L + i) * Lp + j with the PADDED L and Lp = L rounded up to 4, as in the padded layout (the
    kernels address a query by sample and local position, with or without cu_seqlens);
  * the text and region embeddings: unchanged (dropout runs on the [B, T] / [B, R] blocks, before the gather into packed rows).
The oracle still computes padded positions in a packed form (with the keep flag of element 0); the reference's loss multiplies
by the valid mask, so they reach nothing.

The loss.  BCE of the head on the last layer (pos_weight 1.8) where the form uses a head, plus on every listed layer l
    sum(P_l * h_l) / Mv + QUAD / 2 * sum(Q_l * h_l ^ 2) / Mv          (h_l at valid positions, Mv = number of valid positions)
with fixed random P_l ~ (1 + l / 2) N(0, 1) and Q_l ~ U(0.5, 1.5) of the layer's shape, another draw per layer: every listed
layer gets its own, non-uniform upstream gradient of about 1e-2 per element.
"""
import numpy as np
import torch

from oracle import uniter_oracle as O
from oracle import step_oracle as S

CFG = dict(vocab_size=997, hidden_size=512, num_hidden_layers=3, num_attention_heads=8, intermediate_size=1024,
           hidden_act='gelu', hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, max_position_embeddings=160,
           type_vocab_size=2, initializer_range=0.02)
IMG_DIM = 128
NL, H = CFG['num_hidden_layers'], CFG['hidden_size']
STATE_SEED, LN_JITTER = 3, 0.05
B, T, R = 3, 40, 36
TXT_LENS, NUM_BBS = [40, 2, 17], [36, 36, 1]
BATCH_SEED = 17
DROP_SEED, DROP_OFFSET = 0xC0FFEE, 4
POS_WEIGHT = 1.8
QUAD = 0.3
PROBE_SEED = 101

# form -> packed layout, train mode, modality, img_masks, output_all_encoded_layers, layers the loss probes, head in the loss
FORMS = {
    'all_train':             dict(packed=False, train=True,  modality='joint', masks=False, all_layers=True,  probes=(0, 1, 2), head=True),
    'all_eval_grad':         dict(packed=False, train=False, modality='joint', masks=False, all_layers=True,  probes=(0, 1, 2), head=True),
    'mid_only':              dict(packed=False, train=True,  modality='joint', masks=False, all_layers=True,  probes=(1,),      head=False),
    'packed_train':          dict(packed=True,  train=True,  modality='joint', masks=False, all_layers=False, probes=(),        head=True),
    'packed_all_train':      dict(packed=True,  train=True,  modality='joint', masks=False, all_layers=True,  probes=(0, 1, 2), head=True),
    'txt_only_train':        dict(packed=False, train=True,  modality='txt',   masks=False, all_layers=False, probes=(2,),      head=False),
    'img_only_train':        dict(packed=False, train=True,  modality='img',   masks=False, all_layers=False, probes=(2,),      head=False),
    'img_masks_train':       dict(packed=False, train=True,  modality='joint', masks=True,  all_layers=False, probes=(),        head=True),
    'packed_txt_only_train': dict(packed=True,  train=True,  modality='txt',   masks=False, all_layers=False, probes=(2,),      head=False),
}

# the fp32 bars (tests/test_model_gpu.py: test_tiny_forward_matches_reference_golden, test_edge_shapes_match_oracle)
LAYER_BAR = 2e-5
LOGIT_BAR = 2e-5


def grad_bar(ref):
    return 3e-6 + 3e-4 * float(np.abs(ref).max())


def state_dict():
    return O.synth_state_dict(CFG, seed=STATE_SEED, img_dim=IMG_DIM, ln_jitter=LN_JITTER)


def batch(txt_lens=None, num_bbs=None):
    tl, nbb = txt_lens or TXT_LENS, num_bbs or NUM_BBS
    b = O.synth_batch(B, T, R, seed=BATCH_SEED, vocab=CFG['vocab_size'], img_dim=IMG_DIM, txt_lens=tl, num_bbs=nbb)
    g = torch.Generator().manual_seed(BATCH_SEED + 1)
    b['img_masks'] = torch.randint(0, 2, (B, R), generator=g)
    b['img_masks'][:, 0] = 1                        # every sample masks a valid region
    b['txt_lens'], b['num_bbs'] = list(tl), list(nbb)
    return b


def seq_lens(form, b):
    mod = FORMS[form]['modality']
    return [(t if mod != 'img' else 0) + (n if mod != 'txt' else 0) for t, n in zip(b['txt_lens'], b['num_bbs'])]


def attention_mask(form, b):
    """[B, L] float32, right-padded; L = the longest sample of the form's modality"""
    lens = seq_lens(form, b)
    L = {'joint': b['attn_mask'].shape[1], 'txt': T, 'img': R}[FORMS[form]['modality']]
    return (torch.arange(L).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).float()


def forward_kwargs(form, b):
    """what UniterModel.forward / the oracle's uniter_forward take for the form (CPU tensors; seq_lens is the caller's to add)"""
    f = FORMS[form]
    txt, img = f['modality'] != 'img', f['modality'] != 'txt'
    kw = dict(input_ids=b['input_ids'] if txt else None, position_ids=b['position_ids'] if txt else None,
              img_feat=b['img_feat'] if img else None, img_pos_feat=b['img_pos_feat'] if img else None,
              attention_mask=attention_mask(form, b), gather_index=b['gather_index'] if txt and img else None,
              output_all_encoded_layers=f['all_layers'])
    if f['masks']:
        kw['img_masks'] = b['img_masks']
    return kw


def probes(form, b, dtype=torch.float32):
    """layer -> (P_l, Q_l), each [B, L, H]; the same values in either dtype"""
    L = attention_mask(form, b).shape[1]
    out = {}
    for l in FORMS[form]['probes']:
        g = torch.Generator().manual_seed(PROBE_SEED + l)
        p = torch.randn(B, L, H, generator=g) * (1.0 + 0.5 * l)
        q = torch.rand(B, L, H, generator=g) + 0.5
        out[l] = (p.to(dtype), q.to(dtype))
    return out


def form_loss(form, layers, logits, labels, valid, pq, masked=True, bce=S.bce_with_logits):
    """the form's loss from {layer index: [B, L, H]}, the head's logits (or None), labels [B], valid [B, L, 1] and probes()'s
    tensors (on the layers' device).  masked=False leaves the valid mask out of the probe terms: the same value when the padded
    positions hold zeros, and a gradient on padded positions.  Returns (loss, the head's share of it or None).  bce: the head's loss function (the GPU test passes the project's)."""
    f = FORMS[form]
    total = head = None
    if f['head']:
        total = head = bce(logits, labels, POS_WEIGHT)
    mv = valid.sum()
    for l in f['probes']:
        h = layers[l] * valid if masked else layers[l]
        p, q = pq[l]
        term = (p * h).sum() / mv + 0.5 * QUAD * (q * h * h).sum() / mv
        total = term if total is None else total + term
    return total, head


def reference_step(form, prec='fp32', dtype=torch.float32, b=None, p_drop=None, packed_index=None):
    """One oracle step of the form.  prec: 'fp32' | 'bf16' (oracle.uniter_oracle); dtype float64 widens weights and inputs.
    p_drop overrides both dropout probabilities; packed_index overrides whether the packed layout's hidden-dropout index is
    replayed (default: the form's layout).  Returns float64 arrays: 'layer/<l>' (zero at padded positions) for every returned
    layer, 'logits' and 'head_loss' (the BCE term alone) where the form has a head, 'loss', 'grad/<name>' for every parameter (zeros where autograd left none),
    'loss_bar' (the fp32 bar of the loss, below)."""
    f = FORMS[form]
    b = b if b is not None else batch()
    wide = lambda t: t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in state_dict().items()}
    kw = {k: wide(v) for k, v in forward_kwargs(form, b).items()}
    cfg = dict(CFG)
    if p_drop is not None:
        cfg['hidden_dropout_prob'] = cfg['attention_probs_dropout_prob'] = p_drop
    drop = O.DropSpec(DROP_SEED, DROP_OFFSET, cfg['hidden_dropout_prob'], cfg['attention_probs_dropout_prob']) if f['train'] else None
    L = kw['attention_mask'].shape[1]
    use_packed = f['packed'] if packed_index is None else packed_index
    hidx = O.packed_hidden_index(seq_lens(form, b), L, H) if use_packed else None
    outs = O.uniter_forward(sd, cfg, drop=drop, prefix='uniter_model.', prec=prec, hidden_index=hidx, **kw)
    layers = dict(enumerate(outs)) if f['all_layers'] else {NL - 1: outs}
    logits = None
    if f['head']:
        pooled = O.pooler(sd, 'uniter_model.', layers[NL - 1])
        logits = torch.nn.functional.linear(pooled, sd['linear.weight'], sd['linear.bias'])
    valid = kw['attention_mask'].unsqueeze(-1)
    pq = probes(form, b, dtype)
    loss, head_loss = form_loss(form, layers, logits, b['labels'], valid, pq)
    loss.backward()
    out = {'loss': float(loss.detach())}
    if head_loss is not None:
        out['head_loss'] = float(head_loss.detach())
    for l, h in layers.items():
        out['layer/%d' % l] = (h.detach() * valid).double().numpy()
    if logits is not None:
        out['logits'] = logits.detach().double().numpy()
    for n, v in sd.items():
        out['grad/' + n] = (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy()
    # The fp32 bar of the loss, first order in the bars of what it reads: |d BCE / d logit| <= pos_weight (mean over the batch), each
    # probed element moves the loss by (|P| + QUAD Q |h|) / Mv per unit; plus 1e-6 max(1, |loss|) for the float32 sums of the loss itself
    bar = (POS_WEIGHT * LOGIT_BAR if f['head'] else 0.0) + 1e-6 * max(1.0, abs(out['loss']))
    mv = float(valid.sum())
    for l in f['probes']:
        p, q = pq[l]
        bar += LAYER_BAR * float(((p.abs() + QUAD * q * layers[l].detach().abs()) * valid).sum()) / mv
    out['loss_bar'] = bar
    return out


def fp32_shares(got, ref):
    """tensor name -> |got - ref| as a share of the fp32 bar: layers and logits 2e-5, gradients 3e-6 + 3e-4 max|ref|, the loss its
    first-order bar (reference_step).  got: the same keys as ref (float arrays; 'loss' a float)"""
    out = {}
    for k, r in ref.items():
        if k == 'loss_bar':
            continue
        if k in ('loss', 'head_loss'):
            # (the head's term alone: |d BCE / d logit| <= pos_weight, plus the float32 rounding of a loss of order 1)
            out[k] = abs(float(got[k]) - r) / (ref['loss_bar'] if k == 'loss' else POS_WEIGHT * LOGIT_BAR + 1e-6)
            continue
        d = float(np.abs(np.asarray(got[k], dtype=np.float64) - r).max())
        out[k] = d / (grad_bar(r) if k.startswith('grad/') else LOGIT_BAR if k == 'logits' else LAYER_BAR)
    return out


def plan_pieces(lib, M, avail_cus=0):
    """k-pieces the library's plan hands the query|key|value input gradient [M, N = H, K = 3 H] between layers by default
    (csrc/model.cpp make_plan: ns_k3h), per precision, from the host-only planners:
      fp32x3  uniter_gemm_x3_plan on the backward pass's CUs (x3_choose's cost model);
      bf16    the default schedule takes gemm_bf16v2_pick_split (csrc/gemm_bf16_dma.hip; no C ABI of its own), restated here: four
              pieces with <= 128 tiles of 128 x 128 and >= 48 k-tiles of 64, two with <= 320 tiles and >= 24 k-tiles; the persistent
              kernels' planner uniter_gemm_bf16p_plan (UNITER_B16_PERSIST bit 2) is asked as well and returned as 'bf16p';
      fp32    always one (the native fp32 products have no k-piece slabs)."""
    import ctypes as C
    cfg, ns = C.c_int(), C.c_int()
    assert lib.uniter_gemm_x3_plan(M, H, 3 * H, avail_cus, 0, C.byref(cfg), C.byref(ns)) == 0
    x3 = ns.value
    assert lib.uniter_gemm_bf16p_plan(M, H, 3 * H, avail_cus, 0, 0, C.byref(cfg), C.byref(ns)) == 0
    b16p = ns.value
    tiles, nk = ((M + 127) // 128) * ((H + 127) // 128), (3 * H + 63) // 64
    v2 = 4 if (tiles <= 128 and nk >= 48) else 2 if (tiles <= 320 and nk >= 24) else 1
    return {'fp32': 1, 'fp32x3': x3, 'bf16': v2, 'bf16p': b16p}
