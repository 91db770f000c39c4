"""GPU: every call form of UniterModel.forward against the CPU oracle, in the three precisions.

The other model-level tests drive the encoder through one call form (joint padded batch, the last layer alone, train mode).
This file drives the others -- all-layer outputs with a gradient on every layer, the packed layout in train mode, text-only /
image-only / img_masks inputs in train mode, eval mode with gradients -- and compares every returned layer, the logits, the loss
and every parameter gradient with tests/call_forms_ref.py (forms, loss, packed dropout index: see its docstring; the CPU side is
tested by tests/test_call_forms_cpu.py).  It runs in-process: no switch is involved.

Config and batch (tests/call_forms_ref.py): three layers, so layer 1 is neither first nor last; hidden 512 with 8 heads,
intermediate 1024, 160 positions, img_dim 128, ln_jitter 0.05 weights; B = 3, T = 40, R = 36, txt_lens [40, 2, 17], num_bbs
[36, 36, 1]: M = 228 padded rows, L = 76, 132 packed rows (59 text-only); dropout seed 0xC0FFEE, offset 4.

k-pieces.  With a gradient on every layer csrc/model.cpp adds each layer's slice of d_hidden to the next layer's dx (dsum) and
forces ONE k-piece where the plan would hand the query|key|value input gradient [M, N = H, K = 3 H] between layers as k-piece
slabs.  At H = 512 the planners say (test_the_shape_splits_the_qkv_input_gradient asserts > 1; the same for M = 228, 132, 59):
fp32x3 4 pieces (uniter_gemm_x3_plan: 48 k-tiles of 32, one round of tiles), bf16 2 pieces (gemm_bf16v2_pick_split's rule, 24
k-tiles of 64 -- the default schedule's; uniter_gemm_bf16p_plan answers 2 as well), fp32 always 1: the native fp32 mode offers no
shape that splits, its all-layer cases test the gradient injection alone.

Packed dropout index: hidden sites by PACKED row r(b, l) * H + c, attention probabilities and embedding sites as in the padded
layout (oracle.uniter_oracle.packed_hidden_index's docstring).  Every packed form passes with it and fails without it (below).

Bars (none new).  fp32 and fp32x3, against the float32 oracle: layer outputs and logits 2e-5, each gradient 3e-6 + 3e-4 max|ref|
(test_model_gpu.py), the loss first-order in those (call_forms_ref.reference_step), a tensor the oracle leaves exactly zero
exactly zero.  The float32 oracle is within 0.10 (layers), 0.0031 (logits), 0.0036 (gradients) of these bars from the float64
oracle in every form (tests/test_call_forms_cpu.py asserts < 1 / 4).  bf16: the two-sided form, check_bf16.

Measured on an MI355X, worst share of each bar over the nine forms:
  precision   layer outputs            logits               loss (head's term)   gradients
  fp32        0.12 (all_train, 2)      0.0075               0.0032               0.0073 (img_only_train, layer 2 query weight)
  fp32x3      0.095                    0.0058               0.0032               0.012  (img_only_train, layer 0 query weight)
  bf16        0.59 (img_only_train)    0.54 (all_train)     0.35                 0.74   (img_masks_train, layer 1 key weight)
  Wall time per test 0.10 - 0.31 s (library step 0.09 - 0.23 s, the oracle 0.1 s, once per form and arithmetic), the first 1.0 s
  (loads the library); the module 8 s.  No form found a fault in the library.

Planted in a scratch build, one at a time:
  (a) uniter_model_backward_layer takes dy = layers[l + 1].dx with all_layers set (the dsum dropped): all_train, all_eval_grad,
      mid_only and packed_all_train fail in all three precisions (12 tests, 45 tensors each), the other 16 pass; worst gradient at
      3.0e3 - 3.3e3 x its bar in fp32 and fp32x3, 480 - 2.0e3 x in bf16.
  (b) the LayerNorm backward row pass replays the PADDED row's flags for sample 2 of the packed joint batch (rows 114 .. 131 of
      132 draw element (row + 38) * H + c, both hidden sites): packed_train and packed_all_train fail in all three precisions (6
      tests, 58 tensors each; worst gradient 790 - 815 x its bar in fp32 and fp32x3, 264 - 358 x in bf16), everything else passes
      (packed_txt_only_train has 59 rows and is not touched by this plant).

Safety on shared machines: in-process, one step per test; after an error that names a GPU fault no later test of this module
touches the GPU (they fail with that reason).
"""
import time

import numpy as np
import pytest
import torch

import call_forms_ref as R
from test_parity_configs_gpu import _two_sided_slack

pytestmark = pytest.mark.gpu

PRECISIONS = ['fp32', 'fp32x3', 'bf16']
STATE = {'dead': None, 'ref': {}, 'worst': {}}
FAULT_WORDS = ('illegal memory access', 'Memory access fault', 'HSA_STATUS_ERROR', 'hipErrorLaunchFailure', 'unspecified launch failure')


def reference(form, kind):
    """kind 'f32' | 'bf16': the float32 oracle in the reference arithmetic / with the bf16 mode's rounding points; once per module"""
    if (form, kind) not in STATE['ref']:
        STATE['ref'][(form, kind)] = R.reference_step(form, 'bf16' if kind == 'bf16' else 'fp32', torch.float32)
    return STATE['ref'][(form, kind)]


def hip_step(form, precision):
    """one step of the form on the library: the same keys as R.reference_step, float64 arrays"""
    from meme_challenge_amd.model import UniterConfig, UniterModel, pool_head
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.trainer import bce_with_logits_loss
    f = R.FORMS[form]
    cfg = UniterConfig.from_dict(R.CFG)
    m = MemeUniter(UniterModel(cfg, img_dim=R.IMG_DIM), cfg.hidden_size, 1)
    m.load_state_dict(R.state_dict(), strict=True)
    m = m.cuda()
    m = m.train() if f['train'] else m.eval()
    um = m.uniter_model
    um.precision = precision
    um.pack_padded = f['packed']
    um.set_dropout_seed(R.DROP_SEED, R.DROP_OFFSET)
    m.param_store().zero_grads()
    b = R.batch()
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in R.forward_kwargs(form, b).items()}
    if f['packed']:
        kw['seq_lens'] = R.seq_lens(form, b)
    outs = um(**kw)
    layers = dict(enumerate(outs)) if f['all_layers'] else {R.NL - 1: outs}
    logits = pool_head(layers[R.NL - 1], um.pooler, m.linear) if f['head'] else None
    valid = kw['attention_mask'].unsqueeze(-1)
    pq = {l: (p.cuda(), q.cuda()) for l, (p, q) in R.probes(form, b).items()}
    # packed: the probe is NOT masked on this side -- the padded positions hold zeros, so the loss is the same number, and its
    # gradient lands on padded positions too, which the library has to drop
    loss, head_loss = R.form_loss(form, layers, logits, b['labels'].cuda(), valid, pq, masked=not f['packed'], bce=bce_with_logits_loss)
    loss.backward()
    torch.cuda.synchronize()
    out = {'loss': float(loss.detach())}
    if head_loss is not None:
        out['head_loss'] = float(head_loss.detach())
    pad = (valid == 0).expand(-1, -1, R.H)
    for l, h in layers.items():
        h = h.detach()
        if f['packed']:
            assert pad.any() and float(h[pad].abs().max()) == 0.0, 'layer %d is not zero at the padded positions of a packed batch' % l
        out['layer/%d' % l] = (h * valid).double().cpu().numpy()
    if logits is not None:
        out['logits'] = logits.detach().double().cpu().numpy()
    for n, p in m.named_parameters():
        out['grad/' + n] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu().numpy()
    return out


def _rms_rel(got, ref):
    return float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))


def _zero_rule(k, got, ref, problems):
    """a tensor the oracle leaves exactly zero -- the absent modality's embeddings, what lies above the only probed layer, an unused
    mask embedding -- must come back exactly zero; True when the rule applied"""
    if k.startswith('grad/') and float(np.abs(ref[k]).max()) == 0.0:
        if float(np.abs(got[k]).max()) != 0.0:
            problems.append('%s must be exactly zero, max |g| = %.3g' % (k, np.abs(got[k]).max()))
        return True
    return False


def check_fp32(form, got, problems):
    ref = reference(form, 'f32')
    assert set(got) == set(ref) - {'loss_bar'}, sorted(set(got) ^ set(ref))
    shares = R.fp32_shares(got, ref)
    for k, s in shares.items():
        if _zero_rule(k, got, ref, problems):
            continue
        if not s <= 1.0:
            problems.append('%s at %.3g of its bar' % (k, s))
    return shares


def check_bf16(form, got, problems):
    """the two-sided per-tensor form (tests/test_schedule_switches_gpu.py: check_oracle_bf16): the rms-relative error against the exact
    (float32) oracle is at most factor x the bf16-rounding oracle's own + slack; logits and the head's loss within 2 x the rounding
    model's own distance + 2e-4; the key biases, mathematically zero, are noise below a fifth of the query bias.  The layer outputs are
    tensors like the gradients.  Returns tensor -> eh / (factor eo + slack)"""
    exact, model = reference(form, 'f32'), reference(form, 'bf16')
    assert set(got) == set(exact) - {'loss_bar'}, sorted(set(got) ^ set(exact))
    shares = {}
    for k, r in exact.items():
        if k in ('loss', 'loss_bar'):
            continue        # (the probes' share of the loss is a function of the layer outputs, held per tensor below)
        if k in ('logits', 'head_loss'):
            d = float(np.abs(np.asarray(got[k]) - r).max())
            bar = 2.0 * float(np.abs(np.asarray(model[k]) - r).max()) + 2e-4
            shares[k] = d / bar
            if not d <= bar:
                problems.append('%s %.3g from the exact oracle, the rounding model %.3g' % (k, d, (bar - 2e-4) / 2))
            continue
        if _zero_rule(k, got, exact, problems):
            continue
        if k.endswith('attention.self.key.bias'):
            qb = got[k.replace('key.bias', 'query.bias')]
            shares[k] = float(np.abs(got[k]).max()) / (0.2 * float(np.abs(qb).max()) + 1e-12)
            if not shares[k] <= 1.0:
                problems.append('%s is not noise: %.3g against a query bias of %.3g' % (k, np.abs(got[k]).max(), np.abs(qb).max()))
            continue
        eh, eo = _rms_rel(got[k], r), _rms_rel(model[k], r)
        fac, slack = _two_sided_slack(k[len('grad/'):] if k.startswith('grad/') else k, got[k].size)
        shares[k] = eh / (fac * eo + slack)
        if not eh <= fac * eo + slack:
            problems.append('%s rms-relative %.3g, the rounding model %.3g' % (k, eh, eo))
    return shares


def test_the_shape_splits_the_qkv_input_gradient():
    """all-layers forces ONE k-piece where the plan hands the query|key|value input gradient [M, H, 3 H] between layers as slabs:
    the planners must say that it would be more than one at this shape, padded (M = 228) and packed (M = 132, text-only 59)"""
    from meme_challenge_amd import _lib
    lib = _lib.lib()
    seen = {}
    for M in (228, 132, 59):
        p = R.plan_pieces(lib, M)
        seen[M] = p
        assert p['fp32x3'] > 1 and p['bf16'] > 1 and p['bf16p'] > 1, (M, p)
    print('k-pieces of the QKV input gradient by rows:', seen)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('form', list(R.FORMS))
def test_call_form_matches_oracle(form, precision):
    if STATE['dead']:
        pytest.fail('not run: a GPU fault earlier in this module (%s)' % STATE['dead'])
    t0 = time.time()
    try:
        got = hip_step(form, precision)
    except Exception as e:
        if any(w in str(e) for w in FAULT_WORDS):
            STATE['dead'] = '%s %s: %s' % (form, precision, str(e)[:200])
        raise
    t_hip = time.time() - t0
    problems = []
    shares = check_bf16(form, got, problems) if precision == 'bf16' else check_fp32(form, got, problems)
    worst = {}
    for k, s in shares.items():
        kind = k.split('/')[0]
        if s >= worst.get(kind, (-1.0, None))[0]:
            worst[kind] = (s, k)
    print('%s %s: library step %.2f s, with the oracle %.2f s; worst shares %s; %d problems'
          % (form, precision, t_hip, time.time() - t0, {k: '%.3g (%s)' % v for k, v in worst.items()}, len(problems)))
    assert not problems, (form, precision, len(problems), problems[:12])
