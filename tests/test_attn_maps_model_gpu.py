"""`UniterModel.output_attentions` / `last_attentions` and `attribution.attention_maps`, `attention_rollout` on the tiny model of
tests/common.py and the golden batch (B = 3, L = 16, two samples with 6 masked positions).

Reference: the oracle's `uniter_forward(..., return_embed=True)` -- float64 for the fp32 forms, its bf16-rounding arithmetic (prec='bf16',
fp32 tensors) for the bf16 mode -- gives every layer's input; the probabilities are softmax(q k^T / 8 + mask) in float64 of that input's
query and key projections (`O.linear(..., 'bf16', True)` in the bf16 mode: the bf16 values the kernels read).  In train mode the oracle
replays the same Philox dropout, and the captured values are those BEFORE the attention dropout.

Cases: 'fp32', 'fp32x3', 'bf16'; 'mean' and 'all'; padded in eval and train mode, packed (pack_padded) in eval mode.  A packed train
forward is checked structurally only (rows sum to 1, padding 0, outputs unchanged by the capture): in train mode the packed layout draws
the hidden dropout by packed row, so the oracle is not its reference (tests/test_model_gpu.py compares the packed layout in eval mode only
for the same reason).

Tolerance.  The hidden states that feed Q and K carry the model's own error, so no closed form: max |got - oracle| was measured per mode
on an MI355X over all the cases above (profiles/attn_maps_parity.txt), and the assertion is 4 x that, for the fp32 forms capped at 2e-4:

    mode     measured    asserted
    fp32     4.759e-08   1.904e-07
    fp32x3   5.057e-08   2.023e-07
    bf16     4.491e-08   1.796e-07      (against the oracle's bf16 arithmetic; far below the smallest mutation / 10 = 2.5e-4)

The cap keeps the test sharp: on this batch the oracle's own mutations differ from it by far more (test_mutations_are_far_above_the_
tolerances recomputes them on the CPU: layer 1's input in layer 0 2.5e-3, heads swapped 1.8e-2, layers swapped 2.0e-2, mask dropped
6.9e-2, transposed 1.1e-1, post-dropout values -- p / 9 or p -- 1.1e-1), the smallest >= 10 x the cap."""
import numpy as np
import pytest
import torch

from oracle import uniter_oracle as O
from oracle import philox
from common import TINY, TINY_IMG_DIM, sd_from_npz, batch_from_npz, model_kwargs
import attn_probs_ref as PR

MODES = ['fp32', 'fp32x3', 'bf16']
SEED, OFFSET = 0x5EED5EED1234, 9
FP32_CAP = 2e-4
# max |got - oracle| measured on an MI355X per mode (profiles/attn_maps_parity.txt) and the asserted tolerance: 4 x that, capped
MEASURED = {'fp32': 4.759e-8, 'fp32x3': 5.057e-8, 'bf16': 4.491e-8}
TOL = {m: (4 * e if m == 'bf16' else min(4 * e, FP32_CAP)) for m, e in MEASURED.items()}
WORST = {}
NL, NH = TINY['num_hidden_layers'], TINY['num_attention_heads']


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's probabilities
# ---------------------------------------------------------------------------------------------------------------------------
def _probs_of(sd, layer, x, mask, prec, drop_mask=True):
    """float64 [B, nh, L, L] of `layer`'s query / key weights applied to the input x"""
    a = 'uniter_model.encoder.layer.%d.attention.self.' % layer
    rnd = prec != 'fp32'
    B, L, H = x.shape
    q = O.linear(x, sd[a + 'query.weight'], sd[a + 'query.bias'], prec, rnd).double().view(B, L, NH, 64).permute(0, 2, 1, 3)
    k = O.linear(x, sd[a + 'key.weight'], sd[a + 'key.bias'], prec, rnd).double().view(B, L, NH, 64).permute(0, 2, 1, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) / 8.0
    if drop_mask:
        s = s + ((1.0 - mask.double()) * -10000.0)[:, None, None, :]
    return torch.softmax(s, dim=-1)


_ORACLE = {}


def oracle(tiny, prec, train):
    """dict(probs [nl, B, nh, L, L] float64, inputs: every layer's input, sd, mask), computed once per (arithmetic, mode), read only"""
    key = (prec, train)
    if key in _ORACLE:
        return _ORACLE[key]
    dt = torch.float64 if prec == 'fp32' else torch.float32
    sd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd_from_npz(tiny).items()}
    b = batch_from_npz(tiny)
    kw = dict(model_kwargs(b), output_all_encoded_layers=True)
    kw['img_feat'], kw['img_pos_feat'] = kw['img_feat'].to(dt), kw['img_pos_feat'].to(dt)
    drop = O.DropSpec(SEED, OFFSET, TINY['hidden_dropout_prob'], TINY['attention_probs_dropout_prob']) if train else None
    with torch.no_grad():
        layers, emb = O.uniter_forward(sd, TINY, drop=drop, prefix='uniter_model.', return_embed=True, prec=prec, **kw)
        xs = [emb] + list(layers[:-1])
        probs = torch.stack([_probs_of(sd, l, x, b['attn_mask'], prec) for l, x in enumerate(xs)])
    out = dict(probs=probs, inputs=xs + [layers[-1]], sd=sd, mask=b['attn_mask'])
    _ORACLE[key] = out
    return out


def test_mutations_are_far_above_the_tolerances(tiny):
    """CPU: what each wrong capture would differ by from the oracle on this batch; the smallest is >= 10 x the fp32 cap and >= 10 x
    the bf16 tolerance"""
    o = oracle(tiny, 'fp32', False)
    ref, sd, xs, mask = o['probs'], o['sd'], o['inputs'], o['mask']
    with torch.no_grad():
        muts = {
            "layer 1's input in layer 0": (_probs_of(sd, 0, xs[1], mask, 'fp32') - ref[0]).abs().max().item(),
            'heads swapped': (ref.flip(2) - ref).abs().max().item(),
            'layers swapped': (ref.flip(0) - ref).abs().max().item(),
            'mask dropped': max((_probs_of(sd, l, xs[l], mask, 'fp32', drop_mask=False) - ref[l]).abs().max().item() for l in range(NL)),
            'transposed': (ref.transpose(-1, -2) - ref).abs().max().item(),
        }
        # post-dropout values: p * keep / (1 - 0.1), i.e. off by p / 9 or by p
        B, L = mask.shape
        Lp = (L + 3) // 4 * 4
        idx = (torch.arange(B * NH * L, dtype=torch.int64).view(B, NH, L, 1) * Lp + torch.arange(L, dtype=torch.int64).view(1, 1, 1, L))
        spec = O.DropSpec(SEED, OFFSET, 0.1, 0.1)
        dropped = O._apply_dropout(ref[0].clone(), 0.1, spec, philox.site_attn_probs(0), index=idx)
        muts['post-dropout values'] = (dropped - ref[0]).abs().max().item()
    print('\n' + '\n'.join('%-28s %.3e' % kv for kv in muts.items()))
    smallest = min(muts.values())
    assert smallest >= 10 * FP32_CAP, muts
    assert max(TOL.values()) <= smallest / 10, (TOL, muts)
    for m in ('fp32', 'fp32x3'):
        assert TOL[m] <= FP32_CAP


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
def _model(tiny, precision, train, packed=False, deterministic=False):
    from test_model_gpu import build
    m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny), precision)
    m = m.train() if train else m.eval()
    m.uniter_model.pack_padded = packed
    m.uniter_model.deterministic = deterministic
    return m


def _forward(m, tiny, heads, packed=False, all_layers=True):
    """one forward of the encoder from the same dropout state -> (hidden layers stacked, last_attentions)"""
    u = m.uniter_model
    u.set_dropout_seed(SEED, OFFSET)
    b = {k: v.cuda() for k, v in batch_from_npz(tiny).items()}
    kw = dict(model_kwargs(b), output_all_encoded_layers=all_layers)
    if packed:
        kw['seq_lens'] = [int(n) for n in batch_from_npz(tiny)['attn_mask'].sum(1).tolist()]
    u.output_attentions = heads
    out = u(**kw)
    torch.cuda.synchronize()
    return (torch.stack(out) if all_layers else out).detach(), u.last_attentions


def _lens(tiny):
    return [int(n) for n in batch_from_npz(tiny)['attn_mask'].sum(1).tolist()]


def _err(got, ref, lens=None):
    """max |got - ref|; lens: over the rows and columns of each sample that exist (packed), the rest must be exact zeros"""
    got = got.double().cpu()
    if lens is None:
        return (got - ref).abs().max().item()
    err = 0.0
    for b, n in enumerate(lens):
        err = max(err, (got[:, b, ..., :n, :n] - ref[:, b, ..., :n, :n]).abs().max().item())
        assert not got[:, b, ..., n:, :].any() and not got[:, b, ..., :, n:].any(), 'padding of a packed sample must be exact zeros'
    return err


CASES = [(False, False), (False, True), (True, False)]      # (packed, train)


@pytest.mark.gpu
@pytest.mark.parametrize('packed,train', CASES, ids=['padded-eval', 'padded-train', 'packed-eval'])
@pytest.mark.parametrize('precision', MODES)
def test_captured_probabilities_match_the_oracle(tiny, precision, packed, train):
    ref = oracle(tiny, 'bf16' if precision == 'bf16' else 'fp32', train)['probs']
    m = _model(tiny, precision, train, packed)
    lens = _lens(tiny) if packed else None
    hid_off, none = _forward(m, tiny, None, packed)
    assert none is None and m.uniter_model.last_attentions is None
    for heads in ('mean', 'all'):
        hid, got = _forward(m, tiny, heads, packed)
        B, L = 3, 16
        assert got.dtype == torch.float32 and not got.requires_grad
        assert tuple(got.shape) == ((NL, B, L, L) if heads == 'mean' else (NL, B, NH, L, L))
        err = _err(got, ref.mean(2) if heads == 'mean' else ref, lens)
        WORST[precision] = max(WORST.get(precision, 0.0), err)
        print('%s %s %s %s: max |got - oracle| %.3e (asserted %.3e)' % (precision, 'packed' if packed else 'padded',
                                                                        'train' if train else 'eval', heads, err, TOL[precision]))
        assert err <= TOL[precision], (precision, packed, train, heads, err)
        # the capture changes no output: every layer's hidden states bit for bit
        assert torch.equal(hid, hid_off), (precision, heads)
    # ... and does not survive into the next forward: nothing is captured and the tensor handed out before keeps its bits
    kept, copy = got, got.clone()
    _, none = _forward(m, tiny, None, packed)
    assert none is None and m.uniter_model.last_attentions is None and torch.equal(kept, copy)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', MODES)
def test_packed_train_forward_captures_pre_dropout_probabilities(tiny, precision):
    m = _model(tiny, precision, True, packed=True)
    hid_off, _ = _forward(m, tiny, None, True)
    hid, got = _forward(m, tiny, 'all', True)
    assert torch.equal(hid, hid_off)
    got = got.double().cpu()
    for b, n in enumerate(_lens(tiny)):
        assert not got[:, b, :, n:, :].any() and not got[:, b, :, :, n:].any()
        # rows sum to 1 and nothing is scaled by 1 / 0.9 or zeroed: these are the values before the dropout
        assert (got[:, b, :, :n, :n].sum(-1) - 1.0).abs().max().item() < 1e-5
        assert (got[:, b, :, :n, :n] > 0).all()


@pytest.mark.gpu
def test_report_measured_errors():
    print('\nmax |got - oracle| per mode: ' + ', '.join('%s %.3e' % kv for kv in sorted(WORST.items())))


@pytest.mark.gpu
@pytest.mark.parametrize('precision', MODES)
def test_logits_are_bit_identical_with_the_capture_on(tiny, precision):
    for train in (False, True):
        m = _model(tiny, precision, train)
        b = {k: v.cuda() for k, v in batch_from_npz(tiny).items()}
        outs = []
        for heads in (None, 'all', 'mean', None):
            m.uniter_model.set_dropout_seed(SEED, OFFSET)
            m.uniter_model.output_attentions = heads
            outs.append(m(**model_kwargs(b)).detach().clone())
            assert (m.uniter_model.last_attentions is None) == (heads is None)
        assert all(torch.equal(outs[0], o) for o in outs[1:]), (precision, train)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', MODES)
def test_backward_after_a_capturing_forward_gives_the_same_gradients(tiny, precision):
    from meme_challenge_amd.trainer import bce_with_logits_loss
    grads = []
    for heads in (None, 'all'):
        m = _model(tiny, precision, True, deterministic=True)
        m.param_store().zero_grads()
        m.uniter_model.set_dropout_seed(SEED, OFFSET)
        m.uniter_model.output_attentions = heads
        b = {k: v.cuda() for k, v in batch_from_npz(tiny).items()}
        bce_with_logits_loss(m(**model_kwargs(b)), b['labels'], 1.8).backward()
        torch.cuda.synchronize()
        assert (m.uniter_model.last_attentions is None) == (heads is None)
        grads.append(m.param_store().flat_grads.clone())
    assert float(grads[0].abs().max()) > 0 and torch.equal(grads[0], grads[1])


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32x3', 'bf16'])
def test_attention_maps_and_rollout(tiny, precision):
    from meme_challenge_amd.attribution import attention_maps, attention_rollout, split_joint
    m = _model(tiny, precision, True, deterministic=True)
    u = m.uniter_model
    u.output_attentions = 'all'
    hb = batch_from_npz(tiny)
    b = {k: v.cuda() for k, v in hb.items()}
    B, T = hb['input_ids'].shape
    Rn = hb['img_feat'].shape[1]
    maps = attention_maps(m, b)
    assert m.training and u.output_attentions == 'all'              # both restored
    assert tuple(maps.probs.shape) == (NL, B, 16, 16) and tuple(maps.logits.shape) == (B, 1)
    every = attention_maps(m, b, heads='all')
    assert tuple(every.probs.shape) == (NL, B, NH, 16, 16)
    ref = PR.share(maps.probs.double().cpu().numpy(), every.probs.double().mean(2).cpu().numpy(),
                   (NH + 2) * PR.U * every.probs.double().mean(2).cpu().numpy() + PR.TINY)
    assert ref <= 1.0, ref                                          # 'mean' is the mean of 'all' (one eval forward each, same bits)
    for res, start in ((0.5, 0), (0.0, 1)):
        roll = attention_rollout(m, b, residual=res, start_layer=start)
        torch.cuda.synchronize()
        assert m.training and u.output_attentions == 'all'
        want, bound = PR.rollout_reference(maps.probs[start:].cpu().numpy(), res)[-1]
        sh = PR.share(roll.joint.double().cpu().numpy(), want, bound)
        print('%s rollout residual %g from layer %d: share %.3f' % (precision, res, start, sh))
        assert sh <= 1.0, (res, start, sh)
        tok, reg = split_joint(roll.joint[:, 0].cpu(), hb['gather_index'], hb['attn_mask'], T, Rn)
        assert torch.equal(roll.cls_token.cpu(), tok) and torch.equal(roll.cls_region.cpu(), reg)
        assert tuple(tok.shape) == (B, T) and tuple(reg.shape) == (B, Rn)
        assert torch.equal(roll.logits, maps.logits)
    with pytest.raises(ValueError):
        attention_rollout(m, b, start_layer=NL)
    with pytest.raises(ValueError):
        attention_maps(m, b, heads='first')
