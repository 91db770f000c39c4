"""GPU: the encoder across its configuration space against float64 (tests/config_space_ref.py has the cases, the reference, the bars
and the mutations; tests/test_config_space_cpu.py shows that the bars can see what they are meant to see).

Every (configuration, precision) pair the setters accept runs every form below; every pair they refuse is refused before a kernel
runs, with a message naming the sizes, and the same model then runs in fp32:

  step           MemeUniter, eval with gradients and train with replayed dropout: logits, loss, every parameter gradient; in
                 fp32x3 with head_rows_only on and off
  all layers     uniter_model(output_all_encoded_layers=True) in eval: every layer's hidden state
  packed         pack_padded, eval with gradients: hidden states at valid positions (zeros elsewhere), logits, loss, gradients
  deterministic  train, twice from one seed: bit-equal logits and gradients, and within the bars
  mirror         one FusedAdam step, then a forward pass: the fp32x3 / bf16 weight mirror follows the optimizer, in the paired and in
                 the unpaired layout.  The oracle's Adam is fed the gradients the device computed (they are held to float64 by the
                 step form): a first Adam step is lr * g / (|g| + eps), a sign, so feeding it the float64 gradients instead would
                 turn every element whose gradient is noise into a +-lr disagreement that says nothing about the mirror.

Measured on an MI355X (worst share of its bar over all configurations, forms and tensors; <= 1 passes; the module's 102 tests
take 6.5 s, 4 s of it in the tests themselves):

  precision    logits  loss   gradients  hidden states  logits after an Adam step
  fp32         0.012   0.002  0.009      0.220          -
  fp32x3       0.009   0.002  0.005      0.185          0.018
  bf16         0.167   0.079  0.628      0.097          0.304
  bf16_hybrid  0.403   0.374  0.709      0.426          -

  worst cases: fp32 / fp32x3 gradients at h320_i100 (token-type embeddings) and h1024_i1056_l1 (pos_linear.bias), hidden states at
  h1024_i1056_l1; bf16 at h192_i320 (the only configuration it accepts), a value bias in train mode; bf16_hybrid gradients at
  h128_i32 (pos_layer_norm.weight, 128 elements), logits and loss at h1024_i1056_l1.  The median eh / eo of the bf16 legs is 0.96 - 0.98
  for 'bf16' and 0.70 - 0.86 for 'bf16_hybrid' (whose attention stays in fp32, so it is closer to float64 than the rounding model):
  the two-sided factors calibrated at UNITER-base size hold for tensors of a few thousand elements, on the batch of the fp32 legs.
  The planted mutations of tests/config_space_ref.py, for scale: 100 x to 1900 x the fp32 gradient bars, 6 x to 1600 x the bf16 form.
"""
import time

import numpy as np
import pytest
import torch

import config_space_ref as CS
from common import model_kwargs

pytestmark = pytest.mark.gpu

STATE = {'dead': None, 'worst': {}, 't0': None}
FAULT_WORDS = ('illegal memory access', 'Memory access fault', 'HSA_STATUS_ERROR', 'hipErrorLaunchFailure', 'unspecified launch failure')
BF16_MODES = ('bf16', 'bf16_hybrid')
X3_ROWS = [(n, p, hr) for n, p in CS.LEGAL for hr in ((True, False) if p == 'fp32x3' else (True,))]


@pytest.fixture(autouse=True)
def _no_run_after_a_fault():
    """a GPU fault ends the module: nothing is started on a device that has faulted"""
    if STATE['dead']:
        pytest.fail('not run: a GPU fault earlier in this module (%s)' % STATE['dead'])
    if STATE['t0'] is None:
        STATE['t0'] = time.time()


def _remember_fault(e, what):
    if any(w in str(e) for w in FAULT_WORDS):
        STATE['dead'] = '%s: %s' % (what, str(e)[:200])


def build(name, precision='fp32', train=False):
    """as tests/test_model_gpu.py::build, on the configuration's shared state dict"""
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    cfg = UniterConfig.from_dict(CS.cfg(name))
    m = MemeUniter(UniterModel(cfg, img_dim=CS.img_dim(name)), cfg.hidden_size, 1)
    m.load_state_dict(CS.state_dict(name), strict=True)
    m.uniter_model.precision = precision
    m = m.cuda()
    m = m.train() if train else m.eval()
    m.uniter_model.set_dropout_seed(CS.DROP_SEED, CS.DROP_OFFSET)
    return m


def dev_kwargs(name):
    return model_kwargs({k: v.cuda() for k, v in CS.batch(name).items()})


def _grads(m):
    return {'grad/' + n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu().numpy()
            for n, p in m.named_parameters()}


def hip_step(name, precision, train, head_rows=True, packed=False, deterministic=False):
    """one step on the library: the keys of CS.reference_step (float64 arrays), plus 'layer/<l>' for a packed step"""
    from meme_challenge_amd.model import pool_head
    from meme_challenge_amd.trainer import bce_with_logits_loss
    try:
        m = build(name, precision, train)
        m.head_rows_only = head_rows
        um = m.uniter_model
        um.pack_padded = packed
        um.deterministic = deterministic
        kw = dev_kwargs(name)
        out = {}
        if packed:
            kw = dict(kw, seq_lens=CS.seq_lens(), output_all_encoded_layers=True)
            m.param_store()
            layers = um(**kw)
            logits = pool_head(layers[-1], um.pooler, m.linear)
            for l, h in enumerate(layers):
                out['layer/%d' % l] = h.detach().double().cpu().numpy()
        else:
            seen = []
            hook = um.register_forward_hook(lambda mod, a, o: seen.append(float(o.detach()[:, 1:].abs().max())))
            logits = m(**kw)
            hook.remove()
            out['_rest'] = seen[0]          # the largest |value| of the encoder's output outside row 0 of every sample
        loss = bce_with_logits_loss(logits, CS.batch(name)['labels'].cuda(), CS.POS_WEIGHT)
        loss.backward()
        torch.cuda.synchronize()
        out.update(logits=logits.detach().double().cpu().numpy(), loss=float(loss.detach()))
        out.update(_grads(m))
        return out
    except Exception as e:
        _remember_fault(e, '%s %s' % (name, precision))
        raise


def _note(precision, what, share):
    key = (precision, what)
    STATE['worst'][key] = max(STATE['worst'].get(key, (0.0, '')), share)


def check_step(name, precision, train, got, tag):
    """hold a step to the bars of its precision; returns the shares"""
    ref = CS.reference_step(name, train)
    keys = {k: v for k, v in got.items() if not k.startswith(('layer/', '_'))}
    assert set(keys) == set(ref), sorted(set(keys) ^ set(ref))
    if precision in BF16_MODES:
        orc = CS.reference_step(name, train, None, 'bf16', torch.float32)
        noise = CS.bf16_noise(ref, orc)
        assert 1e-6 < noise < 2e-2, noise
        shares, ratios = CS.bf16_shares(keys, ref, orc)
        extra = ', median eh / eo %.2f over %d tensors (printed, not asserted), noise %.2e' % (float(np.median(ratios)), len(ratios), noise)
    else:
        shares, extra = CS.fp32_shares(keys, ref), ''
    wl, wg = shares['logits'], CS.worst(shares, 'grad/')
    print('%s %s %s: logits %.3f, loss %.3f, gradients %.3f (%s)%s' % (name, precision, tag, wl, shares['loss'], wg[0], wg[1], extra))
    _note(precision, 'logits', (wl, '%s %s' % (name, tag)))
    _note(precision, 'loss', (shares['loss'], '%s %s' % (name, tag)))
    _note(precision, 'gradients', (wg[0], '%s %s %s' % (name, tag, wg[1][5:])))
    bad = sorted(((v, k) for k, v in shares.items() if not v <= 1.0), reverse=True)
    assert not bad, '%s %s %s: %d over their bars, worst %s' % (name, precision, tag, len(bad), bad[:6])
    return shares


# ------------------------------------------------------------------------------------------------ step ---
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('name,precision,head_rows', X3_ROWS)
def test_step_against_float64(name, precision, head_rows, train):
    got = hip_step(name, precision, train, head_rows=head_rows)
    check_step(name, precision, train, got, ('train' if train else 'eval') + ('' if head_rows else ' every row'))
    # the short last layer (rows the head reads only) ran where it was asked for in fp32x3, and nowhere else
    assert (got['_rest'] == 0.0) == (head_rows and precision == 'fp32x3'), got['_rest']
    if precision in BF16_MODES:
        ref = CS.reference_step(name, train)
        assert np.abs(got['logits'] - ref['logits']).max() > 2e-6          # really ran on the bf16 pipe: 10 x what fp32 leaves


# ------------------------------------------------------------------------------------------------ all layers ---
def _check_layers(name, precision, layers, valid, tag):
    ref = CS.reference_layers(name)
    assert len(layers) == len(ref) == CS.cfg(name)['num_hidden_layers']
    if precision in BF16_MODES:
        orc = CS.reference_layers(name, 'bf16', torch.float32)
        noise = float((np.abs(orc[-1] - ref[-1]) * valid).max())
        todo, bar = [len(ref) - 1], 2.0 * noise + 2e-4
    else:
        todo, bar = range(len(ref)), CS.LAYER_BAR
    for l in todo:
        assert layers[l].shape == ref[l].shape
        s = float((np.abs(layers[l] - ref[l]) * valid).max()) / bar
        print('%s %s %s: layer %d at %.3f of its bar' % (name, precision, tag, l, s))
        _note(precision, 'hidden states', (s, '%s %s layer %d' % (name, tag, l)))
        assert s <= 1.0, (name, precision, tag, l, s)


@pytest.mark.parametrize('name,precision', CS.LEGAL)
def test_all_layers_against_float64(name, precision):
    try:
        m = build(name, precision)
        m.param_store()
        with torch.no_grad():
            layers = m.uniter_model(**dict(dev_kwargs(name), output_all_encoded_layers=True))
        layers = [h.double().cpu().numpy() for h in layers]
    except Exception as e:
        _remember_fault(e, '%s %s' % (name, precision))
        raise
    _check_layers(name, precision, layers, np.ones((1, 1, 1)), 'all layers')


# ------------------------------------------------------------------------------------------------ packed ---
@pytest.mark.parametrize('name,precision', CS.LEGAL)
def test_packed_step_against_float64(name, precision):
    got = hip_step(name, precision, False, packed=True)
    valid = CS.batch(name)['attn_mask'].double().numpy()[:, :, None]
    layers = [got['layer/%d' % l] for l in range(CS.cfg(name)['num_hidden_layers'])]
    for h in layers:
        assert (valid == 0).any() and np.abs(h * (1.0 - valid)).max() == 0.0          # padded positions of a packed batch are zeros
    _check_layers(name, precision, layers, valid, 'packed')
    check_step(name, precision, False, got, 'packed')


# ------------------------------------------------------------------------------------------------ deterministic ---
@pytest.mark.parametrize('name,precision,head_rows', X3_ROWS)
def test_deterministic_step_is_bit_equal_and_within_the_bars(name, precision, head_rows):
    a = hip_step(name, precision, True, head_rows=head_rows, deterministic=True)
    b = hip_step(name, precision, True, head_rows=head_rows, deterministic=True)
    differ = [k for k in a if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]
    assert not differ, differ
    check_step(name, precision, True, a, 'deterministic' + ('' if head_rows else ' every row'))
    assert (a['_rest'] == 0.0) == (head_rows and precision == 'fp32x3'), a['_rest']


# ------------------------------------------------------------------------------------------------ mirror ---
MIRROR = [(n, p) for n in ('h64_i96_l1', 'h192_i320', 'h1024_i1056_l1') for p in ('fp32x3', 'bf16') if CS.legal(n, p)]


@pytest.mark.parametrize('name,precision', MIRROR)
def test_the_mirror_follows_the_optimizer(name, precision):
    from meme_challenge_amd.trainer import FusedAdam, bce_with_logits_loss
    try:
        m = build(name, precision)
        opt = FusedAdam(m, lr=1e-3, weight_decay=0.0)
        kw = dev_kwargs(name)
        logits0 = m(**kw)
        bce_with_logits_loss(logits0, CS.batch(name)['labels'].cuda(), CS.POS_WEIGHT).backward()
        torch.cuda.synchronize()
        st = m.param_store()
        if precision == 'fp32x3':
            if name == 'h64_i96_l1':
                assert st.pair_dst() is None and not st.mirror_paired()          # really the unpaired layout
            if name == 'h192_i320':
                assert st.pair_dst() is not None and st.mirror_paired()
        p0 = [(n, p.detach().double().cpu().clone()) for n, p in m.named_parameters()]
        g0 = {n: p.grad.detach().double().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
        opt.step(grad_scale=1.0, max_grad_norm=5.0)
        with torch.no_grad():
            logits1 = m(**kw).double().cpu().numpy()
        logits0 = logits0.detach().double().cpu().numpy()
    except Exception as e:
        _remember_fault(e, '%s %s' % (name, precision))
        raise
    from oracle import step_oracle as S
    ora = S.AdamOracle(p0, lr=1e-3, weight_decay=0.0)
    total = float(torch.sqrt(sum((g ** 2).sum() for g in g0.values())))
    coef = S.clip_coef(total, 5.0)
    ora.step({n: g * coef for n, g in g0.items()})
    # the optimizer itself: the fp32 parameters follow the oracle's (float64) Adam to float32 round-off of an lr-sized update
    for n, p in m.named_parameters():
        d = float((p.detach().double().cpu() - ora.p[n]).abs().max())
        assert d <= 1e-2 * 1e-3, (n, d)
    ref = CS.reference_logits(name, ora.p)
    if precision == 'bf16':
        noise = float(np.abs(CS.reference_logits(name, {k: v.float() for k, v in ora.p.items()}, 'bf16', torch.float32) - ref).max())
        bar = 2.0 * noise + 2e-4
    else:
        bar = CS.LOGIT_BAR
    d, moved = float(np.abs(logits1 - ref).max()), float(np.abs(logits1 - logits0).max())
    print('%s %s: logits after the step at %.3f of their bar, moved by %.1f bars' % (name, precision, d / bar, moved / bar))
    _note(precision, 'logits after an Adam step', (d / bar, name))
    assert moved > 10.0 * bar, (moved, bar)
    assert d <= bar, (d, bar)


# ------------------------------------------------------------------------------------------------ refusals ---
@pytest.mark.parametrize('name,precision', CS.ILLEGAL)
def test_an_illegal_precision_is_refused_before_any_kernel(name, precision):
    c = CS.cfg(name)
    try:
        m = build(name, precision)
        with pytest.raises(ValueError) as ei:
            m(**dev_kwargs(name))
        assert 'intermediate_size' in str(ei.value) and precision in str(ei.value)
        assert m.uniter_model._applied_precision is None          # the library never heard of it
        m.uniter_model.precision = 'fp32'
        m.uniter_model.set_dropout_seed(CS.DROP_SEED, CS.DROP_OFFSET)
    except Exception as e:
        _remember_fault(e, '%s %s' % (name, precision))
        raise
    assert c['intermediate_size'] % (32 if precision == 'fp32x3' else 64)
    # the same model then runs in fp32, within its bars
    from meme_challenge_amd.trainer import bce_with_logits_loss
    try:
        logits = m(**dev_kwargs(name))
        loss = bce_with_logits_loss(logits, CS.batch(name)['labels'].cuda(), CS.POS_WEIGHT)
        loss.backward()
        torch.cuda.synchronize()
        got = dict(_grads(m), logits=logits.detach().double().cpu().numpy(), loss=float(loss.detach()))
    except Exception as e:
        _remember_fault(e, '%s fp32 after a refusal' % name)
        raise
    check_step(name, 'fp32', False, got, 'after refusing ' + precision)


@pytest.mark.parametrize('name,precision', CS.ILLEGAL)
def test_the_c_setter_refuses_with_both_sizes(name, precision):
    from meme_challenge_amd import _lib as L
    c = CS.cfg(name)
    m = build(name, 'fp32')
    st = m.param_store()
    um = m.uniter_model
    mirror = st.ensure_mirror(3 if precision == 'fp32x3' else 1)
    lib = L.lib()
    L.check(lib.uniter_model_set_weight_mirror(um._handle, L.ptr(st.flat_params), L.ptr(mirror), st.numel), 'uniter_model_set_weight_mirror')
    rc = lib.uniter_model_set_precision(um._handle, 3 if precision == 'fp32x3' else 2)
    msg = lib.uniter_last_error().decode('utf-8', 'replace')
    assert rc != 0, 'uniter_model_set_precision accepted %s at %s' % (precision, name)
    assert 'set_precision' in msg and '%d, %d' % (c['hidden_size'], c['intermediate_size']) in msg, msg
    with pytest.raises(L.UniterHipError):
        L.check(rc, 'uniter_model_set_precision')
    assert lib.uniter_model_set_precision(um._handle, 0) == 0


# ------------------------------------------------------------------------------------------------ report (last) ---
def test_zz_report_worst_shares():
    print('\nworst shares of the bars, per precision and output:')
    for (precision, what), (share, where) in sorted(STATE['worst'].items()):
        print('  %-12s %-26s %.3f  (%s)' % (precision, what, share, where))
    if STATE['t0'] is not None:
        print('module wall time %.0f s' % (time.time() - STATE['t0']))
