"""No result depends on what an uninitialised buffer held: every `torch.empty` of the package -- the model workspace the library
carves into its plan, outputs, scratch -- is poisoned (tests/poison.py) with zeros, 0xFF bytes, the bytes of 1.0f and the bytes a
pass over another batch left, and the results are the same bits; nothing is NaN under 0xFF; no guard band around the workspace, cut to
the end of its plan, is touched.  DESIGN.md ("Uninitialised memory") states the contract and lists the call sites.

Two models: TINY (tests/common.py) with B = 4, 16 tokens, 6 regions, and the configuration of tests/test_step_det_gpu.py (hidden 256,
4 heads, intermediate 1024, 2 layers, img_dim 2048; B = 16, 64 tokens, 32 regions: the smallest at which the heuristics pick the
split-K and stream-K forms; two layers also use the odd-layer ping-pong buffer of the inference plan).  Batches are ragged with one
sample at full length and one at length 1 (joint batches: one token and one region).  Dropout on with a fixed seed, side and
auxiliary streams on.  Models are built once per module; the whole-step trajectories build their own (they need the same start).

Invalid positions: in a packed batch the hidden outputs beyond a sample's length are exactly 0.0 whatever the buffer held (the
kernel writes them); a padded batch computes those positions like any other, so there the claim is bit-equality alone."""
import numpy as np
import pytest
import torch

from common import (MID, MID_IMG_DIM, TINY, TINY_IMG_DIM, build_meme_uniter, pretrain_dataset, pretrain_loader, pretrain_model, take,
                    trainer_config)
from poison import FILLS, WS_SLACK, Poison

pytestmark = pytest.mark.gpu

DET_ALL = 15
MODELS = {'tiny': (TINY, TINY_IMG_DIM, 4, 16, 6), 'mid': (MID, MID_IMG_DIM, 16, 64, 32)}
MODALITIES = ['txt+img', 'txt', 'img', 'img+masks']
ORDER = ('zeros', 'unit', 'replay', 'ones')          # 0xFF last: the fill that could turn a word somebody waits on into a wrong count
assert set(ORDER) == set(FILLS)
ROUNDOFF = {'fp32': 2e-5, 'fp32x3': 2e-5, 'bf16': 3e-3, 'bf16_hybrid': 3e-3}      # the bar of tests/test_model_det_gpu.py


@pytest.fixture(scope='module')
def dds(tmp_path_factory):
    return pretrain_dataset(tmp_path_factory)


@pytest.fixture(scope='module')
def models():
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    out = {}
    for name, (cfg, img_dim, _, _, _) in MODELS.items():
        c = UniterConfig.from_dict(cfg)
        torch.manual_seed(0)
        m = MemeUniter(UniterModel(c, img_dim=img_dim), c.hidden_size, 1).cuda().train()
        # LayerNorm weights and biases off their 1 / 0, the head off zero: every gradient is a number of its own
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if 'LayerNorm' in n or 'layer_norm' in n or n.endswith('.bias'):
                    p.add_((torch.rand(p.shape, generator=g) - 0.5).to(p.device) * 0.1)
        out[name] = m
    return out


def _lens(name):
    _, _, B, T, R = MODELS[name]
    rng = np.random.Generator(np.random.PCG64(77))
    tl = [int(x) for x in rng.integers(2, T + 1, size=B)]
    nbb = [int(x) for x in rng.integers(2, R + 1, size=B)]
    tl[0], nbb[0] = T, R            # one sample at full length
    tl[1], nbb[1] = 1, 1            # one at length 1
    return tl, nbb


def _batch(name, modality='txt+img', seed=3, lens=None, shape=None):
    """keyword arguments of UniterModel.forward (without output_all_encoded_layers), labels and the valid-position mask"""
    from meme_challenge_amd.utils import make_synthetic_batch
    cfg, img_dim, B, T, R = MODELS[name]
    if shape is not None:
        B, T, R = shape
    tl, nbb = lens if lens is not None else _lens(name)
    b = make_synthetic_batch(B, T, R, seed=seed, vocab=cfg['vocab_size'], img_dim=img_dim, txt_lens=tl, num_bbs=nbb, device='cuda')
    kw = dict(input_ids=b['input_ids'], position_ids=b['position_ids'], img_feat=b['img_feat'], img_pos_feat=b['img_pos_feat'],
              attention_mask=b['attn_mask'], gather_index=b['gather_index'], seq_lens=b['seq_lens'])
    if modality == 'txt':
        mask = (torch.arange(T, device='cuda').unsqueeze(0) < torch.tensor(tl, device='cuda').unsqueeze(1)).float()
        kw.update(img_feat=None, img_pos_feat=None, gather_index=None, attention_mask=mask, seq_lens=list(tl))
    elif modality in ('img', 'img+masks'):
        mask = (torch.arange(R, device='cuda').unsqueeze(0) < torch.tensor(nbb, device='cuda').unsqueeze(1)).float()
        kw.update(input_ids=None, position_ids=None, gather_index=None, attention_mask=mask, seq_lens=list(nbb))
        if modality == 'img+masks':
            g = torch.Generator().manual_seed(seed)
            kw['img_masks'] = ((torch.rand(B, R, generator=g) < 0.3).cuda() & mask.bool()).long()
    return kw, b['labels'], kw['attention_mask'].bool()


def _setup(m, precision, packed, deterministic, train=True):
    enc = m.uniter_model
    enc.precision, enc.pack_padded, enc.deterministic = precision, packed, deterministic
    enc.output_attentions = enc.output_attention_grads = None
    m.train(train)
    assert enc.use_side_stream
    return enc


def _fwd_bwd(m, kw, labels, valid, seed=(11, 0), **more):
    """forward with every layer as an output, a loss on the logits and on every layer's valid positions, backward"""
    from meme_challenge_amd.model import pool_head
    from meme_challenge_amd.trainer import bce_with_logits_loss
    enc = m.uniter_model
    enc.set_dropout_seed(*seed)
    m.zero_grad(set_to_none=False)
    m.param_store().zero_grads()
    layers = enc(output_all_encoded_layers=True, **kw, **more)
    logits = pool_head(layers[-1], enc.pooler, m.linear)
    loss = bce_with_logits_loss(logits.squeeze(1), labels, 1.8)
    loss = loss + 1e-3 * sum((l.masked_fill(~valid.unsqueeze(-1), 0.0) ** 2).sum() * (0.1 + i) for i, l in enumerate(layers))
    loss.backward()
    torch.cuda.synchronize()
    out = {'logits': logits.detach().clone(), 'layers': torch.stack([l.detach() for l in layers]).clone()}
    out.update({'grad:' + n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    return out


def _under_fills(run, other, order=ORDER, again=0):
    """run() under each fill; 'replay' takes its bytes from other(), a pass of another batch, seed and dropout offset through the
    same plan.  -> {fill: run()'s dict}, {fill: the Poison}; `again` more 'zeros' runs under the keys 'zeros2', 'zeros3', ..."""
    with Poison('zeros', capture=True) as cap:
        other()
    res, ps = {}, {}
    for fill in order + tuple('zeros%d' % (2 + i) for i in range(again)):
        with Poison(fill.rstrip('0123456789'), replay=cap.captured) as p:
            res[fill] = run()
        ps[fill] = p
        assert not p.broken and sum(p.sites.values()) > 0            # (a broken band raised at exit already)
        assert not p.passed_through, p.passed_through                # a call site the harness left to torch went unpoisoned
    return res, ps


def _assert_agree(res, precision):
    """the rule for the paths with float atomics: a forward output is the same bits under every fill where the runs under 'zeros'
    are the same bits among themselves; everything lies within the bar of tests/test_model_det_gpu.py -- the round-off of reordered
    sums (2e-5, bf16 3e-3, of the largest entry) plus four times what the 'zeros' runs differ by"""
    a = res['zeros']
    same = [res[k] for k in res if k.startswith('zeros') and k != 'zeros']
    assert same
    for fill in ORDER[1:]:
        r = res[fill]
        for k in a:
            noise = max((z[k] - a[k]).abs().max().item() for z in same)
            if noise == 0 and all(torch.equal(a[k], z[k]) for z in same) and not k.startswith('grad:'):
                assert torch.equal(a[k], r[k]), (fill, k, (r[k] - a[k]).abs().max().item())
            tol = ROUNDOFF[precision] * a[k].abs().max().item() + 4 * noise
            err = (r[k] - a[k]).abs().max().item()
            assert err <= tol, (fill, k, err, tol)                   # (NaN fails the comparison)
    _assert_finite(res['ones'], 'ones')


def _differing(a, b):
    assert set(a) == set(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def _assert_same_bits(res):
    for fill in res:
        bad = _differing(res['zeros'], res[fill])
        assert not bad, (fill, bad[:6], len(bad))


def _assert_finite(d, what):
    bad = [k for k, v in d.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]
    assert not bad, (what, bad[:6])


def _ws_sites(p):
    assert p.count('model.py:_get_ws') > 0, p.report()               # a silently inactive harness must fail
    ws = [r for r in p.records if ':_get_ws:' in r.site]
    assert ws and all(r.band == 65536 for r in ws)
    return ws


# ---- A: encoder forward + backward, deterministic ----------------------------------------------------------------------------
@pytest.mark.parametrize('modality', MODALITIES)
@pytest.mark.parametrize('packed', [False, True], ids=['padded', 'packed'])
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3', 'bf16'])
@pytest.mark.parametrize('name', list(MODELS))
def test_deterministic_pass_is_the_same_bits_under_every_fill(models, name, precision, packed, modality):
    from meme_challenge_amd import _lib
    m = models[name]
    enc = _setup(m, precision, packed, True)
    kw, labels, valid = _batch(name, modality, seed=3)
    kw2, labels2, valid2 = _batch(name, modality, seed=9)
    plain = _fwd_bwd(m, kw, labels, valid)
    assert enc.deterministic_coverage == DET_ALL and enc.bit_reproducible, enc.deterministic_missing()
    res, ps = _under_fills(lambda: _fwd_bwd(m, kw, labels, valid), lambda: _fwd_bwd(m, kw2, labels2, valid2, seed=(23, 5)))
    assert enc.deterministic_coverage == DET_ALL
    _assert_same_bits(res)
    assert not _differing(plain, res['zeros'])                       # ... and the harness itself changes nothing
    _assert_finite(res['ones'], 'ones')
    n_grads = sum(k.startswith('grad:') for k in plain)
    assert n_grads >= 8 + 16 * len(enc.encoder.layer) and all(v.abs().max().item() > 0 for k, v in plain.items() if 'encoder.layer' in k)
    if packed:
        for fill in ('ones', 'unit'):
            beyond = res[fill]['layers'][:, ~valid]
            assert beyond.numel() > 0 and bool((beyond == 0.0).all()), fill
    # the size contract: the workspace ends where the plan uniter_model_ws_bytes carved ends (its WS_SLACK bytes on top cut off), the
    # pass fitted in, the bands are whole
    B, L = valid.shape
    need = _lib.lib().uniter_model_ws_bytes(enc._handle, B, kw['input_ids'].shape[1] if kw['input_ids'] is not None else 0,
                                            kw['img_feat'].shape[1] if kw['img_feat'] is not None else 0, L, 1)
    for fill, p in ps.items():
        assert [r.nbytes for r in _ws_sites(p)] == [need - WS_SLACK]
        assert {'model.py:forward', 'trainer.py:forward'} <= p.functions(), p.report()


# ---- B: the default mode and bf16_hybrid (float atomics) ---------------------------------------------------------------------
@pytest.mark.parametrize('packed', [False, True], ids=['padded', 'packed'])
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3', 'bf16', 'bf16_hybrid'])
@pytest.mark.parametrize('name', list(MODELS))
def test_default_pass_agrees_under_every_fill(models, name, precision, packed):
    """forward outputs the same bits where runs under the same fill are; gradients within the bar (_assert_agree)"""
    m = models[name]
    _setup(m, precision, packed, False)
    kw, labels, valid = _batch(name, seed=3)
    kw2, labels2, valid2 = _batch(name, seed=9)
    res, _ = _under_fills(lambda: _fwd_bwd(m, kw, labels, valid), lambda: _fwd_bwd(m, kw2, labels2, valid2, seed=(23, 5)), again=3)
    _assert_agree(res, precision)


# ---- C: the inference plan --------------------------------------------------------------------------------------------------
def _infer(m, kw):
    from meme_challenge_amd.model import pool_head
    enc = m.uniter_model
    with torch.no_grad():
        layers = enc(output_all_encoded_layers=True, **kw)
        logits = pool_head(layers[-1], enc.pooler, m.linear)
    torch.cuda.synchronize()
    return {'logits': logits.clone(), 'layers': torch.stack(layers).clone()}


@pytest.mark.parametrize('deterministic', [True, False], ids=['det', 'default'])
@pytest.mark.parametrize('packed', [False, True], ids=['padded', 'packed'])
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3', 'bf16', 'bf16_hybrid'])
@pytest.mark.parametrize('name', list(MODELS))
def test_inference_is_the_same_bits_under_every_fill(models, name, precision, packed, deterministic):
    """With `deterministic` on no product of the inference pass has float atomics (the region projection takes its bias-epilogue
    form): the same bits in every precision.  The default mode is run as well; there the native-fp32 region projection is a
    stream-K accumulation at the hidden-256 size (UNITER_IMG_SK), whose order varies from run to run: that one case is held to
    the rule of the default training pass (_assert_agree), every other to the same bits."""
    m = models[name]
    enc = _setup(m, precision, packed, deterministic, train=False)
    kw, _, valid = _batch(name, seed=3)
    kw2, _, _ = _batch(name, seed=9)
    atomics = not deterministic and precision == 'fp32' and name == 'mid'

    def fresh(k):
        enc._ws_cache.clear()            # the cached block is poisoned when it is allocated: a new one per fill
        return _infer(m, k)
    res, ps = _under_fills(lambda: fresh(kw), lambda: fresh(kw2), again=3 if atomics else 0)
    enc._ws_cache.clear()
    if atomics:
        _assert_agree(res, precision)
    else:
        _assert_same_bits(res)
        _assert_finite(res['ones'], 'ones')
    if packed:
        assert bool((res['ones']['layers'][:, ~valid] == 0.0).all())
    for p in ps.values():
        _ws_sites(p)


@pytest.mark.parametrize('packed', [False, True], ids=['padded', 'packed'])
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3', 'bf16', 'bf16_hybrid'])
def test_a_short_batch_behind_a_long_one_in_the_cached_block(models, precision, packed):
    """the inference workspace is cached (_ws_cache[0]): the short batch's plan lies in the bytes the long batch's pass left"""
    m = models['mid']
    enc = _setup(m, precision, packed, True, train=False)
    long_kw, _, _ = _batch('mid', seed=3, lens=([64] * 16, [32] * 16))
    tl, nbb = [16, 1, 9, 5], [8, 1, 3, 8]
    short_kw, _, valid = _batch('mid', seed=4, lens=(tl, nbb), shape=(4, 16, 8))
    enc._ws_cache.clear()
    with Poison('zeros') as p0:
        alone = _infer(m, short_kw)
    enc._ws_cache.clear()
    with Poison('ones') as p1:
        _infer(m, long_kw)
        block = enc._ws_cache[0]
        behind = _infer(m, short_kw)
        assert enc._ws_cache[0] is block and p1.count('model.py:_get_ws') == 1
    assert not p0.passed_through and not p1.passed_through
    enc._ws_cache.clear()
    assert not _differing(alone, behind)
    _assert_finite(behind, 'behind the long batch')
    if packed:
        assert bool((behind['layers'][:, ~valid] == 0.0).all())


# ---- D: optional outputs through the model ----------------------------------------------------------------------------------
D_CASES = [(n, pr, pk) for n in MODELS for pr in ('fp32', 'bf16') for pk in (False, True)]
D_IDS = ['%s-%s-%s' % (n, pr, 'packed' if pk else 'padded') for n, pr, pk in D_CASES]


def _attr_batch(name, seed):
    kw, labels, valid = _batch(name, seed=seed)
    return dict(kw, labels=labels), valid


def _optional(models, name, precision, packed, run, sites, train=False):
    m = models[name]
    enc = _setup(m, precision, packed, True, train=train)
    enc._ws_cache.clear()
    b, valid = _attr_batch(name, 3)
    b2, _ = _attr_batch(name, 9)

    def go(batch):
        enc._ws_cache.clear()
        out = run(m, batch)
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in out.items()}
    res, ps = _under_fills(lambda: go(b), lambda: go(b2))
    enc._ws_cache.clear()
    _assert_same_bits(res)               # (`deterministic` is on: no pass here, training or inference, has float atomics)
    _assert_finite(res['ones'], 'ones')
    for p in ps.values():
        _ws_sites(p)
        assert set(sites) <= p.functions(), (sites, p.report())
    return res, valid


@pytest.mark.parametrize('name,precision,packed', D_CASES, ids=D_IDS)
def test_input_gradients_with_a_text_delta(models, name, precision, packed):
    H = MODELS[name][0]['hidden_size']

    def run(m, b):
        kw = {k: v for k, v in b.items() if k != 'labels'}
        g = torch.Generator().manual_seed(5)
        delta = (torch.randn(tuple(kw['input_ids'].shape) + (H,), generator=g) * 0.01).cuda().requires_grad_(True)
        feat, pos7 = kw['img_feat'].clone().requires_grad_(True), kw['img_pos_feat'].clone().requires_grad_(True)
        kw.update(img_feat=feat, img_pos_feat=pos7)
        valid = kw['attention_mask'].bool()
        out = _fwd_bwd(m, kw, b['labels'], valid, txt_embed_delta=delta)
        return dict(out, d_delta=delta.grad, d_feat=feat.grad, d_pos7=pos7.grad)
    res, _ = _optional(models, name, precision, packed, run, ['model.py:_get_ws', 'model.py:<listcomp>'], train=True)
    assert all(res['zeros'][k].abs().max().item() > 0 for k in ('d_delta', 'd_feat', 'd_pos7'))


@pytest.mark.parametrize('heads', ['all', 'mean'])
@pytest.mark.parametrize('name,precision,packed', D_CASES, ids=D_IDS)
def test_attention_probabilities(models, name, precision, packed, heads):
    from meme_challenge_amd.attribution import attention_maps

    def run(m, b):
        r = attention_maps(m, b, heads)
        return dict(probs=r.probs, logits=r.logits)
    res, valid = _optional(models, name, precision, packed, run, ['model.py:forward'])
    probs = res['ones']['probs']
    assert probs.dim() == (5 if heads == 'all' else 4) and probs.abs().max().item() > 0


@pytest.mark.parametrize('heads', ['all', 'relu_mean'])
@pytest.mark.parametrize('name,precision,packed', D_CASES, ids=D_IDS)
def test_gradient_weighted_attention_and_head_sums(models, name, precision, packed, heads):
    from meme_challenge_amd.attribution import attention_gradients

    def run(m, b):
        r = attention_gradients(m, b, None, heads)
        return dict(maps=r.maps, head_grads=r.head_grads, logits=r.logits)
    res, _ = _optional(models, name, precision, packed, run, ['model.py:forward'])
    assert res['ones']['maps'].abs().max().item() > 0 and res['ones']['head_grads'].abs().max().item() > 0


@pytest.mark.parametrize('name,precision,packed', D_CASES, ids=D_IDS)
def test_rollout_and_relevance(models, name, precision, packed):
    from meme_challenge_amd.attribution import attention_relevance, attention_rollout

    def run(m, b):
        ro, re = attention_rollout(m, b), attention_relevance(m, b)
        return dict(rollout=ro.joint, ro_tok=ro.cls_token, ro_reg=ro.cls_region, relevance=re.joint, re_tok=re.cls_token,
                    re_reg=re.cls_region)
    _optional(models, name, precision, packed, run, ['attribution.py:attention_rollout', 'attribution.py:attention_relevance'])


# ---- E: whole steps ---------------------------------------------------------------------------------------------------------
ROTATION = ('ones', 'unit', 'replay')


def _trajectory(run, other, iters):
    """run(before) under 'zeros', then under a fill that rotates from iteration to iteration (a one-iteration trajectory: once per
    fill); before(i) is called ahead of iteration i.  'replay' takes the bytes that other(before), the same trajectory over OTHER
    batches through the same plans, left behind.  -> the runs' results, the Poisons"""
    with Poison('zeros', capture=True) as cap:
        other(lambda i: None)
    with Poison('zeros') as z:
        outs, ps = [run(lambda i: None)], [z]
    for rot in ([ROTATION] if iters > 1 else [(f,) for f in ROTATION]):
        with Poison(rot[0], replay=cap.captured) as p:
            def before(i, p=p, rot=rot):
                p.fill = rot[i % len(rot)]
            outs.append(run(before))
        ps.append(p)
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        bad = [k for k in o if not torch.equal(o[k], outs[0][k])]
        assert not bad, bad
    for k, v in outs[0].items():
        assert v.numel() > 0 and bool(torch.isfinite(v).all()), k
    for p in ps:
        assert not p.passed_through, p.passed_through
    return outs, ps


def _mid_model(precision):
    m = build_meme_uniter(MID, MID_IMG_DIM, precision)
    m.uniter_model.deterministic = True
    return m


def _train(precision, batches, **adv):
    from meme_challenge_amd import trainer as T

    def run(before):
        m = _mid_model(precision)
        config = trainer_config('adam', **adv)
        assert config['max_grad_norm'] > 0
        opt = T.get_optimizer(m, config)
        assert isinstance(opt, T.FusedAdam)
        step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
        losses = []
        for it, b in enumerate(batches):
            before(it)
            losses.append(step.train_iter(b, iters=it).clone())
        opt.join()
        torch.cuda.synchronize()
        assert m.uniter_model.bit_reproducible
        st = m.param_store()
        return dict(flat_params=st.flat_params.detach().clone(), exp_avg=opt.exp_avg.detach().clone(),
                    exp_avg_sq=opt.exp_avg_sq.detach().clone(), losses=torch.stack(losses))
    return run


def _step_batch(seed, B, T, R):
    from meme_challenge_amd.utils import make_synthetic_batch
    return make_synthetic_batch(B, T, R, seed=seed, vocab=MID['vocab_size'], img_dim=MID_IMG_DIM, device='cuda')


@pytest.mark.parametrize('precision', ['fp32', 'fp32x3', 'bf16'])
def test_four_training_steps_under_rotating_fills(precision):
    """batches of other lengths from step to step: outside the harness the workspace would be the largest seen so far and its tail stale"""
    shapes = [(16, 64, 32), (16, 40, 20), (8, 64, 32), (16, 24, 32)]
    batches, others = ([_step_batch(seed + i, *shape) for i, shape in enumerate(shapes)] for seed in (3, 13))
    outs, ps = _trajectory(_train(precision, batches), _train(precision, others), len(batches))
    assert outs[0]['exp_avg'].abs().max().item() > 0 and outs[0]['exp_avg_sq'].abs().max().item() > 0
    for p in ps:
        ws = _ws_sites(p)
        assert len(ws) == len(batches) and len({r.nbytes for r in ws}) == len(batches)      # exact sizes: one per plan
        assert {'trainer.py:__init__', 'trainer.py:forward', 'model.py:forward'} <= p.functions(), p.report()


@pytest.mark.parametrize('algo', ['freelb', 'villa'])
@pytest.mark.parametrize('precision', ['fp32x3', 'bf16'])
def test_an_adversarial_step_under_every_fill(precision, algo):
    adv = dict(adv_steps=2, adv_lr=0.05, adv_max_norm=0.5, adv_init_mag=0.3, adv_algo=algo)
    if algo == 'villa':
        adv.update(adv_kl_weight=1.0, adv_norm_type='linf', adv_modality='each')
    outs, ps = _trajectory(_train(precision, [_step_batch(3, 16, 64, 32)], **adv), _train(precision, [_step_batch(13, 16, 64, 32)], **adv), 1)
    for p in ps:
        _ws_sites(p)
        assert {'trainer.py:adv_delta_step', 'trainer.py:forward', 'model.py:<listcomp>'} <= p.functions(), p.report()


def test_one_pretraining_step_per_task_under_rotating_fills(dds):
    """the multitask loop of tests/test_device_pretrain_gpu.py, one step each of MLM, MRFR and ITM; 'replay' from the same loop over
    the batches another loader seed draws"""
    from meme_challenge_amd.trainer import FusedAdam
    tasks = ('mlm', 'mrfr', 'itm')

    def trajectory(seed):
        def run(before):
            m = pretrain_model(train=True)
            m.uniter.deterministic = True
            opt = FusedAdam(m, lr=1e-3, weight_decay=1e-3)
            losses = []
            for i, task in enumerate(tasks):
                before(i)
                (_, batch), = take(pretrain_loader(dds, seed=seed, tasks=((task, 1),)), 1)
                loss = m(batch, task).mean()
                loss.backward()
                opt.step(grad_scale=1.0, max_grad_norm=5)
                losses.append(loss.detach().clone())
            opt.join()
            torch.cuda.synchronize()
            return dict(flat_params=opt.store.flat_params.detach().clone(), exp_avg=opt.exp_avg.detach().clone(),
                        exp_avg_sq=opt.exp_avg_sq.detach().clone(), losses=torch.stack(losses))
        return run
    outs, ps = _trajectory(trajectory(3), trajectory(4), len(tasks))
    for p in ps:
        _ws_sites(p)
        # 16 of pretrain.py's 22 torch.empty lines: the other six belong to the MRC task, which the loader does not draw
        lines = {s for s in p.sites if s.startswith('pretrain.py:')}
        assert len(lines) >= 16 and any(s.startswith('data.py:') for s in p.sites), p.report()


def test_optimal_transport_forward_and_backward_under_every_fill():
    import ot_ref as R
    from meme_challenge_amd.ot import optimal_transport_dist

    def case(d, flip=False):
        def run(before):
            before(0)
            # (flip: other inputs of the same shapes and padding, for the pass 'replay' takes its bytes from)
            x, y = ((-t.flip(0) if flip else t).cuda().requires_grad_(True) for t in (d['x'], d['y']))
            dist = optimal_transport_dist(x, y, d['x_pad'].cuda(), d['y_pad'].cuda(), d['beta'], d['iteration'])
            dist.backward(d['g'].cuda())
            torch.cuda.synchronize()
            return dict(dist=dist.detach().clone(), dx=x.grad.clone(), dy=y.grad.clone())
        return run
    for case_id in ('pad_one_each', 'tiny_rows_D257'):
        d = R.make(R.BY_ID[case_id])
        outs, ps = _trajectory(case(d), case(d, flip=True), 1)
        for p in ps:
            assert {'ot.py:forward', 'ot.py:backward'} <= p.functions() and p.count('ot.py:forward') == 2, p.report()


# ---- F: the size contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('train', [True, False], ids=['train', 'inference'])
def test_a_workspace_smaller_than_the_plan_is_refused(models, monkeypatch, train):
    from meme_challenge_amd import _lib
    m = models['tiny']
    enc = _setup(m, 'fp32', False, True, train=train)
    enc._ws_cache.clear()
    kw, labels, valid = _batch('tiny')
    real = _lib.lib().uniter_model_ws_bytes
    monkeypatch.setattr(_lib.lib(), 'uniter_model_ws_bytes', lambda *a: real(*a) // 2)
    with Poison('ones') as p:
        with pytest.raises(_lib.UniterHipError, match='workspace too small'):
            _fwd_bwd(m, kw, labels, valid) if train else _infer(m, kw)
    monkeypatch.undo()
    enc._ws_cache.clear()
    assert p.count('model.py:_get_ws') == 1 and not p.broken and not p.passed_through
    _assert_finite(_fwd_bwd(m, kw, labels, valid) if train else _infer(m, kw), 'the pass after the refusal')
