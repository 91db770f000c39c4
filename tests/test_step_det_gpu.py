"""UniterModel.deterministic covers the whole training step: forward, backward, clip and fused optimizer step give the same bits run
after run, in fp32, fp32x3 and bf16, padded and packed.

The model is the smallest at which the heuristics pick the float-atomic forms the switch has to turn off: hidden 256, 4 heads,
intermediate 1024, 2 layers, img_dim 2048; B = 16, 64 tokens, 32 regions, so L = 96 and B * R = 512 -- the region projection's weight
gradient is 128 tiles x 16 k-units, which the fp32 / fp32x3 launcher runs stream-K on 256 workgroups by default.  Dropout on with a
fixed seed, side and auxiliary streams on."""
import pytest
import torch

from common import MID as CFG, MID_IMG_DIM as IMG_DIM, TINY, TINY_IMG_DIM, model_kwargs

pytestmark = pytest.mark.gpu

B, T, R = 16, 64, 32
PRECISIONS = ['fp32', 'fp32x3', 'bf16']
DET_ALL = 15


def _model(precision, cfg=CFG, img_dim=IMG_DIM, seed=0):
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    c = UniterConfig.from_dict(cfg)
    torch.manual_seed(seed)
    m = MemeUniter(UniterModel(c, img_dim=img_dim), c.hidden_size, 1).cuda().train()
    m.uniter_model.precision = precision
    m.uniter_model.set_dropout_seed(5, 0)
    return m


def _batch(seed=3, **lens):
    from meme_challenge_amd.utils import make_synthetic_batch
    return make_synthetic_batch(B, T, R, seed=seed, vocab=CFG['vocab_size'], img_dim=IMG_DIM, device='cuda', **lens)


def _fwd_bwd(m, b, **kw):
    from meme_challenge_amd.trainer import bce_with_logits_loss
    m.uniter_model.set_dropout_seed(11, 0)
    m.zero_grad(set_to_none=False)
    m.param_store().zero_grads()
    logits = m(**kw, **model_kwargs(b))
    bce_with_logits_loss(logits.squeeze(1), b['labels'], 1.8).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    return logits.detach().clone(), grads


def _ws_bytes(m, L):
    from meme_challenge_amd import _lib
    return _lib.lib().uniter_model_ws_bytes(m.uniter_model._handle, B, T, R, L, 1)


@pytest.fixture(scope='module')
def runs():
    """per precision: two default runs, three deterministic ones of the same model and batch, and what the plan reported; computed once"""
    out = {}
    for precision in PRECISIONS:
        m = _model(precision)
        enc = m.uniter_model
        assert enc.deterministic is False and enc.use_side_stream
        b = _batch()
        L = b['attn_mask'].shape[1]
        assert L == T + R
        default = [_fwd_bwd(m, b) for _ in range(2)]
        info = dict(ws_before=_ws_bytes(m, L), cov_before=enc.deterministic_coverage, repro_before=enc.bit_reproducible)
        enc.deterministic = True
        det = [_fwd_bwd(m, b) for _ in range(3)]
        info.update(cov_on=enc.deterministic_coverage, repro_on=enc.bit_reproducible, ws_on=_ws_bytes(m, L))
        enc.deterministic = False
        info.update(cov_off_at_once=enc.deterministic_coverage)
        _fwd_bwd(m, b)
        info.update(cov_off=enc.deterministic_coverage, repro_off=enc.bit_reproducible, ws_off=_ws_bytes(m, L))
        out[precision] = (default, det, info)
    return out


@pytest.mark.parametrize('precision', PRECISIONS)
def test_every_gradient_is_the_same_bits_in_three_runs(runs, precision):
    _, det, _ = runs[precision]
    (l0, g0), (l1, g1), (l2, g2) = det
    assert len(g0) >= 15 + 16 * CFG['num_hidden_layers'] and 'uniter_model.img_embeddings.img_linear.weight' in g0
    assert all(g.abs().max().item() > 0 for n, g in g0.items() if 'mask_embedding' not in n)
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    differ = [n for n in g0 if not (torch.equal(g0[n], g1[n]) and torch.equal(g0[n], g2[n]))]
    assert not differ, differ


@pytest.mark.parametrize('precision', PRECISIONS)
def test_coverage_is_full_when_on_and_nothing_when_off(runs, precision):
    _, _, info = runs[precision]
    assert info['cov_before'] == 0 and info['repro_before'] is False
    assert info['cov_on'] == DET_ALL and info['repro_on'] is True
    assert info['cov_off_at_once'] == 0 and info['cov_off'] == 0 and info['repro_off'] is False
    # with the switch off the plan asks for what it asked for before the switch was ever set
    assert info['ws_off'] == info['ws_before'] and info['ws_on'] >= info['ws_before']


@pytest.mark.parametrize('precision', PRECISIONS)
def test_deterministic_gradients_agree_with_the_default_path(runs, precision):
    """the bar of tests/test_model_det_gpu.py, unchanged: fp32 round-off of the reordered sums (2e-5, bf16 3e-3, of the largest entry)
    plus four times what two identical runs of the default path differ by (its float atomics)"""
    default, det, _ = runs[precision]
    (la, ga), (lb, gb) = default
    ld, gd = det[0]
    assert set(ga) == set(gd)
    for n in ga:
        noise = (gb[n] - ga[n]).abs().max().item()
        tol = (3e-3 if precision == 'bf16' else 2e-5) * ga[n].abs().max().item() + 4 * noise
        err = (gd[n] - ga[n]).abs().max().item()
        assert err <= tol, (n, err, tol)
    # the logits: the native-fp32 region projection leaves its stream-K form (another order of the same sum); elsewhere the same code
    if precision == 'fp32':
        assert (la - ld).abs().max().item() <= 2e-5 * max(1.0, la.abs().max().item()) + 4 * (la - lb).abs().max().item()
    else:
        assert torch.equal(la, ld) and torch.equal(la, lb)


@pytest.mark.parametrize('precision', ['fp32x3', 'bf16'])
def test_five_training_steps_leave_the_same_parameters_and_moments_twice(precision):
    """Five TrainStep iterations with the fused Adam step, run twice from the same seed: the WHOLE flat parameter buffer and both
    moment buffers are the same bits"""
    from meme_challenge_amd import trainer as T
    from test_trainer_kinds_gpu import _config
    ends = []
    for _ in range(2):
        m = _model(precision)
        m.uniter_model.deterministic = True
        config = _config('adam')
        opt = T.get_optimizer(m, config)
        assert isinstance(opt, T.FusedAdam)
        step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
        bs = [_batch(3), _batch(4)]
        for it in range(5):
            assert torch.isfinite(step.train_iter(bs[it % 2], iters=it))
        opt.join()
        torch.cuda.synchronize()
        assert m.uniter_model.bit_reproducible
        st = m.param_store()
        ends.append((st.flat_params.detach().clone(), opt.exp_avg.detach().clone(), opt.exp_avg_sq.detach().clone()))
    for a, b, name in zip(ends[0], ends[1], ('flat_params', 'exp_avg', 'exp_avg_sq')):
        assert a.numel() > 0 and torch.isfinite(a).all()
        assert torch.equal(a, b), (name, (a != b).sum().item())
    assert ends[0][1].abs().max().item() > 0 and ends[0][2].abs().max().item() > 0


def test_packed_ragged_batch_is_the_same_bits_in_three_runs():
    """token packing on (the valid positions only), driven as tests/test_packed_gpu.py drives it: host lengths beside the batch"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(77))
    tl = [int(x) for x in rng.integers(5, T + 1, size=B)]
    nbb = [int(x) for x in rng.integers(3, R + 1, size=B)]
    tl[0], nbb[0] = T, R                                       # one full-length sample: L stays T + R
    b = _batch(5, txt_lens=tl, num_bbs=nbb)
    m = _model('fp32x3')
    m.uniter_model.pack_padded = True
    m.uniter_model.deterministic = True
    lens = [a + c for a, c in zip(tl, nbb)]
    (l0, g0), (l1, g1), (l2, g2) = [_fwd_bwd(m, b, seq_lens=lens) for _ in range(3)]
    assert m.uniter_model.deterministic_coverage == DET_ALL
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    assert 'uniter_model.img_embeddings.img_linear.weight' in g0 and len(g0) >= 15 + 16 * CFG['num_hidden_layers']
    differ = [n for n in g0 if not (torch.equal(g0[n], g1[n]) and torch.equal(g0[n], g2[n]))]
    assert not differ, differ


@pytest.mark.parametrize('precision', PRECISIONS)
def test_tiny_configuration_reports_full_coverage(precision):
    from meme_challenge_amd.utils import make_synthetic_batch
    from meme_challenge_amd.trainer import bce_with_logits_loss
    m = _model(precision, cfg=TINY, img_dim=TINY_IMG_DIM)
    enc = m.uniter_model
    b = make_synthetic_batch(4, 16, 6, seed=3, vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM, device='cuda')
    assert enc.deterministic_coverage == 0 and not enc.bit_reproducible and enc.deterministic_missing() == [
        'embedding gradients', 'attention bias partials', 'column sums', 'dense products']
    enc.deterministic = True
    logits = m(**model_kwargs(b))
    bce_with_logits_loss(logits.squeeze(1), b['labels'], 1.8).backward()
    torch.cuda.synchronize()
    assert enc.deterministic_coverage == DET_ALL and enc.bit_reproducible and enc.deterministic_missing() == []
