"""GPU: MemeUniter.head_rows_only -- the last encoder layer computes, behind its attention kernel, only the rows the pooled head reads
(uniter_model_set_head_rows, fp32x3 on padded batches).

Short path against full path: the same model built twice from one seed, train mode with dropout on and the same dropout seed;
logits, every parameter gradient and the trainer's clip norm of `head_rows_only = True` against `False`, at the tolerances
tests/test_model_gpu.py::test_tiny_loss_and_all_grads_match_reference_golden holds against the reference (2e-6 + 2e-4 max|ref| per
tensor with the full path as ref, logits within 1e-5, the clip norm to 1e-6 relative), and the rows of the encoder's output the head
does not read are exact zeros.  Fallbacks: where the library ignores the request the results are bit-equal with it on and off."""
import pytest
import torch

from common import TINY, TINY_IMG_DIM, MID, MID_IMG_DIM, build_meme_uniter, maxdiff, trainer_config

pytestmark = pytest.mark.gpu


def _batch(cfg, img_dim, B, T, R, seed=2, **kw):
    from meme_challenge_amd.utils import make_synthetic_batch
    return make_synthetic_batch(B, T, R, seed=seed, vocab=cfg['vocab_size'], img_dim=img_dim, device='cuda', **kw)


def _run(cfg, img_dim, batch, on, precision='fp32x3', packed=False, train=True, deterministic=False):
    """one trainer step at lr = 0 (its clip norm; the parameters stay), then a forward + backward pass by hand: the hooked encoder
    output, logits, gradients, clip norm"""
    from meme_challenge_amd.trainer import FusedAdam, TrainStep, bce_with_logits_loss, get_scheduler
    m = build_meme_uniter(cfg, img_dim, precision, seed=0, train=train)
    m.head_rows_only = on
    m.uniter_model.pack_padded = packed
    m.uniter_model.deterministic = deterministic
    config = trainer_config('adam', lr=0.0, weight_decay=0.0, max_grad_norm=0.05)
    opt = FusedAdam(m, lr=0.0, weight_decay=0.0)
    step = TrainStep(m, opt, get_scheduler(opt, config, steps_per_epoch=10), config)
    step.train_iter(batch, iters=0)
    norm = opt._sumsq.clone().sqrt()
    seen = []
    hook = m.uniter_model.register_forward_hook(lambda mod, a, out: seen.append(out.detach().clone()))
    logits = m(**TrainStep.forward_kwargs(batch))
    hook.remove()
    bce_with_logits_loss(logits.squeeze(1), batch['labels'], 1.8).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    return dict(hidden=seen[0], logits=logits.detach().clone(), grads=grads, norm=float(norm.item()))


CASES = {
    'B1': (TINY, TINY_IMG_DIM, dict(B=1, T=12, R=5)),
    'B3': (TINY, TINY_IMG_DIM, dict(B=3, T=12, R=5)),
    'B4': (TINY, TINY_IMG_DIM, dict(B=4, T=12, R=5)),
    'B33': (TINY, TINY_IMG_DIM, dict(B=33, T=12, R=5)),      # two k-tiles in the compact weight gradients
    'ragged': (TINY, TINY_IMG_DIM, dict(B=4, T=12, R=5, txt_lens=[12, 3, 7, 1], num_bbs=[5, 5, 2, 1])),
    'mid': (MID, MID_IMG_DIM, dict(B=16, T=24, R=8)),        # the sizes at which the split-K forms are picked
}


@pytest.mark.parametrize('case', list(CASES))
def test_short_path_against_full_path(case):
    cfg, img_dim, shape = CASES[case]
    batch = _batch(cfg, img_dim, **shape)
    full = _run(cfg, img_dim, batch, False)
    short = _run(cfg, img_dim, batch, True)
    # the full path really computed every row, the short path left exact zeros in the rows the head does not read
    assert full['hidden'][:, 1:].abs().max().item() > 0
    assert short['hidden'][:, 1:].abs().max().item() == 0
    assert maxdiff(short['hidden'][:, 0], full['hidden'][:, 0]) <= 1e-5
    d = maxdiff(short['logits'], full['logits'])
    print('%s: |dlogits| = %.3e, clip norm %.9e vs %.9e' % (case, d, short['norm'], full['norm']))
    assert d <= 1e-5
    assert set(short['grads']) == set(full['grads'])
    for n, ref in full['grads'].items():
        tol = 2e-6 + 2e-4 * ref.abs().max().item()
        e = maxdiff(short['grads'][n], ref)
        assert e <= tol, (n, e, tol)
    assert full['norm'] > 0 and abs(short['norm'] - full['norm']) <= 1e-6 * full['norm']


def test_eval_mode_logits_agree():
    """a forward pass that saves nothing (no_grad) takes the short path as well"""
    from meme_challenge_amd.trainer import TrainStep
    batch = _batch(TINY, TINY_IMG_DIM, B=4, T=12, R=5)
    out = {}
    for on in (False, True):
        m = build_meme_uniter(TINY, TINY_IMG_DIM, 'fp32x3', seed=0, train=False)
        m.head_rows_only = on
        seen = []
        hook = m.uniter_model.register_forward_hook(lambda mod, a, o: seen.append(o.detach().clone()))
        with torch.no_grad():
            out[on] = m(**TrainStep.forward_kwargs(batch)).clone()
        hook.remove()
        assert (seen[0][:, 1:].abs().max().item() == 0) == on
    assert maxdiff(out[True], out[False]) <= 1e-5


@pytest.mark.parametrize('what', ['packed', 'fp32'])
def test_fallbacks_are_bit_equal(what):
    """a packed batch and the native fp32 mode ignore the request: every row computed, the same bits as without it (order-fixed sums
    on both sides, so that two runs of one path agree bit for bit in the first place)"""
    batch = _batch(TINY, TINY_IMG_DIM, B=4, T=12, R=5, txt_lens=[12, 3, 7, 1], num_bbs=[5, 5, 2, 1])
    kw = dict(precision='fp32' if what == 'fp32' else 'fp32x3', packed=what == 'packed', deterministic=True)
    off = _run(TINY, TINY_IMG_DIM, batch, False, **kw)
    on = _run(TINY, TINY_IMG_DIM, batch, True, **kw)
    assert on['hidden'][:, 1:].abs().max().item() > 0
    assert torch.equal(on['hidden'], off['hidden']) and torch.equal(on['logits'], off['logits'])
    assert set(on['grads']) == set(off['grads'])
    for n in off['grads']:
        assert torch.equal(on['grads'][n], off['grads'][n]), n
    assert on['norm'] == off['norm']


def test_all_layers_through_the_encoder_ignores_the_request():
    """output_all_encoded_layers=True through uniter_model directly, with the request set by hand as MemeUniter sets it"""
    from meme_challenge_amd.trainer import TrainStep
    batch = _batch(TINY, TINY_IMG_DIM, B=4, T=12, R=5)
    kw = dict(TrainStep.forward_kwargs(batch), output_all_encoded_layers=True)
    res = {}
    for on in (False, True):
        m = build_meme_uniter(TINY, TINY_IMG_DIM, 'fp32x3', seed=0, train=True)
        m.uniter_model.deterministic = True
        m.param_store()
        if on:
            m.uniter_model._head_rows_next = True
        layers = m.uniter_model(**kw)
        assert '_head_rows_next' not in m.uniter_model.__dict__
        sum(h.square().sum() for h in layers).backward()
        torch.cuda.synchronize()
        res[on] = ([h.detach().clone() for h in layers],
                   {n: p.grad.detach().clone() for n, p in m.uniter_model.named_parameters() if p.grad is not None})
    assert res[True][0][-1][:, 1:].abs().max().item() > 0
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b)
    assert set(res[True][1]) == set(res[False][1])
    for n in res[False][1]:
        assert torch.equal(res[True][1][n], res[False][1][n]), n


def test_pretraining_model_never_asks():
    """its heads read every row: nothing sets the request, and the encoder's output has every row"""
    from common import PRETRAIN_CFG, PRETRAIN_IMG_DIM, pretrain_model
    from meme_challenge_amd.utils import make_synthetic_pretrain_batch
    m = pretrain_model(train=True)
    enc = m.uniter
    enc.precision = 'fp32x3'
    b = make_synthetic_pretrain_batch('itm', 4, 12, 5, seed=3, vocab=PRETRAIN_CFG['vocab_size'], img_dim=PRETRAIN_IMG_DIM, device='cuda')
    seen = []
    hook = enc.register_forward_hook(lambda mod, a, o: seen.append(o.detach().clone()))
    loss = m(b, 'itm', compute_loss=True)
    hook.remove()
    loss.mean().backward()
    torch.cuda.synchronize()
    assert '_head_rows_next' not in enc.__dict__
    assert seen[0][:, 1:].abs().max().item() > 0
