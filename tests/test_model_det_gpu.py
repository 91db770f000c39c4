"""UniterModel.deterministic: the embedding gradients of a whole forward + backward are the same bits run after run, agree with
the default (atomic) path, cost the default path nothing, and stay the same bits over optimizer steps.

Tiny config, B = 4, 16 tokens, 6 regions, dropout on with a fixed seed, side and auxiliary streams on.  Precision fp32x3: the
gradient that reaches the embeddings comes down the input-gradient chain, which has no float atomics in that mode.  bf16 is in
the parametrisation because its gradient into the embeddings was measured identical run to run on this configuration before the
case was added (DESIGN.md section 4 records it)."""
import pytest
import torch

from common import TINY, TINY_IMG_DIM, model_kwargs
from test_trainer_groups_gpu import _count
from test_trainer_kinds_gpu import _batches, _config, _model

pytestmark = pytest.mark.gpu

EMB = ('uniter_model.embeddings.', 'uniter_model.img_embeddings.')
PRECISIONS = ['fp32x3', 'bf16']


def _fwd_bwd(m, b):
    from meme_challenge_amd.trainer import bce_with_logits_loss
    m.uniter_model.set_dropout_seed(11, 0)
    m.zero_grad(set_to_none=False)
    m.param_store().zero_grads()
    logits = m(**model_kwargs(b))
    bce_with_logits_loss(logits.squeeze(1), b['labels'], 1.8).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if n.startswith(EMB) and p.grad is not None}
    return logits.detach().clone(), grads


@pytest.fixture(scope='module')
def runs():
    """per precision: three deterministic runs and two default ones of the same model and batch, computed once"""
    out = {}
    for precision in PRECISIONS:
        m = _model(precision)
        assert m.uniter_model.deterministic is False and m.uniter_model.use_side_stream
        b = _batches(1)[0]
        default = [_fwd_bwd(m, b) for _ in range(2)]
        m.uniter_model.deterministic = True
        det = [_fwd_bwd(m, b) for _ in range(3)]
        out[precision] = (default, det)
    return out


@pytest.mark.parametrize('precision', PRECISIONS)
def test_embedding_gradients_are_the_same_bits_in_three_runs(runs, precision):
    _, det = runs[precision]
    (l0, g0), (l1, g1), (l2, g2) = det
    assert len(g0) >= 15 and all(g.abs().max().item() > 0 for n, g in g0.items() if 'mask_embedding' not in n)
    assert torch.equal(l0, l1) and torch.equal(l0, l2)
    for n in g0:
        assert torch.equal(g0[n], g1[n]) and torch.equal(g0[n], g2[n]), n


@pytest.mark.parametrize('precision', PRECISIONS)
def test_deterministic_gradients_agree_with_the_default_path(runs, precision):
    """the bar of test_cu_reserve_for_a_gradient_exchange_changes_no_result: fp32 round-off of the reordered sums plus four times
    what two identical runs of the default path differ by (its float atomics)"""
    default, det = runs[precision]
    (la, ga), (lb, gb) = default
    ld, gd = det[0]
    assert torch.equal(la, ld) and torch.equal(la, lb)              # the forward pass is the same code
    for n in ga:
        noise = (gb[n] - ga[n]).abs().max().item()
        tol = (3e-3 if precision == 'bf16' else 2e-5) * ga[n].abs().max().item() + 4 * noise
        err = (gd[n] - ga[n]).abs().max().item()
        assert err <= tol, (n, err, tol)


def test_default_is_off_and_makes_no_new_call():
    """With the switch off the library is driven exactly as before: the Python layer never calls uniter_model_set_deterministic or a
    _det entry point (counted on the library handle, as tests/test_trainer_groups_gpu.py counts the optimizer's), and the plan
    asks for the workspace it asked for before; with it on the plan adds the order-fixed passes' share.  (Which embedding kernels
    uniter_model_backward_embed launches is decided inside the library, out of this counter's sight: the reproducibility
    tests above are the evidence for the `on` side, the workspace size for the `off` side.)"""
    from meme_challenge_amd import _lib
    names = ('uniter_model_set_deterministic', 'uniter_txt_embed_bwd', 'uniter_img_embed_bwd', 'uniter_txt_embed_bwd_det',
             'uniter_img_embed_bwd_det', 'uniter_embed_bwd_det_ws_bytes', 'uniter_model_backward_embed')
    m = _model('fp32x3')
    b = _batches(1)[0]
    enc = m.uniter_model
    calls = _count(names)
    try:
        _fwd_bwd(m, b)
        off = dict(calls.n)
        ws_off = _lib.lib().uniter_model_ws_bytes(enc._handle, 4, 16, 6, b['attn_mask'].shape[1], 1)
        enc.deterministic = True
        _fwd_bwd(m, b)
        _fwd_bwd(m, b)
        on = dict(calls.n)
        ws_on = _lib.lib().uniter_model_ws_bytes(enc._handle, 4, 16, 6, b['attn_mask'].shape[1], 1)
        enc.deterministic = False
        _fwd_bwd(m, b)
        ws_back = _lib.lib().uniter_model_ws_bytes(enc._handle, 4, 16, 6, b['attn_mask'].shape[1], 1)
    finally:
        calls.restore()
    assert off == dict({k: 0 for k in names}, uniter_model_backward_embed=1)
    assert on['uniter_model_set_deterministic'] == 1 and on['uniter_model_backward_embed'] == 3      # applied once, not per step
    assert calls.n['uniter_model_set_deterministic'] == 2
    assert all(calls.n[k] == 0 for k in names[1:6])
    need = _lib.lib().uniter_embed_bwd_det_ws_bytes(4 * 16, 4 * 6, TINY['hidden_size'])
    assert ws_on > ws_off == ws_back and ws_on - ws_off <= 3 * need


def test_five_training_steps_leave_the_same_embedding_parameters_twice():
    """Five TrainStep iterations with the fused Adam step, run twice from the same seed: the embedding slices of the flat parameter
    buffer are the same bits.  (Not the whole buffer: the attention kernels' bias partials are not order-fixed.)"""
    from meme_challenge_amd import trainer as T
    ends = []
    for _ in range(2):
        m = _model('fp32x3')
        m.uniter_model.deterministic = True
        config = _config('adam')
        opt = T.get_optimizer(m, config)
        assert isinstance(opt, T.FusedAdam)
        step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
        bs = _batches(2)
        for it in range(5):
            assert torch.isfinite(step.train_iter(bs[it % 2], iters=it))
        opt.join()
        torch.cuda.synchronize()
        st = m.param_store()
        ends.append({n: p.detach().clone() for n, p in m.named_parameters() if n.startswith(EMB)})
        assert all(p.data_ptr() == st.flat_params.data_ptr() + 4 * st.offsets[n] for n, p in m.named_parameters() if n.startswith(EMB))
    assert len(ends[0]) >= 15
    for n in ends[0]:
        assert torch.equal(ends[0][n], ends[1][n]), n
