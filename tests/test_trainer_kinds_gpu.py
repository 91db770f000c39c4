"""GPU: `--optimizer adamax | sgd` as fused steps (trainer.FusedAdamax / FusedSGD over uniter_optim_step) on the tiny model of the
goldens: what get_optimizer returns, the fused step against torch.optim's own update (trainer.TorchOptimizerStep) from the same
parameters, gradients and state, the weight mirror the update writes, the overlapped launch, the clip norm taken during the
backward pass, and a few training iterations in every precision.

Two optimizers are compared FROM THE SAME INPUTS: the model under training (A) runs forward and backward; right before its step the
parameters, gradients and state are copied into a twin (B), both step, and the results are compared -- so neither the atomics'
order of the embedding gradients nor an earlier step's difference enters a comparison.  Where both sides are fp32 evaluations of one
contract they may differ by 2 E_p per element, E_p the bound of tests/optim_kinds_ref.py on |fp32 - float64|."""
import numpy as np
import pytest
import torch

import optim_kinds_ref as K
import optim_ref as R
from common import TINY, TINY_IMG_DIM, trainer_config as _config

pytestmark = pytest.mark.gpu

OPTS = ('adamax', 'sgd')


def _model(precision, train=True, seed=0):
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    cfg = UniterConfig.from_dict(TINY)
    torch.manual_seed(seed)
    m = MemeUniter(UniterModel(cfg, img_dim=TINY_IMG_DIM), cfg.hidden_size, 1).cuda()
    m = m.train() if train else m.eval()
    m.uniter_model.precision = precision
    m.uniter_model.set_dropout_seed(5, 0)
    return m


def _batches(k=2):
    from meme_challenge_amd.utils import make_synthetic_batch
    return [make_synthetic_batch(4, 16, 6, seed=3 + i, vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM, device='cuda') for i in range(k)]


def _hyper(opt, step, grad_scale, max_norm):
    g0 = opt.param_groups[0]
    if opt.KIND == K.KIND_SGD:
        return R.Hyper(lr=g0['lr'], b1=g0['momentum'], b2=0.0, eps=0.0, wd=g0['weight_decay'], step=step, gscale=grad_scale,
                       max_norm=max_norm)
    return R.Hyper(lr=g0['lr'], b1=g0['betas'][0], b2=g0['betas'][1], eps=g0['eps'], wd=g0['weight_decay'], step=step,
                   gscale=grad_scale, max_norm=max_norm)


def _seed_torch_state(twin, fused):
    """the torch optimizer's per-parameter state := the fused optimizer's (views of the twin's own copies)"""
    st, inner = twin.store, twin.inner
    for n, p in st.params.items():
        o, k = st.offsets[n], p.numel()
        m = fused.exp_avg[o:o + k].view(p.shape).clone()
        if fused.KIND == K.KIND_SGD:
            inner.state[p] = {'momentum_buffer': m}
        else:
            inner.state[p] = {'step': torch.tensor(float(fused.step_count)), 'exp_avg': m,
                              'exp_inf': fused.exp_avg_sq[o:o + k].view(p.shape).clone()}


class Twin:
    """Wraps optimizer A's step(): right before it the parameters, gradients and state go into B (a fused optimizer or a
    TorchOptimizerStep on a model of the same shape), both step, and (A's p, B's p, E_p) is recorded per step.  Installed AFTER the
    learning-rate scheduler, which wraps the optimizer's step method itself when it is built."""

    def __init__(self, a, b):
        self.a, self.b, self.records = a, b, []
        self._orig = a.step
        a.step = lambda **kw: self.step(**kw)

    def step(self, grad_scale=1.0, max_grad_norm=0.0, zero_grads=True, **kw):
        from meme_challenge_amd.trainer import FusedAdam
        a, b = self.a, self.b
        a.join()
        sa, sb = a.store, b.store
        assert sa.numel == sb.numel
        pre = dict(p=sa.flat_params.clone(), g=sa.flat_grads.clone(), m=a.exp_avg.clone(),
                   v=None if a.exp_avg_sq is None else a.exp_avg_sq.clone())
        flags = a._chunk_flags(False).cpu().numpy().copy()
        sb.flat_params.copy_(pre['p'])
        sb.flat_grads.copy_(pre['g'])
        sb.touched.clear()
        sb.touched.update(sa.touched)
        if isinstance(b, FusedAdam):
            b.exp_avg.copy_(pre['m'])
            if pre['v'] is not None:
                b.exp_avg_sq.copy_(pre['v'])
            b.step_count = a.step_count
            for ga, gb in zip(a.param_groups, b.param_groups):
                gb['lr'] = ga['lr']
        else:
            _seed_torch_state(b, a)
            for ga, gb in zip(a.param_groups, b.param_groups):
                gb['lr'] = ga['lr']
        h = _hyper(a, a.step_count + 1, grad_scale, max_grad_norm or 0.0)
        g_np = pre['g'].cpu().numpy()
        sumsq = R.ref_sumsq(g_np, flags) if h.max_norm > 0 else None
        with np.errstate(all='ignore'):
            ref = K.ref_step_kind(a.KIND, pre['p'].cpu().numpy(), g_np, pre['m'].cpu().numpy(),
                                  None if pre['v'] is None else pre['v'].cpu().numpy(), flags, h, sumsq)
        self._orig(grad_scale=grad_scale, max_grad_norm=max_grad_norm, zero_grads=zero_grads, **kw)
        b.step(grad_scale=grad_scale, max_grad_norm=max_grad_norm, zero_grads=zero_grads)
        a.join()
        b.join()
        torch.cuda.synchronize()
        upd = (R.expand_flags(flags, sa.numel) & 3) != 0
        self.records.append(dict(pa=sa.flat_params.cpu().numpy().copy(), pb=sb.flat_params.cpu().numpy().copy(), ref=ref, upd=upd,
                                 pre=pre['p'].cpu().numpy(), ma=a.exp_avg.cpu().numpy().copy(),
                                 mb=b.exp_avg.cpu().numpy().copy() if isinstance(b, FusedAdam) else None,
                                 va=None if a.exp_avg_sq is None else a.exp_avg_sq.cpu().numpy().copy(),
                                 vb=b.exp_avg_sq.cpu().numpy().copy() if isinstance(b, FusedAdam) and b.exp_avg_sq is not None else None,
                                 sumsq_a=float(a._sumsq.item()), sumsq_ref=sumsq, coef=R.clip_coef(sumsq, h) / h.gscale))


def _within(rec, factor):
    """|A - B| / (factor E_p) on the updated elements, A within E_p of float64; the others untouched by both"""
    upd, ref = rec['upd'], rec['ref']
    for side in ('pa', 'pb'):
        assert np.array_equal(rec[side][~upd], rec['pre'][~upd]), side
    assert R.worst_ratio(rec['pa'][upd], ref['p'][upd], ref['E_p'][upd]) <= 1.0
    assert np.isfinite(rec['pa']).all()
    return R.worst_ratio(rec['pa'][upd].astype(np.float64), rec['pb'][upd].astype(np.float64), factor * ref['E_p'][upd])


# ---------------------------------------------------------------------------------------------------------------------------
def test_get_optimizer_returns_the_fused_classes():
    from meme_challenge_amd import trainer as T
    m = _model('fp32')
    ax = T.get_optimizer(m, _config('adamax'))
    assert type(ax) is T.FusedAdamax and isinstance(ax, T.FusedAdam) and isinstance(ax, torch.optim.Optimizer)
    g0, g1 = ax.param_groups
    # torch.optim.Adamax's defaults, not the config's betas (utils/optim_utils.py:36-37)
    assert tuple(g0['betas']) == (0.9, 0.999) and g0['eps'] == 1e-8 and g0['lr'] == 1e-3
    assert g0['weight_decay'] == 1e-2 and g1['weight_decay'] == 0.0
    assert ax.exp_avg_sq is not None and ax.exp_avg_sq.shape == ax.exp_avg.shape
    sg = T.get_optimizer(m, _config('sgd'))
    assert type(sg) is T.FusedSGD and isinstance(sg, T.FusedAdam)
    g0, g1 = sg.param_groups
    assert g0['momentum'] == 0.8 and g0['lr'] == 1e-3 and g0['weight_decay'] == 1e-2 and g1['weight_decay'] == 0.0
    assert sg.exp_avg_sq is None                                 # no second state: 8 bytes per parameter less
    names = dict(m.named_parameters())
    decay = {id(p) for p in g0['params']}
    assert all((id(p) in decay) != T.no_decay(n) for n, p in names.items())
    for opt in (ax, sg):
        assert opt.split_word_rows is False
        with pytest.raises(T.UniterHipError):
            opt.early_word_update()
        sched = T.get_scheduler(opt, _config('sgd'), steps_per_epoch=10)      # the scheduler drives the lr the kernel reads
        assert opt.param_groups[0]['lr'] == 0.0
        sched.step()
        assert opt.param_groups[0]['lr'] == pytest.approx(0.5e-3) and opt.param_groups[1]['lr'] == opt.param_groups[0]['lr']
    for name, inner in (('adamax', torch.optim.Adamax), ('sgd', torch.optim.SGD)):
        tw = T.get_optimizer(m, _config(name), fused=False)
        assert type(tw) is T.TorchOptimizerStep and type(tw.inner) is inner
    assert type(T.get_optimizer(m, _config('adam'))) is T.FusedAdam
    with pytest.raises(T.UniterHipError):
        T.get_optimizer(m, _config('sgd'), group_param_func=lambda *a: None)


@pytest.mark.parametrize('clip', [0.05, 0.0], ids=['clip', 'noclip'])
@pytest.mark.parametrize('optname', OPTS)
def test_fused_step_matches_torchs_update_within_twice_the_bound(optname, clip):
    """four iterations (the first two with gradient accumulation 2: one step from one micro-batch still divided by 2, then one
    from two); the torch twin's state is re-seeded from the fused one before every step"""
    from meme_challenge_amd import trainer as T
    config = _config(optname, max_grad_norm=clip, gradient_accumulation=2)
    ma, mb = _model('fp32'), _model('fp32')
    a, b = T.get_optimizer(ma, config), T.get_optimizer(mb, config, fused=False)
    step = T.TrainStep(ma, a, T.get_scheduler(a, config, steps_per_epoch=10), config)
    tw = Twin(a, b)
    bs = _batches(2)
    a.param_groups[0]['lr'] = a.param_groups[1]['lr'] = 1e-3          # (the warm-up's first lr is 0)
    for it in range(5):
        loss = step.train_iter(bs[it % 2], iters=it)
        assert torch.isfinite(loss)
    assert len(tw.records) == 3
    worst = max(_within(r, 2.0) for r in tw.records)
    print('%s: worst |fused - torch| / (2 E_p) over %d steps: %.3f' % (optname, len(tw.records), worst))
    assert worst <= 1.0
    if clip:
        assert all(r['coef'] < 0.9 for r in tw.records), [r['coef'] for r in tw.records]       # the clip was active
    moved = max(np.abs(r['pa'] - r['pre']).max() for r in tw.records[1:])
    assert moved > 1e-5                                               # and the steps did move the parameters


@pytest.mark.parametrize('precision', ['bf16', 'fp32x3'])
@pytest.mark.parametrize('optname', OPTS)
def test_fused_step_leaves_the_weight_mirror_current(optname, precision):
    """after a fused step the mirror is NOT dirty, the next forward rebuilds nothing, and its logits are bit-identical to those of
    a forward whose mirror was rebuilt from the same parameters; torch's update (fused=False) does leave it dirty"""
    from meme_challenge_amd import trainer as T
    from common import model_kwargs
    config = _config(optname)
    m = _model(precision)
    opt = T.get_optimizer(m, config)
    step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
    bs = _batches(2)
    st = m.param_store()
    for it in range(3):
        step.train_iter(bs[it % 2], iters=it)
    opt.join()
    torch.cuda.synchronize()
    assert st.mirror_dirty is False
    calls = []
    orig = st.refresh_mirror
    st.refresh_mirror = lambda *a, **k: (calls.append(a), orig(*a, **k))[1]
    m.eval()
    with torch.no_grad():
        kept = m(**model_kwargs(bs[0])).clone()
        assert calls == [] and st.mirror_dirty is False          # the forward found the mirror the update wrote
        st.mirror_dirty = True
        rebuilt = m(**model_kwargs(bs[0])).clone()
        assert len(calls) == 1
    torch.cuda.synchronize()
    assert torch.isfinite(kept).all() and torch.equal(kept, rebuilt)
    st.refresh_mirror = orig
    # the comparison partner
    m2 = _model(precision)
    tw = T.get_optimizer(m2, config, fused=False)
    step2 = T.TrainStep(m2, tw, T.get_scheduler(tw, config, steps_per_epoch=10), config)
    step2.train_iter(bs[0], iters=0)
    assert tw.store.mirror_dirty is True          # (read from the store itself: model.param_store() would rebuild the mirror on the way)


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp32x3'])
@pytest.mark.parametrize('optname', OPTS)
def test_overlapped_step_is_the_single_launch_bit_for_bit(optname, precision):
    """overlap_encoder: the update block by block on the side stream beside the next forward (in fp32x3 the layers' blocks walk the
    paired mirror's order) against ONE launch over the flat buffers from the same inputs: parameters and state bit-identical"""
    from meme_challenge_amd import trainer as T
    config = _config(optname)
    ma, mb = _model(precision), _model(precision)
    a, b = T.get_optimizer(ma, config), T.get_optimizer(mb, config)
    a.overlap_encoder = ma.uniter_model
    step = T.TrainStep(ma, a, T.get_scheduler(a, config, steps_per_epoch=10), config)
    tw = Twin(a, b)
    assert ma.uniter_model._grad_hook is not None and a.lazy_zero_encoder is ma.uniter_model
    # (both sides take the clip norm the same way, one pass over the buffer: the backward pass's partial sums add up in another order,
    # and a last-bit difference of the coefficient is not what this test is about)
    ma.uniter_model._grad_hook = None
    bs = _batches(2)
    for it in range(4):
        step.train_iter(bs[it % 2], iters=it)
    assert len(tw.records) == 4
    for r in tw.records:
        assert np.array_equal(r['pa'].view(np.uint32), r['pb'].view(np.uint32))
        assert np.array_equal(r['ma'].view(np.uint32), r['mb'].view(np.uint32))
        assert (r['va'] is None) == (optname == 'sgd')
        if r['va'] is not None:
            assert np.array_equal(r['va'].view(np.uint32), r['vb'].view(np.uint32))
    assert np.abs(tw.records[-1]['pa'] - tw.records[-1]['pre']).max() > 1e-6


@pytest.mark.parametrize('precision', ['fp32', 'fp32x3'])
@pytest.mark.parametrize('optname', OPTS)
def test_train_step_arms_the_norm_hooks_and_the_clip_matches_the_full_pass(optname, precision):
    """TrainStep with max_grad_norm > 0 attaches the clip norm to the backward pass for the new optimizers too; the step that
    joins the backward pass's partial sums against a twin that reduces the same gradient buffer in one pass"""
    from meme_challenge_amd import trainer as T
    config = _config(optname, max_grad_norm=0.05)
    ma, mb = _model(precision), _model(precision)
    a, b = T.get_optimizer(ma, config), T.get_optimizer(mb, config)
    step = T.TrainStep(ma, a, T.get_scheduler(a, config, steps_per_epoch=10), config)
    tw = Twin(a, b)
    assert ma.uniter_model._grad_hook is not None and a._np_buf is not None
    assert mb.uniter_model._grad_hook is None and b._np_buf is None
    armed = []
    orig = tw._orig
    tw._orig = lambda **kw: (armed.append(a._np_blocks), orig(**kw))[1]
    bs = _batches(2)
    for it in range(4):
        step.train_iter(bs[it % 2], iters=it)
    assert len(armed) == 4 and all(n > 0 for n in armed), armed         # every step joined the backward pass's partial sums
    for r in tw.records:
        assert r['coef'] < 0.9                                          # the clip was active
        assert abs(r['sumsq_a'] - r['sumsq_ref']) <= 1e-5 * r['sumsq_ref']
        assert _within(r, 2.0) <= 1.0


@pytest.mark.parametrize('precision', ['fp32', 'fp32x3', 'bf16'])
@pytest.mark.parametrize('optname', OPTS)
def test_three_training_iterations_stay_finite(optname, precision):
    """the way train_template drives it: overlap on, norm hooks, lazy zeroing, the scheduler"""
    from meme_challenge_amd import trainer as T
    config = _config(optname, lr=1e-2)
    m = _model(precision)
    opt = T.get_optimizer(m, config)
    opt.overlap_encoder = m.uniter_model
    step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
    st = m.param_store()
    p0 = st.flat_params.clone()
    bs = _batches(2)
    losses = [step.train_iter(bs[it % 2], iters=it) for it in range(4)]
    opt.join()
    torch.cuda.synchronize()
    assert all(torch.isfinite(x) for x in losses)
    assert torch.isfinite(st.flat_params).all() and torch.isfinite(opt.exp_avg).all()
    assert opt.step_count == 4 and (st.flat_params - p0).abs().max().item() > 1e-5
    if precision != 'fp32':
        assert st.mirror_dirty is False
