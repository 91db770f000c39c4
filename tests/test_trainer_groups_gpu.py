"""GPU: per-group learning rates (get_optimizer(.., group_param_func=..)) and a frozen layer prefix (UniterModel.freeze_prefix) through
the trainer, on the tiny model of the goldens.

The head-learning-rate steps are compared with a torch optimizer built from the same groups by the method of
tests/test_trainer_kinds_gpu.py: right before every step the parameters, gradients and state of the model under training go into a
twin, both step, and |fused - torch| <= 2 E_p with the fused result within E_p of float64 -- E_p evaluated PER GROUP with that
group's hyper-parameters (tests/optim_ref.py, tests/optim_kinds_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_kinds_ref as K
import optim_ref as R
from common import TINY, TINY_IMG_DIM
from test_trainer_kinds_gpu import Twin, _batches, _config, _model

pytestmark = pytest.mark.gpu

ALL_OPTS = ('adam', 'adamw', 'adamax', 'sgd')


def _is_head(name):
    return name.startswith('linear.') or name.startswith('uniter_model.pooler.')


def head_times_ten(named):
    """the reference's recipe (text_based/train_pure_text.py:53-58): the head first, with its own learning rate"""
    return [{'params': [(n, p) for n, p in named if _is_head(n)], 'lr': 1e-2},
            {'params': [(n, p) for n, p in named if not _is_head(n)], 'lr': 1e-3}]


def _torch_twin(model, config):
    """TorchOptimizerStep over torch's own optimizer of config['optimizer'], built from the same groups"""
    from meme_challenge_amd import trainer as T
    name = config['optimizer']
    if name in ('adamax', 'sgd'):
        return T.get_optimizer(model, config, group_param_func=head_times_ten, fused=False)
    st = model.param_store()
    groups = [dict(g, params=[p for _, p in g['params']])
              for g in T.group_layout(list(st.params.items()), config['weight_decay'], head_times_ten)]
    cls = torch.optim.Adam if name == 'adam' else torch.optim.AdamW
    return T.TorchOptimizerStep(model, cls(groups, lr=config['lr'], betas=(config['beta1'], config['beta2'])))


class GroupTwin(Twin):
    """Twin whose float64 reference and bound are evaluated group by group, and whose torch state is seeded for Adam / AdamW too"""

    def step(self, grad_scale=1.0, max_grad_norm=0.0, zero_grads=True, **kw):
        a, b = self.a, self.b
        a.join()
        sa, sb = a.store, b.store
        pre = dict(p=sa.flat_params.clone(), g=sa.flat_grads.clone(), m=a.exp_avg.clone(),
                   v=None if a.exp_avg_sq is None else a.exp_avg_sq.clone())
        flags = a._chunk_flags(False, True).cpu().numpy().copy()
        sb.flat_params.copy_(pre['p'])
        sb.flat_grads.copy_(pre['g'])
        sb.touched.clear()
        sb.touched.update(sa.touched)
        assert len(a.param_groups) == len(b.param_groups) == 4
        name_a, name_b = ({id(p): n for n, p in s.params.items()} for s in (sa, sb))
        for ga, gb in zip(a.param_groups, b.param_groups):          # the same tensors group by group (their order inside a group is free)
            assert {name_a[id(p)] for p in ga['params']} == {name_b[id(p)] for p in gb['params']}
            gb['lr'] = ga['lr']
        for n, p in sb.params.items():
            o, k = sb.offsets[n], p.numel()
            m = a.exp_avg[o:o + k].view(p.shape).clone()
            if a.KIND == K.KIND_SGD:
                b.inner.state[p] = {'momentum_buffer': m}
            else:
                second = a.exp_avg_sq[o:o + k].view(p.shape).clone()
                b.inner.state[p] = {'step': torch.tensor(float(a.step_count)), 'exp_avg': m,
                                    ('exp_inf' if a.KIND == K.KIND_ADAMAX else 'exp_avg_sq'): second}
        n = sa.numel
        np_ = {k: (None if t is None else t.cpu().numpy()) for k, t in pre.items()}
        sumsq = R.ref_sumsq(np_['g'], flags) if max_grad_norm else None
        ref_p, E_p = np.zeros(n), np.zeros(n)
        group_el = R.expand_flags(flags >> 3, n)
        for k, g in enumerate(a.param_groups):
            b1, b2, eps = a._rule_args(g)
            h = R.Hyper(lr=g['lr'], b1=b1, b2=b2, eps=eps, wd=g['weight_decay'], step=a.step_count + 1, adamw=int(a.adamw),
                        gscale=grad_scale, max_norm=max_grad_norm or 0.0)
            with np.errstate(all='ignore'):
                if a.KIND is None:
                    ref = R.ref_step(np_['p'], np_['g'], np_['m'], np_['v'], flags & 7, h, sumsq)
                else:
                    ref = K.ref_step_kind(a.KIND, np_['p'], np_['g'], np_['m'], np_['v'], flags & 7, h, sumsq)
            own = group_el == k
            ref_p[own], E_p[own] = ref['p'][own], ref['E_p'][own]
        self._orig(grad_scale=grad_scale, max_grad_norm=max_grad_norm, zero_grads=zero_grads, **kw)
        b.step(grad_scale=grad_scale, max_grad_norm=max_grad_norm, zero_grads=zero_grads)
        a.join()
        torch.cuda.synchronize()
        upd = (R.expand_flags(flags, n) & 3) != 0
        h0 = R.Hyper(gscale=grad_scale, max_norm=max_grad_norm or 0.0)
        self.records.append(dict(pa=sa.flat_params.cpu().numpy().copy(), pb=sb.flat_params.cpu().numpy().copy(), pre=np_['p'], upd=upd,
                                 ref=dict(p=ref_p, E_p=E_p), group=group_el, coef=R.clip_coef(sumsq, h0) / h0.gscale))


def _within(rec, factor):
    upd, ref = rec['upd'], rec['ref']
    for side in ('pa', 'pb'):
        assert np.array_equal(rec[side][~upd], rec['pre'][~upd]), side
    assert np.isfinite(rec['pa']).all()
    assert R.worst_ratio(rec['pa'][upd], ref['p'][upd], ref['E_p'][upd]) <= 1.0
    return R.worst_ratio(rec['pa'][upd].astype(np.float64), rec['pb'][upd].astype(np.float64), factor * ref['E_p'][upd])


@pytest.mark.parametrize('optname', ALL_OPTS)
def test_head_learning_rate_matches_torch_within_twice_the_bound(optname):
    from meme_challenge_amd import trainer as T
    config = _config(optname, max_grad_norm=0.05, gradient_accumulation=2)
    ma, mb = _model('fp32'), _model('fp32')
    a, b = T.get_optimizer(ma, config, group_param_func=head_times_ten), _torch_twin(mb, config)
    assert [g['lr'] for g in a.param_groups] == [1e-2, 1e-2, 1e-3, 1e-3]
    assert [g['weight_decay'] for g in a.param_groups] == [1e-2, 0.0, 1e-2, 0.0]
    assert [len(g['params']) for g in a.param_groups][:2] == [2, 2]            # pooler and classifier: a weight and a bias each
    step = T.TrainStep(ma, a, T.get_scheduler(a, config, steps_per_epoch=10), config)
    tw = GroupTwin(a, b)
    for g, lr in zip(a.param_groups, (1e-2, 1e-2, 1e-3, 1e-3)):              # (the warm-up's first lr is 0)
        g['lr'] = lr
    calls = _count(('uniter_optim_step_groups', 'uniter_adam_step_x3p', 'uniter_optim_step'))
    bs = _batches(2)
    try:
        for it in range(4):
            assert torch.isfinite(step.train_iter(bs[it % 2], iters=it))
    finally:
        calls.restore()
    assert len(tw.records) == 2
    assert calls.n['uniter_optim_step_groups'] >= 2 and calls.n['uniter_adam_step_x3p'] == 0 and calls.n['uniter_optim_step'] == 0
    worst = max(_within(r, 2.0) for r in tw.records)
    print('%s: worst |fused - torch| / (2 E_p): %.3f' % (optname, worst))
    assert worst <= 1.0
    assert all(r['coef'] < 0.9 for r in tw.records)                            # the clip was active
    r = tw.records[-1]
    moved = [np.abs(r['pa'] - r['pre'])[r['upd'] & (r['group'] == k)].max() for k in range(4)]
    assert min(moved) > 0
    if optname != 'sgd':            # (a step of the Adam family is about lr per element, whatever the gradient's size)
        assert moved[0] > 3 * moved[2]


class _count:
    """counts the calls of entry points on the library handle (and passes them on)"""

    def __init__(self, names):
        from meme_challenge_amd import _lib
        self.lib, self.n, self.orig = _lib.lib(), {k: 0 for k in names}, {}
        for name in names:
            self.orig[name] = fn = getattr(self.lib, name)
            setattr(self.lib, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def call(*args):
            self.n[name] += 1
            return fn(*args)
        return call

    def restore(self):
        for name, fn in self.orig.items():
            setattr(self.lib, name, fn)


def test_without_groups_and_frozen_parameters_the_step_is_todays_entry_points():
    from meme_challenge_amd import trainer as T
    for optname, entry in (('adam', 'uniter_adam_step_x3p'), ('sgd', 'uniter_optim_step')):
        config = _config(optname)
        m = _model('fp32')
        # a grouping that changes no hyper-parameter is no reason for the grouped launch either
        for f in (None, lambda named: [{'params': named[:7]}, {'params': named[7:]}]):
            opt = T.get_optimizer(m, config, group_param_func=f)
            opt.overlap_encoder = m.uniter_model
            step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
            calls = _count(('uniter_optim_step_groups', 'uniter_adam_step_x3p', 'uniter_optim_step', 'uniter_model_backward_end',
                            'uniter_model_backward_embed'))
            try:
                for it in range(2):
                    step.train_iter(_batches(1)[0], iters=it)
                opt.join()
                torch.cuda.synchronize()
            finally:
                calls.restore()
            other = 'uniter_optim_step' if entry == 'uniter_adam_step_x3p' else 'uniter_adam_step_x3p'
            assert calls.n[entry] >= 2 * (1 + TINY['num_hidden_layers']) and calls.n[other] == 0      # per step: the embeddings' and every layer's block at least
            assert calls.n['uniter_optim_step_groups'] == 0
            assert calls.n['uniter_model_backward_end'] == 0 and calls.n['uniter_model_backward_embed'] == 2
            assert len(opt.param_groups) == (2 if f is None else 4)
            m.uniter_model._grad_hook = None


@pytest.mark.parametrize('precision', ['bf16', 'fp32x3'])
def test_grouped_steps_leave_the_weight_mirror_current(precision):
    """the mirror the grouped launches wrote against a fresh refresh from the parameters, bit for bit: one launch over the buffer
    (every chunk) and the overlapped blocks (the encoder layers' range, the only one the overlapped step mirrors)"""
    from meme_challenge_amd import trainer as T, _lib
    config = _config('adamw')
    for overlap in (False, True):
        m = _model(precision)
        opt = T.get_optimizer(m, config, group_param_func=head_times_ten)
        if overlap:
            opt.overlap_encoder = m.uniter_model
        step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
        bs = _batches(2)
        for it in range(3):
            step.train_iter(bs[it % 2], iters=it)
        opt.join()
        torch.cuda.synchronize()
        st = m.param_store()
        assert st.mirror_dirty is False and not opt._uniform()
        wrote = st.mirror.clone()
        st.refresh_mirror(0, st.numel, _lib.cur_stream())
        torch.cuda.synchronize()
        lo, hi = (0, st.numel)
        if overlap:
            blocks = opt._overlap_plan(m.uniter_model)[1][1:]
            lo, hi = min(b[0] for b in blocks), max(b[1] for b in blocks)
        for piece in range(st.mirror_pieces):
            a, b = (t[piece * st.numel + lo:piece * st.numel + hi].view(torch.int16) for t in (wrote, st.mirror))
            assert torch.equal(a, b), (overlap, piece)


@pytest.mark.parametrize('optname', ALL_OPTS)
def test_scheduler_keeps_the_ratio_of_the_two_learning_rates(optname):
    from meme_challenge_amd import trainer as T
    config = _config(optname)
    m = _model('fp32')
    opt = T.get_optimizer(m, config, group_param_func=head_times_ten)
    sched = T.get_scheduler(opt, config, steps_per_epoch=10)
    assert [g['lr'] for g in opt.param_groups] == [0.0] * 4                     # warm-up starts at 0
    for k in range(3):
        sched.step()
        lrs = [g['lr'] for g in opt.param_groups]
        assert lrs[0] == lrs[1] and lrs[2] == lrs[3] and lrs[2] > 0
        assert lrs[0] == pytest.approx(10 * lrs[2], rel=1e-12)
    assert lrs[2] == pytest.approx(1e-3 * T.cosine_warmup_lambda(2, 20)(3))


def _frozen_names(model):
    return {n for n, p in model.named_parameters() if not p.requires_grad}


def _freeze_by_hand(model):
    for n, p in model.named_parameters():
        if 'embeddings.' in n or '.encoder.layer.0.' in n:
            p.requires_grad = False


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp32x3'])
def test_frozen_prefix_is_never_read_or_written(precision):
    from meme_challenge_amd import trainer as T, _lib
    from common import model_kwargs
    config = _config('adam', lr=1e-2)
    m = _model(precision)
    assert m.uniter_model.freeze_prefix(1) == 1
    frozen = _frozen_names(m)
    assert frozen and all('embeddings.' in n or '.encoder.layer.0.' in n for n in frozen)
    assert not any(n in frozen for n, _ in m.named_parameters() if '.encoder.layer.1.' in n or _is_head(n))
    opt = T.get_optimizer(m, config)
    opt.overlap_encoder = m.uniter_model
    step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
    assert m.uniter_model._grad_hook is None                # the clip norm is the flag-aware pass
    st = m.param_store()
    p0 = st.flat_params.clone()
    mirror0 = st.mirror.clone() if precision != 'fp32' else None
    bs = _batches(2)
    for it in range(3):
        assert torch.isfinite(step.train_iter(bs[it % 2], iters=it))
    opt.join()
    torch.cuda.synchronize()
    frozen_el = torch.zeros(st.numel, dtype=torch.bool, device='cuda')
    for n in st.names:
        if n in frozen:
            frozen_el[st.offsets[n]:st.offsets[n] + (st.params[n].numel() + 63) // 64 * 64] = True
    assert 0 < int(frozen_el.sum()) < st.numel
    assert torch.equal(st.flat_params[frozen_el].view(torch.int32), p0[frozen_el].view(torch.int32))
    assert not opt.exp_avg[frozen_el].any() and not opt.exp_avg_sq[frozen_el].any()
    moved = (st.flat_params != p0) & ~frozen_el
    assert float(moved.sum()) > 0.5 * float((~frozen_el).sum()) and opt.exp_avg[~frozen_el].any()
    if mirror0 is not None:
        assert st.mirror_dirty is False
        for piece in range(st.mirror_pieces):
            a, b = (t[piece * st.numel:(piece + 1) * st.numel].view(torch.int16)[frozen_el] for t in (st.mirror, mirror0))
            assert torch.equal(a, b), piece
    # the norm the step clips by: the trainable gradients alone
    loss = T.bce_with_logits_loss(m(**model_kwargs(bs[0])).squeeze(1), bs[0]['labels'], 1.8)
    loss.backward()
    norm = float(opt.grad_norm().item())
    torch.cuda.synchronize()
    want = sum(float(p.grad.double().pow(2).sum().item()) for n, p in m.named_parameters() if n not in frozen) ** 0.5
    assert want > 0 and abs(norm - want) <= 2 * R.SUMSQ_REL * want


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'fp32x3'])
def test_short_backward_trains_what_the_full_backward_trains(precision):
    """freeze_prefix(1) (the backward pass ends above layer 0) against the same tensors frozen by hand (the full backward runs and the
    optimizer ignores what it does not own): the trainable parameters after three steps.  No test of this suite holds the model's
    gradients bit-reproducible from run to run, so the bar is that of test_overlapped_optimizer_step_matches_single_launch for the
    same quantity: the larger of 4 x what two identical runs differ by and 5e-6, with the weight gradients on the main stream and
    dropout off as there."""
    from meme_challenge_amd import trainer as T
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    cfg = UniterConfig.from_dict(dict(TINY, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
    config = _config('adam', max_grad_norm=1.0)
    bs = _batches(2)
    finals, ends = {}, {}
    for how in ('hand', 'prefix', 'hand again'):
        torch.manual_seed(0)
        m = MemeUniter(UniterModel(cfg, img_dim=TINY_IMG_DIM), cfg.hidden_size, 1).cuda().train()
        m.uniter_model.precision = precision
        m.uniter_model.use_side_stream = False
        if how == 'prefix':
            assert m.uniter_model.freeze_prefix(1) == 1
        else:
            _freeze_by_hand(m)
            assert m.uniter_model.backward_floor() == 0
        opt = T.get_optimizer(m, config)
        step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
        calls = _count(('uniter_model_backward_end', 'uniter_model_backward_embed'))
        try:
            for it in range(4):
                step.train_iter(bs[it % 2], iters=it)
            opt.join()
            torch.cuda.synchronize()
        finally:
            calls.restore()
        ends[how] = (calls.n['uniter_model_backward_end'], calls.n['uniter_model_backward_embed'])
        st = m.param_store()
        finals[how] = torch.cat([st.flat_params[st.offsets[n]:st.offsets[n] + p.numel()] for n, p in st.params.items() if p.requires_grad]).clone()
        frozen = _frozen_names(m)
    assert ends == {'hand': (0, 4), 'prefix': (4, 0), 'hand again': (0, 4)}
    assert len(frozen) > 10 and finals['hand'].numel() == finals['prefix'].numel() > 1000
    noise = (finals['hand again'] - finals['hand']).abs().max().item()
    diff = (finals['prefix'] - finals['hand']).abs().max().item()
    print('%s: |prefix - by hand| %.3g, two identical runs %.3g' % (precision, diff, noise))
    assert diff <= max(4 * noise, 5e-6), (diff, noise)


def test_frozen_prefix_shortens_the_launch_schedule():
    """every profiled kind's launches of one step (uniter_prof_enable(-1)): fewer with the floor than without"""
    from meme_challenge_amd import trainer as T, _lib
    config = _config('adam')
    counts = {}
    for floor in (0, 1):
        m = _model('fp32')
        if floor:
            m.uniter_model.freeze_prefix(floor)
        opt = T.get_optimizer(m, config)
        step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
        b = _batches(1)[0]
        step.train_iter(b, iters=0)
        lib, h = _lib.lib(), m.uniter_model._handle
        _lib.check(lib.uniter_prof_enable(h, -1), 'uniter_prof_enable')
        step.train_iter(b, iters=1)
        torch.cuda.synchronize()
        n, ms = (C.c_int * 16)(), (C.c_double * 16)()
        _lib.check(lib.uniter_prof_collect_kinds(h, n, ms, 16), 'uniter_prof_collect_kinds')
        _lib.check(lib.uniter_prof_enable(h, 0), 'uniter_prof_enable')
        counts[floor] = list(n)
    print('profiled launches per kind, full %s, floor 1 %s' % (counts[0], counts[1]))
    assert sum(counts[1]) < sum(counts[0])
    assert counts[1][7] < counts[0][7] and counts[1][6] < counts[0][6]        # UNITER_K_GEMM_WGRAD, UNITER_K_GEMM_DGRAD
    assert counts[1][1:6] == counts[0][1:6]                                    # the forward pass is the one it was


def test_frozen_word_table_stays_fixed_beside_the_row_split_switch(monkeypatch):
    """UNITER_ADAM_WORD_ROWS=1: the ahead-of-time launch over the rows no token looks up (FusedAdam.early_word_update) knows no frozen
    chunk, so a frozen table is never split by rows -- the table and its moments after three steps, bit for bit"""
    from meme_challenge_amd import trainer as T
    monkeypatch.setenv('UNITER_ADAM_WORD_ROWS', '1')
    config = _config('adam', lr=1e-2)
    m = _model('fp32')
    assert m.uniter_model.freeze_prefix(1) == 1
    opt = T.get_optimizer(m, config)
    opt.overlap_encoder = m.uniter_model
    assert opt.split_word_rows and opt._word_table() is None
    step = T.TrainStep(m, opt, T.get_scheduler(opt, config, steps_per_epoch=10), config)
    st = m.param_store()
    name, lo, hi = opt._find_word_table()
    assert name in _frozen_names(m) and hi > lo
    p0 = st.flat_params.clone()
    calls = _count(('uniter_adam_step_rows',))
    bs = _batches(2)
    try:
        for it in range(3):
            assert torch.isfinite(step.train_iter(bs[it % 2], iters=it))
        opt.join()
        torch.cuda.synchronize()
    finally:
        calls.restore()
    assert calls.n['uniter_adam_step_rows'] == 0 and opt._rowmask is None and opt._early is None
    assert torch.equal(st.flat_params[lo:hi].view(torch.int32), p0[lo:hi].view(torch.int32))
    assert not opt.exp_avg[lo:hi].any() and not opt.exp_avg_sq[lo:hi].any()
    assert bool((st.flat_params != p0).any())
