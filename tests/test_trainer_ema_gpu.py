"""GPU: the averaged weights (`ema_decay`) and the optimizer's state_dict through trainer.FusedAdam on the tiny model of the
goldens (tests/common.TINY: 2 layers, H = 128), both dropout probabilities 0, B = 3 with ragged lengths and 4 regions,
`deterministic = True`, precisions fp32x3 and bf16, the overlapped step on (the way train_template drives it).

The runs are shared (module-scoped fixture, computed once per precision): four TrainStep iterations without and with
ema_decay = 0.9, the parameters snapshotted after every step.

Bound of the average after several steps, from the parameter snapshots alone: the float64 recurrence a_t = a_{t-1} + w_t (p_t -
a_{t-1}), a_0 = p_0, with the per-step bound of tests/optim_ema_ref.py carried along -- an error e of a_{t-1} reaches a_t as
(1 - w_t) e, so E_t = (1 - w_t) E_{t-1} + C U (|a_{t-1}| + |w_t (p_t - a_{t-1})|).  The p_t are the kernel's own fp32 values."""
import numpy as np
import pytest
import torch

import optim_ema_ref as E
import optim_ref as R
from common import TINY, TINY_IMG_DIM, model_kwargs

pytestmark = pytest.mark.gpu

PRECISIONS = ['fp32x3', 'bf16']
CFG = dict(TINY, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
DECAY, STEPS = 0.9, 4


def _config(**kw):
    c = dict(optimizer='adamw', lr=1e-3, beta1=0.9, beta2=0.98, weight_decay=1e-2, gradient_accumulation=1, max_grad_norm=0.05,
             pos_wt=1.8, loss_func='bce_logits', scheduler='warmup_cosine', warmup_steps=2, max_epoch=2)
    c.update(kw)
    return c


def _model(precision, seed=0, train=True):
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    cfg = UniterConfig.from_dict(CFG)
    torch.manual_seed(seed)
    m = MemeUniter(UniterModel(cfg, img_dim=TINY_IMG_DIM), cfg.hidden_size, 1).cuda()
    m = m.train() if train else m.eval()
    m.uniter_model.precision = precision
    m.uniter_model.deterministic = True
    return m


def _batches():
    from meme_challenge_amd.utils import make_synthetic_batch
    return [make_synthetic_batch(3, 10, 4, seed=3 + i, vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM, device='cuda',
                                 txt_lens=[10, 7, 5], num_bbs=[4, 3, 2]) for i in range(2)]


def _setup(precision, config, seed=0):
    from meme_challenge_amd import trainer as T
    m = _model(precision, seed=seed)
    opt = T.get_optimizer(m, config)
    opt.overlap_encoder = m.uniter_model
    sched = T.get_scheduler(opt, config, steps_per_epoch=10)
    return m, opt, sched, T.TrainStep(m, opt, sched, config)


def _iterate(step, opt, first, count, snaps=None):
    bs = _batches()
    for it in range(first, first + count):
        assert torch.isfinite(step.train_iter(bs[it % 2], iters=it))
        if snaps is not None:
            opt.join()
            torch.cuda.synchronize()
            snaps.append(opt.store.flat_params.detach().clone())
    opt.join()
    torch.cuda.synchronize()


def _state(opt):
    return dict(p=opt.store.flat_params.detach().clone(), m=opt.exp_avg.detach().clone(), v=opt.exp_avg_sq.detach().clone(),
                avg=None if opt.avg is None else opt.avg.detach().clone(), avg_steps=opt.avg_steps, step=opt.step_count)


@pytest.fixture(scope='module')
def runs():
    out = {}
    for precision in PRECISIONS:
        plain = _setup(precision, _config())
        _iterate(plain[3], plain[1], 0, STEPS)
        ema = _setup(precision, _config(ema_decay=DECAY))
        snaps = [ema[1].store.flat_params.detach().clone()]
        _iterate(ema[3], ema[1], 0, STEPS, snaps)
        out[precision] = dict(plain=_state(plain[1]), ema=_state(ema[1]), snaps=snaps, objects=ema)
    return out


@pytest.mark.parametrize('precision', PRECISIONS)
def test_averaging_leaves_parameters_and_moments_bit_identical(runs, precision):
    a, b = runs[precision]['plain'], runs[precision]['ema']
    assert a['avg'] is None and b['avg'] is not None and b['avg_steps'] == b['step'] == a['step'] == STEPS
    for k in 'pmv':
        assert torch.isfinite(a[k]).all() and a[k].abs().max().item() > 0
        assert torch.equal(a[k], b[k]), (k, (a[k] != b[k]).sum().item())


@pytest.mark.parametrize('precision', PRECISIONS)
def test_average_is_within_the_bound_of_the_float64_recurrence(runs, precision):
    snaps = [s.cpu().numpy() for s in runs[precision]['snaps']]
    assert len(snaps) == STEPS + 1
    a, err = snaps[0].astype(np.float64), np.zeros(snaps[0].size)
    for t in range(STEPS):
        w = E.ref_weight(DECAY, t)
        inc = w * (snaps[t + 1].astype(np.float64) - a)
        err = (1.0 - w) * err + E.C * E.U * (np.abs(a) + np.abs(inc))
        a = a + inc
    got = runs[precision]['ema']['avg'].cpu().numpy()
    moved = snaps[-1] != snaps[0]
    assert moved.mean() > 0.5
    assert np.array_equal(got[~moved], snaps[0][~moved])             # never updated: the average is the parameter, bit for bit
    ratio = R.worst_ratio(got, a, err)
    print('%s: average after %d steps, worst error / bound %.3f' % (precision, STEPS, ratio))
    assert ratio <= 1.0, ratio
    # .. and it is neither end of the run
    assert not np.array_equal(got, snaps[-1]) and not np.array_equal(got, snaps[0])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_averaged_parameters_context(runs, precision):
    """inside: the model IS the averaged model (logits bit-identical to a second model loaded from a state_dict taken inside --
    the weight mirror, paired rows included, was rebuilt); after: the raw parameters and logits are back bit for bit"""
    from meme_challenge_amd import trainer as T
    m, opt = runs[precision]['objects'][:2]
    b = _batches()[0]
    m.eval()
    raw, avg = opt.store.flat_params.detach().clone(), opt.avg.detach().clone()
    assert not torch.equal(raw, avg)
    with torch.no_grad():
        before = m(**model_kwargs(b)).detach().clone()
        with opt.averaged_parameters():
            assert torch.equal(opt.store.flat_params, avg) and torch.equal(opt.avg, raw)
            inside = m(**model_kwargs(b)).detach().clone()
            sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
            with pytest.raises(T.UniterHipError):
                with opt.averaged_parameters():
                    pass
            with pytest.raises(T.UniterHipError):
                opt.step()
            p0 = opt.param_groups[0]['params'][0]       # (exchanged: state_dict() finds the average in the parameters' place)
            o = opt.store.offsets[next(n for n, q in opt.store.params.items() if q is p0)]
            assert torch.equal(opt.state_dict()['averaged'][0].reshape(-1), avg[o:o + p0.numel()])
        after = m(**model_kwargs(b)).detach().clone()
        twin = _model(precision, seed=5, train=False)
        twin.load_state_dict(sd)
        want = twin(**model_kwargs(b)).detach().clone()
    torch.cuda.synchronize()
    assert torch.equal(opt.store.flat_params, raw) and torch.equal(opt.avg, avg)
    assert torch.equal(after, before)
    assert torch.equal(inside, want)
    assert not torch.equal(inside, before)
    m.train()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_state_dict_resumes_the_run_bit_for_bit(runs, precision, tmp_path):
    """two steps, torch.save of state_dict(), fresh model and optimizer objects, load, two more steps = the uninterrupted four"""
    config = _config(ema_decay=DECAY)
    m, opt, sched, step = _setup(precision, config)
    _iterate(step, opt, 0, 2)
    sd = opt.state_dict()
    n_params = sum(len(g['params']) for g in opt.param_groups)
    assert sorted(sd['state']) == list(range(n_params)) and sd['averaged_steps'] == 2 and len(sd['averaged']) == n_params
    assert all(set(e) == {'step', 'exp_avg', 'exp_avg_sq'} and float(e['step']) == 2.0 for e in sd['state'].values())
    torch.save({'optimizer': sd, 'model': m.state_dict(), 'scheduler': sched.state_dict()}, tmp_path / 'run.pt')
    del m, opt, step
    saved = torch.load(tmp_path / 'run.pt', map_location='cuda', weights_only=False)
    m2 = _model(precision, seed=7)
    m2.load_state_dict(saved['model'])
    from meme_challenge_amd import trainer as T
    opt2 = T.get_optimizer(m2, config)
    opt2.overlap_encoder = m2.uniter_model
    sched2 = T.get_scheduler(opt2, config, steps_per_epoch=10)
    opt2.load_state_dict(saved['optimizer'])
    sched2.load_state_dict(saved['scheduler'])
    assert opt2.step_count == 2 and opt2.avg_steps == 2
    _iterate(T.TrainStep(m2, opt2, sched2, config), opt2, 2, 2)
    got, want = _state(opt2), runs[precision]['ema']
    for k in ('p', 'm', 'v', 'avg'):
        assert torch.equal(got[k], want[k]), (k, (got[k] != want[k]).sum().item())
    assert got['avg_steps'] == want['avg_steps'] == STEPS and got['step'] == STEPS


def test_a_torch_adamw_state_loads_exactly():
    from meme_challenge_amd import trainer as T
    m = _model('fp32x3')
    opt = T.get_optimizer(m, _config())
    assert opt.state_dict()['state'] == {}
    clones = [[torch.nn.Parameter(p.detach().clone()) for p in g['params']] for g in opt.param_groups]
    ref = torch.optim.AdamW([dict(params=c, weight_decay=g['weight_decay']) for c, g in zip(clones, opt.param_groups)], lr=3e-4,
                            betas=(0.8, 0.95))
    gen = torch.Generator(device='cuda').manual_seed(1)
    for _ in range(2):
        for c in clones:
            for p in c:
                p.grad = torch.randn(p.shape, generator=gen, device='cuda')
        ref.step()
    opt.load_state_dict(ref.state_dict())
    assert opt.step_count == 2
    assert opt.param_groups[0]['lr'] == 3e-4 and tuple(opt.param_groups[0]['betas']) == (0.8, 0.95)
    st = opt.store
    by_id = {id(p): n for n, p in st.params.items()}
    seen = 0
    for g, c in zip(opt.param_groups, clones):
        for p, q in zip(g['params'], c):
            o, k = st.offsets[by_id[id(p)]], p.numel()
            assert torch.equal(opt.exp_avg[o:o + k], ref.state[q]['exp_avg'].reshape(-1))
            assert torch.equal(opt.exp_avg_sq[o:o + k], ref.state[q]['exp_avg_sq'].reshape(-1))
            seen += k
    assert seen == sum(p.numel() for p in m.parameters())
    # .. and back: torch takes the fused optimizer's dict
    ref2 = torch.optim.AdamW([dict(params=c) for c in clones], lr=1e-3)
    ref2.load_state_dict(opt.state_dict())
    q = clones[0][0]
    assert torch.equal(ref2.state[q]['exp_avg'], ref.state[q]['exp_avg']) and float(ref2.state[q]['step']) == 2.0


def test_averaging_never_issues_a_rows_launch(monkeypatch):
    """UNITER_ADAM_WORD_ROWS=1 splits the word table's update by rows -- not with averaging on (there is no row-split form)"""
    from meme_challenge_amd import _lib, trainer as T
    monkeypatch.setenv('UNITER_ADAM_WORD_ROWS', '1')
    real, names = _lib.lib(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)

    spy = Spy()
    monkeypatch.setattr(_lib, 'lib', lambda: spy)
    for ema, rows in ((None, True), (DECAY, False)):
        del names[:]
        m, opt, sched, step = _setup('bf16', _config(ema_decay=ema))
        assert opt.split_word_rows is rows
        _iterate(step, opt, 0, 2)
        assert ('uniter_adam_step_rows' in names) is rows, sorted(set(names))
        assert ('uniter_optim_step_avg' in names) is (not rows)
