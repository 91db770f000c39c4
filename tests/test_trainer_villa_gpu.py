"""GPU: the VILLA step of trainer.TrainStep (adv_algo = 'villa') on the tiny model, with the helpers and the tolerance form of
tests/test_trainer_adv_gpu.py.

The arithmetic is checked as the FreeLB step's is: dropout 0, FusedSGD with lr 1, momentum 0, no weight decay, no clipping, so that
p - p' is the accumulated gradient g_clean + (1 / K) sum_k g_adv,k (summed over the rounds), against a float64 restatement of the
loop: the oracle forward, torch autograd, the same ascent rule, and the consistency term written out as the two Bernoulli KL
divergences with their four logarithms (the kernel's closed form is not restated here).

What keeps the comparison honest.  The settings are chosen so that the KL term moves the float64 reference gradient of linear.weight
by far more than the tolerance it is compared within -- a term that is silently dropped fails.  Checked on the CPU, in the float64
restatement alone, before these values were chosen (kl_weight 4):
    'txt', l2,   adv_lr 0.3, adv_max_norm 0.5:   max |g_ref(kl_weight) - g_ref(0)| / tolerance = 531
    'each', linf, adv_lr 0.1, adv_max_norm 0.15:  574 (the text round's doing: the tiny model's logits hardly move with the
                                                  regions, whose round ends with a KL term of 1.4e-8)
The test asserts a ratio of at least 10 for both."""
import pytest
import torch
import torch.nn.functional as Fn

import adv_ref as A
from oracle import uniter_oracle as O
from oracle import step_oracle as S
from common import TINY, TINY_IMG_DIM, maxdiff
from test_trainer_adv_gpu import WORD, POS_WT, _NoSchedule, _config, _model, _batch, _step, _ascend

pytestmark = pytest.mark.gpu

KL_WEIGHT = 4.0
SETTINGS = {            # modality, norm_type: adv_lr, adv_max_norm
    ('txt', 'l2'): (0.3, 0.5),
    ('each', 'linf'): (0.1, 0.15),
}
ROUNDS = {'txt': (('txt',),), 'img': (('img',),), 'both': (('txt', 'img'),), 'each': (('txt',), ('img',))}


def _villa_config(modality, norm_type, K, kl_weight=KL_WEIGHT, **kw):
    lr, max_norm = SETTINGS.get((modality, norm_type), (0.05, 0.3))
    c = dict(adv_algo='villa', adv_steps=K, adv_kl_weight=kl_weight, adv_norm_type=norm_type, adv_modality=modality, adv_lr=lr,
             adv_max_norm=max_norm, adv_init_mag=0.0)
    c.update(kw)
    return _config(**c)


def _sym_kl(z, c):
    """mean_b [KL(p||q) + KL(q||p)], p = sigmoid(c) constant, q = sigmoid(z): the four logarithms"""
    c = c.detach()
    p, q = torch.sigmoid(c), torch.sigmoid(z)
    lp, l1p, lq, l1q = Fn.logsigmoid(c), Fn.logsigmoid(-c), Fn.logsigmoid(z), Fn.logsigmoid(-z)
    return (p * (lp - lq) + (1 - p) * (l1p - l1q) + q * (lq - lp) + (1 - q) * (l1q - l1p)).mean()


def _oracle_pass(sd, b, cfg, d_txt, d_img, clean=None, kl_weight=0.0):
    """float64: logits, the loss terms and the parameter gradients of one pass with the perturbations applied (leaves of their own
    where they require a gradient); the word table's gradient is scattered back from the per-token rows"""
    B, T = b['input_ids'].shape
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    rows = leaves[WORD][b['input_ids'].view(-1)] + d_txt.view(B * T, -1)
    use = dict(leaves)
    use[WORD] = rows
    lo = O.meme_uniter_forward(use, cfg, input_ids=torch.arange(B * T).view(B, T), position_ids=b['position_ids'],
                               img_feat=b['img_feat'].double() + d_img, img_pos_feat=b['img_pos_feat'].double(),
                               attention_mask=b['attn_mask'], gather_index=b['gather_index'])
    bce = S.bce_with_logits(lo, b['labels'], POS_WT)
    kl = _sym_kl(lo.squeeze(1), clean) if clean is not None else torch.zeros((), dtype=torch.float64)
    total = bce + kl_weight * kl
    total.backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    g[WORD] = g[WORD].clone()
    g[WORD][0] = 0                     # padding_idx: the table's row 0 receives nothing
    return lo.detach().squeeze(1), (total.detach(), bce.detach(), kl.detach()), g


def _ascend_linf(d, g, lr, max_norm):
    B = d.shape[0]
    gm = g.reshape(B, -1).abs().max(dim=1).values.view(B, 1, 1)
    d = d + torch.where(gm > 0, lr * g / gm.clamp_min(1e-300), torch.zeros_like(g))
    return d.clamp(-max_norm, max_norm) if max_norm > 0 else d


def villa_reference(sd64, hb, cfg, d0, modality, norm_type, K, kl_weight, lr, max_norm):
    """the float64 restatement of a VILLA micro-batch -> dict grad (g_clean + sum over rounds of (1 / K) sum_k g_adv,k), g_clean,
    moved (per parameter, the largest |g_adv - g_clean| over the rounds' last passes), delta ({'txt', 'img'} after the rounds),
    terms (of the last perturbed pass), clean_loss"""
    ascend = _ascend if norm_type == 'l2' else _ascend_linf
    zero = {'txt': torch.zeros_like(d0['txt'], dtype=torch.float64), 'img': torch.zeros_like(d0['img'], dtype=torch.float64)}
    clean, clean_terms, gc = _oracle_pass(sd64, hb, cfg, zero['txt'], zero['img'])
    total = {k: v.clone() for k, v in gc.items()}
    moved = {k: 0.0 for k in gc}
    delta, terms = {'txt': None, 'img': None}, None
    for which in ROUNDS[modality]:
        d = {m: (d0[m].double() if m in which else zero[m]) for m in ('txt', 'img')}
        for k in range(K):
            leaf = {m: d[m].detach().clone().requires_grad_(m in which) for m in d}
            _, terms, g = _oracle_pass(sd64, hb, cfg, leaf['txt'], leaf['img'], clean, kl_weight)
            for n in total:
                total[n] += g[n] / K
            if k < K - 1:
                for m in which:
                    d[m] = ascend(d[m].detach(), leaf[m].grad, lr, max_norm)
        for n in moved:
            moved[n] = max(moved[n], (g[n] - gc[n]).abs().max().item())
        for m in which:
            delta[m] = d[m]
    return dict(grad=total, g_clean=gc, moved=moved, delta=delta, terms=terms, clean_loss=float(clean_terms[1]))


def grad_tolerance(ref, n):
    return 2e-6 + 2e-4 * (ref['grad'][n].abs().max().item() + ref['moved'][n])


def kl_ratio(ref, ref_without):
    """how far the KL term moves linear.weight's reference gradient, in units of the tolerance it is compared within"""
    n = 'linear.weight'
    return (ref['grad'][n] - ref_without['grad'][n]).abs().max().item() / grad_tolerance(ref, n)


def reference_inputs():
    cfg = dict(TINY, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd = O.synth_state_dict(cfg, seed=5, img_dim=TINY_IMG_DIM, ln_jitter=0.05)
    hb = _batch(device=None)
    B, T = hb['input_ids'].shape
    g = torch.Generator().manual_seed(21)
    d0 = {'txt': 0.02 * torch.randn(B, T, cfg['hidden_size'], generator=g), 'img': 0.05 * torch.randn(hb['img_feat'].shape, generator=g)}
    return cfg, sd, hb, d0


_REF = {}


def _reference(modality, norm_type):
    """the float64 restatement with the KL term and without it, computed once for both precisions"""
    key = (modality, norm_type)
    if key not in _REF:
        cfg, sd, hb, d0 = reference_inputs()
        if norm_type == 'linf':
            d0 = {k: v.clamp(-SETTINGS[key][1], SETTINGS[key][1]) for k, v in d0.items()}
        sd64 = {k: v.double() for k, v in sd.items()}
        lr, max_norm = SETTINGS[key]
        _REF[key] = (cfg, sd, d0, villa_reference(sd64, hb, cfg, d0, modality, norm_type, 2, KL_WEIGHT, lr, max_norm),
                     villa_reference(sd64, hb, cfg, d0, modality, norm_type, 2, 0.0, lr, max_norm))
    return _REF[key]


@pytest.mark.parametrize('modality, norm_type', list(SETTINGS))
@pytest.mark.parametrize('precision', ['fp32', 'fp32x3'])
def test_villa_two_passes_match_a_float64_restatement(precision, modality, norm_type, monkeypatch):
    from meme_challenge_amd import trainer
    cfg, sd, d0, ref, ref0 = _reference(modality, norm_type)
    ratio = kl_ratio(ref, ref0)
    print('the KL term moves the reference gradient of linear.weight by %.1f times its tolerance' % ratio)
    assert ratio >= 10.0

    seen = []
    plain = trainer.bce_kl_with_logits_loss

    def recording(logits, clean_logits, labels, *a, **kw):
        seen.append((logits.detach().clone(), clean_logits.detach().clone(), labels, a, kw))
        return plain(logits, clean_logits, labels, *a, **kw)
    monkeypatch.setattr(trainer, 'bce_kl_with_logits_loss', recording)

    m = _model(cfg, sd, precision)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    step = _step(m, _villa_config(modality, norm_type, 2))
    loss = step.train_iter(_batch(), adv_delta0={k: v.cuda() for k, v in d0.items()})
    step.optimizer.join()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert len(seen) == 2 * len(ROUNDS[modality])

    # the logged loss is the clean pass's
    assert abs(float(loss) - ref['clean_loss']) <= 2e-6 + 2e-4 * abs(ref['clean_loss'])

    # the perturbations after the ascent step
    for got, key in zip(step.last_adv_delta, ('txt', 'img')):
        want = ref['delta'][key]
        if want is None:
            assert got is None
            continue
        err, tol = maxdiff(got, want), 2e-6 + 2e-4 * want.abs().max().item()
        print('delta_%s after the ascent step: err %.3e bound %.3e' % (key, err, tol))
        assert err <= tol, (key, err, tol)
        assert maxdiff(got, d0[key]) > 1e-4           # it did move

    # the last perturbed pass's loss terms: within the kernel's bounds for the logits the launch was given, and the restatement's
    z, c, labels, a, kw = seen[-1]
    assert kw.get('grad_scale') == 0.5 and a[:2] == (POS_WT, KL_WEIGHT)
    kref = A.ref_bce_kl(z.cpu().numpy(), c.cpu().numpy(), labels.cpu().numpy(), POS_WT, KL_WEIGHT, 0.5)
    terms = step.last_adv_terms.cpu().numpy()
    for i, key in enumerate(('total', 'bce', 'kl')):
        assert A.worst_ratio(terms[i], kref[key], kref['E_' + key]) <= 1.0, (key, terms[i], kref[key], kref['E_' + key])
        want = float(ref['terms'][i])
        print('%s of the last perturbed pass: %.6e, float64 restatement %.6e' % (key, terms[i], want))
        assert abs(terms[i] - want) <= 2e-6 + 2e-4 * abs(want), (key, terms[i], want)
    assert terms[2] >= 0

    # the accumulated parameter gradient: (p - p') / lr with lr = 1
    worst = (0.0, 0.0, 0.0)
    for n, p in m.named_parameters():
        got = before[n].double().cpu() - p.detach().double().cpu()
        tol = grad_tolerance(ref, n)
        err = (got - ref['grad'][n]).abs().max().item()
        worst = max(worst, (err / tol, ref['grad'][n].abs().max().item(), ref['moved'][n]))
        assert err <= tol, (n, err, tol)
    print('accumulated gradient: worst err / bound %.3f (max |g_ref| %.3e, max |g_adv - g_clean| %.3e there)' % worst)


@pytest.mark.parametrize('precision', ['fp32', 'fp32x3'])
def test_villa_three_passes_with_adam_and_clipping(precision):
    """K = 3, Adam, max_grad_norm > 0, dropout on, a random start: the losses are finite, and the clip norm of the second step -- the
    first one behind an optimizer step that left the encoder's weight gradients for the next pass to overwrite -- is the norm of
    what the 1 + K passes accumulated (taken from a twin run whose second step does not clear the gradients)."""
    sd = O.synth_state_dict(TINY, seed=5, img_dim=TINY_IMG_DIM, ln_jitter=0.05)
    out = []
    for keep in (False, True):
        m = _model(TINY, sd, precision, deterministic=True)
        step = _step(m, _villa_config('both', 'l2', 3, kl_weight=1.0, optimizer='adam', lr=1e-3, beta1=0.9, max_grad_norm=0.05,
                                      adv_lr=0.05, adv_max_norm=0.3, adv_init_mag=0.2))
        opt = step.optimizer
        orig, calls = opt.step, []

        def wrapped(**kw):
            calls.append(1)
            if keep and len(calls) == 2:
                kw['zero_grads'] = False
            return orig(**kw)
        opt.step = wrapped
        losses = [step.train_iter(_batch(seed=3 + i)) for i in range(2)]
        opt.join()
        torch.cuda.synchronize()
        assert len(calls) == 2 and all(torch.isfinite(l) for l in losses) and bool(torch.isfinite(step.last_adv_terms).all())
        out.append((float(opt._sumsq.sqrt()), m.param_store().flat_grads.double().norm().item(), [float(l) for l in losses]))
    clip_norm, accumulated = out[0][0], out[1][1]
    print('clip norm %.9e, norm of the accumulated gradient %.9e' % (clip_norm, accumulated))
    assert out[0][2] == out[1][2]
    assert accumulated > 0 and abs(clip_norm - accumulated) <= 1e-6 * accumulated


@pytest.mark.parametrize('modality, norm_type', [('each', 'linf'), ('both', 'l2')])
def test_two_deterministic_villa_runs_are_bit_equal(modality, norm_type):
    sd = O.synth_state_dict(TINY, seed=5, img_dim=TINY_IMG_DIM, ln_jitter=0.05)
    params, terms = [], []
    for _ in range(2):
        m = _model(TINY, sd, 'fp32x3', deterministic=True)
        step = _step(m, _villa_config(modality, norm_type, 2, kl_weight=1.0, optimizer='adam', lr=1e-3, beta1=0.9, max_grad_norm=0.05,
                                      gradient_accumulation=2, adv_lr=0.05, adv_max_norm=0.1, adv_init_mag=0.2))
        for i in range(3):                              # iteration 0 steps alone, 1 accumulates, 2 steps
            step.train_iter(_batch(seed=3 + i))
        step.optimizer.join()
        torch.cuda.synchronize()
        assert m.uniter_model.bit_reproducible
        params.append(m.param_store().flat_params.clone())
        terms.append(step.last_adv_terms.clone())
    assert torch.equal(params[0], params[1]) and torch.equal(terms[0], terms[1])
    assert bool(torch.isfinite(params[0]).all())


def test_villa_refuses_a_gradient_exchange():
    from meme_challenge_amd._lib import UniterHipError
    from meme_challenge_amd.trainer import TrainStep, get_optimizer
    sd = O.synth_state_dict(TINY, seed=5, img_dim=TINY_IMG_DIM, ln_jitter=0.05)
    m = _model(TINY, sd, 'fp32')
    cfg = _villa_config('txt', 'l2', 2)
    with pytest.raises(UniterHipError, match='gradient exchange'):
        TrainStep(m, get_optimizer(m, cfg), _NoSchedule(), cfg, grad_sync=object())
