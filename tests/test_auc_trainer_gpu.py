"""GPU: the pairwise AUROC term through the Python layers -- trainer.bce_auc_with_logits_loss and its autograd, trainer.ScoreBank,
and trainer.TrainStep with auc_weight > 0 on the tiny model (helpers of tests/test_trainer_adv_gpu.py): which passes carry the term,
which of them push into the bank, and that a run with auc_weight = 0 is today's run bit for bit."""
import numpy as np
import pytest
import torch

import auc_ref as A
from oracle import uniter_oracle as O
from common import TINY, TINY_IMG_DIM
from test_trainer_adv_gpu import POS_WT, _NoSchedule, _config, _model, _batch, _step

pytestmark = pytest.mark.gpu

AUC = dict(auc_weight=0.7, auc_bank=8, auc_surrogate='logistic', auc_margin=1.0)


def _sd():
    return O.synth_state_dict(TINY, seed=5, img_dim=TINY_IMG_DIM, ln_jitter=0.05)


def _record(monkeypatch):
    """every call of trainer.bce_auc_with_logits_loss from here on: (logits, labels, push)"""
    from meme_challenge_amd import trainer
    seen, plain = [], trainer.bce_auc_with_logits_loss

    def recording(logits, labels, *a, **kw):
        seen.append((logits.detach().clone().reshape(-1), labels.detach().clone().reshape(-1), kw.get('push', True)))
        return plain(logits, labels, *a, **kw)
    monkeypatch.setattr(trainer, 'bce_auc_with_logits_loss', recording)
    return seen


def _bank_state(bank):
    return [t.clone() for t in (bank.scores, bank.labels, bank.state)]


def _filled_bank(case):
    from meme_challenge_amd.trainer import ScoreBank
    b, bank = case['bank'], ScoreBank(case['bank'].N, 'cuda')
    bank.scores.copy_(torch.from_numpy(b.scores))
    bank.labels.copy_(torch.from_numpy(b.labels))
    bank.state.copy_(torch.from_numpy(b.state()))
    return bank


@pytest.mark.parametrize('name', ['B5_N8_fill8-logistic', 'label_2-hinge2', 'B2_one_of_each-logistic'])
def test_autograd_hands_back_the_kernels_dlogits(name):
    """the gradient of the loss is the launch's dlogits bit for bit -- through loss.backward(), through unit_gradient, and times an
    upstream gradient -- and the launch pushed; terms, probabilities and the value are the reference's; the extras carry no graph"""
    from meme_challenge_amd import _lib as L
    from meme_challenge_amd.trainer import bce_auc_with_logits_loss, unit_gradient
    case = dict(A.cases())[name]
    ref = A.ref_of(case)
    z, y = torch.from_numpy(case['z']).cuda(), torch.from_numpy(case['y']).cuda()
    sur = {0: 'logistic', 1: 'hinge2'}[case['kind']]
    kw = dict(surrogate=sur, margin=case['margin'], grad_scale=case['grad_scale'], return_terms=True, return_probs=True)

    # the kernel's own dlogits, from the C ABI on a copy of the bank
    bank = _filled_bank(case) if case['bank'] is not None else None
    want = torch.full((z.numel(),), float('nan'), device='cuda')
    bp = (bank.scores.data_ptr(), bank.labels.data_ptr(), bank.state.data_ptr(), bank.capacity) if bank is not None else (None, None, None, 0)
    L.check(L.lib().uniter_bce_auc_logits(z.data_ptr(), y.data_ptr(), case['pos_weight'], case['auc_weight'], case['kind'], case['margin'],
                                          *bp, 0, None, None, None, want.data_ptr(), case['grad_scale'], z.numel(), L.cur_stream()))

    for how in ('backward', 'unit', 'scaled'):
        bank = _filled_bank(case) if case['bank'] is not None else None
        leaf = z.clone().view(-1, 1).requires_grad_(True)              # the head's [B, 1]
        loss, terms, probs = bce_auc_with_logits_loss(leaf.squeeze(1), y, case['pos_weight'], case['auc_weight'], bank=bank, **kw)
        assert loss.requires_grad and not terms.requires_grad and not probs.requires_grad and loss.data_ptr() == terms.data_ptr()
        if how == 'backward':
            loss.backward()
        elif how == 'unit':
            loss.backward(unit_gradient(loss.device))
        else:
            (loss * 0.5).backward()
        got, exp = leaf.grad.reshape(-1), want if how != 'scaled' else want * 0.5
        assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (how, got, exp)
        if bank is not None:
            after = case['bank'].pushed(case['z'], case['y'])
            sc, lb = bank.contents()
            assert np.array_equal(sc.numpy().view(np.uint32), after.oldest_first()[0].view(np.uint32)) and lb.tolist() == after.oldest_first()[1].tolist()
        t = terms.cpu().numpy()
        for i, key in enumerate(('total', 'bce', 'auc')):
            assert A.worst_ratio(t[i], ref[key], ref['E_' + key]) <= 1.0, (key, t[i], ref[key])
        assert A.worst_ratio(probs.cpu().numpy(), ref['probs'], ref['E_probs']) <= 1.0
        assert A.worst_ratio(want.cpu().numpy(), ref['dlogits'], ref['E_dlogits']) <= 1.0

    # push=False leaves the bank alone; a bank on another device and an unknown surrogate are refused
    if case['bank'] is not None:
        bank = _filled_bank(case)
        before = _bank_state(bank)
        bce_auc_with_logits_loss(z, y, POS_WT, 0.7, bank=bank, push=False)
        assert all(torch.equal(a, b) for a, b in zip(before, _bank_state(bank)))
    with pytest.raises(ValueError, match='surrogate'):
        bce_auc_with_logits_loss(z, y, POS_WT, 0.7, surrogate='hinge')


def test_score_bank_reset_and_contents():
    from meme_challenge_amd.trainer import ScoreBank, bce_auc_with_logits_loss
    bank = ScoreBank(8, 'cuda')
    assert bank.contents()[0].numel() == 0
    pushed = []
    for k in range(3):
        z = torch.arange(3, dtype=torch.float32, device='cuda') + 10 * k
        bce_auc_with_logits_loss(z, torch.tensor([1, 0, 2], device='cuda'), POS_WT, 0.5, bank=bank)
        pushed += z.tolist()
    sc, lb = bank.contents()
    assert sc.tolist() == pushed[-8:] and lb.tolist() == [2, 1, 0, 2, 1, 0, 2, 1, 0, 2][-8:] and bank.state.tolist() == [1, 8]
    bank.reset()
    assert bank.state.tolist() == [0, 0] and bank.contents()[0].numel() == 0


@pytest.mark.parametrize('adv', [dict(), dict(adv_algo='villa', adv_steps=2, adv_kl_weight=1.0, adv_lr=0.05, adv_max_norm=0.3)],
                         ids=['plain', 'villa'])
def test_three_iterations_leave_the_last_eight_clean_logits_in_the_bank(adv, monkeypatch):
    """B = 4, auc_bank = 8: after three iterations the bank holds the clean passes' logits of iterations 1 and 2, oldest first.
    VILLA: the clean pass carries the term and pushes; the perturbed passes stay the BCE + KL loss"""
    seen = _record(monkeypatch)
    m = _model(TINY, _sd(), 'fp32', deterministic=True)
    step = _step(m, _config(optimizer='adam', lr=1e-3, beta1=0.9, max_grad_norm=0.05, **AUC, **adv))
    assert step.auc_bank is not None and step.auc_bank.capacity == 8
    batches = [_batch(seed=3 + i) for i in range(3)]
    losses = [step.train_iter(b) for b in batches]
    step.optimizer.join()
    torch.cuda.synchronize()
    assert len(seen) == 3 and all(push for _, _, push in seen) and all(torch.isfinite(l) for l in losses)
    sc, lb = step.auc_bank.contents()
    want = torch.cat([s for s, _, _ in seen])[-8:].cpu()
    assert torch.equal(sc.view(torch.int32), want.view(torch.int32))
    assert lb.tolist() == torch.cat([b['labels'].reshape(-1) for b in batches])[-8:].tolist()
    assert step.auc_bank.state.tolist() == [4, 8]
    # the logged loss is the total with the term, the recorded terms those of the last pass that carried it
    terms = step.last_auc_terms.cpu()
    assert float(losses[-1]) == float(terms[0]) and float(terms[2]) > 0 and float(terms[0]) > float(terms[1])
    ref = A.ref_bce_auc(seen[-1][0].cpu().numpy(), seen[-1][1].cpu().numpy(), POS_WT, 0.7, 0, 1.0, 1.0,
                        A.Bank(torch.cat([s for s, _, _ in seen])[:8].cpu().numpy(), torch.cat([l for _, l, _ in seen])[:8].cpu().numpy(), 0, 8))
    for i, key in enumerate(('total', 'bce', 'auc')):
        assert A.worst_ratio(terms[i].item(), ref[key], ref['E_' + key]) <= 1.0, (key, terms[i].item(), ref[key])
    if adv:
        assert step.last_adv_terms is not None and bool(torch.isfinite(step.last_adv_terms).all())


def test_eval_iter_leaves_the_bank_untouched_and_keeps_the_plain_loss(monkeypatch):
    from meme_challenge_amd.trainer import bce_with_logits_loss
    seen = _record(monkeypatch)
    m = _model(TINY, _sd(), 'fp32')
    step = _step(m, _config(**AUC))
    step.train_iter(_batch(seed=3))
    step.optimizer.join()
    before, calls = _bank_state(step.auc_bank), len(seen)
    m.eval()
    b = _batch(seed=4)
    loss, probs = step.eval_iter(b)
    torch.cuda.synchronize()
    assert len(seen) == calls == 1 and all(torch.equal(x, y) for x, y in zip(before, _bank_state(step.auc_bank)))
    with torch.no_grad():
        plain = bce_with_logits_loss(m(**step.forward_kwargs(b)).squeeze(1), b['labels'], POS_WT)
    assert abs(float(loss) - float(plain)) <= 1e-6


def test_calculate_loss_carries_the_term_when_it_steps_and_not_when_it_evaluates():
    """TrainerTemplate.calculate_loss on a bare instance: grad_step=True logs BCE + the term and pushes; grad_step=False logs the
    plain BCE and leaves the bank alone"""
    from meme_challenge_amd.train_template import EpochLog, TrainerTemplate
    from meme_challenge_amd.trainer import TrainStep, auc_config, bce_with_logits_loss, get_optimizer, new_score_bank
    m = _model(TINY, _sd(), 'fp32')
    cfg = _config(optimizer='adam', lr=1e-3, beta1=0.9, max_grad_norm=0.05, **AUC)
    t = object.__new__(TrainerTemplate)
    t.config, t.auc, t.grad_sync, t.iters, t._ids = cfg, auc_config(cfg), None, 0, None
    t.auc_bank, t.optimizer, t.scheduler, t.log = new_score_bank(t.auc, 'cuda'), get_optimizer(m, cfg), _NoSchedule(), EpochLog('cuda')
    b = _batch(seed=4)                                  # labels 1, 0, 1, 0: four pairs inside the batch
    before = m.param_store().flat_params.clone()
    preds = m(**TrainStep.forward_kwargs(b))
    t.calculate_loss(preds, b['labels'], grad_step=True)
    t.optimizer.join()
    sc, lb = t.auc_bank.contents()
    assert t.auc_bank.state.tolist() == [4, 4] and lb.tolist() == [1, 0, 1, 0]
    assert torch.equal(sc.view(torch.int32), preds.detach().reshape(-1).cpu().view(torch.int32))
    assert not torch.equal(before, m.param_store().flat_params)
    state = _bank_state(t.auc_bank)
    m.eval()
    with torch.no_grad():
        preds2 = m(**TrainStep.forward_kwargs(b))
        t.calculate_loss(preds2, b['labels'], grad_step=False)
        plain2 = bce_with_logits_loss(preds2.squeeze(1), b['labels'], POS_WT)
        plain1 = bce_with_logits_loss(preds.detach().squeeze(1), b['labels'], POS_WT)
    logged = t.log._buf['loss'][:2]
    assert t.log.k == 2 and torch.equal(logged[1], plain2) and float(logged[0]) > float(plain1) + 0.1      # 0.7 softplus(..) of about 0.7
    assert all(torch.equal(x, y) for x, y in zip(state, _bank_state(t.auc_bank)))


def test_a_freelb_micro_batch_pushes_once(monkeypatch):
    seen = _record(monkeypatch)
    m = _model(TINY, _sd(), 'fp32')
    step = _step(m, _config(adv_steps=2, adv_lr=0.3, adv_max_norm=0.5, adv_init_mag=0.1, adv_modality='both', **AUC))
    b = _batch(seed=3)
    step.train_iter(b)
    step.optimizer.join()
    torch.cuda.synchronize()
    assert [push for _, _, push in seen] == [True, False]
    sc, lb = step.auc_bank.contents()
    assert step.auc_bank.state.tolist() == [4, 4] and lb.tolist() == b['labels'].reshape(-1).tolist()
    assert torch.equal(sc.view(torch.int32), seen[0][0].cpu().view(torch.int32))
    assert not torch.equal(seen[0][0], seen[1][0])                     # the second pass ran on the moved perturbation


def test_auc_weight_zero_is_todays_run_bit_for_bit(monkeypatch):
    """deterministic = True: the parameters after three steps with auc_weight = 0 (and a bank size that is then ignored) equal those of
    a run that never sets the keys; no ScoreBank is made and the new loss is never called"""
    seen = _record(monkeypatch)
    params = []
    for extra in (dict(), dict(auc_weight=0.0, auc_bank=8, auc_surrogate='hinge2', auc_margin=0.5)):
        m = _model(TINY, _sd(), 'fp32x3', deterministic=True)
        step = _step(m, _config(optimizer='adam', lr=1e-3, beta1=0.9, max_grad_norm=0.05, gradient_accumulation=2, **extra))
        assert step.auc_bank is None
        for i in range(3):                              # iteration 0 steps alone, 1 accumulates, 2 steps
            step.train_iter(_batch(seed=3 + i))
        step.optimizer.join()
        torch.cuda.synchronize()
        assert m.uniter_model.bit_reproducible
        params.append(m.param_store().flat_params.clone())
    assert not seen and torch.equal(params[0], params[1]) and bool(torch.isfinite(params[0]).all())


def test_the_term_moves_the_parameters():
    """the same three steps with and without the term end at different parameters: the term reaches the optimizer"""
    params = []
    for extra in (dict(), AUC):
        m = _model(TINY, _sd(), 'fp32x3', deterministic=True)
        step = _step(m, _config(optimizer='adam', lr=1e-3, beta1=0.9, max_grad_norm=0.05, **extra))
        for i in range(3):
            step.train_iter(_batch(seed=3 + i))
        step.optimizer.join()
        torch.cuda.synchronize()
        params.append(m.param_store().flat_params.clone())
    assert not torch.equal(params[0], params[1]) and bool(torch.isfinite(params[1]).all())


@pytest.mark.parametrize('config, match', [
    (dict(auc_weight=-0.1), 'auc_weight'),
    (dict(auc_weight=float('nan')), 'auc_weight'),
    (dict(auc_weight=0.5, auc_surrogate='hinge'), 'auc_surrogate'),
    (dict(auc_surrogate='exp'), 'auc_surrogate'),
    (dict(auc_weight=0.5, loss_func='bce'), 'loss_func'),
    (dict(auc_weight=0.5, loss_func='ce'), 'loss_func'),
    (dict(auc_weight=0.5, auc_bank=3, batch_size=4), 'auc_bank'),
    (dict(auc_weight=0.5, auc_bank=8193), 'auc_bank'),
    (dict(auc_weight=0.5, auc_margin=float('nan')), 'auc_margin'),
])
def test_config_refusals(config, match, refusal_model):
    """by auc_config itself, and by a TrainStep before it builds anything"""
    from meme_challenge_amd.trainer import TrainStep, auc_config
    with pytest.raises(ValueError, match=match):
        auc_config(_config(**config))
    m, opt = refusal_model
    with pytest.raises(ValueError, match=match):
        TrainStep(m, opt, _NoSchedule(), _config(**config))


@pytest.fixture(scope='module')
def refusal_model():
    from meme_challenge_amd.trainer import get_optimizer
    m = _model(TINY, _sd(), 'fp32')
    return m, get_optimizer(m, _config())
