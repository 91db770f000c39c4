"""CPU: the batched ensemble weight search (meme_challenge_amd/ensemble_search.py) with its host backend.

The scoring contract is the one written in include/uniter_hip.h, restated in tests/ensemble_ref.py.  Pinned here: that contract's
score is `metrics.aucroc(create_ensemble_prediction(..))` bit for bit on 6-decimal probabilities; the host backend counts what the
contract counts; the batched brute force picks what `brute_force_finder` picks and `find_ensemble` writes the same files through
it; the evolutionary search by its properties (it cannot be compared with `deap`, which is not installed anywhere this suite
runs); the refusals; and that `find_ensemble`'s defaults still take the path they took."""
import csv

import numpy as np
import pytest

import ensemble_ref as R
from conftest import load_golden
from meme_challenge_amd import ensemble as E
from meme_challenge_amd import ensemble_search as S
from meme_challenge_amd.metrics import aucroc
from test_crossval_ensemble_cpu import _write_fold_files


@pytest.fixture(scope='module')
def gold():
    return load_golden('crossval_ensemble.npz')


@pytest.mark.parametrize('M,N,missing', [(3, 60, 0), (3, 60, 10), (5, 200, 0), (5, 200, 20), (8, 500, 0), (8, 500, 30)])
def test_the_contract_score_is_aucroc_of_the_ensemble_prediction_bit_for_bit(M, N, missing):
    pred, gt = R.make_predictions(M, N, N // 2 - 3, missing=missing, seed=M)
    prob, logit, present, n_pos = R.planes_of(pred, gt)
    w = R.make_weights(24, M, seed=N, grid_only=True)
    w[0], w[1] = 0.0, 1.0                                           # nobody votes (every score 0.5); the plain mean
    denominator = 2.0 * n_pos * (N - n_pos)
    for on_logits, plane in ((False, prob), (True, logit)):
        counts = R.auc_counts(plane, present if missing else None, w, n_pos)
        want = [aucroc(E.create_ensemble_prediction(pred, w[c], on_logits), gt) for c in range(w.shape[0])]
        assert (counts / denominator).tolist() == want, on_logits
    assert counts[0] == n_pos * (N - n_pos)


@pytest.mark.parametrize('N,n_pos,M,C', R.shape_matrix())
def test_host_backend_counts_what_the_contract_counts(N, n_pos, M, C):
    pred, gt = R.make_predictions(M, N, n_pos, missing=N // 7, seed=N + M)
    prob, logit, present, n1 = R.planes_of(pred, gt)
    w = R.make_weights(C, M, seed=C)
    scorer = S.EnsembleScorer(pred, gt, backend='host')
    assert (scorer.n_pos, scorer.denominator) == (n_pos, 2 * n_pos * (N - n_pos)) and n1 == n_pos
    for on_logits, plane in ((False, prob), (True, logit)):
        for masked in (True, False):
            got = scorer.counts(w, on_logits, masked=masked)
            assert got.dtype == np.int64 and got.shape == (C,)
            assert np.array_equal(got, R.auc_counts(plane, present if masked else None, w, n_pos)), (on_logits, masked)
    s = scorer.scores(w, True)
    assert s.dtype == np.float64 and (np.array_equal(s, got * 0.0) if scorer.denominator == 0 else s.max() <= 1.0)


def test_host_backend_chunks_its_candidates(monkeypatch):
    pred, gt = R.make_predictions(3, 60, 30, missing=5, seed=1)
    w = R.make_weights(41, 3, seed=2)
    whole = S.EnsembleScorer(pred, gt).counts(w, True)
    monkeypatch.setattr(S, '_HOST_CHUNK_ELEMS', 60 * 4)             # 4 candidates per chunk, the last chunk of one
    assert np.array_equal(S.EnsembleScorer(pred, gt).counts(w, True), whole)


def _fold_predictions(gold, tmp_path):
    dev_files, test_files = _write_fold_files(gold, str(tmp_path))
    dev = E.align_ids([E.load_csv(f) for f in dev_files])
    return dev_files, test_files, np.stack([d['proba'] for d in dev], axis=0), dev[0]['gt']


def _host_eval(predictions, gt):
    predictions = predictions.copy()

    def eval_func(weights, on_logits=True):                        # find_ensemble's, with its in-place fill
        score = float(aucroc(E.create_ensemble_prediction(predictions, weights, on_logits), gt))
        predictions[predictions == -1] = 0.5
        return score,
    return eval_func


@pytest.mark.parametrize('weight_range,max_weights', [((0.0, 0.5, 1.0, 2.0), 10000), ((0.0, 0.5, 1.0, 2.0), 20),
                                                      (tuple(0.25 * k for k in range(9)), 300)])
def test_batched_brute_force_picks_what_brute_force_finder_picks(gold, tmp_path, weight_range, max_weights):
    _, _, predictions, gt = _fold_predictions(gold, tmp_path)
    assert (predictions == -1).any()                                # the folds miss samples: the first evaluation's mask matters
    want_score, want = E.brute_force_finder(_host_eval(predictions, gt), 3, weight_range, max_weights)
    scorer = S.EnsembleScorer(predictions, gt, backend='host')
    score, config = S.brute_force_finder_batched(scorer, 3, weight_range, max_weights)
    assert config == want and score == want_score
    assert scorer.calls == 3                                        # both forms of every tuple, and tuple 0 on logits with the mask


def test_batched_brute_force_draws_the_tuples_of_a_grid_too_large_to_list():
    pred, gt = R.make_predictions(13, 60, 30, seed=4)               # 4^13 > 2e7: seeded draws instead of the grid
    want_score, want = E.brute_force_finder(_host_eval(pred, gt), 13, (0.0, 0.5, 1.0, 2.0), 50)
    score, config = S.brute_force_finder_batched(S.EnsembleScorer(pred, gt), 13, (0.0, 0.5, 1.0, 2.0), 50)
    assert config == want and score == want_score


def _bodies(tmp_path):
    out = {}
    for name in ('uniter_dev_seen_ensemble.csv', 'uniter_test_seen_ensemble.csv'):
        with open(tmp_path / name) as f:
            out[name] = f.read()
    return out


def test_find_ensemble_through_the_scorer_writes_the_files_of_the_default_path(gold, tmp_path):
    dev_files, test_files, predictions, gt = _fold_predictions(gold, tmp_path)
    want = E.find_ensemble(dev_files, test_files)
    want_files = _bodies(tmp_path)
    scorer_made = []
    real = S.EnsembleScorer

    class Spy(real):
        def __init__(self, *a, **kw):
            scorer_made.append(kw.get('backend'))
            real.__init__(self, *a, **kw)
    mp = pytest.MonkeyPatch()
    mp.setattr(S, 'EnsembleScorer', Spy)
    try:      # ea=False with the host backend is the old path.  Through the scorer, then, with an EA that cannot win: no generations,
        #       one individual, weights confined to [0, 0] (every score 0.5)
        got = E.find_ensemble(dev_files, test_files, ea=True,
                              ea_kwargs=dict(population_size=1, num_generations=0, min_weight=0.0, max_weight=0.0))
    finally:
        mp.undo()
    assert scorer_made == ['host']
    assert got['config'] == want['config'] and got['threshold'] == want['threshold'] and got['score'] == want['score']
    assert _bodies(tmp_path) == want_files
    for name, text in want_files.items():                           # (and those are the reference's files)
        rows = list(csv.reader(text.splitlines()))
        body = np.array([[float(v) for v in r] for r in rows[1:]])
        assert np.abs(body - gold['ens/out/%s/body' % name]).max() < 2e-6


def test_find_ensemble_defaults_take_the_old_path(gold, tmp_path, monkeypatch):
    dev_files, test_files, _, _ = _fold_predictions(gold, tmp_path)
    calls = []
    real = E.brute_force_finder

    def spy(eval_func, num_weights, weight_range, max_weights=1e5):
        calls.append((num_weights, tuple(weight_range), max_weights))
        return real(eval_func, num_weights, weight_range, max_weights)
    monkeypatch.setattr(E, 'brute_force_finder', spy)
    monkeypatch.setattr(S, 'EnsembleScorer', None)                  # the default path builds no scorer
    res = E.find_ensemble(dev_files, test_files)
    assert calls == [(3, (0.0, 0.5, 1.0, 2.0), 10000)]
    assert res['config'] == {'weights': (1.0, 0.5, 0.0), 'on_logits': False}
    with pytest.raises(ValueError):
        E.find_ensemble(dev_files, test_files, backend='triton')


# ---- the evolutionary search: population 32, 6 generations, M = 4, N = 60 ------------------------------------------------------
EA = dict(population_size=32, num_generations=6)


@pytest.fixture(scope='module')
def ea_case():
    pred, gt = R.make_predictions(4, 60, 28, missing=6, seed=9)
    individual = [aucroc(np.where(p == -1, 0.5, p), gt) for p in pred]
    return pred, gt, individual


def test_ea_same_seed_same_result_and_weights_in_range(ea_case):
    pred, gt, individual = ea_case
    runs = [S.ea_ensemble_finder(S.EnsembleScorer(pred, gt), 4, individual, seed=7, trace=True, **EA) for _ in range(2)]
    (score, config, trace), (score2, config2, trace2) = runs
    assert score == score2 and config == config2 and np.array_equal(trace, trace2)
    assert config['on_logits'] is True and len(config['weights']) == 4
    assert all(0.0 <= v <= 4.0 for v in config['weights'])
    other = S.ea_ensemble_finder(S.EnsembleScorer(pred, gt), 4, individual, seed=8, trace=True, **EA)
    assert other[1] != config                                       # (the seed is what decides)
    assert S.ea_ensemble_finder(S.EnsembleScorer(pred, gt), 4, individual, seed=7, **EA) == (score, config)


def test_ea_trace_never_decreases_and_starts_at_the_initial_populations_best(ea_case):
    pred, gt, individual = ea_case
    scorer = S.EnsembleScorer(pred, gt)
    score, config, trace = S.ea_ensemble_finder(scorer, 4, individual, seed=7, trace=True, **EA)
    assert trace.dtype == np.int64 and trace.shape == (7,) and np.all(np.diff(trace) >= 0)
    assert scorer.calls == 7                                        # the initial population, then one call per generation
    initial = S.ea_initial_population(np.random.default_rng(7), 4, individual, 32)
    assert initial.shape == (32, 4) and initial.min() >= 0.0 and initial.max() <= 4.0
    first = R.auc_counts(R.planes_of(pred, gt)[1], R.planes_of(pred, gt)[2], initial, scorer.n_pos)
    assert trace[0] == first.max() and trace[-1] >= first.max()
    # the result is the score of the weights it returns
    assert score == trace[-1] / scorer.denominator
    assert R.auc_counts(R.planes_of(pred, gt)[1], R.planes_of(pred, gt)[2], [config['weights']], scorer.n_pos)[0] == trace[-1]


def test_ea_with_equal_individual_scores_does_not_divide_by_zero(ea_case):
    pred, gt, _ = ea_case
    score, config = S.ea_ensemble_finder(S.EnsembleScorer(pred, gt), 4, [0.7] * 4, seed=1, **EA)
    assert np.isfinite(config['weights']).all() and 0.0 <= score <= 1.0


def test_ea_reinitialises_a_stagnant_population(ea_case):
    pred, gt, individual = ea_case
    scorer = S.EnsembleScorer(np.full((4, 60), 0.5), gt)            # every candidate scores the same: no generation improves
    score, config, trace = S.ea_ensemble_finder(scorer, 4, individual, population_size=4, num_generations=52, seed=1, trace=True)
    assert len(set(trace.tolist())) == 1 and score == 0.5
    assert scorer.calls == 1 + 52 + 1                               # one fresh population, scored, after 50 generations


def test_find_ensemble_with_ea_is_at_least_the_brute_force(gold, tmp_path):
    dev_files, test_files, _, _ = _fold_predictions(gold, tmp_path)
    brute = E.find_ensemble(dev_files, test_files)
    got = E.find_ensemble(dev_files, test_files, ea=True, ea_kwargs=dict(seed=3, **EA))
    assert got['score'] >= brute['score']
    assert got['config'] == brute['config'] or (got['config']['on_logits'] is True and got['score'] > brute['score'])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', [(2, 16385), (65, 8)])
def test_hip_backend_refuses_beyond_the_kernels_limits_before_any_library_call(monkeypatch, M, N):
    from meme_challenge_amd import _lib

    def no_library(*a, **kw):
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'lib', no_library)
    gt = np.arange(N) % 2
    with pytest.raises(ValueError, match="backend='host'"):
        S.EnsembleScorer(np.full((M, N), 0.25), gt, backend='hip')
    S.EnsembleScorer(np.full((M, N), 0.25), gt, backend='host')     # the host backend has no such limit


def test_scorer_refuses_bad_weights_labels_and_probabilities():
    pred, gt = R.make_predictions(3, 20, 10, seed=2)
    scorer = S.EnsembleScorer(pred, gt)
    for bad in (np.ones((5, 2)), np.ones((5, 4)), np.ones(2), np.ones((2, 5, 3))):
        with pytest.raises(ValueError):
            scorer.counts(bad, True)
    assert scorer.counts(np.ones(3), True).shape == (1,)           # one vector is one candidate
    for labels in (np.where(gt == 1, 2, gt), gt - 1, gt[:-1]):
        with pytest.raises(ValueError):
            S.EnsembleScorer(pred, labels)
    with pytest.raises(ValueError):
        S.EnsembleScorer(pred + 1.5, gt)
    with pytest.raises(ValueError):
        S.EnsembleScorer(pred, gt, backend='triton')
    with pytest.raises(ValueError):
        S.ea_ensemble_finder(scorer, 4, [0.5] * 4, **EA)


def test_cli_flags_and_crossval_pass_the_backend_and_the_ea_switch(monkeypatch, tmp_path):
    import argparse
    from meme_challenge_amd import crossval as CV
    from meme_challenge_amd.train_template import TrainerTemplate
    parser = argparse.ArgumentParser()
    TrainerTemplate.add_default_argparse(parser)
    args = parser.parse_args([])
    assert (args.ensemble_backend, args.ensemble_ea) == ('host', False)
    args = parser.parse_args(['--ensemble_backend', 'hip', '--ensemble_ea'])
    assert (args.ensemble_backend, args.ensemble_ea) == ('hip', True)
    with pytest.raises(SystemExit):
        parser.parse_args(['--ensemble_backend', 'cuda'])
    seen = []
    monkeypatch.setattr(CV, 'find_ensemble', lambda **kw: seen.append(kw))
    for k in range(2):
        (tmp_path / ('m_fold_%d_dev_seen_preds.csv' % k)).write_text('id,proba,label,gt\n')

    class Loader:
        def __init__(self, path):
            self.dataset = type('D', (), {'name': 'dev_seen'})()

    class Trainer:
        def __init__(self, config):
            pass

        def train_main(self):
            return {'loss': 0.5}, {}
    (tmp_path / 'crossval_16').mkdir()
    for k in range(2):
        for part in ('train', 'dev'):
            (tmp_path / 'crossval_16' / ('%s_%02d.jsonl' % (part, k))).write_text('{}')
    base = {'data_path': str(tmp_path), 'model_path': str(tmp_path), 'model_save_name': 'm.pt', 'seed': 1, 'test_loader': [Loader('x')]}
    funcs = {k: Loader for k in ('train', 'val', 'test')}
    CV.train_crossval(Trainer, dict(base), funcs, num_folds=2, dev_size=16)
    CV.train_crossval(Trainer, dict(base, ensemble_backend='hip', ensemble_ea=True), funcs, num_folds=2, dev_size=16)
    assert [(kw['backend'], kw['ea']) for kw in seen] == [('host', False), ('hip', True)]
