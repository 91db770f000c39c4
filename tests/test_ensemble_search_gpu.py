"""GPU: uniter_ensemble_auc_counts (csrc/ensemble.hip) and what is built on it, against tests/ensemble_ref.py -- the float64 numpy
restatement of the scoring contract in include/uniter_hip.h.

The counts are compared for EXACT equality.  The contract is double multiply, add and divide in a fixed order; the library is
built with -ffp-contract=off (no fused multiply-add), double division is correctly rounded on the device as on the host, and the
result is an integer.  There is no tolerance anywhere in this file.

The C ABI's refusals: the entry point follows the library's convention (include/uniter_hip.h) -- UNITER_E_ARG (-1) for NULL
pointers, UNITER_E_SHAPE (-2), through UCHECK_SHAPE, for N = 16385, M = 65 and C = 0."""
import csv
import ctypes

import numpy as np
import pytest
import torch

import ensemble_ref as R
from conftest import load_golden
from meme_challenge_amd import _lib
from meme_challenge_amd import ensemble as E
from meme_challenge_amd import ensemble_search as S
from meme_challenge_amd import metrics
from poison import Poison
from test_crossval_ensemble_cpu import _write_fold_files

pytestmark = pytest.mark.gpu


def _check_all_forms(pred, gt, w):
    """both planes, with and without `present`: the device's counts are the contract's"""
    prob, logit, present, n_pos = R.planes_of(pred, gt)
    scorer = S.EnsembleScorer(pred, gt, backend='hip')
    for on_logits, plane in ((False, prob), (True, logit)):
        for masked in (True, False):
            got = scorer.counts(w, on_logits, masked=masked)
            assert got.dtype == np.int64 and got.shape == (len(w),)
            want = R.auc_counts(plane, present if masked else None, w, n_pos)
            assert np.array_equal(got, want), (on_logits, masked, int((got != want).sum()), got[:4], want[:4])


@pytest.mark.parametrize('N,n_pos,M,C', R.shape_matrix())
def test_counts_equal_the_contract_exactly(N, n_pos, M, C):
    pred, gt = R.make_predictions(M, N, n_pos, missing=N // 7, seed=N + M)
    _check_all_forms(pred, gt, R.make_weights(C, M, seed=C))


def test_many_candidates():
    """C = 20 001 at N = 60: 64 distinct weight vectors (the reference scores each once) in a shuffled order with repeats"""
    pred, gt = R.make_predictions(3, 60, 29, missing=8, seed=5)
    prob, logit, present, n_pos = R.planes_of(pred, gt)
    distinct = R.make_weights(64, 3, seed=11)
    pick = np.random.default_rng(3).integers(0, 64, size=20001)
    scorer = S.EnsembleScorer(pred, gt, backend='hip')
    for on_logits, plane in ((False, prob), (True, logit)):
        want = R.auc_counts(plane, present, distinct, n_pos)[pick]
        assert np.array_equal(scorer.counts(distinct[pick], on_logits), want)


def test_the_lds_limit_and_the_largest_count():
    """N = 16 384, n_pos = 8 192, C = 2: model 0 separates the classes, so candidate (1, 0) counts 2 * 8192^2"""
    N, n_pos = 16384, 8192
    pred, gt = R.make_predictions(2, N, n_pos, missing=100, seed=6)
    pred[0] = np.round(np.where(gt == 1, 0.6, 0.1) + 0.3 * np.random.default_rng(1).random(N), 6)
    prob, logit, present, n1 = R.planes_of(pred, gt)
    w = np.array([[1.0, 0.0], [0.7, 1.9]])
    want = R.auc_counts(prob, present, w, n_pos)
    assert want[0] == 2 * 8192 * 8192 and 0 < want[1] < want[0]
    scorer = S.EnsembleScorer(pred, gt, backend='hip')
    assert np.array_equal(scorer.counts(w, False), want)
    assert scorer.scores(w, False)[0] == 1.0


def test_heavy_ties():
    M, N, n_pos = 4, 257, 120
    pred, gt = R.make_predictions(M, N, n_pos, missing=40, seed=7, grid=64)         # probabilities on a 1/64 lattice
    pred[:, 5] = -1.0                                               # a column every model misses
    pred[1:, 9] = -1.0                                              # a column whose only present model (0) ...
    w = R.make_weights(33, M, seed=8)
    w[0] = 0.0                                                      # every ws == 0: every score 0.5
    w[1::4, 0] = 0.0                                                # ... has weight 0 in these candidates
    w[2] = 1.0
    _check_all_forms(pred, gt, w)
    scorer = S.EnsembleScorer(pred, gt, backend='hip')
    half = n_pos * (N - n_pos)
    assert scorer.counts(w[:1], True)[0] == half and scorer.counts(w[:1], False, masked=False)[0] == half
    equal = S.EnsembleScorer(np.full((M, N), 0.25), gt, backend='hip')              # all scores equal: half the denominator
    assert equal.counts(w[1:], False).tolist() == [half] * 32 and equal.scores(w[2:3], True)[0] == 0.5


def test_find_ensemble_on_the_device_writes_the_golden_files(tmp_path):
    gold = load_golden('crossval_ensemble.npz')
    dev_files, test_files = _write_fold_files(gold, str(tmp_path))
    want = E.find_ensemble(dev_files, test_files)
    got = E.find_ensemble(dev_files, test_files, backend='hip')
    assert got['config'] == want['config'] == {'weights': (1.0, 0.5, 0.0), 'on_logits': False}
    assert got['threshold'] == want['threshold'] and got['score'] == want['score']
    for name in ('uniter_dev_seen_ensemble.csv', 'uniter_test_seen_ensemble.csv'):
        with open(tmp_path / name) as f:
            rows = list(csv.reader(f))
        assert rows[0] == gold['ens/out/%s/header' % name].tolist()
        body = np.array([[float(v) for v in r] for r in rows[1:]])
        assert np.abs(body - gold['ens/out/%s/body' % name]).max() < 2e-6, name


def test_ea_on_the_device_is_the_host_backends_run():
    pred, gt = R.make_predictions(5, 200, 96, missing=20, seed=12)
    individual = [metrics.aucroc(np.where(p == -1, 0.5, p), gt) for p in pred]
    runs = [S.ea_ensemble_finder(S.EnsembleScorer(pred, gt, backend=b), 5, individual, population_size=64, num_generations=8, seed=5,
                                 trace=True) for b in ('host', 'hip')]
    (score, config, trace), (d_score, d_config, d_trace) = runs
    assert np.array_equal(trace, d_trace) and config == d_config and score == d_score


@pytest.mark.parametrize('N', [2, 65, 1000])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_aucroc_device_equals_aucroc(N, dtype):
    rng = np.random.default_rng(N)
    y = np.arange(N) % 2 if N == 2 else (rng.random(N) < 0.4).astype(np.int64)
    p = torch.from_numpy(np.round(np.clip(rng.normal(0.4 + 0.2 * y, 0.25), 0, 1) * 32) / 32).to(dtype)      # ties included
    assert len(set(p.tolist())) < N or N == 2
    want = metrics.aucroc(p, y)
    assert metrics.aucroc_device(p.cuda(), torch.from_numpy(y).cuda()) == want
    assert metrics.aucroc_device(p.cuda().reshape(-1, 1), torch.from_numpy(y).cuda().to(torch.float32)) == want
    for one in (0, 1):                                              # one class only
        assert metrics.aucroc_device(p.cuda(), torch.full((N,), one, dtype=torch.int64, device='cuda')) == 0.0
    with pytest.raises(_lib.UniterHipError):
        metrics.aucroc_device(p, torch.from_numpy(y))               # host tensors are refused, not moved


@pytest.mark.parametrize('fill', ['ones', 'unit'])
def test_counts_do_not_depend_on_what_the_output_buffer_held(fill):
    pred, gt = R.make_predictions(3, 257, 130, missing=30, seed=13)
    w = R.make_weights(300, 3, seed=14)
    scorer = S.EnsembleScorer(pred, gt, backend='hip')
    plain = scorer.counts(w, True)
    with Poison(fill) as p:
        poisoned = scorer.counts(w, True)
        d_auc = metrics.aucroc_device(torch.from_numpy(pred[0].clip(0, 1)).cuda(), torch.from_numpy(gt).cuda())
    assert np.array_equal(poisoned, plain) and not p.broken
    assert {'ensemble_search.py:counts', 'metrics.py:aucroc_device'} <= p.functions(), p.report()
    assert d_auc == metrics.aucroc(pred[0].clip(0, 1), gt)


def test_c_abi_refuses_without_a_launch():
    lib = _lib.lib()
    M, N, C = 65, 16385, 4                                          # buffers as large as the largest call below claims
    x = torch.full((M, N), 0.25, dtype=torch.float64, device='cuda')
    w = torch.ones(C, M, dtype=torch.float64, device='cuda')
    counts = torch.full((C,), -7, dtype=torch.int64, device='cuda')
    good = dict(x=x, present=None, w=w, counts=counts, M=3, N=60, n_pos=30, C=C)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.uniter_ensemble_auc_counts(_lib.ptr(a['x']), _lib.ptr(a['present']), _lib.ptr(a['w']), _lib.ptr(a['counts']), a['M'],
                                            a['N'], a['n_pos'], a['C'], _lib.cur_stream())
        return rc, lib.uniter_last_error().decode()
    for kw, code, word in ((dict(x=None), -1, 'null'), (dict(w=None), -1, 'null'), (dict(counts=None), -1, 'null'),
                           (dict(N=16385), -2, 'N = 16385'), (dict(M=65), -2, 'M = 65'), (dict(C=0), -2, 'C = 0'),
                           (dict(n_pos=61), -1, 'n_pos = 61'), (dict(N=0, n_pos=0), -2, 'N = 0')):
        rc, message = call(**kw)
        assert rc == code and message.startswith('ensemble_auc_counts:') and word in message, (kw, rc, message)
    odd = ctypes.c_void_p(x.data_ptr() + 4)
    assert lib.uniter_ensemble_auc_counts(odd, None, _lib.ptr(w), _lib.ptr(counts), 3, 60, 30, C, _lib.cur_stream()) == -1
    assert 'aligned' in lib.uniter_last_error().decode()
    torch.cuda.synchronize()
    assert counts.tolist() == [-7] * C                              # nothing ran
    assert call()[0] == 0                                           # and the call they were derived from is good
    torch.cuda.synchronize()
    assert counts.tolist() == [30 * 30] * C                         # (all scores equal)
    with pytest.raises(_lib.UniterHipError, match='N = 16385'):     # the wrapper's check comes first, but the library's is there
        _lib.check(call(N=16385)[0], 'uniter_ensemble_auc_counts')
