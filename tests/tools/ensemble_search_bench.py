"""What does the ensemble weight search cost, candidate by candidate on the host and in batches on either backend?  One GPU, one process:

    python tests/tools/ensemble_search_bench.py [--reps 5] [--parent_reps 3] [--models 15] [--sizes 500,5000]

Synthetic fold predictions (6-decimal probabilities, `--models` models, a fifteenth of every model's entries missing), per dev-set
size N of `--sizes`:

1. the default brute force of find_ensemble (10 000 tuples, both forms of each: 20 000 scored candidates) three ways:
     (a) parent   ensemble.brute_force_finder with find_ensemble's evaluation function: metrics.aucroc of
                  create_ensemble_prediction, one candidate at a time (what the package did before ensemble_search.py);
     (b) host     ensemble_search.brute_force_finder_batched on EnsembleScorer(backend='host');
     (c) hip      the same on EnsembleScorer(backend='hip'): uniter_ensemble_auc_counts;
   the three must pick the same (weights, on_logits);
2. one run of the evolutionary search (512 individuals, 100 generations: 51 712 scored candidates in 101 calls) on (b) and (c),
   which must return the same weights.

Wall clock around a whole search, from a synchronised start to a synchronised end (the scorer's planes are uploaded before the
clock starts; every call's weights go up and its counts come down inside it); one warm-up run per case discarded, then `--reps`
runs (`--parent_reps` for (a), which takes seconds to minutes), in alternating turns; median, minimum and maximum."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import numpy as np
import torch

from meme_challenge_amd import _lib
from meme_challenge_amd import ensemble as E
from meme_challenge_amd import ensemble_search as S
from meme_challenge_amd.metrics import aucroc

WEIGHT_RANGE, MAX_WEIGHTS = (0.0, 0.5, 1.0, 2.0), 10000


def synthetic(M, N, seed=0):
    rng = np.random.default_rng(seed)
    gt = (rng.random(N) < 0.5).astype(np.int64)
    p = np.round(np.clip(rng.normal(0.4 + 0.2 * gt[None, :], 0.25, size=(M, N)), 0.0, 1.0), 6)
    for m in range(M):
        p[m, rng.permutation(N)[:N // 15]] = -1.0
    return p, gt


def parent_brute_force(pred, gt):
    predictions = pred.copy()

    def eval_func(weights, on_logits=True):
        score = float(aucroc(E.create_ensemble_prediction(predictions, weights, on_logits), gt))
        predictions[predictions == -1] = 0.5
        return score,
    return E.brute_force_finder(eval_func, pred.shape[0], WEIGHT_RANGE, MAX_WEIGHTS)


def turns(cases, reps):
    """cases: name -> (callable, reps or None); -> name -> ([seconds per run], last result)"""
    times, last = {name: [] for name in cases}, {}
    for name, (run, _) in cases.items():
        t0 = time.perf_counter()
        last[name] = run()                       # warm-up: allocator, first launch, page cache
        print('  (warm-up %s: %.2f s)' % (name, time.perf_counter() - t0), file=sys.stderr, flush=True)
    for turn in range(max(r or reps for _, r in cases.values())):
        for name, (run, r) in cases.items():
            if turn >= (r or reps):
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = run()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    return times, last


def report(title, times, candidates, base):
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        print('%s %-8s %10.2f ms median (min %.2f max %.2f over %d runs)  %8.3f us per candidate  %7.1f x %s'
              % (title, name, 1e3 * med[name], 1e3 * min(t), 1e3 * max(t), len(t), 1e6 * med[name] / candidates, med[base] / med[name], base),
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5, help='timed runs per case')
    ap.add_argument('--parent_reps', type=int, default=3, help='timed runs of the one-candidate-at-a-time brute force (0: leave it out)')
    ap.add_argument('--models', type=int, default=15)
    ap.add_argument('--sizes', default='500,5000')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    print('device: %s; %s; library %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode(), os.path.basename(_lib.LIB_PATH)))
    M = args.models
    for N in (int(s) for s in args.sizes.split(',')):
        pred, gt = synthetic(M, N, seed=N)
        individual = [aucroc(np.where(p == -1, 0.5, p), gt) for p in pred]
        scorers = {b: S.EnsembleScorer(pred, gt, backend=b) for b in S.BACKENDS}
        print('M = %d models, N = %d samples (%d positive), %d entries missing' % (M, N, scorers['host'].n_pos, int((pred == -1).sum())), flush=True)
        cases = {b: ((lambda b=b: S.brute_force_finder_batched(scorers[b], M, WEIGHT_RANGE, MAX_WEIGHTS)), None) for b in S.BACKENDS}
        if args.parent_reps:
            cases['parent'] = ((lambda: parent_brute_force(pred, gt)), args.parent_reps)
        times, last = turns(cases, args.reps)
        assert len({(tuple(cfg['weights']), cfg['on_logits']) for _, cfg in last.values()}) == 1, last
        brute = last['hip']
        report('N=%-5d brute force 10000 x 2' % N, times, 2 * MAX_WEIGHTS, 'parent' if args.parent_reps else 'host')
        cases = {b: ((lambda b=b: S.ea_ensemble_finder(scorers[b], M, individual)), None) for b in S.BACKENDS}
        times, last = turns(cases, args.reps)
        assert last['host'] == last['hip'], last
        report('N=%-5d EA 512 x 100         ' % N, times, 512 * 101, 'host')
        print('N=%-5d scores: brute force %.6f, EA %.6f' % (N, brute[0], last['hip'][0]), flush=True)


if __name__ == '__main__':
    main()
