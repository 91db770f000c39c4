"""Batched search for the ensemble weights: many weight vectors scored against one fixed prediction matrix.

`ensemble.find_ensemble` scores one candidate at a time (`metrics.aucroc` of `create_ensemble_prediction`).  Here a candidate's
score is an integer pair count defined by the scoring contract in include/uniter_hip.h (the mixed score of
`create_ensemble_prediction` without its final sigmoid; counts = 2 * greater + equal over positive / negative pairs), and C
candidates are scored in one call:

  * `EnsembleScorer(predictions, gt, backend)` prepares the planes once (missing entries filled with 0.5, logits, present mask,
    positives-first column order) and scores weight matrices: backend 'hip' is one `uniter_ensemble_auc_counts` launch
    (csrc/ensemble.hip), backend 'host' the same contract in numpy;
  * `brute_force_finder_batched` is `ensemble.brute_force_finder` on a scorer: the same tuples, the same winner;
  * `ea_ensemble_finder` is the evolutionary search the reference runs when `deap` is installed (utils/ensemble.py:206-272),
    restated on a seeded numpy generator.
"""
import logging

import numpy as np
import torch

from . import _lib
from .ensemble import weight_tuples

logger = logging.getLogger('EnsembleLogger')

MAX_N, MAX_M = 16384, 64          # UNITER_ENSEMBLE_MAX_N / _MAX_M (include/uniter_hip.h)
BACKENDS = ('host', 'hip')
_HOST_CHUNK_ELEMS = 1 << 22       # candidates x samples per host chunk (32 MB of doubles per temporary)


def check_hip_limits(M, N):
    """The kernel keeps a candidate's N scores in LDS; the library refuses beyond these limits, and so does this, before any call."""
    if N > MAX_N or M > MAX_M:
        raise ValueError("backend='hip' scores at most %d samples of at most %d models (got %d samples, %d models): use backend='host'"
                         % (MAX_N, MAX_M, N, M))


class EnsembleScorer(object):
    """predictions: [M, N] probabilities, -1 = the model did not predict the sample; gt: [N] labels in {0, 1}."""

    def __init__(self, predictions, gt, backend='host'):
        if backend not in BACKENDS:
            raise ValueError('backend must be one of %s; got %r' % (BACKENDS, backend))
        p = np.array(np.stack(predictions, axis=0) if isinstance(predictions, (list, tuple)) else predictions, dtype=np.float64)
        y = np.asarray(gt)
        if p.ndim != 2 or y.shape != (p.shape[1],):
            raise ValueError('predictions must be [models, samples] and gt [samples]; got %s and %s' % (p.shape, y.shape))
        if not np.all((y == 0) | (y == 1)):
            raise ValueError('Labels must be binary (0 or 1)')
        self.M, self.N = p.shape
        self.backend = backend
        if backend == 'hip':
            check_hip_limits(self.M, self.N)
        missing = p == -1
        if not np.all(missing | ((p >= 0.0) & (p <= 1.0))):
            raise ValueError('Probabilities must be between 0 and 1 (or -1 for a missing entry)')
        p[missing] = 0.5
        order = np.concatenate([np.flatnonzero(y == 1), np.flatnonzero(y == 0)])       # positives first
        self.n_pos = int((y == 1).sum())
        self.denominator = 2 * self.n_pos * (self.N - self.n_pos)
        self.any_missing = bool(missing.any())
        logits = np.log(np.clip(p, 1e-8, 1.0)) - np.log(np.clip(1 - p, 1e-8, 1.0))    # (0.5 -> exactly 0)
        self._planes = {False: np.ascontiguousarray(p[:, order]), True: np.ascontiguousarray(logits[:, order])}
        self._present = np.ascontiguousarray((1.0 - missing)[:, order])
        self.calls = 0                                                                 # scorer calls so far
        if backend == 'hip':
            _lib.lib()
            self._d_planes = {k: torch.from_numpy(v).cuda() for k, v in self._planes.items()}
            self._d_present = torch.from_numpy(self._present).cuda()

    def _weights(self, weights):
        w = np.ascontiguousarray(np.atleast_2d(np.asarray(weights, dtype=np.float64)))
        if w.ndim != 2 or w.shape[1] != self.M or w.shape[0] < 1:
            raise ValueError('weights must be [candidates, %d]; got %s' % (self.M, w.shape))
        return w

    def counts(self, weights, on_logits, masked=True):
        """int64 [C]: the contract's pair counts of the C rows of `weights`.  masked=False scores the filled planes with every entry
        present (a missing entry votes 0.5 with the model's full weight)."""
        w = self._weights(weights)
        self.calls += 1
        masked = masked and self.any_missing
        if self.backend == 'hip':
            d_w = torch.from_numpy(w).cuda()
            out = torch.empty(w.shape[0], dtype=torch.int64, device=d_w.device)
            _lib.check(_lib.lib().uniter_ensemble_auc_counts(
                _lib.ptr(self._d_planes[bool(on_logits)]), _lib.ptr(self._d_present if masked else None), _lib.ptr(d_w), _lib.ptr(out),
                self.M, self.N, self.n_pos, w.shape[0], _lib.cur_stream()), 'uniter_ensemble_auc_counts')
            return out.cpu().numpy()
        return self._counts_host(w, self._planes[bool(on_logits)], self._present if masked else None)

    def scores(self, weights, on_logits, masked=True):
        """float64 [C]: counts / (2 * positives * negatives); 0.0 with one class only, as metrics.aucroc"""
        c = self.counts(weights, on_logits, masked)
        return c / float(self.denominator) if self.denominator else np.zeros(c.shape, dtype=np.float64)

    def _counts_host(self, w, x, present):
        out = np.zeros(w.shape[0], dtype=np.int64)
        if self.denominator == 0:
            return out
        step = max(1, _HOST_CHUNK_ELEMS // self.N)
        for c0 in range(0, w.shape[0], step):
            wc = w[c0:c0 + step]
            num = np.zeros((wc.shape[0], self.N))
            ws = np.zeros((wc.shape[0], self.N))
            for m in range(self.M):                                  # the contract's order: one model after the other
                wm = wc[:, m:m + 1]
                if present is None:
                    num = num + wm * x[m]
                    ws = ws + wm
                else:
                    num = num + (wm * x[m]) * present[m]
                    ws = ws + wm * present[m]
            s = num / np.minimum(np.maximum(ws, 1e-4), 1e5)
            s[ws == 0.0] = 0.5
            neg = np.sort(s[:, self.n_pos:], axis=1)
            for k in range(wc.shape[0]):                             # negatives below + negatives not above = 2 * greater + equal
                pos = s[k, :self.n_pos]
                out[c0 + k] = int(np.searchsorted(neg[k], pos, side='left').sum()) + int(np.searchsorted(neg[k], pos, side='right').sum())
        return out


def brute_force_finder_batched(scorer, num_weights, weight_range, max_weights=1e5):
    """`ensemble.brute_force_finder` on a scorer: the same tuple list, both forms of every tuple scored in one call each, the first
    maximum in the order "tuple-major, on_logits True then False".  Like `find_ensemble`'s evaluation function (the reference fills
    its input in place), only the very first evaluation -- tuple 0 on logits -- masks the missing entries; every later one scores
    the predictions filled with 0.5.  That one candidate is a call of its own when an entry is missing."""
    tuples = weight_tuples(num_weights, weight_range, max_weights)
    w = np.asarray(tuples, dtype=np.float64).reshape(len(tuples), num_weights)
    both = np.stack([scorer.counts(w, True, masked=False), scorer.counts(w, False, masked=False)], axis=1)
    if scorer.any_missing:
        both[0, 0] = scorer.counts(w[:1], True, masked=True)[0]
    k = int(np.argmax(both.reshape(-1)))                             # numpy's argmax is the first maximum
    best = int(both.reshape(-1)[k])
    score = best / float(scorer.denominator) if scorer.denominator else 0.0
    return score, {'weights': tuples[k // 2], 'on_logits': k % 2 == 0}


def ea_initial_population(rng, num_weights, individual_scores, population_size, min_weight=0.0, max_weight=4.0):
    """[population_size, num_weights]: every individual is, by a coin flip, gauss(1, 0.3) per gene or gauss(e_m / sum(e) * M, 0.3)
    with e = (s - min + 0.01) / (max - min) of the individual scores; clipped to the weight range.  With all individual scores
    equal (the reference divides by zero there) every individual takes the first form."""
    s = np.asarray(individual_scores, dtype=np.float64)
    pop = rng.normal(1.0, 0.3, size=(population_size, num_weights))
    span = float(s.max() - s.min())
    if span > 0.0:
        e = (s - s.min() + 0.01) / span
        informed = rng.random(population_size) <= 0.5
        pop[informed] = rng.normal(e / e.sum() * num_weights, 0.3, size=(population_size, num_weights))[informed]
    return np.clip(pop, min_weight, max_weight)


def _tournament(rng, fitness, k, size=3):
    """k winners of tournaments among `size` uniformly drawn individuals (the first of equal aspirants wins)"""
    aspirants = rng.integers(0, fitness.size, size=(k, size))
    return aspirants[np.arange(k), np.argmax(fitness[aspirants], axis=1)]


def _vary(rng, parents, min_weight, max_weight, cxpb=0.5, indpb=0.5, mutpb=0.9):
    """varAnd: neighbouring pairs mate by uniform crossover with probability cxpb, then every individual mutates with probability
    mutpb: with probability 0.2 a rescale about 1 by U(0.5, 2), otherwise Gaussian noise of sigma ~ U(0.02, 0.2) on each gene with
    probability 0.8; then the clip to the weight range, and genes below 0.2 drop to 0 with probability 0.5."""
    off = parents.copy()
    n, M = off.shape
    pairs = n // 2
    swap = (rng.random(pairs) < cxpb)[:, None] & (rng.random((pairs, M)) < indpb)
    a, b = off[0:2 * pairs:2].copy(), off[1:2 * pairs:2].copy()
    off[0:2 * pairs:2] = np.where(swap, b, a)
    off[1:2 * pairs:2] = np.where(swap, a, b)
    mutate = rng.random(n) < mutpb
    rescale = rng.random(n) < 0.2
    factor = rng.uniform(0.5, 2.0, size=n)
    sigma = rng.uniform(0.02, 0.2, size=n)
    noise = rng.normal(0.0, 1.0, size=(n, M)) * sigma[:, None] * (rng.random((n, M)) < 0.8)
    new = np.where(rescale[:, None], (off - 1.0) * factor[:, None] + 1.0, off + noise)
    new = np.clip(new, min_weight, max_weight)
    new[(new < 0.2) & (rng.random((n, M)) < 0.5)] = 0.0
    return np.where(mutate[:, None], new, off)


def ea_ensemble_finder(scorer, num_weights, individual_scores, population_size=512, min_weight=0.0, max_weight=4.0,
                       num_generations=100, seed=42, trace=False, masked=True):
    """Evolutionary search for the weights on logits (utils/ensemble.py:206-272): tournament selection of size 3, varAnd with uniform
    crossover and the reference's mutation (`_vary`), selection from population plus offspring, a hall of fame of one, a fresh
    population after 50 generations without improvement; on_logits = True throughout.  Returns (best score, {'weights', 'on_logits'}),
    with trace=True also the hall of fame's count after the initial population and after every generation.

    The reference builds this on `deap` and Python's global `random`.  `deap` is not available to this project, so nothing here is
    pinned against it: the operators are restated on a seeded `numpy.random.Generator`, and the tests pin properties instead (same
    seed, same result; weights inside the range; a best count that never decreases and starts at the initial population's best).
    Differences on purpose: the initial population is scored before the first selection (the reference selects on individuals
    without a fitness), the hall of fame sees every scored individual (the reference shows it the survivors only), and equal
    individual scores do not divide by zero.  One scorer call per generation, plus one for a fresh population."""
    if num_weights != scorer.M:
        raise ValueError('num_weights = %d, but the scorer holds %d models' % (num_weights, scorer.M))
    rng = np.random.default_rng(seed)
    fresh = lambda: ea_initial_population(rng, num_weights, individual_scores, population_size, min_weight, max_weight)
    population = fresh()
    fitness = scorer.counts(population, True, masked)
    k = int(np.argmax(fitness))
    best_count, best_weights, best_gen = int(fitness[k]), population[k].copy(), 0
    history = [best_count]
    for gen in range(num_generations):
        offspring = _vary(rng, population[_tournament(rng, fitness, population_size)], min_weight, max_weight)
        pool = np.concatenate([population, offspring])
        pool_fitness = np.concatenate([fitness, scorer.counts(offspring, True, masked)])
        k = int(np.argmax(pool_fitness))
        keep = _tournament(rng, pool_fitness, population_size)
        population, fitness = pool[keep], pool_fitness[keep]
        if int(pool_fitness[k]) > best_count:
            best_count, best_weights, best_gen = int(pool_fitness[k]), pool[k].copy(), gen
        elif gen - best_gen >= 50:
            logger.info('[EA search] Reinitialize population')
            population = fresh()
            fitness = scorer.counts(population, True, masked)
            best_gen = gen
        history.append(best_count)
        if (gen + 1) % 20 == 0:
            logger.info('[EA search] Finished %i generations, current max score: %4.2f%%'
                        % (gen + 1, 100.0 * best_count / max(scorer.denominator, 1)))
    score = best_count / float(scorer.denominator) if scorer.denominator else 0.0
    config = {'weights': [float(v) for v in best_weights], 'on_logits': True}
    return (score, config, np.asarray(history, dtype=np.int64)) if trace else (score, config)
