"""What does the pairwise AUROC term cost?  One measurement on one GPU in one process, the variants in alternating turns (the manner
of tests/tools/adv_villa_bench.py):

    python tests/tools/auc_loss_bench.py [--reps 7] [--steps 20] [--launches 200] [--precision fp32x3] [--no-term]

1. The loss launch alone at B = 16: uniter_bce_logits against uniter_bce_auc_logits (logistic, with a push) without a bank and with a
   full bank of 1024 and of 4096 scores; `--launches` launches per turn between two device events, microseconds per launch.
2. One optimizer step of trainer.TrainStep at BASELINE configs[1] (B = 16, 128 tokens, 36 regions, H = 768), plain against
   auc_weight = 0.5 with auc_bank = 1024; `--steps` steps per turn.

--no-term times the plain variants only: the same tool on a library built from another commit (UNITER_LIB_VARIANT, with
UNITER_DEV_PARTIAL_LIB=1 where it lacks the new symbol) gives that commit's own figures and their spread.  Each line: the median
and min .. max over the turns.  Only time is read; nothing is asserted."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import torch

from bench import BASE
from meme_challenge_amd import _lib
from meme_challenge_amd.meme_uniter import MemeUniter
from meme_challenge_amd.model import UniterConfig, UniterModel
from meme_challenge_amd.trainer import TrainStep, get_optimizer
from meme_challenge_amd.utils import make_synthetic_batch

B, T, R = 16, 128, 36
BANKS = (0, 1024, 4096)
AUC = dict(auc_weight=0.5, auc_bank=1024, auc_surrogate='logistic')


class _NoSchedule(object):
    def step(self):
        pass


def turns(variants, run, reps, stream):
    """run(v, warm) -> the number of units it ran; -> v: [microseconds per unit] over the turns"""
    times = {v: [] for v in variants}
    with torch.cuda.stream(stream):
        for v in variants:
            run(v, True)
        for _ in range(reps):
            for v in variants:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                n = run(v, False)
                t1.record(stream)
                t1.synchronize()
                times[v].append(t0.elapsed_time(t1) * 1e3 / n)
    return times


def report(head, names, times):
    for v, t in times.items():
        print('%s %-44s median %9.2f us  (min %9.2f .. max %9.2f, %d turns)' % (head, names[v], statistics.median(t), min(t), max(t), len(t)),
              flush=True)


def launch_part(args, stream):
    lib = _lib.lib()
    g = torch.Generator(device='cuda').manual_seed(1)
    z = torch.randn(B, device='cuda', generator=g) * 2
    y = (torch.arange(B, device='cuda') % 3 == 0).long()
    out = dict(loss=torch.empty(3, device='cuda'), probs=torch.empty(B, device='cuda'), dlog=torch.empty(B, device='cuda'),
               n=torch.empty(1, dtype=torch.int32, device='cuda'))
    banks = {}
    for N in (() if args.no_term else BANKS):
        if N:
            banks[N] = (torch.randn(N, device='cuda', generator=g) * 2, (torch.arange(N, device='cuda') % 3 == 0).int(),
                        torch.tensor([0, N], dtype=torch.int32, device='cuda'))
    p = lambda t: t.data_ptr()

    def run(v, warm):
        n = 10 if warm else args.launches
        sp = stream.cuda_stream
        for _ in range(n):
            if v == 'bce':
                rc = lib.uniter_bce_logits(p(z), p(y), 1.8, p(out['loss']), p(out['probs']), p(out['dlog']), 1.0, B, sp)
            else:
                bk = [p(t) for t in banks[v]] if v else [None, None, None]
                rc = lib.uniter_bce_auc_logits(p(z), p(y), 1.8, 0.5, 0, 1.0, *bk, v, 1, p(out['loss']), p(out['n']), p(out['probs']),
                                               p(out['dlog']), 1.0, B, sp)
            _lib.check(rc, 'loss launch')
        return n
    variants = ('bce',) + (() if args.no_term else BANKS)
    names = {'bce': 'uniter_bce_logits'}
    names.update({N: 'uniter_bce_auc_logits, ' + ('bank of %d' % N if N else 'no bank') for N in BANKS})
    report('loss launch, B = %d:' % B, names, turns(variants, run, args.reps, stream))


def new_step(args, term):
    torch.manual_seed(0)
    cfg = UniterConfig.from_dict(BASE)
    model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).cuda().train()
    model.uniter_model.precision = args.precision
    model.uniter_model.set_dropout_seed(1234, 0)
    config = dict(optimizer='adam', lr=1e-5, beta1=0.9, beta2=0.999, weight_decay=1e-3, max_grad_norm=5, pos_wt=1.8, loss_func='bce_logits',
                  seed=1, gradient_accumulation=1, batch_size=B)
    if term:
        config.update(AUC)
    return TrainStep(model, get_optimizer(model, config), _NoSchedule(), config)


def step_part(args, stream):
    batch = make_synthetic_batch(B, T, R, seed=1234, device='cuda')
    variants = (False,) if args.no_term else (False, True)
    steps = {v: new_step(args, v) for v in variants}

    def run(v, warm):
        n = 3 if warm else args.steps
        for _ in range(n):
            steps[v].train_iter(batch, iters=0)
        return n
    times = turns(variants, run, args.reps, stream)
    names = {False: 'plain step (BCE)', True: 'with the term (weight %g, bank %d, %s)' % (AUC['auc_weight'], AUC['auc_bank'], AUC['auc_surrogate'])}
    report('step, B=%d T=%d R=%d H=%d %s:' % (B, T, R, BASE['hidden_size'], args.precision), names, times)
    if not args.no_term:
        a, b = statistics.median(times[False]), statistics.median(times[True])
        print('with the term - plain: %+.1f us (%+.2f %%); the plain step itself spans %.1f us over its turns'
              % (b - a, 100.0 * (b - a) / a, max(times[False]) - min(times[False])), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=7, help='turns per variant')
    ap.add_argument('--steps', type=int, default=20, help='optimizer steps per turn')
    ap.add_argument('--launches', type=int, default=200, help='loss launches per turn')
    ap.add_argument('--precision', default='fp32x3')
    ap.add_argument('--no-term', action='store_true', help='the plain variants only (a library without the new symbol)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    print('device: %s; %s; library %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode(), os.path.basename(_lib.LIB_PATH)))
    stream = torch.cuda.Stream()
    launch_part(args, stream)
    step_part(args, stream)


if __name__ == '__main__':
    main()
