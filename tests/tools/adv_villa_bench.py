"""What does a VILLA micro-batch cost beside the forward / backward passes it is made of?  One measurement on one GPU in one
process, the variants in alternating turns (the manner of tests/tools/input_grads_bench.py):

    python tests/tools/adv_villa_bench.py [--reps 7] [--steps 20] [--precision fp32x3] [--norm-type l2] [--modality both] [--kl-weight 1.0]

One optimizer step of trainer.TrainStep fed by three forward / backward passes at BASELINE configs[1] (B = 16, 128 tokens, 36
regions, H = 768): VILLA with adv_steps = 2 -- the clean pass, two perturbed passes with one uniter_bce_kl_logits each, the first of
them returning the perturbations' gradients, one ascent step per perturbation between the two -- against three plain micro-batches
with gradient_accumulation = 3.  Eager, `--steps` steps per turn between two device events.  With --modality each the VILLA
micro-batch has two rounds, five passes, and is set against five plain micro-batches.  Only time is read; nothing is asserted."""
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
K = 2


class _NoSchedule(object):
    def step(self):
        pass


def new_step(args, villa, passes):
    torch.manual_seed(0)
    cfg = UniterConfig.from_dict(BASE)
    model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).cuda().train()
    model.uniter_model.precision = args.precision
    model.uniter_model.set_dropout_seed(1234, 0)
    config = dict(optimizer='adam', lr=1e-5, beta1=0.9, beta2=0.999, weight_decay=1e-3, max_grad_norm=5, pos_wt=1.8, loss_func='bce_logits',
                  seed=1, gradient_accumulation=1 if villa else passes)
    if villa:
        config.update(adv_algo='villa', adv_steps=K, adv_lr=0.1, adv_max_norm=1.0, adv_init_mag=0.0, adv_modality=args.modality,
                      adv_kl_weight=args.kl_weight, adv_norm_type=args.norm_type)
    return TrainStep(model, get_optimizer(model, config), _NoSchedule(), config)


def one_step(step, batch, villa, passes):
    if villa:
        step.train_iter(batch, iters=0)
    else:
        for i in range(1, passes + 1):            # passes - 1 accumulate, the last accumulates and steps
            step.train_iter(batch, iters=i)


def turns(variants, run, reps, stream):
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=7, help='turns per variant')
    ap.add_argument('--steps', type=int, default=20, help='optimizer steps per turn')
    ap.add_argument('--precision', default='fp32x3')
    ap.add_argument('--norm-type', default='l2', choices=('l2', 'linf'))
    ap.add_argument('--modality', default='both', choices=('both', 'txt', 'img', 'each'))
    ap.add_argument('--kl-weight', type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    print('device: %s; %s; library %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode(), os.path.basename(_lib.LIB_PATH)))
    passes = 1 + K * (2 if args.modality == 'each' else 1)
    stream = torch.cuda.Stream()
    batch = make_synthetic_batch(B, T, R, seed=1234, device='cuda')
    variants = (False, True)
    steps = {v: new_step(args, v, passes) for v in variants}

    def train(v, warm):
        n = 3 if warm else args.steps
        for _ in range(n):
            one_step(steps[v], batch, v, passes)
        return n
    times = turns(variants, train, args.reps, stream)
    names = {False: '%d accumulation micro-batches' % passes, True: 'VILLA K = %d (%s, %s, kl_weight %g)' % (K, args.modality, args.norm_type, args.kl_weight)}
    med = {v: statistics.median(t) for v, t in times.items()}
    parts = ['%s %.1f us (min %.1f max %.1f)' % (names[v], med[v], min(times[v]), max(times[v])) for v in variants]
    parts.append('VILLA - plain %+.1f us (%+.2f %%)' % (med[True] - med[False], 100.0 * (med[True] - med[False]) / med[False]))
    print('B=%d T=%d R=%d H=%d %s, one optimizer step behind %d forward / backward passes: %s'
          % (B, T, R, BASE['hidden_size'], args.precision, passes, '  '.join(parts)), flush=True)


if __name__ == '__main__':
    main()
