"""What does a bit-reproducible training step (UniterModel.deterministic) cost?  Times whole training steps -- forward, backward, clip,
fused Adam step, as bench.py's fine-tuning workload drives them -- with the switch off (the code every earlier commit runs) and on,
on one GPU in one process:

    python tests/tools/step_det_bench.py [--reps 5] [--steps 50]

Shapes: BASELINE configs[1] (B = 16, 128 tokens, 36 regions, UNITER-base) padded in fp32x3 and bf16, and the ragged batch of
`bench.py --ragged --packed` (the same lengths, token packing on) in fp32x3.  Two models per case, one with the switch off and one with
it on, are stepped in turns -- off, on, off, on ... -- `--steps` steps per turn between two device events; the median turn of each is
printed in milliseconds per step with its spread, and what the deterministic plan reports as covered.  Only time is read."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import numpy as np
import torch

from bench import BASE
from meme_challenge_amd import _lib
from meme_challenge_amd.meme_uniter import MemeUniter
from meme_challenge_amd.model import UniterConfig, UniterModel
from meme_challenge_amd.trainer import FusedAdam, TrainStep, get_scheduler
from meme_challenge_amd.utils import make_synthetic_batch

B, T, R = 16, 128, 36
CONFIG = dict(optimizer='adam', lr=3e-5, beta1=0.9, beta2=0.999, weight_decay=1e-3, gradient_accumulation=1, max_grad_norm=5,
              pos_wt=1.8, loss_func='bce_logits', scheduler='warmup_cosine', warmup_steps=500, max_epoch=30)      # bench.py's


def make(det, packed, precision):
    lens = {}
    if packed:
        rng = np.random.Generator(np.random.PCG64(4321))                          # bench.py --ragged
        lens = dict(txt_lens=[int(x) for x in rng.integers(8, T + 1, size=B)], num_bbs=[int(x) for x in rng.integers(10, R + 1, size=B)])
    batch = make_synthetic_batch(B, T, R, seed=1234, device='cuda', **lens)
    if packed:
        batch['seq_lens'] = [a + c for a, c in zip(lens['txt_lens'], lens['num_bbs'])]
    torch.manual_seed(0)
    cfg = UniterConfig.from_dict(BASE)
    model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).cuda().train()
    enc = model.uniter_model
    enc.precision, enc.pack_padded, enc.deterministic = precision, packed, det
    enc.set_dropout_seed(1234, 0)
    opt = FusedAdam(model, lr=CONFIG['lr'], weight_decay=CONFIG['weight_decay'])
    step = TrainStep(model, opt, get_scheduler(opt, CONFIG, steps_per_epoch=1000), CONFIG)
    return model, opt, step, batch


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5, help='turns per variant')
    ap.add_argument('--steps', type=int, default=50, help='training steps per turn')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    print('device: %s; %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode()))
    for precision, packed in (('fp32x3', False), ('bf16', False), ('fp32x3', True)):
        runs = {det: make(det, packed, precision) for det in (False, True)}
        times = {False: [], True: []}
        for det in (False, True):                        # warm-up: plans, workspaces, the side stream
            for it in range(5):
                runs[det][2].train_iter(runs[det][3], iters=0)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for det in (False, True):
                _, opt, step, batch = runs[det]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.steps):
                    step.train_iter(batch, iters=0)
                opt.join()
                t1.record()
                t1.synchronize()
                times[det].append(t0.elapsed_time(t1) / args.steps)
        cov = runs[True][0].uniter_model.deterministic_coverage
        name = 'ragged, packed (bench.py --ragged --packed)' if packed else 'padded (configs[1])'
        off, on = statistics.median(times[False]), statistics.median(times[True])
        print('%s B=%d T=%d R=%d H=%d %s: training step  off %.3f ms (min %.3f max %.3f)  on %.3f ms (min %.3f max %.3f)  on / off %+.2f %%  '
              'coverage %d of 15' % (name, B, T, R, BASE['hidden_size'], precision, off, min(times[False]), max(times[False]), on,
                                     min(times[True]), max(times[True]), 100.0 * (on / off - 1.0), cov), flush=True)
        del runs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
