"""What the averaged weights cost inside the fused optimizer step (`ema_decay`, uniter_optim_step_avg) against no averaging and
against the separate pass the fusion replaces, same process, same GPU:

(i)  the optimizer launch alone at UNITER-base's 109.9 M parameters for Adam, Adamax and SGD, without and with the average: ms,
     bytes per parameter and TB/s (accounted as tests/tools/optim_kinds_bench.py does, + 8 B per parameter for the average);
(ii) the training step of bench.py's flagship shapes (UNITER-base, batch 16, 128 text tokens, 36 regions x 2048-d; BASELINE
     configs[1]) in the fp32x3 and bf16 modes, three ways in alternating passes behind a warm-up: averaging off, fused
     (`ema_decay`), and separate -- averaging off, then `join()` and `avg.lerp_(p, w)` behind every step, which is what a trainer
     without the fused form has to do (12 B per parameter in front of the next forward pass, and no overlap with it).

    python tests/tools/optim_ema_bench.py [--steps 20] [--warmup 10] [--passes 2] [--out FILE]

Prints one line per measurement; --out also writes them to FILE.  No pass / fail threshold: the numbers are a statement."""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASE = dict(attention_probs_dropout_prob=0.1, hidden_act='gelu', hidden_dropout_prob=0.1, hidden_size=768, initializer_range=0.02,
            intermediate_size=3072, max_position_embeddings=512, num_attention_heads=12, num_hidden_layers=12, type_vocab_size=2,
            vocab_size=28996)
DECAY = 0.999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.trainer import TrainStep, ema_weight, get_optimizer, get_scheduler
    from meme_challenge_amd.utils import make_synthetic_batch
    dev = torch.device('cuda', 0)
    cfg = UniterConfig.from_dict(BASE)
    batch = make_synthetic_batch(16, 128, 36, seed=1234, device=dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def setup(optname, precision, way):
        """way: 'off' | 'fused' | 'separate'"""
        torch.manual_seed(0)
        model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).to(dev).train()
        enc = model.uniter_model
        enc.precision = precision
        enc.set_dropout_seed(1234, 0)
        config = dict(optimizer=optname, lr=3e-5, beta1=0.9, beta2=0.999, weight_decay=1e-3, gradient_accumulation=1, max_grad_norm=5,
                      pos_wt=1.8, loss_func='bce_logits', scheduler='warmup_cosine', warmup_steps=500, max_epoch=30,
                      ema_decay=DECAY if way == 'fused' else 0)
        opt = get_optimizer(model, config)
        opt.overlap_encoder = enc                     # as train_template.init_optimizer drives the fused step
        step = TrainStep(model, opt, get_scheduler(opt, config, steps_per_epoch=1000), config)
        if way != 'separate':
            return model, opt, (lambda: step.train_iter(batch, iters=0))
        st = model.param_store()
        avg, count = st.flat_params.detach().clone(), [0]

        def one():
            step.train_iter(batch, iters=0)
            opt.join()
            with torch.no_grad():
                avg.lerp_(st.flat_params, ema_weight(DECAY, count[0]))
            count[0] += 1
        return model, opt, one

    def timed(one_step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            one_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def launch_alone(opt, model):
        """optim_kinds_bench's: 10 launches behind 2 warm-ups, every chunk on the update path, gradients already zero"""
        opt.join()
        torch.cuda.synchronize()
        st = model.param_store()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        saved, opt.overlap_encoder = opt.overlap_encoder, None
        for it in range(12):
            if it == 2:
                e0.record()
            st.touch(st.names)
            opt.step(grad_scale=1.0, max_grad_norm=0.0, zero_grads=True)
        e1.record()
        torch.cuda.synchronize()
        opt.overlap_encoder = saved
        ms = e0.elapsed_time(e1) / 10
        mirror_b = 2 * getattr(st, 'mirror_pieces', 1) if getattr(st, 'mirror', None) is not None else 0
        per = (28 if opt.exp_avg_sq is not None else 20) + mirror_b + (8 if opt.avg is not None else 0)
        return ms, per, per * st.numel / (ms * 1e-3) / 1e12

    say('averaged weights in the fused step on %s, UNITER-base B=16 T=128 R=36, %d warm-up + %d passes x %d steps per path'
        % (torch.cuda.get_device_name(0), args.warmup, args.passes, args.steps))
    say('(i) the launch alone (fp32 mode: no weight mirror)')
    for optname in ('adam', 'adamax', 'sgd'):
        for way in ('off', 'fused'):
            model, opt, one = setup(optname, 'fp32', way)
            one()                                         # (a forward / backward: the store's gradients exist)
            ms, per, tbs = launch_alone(opt, model)
            say('%-6s averaging %-5s launch alone %.4f ms, %d B per parameter, %.3f TB/s (%d parameters)'
                % (optname, way, ms, per, tbs, model.param_store().numel))
            del model, opt, one
            gc.collect()
            torch.cuda.empty_cache()
    say('(ii) the training step, adam')
    for precision in ('fp32x3', 'bf16'):
        paths = {}
        for way in ('off', 'fused', 'separate'):
            paths[way] = setup('adam', precision, way)
            timed(paths[way][2], args.warmup)
        ms = {k: [] for k in paths}
        for _ in range(args.passes):
            for way in paths:
                ms[way].append(timed(paths[way][2], args.steps))
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        for way in paths:
            say('%-6s step, averaging %-8s ms per pass %s  mean %.3f' % (precision, way, ' '.join('%.3f' % x for x in ms[way]), mean[way]))
        say('%-6s fused - off = %+.3f ms, separate - off = %+.3f ms, fused %s the separate pass'
            % (precision, mean['fused'] - mean['off'], mean['separate'] - mean['off'],
               'beats' if mean['fused'] < mean['separate'] else 'DOES NOT beat'))
        del paths
        gc.collect()
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
