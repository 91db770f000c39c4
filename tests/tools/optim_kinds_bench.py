"""What the fused Adamax / SGD steps cost against torch's update on the flat buffers (trainer.TorchOptimizerStep), same process,
same GPU: the training step of bench.py's flagship shapes (UNITER-base, batch 16, 128 text tokens, 36 regions x 2048-d; BASELINE
configs[1]) in the fp32x3 and bf16 modes with `get_optimizer(.., fused=True)` and `fused=False` in alternating passes behind a
warm-up, and the optimizer launch alone (bytes per parameter and TB/s, accounted as bench.py's optimizer_alone does).

    python tests/tools/optim_kinds_bench.py [--steps 20] [--warmup 10] [--passes 2] [--out FILE]

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
    from meme_challenge_amd.trainer import TrainStep, get_optimizer, get_scheduler
    from meme_challenge_amd.utils import make_synthetic_batch
    dev = torch.device('cuda', 0)
    cfg = UniterConfig.from_dict(BASE)
    batch = make_synthetic_batch(16, 128, 36, seed=1234, device=dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def setup(optname, precision, fused):
        torch.manual_seed(0)
        model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).to(dev).train()
        enc = model.uniter_model
        enc.precision = precision
        enc.set_dropout_seed(1234, 0)
        config = dict(optimizer=optname, lr=3e-5, beta1=0.9, beta2=0.999, weight_decay=1e-3, gradient_accumulation=1, max_grad_norm=5,
                      pos_wt=1.8, loss_func='bce_logits', scheduler='warmup_cosine', warmup_steps=500, max_epoch=30)
        opt = get_optimizer(model, config, fused=fused)
        if hasattr(opt, 'overlap_encoder'):
            opt.overlap_encoder = enc                     # as train_template.init_optimizer drives the fused step
        step = TrainStep(model, opt, get_scheduler(opt, config, steps_per_epoch=1000), config)
        return model, opt, (lambda: step.train_iter(batch, iters=0))

    def timed(one_step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            one_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def launch_alone(opt, model):
        """bench.py's optimizer_alone: 10 launches behind 2 warm-ups, every chunk on the update path, gradients already zero"""
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
        # read p, g, state + write p, state: 28 B per parameter with two state buffers, 20 B with one (SGD); + the mirror
        per = (28 if opt.exp_avg_sq is not None else 20) + mirror_b
        return ms, per, per * st.numel / (ms * 1e-3) / 1e12

    say('optimizer kinds on %s, UNITER-base B=16 T=128 R=36, %d warm-up + %d passes x %d steps per path'
        % (torch.cuda.get_device_name(0), args.warmup, args.passes, args.steps))
    for precision in ('fp32x3', 'bf16'):
        for optname in ('sgd', 'adamax', 'adam'):
            paths = {}
            for fused in ((True,) if optname == 'adam' else (True, False)):
                paths[fused] = setup(optname, precision, fused)
                timed(paths[fused][2], args.warmup)
            ms = {k: [] for k in paths}
            for _ in range(args.passes):
                for fused in paths:
                    ms[fused].append(timed(paths[fused][2], args.steps))
            for fused in paths:
                say('%-6s %-6s step %-5s ms per pass %s  mean %.3f' % (precision, optname, 'fused' if fused else 'torch',
                                                                      ' '.join('%.3f' % x for x in ms[fused]), sum(ms[fused]) / len(ms[fused])))
            if False in paths:
                f, t = sum(ms[True]) / len(ms[True]), sum(ms[False]) / len(ms[False])
                say('%-6s %-6s fused / torch = %.3f (%+.3f ms per step)' % (precision, optname, f / t, f - t))
            model, opt, _ = paths[True]
            o_ms, per, tbs = launch_alone(opt, model)
            say('%-6s %-6s launch alone %.4f ms, %d B per parameter, %.3f TB/s' % (precision, optname, o_ms, per, tbs))
            del paths, model, opt
            gc.collect()
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
