"""What per-group hyper-parameters and a frozen prefix cost or save, one process, one GPU.

(i)  The optimizer launch alone at UNITER-base's size (109.9 M parameters, AdamW, the three-piece mirror): uniter_optim_step against
     uniter_optim_step_groups with 1, 2 and 4 groups (the groups interleaved tensor-sized, 1.5 M elements each), the launches
     interleaved round by round behind a warm-up; median and the min .. max spread of each, in microseconds (HIP events around one
     launch, the L2s / MALL cannot hold the 3.1 GB a launch moves).
(ii) The training step of BASELINE configs[1] (UNITER-base, batch 16, 128 tokens, 36 regions, fp32x3) unfrozen and with
     freeze_prefix(6), alternating passes of --steps steps behind a warm-up; wall-clock per step, median over the passes.

    python tests/tools/optim_groups_bench.py [--reps 40] [--steps 20] [--warmup 10] [--passes 3] [--out FILE]

Prints one line per measurement; --out also writes them to FILE.  No pass / fail threshold: the numbers are a statement."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASE = dict(attention_probs_dropout_prob=0.1, hidden_act='gelu', hidden_dropout_prob=0.1, hidden_size=768, initializer_range=0.02,
            intermediate_size=3072, max_position_embeddings=512, num_attention_heads=12, num_hidden_layers=12, type_vocab_size=2,
            vocab_size=28996)
N = 109_900_032          # UNITER-base's parameters rounded to whole chunks


def kernel_times(args, say):
    import torch
    from meme_challenge_amd import _lib
    lib = _lib.lib()
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    p, g = torch.randn(N, device=dev) * 0.05, torch.randn(N, device=dev) * 1e-3
    m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    mirror = torch.empty(3 * N, dtype=torch.bfloat16, device=dev)
    sumsq = torch.ones(1, dtype=torch.float64, device=dev)
    chunks = N // 64
    tensor = torch.arange(chunks, device=dev) // 24576          # "tensors" of 1.5 M elements
    hyper = [(3e-5, 0.9, 0.999, 1e-8, 1e-3), (3e-4, 0.9, 0.999, 1e-8, 0.0), (1e-4, 0.8, 0.99, 1e-6, 1e-2), (3e-5, 0.9, 0.98, 1e-8, 1e-3)]
    st = _lib.cur_stream()
    head = (ptr(p), ptr(g), None, ptr(m), ptr(v))
    tail = (ptr(mirror), N, None, 0, 0, st)

    def flags_of(k):
        return ((tensor % k) << 3 | 2).to(torch.uint8).contiguous()

    launches = {}
    f0 = flags_of(1)
    launches['uniter_optim_step'] = lambda: lib.uniter_optim_step(1, *head, ptr(f0), N, ptr(sumsq), 1.0, 5.0, *hyper[0], 1, 1, 0, *tail)
    keep = [f0]
    for k in (1, 2, 4):
        fk, table = flags_of(k), (_lib.OptimGroupC * k)(*[_lib.OptimGroupC(*h) for h in hyper[:k]])
        keep += [fk, table]
        launches['groups, n_groups = %d' % k] = (lambda fk=fk, table=table, k=k: lib.uniter_optim_step_groups(
            1, *head, ptr(fk), N, ptr(sumsq), 1.0, 5.0, C.cast(table, C.c_void_p), k, 1, 0, *tail))
    times = {name: [] for name in launches}
    for rep in range(args.warmup + args.reps):
        for name, launch in launches.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(launch(), name)
            b.record()
            b.synchronize()
            if rep >= args.warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    base = statistics.median(times['uniter_optim_step'])
    for name, t in times.items():
        say('(i) %-28s median %7.1f us  min %7.1f  max %7.1f  (%+.2f %% of uniter_optim_step)  %d launches'
            % (name, statistics.median(t), min(t), max(t), 100.0 * (statistics.median(t) / base - 1.0), len(t)))


def ptr(t):
    return C.c_void_p(t.data_ptr())


def step_times(args, say):
    import torch
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.trainer import TrainStep, get_optimizer, get_scheduler
    from meme_challenge_amd.utils import make_synthetic_batch
    dev = torch.device('cuda', 0)
    cfg = UniterConfig.from_dict(BASE)
    batch = make_synthetic_batch(16, 128, 36, seed=1234, device=dev)
    config = dict(optimizer='adamw', lr=3e-5, beta1=0.9, beta2=0.999, weight_decay=1e-3, gradient_accumulation=1, max_grad_norm=5,
                  pos_wt=1.8, loss_func='bce_logits', scheduler='warmup_cosine', warmup_steps=500, max_epoch=30)

    def setup(floor):
        torch.manual_seed(0)
        model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).to(dev).train()
        enc = model.uniter_model
        enc.precision = 'fp32x3'
        enc.set_dropout_seed(1234, 0)
        if floor:
            assert enc.freeze_prefix(floor) == floor
        opt = get_optimizer(model, config)
        opt.overlap_encoder = enc
        step = TrainStep(model, opt, get_scheduler(opt, config, steps_per_epoch=1000), config)
        return model, opt, (lambda: step.train_iter(batch, iters=0))

    def timed(one_step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            one_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    runs = {0: setup(0), 6: setup(6)}
    for floor, (_, _, one) in runs.items():
        timed(one, args.warmup)
    ms = {0: [], 6: []}
    for _ in range(args.passes):
        for floor, (_, _, one) in runs.items():
            ms[floor].append(timed(one, args.steps))
    for floor, t in ms.items():
        say('(ii) step, %-18s median %.3f ms  passes %s' % ('freeze_prefix(6)' if floor else 'nothing frozen', statistics.median(t),
                                                          ' '.join('%.3f' % x for x in t)))
    say('(ii) saving %.3f ms per step' % (statistics.median(ms[0]) - statistics.median(ms[6])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    kernel_times(args, say)
    step_times(args, say)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
