"""What does capturing the gradient-weighted attention cost?  One GPU, one process, the variants in alternating turns:

    python tests/tools/attn_grad_bench.py [--reps 7] [--iters 20] [--precisions fp32x3,bf16]

At BASELINE configs[2]'s shapes (B = 16, 128 tokens + 36 regions: L = 164, 12 layers, 12 heads):
1. a saliency-style pass of MemeUniter -- an eval-mode forward with gradients and the backward of the logits' sum, img_feat as a
   differentiable input -- with `UniterModel.output_attention_grads` None, 'relu_mean' and 'all', eager, `--iters` passes per turn
   between two device events;
2. uniter_attn_grad alone on one layer's query|key|value buffer and context gradient (fp32 and bf16 qkv; per head and reduced, with
   the head sums), and uniter_attn_relevance alone over 12 layers' maps.

Beside each kernel time two floors: bytes / 8 TB/s -- the 'all' store is B nh L L 4 = 20.7 MB per layer, the reduced store 1.7 MB, the
qkv read 36 MB in fp32, the context gradient 8 MB -- and FLOP / 157 TFLOP/s of fp32 vector arithmetic: two passes over the keys for q.k
and one for dO.v, 2 * 64 * 3 B nh L L = 1.98 GFLOP per layer.  Only time is read; nothing is asserted."""
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
from meme_challenge_amd.utils import make_synthetic_batch

B, T, R = 16, 128, 36
L, NL, NH = T + R, BASE['num_hidden_layers'], BASE['num_attention_heads']
HBM = 8e12        # bytes / s
VALU = 157e12     # fp32 FLOP / s on the vector pipe


def new_model(precision):
    torch.manual_seed(0)
    cfg = UniterConfig.from_dict(BASE)
    model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).cuda().eval()
    model.uniter_model.precision = precision
    return model


def turns(variants, run, reps):
    """{variant: [us per iteration, one per turn]}; every variant runs once unmeasured first"""
    stream = torch.cuda.current_stream()
    times = {v: [] for v in variants}
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


def report(what, times, floors=None):
    for v, t in times.items():
        floor = ''
        if floors and floors.get(v) is not None:
            by, fl = floors[v]
            floor = '  floors: bytes %.1f us, FLOP %.1f us (%.1f x the larger)' % (by, fl, statistics.median(t) / max(by, fl))
        print('%s %-14s %9.1f us (min %.1f max %.1f)%s' % (what, v, statistics.median(t), min(t), max(t), floor), flush=True)
    if 'off' in times:
        off = statistics.median(times['off'])
        for v, t in times.items():
            if v != 'off':
                print('%s %-14s %+9.1f us over the capture off' % (what, v, statistics.median(t) - off), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=7, help='turns per variant')
    ap.add_argument('--iters', type=int, default=20, help='passes / launches per turn')
    ap.add_argument('--precisions', default='fp32x3,bf16')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    lib = _lib.lib()
    print('device: %s; %s; library %s' % (torch.cuda.get_device_name(0), lib.uniter_build_info().decode(), os.path.basename(_lib.LIB_PATH)))
    print('B %d L %d layers %d heads %d' % (B, L, NL, NH))
    batch = make_synthetic_batch(B, T, R, seed=1234, device='cuda')
    kw = dict(img_feat=batch['img_feat'].detach().requires_grad_(True), img_pos_feat=batch['img_pos_feat'], input_ids=batch['input_ids'],
              position_ids=batch['position_ids'], attention_mask=batch['attn_mask'], gather_index=batch['gather_index'],
              output_all_encoded_layers=False)
    variants = {'off': None, 'relu_mean': 'relu_mean', 'all': 'all'}
    for precision in args.precisions.split(','):
        model = new_model(precision)

        def saliency(v, warm):
            n = 3 if warm else args.iters
            model.uniter_model.output_attention_grads = variants[v]
            for _ in range(n):
                kw['img_feat'].grad = None
                model(**kw).sum().backward()
            return n
        report('forward + backward %-7s' % precision, turns(list(variants), saliency, args.reps))
        del model

    # ---- the kernels alone ----
    H = NH * 64
    qkv = torch.randn(B * L, 3 * H, device='cuda')
    ops = {'f32': qkv, 'b16': qkv.bfloat16()}
    dctx = torch.randn(B * L, H, device='cuda')
    mask = torch.ones(B, L, device='cuda')
    outs = {0: torch.empty(B, NH, L, L, device='cuda'), 1: torch.empty(B, L, L, device='cuda')}
    sums = torch.empty(B, NH, device='cuda')
    nws = lib.uniter_attn_grad_ws_bytes(B, L, NH)
    ws = torch.empty((nws + 3) // 4, device='cuda')
    kinds = [(o, red) for o in ops for red in (0, 1)]
    name = {(o, red): '%s %s' % (o, 'relu_mean' if red else 'all') for o, red in kinds}

    def grad(kind, warm):
        o, red = kind
        n = 3 if warm else args.iters
        for _ in range(n):
            _lib.check(lib.uniter_attn_grad(_lib.ptr(ops[o]), int(o == 'b16'), _lib.ptr(mask), None, _lib.ptr(dctx), 1, 0, _lib.ptr(outs[red]),
                                            _lib.ptr(sums), _lib.ptr(ws), nws, B, L, NH, red, _lib.cur_stream()), 'uniter_attn_grad')
        return n
    t = turns(kinds, grad, args.reps)
    flop = 2.0 * 64 * 3 * B * NH * L * L
    report('uniter_attn_grad, one layer', {name[k]: t[k] for k in kinds},
           {name[(o, red)]: ((outs[red].numel() * 4 + ops[o].numel() * ops[o].element_size() + dctx.numel() * 4) / HBM * 1e6, flop / VALU * 1e6)
            for o, red in kinds})

    maps = torch.rand(NL, B, L, L, device='cuda') / L
    rel, tmp = torch.empty(B, L, L, device='cuda'), torch.empty(B, L, L, device='cuda')

    def relevance(_, warm):
        n = 3 if warm else args.iters
        for _ in range(n):
            _lib.check(lib.uniter_attn_relevance(_lib.ptr(maps), _lib.ptr(rel), _lib.ptr(tmp), NL, B, L, _lib.cur_stream()),
                       'uniter_attn_relevance')
        return n
    report('uniter_attn_relevance', {'12 layers': turns(['x'], relevance, args.reps)['x']},
           {'12 layers': ((maps.numel() * 4 + 2 * (NL - 1) * rel.numel() * 4 + rel.numel() * 4) / HBM * 1e6,
                          2.0 * (NL - 1) * B * L * L * L / VALU * 1e6)})


if __name__ == '__main__':
    main()
