"""What do the input gradients and a FreeLB step cost?  Two measurements on one GPU in one process, the variants in alternating turns:

    python tests/tools/input_grads_bench.py [--reps 7] [--replays 200] [--steps 20] [--precision fp32x3] [--only-off]

1. uniter_model_backward_embed alone, by graph replay (as tests/tools/embed_det_bench.py), without and with the three input
   gradients (img_feat, img_pos_feat, txt_embed_delta) at BASELINE configs[1] (B = 16, 128 tokens, 36 regions, H = 768): the added
   launches are the per-token text gradient (auxiliary stream), the region-feature product d_imgfc @ W_img and the 7-column
   position gradient (main stream).
2. One optimizer step of trainer.TrainStep fed by two forward / backward passes: FreeLB with adv_steps = 2 (the first pass returns the
   perturbations' gradients, one uniter_adv_delta_step each between the passes) against two plain micro-batches with
   gradient_accumulation = 2.  Eager, `--steps` steps per turn between two device events.

--only-off runs the unchanged path alone (part 1 without input gradients, part 2's plain accumulation): with
UNITER_LIB_VARIANT=<name> UNITER_DEV_PARTIAL_LIB=1 it times a library built from another source tree, e.g. the parent commit's
(meme_challenge_amd/build.py, `variant`).  Only time is read; replays add the same gradients onto the buffers again."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import torch

from bench import BASE
from meme_challenge_amd import _lib
from meme_challenge_amd.meme_uniter import MemeUniter
from meme_challenge_amd.model import UniterConfig, UniterModel
from meme_challenge_amd.trainer import TrainStep, bce_with_logits_loss, get_optimizer
from meme_challenge_amd.utils import make_synthetic_batch

B, T, R = 16, 128, 36


def new_model(precision):
    torch.manual_seed(0)
    cfg = UniterConfig.from_dict(BASE)
    model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).cuda().train()
    model.uniter_model.precision = precision
    model.uniter_model.set_dropout_seed(1234, 0)
    return model


def capture(want, precision, stream):
    """one training forward + backward with uniter_model_backward_embed's launches captured; returns (graph, what must stay alive)"""
    batch = make_synthetic_batch(B, T, R, seed=1234, device='cuda')
    model = new_model(precision)
    enc = model.uniter_model
    enc.use_side_stream = False
    alive = [batch, model]
    get_ws = enc._get_ws

    def keep_ws(nbytes, mode):            # the plan's buffers: what the captured launches read
        alive.append(get_ws(nbytes, mode))
        return alive[-1]
    enc._get_ws = keep_ws
    lib = _lib.lib()
    embed = lib.uniter_model_backward_embed
    aux = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    alive.append(aux)

    def captured_embed(handle):
        _lib.check(lib.uniter_model_set_aux_stream(handle, C.c_void_p(aux.cuda_stream)), 'uniter_model_set_aux_stream')
        with torch.cuda.graph(graph, stream=torch.cuda.current_stream()):
            rc = embed(handle)
        return rc
    lib.uniter_model_backward_embed = captured_embed
    kw = dict(img_feat=batch['img_feat'], img_pos_feat=batch['img_pos_feat'], input_ids=batch['input_ids'],
              position_ids=batch['position_ids'], attention_mask=batch['attn_mask'], gather_index=batch['gather_index'],
              output_all_encoded_layers=False)
    if want:
        kw['img_feat'] = batch['img_feat'].clone().requires_grad_(True)
        kw['img_pos_feat'] = batch['img_pos_feat'].clone().requires_grad_(True)
        kw['txt_embed_delta'] = torch.zeros(B, T, BASE['hidden_size'], device='cuda', requires_grad=True)
        alive.append(kw)                  # (the leaves hold the gradient buffers the captured launches write)
    try:
        with torch.cuda.stream(stream):
            logits = model(**kw)
            bce_with_logits_loss(logits.squeeze(1), batch['labels'], 1.8).backward()
        torch.cuda.synchronize()
    finally:
        lib.uniter_model_backward_embed = embed
    return graph, alive


class _NoSchedule(object):
    def step(self):
        pass


def new_step(precision, adv):
    model = new_model(precision)
    config = dict(optimizer='adam', lr=1e-5, beta1=0.9, beta2=0.999, weight_decay=1e-3, max_grad_norm=5, pos_wt=1.8, loss_func='bce_logits',
                  seed=1, gradient_accumulation=1 if adv else 2)
    if adv:
        config.update(adv_steps=2, adv_lr=0.1, adv_max_norm=1.0, adv_init_mag=0.0, adv_modality='both')
    return TrainStep(model, get_optimizer(model, config), _NoSchedule(), config)


def one_step(step, batch, adv):
    if adv:
        step.train_iter(batch, iters=0)
    else:
        step.train_iter(batch, iters=1)           # accumulates
        step.train_iter(batch, iters=2)           # accumulates and steps


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


def report(what, times, names):
    med = {v: statistics.median(t) for v, t in times.items()}
    parts = ['%s %.1f us (min %.1f max %.1f)' % (names[v], med[v], min(times[v]), max(times[v])) for v in times]
    if len(med) == 2:
        a, b = list(med)
        parts.append('%s - %s %+.1f us' % (names[b], names[a], med[b] - med[a]))
    print('%s: %s' % (what, '  '.join(parts)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=7, help='turns per variant')
    ap.add_argument('--replays', type=int, default=200, help='graph replays per turn (part 1)')
    ap.add_argument('--steps', type=int, default=20, help='optimizer steps per turn (part 2)')
    ap.add_argument('--precision', default='fp32x3')
    ap.add_argument('--only-off', action='store_true', help='the unchanged path alone (a library without the input gradients)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    print('device: %s; %s; library %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode(), os.path.basename(_lib.LIB_PATH)))
    variants = (False,) if args.only_off else (False, True)
    stream = torch.cuda.Stream()

    graphs = {w: capture(w, args.precision, stream) for w in variants}

    def replay(w, warm):
        n = 20 if warm else args.replays
        for _ in range(n):
            graphs[w][0].replay()
        return n
    report('padded (configs[1]) B=%d T=%d R=%d H=%d %s: uniter_model_backward_embed' % (B, T, R, BASE['hidden_size'], args.precision),
           turns(variants, replay, args.reps, stream), {False: 'without', True: 'with the three input gradients'})
    del graphs

    batch = make_synthetic_batch(B, T, R, seed=1234, device='cuda')
    steps = {a: new_step(args.precision, a) for a in variants}

    def train(a, warm):
        n = 3 if warm else args.steps
        for _ in range(n):
            one_step(steps[a], batch, a)
        return n
    report('one optimizer step behind two forward / backward passes, same shapes',
           turns(variants, train, args.reps, stream), {False: 'two accumulation micro-batches', True: 'FreeLB K = 2'})


if __name__ == '__main__':
    main()
