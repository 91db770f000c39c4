"""What do pretraining batches drawn on the device cost?  One GPU, one process:

    python tests/tools/device_pretrain_bench.py [--reps 5] [--steps 24] [--samples 256] [--batches 32,256]

1. uniter_collate_pretrain_batch alone, per task, at R = 36, T = 128, D = 2048 and each batch size of --batches: device-event time
   per launch over `--launches` launches into preallocated outputs, issued one by one from Python (bounded by the host's launch
   rate) and replayed from one captured graph (the kernel's own time), with mask_prob 0.15.  The plain uniter_collate_batch at the
   same shape stands beside it: the difference is what the masks, their compaction and the B^2 recomputation add.
2. The multitask step (UniterForPretraining at BASELINE configs[4] shapes: B = 32, 36 regions, 128 tokens; fused Adam, as
   tests/tools/pretrain_bench.py runs it) fed by data.DevicePretrainLoader, against the same step on frozen batches: the first
   `--steps` (task, batch) pairs of the same loader, staged once and replayed.  One turn = `--steps` steps, wall clock from a
   synchronised start to a synchronised end, the two cases in alternating turns after a warm-up turn each; median, minimum and
   maximum over the turns.  The live case pays the collate launch and the n_masked read per step; the frozen case pays the model's
   own nonzero instead when --frozen_nonzero is given (masked_positions removed from the staged batches)."""
import argparse
import os
import statistics
import sys
import tempfile
import time
from functools import partial

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import torch

from bench import BASE
from meme_challenge_amd import _lib
from meme_challenge_amd.data import (DeviceFeaturePool, DeviceMemeDataset, DevicePretrainLoader, HashTokenizer, MemeDataset, collate_batch,
                                     collate_pretrain_batch, write_synthetic_dataset)
from meme_challenge_amd.model import UniterConfig
from meme_challenge_amd.pretrain import UniterForPretraining
from meme_challenge_amd.trainer import FusedAdam

R, IMG_DIM = 36, 2048


def timed(stream, run, launches, passes=6):
    times = []
    for _ in range(passes):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        run()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / launches)
    return times[1:]                     # the first pass pays the graph's upload


def collate_alone(dds, B, launches):
    pool = dds.pool
    n_samples = len(dds)
    sel = (torch.arange(B, dtype=torch.int64, device='cuda') * 7 + 3) % n_samples
    txt_sel = torch.where(torch.arange(B, device='cuda') % 2 == 0, sel, (sel + 1) % n_samples)
    L_out = dds.T + R
    args = (pool.feat[:pool.rows], pool.pos[:pool.rows], dds.d_row_start, dds.d_row_cnt, dds.d_input_ids, dds.d_token_type_ids,
            dds.d_txt_len, dds.d_labels, dds.d_ids)
    calls = {'plain': lambda out: collate_batch(sel, *args, R=R, L_out=L_out, ragged_regions=False, out=out)}
    for task in ('mlm', 'mrfr', 'itm'):
        calls[task] = partial(lambda out, task: collate_pretrain_batch(task, sel, txt_sel if task == 'itm' else None, *args, R=R, L_out=L_out,
                                                                       ragged_regions=False, seed=1, draw=0, prob=0.15, out=out), task=task)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for name, call in calls.items():
            out = call(None)
            stream.synchronize()
            n_masked = int(out['n_masked'].item()) if 'n_masked' in out else 0

            def eager(k):
                for _ in range(k):
                    call(out)
            graph = torch.cuda.CUDAGraph()
            eager(3)
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                eager(launches)
            for how, run in (('one by one', lambda: eager(launches)), ('graph replay', graph.replay)):
                t = timed(stream, run, launches)
                print('collate alone, %-5s B=%d R=%d T=%d D=%d n_masked=%d, %s: %.2f us per launch (min %.2f max %.2f over %d passes of %d launches)'
                      % (name, B, R, dds.T, IMG_DIM, n_masked, how, statistics.median(t), min(t), max(t), len(t), launches), flush=True)


def new_step():
    torch.manual_seed(0)
    model = UniterForPretraining(UniterConfig.from_dict(BASE), img_dim=IMG_DIM, img_label_dim=1601).cuda().train()
    model.uniter.set_dropout_seed(1, 0)
    opt = FusedAdam(model, lr=3e-5, weight_decay=1e-3)

    def step(task, batch):
        loss = model(batch, task).mean()
        loss.backward()
        opt.step(grad_scale=1.0, max_grad_norm=5)
    return step


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5, help='turns per case')
    ap.add_argument('--steps', type=int, default=24, help='steps per turn')
    ap.add_argument('--samples', type=int, default=256, help='samples of the synthetic training file')
    ap.add_argument('--batches', default='32,256', help='batch sizes of part 1')
    ap.add_argument('--batch_size', type=int, default=32, help='batch size of part 2')
    ap.add_argument('--max_txt_len', type=int, default=128)
    ap.add_argument('--launches', type=int, default=100, help='collate launches per timed pass (part 1)')
    ap.add_argument('--frozen_nonzero', action='store_true', help='the frozen batches go through the model\'s own nonzero')
    ap.add_argument('--skip_step', action='store_true', help='part 1 only')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    print('device: %s; %s; library %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode(), os.path.basename(_lib.LIB_PATH)))
    T = args.max_txt_len
    with tempfile.TemporaryDirectory() as root:
        write_synthetic_dataset(root, n=args.samples, num_bb=(R, R), img_dim=IMG_DIM, splits=('train',), text_words=(T // 2, T))
        tok = partial(HashTokenizer(max_length=T), max_length=T)
        ds = MemeDataset(os.path.join(root, 'train.jsonl'), os.path.join(root, 'img_feats'), text_padding=tok)
        dds = DeviceMemeDataset(ds, DeviceFeaturePool('cuda'))
    torch.cuda.synchronize()
    print('dataset: %d samples, %d regions x %d, up to %d tokens; %.1f MB of region rows resident'
          % (len(ds), R, IMG_DIM, T, dds.pool.resident_bytes / 1e6), flush=True)
    for B in [int(b) for b in args.batches.split(',')]:
        collate_alone(dds, B, args.launches)
    if args.skip_step:
        return
    B = args.batch_size
    staged = []
    for task, batch in DevicePretrainLoader(dds, B, seed=0):
        staged.append((task, {k: v for k, v in batch.items() if not (args.frozen_nonzero and k == 'masked_positions')}))
        if len(staged) == args.steps:
            break
    step = new_step()

    def live():
        loader = DevicePretrainLoader(dds, B, seed=0)           # the same (task, batch) sequence as the staged one
        for i, (task, batch) in enumerate(loader):
            step(task, batch)
            if i + 1 == args.steps:
                break

    def frozen():
        for task, batch in staged:
            step(task, batch)
    cases = {'frozen batches': frozen, 'device pretrain loader': live}
    times = {name: [] for name in cases}
    for run in cases.values():
        run()
    for _ in range(args.reps):
        for name, run in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps)
    base = statistics.median(times['frozen batches'])
    mix = ', '.join('%s x %d' % (t, sum(1 for x, _ in staged if x == t)) for t in ('mlm', 'mrfr', 'itm'))
    for name, t in times.items():
        med = statistics.median(t)
        print('multitask step B=%d (%s%s), %-24s %.3f ms per step (min %.3f max %.3f over %d turns of %d steps)  %.1f samples/s  %+.3f ms against frozen'
              % (B, mix, '; frozen through nonzero' if args.frozen_nonzero else '', name + ':', med * 1e3, min(t) * 1e3, max(t) * 1e3, len(t),
                 args.steps, B / med, (med - base) * 1e3), flush=True)


if __name__ == '__main__':
    main()
