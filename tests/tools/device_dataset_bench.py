"""What does the input side cost the training step, and what does the device-resident dataset change?  One GPU, one process:

    python tests/tools/device_dataset_bench.py [--reps 5] [--samples 256] [--max_txt_len 128] [--precisions bf16,fp32x3]

1. Train samples/s over a synthetic full-length dataset in the reference's on-disk format (data.write_synthetic_dataset: 36 regions,
   --max_txt_len tokens, batch 16; BASELINE configs[1] shapes), one turn = one epoch of trainer.TrainStep steps, wall clock from a
   synchronised start to a synchronised end, the three cases in alternating turns after a warm-up turn each:
     (a) bare      the step alone, every iteration on one pre-staged batch;
     (b) host      today's default: DataLoader(num_workers=0, pin_memory) + the host collate behind the threaded data.DevicePrefetcher;
     (c) device    data.DeviceLoader: the dataset resident in device memory, one uniter_collate_batch launch per batch.
   Median, minimum and maximum over the turns.
2. The collate launch alone at that shape: device-event time per launch over `--launches` launches into preallocated outputs, issued one
   by one from Python (bounded by the host's launch rate) and replayed from one captured graph (the kernel's own time), with the bytes
   the launch reads and writes and the resulting GB/s."""
import argparse
import os
import statistics
import sys
import tempfile
import time
from functools import partial

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

import torch
from torch.utils import data

from bench import BASE
from meme_challenge_amd import _lib
from meme_challenge_amd.data import (DeviceFeaturePool, DeviceLoader, DeviceMemeDataset, DevicePrefetcher, HashTokenizer, MemeDataset,
                                     collate_batch, write_synthetic_dataset)
from meme_challenge_amd.meme_uniter import MemeUniter
from meme_challenge_amd.model import UniterConfig, UniterModel
from meme_challenge_amd.trainer import TrainStep, get_optimizer

B, R, IMG_DIM = 16, 36, 2048


class _NoSchedule(object):
    def step(self):
        pass


def new_step(precision):
    torch.manual_seed(0)
    cfg = UniterConfig.from_dict(BASE)
    model = MemeUniter(UniterModel(cfg, img_dim=IMG_DIM), cfg.hidden_size, 1).cuda().train()
    model.uniter_model.precision = precision
    model.uniter_model.set_dropout_seed(1234, 0)
    config = dict(optimizer='adam', lr=1e-5, beta1=0.9, beta2=0.999, weight_decay=1e-3, max_grad_norm=5, pos_wt=1.8, loss_func='bce_logits',
                  seed=1, gradient_accumulation=1)
    return TrainStep(model, get_optimizer(model, config), _NoSchedule(), config)


def epoch(step, batches):
    n = 0
    for it, batch in enumerate(batches):
        step.train_iter(batch, iters=it)
        n += int(batch['labels'].shape[0])
    return n


def turns(cases, reps):
    """cases: name -> callable running one epoch and returning its sample count; -> name -> [samples/s per turn]"""
    rates = {name: [] for name in cases}
    for name, run in cases.items():             # warm-up: allocator, workspaces, page cache
        run()
    for _ in range(reps):
        for name, run in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = run()
            torch.cuda.synchronize()
            rates[name].append(n / (time.perf_counter() - t0))
    return rates


def collate_alone(dds, launches):
    pool = dds.pool
    sel = torch.arange(B, dtype=torch.int64, device='cuda')
    tl, n = dds.txt_len[:B].astype('int64'), dds.row_cnt[:B].astype('int64')
    Rb, L_out = int(n.max()), int((tl + n.max()).max())
    args = (sel, pool.feat[:pool.rows], pool.pos[:pool.rows], dds.d_row_start, dds.d_row_cnt, dds.d_input_ids, dds.d_token_type_ids,
            dds.d_txt_len, dds.d_labels, dds.d_ids)
    out = collate_batch(*args, R=Rb, L_out=L_out, ragged_regions=False)
    written = sum(t.numel() * t.element_size() for t in out.values() if t is not None)
    read = int(n.sum()) * (pool.dim + 7) * 4 + B * dds.T * 8 * (2 if dds.d_token_type_ids is not None else 1) + B * 40
    nbytes = read + written
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        def eager(k):
            for _ in range(k):
                collate_batch(*args, R=Rb, L_out=L_out, ragged_regions=False, out=out)
        graph = torch.cuda.CUDAGraph()
        eager(3)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            eager(launches)
        for name, run in (('one by one', lambda: eager(launches)), ('graph replay', graph.replay)):
            times = []
            for _ in range(6):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                run()
                t1.record(stream)
                t1.synchronize()
                times.append(t0.elapsed_time(t1) * 1e3 / launches)
            res[name] = times[1:]                # the first pass pays the graph's upload
    return nbytes, (B, Rb, L_out), res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5, help='turns per case')
    ap.add_argument('--samples', type=int, default=256, help='samples of the synthetic training file (one turn = one epoch over them)')
    ap.add_argument('--max_txt_len', type=int, default=128)
    ap.add_argument('--precisions', default='bf16,fp32x3')
    ap.add_argument('--launches', type=int, default=200, help='collate launches per timed pass (part 2)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    torch.set_num_threads(min(torch.get_num_threads(), 8))          # as train_uniter._cap_cpu_threads
    print('device: %s; %s; library %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode(), os.path.basename(_lib.LIB_PATH)))
    T = args.max_txt_len
    with tempfile.TemporaryDirectory() as root:
        write_synthetic_dataset(root, n=args.samples, num_bb=(R, R), img_dim=IMG_DIM, splits=('train',), text_words=(T, T))
        tok = partial(HashTokenizer(max_length=T), max_length=T)
        ds = MemeDataset(os.path.join(root, 'train.jsonl'), os.path.join(root, 'img_feats'), text_padding=tok)
        host = DevicePrefetcher(data.DataLoader(ds, batch_size=B, num_workers=0, collate_fn=ds.get_collate_fn(), pin_memory=True), 'cuda')
        t0 = time.perf_counter()
        dds = DeviceMemeDataset(ds, DeviceFeaturePool('cuda'))
        torch.cuda.synchronize()
        print('dataset: %d samples, %d regions x %d, %d tokens, batch %d; resident in %.2f s, %.1f MB of region rows'
              % (len(ds), R, IMG_DIM, T, B, time.perf_counter() - t0, dds.pool.resident_bytes / 1e6), flush=True)
        device = DeviceLoader(dds, B)
        staged = next(iter(device))
        steps_per_epoch = len(device)
        for precision in args.precisions.split(','):
            step = new_step(precision)
            cases = {'(a) bare step': lambda: epoch(step, (staged for _ in range(steps_per_epoch))),
                     '(b) host collate + prefetch thread': lambda: epoch(step, host),
                     '(c) device loader': lambda: epoch(step, device)}
            rates = turns(cases, args.reps)
            bare = statistics.median(rates['(a) bare step'])
            for name, r in rates.items():
                med = statistics.median(r)
                print('%s %-36s %8.1f samples/s (min %.1f max %.1f over %d turns of %d steps)  %5.1f %% of (a)  %.3f ms per step'
                      % (precision, name, med, min(r), max(r), len(r), steps_per_epoch, 100.0 * med / bare, 1e3 * B / med), flush=True)
            del step
        nbytes, shape, res = collate_alone(dds, args.launches)
        for name, t in res.items():
            med = statistics.median(t)
            print('uniter_collate_batch alone, B=%d R=%d L_out=%d D=%d, %s: %.2f us per launch (min %.2f max %.2f over %d passes of %d launches), '
                  '%.2f MB read + written, %.0f GB/s' % (shape + (IMG_DIM, name, med, min(t), max(t), len(t), args.launches, nbytes / 1e6,
                                                          nbytes / med / 1e3)), flush=True)


if __name__ == '__main__':
    main()
