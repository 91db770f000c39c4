"""What do MRC / MRC-kl batches drawn on the device cost?  One GPU, one process:

    python tests/tools/device_mrc_bench.py [--reps 5] [--steps 24] [--samples 256]

All at B = 32, T = 128, R = 36, D = 2048, C = 1601, mask_prob 0.15.
1. uniter_collate_mrc_batch alone against uniter_collate_pretrain_batch's MRFR launch in the same process: device-event time per
   launch over `--launches` launches into preallocated outputs, issued one by one from Python (bounded by the host's launch rate)
   and replayed from one captured graph (the kernel's own time).  The MRC launch in its three forms: label_ids alone (what the
   loader asks for 'mrc'), label_targets alone ('mrc-kl'), both.
2. For 'mrc': label_ids from the collate launch against label_targets from the collate launch plus uniter_row_argmax over the
   n_masked rows (what forward_mrc runs without label_ids) -- the same measurement, two launches per turn.
3. An 'mrc' step and an 'mrc-kl' step (UniterForPretraining at BASELINE configs[4] shapes, fused Adam, as
   tests/tools/device_pretrain_bench.py runs it) fed by data.DevicePretrainLoader, against the same steps on frozen batches: the
   first `--steps` batches of the same loader, staged once and replayed.  One turn = `--steps` steps, wall clock from a
   synchronised start to a synchronised end, the two cases in alternating turns after a warm-up turn each; median, minimum and
   maximum over the turns."""
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
from meme_challenge_amd.data import (DeviceFeaturePool, DeviceMemeDataset, DevicePretrainLoader, HashTokenizer, MemeDataset,
                                     collate_mrc_batch, collate_pretrain_batch, write_synthetic_dataset)
from meme_challenge_amd.model import UniterConfig
from meme_challenge_amd.pretrain import UniterForPretraining, _hard_region_labels
from meme_challenge_amd.trainer import FusedAdam

R, IMG_DIM, LABEL_DIM = 36, 2048, 1601


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
    L_out = dds.T + R
    tail = (dds.d_row_start, dds.d_row_cnt, dds.d_input_ids, dds.d_token_type_ids, dds.d_txt_len, dds.d_labels, dds.d_ids)
    feat, pos, soft = pool.feat[:pool.rows], pool.pos[:pool.rows], pool.soft[:pool.rows]
    common = dict(R=R, L_out=L_out, ragged_regions=False, seed=1, draw=0, prob=0.15)

    def mrc(hard, soft_out):
        return lambda out: collate_mrc_batch(sel, feat, pos, soft, *tail, label_dim=LABEL_DIM, hard=hard, soft_out=soft_out, out=out, **common)

    def rows_then_argmax(out):
        out = mrc(False, True)(out)
        _hard_region_labels(out['label_targets'][:rows_then_argmax.n])
        return out
    calls = {'mrfr': lambda out: collate_pretrain_batch('mrfr', sel, None, feat, pos, *tail, out=out, **common),
             'mrc label_ids': mrc(True, False), 'mrc-kl label_targets': mrc(False, True), 'mrc both': mrc(True, True),
             'label_targets + row_argmax': rows_then_argmax}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rows_then_argmax.n = int(mrc(False, True)(None)['n_masked'].item())
        for name, call in calls.items():
            out = call(None)
            stream.synchronize()
            n_masked = int(out['n_masked'].item())

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
                print('collate alone, %-26s B=%d R=%d T=%d D=%d C=%d n_masked=%d, %s: %.2f us per turn (min %.2f max %.2f over %d passes of %d)'
                      % (name, B, R, dds.T, IMG_DIM, LABEL_DIM, n_masked, how, statistics.median(t), min(t), max(t), len(t), launches), flush=True)


def new_step():
    torch.manual_seed(0)
    model = UniterForPretraining(UniterConfig.from_dict(BASE), img_dim=IMG_DIM, img_label_dim=LABEL_DIM).cuda().train()
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
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--max_txt_len', type=int, default=128)
    ap.add_argument('--launches', type=int, default=100, help='collate launches per timed pass (parts 1 and 2)')
    ap.add_argument('--skip_step', action='store_true', help='parts 1 and 2 only')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    print('device: %s; %s; library %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode(), os.path.basename(_lib.LIB_PATH)))
    T, B = args.max_txt_len, args.batch_size
    with tempfile.TemporaryDirectory() as root:
        write_synthetic_dataset(root, n=args.samples, num_bb=(R, R), img_dim=IMG_DIM, splits=('train',), text_words=(T // 2, T),
                                label_dim=LABEL_DIM)
        tok = partial(HashTokenizer(max_length=T), max_length=T)
        ds = MemeDataset(os.path.join(root, 'train.jsonl'), os.path.join(root, 'img_feats'), text_padding=tok, soft_labels=True)
        dds = DeviceMemeDataset(ds, DeviceFeaturePool('cuda', soft_labels=True))
    torch.cuda.synchronize()
    print('dataset: %d samples, %d regions x %d, %d classes (ld_soft %d), up to %d tokens; %.1f MB resident'
          % (len(ds), R, IMG_DIM, dds.label_dim, dds.pool.ld_soft, T, dds.pool.resident_bytes / 1e6), flush=True)
    collate_alone(dds, B, args.launches)
    if args.skip_step:
        return
    step = new_step()
    for task in ('mrc', 'mrc-kl'):
        staged = []
        for _, batch in DevicePretrainLoader(dds, B, tasks=((task, 1),), seed=0):
            staged.append(batch)
            if len(staged) == args.steps:
                break

        def live():
            for i, (_, batch) in enumerate(DevicePretrainLoader(dds, B, tasks=((task, 1),), seed=0)):      # the staged sequence again
                step(task, batch)
                if i + 1 == args.steps:
                    break

        def frozen():
            for batch in staged:
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
        for name, t in times.items():
            med = statistics.median(t)
            print('%s step B=%d, %-24s %.3f ms per step (min %.3f max %.3f over %d turns of %d steps)  %.1f samples/s  %+.3f ms against frozen'
                  % (task, B, name + ':', med * 1e3, min(t) * 1e3, max(t) * 1e3, len(t), args.steps, B / med, (med - base) * 1e3), flush=True)


if __name__ == '__main__':
    main()
