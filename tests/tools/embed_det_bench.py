"""What does the order-fixed embedding backward (UniterModel.deterministic) cost?  Times uniter_model_backward_embed alone, by graph
replay, with the switch off (the atomic kernels, the code every earlier commit runs) and on, on one GPU in one process:

    python tests/tools/embed_det_bench.py [--reps 7] [--replays 200] [--precision fp32x3]

Shapes: BASELINE configs[1] (B = 16, 128 tokens, 36 regions, H = 768) padded, and the ragged batch of `bench.py --ragged --packed`
(the same lengths, token packing on).  One forward + backward per variant runs eagerly; the launches uniter_model_backward_embed
makes in it are captured into a graph (main stream plus the auxiliary stream the text branch runs on; no side stream: the
encoder layers' weight gradients are not part of what is timed).  The graphs are then replayed in turns -- off, on, off, on ... --
`--replays` times per turn between two device events, and the median turn of each is printed in microseconds per replay with
its spread.  Replays add the same gradients onto the buffers again; only time is read."""
import argparse
import ctypes as C
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
from meme_challenge_amd.trainer import bce_with_logits_loss
from meme_challenge_amd.utils import make_synthetic_batch

B, T, R = 16, 128, 36


def capture(det, packed, precision, stream):
    """one training forward + backward with uniter_model_backward_embed's launches captured; returns (graph, what must stay alive)"""
    lens = {}
    if packed:
        rng = np.random.Generator(np.random.PCG64(4321))                          # bench.py --ragged
        lens = dict(txt_lens=[int(x) for x in rng.integers(8, T + 1, size=B)], num_bbs=[int(x) for x in rng.integers(10, R + 1, size=B)])
    batch = make_synthetic_batch(B, T, R, seed=1234, device='cuda', **lens)
    torch.manual_seed(0)
    cfg = UniterConfig.from_dict(BASE)
    model = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).cuda().train()
    enc = model.uniter_model
    enc.precision, enc.pack_padded, enc.use_side_stream, enc.deterministic = precision, packed, False, det
    enc.set_dropout_seed(1234, 0)
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
        # the text branch beside the image branch, as in a training step with the side stream on (model.py sets this stream there)
        _lib.check(lib.uniter_model_set_aux_stream(handle, C.c_void_p(aux.cuda_stream)), 'uniter_model_set_aux_stream')
        with torch.cuda.graph(graph, stream=torch.cuda.current_stream()):
            rc = embed(handle)
        return rc
    lib.uniter_model_backward_embed = captured_embed
    try:
        with torch.cuda.stream(stream):
            logits = model(img_feat=batch['img_feat'], img_pos_feat=batch['img_pos_feat'], input_ids=batch['input_ids'],
                           position_ids=batch['position_ids'], attention_mask=batch['attn_mask'], gather_index=batch['gather_index'],
                           output_all_encoded_layers=False, seq_lens=batch.get('seq_lens'))
            bce_with_logits_loss(logits.squeeze(1), batch['labels'], 1.8).backward()
        torch.cuda.synchronize()
    finally:
        lib.uniter_model_backward_embed = embed
    return graph, alive


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=7, help='turns per variant')
    ap.add_argument('--replays', type=int, default=200, help='graph replays per turn')
    ap.add_argument('--precision', default='fp32x3')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    print('device: %s; %s' % (torch.cuda.get_device_name(0), _lib.lib().uniter_build_info().decode()))
    stream = torch.cuda.Stream()
    for packed in (False, True):
        graphs = {det: capture(det, packed, args.precision, stream) for det in (False, True)}
        times = {False: [], True: []}
        with torch.cuda.stream(stream):
            for det in (False, True):
                for _ in range(20):
                    graphs[det][0].replay()
            for _ in range(args.reps):
                for det in (False, True):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    for _ in range(args.replays):
                        graphs[det][0].replay()
                    t1.record(stream)
                    t1.synchronize()
                    times[det].append(t0.elapsed_time(t1) * 1e3 / args.replays)
        name = 'ragged, packed (bench.py --ragged --packed)' if packed else 'padded (configs[1])'
        off, on = statistics.median(times[False]), statistics.median(times[True])
        print('%s B=%d T=%d R=%d H=%d %s: uniter_model_backward_embed  off %.1f us (min %.1f max %.1f)  on %.1f us (min %.1f max %.1f)  '
              'on - off %+.1f us' % (name, B, T, R, BASE['hidden_size'], args.precision, off, min(times[False]), max(times[False]), on,
                                     min(times[True]), max(times[True]), on - off), flush=True)
        del graphs


if __name__ == '__main__':
    main()
