"""One training step per case under whatever UNITER_* switches this process was started with.

    python tests/tools/schedule_probe.py --precision {fp32,fp32x3,bf16} --out result.npz

The C library reads its switches once per process (csrc/switches.h), so a test of another schedule starts this program as a child
with the variables set (tests/test_schedule_switches_gpu.py) and compares what it wrote with the CPU oracle and with the default
schedule's run.  It builds MemeUniter on oracle.uniter_oracle.synth_state_dict at config S, runs every case of CASES in train mode
with a fixed dropout seed, takes the project's BCE loss, runs backward, synchronises and writes logits, loss and every parameter
gradient -- TWICE per case in the same process (keys '<case>/<repeat>/...'), so the reader learns the run-to-run noise of the
schedule (float atomics).  It starts no further process and reads nothing but the repository.

The auxiliary stream UNITER_HIDDEN_PREGEN and UNITER_EMBED_BWD_PAR act on is the one every training forward pass sets
(UniterModel.use_side_stream, the default: model.py hands the library the shared 'aux' stream as the trainer's steps do).

Config S and the cases are small and sit past every threshold csrc/model.cpp tests:
  hidden 128, 2 heads, 2 layers; intermediate 2048 (the "wide" products of UNITER_B16_PERSIST bit 8 need N >= 2048; the FFN-down
  products have K = 2048 >= 512, so their k-pieces exist); 3 H = 384 = 2 x 192; 512 positions; img_dim 4096 (>= 1024, a multiple of
  64, and NOT the intermediate size: gemm() would take the region projection's weight gradient for a layer's [H, I] product).
  a  B = 3, T = 40, R = 36, ragged: M = B L = 228 rows -- two 128-row tiles, the last ragged, M % 64 != 0, M % 32 != 0
  b  B = 1, T = 1, R = 1: M = 2
  c  B = 2, T = 300, R = 20: L = 320 > 256, the streaming attention kernels and the L > uniter_attn_x3_max_len() branches
  d  B = 16, T = 8, R = 56: 896 region rows and M = 1024 -- the stream-K forms of the native fp32 products need >= 8 tiles and
     >= 2048 k-units (gemm_f32.hip: launch_v3): the region projection (UNITER_IMG_SK: 28 tiles x 128 units), its weight gradient
     (128 tiles x 28) and, with UNITER_WGRAD_WHOLE=0, the [H, I] / [I, H] weight gradients (64 tiles x 32)
"""
import argparse
import os
import sys
import time

T_START = time.time()

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIG_S = dict(vocab_size=997, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=2048,
                hidden_act='gelu', hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, max_position_embeddings=512,
                type_vocab_size=2, initializer_range=0.02)
IMG_DIM = 4096
STATE_SEED, LN_JITTER = 3, 0.05
DROP_SEED, DROP_OFFSET = 0xC0FFEE, 4
POS_WEIGHT = 1.8
PRECISIONS = ('fp32', 'fp32x3', 'bf16')
REPEATS = 2
# name -> (B, T, R, txt_lens, num_bbs, batch seed)
CASES = {
    'a': (3, 40, 36, [40, 2, 17], [36, 36, 1], 17),
    'b': (1, 1, 1, [1], [1], 18),
    'c': (2, 300, 20, [300, 37], [20, 3], 19),
    'd': (16, 8, 56, [8, 3, 5, 8, 1, 7, 8, 2, 6, 8, 4, 8, 8, 5, 3, 8], [56, 56, 40, 17, 56, 1, 56, 33, 56, 56, 9, 56, 48, 56, 56, 56], 20),
}


def state_dict():
    from oracle import uniter_oracle as O
    return O.synth_state_dict(CONFIG_S, seed=STATE_SEED, img_dim=IMG_DIM, ln_jitter=LN_JITTER)


def batch(name):
    from oracle import uniter_oracle as O
    B, T, R, tl, nbb, seed = CASES[name]
    return O.synth_batch(B, T, R, seed=seed, vocab=CONFIG_S['vocab_size'], img_dim=IMG_DIM, txt_lens=tl, num_bbs=nbb)


def model_kwargs(b):
    return dict(img_feat=b['img_feat'], img_pos_feat=b['img_pos_feat'], input_ids=b['input_ids'], position_ids=b['position_ids'],
                attention_mask=b['attn_mask'], gather_index=b['gather_index'], output_all_encoded_layers=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precision', choices=PRECISIONS, required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--cases', default=','.join(CASES))
    a = ap.parse_args()
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import numpy as np
    import torch
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.trainer import bce_with_logits_loss
    assert torch.cuda.is_available(), 'schedule_probe needs a GPU'
    cfg = UniterConfig.from_dict(CONFIG_S)
    m = MemeUniter(UniterModel(cfg, img_dim=IMG_DIM), cfg.hidden_size, 1)
    m.load_state_dict(state_dict(), strict=True)
    m = m.cuda().train()
    m.uniter_model.precision = a.precision
    store = m.param_store()
    out = {}
    for name in a.cases.split(','):
        b = {k: v.cuda() for k, v in batch(name).items()}
        for rep in range(REPEATS):
            store.zero_grads()
            m.uniter_model.set_dropout_seed(DROP_SEED, DROP_OFFSET)
            logits = m(**model_kwargs(b))
            loss = bce_with_logits_loss(logits.squeeze(1), b['labels'], POS_WEIGHT)
            loss.backward()
            torch.cuda.synchronize()
            key = '%s/%d/' % (name, rep)
            out[key + 'logits'] = logits.detach().cpu().numpy()
            out[key + 'loss'] = loss.detach().cpu().numpy()
            for n, p in m.named_parameters():
                g = p.grad if p.grad is not None else torch.zeros_like(p)
                out[key + 'grad/' + n] = g.detach().cpu().numpy().copy()
    out['seconds'] = np.float64(time.time() - T_START)
    np.savez(a.out, **out)
    print('schedule_probe %s: %d cases x %d repeats in %.1f s -> %s' % (a.precision, len(a.cases.split(',')), REPEATS,
                                                                       time.time() - T_START, a.out))


if __name__ == '__main__':
    main()
