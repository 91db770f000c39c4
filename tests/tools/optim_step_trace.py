"""What FusedAdam.step hands the library, call by call: every optimizer entry point of the loaded library is wrapped with a
recorder, a small matrix of cases runs three steps each on the TINY model with seeded gradients written straight into the flat
buffer (no backward pass: no float atomics, reproducible bits), and the log and a hash of the updated buffers are printed.
Two commits whose output is equal issue the same launches with the same arguments and compute the same bits.

    python tests/tools/optim_step_trace.py > trace.txt        (on each commit; then diff the two files)

Pointers are logged as (buffer, byte offset), streams as main / side, scalars verbatim."""
import ctypes as C
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

from common import TINY, TINY_IMG_DIM                                  # noqa: E402
from meme_challenge_amd import _lib                                     # noqa: E402
from meme_challenge_amd.meme_uniter import MemeUniter                   # noqa: E402
from meme_challenge_amd.model import UniterConfig, UniterModel          # noqa: E402
from meme_challenge_amd.trainer import FusedAdam, FusedAdamax, FusedSGD, TrainStep, get_scheduler      # noqa: E402
from meme_challenge_amd.utils import make_synthetic_batch               # noqa: E402

ENTRY_POINTS = ('uniter_adam_step_x3p', 'uniter_optim_step', 'uniter_adam_step_rows', 'uniter_grad_sumsq', 'uniter_grad_sumsq_bf16',
                'uniter_grad_sumsq_part', 'uniter_sumsq_combine')
STATE = {'opt': None, 'payload': None, 'main': None, 'side': None}


def out(*a):
    print(*a, flush=True)


def value(a):
    return (a.value or 0) if isinstance(a, C.c_void_p) else (0 if a is None else a)


def buffers():
    opt = STATE['opt']
    st = opt.store
    named = [('flat_params', st.flat_params), ('flat_grads', st.flat_grads), ('exp_avg', opt.exp_avg), ('exp_avg_sq', opt.exp_avg_sq),
             ('flags', opt._flags), ('mirror', getattr(st, 'mirror', None)), ('pair_table', getattr(st, '_pair_src', None)),
             ('sumsq', opt._sumsq), ('np_buf', opt._np_buf), ('parts', opt._parts), ('rowmask', opt._rowmask), ('ws', opt._ws),
             ('payload', STATE['payload'])]
    named += [('row_flags' if isinstance(k, tuple) and k[0] == 'rows' else 'flags', t) for k, t in opt._flags_cache.items()]
    return [(n, t) for n, t in named if t is not None]


def where(p):
    if p == 0:
        return 'NULL'
    for name, t in buffers():
        if t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size():
            return '%s+%d' % (name, p - t.data_ptr())
    return 'unknown'


def stream_name(p):
    return 'main' if p == STATE['main'] else 'side' if p == STATE['side'] else 'other'


def wrap(lib, name):
    orig, kinds = getattr(lib, name), _lib._SIGS[name][1]

    def recorder(*args):
        rc = orig(*args)                 # (first: the call may allocate nothing, but the log reads the optimizer's buffers)
        if STATE['opt'] is not None:
            shown = []
            for k, (a, kind) in enumerate(zip(args, kinds)):
                if kind is not C.c_void_p:
                    shown.append(repr(a))
                elif k == len(args) - 1:
                    shown.append(stream_name(value(a)))
                else:
                    shown.append(where(value(a)))
            out('  %s(%s) -> %d' % (name, ', '.join(shown), rc))
        return rc
    setattr(lib, name, recorder)


def grad_ready(lo, hi):
    out('  grad_ready(%d, %d) on %s' % (lo, hi, stream_name(torch.cuda.current_stream().cuda_stream)))


def build(precision, optimizer, overlap, lazy):
    torch.manual_seed(0)
    cfg = UniterConfig.from_dict(TINY)
    m = MemeUniter(UniterModel(cfg, img_dim=TINY_IMG_DIM), cfg.hidden_size, 1).cuda().train()
    enc = m.uniter_model
    enc.precision = precision
    enc.set_dropout_seed(5, 0)
    if optimizer in ('adam', 'adamw'):
        opt = FusedAdam(m, lr=1e-3, weight_decay=1e-2, adamw=(optimizer == 'adamw'))
    elif optimizer == 'adamax':
        opt = FusedAdamax(m, lr=1e-3, weight_decay=1e-2)
    else:
        opt = FusedSGD(m, lr=1e-3, momentum=0.9, weight_decay=1e-2)
    if overlap:
        opt.overlap_encoder = enc
    if lazy:
        opt.lazy_zero_encoder = enc
    orig = enc._set_ready_events
    enc._set_ready_events = lambda events: (out('  set_ready_events(%d events)' % len(events)), orig(events))[1]
    return m, enc, opt


def digest(opt):
    st = opt.store
    opt.join()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (st.flat_params, opt.exp_avg, opt.exp_avg_sq, getattr(st, 'mirror', None)):
        if t is not None:
            h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def injected(name, precision='fp32', optimizer='adam', overlap=False, clip=0.0, ready=False, pieces=False, payload=False,
             rows=False, lazy=False, env=None):
    out('CASE %s' % name)
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        m, enc, opt = build(precision, optimizer, overlap, lazy)
        st = opt.store
        batch = make_synthetic_batch(4, 16, 6, seed=3, vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM, device='cuda')
        with torch.no_grad():           # one forward pass: the library handle and the mode's weight mirror exist as in training
            m(img_feat=batch['img_feat'], img_pos_feat=batch['img_pos_feat'], input_ids=batch['input_ids'],
              position_ids=batch['position_ids'], attention_mask=batch['attn_mask'], gather_index=batch['gather_index'],
              output_all_encoded_layers=False)
        if rows:
            opt.split_word_rows = True
            opt._word_cache = None
        gen = torch.Generator(device='cuda').manual_seed(11)
        cuts = [0] + [r[1] for r in sorted(st.bucket_ranges)]
        third = [(cuts[0], cuts[1]), (cuts[1], cuts[-2]), (cuts[-2], cuts[-1])]
        STATE['opt'] = opt
        for k in range(3):
            out(' step %d' % k)
            if rows:
                opt.note_tokens(batch['input_ids'])
                out('  early_word_update -> %r' % opt.early_word_update())
            st.flat_grads.copy_(torch.randn(st.numel, device='cuda', generator=gen) * 1e-2)
            st.touch(st.names)
            kw = {}
            if payload:
                STATE['payload'] = kw['grad_bf16'] = st.flat_grads.to(torch.bfloat16)
            if ready:
                kw['grad_ready'] = grad_ready
            if pieces:
                kw['grad_pieces'] = third
            opt.step(grad_scale=0.5, max_grad_norm=clip, zero_grads=True, **kw)
        out('HASH %s %s' % (name, digest(opt)))
    finally:
        STATE['opt'] = STATE['payload'] = None
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def through_train_iter(name):
    """TrainStep.train_iter with the clip norm taken during the backward pass (attach_norm_hooks), encoder on one stream; the
    backward's float atomics make the bits vary from run to run: the log only"""
    out('CASE %s' % name)
    m, enc, opt = build('fp32', 'adam', True, False)
    enc.use_side_stream = False
    config = dict(optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=1e-2, gradient_accumulation=1, max_grad_norm=0.05,
                  pos_wt=1.8, loss_func='bce_logits', scheduler='warmup_cosine', warmup_steps=2, max_epoch=2)
    step = TrainStep(m, opt, get_scheduler(opt, config, steps_per_epoch=10), config)
    batch = make_synthetic_batch(4, 16, 6, seed=3, vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM, device='cuda')
    STATE['opt'] = opt
    try:
        for k in range(3):
            out(' step %d' % k)
            step.train_iter(batch, iters=0)
        opt.join()
        torch.cuda.synchronize()
    finally:
        STATE['opt'] = None


def main():
    dev = torch.device('cuda:0')
    STATE['main'] = torch.cuda.current_stream().cuda_stream
    STATE['side'] = _lib.shared_stream(dev, 'side').cuda_stream
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        wrap(lib, name)
    # one launch on the caller's stream
    injected('plain_adam_fp32')
    injected('plain_adamw_bf16_clip', precision='bf16', optimizer='adamw', clip=0.05)
    injected('plain_adamax_fp32x3_clip_lazy', precision='fp32x3', optimizer='adamax', clip=0.05, lazy=True)
    injected('plain_sgd_fp32', optimizer='sgd')
    injected('plain_adam_ready_pieces_clip', clip=0.05, ready=True, pieces=True)
    injected('plain_adam_ready_pieces_payload_clip', clip=0.05, ready=True, pieces=True, payload=True)
    injected('plain_adamw_payload', optimizer='adamw', payload=True)
    injected('plain_adam_ready', ready=True)
    injected('plain_adam_rows_clip', clip=0.05, rows=True)
    injected('plain_adamw_rows_ready', optimizer='adamw', rows=True, ready=True)
    # block by block beside the next forward pass
    injected('overlap_adam_fp32x3_clip_lazy', precision='fp32x3', overlap=True, clip=0.05, lazy=True)
    injected('overlap_adamw_bf16', precision='bf16', optimizer='adamw', overlap=True)
    injected('overlap_adamax_fp32_clip', optimizer='adamax', overlap=True, clip=0.05)
    injected('overlap_sgd_fp32x3', precision='fp32x3', optimizer='sgd', overlap=True)
    injected('overlap_adam_ready_pieces_clip', overlap=True, clip=0.05, ready=True, pieces=True)
    injected('overlap_adam_bf16_ready_payload', precision='bf16', overlap=True, ready=True, payload=True)
    injected('overlap_adam_rows_clip', overlap=True, clip=0.05, rows=True)
    injected('overlap_adamw_fp32x3_rows_ready', precision='fp32x3', optimizer='adamw', overlap=True, rows=True, ready=True)
    injected('overlap_adam_emb_side', overlap=True, env={'UNITER_ADAM_EMB_MAIN': '0'})
    injected('overlap_adam_bf16_no_word_split', precision='bf16', overlap=True, clip=0.05, env={'UNITER_ADAM_WORD_SPLIT': '0'})
    injected('overlap_adam_grids', overlap=True, rows=True, env={'UNITER_ADAM_WORD_WGS': '96', 'UNITER_ADAM_EARLY_WGS': '48'})
    through_train_iter('train_iter_norm_hooks_one_stream')
    out('DONE')


if __name__ == '__main__':
    main()
