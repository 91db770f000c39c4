"""GPU: whole-model parity of the HIP path (through the C ABI via the Python
mirror) against (a) golden vectors produced by the reference and (b) the oracle
on the same seeded inputs, including train mode with replayed dropout masks."""
import numpy as np
import pytest
import torch

from oracle import uniter_oracle as O
from oracle import step_oracle as S
from common import (TINY, TINY_IMG_DIM, BASE, LARGE, sd_from_npz, batch_from_npz, model_kwargs, maxdiff)

pytestmark = pytest.mark.gpu


# the two forms of the fp32 path: native fp32 MFMA kernels, and the same products from three bf16 pieces per value on the bf16
# matrix pipe (csrc/gemm_split3.hip) -- both are held to the SAME golden vectors at the SAME tolerances
FP32_MODES = ['fp32', 'fp32x3']


def build(cfg_dict, img_dim, sd, precision='fp32'):
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    cfg = UniterConfig.from_dict(cfg_dict)
    m = MemeUniter(UniterModel(cfg, img_dim=img_dim), cfg.hidden_size, 1)
    missing = m.load_state_dict(sd, strict=True)
    m.uniter_model.precision = precision
    return m.cuda()


def to_dev(b):
    return {k: v.cuda() for k, v in b.items()}


@pytest.mark.parametrize('precision', FP32_MODES)
def test_tiny_forward_matches_reference_golden(tiny, precision):
    sd = sd_from_npz(tiny)
    m = build(TINY, TINY_IMG_DIM, sd, precision).eval()
    b = to_dev(batch_from_npz(tiny))
    with torch.no_grad():
        kw = model_kwargs(b)
        kw['output_all_encoded_layers'] = True
        layers = m.uniter_model(**kw)
        for i, l in enumerate(layers):
            assert maxdiff(l, tiny['out/layer%d' % i]) < 2e-5, i
        pooled = m.uniter_model.pooler(layers[-1])
        assert maxdiff(pooled, tiny['out/pooled']) < 1e-5
        logits = m(**model_kwargs(b))
        assert maxdiff(logits, tiny['out/logits']) < 1e-5
        B, T = b['input_ids'].shape
        R = b['img_feat'].shape[1]
        t = m.uniter_model(b['input_ids'], b['position_ids'], None, None, torch.ones(B, T, device='cuda'),
                           output_all_encoded_layers=False)
        assert maxdiff(t, tiny['out/txt_only']) < 2e-5
        i = m.uniter_model(None, None, b['img_feat'], b['img_pos_feat'], torch.ones(B, R, device='cuda'),
                           output_all_encoded_layers=False)
        assert maxdiff(i, tiny['out/img_only']) < 2e-5
        kw = model_kwargs(b)
        kw['img_masks'] = b['img_masks']
        mk = m.uniter_model(**kw)
        assert maxdiff(mk, tiny['out/masked']) < 2e-5


@pytest.mark.parametrize('precision', FP32_MODES)
def test_tiny_loss_and_all_grads_match_reference_golden(tiny, precision):
    from meme_challenge_amd.trainer import bce_with_logits_loss
    sd = sd_from_npz(tiny)
    m = build(TINY, TINY_IMG_DIM, sd, precision).eval()      # eval + grad enabled, as the golden was made
    b = to_dev(batch_from_npz(tiny))
    logits = m(**model_kwargs(b))
    loss = bce_with_logits_loss(logits, b['labels'], 1.8)
    assert abs(loss.item() - float(tiny['out/loss'])) < 1e-6
    loss.backward()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        ref = torch.from_numpy(tiny['grad/' + n])
        tol = 2e-6 + 2e-4 * ref.abs().max().item()
        assert maxdiff(p.grad, ref) <= tol, (n, maxdiff(p.grad, ref), tol)


@pytest.mark.parametrize('precision', FP32_MODES)
@pytest.mark.parametrize('name', ['cfg1_full', 'cfg1_ragged', 'cfg2_full'])
def test_base_logits_and_grads_match_reference_golden(shapes_base, name, precision):
    from meme_challenge_amd.trainer import bce_with_logits_loss
    from meme_challenge_amd.utils import make_synthetic_batch
    z = shapes_base
    sd = O.synth_state_dict(BASE, seed=0, ln_jitter=0.02)
    m = build(BASE, 2048, sd, precision).eval()
    B, T, R, seed = z[name + '/shape'].tolist()
    tl = z[name + '/txt_lens'].tolist() if name + '/txt_lens' in z.files else None
    nbb = z[name + '/num_bbs'].tolist() if name + '/num_bbs' in z.files else None
    b = make_synthetic_batch(B, T, R, seed=seed, txt_lens=tl, num_bbs=nbb, device='cuda')
    logits = m(**model_kwargs(b))
    # north_star: logits within 1e-3 (fp32) of the reference CPU path
    assert maxdiff(logits, z[name + '/logits']) < 1e-3
    assert maxdiff(logits, z[name + '/logits']) < 5e-5     # what fp32 MFMA actually achieves
    loss = bce_with_logits_loss(logits, b['labels'], 1.8)
    assert abs(loss.item() - float(z[name + '/loss'])) < 1e-5
    loss.backward()
    torch.cuda.synchronize()
    names = list(z['param_names'])
    norms = z[name + '/grad_norms']
    params = dict(m.named_parameters())
    for n, ref in zip(names, norms):
        got = params[n].grad.double().norm().item()
        assert abs(got - ref) <= 1e-6 + 2e-3 * ref, (n, got, ref)
    for key in [k for k in z.files if k.startswith(name + '/gslice/')]:
        n = key.split('/gslice/')[1]
        ref = torch.from_numpy(z[key])
        got = params[n].grad.reshape(-1)[:4096]
        assert maxdiff(got, ref) <= 1e-7 + 1e-3 * ref.abs().max().item(), n
    rows = torch.from_numpy(z[name + '/word_rows'])
    got = params['uniter_model.embeddings.word_embeddings.weight'].grad[rows.cuda()]
    ref = torch.from_numpy(z[name + '/word_grad_rows'])
    assert maxdiff(got, ref) <= 1e-7 + 1e-3 * ref.abs().max().item()


@pytest.mark.parametrize('precision', FP32_MODES)
def test_large_logits_match_reference_golden(shapes_large, precision):
    from meme_challenge_amd.utils import make_synthetic_batch
    z = shapes_large
    sd = O.synth_state_dict(LARGE, seed=0, ln_jitter=0.02)
    m = build(LARGE, 2048, sd, precision).eval()
    B, T, R, seed = z['cfg4_full/shape'].tolist()
    b = make_synthetic_batch(B, T, R, seed=seed, device='cuda')
    with torch.no_grad():
        logits = m(**model_kwargs(b))
    assert maxdiff(logits, z['cfg4_full/logits']) < 1e-3


@pytest.mark.parametrize('precision', FP32_MODES)
def test_train_mode_dropout_replay_matches_oracle(tiny, precision):
    """Train mode: same Philox masks in the oracle and in the kernels -> forward
    and every parameter gradient agree to fp32 round-off."""
    from meme_challenge_amd.trainer import bce_with_logits_loss
    sd = sd_from_npz(tiny)
    m = build(TINY, TINY_IMG_DIM, sd, precision).train()
    seed, offset = 0x5EED5EED1234, 9
    m.uniter_model.set_dropout_seed(seed, offset)
    b = batch_from_npz(tiny)
    logits = m(**model_kwargs(to_dev(b)))
    loss = bce_with_logits_loss(logits, b['labels'].cuda(), 1.8)
    loss.backward()
    torch.cuda.synchronize()
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    drop = O.DropSpec(seed, offset, TINY['hidden_dropout_prob'], TINY['attention_probs_dropout_prob'])
    lo = O.meme_uniter_forward(sdo, TINY, drop=drop, **model_kwargs(b))
    assert maxdiff(logits, lo) < 1e-5
    S.bce_with_logits(lo, b['labels'], 1.8).backward()
    for n, p in m.named_parameters():
        ref = sdo[n].grad if sdo[n].grad is not None else torch.zeros_like(sdo[n])
        tol = 2e-6 + 2e-4 * ref.abs().max().item()
        assert maxdiff(p.grad, ref) <= tol, (n, maxdiff(p.grad, ref), tol)
    # a second forward draws different masks (offset advanced)
    l2 = m(**model_kwargs(to_dev(b)))
    assert maxdiff(l2, logits) > 1e-6


@pytest.mark.parametrize('mode', ['bf16', 'bf16_hybrid'])
def test_bf16_mfma_mode_tracks_fp32_reference(shapes_base, mode):
    """precision='bf16' (bf16-resident operands: weight mirror + bf16 activation copies) and
    'bf16_hybrid' (fp32 operands rounded in flight): dense GEMM inputs in bf16, fp32 accumulate,
    fp32 everything else.  Not the 1e-3 fp32 parity bar: bf16 has 8 significant bits, so the bar is
    closeness + gradient direction."""
    from meme_challenge_amd.trainer import bce_with_logits_loss
    from meme_challenge_amd.utils import make_synthetic_batch
    z = shapes_base
    sd = O.synth_state_dict(BASE, seed=0, ln_jitter=0.02)
    m = build(BASE, 2048, sd).eval()
    m.uniter_model.precision = mode
    B, T, R, seed = z['cfg1_full/shape'].tolist()
    b = make_synthetic_batch(B, T, R, seed=seed, device='cuda')
    logits = m(**model_kwargs(b))
    ref = torch.from_numpy(z['cfg1_full/logits'])
    assert maxdiff(logits, ref) < 3e-2
    assert maxdiff(logits, ref) > 1e-6            # really ran the bf16 path
    loss = bce_with_logits_loss(logits, b['labels'], 1.8)
    loss.backward()
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    names = list(z['param_names'])
    norms = z['cfg1_full/grad_norms']
    rel = [abs(params[n].grad.double().norm().item() - r) / max(r, 1e-12) for n, r in zip(names, norms) if r > 1e-8]
    assert np.median(rel) < 2e-2 and max(rel) < 0.25
    for key in [k for k in z.files if k.startswith('cfg1_full/gslice/')]:
        n = key.split('/gslice/')[1]
        r = torch.from_numpy(z[key]).double()
        g = params[n].grad.reshape(-1)[:4096].cpu().double()
        cos = (g @ r) / (g.norm() * r.norm() + 1e-30)
        assert cos > 0.99, (n, cos.item())
    m.uniter_model.precision = 'fp32'
    l2 = m(**model_kwargs(b))
    assert maxdiff(l2, ref) < 5e-5               # switching back restores exact fp32 parity


def test_bf16_resident_equals_hybrid_and_follows_weight_updates(shapes_base):
    """The resident path's GEMMs multiply the same bf16 values as the hybrid one; it additionally runs the
    attention products on the bf16 pipe, so the two agree to bf16 accuracy.  Its bf16 weight mirror
    follows both torch-side writes (load_state_dict) and FusedAdam steps."""
    from meme_challenge_amd.trainer import bce_with_logits_loss, FusedAdam
    from meme_challenge_amd.utils import make_synthetic_batch
    z = shapes_base
    sd = O.synth_state_dict(BASE, seed=0, ln_jitter=0.02)
    B, T, R, seed = z['cfg1_full/shape'].tolist()
    b = make_synthetic_batch(B, T, R, seed=seed, device='cuda')
    out = {}
    for mode in ('bf16_hybrid', 'bf16'):
        m = build(BASE, 2048, sd).eval()
        m.uniter_model.precision = mode
        opt = FusedAdam(m, lr=1e-3, weight_decay=0.0)
        logits0 = m(**model_kwargs(b))
        bce_with_logits_loss(logits0, b['labels'], 1.8).backward()
        g = m.uniter_model.encoder.layer[3].intermediate.dense.weight.grad.detach().clone()
        opt.step(grad_scale=1.0, max_grad_norm=5.0)
        with torch.no_grad():
            logits1 = m(**model_kwargs(b))                  # must see the updated weights
            m.load_state_dict(sd)
            logits2 = m(**model_kwargs(b))                  # and the restored ones
        out[mode] = (logits0.detach(), g, logits1, logits2)
    h, r = out['bf16_hybrid'], out['bf16']
    assert maxdiff(r[0], h[0]) < 5e-3
    assert maxdiff(r[1], h[1]) < 1e-6 + 5e-2 * h[1].abs().max().item()
    # one Adam step at lr 1e-3 moves the logits by ~4; Adam's sign-like update amplifies bf16-level gradient differences
    assert maxdiff(r[2], h[2]) < 0.1 and maxdiff(r[2], r[0]) > 1.0
    assert maxdiff(r[3], r[0]) < 1e-6


@pytest.mark.parametrize('B,T,R,tl,nbb,train', [
    (1, 1, 1, [1], [1], True),                        # smallest legal batch: one token, one region
    (2, 300, 20, [300, 37], [20, 3], True),           # joint length 320 > 256: streaming attention kernels
    (1, 500, 12, [500], [12], False),                 # positions up to max_position_embeddings = 512
    (3, 40, 36, [40, 2, 17], [36, 36, 1], True),      # ragged on both sides
])
@pytest.mark.parametrize('precision', FP32_MODES)
def test_edge_shapes_match_oracle(B, T, R, tl, nbb, train, precision):
    """Edge cases the reference's collate can produce: single-token samples, sequences beyond
    the LDS-resident attention kernels, the position table's end, heavy raggedness -- forward, loss and all
    gradients against the CPU oracle on the same weights (dropout masks replayed in train mode)."""
    from meme_challenge_amd.trainer import bce_with_logits_loss
    CFG = dict(TINY, max_position_embeddings=512)
    sd = O.synth_state_dict(CFG, seed=3, img_dim=TINY_IMG_DIM, ln_jitter=0.05)
    b = O.synth_batch(B, T, R, seed=17, vocab=CFG['vocab_size'], img_dim=TINY_IMG_DIM, txt_lens=tl, num_bbs=nbb)
    m = build(CFG, TINY_IMG_DIM, sd, precision)         # fp32x3: x3 attention up to L = 192, the fp32-MFMA kernels beyond
    m = m.train() if train else m.eval()
    seed, offset = 0xC0FFEE, 4
    m.uniter_model.set_dropout_seed(seed, offset)
    logits = m(**model_kwargs(to_dev(b)))
    loss = bce_with_logits_loss(logits, b['labels'].cuda(), 1.8)
    loss.backward()
    torch.cuda.synchronize()
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    drop = O.DropSpec(seed, offset, CFG['hidden_dropout_prob'], CFG['attention_probs_dropout_prob']) if train else None
    lo = O.meme_uniter_forward(sdo, CFG, drop=drop, **model_kwargs(b))
    assert maxdiff(logits, lo) < 2e-5
    S.bce_with_logits(lo, b['labels'], 1.8).backward()
    for n, p in m.named_parameters():
        ref = sdo[n].grad if sdo[n].grad is not None else torch.zeros_like(sdo[n])
        tol = 3e-6 + 3e-4 * ref.abs().max().item()
        assert maxdiff(p.grad, ref) <= tol, (n, maxdiff(p.grad, ref), tol)


# packed in eval only: in train mode the packed layout draws the encoder's dropout masks by packed row, not by the padded
# (b * L + j) index the oracle replays
@pytest.mark.parametrize('types,packed,train', [(t, False, tr) for t in ('txt', 'img', 'both') for tr in (True, False)]
                         + [('txt', True, False)])
@pytest.mark.parametrize('precision', FP32_MODES)
def test_explicit_token_types_match_oracle(types, packed, train, precision):
    """txt_type_ids / img_type_ids passed explicitly (UniterModel.forward's optional arguments): explicit ids take the atomic
    scatter into the token-type table's gradient instead of the per-block partials and finalize the implicit ids take (text:
    row 0, image: row 1).  Each side mixes 0 and 1, so with one side explicit and the other implicit the atomics land on the row
    the other branch finalizes -- the two branches must not run unordered then.  Logits and every gradient against the oracle."""
    from meme_challenge_amd.trainer import bce_with_logits_loss
    B, T, R, tl, nbb = 3, 12, 8, [12, 5, 9], [8, 8, 3]
    sd = O.synth_state_dict(TINY, seed=5, img_dim=TINY_IMG_DIM, ln_jitter=0.05)
    b = O.synth_batch(B, T, R, seed=23, vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM, txt_lens=tl, num_bbs=nbb)
    g = torch.Generator().manual_seed(29)
    tt = {}
    if types in ('txt', 'both'):
        tt['txt_type_ids'] = torch.randint(0, 2, (B, T), generator=g)
        tt['txt_type_ids'][:, :2] = torch.tensor([0, 1])
    if types in ('img', 'both'):
        tt['img_type_ids'] = torch.randint(0, 2, (B, R), generator=g)
        tt['img_type_ids'][:, :2] = torch.tensor([1, 0])
    m = build(TINY, TINY_IMG_DIM, sd, precision)
    m = m.train() if train else m.eval()
    m.uniter_model.pack_padded = packed
    seed, offset = 0xBADC0DE, 6
    m.uniter_model.set_dropout_seed(seed, offset)
    kw = dict(model_kwargs(to_dev(b)), **{k: v.cuda() for k, v in tt.items()})
    if packed:
        kw['seq_lens'] = [a + c for a, c in zip(tl, nbb)]
    logits = m(**kw)
    loss = bce_with_logits_loss(logits, b['labels'].cuda(), 1.8)
    loss.backward()
    torch.cuda.synchronize()
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    drop = O.DropSpec(seed, offset, TINY['hidden_dropout_prob'], TINY['attention_probs_dropout_prob']) if train else None
    lo = O.meme_uniter_forward(sdo, TINY, drop=drop, **model_kwargs(b), **tt)
    assert maxdiff(logits, lo) < 2e-5
    S.bce_with_logits(lo, b['labels'], 1.8).backward()
    for n, p in m.named_parameters():
        ref = sdo[n].grad if sdo[n].grad is not None else torch.zeros_like(sdo[n])
        tol = 3e-6 + 3e-4 * ref.abs().max().item()
        assert maxdiff(p.grad, ref) <= tol, (n, maxdiff(p.grad, ref), tol)
    gt = sdo['uniter_model.embeddings.token_type_embeddings.weight'].grad
    assert gt[0].abs().max() > 0 and gt[1].abs().max() > 0            # both rows of the type table receive gradient


@pytest.mark.parametrize('train', [True, False])
def test_backward_of_a_stale_forward_fails_loudly(tiny, train):
    """The library keeps the activations of ONE forward per model: backpropagating through an earlier forward after
    another one has run must raise (train mode AND eval-with-grad), never return the other forward's gradients."""
    from meme_challenge_amd._lib import UniterHipError
    from meme_challenge_amd.trainer import bce_with_logits_loss
    sd = sd_from_npz(tiny)
    m = build(TINY, TINY_IMG_DIM, sd)
    m = m.train() if train else m.eval()
    b = to_dev(batch_from_npz(tiny))
    first = bce_with_logits_loss(m(**model_kwargs(b)), b['labels'], 1.8)
    second = bce_with_logits_loss(m(**model_kwargs(b)), b['labels'], 1.8)
    with pytest.raises(UniterHipError):
        first.backward()
    second.backward()                      # the latest forward still backpropagates
    with torch.no_grad():
        m(**model_kwargs(b))               # no-grad forwards in between do count (they overwrite the plan) ...
    third = bce_with_logits_loss(m(**model_kwargs(b)), b['labels'], 1.8)
    third.backward()                       # ... and a fresh forward works again


@pytest.mark.parametrize('env', [{'UNITER_WGRAD_GROUP_F32': '1'}, {'UNITER_WGRAD_WHOLE': '0', 'UNITER_LAZY_ZERO': '0'},
                                 {'UNITER_KEEP_PREGEN': '0', 'UNITER_ADAM_WORD_SPLIT': '0', 'UNITER_WGRAD_GROUP_F32': '0', 'UNITER_ATTN_BWD_FUSED': '0',
                                  'UNITER_ADAM_EMB_MAIN': '0'},
                                 {'UNITER_ATTN_X3': '0', 'UNITER_X3_CFG': '2'}, {'UNITER_DCTX_SPLIT': '0', 'UNITER_X3_CFG': '1'},
                                 {'UNITER_X3_BALANCED': '3'}])
def test_alternative_schedules_keep_the_golden_gradients(env):
    """The switches that select another form of the same arithmetic (the layer's weight gradients as one grouped whole-K
    launch; the stream-K form with a clearing zero_grad; dropout flags drawn inside the attention kernels, the embeddings'
    optimizer block in one launch on the side stream, the attention backward as two launches; in the fp32x3 form: attention on the
    fp32 MFMAs, the other wave geometries / MFMA shape of the x3 products, the attention-output input gradient as one tensor, the balanced walk of the
    128 x 256-tile launches) are read once per process: the reference-golden gradient, dropout-replay and trainer-step
    tests run again in a child process with the switch set."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider',
                        'tests/test_model_gpu.py::test_tiny_loss_and_all_grads_match_reference_golden',
                        'tests/test_model_gpu.py::test_base_logits_and_grads_match_reference_golden',
                        'tests/test_model_gpu.py::test_train_mode_dropout_replay_matches_oracle',
                        'tests/test_trainer_gpu.py::test_trainer_steps_match_reference'],
                       cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]


def test_alternative_bf16_schedules_keep_parity():
    """The bf16 mode's switches (the grouped weight-gradient launch with one workgroup per tile instead of 256 walking
    workgroups, the attention backward as two launches, stream-K weight gradients instead of the grouped launch): the bf16
    parity and lazy-zero tests run again in a child process with each set."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env in ({'UNITER_WGRAD_GROUP_WGS': '0', 'UNITER_ATTN_BWD_FUSED': '0'}, {'UNITER_WGRAD_GROUP': '0'}):
        r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider',
                            'tests/test_model_gpu.py::test_bf16_mfma_mode_tracks_fp32_reference',
                            'tests/test_trainer_gpu.py::test_lazy_zero_grad_overwrite_equals_clearing'],
                           cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-2000:])
        assert ' passed' in r.stdout and 'failed' not in r.stdout, (env, r.stdout[-500:])


def test_launch_stamps_put_the_gemms_on_one_clock(tiny):
    """uniter_prof_enable_stamps + uniter_prof_stamp_spans (measurement only): with stamps on, a forward + backward leaves
    one [start, end] interval per GEMM launch, in launch order, on the GPU's own clock -- forward kinds first, each interval
    non-empty, forward GEMMs strictly one after the other (they share a stream), everything inside a sane span."""
    import ctypes as C
    from meme_challenge_amd import _lib
    from meme_challenge_amd.trainer import bce_with_logits_loss
    m = build(TINY, TINY_IMG_DIM, sd_from_npz(tiny)).train()
    b = to_dev(batch_from_npz(tiny))
    enc = m.uniter_model
    bce_with_logits_loss(m(**model_kwargs(b)), b['labels'], 1.8).backward()      # builds the handle
    lib = _lib.lib()
    _lib.check(lib.uniter_prof_enable_stamps(enc._handle, 1, None))
    bce_with_logits_loss(m(**model_kwargs(b)), b['labels'], 1.8).backward()
    cap = 512
    kinds, t0, t1, n = (C.c_int * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), C.c_int(0)
    _lib.check(lib.uniter_prof_stamp_spans(enc._handle, kinds, t0, t1, cap, C.byref(n)))
    _lib.check(lib.uniter_prof_enable_stamps(enc._handle, 0, None))
    spans = [(kinds[i], t0[i], t1[i]) for i in range(n.value)]
    nl = TINY['num_hidden_layers']
    fwd = [s for s in spans if s[0] in (1, 2, 3, 4)]
    assert len(fwd) == 4 * nl and spans[:len(fwd)] == fwd                        # QKV, attention output, FFN up, FFN down per layer
    assert sum(1 for s in spans if s[0] == 6) == 4 * nl                          # input gradients
    assert sum(1 for s in spans if s[0] == 7) >= 1                               # weight gradients (grouped or one by one)
    assert spans[0][1] == 0.0 and all(0.0 <= a < e < 1e6 for _, a, e in spans)
    assert all(x[2] <= y[1] for x, y in zip(fwd, fwd[1:]))


@pytest.mark.parametrize('precision', ['fp32x3', 'bf16'])
def test_cu_reserve_for_a_gradient_exchange_changes_no_result(precision):
    """uniter_model_set_cu_reserve (dp.attach sets UniterModel.cu_reserve): with 16 CUs left to a gradient exchange's kernels the
    backward pass plans its k-pieces and tile geometry for 240 CUs (uniter_gemm_x3_plan) -- different slabs, a workspace sized
    for them, the same gradients to fp32 round-off; the forward pass keeps every CU and its output bit for bit."""
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.utils import make_synthetic_batch
    from meme_challenge_amd.trainer import bce_with_logits_loss
    cfg = UniterConfig.from_dict(BASE)
    torch.manual_seed(0)
    m = MemeUniter(UniterModel(cfg, img_dim=2048), cfg.hidden_size, 1).cuda().train()
    m.uniter_model.precision = precision
    b = make_synthetic_batch(16, 128, 36, seed=7, device='cuda')
    kw = dict(img_feat=b['img_feat'], img_pos_feat=b['img_pos_feat'], input_ids=b['input_ids'], position_ids=b['position_ids'],
              attention_mask=b['attn_mask'], gather_index=b['gather_index'], output_all_encoded_layers=False)
    names = ['uniter_model.encoder.layer.11.output.dense.weight', 'uniter_model.encoder.layer.5.attention.self.query.weight',
             'uniter_model.encoder.layer.0.intermediate.dense.bias', 'uniter_model.encoder.layer.0.attention.output.LayerNorm.weight',
             'uniter_model.embeddings.position_embeddings.weight']
    res = {}
    for reserve in (0, 16, 0):
        m.uniter_model.cu_reserve = reserve
        m.uniter_model.set_dropout_seed(11, 0)
        m.zero_grad(set_to_none=False)
        st = m.param_store(); st.zero_grads()
        logits = m(**kw)
        bce_with_logits_loss(logits.squeeze(1), b['labels'], 1.8).backward()
        torch.cuda.synchronize()
        params = dict(m.named_parameters())
        res.setdefault(reserve, []).append((logits.detach().clone(), {n: params[n].grad.detach().clone() for n in names}))
    (l0, g0), (l0b, g0b) = res[0]
    l16, g16 = res[16][0]
    assert torch.equal(l0, l16) and torch.equal(l0, l0b)
    for n in names:
        ref = g0[n]
        noise = (g0b[n] - ref).abs().max().item()          # two identical runs (float atomics in the embedding gradients)
        tol = (3e-3 if precision == 'bf16' else 2e-5) * ref.abs().max().item() + 4 * noise
        assert (g16[n] - ref).abs().max().item() <= tol, (n, (g16[n] - ref).abs().max().item(), tol)
