"""The encoder's configuration space: cases, float64 reference, bars and planted mutations (test infrastructure;
tests/test_config_space_cpu.py and tests/test_config_space_gpu.py share it).

What sits between the kernels and the user -- csrc/model.cpp's make_plan, gemm, linear, wgrad_group, head_rows_forward and the
backward layer -- decides by arithmetic on hidden_size H, intermediate_size I, img_dim and the layer count.  CONFIGS holds five
models the library accepts and no other test builds; each reaches branches the usual sizes (I a multiple of 256, img_dim of 64,
H = 64 * 2^k or 768, two or more layers) never do:

  h64_i96_l1      smallest H; I = 32 * 3: the fp32x3 weight mirror stays unpaired (ParamStore.pair_dst is None) and the head-rows
                  products run on one k-piece; layer 0 is also the last layer; three token types
  h128_i32        the FFN-down product is a single 32-deep k-tile
  h192_i320       H no power of two; I = 64 * 5; every precision legal
  h320_i100       I = 4 * 25: fp32 and bf16_hybrid only; img_dim >= 1024 but no multiple of 64
  h1024_i1056_l1  widest rows; I = 32 * 33; img_dim = 64 * 17 takes the split-K region projection in fp32; one layer

The reference is oracle/uniter_oracle.py (functional torch) fed a float64 state dict and float64 inputs: it then runs in float64,
dropout replay included, so the bars below hold the kernels and not the oracle's own float32 round-off
(tests/test_config_space_cpu.py measures that round-off against the same bars).

Bars.  fp32 and fp32x3: the project's own bars of tests/test_model_gpu.py (test_edge_shapes_match_oracle,
test_tiny_forward_matches_reference_golden), now against float64 -- logits and hidden states 2e-5, every gradient tensor
3e-6 + 3e-4 max|ref|; a tensor whose reference gradient is exactly zero must be exactly zero.  bf16 and bf16_hybrid: the two-sided
form of tests/test_parity_configs_gpu.py with its factors unchanged -- noise = the bf16-rounding oracle against float64; logits
within 2 noise + 2e-4; per tensor the rms-relative error eh <= fac * eo + slack (eo: the bf16 oracle's own); a key bias
(mathematically zero) within 0.2 of its query bias.  Everything is reported as a share of its bar (<= 1 passes).

Mutations.  Each plants one dispatcher error in the oracle: a dropped k-tail, a bias tail, the region projection's tail, the last
head of the value projection, the attention output's k-tail, the hidden dropout of the last layer drawn by compact row instead of
by the padded row (what csrc's LnCall::drop_row_step exists to prevent), one dropped k-slab of the FFN-down product.  The CPU test
shows that every one of them breaks the bars by a wide margin, so a kernel with that error could not pass.
"""
import functools

import numpy as np
import torch

from oracle import uniter_oracle as O
from oracle import step_oracle as S
from common import TINY, model_kwargs
from test_parity_configs_gpu import _two_sided_slack, _rms_rel

# id -> (overrides of the base configuration, img_dim)
CONFIGS = {
    'h64_i96_l1': (dict(hidden_size=64, num_attention_heads=1, intermediate_size=96, num_hidden_layers=1, type_vocab_size=3), 36),
    'h128_i32': (dict(hidden_size=128, num_attention_heads=2, intermediate_size=32, num_hidden_layers=2), 68),
    'h192_i320': (dict(hidden_size=192, num_attention_heads=3, intermediate_size=320, num_hidden_layers=2), 100),
    'h320_i100': (dict(hidden_size=320, num_attention_heads=5, intermediate_size=100, num_hidden_layers=2), 1028),
    'h1024_i1056_l1': (dict(hidden_size=1024, num_attention_heads=16, intermediate_size=1056, num_hidden_layers=1), 1088),
}
PRECISIONS = ('fp32', 'fp32x3', 'bf16', 'bf16_hybrid')
STATE_SEED, LN_JITTER = 3, 0.05
BATCH_SEED, VOCAB = 17, 61
B, T, R, TXT_LENS, NUM_BBS = 3, 11, 7, [11, 2, 6], [7, 7, 1]          # L = 18, M = 54: no multiple of 8 anywhere
DROP_SEED, DROP_OFFSET = 0xC0FFEE, 4
POS_WEIGHT = 1.8
LOGIT_BAR = LAYER_BAR = 2e-5


def cfg(name):
    return dict(TINY, max_position_embeddings=64, vocab_size=VOCAB, **CONFIGS[name][0])


def img_dim(name):
    return CONFIGS[name][1]


def legal(name, precision):
    """the setters' own rules (model.py _ensure_handle, uniter_model_set_precision)"""
    I = cfg(name)['intermediate_size']
    return {'fp32': True, 'bf16_hybrid': True, 'fp32x3': I % 32 == 0, 'bf16': I % 64 == 0}[precision]


LEGAL = [(n, p) for n in CONFIGS for p in PRECISIONS if legal(n, p)]
ILLEGAL = [(n, p) for n in CONFIGS for p in PRECISIONS if not legal(n, p)]


def pieces_for(K):
    """csrc/model.cpp make_plan: k-pieces of the head-rows products"""
    return min(max(K // 32 // 2, 1), 8)


def grad_bar(ref):
    return 3e-6 + 3e-4 * float(np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def state_dict(name):
    """float32 weights of the configuration; shared, never written"""
    return O.synth_state_dict(cfg(name), seed=STATE_SEED, img_dim=img_dim(name), ln_jitter=LN_JITTER)


@functools.lru_cache(maxsize=None)
def batch(name):
    b = O.synth_batch(B, T, R, seed=BATCH_SEED, vocab=VOCAB, img_dim=img_dim(name), txt_lens=TXT_LENS, num_bbs=NUM_BBS)
    assert b['attn_mask'].shape == (3, 18)
    return b


def seq_lens():
    return [t + r for t, r in zip(TXT_LENS, NUM_BBS)]


def drop_spec(name):
    c = cfg(name)
    return O.DropSpec(DROP_SEED, DROP_OFFSET, c['hidden_dropout_prob'], c['attention_probs_dropout_prob'])


# ------------------------------------------------------------------------------------------------ mutations ---
def _last(name):
    return 'uniter_model.encoder.layer.%d.' % (cfg(name)['num_hidden_layers'] - 1)


def _scale_cols(w, n, f=0.0):
    m = torch.ones_like(w)
    m[..., w.shape[-1] - n:] = f
    return w * m


def _scale_rows(w, n, f=0.0):
    m = torch.ones_like(w)
    m[w.shape[0] - n:] = f
    return w * m


def _tail(name):
    return cfg(name)['intermediate_size'] % 64 or 32


# mutation -> (state-dict key below the last layer's prefix or absolute, function of (tensor, configuration name))
_SD_MUTATIONS = {
    'ffn_down_ktail': ('L:output.dense.weight', lambda w, n: _scale_cols(w, _tail(n))),
    'ffn_up_bias_tail': ('L:intermediate.dense.bias', lambda w, n: _scale_cols(w, _tail(n))),
    'img_tail': ('uniter_model.img_embeddings.img_linear.weight', lambda w, n: _scale_cols(w, img_dim(n) % 64 or 4)),
    'last_head_v': ('L:attention.self.value.weight', lambda w, n: _scale_rows(w, 64)),
    'attn_out_ktail': ('L:attention.output.dense.weight', lambda w, n: _scale_cols(w, 32)),
    'kpiece': ('L:output.dense.weight', lambda w, n: w * 0.5),
}
MUTATIONS = tuple(_SD_MUTATIONS) + ('dropout_row',)


def applies(mutation, name, train=True):
    if mutation == 'kpiece':
        return pieces_for(cfg(name)['intermediate_size']) > 1
    if mutation == 'dropout_row':
        return train
    return True


def _mutated(sd, name, mutation):
    """the state dict the forward pass reads: the leaves of `sd` with the mutation between them and the products (gradients
    still arrive at the leaves)"""
    if mutation not in _SD_MUTATIONS:
        return sd
    key, fn = _SD_MUTATIONS[mutation]
    key = _last(name) + key[2:] if key.startswith('L:') else key
    out = dict(sd)
    out[key] = fn(sd[key], name)
    return out


def _wide(b, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.items()}


def _forward_dropout_row(sd, c, kw, drop, prec):
    """the forward pass with the last layer's two hidden-dropout sites drawn for row 0 of sample b at compact row b instead of
    padded row b * L (every other row as usual)"""
    nl, H = c['num_hidden_layers'], c['hidden_size']
    kw = dict(kw, output_all_encoded_layers=False)
    h = O.uniter_forward(sd, dict(c, num_hidden_layers=nl - 1), drop=drop, prefix='uniter_model.', prec=prec, **kw)
    Bn, L = kw['attention_mask'].shape
    idx = torch.arange(Bn * L * H, dtype=torch.int64).view(Bn, L, H).clone()
    idx[:, 0] = torch.arange(Bn, dtype=torch.int64).view(Bn, 1) * H + torch.arange(H, dtype=torch.int64).view(1, H)
    ext = (1.0 - kw['attention_mask'].unsqueeze(1).unsqueeze(2).to(torch.float32)) * -10000.0
    h = O.bert_layer(sd, 'uniter_model.encoder.layer.%d.' % (nl - 1), h, ext, c, drop, nl - 1, prec, idx)
    pooled = O.pooler(sd, 'uniter_model.', h)
    return torch.nn.functional.linear(pooled, sd['linear.weight'], sd['linear.bias'])


def _step(name, train, mutation, prec, dtype, weights=None):
    c = cfg(name)
    src = weights if weights is not None else state_dict(name)
    sd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in src.items()}
    b = _wide(batch(name), dtype)
    drop = drop_spec(name) if train else None
    fsd = _mutated(sd, name, mutation)
    if mutation == 'dropout_row':
        assert train
        logits = _forward_dropout_row(fsd, c, model_kwargs(b), drop, prec)
    else:
        logits = O.meme_uniter_forward(fsd, c, drop=drop, prec=prec, **model_kwargs(b))
    loss = S.bce_with_logits(logits, b['labels'], POS_WEIGHT)
    loss.backward()
    out = {'logits': logits.detach().double().numpy(), 'loss': float(loss.detach())}
    for n, v in sd.items():
        out['grad/' + n] = (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy()
    return out


@functools.lru_cache(maxsize=None)
def reference_step(name, train, mutation=None, prec='fp32', dtype=torch.float64):
    """One oracle step of the configuration: 'logits' [B, 1], 'loss', 'grad/<name>' for every parameter (zeros where autograd left
    none), float64 arrays.  prec 'fp32' with dtype float64 is THE reference; ('bf16', float32) is the bf16-rounding oracle,
    ('fp32', float32) the oracle as the other model tests use it.  Cached: callers must not write the arrays."""
    return _step(name, train, mutation, prec, dtype)


def reference_logits(name, weights, prec='fp32', dtype=torch.float64):
    """eval-mode logits on other weights ({name: tensor}), float64 array"""
    c = cfg(name)
    sd = {k: v.detach().to(dtype) for k, v in weights.items()}
    with torch.no_grad():
        return O.meme_uniter_forward(sd, c, prec=prec, **model_kwargs(_wide(batch(name), dtype))).double().numpy()


@functools.lru_cache(maxsize=None)
def reference_layers(name, prec='fp32', dtype=torch.float64):
    """every layer's hidden state in eval mode, [B, L, H] float64 arrays (padded positions as the oracle computes them)"""
    sd = {k: v.to(dtype) for k, v in state_dict(name).items()}
    kw = dict(model_kwargs(_wide(batch(name), dtype)), output_all_encoded_layers=True)
    with torch.no_grad():
        return [h.double().numpy() for h in O.uniter_forward(sd, cfg(name), prefix='uniter_model.', prec=prec, **kw)]


# ------------------------------------------------------------------------------------------------ bars ---
def fp32_shares(got, ref):
    """name -> |got - ref| as a share of the fp32 bar: logits 2e-5, a gradient 3e-6 + 3e-4 max|ref|, the loss pos_weight * 2e-5
    + 1e-6 (|d BCE / d logit| <= pos_weight in the batch mean, plus the float32 sum of a loss of order 1).  A gradient whose
    reference is exactly zero: 0 if exactly zero, inf otherwise."""
    out = {}
    for k, r in ref.items():
        if k == 'loss':
            out[k] = abs(float(got[k]) - r) / (POS_WEIGHT * LOGIT_BAR + 1e-6)
            continue
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if k.startswith('grad/') and not np.abs(r).max() > 0.0:
            out[k] = 0.0 if not np.abs(g).max() > 0.0 else float('inf')
            continue
        out[k] = float(np.abs(g - r).max()) / (grad_bar(r) if k.startswith('grad/') else LOGIT_BAR)
    return out


def _rms(a, b):
    return _rms_rel(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def bf16_noise(ref, orc):
    return float(np.abs(orc['logits'] - ref['logits']).max())


def bf16_shares(got, ref, orc):
    """The two-sided form of tests/test_parity_configs_gpu.py (_check_bf16_step_against_bf16_oracle) as shares of its bars:
    ref the float64 step, orc the bf16-rounding oracle's.  logits: max|got - ref| / (2 noise + 2e-4); the loss alike on its own
    noise; a gradient: eh / (fac eo + slack) with _two_sided_slack's factors; a key bias: max|g| / (0.2 max|query bias| + 1e-12);
    an exactly zero reference gradient as in fp32_shares.  Returns (shares, ratios eh / eo of the ordinary tensors)."""
    out, ratios = {}, []
    out['logits'] = float(np.abs(np.asarray(got['logits'], dtype=np.float64) - ref['logits']).max()) / (2.0 * bf16_noise(ref, orc) + 2e-4)
    out['loss'] = abs(float(got['loss']) - ref['loss']) / (2.0 * abs(orc['loss'] - ref['loss']) + 2e-4)
    for k, r in ref.items():
        if not k.startswith('grad/'):
            continue
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if k.endswith('attention.self.key.bias'):
            qb = np.asarray(got[k.replace('key.bias', 'query.bias')], dtype=np.float64)
            out[k] = float(np.abs(g).max()) / (0.2 * float(np.abs(qb).max()) + 1e-12)
            continue
        if not np.abs(r).max() > 0.0:
            out[k] = 0.0 if not np.abs(g).max() > 0.0 else float('inf')
            continue
        eh, eo = _rms(g, r), _rms(orc[k], r)
        fac, slack = _two_sided_slack(k[len('grad/'):], g.size)
        out[k] = eh / (fac * eo + slack)
        ratios.append(eh / max(eo, 1e-30))
    return out, ratios


def worst(shares, prefix=''):
    """(share, name) of the largest share among the names with the prefix"""
    return max((v, k) for k, v in shares.items() if k.startswith(prefix))
