"""Float64 reference of the attention kernels (csrc/attention_f32.hip, attention_x3.hip, attention_bf16.hip), per-element error bounds for
an fp32 evaluation, and the case lists tests/test_attn_bounds_cpu.py (CPU) and tests/test_attention_f64_gpu.py (GPU) share.  Plain
numpy / torch on the CPU: no GPU, no library.

The reference takes the fp32 INPUT VALUES the kernel gets, widened to float64, one (sample, head) at a time:

    bias_j = (1 - mask_j) * -10000             additive and finite (model/model.py:345); a packed sample has no mask: bias = 0
    m_ij   in {0, fp32(1) / fp32(1 - p)}       oracle.philox.keep_mask at element ((b nh + h) L + i) Lp + j, Lp = ceil4(L); in a packed
                                               batch L is Lmax
    s_ij   = q_i . k_j / 8 + bias_j
    lse_i  = log sum_j exp(s_ij),  p_ij = exp(s_ij - lse_i),  ctx_i = sum_j p_ij m_ij v_j

The backward reference takes ctx_in and lse_in as INPUTS, as the C ABI does: it is the exact function of those fp32 values, whoever
computed them, so a forward error cannot hide a backward one (p_ij = exp(s_ij - lse_in_i), which need not sum to 1):

    delta_i = sum_d ctx_in_id dO_id,  dP_ij = dO_i . v_j,  g_ij = dP_ij m_ij - delta_i,  dS_ij = p_ij g_ij
    dQ_i = sum_j dS_ij k_j / 8,  dK_j = sum_i dS_ij q_i / 8,  dV_j = sum_i p_ij m_ij dO_i
    bias_part[b] = column sums of sample b's dqkv rows: ALL L rows in the mask form (a padded query is an ordinary query there),
                   the sample's own rows in the packed form

Bounds.  U = 2^-24 (half an ulp, relative), a_ij = sum_d |q_id k_jd| / 8, T = 2^-126 (the smallest normal fp32 number):

    E_s     = U (A_S a_ij + |s_ij| + |bias_j|)       the dot product relative to its absolute terms; the roundings of the scaled sum
                                                     and of the addition of the bias relative to the larger of the two
    E_lse   = sum_j p_ij E_s_ij + U (A_L max(1, |lse_i|, |max_j s_ij|) + B_L)
                                                     the scores' errors reach lse through the softmax weights; m + log(l) is rounded
                                                     relative to the larger operand; the relative error of l (each exp, the summation
                                                     order, the alpha rescalings) becomes an absolute one through the log
    E_p     = p_ij expm1(E_s_ij + E_lse_i + A_P U (1 + |s_ij - lse_i|)) + T
                                                     the argument's error is a relative error of exp; the fast exponential evaluates
                                                     exp2(x log2 e), whose product is rounded relative to |x|.  T: a probability below
                                                     the normal range is flushed to 0 (or keeps fewer bits), e.g. p = e^-104
    E_ctx   = sum_j E_p m_ij |v_j| + A_O U sum_j p_ij m_ij |v_j|
    backward: E_p carries U |lse_in_i| (the rounding of s - lse_in) in place of E_lse
    E_delta = A_D U sum_d |ctx_in dO|
    E_dP    = A_S U sum_d |dO_id v_jd|
    E_dS    = E_p |g| + p (E_dP m + E_delta + U (|dP m| + |delta|)) + U |dS| + T
    E_dQ    = (sum_j E_dS |k_j| + A_O U sum_j |dS k_j|) / 8         (dK likewise, over i with q_i)
    E_dV    = sum_i E_p m |dO_i| + A_O U sum_i p m |dO_i|
    bias_part: sum_rows E + A_B U sum_rows |dqkv|
  A backward pass CHAINED to a device forward gets ctx and lse that are off by up to E_ctx + U |ctx| and E_lse + U |lse| from the
  values the reference was given: E_delta gains sum_d (E_ctx + U |ctx|) |dO| and E_p's exponent gains E_lse + U |lse|.
  Where a bound is 0 the result must be exact (gemm_ref.worst_ratio).

Constants.  They are not fitted to the kernels.  tests/test_attn_bounds_cpu.py evaluates the same formulas in numpy fp32 twice, independently
written -- a two-pass softmax with serial sums, and a blocked online softmax over 32-key chunks whose products are six bf16-piece
products -- over every case list below; each constant is at least twice the worst share either reaches.  The starting values
A_S = 8, A_P = 4, A_O = 8, A_L = 4, B_L = 8, A_D = 8, A_B = 8 sat on that rule's edge: at a common offset of -350 (SCORES, `offset-`)
dQ reached 0.496 and lse 0.384 here (0.53 for lse in an evaluation with another summation order).  Both shares rest on A_S -- doubling
B_L moves lse by 0.002, doubling A_S takes it to 0.238: with q += 50 u, k -= 50 u one term of the 64-term dot product is -2500, every
later addition of a serial sum rounds relative to it, and the error walks ~sqrt(63) U a = 7.9 U a against A_S = 8.  A_S = 16 is twice
that walk (the worst case of a serial sum is 64 U a).  Final constants:

    A_S = 16, A_P = 4, A_O = 8, A_L = 4, B_L = 8, A_D = 8, A_B = 8

and the worst shares the two evaluations reach with them (two-pass | blocked), each on the case named:

    ctx        0.129 | 0.120   SCORES p = 0 (`offset-`)
    lse        0.238 | 0.207   SCORES p = 0 (`offset-`)
    dq         0.278 | 0.234   SCORES (`offset-`)
    dk         0.181 | 0.138   SCORES p = 0
    dv         0.201 | 0.174   SCORES
    delta      0.461 | 0.203   LENGTHS L = 33 (a serial 64-term sum that cancels) | PACKED p = 0
    bias_part  0.145 | 0.155   SCORES p = 0 (q = 0, one-hot V)"""
import functools

import numpy as np
import torch

from oracle import philox

F = np.float32
D = np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
A_S, A_P, A_O, A_L, B_L, A_D, A_B = 16.0, 4.0, 8.0, 4.0, 8.0, 8.0, 8.0
HD = 64
SEED, OFFSET, SITE = 0xABCDEF0123, 5, 2


# ---------------------------------------------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------------------------------------------
class Call:
    """one library call: qkv [rows, 3 H] and dO [rows, H] fp32, and either mask [B, L] (0 / 1) or lens (packed: rows of sample b
    follow those of sample b - 1, L = max(lens))"""

    def __init__(self, name, nh, p, qkv, dO, mask=None, lens=None):
        self.name, self.nh, self.p, self.H = name, nh, float(p), nh * HD
        self.qkv, self.dO = np.ascontiguousarray(qkv, dtype=F), np.ascontiguousarray(dO, dtype=F)
        self.packed = lens is not None
        if self.packed:
            self.lens = [int(n) for n in lens]
            self.B, self.L, self.mask = len(lens), max(lens), None
            self.cu = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        else:
            self.mask = np.ascontiguousarray(mask, dtype=F)
            self.B, self.L = self.mask.shape
            self.lens = [self.L] * self.B
            self.cu = (np.arange(self.B + 1) * self.L).astype(np.int32)
        self.rows = int(self.cu[-1])
        assert self.qkv.shape == (self.rows, 3 * self.H) and self.dO.shape == (self.rows, self.H)

    def __repr__(self):
        return 'Call(%s)' % self.name

    def valid_pos(self):
        """bool [B, nh, L]: the positions of lse / delta that belong to a sample"""
        v = np.zeros((self.B, self.nh, self.L), dtype=bool)
        for b, n in enumerate(self.lens):
            v[b, :, :n] = True
        return v


def keep_mult(call, lp=None, transposed=False, scaled=True):
    """float64 [B, nh, L, L]: 0 or fp32(1) / fp32(1 - p).  lp / transposed / scaled are the handles of the CPU test's mutations."""
    B, nh, L, p = call.B, call.nh, call.L, call.p
    if p <= 0.0:
        return np.ones((B, nh, L, L), dtype=D)
    Lp = (L + 3) // 4 * 4 if lp is None else lp
    i, j = (np.arange(L)[None, :], np.arange(L)[:, None]) if transposed else (np.arange(L)[:, None], np.arange(L)[None, :])
    idx = (np.arange(B * nh).reshape(B, nh, 1, 1) * L + i[None, None]) * Lp + j[None, None]
    keep = philox.keep_mask(int(idx.max()) + 1, p, SEED, OFFSET, SITE)[idx]
    return keep.astype(D) * (float(F(1.0) / F(1.0 - p)) if scaled else 1.0)


def heads(x, nh):
    """[n, nh * 64] -> [nh, n, 64]"""
    return np.ascontiguousarray(x.reshape(x.shape[0], nh, HD).transpose(1, 0, 2))


def unheads(x):
    """[nh, n, 64] -> [n, nh * 64]"""
    return np.ascontiguousarray(x.transpose(1, 0, 2).reshape(x.shape[1], -1))


def samples(call, **keep_args):
    """yields (b, row0, n, q, k, v, dO [nh, n, 64] fp32, bias [n] fp32, m [nh, n, n] float64) per sample"""
    km = keep_mult(call, **keep_args)
    H = call.H
    for b, n in enumerate(call.lens):
        r0 = int(call.cu[b])
        x = call.qkv[r0:r0 + n]
        q, k, v = (heads(x[:, t * H:(t + 1) * H], call.nh) for t in range(3))
        bias = np.zeros(n, dtype=F) if call.packed else ((F(1.0) - call.mask[b]) * F(-10000.0)).astype(F)
        yield b, r0, n, q, k, v, heads(call.dO[r0:r0 + n], call.nh), bias, km[b, :, :n, :n]


# ---------------------------------------------------------------------------------------------------------------------------
# the reference, one sample (all heads) at a time
# ---------------------------------------------------------------------------------------------------------------------------
def _scores(q, k, bias):
    s = np.einsum('hid,hjd->hij', q, k) / 8.0 + bias[None, None, :]
    a = np.einsum('hid,hjd->hij', np.abs(q), np.abs(k)) / 8.0
    return s, U * (A_S * a + np.abs(s) + np.abs(bias)[None, None, :])


def forward_sample(q, k, v, bias, m):
    q, k, v, bias = (np.asarray(t, dtype=D) for t in (q, k, v, bias))
    s, E_s = _scores(q, k, bias)
    mx = s.max(-1)
    lse = mx + np.log(np.exp(s - mx[..., None]).sum(-1))
    p = np.exp(s - lse[..., None])
    E_lse = (p * E_s).sum(-1) + U * (A_L * np.maximum(1.0, np.maximum(np.abs(lse), np.abs(mx))) + B_L)
    E_p = p * np.expm1(E_s + E_lse[..., None] + A_P * U * (1.0 + np.abs(s - lse[..., None]))) + TINY
    pm = p * m
    ctx = pm @ v
    E_ctx = (E_p * m) @ np.abs(v) + A_O * U * (pm @ np.abs(v))
    return dict(ctx=ctx, lse=lse, E_ctx=E_ctx, E_lse=E_lse)


def backward_sample(q, k, v, bias, m, dO, ctx_in, lse_in, E_ctx=None, E_lse=None):
    """dq, dk, dv, delta with their bounds; given the forward bounds also the bounds of a pass chained to a device forward (`_ch`)"""
    q, k, v, bias, dO, ctx_in, lse_in = (np.asarray(t, dtype=D) for t in (q, k, v, bias, dO, ctx_in, lse_in))
    s, E_s = _scores(q, k, bias)
    x = s - lse_in[..., None]
    p = np.exp(x)
    delta = (ctx_in * dO).sum(-1)
    dP = dO @ v.transpose(0, 2, 1)
    E_dP = A_S * U * (np.abs(dO) @ np.abs(v).transpose(0, 2, 1))
    g = dP * m - delta[..., None]
    dS = p * g
    pm = p * m
    out = dict(dq=dS @ k / 8.0, dk=dS.transpose(0, 2, 1) @ q / 8.0, dv=pm.transpose(0, 2, 1) @ dO, delta=delta)
    sets = [('', U * np.abs(lse_in), A_D * U * np.abs(ctx_in * dO).sum(-1))]
    if E_ctx is not None:
        sets.append(('_ch', sets[0][1] + E_lse + U * np.abs(lse_in), sets[0][2] + ((E_ctx + U * np.abs(ctx_in)) * np.abs(dO)).sum(-1)))
    for tag, e_l, E_delta in sets:
        E_p = p * np.expm1(E_s + e_l[..., None] + A_P * U * (1.0 + np.abs(x))) + TINY
        E_dS = (E_p * np.abs(g) + p * (E_dP * m + E_delta[..., None] + U * (np.abs(dP * m) + np.abs(delta)[..., None]))
                + U * np.abs(dS) + TINY)
        out['E_dq' + tag] = (E_dS @ np.abs(k) + A_O * U * (np.abs(dS) @ np.abs(k))) / 8.0
        out['E_dk' + tag] = (E_dS.transpose(0, 2, 1) @ np.abs(q) + A_O * U * (np.abs(dS).transpose(0, 2, 1) @ np.abs(q))) / 8.0
        out['E_dv' + tag] = (E_p * m).transpose(0, 2, 1) @ np.abs(dO) + A_O * U * (pm.transpose(0, 2, 1) @ np.abs(dO))
        out['E_delta' + tag] = E_delta
    return out


def assemble(call, per_sample, bias_rows='all'):
    """per-sample results ({name: [nh, n, 64] or [nh, n]}, in sample order) -> the library's layouts: [rows, H] / [rows, 3 H] (dq | dk |
    dv joined as dqkv) / [B, nh, L] (positions beyond a packed sample's length: NaN).  With dqkv present also bias_part [B, 3 H] (and,
    for a reference, its bound from E_dqkv)."""
    out = {}
    for (b, n), res in zip(enumerate(call.lens), per_sample):
        r0 = int(call.cu[b])
        for name, val in res.items():
            if val.ndim == 3:
                out.setdefault(name, np.zeros((call.rows, call.H), dtype=val.dtype))[r0:r0 + n] = unheads(val)
            else:
                out.setdefault(name, np.full((call.B, call.nh, call.L), np.nan, dtype=val.dtype))[b, :, :n] = val
    for tag in ('', '_ch'):
        for pre in ('', 'E_'):
            names = [pre + t + tag for t in ('dq', 'dk', 'dv')]
            if all(t in out for t in names):
                out[pre + 'dqkv' + tag] = np.concatenate([out.pop(t) for t in names], axis=1)
    if 'dqkv' in out:
        for tag in ('', '_ch'):
            if tag and 'E_dqkv' + tag not in out:
                continue
            part, E_part = (np.zeros((call.B, 3 * call.H), dtype=out['dqkv'].dtype) for _ in range(2))
            for b, n in enumerate(call.lens):
                r0 = int(call.cu[b])
                rows = slice(r0, r0 + n)
                if bias_rows == 'valid' and not call.packed:
                    rows = r0 + np.nonzero(call.mask[b])[0]
                x = out['dqkv'][rows]
                part[b] = serial_sum(x) if x.dtype == F else x.sum(0)
                if 'E_dqkv' + tag in out:
                    E_part[b] = out['E_dqkv' + tag][rows].sum(0) + A_B * U * np.abs(x).sum(0)
            if not tag:
                out['bias_part'] = part
            if 'E_dqkv' + tag in out:
                out['E_bias_part' + tag] = E_part
    return out


def serial_sum(x):
    """fp32 sum over axis 0, one row after the other"""
    acc = np.zeros(x.shape[1:], dtype=F)
    for r in range(x.shape[0]):
        acc = acc + x[r]
    return acc


_REF_CACHE = {}


def reference(call):
    """everything the tests compare, computed once per call: ctx, lse, dqkv, delta, bias_part, their bounds E_*, the chained
    bounds E_*_ch, and ctx_in / lse_in (fp32: what the judged backward run is given)"""
    if call.name in _REF_CACHE:
        return _REF_CACHE[call.name]
    fw, bw = [], []
    for b, r0, n, q, k, v, dO, bias, m in samples(call):
        f = forward_sample(q, k, v, bias, m)
        ctx_in, lse_in = f['ctx'].astype(F), f['lse'].astype(F)
        bw.append(backward_sample(q, k, v, bias, m, dO, ctx_in, lse_in, f['E_ctx'], f['E_lse']))
        fw.append(dict(f, ctx_in=ctx_in, lse_in=lse_in))
    out = dict(assemble(call, fw), **assemble(call, bw))
    _REF_CACHE[call.name] = out
    return out


OUTPUTS_FWD = ('ctx', 'lse')
OUTPUTS_BWD = ('dq', 'dk', 'dv', 'delta', 'bias_part')


def shares(call, ref, got, chained=False, names=None):
    """{output: worst |got - ref| / bound} over the positions that belong to a sample; got in the library's layouts"""
    from gemm_ref import worst_ratio
    H, tag = call.H, '_ch' if chained else ''
    valid = call.valid_pos()
    out = {}
    for name in names or got:
        if name in ('dq', 'dk', 'dv'):
            sl = slice(('dq', 'dk', 'dv').index(name) * H, (('dq', 'dk', 'dv').index(name) + 1) * H)
            out[name] = worst_ratio(got['dqkv'][:, sl], ref['dqkv'][:, sl], ref['E_dqkv' + tag][:, sl])
        elif name in ('lse', 'delta'):
            e = ref['E_' + name + (tag if name == 'delta' else '')]
            out[name] = worst_ratio(np.asarray(got[name])[valid], ref[name][valid], e[valid])
        elif name == 'bias_part':
            out[name] = worst_ratio(got[name], ref[name], ref['E_bias_part' + tag])
        elif name == 'ctx':
            out[name] = worst_ratio(got[name], ref[name], ref['E_ctx'])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------------------
def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy()


def _operands(seed, B, L, nh):
    """qkv as [B, L, 3, nh, 64] and dO as [B, L, nh, 64]: seeded randn"""
    return _randn(seed, B, L, 3, nh, HD), _randn(seed + 1, B, L, nh, HD)


def _flat(x5, d4):
    B, L = x5.shape[:2]
    return x5.reshape(B * L, -1), d4.reshape(B * L, -1)


MASK_NAMES = ('ones', 'right-pad-40', 'model-layout', 'chunk1-masked', 'chunk0-masked', 'only-163', 'only-0', 'alternating', 'zeros')
MASK_L = 164


def mask_patterns():
    L = MASK_L
    m = np.zeros((len(MASK_NAMES), L), dtype=F)
    m[0] = 1
    m[1, :L - 40] = 1
    m[2, :20] = 1; m[2, 128:158] = 1                  # [20 valid | 108 pad | 30 valid | 6 pad]
    m[3] = 1; m[3, 32:64] = 0
    m[4] = 1; m[4, 0:32] = 0
    m[5, 163] = 1
    m[6, 0] = 1
    m[7, 0::2] = 1
    return m


@functools.lru_cache(maxsize=None)
def masks_call(p, patterns=None):
    """MASKS: one call, L = 164, nh = 2, one sample per pattern (`patterns`: a tuple of MASK_NAMES to keep)"""
    m = mask_patterns()
    names = MASK_NAMES if patterns is None else patterns
    m = m[[MASK_NAMES.index(t) for t in names]]
    x, d = _operands(100, len(MASK_NAMES), MASK_L, 2)
    sel = [MASK_NAMES.index(t) for t in names]
    qkv, dO = _flat(x[sel], d[sel])
    left_out = [t for t in MASK_NAMES if t not in names]
    return Call('masks-p%g%s' % (p, ''.join('-no-' + t for t in left_out)), 2, p, qkv, dO, mask=m)


SCORE_NAMES = ('randn', 'x4', 'x10', 'offset+', 'offset-', 'q0-onehot-v', 'one-key-ahead', 'v-2^20')
SCORE_L = 100


@functools.lru_cache(maxsize=None)
def scores_call(p):
    """SCORES: one call, L = 100, nh = 1, one sample per regime"""
    L = SCORE_L
    x, d = _operands(200, len(SCORE_NAMES), L, 1)
    u = _randn(202, HD).astype(D)
    u = (u / np.sqrt((u * u).sum())).astype(F)
    x[1, :, 0:2] *= 4
    x[2, :, 0:2] *= 10
    x[3, :, 0] += 50 * u; x[3, :, 1] += 50 * u
    x[4, :, 0] += 50 * u; x[4, :, 1] -= 50 * u
    x[5, :, 0] = 0
    x[5, :, 2] = one_hot_v(L)[:, None, :]
    x[6, :, 0] += 30 * u
    x[6, 17, 1] = 60 * u
    x[7, :, 2] *= 2.0 ** 20
    d[7] *= 2.0 ** -20
    s = np.einsum('id,jd->ij', x[6, :, 0, 0].astype(D), x[6, :, 1, 0].astype(D)) / 8.0
    assert (s[:, 17] - np.delete(s, 17, axis=1).max(1)).min() > 104.0, 'one key must lead by more than 104'
    qkv, dO = _flat(x, d)
    return Call('scores-p%g' % p, 1, p, qkv, dO, mask=np.ones((len(SCORE_NAMES), L), dtype=F))


def one_hot_v(L):
    v = np.zeros((L, HD), dtype=F)
    v[np.arange(L), np.arange(L) % HD] = 1
    return v


LENGTHS = (1, 15, 16, 17, 31, 32, 33, 64, 65, 96, 97, 160, 161, 191, 192)
LONG = (193, 224, 255, 256, 257, 288, 320, 321)


@functools.lru_cache(maxsize=None)
def length_call(L, p, nh=2):
    """LENGTHS and LONG: B = 2, sample 1 right-padded by 7 % L"""
    x, d = _operands(300 + L, 2, L, nh)
    m = np.ones((2, L), dtype=F)
    if 7 % L:
        m[1, L - 7 % L:] = 0
    qkv, dO = _flat(x, d)
    return Call('len%d-nh%d-p%g' % (L, nh, p), nh, p, qkv, dO, mask=m)


def lengths_calls():
    """p alternates 0 and 0.1 along the list"""
    return [length_call(L, 0.1 * (i % 2)) for i, L in enumerate(LENGTHS)]


def long_calls(thin=False):
    """uniter_attn_fwd / uniter_attn_bwd only; nh = 3"""
    ls = (193, 256, 321) if thin else LONG
    return [length_call(L, 0.1 * (LONG.index(L) % 2), nh=3) for L in ls]


PACKED_LENS = (192, 1, 15, 16, 17, 31, 32, 33, 64, 65, 97, 161, 191)


@functools.lru_cache(maxsize=None)
def packed_call(p):
    lens = PACKED_LENS
    rows = sum(lens)
    return Call('packed-p%g' % p, 2, p, _randn(400, rows, 3 * 2 * HD), _randn(401, rows, 2 * HD), lens=lens)


@functools.lru_cache(maxsize=None)
def dropout_call(L, p):
    """DROPOUT: q = 0 and V[j, d] = [d == j % 64], so that ctx_i[d] = sum over j = d (mod 64) of m_ij / L: every keep flag is visible"""
    B, nh = (2, 3) if L < 64 else (1, 1)
    x, d = _operands(500 + L, B, L, nh)
    x[:, :, 0] = 0
    x[:, :, 2] = one_hot_v(L)[None, :, None, :]
    qkv, dO = _flat(x, d)
    return Call('dropout-L%d-p%g' % (L, p), nh, p, qkv, dO, mask=np.ones((B, L), dtype=F))


def dropout_calls():
    return [dropout_call(L, p) for L in (33, 164) for p in (0.5, 0.9)]


def masks_calls():
    return [masks_call(0.0), masks_call(0.1)]


def scores_calls():
    return [scores_call(0.0), scores_call(0.1)]


def packed_calls():
    return [packed_call(0.0), packed_call(0.1)]


def sample_slice(call, out, name, b):
    """the part of output `name` (library layout) that belongs to sample b -- for per-sample shares of MASKS / SCORES"""
    r0, n = int(call.cu[b]), call.lens[b]
    x = out[name]
    return x[r0:r0 + n] if x.shape[0] == call.rows and x.ndim == 2 and name != 'bias_part' else x[b]
