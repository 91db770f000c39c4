"""CPU: the optimizer-step, LayerNorm row-pass and embedding entry points of the C ABI refuse bad calls before any HIP call, with
the return code and the message recorded from the library before these launchers took StepCall / LnCall / TxtEmbedCall /
ImgEmbedCall; their workspace size functions (host arithmetic) return the integers recorded from that same library.

Every row of REFUSED is a call that must be refused: pointers are fake aligned integers that nothing may dereference (the one
exception is the parameter-group table, which the host reads: real memory of the child).  So that a regression (a row that is no
longer refused) cannot reach a device with them, the table runs in ONE child process that sees no GPU (HIP_VISIBLE_DEVICES=-1)
and loads the library with ctypes alone: `python tests/test_rowpass_refusals_cpu.py LIB` prints the observed values as JSON, and
the tests compare them with the literals below.  A second child runs with UNITER_LNB_WAVES=8 UNITER_LNB_ROWS=1 (`... LIB lnb8`):
the backward row pass's workspace is sized through those switches (8 waves of one row: as many rows per workgroup as the default's
4 waves of 2, so the integers agree).

Left out on purpose: a call the library refuses only behind a HIP call.  The hidden sizes beyond 1024 that the row passes and the
plain embedding forms turn away in their kernel dispatch are refused BEFORE any HIP call and are in the table (H_1028)."""
import ctypes as C
import json
import os
import subprocess
import sys

(P0, P1, P2, P3, P4, P5, P6, P7, P8, P9, P10, P11, P12, P13, P14, P15, P16, P17, P18, P19, P20, P21, P22, P23,
 WS) = (0x10000 * (i + 1) for i in range(25))      # fake 64-KiB aligned pointers
ODD = 4                                              # added to a pointer: 4-byte aligned only
TABLE = 'TABLE'                                      # the child's own array of 32 uniter_optim_group_t
DET_MAX_ROWS = 16384                                 # UNITER_EMBED_DET_MAX_ROWS


class Ws:
    """ws_bytes of a call = what the named size function returns for the call's own dims (resolved in the child, after the row's
    overrides), minus `short`"""
    def __init__(self, fn, dims, short=0):
        self.fn, self.dims, self.short = fn, dims, short

    def less(self, k):
        return Ws(self.fn, self.dims, k)


# ---- the entry points: (ctypes signature, parameter names with the defaults of one valid call) ----
# i = int, p = pointer, f = float, q = uint64, u = uint32, z = size_t
_S = dict(stream=None)
_RNG = dict(p=0.0, seed=1, offset=0)

# optimizer step (optim.hip): n = 128, two chunks
_BUF = dict(params=P0, grads=P1, m=P2, v=P3, flags=P4, n=128, sumsq=P5, grad_scale=1.0, max_norm=0.0)
_BUF16 = dict(params=P0, grads=P1, g16=None, m=P2, v=P3, flags=P4, n=128, sumsq=P5, grad_scale=1.0, max_norm=0.0)
_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
_STEP = dict(step=1, adamw=0, zero_grads=1)
_PAIR = dict(mirror=None, ps=0, pair=None, first=0)
_GROUPS = dict(groups=TABLE, n_groups=2, step=1, zero_grads=1)
_AVG = dict(avg=P9, avg_weight=0.5)
_OPTIM = {
    'uniter_adam_step': ('pppppzpfffffffiiip', dict(**_BUF, **_HP, **_STEP, **_S)),
    'uniter_adam_step_mirror': ('pppppzpfffffffiiipp', dict(**_BUF, **_HP, **_STEP, mirror=None, **_S)),
    'uniter_adam_step_ex': ('pppppzpfffffffiiipip', dict(**_BUF, **_HP, **_STEP, mirror=None, max_wgs=0, **_S)),
    'uniter_adam_step_g16': ('ppppppzpfffffffiiipip', dict(**_BUF16, **_HP, **_STEP, mirror=None, max_wgs=0, **_S)),
    'uniter_adam_step_x3': ('ppppppzpfffffffiiipzip', dict(**_BUF16, **_HP, **_STEP, mirror=None, ps=0, max_wgs=0, **_S)),
    'uniter_adam_step_x3p': ('ppppppzpfffffffiiipzpzip', dict(**_BUF16, **_HP, **_STEP, **_PAIR, max_wgs=0, **_S)),
    'uniter_adam_step_rows': ('pppppzpfffffffiiipiiip', dict(**_BUF, **_HP, **_STEP, row_mask=P8, row_len=64, rows_touched=1, max_wgs=0, **_S)),
    'uniter_optim_step': ('ippppppzpfffffffiiipzpzip', dict(kind=0, **_BUF16, **_HP, **_STEP, **_PAIR, max_wgs=0, **_S)),
    'uniter_optim_step_groups': ('ippppppzpffpiiipzpzip', dict(kind=0, **_BUF16, **_GROUPS, **_PAIR, max_wgs=0, **_S)),
    'uniter_optim_step_avg': ('ippppppzpfffffffiiipzpzpfip', dict(kind=0, **_BUF16, **_HP, **_STEP, **_PAIR, **_AVG, max_wgs=0, **_S)),
    'uniter_optim_step_groups_avg': ('ippppppzpffpiiipzpzpfip', dict(kind=0, **_BUF16, **_GROUPS, **_PAIR, **_AVG, max_wgs=0, **_S)),
}

# LayerNorm row passes (layernorm.hip): M = 5 rows of H = 64
_MH = dict(M=5, H=64, p=0.0, seed=1, offset=0, site=3)
_LNWS = dict(ws=WS, ws_bytes=Ws('uniter_ln_bwd_ws_bytes', ('M', 'H')))
_FWD_IN, _FWD_ST = dict(res=P1, gamma=P2, beta=P3), dict(mean=P7, rstd=P8)
_BWD_IN = dict(z=P1, mean=P2, rstd=P3, gamma=P4)
_SLABS = dict(nslab=1, slab_stride=0)
_LN = {
    'uniter_ln_fwd': ('ppppppppiifquup', dict(x=P0, **_FWD_IN, z_out=P4, y=P5, **_FWD_ST, **_MH, **_S)),
    'uniter_ln_fwd_b16': ('pppppppppiifquup', dict(x=P0, **_FWD_IN, z_out=P4, y=P5, copy=P6, **_FWD_ST, **_MH, **_S)),
    'uniter_ln_fwd_slabs': ('pizppppppppiifquup', dict(x=P0, **_SLABS, **_FWD_IN, z_out=P4, y=P5, copy=P6, **_FWD_ST, **_MH, **_S)),
    'uniter_ln_fwd_slabs_x3': ('pizppppppppiifquup', dict(x=P0, **_SLABS, **_FWD_IN, z_out=P4, y=P5, copy=P6, **_FWD_ST, **_MH, **_S)),
    'uniter_ln_bwd': ('ppppppppppiifquupzp', dict(dy=P0, **_BWD_IN, dz=P5, dx=P6, dgamma=P8, dbeta=P9, dbias=P10, **_MH, **_LNWS, **_S)),
    'uniter_ln_bwd_b16': ('pppppppppppiifquupzp', dict(dy=P0, **_BWD_IN, dz=P5, dx=P6, copy=P7, dgamma=P8, dbeta=P9, dbias=P10, **_MH,
                                                       **_LNWS, **_S)),
    'uniter_ln_bwd_rows': ('ppppppppiiifquupzp', dict(dy=P0, **_BWD_IN, dz=P5, dx=P6, copy=P7, want_dbias=1, **_MH, **_LNWS, **_S)),
    'uniter_ln_bwd_rows_slabs': ('pizpppppppiiifquupzp', dict(dy=P0, **_SLABS, **_BWD_IN, dz=P5, dx=P6, copy=P7, want_dbias=1, **_MH,
                                                             **_LNWS, **_S)),
    'uniter_ln_bwd_rows_slabs_x3': ('pizpppppppiiifquupzp', dict(dy=P0, **_SLABS, **_BWD_IN, dz=P5, dx=P6, copy=P7, want_dbias=1, **_MH,
                                                                **_LNWS, **_S)),
}
_LN_REQUIRED = {fn: (('x', 'gamma', 'beta', 'y') if '_fwd' in fn else ('dy', 'z', 'mean', 'rstd', 'gamma', 'ws')) for fn in _LN}
_LN_REQUIRED['uniter_ln_bwd'] += ('dgamma', 'dbeta')
_LN_REQUIRED['uniter_ln_bwd_b16'] += ('dgamma', 'dbeta')
_ROWOPS = {
    'uniter_ln_bwd_finalize': ('pziipppp', dict(ws=WS, ws_bytes=Ws('uniter_ln_bwd_ws_bytes', ('M', 'H')), M=5, H=64, dgamma=P0, dbeta=P1,
                                                dbias=P2, **_S)),
    'uniter_hidden_keep_bits_gen': ('pziuuuzfqup', dict(bits=P0, site_stride=64, nsites=2, site_a0=3, site_b0=4, site_step=4, elements=320,
                                                        p=0.1, seed=1, offset=0, **_S)),
    'uniter_colsum_f32': ('piiipipzp', dict(X=P0, M=5, N=64, ld=64, out=P1, beta=0, ws=WS, ws_bytes=Ws('uniter_colsum_ws_bytes', ('M', 'N')),
                                            **_S)),
    'uniter_slab_reduce_add': ('pizpzp', dict(slabs=P0, nslab=2, slab_stride=320, out=P1, n=320, **_S)),
    'uniter_colsum_bf16_add': ('piiipp', dict(X=P0, M=5, N=64, ld=64, out=P1, **_S)),
    'uniter_colsum_bf16_add_det': ('piiippzp', dict(X=P0, M=5, N=64, ld=64, out=P1, ws=WS,
                                                    ws_bytes=Ws('uniter_colsum_det_ws_bytes', ('M', 'N')), **_S)),
}

# embeddings (embed.hip, input_grads.hip): B = 2 samples of T = 3 tokens and R = 2 regions in S = 6 rows of H = 64
_TXT_IN = dict(ids=P0, pos_ids=P1, type_ids=P2, word=P3, pos=P4, type=P5, gamma=P6)
_TXT_DIMS = dict(B=2, T=3, S=6, H=64, vocab=97, max_pos=40, type_vocab=2, pos_bcast=0)
_TXT_GRADS = dict(dword=P8, dpos=P9, dtype=P10, dgamma=P11, dbeta=P12)
_IMG_IN = dict(imgfc=P0, pos7=P1, type_ids=None, Wp=P2, bp=P3, type=P4, g_i=P5, b_i=P6, g_p=P7, b_p=P8, g_f=P9)
_IMG_GRADS = dict(d_imgfc=P13, d_posfc=P14, dWp=P15, dbp=P16, dtype=P17, dg_i=P18, db_i=P19, dg_p=P20, db_p=P21, dg_f=P22, db_f=P23)
_IMG_DIMS = dict(B=2, R=2, T0=3, S=6, H=64, type_vocab=2)
_TXT_WS = dict(ws=WS, ws_bytes=Ws('uniter_embed_bwd_ws_bytes', (('B', 'T'), 'H')))
_IMG_WS = dict(ws=WS, ws_bytes=Ws('uniter_embed_bwd_ws_bytes', (('B', 'R'), 'H')))
_TXT_DET_WS = dict(ws=WS, ws_bytes=Ws('uniter_embed_bwd_det_ws_bytes', (('B', 'T'), 0, 'H')))
_IMG_DET_WS = dict(ws=WS, ws_bytes=Ws('uniter_embed_bwd_det_ws_bytes', (0, ('B', 'R'), 'H')))
_EMBED = {
    'uniter_txt_embed_fwd': ('p' * 9 + 'i' * 8 + 'fqup', dict(**_TXT_IN, beta=P7, cat=P8, **_TXT_DIMS, **_RNG, **_S)),
    'uniter_txt_embed_fwd_delta': ('p' * 10 + 'i' * 8 + 'fqup', dict(**_TXT_IN, beta=P7, delta=P9, cat=P8, **_TXT_DIMS, **_RNG, **_S)),
    'uniter_txt_embed_bwd': ('p' * 13 + 'i' * 8 + 'fqupzp', dict(dcat=P7, **_TXT_IN, **_TXT_GRADS, **_TXT_DIMS, **_RNG, **_TXT_WS, **_S)),
    'uniter_txt_embed_bwd_det': ('p' * 13 + 'i' * 8 + 'fqupzp', dict(dcat=P7, **_TXT_IN, **_TXT_GRADS, **_TXT_DIMS, **_RNG, **_TXT_DET_WS,
                                                                     **_S)),
    'uniter_txt_embed_bwd_rows': ('p' * 10 + 'i' * 8 + 'fqup', dict(dcat=P7, **_TXT_IN, delta=P9, d_rows=P8, **_TXT_DIMS, **_RNG, **_S)),
    'uniter_img_embed_fwd': ('p' * 14 + 'i' * 6 + 'fqup', dict(**_IMG_IN, b_f=P10, cat=P11, stats=P12, **_IMG_DIMS, **_RNG, **_S)),
    'uniter_img_embed_bwd': ('p' * 24 + 'i' * 6 + 'fqupzp', dict(dcat=P11, **_IMG_IN, stats=P12, **_IMG_GRADS, **_IMG_DIMS, **_RNG, **_IMG_WS,
                                                                 **_S)),
    'uniter_img_embed_bwd_det': ('p' * 24 + 'i' * 6 + 'fqupzp', dict(dcat=P11, **_IMG_IN, stats=P12, **_IMG_GRADS, **_IMG_DIMS, **_RNG,
                                                                     **_IMG_DET_WS, **_S)),
}
_EMBED_OPTIONAL = ('type_ids', 'delta', 'stream')      # (img_embed_fwd alone does without stats: below)
FUNCS = dict(**_OPTIM, **_LN, **_ROWOPS, **_EMBED)


def _optim_rows(fn):
    d = FUNCS[fn][1]
    rows = [('null_' + k, {k: None}) for k in ('params', 'grads', 'm', 'v', 'flags')]      # (v: kind 0 = Adam; SGD takes a NULL one)
    rows += [('n_96', dict(n=96)), ('step_0', dict(step=0)), ('clipping_without_sumsq', dict(max_norm=1.0, sumsq=None))]
    if 'g16' in d:
        rows += [('misaligned_g16', dict(g16=P6 + ODD))]
    if 'ps' in d:
        rows += [('piece_stride_without_mirror', dict(ps=128)), ('odd_piece_stride', dict(mirror=P7, ps=130))]
    if 'pair' in d:
        rows += [('pair_source_without_mirror', dict(pair=P10)), ('misaligned_pair_source', dict(mirror=P7, ps=128, pair=P10 + ODD)),
                 ('first_element_32', dict(mirror=P7, ps=128, pair=P10, first=32))]
    if 'kind' in d:
        rows += [('kind_minus_1', dict(kind=-1)), ('kind_4', dict(kind=4))]
    if 'n_groups' in d:
        rows += [('n_groups_0', dict(n_groups=0)), ('n_groups_33', dict(n_groups=33)), ('null_groups', dict(groups=None))]
    if 'avg' in d:
        rows += [('null_avg', dict(avg=None)), ('misaligned_avg', dict(avg=P9 + ODD)), ('avg_weight_negative', dict(avg_weight=-0.1)),
                 ('avg_weight_1_5', dict(avg_weight=1.5))]
    if 'row_mask' in d:
        rows += [('row_len_96', dict(row_len=96)), ('row_len_not_dividing_n', dict(row_len=192)), ('null_row_mask', dict(row_mask=None))]
    return rows


def _ln_rows(fn):
    d = FUNCS[fn][1]
    rows = [('null_' + k, {k: None}) for k in _LN_REQUIRED[fn]]
    if 'nslab' in d:
        rows += [('nslab_0', dict(nslab=0)), ('slab_stride_below_MH', dict(nslab=2, slab_stride=319))]
    if '_fwd' in fn:
        rows += [('mean_without_rstd', dict(rstd=None)), ('rstd_without_mean', dict(mean=None)), ('p_negative', dict(p=-0.25)),
                 ('p_one', dict(p=1.0))]      # (the backward pass has never checked p: a call it does not refuse is not in the table)
    else:
        rows += [('ws_one_byte_short', dict(ws_bytes=d['ws_bytes'].less(1))), ('none_of_dz_dx_copy', dict(dz=None, dx=None, copy=None)
                 if 'copy' in d else dict(dz=None, dx=None))]
    rows += [('H_6', dict(H=6)), ('H_1028', dict(H=1028))]
    if fn.endswith('_x3'):
        rows += [('H_12', dict(H=12)), ('misaligned_copy', dict(copy=d['copy'] + ODD))]
    return rows


def _embed_rows(fn):
    d = FUNCS[fn][1]
    det, txt = fn.endswith('_det'), '_txt_' in fn
    optional = _EMBED_OPTIONAL + (('stats',) if fn == 'uniter_img_embed_fwd' else ())
    rows = [('null_' + k, {k: None}) for k, v in d.items() if isinstance(v, int) and v >= P0 and k not in optional]
    rows += [('H_6', dict(H=6)), ('H_1028', dict(H=1028))]
    rows += [('T_above_S', dict(T=7))] if txt else [('T0_plus_R_above_S', dict(T0=5)), ('type_vocab_1', dict(type_vocab=1))]
    if 'ws' in d:
        rows += [('ws_one_byte_short', dict(ws_bytes=d['ws_bytes'].less(1)))]
    if det:
        rows += [('rows_above_the_cap', dict(B=DET_MAX_ROWS // 2 + 1))]
    if 'delta' in d:
        rows += [('misaligned_delta', dict(delta=P9 + ODD))]
    if 'd_rows' in d:
        rows += [('misaligned_d_rows', dict(d_rows=P8 + ODD))]
    return rows


FIN, GEN, CS, SRA, CSB, CSD = _ROWOPS
_ROWOPS_ROWS = [
    (FIN, 'null_ws', dict(ws=None)), (FIN, 'null_dgamma', dict(dgamma=None)), (FIN, 'null_dbeta', dict(dbeta=None)),
    (FIN, 'ws_one_byte_short', dict(ws_bytes=FUNCS[FIN][1]['ws_bytes'].less(1))),
    (GEN, 'null_bits', dict(bits=None)), (GEN, 'nsites_0', dict(nsites=0)), (GEN, 'elements_0', dict(elements=0)), (GEN, 'p_zero', dict(p=0.0)),
    (GEN, 'p_one', dict(p=1.0)), (GEN, 'elements_6', dict(elements=6)), (GEN, 'site_stride_6', dict(site_stride=6)),
    (GEN, 'site_stride_short', dict(site_stride=36)), (GEN, 'misaligned_bits', dict(bits=P0 + 2)),
    (CS, 'null_X', dict(X=None)), (CS, 'null_out', dict(out=None)), (CS, 'null_ws', dict(ws=None)), (CS, 'N_6', dict(N=6, ld=8)),
    (CS, 'ld_6', dict(N=4, ld=6)), (CS, 'ws_one_byte_short', dict(ws_bytes=FUNCS[CS][1]['ws_bytes'].less(1))),
    (SRA, 'null_slabs', dict(slabs=None)), (SRA, 'null_out', dict(out=None)), (SRA, 'nslab_0', dict(nslab=0)), (SRA, 'n_6', dict(n=6)),
    (SRA, 'slab_stride_6', dict(slab_stride=6)), (SRA, 'misaligned_slabs', dict(slabs=P0 + ODD)), (SRA, 'misaligned_out', dict(out=P1 + ODD)),
    (CSB, 'null_X', dict(X=None)), (CSB, 'null_out', dict(out=None)), (CSB, 'M_0', dict(M=0)), (CSB, 'N_0', dict(N=0)),
    (CSB, 'N_12', dict(N=12, ld=16)), (CSB, 'ld_12', dict(N=8, ld=12)), (CSB, 'misaligned_X', dict(X=P0 + 8)),
    (CSD, 'null_X', dict(X=None)), (CSD, 'null_out', dict(out=None)), (CSD, 'null_ws', dict(ws=None)), (CSD, 'M_0', dict(M=0)),
    (CSD, 'N_0', dict(N=0)), (CSD, 'ld_below_N', dict(ld=56)), (CSD, 'N_12', dict(N=12, ld=16)), (CSD, 'ld_12', dict(N=8, ld=12)),
    (CSD, 'misaligned_X', dict(X=P0 + 8)), (CSD, 'misaligned_out', dict(out=P1 + 2)), (CSD, 'misaligned_ws', dict(ws=WS + 2)),
    (CSD, 'ws_one_byte_short', dict(ws_bytes=FUNCS[CSD][1]['ws_bytes'].less(1))),
]
REFUSED = ([(fn, name, kw) for fn in _OPTIM for name, kw in _optim_rows(fn)] + [(fn, name, kw) for fn in _LN for name, kw in _ln_rows(fn)] +
           _ROWOPS_ROWS + [(fn, name, kw) for fn in _EMBED for name, kw in _embed_rows(fn)])

# ---- host arithmetic: one tiny shape, the workload's own, one at a cap, one zero ----
NUMBERS = (
    [('uniter_grad_sumsq_ws_bytes', 'n%d' % n, (n,)) for n in (192, 110_000_000, 2048 * 1024, 0)] +
    [('uniter_ln_bwd_ws_bytes', 'M%d_H%d' % s, s) for s in ((5, 64), (2624, 768), (1 << 20, 1024), (0, 64))] +
    [('uniter_colsum_ws_bytes', 'M%d_N%d' % s, s) for s in ((5, 64), (2624, 3072), (2048, 768), (0, 64))] +
    [('uniter_colsum_det_ws_bytes', 'M%d_N%d' % s, s) for s in ((5, 64), (2624, 3072), (64, 768), (0, 64))] +
    [('uniter_hidden_keep_bits_bytes', 'n%d' % n, (n,)) for n in (320, 2624 * 768, 28, 0)] +
    [('uniter_embed_bwd_ws_bytes', 'rows%d_H%d' % s, s) for s in ((6, 64), (2048, 768), (1024, 1024), (0, 64))] +
    [('uniter_embed_bwd_det_ws_bytes', 'txt%d_img%d_H%d' % s, s) for s in ((6, 4, 64), (2048, 576, 768), (DET_MAX_ROWS, DET_MAX_ROWS, 1024),
                                                                           (0, 0, 64))])
_SIZE_T_ARGS = ('uniter_grad_sumsq_ws_bytes', 'uniter_hidden_keep_bits_bytes')
NUMBERS_LNB8 = [r for r in NUMBERS if r[0] == 'uniter_ln_bwd_ws_bytes']

_CT = {'i': C.c_int, 'p': C.c_void_p, 'f': C.c_float, 'q': C.c_uint64, 'u': C.c_uint32, 'z': C.c_size_t}


def _size(lib, fn, args):
    f = getattr(lib, fn)
    f.restype, f.argtypes = C.c_size_t, [C.c_size_t if fn in _SIZE_T_ARGS else C.c_int] * len(args)
    return f(*args)


def _call(lib, fn, overrides, table):
    sig, defaults = FUNCS[fn]
    unknown = set(overrides) - set(defaults)
    assert not unknown and len(sig) == len(defaults), (fn, unknown, len(sig), len(defaults))
    a = dict(defaults, **overrides)
    dim = lambda e: e if isinstance(e, int) else a[e] if isinstance(e, str) else a[e[0]] * a[e[1]]
    for k, v in a.items():
        if isinstance(v, Ws):
            a[k] = _size(lib, v.fn, [dim(e) for e in v.dims]) - v.short
        elif v == TABLE:
            a[k] = C.addressof(table)
    f = getattr(lib, fn)
    f.restype, f.argtypes = C.c_int, [_CT[ch] for ch in sig]
    return f(*a.values())


def observe(lib_path, lnb8):
    """{'refused': {id: [rc, message]}, 'numbers': {id: value}} of the library at lib_path"""
    lib = C.CDLL(lib_path)
    lib.uniter_last_error.restype = C.c_char_p
    table = (C.c_float * (5 * 32))(*([1e-3, 0.9, 0.999, 1e-8, 0.01] * 32))
    out = {'refused': {}, 'numbers': {}}
    for fn, name, kw in ([] if lnb8 else REFUSED):
        rc = _call(lib, fn, kw, table)
        out['refused']['%s:%s' % (fn, name)] = [rc, lib.uniter_last_error().decode() if rc else '']
    for fn, name, args in (NUMBERS_LNB8 if lnb8 else NUMBERS):
        out['numbers']['%s:%s' % (fn, name)] = _size(lib, fn, args)
    return out


if __name__ == '__main__':
    print(json.dumps(observe(sys.argv[1], sys.argv[2:] == ['lnb8'])))
    sys.exit(0)

import pytest      # noqa: E402  (the child process above needs neither pytest nor the package)

E_ARG, E_SHAPE = -1, -2
EXPECTED = json.loads(r'''
{"refused": {
  "uniter_adam_step:null_params": [-1, "adam_step: null pointer"],
  "uniter_adam_step:null_grads": [-1, "adam_step: null pointer"],
  "uniter_adam_step:null_m": [-1, "adam_step: null pointer"],
  "uniter_adam_step:null_v": [-1, "adam_step: null pointer"],
  "uniter_adam_step:null_flags": [-1, "adam_step: null pointer"],
  "uniter_adam_step:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_adam_step:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_adam_step:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_adam_step_mirror:null_params": [-1, "adam_step: null pointer"],
  "uniter_adam_step_mirror:null_grads": [-1, "adam_step: null pointer"],
  "uniter_adam_step_mirror:null_m": [-1, "adam_step: null pointer"],
  "uniter_adam_step_mirror:null_v": [-1, "adam_step: null pointer"],
  "uniter_adam_step_mirror:null_flags": [-1, "adam_step: null pointer"],
  "uniter_adam_step_mirror:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_adam_step_mirror:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_adam_step_mirror:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_adam_step_ex:null_params": [-1, "adam_step: null pointer"],
  "uniter_adam_step_ex:null_grads": [-1, "adam_step: null pointer"],
  "uniter_adam_step_ex:null_m": [-1, "adam_step: null pointer"],
  "uniter_adam_step_ex:null_v": [-1, "adam_step: null pointer"],
  "uniter_adam_step_ex:null_flags": [-1, "adam_step: null pointer"],
  "uniter_adam_step_ex:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_adam_step_ex:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_adam_step_ex:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_adam_step_g16:null_params": [-1, "adam_step: null pointer"],
  "uniter_adam_step_g16:null_grads": [-1, "adam_step: null pointer"],
  "uniter_adam_step_g16:null_m": [-1, "adam_step: null pointer"],
  "uniter_adam_step_g16:null_v": [-1, "adam_step: null pointer"],
  "uniter_adam_step_g16:null_flags": [-1, "adam_step: null pointer"],
  "uniter_adam_step_g16:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_adam_step_g16:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_adam_step_g16:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_adam_step_g16:misaligned_g16": [-2, "adam_step: bf16 gradients must be 8-byte aligned"],
  "uniter_adam_step_x3:null_params": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3:null_grads": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3:null_m": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3:null_v": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3:null_flags": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_adam_step_x3:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_adam_step_x3:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_adam_step_x3:misaligned_g16": [-2, "adam_step: bf16 gradients must be 8-byte aligned"],
  "uniter_adam_step_x3:piece_stride_without_mirror": [-2, "adam_step: bad mirror piece stride"],
  "uniter_adam_step_x3:odd_piece_stride": [-2, "adam_step: bad mirror piece stride"],
  "uniter_adam_step_x3p:null_params": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3p:null_grads": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3p:null_m": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3p:null_v": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3p:null_flags": [-1, "adam_step: null pointer"],
  "uniter_adam_step_x3p:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_adam_step_x3p:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_adam_step_x3p:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_adam_step_x3p:misaligned_g16": [-2, "adam_step: bf16 gradients must be 8-byte aligned"],
  "uniter_adam_step_x3p:piece_stride_without_mirror": [-2, "adam_step: bad mirror piece stride"],
  "uniter_adam_step_x3p:odd_piece_stride": [-2, "adam_step: bad mirror piece stride"],
  "uniter_adam_step_x3p:pair_source_without_mirror": [-1, "adam_step_x3p: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_adam_step_x3p:misaligned_pair_source": [-1, "adam_step_x3p: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_adam_step_x3p:first_element_32": [-1, "adam_step_x3p: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_adam_step_rows:null_params": [-1, "adam_step: null pointer"],
  "uniter_adam_step_rows:null_grads": [-1, "adam_step: null pointer"],
  "uniter_adam_step_rows:null_m": [-1, "adam_step: null pointer"],
  "uniter_adam_step_rows:null_v": [-1, "adam_step: null pointer"],
  "uniter_adam_step_rows:null_flags": [-1, "adam_step: null pointer"],
  "uniter_adam_step_rows:n_96": [-1, "adam_step_rows: row_len must be a multiple of 64 dividing n"],
  "uniter_adam_step_rows:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_adam_step_rows:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_adam_step_rows:row_len_96": [-1, "adam_step_rows: row_len must be a multiple of 64 dividing n"],
  "uniter_adam_step_rows:row_len_not_dividing_n": [-1, "adam_step_rows: row_len must be a multiple of 64 dividing n"],
  "uniter_adam_step_rows:null_row_mask": [-1, "adam_step_rows: row_len must be a multiple of 64 dividing n"],
  "uniter_optim_step:null_params": [-1, "adam_step: null pointer"],
  "uniter_optim_step:null_grads": [-1, "adam_step: null pointer"],
  "uniter_optim_step:null_m": [-1, "adam_step: null pointer"],
  "uniter_optim_step:null_v": [-1, "adam_step: null pointer"],
  "uniter_optim_step:null_flags": [-1, "adam_step: null pointer"],
  "uniter_optim_step:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_optim_step:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_optim_step:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_optim_step:misaligned_g16": [-2, "adam_step: bf16 gradients must be 8-byte aligned"],
  "uniter_optim_step:piece_stride_without_mirror": [-2, "adam_step: bad mirror piece stride"],
  "uniter_optim_step:odd_piece_stride": [-2, "adam_step: bad mirror piece stride"],
  "uniter_optim_step:pair_source_without_mirror": [-1, "adam_step_x3p: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step:misaligned_pair_source": [-1, "adam_step_x3p: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step:first_element_32": [-1, "adam_step_x3p: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step:kind_minus_1": [-1, "optim_step: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)"],
  "uniter_optim_step:kind_4": [-1, "optim_step: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)"],
  "uniter_optim_step_groups:null_params": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups:null_grads": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups:null_m": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups:null_v": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups:null_flags": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_optim_step_groups:step_0": [-1, "optim_step_groups: step must be >= 1"],
  "uniter_optim_step_groups:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_optim_step_groups:misaligned_g16": [-2, "adam_step: bf16 gradients must be 8-byte aligned"],
  "uniter_optim_step_groups:piece_stride_without_mirror": [-2, "adam_step: bad mirror piece stride"],
  "uniter_optim_step_groups:odd_piece_stride": [-2, "adam_step: bad mirror piece stride"],
  "uniter_optim_step_groups:pair_source_without_mirror": [-1, "optim_step_groups: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_groups:misaligned_pair_source": [-1, "optim_step_groups: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_groups:first_element_32": [-1, "optim_step_groups: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_groups:kind_minus_1": [-1, "optim_step_groups: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)"],
  "uniter_optim_step_groups:kind_4": [-1, "optim_step_groups: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)"],
  "uniter_optim_step_groups:n_groups_0": [-1, "optim_step_groups: n_groups must be 1 .. 32 (got 0) with a table"],
  "uniter_optim_step_groups:n_groups_33": [-1, "optim_step_groups: n_groups must be 1 .. 32 (got 33) with a table"],
  "uniter_optim_step_groups:null_groups": [-1, "optim_step_groups: n_groups must be 1 .. 32 (got 2) with a table"],
  "uniter_optim_step_avg:null_params": [-1, "adam_step: null pointer"],
  "uniter_optim_step_avg:null_grads": [-1, "adam_step: null pointer"],
  "uniter_optim_step_avg:null_m": [-1, "adam_step: null pointer"],
  "uniter_optim_step_avg:null_v": [-1, "adam_step: null pointer"],
  "uniter_optim_step_avg:null_flags": [-1, "adam_step: null pointer"],
  "uniter_optim_step_avg:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_optim_step_avg:step_0": [-1, "adam_step: step must be >= 1"],
  "uniter_optim_step_avg:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_optim_step_avg:misaligned_g16": [-2, "adam_step: bf16 gradients must be 8-byte aligned"],
  "uniter_optim_step_avg:piece_stride_without_mirror": [-2, "adam_step: bad mirror piece stride"],
  "uniter_optim_step_avg:odd_piece_stride": [-2, "adam_step: bad mirror piece stride"],
  "uniter_optim_step_avg:pair_source_without_mirror": [-1, "optim_step_avg: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_avg:misaligned_pair_source": [-1, "optim_step_avg: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_avg:first_element_32": [-1, "optim_step_avg: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_avg:kind_minus_1": [-1, "optim_step_avg: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)"],
  "uniter_optim_step_avg:kind_4": [-1, "optim_step_avg: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)"],
  "uniter_optim_step_avg:null_avg": [-1, "optim_step_avg: avg is NULL"],
  "uniter_optim_step_avg:misaligned_avg": [-2, "optim_step_avg: avg must be 16-byte aligned"],
  "uniter_optim_step_avg:avg_weight_negative": [-1, "optim_step_avg: avg_weight must lie in [0, 1] (got -0.1)"],
  "uniter_optim_step_avg:avg_weight_1_5": [-1, "optim_step_avg: avg_weight must lie in [0, 1] (got 1.5)"],
  "uniter_optim_step_groups_avg:null_params": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups_avg:null_grads": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups_avg:null_m": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups_avg:null_v": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups_avg:null_flags": [-1, "adam_step: null pointer"],
  "uniter_optim_step_groups_avg:n_96": [-2, "adam_step: n must be a multiple of 64"],
  "uniter_optim_step_groups_avg:step_0": [-1, "optim_step_groups_avg: step must be >= 1"],
  "uniter_optim_step_groups_avg:clipping_without_sumsq": [-1, "adam_step: clipping needs sumsq"],
  "uniter_optim_step_groups_avg:misaligned_g16": [-2, "adam_step: bf16 gradients must be 8-byte aligned"],
  "uniter_optim_step_groups_avg:piece_stride_without_mirror": [-2, "adam_step: bad mirror piece stride"],
  "uniter_optim_step_groups_avg:odd_piece_stride": [-2, "adam_step: bad mirror piece stride"],
  "uniter_optim_step_groups_avg:pair_source_without_mirror": [-1, "optim_step_groups_avg: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_groups_avg:misaligned_pair_source": [-1, "optim_step_groups_avg: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_groups_avg:first_element_32": [-1, "optim_step_groups_avg: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table"],
  "uniter_optim_step_groups_avg:kind_minus_1": [-1, "optim_step_groups_avg: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)"],
  "uniter_optim_step_groups_avg:kind_4": [-1, "optim_step_groups_avg: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)"],
  "uniter_optim_step_groups_avg:n_groups_0": [-1, "optim_step_groups_avg: n_groups must be 1 .. 32 (got 0) with a table"],
  "uniter_optim_step_groups_avg:n_groups_33": [-1, "optim_step_groups_avg: n_groups must be 1 .. 32 (got 33) with a table"],
  "uniter_optim_step_groups_avg:null_groups": [-1, "optim_step_groups_avg: n_groups must be 1 .. 32 (got 2) with a table"],
  "uniter_optim_step_groups_avg:null_avg": [-1, "optim_step_groups_avg: avg is NULL"],
  "uniter_optim_step_groups_avg:misaligned_avg": [-2, "optim_step_groups_avg: avg must be 16-byte aligned"],
  "uniter_optim_step_groups_avg:avg_weight_negative": [-1, "optim_step_groups_avg: avg_weight must lie in [0, 1] (got -0.1)"],
  "uniter_optim_step_groups_avg:avg_weight_1_5": [-1, "optim_step_groups_avg: avg_weight must lie in [0, 1] (got 1.5)"],
  "uniter_ln_fwd:null_x": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd:null_gamma": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd:null_beta": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd:null_y": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd:mean_without_rstd": [-1, "ln_fwd: mean/rstd must both be given or NULL"],
  "uniter_ln_fwd:rstd_without_mean": [-1, "ln_fwd: mean/rstd must both be given or NULL"],
  "uniter_ln_fwd:p_negative": [-1, "ln_fwd: bad dropout p"],
  "uniter_ln_fwd:p_one": [-1, "ln_fwd: bad dropout p"],
  "uniter_ln_fwd:H_6": [-2, "ln_fwd: H must be a multiple of 4"],
  "uniter_ln_fwd:H_1028": [-2, "layernorm: hidden size 1028 unsupported (max 1024)"],
  "uniter_ln_fwd_b16:null_x": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_b16:null_gamma": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_b16:null_beta": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_b16:null_y": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_b16:mean_without_rstd": [-1, "ln_fwd: mean/rstd must both be given or NULL"],
  "uniter_ln_fwd_b16:rstd_without_mean": [-1, "ln_fwd: mean/rstd must both be given or NULL"],
  "uniter_ln_fwd_b16:p_negative": [-1, "ln_fwd: bad dropout p"],
  "uniter_ln_fwd_b16:p_one": [-1, "ln_fwd: bad dropout p"],
  "uniter_ln_fwd_b16:H_6": [-2, "ln_fwd: H must be a multiple of 4"],
  "uniter_ln_fwd_b16:H_1028": [-2, "layernorm: hidden size 1028 unsupported (max 1024)"],
  "uniter_ln_fwd_slabs:null_x": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_slabs:null_gamma": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_slabs:null_beta": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_slabs:null_y": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_slabs:nslab_0": [-1, "ln_fwd: bad slab count / stride"],
  "uniter_ln_fwd_slabs:slab_stride_below_MH": [-1, "ln_fwd: bad slab count / stride"],
  "uniter_ln_fwd_slabs:mean_without_rstd": [-1, "ln_fwd: mean/rstd must both be given or NULL"],
  "uniter_ln_fwd_slabs:rstd_without_mean": [-1, "ln_fwd: mean/rstd must both be given or NULL"],
  "uniter_ln_fwd_slabs:p_negative": [-1, "ln_fwd: bad dropout p"],
  "uniter_ln_fwd_slabs:p_one": [-1, "ln_fwd: bad dropout p"],
  "uniter_ln_fwd_slabs:H_6": [-2, "ln_fwd: H must be a multiple of 4"],
  "uniter_ln_fwd_slabs:H_1028": [-2, "layernorm: hidden size 1028 unsupported (max 1024)"],
  "uniter_ln_fwd_slabs_x3:null_x": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_slabs_x3:null_gamma": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_slabs_x3:null_beta": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_slabs_x3:null_y": [-1, "ln_fwd: null pointer"],
  "uniter_ln_fwd_slabs_x3:nslab_0": [-1, "ln_fwd: bad slab count / stride"],
  "uniter_ln_fwd_slabs_x3:slab_stride_below_MH": [-1, "ln_fwd: bad slab count / stride"],
  "uniter_ln_fwd_slabs_x3:mean_without_rstd": [-1, "ln_fwd: mean/rstd must both be given or NULL"],
  "uniter_ln_fwd_slabs_x3:rstd_without_mean": [-1, "ln_fwd: mean/rstd must both be given or NULL"],
  "uniter_ln_fwd_slabs_x3:p_negative": [-1, "ln_fwd: bad dropout p"],
  "uniter_ln_fwd_slabs_x3:p_one": [-1, "ln_fwd: bad dropout p"],
  "uniter_ln_fwd_slabs_x3:H_6": [-2, "ln_fwd: the x3 copy needs H % 8 == 0 and a 16-byte aligned buffer"],
  "uniter_ln_fwd_slabs_x3:H_1028": [-2, "ln_fwd: the x3 copy needs H % 8 == 0 and a 16-byte aligned buffer"],
  "uniter_ln_fwd_slabs_x3:H_12": [-2, "ln_fwd: the x3 copy needs H % 8 == 0 and a 16-byte aligned buffer"],
  "uniter_ln_fwd_slabs_x3:misaligned_copy": [-2, "ln_fwd: the x3 copy needs H % 8 == 0 and a 16-byte aligned buffer"],
  "uniter_ln_bwd:null_dy": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd:null_z": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd:null_mean": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd:null_rstd": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd:null_gamma": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd:null_ws": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd:null_dgamma": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd:null_dbeta": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd:ws_one_byte_short": [-1, "ln_bwd: workspace too small"],
  "uniter_ln_bwd:none_of_dz_dx_copy": [-1, "ln_bwd: need dz or dx"],
  "uniter_ln_bwd:H_6": [-2, "ln_bwd: H must be a multiple of 4"],
  "uniter_ln_bwd:H_1028": [-2, "layernorm: hidden size 1028 unsupported (max 1024)"],
  "uniter_ln_bwd_b16:null_dy": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_b16:null_z": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_b16:null_mean": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_b16:null_rstd": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_b16:null_gamma": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_b16:null_ws": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_b16:null_dgamma": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_b16:null_dbeta": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_b16:ws_one_byte_short": [-1, "ln_bwd: workspace too small"],
  "uniter_ln_bwd_b16:none_of_dz_dx_copy": [-1, "ln_bwd: need dz or dx"],
  "uniter_ln_bwd_b16:H_6": [-2, "ln_bwd: H must be a multiple of 4"],
  "uniter_ln_bwd_b16:H_1028": [-2, "layernorm: hidden size 1028 unsupported (max 1024)"],
  "uniter_ln_bwd_rows:null_dy": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows:null_z": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows:null_mean": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows:null_rstd": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows:null_gamma": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows:null_ws": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows:ws_one_byte_short": [-1, "ln_bwd: workspace too small"],
  "uniter_ln_bwd_rows:none_of_dz_dx_copy": [-1, "ln_bwd: need dz or dx"],
  "uniter_ln_bwd_rows:H_6": [-2, "ln_bwd: H must be a multiple of 4"],
  "uniter_ln_bwd_rows:H_1028": [-2, "layernorm: hidden size 1028 unsupported (max 1024)"],
  "uniter_ln_bwd_rows_slabs:null_dy": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs:null_z": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs:null_mean": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs:null_rstd": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs:null_gamma": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs:null_ws": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs:nslab_0": [-1, "ln_bwd: bad slab count / stride"],
  "uniter_ln_bwd_rows_slabs:slab_stride_below_MH": [-1, "ln_bwd: bad slab count / stride"],
  "uniter_ln_bwd_rows_slabs:ws_one_byte_short": [-1, "ln_bwd: workspace too small"],
  "uniter_ln_bwd_rows_slabs:none_of_dz_dx_copy": [-1, "ln_bwd: need dz or dx"],
  "uniter_ln_bwd_rows_slabs:H_6": [-2, "ln_bwd: H must be a multiple of 4"],
  "uniter_ln_bwd_rows_slabs:H_1028": [-2, "layernorm: hidden size 1028 unsupported (max 1024)"],
  "uniter_ln_bwd_rows_slabs_x3:null_dy": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs_x3:null_z": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs_x3:null_mean": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs_x3:null_rstd": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs_x3:null_gamma": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs_x3:null_ws": [-1, "ln_bwd: null pointer"],
  "uniter_ln_bwd_rows_slabs_x3:nslab_0": [-1, "ln_bwd: bad slab count / stride"],
  "uniter_ln_bwd_rows_slabs_x3:slab_stride_below_MH": [-1, "ln_bwd: bad slab count / stride"],
  "uniter_ln_bwd_rows_slabs_x3:ws_one_byte_short": [-1, "ln_bwd: workspace too small"],
  "uniter_ln_bwd_rows_slabs_x3:none_of_dz_dx_copy": [-1, "ln_bwd: need dz or dx"],
  "uniter_ln_bwd_rows_slabs_x3:H_6": [-2, "ln_bwd: the x3 copy needs H % 8 == 0 and a 16-byte aligned buffer"],
  "uniter_ln_bwd_rows_slabs_x3:H_1028": [-2, "ln_bwd: the x3 copy needs H % 8 == 0 and a 16-byte aligned buffer"],
  "uniter_ln_bwd_rows_slabs_x3:H_12": [-2, "ln_bwd: the x3 copy needs H % 8 == 0 and a 16-byte aligned buffer"],
  "uniter_ln_bwd_rows_slabs_x3:misaligned_copy": [-2, "ln_bwd: the x3 copy needs H % 8 == 0 and a 16-byte aligned buffer"],
  "uniter_ln_bwd_finalize:null_ws": [-1, "ln_bwd_finalize: bad argument"],
  "uniter_ln_bwd_finalize:null_dgamma": [-1, "ln_bwd_finalize: bad argument"],
  "uniter_ln_bwd_finalize:null_dbeta": [-1, "ln_bwd_finalize: bad argument"],
  "uniter_ln_bwd_finalize:ws_one_byte_short": [-1, "ln_bwd_finalize: bad argument"],
  "uniter_hidden_keep_bits_gen:null_bits": [-1, "hidden_keep_bits_gen: bad argument"],
  "uniter_hidden_keep_bits_gen:nsites_0": [-1, "hidden_keep_bits_gen: bad argument"],
  "uniter_hidden_keep_bits_gen:elements_0": [-1, "hidden_keep_bits_gen: bad argument"],
  "uniter_hidden_keep_bits_gen:p_zero": [-1, "hidden_keep_bits_gen: bad argument"],
  "uniter_hidden_keep_bits_gen:p_one": [-1, "hidden_keep_bits_gen: bad argument"],
  "uniter_hidden_keep_bits_gen:elements_6": [-2, "hidden_keep_bits_gen: elements % 4, a 4-byte aligned buffer and site stride >= uniter_hidden_keep_bits_bytes"],
  "uniter_hidden_keep_bits_gen:site_stride_6": [-2, "hidden_keep_bits_gen: elements % 4, a 4-byte aligned buffer and site stride >= uniter_hidden_keep_bits_bytes"],
  "uniter_hidden_keep_bits_gen:site_stride_short": [-2, "hidden_keep_bits_gen: elements % 4, a 4-byte aligned buffer and site stride >= uniter_hidden_keep_bits_bytes"],
  "uniter_hidden_keep_bits_gen:misaligned_bits": [-2, "hidden_keep_bits_gen: elements % 4, a 4-byte aligned buffer and site stride >= uniter_hidden_keep_bits_bytes"],
  "uniter_colsum_f32:null_X": [-1, "colsum: null pointer"],
  "uniter_colsum_f32:null_out": [-1, "colsum: null pointer"],
  "uniter_colsum_f32:null_ws": [-1, "colsum: null pointer"],
  "uniter_colsum_f32:N_6": [-2, "colsum: N and ld must be multiples of 4"],
  "uniter_colsum_f32:ld_6": [-2, "colsum: N and ld must be multiples of 4"],
  "uniter_colsum_f32:ws_one_byte_short": [-1, "colsum: workspace too small"],
  "uniter_slab_reduce_add:null_slabs": [-1, "slab_reduce_add: bad argument"],
  "uniter_slab_reduce_add:null_out": [-1, "slab_reduce_add: bad argument"],
  "uniter_slab_reduce_add:nslab_0": [-1, "slab_reduce_add: bad argument"],
  "uniter_slab_reduce_add:n_6": [-2, "slab_reduce_add: n and the slab stride must be multiples of 4, buffers 16-byte aligned"],
  "uniter_slab_reduce_add:slab_stride_6": [-2, "slab_reduce_add: n and the slab stride must be multiples of 4, buffers 16-byte aligned"],
  "uniter_slab_reduce_add:misaligned_slabs": [-2, "slab_reduce_add: n and the slab stride must be multiples of 4, buffers 16-byte aligned"],
  "uniter_slab_reduce_add:misaligned_out": [-2, "slab_reduce_add: n and the slab stride must be multiples of 4, buffers 16-byte aligned"],
  "uniter_colsum_bf16_add:null_X": [-1, "colsum_bf16: bad argument"],
  "uniter_colsum_bf16_add:null_out": [-1, "colsum_bf16: bad argument"],
  "uniter_colsum_bf16_add:M_0": [-1, "colsum_bf16: bad argument"],
  "uniter_colsum_bf16_add:N_0": [-1, "colsum_bf16: bad argument"],
  "uniter_colsum_bf16_add:N_12": [-2, "colsum_bf16: N, ld multiples of 8 and a 16-byte aligned operand required"],
  "uniter_colsum_bf16_add:ld_12": [-2, "colsum_bf16: N, ld multiples of 8 and a 16-byte aligned operand required"],
  "uniter_colsum_bf16_add:misaligned_X": [-2, "colsum_bf16: N, ld multiples of 8 and a 16-byte aligned operand required"],
  "uniter_colsum_bf16_add_det:null_X": [-1, "colsum_bf16_det: bad argument"],
  "uniter_colsum_bf16_add_det:null_out": [-1, "colsum_bf16_det: bad argument"],
  "uniter_colsum_bf16_add_det:null_ws": [-1, "colsum_bf16_det: bad argument"],
  "uniter_colsum_bf16_add_det:M_0": [-1, "colsum_bf16_det: bad argument"],
  "uniter_colsum_bf16_add_det:N_0": [-1, "colsum_bf16_det: bad argument"],
  "uniter_colsum_bf16_add_det:ld_below_N": [-1, "colsum_bf16_det: bad argument"],
  "uniter_colsum_bf16_add_det:N_12": [-2, "colsum_bf16_det: N, ld multiples of 8, a 16-byte aligned operand and 4-byte aligned out / ws required"],
  "uniter_colsum_bf16_add_det:ld_12": [-2, "colsum_bf16_det: N, ld multiples of 8, a 16-byte aligned operand and 4-byte aligned out / ws required"],
  "uniter_colsum_bf16_add_det:misaligned_X": [-2, "colsum_bf16_det: N, ld multiples of 8, a 16-byte aligned operand and 4-byte aligned out / ws required"],
  "uniter_colsum_bf16_add_det:misaligned_out": [-2, "colsum_bf16_det: N, ld multiples of 8, a 16-byte aligned operand and 4-byte aligned out / ws required"],
  "uniter_colsum_bf16_add_det:misaligned_ws": [-2, "colsum_bf16_det: N, ld multiples of 8, a 16-byte aligned operand and 4-byte aligned out / ws required"],
  "uniter_colsum_bf16_add_det:ws_one_byte_short": [-1, "colsum_bf16_det: workspace too small"],
  "uniter_txt_embed_fwd:null_ids": [-1, "txt_embed_fwd: null pointer"],
  "uniter_txt_embed_fwd:null_pos_ids": [-1, "txt_embed_fwd: null pointer"],
  "uniter_txt_embed_fwd:null_word": [-1, "txt_embed_fwd: null pointer"],
  "uniter_txt_embed_fwd:null_pos": [-1, "txt_embed_fwd: null pointer"],
  "uniter_txt_embed_fwd:null_type": [-1, "txt_embed_fwd: null pointer"],
  "uniter_txt_embed_fwd:null_gamma": [-1, "txt_embed_fwd: null pointer"],
  "uniter_txt_embed_fwd:null_beta": [-1, "txt_embed_fwd: null pointer"],
  "uniter_txt_embed_fwd:null_cat": [-1, "txt_embed_fwd: null pointer"],
  "uniter_txt_embed_fwd:H_6": [-2, "txt_embed_fwd: bad shape"],
  "uniter_txt_embed_fwd:H_1028": [-2, "embed: hidden size 1028 unsupported (max 1024)"],
  "uniter_txt_embed_fwd:T_above_S": [-2, "txt_embed_fwd: bad shape"],
  "uniter_txt_embed_fwd_delta:null_ids": [-1, "txt_embed_fwd_delta: null pointer"],
  "uniter_txt_embed_fwd_delta:null_pos_ids": [-1, "txt_embed_fwd_delta: null pointer"],
  "uniter_txt_embed_fwd_delta:null_word": [-1, "txt_embed_fwd_delta: null pointer"],
  "uniter_txt_embed_fwd_delta:null_pos": [-1, "txt_embed_fwd_delta: null pointer"],
  "uniter_txt_embed_fwd_delta:null_type": [-1, "txt_embed_fwd_delta: null pointer"],
  "uniter_txt_embed_fwd_delta:null_gamma": [-1, "txt_embed_fwd_delta: null pointer"],
  "uniter_txt_embed_fwd_delta:null_beta": [-1, "txt_embed_fwd_delta: null pointer"],
  "uniter_txt_embed_fwd_delta:null_cat": [-1, "txt_embed_fwd_delta: null pointer"],
  "uniter_txt_embed_fwd_delta:H_6": [-2, "txt_embed_fwd_delta: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_fwd_delta:H_1028": [-2, "txt_embed_fwd_delta: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_fwd_delta:T_above_S": [-2, "txt_embed_fwd_delta: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_fwd_delta:misaligned_delta": [-1, "txt_embed_fwd_delta: delta must be 16-byte aligned"],
  "uniter_txt_embed_bwd:null_dcat": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_ids": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_pos_ids": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_word": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_pos": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_type": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_gamma": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_dword": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_dpos": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_dtype": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_dgamma": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_dbeta": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:null_ws": [-1, "txt_embed_bwd: null pointer"],
  "uniter_txt_embed_bwd:H_6": [-2, "txt_embed_bwd: bad shape"],
  "uniter_txt_embed_bwd:H_1028": [-2, "embed: hidden size 1028 unsupported (max 1024)"],
  "uniter_txt_embed_bwd:T_above_S": [-2, "txt_embed_bwd: bad shape"],
  "uniter_txt_embed_bwd:ws_one_byte_short": [-1, "txt_embed_bwd: workspace too small"],
  "uniter_txt_embed_bwd_det:null_dcat": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_ids": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_pos_ids": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_word": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_pos": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_type": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_gamma": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_dword": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_dpos": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_dtype": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_dgamma": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_dbeta": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:null_ws": [-1, "txt_embed_bwd_det: null pointer"],
  "uniter_txt_embed_bwd_det:H_6": [-2, "txt_embed_bwd_det: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_bwd_det:H_1028": [-2, "txt_embed_bwd_det: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_bwd_det:T_above_S": [-2, "txt_embed_bwd_det: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_bwd_det:ws_one_byte_short": [-1, "txt_embed_bwd_det: workspace too small"],
  "uniter_txt_embed_bwd_det:rows_above_the_cap": [-2, "txt_embed_bwd_det: 24579 rows, the stable rank covers at most 16384"],
  "uniter_txt_embed_bwd_rows:null_dcat": [-1, "txt_embed_bwd_rows: null pointer"],
  "uniter_txt_embed_bwd_rows:null_ids": [-1, "txt_embed_bwd_rows: null pointer"],
  "uniter_txt_embed_bwd_rows:null_pos_ids": [-1, "txt_embed_bwd_rows: null pointer"],
  "uniter_txt_embed_bwd_rows:null_word": [-1, "txt_embed_bwd_rows: null pointer"],
  "uniter_txt_embed_bwd_rows:null_pos": [-1, "txt_embed_bwd_rows: null pointer"],
  "uniter_txt_embed_bwd_rows:null_type": [-1, "txt_embed_bwd_rows: null pointer"],
  "uniter_txt_embed_bwd_rows:null_gamma": [-1, "txt_embed_bwd_rows: null pointer"],
  "uniter_txt_embed_bwd_rows:null_d_rows": [-1, "txt_embed_bwd_rows: null pointer"],
  "uniter_txt_embed_bwd_rows:H_6": [-2, "txt_embed_bwd_rows: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_bwd_rows:H_1028": [-2, "txt_embed_bwd_rows: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_bwd_rows:T_above_S": [-2, "txt_embed_bwd_rows: bad shape (H % 4, H <= 1024, T <= S)"],
  "uniter_txt_embed_bwd_rows:misaligned_delta": [-1, "txt_embed_bwd_rows: delta and d_rows must be 16-byte aligned"],
  "uniter_txt_embed_bwd_rows:misaligned_d_rows": [-1, "txt_embed_bwd_rows: delta and d_rows must be 16-byte aligned"],
  "uniter_img_embed_fwd:null_imgfc": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_pos7": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_Wp": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_bp": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_type": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_g_i": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_b_i": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_g_p": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_b_p": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_g_f": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_b_f": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:null_cat": [-1, "img_embed_fwd: null pointer"],
  "uniter_img_embed_fwd:H_6": [-2, "img_embed_fwd: bad shape"],
  "uniter_img_embed_fwd:H_1028": [-2, "embed: hidden size 1028 unsupported (max 1024)"],
  "uniter_img_embed_fwd:T0_plus_R_above_S": [-2, "img_embed_fwd: bad shape"],
  "uniter_img_embed_fwd:type_vocab_1": [-2, "img_embed_fwd: bad shape"],
  "uniter_img_embed_bwd:null_dcat": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_imgfc": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_pos7": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_Wp": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_bp": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_type": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_g_i": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_b_i": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_g_p": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_b_p": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_g_f": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_stats": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_d_imgfc": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_d_posfc": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_dWp": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_dbp": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_dtype": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_dg_i": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_db_i": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_dg_p": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_db_p": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_dg_f": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_db_f": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:null_ws": [-1, "img_embed_bwd: null pointer"],
  "uniter_img_embed_bwd:H_6": [-2, "img_embed_bwd: bad shape"],
  "uniter_img_embed_bwd:H_1028": [-2, "embed: hidden size 1028 unsupported (max 1024)"],
  "uniter_img_embed_bwd:T0_plus_R_above_S": [-2, "img_embed_bwd: bad shape"],
  "uniter_img_embed_bwd:type_vocab_1": [-2, "img_embed_bwd: bad shape"],
  "uniter_img_embed_bwd:ws_one_byte_short": [-1, "img_embed_bwd: workspace too small"],
  "uniter_img_embed_bwd_det:null_dcat": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_imgfc": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_pos7": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_Wp": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_bp": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_type": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_g_i": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_b_i": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_g_p": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_b_p": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_g_f": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_stats": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_d_imgfc": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_d_posfc": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_dWp": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_dbp": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_dtype": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_dg_i": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_db_i": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_dg_p": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_db_p": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_dg_f": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_db_f": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:null_ws": [-1, "img_embed_bwd_det: null pointer"],
  "uniter_img_embed_bwd_det:H_6": [-2, "img_embed_bwd_det: bad shape (H % 4, H <= 1024, T0 + R <= S, type_vocab >= 2)"],
  "uniter_img_embed_bwd_det:H_1028": [-2, "img_embed_bwd_det: bad shape (H % 4, H <= 1024, T0 + R <= S, type_vocab >= 2)"],
  "uniter_img_embed_bwd_det:T0_plus_R_above_S": [-2, "img_embed_bwd_det: bad shape (H % 4, H <= 1024, T0 + R <= S, type_vocab >= 2)"],
  "uniter_img_embed_bwd_det:type_vocab_1": [-2, "img_embed_bwd_det: bad shape (H % 4, H <= 1024, T0 + R <= S, type_vocab >= 2)"],
  "uniter_img_embed_bwd_det:ws_one_byte_short": [-1, "img_embed_bwd_det: workspace too small"],
  "uniter_img_embed_bwd_det:rows_above_the_cap": [-2, "img_embed_bwd_det: 16386 rows, the stable rank covers at most 16384"]
},
"numbers": {
  "uniter_grad_sumsq_ws_bytes:n192": 8,
  "uniter_grad_sumsq_ws_bytes:n110000000": 16384,
  "uniter_grad_sumsq_ws_bytes:n2097152": 16384,
  "uniter_grad_sumsq_ws_bytes:n0": 8,
  "uniter_ln_bwd_ws_bytes:M5_H64": 768,
  "uniter_ln_bwd_ws_bytes:M2624_H768": 3022848,
  "uniter_ln_bwd_ws_bytes:M1048576_H1024": 12582912,
  "uniter_ln_bwd_ws_bytes:M0_H64": 768,
  "uniter_colsum_ws_bytes:M5_N64": 256,
  "uniter_colsum_ws_bytes:M2624_N3072": 786432,
  "uniter_colsum_ws_bytes:M2048_N768": 196608,
  "uniter_colsum_ws_bytes:M0_N64": 256,
  "uniter_colsum_det_ws_bytes:M5_N64": 256,
  "uniter_colsum_det_ws_bytes:M2624_N3072": 503808,
  "uniter_colsum_det_ws_bytes:M64_N768": 3072,
  "uniter_colsum_det_ws_bytes:M0_N64": 0,
  "uniter_hidden_keep_bits_bytes:n320": 40,
  "uniter_hidden_keep_bits_bytes:n2015232": 251904,
  "uniter_hidden_keep_bits_bytes:n28": 4,
  "uniter_hidden_keep_bits_bytes:n0": 0,
  "uniter_embed_bwd_ws_bytes:rows6_H64": 3584,
  "uniter_embed_bwd_ws_bytes:rows2048_H768": 5505024,
  "uniter_embed_bwd_ws_bytes:rows1024_H1024": 7340032,
  "uniter_embed_bwd_ws_bytes:rows0_H64": 1792,
  "uniter_embed_bwd_det_ws_bytes:txt6_img4_H64": 5408,
  "uniter_embed_bwd_det_ws_bytes:txt2048_img576_H768": 9879552,
  "uniter_embed_bwd_det_ws_bytes:txt16384_img16384_H1024": 95551488,
  "uniter_embed_bwd_det_ws_bytes:txt0_img0_H64": 0
}}
''')
EXPECTED_LNB8 = json.loads(r'''
{"refused": {

},
"numbers": {
  "uniter_ln_bwd_ws_bytes:M5_H64": 768,
  "uniter_ln_bwd_ws_bytes:M2624_H768": 3022848,
  "uniter_ln_bwd_ws_bytes:M1048576_H1024": 12582912,
  "uniter_ln_bwd_ws_bytes:M0_H64": 768
}}
''')


def _observe(extra_env, *mode):
    from meme_challenge_amd import _lib
    env = dict({k: v for k, v in os.environ.items() if not k.startswith('UNITER_')}, HIP_VISIBLE_DEVICES='-1', **extra_env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _lib.LIB_PATH, *mode], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def observed():
    return _observe({})      # no GPU, and the switches' defaults


@pytest.fixture(scope='module')
def observed_lnb8():
    return _observe(dict(UNITER_LNB_WAVES='8', UNITER_LNB_ROWS='1'), 'lnb8')


def _ids(rows):
    return ['%s:%s' % (f, n) for f, n, _ in rows]


def test_the_table_is_recorded_in_full():
    assert sorted(EXPECTED['refused']) == sorted(_ids(REFUSED)) and sorted(EXPECTED['numbers']) == sorted(_ids(NUMBERS))
    assert sorted(EXPECTED_LNB8['numbers']) == sorted(_ids(NUMBERS_LNB8))
    assert (len(_OPTIM), len(_LN) + 1, len(_EMBED)) == (11, 10, 8) and len(set(_ids(REFUSED))) == len(REFUSED)
    assert all(rc in (E_ARG, E_SHAPE) and message for rc, message in EXPECTED['refused'].values())


@pytest.mark.parametrize('row', _ids(REFUSED))
def test_refused_with_the_recorded_code_and_message(observed, row):
    assert observed['refused'][row] == EXPECTED['refused'][row]


@pytest.mark.parametrize('row', _ids(NUMBERS))
def test_sizes_are_the_recorded_integers(observed, row):
    assert observed['numbers'][row] == EXPECTED['numbers'][row]


@pytest.mark.parametrize('row', _ids(NUMBERS_LNB8))
def test_the_backward_row_pass_workspace_at_eight_waves_of_one_row(observed_lnb8, row):
    assert observed_lnb8['numbers'][row] == EXPECTED_LNB8['numbers'][row]
