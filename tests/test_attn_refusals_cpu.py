"""CPU: the attention entry points of the C ABI refuse bad calls before any HIP call, with the return code and the message prefix
recorded from the library before the launcher layer took AttnCall; the workspace and keep-flag size functions (host arithmetic)
return the integers recorded from that same library.

Every row of REFUSED is a call that must be refused: pointers are fake aligned integers that nothing may dereference.  So that
a regression (a row that is no longer refused) cannot reach a device with them, the table runs in ONE child process that
sees no GPU (HIP_VISIBLE_DEVICES=-1) and loads the library with ctypes alone: `python tests/test_attn_refusals_cpu.py LIB`
prints the observed values as JSON, and the tests compare them with the literals below.  A second child runs with
UNITER_ATTN_SPLIT=0 (`... LIB split0`): uniter_attn_varlen_max_len() is 0 there, and the fp32 forms limited to it refuse L = 32."""
import ctypes as C
import json
import os
import subprocess
import sys

(QKV, MASK, CU, CTX, LSE, DCTX, DQKV, COPY, PART, KEEP, DELTA, WS) = (0x10000 * (i + 1) for i in range(12))      # fake 64-KiB aligned pointers
ODD = 4                                         # added to a pointer: 4-byte aligned only
B, L, NH = 2, 33, 2                             # the valid call of every row: two samples, two heads, 33 rows (Lr = 64)
WS_F32, WS_BF16 = 2 * B * NH * 64 * 64 * 4, 2 * B * NH * 64 * 64 * 2
WS_BIG = 1 << 30

# ---- the entry points: (ctypes signature, parameter names with the defaults of one valid call) ----
# i = int, p = pointer, f = float, q = uint64, u = uint32, z = size_t
_DIMS = dict(B=B, L=L, nh=NH, p=0.0)
_RNG = dict(seed=1, offset=0, site=3)
_OUT = dict(ctx=CTX, copy=COPY, lse=LSE)
_GRADS = dict(dqkv=DQKV, copy=COPY, part=PART, keep=None, delta=DELTA)
_WS32, _WS16 = dict(ws=WS, ws_bytes=WS_F32), dict(ws=WS, ws_bytes=WS_BF16)
_S = dict(stream=None)
_BWD_IN = dict(ctx=CTX, lse=LSE, dctx=DCTX)
FUNCS = {
    'uniter_attn_fwd': ('ppppiiifquup', dict(qkv=QKV, mask=MASK, ctx=CTX, lse=LSE, **_DIMS, **_RNG, **_S)),
    'uniter_attn_bwd': ('pppppppiiifquupzp', dict(qkv=QKV, mask=MASK, **_BWD_IN, dqkv=DQKV, delta=DELTA, **_DIMS, **_RNG, **_WS32, **_S)),
    'uniter_attn_fwd_varlen': ('ppppiiifquup', dict(qkv=QKV, cu=CU, ctx=CTX, lse=LSE, **_DIMS, **_RNG, **_S)),
    'uniter_attn_bwd_varlen': ('pppppppiiifquupzp', dict(qkv=QKV, cu=CU, **_BWD_IN, dqkv=DQKV, delta=DELTA, **_DIMS, **_RNG, **_WS32, **_S)),
    'uniter_attn_fwd_ex': ('pppppppiiifquup', dict(qkv=QKV, mask=MASK, cu=None, **_OUT, keep=None, **_DIMS, **_RNG, **_S)),
    'uniter_attn_fwd_pre': ('pppppppiiiifquup', dict(qkv=QKV, mask=MASK, cu=None, **_OUT, keep=None, keep_ready=0, **_DIMS, **_RNG, **_S)),
    'uniter_attn_fwd_pre_x3': ('pppppppiiiifquup', dict(qkv=QKV, mask=MASK, cu=None, **_OUT, keep=None, keep_ready=0, **_DIMS, **_RNG, **_S)),
    'uniter_attn_bwd_ex': ('pppppppppppiiifquupzp', dict(qkv=QKV, mask=MASK, cu=None, **_BWD_IN, **_GRADS, **_DIMS, **_RNG, **_WS32, **_S)),
    'uniter_attn_bwd_ex_x3': ('pppppppppppiiifquupzp', dict(qkv=QKV, mask=MASK, cu=None, **_BWD_IN, **_GRADS, **_DIMS, **_RNG, **_WS32, **_S)),
    'uniter_attn_x3_fwd': ('pppppppiiifp', dict(qkv=QKV, mask=MASK, cu=None, **_OUT, keep=None, **_DIMS, **_S)),
    'uniter_attn_x3_bwd': ('ppppppizpppppiiifp', dict(qkv=QKV, mask=MASK, cu=None, **_BWD_IN, slabs=1, slab_stride=0, **_GRADS, **_DIMS, **_S)),
    'uniter_attn_b16x_fwd': ('pippppppiiifp', dict(qkv=QKV, qkv_is_bf16=1, mask=MASK, cu=None, **_OUT, keep=None, **_DIMS, **_S)),
    'uniter_attn_b16x_bwd': ('pippppppppppiiifp', dict(qkv=QKV, qkv_is_bf16=1, mask=MASK, cu=None, **_BWD_IN, **_GRADS, **_DIMS, **_S)),
    'uniter_attn_bf16_fwd': ('pippppppiiifquup', dict(qkv=QKV, qkv_is_bf16=1, mask=MASK, cu=None, **_OUT, keep=None, **_DIMS, **_RNG, **_S)),
    'uniter_attn_bf16_fwd_pre': ('pippppppiiiifquup', dict(qkv=QKV, qkv_is_bf16=1, mask=MASK, cu=None, **_OUT, keep=None, keep_ready=0, **_DIMS,
                                                           **_RNG, **_S)),
    'uniter_attn_bf16_bwd': ('pippppppppppiiifquupzp', dict(qkv=QKV, qkv_is_bf16=1, mask=MASK, cu=None, **_BWD_IN, **_GRADS, **_DIMS, **_RNG,
                                                             **_WS16, **_S)),
    'uniter_attn_keep_bits_gen': ('pziiiifquuup', dict(keep=KEEP, layer_stride=1 << 16, nlayers=2, **_DIMS, seed=1, offset=0, site0=3,
                                                       site_step=8, **_S)),
}
LAUNCHERS = [f for f in FUNCS if f != 'uniter_attn_keep_bits_gen']      # the 16 launch entry points
ANY_LENGTH = ('uniter_attn_fwd', 'uniter_attn_bwd')                     # every other form has the L <= 192 kernels only
PIECES = ('uniter_attn_x3_fwd', 'uniter_attn_x3_bwd', 'uniter_attn_b16x_fwd', 'uniter_attn_b16x_bwd')      # attention_x3.hip
# the fp32 forms limited to uniter_attn_varlen_max_len()
SPLIT_ONLY = ('uniter_attn_fwd_varlen', 'uniter_attn_bwd_varlen', 'uniter_attn_fwd_ex', 'uniter_attn_fwd_pre', 'uniter_attn_fwd_pre_x3',
              'uniter_attn_bwd_ex', 'uniter_attn_bwd_ex_x3')
# the pointers an entry point cannot do without (the outputs that have an alternative -- ctx / its copy, dqkv / its copy -- below)
_FWD_PTRS, _BWD_PTRS = ('qkv', 'ctx'), ('qkv', 'ctx', 'lse', 'dctx', 'delta')
REQUIRED = {
    'uniter_attn_fwd': ('qkv', 'mask', 'ctx'), 'uniter_attn_bwd': _BWD_PTRS + ('mask', 'dqkv'),
    'uniter_attn_fwd_varlen': ('qkv', 'cu', 'ctx'), 'uniter_attn_bwd_varlen': _BWD_PTRS + ('cu', 'dqkv'),
    'uniter_attn_fwd_ex': _FWD_PTRS, 'uniter_attn_fwd_pre': _FWD_PTRS, 'uniter_attn_fwd_pre_x3': _FWD_PTRS,
    'uniter_attn_bwd_ex': _BWD_PTRS + ('dqkv',), 'uniter_attn_bwd_ex_x3': _BWD_PTRS,
    'uniter_attn_x3_fwd': ('qkv',), 'uniter_attn_x3_bwd': _BWD_PTRS, 'uniter_attn_b16x_fwd': ('qkv',), 'uniter_attn_b16x_bwd': _BWD_PTRS,
    'uniter_attn_bf16_fwd': _FWD_PTRS, 'uniter_attn_bf16_fwd_pre': _FWD_PTRS, 'uniter_attn_bf16_bwd': _BWD_PTRS,
}


def _launcher_rows(fn):
    d = FUNCS[fn][1]
    rows = [('null_' + name, {name: None}) for name in REQUIRED[fn]]
    if 'mask' in d and 'cu' in d:
        rows += [('mask_and_cu_seqlens', dict(cu=CU)), ('neither_mask_nor_cu_seqlens', dict(mask=None))]
    rows += [('B_0', dict(B=0)), ('L_0', dict(L=0)), ('nh_0', dict(nh=0)), ('p_negative', dict(p=-0.25)), ('p_one', dict(p=1.0))]
    if fn not in ANY_LENGTH:
        rows += [('L_193', dict(L=193, ws_bytes=WS_BIG) if 'ws' in d else dict(L=193))]
    if 'keep_ready' in d:
        rows += [('ready_without_keep_bits', dict(keep_ready=1, p=0.1))]
    if fn in PIECES:
        rows += [('dropout_without_keep_bits', dict(p=0.1)), ('misaligned_qkv', dict(qkv=QKV + ODD)), ('misaligned_ctx', dict(ctx=CTX + ODD)),
                 ('misaligned_copy', dict(copy=COPY + ODD))]
        if 'dctx' in d:
            rows += [('misaligned_dctx', dict(dctx=DCTX + ODD)), ('misaligned_dqkv', dict(dqkv=DQKV + ODD))]
        else:
            rows += [('neither_ctx_nor_copy', dict(ctx=None, copy=None))]
    if fn in ('uniter_attn_fwd_pre_x3', 'uniter_attn_bwd_ex_x3'):
        rows += [('misaligned_pieces', dict(copy=COPY + ODD)), ('null_pieces', dict(copy=None))]
    if 'dqkv' in d and 'copy' in d:
        rows += [('neither_dqkv_nor_copy', dict(dqkv=None, copy=None))]
    if 'slabs' in d:
        rows += [('slabs_0', dict(slabs=0)), ('slabs_5', dict(slabs=5)), ('slab_stride_6', dict(slabs=2, slab_stride=6))]
    if 'ws' in d:
        rows += [('null_ws', dict(ws=None)), ('ws_one_byte_short', dict(ws_bytes=d['ws_bytes'] - 1))]
    return [(fn, name, kw) for name, kw in rows]


GEN = 'uniter_attn_keep_bits_gen'
REFUSED = [row for fn in LAUNCHERS for row in _launcher_rows(fn)] + [
    (GEN, 'null_keep_bits', dict(keep=None)), (GEN, 'nlayers_0', dict(nlayers=0)), (GEN, 'nlayers_65536', dict(nlayers=65536)),
    (GEN, 'B_0', dict(B=0)), (GEN, 'L_0', dict(L=0)), (GEN, 'nh_0', dict(nh=0)), (GEN, 'odd_layer_stride', dict(layer_stride=(1 << 16) + 1)),
    (GEN, 'p_negative', dict(p=-0.25)), (GEN, 'p_one', dict(p=1.0)), (GEN, 'L_193', dict(L=193, layer_stride=1 << 20)),
    (GEN, 'layers_overlap', dict(layer_stride=1054))]      # one layer: 2 * 2 * 33 * 2 * 2 words of 2 bytes = 1056
# UNITER_ATTN_SPLIT=0: the valid call of each fp32 form that has only the L <= 192 kernels, at L = 32
REFUSED_SPLIT0 = [(fn, 'L_32', dict(L=32)) for fn in SPLIT_ONLY]

# ---- host arithmetic ----
SIZES = ('uniter_attn_bwd_ws_bytes', 'uniter_attn_bf16_bwd_ws_bytes', 'uniter_attn_keep_bits_bytes')
SHAPES = ((2, 33, 2), (16, 164, 12), (1, 192, 1), (1, 193, 1), (0, 32, 1))
NUMBERS = [(fn, 'B%d_L%d_nh%d' % s, s) for fn in SIZES for s in SHAPES] + [('uniter_attn_varlen_max_len', 'value', ()),
                                                                             ('uniter_attn_x3_max_len', 'value', ())]
NUMBERS_SPLIT0 = [('uniter_attn_bwd_ws_bytes', 'B%d_L%d_nh%d' % s, s) for s in SHAPES[:1]] + [('uniter_attn_varlen_max_len', 'value', ())]

_CT = {'i': C.c_int, 'p': C.c_void_p, 'f': C.c_float, 'q': C.c_uint64, 'u': C.c_uint32, 'z': C.c_size_t}


def _call(lib, fn, overrides):
    sig, defaults = FUNCS[fn]
    unknown = set(overrides) - set(defaults)
    assert not unknown and len(sig) == len(defaults), (fn, unknown, len(sig), len(defaults))
    f = getattr(lib, fn)
    f.restype, f.argtypes = C.c_int, [_CT[ch] for ch in sig]
    return f(*dict(defaults, **overrides).values())


def observe(lib_path, split0):
    """{'refused': {id: [rc, message prefix]}, 'numbers': {id: value}} of the library at lib_path"""
    lib = C.CDLL(lib_path)
    lib.uniter_last_error.restype = C.c_char_p
    out = {'refused': {}, 'numbers': {}}
    for fn, name, kw in (REFUSED_SPLIT0 if split0 else REFUSED):
        rc = _call(lib, fn, kw)
        out['refused']['%s:%s' % (fn, name)] = [rc, lib.uniter_last_error().decode().split(':')[0] if rc else '']
    for fn, name, args in (NUMBERS_SPLIT0 if split0 else NUMBERS):
        f = getattr(lib, fn)
        f.restype, f.argtypes = (C.c_size_t if args else C.c_int), [C.c_int] * len(args)
        out['numbers']['%s:%s' % (fn, name)] = f(*args)
    return out


if __name__ == '__main__':
    print(json.dumps(observe(sys.argv[1], sys.argv[2:] == ['split0'])))
    sys.exit(0)

import pytest      # noqa: E402  (the child process above needs neither pytest nor the package)

E_ARG, E_SHAPE = -1, -2
EXPECTED = json.loads(r'''
{"refused": {
  "uniter_attn_fwd:null_qkv": [-1, "attn_fwd"],
  "uniter_attn_fwd:null_mask": [-1, "attn_fwd"],
  "uniter_attn_fwd:null_ctx": [-1, "attn_fwd"],
  "uniter_attn_fwd:B_0": [-1, "attention"],
  "uniter_attn_fwd:L_0": [-1, "attention"],
  "uniter_attn_fwd:nh_0": [-1, "attention"],
  "uniter_attn_fwd:p_negative": [-1, "attention"],
  "uniter_attn_fwd:p_one": [-1, "attention"],
  "uniter_attn_bwd:null_qkv": [-1, "attn_bwd"],
  "uniter_attn_bwd:null_ctx": [-1, "attn_bwd"],
  "uniter_attn_bwd:null_lse": [-1, "attn_bwd"],
  "uniter_attn_bwd:null_dctx": [-1, "attn_bwd"],
  "uniter_attn_bwd:null_delta": [-1, "attn_bwd"],
  "uniter_attn_bwd:null_mask": [-1, "attn_bwd"],
  "uniter_attn_bwd:null_dqkv": [-1, "attn_bwd"],
  "uniter_attn_bwd:B_0": [-1, "attention"],
  "uniter_attn_bwd:L_0": [-1, "attention"],
  "uniter_attn_bwd:nh_0": [-1, "attention"],
  "uniter_attn_bwd:p_negative": [-1, "attention"],
  "uniter_attn_bwd:p_one": [-1, "attention"],
  "uniter_attn_bwd:null_ws": [-1, "attn_bwd"],
  "uniter_attn_bwd:ws_one_byte_short": [-1, "attn_bwd"],
  "uniter_attn_fwd_varlen:null_qkv": [-1, "attn_fwd_varlen"],
  "uniter_attn_fwd_varlen:null_cu": [-1, "attn_fwd_varlen"],
  "uniter_attn_fwd_varlen:null_ctx": [-1, "attn_fwd_varlen"],
  "uniter_attn_fwd_varlen:B_0": [-1, "attention"],
  "uniter_attn_fwd_varlen:L_0": [-1, "attention"],
  "uniter_attn_fwd_varlen:nh_0": [-1, "attention"],
  "uniter_attn_fwd_varlen:p_negative": [-1, "attention"],
  "uniter_attn_fwd_varlen:p_one": [-1, "attention"],
  "uniter_attn_fwd_varlen:L_193": [-2, "attn_fwd_varlen"],
  "uniter_attn_bwd_varlen:null_qkv": [-1, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:null_ctx": [-1, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:null_lse": [-1, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:null_dctx": [-1, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:null_delta": [-1, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:null_cu": [-1, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:null_dqkv": [-1, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:B_0": [-1, "attention"],
  "uniter_attn_bwd_varlen:L_0": [-1, "attention"],
  "uniter_attn_bwd_varlen:nh_0": [-1, "attention"],
  "uniter_attn_bwd_varlen:p_negative": [-1, "attention"],
  "uniter_attn_bwd_varlen:p_one": [-1, "attention"],
  "uniter_attn_bwd_varlen:L_193": [-2, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:null_ws": [-1, "attn_bwd_varlen"],
  "uniter_attn_bwd_varlen:ws_one_byte_short": [-1, "attn_bwd_varlen"],
  "uniter_attn_fwd_ex:null_qkv": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_ex:null_ctx": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_ex:mask_and_cu_seqlens": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_ex:neither_mask_nor_cu_seqlens": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_ex:B_0": [-1, "attention"],
  "uniter_attn_fwd_ex:L_0": [-1, "attention"],
  "uniter_attn_fwd_ex:nh_0": [-1, "attention"],
  "uniter_attn_fwd_ex:p_negative": [-1, "attention"],
  "uniter_attn_fwd_ex:p_one": [-1, "attention"],
  "uniter_attn_fwd_ex:L_193": [-2, "attn_fwd_ex"],
  "uniter_attn_fwd_pre:null_qkv": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_pre:null_ctx": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_pre:mask_and_cu_seqlens": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_pre:neither_mask_nor_cu_seqlens": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_pre:B_0": [-1, "attention"],
  "uniter_attn_fwd_pre:L_0": [-1, "attention"],
  "uniter_attn_fwd_pre:nh_0": [-1, "attention"],
  "uniter_attn_fwd_pre:p_negative": [-1, "attention"],
  "uniter_attn_fwd_pre:p_one": [-1, "attention"],
  "uniter_attn_fwd_pre:L_193": [-2, "attn_fwd_ex"],
  "uniter_attn_fwd_pre:ready_without_keep_bits": [-1, "attn_fwd_pre"],
  "uniter_attn_fwd_pre_x3:null_qkv": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_pre_x3:null_ctx": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_pre_x3:mask_and_cu_seqlens": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_pre_x3:neither_mask_nor_cu_seqlens": [-1, "attn_fwd_ex"],
  "uniter_attn_fwd_pre_x3:B_0": [-1, "attention"],
  "uniter_attn_fwd_pre_x3:L_0": [-1, "attention"],
  "uniter_attn_fwd_pre_x3:nh_0": [-1, "attention"],
  "uniter_attn_fwd_pre_x3:p_negative": [-1, "attention"],
  "uniter_attn_fwd_pre_x3:p_one": [-1, "attention"],
  "uniter_attn_fwd_pre_x3:L_193": [-2, "attn_fwd_ex"],
  "uniter_attn_fwd_pre_x3:ready_without_keep_bits": [-1, "attn_fwd_pre"],
  "uniter_attn_fwd_pre_x3:misaligned_pieces": [-1, "attn_fwd_pre_x3"],
  "uniter_attn_fwd_pre_x3:null_pieces": [-1, "attn_fwd_pre_x3"],
  "uniter_attn_bwd_ex:null_qkv": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:null_ctx": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:null_lse": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:null_dctx": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:null_delta": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:null_dqkv": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:mask_and_cu_seqlens": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:neither_mask_nor_cu_seqlens": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:B_0": [-1, "attention"],
  "uniter_attn_bwd_ex:L_0": [-1, "attention"],
  "uniter_attn_bwd_ex:nh_0": [-1, "attention"],
  "uniter_attn_bwd_ex:p_negative": [-1, "attention"],
  "uniter_attn_bwd_ex:p_one": [-1, "attention"],
  "uniter_attn_bwd_ex:L_193": [-2, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:neither_dqkv_nor_copy": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:null_ws": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex:ws_one_byte_short": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:null_qkv": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:null_ctx": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:null_lse": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:null_dctx": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:null_delta": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:mask_and_cu_seqlens": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:neither_mask_nor_cu_seqlens": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:B_0": [-1, "attention"],
  "uniter_attn_bwd_ex_x3:L_0": [-1, "attention"],
  "uniter_attn_bwd_ex_x3:nh_0": [-1, "attention"],
  "uniter_attn_bwd_ex_x3:p_negative": [-1, "attention"],
  "uniter_attn_bwd_ex_x3:p_one": [-1, "attention"],
  "uniter_attn_bwd_ex_x3:L_193": [-2, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:misaligned_pieces": [-1, "attn_bwd_ex_x3"],
  "uniter_attn_bwd_ex_x3:null_pieces": [-1, "attn_bwd_ex_x3"],
  "uniter_attn_bwd_ex_x3:neither_dqkv_nor_copy": [-1, "attn_bwd_ex_x3"],
  "uniter_attn_bwd_ex_x3:null_ws": [-1, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:ws_one_byte_short": [-1, "attn_bwd_ex"],
  "uniter_attn_x3_fwd:null_qkv": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:mask_and_cu_seqlens": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:neither_mask_nor_cu_seqlens": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:B_0": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:L_0": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:nh_0": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:p_negative": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:p_one": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:L_193": [-2, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:dropout_without_keep_bits": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:misaligned_qkv": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:misaligned_ctx": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:misaligned_copy": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_fwd:neither_ctx_nor_copy": [-1, "attn_x3_fwd"],
  "uniter_attn_x3_bwd:null_qkv": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:null_ctx": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:null_lse": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:null_dctx": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:null_delta": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:mask_and_cu_seqlens": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:neither_mask_nor_cu_seqlens": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:B_0": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:L_0": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:nh_0": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:p_negative": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:p_one": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:L_193": [-2, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:dropout_without_keep_bits": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:misaligned_qkv": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:misaligned_ctx": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:misaligned_copy": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:misaligned_dctx": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:misaligned_dqkv": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:neither_dqkv_nor_copy": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:slabs_0": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:slabs_5": [-1, "attn_x3_bwd"],
  "uniter_attn_x3_bwd:slab_stride_6": [-1, "attn_x3_bwd"],
  "uniter_attn_b16x_fwd:null_qkv": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:mask_and_cu_seqlens": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:neither_mask_nor_cu_seqlens": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:B_0": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:L_0": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:nh_0": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:p_negative": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:p_one": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:L_193": [-2, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:dropout_without_keep_bits": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:misaligned_qkv": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:misaligned_ctx": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:misaligned_copy": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_fwd:neither_ctx_nor_copy": [-1, "attn_b16x_fwd"],
  "uniter_attn_b16x_bwd:null_qkv": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:null_ctx": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:null_lse": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:null_dctx": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:null_delta": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:mask_and_cu_seqlens": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:neither_mask_nor_cu_seqlens": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:B_0": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:L_0": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:nh_0": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:p_negative": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:p_one": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:L_193": [-2, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:dropout_without_keep_bits": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:misaligned_qkv": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:misaligned_ctx": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:misaligned_copy": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:misaligned_dctx": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:misaligned_dqkv": [-1, "attn_b16x_bwd"],
  "uniter_attn_b16x_bwd:neither_dqkv_nor_copy": [-1, "attn_b16x_bwd"],
  "uniter_attn_bf16_fwd:null_qkv": [-1, "attn_bf16_fwd"],
  "uniter_attn_bf16_fwd:null_ctx": [-1, "attn_bf16_fwd"],
  "uniter_attn_bf16_fwd:mask_and_cu_seqlens": [-1, "attn_bf16_fwd"],
  "uniter_attn_bf16_fwd:neither_mask_nor_cu_seqlens": [-1, "attn_bf16_fwd"],
  "uniter_attn_bf16_fwd:B_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd:L_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd:nh_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd:p_negative": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd:p_one": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd:L_193": [-2, "attn_bf16"],
  "uniter_attn_bf16_fwd_pre:null_qkv": [-1, "attn_bf16_fwd"],
  "uniter_attn_bf16_fwd_pre:null_ctx": [-1, "attn_bf16_fwd"],
  "uniter_attn_bf16_fwd_pre:mask_and_cu_seqlens": [-1, "attn_bf16_fwd"],
  "uniter_attn_bf16_fwd_pre:neither_mask_nor_cu_seqlens": [-1, "attn_bf16_fwd"],
  "uniter_attn_bf16_fwd_pre:B_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd_pre:L_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd_pre:nh_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd_pre:p_negative": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd_pre:p_one": [-1, "attn_bf16"],
  "uniter_attn_bf16_fwd_pre:L_193": [-2, "attn_bf16"],
  "uniter_attn_bf16_fwd_pre:ready_without_keep_bits": [-1, "attn_bf16_fwd_pre"],
  "uniter_attn_bf16_bwd:null_qkv": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:null_ctx": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:null_lse": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:null_dctx": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:null_delta": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:mask_and_cu_seqlens": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:neither_mask_nor_cu_seqlens": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:B_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_bwd:L_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_bwd:nh_0": [-1, "attn_bf16"],
  "uniter_attn_bf16_bwd:p_negative": [-1, "attn_bf16"],
  "uniter_attn_bf16_bwd:p_one": [-1, "attn_bf16"],
  "uniter_attn_bf16_bwd:L_193": [-2, "attn_bf16"],
  "uniter_attn_bf16_bwd:neither_dqkv_nor_copy": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:null_ws": [-1, "attn_bf16_bwd"],
  "uniter_attn_bf16_bwd:ws_one_byte_short": [-1, "attn_bf16_bwd"],
  "uniter_attn_keep_bits_gen:null_keep_bits": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:nlayers_0": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:nlayers_65536": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:B_0": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:L_0": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:nh_0": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:odd_layer_stride": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:p_negative": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:p_one": [-1, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:L_193": [-2, "attn_keep_bits_gen"],
  "uniter_attn_keep_bits_gen:layers_overlap": [-1, "attn_keep_bits_gen"]
},
"numbers": {
  "uniter_attn_bwd_ws_bytes:B2_L33_nh2": 131072,
  "uniter_attn_bwd_ws_bytes:B16_L164_nh12": 56623104,
  "uniter_attn_bwd_ws_bytes:B1_L192_nh1": 294912,
  "uniter_attn_bwd_ws_bytes:B1_L193_nh1": 0,
  "uniter_attn_bwd_ws_bytes:B0_L32_nh1": 0,
  "uniter_attn_bf16_bwd_ws_bytes:B2_L33_nh2": 65536,
  "uniter_attn_bf16_bwd_ws_bytes:B16_L164_nh12": 28311552,
  "uniter_attn_bf16_bwd_ws_bytes:B1_L192_nh1": 147456,
  "uniter_attn_bf16_bwd_ws_bytes:B1_L193_nh1": 0,
  "uniter_attn_bf16_bwd_ws_bytes:B0_L32_nh1": 0,
  "uniter_attn_keep_bits_bytes:B2_L33_nh2": 1056,
  "uniter_attn_keep_bits_bytes:B16_L164_nh12": 755712,
  "uniter_attn_keep_bits_bytes:B1_L192_nh1": 4608,
  "uniter_attn_keep_bits_bytes:B1_L193_nh1": 5404,
  "uniter_attn_keep_bits_bytes:B0_L32_nh1": 0,
  "uniter_attn_varlen_max_len:value": 192,
  "uniter_attn_x3_max_len:value": 192
}}
''')
EXPECTED_SPLIT0 = json.loads(r'''
{"refused": {
  "uniter_attn_fwd_varlen:L_32": [-2, "attn_fwd_varlen"],
  "uniter_attn_bwd_varlen:L_32": [-2, "attn_bwd_varlen"],
  "uniter_attn_fwd_ex:L_32": [-2, "attn_fwd_ex"],
  "uniter_attn_fwd_pre:L_32": [-2, "attn_fwd_ex"],
  "uniter_attn_fwd_pre_x3:L_32": [-2, "attn_fwd_ex"],
  "uniter_attn_bwd_ex:L_32": [-2, "attn_bwd_ex"],
  "uniter_attn_bwd_ex_x3:L_32": [-2, "attn_bwd_ex"]
},
"numbers": {
  "uniter_attn_bwd_ws_bytes:B2_L33_nh2": 0,
  "uniter_attn_varlen_max_len:value": 0
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
def observed_split0():
    return _observe(dict(UNITER_ATTN_SPLIT='0'), 'split0')


def _ids(rows):
    return ['%s:%s' % (f, n) for f, n, _ in rows]


def test_the_table_is_recorded_in_full():
    assert sorted(EXPECTED['refused']) == sorted(_ids(REFUSED)) and sorted(EXPECTED['numbers']) == sorted(_ids(NUMBERS))
    assert sorted(EXPECTED_SPLIT0['refused']) == sorted(_ids(REFUSED_SPLIT0))
    assert sorted(EXPECTED_SPLIT0['numbers']) == sorted(_ids(NUMBERS_SPLIT0))
    assert len(LAUNCHERS) == 16 and len(set(_ids(REFUSED))) == len(REFUSED)
    for exp in (EXPECTED, EXPECTED_SPLIT0):
        assert all(rc in (E_ARG, E_SHAPE) and prefix for rc, prefix in exp['refused'].values())
    assert all(rc == E_SHAPE for rc, _ in EXPECTED_SPLIT0['refused'].values())
    assert all(EXPECTED['refused']['%s:L_193' % fn][0] == E_SHAPE for fn in LAUNCHERS if fn not in ANY_LENGTH)


@pytest.mark.parametrize('row', _ids(REFUSED))
def test_refused_with_the_recorded_code_and_prefix(observed, row):
    assert observed['refused'][row] == EXPECTED['refused'][row]


@pytest.mark.parametrize('row', _ids(NUMBERS))
def test_sizes_are_the_recorded_integers(observed, row):
    assert observed['numbers'][row] == EXPECTED['numbers'][row]


@pytest.mark.parametrize('row', _ids(REFUSED_SPLIT0) + _ids(NUMBERS_SPLIT0))
def test_without_the_split_kernels_the_limited_forms_refuse_every_length(observed_split0, row):
    kind = 'refused' if row in EXPECTED_SPLIT0['refused'] else 'numbers'
    assert observed_split0[kind][row] == EXPECTED_SPLIT0[kind][row]
