"""CPU: the dense-product entry points of the C ABI refuse bad calls before any HIP call, with the return code and the family
prefix recorded from the library before the launcher layer took GemmCall / WgradGroupCall; the slot and plan functions (host
arithmetic) return the integers recorded from that same library.

Every row of REFUSED is a call that must be refused: pointers are fake aligned integers that nothing may dereference.  So that
a regression (a row that is no longer refused) cannot reach a device with them, the table runs in ONE child process that
sees no GPU (HIP_VISIBLE_DEVICES=-1) and loads the library with ctypes alone: `python tests/test_gemm_refusals_cpu.py LIB`
prints the observed values as JSON, and the tests compare them with the literals below."""
import ctypes as C
import json
import os
import subprocess
import sys

P0, P1, P2, P3, P4, P5 = (0x10000 * (i + 1) for i in range(6))      # fake 64-KiB aligned pointers
ODD = 4                                                             # added to a pointer: 4-byte aligned only
BIG = 1 << 24                                                       # rows: x 64 bf16 = 2^31 bytes
H, I3, FF, ROWS = 768, 2304, 3072, 2624                             # UNITER-base layer shape, rows of the flagship batch
WS_BYTES = 16384 + 256 * 128 * 256 * 4                              # uniter_gemm_x3_balanced_ws_bytes() on 256 CUs

# ---- the entry points: (ctypes signature, parameter names with the defaults of one valid 128 x 128 x 64 product) ----
# i = int, p = pointer, l = long, z = size_t
_G32 = dict(cfg=0, akm=0, bkm=0, M=128, N=128, K=64, A=P0, lda=64, B=P1, ldb=64, C=P2, ldc=128, epi=0, bias=None, aux_in=None,
            aux_out=None, ld_aux=128, beta=0, stream=None)
_RES = dict(cfg=0, akm=0, bkm=0, M=128, N=128, K=64, A=P0, lda=64, B=P1, ldb=64, C=P2, ldc=128, Cb=None, ldcb=128, epi=0, bias=None,
            aux_in=None, aux_out=None, ld_aux=128, beta=0, stream=None)
_V2 = dict(cfg=0, nsplit=1, akm=0, bkm=0, M=128, N=128, K=64, A=P0, lda=64, B=P1, ldb=64, C=P2, ldc=128, css=128 * 128, Cb=None,
           ldcb=128, epi=0, bias=None, aux_in=None, aux_in_bf16=0, aux_out=None, aux_out_bf16=0, ld_aux=128, beta=0, stream=None)
_X3 = dict(cfg=0, nsplit=1, akm=0, bkm=0, M=128, N=128, K=32, A=P0, lda=96, psa=32, B=P1, ldb=96, psb=32, C=P2, ldc=128,
           css=128 * 128, Cx=None, ldcx=384, pscx=128, epi=0, bias=None, aux_in=None, aux_out=None, ld_aux=128, stream=None)
_X3CP = dict(cfg=0, akm=0, bkm=1, M=128, N=128, K=32, A=P0, lda=96, psa=32, B=P1, ldb=384, psb=128, C=P2, ldc=128, Cx=None, ldcx=384,
             pscx=128, aux_in=P3, ld_aux=128, colsum_part=P4, stream=None)
_PCP = dict(bkm=1, M=128, N=256, K=64, A=P0, lda=64, B=P1, ldb=256, C=P2, ldc=256, Cb=None, ldcb=256, aux_in=P3, aux_in_bf16=0,
            ld_aux=256, colsum_part=P4, stream=None)
_MO, _NO = [FF, H, I3, H], [H, FF, H, H]                            # a layer's four weight gradients, the grouped launch's order
_GRP = dict(cfg=1, n=4, Mo=_MO, No=_NO, K=ROWS, A=[P0, P1, P2, P3], B=[P1, P2, P3, P4], dW=[P2, P3, P4, P5], overwrite=0, max_wgs=0,
            riders=None, stream=None)
_GRPF = dict(n=4, Mo=_MO, No=_NO, K=ROWS, A=[P0, P1, P2, P3], B=[P1, P2, P3, P4], dW=[P2, P3, P4, P5], overwrite=0, stream=None)
FUNCS = {
    'uniter_gemm_f32_cfg': ('iiiiiipipipiipppiip', _G32),
    'uniter_gemm_bf16_cfg': ('iiiiiipipipiipppiip', _G32),
    'uniter_gemm_bf16res_cfg': ('iiiiiipipipipiipppiip', _RES),
    'uniter_gemm_bf16v2_cfg': ('iiiiiiipipipilpiippipiiip', _V2),
    'uniter_gemm_x3_cfg': ('iiiiiiipiipiipilpiiipppip', _X3),
    'uniter_gemm_x3_cfg_ws': ('iiiiiiipiipiipilpiiipppipzp', dict(list(_X3.items())[:-1] + [('ws', None), ('ws_bytes', 0), ('stream', None)])),
    'uniter_gemm_x3_colpart': ('iiiiiipiipiipipiipipp', _X3CP),
    'uniter_gemm_bf16p_colpart': ('iiiipipipipipiipp', _PCP),
    'uniter_wgrad_f32_group': ('ippipppip', _GRPF),
    'uniter_wgrad_bf16_group_riders': ('iippipppiipp', _GRP),
    'uniter_wgrad_x3_group_riders': ('iippipppiipp', dict(_GRP, cfg=3)),
    'uniter_wgrad_x3_group_ws': ('iippipppiippzp', dict(list(dict(_GRP, cfg=3).items())[:-1] + [('ws', None), ('ws_bytes', 0), ('stream', None)])),
    'uniter_wgrad_bf16_group_slots': ('ippi', dict(n=4, Mo=_MO, No=_NO, max_wgs=0)),
    'uniter_wgrad_bf16_group_slots_cfg': ('iippi', dict(cfg=1, n=4, Mo=_MO, No=_NO, max_wgs=0)),
    'uniter_wgrad_x3_group_slots': ('iippi', dict(cfg=3, n=4, Mo=_MO, No=_NO, max_wgs=0)),
    'uniter_wgrad_x3_group_slots_ws': ('iippiiz', dict(cfg=4, n=4, Mo=_MO, No=_NO, K=ROWS, max_wgs=0, ws_bytes=WS_BYTES)),
    'uniter_gemm_x3_plan': ('iiiiipp', dict(M=ROWS, N=H, K=H, avail=0, nsplit_fixed=0, cfg='out', nsplit='out')),
    'uniter_gemm_x3_plan_fwd32': ('iiiiipp', dict(M=ROWS, N=H, K=H, avail=0, nsplit_fixed=0, cfg='out', nsplit='out')),
}

F32, B16, RES, V2, X3 = ('uniter_gemm_f32_cfg', 'uniter_gemm_bf16_cfg', 'uniter_gemm_bf16res_cfg', 'uniter_gemm_bf16v2_cfg',
                         'uniter_gemm_x3_cfg')
X3CP, PCP = 'uniter_gemm_x3_colpart', 'uniter_gemm_bf16p_colpart'
GF, GB, GX = 'uniter_wgrad_f32_group', 'uniter_wgrad_bf16_group_riders', 'uniter_wgrad_x3_group_riders'
EPI_BIAS, EPI_BIAS_GELU, EPI_ADD, EPI_GELU_D, EPI_MUL = 1, 2, 4, 5, 6


def _forward_rows():
    rows = []
    # the fp32-operand families; gemm_bf16 hands what its kernel does not cover to the fp32 launcher, whose refusal it then is.
    # (no row for k-major A -- every layout is built --, split-K -- there is none -- or 31-bit offsets -- the one-tile kernel takes them)
    for f in (F32, B16):
        rows += [(f, 'null_operand', dict(A=None)), (f, 'bad_epilogue', dict(epi=9)), (f, 'no_bias', dict(epi=EPI_BIAS)),
                 (f, 'no_aux_in', dict(epi=EPI_ADD)), (f, 'misaligned', dict(A=P0 + ODD)), (f, 'ld_off', dict(lda=66)),
                 (f, 'k_off', dict(K=66, lda=68, ldb=68)), (f, 'bad_dims', dict(M=0))]
    rows += [(F32, 'bad_cfg', dict(cfg=7))]
    rows += [(RES, 'null_operand', dict(A=None)), (RES, 'bad_epilogue', dict(epi=9)), (RES, 'no_bias', dict(epi=EPI_BIAS)),
             (RES, 'no_aux_in', dict(epi=EPI_MUL)), (RES, 'a_kmajor', dict(akm=1)), (RES, 'beta_with_copy', dict(beta=1, Cb=P3)),
             (RES, 'misaligned', dict(B=P1 + ODD)), (RES, 'ld_off', dict(lda=68)), (RES, 'k_off', dict(K=72, lda=72, ldb=72)),
             (RES, 'beyond_31_bits', dict(M=BIG)), (RES, 'bad_cfg', dict(cfg=2))]
    rows += [(V2, 'null_operand', dict(B=None)), (V2, 'bad_epilogue', dict(epi=9)), (V2, 'no_bias', dict(epi=EPI_BIAS)),
             (V2, 'no_aux_in', dict(epi=EPI_ADD)), (V2, 'no_aux_out', dict(epi=EPI_BIAS_GELU, bias=P3)),
             (V2, 'no_aux_out_gelu_d', dict(epi=EPI_GELU_D, bias=P3)), (V2, 'a_kmajor', dict(akm=1)),
             (V2, 'split_with_copy', dict(nsplit=2, Cb=P3)), (V2, 'split_with_beta', dict(nsplit=2, beta=1)),
             (V2, 'beta_with_epilogue', dict(beta=1, epi=EPI_BIAS, bias=P3)), (V2, 'misaligned', dict(A=P0 + ODD)),
             (V2, 'misaligned_bias', dict(epi=EPI_BIAS, bias=P3 + ODD)), (V2, 'ld_off', dict(ldb=68)), (V2, 'ld_aux_off', dict(ld_aux=130)),
             (V2, 'k_off', dict(K=72, lda=72, ldb=72)), (V2, 'beyond_31_bits', dict(M=BIG)), (V2, 'bad_cfg', dict(cfg=9, akm=1, bkm=1)),
             (V2, 'wgrad_cfg', dict(cfg=2, akm=1, bkm=1, lda=128, ldb=128))]
    # the persistent kernels behind cfg 6 .. 8 of uniter_gemm_bf16v2_cfg, and behind uniter_gemm_bf16p_colpart
    rows += [(V2, 'p_bad_epilogue', dict(cfg=7, epi=EPI_BIAS_GELU, bias=P3, aux_out=P4)), (V2, 'p_no_bias', dict(cfg=7, epi=EPI_BIAS)),
             (V2, 'p_no_aux_out', dict(cfg=7, epi=EPI_GELU_D, bias=P3)), (V2, 'p_a_kmajor', dict(cfg=7, akm=1, bkm=1, lda=128, ldb=128)),
             (V2, 'p_beta', dict(cfg=6, beta=1)), (V2, 'p_split_with_copy', dict(cfg=6, nsplit=2, Cb=P3)),
             (V2, 'p_epilogue_kmajor_weights', dict(cfg=7, bkm=1, ldb=128, epi=EPI_BIAS, bias=P3)),
             (V2, 'p_epilogue_kcontiguous_weights', dict(cfg=7, epi=EPI_ADD, aux_in=P3)), (V2, 'p_cfg8_kmajor', dict(cfg=8, bkm=1, ldb=128)),
             (PCP, 'null_operand', dict(A=None)), (PCP, 'no_aux_in', dict(aux_in=None)), (PCP, 'no_colpart', dict(colsum_part=None)),
             (PCP, 'colpart_misaligned', dict(colsum_part=P4 + ODD)), (PCP, 'misaligned', dict(B=P1 + ODD)), (PCP, 'ld_off', dict(lda=68)),
             (PCP, 'k_off', dict(K=72, lda=72)), (PCP, 'beyond_31_bits', dict(M=BIG))]
    rows += [(X3, 'null_operand', dict(A=None)), (X3, 'bad_epilogue', dict(epi=9)), (X3, 'epilogue_not_built', dict(epi=EPI_BIAS_GELU, bias=P3)),
             (X3, 'no_bias', dict(epi=EPI_BIAS)), (X3, 'no_aux_in', dict(epi=EPI_ADD, bkm=1, ldb=384, psb=128)),
             (X3, 'no_aux_out', dict(epi=EPI_GELU_D, bias=P3)), (X3, 'a_kmajor', dict(akm=1)),
             (X3, 'a_kmajor_epilogue', dict(akm=1, bkm=1, lda=384, psa=128, ldb=384, psb=128, epi=EPI_MUL, aux_in=P3)),
             (X3, 'split_with_copy', dict(nsplit=2, Cx=P3)), (X3, 'split_stride_short', dict(nsplit=2, css=64)),
             (X3, 'misaligned', dict(A=P0 + ODD)), (X3, 'ld_off', dict(lda=100)), (X3, 'piece_stride_off', dict(psa=36)),
             (X3, 'k_off', dict(K=48, lda=144, psa=48, ldb=144, psb=48)), (X3, 'beyond_31_bits', dict(M=BIG)),
             (X3, 'cfg5_not_forward', dict(cfg=5, bkm=1, ldb=384, psb=128)), (X3, 'cfg5_with_copy', dict(cfg=5, Cx=P3)),
             (X3, 'paired_rows_on_a', dict(cfg=3 | 64, akm=1, bkm=1, lda=384, psa=128, ldb=384, psb=128)),
             (X3, 'paired_rows_row_length', dict(cfg=3 | 64, K=48, lda=144, psa=48, ldb=144, psb=48)), (X3, 'bad_cfg', dict(cfg=9)),
             (X3, 'cfg4_wgrad', dict(cfg=4, akm=1, bkm=1, lda=384, psa=128, ldb=384, psb=128)),
             ('uniter_gemm_x3_cfg_ws', 'ws_null_operand', dict(B=None, ws=P5, ws_bytes=WS_BYTES)),
             (X3CP, 'colpart_wrong_geometry', dict(cfg=1)), (X3CP, 'colpart_misaligned', dict(colsum_part=P4 + ODD)),
             (X3CP, 'no_aux_in', dict(aux_in=None)), (X3CP, 'null_operand', dict(A=None))]
    return rows


def _group_rows():
    rows = []
    bad_a, odd_a = [P0, None, P2, P3], [P0 + ODD, P1, P2, P3]
    for f, kw in ((GF, {}), (GB, dict(cfg=1)), (GB, dict(cfg=7)), (GX, dict(cfg=3)), (GX, dict(cfg=4))):
        tag = 'cfg%d_' % kw['cfg'] if kw else ''
        rows += [(f, tag + 'n0', dict(kw, n=0)), (f, tag + 'n5', dict(kw, n=5)), (f, tag + 'null_product', dict(kw, A=bad_a)),
                 (f, tag + 'misaligned_product', dict(kw, A=odd_a)), (f, tag + 'null_shapes', dict(kw, Mo=None)),
                 (f, tag + 'empty_product', dict(kw, Mo=[FF, 0, I3, H]))]
    rows += [(GB, 'riders_on_three_stages', dict(cfg=4, riders={})), (GX, 'riders_on_cfg1', dict(cfg=1, riders={})),
             (GB, 'colsum_out_on_128x256', dict(cfg=7, riders=dict(colsum_out=P5))),
             (GX, 'colsum_out_on_128x256', dict(cfg=4, riders=dict(colsum_out=P5))),
             (GX, 'bad_reduction_job', dict(cfg=3, riders=dict(njobs=5))), (GB, 'bad_reduction_job', dict(cfg=1, riders=dict(njobs=5))),
             ('uniter_wgrad_x3_group_ws', 'ws_n0', dict(n=0, ws=P5, ws_bytes=WS_BYTES)), (GX, 'bad_cfg', dict(cfg=9))]
    return rows


REFUSED = _forward_rows() + _group_rows()

# ---- host arithmetic: slots of the grouped launches with riders, plans of the forward products ----
_TINY = dict(n=1, Mo=[64], No=[64])
NUMBERS = (
    [('uniter_wgrad_bf16_group_slots', 'layer_wgs%d' % w, dict(max_wgs=w)) for w in (0, 64, 200)]
    + [('uniter_wgrad_bf16_group_slots', 'tiny', _TINY), ('uniter_wgrad_bf16_group_slots', 'n5', dict(n=5)),
       ('uniter_wgrad_bf16_group_slots', 'null', dict(Mo=None))]
    + [('uniter_wgrad_bf16_group_slots_cfg', 'layer_cfg%d_wgs%d' % (c, w), dict(cfg=c, max_wgs=w)) for c in (1, 7) for w in (0, 64)]
    + [('uniter_wgrad_bf16_group_slots_cfg', 'tiny_cfg7', dict(_TINY, cfg=7))]
    + [('uniter_wgrad_x3_group_slots', 'layer_cfg%d_wgs%d' % (c, w), dict(cfg=c, max_wgs=w)) for c in (3, 4) for w in (0, 64, 200)]
    + [('uniter_wgrad_x3_group_slots', 'tiny_cfg%d' % c, dict(_TINY, cfg=c)) for c in (3, 4)]
    + [('uniter_wgrad_x3_group_slots', 'n0', dict(n=0))]
    + [('uniter_wgrad_x3_group_slots_ws', 'layer_cfg%d_wgs%d' % (c, w), dict(cfg=c, max_wgs=w)) for c in (3, 4) for w in (0, 64)]
    + [('uniter_wgrad_x3_group_slots_ws', 'layer_small_ws', dict(ws_bytes=4096)), ('uniter_wgrad_x3_group_slots_ws', 'tiny', dict(_TINY, K=64))]
    + [(f, 'n%d_k%d_cus%d_ns%d' % (n, k, a, ns), dict(N=n, K=k, avail=a, nsplit_fixed=ns))
       for f in ('uniter_gemm_x3_plan', 'uniter_gemm_x3_plan_fwd32')
       for n, k in ((H, H), (H, FF), (I3, H), (FF, H), (H, I3)) for a, ns in ((0, 0), (240, 0), (0, 1))]
    + [(f, 'tiny', dict(M=64, N=64, K=64)) for f in ('uniter_gemm_x3_plan', 'uniter_gemm_x3_plan_fwd32')]
)


class _Riders(C.Structure):      # uniter_x3_riders_t (include/uniter_hip.h)
    _fields_ = [('ssq', C.c_void_p), ('colsum_out', C.c_void_p), ('grid', C.c_int), ('njobs', C.c_int), ('nred', C.c_int),
                ('part', C.c_void_p * 4), ('nparts', C.c_int * 4), ('stride', C.c_int * 4), ('n', C.c_int * 4), ('seg', C.c_int * 4),
                ('out', (C.c_void_p * 3) * 4), ('first_item', C.c_int * 5)]


_CT = {'i': C.c_int, 'p': C.c_void_p, 'l': C.c_long, 'z': C.c_size_t}


def _call(lib, fn, overrides):
    sig, defaults = FUNCS[fn]
    unknown = set(overrides) - set(defaults)
    assert not unknown and len(sig) == len(defaults), (fn, unknown)
    f = getattr(lib, fn)
    f.restype, f.argtypes = C.c_int, [_CT[ch] for ch in sig]
    keep, outs, args = [], [], []
    for name, v in dict(defaults, **overrides).items():
        if isinstance(v, list):
            v = ((C.c_int if name in ('Mo', 'No') else C.c_void_p) * len(v))(*v)
        elif isinstance(v, dict):
            v = _Riders(**v)
        elif v == 'out':
            v = C.c_int(-1)
            outs.append(v)
        if isinstance(v, (C.Array, C.Structure, C.c_int)):
            keep.append(v)
            v = C.cast(C.pointer(v), C.c_void_p)
        args.append(v)
    rc = f(*args)
    return rc, [o.value for o in outs]


def observe(lib_path):
    """{'refused': {id: [rc, message prefix]}, 'numbers': {id: [rc, outputs...]}} of the library at lib_path"""
    lib = C.CDLL(lib_path)
    lib.uniter_last_error.restype = C.c_char_p
    out = {'refused': {}, 'numbers': {}}
    for fn, name, kw in REFUSED:
        rc, _ = _call(lib, fn, kw)
        out['refused']['%s:%s' % (fn, name)] = [rc, lib.uniter_last_error().decode().split(':')[0] if rc else '']
    for fn, name, kw in NUMBERS:
        rc, outs = _call(lib, fn, kw)
        out['numbers']['%s:%s' % (fn, name)] = [rc] + outs
    return out


if __name__ == '__main__':
    print(json.dumps(observe(sys.argv[1])))
    sys.exit(0)

import pytest      # noqa: E402  (the child process above needs neither pytest nor the package)

E_ARG, E_SHAPE = -1, -2
EXPECTED = json.loads(r'''
{"refused": {
  "uniter_gemm_f32_cfg:null_operand": [-1, "gemm"],
  "uniter_gemm_f32_cfg:bad_epilogue": [-1, "gemm"],
  "uniter_gemm_f32_cfg:no_bias": [-1, "gemm"],
  "uniter_gemm_f32_cfg:no_aux_in": [-1, "gemm"],
  "uniter_gemm_f32_cfg:misaligned": [-1, "gemm"],
  "uniter_gemm_f32_cfg:ld_off": [-2, "gemm"],
  "uniter_gemm_f32_cfg:k_off": [-2, "gemm"],
  "uniter_gemm_f32_cfg:bad_dims": [-1, "gemm"],
  "uniter_gemm_bf16_cfg:null_operand": [-1, "gemm_bf16"],
  "uniter_gemm_bf16_cfg:bad_epilogue": [-1, "gemm_bf16"],
  "uniter_gemm_bf16_cfg:no_bias": [-1, "gemm_bf16"],
  "uniter_gemm_bf16_cfg:no_aux_in": [-1, "gemm_bf16"],
  "uniter_gemm_bf16_cfg:misaligned": [-1, "gemm"],
  "uniter_gemm_bf16_cfg:ld_off": [-2, "gemm"],
  "uniter_gemm_bf16_cfg:k_off": [-2, "gemm"],
  "uniter_gemm_bf16_cfg:bad_dims": [-1, "gemm_bf16"],
  "uniter_gemm_f32_cfg:bad_cfg": [-1, "gemm"],
  "uniter_gemm_bf16res_cfg:null_operand": [-1, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:bad_epilogue": [-1, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:no_bias": [-1, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:no_aux_in": [-1, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:a_kmajor": [-1, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:beta_with_copy": [-1, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:misaligned": [-2, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:ld_off": [-2, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:k_off": [-2, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:beyond_31_bits": [-2, "gemm_bf16res"],
  "uniter_gemm_bf16res_cfg:bad_cfg": [-1, "gemm_bf16res"],
  "uniter_gemm_bf16v2_cfg:null_operand": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:bad_epilogue": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:no_bias": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:no_aux_in": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:no_aux_out": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:no_aux_out_gelu_d": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:a_kmajor": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:split_with_copy": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:split_with_beta": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:beta_with_epilogue": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:misaligned": [-2, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:misaligned_bias": [-2, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:ld_off": [-2, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:ld_aux_off": [-2, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:k_off": [-2, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:beyond_31_bits": [-2, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:bad_cfg": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:wgrad_cfg": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:p_bad_epilogue": [-1, "gemm_bf16p"],
  "uniter_gemm_bf16v2_cfg:p_no_bias": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:p_no_aux_out": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:p_a_kmajor": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:p_beta": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:p_split_with_copy": [-1, "gemm_bf16v2"],
  "uniter_gemm_bf16v2_cfg:p_epilogue_kmajor_weights": [-1, "gemm_bf16p"],
  "uniter_gemm_bf16v2_cfg:p_epilogue_kcontiguous_weights": [-1, "gemm_bf16p"],
  "uniter_gemm_bf16v2_cfg:p_cfg8_kmajor": [-1, "gemm_bf16p"],
  "uniter_gemm_bf16p_colpart:null_operand": [-1, "gemm_bf16p"],
  "uniter_gemm_bf16p_colpart:no_aux_in": [-1, "gemm_bf16p"],
  "uniter_gemm_bf16p_colpart:no_colpart": [-1, "gemm_bf16p_colpart"],
  "uniter_gemm_bf16p_colpart:colpart_misaligned": [-1, "gemm_bf16p"],
  "uniter_gemm_bf16p_colpart:misaligned": [-2, "gemm_bf16p"],
  "uniter_gemm_bf16p_colpart:ld_off": [-2, "gemm_bf16p"],
  "uniter_gemm_bf16p_colpart:k_off": [-2, "gemm_bf16p"],
  "uniter_gemm_bf16p_colpart:beyond_31_bits": [-2, "gemm_bf16p"],
  "uniter_gemm_x3_cfg:null_operand": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:bad_epilogue": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:epilogue_not_built": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:no_bias": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:no_aux_in": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:no_aux_out": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:a_kmajor": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:a_kmajor_epilogue": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:split_with_copy": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:split_stride_short": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:misaligned": [-2, "gemm_x3"],
  "uniter_gemm_x3_cfg:ld_off": [-2, "gemm_x3"],
  "uniter_gemm_x3_cfg:piece_stride_off": [-2, "gemm_x3"],
  "uniter_gemm_x3_cfg:k_off": [-2, "gemm_x3"],
  "uniter_gemm_x3_cfg:beyond_31_bits": [-2, "gemm_x3"],
  "uniter_gemm_x3_cfg:cfg5_not_forward": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:cfg5_with_copy": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:paired_rows_on_a": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:paired_rows_row_length": [-2, "gemm_x3"],
  "uniter_gemm_x3_cfg:bad_cfg": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg:cfg4_wgrad": [-1, "gemm_x3"],
  "uniter_gemm_x3_cfg_ws:ws_null_operand": [-1, "gemm_x3"],
  "uniter_gemm_x3_colpart:colpart_wrong_geometry": [-1, "gemm_x3"],
  "uniter_gemm_x3_colpart:colpart_misaligned": [-1, "gemm_x3"],
  "uniter_gemm_x3_colpart:no_aux_in": [-1, "gemm_x3"],
  "uniter_gemm_x3_colpart:null_operand": [-1, "gemm_x3"],
  "uniter_wgrad_f32_group:n0": [-1, "wgrad_group_f32"],
  "uniter_wgrad_f32_group:n5": [-1, "wgrad_group_f32"],
  "uniter_wgrad_f32_group:null_product": [-1, "wgrad_group_f32"],
  "uniter_wgrad_f32_group:misaligned_product": [-2, "wgrad_group_f32"],
  "uniter_wgrad_f32_group:null_shapes": [-1, "wgrad_group_f32"],
  "uniter_wgrad_f32_group:empty_product": [-1, "wgrad_group_f32"],
  "uniter_wgrad_bf16_group_riders:cfg1_n0": [-1, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg1_n5": [-1, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg1_null_product": [-1, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg1_misaligned_product": [-2, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg1_null_shapes": [-1, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg1_empty_product": [-1, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg7_n0": [-1, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg7_n5": [-1, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg7_null_product": [-1, "wgrad_bf16p_group"],
  "uniter_wgrad_bf16_group_riders:cfg7_misaligned_product": [-2, "wgrad_bf16p_group"],
  "uniter_wgrad_bf16_group_riders:cfg7_null_shapes": [-1, "wgrad_group"],
  "uniter_wgrad_bf16_group_riders:cfg7_empty_product": [-1, "wgrad_bf16p_group"],
  "uniter_wgrad_x3_group_riders:cfg3_n0": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg3_n5": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg3_null_product": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg3_misaligned_product": [-2, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg3_null_shapes": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg3_empty_product": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg4_n0": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg4_n5": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg4_null_product": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg4_misaligned_product": [-2, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg4_null_shapes": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:cfg4_empty_product": [-1, "wgrad_x3_group"],
  "uniter_wgrad_bf16_group_riders:riders_on_three_stages": [-1, "wgrad_group"],
  "uniter_wgrad_x3_group_riders:riders_on_cfg1": [-1, "wgrad_x3_group"],
  "uniter_wgrad_bf16_group_riders:colsum_out_on_128x256": [-1, "wgrad_bf16p_group"],
  "uniter_wgrad_x3_group_riders:colsum_out_on_128x256": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:bad_reduction_job": [-1, "wgrad_x3_group"],
  "uniter_wgrad_bf16_group_riders:bad_reduction_job": [-1, "wgrad_bf16_group"],
  "uniter_wgrad_x3_group_ws:ws_n0": [-1, "wgrad_x3_group"],
  "uniter_wgrad_x3_group_riders:bad_cfg": [-1, "gemm_x3"]
},
"numbers": {
  "uniter_wgrad_bf16_group_slots:layer_wgs0": [1024],
  "uniter_wgrad_bf16_group_slots:layer_wgs64": [256],
  "uniter_wgrad_bf16_group_slots:layer_wgs200": [800],
  "uniter_wgrad_bf16_group_slots:tiny": [32],
  "uniter_wgrad_bf16_group_slots:n5": [0],
  "uniter_wgrad_bf16_group_slots:null": [0],
  "uniter_wgrad_bf16_group_slots_cfg:layer_cfg1_wgs0": [1024],
  "uniter_wgrad_bf16_group_slots_cfg:layer_cfg1_wgs64": [256],
  "uniter_wgrad_bf16_group_slots_cfg:layer_cfg7_wgs0": [1728],
  "uniter_wgrad_bf16_group_slots_cfg:layer_cfg7_wgs64": [512],
  "uniter_wgrad_bf16_group_slots_cfg:tiny_cfg7": [64],
  "uniter_wgrad_x3_group_slots:layer_cfg3_wgs0": [1024],
  "uniter_wgrad_x3_group_slots:layer_cfg3_wgs64": [256],
  "uniter_wgrad_x3_group_slots:layer_cfg3_wgs200": [800],
  "uniter_wgrad_x3_group_slots:layer_cfg4_wgs0": [1728],
  "uniter_wgrad_x3_group_slots:layer_cfg4_wgs64": [512],
  "uniter_wgrad_x3_group_slots:layer_cfg4_wgs200": [1600],
  "uniter_wgrad_x3_group_slots:tiny_cfg3": [32],
  "uniter_wgrad_x3_group_slots:tiny_cfg4": [64],
  "uniter_wgrad_x3_group_slots:n0": [0],
  "uniter_wgrad_x3_group_slots_ws:layer_cfg3_wgs0": [1024],
  "uniter_wgrad_x3_group_slots_ws:layer_cfg3_wgs64": [256],
  "uniter_wgrad_x3_group_slots_ws:layer_cfg4_wgs0": [2048],
  "uniter_wgrad_x3_group_slots_ws:layer_cfg4_wgs64": [512],
  "uniter_wgrad_x3_group_slots_ws:layer_small_ws": [1728],
  "uniter_wgrad_x3_group_slots_ws:tiny": [64],
  "uniter_gemm_x3_plan:n768_k768_cus0_ns0": [0, 3, 2],
  "uniter_gemm_x3_plan:n768_k768_cus240_ns0": [0, 4, 3],
  "uniter_gemm_x3_plan:n768_k768_cus0_ns1": [0, 3, 1],
  "uniter_gemm_x3_plan:n768_k3072_cus0_ns0": [0, 3, 2],
  "uniter_gemm_x3_plan:n768_k3072_cus240_ns0": [0, 4, 3],
  "uniter_gemm_x3_plan:n768_k3072_cus0_ns1": [0, 3, 1],
  "uniter_gemm_x3_plan:n2304_k768_cus0_ns0": [0, 4, 1],
  "uniter_gemm_x3_plan:n2304_k768_cus240_ns0": [0, 4, 1],
  "uniter_gemm_x3_plan:n2304_k768_cus0_ns1": [0, 4, 1],
  "uniter_gemm_x3_plan:n3072_k768_cus0_ns0": [0, 4, 1],
  "uniter_gemm_x3_plan:n3072_k768_cus240_ns0": [0, 3, 1],
  "uniter_gemm_x3_plan:n3072_k768_cus0_ns1": [0, 4, 1],
  "uniter_gemm_x3_plan:n768_k2304_cus0_ns0": [0, 3, 2],
  "uniter_gemm_x3_plan:n768_k2304_cus240_ns0": [0, 4, 3],
  "uniter_gemm_x3_plan:n768_k2304_cus0_ns1": [0, 3, 1],
  "uniter_gemm_x3_plan_fwd32:n768_k768_cus0_ns0": [0, 3, 2],
  "uniter_gemm_x3_plan_fwd32:n768_k768_cus240_ns0": [0, 4, 3],
  "uniter_gemm_x3_plan_fwd32:n768_k768_cus0_ns1": [0, 3, 1],
  "uniter_gemm_x3_plan_fwd32:n768_k3072_cus0_ns0": [0, 3, 2],
  "uniter_gemm_x3_plan_fwd32:n768_k3072_cus240_ns0": [0, 4, 3],
  "uniter_gemm_x3_plan_fwd32:n768_k3072_cus0_ns1": [0, 3, 1],
  "uniter_gemm_x3_plan_fwd32:n2304_k768_cus0_ns0": [0, 5, 1],
  "uniter_gemm_x3_plan_fwd32:n2304_k768_cus240_ns0": [0, 4, 1],
  "uniter_gemm_x3_plan_fwd32:n2304_k768_cus0_ns1": [0, 5, 1],
  "uniter_gemm_x3_plan_fwd32:n3072_k768_cus0_ns0": [0, 4, 1],
  "uniter_gemm_x3_plan_fwd32:n3072_k768_cus240_ns0": [0, 5, 1],
  "uniter_gemm_x3_plan_fwd32:n3072_k768_cus0_ns1": [0, 4, 1],
  "uniter_gemm_x3_plan_fwd32:n768_k2304_cus0_ns0": [0, 3, 2],
  "uniter_gemm_x3_plan_fwd32:n768_k2304_cus240_ns0": [0, 4, 3],
  "uniter_gemm_x3_plan_fwd32:n768_k2304_cus0_ns1": [0, 3, 1],
  "uniter_gemm_x3_plan:tiny": [0, 3, 1],
  "uniter_gemm_x3_plan_fwd32:tiny": [0, 3, 1]
}}
''')


@pytest.fixture(scope='module')
def observed():
    from meme_challenge_amd import _lib
    # no GPU, and the switches' defaults (the slot counts and plans below depend on them)
    env = dict({k: v for k, v in os.environ.items() if not k.startswith('UNITER_')}, HIP_VISIBLE_DEVICES='-1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _lib.LIB_PATH], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_table_is_recorded_in_full():
    assert sorted(EXPECTED['refused']) == sorted('%s:%s' % (f, n) for f, n, _ in REFUSED)
    assert sorted(EXPECTED['numbers']) == sorted('%s:%s' % (f, n) for f, n, _ in NUMBERS)
    assert all(rc in (E_ARG, E_SHAPE) and prefix for rc, prefix in EXPECTED['refused'].values())


@pytest.mark.parametrize('row', ['%s:%s' % (f, n) for f, n, _ in REFUSED])
def test_refused_with_the_recorded_code_and_family_prefix(observed, row):
    assert observed['refused'][row] == EXPECTED['refused'][row]


@pytest.mark.parametrize('row', ['%s:%s' % (f, n) for f, n, _ in NUMBERS])
def test_slots_and_plans_are_the_recorded_integers(observed, row):
    assert observed['numbers'][row] == EXPECTED['numbers'][row]
