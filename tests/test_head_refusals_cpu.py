"""CPU: the six pooler / classifier entry points of csrc/head.hip refuse every bad call their contract lists (include/uniter_hip.h)
before any HIP call: UNITER_E_ARG and a message that starts with the entry point's own prefix in uniter_last_error.

Per entry point: each required pointer NULL, each of B, L, H, Cn at 0 and at -1, Cn > H for the two backward launches that require
Cn <= H, and for the two one-launch forms H = 4097 (both honour the stated limit of 4096) and a pooled tensor of B * H * 4 bytes at
or beyond the buffer descriptor's out-of-range offset 0x7ffffff0 (B = 131072, H = 4096: 2^31 bytes; B = 134217727, H = 4: exactly
the offset).  Optional pointers (dhidden; dx, dW, db) are NOT refused when NULL: tests/test_head_f64_gpu.py runs those calls.

Pointers are fake aligned integers that nothing may dereference.  So that a regression (a row that is no longer refused) cannot
reach a device with them, the table runs in ONE child process that sees no GPU (HIP_VISIBLE_DEVICES=-1) and loads the library with
ctypes alone, the manner of tests/test_auc_refusals_cpu.py: `python tests/test_head_refusals_cpu.py LIB` prints what it observed as
JSON."""
import ctypes as C
import json
import os
import subprocess
import sys

P = [0x10000 * (i + 1) for i in range(10)]        # fake 64-KiB aligned pointers
DIMS = dict(B=16, L=3, H=768, Cn=2)
# entry point -> (message prefix, signature (i = int, p = pointer), argument names; a name in brackets is an optional pointer)
TABLE = {
    'uniter_pooler_fwd': ('pooler_fwd: ', 'ppppiiip', 'hidden Wp bp pooled B L H stream'),
    'uniter_pooler_bwd': ('pooler_bwd: ', 'pppppppiiiip', 'dpooled pooled hidden Wp dWp dbp [dhidden] B L H beta stream'),
    'uniter_linear_small_fwd': ('linear_small_fwd: ', 'ppppiiip', 'x W b y B H Cn stream'),
    'uniter_linear_small_bwd': ('linear_small_bwd: ', 'ppppppiiip', 'dy x W [dx] [dW] [db] B H Cn stream'),
    'uniter_pool_head_fwd': ('pool_head_fwd: ', 'ppppppppiiiip', 'hidden Wp bp Wl bl pooled logits ticket B L H Cn stream'),
    'uniter_pool_head_bwd': ('pool_head_bwd: ', 'ppppppppppiiiiip','dlogits pooled hidden Wp Wl dWp dbp dWl dbl [dhidden] B L H Cn beta stream'),
}
CN_LE_H = ('uniter_linear_small_bwd', 'uniter_pool_head_bwd')
FUSED = ('uniter_pool_head_fwd', 'uniter_pool_head_bwd')
_CT = {'i': C.c_int, 'p': C.c_void_p}
E_ARG = -1


def valid(fn):
    """the argument dict of a call that passes every check"""
    names = TABLE[fn][2].split()
    out, k = {}, 0
    for nm, ch in zip(names, TABLE[fn][1]):
        nm = nm.strip('[]')
        if nm == 'stream':
            out[nm] = None
        elif ch == 'p':
            out[nm], k = P[k], k + 1
        else:
            out[nm] = DIMS.get(nm, 0)
    return out


def rows():
    """[(row name, entry point, overrides)]"""
    out = []
    for fn, (_, sig, names) in TABLE.items():
        names = names.split()
        assert len(names) == len(sig), fn
        for nm, ch in zip(names, sig):
            if ch == 'p' and nm != 'stream' and not nm.startswith('['):
                out.append(('%s:null_%s' % (fn, nm), fn, {nm: None}))
            if nm in DIMS:
                out.append(('%s:%s_0' % (fn, nm), fn, {nm: 0}))
                out.append(('%s:%s_minus_1' % (fn, nm), fn, {nm: -1}))
        if fn in CN_LE_H:
            out.append(('%s:Cn_above_H' % fn, fn, dict(H=4, Cn=5)))
        if fn in FUSED:
            out.append(('%s:H_4097' % fn, fn, dict(H=4097)))
            out.append(('%s:B_131072_H_4096' % fn, fn, dict(B=131072, H=4096)))
            out.append(('%s:B_H_4_at_the_offset' % fn, fn, dict(B=134217727, H=4)))
    return out


def observe(lib_path):
    """{row: [rc, message]} of the library at lib_path"""
    lib = C.CDLL(lib_path)
    lib.uniter_last_error.restype = C.c_char_p
    out = {}
    for name, fn, kw in rows():
        f = getattr(lib, fn)
        f.restype, f.argtypes = C.c_int, [_CT[ch] for ch in TABLE[fn][1]]
        args = valid(fn)
        assert not set(kw) - set(args), name
        rc = f(*dict(args, **kw).values())
        out[name] = [rc, lib.uniter_last_error().decode() if rc else '']
    return out


if __name__ == '__main__':
    print(json.dumps(observe(sys.argv[1])))
    sys.exit(0)

import pytest      # noqa: E402  (the child process above needs neither pytest nor the package)


@pytest.fixture(scope='module')
def observed():
    from meme_challenge_amd import _lib
    env = dict({k: v for k, v in os.environ.items() if not k.startswith('UNITER_')}, HIP_VISIBLE_DEVICES='-1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _lib.LIB_PATH], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize('fn', list(TABLE))
def test_the_binding_declares_the_signature_the_table_uses(fn):
    from meme_challenge_amd import _lib
    res, args = _lib._SIGS[fn]
    assert res is C.c_int and [{C.c_int: 'i', C.c_void_p: 'p'}[a] for a in args] == list(TABLE[fn][1])
    assert fn in _lib.EXPORTED_SYMBOLS


def test_the_table_holds_the_rows_it_promises():
    names = [n for n, _, _ in rows()]
    assert len(set(names)) == len(names)
    for fn, (_, sig, argn) in TABLE.items():
        required = [a for a, ch in zip(argn.split(), sig) if ch == 'p' and a != 'stream' and not a.startswith('[')]
        dims = [a for a in argn.split() if a in DIMS]
        mine = [n for n in names if n.startswith(fn + ':')]
        assert len(mine) == len(required) + 2 * len(dims) + (fn in CN_LE_H) + 3 * (fn in FUSED), fn
        assert len(dims) == (4 if fn in FUSED else 3)
    # the valid call of each entry point passes the checks the rows override: 0 < Cn <= H <= 4096, B * H * 4 below the offset
    assert 0 < DIMS['Cn'] <= DIMS['H'] <= 4096 and DIMS['B'] * DIMS['H'] * 4 < 0x7ffffff0
    assert 131072 * 4096 * 4 == 2 ** 31 and 134217727 * 4 * 4 == 0x7ffffff0


@pytest.mark.parametrize('row', [n for n, _, _ in rows()])
def test_refused_with_the_argument_error_and_its_own_prefix(observed, row):
    rc, message = observed[row]
    assert rc == E_ARG, (row, rc, message)
    assert message.startswith(TABLE[row.split(':')[0]][0]), (row, message)
