"""CPU: uniter_bce_auc_logits refuses every bad call its contract lists (include/uniter_hip.h) before any HIP call: UNITER_E_ARG and a
message of its own in uniter_last_error.

Pointers are fake aligned integers that nothing may dereference.  So that a regression (a row that is no longer refused) cannot
reach a device with them, the table runs in ONE child process that sees no GPU (HIP_VISIBLE_DEVICES=-1) and loads the library with
ctypes alone, the manner of tests/test_adv_refusals_cpu.py: `python tests/test_auc_refusals_cpu.py LIB` prints what it observed as
JSON."""
import ctypes as C
import json
import os
import subprocess
import sys

P = [0x10000 * (i + 1) for i in range(9)]        # fake 64-KiB aligned pointers
NAN = float('nan')
FN = 'uniter_bce_auc_logits'
SIG = 'ppffifpppiippppfip'                       # i = int, p = pointer, f = float
VALID = dict(logits=P[0], labels=P[1], pos_weight=1.8, auc_weight=0.5, kind=0, margin=1.0, bank_scores=P[2], bank_labels=P[3],
             bank_state=P[4], N=1024, push=1, terms=P[5], n_pairs=P[6], probs=P[7], dlogits=P[8], grad_scale=1.0, B=16, stream=None)
REFUSED = [
    ('null_logits', dict(logits=None)), ('null_labels', dict(labels=None)),
    ('B_0', dict(B=0)), ('B_minus_1', dict(B=-1)), ('B_4097', dict(B=4097, N=8192)),
    ('B_0_no_bank', dict(B=0, bank_scores=None)), ('B_4097_no_bank', dict(B=4097, N=0)),
    ('N_below_B', dict(N=15)), ('N_minus_1', dict(N=-1)), ('N_8193', dict(N=8193)),
    ('null_bank_labels', dict(bank_labels=None)), ('null_bank_state', dict(bank_state=None)),
    ('auc_weight_negative', dict(auc_weight=-0.5)), ('auc_weight_nan', dict(auc_weight=NAN)),
    ('auc_weight_nan_no_bank', dict(auc_weight=NAN, bank_scores=None, bank_labels=None, bank_state=None)),
    ('kind_minus_1', dict(kind=-1)), ('kind_2', dict(kind=2)), ('margin_nan', dict(margin=NAN)),
    ('margin_nan_logistic_no_bank', dict(margin=NAN, N=0)),
]
_CT = {'i': C.c_int, 'p': C.c_void_p, 'f': C.c_float}
E_ARG = -1


def observe(lib_path):
    """{row: [rc, message]} of the library at lib_path"""
    lib = C.CDLL(lib_path)
    lib.uniter_last_error.restype = C.c_char_p
    f = getattr(lib, FN)
    f.restype, f.argtypes = C.c_int, [_CT[ch] for ch in SIG]
    assert len(SIG) == len(VALID)
    out = {}
    for name, kw in REFUSED:
        assert not set(kw) - set(VALID), name
        rc = f(*dict(VALID, **kw).values())
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


def test_the_binding_declares_the_signature_the_table_uses():
    from meme_challenge_amd import _lib
    res, args = _lib._SIGS[FN]
    assert res is C.c_int and [{C.c_int: 'i', C.c_void_p: 'p', C.c_float: 'f'}[a] for a in args] == list(SIG)
    assert FN in _lib.EXPORTED_SYMBOLS and len({n for n, _ in REFUSED}) == len(REFUSED)


@pytest.mark.parametrize('row', [n for n, _ in REFUSED])
def test_refused_with_the_argument_error_and_a_message(observed, row):
    rc, message = observed[row]
    assert rc == E_ARG, (row, rc, message)
    assert message.startswith('bce_auc_logits: '), (row, message)
