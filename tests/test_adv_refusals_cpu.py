"""CPU: the adversarial step's entry points of the C ABI -- the two logits losses (uniter_bce_logits, uniter_bce_kl_logits) and the
perturbation's ascent step in both norms (uniter_adv_delta_step, uniter_adv_delta_step_linf) -- refuse bad calls before any HIP
call, with the return code and the message recorded from the library before the two losses became one kernel template and the two
steps one launcher; the two workspace size functions (host arithmetic) return the integers recorded from that same library.

Pointers are fake aligned integers that nothing may dereference.  So that a regression (a row that is no longer refused) cannot
reach a device with them, the table runs in ONE child process that sees no GPU (HIP_VISIBLE_DEVICES=-1) and loads the library
with ctypes alone: `python tests/test_adv_refusals_cpu.py LIB` prints the observed values as JSON, and the tests compare them
with the literals below.  ACCEPTED holds the calls the steps take without a launch (no samples, or no elements): they return 0."""
import ctypes as C
import json
import os
import subprocess
import sys

P0, P1, P2, P3, P4, P5, WS = (0x10000 * (i + 1) for i in range(7))      # fake 64-KiB aligned pointers
ODD = 4                                                                  # added to a pointer: 4-byte aligned only
NAN = float('nan')

# ---- the entry points: (ctypes signature, parameter names with the defaults of one valid call); i = int, p = pointer, f = float ----
_STEP = dict(delta=P0, grad=P1, B=3, n=4100, step_size=0.1, max_norm=1.0, ws=WS, stream=None)
FUNCS = {
    'uniter_bce_logits': ('ppfpppfip', dict(logits=P0, labels=P1, pos_weight=1.8, loss=P2, probs=P3, dlogits=P4, grad_scale=1.0, B=16,
                                            stream=None)),
    'uniter_bce_kl_logits': ('pppffpppfip', dict(logits=P0, clean=P5, labels=P1, pos_weight=1.8, kl_weight=0.3, terms=P2, probs=P3,
                                                 dlogits=P4, grad_scale=0.5, B=16, stream=None)),
    'uniter_adv_delta_step': ('ppiiffpp', _STEP),
    'uniter_adv_delta_step_linf': ('ppiiffpp', _STEP),
}
BCE, KL, L2, LINF = FUNCS
_LOSS_ROWS = [('B_0', dict(B=0)), ('B_minus_1', dict(B=-1))]
_STEP_ROWS = ([('null_' + k, {k: None}) for k in ('delta', 'grad', 'ws')] +
              [('misaligned_delta', dict(delta=P0 + ODD)), ('misaligned_grad', dict(grad=P1 + ODD)), ('misaligned_ws', dict(ws=WS + ODD)),
               ('step_size_nan', dict(step_size=NAN)), ('max_norm_nan', dict(max_norm=NAN)), ('n_6', dict(n=6)), ('n_minus_4', dict(n=-4)),
               ('B_minus_1', dict(B=-1)), ('B_65536', dict(B=65536))])
REFUSED = ([(BCE, 'null_' + k, {k: None}) for k in ('logits', 'labels')] + [(BCE, n, kw) for n, kw in _LOSS_ROWS] +
           [(KL, 'null_' + k, {k: None}) for k in ('logits', 'clean', 'labels')] + [(KL, n, kw) for n, kw in _LOSS_ROWS] +
           [(KL, 'kl_weight_nan', dict(kl_weight=NAN))] + [(fn, n, kw) for fn in (L2, LINF) for n, kw in _STEP_ROWS])
ACCEPTED = [(fn, n, kw) for fn in (L2, LINF) for n, kw in (('B_0', dict(B=0)), ('n_0', dict(n=0)))]
NUMBERS = [(fn, 'B%d_n%d' % s, s) for fn in ('uniter_adv_delta_ws_bytes', 'uniter_adv_delta_linf_ws_bytes')
           for s in ((0, 4), (3, 4), (3, 4096), (3, 4100), (16, 98304))]

_CT = {'i': C.c_int, 'p': C.c_void_p, 'f': C.c_float}


def _call(lib, fn, overrides):
    sig, defaults = FUNCS[fn]
    unknown = set(overrides) - set(defaults)
    assert not unknown and len(sig) == len(defaults), (fn, unknown, len(sig), len(defaults))
    f = getattr(lib, fn)
    f.restype, f.argtypes = C.c_int, [_CT[ch] for ch in sig]
    return f(*dict(defaults, **overrides).values())


def observe(lib_path):
    """{'refused': {id: [rc, message]}, 'accepted': {id: rc}, 'numbers': {id: value}} of the library at lib_path"""
    lib = C.CDLL(lib_path)
    lib.uniter_last_error.restype = C.c_char_p
    out = {'refused': {}, 'accepted': {}, 'numbers': {}}
    for fn, name, kw in REFUSED:
        rc = _call(lib, fn, kw)
        out['refused']['%s:%s' % (fn, name)] = [rc, lib.uniter_last_error().decode() if rc else '']
    for fn, name, kw in ACCEPTED:
        out['accepted']['%s:%s' % (fn, name)] = _call(lib, fn, kw)
    for fn, name, args in NUMBERS:
        f = getattr(lib, fn)
        f.restype, f.argtypes = C.c_size_t, [C.c_int, C.c_int]
        out['numbers']['%s:%s' % (fn, name)] = f(*args)
    return out


if __name__ == '__main__':
    print(json.dumps(observe(sys.argv[1])))
    sys.exit(0)

import pytest      # noqa: E402  (the child process above needs neither pytest nor the package)

E_ARG, E_SHAPE = -1, -2
EXPECTED = json.loads(r'''
{"refused": {
  "uniter_bce_logits:null_logits": [-1, "bce_logits: bad argument"],
  "uniter_bce_logits:null_labels": [-1, "bce_logits: bad argument"],
  "uniter_bce_logits:B_0": [-1, "bce_logits: bad argument"],
  "uniter_bce_logits:B_minus_1": [-1, "bce_logits: bad argument"],
  "uniter_bce_kl_logits:null_logits": [-1, "bce_kl_logits: bad argument"],
  "uniter_bce_kl_logits:null_clean": [-1, "bce_kl_logits: bad argument"],
  "uniter_bce_kl_logits:null_labels": [-1, "bce_kl_logits: bad argument"],
  "uniter_bce_kl_logits:B_0": [-1, "bce_kl_logits: bad argument"],
  "uniter_bce_kl_logits:B_minus_1": [-1, "bce_kl_logits: bad argument"],
  "uniter_bce_kl_logits:kl_weight_nan": [-1, "bce_kl_logits: kl_weight is NaN"],
  "uniter_adv_delta_step:null_delta": [-1, "adv_delta_step: null pointer"],
  "uniter_adv_delta_step:null_grad": [-1, "adv_delta_step: null pointer"],
  "uniter_adv_delta_step:null_ws": [-1, "adv_delta_step: null pointer"],
  "uniter_adv_delta_step:misaligned_delta": [-1, "adv_delta_step: delta and grad must be 16-byte aligned, the workspace 8-byte"],
  "uniter_adv_delta_step:misaligned_grad": [-1, "adv_delta_step: delta and grad must be 16-byte aligned, the workspace 8-byte"],
  "uniter_adv_delta_step:misaligned_ws": [-1, "adv_delta_step: delta and grad must be 16-byte aligned, the workspace 8-byte"],
  "uniter_adv_delta_step:step_size_nan": [-1, "adv_delta_step: step_size / max_norm is NaN"],
  "uniter_adv_delta_step:max_norm_nan": [-1, "adv_delta_step: step_size / max_norm is NaN"],
  "uniter_adv_delta_step:n_6": [-2, "adv_delta_step: n must be a multiple of 4 (got 6)"],
  "uniter_adv_delta_step:n_minus_4": [-2, "adv_delta_step: n must be a multiple of 4 (got -4)"],
  "uniter_adv_delta_step:B_minus_1": [-2, "adv_delta_step: n must be a multiple of 4 (got 4100)"],
  "uniter_adv_delta_step:B_65536": [-2, "adv_delta_step: at most 65535 samples (got 65536)"],
  "uniter_adv_delta_step_linf:null_delta": [-1, "adv_delta_step_linf: null pointer"],
  "uniter_adv_delta_step_linf:null_grad": [-1, "adv_delta_step_linf: null pointer"],
  "uniter_adv_delta_step_linf:null_ws": [-1, "adv_delta_step_linf: null pointer"],
  "uniter_adv_delta_step_linf:misaligned_delta": [-1, "adv_delta_step_linf: delta and grad must be 16-byte aligned, the workspace 8-byte"],
  "uniter_adv_delta_step_linf:misaligned_grad": [-1, "adv_delta_step_linf: delta and grad must be 16-byte aligned, the workspace 8-byte"],
  "uniter_adv_delta_step_linf:misaligned_ws": [-1, "adv_delta_step_linf: delta and grad must be 16-byte aligned, the workspace 8-byte"],
  "uniter_adv_delta_step_linf:step_size_nan": [-1, "adv_delta_step_linf: step_size / max_norm is NaN"],
  "uniter_adv_delta_step_linf:max_norm_nan": [-1, "adv_delta_step_linf: step_size / max_norm is NaN"],
  "uniter_adv_delta_step_linf:n_6": [-2, "adv_delta_step_linf: n must be a multiple of 4 (got 6)"],
  "uniter_adv_delta_step_linf:n_minus_4": [-2, "adv_delta_step_linf: n must be a multiple of 4 (got -4)"],
  "uniter_adv_delta_step_linf:B_minus_1": [-2, "adv_delta_step_linf: n must be a multiple of 4 (got 4100)"],
  "uniter_adv_delta_step_linf:B_65536": [-2, "adv_delta_step_linf: at most 65535 samples (got 65536)"]
},
"numbers": {
  "uniter_adv_delta_ws_bytes:B0_n4": 0,
  "uniter_adv_delta_ws_bytes:B3_n4": 72,
  "uniter_adv_delta_ws_bytes:B3_n4096": 72,
  "uniter_adv_delta_ws_bytes:B3_n4100": 144,
  "uniter_adv_delta_ws_bytes:B16_n98304": 9216,
  "uniter_adv_delta_linf_ws_bytes:B0_n4": 0,
  "uniter_adv_delta_linf_ws_bytes:B3_n4": 16,
  "uniter_adv_delta_linf_ws_bytes:B3_n4096": 16,
  "uniter_adv_delta_linf_ws_bytes:B3_n4100": 24,
  "uniter_adv_delta_linf_ws_bytes:B16_n98304": 1536
}}
''')


@pytest.fixture(scope='module')
def observed():
    from meme_challenge_amd import _lib
    env = dict({k: v for k, v in os.environ.items() if not k.startswith('UNITER_')}, HIP_VISIBLE_DEVICES='-1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), _lib.LIB_PATH], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _ids(rows):
    return ['%s:%s' % (f, n) for f, n, _ in rows]


def test_the_table_is_recorded_in_full():
    assert sorted(EXPECTED['refused']) == sorted(_ids(REFUSED)) and sorted(EXPECTED['numbers']) == sorted(_ids(NUMBERS))
    assert len(set(_ids(REFUSED))) == len(REFUSED) == 4 + 6 + 2 * 12 and len(NUMBERS) == 10
    assert all(rc in (E_ARG, E_SHAPE) and message for rc, message in EXPECTED['refused'].values())


@pytest.mark.parametrize('row', _ids(REFUSED))
def test_refused_with_the_recorded_code_and_message(observed, row):
    assert observed['refused'][row] == EXPECTED['refused'][row]


@pytest.mark.parametrize('row', _ids(ACCEPTED))
def test_a_call_without_samples_or_elements_returns_0_without_a_launch(observed, row):
    assert observed['accepted'][row] == 0


@pytest.mark.parametrize('row', _ids(NUMBERS))
def test_sizes_are_the_recorded_integers(observed, row):
    assert observed['numbers'][row] == EXPECTED['numbers'][row]
