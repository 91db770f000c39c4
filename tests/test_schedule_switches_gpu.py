"""GPU: one training step through the model under every schedule switch of the C library (csrc/switches.h).

What csrc/model.cpp launches -- which kernel runs a product, with how many k-pieces, into which buffer, what rides on which
launch, how the workspace is carved -- is chosen per process by the switches.  Every kernel family has a float64 test through
the C ABI; this file tests the WIRING behind each switch: tests/tools/schedule_probe.py runs as a child process with the row's
environment, and what it wrote is compared (1) with the CPU oracle, computed here once per precision, and (2) with the default
schedule's run, by the row's declared expectation.

The table ROWS below is (precision, environment, expectation, why).  Expectations against the default run:
  same_bits          work moves between streams, grids or priorities, no sum changes its order: every tensor is bit-identical
                     to the default run's.  Holds per tensor only where the default run's two in-process repeats were
                     bit-identical; where they were not (float atomics) the bound is 4 x that measured repeat difference.
  forward_same_bits  backward-only switch: logits and loss as same_bits.  In the bf16 mode every gradient is also held to the
                     fp32 bar AGAINST THE DEFAULT RUN (3e-6 + 3e-4 max|default|, plus 4 x the repeat difference of either run
                     where float atomics are at work): the input-gradient chain is untouched, and the weight and bias gradients
                     sum the same bf16 products in another fp32 order -- two orders of magnitude below the bf16 noise the
                     oracle bar has to allow, which is what makes the bf16 rows sharp.
  differs            a summation order or a rounding point changes: the oracle bar applies, and the run must be told apart from
                     the default: some tensor whose default repeats were bit-identical differs in bits, or some tensor whose
                     default repeats differed (float atomics) is bit-reproducible here.  (A bare "some bit differs" would be
                     satisfied by atomics noise alone.)  That proves the switch reached its path at these shapes.

Oracle bars.  fp32 and fp32x3: those of test_model_gpu.py::test_edge_shapes_match_oracle against the float64 oracle --
logits 2e-5, each gradient 3e-6 + 3e-4 max|ref|.  bf16: the two-sided form of tests/test_parity_configs_gpu.py per tensor
(rms-relative error against the exact oracle <= factor x the bf16-rounding oracle's own + slack, _two_sided_slack imported
from there; the key-bias and zero-gradient cases kept), logits and loss within 2 x the rounding model's own distance + 2e-4;
not the median-ratio window (measured over 190 tensors at BASE size; config S has 45).  A wiring error is far outside either
bar: a missed 36-row partial block of 228 rows is ~16 % of a bias gradient.

Safety on shared machines: children run one at a time under subprocess.run(timeout = 3 x the default run's measured wall time
+ 15 s of start-up allowance; the default runs themselves get DEFAULT_TIMEOUT); a child that ends by a signal, with an abort
status, at its time limit or with a GPU fault in its output sets a module flag and every later test of this module skips with
that reason: no further GPU process is started from this file after a fault, and no test retries a child.

Float atomics.  The default schedule sums some gradients with float atomics (see _atomics below, and in the native fp32 mode the
stream-K region projection makes case d's whole forward pass vary from run to run).  Two repeats are a thin sample of that noise, so
those tensors are never asked to be bit-identical and never taken as proof that a run differs; their bound is 4 x the larger repeat
difference of the two runs, and never less than one ulp of the tensor's largest element.  Every other tensor of a same_bits row --
every weight gradient, LayerNorm gradient, dense bias, the logits and the loss of cases a, b, c and, outside fp32, d -- must be
bit-identical.

Measured on an MI355X (config S, cases a - d of tests/tools/schedule_probe.py, two repeats each):
  default run     child wall time   worst share of the oracle bar   tensors (of 216) that differ between the two repeats
  fp32            2.7 s             0.0038                          55, by at most 1.7e-6 of the tensor; 28 outside the float-atomics set, all in case d
  fp32x3          2.6 s             0.0021                          15, at most 3.2e-7; none outside the set
  bf16            2.5 s             0.77                            17, at most 2.1e-7; none outside the set
  (the probe's own share of the wall time is 2.1 - 2.2 s; a row's child takes 2.2 - 3.2 s.  The key biases, mathematically zero and
  all noise, are left out of the "of the tensor" figures.)  The fp32 bars of test_edge_shapes_match_oracle hold at config S with a
  factor 260 to spare, so they stand as they are; the float32 oracle is itself 0.0039 of the bar from the float64 one here.
  Worst share of the oracle bar over all rows: fp32 0.0038, fp32x3 0.0026, bf16 0.82 (UNITER_GELU_D=0, against the oracle with that
  switch's rounding point: _GeluB16KeepsU; against the default rounding model the same run is at 1.03, a key weight gradient).
  differs rows: tensors outside the float-atomics set that differ in bits from the default run, and the largest such difference
  relative to the tensor's largest element:
    fp32    GEMM_SK=0 and IMG_SK=0: none -- told apart by case d becoming reproducible (10 - 12 tensors differ between the row's
            repeats, all in the set, against 55); ATTN_SPLIT=0 28, 7.2e-7; GELU_D=0 85, 2.2e-6
    fp32x3  X3_CFG_FFN_UP_FWD=4 112, 1.4e-6; X3_CFG=1 and 2 112, 2.0e-6; ATTN_X3=0 84, 1.9e-6; KEEP_PREGEN=0 84, 2.2e-6
    bf16    KEEP_PREGEN=0 6, 1.5e-7; ATTN_B16X=0 (with and without ATTN_BWD_FUSED=0) 10, 1.8e-4; GELU_D=0 (alone and with
            B16_PERSIST=12) 96, 1.5e-2; B16_PERSIST=12 and 15 18, 5.1e-7 (the riders' column reductions)
  Rows reclassified from the issue's first guess, each with its reason in the table: UNITER_B16_PERSIST = 1, 2, 8 and 12 with
  B16_RIDERS=0 are bit-identical to the default run (same_bits, not differs); UNITER_KEEP_PREGEN=0 changes the forward attention
  kernel in the fp32x3 and bf16 modes (differs, not same_bits); UNITER_X3_WIDE=0, UNITER_X3_192=0 and UNITER_X3_BALANCED=2 cannot
  change a launch at config S (same_bits: they need more than 256 tiles of 128 x 128, i.e. M > 2048 rows); UNITER_GEMM_SK=2 equals 1
  below 901 tiles.  UNITER_DCTX_SPLIT=0 and UNITER_X3_BALANCED=1 left every tensor outside the set bit-identical as well (K = 128 has
  one k-piece; the grouped launch of config S fits one round).  No switch was found dead in the code, and no row found a wiring fault.
  Planted in a scratch build: `nparts = M / 64` in fill_layer_riders makes the library refuse case b (M = 2: "bad reduction job 3")
  in the fp32x3 default run and under B16_PERSIST=12; one slab fewer in the row pass behind a B16_PERSIST=2 product puts a LayerNorm
  gradient at 3.3e-2 rms-relative where the rounding model allows 1.5e-3.
"""
import importlib.util
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import uniter_oracle as O
from oracle import step_oracle as S
from test_parity_configs_gpu import _two_sided_slack
from test_switches_cpu import SWITCHES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(REPO, 'tests', 'tools', 'schedule_probe.py')
_spec = importlib.util.spec_from_file_location('schedule_probe', PROBE_PATH)
PROBE = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(PROBE)

gpu = pytest.mark.gpu
DEFAULT_TIMEOUT = 300

SAME, FWD, DIFF = 'same_bits', 'forward_same_bits', 'differs'

# (precision, environment, expectation, why)
ROWS = [
    # ---------------------------------------------------------------------------------------------- native fp32
    ('fp32', {'UNITER_MAIN_PRIO': '2'}, SAME, 'wave priority of the main stream\'s products only'),
    ('fp32', {'UNITER_ATTN_PRIO': '0'}, SAME, 'wave priority of the attention kernels only'),
    ('fp32', {'UNITER_GEMM_SK': '0'}, DIFF, 'case d: the region projection and its weight gradient leave the stream-K form (no float atomics left in the forward pass)'),
    ('fp32', {'UNITER_GEMM_SK': '2', 'UNITER_WGRAD_WHOLE': '0'}, FWD,
     '2 differs from the heuristic only for products that fill >= 88 % of their rounds\' slots (>= 901 tiles of 64 x 64: UNITER-large\'s FFN '
     'weight gradients); at config S every product that may go stream-K already does under 1, so the row is WGRAD_WHOLE=0 with the mode read'),
    ('fp32', {'UNITER_IMG_SK': '0'}, DIFF, 'case d (28 tiles, 3584 k-units): the region projection as a bias-epilogue product instead of stream-K on bias rows'),
    ('fp32', {'UNITER_WGRAD_WHOLE': '0', 'UNITER_WGRAD_CFG': '21'}, FWD, 'weight gradients on 128 x 128 stream-K tiles'),
    ('fp32', {'UNITER_WGRAD_WHOLE': '0', 'UNITER_WGRAD_CFG': '24'}, FWD, 'weight gradients on 64 x 64 stream-K tiles (case d: 64 tiles x 32 k-units go stream-K)'),
    ('fp32', {'UNITER_WGRAD_WHOLE': '5'}, FWD, 'two of the four shapes on whole tiles: the grouped layer-0 launch must stand down'),
    ('fp32', {'UNITER_WGRAD_WHOLE': '0', 'UNITER_WGRAD_SLOTS_F32': '256'}, FWD, 'pieces of the stream-K weight gradients'),
    ('fp32', {'UNITER_WGRAD_GROUP_F32': '1', 'UNITER_WGRAD_GROUP_F32_SLOTS': '64'}, FWD, 'every layer\'s weight gradients as one grouped launch, 64 workgroups walking the tiles'),
    ('fp32', {'UNITER_WGRAD_GROUP_F32': '0'}, FWD, 'no grouped launch: four launches in layer 0 too'),
    ('fp32', {'UNITER_ATTN_SPLIT': '0'}, DIFF, 'the one-wave-per-block resident attention kernels; no fused query|key|value bias partials'),
    ('fp32', {'UNITER_ATTN_BWD_FUSED': '0'}, FWD, 'the L <= 192 attention backward as two launches'),
    ('fp32', {'UNITER_KEEP_PREGEN': '0'}, SAME, 'the attention kernels draw the keep flags themselves: the same Philox words'),
    ('fp32', {'UNITER_HIDDEN_PREGEN': '1'}, SAME, 'the row passes read pre-drawn keep flags: the same Philox words'),
    ('fp32', {'UNITER_EMBED_BWD_PAR': '0'}, SAME, 'the embedding backward\'s two branches on one stream (implicit type ids: the branches share no row)'),
    ('fp32', {'UNITER_GELU_D': '0'}, DIFF, 'the FFN-up epilogue stores u, the backward evaluates gelu\' by libm erf'),
    ('fp32', {'UNITER_LNB_WAVES': '8', 'UNITER_LNB_ROWS': '1'}, FWD, 'geometry of the LayerNorm backward row pass: other partial rows'),
    # ---------------------------------------------------------------------------------------------- fp32 from three bf16 pieces
    ('fp32x3', {'UNITER_MAIN_PRIO_X3': '2'}, SAME, 'wave priority only'),
    ('fp32x3', {'UNITER_ATTN_PRIO': '0'}, SAME, 'wave priority only'),
    ('fp32x3', {'UNITER_X3_BAND_H': '1'}, SAME, 'the order of the tile walk only'),
    ('fp32x3', {'UNITER_WGRAD_X3_WGS': '0'}, SAME, 'grid of the grouped weight-gradient launch: whole-K tiles, reduction items by one workgroup each'),
    ('fp32x3', {'UNITER_WGRAD_X3_WGS': '64'}, SAME, 'the same with 64 workgroups walking the tiles and the riders\' items'),
    ('fp32x3', {'UNITER_HIDDEN_PREGEN': '1'}, SAME, 'pre-drawn keep flags of the row passes'),
    ('fp32x3', {'UNITER_EMBED_BWD_PAR': '0'}, SAME, 'one stream for the embedding backward'),
    ('fp32x3', {'UNITER_GATHER_EX': '0'}, SAME, 'gather and operand copy as two launches: the same fp32 rows, the same three pieces of them'),
    ('fp32x3', {'UNITER_X3_WIDE': '0'}, SAME,
     'x3_choose prices one round of 128 x 128 tiles cheapest for every product with <= 256 of them (config S: <= 128), so the 128 x 256 / '
     '128 x 192 candidates the switch removes never win here: it needs M > 2048 rows at N = 2048.  The row checks that reading it breaks nothing'),
    ('fp32x3', {'UNITER_X3_192': '0'}, SAME, 'as UNITER_X3_WIDE: 128 x 192 tiles win only with > 256 tiles of 128 x 128 (M > 10 900 rows at N = 384)'),
    ('fp32x3', {'UNITER_X3_CFG_FFN_UP_FWD': '4'}, DIFF, 'the FFN-up forward alone on 128 x 256 tiles (two ragged tile rows at M = 228)'),
    ('fp32x3', {'UNITER_X3_CFG': '1'}, DIFF, 'every x3 product on the 64 x 32-wave geometry; the grouped launch without riders: separate finalize / column-sum launches'),
    ('fp32x3', {'UNITER_X3_CFG': '2'}, DIFF, 'the 64 x 64-wave geometry of the older MFMA shape; no riders'),
    ('fp32x3', {'UNITER_X3_CFG': '3'}, FWD, 'x3_choose picks 128 x 128 for every product of config S anyway; the grouped launch moves to 128 x 128 tiles with colsum_out riding'),
    ('fp32x3', {'UNITER_X3_BALANCED': '1'}, FWD, 'the balanced walk of the grouped weight gradients; its workspace carved behind the layers'),
    ('fp32x3', {'UNITER_X3_BALANCED': '2'}, SAME,
     'bit 1 carves and clears the main-stream workspace, but the balanced walk acts on 128 x 256-tile bias-epilogue products and x3_choose puts none '
     'of config S there: the row checks the carving (test_model_gpu.py runs UNITER_X3_BALANCED=3 at BASE size, where the walk runs)'),
    ('fp32x3', {'UNITER_X3_RIDERS': '0'}, FWD, 'separate finalize / column-sum / sum-of-squares launches instead of riders'),
    ('fp32x3', {'UNITER_X3_WGRAD_CFG': '3'}, FWD, 'the grouped launch on 128 x 128 tiles: colsum_out rides, no column partials from the dU product'),
    ('fp32x3', {'UNITER_DCTX_SPLIT': '0'}, FWD, 'the attention-output input gradient as one tensor'),
    ('fp32x3', {'UNITER_ATTN_X3': '0'}, DIFF, 'attention on the fp32 MFMA kernels'),
    ('fp32x3', {'UNITER_KEEP_PREGEN': '0'}, DIFF,
     'without pre-drawn keep flags attn_kernel() pairs the fp32-MFMA forward kernel (ATTN_F32_PRE_X3) with the x3 backward: other arithmetic in the forward pass'),
    ('fp32x3', {'UNITER_ATTN_BWD_FUSED': '0'}, SAME, 'read by attention_f32.hip / attention_bf16.hip only: cases a, b, d run the x3 backward, case c (L = 320) the streaming one'),
    ('fp32x3', {'UNITER_LNB_ROWS': '1'}, FWD, 'rows per wave of the LayerNorm backward row pass'),
    # ---------------------------------------------------------------------------------------------- bf16-resident
    ('bf16', {'UNITER_MAIN_PRIO_BF16': '0'}, SAME, 'wave priority only'),
    ('bf16', {'UNITER_ATTN_PRIO': '0'}, SAME, 'wave priority only'),
    ('bf16', {'UNITER_HIDDEN_PREGEN': '1'}, SAME, 'pre-drawn keep flags of the row passes'),
    ('bf16', {'UNITER_EMBED_BWD_PAR': '0'}, SAME, 'one stream for the embedding backward'),
    ('bf16', {'UNITER_GATHER_EX': '0'}, SAME, 'gather and operand copy as two launches: the same rows, the same rounding'),
    ('bf16', {'UNITER_WGRAD_GROUP_WGS': '0'}, SAME, 'one workgroup per tile of the grouped launch: whole-K tiles'),
    ('bf16', {'UNITER_KEEP_PREGEN': '0'}, DIFF,
     'without pre-drawn keep flags attn_kernel() takes attention_bf16.hip\'s forward kernel (ATTN_BF16_PRE) and the context\'s operand copy is made after the fact'),
    ('bf16', {'UNITER_ATTN_B16X': '0'}, DIFF, 'attention_bf16.hip\'s kernels forward and backward'),
    ('bf16', {'UNITER_ATTN_B16X': '0', 'UNITER_ATTN_BWD_FUSED': '0'}, DIFF, 'and their backward as two launches'),
    ('bf16', {'UNITER_GELU_D': '0'}, DIFF, 'u stored as bf16, gelu\' by libm erf in the dU epilogue'),
    ('bf16', {'UNITER_B16_PERSIST': '1'}, SAME,
     'QKV forward on persistent 128 x 192 tiles'
     ' -- measured bit-identical to the default run: gemm_dma_kernel (32x32x16 MFMA) and the persistent kernels (16x16x32) add the same exact '
     'bf16 products over k in ascending order from zero, in the same k-pieces, and agree in every bit on this hardware; so the row asks for '
     'exact equality, which no mis-wired slab, buffer or epilogue survives.  That the path runs is read from linear(): ' 'K = 128 is a multiple of 64 and 3 H = 384 of 192'),
    ('bf16', {'UNITER_B16_PERSIST': '2'}, SAME,
     'N = hidden products with k-pieces on persistent 128 x 128 tiles, the pieces by b1p_choose (two for K = 2048 at every case, as gemm_bf16v2_pick_split says)'
     ' -- measured bit-identical to the default run: gemm_dma_kernel (32x32x16 MFMA) and the persistent kernels (16x16x32) add the same exact '
     'bf16 products over k in ascending order from zero, in the same k-pieces, and agree in every bit on this hardware; so the row asks for '
     'exact equality, which no mis-wired slab, buffer or epilogue survives.  That the path runs is read from linear(): ' 'the FFN-down forward and the FFN-up input gradient have two pieces and N = 128'),
    ('bf16', {'UNITER_B16_PERSIST': '4'}, FWD, 'grouped weight gradients on the persistent 128 x 256 kernel; without bit 8 no riders'),
    ('bf16', {'UNITER_B16_PERSIST': '8'}, SAME,
     'the wide products on persistent 128 x 256 tiles'
     ' -- measured bit-identical to the default run: gemm_dma_kernel (32x32x16 MFMA) and the persistent kernels (16x16x32) add the same exact '
     'bf16 products over k in ascending order from zero, in the same k-pieces, and agree in every bit on this hardware; so the row asks for '
     'exact equality, which no mis-wired slab, buffer or epilogue survives.  That the path runs is read from linear(): ' 'the FFN-up forward and the dU product have one piece and N = 2048'),
    ('bf16', {'UNITER_B16_PERSIST': '12'}, DIFF, 'bits 4 + 8: riders on, dU\'s column partials from the producing product (gemm_b1p_run with colpart), finished by a fourth reduction job'),
    ('bf16', {'UNITER_B16_PERSIST': '12', 'UNITER_B16_RIDERS': '0'}, SAME,
     'bits 4 + 8 without riders: the default schedule\'s separate finalize / column-sum launches behind persistent products -- bit-identical as the rows of bits 1, 2, 8'),
    ('bf16', {'UNITER_B16_PERSIST': '15'}, DIFF, 'all four bits'),
    ('bf16', {'UNITER_B16_PERSIST': '12', 'UNITER_GELU_D': '0'}, DIFF, 'without the gelu\' form there is no x aux epilogue to carry column partials: riders must stand down'),
    ('bf16', {'UNITER_B16_RIDERS': '1'}, FWD, 'riders on the default grouped launch (gemm_bf16_dma.hip)'),
    ('bf16', {'UNITER_WGRAD_GROUP': '0'}, FWD, 'four stream-K launches with float atomics'),
    ('bf16', {'UNITER_WGRAD_GROUP': '0', 'UNITER_WGRAD_SLABS': '1'}, FWD, 'split-K slabs + one reduce pass (case d: K = 1024 rows)'),
    ('bf16', {'UNITER_WGRAD_GROUP': '0', 'UNITER_WGRAD_SLOTS': '384'}, FWD, 'pieces of the stream-K weight gradients'),
    ('bf16', {'UNITER_WGRAD_GROUP': '2'}, FWD, 'three early products next to the attention backward, the fourth behind it'),
    ('bf16', {'UNITER_WGRAD_GROUP': '4'}, FWD, 'the grouped launch with three LDS stages'),
    ('bf16', {'UNITER_ATTN_BWD_FUSED': '0'}, SAME, 'read by attention_bf16.hip / attention_f32.hip: the default bf16 backward is attention_x3.hip\'s for L <= 192; case c runs attention_f32.hip\'s streaming kernel'),
    ('bf16', {'UNITER_LNB_WAVES': '8'}, FWD, 'waves per workgroup of the LayerNorm backward row pass'),
]

# switches with no model-level row, and why
EXEMPT = {
    'UNITER_ATTN_X3_LAB': 'measurement builds only (-DUNITER_X3_LAB): the library as built does not read it',
}


def row_id(row):
    return '%s-%s' % (row[0], ','.join('%s=%s' % (k.replace('UNITER_', ''), v) for k, v in sorted(row[1].items())))


def test_every_switch_has_a_model_level_row():
    """CPU: the names in ROWS plus the exemptions are exactly the switch table's names (tests/test_switches_cpu.py): a new switch
    cannot arrive without a row here"""
    named = set()
    for prec, env, expect, why in ROWS:
        assert prec in PROBE.PRECISIONS and expect in (SAME, FWD, DIFF) and why and env
        named.update(env)
    assert not (named & set(EXEMPT)), 'exempt and tested: %s' % sorted(named & set(EXEMPT))
    assert named | set(EXEMPT) == set(SWITCHES), (sorted(set(SWITCHES) - named - set(EXEMPT)), sorted((named | set(EXEMPT)) - set(SWITCHES)))
    assert len({row_id(r) for r in ROWS}) == len(ROWS)


# ---------------------------------------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------------------------------------
STATE = {'dead': None, 'wall': {}, 'default': {}, 'oracle': {}}
FAULT_WORDS = ('illegal memory access', 'Memory access fault', 'HSA_STATUS_ERROR', 'hipErrorLaunchFailure', 'Aborted', 'Segmentation fault')


def run_probe(precision, env, out, timeout):
    """One child, never retried.  Returns (arrays, wall seconds); a fault closes the module (STATE['dead'])."""
    if STATE['dead']:
        pytest.skip('no GPU process after a fault: ' + STATE['dead'])
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}        # the default run is the default schedule
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, PROBE_PATH, '--precision', precision, '--out', out], cwd=REPO, env=dict(base, **env),
                           capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        STATE['dead'] = '%s %s hit its time limit of %.0f s' % (precision, env, timeout)
        pytest.fail(STATE['dead'])
    wall = time.time() - t0
    tail = (r.stdout[-1500:] + r.stderr[-2500:])
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137) or any(w in tail for w in FAULT_WORDS):
        STATE['dead'] = '%s %s ended with status %d' % (precision, env, r.returncode)
        pytest.fail(STATE['dead'] + '\n' + tail)
    assert r.returncode == 0, (precision, env, r.returncode, tail)
    with np.load(out) as z:
        arrays = {k: z[k] for k in z.files}
    os.remove(out)
    return arrays, wall


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp('schedule_probe')


@pytest.fixture(scope='module')
def default_run(workdir):
    """precision -> the default schedule's run, launched once per precision and module"""
    def get(precision):
        if precision not in STATE['default']:
            arrays, wall = run_probe(precision, {}, str(workdir / ('default_%s.npz' % precision)), DEFAULT_TIMEOUT)
            STATE['default'][precision] = arrays
            STATE['wall'][precision] = wall
            print('default run %s: wall %.1f s (the probe\'s own %.1f s)' % (precision, wall, float(arrays['seconds'])))
        return STATE['default'][precision]
    return get


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle, on the CPU, once per module
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_step(name, prec, dtype):
    sd = PROBE.state_dict()
    b = PROBE.batch(name)
    if dtype == torch.float64:
        b = {k: (v.double() if v.is_floating_point() else v) for k, v in b.items()}
    sdo = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    cfg = PROBE.CONFIG_S
    drop = O.DropSpec(PROBE.DROP_SEED, PROBE.DROP_OFFSET, cfg['hidden_dropout_prob'], cfg['attention_probs_dropout_prob'])
    lo = O.meme_uniter_forward(sdo, cfg, drop=drop, prec=prec, **PROBE.model_kwargs(b))
    loss = S.bce_with_logits(lo, b['labels'], PROBE.POS_WEIGHT)
    loss.backward()
    out = {'logits': lo.detach().double().numpy(), 'loss': float(loss.detach())}
    for n, v in sdo.items():
        out['grad/' + n] = (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy()
    return out


class _GeluB16KeepsU(torch.autograd.Function):
    """the bf16 mode's GELU with UNITER_GELU_D=0: the FFN-up epilogue stores the pre-activation u as bf16 (not gelu'(u)), and the dU
    epilogue evaluates gelu' of that rounded u -- dU = bf(dH * gelu'(bf(u))) where the default path has bf(dH * bf(gelu'(u))).
    The two-sided bar compares the kernels with an oracle that rounds WHAT THEY ROUND (oracle/uniter_oracle.py); the key / query
    weight gradients, mostly rounding noise, move by +-40 % rms between the two rounding points."""

    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(O.bf(u))
        return O.bf(u * (0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))))

    @staticmethod
    def backward(ctx, dh):
        (ub,) = ctx.saved_tensors
        cdf = 0.5 * (1.0 + torch.erf(ub / math.sqrt(2.0)))
        pdf = torch.exp(-0.5 * ub * ub) / math.sqrt(2.0 * math.pi)
        return O.bf(dh * (cdf + ub * pdf))


def oracle(kind):
    """kind 'f64': the reference arithmetic in float64; 'f32': the same in float32; 'bf16': the bf16-rounding mode (float32);
    'bf16_u': that mode with UNITER_GELU_D=0's rounding point (_GeluB16KeepsU).  case -> {logits, loss, grad/<name>} as float64 arrays"""
    if kind not in STATE['oracle']:
        prec, dtype = {'f64': ('fp32', torch.float64), 'f32': ('fp32', torch.float32), 'bf16': ('bf16', torch.float32),
                       'bf16_u': ('bf16', torch.float32)}[kind]
        default_gelu = O._GeluB16
        try:
            if kind == 'bf16_u':
                O._GeluB16 = _GeluB16KeepsU
            STATE['oracle'][kind] = {c: _oracle_step(c, prec, dtype) for c in PROBE.CASES}
        finally:
            O._GeluB16 = default_gelu
    return STATE['oracle'][kind]


# ---------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------
LOGIT_BAR = 2e-5
LOSS_BAR = PROBE.POS_WEIGHT * LOGIT_BAR + 1e-6      # |d loss / d logit| <= pos_weight, mean over the batch; 1e-6: fp32 rounding of a loss ~ 1


def grad_bar(ref):
    return 3e-6 + 3e-4 * float(np.abs(ref).max())


def _maxdiff(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max()) if np.size(a) else 0.0


def _rms_rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def tensors(run, case, rep=0):
    pre = '%s/%d/' % (case, rep)
    return {k[len(pre):]: v for k, v in run.items() if k.startswith(pre)}


def repeat_noise(run):
    """(case, tensor) -> max |repeat 1 - repeat 0| of one run"""
    out = {}
    for c in PROBE.CASES:
        t0, t1 = tensors(run, c, 0), tensors(run, c, 1)
        for k in t0:
            out[(c, k)] = 0.0 if _same_bits(t0[k], t1[k]) else max(_maxdiff(t0[k], t1[k]), 1e-45)
    return out


def check_oracle_fp32(run, problems, shares=None):
    """logits 2e-5, each gradient 3e-6 + 3e-4 max|ref| against the float64 oracle; both repeats"""
    ref = oracle('f64')
    worst = 0.0
    for c in PROBE.CASES:
        for rep in range(PROBE.REPEATS):
            t = tensors(run, c, rep)
            assert len(t) == len(ref[c]), (c, sorted(set(ref[c]) ^ set(t)))
            for k, r in ref[c].items():
                if k == 'loss':
                    share = abs(float(t[k]) - r) / LOSS_BAR
                elif k == 'logits':
                    share = _maxdiff(t[k].reshape(-1), r.reshape(-1)) / LOGIT_BAR
                else:
                    share = _maxdiff(t[k], r) / grad_bar(r)
                worst = max(worst, share)
                if not share <= 1.0:
                    problems.append('oracle: case %s repeat %d %s at %.3g of its bar' % (c, rep, k, share))
    return worst


def check_oracle_bf16(run, problems, model='bf16'):
    """the two-sided per-tensor form of tests/test_parity_configs_gpu.py (module docstring); returns the worst eh / (fac eo + slack)"""
    gf, gb = oracle('f64'), oracle(model)
    worst = 0.0
    for c in PROBE.CASES:
        noise = _maxdiff(gb[c]['logits'], gf[c]['logits'])
        lnoise = abs(gb[c]['loss'] - gf[c]['loss'])
        for rep in range(PROBE.REPEATS):
            t = tensors(run, c, rep)
            assert len(t) == len(gf[c]), (c, sorted(set(gf[c]) ^ set(t)))
            d = _maxdiff(t['logits'].reshape(-1), gf[c]['logits'].reshape(-1))
            worst = max(worst, d / (2.0 * noise + 2e-4))
            if not d <= 2.0 * noise + 2e-4:
                problems.append('oracle: case %s repeat %d logits %.3g from the exact oracle, the rounding model %.3g' % (c, rep, d, noise))
            if not abs(float(t['loss']) - gf[c]['loss']) <= 2.0 * lnoise + 2e-4:
                problems.append('oracle: case %s repeat %d loss %.6g, exact %.6g, rounding model %.6g' % (c, rep, float(t['loss']), gf[c]['loss'], gb[c]['loss']))
            for k, r in gf[c].items():
                if not k.startswith('grad/'):
                    continue
                g = t[k]
                if k.endswith('attention.self.key.bias'):
                    # mathematically zero (a constant added to every key's score does not move the softmax): rounding noise only
                    qb = t[k.replace('key.bias', 'query.bias')]
                    if not float(np.abs(g).max()) <= 0.2 * float(np.abs(qb).max()) + 1e-12:
                        problems.append('oracle: case %s repeat %d %s is not noise: %.3g against a query bias of %.3g' % (c, rep, k, np.abs(g).max(), np.abs(qb).max()))
                    continue
                if float(np.abs(r).max()) == 0.0:
                    if float(np.abs(g).max()) != 0.0:
                        problems.append('oracle: case %s repeat %d %s must be zero' % (c, rep, k))
                    continue
                eh, eo = _rms_rel(g, r), _rms_rel(gb[c][k], r)
                fac, slack = _two_sided_slack(k[len('grad/'):], g.size)
                worst = max(worst, eh / (fac * eo + slack))
                if not eh <= fac * eo + slack:
                    problems.append('oracle: case %s repeat %d %s rms-relative %.3g, the rounding model %.3g' % (c, rep, k, eh, eo))
    return worst


# Gradients the DEFAULT schedule sums with float atomics, in arrival order (UniterModel.deterministic lists what it takes to fix
# them): both embedding branches' parameters, the query|key|value bias partials of the attention backward, intermediate.dense's
# bias where a separate column-sum launch forms it.  Two repeats are a thin sample of such noise -- a tensor's repeats can coincide
# and the next process still lands one ulp away -- so these tensors are never asked to be bit-identical and never taken as proof
# that a run differs.  In the native fp32 mode the stream-K region projection (UNITER_IMG_SK) makes a whole case's forward pass
# noisy: then every tensor of that case is treated so.
def _atomics(k):
    return (k.startswith('grad/uniter_model.embeddings.') or k.startswith('grad/uniter_model.img_embeddings.')
            or k.endswith('attention.self.query.bias') or k.endswith('attention.self.key.bias') or k.endswith('attention.self.value.bias')
            or k.endswith('intermediate.dense.bias'))


def compare_with_default(precision, expect, run, dflt, problems):
    """the row's expectation against the default run (module docstring); returns (tensors outside the float-atomics set that differ
    in bits from the default run, the largest such difference relative to the tensor's largest element, where)"""
    nd, nr = repeat_noise(dflt), repeat_noise(run)
    told_apart, ndiff, biggest = False, 0, (0.0, None)
    for c in PROBE.CASES:
        a, b = tensors(dflt, c, 0), tensors(run, c, 0)
        fwd_noise = max(nd[(c, 'logits')], nr[(c, 'logits')])
        rel_fwd = fwd_noise / max(float(np.abs(a['logits']).max()), 1e-30)
        # a case whose forward pass is noisy in the default run (stream-K region projection: tensors OUTSIDE the float-atomics set differ
        # between its repeats) and reproducible here: the atomics left the forward pass
        free = [k for k in a if not _atomics(k)]
        if sum(1 for k in free if nd[(c, k)] > 0.0) >= 8 and not any(nr[(c, k)] > 0.0 for k in free):
            told_apart = True
        for k in a:
            same = _same_bits(a[k], b[k])
            d = 0.0 if same else _maxdiff(a[k], b[k])
            scale = float(np.abs(a[k]).max())
            if k.endswith('attention.self.key.bias'):      # (mathematically zero: its noise is an ulp of dK's terms, which are the size of dQ's)
                scale = max(scale, float(np.abs(a[k.replace('key.bias', 'query.bias')]).max()))
            exposed = _atomics(k) or fwd_noise > 0.0 or nd[(c, k)] > 0.0
            if not exposed and not same:
                told_apart, ndiff = True, ndiff + 1
                if scale > 0 and d / scale > biggest[0]:
                    biggest = (d / scale, '%s %s' % (c, k))
            # what 4 x the repeat difference is taken of: either run's sample, and never less than one ulp of the tensor's largest
            # element or the relative noise of the case's logits (a small tensor's two repeats coincide easily)
            noise = max(nd[(c, k)], nr[(c, k)], 2.0 ** -23 * scale, rel_fwd * scale)
            if expect == SAME or (expect == FWD and k in ('logits', 'loss')):
                if not exposed:
                    if not same:
                        problems.append('default: case %s %s is not bit-identical to the default run (off by %.3g, scale %.3g)' % (c, k, d, scale))
                elif not d <= 4.0 * noise:
                    problems.append('default: case %s %s off by %.3g, 4 x the repeat difference is %.3g' % (c, k, d, 4.0 * noise))
            elif expect == FWD and precision == 'bf16':
                bar = grad_bar(a[k]) + (4.0 * noise if exposed or nr[(c, k)] > 0.0 else 0.0)
                if not d <= bar:
                    problems.append('default: case %s %s off by %.3g from the default run, bar %.3g' % (c, k, d, bar))
    if expect == DIFF and not told_apart:
        problems.append('default: nothing tells this run from the default run: the switch did not reach its path at these shapes')
    return ndiff, biggest


def evaluate(row, default_run, workdir):
    precision, env, expect, why = row
    dflt = default_run(precision)
    run, wall = run_probe(precision, env, str(workdir / 'row.npz'), 3.0 * STATE['wall'][precision] + 15.0)
    problems = []
    if precision == 'bf16':
        share = check_oracle_bf16(run, problems, 'bf16_u' if env.get('UNITER_GELU_D') == '0' else 'bf16')
    else:
        share = check_oracle_fp32(run, problems)
    ndiff, biggest = compare_with_default(precision, expect, run, dflt, problems)
    noisy = sum(1 for v in repeat_noise(run).values() if v > 0.0)
    print('%s [%s]: wall %.1f s, worst share of the oracle bar %.3g; outside the float-atomics set %d tensors differ in bits from the default run, '
          'at most %.3g of the tensor (%s); %d tensors differ between its own repeats; %d problems'
          % (row_id(row), expect, wall, share, ndiff, biggest[0], biggest[1], noisy, len(problems)))
    return problems


@gpu
@pytest.mark.parametrize('precision', PROBE.PRECISIONS)
def test_default_schedule_at_config_s(precision, default_run):
    """the default schedule itself against the oracle at config S, both repeats; its repeat differences are what the rows' bounds use"""
    dflt = default_run(precision)
    problems = []
    share = check_oracle_bf16(dflt, problems) if precision == 'bf16' else check_oracle_fp32(dflt, problems)
    noise = {k: v for k, v in repeat_noise(dflt).items() if v > 0.0}
    # (relative to the tensor's largest element; the key biases, mathematically zero, are all noise and left out of the figure)
    rel = max([v / max(float(np.abs(tensors(dflt, c, 0)[k]).max()), 1e-30) for (c, k), v in noise.items() if not k.endswith('key.bias')] or [0.0])
    free = sorted({'%s %s' % (c, k) for (c, k) in noise if not _atomics(k)})
    print('default %s: worst share of the oracle bar %.3g; %d of %d tensors differ between the two repeats, at most %.3g of the tensor; '
          '%d of them outside the float-atomics set: %s' % (precision, share, len(noise), len(repeat_noise(dflt)), rel, len(free), free[:6]))
    assert not problems, problems[:20]


@gpu
@pytest.mark.parametrize('row', ROWS, ids=row_id)
def test_schedule_switch(row, default_run, workdir):
    problems = evaluate(row, default_run, workdir)
    assert not problems, (row_id(row), row[3], problems[:20])
