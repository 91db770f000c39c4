"""CPU: the reference side of tests/test_call_forms_gpu.py (tests/call_forms_ref.py over oracle/uniter_oracle.py).

The packed layout's hidden-dropout index (oracle.uniter_oracle.packed_hidden_index) is the identity of the default index when
no sample is padded, does nothing at p = 0 and changes the step with ragged lengths and p > 0; and the float32 oracle stands
within a quarter of the fp32 bars from the float64 oracle in every call form, which is what lets the GPU test compare with the
float32 one.  Measured shares (float32 against float64 oracle, worst tensor of each kind over the nine forms):
layer outputs 0.10 of 2e-5 (img_masks_train, layer 2), logits 0.0031 (all_eval_grad), gradients 0.0036 of 3e-6 + 3e-4 max|ref|
(img_only_train, layer 0's query weight), loss 0.0024 of its first-order bar (img_masks_train).
"""
import numpy as np
import pytest
import torch

from oracle import uniter_oracle as O
import call_forms_ref as R


def _same(a, b):
    """the forward pass and the loss in every bit; the gradients to 1e-6 of the tensor's largest element (torch's threaded
    embedding backward sums rows in an order that varies from run to run: two runs of the SAME step differ by an ulp or two)"""
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k.startswith('grad/'):
            assert np.abs(x - y).max() <= 1e-6 * np.abs(x).max(), k
        else:
            assert np.array_equal(x, y), k


def test_packed_index_is_the_identity_at_full_length():
    L = R.T + R.R
    idx = O.packed_hidden_index([L] * R.B, L, R.H)
    assert torch.equal(idx.reshape(-1), torch.arange(R.B * L * R.H))
    b = R.batch([R.T] * R.B, [R.R] * R.B)
    _same(R.reference_step('packed_all_train', b=b, packed_index=True), R.reference_step('packed_all_train', b=b, packed_index=False))


def test_packed_index_maps_valid_positions_to_packed_rows():
    lens = [3, 1, 2]
    idx = O.packed_hidden_index(lens, 4, 2)
    rows = idx[..., 0] // 2
    assert rows.tolist() == [[0, 1, 2, 0], [3, 0, 0, 0], [4, 5, 0, 0]]        # (padded positions: element 0)
    assert torch.equal(idx[..., 1][rows > 0], idx[..., 0][rows > 0] + 1)
    assert int(idx.max()) == sum(lens) * 2 - 1


def test_packed_index_changes_nothing_without_dropout():
    _same(R.reference_step('packed_all_train', p_drop=0.0, packed_index=True), R.reference_step('packed_all_train', p_drop=0.0, packed_index=False))


@pytest.mark.parametrize('form', ['packed_train', 'packed_all_train', 'packed_txt_only_train'])
def test_packed_index_changes_a_ragged_training_step(form):
    a, b = R.reference_step(form, packed_index=True), R.reference_step(form, packed_index=False)
    assert a['loss'] != b['loss']
    # sample 0 starts at packed row 0 = padded row 0: its rows draw the same flags either way, and with them layer 0's output
    # of that sample; the other samples' rows do not
    last = 'layer/%d' % (R.NL - 1)
    assert not np.array_equal(a[last][1:], b[last][1:])
    g = 'grad/uniter_model.encoder.layer.0.output.dense.weight'
    d = np.abs(a[g] - b[g]).max()
    assert d > 100 * R.grad_bar(a[g]), (d, R.grad_bar(a[g]))        # far outside the bar the GPU test holds the library to


@pytest.mark.parametrize('form', list(R.FORMS))
def test_float32_oracle_within_a_quarter_of_the_fp32_bars(form):
    """the float32 oracle's distance from the float64 oracle as a share of the fp32 bars of the GPU test: under 1 / 4 for every
    layer output, the logits, the loss and every gradient"""
    f32, f64 = R.reference_step(form, 'fp32', torch.float32), R.reference_step(form, 'fp32', torch.float64)
    shares = R.fp32_shares(f32, f64)
    worst = {}
    for k, s in shares.items():
        kind = k.split('/')[0]
        if s >= worst.get(kind, (-1.0, None))[0]:
            worst[kind] = (s, k)
    print('%s: float32 against float64 oracle, worst shares %s' % (form, {k: '%.2g (%s)' % v for k, v in worst.items()}))
    bad = {k: s for k, s in shares.items() if not s < 0.25}
    assert not bad, bad
    f = R.FORMS[form]
    assert sorted(k for k in f64 if k.startswith('layer/')) == ['layer/%d' % l for l in (range(R.NL) if f['all_layers'] else [R.NL - 1])]
    assert ('logits' in f64) == f['head']


def test_forms_give_every_probed_layer_its_own_gradient():
    """what makes the GPU test sharp: in all_train the loss reaches the parameters through every layer's output (dropping one
    layer's probe moves layer 0's gradients far outside the bar), and in mid_only nothing above layer 1 gets a gradient"""
    full = R.reference_step('all_train')
    saved = dict(R.FORMS['all_train'])
    try:
        for drop in (0, 1, 2):
            R.FORMS['all_train'] = dict(saved, probes=tuple(l for l in (0, 1, 2) if l != drop))
            part = R.reference_step('all_train')
            g = 'grad/uniter_model.encoder.layer.0.output.dense.weight'
            assert np.abs(full[g] - part[g]).max() > 100 * R.grad_bar(full[g]), drop
    finally:
        R.FORMS['all_train'] = saved
    mid = R.reference_step('mid_only')
    for k, v in mid.items():
        if k.startswith('grad/') and 'mask_embedding' not in k:        # (no img_masks in this form: unused)
            above = '.layer.2.' in k or '.pooler.' in k or k.startswith('grad/linear.')
            assert (np.abs(v).max() == 0.0) == above, k
