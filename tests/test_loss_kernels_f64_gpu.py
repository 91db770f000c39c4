"""uniter_bce_logits (csrc/head.hip) and the kernels of csrc/heads.hip -- cross-entropy, KL divergence, row argmax, MSE, dgelu_mul, row
gather and scatter-add -- through the C ABI, against the float64 references, case lists and bounds of tests/loss_ref.py (derivation
there; tests/test_loss_bounds_cpu.py is the standing proof that an fp32 evaluation of the formulas keeps them and that wrong formulas
do not).

Every output is prefilled with a recognisable NaN (-7 for the int64 argmax output) and every row output carries GUARD rows behind
row n - 1 that must still hold the prefill, as must the [C, ld) padding of every output row.  Inputs with ld > C hold NaN in their
padding (+inf for the argmax input: NaN loses every comparison and would hide a read past C) and must come back bit-identical.  The
backward launches get the float64 log-sum-exp rounded to fp32, so an error of the forward kernel can neither mask nor fake one of
the backward; one case chains the two launches as the model does.  Nothing here reads or writes outside its buffers: indices and
targets outside their range take only the values the kernels guard in memory (-1, one past the end, 2^33 + 1).

The worst error / bound ratios per quantity are collected in WORST and printed at the end of the module (-s shows them).
Recorded on an MI355X: CE lse 0.198, loss 0.198, dlogits 0.346; KL lse 0.198, loss 0.203, dlogits 0.327; BCE loss 0.045, probs 0.359,
dlogits 0.351; MSE 0.474, its backward 0.271; dgelu_mul 0.296; 68 tests in 3 s."""
import itertools

import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 2
NANBITS = 0x7fc0beef
NANF = np.array([NANBITS], dtype=np.uint32).view(F)[0]
INF = F(np.inf)
WORST = {}


def _L():
    from meme_challenge_amd import _lib
    return _lib


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nloss kernels, worst |got - float64| / bound: ' + ', '.join('%s %.3f' % kv for kv in WORST.items()))


def _hold(key, got, ref, bound, what=''):
    r = R.worst_ratio(got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    print('%s %s: %.3f of the bound' % (key, what, r))
    assert r <= 1.0, (key, what, r)


class Mat:
    """[n + guard, ld] on the device: rows [0, n) x columns [0, C) hold `data` (or the prefill), everything else `pad` (inputs) or
    the prefill (outputs); compared as bit patterns"""

    def __init__(self, n, C, ld=None, data=None, pad=NANF, fill=NANF, guard=GUARD, dtype=F):
        ld = C if ld is None else ld
        host = np.full((n + guard, ld), fill, dtype=dtype)
        if data is not None:
            if ld > C:
                host[:n, C:] = pad
            host[:n, :C] = np.asarray(data, dtype=dtype).reshape(n, C)
        self.n, self.C, self.ld = n, C, ld
        self.init = host
        self.dev = torch.from_numpy(host.copy()).cuda()

    def ptr(self):
        return self.dev.data_ptr()

    def host(self):
        return self.dev.cpu().numpy()

    def got(self):
        return self.host()[:self.n, :self.C].copy()

    def _bits(self, a):
        return a.view(np.uint32 if a.dtype == F else np.uint64)

    def unchanged(self):
        return np.array_equal(self._bits(self.host()), self._bits(self.init))

    def intact(self):
        """the padding of rows [0, n) and the guard rows hold what they held"""
        h, i = self._bits(self.host()), self._bits(self.init)
        return np.array_equal(h[:self.n, self.C:], i[:self.n, self.C:]) and np.array_equal(h[self.n:], i[self.n:])


def Vec(n, data=None, **kw):
    """a per-row vector [n] with guard elements behind it"""
    return Mat(n, 1, 1, data, **kw)


def _call(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*args, L.cur_stream()), name)
    torch.cuda.synchronize()


def _refused(name, *args):
    L = _L()
    rc = getattr(L.lib(), name)(*args, L.cur_stream())
    assert rc != 0, name
    with pytest.raises(L.UniterHipError):
        L.check(rc, name)


# ---------------------------------------------------------------------------------------------------------------------------
# cross-entropy
# ---------------------------------------------------------------------------------------------------------------------------
def _ce_run(c, C, ld, chain=False, alias=False):
    x, t, g = c['x'], c['t'], c['dloss']
    n = x.shape[0]
    X, T, G = Mat(n, C, ld, x), Vec(n, t, dtype=np.int64, fill=-7), Vec(n, g)
    loss, lse = Vec(n), Vec(n)
    _call('uniter_cross_entropy_fwd', X.ptr(), T.ptr(), loss.ptr(), lse.ptr(), n, C, ld)
    assert X.unchanged() and T.unchanged() and loss.intact() and lse.intact()
    ref = R.ref_ce_fwd(x, t)
    what = 'C=%d n=%d ld=%d' % (C, n, ld)
    _hold('ce_lse', lse.got()[:, 0], ref['lse'], ref['E_lse'], what)
    _hold('ce_loss', loss.got()[:, 0], ref['loss'], ref['E_loss'], what)
    lse_in = lse.got()[:, 0] if chain else ref['lse'].astype(F)
    LSE = Vec(n, lse_in)
    out = Mat(n, C, ld)
    _call('uniter_cross_entropy_bwd', X.ptr(), T.ptr(), LSE.ptr(), G.ptr(), out.ptr(), n, C, ld)
    assert X.unchanged() and T.unchanged() and LSE.unchanged() and G.unchanged() and out.intact()
    ref_d, E_d = R.ref_ce_bwd(x, t, lse_in, g)
    _hold('ce_dlogits', out.got(), ref_d, E_d, what)
    if alias:                                   # dlogits == logits, which the header allows: bit for bit the out-of-place result
        _call('uniter_cross_entropy_bwd', X.ptr(), T.ptr(), LSE.ptr(), G.ptr(), X.ptr(), n, C, ld)
        assert X.intact() and np.array_equal(X.got().view(np.uint32), out.got().view(np.uint32))
    return out


@pytest.mark.parametrize('C', R.ROW_CS)
def test_cross_entropy_matches_float64(C):
    """n = 1, 5 and the planted rows (a maximum on every edge column, +-1e4 shifts, equal maxima, the target the maximum and 40
    below it, targets -1 / C / 2^33 + 1 against the reference at the clamped target), each at ld = C, C + 3, roundup4(C) + 4"""
    for n, ld in itertools.product(R.ROW_NS, R.row_lds(C)):
        _ce_run(R.ce_case(C, n), C, ld, alias=(ld != C + 3))


def test_cross_entropy_at_the_vocabulary_size():
    _ce_run(R.ce_case(R.VOCAB, 3), R.VOCAB, R.VOCAB, alias=True)


@pytest.mark.parametrize('C', [2, 257, 1601])
def test_cross_entropy_forward_chained_into_backward(C):
    """the way the model does it: the backward launch reads the lse the forward launch left on the device"""
    _ce_run(R.ce_case(C, 'planted'), C, C + 3, chain=True)


@pytest.mark.parametrize('C', [1, 2, 65, 1601])
def test_cross_entropy_targets_outside_the_range_agree_forward_and_backward(C):
    """targets -1, C and 2^33 + 1 (which narrows to 1): loss and one-hot of the SAME, clamped, column.  With the backward kernel's
    earlier `c == (int)targets[row]` the one-hot sat nowhere (-1, C) or on column 1 and this test failed; it passes with the
    clamp shared by both launches."""
    r = np.random.default_rng(C)
    t = np.array([-1, C, 2 ** 33 + 1], dtype=np.int64)
    c = dict(x=(3.0 * r.standard_normal((3, C))).astype(F), t=t, dloss=np.array([1.0, -2.0, 0.5], dtype=F))
    out = _ce_run(c, C, C + 3).got()
    tc = R.clamp_targets(t, C)
    assert list(tc) == [0, C - 1, C - 1]
    if C > 1:                                    # the one-hot column is the only one whose sign is that of -dloss
        assert np.array_equal(np.argmax(-out * np.sign(c['dloss'])[:, None], axis=1), tc)


# ---------------------------------------------------------------------------------------------------------------------------
# KL divergence
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', R.ROW_CS)
def test_kl_div_matches_float64(C):
    """as the cross-entropy list; targets softmax(randn * 2) with a tenth of exact zeros, a row of zeros and a one-hot row"""
    for n, ld in itertools.product(R.ROW_NS, R.row_lds(C)):
        c = R.kl_case(C, n)
        x, t, dl = c['x'], c['t'], c['dloss']
        rows = x.shape[0]
        what = 'C=%d n=%d ld=%d' % (C, rows, ld)
        X, T, DL = Mat(rows, C, ld, x), Mat(rows, C, ld, t), Mat(rows, C, ld, dl)
        loss, lse = Mat(rows, C, ld), Vec(rows)
        _call('uniter_kl_div_fwd', X.ptr(), T.ptr(), loss.ptr(), lse.ptr(), rows, C, ld)
        assert X.unchanged() and T.unchanged() and loss.intact() and lse.intact()
        ref = R.ref_kl_fwd(x, t)
        _hold('kl_lse', lse.got()[:, 0], ref['lse'], ref['E_lse'], what)
        _hold('kl_loss', loss.got(), ref['loss'], ref['E_loss'], what)
        assert not loss.got()[t == 0].view(np.uint32).any()         # +0.0 where the target is 0
        lse_in = ref['lse'].astype(F)
        LSE, out = Vec(rows, lse_in), Mat(rows, C, ld)
        _call('uniter_kl_div_bwd', X.ptr(), T.ptr(), LSE.ptr(), DL.ptr(), out.ptr(), rows, C, ld)
        assert X.unchanged() and T.unchanged() and LSE.unchanged() and DL.unchanged() and out.intact()
        _hold('kl_dlogits', out.got(), *R.ref_kl_bwd(x, t, lse_in, dl), what)


# ---------------------------------------------------------------------------------------------------------------------------
# row argmax
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', R.ARGMAX_CS)
def test_row_argmax_is_the_first_maximum_behind_c0(C):
    """n = 1, 3, 4, 5 rows of distinct values and the planted rows (ties in one lane, in neighbouring lanes and across the lane wrap,
    the maximum at c0, larger values in [0, c0), all -inf -> c0), c0 = 0, 1, C - 1, ld = C and C + 5 with +inf in the padding"""
    for c0, n, ld in itertools.product(R.argmax_c0s(C), R.ARGMAX_NS, R.argmax_lds(C)):
        x, names = R.argmax_case(C, n, c0)
        rows = x.shape[0]
        X, out = Mat(rows, C, ld, x, pad=INF), Vec(rows, dtype=np.int64, fill=-7)
        _call('uniter_row_argmax', X.ptr(), rows, C, ld, c0, out.ptr())
        assert X.unchanged() and out.intact()
        got, ref = out.got()[:, 0], R.ref_argmax(x, c0)
        assert np.array_equal(got, ref), (C, c0, n, ld, [(nm, g, r) for nm, g, r in zip(names, got, ref) if g != r])
        assert np.array_equal(ref, torch.max(torch.from_numpy(x)[:, c0:], dim=-1)[1].numpy() + c0)


# ---------------------------------------------------------------------------------------------------------------------------
# BCE with logits
# ---------------------------------------------------------------------------------------------------------------------------
def _bce_run(x, y, pw, gs, want=(1, 1, 1)):
    B = x.size
    X, Y = Vec(B, x), Vec(B, y, dtype=np.int64, fill=-7)
    loss, probs, dlog = Vec(1), Vec(B), Vec(B)
    outs = [o.ptr() if w else None for o, w in zip((loss, probs, dlog), want)]
    _call('uniter_bce_logits', X.ptr(), Y.ptr(), pw, outs[0], outs[1], outs[2], gs, B)
    assert X.unchanged() and Y.unchanged()
    ref = R.ref_bce(x, y, pw, gs)
    what = 'B=%d pw=%g gs=%g' % (B, pw, gs)
    for key, o, w in zip(('loss', 'probs', 'dlogits'), (loss, probs, dlog), want):
        if w:
            assert o.intact()
            _hold('bce_' + key, o.got()[:, 0], ref[key], ref['E_' + key], what)
        else:
            assert o.unchanged()


@pytest.mark.parametrize('B', R.BCE_BS)
def test_bce_logits_matches_float64(B):
    """pos_weight 1, 1.8, 0.25 x grad_scale 1, 0.5, 0.125 x labels all 0, all 1, mixed; the leading logits 0, +-30, +-88, +-100"""
    for pw, gs, labels in itertools.product(R.BCE_PWS, R.BCE_GSS, R.BCE_LABELS):
        _bce_run(*R.bce_case(B, labels), pw, gs)


@pytest.mark.parametrize('B', R.BCE_BS)
def test_bce_logits_with_outputs_left_out(B):
    """every combination of loss, probs and dlogits NULL or given: the given ones are right, the others untouched"""
    for i, want in enumerate(itertools.product((0, 1), repeat=3)):
        _bce_run(*R.bce_case(B, R.BCE_LABELS[i % 3], seed=1), R.BCE_PWS[i % 3], R.BCE_GSS[(i // 3) % 3], want)


def test_bce_logits_at_large_logits_with_both_labels():
    for pw in R.BCE_PWS:
        _bce_run(*R.bce_planted_case(), pw, 0.5)


# ---------------------------------------------------------------------------------------------------------------------------
# MSE, dgelu_mul
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', R.ELEM_NS)
def test_mse_matches_float64(n):
    p, t, dl = R.mse_case(n)
    P, T, DL, loss, dp = Vec(n, p), Vec(n, t), Vec(n, dl), Vec(n), Vec(n)
    _call('uniter_mse_fwd', P.ptr(), T.ptr(), loss.ptr(), n)
    _call('uniter_mse_bwd', P.ptr(), T.ptr(), DL.ptr(), dp.ptr(), n)
    assert P.unchanged() and T.unchanged() and DL.unchanged() and loss.intact() and dp.intact()
    _hold('mse', loss.got()[:, 0], *R.ref_mse_fwd(p, t), 'n=%d' % n)
    _hold('mse_bwd', dp.got()[:, 0], *R.ref_mse_bwd(p, t, dl), 'n=%d' % n)
    assert not loss.got()[:, 0][p == t].any() and not dp.got()[:, 0][p == t].any()


@pytest.mark.parametrize('n', R.ELEM_NS)
def test_dgelu_mul_matches_float64(n):
    """u ~ 2 randn and 0, +-1e-4, +-1, +-5, +-6, +-10, +-40"""
    dy, u = R.dgelu_case(n)
    DY, Uu, out = Vec(n, dy), Vec(n, u), Vec(n)
    _call('uniter_dgelu_mul', DY.ptr(), Uu.ptr(), out.ptr(), n)
    assert DY.unchanged() and Uu.unchanged() and out.intact()
    _hold('dgelu', out.got()[:, 0], *R.ref_dgelu_mul(dy, u), 'n=%d' % n)


# ---------------------------------------------------------------------------------------------------------------------------
# row gather and scatter-add
# ---------------------------------------------------------------------------------------------------------------------------
def _gather_scatter(n, H, oob=False):
    src, rows, idx = R.gather_case(n, H, seed=n, oob=oob)
    S, I, dst = Mat(R.NSRC, H, data=src), Vec(n, idx, dtype=np.int64, fill=-7), Mat(n, H)
    _call('uniter_row_gather', S.ptr(), I.ptr(), dst.ptr(), n, H, R.NSRC)
    assert S.unchanged() and I.unchanged() and dst.intact()
    assert np.array_equal(dst.got().view(np.uint32), R.ref_gather(src, idx).view(np.uint32)), (n, H)
    Rw, acc = Mat(n, H, data=rows), Mat(R.NSRC, H, data=src)
    _call('uniter_row_scatter_add', Rw.ptr(), I.ptr(), acc.ptr(), n, H, R.NSRC)
    assert Rw.unchanged() and I.unchanged() and acc.intact()
    assert np.array_equal(acc.got().view(np.uint32), R.ref_scatter_add(rows, idx, src).view(np.uint32)), (n, H)


@pytest.mark.parametrize('H', R.GATHER_HS)
def test_row_gather_and_scatter_add_are_exact(H):
    """n = 1, 3, 4, 5, 9 rows out of / into 11, the indices 0 and 10 among them"""
    for n in R.GATHER_NS:
        _gather_scatter(n, H)


@pytest.mark.parametrize('H', [4, 260])
def test_row_gather_clamps_and_scatter_add_skips_indices_outside_the_range(H):
    for n in (5, 9):
        _gather_scatter(n, H, oob=True)


# ---------------------------------------------------------------------------------------------------------------------------
# nothing to do, and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_empty_calls_return_zero_and_touch_nothing():
    a, b, c, d = Vec(8), Vec(8), Vec(8), Vec(8)
    idx = Vec(4, np.zeros(4), dtype=np.int64, fill=-7)
    for name, args in (('uniter_mse_fwd', (a.ptr(), b.ptr(), c.ptr(), 0)), ('uniter_mse_bwd', (a.ptr(), b.ptr(), c.ptr(), d.ptr(), 0)),
                       ('uniter_dgelu_mul', (a.ptr(), b.ptr(), c.ptr(), 0)),
                       ('uniter_row_gather', (a.ptr(), idx.ptr(), b.ptr(), 0, 4, 2)),
                       ('uniter_row_scatter_add', (a.ptr(), idx.ptr(), b.ptr(), 0, 4, 2)),
                       ('uniter_cross_entropy_fwd', (a.ptr(), idx.ptr(), b.ptr(), c.ptr(), 0, 2, 2)),
                       ('uniter_cross_entropy_bwd', (a.ptr(), idx.ptr(), b.ptr(), c.ptr(), d.ptr(), 0, 2, 2)),
                       ('uniter_kl_div_fwd', (a.ptr(), b.ptr(), c.ptr(), d.ptr(), 0, 2, 2)),
                       ('uniter_kl_div_bwd', (a.ptr(), b.ptr(), c.ptr(), d.ptr(), d.ptr(), 0, 2, 2)),
                       ('uniter_row_argmax', (a.ptr(), 0, 2, 2, 0, idx.ptr()))):
        _call(name, *args)
    assert all(m.unchanged() for m in (a, b, c, d, idx))


def test_refused_calls_touch_nothing():
    """NULL pointers, C = 0, ld < C, c0 >= C, B = 0, H % 4 != 0: nonzero, an error text, and every buffer as it was"""
    L = _L()
    a, b, c, d, e = (Mat(4, 8) for _ in range(5))
    idx = Vec(4, np.zeros(4), dtype=np.int64, fill=-7)
    A, Bp, Cp, Dp, E, I = (m.ptr() for m in (a, b, c, d, e, idx))
    refused = [
        ('uniter_cross_entropy_fwd', (None, I, Bp, Cp, 4, 8, 8)), ('uniter_cross_entropy_fwd', (A, None, Bp, Cp, 4, 8, 8)),
        ('uniter_cross_entropy_fwd', (A, I, None, Cp, 4, 8, 8)), ('uniter_cross_entropy_fwd', (A, I, Bp, None, 4, 8, 8)),
        ('uniter_cross_entropy_fwd', (A, I, Bp, Cp, 4, 0, 8)), ('uniter_cross_entropy_fwd', (A, I, Bp, Cp, 4, 8, 7)),
        ('uniter_cross_entropy_fwd', (A, I, Bp, Cp, -1, 8, 8)),
        ('uniter_cross_entropy_bwd', (None, I, Bp, Cp, Dp, 4, 8, 8)), ('uniter_cross_entropy_bwd', (A, None, Bp, Cp, Dp, 4, 8, 8)),
        ('uniter_cross_entropy_bwd', (A, I, None, Cp, Dp, 4, 8, 8)), ('uniter_cross_entropy_bwd', (A, I, Bp, None, Dp, 4, 8, 8)),
        ('uniter_cross_entropy_bwd', (A, I, Bp, Cp, None, 4, 8, 8)), ('uniter_cross_entropy_bwd', (A, I, Bp, Cp, Dp, 4, 0, 8)),
        ('uniter_cross_entropy_bwd', (A, I, Bp, Cp, Dp, 4, 8, 7)),
        ('uniter_kl_div_fwd', (None, Bp, Cp, Dp, 4, 8, 8)), ('uniter_kl_div_fwd', (A, None, Cp, Dp, 4, 8, 8)),
        ('uniter_kl_div_fwd', (A, Bp, None, Dp, 4, 8, 8)), ('uniter_kl_div_fwd', (A, Bp, Cp, None, 4, 8, 8)),
        ('uniter_kl_div_fwd', (A, Bp, Cp, Dp, 4, 0, 8)), ('uniter_kl_div_fwd', (A, Bp, Cp, Dp, 4, 8, 7)),
        ('uniter_kl_div_bwd', (None, Bp, Cp, Dp, E, 4, 8, 8)), ('uniter_kl_div_bwd', (A, None, Cp, Dp, E, 4, 8, 8)),
        ('uniter_kl_div_bwd', (A, Bp, None, Dp, E, 4, 8, 8)), ('uniter_kl_div_bwd', (A, Bp, Cp, None, E, 4, 8, 8)),
        ('uniter_kl_div_bwd', (A, Bp, Cp, Dp, None, 4, 8, 8)), ('uniter_kl_div_bwd', (A, Bp, Cp, Dp, E, 4, 0, 8)),
        ('uniter_kl_div_bwd', (A, Bp, Cp, Dp, E, 4, 8, 7)),
        ('uniter_row_argmax', (None, 4, 8, 8, 0, I)), ('uniter_row_argmax', (A, 4, 8, 8, 0, None)),
        ('uniter_row_argmax', (A, 4, 0, 8, 0, I)), ('uniter_row_argmax', (A, 4, 8, 7, 0, I)),
        ('uniter_row_argmax', (A, 4, 8, 8, 8, I)), ('uniter_row_argmax', (A, 4, 8, 8, -1, I)),
        ('uniter_bce_logits', (None, I, 1.8, Bp, Cp, Dp, 1.0, 4)), ('uniter_bce_logits', (A, None, 1.8, Bp, Cp, Dp, 1.0, 4)),
        ('uniter_bce_logits', (A, I, 1.8, Bp, Cp, Dp, 1.0, 0)),
        ('uniter_mse_fwd', (None, Bp, Cp, 4)), ('uniter_mse_fwd', (A, None, Cp, 4)), ('uniter_mse_fwd', (A, Bp, None, 4)),
        ('uniter_mse_bwd', (None, Bp, Cp, Dp, 4)), ('uniter_mse_bwd', (A, None, Cp, Dp, 4)), ('uniter_mse_bwd', (A, Bp, None, Dp, 4)),
        ('uniter_mse_bwd', (A, Bp, Cp, None, 4)),
        ('uniter_dgelu_mul', (None, Bp, Cp, 4)), ('uniter_dgelu_mul', (A, None, Cp, 4)), ('uniter_dgelu_mul', (A, Bp, None, 4)),
        ('uniter_row_gather', (None, I, Bp, 4, 8, 4)), ('uniter_row_gather', (A, None, Bp, 4, 8, 4)),
        ('uniter_row_gather', (A, I, None, 4, 8, 4)), ('uniter_row_gather', (A, I, Bp, 4, 6, 4)),
        ('uniter_row_gather', (A, I, Bp, 4, 8, 0)),
        ('uniter_row_scatter_add', (None, I, Bp, 4, 8, 4)), ('uniter_row_scatter_add', (A, None, Bp, 4, 8, 4)),
        ('uniter_row_scatter_add', (A, I, None, 4, 8, 4)), ('uniter_row_scatter_add', (A, I, Bp, 4, 6, 4)),
        ('uniter_row_scatter_add', (A, I, Bp, 4, 8, 0)),
    ]
    for name, args in refused:
        _refused(name, *args)
        assert L.lib().uniter_last_error(), name
    torch.cuda.synchronize()
    assert all(m.unchanged() for m in (a, b, c, d, e, idx))
    # and the library is left in working order
    _gather_scatter(3, 8)
