"""uniter_bce_kl_logits (csrc/head.hip) and uniter_adv_delta_step_linf (csrc/adv.hip) through the C ABI, against the float64 references, case lists
and bounds of tests/adv_ref.py (derivation there; tests/test_adv_bounds_cpu.py is the standing proof that an fp32 evaluation of the
formulas keeps them and that wrong formulas do not).

Every output is prefilled with a recognisable NaN and carries GUARD elements behind its last one that must still hold the prefill;
inputs must come back bit-identical.  The worst error / bound ratios per quantity are collected in WORST and printed at the end of
the module (-s shows them).
Recorded on an MI355X: total 0.061, bce 0.037, kl 0.068, probs 0.362, dlogits 0.353, Linf 0.304; 49 tests in 3 s."""
import itertools

import numpy as np
import pytest
import torch

import adv_ref as A

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 2
NANBITS = 0x7fc0beef
NANF = np.array([NANBITS], dtype=np.uint32).view(F)[0]
WORST = {}


def _L():
    from meme_challenge_amd import _lib
    return _lib


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nVILLA kernels, worst |got - float64| / bound: ' + ', '.join('%s %.3f' % kv for kv in WORST.items()))


def _hold(key, got, ref, bound, what=''):
    r = A.worst_ratio(got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, (key, what, r)


class Vec:
    """[n + GUARD] on the device: elements [0, n) hold `data` (or the prefill), the guard the prefill; compared as bit patterns"""

    def __init__(self, n, data=None, fill=NANF, dtype=F):
        host = np.full(n + GUARD, fill, dtype=dtype)
        if data is not None:
            host[:n] = np.asarray(data, dtype=dtype).reshape(n)
        self.n, self.init = n, host
        self.dev = torch.from_numpy(host.copy()).cuda()

    def ptr(self):
        return self.dev.data_ptr()

    def _bits(self, a):
        return a.view(np.uint32 if a.dtype == F else np.uint64)

    def host(self):
        return self.dev.cpu().numpy()

    def got(self):
        return self.host()[:self.n].copy()

    def unchanged(self):
        return np.array_equal(self._bits(self.host()), self._bits(self.init))

    def intact(self):
        return np.array_equal(self._bits(self.host())[self.n:], self._bits(self.init)[self.n:])


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _call(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*args, L.cur_stream()), name)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# uniter_bce_kl_logits
# ---------------------------------------------------------------------------------------------------------------------------
def _launch(z, c, y, pw, klw, gs, want=(1, 1, 1)):
    """-> (terms [3], probs [B], dlogits [B]), None for an output left out; the inputs and the outputs left out are checked to be
    untouched, the guards of the others intact"""
    B = z.size
    Z, C, Y = Vec(B, z), Vec(B, c), Vec(B, y, dtype=np.int64, fill=-7)
    outs = (Vec(3), Vec(B), Vec(B))
    ptrs = [o.ptr() if w else None for o, w in zip(outs, want)]
    _call('uniter_bce_kl_logits', Z.ptr(), C.ptr(), Y.ptr(), pw, klw, ptrs[0], ptrs[1], ptrs[2], gs, B)
    assert Z.unchanged() and C.unchanged() and Y.unchanged()
    res = []
    for o, w in zip(outs, want):
        assert o.intact() if w else o.unchanged()
        res.append(o.got() if w else None)
    return res


def _run(z, c, y, pw, klw, gs, want=(1, 1, 1)):
    terms, probs, dlog = _launch(z, c, y, pw, klw, gs, want)
    ref = A.ref_bce_kl(z, c, y, pw, klw, gs)
    what = 'B=%d pw=%g klw=%g gs=%g' % (z.size, pw, klw, gs)
    if terms is not None:
        for i, key in enumerate(('total', 'bce', 'kl')):
            _hold(key, terms[i], ref[key], ref['E_' + key], what)
        assert terms[2] >= 0
    if probs is not None:
        _hold('probs', probs, ref['probs'], ref['E_probs'], what)
    if dlog is not None:
        _hold('dlogits', dlog, ref['dlogits'], ref['E_dlogits'], what)
    return terms, probs, dlog


@pytest.mark.parametrize('B', A.BS)
def test_bce_kl_logits_matches_float64(B):
    """pos_weight 1, 1.8, 0.25 x kl_weight 0, 1, 0.3 x grad_scale 1, 0.5, 1/3 x labels all 0, all 1, mixed; from B = 64 on the leading
    logit pairs are the 49 of {0, +-30, +-88, +-100}^2"""
    for pw, klw, gs, labels in itertools.product(A.PWS, A.KLWS, A.GSS, A.LABELS):
        _run(*A.bce_kl_case(B, labels), pw, klw, gs)


def test_bce_kl_logits_at_the_planted_pairs_with_both_labels():
    for pw, klw, gs in itertools.product(A.PWS, A.KLWS, (0.5, 1.0 / 3.0)):
        _run(*A.bce_kl_planted_case(), pw, klw, gs)


@pytest.mark.parametrize('B', A.BS)
def test_bce_kl_logits_with_outputs_left_out(B):
    """every combination of terms, probs and dlogits NULL or given: the given ones are right, the others untouched"""
    for i, want in enumerate(itertools.product((0, 1), repeat=3)):
        _run(*A.bce_kl_case(B, A.LABELS[i % 3], seed=1), A.PWS[i % 3], A.KLWS[1 + i % 2], A.GSS[(i // 3) % 3], want)


@pytest.mark.parametrize('B', A.BS)
def test_equal_logits_give_an_exactly_zero_kl_term_and_gradient_share(B):
    z, c, y = A.bce_kl_equal_case(B)
    for klw in (1.0, 0.3):
        terms, probs, dlog = _run(z, c, y, 1.8, klw, 0.5)
        t0, p0, d0 = _launch(z, c, y, 1.8, 0.0, 0.5)
        assert terms[2] == 0.0 and np.array_equal(_bits(dlog), _bits(d0)) and _bits(terms[0]).tolist() == _bits(t0[0]).tolist()
    # and, among other pairs, the elements with z == c contribute nothing: the planted case's gradient there is the BCE one
    z, c, y = A.bce_kl_planted_case()
    _, _, dlog = _launch(z, c, y, 1.8, 1.0, 0.5)
    _, _, d0 = _launch(z, c, y, 1.8, 0.0, 0.5)
    same = z == c
    assert same.sum() == 14 and np.array_equal(_bits(dlog[same]), _bits(d0[same])) and not np.array_equal(_bits(dlog[~same]), _bits(d0[~same]))


@pytest.mark.parametrize('B', A.BS)
def test_kl_weight_zero_is_bce_logits_bit_for_bit(B):
    for pw, gs, labels in itertools.product(A.PWS, A.GSS, A.LABELS):
        z, c, y = A.bce_kl_case(B, labels)
        terms, probs, dlog = _launch(z, c, y, pw, 0.0, gs)
        Z, Y = Vec(B, z), Vec(B, y, dtype=np.int64, fill=-7)
        loss, p0, d0 = Vec(1), Vec(B), Vec(B)
        _call('uniter_bce_logits', Z.ptr(), Y.ptr(), pw, loss.ptr(), p0.ptr(), d0.ptr(), gs, B)
        assert _bits(terms[0]).tolist() == _bits(loss.got()[0]).tolist() == _bits(terms[1]).tolist()
        assert np.array_equal(_bits(probs), _bits(p0.got())) and np.array_equal(_bits(dlog), _bits(d0.got()))


@pytest.mark.parametrize('B', [3, 257, 1000])
def test_two_identical_launches_are_bit_equal(B):
    z, c, y = A.bce_kl_case(B, 'mixed', seed=2)
    a, b = _launch(z, c, y, 1.8, 0.3, 1.0 / 3.0), _launch(z, c, y, 1.8, 0.3, 1.0 / 3.0)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def test_bce_kl_logits_refusals_touch_nothing():
    """a NULL input, B <= 0, a NaN kl_weight: the argument error's code, an error text, and every buffer as it was"""
    L = _L()
    z, c, y = A.bce_kl_case(64, 'mixed')
    Z, C, Y = Vec(64, z), Vec(64, c), Vec(64, y, dtype=np.int64, fill=-7)
    T, P, Dl = Vec(3), Vec(64), Vec(64)
    ok = (Z.ptr(), C.ptr(), Y.ptr(), 1.8, 1.0, T.ptr(), P.ptr(), Dl.ptr(), 1.0, 64)
    for i, v in ((0, None), (1, None), (2, None), (9, 0), (9, -1), (4, float('nan'))):
        args = list(ok)
        args[i] = v
        rc = L.lib().uniter_bce_kl_logits(*args, L.cur_stream())
        assert rc == -1, (i, v, rc)
        assert L.lib().uniter_last_error()
        with pytest.raises(L.UniterHipError):
            L.check(rc, 'uniter_bce_kl_logits')
    torch.cuda.synchronize()
    assert all(v.unchanged() for v in (Z, C, Y, T, P, Dl))
    _run(z, c, y, 1.8, 1.0, 1.0)                                   # and the library is left in working order


# ---------------------------------------------------------------------------------------------------------------------------
# uniter_adv_delta_step_linf
# ---------------------------------------------------------------------------------------------------------------------------
def _linf_launch(delta, grad, step, max_norm):
    L = _L()
    B, n = delta.shape
    Dv, G = Vec(B * n, delta), Vec(B * n, grad)
    nws = L.lib().uniter_adv_delta_linf_ws_bytes(B, n)
    assert nws >= 4 * B * ((n + 4095) // 4096)
    ws = torch.empty(max(nws, 8), dtype=torch.uint8, device='cuda')
    _call('uniter_adv_delta_step_linf', Dv.ptr(), G.ptr(), B, n, step, max_norm, ws.data_ptr())
    assert G.unchanged() and Dv.intact()
    return Dv.got().reshape(B, n)


@pytest.mark.parametrize('n', A.LINF_NS)
@pytest.mark.parametrize('B', A.LINF_BS)
def test_linf_step_matches_float64_and_repeats(B, n):
    """the maximum at the first element, at the last element of the last chunk, negative, tied, and one sample without a gradient;
    with the clamp and without"""
    for kind, mn in itertools.product(A.LINF_KINDS, (A.LINF_MAX_NORM, 0.0)):
        delta, grad = A.linf_case(B, n, kind)
        got = _linf_launch(delta, grad, A.LINF_STEP, mn)
        ref, E = A.ref_linf(delta, grad, A.LINF_STEP, mn)
        _hold('linf', got, ref, E, 'B=%d n=%d %s max_norm=%g' % (B, n, kind, mn))
        moved = np.abs(got.astype(np.float64) - delta).max(axis=1)
        for b in range(B):
            if kind == 'zero' and b == B // 2:                                 # no gradient: the same bits, or exactly the clamp
                assert np.array_equal(_bits(got[b]), _bits(np.clip(delta[b], -F(mn), F(mn)) if mn > 0 else delta[b]))
            elif mn == 0:
                assert moved[b] > 0.29                                         # the planted element moved by the whole step
        if mn > 0:
            assert np.abs(got).max() <= F(mn) and (n < 4092 or ((got == F(mn)).any() and (got == -F(mn)).any()))
            assert (np.abs(got) < F(mn)).any()
        assert np.array_equal(_bits(got), _bits(_linf_launch(delta, grad, A.LINF_STEP, mn)))


@pytest.mark.parametrize('n', A.LINF_NS)
def test_linf_step_size_zero_is_an_exact_clamp(n):
    delta, grad = A.linf_case(3, n, 'last')
    delta = (delta * F(4.0)).astype(F)                                          # up to 2: well outside the ball
    delta[0, 0] = F(-0.0)
    got = _linf_launch(delta, grad, 0.0, A.LINF_MAX_NORM)
    mn = F(A.LINF_MAX_NORM)
    assert np.array_equal(_bits(got), _bits(np.clip(delta, -mn, mn))) and (np.abs(delta) > mn).any()
    assert np.array_equal(_bits(_linf_launch(delta, grad, 0.0, 0.0)), _bits(delta))      # neither a step nor a clamp: the same bits


def test_linf_step_refusals():
    """the refusals of the L2 twin: NULL pointers, misaligned delta / grad / workspace, n % 4, B > 65535, NaN scalars"""
    L = _L()
    lib, cs = L.lib(), L.cur_stream()
    buf = Vec(64, np.zeros(64))
    p = buf.ptr()
    assert p % 16 == 0
    for args, code in (((None, p, 1, 4, 1.0, 1.0, p), -1), ((p, None, 1, 4, 1.0, 1.0, p), -1), ((p, p, 1, 4, 1.0, 1.0, None), -1),
                       ((p + 4, p, 1, 4, 1.0, 1.0, p), -1), ((p, p + 8, 1, 4, 1.0, 1.0, p), -1), ((p, p, 1, 4, 1.0, 1.0, p + 4), -1),
                       ((p, p, 1, 4, float('nan'), 1.0, p), -1), ((p, p, 1, 4, 1.0, float('nan'), p), -1),
                       ((p, p, 1, 6, 1.0, 1.0, p), -2), ((p, p, 1, -4, 1.0, 1.0, p), -2), ((p, p, -1, 4, 1.0, 1.0, p), -2),
                       ((p, p, 65536, 4, 1.0, 1.0, p), -2)):
        rc = lib.uniter_adv_delta_step_linf(*args, cs)
        assert rc == code, (args, rc)
        assert lib.uniter_last_error()
    assert lib.uniter_adv_delta_step_linf(p, p, 0, 4, 1.0, 1.0, p, cs) == 0 and lib.uniter_adv_delta_step_linf(p, p, 1, 0, 1.0, 1.0, p, cs) == 0
    assert lib.uniter_adv_delta_linf_ws_bytes(0, 4) == 0 and lib.uniter_adv_delta_linf_ws_bytes(3, 4100) >= 24
    torch.cuda.synchronize()
    assert buf.unchanged()
