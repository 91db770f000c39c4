"""The six pooler / classifier entry points of csrc/head.hip -- uniter_pooler_fwd / _bwd, uniter_linear_small_fwd / _bwd and the
one-launch forms uniter_pool_head_fwd / _bwd -- through the C ABI, against the float64 references, case lists and bounds of
tests/head_ref.py (derivation there; tests/test_head_bounds_cpu.py is the standing proof that an fp32 evaluation of the formulas
keeps them and that wrong formulas do not).

Every case runs the separate chain and the fused pair, each with beta_dhidden 0 and 1.  Rows 1 .. L-1 of `hidden` hold NaN (only
row 0 may be read: every result must be finite), pooled and logits start as NaN (every element must be overwritten), rows 1 .. L-1
of dhidden hold a NaN-free sentinel bit pattern that must survive bit for bit, and row 0 of a beta = 0 launch starts as NaN (it is
assigned, not added to).  The backward references are evaluated on the kernel's own fp32 pooled rows (and, for uniter_pooler_bwd,
on the kernel's own fp32 dpooled), so an error of one launch can neither mask nor fake one of the next.  The header's claim that the
fused launches EQUAL the separate ones is asserted with torch.equal on all seven outputs of every case.

The worst error / bound ratios per quantity are collected in WORST and printed at the end of the module (-s shows them).
Recorded on an MI355X: pooler_fwd pooled 0.074; linear_small_fwd logits 0.082; linear_small_bwd dx 0.428, dW 0.442, db 0.215;
pooler_bwd dWp 0.498, dbp 0.485, dhidden 0.091 (beta = 1: 0.486); pool_head_fwd pooled 0.074, logits 0.082; pool_head_bwd dWp
0.498, dbp 0.484, dWl 0.442, dbl 0.215, dhidden 0.066 (beta = 1: 0.484); the ticket sequence's logits 0.082; through the model
0.004 (16 classes, fused) and 0.003 (17, separate).  The accumulating outputs sit just below one half because the final add's
rounding alone reaches U |g0 + s| of a bound that ends in 2 U |g0 + s| (head_ref.py).  Every fused output was bit-equal to the
separate launches' at every case; 67 tests in 5 s."""
import functools

import numpy as np
import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
SENT_BITS = 0x4b3c2d1e                       # 12332318.0f: finite, so a beta = 1 launch that touched a row would change it
TICKET_WORDS = 17 * 64                       # UNITER_POOL_HEAD_TICKET_WORDS
WORST = {}
CASES = R.cases()
IDS = [R.case_id(s, p) for s, p in CASES]
ARRAYS = ('hidden', 'Wp', 'bp', 'Wl', 'bl', 'dlog', 'dWp0', 'dbp0', 'dWl0', 'dbl0', 'dh_prev')


def _L():
    from meme_challenge_amd import _lib
    return _lib


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nhead kernels, worst |got - float64| / bound: ' + ', '.join('%s %.3f' % kv for kv in sorted(WORST.items())))


def _hold(key, got, ref, bound, what=''):
    r = R.worst_ratio(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    print('%s %s: %.3f of the bound' % (key, what, r))
    assert r <= 1.0, (key, what, r)


def _call(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*[L.ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], L.cur_stream()), name)


@functools.lru_cache(maxsize=None)
def _case(shape, pattern='randn', seed=0):
    """the host case (shared, never modified) and the forward reference of it"""
    c = R.head_case(shape, pattern, seed)
    return c, R.ref_pooler_fwd(c['hidden'], c['Wp'], c['bp'])


def _dev(c):
    """the case on the device; rows 1 .. L-1 of hidden are NaN"""
    d = {k: torch.from_numpy(c[k]).cuda() for k in ARRAYS}
    d['hidden_live'] = d['hidden']
    d['hidden'] = d['hidden'].clone()
    d['hidden'][:, 1:] = float('nan')
    return d


def _ticket():
    return torch.zeros(TICKET_WORDS, dtype=torch.int32, device='cuda')


def _sentinel(shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device='cuda').view(torch.float32)


def _dhidden(d, beta):
    """the sentinel in rows 1 .. L-1; row 0: the prior value a beta = 1 launch adds to, NaN for a beta = 0 launch"""
    t = _sentinel(d['hidden'].shape)
    t[:, 0] = d['dh_prev'][:, 0] if beta else float('nan')
    return t


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_separate(d, beta, hidden=None, bwd_hidden=None):
    hidden = d['hidden'] if hidden is None else hidden
    B, L, H = hidden.shape
    Cn = d['Wl'].shape[0]
    o = dict(pooled=_nan(B, H), logits=_nan(B, Cn), dpooled=_nan(B, H), dhidden=_dhidden(d, beta))
    o.update({k: d[k + '0'].clone() for k in ('dWp', 'dbp', 'dWl', 'dbl')})
    _call('uniter_pooler_fwd', hidden, d['Wp'], d['bp'], o['pooled'], B, L, H)
    _call('uniter_linear_small_fwd', o['pooled'], d['Wl'], d['bl'], o['logits'], B, H, Cn)
    _call('uniter_linear_small_bwd', d['dlog'], o['pooled'], d['Wl'], o['dpooled'], o['dWl'], o['dbl'], B, H, Cn)
    _call('uniter_pooler_bwd', o['dpooled'], o['pooled'], hidden if bwd_hidden is None else bwd_hidden, d['Wp'], o['dWp'], o['dbp'],
          o['dhidden'], B, L, H, beta)
    return o


def run_fused(d, ticket, beta, hidden=None, bwd_hidden=None, with_dhidden=True):
    hidden = d['hidden'] if hidden is None else hidden
    B, L, H = hidden.shape
    Cn = d['Wl'].shape[0]
    o = dict(pooled=_nan(B, H), logits=_nan(B, Cn), dhidden=_dhidden(d, beta) if with_dhidden else None)
    o.update({k: d[k + '0'].clone() for k in ('dWp', 'dbp', 'dWl', 'dbl')})
    _call('uniter_pool_head_fwd', hidden, d['Wp'], d['bp'], d['Wl'], d['bl'], o['pooled'], o['logits'], ticket, B, L, H, Cn)
    _call('uniter_pool_head_bwd', d['dlog'], o['pooled'], hidden if bwd_hidden is None else bwd_hidden, d['Wp'], d['Wl'], o['dWp'],
          o['dbp'], o['dWl'], o['dbl'], o['dhidden'], B, L, H, Cn, beta)
    return o


OUTPUTS = ('pooled', 'logits', 'dWp', 'dbp', 'dWl', 'dbl', 'dhidden')


def _check_frame(o, what):
    """every output written and finite; rows 1 .. L-1 of dhidden hold the sentinel's bits"""
    for k in OUTPUTS:
        assert torch.isfinite(o[k]).all(), (what, k)
    assert bool((_bits(o['dhidden'][:, 1:]) == SENT_BITS).all()), what


# ---------------------------------------------------------------------------------------------------------------------------
# bounds, exact properties, fused == separate: every case
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,pattern', CASES, ids=IDS)
def test_both_paths_keep_the_bounds_and_equal_each_other(shape, pattern):
    c, fwd = _case(shape, pattern)
    d = _dev(c)
    ticket = _ticket()
    what = R.case_id(shape, pattern)
    for beta in (0, 1):
        sep = run_separate(d, beta)
        fus = run_fused(d, ticket, beta)
        torch.cuda.synchronize()
        assert int(ticket.abs().sum()) == 0, what
        _check_frame(sep, what + ' separate')
        _check_frame(fus, what + ' fused')
        assert torch.isfinite(sep['dpooled']).all()
        for k in OUTPUTS:                                         # the header: the fused results EQUAL the separate launches'
            assert torch.equal(fus[k], sep[k]), (what, 'beta=%d' % beta, k, float((fus[k] - sep[k]).abs().max()))
        # the references: the forward's of the inputs, everything behind it of the kernel's own fp32 pooled rows
        # (computed once: the second pass of the loop must reproduce pooled and dpooled bit for bit)
        if beta == 0:
            first = sep
            pooled = sep['pooled'].cpu().numpy()
            lg, E_lg = R.ref_linear_fwd(pooled, c['Wl'], c['bl'])
            lb = R.ref_linear_bwd(c['dlog'], pooled, c['Wl'], c['dWl0'], c['dbl0'])
            pb = R.ref_pooler_bwd(sep['dpooled'].cpu().numpy(), pooled, c['hidden'], c['Wp'], c['dWp0'], c['dbp0'], c['dh_prev'])
            hb = R.ref_head_bwd(c, pooled)
        else:
            assert torch.equal(sep['pooled'], first['pooled']) and torch.equal(sep['dpooled'], first['dpooled'])
        dh = 'dh0_add' if beta else 'dh0'
        _hold('pooler_fwd.pooled', sep['pooled'], fwd['pooled'], fwd['E_pooled'], what)
        _hold('linear_small_fwd.logits', sep['logits'], lg, E_lg, what)
        _hold('linear_small_bwd.dx', sep['dpooled'], lb['dx'], lb['E_dx'], what)
        _hold('linear_small_bwd.dW', sep['dWl'], lb['dW'], lb['E_dW'], what)
        _hold('linear_small_bwd.db', sep['dbl'], lb['db'], lb['E_db'], what)
        _hold('pooler_bwd.dWp', sep['dWp'], pb['dWp'], pb['E_dWp'], what)
        _hold('pooler_bwd.dbp', sep['dbp'], pb['dbp'], pb['E_dbp'], what)
        _hold('pooler_bwd.' + dh, sep['dhidden'][:, 0], pb[dh], pb['E_' + dh], what)
        _hold('pool_head_fwd.pooled', fus['pooled'], fwd['pooled'], fwd['E_pooled'], what)
        _hold('pool_head_fwd.logits', fus['logits'], lg, E_lg, what)
        for k in ('dWp', 'dbp', 'dWl', 'dbl'):
            _hold('pool_head_bwd.' + k, fus[k], hb[k], hb['E_' + k], what)
        _hold('pool_head_bwd.' + dh, fus['dhidden'][:, 0], hb[dh], hb['E_' + dh], what)
        # the exact values the patterns promise
        prev0 = d['dh_prev'][:, 0]
        for o in (sep, fus):
            if pattern == 'zero_pre':
                assert not o['pooled'].any() and torch.equal(o['logits'], d['bl'].expand_as(o['logits']))
            if pattern == 'saturated':
                rows = c['sat_rows']
                assert torch.equal(o['pooled'][rows], torch.from_numpy(np.sign(fwd['pre'][rows]).astype(F)).cuda())
                assert torch.equal(o['dhidden'][rows, 0], prev0[rows] if beta else torch.zeros_like(prev0[rows]))
            if pattern == 'zero_dlog':
                assert all(torch.equal(o[k], d[k + '0']) for k in ('dWp', 'dbp', 'dWl', 'dbl'))
                assert torch.equal(o['dhidden'][:, 0], prev0 if beta else torch.zeros_like(prev0))
        if pattern == 'saturated':
            assert not sep['dpooled'][c['sat_rows']].eq(0).all()          # (dpre is 0 through 1 - p^2, not through dpooled)


@pytest.mark.parametrize('shape', R.PATTERN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_a_saturated_sample_adds_exactly_nothing_to_the_pooler_gradients(shape):
    """dpre == 0 on every unit of the saturated samples: dWp and dbp keep their bits when those samples' hidden row 0 changes"""
    c, _ = _case(shape, 'saturated')
    d = _dev(c)
    other = d['hidden'].clone()
    other[c['sat_rows'], 0] = other[c['sat_rows'], 0] * -3.0 + 1.0
    ticket = _ticket()
    for run in (run_separate, lambda d_, beta, **kw: run_fused(d_, ticket, beta, **kw)):
        a, b = run(d, 0), run(d, 0, bwd_hidden=other)
        assert torch.equal(a['pooled'], b['pooled'])
        assert torch.equal(a['dWp'], b['dWp']) and torch.equal(a['dbp'], b['dbp']) and torch.equal(a['dhidden'], b['dhidden'])
        assert not torch.equal(a['dWp'], d['dWp0']) or len(c['sat_rows']) == shape[0]     # (the live samples did add)


@pytest.mark.parametrize('shape', R.PATTERN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_only_row_zero_of_hidden_is_read(shape):
    """NaN in rows 1 .. L-1 against the random values the case holds there: every result unchanged, bit for bit"""
    c, _ = _case(shape, 'randn')
    d = _dev(c)
    ticket = _ticket()
    for beta in (0, 1):
        for a, b in ((run_separate(d, beta), run_separate(d, beta, hidden=d['hidden_live'])),
                     (run_fused(d, ticket, beta), run_fused(d, ticket, beta, hidden=d['hidden_live']))):
            for k in OUTPUTS:
                assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), (shape, beta, k)


# ---------------------------------------------------------------------------------------------------------------------------
# optional outputs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.PATTERN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_optional_outputs_may_be_null(shape):
    c, _ = _case(shape, 'randn')
    d = _dev(c)
    B, L, H, Cn = shape
    ticket = _ticket()
    full = run_fused(d, ticket, 0)
    part = run_fused(d, ticket, 0, with_dhidden=False)                       # nX = 0: the X role has no workgroups
    for k in ('dWp', 'dbp', 'dWl', 'dbl'):
        assert torch.equal(full[k], part[k]), ('pool_head_bwd without dhidden', k)
    sep = run_separate(d, 0)
    dWp, dbp = d['dWp0'].clone(), d['dbp0'].clone()
    _call('uniter_pooler_bwd', sep['dpooled'], sep['pooled'], d['hidden'], d['Wp'], dWp, dbp, None, B, L, H, 0)
    assert torch.equal(dWp, sep['dWp']) and torch.equal(dbp, sep['dbp'])
    # linear_small_bwd: dx | dW | db in one buffer behind each other, so that a store through a NULL argument's neighbour shows
    n = (B * H, Cn * H, Cn)
    for skip in (None, 0, 1, 2):
        flat = _sentinel((sum(n) + 64,))
        parts = [flat[sum(n[:i]):sum(n[:i + 1])] for i in range(3)]
        parts[1].copy_(d['dWl0'].reshape(-1))
        parts[2].copy_(d['dbl0'])
        init = flat.clone()
        args = [None if i == skip else p for i, p in enumerate(parts)]
        _call('uniter_linear_small_bwd', d['dlog'], sep['pooled'], d['Wl'], *args, B, H, Cn)
        for i, (p, ref) in enumerate(zip(parts, (sep['dpooled'], sep['dWl'], sep['dbl']))):
            if i == skip:
                assert torch.equal(_bits(p), _bits(init[sum(n[:i]):sum(n[:i + 1])])), (skip, 'the NULL output was written')
            else:
                assert torch.equal(p, ref.reshape(-1)), (skip, i)
        assert bool((_bits(flat[sum(n):]) == SENT_BITS).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the ticket
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_ticket_buffer_serves_every_grid_in_sequence():
    """total = 1, 2, 15 (fewer workgroups than counter groups) ... 2048: the counters are zero after every launch and the last
    workgroup's logits within bound"""
    ticket = _ticket()
    for shape in R.SHAPES:
        c, _ = _case(shape, 'randn')
        B, L, H, Cn = shape
        hidden, Wp, bp, Wl, bl = (torch.from_numpy(c[k]).cuda() for k in ('hidden', 'Wp', 'bp', 'Wl', 'bl'))
        pooled, logits = _nan(B, H), _nan(B, Cn)
        _call('uniter_pool_head_fwd', hidden, Wp, bp, Wl, bl, pooled, logits, ticket, B, L, H, Cn)
        torch.cuda.synchronize()
        assert int(ticket.abs().sum()) == 0, shape
        assert torch.isfinite(pooled).all() and torch.isfinite(logits).all(), shape
        _hold('ticket.logits', logits, *R.ref_linear_fwd(pooled.cpu().numpy(), c['Wl'], c['bl']), what='%s, %d workgroups' % (shape, R.workgroups(shape)))


def test_back_to_back_launches_read_their_own_pooled_rows():
    """two input sets alternate for 32 launches on one stream through ONE pooled buffer and ONE ticket, no host synchronisation in
    between, each launch into its own logits slot: a last workgroup that read a stale pooled value (the previous launch's) would
    give the other set's logits.  Every slot equals the first slot of its set bit for bit."""
    shape = (16, 3, 768, 1)
    B, L, H, Cn = shape
    sets = []
    for seed in (0, 1):
        c = R.head_case(shape, 'randn', seed) if seed else _case(shape, 'randn')[0]
        sets.append([torch.from_numpy(c[k]).cuda() for k in ('hidden', 'Wp', 'bp', 'Wl', 'bl')])
    N = 32
    ticket, pooled, slots = _ticket(), _nan(B, H), _nan(N, B, Cn)
    torch.cuda.synchronize()
    for i in range(N):
        _call('uniter_pool_head_fwd', *sets[i % 2], pooled, slots[i], ticket, B, L, H, Cn)
    torch.cuda.synchronize()
    assert int(ticket.abs().sum()) == 0 and torch.isfinite(slots).all()
    assert not torch.equal(slots[0], slots[1])
    for i in range(N):
        assert torch.equal(slots[i], slots[i % 2]), i
    # and the first slots are right: against the separate launches
    for s in range(2):
        p, y = _nan(B, H), _nan(B, Cn)
        _call('uniter_pooler_fwd', sets[s][0], sets[s][1], sets[s][2], p, B, L, H)
        _call('uniter_linear_small_fwd', p, sets[s][3], sets[s][4], y, B, H, Cn)
        assert torch.equal(slots[s], y)


# ---------------------------------------------------------------------------------------------------------------------------
# the model's dispatch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_classes,fused', [(16, True), (17, False)])
def test_pool_head_dispatch_through_the_model(n_classes, fused, monkeypatch):
    """pool_head (model.py): up to 16 classes take the fused launch, 17 the separate modules; both within the float64 bound"""
    from common import TINY, TINY_IMG_DIM
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.trainer import TrainStep
    from meme_challenge_amd.utils import make_synthetic_batch
    monkeypatch.delenv('UNITER_FUSED_HEAD', raising=False)
    cfg = UniterConfig.from_dict(TINY)
    torch.manual_seed(5)
    model = MemeUniter(UniterModel(cfg, img_dim=TINY_IMG_DIM), cfg.hidden_size, n_classes).cuda()
    model.eval()
    batch = make_synthetic_batch(4, 12, 5, seed=2, vocab=TINY['vocab_size'], img_dim=TINY_IMG_DIM, device='cuda')
    seen = []
    hook = model.uniter_model.register_forward_hook(lambda m, a, out: seen.append(out.detach()))
    logits = model(**TrainStep.forward_kwargs(batch))
    hook.remove()
    torch.cuda.synchronize()
    node = type(logits.grad_fn).__name__
    if fused:
        assert node == '_PoolHeadFnBackward', node
    else:
        assert node == '_LinearSmallFnBackward', node
        assert '_PoolerFnBackward' in [type(f).__name__ for f, _ in logits.grad_fn.next_functions if f is not None]
    hidden = seen[0].cpu().numpy()
    Wp, bp = (t.detach().cpu().numpy() for t in (model.uniter_model.pooler.dense.weight, model.uniter_model.pooler.dense.bias))
    Wl, bl = (t.detach().cpu().numpy() for t in (model.linear.weight, model.linear.bias))
    fwd = R.ref_pooler_fwd(hidden, Wp, bp)
    lg, E_lg = R.ref_linear_fwd(fwd['pooled'], Wl, bl)
    # (the pooled rows stay inside the node: their bound reaches the logits through |Wl|)
    _hold('model.logits[%d]' % n_classes, logits, lg, E_lg + fwd['E_pooled'] @ np.abs(Wl.astype(np.float64)).T)
    assert logits.shape == (4, n_classes)
