"""tests/poison.py on CPU tensors: the fill is applied, the tensor is what torch.empty would have returned but for its bytes, an
out-of-window write is reported, and the patch is gone after exit.  No GPU, no library call."""
import struct

import pytest
import torch
from torch import nn

import poison
from poison import BAND, GUARD, GuardBandError, Poison


def _model_module():
    import meme_challenge_amd.model as M
    return M


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.int64, torch.uint8])
def test_fills_are_applied(dtype):
    M = _model_module()
    with Poison('zeros', capture=True) as z:
        a = M.torch.empty(5, 7, dtype=dtype)
        assert not _bytes(a).any()
        a.view(-1)[:] = 3
    with Poison('ones') as o:
        b = M.torch.empty((5, 7), dtype=dtype)
        assert bool((_bytes(b) == 0xFF).all())
    with Poison('unit') as u:
        c = M.torch.empty(5, 7, dtype=dtype)
        want = torch.tensor(list(struct.pack('<f', 1.0)), dtype=torch.uint8).repeat(5 * 7 * 8 // 4 + 1)
        assert torch.equal(_bytes(c), want[:_bytes(c).numel()])
    with Poison('replay', replay=z.captured) as r:
        d = M.torch.empty(5, 7, dtype=dtype)            # another line of this function: a site the capture never saw -> 'unit'
        assert torch.equal(_bytes(d), _bytes(c))
    for p in (z, o, u, r):
        assert sum(p.sites.values()) == 1 and not p.broken
    if dtype == torch.float32:
        assert torch.isnan(b).all() and bool((c == 1.0).all())
    if dtype == torch.bfloat16:
        assert torch.isnan(b).all() and set(c.float().view(-1).tolist()) == {0.0, 1.0}
    if dtype == torch.int64:
        assert bool((b == -1).all())


def test_replay_returns_the_captured_bytes_site_by_site():
    M = _model_module()

    def alloc(n):
        return [M.torch.empty(n, dtype=torch.float32) for _ in range(2)]       # one call site, two allocations
    with Poison('zeros', capture=True) as first:
        for i, t in enumerate(alloc(6)):
            t.fill_(i + 2.5)
    with Poison('replay', replay=first.captured) as again:
        x, y = alloc(6)
        assert bool((x == 2.5).all()) and bool((y == 3.5).all())
        again.fill = 'replay'                                                   # a new pass: the ordinals start over
        big, = alloc(9)[:1]
        assert bool((big == 2.5).all())                                         # another size: repeated to fit
        small = alloc(2)[1]
        assert bool((small == 3.5).all())
    assert again.count('test_poison_cpu.py:<listcomp>') + again.count('test_poison_cpu.py:alloc') == 6
    with pytest.raises(ValueError):
        Poison('replay')


@pytest.mark.parametrize('shape,dtype', [((3, 5), torch.float32), ((), torch.float32), ((0, 4), torch.float32), ((33,), torch.uint8),
                                         ((2, 3, 4), torch.bfloat16), ((1,), torch.int32)])
def test_the_tensor_is_what_was_asked_for(shape, dtype):
    M = _model_module()
    src = torch.zeros(shape, dtype=dtype)
    with Poison('ones') as p:
        for t in (M.torch.empty(*shape, dtype=dtype) if shape else M.torch.empty((), dtype=dtype),
                  M.torch.empty(shape, dtype=dtype, device='cpu'), M.torch.empty_like(src),
                  M.torch.empty_like(src.float(), dtype=dtype)):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == 'cpu'
            assert t.is_contiguous() and t.data_ptr() % 256 == 0 and not t.requires_grad
        for src2 in (torch.zeros(4, 6).t(), torch.zeros(2, 3, 4).permute(2, 0, 1), torch.zeros(4, 6)[:, ::2]):
            t, want = M.torch.empty_like(src2), torch.empty_like(src2)          # strides as torch.empty_like chooses them
            assert t.shape == want.shape and t.stride() == want.stride() and t.data_ptr() % 256 == 0
            assert bool((_bytes(t) == 0xFF).all()) and _bytes(t).numel() == 4 * src2.numel()
        assert M.torch.empty(3).dtype == torch.get_default_dtype()
        assert M.torch.empty(3, requires_grad=True).requires_grad
    assert sum(p.sites.values()) == 9 and not p.passed_through and all(s.startswith('test_poison_cpu.py:test_the_tensor_is_what_was_asked_for:') for s in p.sites)


def test_guard_bands_surround_the_payload_and_a_write_outside_is_reported():
    M = _model_module()
    with Poison('zeros') as clean:
        t = M.torch.empty(10, dtype=torch.float32)
        t.fill_(7.0)                                                            # every byte of the window: nothing to report
    rec = clean.records[0]
    assert rec.nbytes == 40 and rec.band == BAND and rec.start % 256 == (-rec.base.data_ptr()) % 256
    assert all(bool((b == GUARD).all()) and b.numel() == BAND for b in rec.bands()) and not clean.broken
    for where, offset in (('back', 40), ('back', 40 + BAND - 1), ('front', -1), ('front', -BAND)):
        with pytest.raises(GuardBandError, match=where):
            with Poison('zeros') as p:
                t = M.torch.empty(10, dtype=torch.float32)
                r = p.records[0]
                r.base[r.start + offset] = 0                                    # the deliberate out-of-window write
        assert [(s.split(':')[1], side) for s, side, _ in p.broken] == [
            ('test_guard_bands_surround_the_payload_and_a_write_outside_is_reported', where)]
    # one element past the end through the tensor's own storage, as a kernel with a wrong bound would write it
    with Poison('ones', check=False) as q:
        t = M.torch.empty(10, dtype=torch.float32)
        torch.as_strided(t, (11,), (1,))[10] = 0.0
    assert len(q.broken) == 1 and q.broken[0][1:] == ('back', 0)


def test_the_model_workspace_has_wide_bands_and_ends_where_the_plan_ends():
    M = _model_module()

    class Stub(object):
        class embeddings(object):
            class LayerNorm(object):
                weight = torch.zeros(1)
        _ws_cache = {}
    stub = Stub()
    stub._ws_high = 1 << 20                                                     # an earlier, longer batch
    plain = M.UniterModel._get_ws(stub, 1000, 1)
    assert plain.numel() == 1 << 20
    with Poison('unit') as p:
        ws = M.UniterModel._get_ws(stub, 1000, 1)
        assert ws.numel() == 1000 - poison.WS_SLACK and ws.dtype == torch.uint8 and ws.data_ptr() % 256 == 0
        inf = M.UniterModel._get_ws(stub, 500, 0)
        assert inf.numel() == 500 - poison.WS_SLACK and M.UniterModel._get_ws(stub, 400, 0) is inf      # the inference block is cached as ever
    assert p.count('model.py:_get_ws') == 2 and [r.band for r in p.records] == [poison.BAND_WS] * 2
    assert p.records[0].nbytes == 1000 - poison.WS_SLACK


def test_a_call_the_harness_does_not_rebuild_is_recorded():
    """a keyword beyond dtype / device / requires_grad goes to torch as it is -- and is counted, so that the GPU tests can refuse it"""
    M = _model_module()
    with Poison('ones') as p:
        t = M.torch.empty(4, 3, memory_format=torch.contiguous_format)
        u = M.torch.empty_like(t, memory_format=torch.preserve_format)
    assert t.shape == u.shape == (4, 3) and not p.sites and sum(p.passed_through.values()) == 2
    assert all(s.startswith('test_poison_cpu.py:test_a_call_the_harness_does_not_rebuild_is_recorded:') for s in p.passed_through)


def test_parameters_can_be_built_inside():
    M = _model_module()
    with Poison('ones') as p:
        lin = M._ParamLinear(6, 4)
        head = M.HipLinear(6, 2)
        assert isinstance(lin.weight, nn.Parameter) and lin.weight.requires_grad and tuple(lin.weight.shape) == (4, 6)
        assert torch.isnan(lin.weight).all()                                    # poisoned until init_weights fills it
        assert torch.isfinite(head.weight).all() and torch.isfinite(head.bias).all()      # HipLinear initialises itself
        w = nn.Parameter(M.torch.empty(3, 3))
        w.data.normal_()
        (w * 2).sum().backward()
        assert torch.equal(w.grad, torch.full((3, 3), 2.0))
    assert p.count('model.py:__init__') == 3 and not p.broken
    assert 'model.py:__init__' in p.functions() and 'model.py:__init__:' in p.report()


def test_the_patch_is_scoped_to_the_package_and_gone_after_exit():
    import meme_challenge_amd.trainer as T
    M = _model_module()
    real_get_ws = M.UniterModel._get_ws
    assert M.torch is torch and T.torch is torch
    with Poison('ones') as p:
        assert M.torch is not torch and T.torch is M.torch
        assert M.torch.float32 is torch.float32 and M.torch.Tensor is torch.Tensor and M.torch.nn is nn
        assert M.UniterModel._get_ws is not real_get_ws
        mine = torch.empty(4)                                                   # this module's torch is the real one
        assert M.torch.empty is not torch.empty and M.torch.zeros is torch.zeros
    assert M.torch is torch and T.torch is torch and M.UniterModel._get_ws is real_get_ws
    assert sum(p.sites.values()) == 0 and mine.shape == (4,)
    with pytest.raises(RuntimeError):
        with Poison('zeros'):
            raise RuntimeError('the body failed')
    assert M.torch is torch and M.UniterModel._get_ws is real_get_ws           # ... also when the body raised
