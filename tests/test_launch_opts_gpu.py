"""Launch options are arguments of the launch that uses them (csrc/common.h: LaunchOpts), not state a model call leaves behind on
its host thread: what a model handle did earlier decides nothing about a later direct call or query of the C ABI."""
import ctypes as C

import pytest
import torch

from common import TINY, TINY_IMG_DIM, sd_from_npz, batch_from_npz, model_kwargs

pytestmark = pytest.mark.gpu


def _tiny_x3(tiny):
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    cfg = UniterConfig.from_dict(TINY)
    m = MemeUniter(UniterModel(cfg, img_dim=TINY_IMG_DIM), cfg.hidden_size, 1)
    m.load_state_dict(sd_from_npz(tiny), strict=True)
    m.uniter_model.precision = 'fp32x3'
    m = m.cuda().train()
    m.param_store()
    b = {k: v.cuda() for k, v in batch_from_npz(tiny).items()}
    return m.uniter_model, model_kwargs(b)


def _forward(enc, kw, reserve):
    enc.cu_reserve = reserve
    return enc(**kw)


def _backward_on_this_thread(hidden):
    """The encoder's backward pass on the CALLING thread: loss.backward() would run it on the autograd engine's device thread."""
    hidden.grad_fn.apply(torch.ones_like(hidden))
    torch.cuda.synchronize()


def _chip_queries():
    """Three host-only queries of the C ABI whose answer is a grid: far more tiles than CUs (4 products of 4096 x 4096), so the
    grid is the cap and 16 CUs less would change it; they allocate nothing."""
    from meme_challenge_amd import _lib
    lib = _lib.lib()
    IA = C.c_int * 4
    M, N = IA(*[4096] * 4), IA(*[4096] * 4)
    x3 = lib.uniter_wgrad_x3_group_slots(0, 4, M, N, 0)
    b16 = lib.uniter_wgrad_bf16_group_slots(4, M, N, 0)
    cfg, ns = C.c_int(0), C.c_int(0)
    _lib.check(lib.uniter_gemm_x3_plan(2624, 768, 3072, 0, 0, C.byref(cfg), C.byref(ns)), 'uniter_gemm_x3_plan')
    return x3, b16, (cfg.value, ns.value)


def test_a_models_cu_reserve_ends_with_the_model_call(tiny):
    """uniter_model_set_cu_reserve is the model's: after a forward + backward pass with 16 CUs reserved -- on this thread -- the
    public slot and plan queries answer for the whole chip, as before it."""
    enc, kw = _tiny_x3(tiny)
    before = _chip_queries()
    print('before:', before)
    assert before[0] > 0 and before[1] > 0
    _backward_on_this_thread(_forward(enc, kw, 16))
    after = _chip_queries()
    print('after: ', after)
    assert after == before


def test_riders_slot_count_is_what_the_trainer_sees_today(tiny):
    """uniter_model_norm_partials_per_layer announces the reserve-0 count, whatever ran before on the handle: the same after a
    forward and after a backward pass, with no CUs reserved and with 16."""
    enc, kw = _tiny_x3(tiny)
    counts = []
    for reserve in (0, 16):
        hidden = _forward(enc, kw, reserve)
        counts.append(enc.norm_partials_per_layer())
        _backward_on_this_thread(hidden)
        counts.append(enc.norm_partials_per_layer())
    print('slots per layer:', counts)
    assert counts[0] == counts[1] == counts[2] == counts[3]
