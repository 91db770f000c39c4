"""CPU: uniter_model_set_head_rows refuses a null handle before any HIP call, and the Python side's one-shot request never outlives
the call that set it."""
import pytest
import torch


def test_set_head_rows_refuses_a_null_handle():
    from meme_challenge_amd import _lib
    lib = _lib.lib()
    for on in (0, 1):
        assert lib.uniter_model_set_head_rows(None, on) == -1          # UNITER_E_ARG
        assert b'set_head_rows' in lib.uniter_last_error()


def test_request_is_dropped_when_the_encoder_call_is_refused():
    """MemeUniter.forward sets the one-shot on the encoder module; a call that raises before it reaches the library (here: no inputs
    at all) must not leave it behind for a later direct call of the encoder, whose caller reads every row"""
    from common import TINY, TINY_IMG_DIM
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.meme_uniter import MemeUniter
    cfg = UniterConfig.from_dict(TINY)
    m = MemeUniter(UniterModel(cfg, img_dim=TINY_IMG_DIM), cfg.hidden_size, 1)
    assert m.head_rows_only is True
    with pytest.raises(Exception):
        m(input_ids=None, position_ids=None, img_feat=None, img_pos_feat=None, attention_mask=torch.ones(1, 4), gather_index=None)
    assert '_head_rows_next' not in m.uniter_model.__dict__
