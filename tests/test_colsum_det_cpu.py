"""The order of the order-fixed column sums, restated in numpy float32 (tests/colsum_det_ref.py): it agrees with a float64 sum within
the bound of a sum of that depth, it IS an order (a constructed input tells it from every other block order), it handles a ragged
last block -- and the trainer's --deterministic flag reaches UniterModel.deterministic.  No GPU."""
import itertools

import numpy as np
import pytest

import colsum_det_ref as R


def _data(rows, cols, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((rows, cols)).astype(np.float32) * np.float32(3.0)


@pytest.mark.parametrize('rows,cols', [(197, 8), (64, 16), (1, 8), (300, 24), (8, 8)])
def test_agrees_with_float64_within_the_bound_of_the_sum(rows, cols):
    """|result - float64 sum| <= rows * 2^-24 * sum |x| per column (prior out = 0: the final add is then exact).  Every value passes
    through at most rows roundings of relative size 2^-24 -- far fewer, in fact: 16 + 2 inside a block, then one per block"""
    x = _data(rows, cols, rows)
    xb = R.to_bf16(x)
    got = R.colsum_bf16_add_det(xb, np.zeros(cols, np.float32))
    assert got.dtype == np.float32
    bound = rows * 2.0 ** -24 * np.abs(xb.astype(np.float64)).sum(0)
    assert (np.abs(got.astype(np.float64) - xb.astype(np.float64).sum(0)) <= bound).all()
    p = R.split3(x)
    got3 = R.colsum_x3_add_det(p, np.zeros(cols, np.float32))
    exact = p.astype(np.float64).sum(1)                 # the values the pieces stand for
    bound3 = rows * 2.0 ** -24 * np.abs(exact).sum(0)
    assert (np.abs(got3.astype(np.float64) - exact.sum(0)) <= bound3).all()
    # three pieces carry a float32 value to within 2^-24 relative (its last bit or two may need a fourth piece)
    assert (np.abs(exact - x.astype(np.float64)) <= 2.0 ** -24 * np.abs(x)).all()


def test_helpers_round_to_bf16():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, -2.0 ** 24, 0.0, 2.0 ** -130], dtype=np.float32)
    b = R.to_bf16(x)
    assert (b.view(np.uint32) & 0xffff == 0).all()
    assert b[0] == 1.0 and b[1] == 1.0 and b[2] == np.float32(1.0 + 2.0 ** -7) and b[3] == -2.0 ** 24      # ties to even, both ways


def test_the_stated_order_is_told_from_every_other_block_order():
    x, out = R.constructed()
    assert (R.to_bf16(x) == x).all()
    p = R.split3(x)
    assert (p[:, 0] == x).all() and not p[:, 1:].any()                    # exact as x3 pieces
    for got in (R.colsum_bf16_add_det(x, out), R.colsum_x3_add_det(p, out)):
        assert got[3] == np.float32(1.5)                                  # ((2^24 + 1) - 2^24) + 1 = 1, on 0.5
        assert (np.delete(got, 3) == np.float32(0.5)).all()
    assert out[3] + x.astype(np.float64).sum(0)[3] == 2.5                 # the exact sum
    seen = set()
    for order in itertools.permutations(range(4)):
        v = float(R.colsum_bf16_add_det(x, out, order=order)[3])
        seen.add(v)
        if order != (0, 1, 2, 3):
            assert v in (0.5, 1.5, 2.5)
    assert seen == {0.5, 1.5, 2.5}
    # an order that pairs the two large values first is exact; one that adds both units to 2^24 loses both
    assert float(R.colsum_bf16_add_det(x, out, order=(0, 2, 1, 3))[3]) == 2.5
    assert float(R.colsum_bf16_add_det(x, out, order=(0, 1, 3, 2))[3]) == 0.5
    # (one value per block: the block partials are the values themselves)
    assert (R.block_partials(x)[:, 3] == np.array([2.0 ** 24, 1.0, -2.0 ** 24, 1.0], np.float32)).all()


def test_ragged_last_block_and_row_lanes():
    """197 rows: three full blocks and one of 5 rows (lanes 0..3 get 2, 1, 1, 1 rows); the partials follow the stated lane order"""
    x = R.to_bf16(_data(197, 8, 7))
    P = R.block_partials(x)
    assert P.shape == (4, 8)
    last = x[192:]
    s = [last[0] + last[4], last[1], last[2], last[3]]
    assert (P[3] == (s[0] + s[1]) + (s[2] + s[3])).all()
    blk = x[64:128]
    lanes = []
    for w in range(4):
        a = np.zeros(8, np.float32)
        for r in range(w, 64, 4):
            a = a + blk[r]
        lanes.append(a)
    assert (P[1] == (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])).all()
    out = np.float32(0.25) * np.ones(8, np.float32)
    assert (R.colsum_bf16_add_det(x, out) == out + (((P[0] + P[1]) + P[2]) + P[3])).all()
    # one row: the value itself, added to out once
    one = R.to_bf16(_data(1, 8, 9))
    assert (R.colsum_bf16_add_det(one, out) == out + one[0]).all()


def test_deterministic_flag_reaches_the_models_property():
    """--deterministic is a store_true flag of the trainer's default arguments; TrainerUniter applies it to the encoder object (the
    library handle is created lazily, so this needs no GPU)"""
    import train_uniter
    from common import TINY, TINY_IMG_DIM
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.model import UniterConfig, UniterModel
    from meme_challenge_amd.train_template import TrainerTemplate
    assert ('deterministic', None, False) in TrainerTemplate.FLAGS
    parser = train_uniter.build_parser()
    assert parser.parse_known_args([])[0].deterministic is False
    for argv, want in (([], False), (['--deterministic'], True)):
        args, _ = parser.parse_known_args(argv + ['--precision', 'fp32'])
        t = object.__new__(train_uniter.TrainerUniter)
        t.config = dict(vars(args))
        t.model = MemeUniter(UniterModel(UniterConfig.from_dict(TINY), img_dim=TINY_IMG_DIM), TINY['hidden_size'], 1)
        assert t.model.uniter_model.deterministic is False
        t._apply_runtime_options()
        enc = t.model.uniter_model
        assert enc.deterministic is want and enc.precision == 'fp32'
        assert enc.deterministic_coverage == 0 and enc.bit_reproducible is False and enc._handle is None      # no forward pass yet
        assert enc.DET_ALL == 15 and enc.DET_EMBED | enc.DET_ATTN | enc.DET_COLSUM | enc.DET_GEMM == 15
