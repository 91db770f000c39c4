"""The order-fixed embedding backward without a GPU: the rank / segment / chunk bookkeeping restated in numpy
(tests/embed_det_ref.py), the ctypes signatures of the new entry points against the built library, and the workspace size."""
import ctypes as C

import numpy as np
import pytest

import embed_det_ref as R


def _key_sets():
    g = np.random.default_rng(5)
    n = 3 * R.CHUNK + 7
    return {
        'random': g.integers(0, 50, 300),
        'one key': np.full(n, 23),                                               # one segment over four chunks
        'two keys': (np.arange(200) % 3 == 0).astype(np.int64),                  # the token-type table
        'positions': np.tile(np.arange(40), 5),                                  # every key five times, rows far apart
        'padding': np.concatenate([np.zeros(70, dtype=np.int64), g.integers(0, 9, 60)]),
        'sorted already': np.repeat(np.arange(5), R.CHUNK),                      # segments end exactly at chunk borders
        'single': np.array([4]),
        'out of range': R.keys_of(np.array([-5, 1 << 40, 49, 50, 0, -1, 7]), 50),
    }


@pytest.mark.parametrize('name', list(_key_sets()))
def test_rank_is_a_stable_sort_and_chunks_respect_keys(name):
    keys = np.asarray(_key_sets()[name])
    n = len(keys)
    rank = R.stable_rank(keys)
    assert sorted(rank.tolist()) == list(range(n))                               # a permutation: one writer per slot
    order = np.empty(n, dtype=np.int64)
    order[rank] = np.arange(n)
    assert np.array_equal(order, np.argsort(keys, kind='stable'))                # stability: equal keys keep ascending row index
    skip = 0 if name == 'padding' else -1
    rs = R.runs(keys)
    # every row in exactly one run, and every run inside one chunk and one key
    seen = sorted(r for run in rs for r in run['rows'])
    assert seen == list(range(n))
    for run in rs:
        assert len(run['rows']) <= R.CHUNK and run['rows'] == sorted(run['rows'])
        assert all(keys[r] == run['key'] for r in run['rows'])
        assert all(rank[r] // R.CHUNK == run['chunk'] for r in run['rows'])
    # at most one piece per (chunk, slot): the two piece slots of a chunk are never written twice
    slots = [(run['chunk'], run['slot']) for run in rs if run['slot'] is not None]
    assert len(slots) == len(set(slots))
    # one owner per key; it sees every row of the key once, in ascending row index overall; the skipped key has none
    own = R.owners(keys, skip)
    assert set(own) == set(keys.tolist()) - {skip}
    for key, (chunk, runs_) in own.items():
        rows = [r for run in runs_ for r in run['rows']]
        assert rows == np.flatnonzero(keys == key).tolist()
        assert chunk == runs_[0]['chunk'] and [run['chunk'] for run in runs_] == list(range(chunk, chunk + len(runs_)))
    if skip == 0:
        assert all(keys[r] != 0 for _, runs_ in own.values() for run in runs_ for r in run['rows'])


def test_keys_follow_the_forward_clamp_and_broadcast():
    assert R.keys_of([-5, 1 << 40, 49, 50, 0], 50).tolist() == [0, 49, 49, 49, 0]
    assert R.keys_of([3, 1, 2], 40, rows=7, bcast_T=3).tolist() == [3, 1, 2, 3, 1, 2, 3]


def test_scatter_sum_in_kernel_order_is_the_plain_sum():
    g = np.random.default_rng(2)
    keys = g.integers(0, 6, 150)
    d = g.standard_normal((150, 8))
    got = R.scatter_sum(keys, d, 6, skip=0, dtype=np.float64)
    ref = np.zeros((6, 8))
    np.add.at(ref, keys, d)
    ref[0] = 0
    assert np.allclose(got, ref, rtol=0, atol=1e-12)


def test_new_entry_points_resolve_with_their_twins_signatures():
    from meme_challenge_amd import _lib
    lib = _lib.lib()

    for det, twin in (('uniter_txt_embed_bwd_det', 'uniter_txt_embed_bwd'), ('uniter_img_embed_bwd_det', 'uniter_img_embed_bwd')):
        f, t = getattr(lib, det), getattr(lib, twin)
        assert f.restype == t.restype == C.c_int and list(f.argtypes) == list(t.argtypes)
    assert lib.uniter_embed_bwd_det_ws_bytes.restype == C.c_size_t and len(lib.uniter_embed_bwd_det_ws_bytes.argtypes) == 3
    assert lib.uniter_model_set_deterministic.restype == C.c_int and len(lib.uniter_model_set_deterministic.argtypes) == 2
    assert lib.uniter_model_set_deterministic(None, 1) != 0 and b'set_deterministic' in lib.uniter_last_error()



def test_workspace_size_is_monotone_aligned_and_covers_the_atomic_path():
    from meme_challenge_amd import _lib
    ws = _lib.lib().uniter_embed_bwd_det_ws_bytes
    old = _lib.lib().uniter_embed_bwd_ws_bytes
    assert ws(0, 0, 768) == 0
    for H in (128, 768, 1024):
        prev = 0
        for rows in (1, 3, 31, 32, 33, 255, 256, 257, 1000, 2048, 4096, R.MAX_ROWS):
            t, i, both = ws(rows, 0, H), ws(0, rows, H), ws(rows, rows, H)
            assert t % 16 == 0 and i % 16 == 0
            assert both == max(t, i) and t >= prev                               # enough for either call; grows with the rows
            # the column partials (uniter_embed_bwd_ws_bytes counts the image pass's 7 columns; the text pass has 3) + per-row gradients
            assert t >= old(rows, H) * 3 // 7 + rows * H * 4 and i >= old(rows, H) + rows * H * 4
            prev = t
        assert ws(64, 0, H) <= ws(64, 100, H) and ws(0, 64, H) <= ws(100, 64, H)
    assert ws(100, 0, 128) < ws(100, 0, 768) < ws(100, 0, 1024)


def test_model_property_defaults_off_and_needs_no_handle():
    from meme_challenge_amd.model import UniterConfig, UniterModel
    import common
    m = UniterModel(UniterConfig.from_dict(common.TINY), img_dim=common.TINY_IMG_DIM)
    assert m.deterministic is False
    m.deterministic = 1
    assert m.deterministic is True
    m.deterministic = False
    assert m.deterministic is False
