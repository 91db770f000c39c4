"""uniter_collate_batch (csrc/collate.hip) through data.collate_batch against the numpy restatement tests/collate_ref.py, bit for bit
(torch.equal: the kernel copies values and does integer arithmetic).  Every output lies inside a larger buffer, pre-filled with a
sentinel byte between two guard bands: afterwards no sentinel is left inside the extent and every guard byte is unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from collate_guard import Guarded, sentinel_of, to_device
from collate_ref import collate_ref
from meme_challenge_amd import _lib
from meme_challenge_amd.data import collate_batch

pytestmark = pytest.mark.gpu

OUT_KEYS = ('img_feat', 'img_pos_feat', 'input_ids', 'position_ids', 'token_type_ids', 'attn_mask', 'gather_index', 'labels', 'ids')
ARRAY_KEYS = ('feat', 'pos', 'row_start', 'row_cnt', 'input_ids', 'token_type_ids', 'txt_len', 'labels', 'ids')


def synth(D, R, T, token_types, seed=0):
    """Six samples with region counts R, 0, 1, R, min(2, R), 1 and text lengths in {1, T}; their pool rows lie far apart and
    out of order (row_start is not monotonic), with rows nobody owns between them."""
    rng = np.random.default_rng(seed)
    cnt = np.array([R, 0, 1, R, min(2, R), 1], np.int32)
    txt = np.array([T, 1, T, 1, T, 1], np.int32)
    N = len(cnt)
    place = [3, 5, 0, 4, 2, 1]                      # pool order of the samples
    row_start, at = np.zeros(N, np.int64), 3
    for s in place:
        row_start[s] = at
        at += int(cnt[s]) + 11
    assert np.any(np.diff(row_start) < 0)
    rows = at
    a = {'feat': rng.standard_normal((rows, D)).astype(np.float32), 'pos': rng.random((rows, 7)).astype(np.float32),
         'row_start': row_start, 'row_cnt': cnt, 'input_ids': rng.integers(1, 28996, (N, T)).astype(np.int64),
         'token_type_ids': rng.integers(0, 2, (N, T)).astype(np.int64) if token_types else None, 'txt_len': txt,
         'labels': rng.integers(0, 2, N).astype(np.int64), 'ids': rng.integers(0, 99999, N).astype(np.int64)}
    return a


def guarded_outputs(B, R, D, T, L_out, token_types):
    shapes = {'img_feat': ((B, R, D), torch.float32), 'img_pos_feat': ((B, R, 7), torch.float32), 'input_ids': ((B, T), torch.int64),
              'position_ids': ((B, T), torch.int64), 'token_type_ids': ((B, T), torch.int64), 'attn_mask': ((B, L_out), torch.float32),
              'gather_index': ((B, L_out), torch.int64), 'labels': ((B,), torch.int64), 'ids': ((B,), torch.int64)}
    return {k: Guarded(s, dt) for k, (s, dt) in shapes.items() if token_types or k != 'token_type_ids'}


def run_and_check(a, d, sel, R, ragged):
    T, D = a['input_ids'].shape[1], a['feat'].shape[1]
    il = a['row_cnt'][sel] if ragged else R
    L_out = int((a['txt_len'][sel] + il).max())
    want = collate_ref(sel, *[a[k] for k in ARRAY_KEYS], R=R, L_out=L_out, ragged=ragged)
    g = guarded_outputs(len(sel), R, D, T, L_out, a['token_type_ids'] is not None)
    out = {k: (g[k].t if k in g else None) for k in OUT_KEYS}
    got = collate_batch(torch.tensor(sel, dtype=torch.int64, device='cuda'), *[d[k] for k in ARRAY_KEYS], R=R, L_out=L_out,
                        ragged_regions=ragged, out=out)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        what = '%s (sel %s, R %d)' % (k, sel, R)
        if want[k] is None:
            assert got[k] is None, what
            continue
        g[k].check_guards(what)
        t = got[k].cpu()
        assert not bool((t == sentinel_of(t.dtype)).any()), '%s: a sentinel is left inside the extent' % what
        assert torch.equal(t, torch.from_numpy(want[k])), what


@pytest.mark.parametrize('token_types', [True, False])
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('T', [1, 16])
@pytest.mark.parametrize('R', [1, 5, 37])
@pytest.mark.parametrize('D', [4, 260, 2048])
def test_collate_batch_equals_the_reference(D, R, T, ragged, token_types):
    """D: one 16-byte item per row, one more than a wave's 64, the model's.  R: no multiple of the four items of a workgroup.
    Batches: region counts {R, 0, 1} together; B = 1 with R, 1 and 0 regions (the last with R = 0 as well: no region items at
    all); an unsorted selection holding one sample twice."""
    a = synth(D, R, T, token_types, seed=D + R + T)
    d = to_device(a)
    for sel, r in (([0, 1, 2], R), ([3], R), ([2], R), ([1], R), ([1], 0), ([4, 2, 4, 0, 5], R)):
        run_and_check(a, d, sel, r, ragged)


def test_a_pool_beyond_2_to_the_31_elements():
    """D = 2048 and 2^20 + 16 rows: the last sample's rows start past element 2^31.  The pool is torch.empty; only the rows of the
    two samples are written."""
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip('needs 16 GB of free device memory for an 8.6-GB pool; %.1f GB are free' % (free / 2.0 ** 30))
    D, rows, T = 2048, (1 << 20) + 16, 4
    assert (rows - 3) * D > 1 << 31
    rng = np.random.default_rng(5)
    a = {'row_start': np.array([rows - 3, 0], np.int64), 'row_cnt': np.array([3, 2], np.int32),
         'input_ids': rng.integers(1, 999, (2, T)).astype(np.int64), 'token_type_ids': None, 'txt_len': np.array([4, 2], np.int32),
         'labels': np.array([1, 0], np.int64), 'ids': np.array([17, 4], np.int64)}
    head, tail = rng.standard_normal((2, D)).astype(np.float32), rng.standard_normal((3, D)).astype(np.float32)
    phead, ptail = rng.random((2, 7)).astype(np.float32), rng.random((3, 7)).astype(np.float32)
    d = to_device({k: v for k, v in a.items()})
    d['feat'] = torch.empty((rows, D), dtype=torch.float32, device='cuda')
    d['pos'] = torch.empty((rows, 7), dtype=torch.float32, device='cuda')
    d['feat'][:2], d['feat'][rows - 3:] = torch.from_numpy(head).cuda(), torch.from_numpy(tail).cuda()
    d['pos'][:2], d['pos'][rows - 3:] = torch.from_numpy(phead).cuda(), torch.from_numpy(ptail).cuda()
    got = collate_batch(torch.tensor([1, 0], device='cuda'), *[d[k] for k in ARRAY_KEYS], R=3, L_out=7, ragged_regions=True)
    torch.cuda.synchronize()
    # the reference on a pool that holds the same five rows close together
    small = dict(a, feat=np.concatenate([head, tail]), pos=np.concatenate([phead, ptail]), row_start=np.array([2, 0], np.int64))
    want = collate_ref([1, 0], *[small[k] for k in ARRAY_KEYS], R=3, L_out=7, ragged=True)
    for k in OUT_KEYS:
        if want[k] is not None:
            assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    assert got['token_type_ids'] is None
    del d, got
    torch.cuda.empty_cache()


# ---- refusals: an error code, a message, nothing launched ------------------------------------------------------------
def raw_call(d, sel, outs, B, R, L_out, D=None, T=None, feat_ptr=None, drop=(), ds_null=False, sel_null=False):
    """the C call itself; drop: 'ds.<field>' / 'out.<name>' pointers passed as NULL"""
    p = lambda t: None if t is None else t.data_ptr()
    f = {k: (None if 'ds.' + k in drop else p(d[k])) for k in ARRAY_KEYS}
    if feat_ptr is not None:
        f['feat'] = feat_ptr
    ds = _lib.UniterDatasetC(f['feat'], f['pos'], f['row_start'], f['row_cnt'], f['input_ids'], f['token_type_ids'], f['txt_len'],
                             f['labels'], f['ids'], d['row_start'].shape[0], d['feat'].shape[0],
                             d['feat'].shape[1] if D is None else D, d['input_ids'].shape[1] if T is None else T)
    o = [None if 'out.' + k in drop else C.c_void_p(outs[k].t.data_ptr()) for k in OUT_KEYS]
    return _lib.lib().uniter_collate_batch(None if ds_null else C.byref(ds), None if sel_null else C.c_void_p(sel.data_ptr()),
                                           B, R, L_out, 0, *o, _lib.cur_stream())


def test_refusals_return_their_codes_and_write_nothing():
    D, R, T, B = 8, 5, 16, 3
    a = synth(D, R, T, True)
    d = to_device(a)
    sel = torch.tensor([0, 1, 2], device='cuda')
    L_out = T + R
    outs = guarded_outputs(B, R, D, T, L_out, True)
    E_ARG, E_SHAPE = -1, -2
    cases = [('a NULL dataset', E_ARG, dict(ds_null=True)), ('a NULL selection', E_ARG, dict(sel_null=True))]
    cases += [('dataset pointer %s NULL' % k, E_ARG, dict(drop=('ds.' + k,))) for k in ARRAY_KEYS if k != 'token_type_ids']
    cases += [('output %s NULL' % k, E_ARG, dict(drop=('out.' + k,))) for k in OUT_KEYS if k != 'token_type_ids']
    cases += [('D % 4 != 0', E_SHAPE, dict(D=6)), ('a misaligned feat', E_ARG, dict(feat_ptr=d['feat'].data_ptr() + 4)),
              ('B = 0', E_SHAPE, dict(B=0)), ('B < 0', E_SHAPE, dict(B=-1)), ('T = 0', E_SHAPE, dict(T=0)),
              ('L_out = 0', E_SHAPE, dict(L_out=0)), ('L_out > T + R', E_SHAPE, dict(L_out=T + R + 1))]
    lib = _lib.lib()
    for what, code, kw in cases:
        rc = raw_call(d, sel, outs, **dict(dict(B=B, R=R, L_out=L_out), **kw))
        assert rc == code, '%s: rc %d' % (what, rc)
        assert b'collate_batch' in lib.uniter_last_error(), what
    torch.cuda.synchronize()
    for k, g in outs.items():
        assert g.untouched(), '%s was written by a refused call' % k
        g.check_guards(k)
    # the wrapper refuses what is not a GPU tensor of the right type itself
    with pytest.raises(_lib.UniterHipError, match='must live on the GPU'):
        collate_batch(sel.cpu(), *[d[k] for k in ARRAY_KEYS], R=R, L_out=L_out)
    with pytest.raises(_lib.UniterHipError, match='row_cnt must be torch.int32'):
        collate_batch(sel, *[(d[k].long() if k == 'row_cnt' else d[k]) for k in ARRAY_KEYS], R=R, L_out=L_out)
    # and the valid call on the same buffers goes through
    assert raw_call(d, sel, outs, B, R, L_out) == 0
    torch.cuda.synchronize()
    assert not any(g.untouched() for g in outs.values())
