"""Device-resident dataset, the parts that need no GPU: the numpy restatement of uniter_collate_batch equals the host collate it
must reproduce, the loader's host planning equals what that collate returns, and the refusals happen before any allocation."""
from functools import partial

import numpy as np
import pytest
import torch
from torch.utils import data

from collate_ref import arrays_of, collate_ref
from meme_challenge_amd.data import (DeviceFeaturePool, DeviceLoader, DeviceMemeDataset, HashTokenizer, MemeDataset, plan_batches,
                                     write_synthetic_dataset)

T = 12
TENSOR_KEYS = ('img_feat', 'img_pos_feat', 'input_ids', 'position_ids', 'token_type_ids', 'attn_mask', 'gather_index', 'labels', 'ids')


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('devds'))
    write_synthetic_dataset(d, n=13, num_bb=(2, 9), img_dim=16, seed=3, splits=('train',), text_words=(1, 9))
    return d


def dataset(root, ragged, **kw):
    tok = partial(HashTokenizer(max_length=T), max_length=T)
    return MemeDataset(root + '/train.jsonl', root + '/img_feats', text_padding=tok, return_ids=True, ragged_regions=ragged, **kw)


class NoTokenTypes(HashTokenizer):
    def __call__(self, texts, **kw):
        out = HashTokenizer.__call__(self, texts, **kw)
        del out['token_type_ids']
        return out


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('thr', [0.0, 0.45])
def test_collate_ref_equals_the_host_collate(root, ragged, thr):
    ds = dataset(root, ragged, confidence_threshold=thr)
    arrays = arrays_of(ds)
    row_cnt, txt_len = arrays[3], arrays[6]
    sel = [7, 2, 11, 2, 0]                       # unsorted, one sample twice
    assert len(set(row_cnt[sel])) > 1 and len(set(txt_len[sel])) > 1, 'the case needs different region counts and text lengths'
    want = ds.get_collate_fn()([ds[i] for i in sel])
    R, L_out = want['img_feat'].shape[1], want['attn_mask'].shape[1]
    got = collate_ref(sel, *arrays, R=R, L_out=L_out, ragged=ragged)
    for k in TENSOR_KEYS:
        assert got[k].dtype == want[k].numpy().dtype and got[k].shape == tuple(want[k].shape), k
        assert np.array_equal(got[k], want[k].numpy()), k


def test_collate_ref_without_token_types_and_with_rows_out_of_order(root):
    ds = dataset(root, True)
    ds.text_padding = partial(NoTokenTypes(max_length=T), max_length=T)
    arrays = arrays_of(ds, order=[5, 12, 0, 9, 3, 1, 11, 2, 10, 4, 8, 6, 7])
    assert np.any(np.diff(arrays[2]) < 0)
    sel = [3, 4, 5]
    want = ds.get_collate_fn()([ds[i] for i in sel])
    got = collate_ref(sel, *arrays, R=want['img_feat'].shape[1], L_out=want['attn_mask'].shape[1], ragged=True)
    assert want['token_type_ids'] is None and got['token_type_ids'] is None
    for k in TENSOR_KEYS:
        if want[k] is not None:
            assert np.array_equal(got[k], want[k].numpy()), k


@pytest.mark.parametrize('ragged', [False, True])
def test_host_planning_equals_the_host_collate(root, ragged):
    """R, L_out, seq_lens and the batch boundaries (13 samples in batches of 4: the last holds one) against a DataLoader
    over the same order; the wrapped dataset lives on the CPU here, which the planning never notices."""
    ds = dataset(root, ragged, confidence_threshold=0.3)
    dds = DeviceMemeDataset(ds, DeviceFeaturePool('cpu'))
    order = [4, 9, 1, 12, 0, 3, 3, 7, 11, 2, 5, 10, 8, 6]
    loader = DeviceLoader(dds, 4, sampler=order)
    assert loader.dataset is dds and len(dds) == 13 and dds.name == 'train' and dds.return_ids and dds.data is ds.data
    assert dds.ragged_regions == ragged
    host = list(data.DataLoader(ds, batch_size=4, sampler=order, collate_fn=ds.get_collate_fn()))
    plan = loader.plan(loader.order())
    assert len(plan) == len(host) == len(loader) == 4
    at = 0
    for (a, b, R, L_out, seq_lens), want in zip(plan, host):
        assert (a, b) == (at, at + want['labels'].shape[0])
        at = b
        assert R == want['img_feat'].shape[1] and L_out == want['attn_mask'].shape[1]
        assert seq_lens == want['seq_lens'] and all(type(x) is int for x in seq_lens)
    assert at == len(order) and plan[-1][1] - plan[-1][0] == 2
    assert plan == plan_batches(order, 4, dds.txt_len, dds.row_cnt, ragged)
    assert dds.txt_len.dtype == np.int32 and dds.row_cnt.dtype == np.int32
    with pytest.raises(ValueError, match=r'outside \[0, 13\)'):
        DeviceLoader(dds, 4, sampler=[0, 13]).order()
    with pytest.raises(ValueError, match=r'outside \[0, 13\)'):
        DeviceLoader(dds, 4, sampler=[-1]).order()


def test_pool_keeps_one_copy_of_an_image(root):
    ds = dataset(root, False)
    pool = DeviceFeaturePool('cpu')
    rs, rc = pool.add(ds)
    want = sum(ds[i]['img_feat'].shape[0] for i in range(len(ds)))
    assert pool.rows == want == int(rc.sum()) and pool.resident_bytes == want * (16 + 7) * 4
    rs2, rc2 = pool.add(dataset(root, True))
    assert pool.rows == want and np.array_equal(rs, rs2) and np.array_equal(rc, rc2)
    pool.add(dataset(root, False, confidence_threshold=0.5))       # another filter: other rows
    assert pool.rows > want
    s = ds[5]
    assert torch.equal(pool.feat[rs[5]:rs[5] + rc[5]], s['img_feat']) and torch.equal(pool.pos[rs[5]:rs[5] + rc[5]], s['img_pos_feat'])


def test_refusals_come_before_any_allocation(root):
    """device 'cuda' with no GPU in the process: an allocation would raise something else than ValueError"""
    pool = DeviceFeaturePool('cuda', max_gb=1e-6)
    with pytest.raises(ValueError, match='text_only.*not built'):
        DeviceMemeDataset(dataset(root, False, text_only=True), pool)
    with pytest.raises(ValueError, match='compact_batch=False.*not built'):
        DeviceMemeDataset(dataset(root, False, compact_batch=False), pool)
    with pytest.raises(ValueError, match=r'\d+ bytes of region features needed, 1073 allowed'):
        DeviceMemeDataset(dataset(root, False), pool)
    assert pool.feat is None and pool.rows == 0 and pool.resident_bytes == 0
