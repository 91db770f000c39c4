"""data.DevicePretrainLoader with resident soft labels: MRC and MRC-kl batches drawn on the device feed UniterForPretraining;
`label_ids` replaces the model's own argmax and `masked_positions` its nonzero without changing a bit of the loss, and the three
older tasks' sequences stay where they were."""
import os
from functools import partial

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pad_sequence

from common import (PRETRAIN_BATCH as BATCH, PRETRAIN_IMG_DIM, PRETRAIN_N as N, PRETRAIN_T, pretrain_dataset, pretrain_loader as _loader,
                    pretrain_model as _model, take as _take)

pytestmark = pytest.mark.gpu

LABEL_DIM = 12                     # pretrain_model's img_label_dim
FIVE = (('mlm', 1), ('mrfr', 1), ('itm', 1), ('mrc', 1), ('mrc-kl', 1))


@pytest.fixture(scope='module')
def dds(tmp_path_factory):
    """common.pretrain_dataset's files plus cls_prob, resident with their soft labels"""
    from meme_challenge_amd.data import DeviceFeaturePool, DeviceMemeDataset, HashTokenizer, MemeDataset, write_synthetic_dataset
    d = str(tmp_path_factory.mktemp('devmrc'))
    write_synthetic_dataset(d, n=N, num_bb=(3, 11), img_dim=PRETRAIN_IMG_DIM, seed=2, splits=('train',), text_words=(1, 9),
                            label_dim=LABEL_DIM)
    tok = partial(HashTokenizer(max_length=PRETRAIN_T), max_length=PRETRAIN_T)
    ds = MemeDataset(os.path.join(d, 'train.jsonl'), os.path.join(d, 'img_feats'), text_padding=tok, return_ids=True, ragged_regions=True,
                     soft_labels=True)
    return DeviceMemeDataset(ds, DeviceFeaturePool('cuda', soft_labels=True))


def samples_of(dds, batch):
    return [int(np.flatnonzero(dds.data.ids.numpy() == i)[0]) for i in batch['ids'].tolist()]


def both_labels(dds, batch, draw):
    """the same samples collated again with both label outputs (seed 3 is pretrain_loader's)"""
    from meme_challenge_amd.data import collate_mrc_batch
    pool = dds.pool
    sel = torch.tensor(samples_of(dds, batch), dtype=torch.int64, device='cuda')
    return collate_mrc_batch(sel, pool.feat[:pool.rows], pool.pos[:pool.rows], pool.soft[:pool.rows], dds.d_row_start, dds.d_row_cnt,
                             dds.d_input_ids, dds.d_token_type_ids, dds.d_txt_len, dds.d_labels, dds.d_ids, batch['img_feat'].shape[1],
                             batch['attn_masks'].shape[1], LABEL_DIM, ragged_regions=True, seed=3, draw=draw, prob=0.15)


@pytest.mark.parametrize('task', ['mrc', 'mrc-kl'])
def test_loss_with_the_loaders_batch_is_the_same_bits(dds, task):
    """the loader's batch; the same without `masked_positions` (the model's nonzero); for mrc the same with `label_targets` in place of
    `label_ids` (the model's argmax launch)"""
    assert dds.label_dim == LABEL_DIM and dds.pool.ld_soft == 12
    m = _model()
    loader = _loader(dds, tasks=((task, 1),))
    assert len(loader) == (N + BATCH - 1) // BATCH
    seen = _take(loader, len(loader) + 1)                   # one epoch and the first batch of the next
    assert [t for t, _ in seen] == [task] * len(seen) and loader.epochs[task] == 2
    assert seen[len(loader) - 1][1]['labels'].shape[0] == N % BATCH          # the short last batch
    for i, (_, batch) in enumerate(seen):
        n = batch['n_masked']
        assert ('label_ids' in batch, 'label_targets' in batch) == (task == 'mrc', task == 'mrc-kl')
        assert batch['seq_lens'] == [int(x) for x in batch['attn_masks'].sum(1).tolist()]
        assert n >= batch['labels'].shape[0] and tuple(batch['masked_positions'].shape) == (n, 2)
        assert torch.equal(batch['masked_positions'], torch.nonzero(batch['img_mask_tgt'], as_tuple=False))
        with torch.no_grad():
            fast = m(batch, task)
            slow = m({k: v for k, v in batch.items() if k != 'masked_positions'}, task)
        assert torch.isfinite(fast).all() and torch.equal(fast, slow)
        again = both_labels(dds, batch, draw=i // len(loader))
        assert int(again['n_masked'].item()) == n and torch.equal(again['masked_positions'][:n], batch['masked_positions'])
        if task == 'mrc':
            assert tuple(fast.shape) == (n,) and tuple(batch['label_ids'].shape) == (n,) and batch['label_ids'].dtype == torch.int64
            assert torch.equal(again['label_ids'][:n], batch['label_ids'])
            targets = again['label_targets'][:n]
            assert torch.equal(batch['label_ids'], 1 + targets[:, 1:].argmax(dim=1))
            by_argmax = {k: v for k, v in batch.items() if k != 'label_ids'}
            by_argmax['label_targets'] = targets
            with torch.no_grad():
                assert torch.equal(m(by_argmax, task), fast)
        else:
            assert tuple(fast.shape) == (n, LABEL_DIM) and tuple(batch['label_targets'].shape) == (n, LABEL_DIM)
            assert torch.equal(again['label_targets'][:n], batch['label_targets'])


def test_label_targets_are_the_soft_rows_the_masks_name_and_the_batch_is_the_hosts(dds):
    """against the pool, and against the host collate of the same samples with the upstream MRC collate's own steps on top:
    label_targets = pad(soft)[img_masks.bool()], img_feat zeroed under the mask, img_mask_tgt = the mask behind each text"""
    loader = _loader(dds, tasks=(('mrc-kl', 1),))
    ds = dds.dataset
    for _, batch in _take(loader, len(loader)):
        sel = samples_of(dds, batch)
        assert all(s in loader.epoch_orders['mrc-kl'][0] for s in sel)
        masks = batch['img_masks'].cpu()
        assert masks.dtype == torch.int64 and batch['img_mask_tgt'].dtype == torch.bool
        rows = []
        for b, s in enumerate(sel):
            n, start = int(dds.row_cnt[s]), int(dds.d_row_start[s])
            assert masks[b, :n].sum() >= 1 and not masks[b, n:].any()
            rows += [start + r for r in torch.nonzero(masks[b]).flatten().tolist()]
        want = dds.pool.soft[torch.tensor(rows, device='cuda'), :LABEL_DIM]
        assert torch.equal(batch['label_targets'], want) and batch['label_targets'].shape[0] == batch['n_masked']
        samples = [ds[s] for s in sel]
        host = ds.get_collate_fn()(samples)
        soft = pad_sequence([s['img_soft_label'] for s in samples], batch_first=True, padding_value=0)
        assert torch.equal(batch['label_targets'].cpu(), soft[masks.bool()])
        assert torch.equal(batch['img_feat'].cpu(), host['img_feat'].masked_fill(masks.bool().unsqueeze(-1), 0))
        tgt = torch.zeros_like(batch['img_mask_tgt'].cpu())
        for b, s in enumerate(sel):
            tl = int(dds.txt_len[s])
            tgt[b, tl:tl + masks.shape[1]] = masks[b, :tgt.shape[1] - tl].bool()
        assert torch.equal(batch['img_mask_tgt'].cpu(), tgt)
        for k, hk in (('img_pos_feat', 'img_pos_feat'), ('input_ids', 'input_ids'), ('position_ids', 'position_ids'),
                      ('token_type_ids', 'token_type_ids'), ('attn_masks', 'attn_mask'), ('gather_index', 'gather_index'),
                      ('labels', 'labels'), ('ids', 'ids')):
            assert torch.equal(batch[k].cpu(), host[hk]), k
        assert batch['seq_lens'] == host['seq_lens']


def same_batches(one, two):
    for (ta, a), (tb, b) in zip(one, two):
        assert ta == tb and set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


def test_the_five_task_sequence_is_reproducible_and_the_three_task_one_has_not_moved(dds, tmp_path_factory):
    one, two = _take(_loader(dds, tasks=FIVE), 25), _take(_loader(dds, tasks=FIVE), 25)
    assert {t for t, _ in one} == {'mlm', 'mrfr', 'itm', 'mrc', 'mrc-kl'}
    same_batches(one, two)
    # a sample's MRC mask is not its MRFR mask
    mrc = next(b for t, b in _take(_loader(dds, tasks=(('mrc', 1),), samplers={'mrc': range(N)}), 1))
    mrfr = next(b for t, b in _take(_loader(dds, tasks=(('mrfr', 1),), samplers={'mrfr': range(N)}), 1))
    assert torch.equal(mrc['ids'], mrfr['ids']) and not torch.equal(mrc['img_masks'], mrfr['img_masks'])
    # the default three tasks: on this dataset, and on the same files resident without soft labels
    plain = pretrain_dataset(tmp_path_factory)
    assert plain.label_dim is None and plain.pool.soft is None
    here, there = _take(_loader(dds, accum_steps=2), 14), _take(_loader(plain, accum_steps=2), 14)
    assert {t for t, _ in here} == {'mlm', 'mrfr', 'itm'}
    same_batches(here, there)
    with pytest.raises(ValueError, match='unknown task'):
        _loader(plain, tasks=(('mlm', 1), ('mrc', 1)))


def test_fifteen_multitask_training_steps(dds):
    from meme_challenge_amd.trainer import FusedAdam
    m = _model(train=True)
    opt = FusedAdam(m, lr=1e-3, weight_decay=1e-3)
    losses, tasks = [], []
    for task, batch in _take(_loader(dds, tasks=FIVE), 15):
        loss = m(batch, task).mean()
        loss.backward()
        opt.step(grad_scale=1.0, max_grad_norm=5)
        losses.append(loss.detach())
        tasks.append(task)
    if hasattr(opt, 'join'):
        opt.join()
    torch.cuda.synchronize()
    assert set(tasks) == {'mlm', 'mrfr', 'itm', 'mrc', 'mrc-kl'}, tasks
    assert all(bool(torch.isfinite(l)) for l in losses), [float(l) for l in losses]
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
