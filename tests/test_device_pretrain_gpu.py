"""data.DevicePretrainLoader end to end: MLM / MRFR / ITM batches drawn on the device from a resident dataset feed
UniterForPretraining; `masked_positions` replaces the model's own nonzero without changing a bit of the loss."""
import numpy as np
import pytest
import torch

from common import (PRETRAIN_BATCH as BATCH, PRETRAIN_N as N, pretrain_dataset, pretrain_loader as _loader,
                    pretrain_model as _model, take as _take)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dds(tmp_path_factory):
    return pretrain_dataset(tmp_path_factory)


def test_text_class_indexes_the_distinct_texts(dds):
    texts = dds.data.text
    assert dds.text_class.dtype == np.int32 and dds.text_class.shape == (N,)
    for i in range(N):
        for j in range(N):
            assert (dds.text_class[i] == dds.text_class[j]) == (texts[i] == texts[j])


@pytest.mark.parametrize('task', ['mlm', 'mrfr', 'itm'])
def test_loss_with_and_without_masked_positions_is_the_same_bits(dds, task):
    """the loader's batch, and the same batch without `masked_positions` (today's nonzero path)"""
    m = _model()
    loader = _loader(dds, tasks=((task, 1),))
    assert len(loader) == (N + BATCH - 1) // BATCH
    seen = _take(loader, len(loader) + 1)                   # one epoch and the first batch of the next
    assert [t for t, _ in seen] == [task] * len(seen) and loader.epochs[task] == 2
    assert seen[len(loader) - 1][1]['labels'].shape[0] == N % BATCH          # the short last batch
    for _, batch in seen:
        assert ('masked_positions' in batch) == (task != 'itm')
        assert batch['seq_lens'] == [int(x) for x in batch['attn_masks'].sum(1).tolist()]
        with torch.no_grad():
            fast = m(batch, task)
            slow = m({k: v for k, v in batch.items() if k != 'masked_positions'}, task)
        assert fast.shape == slow.shape and torch.isfinite(fast).all() and torch.equal(fast, slow)
        if task == 'itm':
            continue
        n = batch['n_masked']
        mask = (batch['txt_labels'] != -1) if task == 'mlm' else batch['img_mask_tgt']
        assert n >= batch['labels'].shape[0] and tuple(batch['masked_positions'].shape) == (n, 2)
        assert torch.equal(batch['masked_positions'], torch.nonzero(mask, as_tuple=False)) and fast.shape[0] == n


def test_feat_targets_are_the_pool_rows_the_masks_name(dds):
    loader = _loader(dds, tasks=(('mrfr', 1),))
    for _, batch in _take(loader, len(loader)):
        order = loader.epoch_orders['mrfr'][0]
        sel = [int(np.flatnonzero(dds.data.ids.numpy() == i)[0]) for i in batch['ids'].tolist()]
        assert all(s in order for s in sel)
        rows = []
        masks = batch['img_masks'].cpu()
        assert masks.dtype == torch.int64 and batch['img_mask_tgt'].dtype == torch.bool
        for b, s in enumerate(sel):
            n, start = int(dds.row_cnt[s]), int(dds.d_row_start[s])
            assert masks[b, :n].sum() >= 1 and not masks[b, n:].any()
            for r in torch.nonzero(masks[b]).flatten().tolist():
                rows.append(start + r)
                assert not batch['img_feat'][b, r].any()                      # the masked region's features are zero
        want = dds.pool.feat[torch.tensor(rows, device='cuda')]
        assert torch.equal(batch['feat_targets'], want) and batch['feat_targets'].shape[0] == batch['n_masked']


def test_itm_targets_agree_with_itm_pairs(dds):
    from meme_challenge_amd.data import DevicePretrainLoader, itm_pairs
    loader = _loader(dds, tasks=(('itm', 1),), replace_prob=0.5)
    batches = [b for _, b in _take(loader, len(loader))]
    order, txt_order = loader.epoch_orders['itm']
    rng = DevicePretrainLoader.task_rng(3, 'itm')                             # the loader's own draws, again
    assert np.array_equal(order, rng.permutation(N)) and np.array_equal(txt_order, itm_pairs(order, dds.text_class, 0.5, rng))
    targets = torch.cat([b['targets'] for b in batches]).cpu().numpy()
    assert np.array_equal(targets, (txt_order == order).astype(np.int64)) and 0 < targets.sum() < N
    assert np.array_equal(torch.cat([b['ids'] for b in batches]).cpu().numpy(), dds.data.ids.numpy()[order])
    assert torch.equal(torch.cat([b['input_ids'] for b in batches]), dds.d_input_ids[torch.from_numpy(txt_order).cuda()])
    # a replaced text is another string
    texts = dds.data.text
    assert all(texts[t] != texts[s] for s, t in zip(order, txt_order) if s != t)


def test_the_sequence_is_reproducible_and_the_refusals_come_before_any_launch(dds):
    from meme_challenge_amd.data import DevicePretrainLoader
    one, two = _take(_loader(dds, accum_steps=2), 14), _take(_loader(dds, accum_steps=2), 14)
    assert [t for t, _ in one] == [t for t, _ in two] and {t for t, _ in one} == {'mlm', 'mrfr', 'itm'}
    assert all(one[i][0] == one[i + 1][0] for i in range(0, 14, 2))          # a task holds for accum_steps steps
    for (_, a), (_, b) in zip(one, two):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    other = _take(DevicePretrainLoader(dds, BATCH, seed=4, accum_steps=2), 14)
    assert [t for t, _ in other] != [t for t, _ in one] or not torch.equal(other[0][1]['ids'], one[0][1]['ids'])
    assert len(_loader(dds)) == 3 * ((N + BATCH - 1) // BATCH) and len(_loader(dds, tasks=(('mlm', 2), ('itm', 1)))) == 2 * 5
    with pytest.raises(ValueError, match='no task'):
        _loader(dds, tasks=())
    with pytest.raises(ValueError, match='unknown task'):
        _loader(dds, tasks=(('mlm', 1), ('mrc', 1)))
    for bad in ([0, N], [-1, 2]):
        with pytest.raises(ValueError, match='outside'):
            next(iter(_loader(dds, tasks=(('mlm', 1),), samplers={'mlm': bad})))
    # a sampler's order is walked as given
    _, batch = next(iter(_loader(dds, tasks=(('mrfr', 1),), samplers={'mrfr': [7, 7, 2, 0, 19, 4]})))
    assert batch['ids'].tolist() == dds.data.ids[[7, 7, 2, 0, 19]].tolist()


def test_twelve_multitask_training_steps(dds):
    from meme_challenge_amd.trainer import FusedAdam
    m = _model(train=True)
    opt = FusedAdam(m, lr=1e-3, weight_decay=1e-3)
    losses, tasks = [], []
    for task, batch in _take(_loader(dds), 12):
        loss = m(batch, task).mean()
        loss.backward()
        opt.step(grad_scale=1.0, max_grad_norm=5)
        losses.append(loss.detach())
        tasks.append(task)
    if hasattr(opt, 'join'):
        opt.join()
    torch.cuda.synchronize()
    assert set(tasks) == {'mlm', 'mrfr', 'itm'}, tasks
    assert all(bool(torch.isfinite(l)) for l in losses), [float(l) for l in losses]
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
