"""Device-resident dataset end to end: data.DeviceLoader yields what the host collate yields, bit for bit; images shared between
datasets are resident once; batches stay intact while their steps are in flight; the CLI trains and scores through it."""
import json
import os
from functools import partial

import pytest
import torch
from torch.utils import data

from common import TINY

pytestmark = pytest.mark.gpu

T, IMG_DIM = 16, 64
CFG = dict(TINY, vocab_size=28996, max_position_embeddings=64)


def _tok():
    from meme_challenge_amd.data import HashTokenizer
    return partial(HashTokenizer(max_length=T), max_length=T)


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    from meme_challenge_amd.data import write_synthetic_dataset, build_feature_shard
    d = str(tmp_path_factory.mktemp('devds'))
    write_synthetic_dataset(d, n=24, num_bb=(3, 11), img_dim=IMG_DIM, seed=2, splits=('train',), text_words=(1, 9))
    lines = open(os.path.join(d, 'train.jsonl')).read().splitlines()
    with open(os.path.join(d, 'fold.jsonl'), 'w') as f:             # a cross-validation fold: a subset of the same images
        f.write('\n'.join(lines[3:17:2]) + '\n')
    build_feature_shard(os.path.join(d, 'img_feats'), [json.loads(l)['id'] for l in lines], os.path.join(d, 'train_shard'))
    return d


def _dataset(root, fname='train.jsonl', **kw):
    from meme_challenge_amd.data import MemeDataset
    return MemeDataset(os.path.join(root, fname), os.path.join(root, 'img_feats'), text_padding=_tok(), return_ids=True, **kw)


def _assert_same_batch(got, want, what):
    assert set(got) == set(want), what
    for k, w in want.items():
        g = got[k]
        if w is None:
            assert g is None, (what, k)
        elif torch.is_tensor(w):
            assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, tuple(g.shape))
            assert torch.equal(g.cpu(), w), (what, k)
        else:
            assert type(g) is list and g == w, (what, k)


@pytest.mark.parametrize('ragged,thr,shard', [(False, 0.0, True), (True, 0.4, False)])
def test_device_loader_yields_the_host_collate_bit_for_bit(root, ragged, thr, shard):
    from meme_challenge_amd.data import DeviceFeaturePool, DeviceLoader, DeviceMemeDataset
    ds = _dataset(root, ragged_regions=ragged, confidence_threshold=thr,
                  feature_shard=os.path.join(root, 'train_shard') if shard else None)
    order = [5, 23, 0, 11, 7, 7, 19, 2, 14, 1, 22, 9, 3, 16, 8, 20, 4, 13, 21, 6, 18, 10, 15]     # 23 in batches of 5: a short last one
    host = data.DataLoader(ds, batch_size=5, sampler=order, collate_fn=ds.get_collate_fn())
    loader = DeviceLoader(DeviceMemeDataset(ds, DeviceFeaturePool('cuda')), 5, sampler=order)
    assert len(loader) == len(host) == 5
    for epoch in range(2):                       # a loader is iterated once per epoch
        got, want = list(loader), list(host)
        assert len(got) == len(want) == 5 and got[-1]['labels'].shape[0] == 3
        for i, (g, w) in enumerate(zip(got, want)):
            _assert_same_batch(g, w, 'epoch %d batch %d' % (epoch, i))
    if thr > 0:
        assert len({b['img_feat'].shape[1] for b in got}) > 1      # the filter leaves the batches different region counts
    # without a sampler: the file's order
    plain = DeviceLoader(loader.dataset, 7)
    for g, w in zip(plain, data.DataLoader(ds, batch_size=7, collate_fn=ds.get_collate_fn())):
        _assert_same_batch(g, w, 'sequential')
    assert len(plain) == 4


def test_datasets_that_share_images_upload_each_image_once(root):
    from meme_challenge_amd.data import DeviceFeaturePool, DeviceLoader, DeviceMemeDataset
    pool = DeviceFeaturePool('cuda')
    full = DeviceMemeDataset(_dataset(root), pool)
    resident = pool.resident_bytes
    assert resident == int(full.row_cnt.sum()) * (IMG_DIM + 7) * 4 > 0
    fold_ds = _dataset(root, 'fold.jsonl')
    fold = DeviceMemeDataset(fold_ds, pool)
    assert pool.resident_bytes == resident and len(fold) == 7
    for g, w in zip(DeviceLoader(fold, 4), data.DataLoader(fold_ds, batch_size=4, collate_fn=fold_ds.get_collate_fn())):
        _assert_same_batch(g, w, 'fold')
    with pytest.raises(ValueError, match='bytes of region features needed'):
        DeviceMemeDataset(_dataset(root), DeviceFeaturePool('cuda', max_gb=1e-5))


def _train(batches_of_epoch, epochs):
    from meme_challenge_amd import trainer as TR
    from meme_challenge_amd.meme_uniter import MemeUniter
    from meme_challenge_amd.model import UniterConfig, UniterModel
    c = UniterConfig.from_dict(CFG)
    torch.manual_seed(0)
    m = MemeUniter(UniterModel(c, img_dim=IMG_DIM), c.hidden_size, 1).cuda().train()
    m.uniter_model.set_dropout_seed(5, 0)
    m.uniter_model.deterministic = True
    config = dict(optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=1e-2, gradient_accumulation=1, max_grad_norm=5,
                  pos_wt=1.8, loss_func='bce_logits', scheduler='warmup_cosine', warmup_steps=2, max_epoch=epochs)
    opt = TR.get_optimizer(m, config)
    step = TR.TrainStep(m, opt, TR.get_scheduler(opt, config, steps_per_epoch=6), config)
    for _ in range(epochs):
        for it, batch in enumerate(batches_of_epoch()):
            step.train_iter(batch, iters=it)                # nothing waits for the device between two steps
    if hasattr(opt, 'join'):
        opt.join()
    torch.cuda.synchronize()
    assert m.uniter_model.bit_reproducible
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def test_training_from_the_device_loader_leaves_the_host_path_parameters(root):
    """Two epochs with no synchronisation between the steps, once from the DeviceLoader and once from the host-collated batches
    moved to the device: every parameter bit-equal.  The batches are equal (above), so a difference here is a batch that was
    overwritten or freed while its step was still in flight."""
    from meme_challenge_amd.data import DeviceFeaturePool, DeviceLoader, DeviceMemeDataset
    ds = _dataset(root, ragged_regions=True)
    order = list(range(23, -1, -1))
    host = [{k: v for k, v in b.items()} for b in data.DataLoader(ds, batch_size=4, sampler=order, collate_fn=ds.get_collate_fn())]
    loader = DeviceLoader(DeviceMemeDataset(ds, DeviceFeaturePool('cuda')), 4, sampler=order)
    want = _train(lambda: ({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()} for b in host), 2)
    got = _train(lambda: loader, 2)
    assert set(got) == set(want)
    for n in want:
        assert torch.isfinite(want[n]).all() and torch.equal(got[n], want[n]), n


# ---- the CLI ------------------------------------------------------------------------------------------------------------
def _cli_args(tmp, extra=()):
    cfg = tmp / 'tiny.json'
    cfg.write_text(json.dumps(dict(TINY, vocab_size=28996, max_position_embeddings=64)))
    return ['--config', str(cfg), '--data_path', str(tmp / 'data'), '--model_path', str(tmp / 'ckpt'), '--vis_path', str(tmp / 'vis'),
            '--synthetic', '48', '--batch_size', '8', '--max_epoch', '3', '--lr', '1e-3', '--warmup_steps', '2',
            '--gradient_accumulation', '2', '--pos_wt', '1.8', '--max_txt_len', '16', '--seed', '1', '--log_every', '3',
            '--ragged_regions'] + list(extra)


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """the arguments of test_cli_trains_exports_and_checkpoint_reloads[ragged=True] plus --device_dataset, run once"""
    import train_uniter
    tmp = tmp_path_factory.mktemp('cli')
    best, test_metrics = train_uniter.main(_cli_args(tmp, ['--device_dataset']))
    return tmp, best, test_metrics


def test_cli_trains_and_exports_with_a_device_dataset(trained):
    tmp, best, test_metrics = trained
    model_dir = str(tmp / 'ckpt')
    assert 0.9 < best['aucroc'] <= 1.0
    ck = torch.load(os.path.join(model_dir, 'best_model.pt'))
    assert set(ck) == {'model_state_dict'} and 'uniter_model.encoder.layer.1.output.dense.weight' in ck['model_state_dict']
    metrics = json.load(open(os.path.join(model_dir, 'best_model_metrics.json')))
    assert {'dev', 'train'} <= set(metrics) and 'loss' in metrics['dev']
    csv = open(os.path.join(model_dir, 'best_model_dev_seen_preds.csv')).read().splitlines()
    assert csv[0] == 'id,proba,label,gt' and len(csv) == 49
    assert 'test_seen' in test_metrics


def test_cli_trains_with_a_device_dataset_and_token_packing(tmp_path):
    import train_uniter
    best, test_metrics = train_uniter.main(_cli_args(tmp_path, ['--device_dataset', '--pack_padded']))
    assert 0.0 < best['aucroc'] <= 1.0 and 'test_seen' in test_metrics
    assert os.path.isfile(str(tmp_path / 'ckpt' / 'best_model_dev_seen_preds.csv'))


def test_cli_scores_a_checkpoint_alike_through_both_loaders(trained):
    """The CLI has no evaluate-only flag, so this takes the second route: the CLI's own set-up (train_uniter._setup: flags -> config
    and loaders) and the trainer's final evaluation (TrainerTemplate._final_evaluation: reload the best checkpoint, threshold on
    dev_seen, export_val_predictions of every test set), once with --no_prefetch (the plain DataLoader) and once with
    --device_dataset.  The prediction files are the same bytes."""
    import train_uniter
    tmp = trained[0]
    model_dir = str(tmp / 'ckpt')
    files = ('best_model_dev_seen_preds.csv', 'best_model_test_seen_preds.csv')
    out = {}
    for route in ('--no_prefetch', '--device_dataset'):
        for f in files:
            os.replace(os.path.join(model_dir, f), os.path.join(model_dir, f + '.before'))
        config, make = train_uniter._setup(_cli_args(tmp, [route]))
        config['train_loader'], config['val_loader'] = make('train.jsonl', train=True), make('dev_seen.jsonl')
        from meme_challenge_amd.data import DeviceLoader
        assert isinstance(config['val_loader'], DeviceLoader) == (route == '--device_dataset')
        trainer = train_uniter.TrainerUniter(config)
        trainer._final_evaluation()
        config['writer'].close()
        out[route] = [open(os.path.join(model_dir, f), 'rb').read() for f in files]
    for a, b in zip(*out.values()):
        assert a == b and a.count(b'\n') == 49
