"""The host side of the MRC path, without a GPU: the numpy restatement tests/mrc_collate_ref.py against a brute-force loop, the
soft labels through write_synthetic_dataset / MemeDataset / DeviceFeaturePool (on the CPU), what the cases of
tests/test_mrc_collate_gpu.py contain at the seeds they use, and the loader's refusal on a dataset without soft labels."""
import filecmp
import os
from functools import partial

import numpy as np
import pytest
import torch

from meme_challenge_amd import data
from meme_challenge_amd.data import (DeviceFeaturePool, DeviceMemeDataset, DevicePretrainLoader, HashTokenizer, MemeDataset,
                                     build_feature_shard, load_soft_labels, write_synthetic_dataset)
from mrc_cases import ARRAY_KEYS, BATCHES, CFG, COUNTS, CRAFTED, MAIN, crafted_rows, leading_dimensions, shape_of, synth
from mrc_collate_ref import STREAM_MRC, hard_label, mrc_collate_ref, mrc_forced, mrc_sample
from oracle.philox import philox4x32_10
from pretrain_collate_ref import DEFAULT_CFG, STREAM_MRFR, mrfr_sample

T, IMG_DIM, LABEL_DIM, N = 16, 16, 12, 10


def ref(a, sel, C, ragged, prob):
    R, L_out = shape_of(a, sel, ragged)
    return mrc_collate_ref(sel, *[a[k] for k in ('feat', 'pos', 'soft')], C, *[a[k] for k in ARRAY_KEYS[3:]], R=R, L_out=L_out,
                           ragged=ragged, cfg=dict(CFG, prob=prob))


def drawn(position, sample, prob):
    """one Philox call per position, straight from the header's words"""
    seed = CFG['seed']
    x = int(philox4x32_10(np.uint64(position), np.uint64(sample), np.uint64(0xFFFF0004), np.uint64(CFG['draw']), seed & 0xFFFFFFFF,
                          seed >> 32)[0])
    return x, (prob >= 1.0 or x < int(np.floor(float(np.float32(prob)) * 4294967296.0)))


@pytest.mark.parametrize('C', [5, 12])
def test_the_restatement_equals_a_brute_force_loop(C):
    assert STREAM_MRC == 0xFFFF0004 and STREAM_MRC != STREAM_MRFR
    a = synth(C, leading_dimensions(C)['odd'], seed=C)
    rows = a['feat'].shape[0]
    for name, sel in BATCHES.items():
        for prob in (0.0, 0.15, 1.0):
            got = ref(a, sel, C, True, prob)
            R, L_out = shape_of(a, sel, True)
            positions, targets, ids = [], [], []
            masks, tgt, feat = np.zeros((len(sel), R), np.int64), np.zeros((len(sel), L_out), bool), np.zeros((len(sel), R, 64), np.float32)
            for b, s in enumerate(sel):
                n, tl = int(a['row_cnt'][s]), int(a['txt_len'][s])
                hits = [r for r in range(n) if drawn(r, s, prob)[1]]
                if not hits and n:
                    hits = [(drawn(0xFFFFFFFF, s, prob)[0] * n) >> 32]
                for r in range(n):
                    src = int(a['row_start'][s]) + r
                    inside = 0 <= src < rows
                    if r in hits:
                        masks[b, r], tgt[b, tl + r] = 1, True
                        positions.append((b, tl + r))
                        targets.append(a['soft'][src, :C] if inside else np.zeros(C, np.float32))
                        ids.append(1 + int(np.argmax(targets[-1][1:])))
                    elif inside:
                        feat[b, r] = a['feat'][src]
            what = '%s prob %g' % (name, prob)
            assert np.array_equal(got['img_masks'], masks) and np.array_equal(got['img_mask_tgt'], tgt), what
            assert np.array_equal(got['img_feat'], feat), what
            assert got['n_masked'] == len(positions) and np.array_equal(got['masked_positions'], np.asarray(positions).reshape(-1, 2)), what
            assert np.array_equal(got['label_targets'], np.asarray(targets, np.float32).reshape(-1, C)), what
            assert got['label_ids'].tolist() == ids, what
            assert not np.isnan(got['label_targets']).any(), 'a pad column of soft reached label_targets: ' + what
    assert hard_label(np.array([9, -np.inf, -np.inf], np.float32)) == 1 and hard_label(np.array([0, np.nan, 1, 1], np.float32)) == 2


@pytest.mark.parametrize('C', [5, 12, 1601])
def test_the_gpu_cases_contain_what_they_claim(C):
    a = synth(C, leading_dimensions(C)['aligned'], seed=C)
    cfg = dict(DEFAULT_CFG, **dict(CFG, prob=0.15))
    cnt = a['row_cnt']
    assert sorted(set(cnt[MAIN].tolist())) == [3, 5, 7, 11] and cnt[3] == 0 and np.array_equal(cnt, COUNTS)
    # at prob 0.15 the main batch has a sample that takes the forced region, one with at least two regions, and one whose MRC mask
    # is not its MRFR mask (the masks depend on the seed and the sample alone, not on C)
    raw = {s: [drawn(r, s, 0.15)[1] for r in range(int(cnt[s]))] for s in MAIN}
    masks = {s: mrc_sample(int(cnt[s]), s, cfg) for s in MAIN}
    forced = [s for s in MAIN if not any(raw[s])]
    assert forced and all(sum(masks[s]) == 1 and masks[s][mrc_forced(int(cnt[s]), s, cfg)] for s in forced)
    assert any(sum(m) >= 2 for m in masks.values())
    assert any(masks[s] != mrfr_sample(int(cnt[s]), s, cfg) for s in MAIN)
    # prob 0: every sample with regions takes exactly its forced one
    zero = dict(cfg, prob=0.0)
    assert all(sum(mrc_sample(int(cnt[s]), s, zero)) == 1 for s in range(len(cnt)) if cnt[s])
    # pool rows out of order, shared, and outside
    rs, rows = a['row_start'], a['feat'].shape[0]
    assert np.any(np.diff(rs[:7]) < 0) and rs[7] == rs[0] + 1 and rs[7] + cnt[7] <= rs[0] + cnt[0]
    assert rs[8] + 2 == rows and cnt[8] == 6
    out = ref(a, BATCHES['outside the pool'], C, True, 1.0)
    assert int((out['label_targets'] == 0).all(axis=1).sum()) == 8 and (out['label_ids'][(out['label_targets'] == 0).all(axis=1)] == 1).all()
    assert shape_of(a, BATCHES['no regions at all'], True)[0] == 0
    # the crafted rows: a tie (the first wins), all equal, column 0 ignored, the last column, a tie inside one lane
    crafted, want = crafted_rows(C)
    assert [hard_label(r) for r in crafted] == want and want[1] == 1 and want[3] == C - 1
    assert crafted[0][2] == crafted[0][C - 1] == crafted[0].max() and int(np.argmax(crafted[2])) == 0 and want[2] != 0
    q, r = (want[4], want[4] + 256) if C > 326 else (1, 3)
    assert crafted[4][q] == crafted[4][r] == crafted[4].max()
    if C > 326:                  # one lane in both layouts: floats (column % 64) and 16-byte items ((column // 4) % 64)
        assert q % 64 == r % 64 and (q // 4) % 64 == (r // 4) % 64
    full = ref(a, MAIN, C, True, 1.0)
    first = int(cnt[MAIN[:MAIN.index(CRAFTED)]].sum())
    assert full['label_ids'][first:first + 5].tolist() == want
    assert np.isnan(a['soft'][:, C:]).all() and not np.isnan(a['soft'][:, :C]).any()
    kinds = leading_dimensions(C)
    assert kinds['C'] == C and kinds['aligned'] % 4 == 0 and kinds['aligned'] > C and kinds['odd'] % 4 != 0 and kinds['odd'] > C


# ---- the host dataset path ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def roots(tmp_path_factory):
    plain, soft = str(tmp_path_factory.mktemp('plain')), str(tmp_path_factory.mktemp('soft'))
    kw = dict(n=N, num_bb=(3, 9), img_dim=IMG_DIM, seed=4, splits=('train',), text_words=(1, 6))
    write_synthetic_dataset(plain, **kw)
    write_synthetic_dataset(soft, label_dim=LABEL_DIM, **kw)
    return plain, soft


def dataset(root, **kw):
    tok = partial(HashTokenizer(max_length=T), max_length=T)
    return MemeDataset(os.path.join(root, 'train.jsonl'), os.path.join(root, 'img_feats'), text_padding=tok, return_ids=True,
                       ragged_regions=True, **kw)


def test_label_dim_changes_nothing_but_cls_prob(roots):
    plain, soft = roots
    assert filecmp.cmp(os.path.join(plain, 'train.jsonl'), os.path.join(soft, 'train.jsonl'), shallow=False)
    for i in range(N):
        name = data.expand_id(i)
        assert filecmp.cmp(os.path.join(plain, 'img_feats', name + '.npy'), os.path.join(soft, 'img_feats', name + '.npy'), shallow=False)
        p = np.load(os.path.join(plain, 'img_feats', name + '_info.npy'), allow_pickle=True).item()
        s = np.load(os.path.join(soft, 'img_feats', name + '_info.npy'), allow_pickle=True).item()
        assert set(s) == set(p) | {'cls_prob'}
        for k in p:
            assert np.array_equal(np.asarray(p[k]), np.asarray(s[k])) and np.asarray(p[k]).dtype == np.asarray(s[k]).dtype, k
        q = s['cls_prob']
        assert q.dtype == np.float32 and q.shape == (len(p['bbox']), LABEL_DIM) and (q > 0).all()
        # rows sum to 1 in fp32: each of the 12 terms is rounded once (together at most eps / 2) and so is each of 11 partial sums
        assert np.abs(q.sum(axis=1, dtype=np.float32) - 1).max() <= 6 * np.finfo(np.float32).eps
        assert torch.equal(load_soft_labels(os.path.join(soft, 'img_feats'), i), torch.from_numpy(q))
    # two images do not share their draws
    a = np.load(os.path.join(soft, 'img_feats', data.expand_id(0) + '_info.npy'), allow_pickle=True).item()['cls_prob']
    b = np.load(os.path.join(soft, 'img_feats', data.expand_id(1) + '_info.npy'), allow_pickle=True).item()['cls_prob']
    assert not np.array_equal(a[:3], b[:3])


def test_soft_labels_follow_the_features_through_the_confidence_filter(roots):
    plain, soft = roots
    feat_dir = os.path.join(soft, 'img_feats')
    off, on, filtered = dataset(soft), dataset(soft, soft_labels=True), dataset(soft, soft_labels=True, confidence_threshold=0.4)
    cached = dataset(soft, soft_labels=True, confidence_threshold=0.4, preload_images=True)
    dropped = kept = 0
    for i in range(N):
        assert 'img_soft_label' not in off[i] and set(on[i]) == set(off[i]) | {'img_soft_label'}
        full = load_soft_labels(feat_dir, i)
        assert torch.equal(on[i]['img_soft_label'], full) and full.dtype == torch.float32
        assert torch.equal(on[i]['img_feat'], off[i]['img_feat'])
        conf = np.load(os.path.join(feat_dir, data.expand_id(i) + '_info.npy'), allow_pickle=True).item()['objects_conf']
        keep = torch.from_numpy(conf > 0.4)
        s = filtered[i]
        assert torch.equal(s['img_soft_label'], full[keep]) and torch.equal(s['img_feat'], on[i]['img_feat'][keep])
        assert s['img_soft_label'].shape[0] == s['img_feat'].shape[0]
        assert torch.equal(cached[i]['img_soft_label'], s['img_soft_label']) and torch.equal(cached[i]['img_feat'], s['img_feat'])
        dropped += int((~keep).sum())
        kept += int(keep.sum())
    assert dropped > 0 and kept > 0              # the threshold drops some regions but not all
    # a missing cls_prob names the file; a shard is refused
    with pytest.raises(ValueError, match=r'00003_info\.npy has no cls_prob'):
        load_soft_labels(os.path.join(plain, 'img_feats'), 3)
    with pytest.raises(ValueError, match='no cls_prob'):
        dataset(plain, soft_labels=True)[0]
    prefix = os.path.join(soft, 'shard')
    build_feature_shard(feat_dir, range(N), prefix)
    assert 'img_soft_label' not in dataset(soft, feature_shard=prefix)[0]
    with pytest.raises(ValueError, match='shard.*no cls_prob'):
        dataset(soft, feature_shard=prefix, soft_labels=True)


def test_the_pool_keeps_soft_rows_beside_the_feature_rows(roots):
    plain, soft = roots
    ds = dataset(soft, soft_labels=True)
    pool = DeviceFeaturePool('cpu', soft_labels=True)
    dds = DeviceMemeDataset(ds, pool)
    rows = sum(ds[i]['img_feat'].shape[0] for i in range(N))
    assert dds.label_dim == pool.label_dim == LABEL_DIM and pool.ld_soft == 12 and pool.rows == rows
    assert pool.resident_bytes == rows * (IMG_DIM + 7 + 12) * 4
    rs, rc = dds.d_row_start.numpy(), dds.row_cnt
    for i in range(N):
        s = ds[i]
        assert torch.equal(pool.soft[rs[i]:rs[i] + rc[i], :LABEL_DIM], s['img_soft_label'])
        assert torch.equal(pool.feat[rs[i]:rs[i] + rc[i]], s['img_feat'])
    # another filter: more rows, the earlier ones kept through the growth of the buffers
    before = pool.soft[:rows].clone()
    DeviceMemeDataset(dataset(soft, soft_labels=True, confidence_threshold=0.4), pool)
    assert pool.rows > rows and torch.equal(pool.soft[:rows], before) and pool.soft.shape[0] == pool.feat.shape[0]
    # a leading dimension beyond C: zero columns behind the distribution
    odd = DeviceFeaturePool('cpu', soft_labels=True)
    odd_ds = dataset(soft, soft_labels=True)
    real = odd_ds.__class__.__getitem__

    class Narrow(MemeDataset):
        def __getitem__(self, idx):
            s = real(self, idx)
            s['img_soft_label'] = s['img_soft_label'][:, :9].contiguous()
            return s
    odd_ds.__class__ = Narrow
    DeviceMemeDataset(odd_ds, odd)
    assert (odd.label_dim, odd.ld_soft) == (9, 12) and not odd.soft[:odd.rows, 9:].any()
    assert torch.equal(odd.soft[:odd.rows, :9], pool.soft[:rows, :9])
    # one common C, and the image that breaks it
    with pytest.raises(ValueError, match=r'image \d+ has soft labels of 12 classes, the pool holds rows of 9'):
        odd.add(dataset(soft, soft_labels=True, confidence_threshold=0.2))
    with pytest.raises(ValueError, match=r'image 0 first.*soft_labels=True'):
        DeviceFeaturePool('cpu', soft_labels=True).add(dataset(soft))
    # the budget counts the soft rows: what fits without them does not fit with them
    need = rows * (IMG_DIM + 7) * 4
    DeviceFeaturePool('cpu', max_gb=(need + 8) / float(1 << 30)).add(dataset(soft))
    with pytest.raises(ValueError, match=r'%d bytes of region features needed' % (rows * (IMG_DIM + 7 + 12) * 4)):
        DeviceFeaturePool('cpu', max_gb=(need + 8) / float(1 << 30), soft_labels=True).add(dataset(soft, soft_labels=True))
    # without soft labels nothing changes
    old = DeviceMemeDataset(dataset(soft, soft_labels=True), DeviceFeaturePool('cpu'))
    assert old.label_dim is None and old.pool.soft is None and old.pool.resident_bytes == need
    # 8500 images x 36 regions x 1601 classes, as stored: under 2 GB
    assert 8500 * 36 * ((1601 + 3) // 4 * 4) * 4 < 2 * 10 ** 9


def test_the_loader_serves_the_mrc_tasks_with_resident_soft_labels_only(roots):
    plain, soft = roots
    without = DeviceMemeDataset(dataset(plain), DeviceFeaturePool('cpu'))
    with pytest.raises(ValueError, match=r"unknown task 'mrc' .*serves mlm, mrfr, itm; mrc and mrc-kl need .*soft_labels=True"):
        DevicePretrainLoader(without, 4, tasks=(('mlm', 1), ('mrc', 1)))
    with pytest.raises(ValueError, match='unknown task'):
        DevicePretrainLoader(without, 4, tasks=(('mrc-kl', 1),))
    assert data.PRETRAIN_TASKS == ('mlm', 'mrfr', 'itm') and data.MRC_TASKS == ('mrc', 'mrc-kl')
    with_soft = DeviceMemeDataset(dataset(soft, soft_labels=True), DeviceFeaturePool('cpu', soft_labels=True))
    loader = DevicePretrainLoader(with_soft, 4, tasks=(('mlm', 1), ('mrc', 2), ('mrc-kl', 1)), seed=3)
    assert loader.tasks == ['mlm', 'mrc', 'mrc-kl'] and len(loader) == 3 * 3
    with pytest.raises(ValueError, match=r"unknown task 'vqa' .*serves mlm, mrfr, itm, mrc, mrc-kl"):
        DevicePretrainLoader(with_soft, 4, tasks=(('vqa', 1),))
    # the generators: the old tasks keep 0, 1, 2, the new ones take 3 and 4, the task choice keeps [seed, 3]
    for k, task in enumerate(('mlm', 'mrfr', 'itm', 'mrc', 'mrc-kl')):
        assert np.array_equal(DevicePretrainLoader.task_rng(3, task).permutation(50), np.random.default_rng([3, k]).permutation(50))
    assert loader._task_rng.integers(1 << 30) == np.random.default_rng([3, 3]).integers(1 << 30)
    assert np.array_equal(loader.order('mrc'), np.random.default_rng([3, 3]).permutation(N))
