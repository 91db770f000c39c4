"""The numpy restatement of uniter_collate_pretrain_batch (tests/pretrain_collate_ref.py) and the host functions of the pretraining
loader (data.itm_pairs, data.plan_pretrain_batches) check themselves, without a GPU."""
import numpy as np
import pytest

from pretrain_collate_ref import DEFAULT_CFG, mlm_sample, mrfr_sample, pretrain_collate_ref

CLS, SEP, PAD, MASK = 101, 102, 0, 103
ARRAY_KEYS = ('feat', 'pos', 'row_start', 'row_cnt', 'input_ids', 'token_type_ids', 'txt_len', 'labels', 'ids')


def dataset(N=9, T=12, R=6, D=4, seed=0):
    """N samples: texts [CLS] words [SEP] [PAD].. of every length from 2 ([CLS] [SEP] alone) to T, region counts 0 .. R"""
    rng = np.random.default_rng(seed)
    txt_len = np.array([2 + (i * 5) % (T - 1) for i in range(N)], np.int32)
    txt_len[0], txt_len[1] = 2, T
    input_ids = np.zeros((N, T), np.int64)
    for i, tl in enumerate(txt_len):
        input_ids[i, :tl] = [CLS] + list(rng.integers(1000, 28996, tl - 2)) + [SEP]
    cnt = np.array([(i * 3) % (R + 1) for i in range(N)], np.int32)
    cnt[0], cnt[1], cnt[2] = R, 0, 1
    row_start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    rows = int(cnt.sum())
    return {'feat': rng.standard_normal((rows, D)).astype(np.float32), 'pos': rng.random((rows, 7)).astype(np.float32),
            'row_start': row_start, 'row_cnt': cnt, 'input_ids': input_ids, 'token_type_ids': None, 'txt_len': txt_len,
            'labels': rng.integers(0, 2, N).astype(np.int64), 'ids': np.arange(N, dtype=np.int64) + 500}


def run(task, a, sel, txt_sel=None, ragged=True, **cfg):
    sel = np.asarray(sel)
    ts = sel if txt_sel is None else np.asarray(txt_sel)
    R = int(a['row_cnt'][sel].max())
    L_out = int((a['txt_len'][ts] + (a['row_cnt'][sel] if ragged else R)).max())
    return pretrain_collate_ref(task, sel, txt_sel, *[a[k] for k in ARRAY_KEYS], R=R, L_out=L_out, ragged=ragged, cfg=cfg)


def test_mlm_invariants():
    a = dataset()
    sel = [3, 0, 1, 8, 2]
    for prob in (0.0, 0.15, 0.5, 1.0):
        out = run('mlm', a, sel, prob=prob, seed=11)
        n = 0
        for b, s in enumerate(sel):
            src, got, lab = a['input_ids'][s], out['input_ids'][b], out['txt_labels'][b]
            chosen = lab != -1
            assert chosen.sum() >= 1                                          # every sample has at least one selection
            assert np.array_equal(lab[chosen], src[chosen]) and np.array_equal(got[~chosen], src[~chosen])
            special = np.isin(src, (CLS, SEP, PAD))
            forced = not (chosen & ~special).any()
            if forced:                                                        # position 1, literally, whatever it holds
                assert chosen.sum() == 1 and chosen[1] and got[1] == MASK
            else:
                assert not (chosen & special).any()
            assert all(g == x or g == MASK or 1000 <= g < 28996 for g, x in zip(got[chosen], src[chosen]))
            n += int(chosen.sum())
        assert out['n_masked'] == n == len(out['masked_positions'])
        mp = out['masked_positions']
        assert all(tuple(mp[i]) < tuple(mp[i + 1]) for i in range(n - 1))     # strictly increasing in (b, position)
        assert all(out['txt_labels'][b, t] != -1 for b, t in mp)
    # a text of [CLS] [SEP] only: position 1 is [SEP] and is taken
    out = run('mlm', a, [0], prob=1.0)
    assert out['txt_labels'][0].tolist()[:3] == [-1, SEP, -1] and out['input_ids'][0, 1] == MASK


def test_mrfr_invariants():
    a = dataset()
    sel = [0, 1, 2, 5, 7]
    for ragged in (False, True):
        for prob in (0.0, 0.15, 1.0):
            out = run('mrfr', a, sel, ragged=ragged, prob=prob, seed=4)
            rows = []
            for b, s in enumerate(sel):
                n, tl = int(a['row_cnt'][s]), int(a['txt_len'][s])
                m = out['img_masks'][b]
                assert set(m.tolist()) <= {0, 1} and not m[n:].any() and (m.sum() >= 1) == (n > 0)
                tgt = np.zeros(out['img_mask_tgt'].shape[1], bool)
                tgt[tl:tl + n] = m[:n].astype(bool)
                assert np.array_equal(out['img_mask_tgt'][b], tgt)
                for r in range(n):
                    src = a['feat'][a['row_start'][s] + r]
                    assert np.array_equal(out['img_feat'][b, r], np.zeros_like(src) if m[r] else src)
                    assert np.array_equal(out['img_pos_feat'][b, r], a['pos'][a['row_start'][s] + r])
                    if m[r]:
                        rows.append(((b, tl + r), src))
            assert out['n_masked'] == len(rows)
            assert [tuple(p) for p in out['masked_positions']] == [p for p, _ in rows]
            assert np.array_equal(out['feat_targets'], np.asarray([f for _, f in rows], np.float32).reshape(-1, a['feat'].shape[1]))
            if prob == 0.0:
                assert out['n_masked'] == sum(1 for s in sel if a['row_cnt'][s] > 0)
            if prob == 1.0:
                assert out['n_masked'] == int(a['row_cnt'][sel].sum())


def test_probability_endpoints_do_not_depend_on_the_generator():
    a = dataset()
    sel = [4, 0, 1, 6]
    for task, keys in (('mlm', ('txt_labels', 'masked_positions')), ('mrfr', ('img_masks', 'img_mask_tgt', 'masked_positions'))):
        for prob in (0.0, 1.0):
            if task == 'mrfr' and prob == 0.0:
                continue                     # the forced region is drawn
            one, two = run(task, a, sel, prob=prob, seed=1, draw=0), run(task, a, sel, prob=prob, seed=2 ** 40 + 9, draw=3)
            for k in keys:
                assert np.array_equal(one[k], two[k]), (task, prob, k)
    out = run('mlm', a, sel, prob=0.0)
    assert [tuple(p) for p in out['masked_positions']] == [(b, 1) for b in range(len(sel))]          # exactly the forced one
    assert np.array_equal(out['input_ids'][:, 1], np.full(len(sel), MASK))
    out = run('mlm', a, sel, prob=1.0)
    eligible = ~np.isin(a['input_ids'][sel], (CLS, SEP, PAD))
    eligible[1, 1] = True                    # sample 0 is [CLS] [SEP]: nothing eligible, position 1 forced
    assert np.array_equal(out['txt_labels'] != -1, eligible)
    out = run('mrfr', a, sel, prob=0.0, seed=5)
    assert (out['img_masks'].sum(1) == (a['row_cnt'][sel] > 0)).all()                                 # one forced region per sample


def test_a_mask_depends_on_the_sample_not_on_the_batch():
    a = dataset()
    cfg = dict(prob=0.3, seed=77)
    for task, key in (('mlm', 'txt_labels'), ('mrfr', 'img_masks')):
        one = run(task, a, [3, 5, 8, 0], **cfg)
        two = run(task, a, [0, 7, 5], **cfg)                  # other neighbours, other slots
        for s, b1, b2 in ((5, 1, 2), (0, 3, 0)):
            w = int(a['row_cnt'][s]) if task == 'mrfr' else one[key].shape[1]      # (img_masks is R wide, R the batch's)
            assert np.array_equal(one[key][b1, :w], two[key][b2, :w]), (task, s)
        if task == 'mlm':
            assert np.array_equal(one['input_ids'][1], two['input_ids'][2])
        other = run(task, a, [3, 5, 8, 0], draw=1, **cfg)
        assert not np.array_equal(one[key], other[key]), task
    # the text's owner keys a token's draw: sample 5's text is masked alike wherever it is paired
    own, paired = run('mlm', a, [5], **cfg), run('mlm', a, [2], txt_sel=[5], **cfg)
    assert np.array_equal(own['txt_labels'], paired['txt_labels']) and np.array_equal(own['input_ids'], paired['input_ids'])
    assert paired['ids'][0] == a['ids'][2]


def test_itm_targets_and_text_source():
    a = dataset()
    out = run('itm', a, [1, 4, 6, 2], txt_sel=[1, 7, 6, 0])
    assert out['targets'].tolist() == [1, 0, 1, 0]
    assert np.array_equal(out['input_ids'], a['input_ids'][[1, 7, 6, 0]]) and np.array_equal(out['ids'], a['ids'][[1, 4, 6, 2]])
    assert run('itm', a, [1, 4])['targets'].tolist() == [1, 1]
    tl, n = a['txt_len'][[1, 7, 6, 0]], a['row_cnt'][[1, 4, 6, 2]]
    assert np.array_equal(out['attn_masks'].sum(1), (tl + n).astype(np.float32))


FREQ_SEED = 2024


def test_frequencies_guard_the_sense_of_the_thresholds():
    """64 samples x 128 eligible tokens at FREQ_SEED: the selected share within 5 binomial standard deviations of 0.15 (+- 0.02 from
    sqrt(0.15 * 0.85 / 8192)), the 80 / 10 / 10 split of the selected within 5 standard deviations for its count.  A seed for which
    the restatement passes; the condition guards the thresholds' sense (0.15 against 0.85, 80 % [MASK] against 80 % kept)."""
    rng = np.random.default_rng(0)
    cfg = dict(DEFAULT_CFG, seed=FREQ_SEED)
    kinds = []
    for s in range(64):
        _, _, kind = mlm_sample(rng.integers(1000, 28996, 128), s, cfg)
        kinds += kind
    total = len(kinds)
    chosen = sum(1 for k in kinds if k)
    assert total == 8192 and 'forced' not in kinds
    assert abs(chosen / total - 0.15) <= 5 * np.sqrt(0.15 * 0.85 / total)
    for kind, share in (('mask', 0.8), ('random', 0.1), ('keep', 0.1)):
        got = sum(1 for k in kinds if k == kind)
        assert abs(got - share * chosen) <= 5 * np.sqrt(share * (1 - share) * chosen), (kind, got, chosen)
    regions = sum(sum(mrfr_sample(128, s, cfg)) for s in range(64))
    assert abs(regions / total - 0.15) <= 5 * np.sqrt(0.15 * 0.85 / total)


# ---- host functions ------------------------------------------------------------------------------------------------------
def test_itm_pairs():
    from meme_challenge_amd.data import itm_pairs
    text_class = np.array([0, 1, 2, 0, 1, 3, 3, 3, 4, 0] * 40, np.int32)         # 400 samples, shared texts
    order = np.random.default_rng(1).permutation(len(text_class))
    for p in (0.0, 0.3, 0.5, 1.0):
        txt = itm_pairs(order, text_class, p, np.random.default_rng(7))
        assert txt.dtype == np.int64 and txt.shape == order.shape and txt.min() >= 0 and txt.max() < len(text_class)
        replaced = txt != order
        assert (text_class[txt[replaced]] != text_class[order[replaced]]).all()        # a replaced text always differs
        assert abs(replaced.mean() - p) <= 5 * np.sqrt(p * (1 - p) / len(order))
        assert np.array_equal(txt, itm_pairs(order, text_class, p, np.random.default_rng(7)))      # deterministic per seed
    assert not np.array_equal(itm_pairs(order, text_class, 0.5, np.random.default_rng(7)),
                              itm_pairs(order, text_class, 0.5, np.random.default_rng(8)))
    one_text = np.zeros(50, np.int32)
    assert np.array_equal(itm_pairs(np.arange(50), one_text, 1.0, np.random.default_rng(0)), np.arange(50))      # keeps all
    assert itm_pairs(np.zeros(0, np.int64), text_class, 0.5, np.random.default_rng(0)).size == 0


@pytest.mark.parametrize('ragged', [False, True])
def test_plan_pretrain_batches(ragged):
    from meme_challenge_amd.data import plan_batches, plan_pretrain_batches
    rng = np.random.default_rng(3)
    txt_len, row_cnt = rng.integers(2, 40, 57).astype(np.int32), rng.integers(0, 37, 57).astype(np.int32)
    order = rng.permutation(57)
    assert plan_pretrain_batches(order, order, 8, txt_len, row_cnt, ragged) == plan_batches(order, 8, txt_len, row_cnt, ragged)
    txt_order = rng.permutation(57)
    plan = plan_pretrain_batches(order, txt_order, 8, txt_len, row_cnt, ragged)
    assert [(a, b) for a, b, _, _, _ in plan] == [(a, min(a + 8, 57)) for a in range(0, 57, 8)]
    for a, b, R, L_out, seq in plan:
        n, tl = row_cnt[order[a:b]].astype(int), txt_len[txt_order[a:b]].astype(int)
        assert R == n.max() and seq == list(tl + (n if ragged else R)) and L_out == max(seq)
    with pytest.raises(ValueError):
        plan_pretrain_batches(order, txt_order[:5], 8, txt_len, row_cnt, ragged)
