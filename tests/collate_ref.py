"""numpy restatement of uniter_collate_batch (include/uniter_hip.h): one batch of data.MemeDataset.get_collate_fn()
(compact_batch = True) from the arrays of a resident dataset.  Written from the header's semantics, element by element, so it
shares no code with the kernel or with the torch collate; tests/test_device_dataset_cpu.py pins it on that collate."""
import numpy as np


def collate_ref(sel, feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids, R, L_out, ragged):
    """-> dict of numpy arrays with the host collate's tensor keys (token_type_ids None when the dataset has none)."""
    sel = np.asarray(sel, dtype=np.int64)
    B, T, D = len(sel), input_ids.shape[1], feat.shape[1]
    out = {'img_feat': np.zeros((B, R, D), np.float32), 'img_pos_feat': np.zeros((B, R, 7), np.float32),
           'input_ids': np.zeros((B, T), np.int64), 'position_ids': np.zeros((B, T), np.int64),
           'token_type_ids': None if token_type_ids is None else np.zeros((B, T), np.int64),
           'attn_mask': np.zeros((B, L_out), np.float32), 'gather_index': np.zeros((B, L_out), np.int64),
           'labels': np.zeros(B, np.int64), 'ids': np.zeros(B, np.int64)}
    for b, s in enumerate(sel):
        n, tl = int(row_cnt[s]), int(txt_len[s])
        il = n if ragged else R
        for r in range(n):
            out['img_feat'][b, r] = feat[row_start[s] + r]
            out['img_pos_feat'][b, r] = pos[row_start[s] + r]
        out['input_ids'][b] = input_ids[s]
        if token_type_ids is not None:
            out['token_type_ids'][b] = token_type_ids[s]
        out['position_ids'][b] = np.arange(T)
        for j in range(L_out):
            out['attn_mask'][b, j] = 1.0 if j < tl + il else 0.0
            out['gather_index'][b, j] = j - tl + T if tl <= j < tl + il else j
        out['labels'][b], out['ids'][b] = labels[s], ids[s]
    return out


def arrays_of(dataset, order=None):
    """The resident form of a data.MemeDataset as numpy arrays, built the slow way (one __getitem__ and one tokenizer call per
    sample): (feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids).  `order`: the pool order of the
    samples' rows (default: sample order)."""
    n = len(dataset)
    samples = [dataset[i] for i in range(n)]
    order = list(range(n)) if order is None else list(order)
    row_start, at = np.zeros(n, np.int64), 0
    for s in order:
        row_start[s] = at
        at += samples[s]['img_feat'].shape[0]
    feat = np.concatenate([samples[s]['img_feat'].numpy() for s in order]).astype(np.float32)
    pos = np.concatenate([samples[s]['img_pos_feat'].numpy() for s in order]).astype(np.float32)
    row_cnt = np.array([s['img_feat'].shape[0] for s in samples], np.int32)
    toks = [dataset.text_padding([s['text']]) for s in samples]
    input_ids = np.concatenate([t['input_ids'].numpy() for t in toks]).astype(np.int64)
    tt = None
    if toks[0].get('token_type_ids') is not None:
        tt = np.concatenate([t['token_type_ids'].numpy() for t in toks]).astype(np.int64)
    txt_len = np.array([int(t['length'][0]) for t in toks], np.int32)
    return (feat, pos, row_start, row_cnt, input_ids, tt, txt_len, dataset.data.labels.numpy().astype(np.int64),
            dataset.data.ids.numpy().astype(np.int64))
