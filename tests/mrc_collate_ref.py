"""numpy restatement of uniter_collate_mrc_batch (include/uniter_hip.h), element by element, from the header's words: MRFR's dense
outputs drawn on UNITER_STREAM_MRC, and per selected region its soft-label row and 1 + the first maximum of the row's columns
1 .. C-1.  The stream and the probability rule are those of tests/pretrain_collate_ref.py; it shares no code with the kernel or
with data.py."""
import numpy as np

from pretrain_collate_ref import DEFAULT_CFG, words, with_probability

STREAM_MRC = 0xFFFF0004


def mrc_sample(n, s, cfg):
    """the region mask of dataset sample s with n regions -> list of n bools"""
    mask = [with_probability(cfg['prob'], x) for x in words(range(n), s, STREAM_MRC, cfg)[0]]
    if n > 0 and not any(mask):
        mask[mrc_forced(n, s, cfg)] = True
    return mask


def mrc_forced(n, s, cfg):
    """the region a sample without a drawn one takes"""
    return (words([0xFFFFFFFF], s, STREAM_MRC, cfg)[0][0] * n) >> 32


def hard_label(row):
    """1 + index of the first maximum of row[1:], as torch.max / uniter_row_argmax(c0 = 1): NaN never wins, 1 without a winner"""
    if not np.isnan(row[1:]).any():
        return 1 + int(np.argmax(row[1:]))             # numpy's first maximum; all -inf: column 0 of the slice
    best, at = -np.inf, 1
    for c in range(1, len(row)):
        if row[c] > best:
            best, at = row[c], c
    return at


def mrc_collate_ref(sel, feat, pos, soft, C, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids, R, L_out, ragged,
                    cfg=None):
    """soft: [pool_rows, ld_soft >= C].  -> dict of numpy arrays: the common keys (attn_masks, sic), img_masks, img_mask_tgt, and
    masked_positions [n, 2], label_targets [n, C], label_ids [n], n_masked holding the defined rows only.  A pool row outside the
    pool reads as padding (features) and as a zero row (soft labels), as the header says."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    sel = np.asarray(sel, dtype=np.int64)
    B, T, D = len(sel), input_ids.shape[1], feat.shape[1]
    rows = feat.shape[0]
    out = {'img_feat': np.zeros((B, R, D), np.float32), 'img_pos_feat': np.zeros((B, R, 7), np.float32),
           'input_ids': np.zeros((B, T), np.int64), 'position_ids': np.zeros((B, T), np.int64),
           'token_type_ids': None if token_type_ids is None else np.zeros((B, T), np.int64),
           'attn_masks': np.zeros((B, L_out), np.float32), 'gather_index': np.zeros((B, L_out), np.int64),
           'labels': np.zeros(B, np.int64), 'ids': np.zeros(B, np.int64),
           'img_masks': np.zeros((B, R), np.int64), 'img_mask_tgt': np.zeros((B, L_out), np.bool_)}
    positions, targets, hard = [], [], []
    for b, s in enumerate(sel):
        n, tl = min(max(int(row_cnt[s]), 0), R), int(txt_len[s])
        il = n if ragged else R
        mask = mrc_sample(n, int(s), cfg)
        for r in range(n):
            src = int(row_start[s]) + r
            real = 0 <= src < rows
            if real:
                out['img_pos_feat'][b, r] = pos[src]
            if mask[r]:
                out['img_masks'][b, r] = 1
                out['img_mask_tgt'][b, tl + r] = True
                positions.append((b, tl + r))
                row = np.array(soft[src, :C], np.float32) if real else np.zeros(C, np.float32)
                targets.append(row)
                hard.append(hard_label(row))
            elif real:
                out['img_feat'][b, r] = feat[src]
        out['input_ids'][b] = input_ids[s]
        if token_type_ids is not None:
            out['token_type_ids'][b] = token_type_ids[s]
        out['position_ids'][b] = np.arange(T)
        for j in range(L_out):
            out['attn_masks'][b, j] = 1.0 if j < tl + il else 0.0
            out['gather_index'][b, j] = j - tl + T if tl <= j < tl + il else j
        out['labels'][b], out['ids'][b] = labels[s], ids[s]
    out['masked_positions'] = np.asarray(positions, np.int64).reshape(-1, 2)
    out['n_masked'] = len(positions)
    out['label_targets'] = np.asarray(targets, np.float32).reshape(-1, C)
    out['label_ids'] = np.asarray(hard, np.int64).reshape(-1)
    return out
