"""numpy restatement of uniter_collate_pretrain_batch (include/uniter_hip.h), element by element, from the header's words: the
copy of uniter_collate_batch with the text of sample txt_sel[b], the MLM / MRFR masks from the Philox stream the header
specifies (oracle.philox.philox4x32_10) and their row-major compaction.  It shares no code with the kernel or with data.py."""
import numpy as np

from oracle.philox import philox4x32_10

STREAM_MLM, STREAM_MRFR = 0xFFFF0001, 0xFFFF0002
TWO32 = 4294967296
KEEP80, KEEP90 = 3435973836, 3865470566           # floor(0.8 * 2^32), floor(0.9 * 2^32)
assert (KEEP80, KEEP90) == (int(np.floor(0.8 * TWO32)), int(np.floor(0.9 * TWO32)))

DEFAULT_CFG = dict(seed=0, draw=0, prob=0.15, cls=101, sep=102, pad=0, mask_token=103, vocab_lo=1000, vocab_hi=28996)


def words(position, sample, stream, cfg):
    """w = philox4x32_10(c0 = position, c1 = lo32(sample), c2 = stream id, c3 = draw, key = (lo32(seed), hi32(seed))) for every
    position of the list -> four lists (x, y, z, w) of Python ints"""
    seed = int(cfg['seed'])
    c0 = np.asarray([int(p) & 0xFFFFFFFF for p in position], dtype=np.uint64)
    w = philox4x32_10(c0, np.uint64(int(sample) & 0xFFFFFFFF), np.uint64(stream), np.uint64(int(cfg['draw']) & 0xFFFFFFFF),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [[int(v) for v in x] for x in w]


def with_probability(p, word):
    """p >= 1 || word < floor(p * 2^32), p being the float the configuration struct holds"""
    p = float(np.float32(p))
    return p >= 1.0 or word < int(np.floor(p * TWO32))


def mlm_sample(tokens, ts, cfg):
    """get_masked_txt for the tokens of dataset sample ts -> (tokens after masking, labels, what happened per token: '' / 'mask' /
    'random' / 'keep' / 'forced')"""
    tokens = [int(t) for t in tokens]
    out, labels, kind = list(tokens), [-1] * len(tokens), [''] * len(tokens)
    xs, ys, zs, _ = words(range(len(tokens)), ts, STREAM_MLM, cfg)
    for t, tok in enumerate(tokens):
        if tok in (cfg['cls'], cfg['sep'], cfg['pad']):
            continue
        x, y, z = xs[t], ys[t], zs[t]
        if not with_probability(cfg['prob'], x):
            continue
        labels[t] = tok
        if y < KEEP80:
            out[t], kind[t] = cfg['mask_token'], 'mask'
        elif y < KEEP90:
            out[t], kind[t] = cfg['vocab_lo'] + ((z * (cfg['vocab_hi'] - cfg['vocab_lo'])) >> 32), 'random'
        else:
            kind[t] = 'keep'
    if all(k == '' for k in kind):
        labels[1], out[1], kind[1] = tokens[1], cfg['mask_token'], 'forced'
    return out, labels, kind


def mrfr_sample(n, s, cfg):
    """_get_img_mask for the n regions of dataset sample s -> list of n bools"""
    mask = [with_probability(cfg['prob'], x) for x in words(range(n), s, STREAM_MRFR, cfg)[0]]
    if n > 0 and not any(mask):
        mask[(words([0xFFFFFFFF], s, STREAM_MRFR, cfg)[0][0] * n) >> 32] = True
    return mask


def pretrain_collate_ref(task, sel, txt_sel, feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids, R, L_out,
                         ragged, cfg=None):
    """-> dict of numpy arrays: the common keys (attn_masks, sic), the task's keys, and for mlm / mrfr masked_positions [n, 2],
    n_masked and (mrfr) feat_targets [n, D] holding the defined rows only."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    sel = np.asarray(sel, dtype=np.int64)
    txt_sel = sel if txt_sel is None else np.asarray(txt_sel, dtype=np.int64)
    B, T, D = len(sel), input_ids.shape[1], feat.shape[1]
    out = {'img_feat': np.zeros((B, R, D), np.float32), 'img_pos_feat': np.zeros((B, R, 7), np.float32),
           'input_ids': np.zeros((B, T), np.int64), 'position_ids': np.zeros((B, T), np.int64),
           'token_type_ids': None if token_type_ids is None else np.zeros((B, T), np.int64),
           'attn_masks': np.zeros((B, L_out), np.float32), 'gather_index': np.zeros((B, L_out), np.int64),
           'labels': np.zeros(B, np.int64), 'ids': np.zeros(B, np.int64)}
    positions, targets = [], []
    if task == 'mlm':
        out['txt_labels'] = np.full((B, T), -1, np.int64)
    elif task == 'mrfr':
        out['img_masks'] = np.zeros((B, R), np.int64)
        out['img_mask_tgt'] = np.zeros((B, L_out), np.bool_)
    elif task == 'itm':
        out['targets'] = np.zeros(B, np.int64)
    else:
        raise ValueError(task)
    for b, (s, ts) in enumerate(zip(sel, txt_sel)):
        n, tl = int(row_cnt[s]), int(txt_len[ts])
        il = n if ragged else R
        mask = mrfr_sample(n, int(s), cfg) if task == 'mrfr' else [False] * n
        for r in range(n):
            out['img_pos_feat'][b, r] = pos[row_start[s] + r]
            if mask[r]:
                out['img_masks'][b, r] = 1
                out['img_mask_tgt'][b, tl + r] = True
                positions.append((b, tl + r))
                targets.append(feat[row_start[s] + r])
            else:
                out['img_feat'][b, r] = feat[row_start[s] + r]
        if task == 'mlm':
            toks, labs, _ = mlm_sample(input_ids[ts], int(ts), cfg)
            out['input_ids'][b], out['txt_labels'][b] = toks, labs
            positions += [(b, t) for t in range(T) if labs[t] != -1]
        else:
            out['input_ids'][b] = input_ids[ts]
        if token_type_ids is not None:
            out['token_type_ids'][b] = token_type_ids[ts]
        out['position_ids'][b] = np.arange(T)
        for j in range(L_out):
            out['attn_masks'][b, j] = 1.0 if j < tl + il else 0.0
            out['gather_index'][b, j] = j - tl + T if tl <= j < tl + il else j
        out['labels'][b], out['ids'][b] = labels[s], ids[s]
        if task == 'itm':
            out['targets'][b] = 1 if ts == s else 0
    if task != 'itm':
        out['masked_positions'] = np.asarray(positions, np.int64).reshape(-1, 2)
        out['n_masked'] = len(positions)
    if task == 'mrfr':
        out['feat_targets'] = np.asarray(targets, np.float32).reshape(-1, D)
    return out
