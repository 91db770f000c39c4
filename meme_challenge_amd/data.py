"""Input side of the hot path: the batch dict the model consumes.

Counterpart of data/dataset_template.py:92-114 (`_load_img_feature`: `<id>.npy` fp32
[nbb,2048] + `<id>_info.npy` pickled dict with bbox / image_width / image_height / objects /
objects_conf|cls_prob -> 7-d box features (x1,y1,x2,y2,w,h,w*h), normalised), of
data/meme_dataset.py:27-214 (jsonl list, `__getitem__`, `collate_fn` with compact batches) and
of `ConfounderSampler` (:221-271).  Same file formats, same batch keys:
  input_ids, position_ids, img_feat, img_pos_feat, token_type_ids, attn_mask, gather_index,
  labels, ids.
"""
import ctypes as C
import json
import os
from itertools import chain
from random import shuffle
from types import SimpleNamespace

import numpy as np
import torch
import torch.utils.data as data
from torch.nn.utils.rnn import pad_sequence

from . import _lib
from .utils import get_attention_mask, get_gather_index


def expand_id(img_id):
    return str(img_id).zfill(5)


def load_img_feature(feature_dir, img_id, normalize=True):
    """-> (feat [nbb, D] fp32, pos [nbb, 7] fp32, objects, objects_conf)"""
    sid = expand_id(img_id)
    feat = torch.from_numpy(np.load(os.path.join(feature_dir, '%s.npy' % sid)))
    info = np.load(os.path.join(feature_dir, '%s_info.npy' % sid), allow_pickle=True).item()
    x1, y1, x2, y2 = [c.astype(np.float32).copy() for c in np.split(info['bbox'], 4, axis=1)]
    conf = info['objects_conf'] if 'objects_conf' in info else info['cls_prob'].max(axis=-1)
    if normalize:
        x1 /= info['image_width']; x2 /= info['image_width']
        y1 /= info['image_height']; y2 /= info['image_height']
    w, h = x2 - x1, y2 - y1
    pos = torch.from_numpy(np.concatenate((x1, y1, x2, y2, w, h, w * h), axis=1).astype(np.float32))
    return feat.float(), pos, info['objects'], conf


def load_soft_labels(feature_dir, img_id):
    """-> the detector's class distribution of every region, `cls_prob` of `<id>_info.npy`, fp32 [nbb, C] (column 0 is the
    background): the `label_targets` of masked region classification, which load_img_feature reduces to one confidence."""
    path = os.path.join(feature_dir, '%s_info.npy' % expand_id(img_id))
    info = np.load(path, allow_pickle=True).item()
    if 'cls_prob' not in info:
        raise ValueError('%s has no cls_prob: soft labels need the detector\'s class distribution per region' % path)
    soft = np.asarray(info['cls_prob'], dtype=np.float32)
    if soft.ndim != 2:
        raise ValueError('%s: cls_prob must be [nbb, C]; got %s' % (path, soft.shape))
    return torch.from_numpy(np.ascontiguousarray(soft))


# ---- packed feature shard -------------------------------------------------------
# At >1000 samples/s per GPU the per-sample `<id>.npy` + pickled `<id>_info.npy` pair (two opens, one
# unpickle, 295 KB) is the input bottleneck.  A shard is the same data laid out for streaming: one
# fp32 matrix of all region features, one of the 7-d box features already computed as
# load_img_feature does, one of the detector confidences, and an index; all memory-mapped, so a
# sample is two slices of page cache and DataLoader workers share the pages.
SHARD_MAGIC = 'uniter-feature-shard-v1'


def build_feature_shard(feature_dir, img_ids, out_prefix, normalize=True):
    """Pack the reference-format feature files of `img_ids` into `<out_prefix>.{feat,pos,conf}.npy` +
    `<out_prefix>.index.json`.  Returns the index dict."""
    ids = [int(i) for i in img_ids]
    loaded = [load_img_feature(feature_dir, i, normalize=normalize) for i in ids]
    counts = [int(f.shape[0]) for f, _, _, _ in loaded]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    dim = int(loaded[0][0].shape[1]) if loaded else 0
    feat = np.lib.format.open_memmap(out_prefix + '.feat.npy', mode='w+', dtype=np.float32, shape=(int(offs[-1]), dim))
    pos = np.lib.format.open_memmap(out_prefix + '.pos.npy', mode='w+', dtype=np.float32, shape=(int(offs[-1]), 7))
    conf = np.lib.format.open_memmap(out_prefix + '.conf.npy', mode='w+', dtype=np.float32, shape=(int(offs[-1]),))
    for k, (f, p, _, c) in enumerate(loaded):
        feat[offs[k]:offs[k + 1]] = f.numpy()
        pos[offs[k]:offs[k + 1]] = p.numpy()
        conf[offs[k]:offs[k + 1]] = np.asarray(c, dtype=np.float32).reshape(-1)
    for a in (feat, pos, conf):
        a.flush()
    index = {'magic': SHARD_MAGIC, 'ids': ids, 'offsets': offs.tolist(), 'dim': dim, 'normalize': bool(normalize)}
    with open(out_prefix + '.index.json', 'w') as f:
        json.dump(index, f)
    return index


class FeatureShard(object):
    """Read side of build_feature_shard: `shard[img_id] -> (feat [nbb, D], pos [nbb, 7], conf [nbb])` as torch
    views of the memory map (zero copy until collate pads them)."""

    def __init__(self, prefix):
        with open(prefix + '.index.json') as f:
            idx = json.load(f)
        if idx.get('magic') != SHARD_MAGIC:
            raise ValueError('%s.index.json is not a feature shard' % prefix)
        self.offsets = np.asarray(idx['offsets'], dtype=np.int64)
        self.row = {int(i): k for k, i in enumerate(idx['ids'])}
        self.feat = np.load(prefix + '.feat.npy', mmap_mode='r')
        self.pos = np.load(prefix + '.pos.npy', mmap_mode='r')
        self.conf = np.load(prefix + '.conf.npy', mmap_mode='r')

    def __contains__(self, img_id):
        return int(img_id) in self.row

    def __getitem__(self, img_id):
        k = self.row[int(img_id)]
        a, b = int(self.offsets[k]), int(self.offsets[k + 1])
        # np.array(copy) of a contiguous slice: one memcpy out of the page cache, then an owned tensor
        return (torch.from_numpy(np.array(self.feat[a:b])), torch.from_numpy(np.array(self.pos[a:b])),
                np.array(self.conf[a:b]))


class DevicePrefetcher(object):
    """Iterates a DataLoader one batch ahead: batch i+1 is copied to the GPU on a side stream (from the
    loader's pinned buffers, non-blocking) while step i computes, so the hot path never waits for PCIe.
    Non-tensor entries (seq_lens lists, None) pass through."""

    def __init__(self, loader, device, threaded=None, depth=3):
        """threaded (round 6; None: on unless UNITER_PREFETCH_THREAD=0): the loader's own work -- reading the feature files and the
        collate of data/meme_dataset.py:152-214, 2.3 ms per batch of configs[1] with --num_workers 0 -- runs in a background thread, up
        to `depth` batches ahead, instead of between two steps on the thread that launches the kernels: with a 4.4-ms bf16 step the
        launching thread had 2 ms of it taken away every iteration (the CLI ran at 72-80 % of the bare step's rate)."""
        self.loader, self.device = loader, torch.device(device)
        self.stream = _lib.shared_stream(self.device, 'copy')      # one copy stream per device, whatever the number of loaders
        self.threaded = (os.environ.get('UNITER_PREFETCH_THREAD', '1') != '0') if threaded is None else bool(threaded)
        self.depth = max(1, int(depth))

    def __len__(self):
        return len(self.loader)

    @property
    def dataset(self):
        return self.loader.dataset

    def _to_device(self, batch):
        with torch.cuda.stream(self.stream):
            return {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def _iter_threaded(self):
        import queue
        import threading
        q = queue.Queue(maxsize=self.depth)
        stop = threading.Event()

        def put(item):
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    continue
            return False

        # (the consuming thread's device: a new thread starts on device 0 whatever the caller selected)
        dev_index = (self.device.index if self.device.index is not None else torch.cuda.current_device()) if self.device.type == 'cuda' else None

        def work():
            try:
                if dev_index is not None:
                    torch.cuda.set_device(dev_index)
                for b in self.loader:
                    d = self._to_device(b)
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                    if not put((d, ev)):
                        return
                put(None)
            except BaseException as e:             # noqa: BLE001 -- handed to the consuming thread, which raises it
                put(e)

        t = threading.Thread(target=work, name='uniter-prefetch', daemon=True)
        t.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                cur, ev = item
                cs = torch.cuda.current_stream(self.device)
                cs.wait_event(ev)                                                 # cur's copies are done
                for v in cur.values():
                    if torch.is_tensor(v):
                        v.record_stream(cs)                                       # allocator: in use on the compute stream
                yield cur
        finally:
            stop.set()
            while not q.empty():
                try:
                    q.get_nowait()
                except queue.Empty:
                    break
            t.join(timeout=10)

    def __iter__(self):
        if self.threaded:
            yield from self._iter_threaded()
            return
        it = iter(self.loader)
        try:
            nxt = self._to_device(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur = nxt
            torch.cuda.current_stream(self.device).wait_stream(self.stream)       # cur's copies are done
            for v in cur.values():
                if torch.is_tensor(v):
                    v.record_stream(torch.cuda.current_stream(self.device))       # allocator: in use on the compute stream
            try:
                nxt = self._to_device(next(it))                                  # overlaps with the caller's step on `cur`
            except StopIteration:
                nxt = None
            yield cur


class MemeDataset(data.Dataset):
    def __init__(self, filepath, feature_dir=None, text_padding=None, return_ids=False, compact_batch=True,
                 confidence_threshold=0.0, preload_images=False, text_only=False, debug=False,
                 feature_shard=None, ragged_regions=False, soft_labels=False, **unused):
        """`soft_labels=True` adds 'img_soft_label' [kept, C] to every sample: the detector's class distribution of the regions
        the sample keeps (load_soft_labels), for masked region classification.  Feature shards carry no cls_prob and are refused.
        `ragged_regions=False` reproduces the reference's collate exactly: it measures the region count of every
        sample on the already zero-padded stack (data/meme_dataset.py:161,191), so every sample of a batch carries the
        batch's largest region count and the zero rows are attended like real regions (pinned by
        tests/golden/data_pipeline.npz).  True masks each sample at its own region count instead (what
        utils/utils.py:111-125 describes; fewer valid positions for token packing)."""
        self.ragged_regions = ragged_regions
        self.soft_labels = bool(soft_labels) and not text_only
        if self.soft_labels and feature_shard:
            raise ValueError('soft_labels=True needs the per-image feature files: the feature shard %s carries no cls_prob' % feature_shard)
        assert os.path.isfile(filepath), "Dataset file cannot be found: \"%s\"." % filepath
        assert filepath.endswith(".jsonl"), "The filepath requires a JSON list file (\".jsonl\")."
        self.filepath, self.feature_dir = filepath, feature_dir
        self.name = filepath.split("/")[-1].split(".")[0]
        self.text_padding, self.return_ids, self.compact_batch = text_padding, return_ids, compact_batch
        self.confidence_threshold, self.text_only = confidence_threshold, text_only
        with open(filepath, "r") as f:
            js = [json.loads(l) for l in f if l.strip()]
        self.data = SimpleNamespace(
            ids=torch.LongTensor([int(j["id"]) for j in js]),
            labels=torch.LongTensor([j.get("label", -1) for j in js]),
            text=[j["text"] for j in js],
            imgs=[os.path.join(os.path.dirname(filepath), j.get("img", "")) for j in js])
        self.feature_shard = feature_shard if not text_only else None
        self.shard = FeatureShard(feature_shard) if (feature_shard and not text_only) else None
        if not text_only:
            for i in self.data.ids.tolist():
                if self.shard is not None:
                    assert i in self.shard, "Image %d is not in the feature shard %s." % (i, feature_shard)
                    continue
                for suffix in ('.npy', '_info.npy'):
                    p = os.path.join(feature_dir, expand_id(i) + suffix)
                    assert os.path.isfile(p), "Feature file %s does not exist." % p
        self._cache = None
        if preload_images and not text_only:
            self._cache = [load_img_feature(feature_dir, i) for i in self.data.ids.tolist()]
            if self.soft_labels:
                self._soft_cache = [load_soft_labels(feature_dir, i) for i in self.data.ids.tolist()]

    def __len__(self):
        return len(self.data.ids)

    def __getitem__(self, idx):
        data_id, label = self.data.ids[idx], self.data.labels[idx]
        feat = pos = soft = None
        if not self.text_only:
            if self._cache is not None:
                feat, pos, _, conf = self._cache[idx]
            elif self.shard is not None:
                feat, pos, conf = self.shard[data_id.item()]
            else:
                feat, pos, _, conf = load_img_feature(self.feature_dir, data_id.item())
            if self.confidence_threshold > 0.0:
                keep = torch.from_numpy(np.asarray(conf) > self.confidence_threshold)
                feat, pos = feat[keep], pos[keep]
            if self.soft_labels:
                soft = self._soft_cache[idx] if self._cache is not None else load_soft_labels(self.feature_dir, data_id.item())
                if soft.shape[0] != conf.shape[0]:
                    raise ValueError('image %d: cls_prob has %d rows for %d regions' % (data_id.item(), soft.shape[0], conf.shape[0]))
                if self.confidence_threshold > 0.0:
                    soft = soft[keep]
        sample = {'img_feat': feat, 'img_pos_feat': pos, 'text': self.data.text[idx], 'label': label, 'data_id': data_id}
        if self.soft_labels:
            sample['img_soft_label'] = soft
        return sample

    def get_collate_fn(self):
        def collate_fn(samples):
            texts = self.text_padding([s['text'] for s in samples])
            input_ids = texts['input_ids']
            text_len = [int(x) for x in (texts['length'].tolist() if torch.is_tensor(texts['length'])
                                         else texts['length'])]
            B, T = input_ids.shape
            batch = {'input_ids': input_ids,
                     'position_ids': torch.arange(T, dtype=torch.long).unsqueeze(0).repeat(B, 1),
                     'token_type_ids': texts.get('token_type_ids') if hasattr(texts, 'get') else None,
                     'labels': torch.stack([s['label'] for s in samples]),
                     'ids': torch.stack([s['data_id'] for s in samples])}
            if self.text_only:
                batch.update(img_feat=None, img_pos_feat=None, attn_mask=texts['attention_mask'], gather_index=None)
                return batch
            img_feat = pad_sequence([s['img_feat'] for s in samples], batch_first=True, padding_value=0)
            img_pos = pad_sequence([s['img_pos_feat'] for s in samples], batch_first=True, padding_value=0)
            img_len = [s['img_feat'].size(0) for s in samples] if self.ragged_regions else [img_feat.size(1)] * B
            if self.compact_batch:
                attn = get_attention_mask(text_len, img_len)
            else:
                attn = torch.cat((texts['attention_mask'].float(), get_attention_mask([0] * B, img_len)), dim=1)
            gi = get_gather_index(text_len, img_len, B, T, attn.shape[1])
            batch.update(img_feat=img_feat, img_pos_feat=img_pos, attn_mask=attn, gather_index=gi)
            if self.compact_batch:
                # host-side lengths (extension): lets UniterModel.pack_padded skip a device->host copy
                batch['seq_lens'] = [int(t) + int(n) for t, n in zip(text_len, img_len)]
            return batch
        return collate_fn


class ConfounderSampler(data.Sampler):
    """Repeats the text confounders (same text, both labels) `repeat_factor` times per epoch
    (data/meme_dataset.py:221-271)."""

    def __init__(self, dataset, repeat_factor=1):
        self.dataset, self.repeat_factor = dataset, repeat_factor
        labels_of = {}
        for idx, text in enumerate(dataset.data.text):
            labels_of.setdefault(text, set()).add(int(dataset.data.labels[idx]))
        conf_text = {t for t, ls in labels_of.items() if ls == {0, 1}}
        self.confounders = [i for i, t in enumerate(dataset.data.text) if t in conf_text]
        self.non_confounders = [i for i, t in enumerate(dataset.data.text) if t not in conf_text]
        self._generate()

    def _generate(self):
        plain = self.non_confounders[:]
        shuffle(plain)
        n, k = len(plain), self.repeat_factor
        splits = [(n // k) * i for i in range(k)] + [n]
        out = []
        for i in range(k):
            sub = plain[splits[i]:splits[i + 1]] + self.confounders
            shuffle(sub)
            out += sub
        self.sample_list = out

    def __iter__(self):
        self._generate()
        return iter(self.sample_list)

    def __len__(self):
        return len(self.sample_list)


class HashTokenizer(object):
    """Offline stand-in for `BertTokenizer('bert-base-cased')` (which needs the hub): lower-cased
    whitespace tokens hashed into the vocabulary, [CLS]=101 / [SEP]=102 / [PAD]=0, same call
    signature and return fields as the partial built at train_uniter.py:124-126."""

    def __init__(self, vocab_size=28996, max_length=60):
        self.vocab_size, self.max_length = vocab_size, max_length

    def __call__(self, texts, **kw):
        T = kw.get('max_length', self.max_length)
        ids = torch.zeros(len(texts), T, dtype=torch.long)
        lens = []
        for b, t in enumerate(texts):
            toks = [101] + [1000 + (hash_str(w) % (self.vocab_size - 1000)) for w in str(t).lower().split()][:T - 2] + [102]
            ids[b, :len(toks)] = torch.tensor(toks)
            lens.append(len(toks))
        return {'input_ids': ids, 'length': torch.tensor(lens), 'attention_mask': (ids != 0).long(),
                'token_type_ids': torch.zeros_like(ids)}


def hash_str(s):
    h = 2166136261
    for c in s.encode('utf-8'):
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


def write_synthetic_dataset(root, n=64, num_bb=(10, 36), img_dim=2048, seed=0, splits=('train', 'dev_seen'), text_words=(3, 8),
                            label_dim=None):
    """Create a dataset in the reference's ON-DISK FORMAT (jsonl + per-image .npy feature files) with
    a learnable signal: label 1 memes have a shifted feature mean and contain a marker word.  text_words / num_bb: (min, max)
    words per caption and regions per image (BASELINE configs[1] shapes: text_words=(126, 126), num_bb=(36, 36)).  label_dim: every
    info dict also gets `cls_prob` [nbb, label_dim], a softmax of normals (strictly positive, rows summing to 1 up to fp32 rounding), from a
    generator of its own: every other field is bit-identical to the call without it."""
    rng = np.random.default_rng(seed)
    soft_rng = np.random.default_rng([seed, 1]) if label_dim is not None else None
    feat_dir = os.path.join(root, 'img_feats')
    os.makedirs(feat_dir, exist_ok=True)
    words = ['cat', 'dog', 'meme', 'funny', 'sky', 'tree', 'car', 'look', 'when', 'you', 'me', 'nobody']
    idx = 0
    for split in splits:
        with open(os.path.join(root, split + '.jsonl'), 'w') as f:
            for _ in range(n):
                label = int(rng.random() < 0.4)
                nbb = int(rng.integers(num_bb[0], num_bb[1] + 1))
                feat = np.abs(rng.standard_normal((nbb, img_dim))).astype(np.float32) + 0.5 * label
                W, H = 640, 480
                x1 = rng.random((nbb, 1)) * 0.7 * W; y1 = rng.random((nbb, 1)) * 0.7 * H
                bw = (rng.random((nbb, 1)) * 0.25 + 0.05) * W; bh = (rng.random((nbb, 1)) * 0.25 + 0.05) * H
                info = {'bbox': np.concatenate([x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32),
                        'image_width': W, 'image_height': H,
                        'objects': rng.integers(0, 1600, nbb), 'objects_conf': rng.random(nbb).astype(np.float32)}
                if soft_rng is not None:
                    z = soft_rng.standard_normal((nbb, int(label_dim)))
                    e = np.exp(z - z.max(axis=1, keepdims=True))
                    info['cls_prob'] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
                np.save(os.path.join(feat_dir, expand_id(idx) + '.npy'), feat)
                np.save(os.path.join(feat_dir, expand_id(idx) + '_info.npy'), info, allow_pickle=True)
                text = ' '.join(rng.choice(words, int(rng.integers(text_words[0], text_words[1] + 1)))) + (' hateful' if label else ' nice')
                f.write(json.dumps({'id': idx, 'img': 'img/%s.png' % expand_id(idx), 'label': label, 'text': text}) + '\n')
                idx += 1
    return feat_dir


# ---- device-resident dataset: batches collated on the GPU from HBM (csrc/collate.hip) ------------------------------
# Fifteen cross-validation folds of up to 30 epochs read the same ~10 000 memes; at --max_bb 100 every region feature of
# train + dev + test together is under 9 GB of fp32.  Held in HBM once per process, a batch is ONE launch from a device-side
# list of sample indices: no per-step host tensor work, no host -> device copy, no background thread, no worker processes.
# The batch is bit-identical to MemeDataset.get_collate_fn()'s for the same samples (tests/test_device_dataset_gpu.py).
_GB = float(1 << 30)


class DeviceFeaturePool(object):
    """The process-wide store of region rows on `device`: feat [rows, D] and pos [rows, 7], fp32, growing.  A sample is
    keyed by (feature source, image id, confidence threshold), so datasets that share images -- the fold files of a
    cross-validation run -- upload every image once.

    soft_labels=True keeps a third buffer beside them, soft [rows, ld_soft]: row i holds the detector's class distribution
    ('img_soft_label', C = label_dim columns) of the region of row i of feat.  ld_soft is C rounded up to a multiple of 4, so
    that with torch's 512-byte aligned allocations every row starts 16-byte aligned and uniter_collate_mrc_batch reads it as
    16-byte items (C = 1601: 1604 floats, 0.2 % more memory); the columns [C, ld_soft) are zero.  At 8500 images x 36 regions
    x 1601 classes that is 1.96 GB, counted by resident_bytes and the max_gb budget."""

    CHUNK_BYTES = 256 << 20          # host rows gathered before one upload (and one budget check)

    def __init__(self, device, max_gb=32.0, soft_labels=False):
        self.device = torch.device(device)
        self.max_bytes = int(float(max_gb) * _GB)
        self.soft_labels = bool(soft_labels)
        self.feat = self.pos = self.soft = None        # [capacity, D] / [capacity, 7] / [capacity, ld_soft]; rows [0, self.rows) are in use
        self.rows, self.dim = 0, None
        self.label_dim = self.ld_soft = None # C and the leading dimension of soft, from the first image
        self._where = {}                     # key -> (row_start, row_cnt)

    @property
    def resident_bytes(self):
        return 0 if self.dim is None else self.rows * self._row_floats() * 4

    def _row_floats(self):
        return self.dim + 7 + ((self.ld_soft or 0) if self.soft_labels else 0)

    @staticmethod
    def source_of(dataset):
        src = getattr(dataset, 'feature_shard', None) or dataset.feature_dir
        return os.path.abspath(str(src))

    def _reserve(self, rows):
        cap = -1 if self.feat is None else self.feat.shape[0]
        if rows <= cap:
            return
        new_cap = max(rows, cap + cap // 2)
        feat = torch.empty((new_cap, self.dim), dtype=torch.float32, device=self.device)
        pos = torch.empty((new_cap, 7), dtype=torch.float32, device=self.device)
        soft = torch.empty((new_cap, self.ld_soft), dtype=torch.float32, device=self.device) if self.soft_labels else None
        if self.rows:
            feat[:self.rows].copy_(self.feat[:self.rows])
            pos[:self.rows].copy_(self.pos[:self.rows])
            if soft is not None:
                soft[:self.rows].copy_(self.soft[:self.rows])
        self.feat, self.pos, self.soft = feat, pos, soft      # (the old buffers go back to torch's allocator, in stream order)

    def _upload(self, feats, poss, softs, pending):
        """append the host rows to the device buffers; the budget is checked before anything is allocated"""
        n = sum(int(f.shape[0]) for f in feats)
        need = (self.rows + n) * self._row_floats() * 4
        if need > self.max_bytes:
            raise ValueError('device dataset: %d bytes of region features needed, %d allowed (--device_dataset_max_gb %.3g)'
                             % (need, self.max_bytes, self.max_bytes / _GB))
        self._reserve(self.rows + n)
        if n:
            self.feat[self.rows:self.rows + n].copy_(torch.cat(feats))
            self.pos[self.rows:self.rows + n].copy_(torch.cat(poss))
            if self.soft_labels:
                self.soft[self.rows:self.rows + n, :self.label_dim].copy_(torch.cat(softs))
                self.soft[self.rows:self.rows + n, self.label_dim:].zero_()
        self.rows += n
        self._where.update(pending)          # resident from here on

    def add(self, dataset):
        """Make every sample of `dataset` resident (each not-yet-resident one is read ONCE, through dataset[idx]: the host path's
        feature directory, shard and confidence threshold) -> (row_start int64 [N], row_cnt int32 [N]) numpy arrays.  A pool with
        soft labels takes 'img_soft_label' [regions, C] of one common C from every sample of every dataset."""
        src, thr = self.source_of(dataset), float(dataset.confidence_threshold)
        ids = dataset.data.ids.tolist()
        if self.soft_labels and ids and not getattr(dataset, 'soft_labels', False):
            raise ValueError('device dataset: the pool keeps soft labels, but dataset %s (image %d first) gives no img_soft_label: '
                             'build it with soft_labels=True' % (getattr(dataset, 'name', '?'), int(ids[0])))
        row_start, row_cnt = np.zeros(len(ids), dtype=np.int64), np.zeros(len(ids), dtype=np.int32)
        feats, poss, softs, pending, held, at = [], [], [], {}, 0, self.rows
        for idx, img in enumerate(ids):
            key = (src, int(img), thr)
            if key not in self._where and key not in pending:
                s = dataset[idx]
                f, p = s['img_feat'].float().contiguous(), s['img_pos_feat'].float().contiguous()
                if self.dim is None:
                    self.dim = int(f.shape[1])
                if int(f.shape[1]) != self.dim or tuple(p.shape) != (int(f.shape[0]), 7):
                    raise ValueError('device dataset: image %d has features %s / %s, the pool holds rows of %d'
                                     % (int(img), tuple(f.shape), tuple(p.shape), self.dim))
                if self.soft_labels:
                    q = s.get('img_soft_label')
                    if q is None or q.dim() != 2 or int(q.shape[0]) != int(f.shape[0]):
                        raise ValueError('device dataset: image %d has soft labels %s for %d regions'
                                         % (int(img), None if q is None else tuple(q.shape), int(f.shape[0])))
                    if self.label_dim is None:
                        if int(q.shape[1]) < 2:
                            raise ValueError('device dataset: image %d has soft labels of %d classes; a background and a class are the least'
                                             % (int(img), int(q.shape[1])))
                        self.label_dim = int(q.shape[1])
                        self.ld_soft = (self.label_dim + 3) // 4 * 4
                    if int(q.shape[1]) != self.label_dim:
                        raise ValueError('device dataset: image %d has soft labels of %d classes, the pool holds rows of %d'
                                         % (int(img), int(q.shape[1]), self.label_dim))
                    softs.append(q.float().contiguous())
                    held += q.numel() * 4
                pending[key] = (at, int(f.shape[0]))
                at += int(f.shape[0])
                feats.append(f); poss.append(p)
                held += f.numel() * 4
                if held >= self.CHUNK_BYTES:
                    self._upload(feats, poss, softs, pending)
                    feats, poss, softs, pending, held = [], [], [], {}, 0
            row_start[idx], row_cnt[idx] = self._where[key] if key in self._where else pending[key]
        if self.dim is not None:
            self._upload(feats, poss, softs, pending)
        return row_start, row_cnt


class DeviceMemeDataset(object):
    """A MemeDataset whose samples live on the device: region rows in `pool`, the tokenised texts, lengths, labels and ids
    as device tensors.  Texts are tokenised once with the dataset's own `text_padding` (in chunks), which must pad to a fixed
    length (padding='max_length') as the CLI's does: T and `length` are the tokenizer's own."""

    TEXT_CHUNK = 1024

    def __init__(self, dataset, pool):
        if dataset.text_only:
            raise ValueError('device dataset: text_only datasets are not built (there is no region pool to keep resident)')
        if not dataset.compact_batch:
            raise ValueError('device dataset: compact_batch=False is not built (the kernel writes the compact mask and gather index)')
        self.dataset, self.pool = dataset, pool
        self.name, self.return_ids, self.data = dataset.name, dataset.return_ids, dataset.data
        self.ragged_regions = bool(dataset.ragged_regions)
        row_start, self.row_cnt = pool.add(dataset)               # raises before any allocation when over budget
        self.label_dim = pool.label_dim if getattr(pool, 'soft_labels', False) else None      # C of the resident soft labels
        ids, tts, lens = [], [], []
        for a in range(0, len(dataset), self.TEXT_CHUNK):
            texts = dataset.text_padding(dataset.data.text[a:a + self.TEXT_CHUNK])
            ids.append(texts['input_ids'])
            tts.append(texts.get('token_type_ids') if hasattr(texts, 'get') else None)
            ln = texts['length']
            lens += [int(x) for x in (ln.tolist() if torch.is_tensor(ln) else ln)]
            if ids[-1].shape[1] != ids[0].shape[1]:
                raise ValueError('device dataset: text_padding must pad every text to one length (padding="max_length"); got %d and %d'
                                 % (ids[0].shape[1], ids[-1].shape[1]))
        if not ids:
            raise ValueError('device dataset: %s is empty' % dataset.name)
        self.txt_len = np.asarray(lens, dtype=np.int32)
        dev = pool.device
        self.T = int(ids[0].shape[1])
        self.d_input_ids = torch.cat(ids).long().contiguous().to(dev)
        self.d_token_type_ids = None if any(t is None for t in tts) else torch.cat(tts).long().contiguous().to(dev)
        self.d_txt_len = torch.from_numpy(self.txt_len).to(dev)
        self.d_row_start = torch.from_numpy(row_start).to(dev)
        self.d_row_cnt = torch.from_numpy(self.row_cnt).to(dev)
        self.d_labels = dataset.data.labels.long().contiguous().to(dev)
        self.d_ids = dataset.data.ids.long().contiguous().to(dev)
        # the index of each sample's distinct text string (itm_pairs: a replaced text must differ from the sample's own)
        seen = {}
        self.text_class = np.asarray([seen.setdefault(str(t), len(seen)) for t in dataset.data.text], dtype=np.int32)

    def __len__(self):
        return len(self.dataset)


def plan_batches(order, batch_size, txt_len, row_cnt, ragged_regions):
    """The host side of a DeviceLoader epoch, from the numpy length arrays alone: [(first, last, R, L_out, seq_lens)] over
    `order` in batches of batch_size (the last may be short).  R, L_out and seq_lens are what the host collate derives: the
    batch's largest region count, its longest text + image length, and the per-sample lengths as a list of ints."""
    return plan_pretrain_batches(order, order, batch_size, txt_len, row_cnt, ragged_regions)


def _checked_order(order, n, who):
    """a sampler's draw as an int64 numpy array of indices into [0, n)"""
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    if order.size and (order.min() < 0 or order.max() >= n):
        raise ValueError('%s drew an index outside [0, %d)' % (who, n))
    return order


# the tensors of uniter_dataset_t (include/uniter_hip.h) in its order, as every collate wrapper takes them
_DATASET_NAMES = ('feat', 'pos', 'row_start', 'row_cnt', 'input_ids', 'token_type_ids', 'txt_len', 'labels', 'ids')
_DATASET_DTYPES = (torch.float32, torch.float32, torch.int64, torch.int32, torch.int64, torch.int64, torch.int32, torch.int64, torch.int64)


def _collate_setup(who, sel, txt_sel, extra, arrays, R, L_out, mask_key, more_shapes, out):
    """What the wrappers of the three uniter_collate_* entry points (include/uniter_hip.h) share.  Inputs: `sel`, `txt_sel`, the entry's
    own `extra` as (name, tensor, dtype) and the dataset's `arrays` (_DATASET_NAMES): each a GPU tensor of its type (token_type_ids
    and txt_sel may be None), the dataset's of one N and T, txt_sel of sel's length.  Outputs: the nine every entry writes -- the mask
    under `mask_key` -- and the entry's own, more_shapes(B, T, D) -> {key: (shape, dtype)} (None: none): allocated, or taken from
    `out` and validated.  -> (uniter_dataset_t, B, out, o), o(key) the pointer of an output or None where there is none."""
    require = _lib.require_gpu_tensor
    for name, t, dt in chain((('sel', sel, torch.int64), ('txt_sel', txt_sel, torch.int64)), extra, zip(_DATASET_NAMES, arrays, _DATASET_DTYPES)):
        if t is None and name not in ('token_type_ids', 'txt_sel'):
            raise _lib.UniterHipError('%s: %s is missing' % (who, name))
        require(t, dt, name)
    feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids = arrays
    N, T, B, D = int(row_start.shape[0]), int(input_ids.shape[1]), int(sel.shape[0]), int(feat.shape[1])
    if feat.dim() != 2 or pos.dim() != 2 or pos.shape[1] != 7 or pos.shape[0] != feat.shape[0]:
        raise _lib.UniterHipError('%s: feat [rows, D] / pos [rows, 7] expected; got %s / %s' % (who, tuple(feat.shape), tuple(pos.shape)))
    for name, t, shape in (('row_cnt', row_cnt, (N,)), ('input_ids', input_ids, (N, T)), ('txt_len', txt_len, (N,)), ('labels', labels, (N,)),
                           ('ids', ids, (N,)), ('token_type_ids', token_type_ids, (N, T)), ('txt_sel', txt_sel, (B,))):
        if t is not None and t.shape != shape:            # (torch.Size is a tuple)
            raise _lib.UniterHipError('%s: %s must be %s; got %s' % (who, name, shape, tuple(t.shape)))
    i64, f32 = torch.int64, torch.float32
    R, L_out = max(R, 0), max(L_out, 0)
    shapes = {'img_feat': ((B, R, D), f32), 'img_pos_feat': ((B, R, 7), f32), 'input_ids': ((B, T), i64), 'position_ids': ((B, T), i64),
              'token_type_ids': ((B, T), i64), mask_key: ((B, L_out), f32), 'gather_index': ((B, L_out), i64), 'labels': ((B,), i64),
              'ids': ((B,), i64)}
    if more_shapes is not None:
        shapes.update(more_shapes(B, T, D))
    if out is None:
        out = {k: (None if (k == 'token_type_ids' and token_type_ids is None) else torch.empty(s, dtype=dt, device=sel.device))
               for k, (s, dt) in shapes.items()}
    else:
        for k, (s, dt) in shapes.items():
            t = out.get(k)
            if t is None and k == 'token_type_ids':
                continue
            if t is None or t.shape != s:
                raise _lib.UniterHipError('%s: output %s must be %s; got %s' % (who, k, s, None if t is None else tuple(t.shape)))
            require(t, dt, 'output ' + k)
    ds = _lib.UniterDatasetC(feat.data_ptr(), pos.data_ptr(), row_start.data_ptr(), row_cnt.data_ptr(), input_ids.data_ptr(),
                             None if token_type_ids is None else token_type_ids.data_ptr(), txt_len.data_ptr(), labels.data_ptr(),
                             ids.data_ptr(), N, int(feat.shape[0]), D, T)
    for t in chain((sel, txt_sel), [e[1] for e in extra], arrays, out.values()):
        assert t is None or t.is_contiguous(), 'libuniter_hip needs contiguous tensors'

    def o(k):
        t = out.get(k)
        return None if t is None else C.c_void_p(t.data_ptr())
    return ds, B, out, o


def collate_batch(sel, feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids, R, L_out,
                  ragged_regions=False, out=None):
    """uniter_collate_batch (include/uniter_hip.h) on the current stream: the batch of the samples `sel` (int64, device) of a
    dataset given by its device tensors -> dict with the host collate's tensor keys.  `out`: the same dict of preallocated
    outputs to write into (tests); default: fresh tensors from torch's allocator."""
    R, L_out = int(R), int(L_out)                     # (handed to the library as they are: it refuses a negative one)
    arrays = (feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids)
    ds, B, out, o = _collate_setup('collate_batch', sel, None, (), arrays, R, L_out, 'attn_mask', None, out)
    with torch.cuda.device(sel.device):
        _lib.check(_lib.lib().uniter_collate_batch(
            C.byref(ds), C.c_void_p(sel.data_ptr()), B, R, L_out, 1 if ragged_regions else 0, o('img_feat'), o('img_pos_feat'),
            o('input_ids'), o('position_ids'), o('token_type_ids'), o('attn_mask'), o('gather_index'), o('labels'), o('ids'),
            _lib.cur_stream()), 'uniter_collate_batch')
    return out


class DeviceLoader(object):
    """Iterates a DeviceMemeDataset in batches built on the device.  Per epoch: the sampler's order (or range(N)), validated
    and uploaded once as one int64 tensor on the current stream; per batch: R, L_out and seq_lens from the host length arrays,
    fresh outputs from torch's allocator and one uniter_collate_batch launch on the current stream.  Yields the host collate's
    dict (tensors on the device, `token_type_ids` None when the tokenizer gives none, `seq_lens` the same Python list).  No
    thread, no side stream, and the loader never touches a yielded tensor's memory again."""

    def __init__(self, device_dataset, batch_size, sampler=None):
        if int(batch_size) < 1:
            raise ValueError('DeviceLoader: batch_size must be positive')
        self.dataset, self.batch_size, self.sampler = device_dataset, int(batch_size), sampler
        self.epoch_order = None              # the last epoch's order as the device tensor (kept alive while its batches are built)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return (n + self.batch_size - 1) // self.batch_size

    def order(self):
        """One epoch's sample order as a validated int64 numpy array (draws from the sampler)."""
        n = len(self.dataset)
        return _checked_order(list(self.sampler) if self.sampler is not None else range(n), n, 'DeviceLoader: the sampler')

    def plan(self, order):
        d = self.dataset
        return plan_batches(order, self.batch_size, d.txt_len, d.row_cnt, d.ragged_regions)

    def __iter__(self):
        d = self.dataset
        order = self.order()
        if order.size == 0:
            return
        self.epoch_order = dev_order = torch.from_numpy(order).to(d.pool.device)      # the epoch's one host -> device copy
        for a, b, R, L_out, seq_lens in self.plan(order):
            if L_out < 1:
                raise ValueError('DeviceLoader: a batch without a single valid position')
            pool = d.pool                    # (its buffers may have grown since the last batch: another dataset's add)
            batch = collate_batch(dev_order[a:b], pool.feat[:pool.rows], pool.pos[:pool.rows], d.d_row_start, d.d_row_cnt,
                                  d.d_input_ids, d.d_token_type_ids, d.d_txt_len, d.d_labels, d.d_ids, R, L_out,
                                  ragged_regions=d.ragged_regions)
            batch['seq_lens'] = seq_lens
            yield batch


# ---- pretraining batches from the resident dataset: MLM / MRFR masks and ITM targets drawn in the collate launch -------------------
# Counterpart of data/pretrain_mlm.py:35-69, data/pretrain_mrfr.py:29-51, data/pretrain_itm.py:27-47 and of MetaLoader
# (data/pretrain_meme_dataset.py:21-58).  The masks come from the Philox stream of include/uniter_hip.h (a function of seed, the
# task's epoch, the dataset sample and the position -- not of the batch); what the host decides is what it must know without a
# synchronisation: the order, the ITM pairing (the batch's L_out depends on it) and the task of every step.
PRETRAIN_TASKS = ('mlm', 'mrfr', 'itm')


def itm_pairs(order, text_class, replace_prob, rng):
    """The text of every position of `order` for image-text matching -> txt_order (int64, like order).  With probability
    replace_prob a position takes the text of a uniformly drawn sample whose text string differs from its own (rejection on
    text_class, the index of each sample's distinct string), otherwise it keeps its own: txt_order[i] == order[i] is the ITM
    target.  A dataset with one distinct text keeps all.  rng: a numpy Generator."""
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    text_class = np.asarray(text_class)
    txt_order = order.copy()
    if order.size == 0 or text_class.min() == text_class.max():
        return txt_order
    todo = np.flatnonzero(rng.random(order.size) < replace_prob)
    while todo.size:
        cand = rng.integers(0, len(text_class), todo.size)
        ok = text_class[cand] != text_class[order[todo]]
        txt_order[todo[ok]] = cand[ok]
        todo = todo[~ok]
    return txt_order


def plan_pretrain_batches(order, txt_order, batch_size, txt_len, row_cnt, ragged_regions):
    """plan_batches with the text lengths of txt_order (the samples the texts come from) and the region counts of order."""
    order, txt_order = np.asarray(order, dtype=np.int64), np.asarray(txt_order, dtype=np.int64)
    if order.shape != txt_order.shape:
        raise ValueError('plan_pretrain_batches: order and txt_order differ in shape: %s / %s' % (order.shape, txt_order.shape))
    out = []
    for a in range(0, len(order), batch_size):
        sel, tsel = order[a:a + batch_size], txt_order[a:a + batch_size]
        n, tl = row_cnt[sel].astype(np.int64), txt_len[tsel].astype(np.int64)
        R = int(n.max())
        seq = tl + (n if ragged_regions else R)
        out.append((a, a + len(sel), R, int(seq.max()), [int(x) for x in seq]))
    return out


def collate_pretrain_batch(task, sel, txt_sel, feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids, R, L_out,
                           ragged_regions=False, seed=0, draw=0, prob=0.15, cls_token=101, sep_token=102, pad_token=0, mask_token=103,
                           vocab_range=(1000, 28996), out=None):
    """uniter_collate_pretrain_batch (include/uniter_hip.h) on the current stream: the `task` ('mlm' / 'mrfr' / 'itm') batch of
    the samples `sel` with the texts of `txt_sel` (None: their own) -> dict with the reference collates' keys (`attn_masks`, sic),
    `labels` / `ids` / `token_type_ids` as collate_batch gives them, and for mlm / mrfr the compaction at full capacity:
    `masked_positions` [B*T or B*R, 2], `n_masked` (int32 [1], on the device; the first n_masked rows are defined) and, for
    mrfr, `feat_targets` [B*R, D].  `out`: the same dict of preallocated outputs to write into (tests)."""
    if task not in _lib.TASK_IDS:
        raise ValueError('collate_pretrain_batch: unknown task %r (one of %s)' % (task, ', '.join(PRETRAIN_TASKS)))
    i64, i32, f32 = torch.int64, torch.int32, torch.float32
    R, L_out = max(int(R), 0), max(int(L_out), 0)

    def more_shapes(B, T, D):
        if task == 'mlm':
            return dict(txt_labels=((B, T), i64), masked_positions=((B * T, 2), i64), n_masked=((1,), i32))
        if task == 'mrfr':
            return dict(img_masks=((B, R), i64), img_mask_tgt=((B, L_out), torch.bool), feat_targets=((B * R, D), f32),
                        masked_positions=((B * R, 2), i64), n_masked=((1,), i32))
        return dict(targets=((B,), i64))
    arrays = (feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids)
    ds, B, out, o = _collate_setup('collate_pretrain_batch', sel, txt_sel, (), arrays, R, L_out, 'attn_masks', more_shapes, out)
    cfg = _lib.UniterMaskCfgC(int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, float(prob), int(cls_token), int(sep_token),
                              int(pad_token), int(mask_token), int(vocab_range[0]), int(vocab_range[1]))
    with torch.cuda.device(sel.device):
        _lib.check(_lib.lib().uniter_collate_pretrain_batch(
            C.byref(ds), C.c_void_p(sel.data_ptr()), None if txt_sel is None else C.c_void_p(txt_sel.data_ptr()), _lib.TASK_IDS[task],
            C.byref(cfg), B, R, L_out, 1 if ragged_regions else 0, o('img_feat'), o('img_pos_feat'), o('input_ids'), o('position_ids'),
            o('token_type_ids'), o('attn_masks'), o('gather_index'), o('labels'), o('ids'), o('txt_labels'), o('img_masks'),
            o('img_mask_tgt'), o('feat_targets'), o('targets'), o('masked_positions'), o('n_masked'), _lib.cur_stream()),
            'uniter_collate_pretrain_batch')
    return out


# Masked region classification (data/pretrain_mrc.py; model/pretrain.py:205-233) needs what the three tasks above do not: the
# detector's class distribution of every region, resident beside the features (DeviceFeaturePool(soft_labels=True)).  Both tasks
# draw their region masks from one stream of their own; 'mrc' takes the classes, 'mrc-kl' the distributions.
MRC_TASKS = ('mrc', 'mrc-kl')


def collate_mrc_batch(sel, feat, pos, soft, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids, R, L_out, label_dim,
                      hard=True, soft_out=True, ragged_regions=False, seed=0, draw=0, prob=0.15, out=None):
    """uniter_collate_mrc_batch (include/uniter_hip.h) on the current stream: the MRC / MRC-kl batch of the samples `sel`.  `soft`
    [rows, ld_soft >= label_dim] holds the soft labels of the rows of `feat`.  -> dict with the reference collate's keys
    (`attn_masks`, `img_masks`, `img_mask_tgt`, `label_targets`), `labels` / `ids` / `token_type_ids` as collate_batch gives them,
    and the compaction at full capacity: `masked_positions` [B*R, 2], `n_masked` (int32 [1], on the device; the first n_masked rows
    are defined), `label_targets` [B*R, label_dim] (soft_out) and `label_ids` [B*R] (hard: 1 + the first maximum of a row's columns
    1 .., what pretrain._hard_region_labels finds).  At least one of hard and soft_out.  `out`: the same dict of preallocated
    outputs to write into (tests)."""
    if not (hard or soft_out):
        raise ValueError('collate_mrc_batch: neither label_ids (hard) nor label_targets (soft_out) asked for')
    i64, i32, f32 = torch.int64, torch.int32, torch.float32
    R, L_out, Cn = max(int(R), 0), max(int(L_out), 0), int(label_dim)

    def more_shapes(B, T, D):
        if soft.dim() != 2 or soft.shape[0] != feat.shape[0] or Cn < 2 or int(soft.shape[1]) < Cn:
            raise _lib.UniterHipError('collate_mrc_batch: soft [%d rows, ld_soft >= label_dim = %d >= 2] expected; got %s'
                                      % (int(feat.shape[0]), Cn, tuple(soft.shape)))
        shapes = dict(img_masks=((B, R), i64), img_mask_tgt=((B, L_out), torch.bool), masked_positions=((B * R, 2), i64),
                      n_masked=((1,), i32))
        if soft_out:
            shapes['label_targets'] = ((B * R, Cn), f32)
        if hard:
            shapes['label_ids'] = ((B * R,), i64)
        return shapes
    arrays = (feat, pos, row_start, row_cnt, input_ids, token_type_ids, txt_len, labels, ids)
    ds, B, out, o = _collate_setup('collate_mrc_batch', sel, None, (('soft', soft, f32),), arrays, R, L_out, 'attn_masks', more_shapes, out)
    cfg = _lib.UniterMaskCfgC(int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, float(prob), 0, 0, 0, 0, 0, 0)
    with torch.cuda.device(sel.device):
        # (an output that was not asked for is NULL to the library, whatever `out` holds under its key)
        _lib.check(_lib.lib().uniter_collate_mrc_batch(
            C.byref(ds), C.c_void_p(soft.data_ptr()), Cn, int(soft.shape[1]), C.c_void_p(sel.data_ptr()), C.byref(cfg), B, R, L_out,
            1 if ragged_regions else 0, o('img_feat'), o('img_pos_feat'), o('input_ids'), o('position_ids'), o('token_type_ids'),
            o('attn_masks'), o('gather_index'), o('labels'), o('ids'), o('img_masks'), o('img_mask_tgt'),
            o('label_targets') if soft_out else None, o('label_ids') if hard else None, o('masked_positions'), o('n_masked'),
            _lib.cur_stream()), 'uniter_collate_mrc_batch')
    return out


class DevicePretrainLoader(object):
    """MetaLoader over a DeviceMemeDataset: an indefinite iterator of (task, batch).  Every `accum_steps` steps the task is drawn
    from the ratio pool (`tasks`: (name, ratio) pairs) by a generator seeded from `seed`.  Every task walks its own epochs: its
    own order per epoch (samplers[name], an iterable of sample indices as DeviceLoader's sampler; default: a permutation from the
    task's own generator), for 'itm' its own pairing (itm_pairs), and its own `draw` counter -- the task's epoch index -- so that a
    sample's mask changes from epoch to epoch and depends on nothing else.  Per batch: one uniter_collate_pretrain_batch launch
    on the current stream; for mlm / mrfr the loader then reads n_masked -- the step's ONE host synchronisation, which waits for
    the collate launch queued behind the previous step's tail -- and yields `masked_positions[:n]` / `feat_targets[:n]` as views
    (UniterForPretraining uses masked_positions in place of its own nonzero).  Batches carry the reference collates' keys
    (`attn_masks`; `txt_labels` | `img_masks`, `img_mask_tgt`, `feat_targets` | `targets`), `labels`, `ids`, `token_type_ids` and
    the host list `seq_lens`.  len() is the sum of the tasks' batches per epoch.

    A dataset with resident soft labels (`label_dim` is not None) also serves 'mrc' and 'mrc-kl': one uniter_collate_mrc_batch
    launch, the same one read of n_masked, then views [:n] of `masked_positions` and of `label_ids` ('mrc': the classes alone, no
    label_dim-wide row is written) or `label_targets` ('mrc-kl': the distributions alone)."""

    # per task with a compaction: what is cut to n_masked rows besides masked_positions
    COMPACTED = {'mlm': (), 'mrfr': ('feat_targets',), 'mrc': ('label_ids',), 'mrc-kl': ('label_targets',)}

    def __init__(self, device_dataset, batch_size, tasks=(('mlm', 1), ('mrfr', 1), ('itm', 1)), seed=0, mask_prob=0.15, replace_prob=0.5,
                 accum_steps=1, samplers=None, cls_token=101, sep_token=102, pad_token=0, mask_token=103, vocab_range=(1000, 28996)):
        if int(batch_size) < 1:
            raise ValueError('DevicePretrainLoader: batch_size must be positive')
        tasks = [(str(n), int(r)) for n, r in tasks]
        if not tasks:
            raise ValueError('DevicePretrainLoader: no task given')
        served = PRETRAIN_TASKS + (MRC_TASKS if getattr(device_dataset, 'label_dim', None) is not None else ())
        for name, ratio in tasks:
            if name not in served:
                raise ValueError('DevicePretrainLoader: unknown task %r (this dataset serves %s%s)'
                                 % (name, ', '.join(served), '' if len(served) > len(PRETRAIN_TASKS) else
                                    '; %s need resident soft labels: MemeDataset and DeviceFeaturePool with soft_labels=True'
                                    % ' and '.join(MRC_TASKS)))
            if ratio < 1:
                raise ValueError('DevicePretrainLoader: task %s has ratio %d; ratios are positive integers' % (name, ratio))
        if len({n for n, _ in tasks}) != len(tasks):
            raise ValueError('DevicePretrainLoader: a task is listed twice')
        if not (0.0 <= float(mask_prob) <= 1.0 and 0.0 <= float(replace_prob) <= 1.0):
            raise ValueError('DevicePretrainLoader: mask_prob and replace_prob are probabilities')
        if int(accum_steps) < 1:
            raise ValueError('DevicePretrainLoader: accum_steps must be positive')
        self.dataset, self.batch_size, self.seed = device_dataset, int(batch_size), int(seed)
        self.tasks = [n for n, _ in tasks]
        self.sampling_pool = [n for n, r in tasks for _ in range(r)]
        self.mask_prob, self.replace_prob, self.accum_steps = float(mask_prob), float(replace_prob), int(accum_steps)
        self.samplers = dict(samplers or {})
        for name in self.samplers:
            if name not in self.tasks:
                raise ValueError('DevicePretrainLoader: a sampler for %r, which is not among the tasks' % name)
        self.tokens = dict(cls_token=int(cls_token), sep_token=int(sep_token), pad_token=int(pad_token), mask_token=int(mask_token),
                           vocab_range=(int(vocab_range[0]), int(vocab_range[1])))
        self.step = 0
        self.epochs = {n: 0 for n in self.tasks}          # epochs begun per task: the next epoch's `draw`
        self.epoch_orders = {}                            # task -> (order, txt_order) of its current epoch, numpy
        self._task_rng = np.random.default_rng([self.seed, len(PRETRAIN_TASKS)])
        self._rngs = {n: self.task_rng(self.seed, n) for n in self.tasks}
        self._iters, self._dev_orders = {}, {}

    @staticmethod
    def task_rng(seed, task):
        """the generator behind a task's default orders and ITM pairings: [seed, 0 .. 2] for the three tasks of PRETRAIN_TASKS,
        [seed, 3] and [seed, 4] for 'mrc' and 'mrc-kl' (the task choice is seeded [seed, 3] as well, and stays so: the sequences of
        the three older tasks must not move; the two generators are separate objects)"""
        return np.random.default_rng([int(seed), (PRETRAIN_TASKS + MRC_TASKS).index(task)])

    def _epoch_len(self, task):
        s = self.samplers.get(task)
        return len(s) if s is not None else len(self.dataset)

    def __len__(self):
        return sum((self._epoch_len(t) + self.batch_size - 1) // self.batch_size for t in self.tasks)

    def order(self, task):
        """One epoch's validated sample order of `task` (draws from its sampler or its generator)."""
        n = len(self.dataset)
        s = self.samplers.get(task)
        order = _checked_order(list(s) if s is not None else self._rngs[task].permutation(n), n,
                               'DevicePretrainLoader: the sampler of task %s' % task)
        if order.size == 0:
            raise ValueError('DevicePretrainLoader: the order of task %s is empty' % task)
        return order

    def _epoch(self, task):
        d = self.dataset
        draw = self.epochs[task]
        self.epochs[task] += 1
        order = self.order(task)
        txt_order = itm_pairs(order, d.text_class, self.replace_prob, self._rngs[task]) if task == 'itm' else order
        self.epoch_orders[task] = (order, txt_order)
        plan = plan_pretrain_batches(order, txt_order, self.batch_size, d.txt_len, d.row_cnt, d.ragged_regions)
        if any(L_out < 1 for _, _, _, L_out, _ in plan):
            raise ValueError('DevicePretrainLoader: a batch without a single valid position')
        # the epoch's one host -> device copy (kept alive while its batches are built)
        self._dev_orders[task] = dev = torch.from_numpy(np.stack([order, txt_order])).to(d.pool.device)
        for a, b, R, L_out, seq_lens in plan:
            pool = d.pool
            regions = (pool.feat[:pool.rows], pool.pos[:pool.rows])
            rest = (d.d_row_start, d.d_row_cnt, d.d_input_ids, d.d_token_type_ids, d.d_txt_len, d.d_labels, d.d_ids, R, L_out)
            draws = dict(ragged_regions=d.ragged_regions, seed=self.seed, draw=draw, prob=self.mask_prob)
            if task in MRC_TASKS:
                batch = collate_mrc_batch(dev[0, a:b], *regions, pool.soft[:pool.rows], *rest, d.label_dim, hard=task == 'mrc',
                                          soft_out=task != 'mrc', **draws)
            else:
                batch = collate_pretrain_batch(task, dev[0, a:b], dev[1, a:b] if task == 'itm' else None, *regions, *rest, **draws,
                                               **self.tokens)
            if task in self.COMPACTED:
                n = batch['n_masked'] = int(batch['n_masked'].item())          # the step's one host synchronisation
                for k in ('masked_positions',) + self.COMPACTED[task]:
                    batch[k] = batch[k][:n]
            batch['seq_lens'] = seq_lens
            yield batch

    def __iter__(self):
        """runs indefinitely; the tasks' epochs carry on where an earlier iteration left them"""
        task = self.sampling_pool[0]
        while True:
            if self.step % self.accum_steps == 0:
                task = self.sampling_pool[int(self._task_rng.integers(len(self.sampling_pool)))]
            self.step += 1
            if task not in self._iters:
                self._iters[task] = self._epoch(task)
            try:
                batch = next(self._iters[task])
            except StopIteration:
                self._iters[task] = self._epoch(task)
                batch = next(self._iters[task])
            yield task, batch
