"""The bookkeeping of the order-fixed embedding backward (csrc/embed.hip, uniter_txt_embed_bwd_det), restated in numpy: the stable
rank of the rows by table key, the chunks of ranked rows, the runs of one key inside a chunk, and who adds a key's total to its
table row.  CHUNK, RANK_WG, WG_ROWS and MAX_ROWS repeat the kernel file's constants (DET_CHUNK, DET_RANK_WG, DET_WG_ROWS) and the
header's UNITER_EMBED_DET_MAX_ROWS."""
import numpy as np

CHUNK = 32          # ranked rows per chunk
RANK_WG = 256       # rows one workgroup ranks
WG_ROWS = 32        # rows per partial sum of the position projection's weight gradient
MAX_ROWS = 16384


def keys_of(ids, hi, rows=None, bcast_T=0):
    """the table row each of `rows` rows reads: the id clamped to 0 .. hi - 1, row r reading ids[r % bcast_T] when broadcast"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    rows = len(ids) if rows is None else rows
    src = np.arange(rows) % bcast_T if bcast_T else np.arange(rows)
    return np.clip(ids[src], 0, hi - 1).astype(np.int64)


def stable_rank(keys):
    """rank(r) = #{r' : key[r'] < key[r] or (key[r'] == key[r] and r' < r)}, by the definition (O(n^2))"""
    k = np.asarray(keys)
    r = np.arange(len(k))
    less = (k[None, :] < k[:, None]) | ((k[None, :] == k[:, None]) & (r[None, :] < r[:, None]))
    return less.sum(1)


def runs(keys, skip=-1):
    """The sums the chunk kernel forms, in launch order: a list of dicts(chunk, key, rows (ascending), slot) where slot is
    None for a run that is a whole segment (added to the table there and then), 0 for a piece of a segment that began in an
    earlier chunk and 1 for the piece that begins a segment going on behind the chunk.  Runs of the skipped key are listed
    too (the kernel sums them and adds them nowhere)."""
    keys = np.asarray(keys)
    n = len(keys)
    rank = stable_rank(keys)
    order = np.empty(n, dtype=np.int64)
    order[rank] = np.arange(n)
    skey = keys[order]
    out = []
    for c in range((n + CHUNK - 1) // CHUNK):
        r0, r1 = c * CHUNK, min(n, (c + 1) * CHUNK)
        prev = skey[r0 - 1] if r0 > 0 else -1
        nxt = skey[r1] if r1 < n else -1
        i = r0
        while i < r1:
            j = i + 1
            while j < r1 and skey[j] == skey[i]:
                j += 1
            open_l, open_r = i == r0 and skey[i] == prev, j == r1 and skey[i] == nxt
            out.append(dict(chunk=c, key=int(skey[i]), rows=order[i:j].tolist(),
                            slot=(0 if open_l else 1) if (open_l or open_r) else None))
            i = j
    return out


def owners(keys, skip=-1):
    """{key: (owning chunk, [the runs of that key in the order they are added])} for every key but `skip`"""
    own = {}
    for run in runs(keys):
        if run['key'] == skip:
            continue
        if run['key'] not in own:
            assert run['slot'] in (None, 1), run         # a segment begins with a whole run or with a slot-1 piece
            own[run['key']] = (run['chunk'], [run])
        else:
            assert run['slot'] == 0, run                 # and goes on in slot 0 of the following chunks
            own[run['key']][1].append(run)
    return own


def scatter_sum(keys, d, n_keys, skip=-1, dtype=np.float32):
    """the table gradient in the kernels' order and precision: rows of a run left to right, runs in chunk order"""
    d = np.asarray(d, dtype=dtype)
    out = np.zeros((n_keys, d.shape[1]), dtype=dtype)
    for key, (_, rs) in owners(keys, skip).items():
        total = None
        for run in rs:
            acc = d[run['rows'][0]].copy()
            for r in run['rows'][1:]:
                acc = acc + d[r]
            total = acc if total is None else total + acc
        out[key] = total
    return out
