// Collate on the device: one batch of data.MemeDataset.get_collate_fn() (compact_batch = True) assembled from a dataset that is
// resident in device memory (uniter_dataset_t, include/uniter_hip.h), in ONE launch.
//
// Decomposition ("Device-resident dataset").  The work is B * R region rows of D floats plus a few hundred small
// integers per sample, and at the flagship shape (16 x 36 rows of 8 KB: 4.7 MB read, 4.7 MB written) it is over in a few
// microseconds: what counts is how many 16-byte loads are in flight, not a tiling.  So the grid is sized from the items:
//   * a region item is (output row, 4-KB piece of it): one wave moves up to 256 float4, four per lane, all four loads issued
//     before the first store; consecutive lanes take consecutive float4 (one wave-instruction = 1 KB of one row).  The wave of a
//     row's first piece also writes the row's 7 box features (28-byte rows: scalar accesses).  Four items per workgroup.
//   * one workgroup per sample writes what is small: input_ids, position_ids, token_type_ids, attn_mask, gather_index, the
//     label and the id.
// Every output element has one writer and is written (padding rows as zeros); no atomics, no LDS, no workspace.
#include "common.h"
#include "philox.h"

namespace {

constexpr int PIECE4 = 256;            // float4 per region item (4 KB): 4 per lane

struct CollateArgs {
  uniter_dataset_t ds;
  const int64_t* sel;
  int B, R, L_out, ragged;
  int D4, pieces;                      // float4 per row, region items per row
  long long region_items;              // B * R * pieces
  unsigned region_blocks;              // ceil(region_items / 4)
  float* img_feat;
  float* img_pos_feat;
  int64_t* input_ids;
  int64_t* position_ids;
  int64_t* token_type_ids;
  float* attn_mask;
  int64_t* gather_index;
  int64_t* labels;
  int64_t* ids;
};

// memory safety only (include/uniter_hip.h): a sample index outside [0, N) is clamped, a region count to [0, R]
__device__ __forceinline__ long long sample_of(const CollateArgs& a, int b) {
  long long s = a.sel[b];
  return s < 0 ? 0 : (s >= a.ds.N ? a.ds.N - 1 : s);
}
__device__ __forceinline__ int regions_of(const CollateArgs& a, long long s) {
  const int n = a.ds.row_cnt[s];
  return n < 0 ? 0 : (n > a.R ? a.R : n);
}

// ---- the pieces every collate kernel is built from ---------------------------------------------------------------------------
// A region item decoded: output row b * R + r, the 4-KB piece of it, the dataset sample s with its n regions and the pool row.
struct RegionItem {
  long long row, s, src_row;
  int piece, b, r, n;
  bool real;                           // a pool row outside the pool reads as padding (never dereferenced)
};
// the item of this wave (four per workgroup); false beyond the last one.  Uniform over the wave.
__device__ __forceinline__ bool region_item(const CollateArgs& a, RegionItem& it) {
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.region_items) return false;
  it.row = item / a.pieces;
  it.piece = (int)(item - it.row * a.pieces);
  it.b = (int)(it.row / a.R);
  it.r = (int)(it.row - (long long)it.b * a.R);
  it.s = sample_of(a, it.b);
  it.src_row = a.ds.row_start[it.s] + it.r;
  it.n = regions_of(a, it.s);
  it.real = it.r < it.n && it.src_row >= 0 && it.src_row < a.ds.pool_rows;
  return true;
}
// the lane's four float4 of the item: the pool row's when `take`, else zeros; all four loads are issued before anything is stored
__device__ __forceinline__ void piece_load(const CollateArgs& a, const RegionItem& it, bool take, int lane, f32x4 (&v)[4]) {
  const int c0 = it.piece * PIECE4 + lane;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (take) {
    const f32x4* sp = reinterpret_cast<const f32x4*>(a.ds.feat) + (size_t)it.src_row * a.D4;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + 64 * k < a.D4) v[k] = sp[c0 + 64 * k];
  }
}
// ... to the item's piece of row `row` of `base` (rows of D floats: img_feat, feat_targets)
__device__ __forceinline__ void piece_store(const CollateArgs& a, const RegionItem& it, int lane, float* base, long long row,
                                            const f32x4 (&v)[4]) {
  f32x4* dp = reinterpret_cast<f32x4*>(base) + (size_t)row * a.D4;
  const int c0 = it.piece * PIECE4 + lane;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c0 + 64 * k < a.D4) dp[c0 + 64 * k] = v[k];
}
// the row's 7 box features, by the wave of its first piece
__device__ __forceinline__ void box_row(const CollateArgs& a, const RegionItem& it, int lane) {
  if (it.piece == 0 && lane < 7)
    a.img_pos_feat[(size_t)it.row * 7 + lane] = it.real ? a.ds.pos[(size_t)it.src_row * 7 + lane] : 0.f;
}
// What the workgroup of sample b writes in every entry: position_ids, token_type_ids, attn_mask, gather_index, the label and the
// id of sample s, for the text of sample ts (tl tokens) and il image positions.  copy_text: input_ids as well (the text unchanged).
__device__ __forceinline__ void sample_frame(const CollateArgs& a, int b, long long s, long long ts, long long tl, long long il,
                                             bool copy_text) {
  const int T = a.ds.T;
  for (int t = threadIdx.x; t < T; t += 256) {
    if (copy_text) a.input_ids[(size_t)b * T + t] = a.ds.input_ids[(size_t)ts * T + t];
    a.position_ids[(size_t)b * T + t] = t;
    if (a.token_type_ids) a.token_type_ids[(size_t)b * T + t] = a.ds.token_type_ids[(size_t)ts * T + t];
  }
  for (int j = threadIdx.x; j < a.L_out; j += 256) {
    a.attn_mask[(size_t)b * a.L_out + j] = j < tl + il ? 1.0f : 0.0f;
    a.gather_index[(size_t)b * a.L_out + j] = (tl <= j && j < tl + il) ? j - tl + T : j;     // utils.get_gather_index, max_len = T
  }
  if (threadIdx.x == 0) {
    a.labels[b] = a.ds.labels[s];
    a.ids[b] = a.ds.ids[s];
  }
}

__global__ __launch_bounds__(256) void collate_batch_kernel(const CollateArgs a) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x < a.region_blocks) {
    RegionItem it;
    if (!region_item(a, it)) return;
    f32x4 v[4];
    piece_load(a, it, it.real, lane, v);
    piece_store(a, it, lane, a.img_feat, it.row, v);
    box_row(a, it, lane);
    return;
  }
  const int b = (int)(blockIdx.x - a.region_blocks);
  const long long s = sample_of(a, b);
  sample_frame(a, b, s, s, a.ds.txt_len[s], a.ragged ? regions_of(a, s) : a.R, true);
}

// ---- the host side every entry shares ----------------------------------------------------------------------------------------
// The checks of the dataset, the shapes and the nine common outputs (already in c), under the entry's name.
int check_common(const char* who, const uniter_dataset_t* ds, const CollateArgs& c) {
  const int B = c.B, R = c.R, L_out = c.L_out;
  UCHECK_ARG(ds && c.sel, "%s: null dataset or selection", who);
  UCHECK_ARG(ds->row_start && ds->row_cnt && ds->input_ids && ds->txt_len && ds->labels && ds->ids, "%s: null pointer in the dataset", who);
  UCHECK_ARG(c.input_ids && c.position_ids && c.attn_mask && c.gather_index && c.labels && c.ids, "%s: null output pointer", who);
  UCHECK_ARG(ds->N > 0 && ds->pool_rows >= 0, "%s: dataset of %lld samples, %lld pool rows", who, (long long)ds->N, (long long)ds->pool_rows);
  UCHECK_SHAPE(B > 0 && ds->T > 0 && L_out > 0 && R >= 0, "%s: B = %d, T = %d, L_out = %d, R = %d (B, T, L_out > 0, R >= 0)", who, B, ds->T,
               L_out, R);
  UCHECK_SHAPE((long long)L_out <= (long long)ds->T + R, "%s: L_out = %d exceeds T + R = %d + %d", who, L_out, ds->T, R);
  UCHECK_SHAPE(ds->D > 0 && ds->D % 4 == 0, "%s: D = %d must be a positive multiple of 4 (rows move as 16-byte items)", who, ds->D);
  // an empty pool (every sample's confidence filter left nothing) has no rows to point at; R == 0 has no region output
  UCHECK_ARG((ds->feat && ds->pos) || ds->pool_rows == 0, "%s: null feat / pos with %lld pool rows", who, (long long)ds->pool_rows);
  UCHECK_ARG((c.img_feat && c.img_pos_feat) || R == 0, "%s: null img_feat / img_pos_feat with R = %d", who, R);
  UCHECK_ARG(((uintptr_t)ds->feat & 15) == 0, "%s: feat is not 16-byte aligned", who);
  UCHECK_ARG(((uintptr_t)c.img_feat & 15) == 0, "%s: img_feat is not 16-byte aligned", who);
  return 0;
}

// c from the arguments every entry has, checked (check_common, then the size of the launch); the grid is region_blocks + B
int fill_args(const char* who, CollateArgs& c, const uniter_dataset_t* ds, const int64_t* sel, int B, int R, int L_out, int flags,
              float* img_feat, float* img_pos_feat, int64_t* input_ids, int64_t* position_ids, int64_t* token_type_ids, float* attn_mask,
              int64_t* gather_index, int64_t* labels, int64_t* ids) {
  c.sel = sel; c.B = B; c.R = R; c.L_out = L_out; c.ragged = flags & 1;
  c.img_feat = img_feat; c.img_pos_feat = img_pos_feat; c.input_ids = input_ids; c.position_ids = position_ids;
  c.token_type_ids = token_type_ids; c.attn_mask = attn_mask; c.gather_index = gather_index; c.labels = labels; c.ids = ids;
  UCHECK_RC(check_common(who, ds, c));
  c.ds = *ds;
  if (!ds->token_type_ids) c.token_type_ids = nullptr;
  c.D4 = ds->D / 4;
  c.pieces = (c.D4 + PIECE4 - 1) / PIECE4;
  c.region_items = (long long)B * R * c.pieces;
  const long long region_blocks = (c.region_items + 3) / 4;
  UCHECK_SHAPE(region_blocks + B < 0x7fffffffLL, "%s: %lld region items exceed one launch", who, c.region_items);
  c.region_blocks = (unsigned)region_blocks;
  return 0;
}

}  // namespace

extern "C" int uniter_collate_batch(const uniter_dataset_t* ds, const int64_t* sel, int B, int R, int L_out, int flags,
                                    float* img_feat, float* img_pos_feat, int64_t* input_ids, int64_t* position_ids,
                                    int64_t* token_type_ids, float* attn_mask, int64_t* gather_index, int64_t* labels,
                                    int64_t* ids, void* stream) {
  CollateArgs a;
  UCHECK_RC(fill_args("collate_batch", a, ds, sel, B, R, L_out, flags, img_feat, img_pos_feat, input_ids, position_ids, token_type_ids,
                      attn_mask, gather_index, labels, ids));
  hipLaunchKernelGGL(collate_batch_kernel, dim3(a.region_blocks + (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  UCHECK_LAUNCH();
  return 0;
}

// ---- pretraining batches: the same copy, plus the MLM / MRFR masks drawn here and their compaction -----------------------------
// Same grid as above (region items, then one workgroup per sample); the specification of the random stream and of every output is
// in include/uniter_hip.h.  What is new is the order of the compacted outputs (masked_positions, feat_targets): entry (b, position)
// lands at [entries selected in samples < b] + [entries selected in sample b before position].  No workgroup waits for another: the
// masks are a pure function of (seed, draw, sample, position), so whoever needs the first term draws those masks again.
//   MLM   the workgroup of sample b: its four waves walk the samples in front of it (one sample per wave and trip, the lanes over
//         its tokens), then the workgroup ranks its own tokens in chunks of 256 (ballot + popcount per wave, four wave totals
//         through LDS).
//   MRFR  a wave moving region row (b, r) draws its own sample's n <= R regions (lanes over regions); only when the row is selected
//         does it count the samples in front (one sample per lane, serial over its regions).  The workgroup of sample b writes the
//         dense img_masks / img_mask_tgt; the last one counts every sample (one per thread) for n_masked.
//   MRC   MRFR on its own stream.  A selected region keeps no copy of its features, so the wave of its first piece has no loads
//         of its own: it moves the region's soft-label row instead and finds the row's class on the way (soft_row).
namespace {

struct PretrainArgs {
  CollateArgs c;
  const int64_t* txt_sel;
  int task;
  uint32_t k0, k1, draw, thresh;
  int always;                            // prob >= 1
  long long cls, sep, pad, mask_token, vocab_lo;
  unsigned long long vocab_span;
  int64_t* txt_labels;
  int64_t* img_masks;
  unsigned char* img_mask_tgt;
  float* feat_targets;
  int64_t* targets;
  int64_t* masked_positions;
  int32_t* n_masked;
  // uniter_collate_mrc_batch only (collate_pretrain_kernel<true>): the soft-label rows beside ds.feat and their two outputs
  const float* soft;
  int C, ld_soft, soft4;                 // soft4: rows of `soft` start 16-byte aligned (base aligned, ld_soft % 4 == 0)
  float* label_targets;
  int64_t* label_ids;
};

__device__ __forceinline__ long long text_sample_of(const PretrainArgs& a, int b) {
  if (!a.txt_sel) return sample_of(a.c, b);
  long long s = a.txt_sel[b];
  return s < 0 ? 0 : (s >= a.c.ds.N ? a.c.ds.N - 1 : s);
}
__device__ __forceinline__ bool hit(const PretrainArgs& a, uint32_t word) { return a.always || word < a.thresh; }

// token t of dataset sample ts, holding `tok`: selected by its own draw?  (w: the draw, for the 80 / 10 / 10 split)
__device__ __forceinline__ bool mlm_drawn(const PretrainArgs& a, long long ts, int t, long long tok, u32x4& w) {
  w = philox4x32_10((uint32_t)t, (uint32_t)ts, UNITER_STREAM_MLM, a.draw, a.k0, a.k1);
  return tok != a.cls && tok != a.sep && tok != a.pad && hit(a, w.x);
}
// selected tokens of sample ts, the forced one included; the whole wave calls it and every lane gets the result
__device__ __forceinline__ int mlm_count_wave(const PretrainArgs& a, long long ts, int lane) {
  const int T = a.c.ds.T;
  const int64_t* src = a.c.ds.input_ids + (size_t)ts * T;
  int cnt = 0;
  for (int base = 0; base < T; base += 64) {
    const int t = base + lane;
    u32x4 w;
    const bool f = t < T && mlm_drawn(a, ts, t, src[t], w);
    cnt += __popcll(__ballot(f));
  }
  return cnt > 0 ? cnt : 1;              // T >= 2: position 1 exists
}

// The region masks of MRFR and of MRC are the same rule on two streams; MRC selects the stream of uniter_collate_mrc_batch.
template <bool MRC>
__device__ __forceinline__ bool region_drawn(const PretrainArgs& a, long long s, int r) {
  constexpr uint32_t stream = MRC ? UNITER_STREAM_MRC : UNITER_STREAM_MRFR;
  return hit(a, philox4x32_10((uint32_t)r, (uint32_t)s, stream, a.draw, a.k0, a.k1).x);
}
// the region taken when none of the n > 0 regions of sample s was drawn
template <bool MRC>
__device__ __forceinline__ int region_forced(const PretrainArgs& a, long long s, int n) {
  constexpr uint32_t stream = MRC ? UNITER_STREAM_MRC : UNITER_STREAM_MRFR;
  const u32x4 w = philox4x32_10(0xFFFFFFFFu, (uint32_t)s, stream, a.draw, a.k0, a.k1);
  return (int)(((unsigned long long)w.x * (unsigned long long)n) >> 32);
}
// selected regions of sample s, by ONE thread
template <bool MRC>
__device__ __forceinline__ int region_count_serial(const PretrainArgs& a, long long s) {
  const int n = regions_of(a.c, s);
  int cnt = 0;
  for (int r = 0; r < n; ++r) cnt += region_drawn<MRC>(a, s, r) ? 1 : 0;
  return (cnt == 0 && n > 0) ? 1 : cnt;
}
// Region r < n of sample s = sel[b], by the whole wave: is it selected, and if so which row of the compacted outputs
// (masked_positions, feat_targets | label_targets, label_ids) is its own?  Uniform over the wave.
template <bool MRC>
__device__ __forceinline__ bool region_slot(const PretrainArgs& a, long long s, int n, int b, int r, int lane, long long& dest) {
  int before = 0, total = 0;
  bool mine = false;
  for (int base = 0; base < n; base += 64) {
    const int rr = base + lane;
    const unsigned long long bal = __ballot(rr < n && region_drawn<MRC>(a, s, rr));
    total += __popcll(bal);
    if (r >= base + 64) before += __popcll(bal);
    else if (r >= base) {
      before += __popcll(bal & ((1ull << (r - base)) - 1ull));
      mine = (bal >> (r - base)) & 1ull;
    }
  }
  bool masked;
  if (total == 0) { masked = r == region_forced<MRC>(a, s, n); before = 0; }
  else masked = mine;
  if (masked) {
    int front = 0;
    for (int bp = lane; bp < b; bp += 64) front += region_count_serial<MRC>(a, sample_of(a.c, bp));
    for (int o = 32; o > 0; o >>= 1) front += __shfl_xor(front, o, 64);
    dest = (long long)front + before;                  // < B * R: every sample contributes at most its n <= R
  }
  return masked;
}

// MRC: one wave moves the soft-label row of a selected region to row `dest` of label_targets and finds its class for label_ids
// in the same walk (the first maximum of columns 1 .. C-1, as heads.hip's row_argmax_kernel with c0 = 1: NaN never wins, a row
// without a winner gives 1).  The row is walked in chunks of 2048 columns -- C = 1601 is one chunk -- and a chunk's loads are all
// issued before its first store.  Source rows are read as 16-byte items when they start aligned (a.soft4; the columns between C
// and ld_soft belong to the row and are read but neither stored nor compared), else as single floats, consecutive lanes taking
// consecutive items either way.  Destination rows lie C floats apart, so in general only 4-byte aligned: single-float stores.
// src == nullptr (a pool row outside the pool): a zero row.
__device__ __forceinline__ void soft_row(const PretrainArgs& a, const float* src, long long dest, int lane) {
  const int C = a.C;
  float* dst = a.label_targets ? a.label_targets + (size_t)dest * C : nullptr;
  float best = -__builtin_huge_valf();
  int at = 0x7fffffff;
  if (src == nullptr) {
    if (dst)
      for (int col = lane; col < C; col += 64) dst[col] = 0.f;
    best = 0.f; at = 1;                                // every column equal: the first one
  } else if (a.soft4) {
    const f32x4* sp = reinterpret_cast<const f32x4*>(src);
    const int n4 = (C + 3) >> 2;                       // <= ld_soft / 4
    for (int base = 0; base < n4; base += 512) {
      f32x4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int q = base + lane + 64 * k;
        v[k] = q < n4 ? sp[q] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int col = 4 * (base + lane + 64 * k);
        const float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (col + j < C) {
            if (dst) dst[col + j] = e[j];
            if (col + j >= 1 && e[j] > best) { best = e[j]; at = col + j; }      // ascending columns per lane: its first maximum
          }
        }
      }
    }
  } else {
    for (int base = 0; base < C; base += 1024) {
      float v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int col = base + lane + 64 * k;
        v[k] = col < C ? src[col] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int col = base + lane + 64 * k;
        if (col < C) {
          if (dst) dst[col] = v[k];
          if (col >= 1 && v[k] > best) { best = v[k]; at = col; }
        }
      }
    }
  }
  if (a.label_ids) {
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (lane == 0) a.label_ids[dest] = at == 0x7fffffff ? 1 : at;
  }
}

// MRC = false: uniter_collate_pretrain_batch;  MRC = true: uniter_collate_mrc_batch, whose dense outputs are MRFR's on its own
// stream (a.task is UNITER_TASK_MRFR) and whose selected rows carry soft labels instead of feat_targets.
template <bool MRC>
__global__ __launch_bounds__(256) void collate_pretrain_kernel(const PretrainArgs a) {
  __shared__ int sh[4];
  const CollateArgs& c = a.c;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x < c.region_blocks) {
    RegionItem it;
    if (!region_item(c, it)) return;
    // (everything up to `dest` is uniform over the wave)
    bool masked = false;
    long long dest = 0;                                // row of feat_targets | label_targets, label_ids and masked_positions
    if (a.task == UNITER_TASK_MRFR && it.r < it.n) masked = region_slot<MRC>(a, it.s, it.n, it.b, it.r, lane, dest);
    f32x4 v[4];
    piece_load(c, it, it.real && !(MRC && masked), lane, v);      // (MRC keeps no copy of a selected region's features)
    // a selected region leaves zeros in img_feat: MRFR moves its features to feat_targets, MRC its soft labels to label_targets
    if (masked) {
      if (!MRC) piece_store(c, it, lane, a.feat_targets, dest, v);
      else if (it.piece == 0) soft_row(a, it.real ? a.soft + (size_t)it.src_row * a.ld_soft : nullptr, dest, lane);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    piece_store(c, it, lane, c.img_feat, it.row, v);
    box_row(c, it, lane);
    if (it.piece == 0 && masked && lane == 0) {
      a.masked_positions[2 * dest] = it.b;
      a.masked_positions[2 * dest + 1] = (long long)c.ds.txt_len[text_sample_of(a, it.b)] + it.r;
    }
    return;
  }

  const int b = (int)(blockIdx.x - c.region_blocks);
  const long long s = sample_of(c, b), ts = text_sample_of(a, b);
  const int T = c.ds.T;
  const long long tl = c.ds.txt_len[ts];
  const int n = regions_of(c, s);
  const long long il = c.ragged ? n : c.R;
  const int64_t* src = c.ds.input_ids + (size_t)ts * T;

  if (a.task == UNITER_TASK_MLM) {
    // entries selected in the samples in front of this one
    int acc = 0;
    for (int bp = wave; bp < b; bp += 4) acc += mlm_count_wave(a, text_sample_of(a, bp), lane);
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    const int front = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    // this sample: is anything drawn at all?
    int drawn = 0;
    for (int base = 0; base < T; base += 256) {
      const int t = base + (int)threadIdx.x;
      u32x4 w;
      drawn += __syncthreads_count(t < T && mlm_drawn(a, ts, t, src[t], w));
    }
    const bool forced = drawn == 0;
    int run = 0;                                       // selected in the chunks already written
    for (int base = 0; base < T; base += 256) {
      const int t = base + (int)threadIdx.x;
      long long tok = 0;
      u32x4 w = u32x4{0u, 0u, 0u, 0u};
      bool f = false;
      if (t < T) {
        tok = src[t];
        f = mlm_drawn(a, ts, t, tok, w);
        if (forced) f = t == 1;
      }
      const unsigned long long bal = __ballot(f);
      if (lane == 0) sh[wave] = __popcll(bal);
      __syncthreads();
      int off = 0, chunk = 0;
      for (int k = 0; k < 4; ++k) { off += k < wave ? sh[k] : 0; chunk += sh[k]; }
      __syncthreads();
      if (t < T) {
        long long out_tok = tok;
        if (f) {
          if (forced || w.y < UNITER_MASK_KEEP80) out_tok = a.mask_token;
          else if (w.y < UNITER_MASK_KEEP90) out_tok = a.vocab_lo + (long long)(((unsigned long long)w.z * a.vocab_span) >> 32);
          const long long at = (long long)front + run + off + __popcll(bal & ((1ull << lane) - 1ull));      // < B * T
          a.masked_positions[2 * at] = b;
          a.masked_positions[2 * at + 1] = t;
        }
        c.input_ids[(size_t)b * T + t] = out_tok;
        a.txt_labels[(size_t)b * T + t] = f ? tok : -1;
      }
      run += chunk;
    }
    if (b == c.B - 1 && threadIdx.x == 0) *a.n_masked = front + run;
  }
  sample_frame(c, b, s, ts, tl, il, a.task != UNITER_TASK_MLM);
  if (a.task == UNITER_TASK_ITM && threadIdx.x == 0) a.targets[b] = ts == s ? 1 : 0;
  if (a.task == UNITER_TASK_MRFR) {
    int any = 0;
    for (int base = 0; base < n; base += 256) {
      const int r = base + (int)threadIdx.x;
      any |= __syncthreads_or(r < n && region_drawn<MRC>(a, s, r));
    }
    const int forced = (any || n == 0) ? -1 : region_forced<MRC>(a, s, n);
    for (int r = threadIdx.x; r < c.R; r += 256)
      a.img_masks[(size_t)b * c.R + r] = (r < n && (forced >= 0 ? r == forced : region_drawn<MRC>(a, s, r))) ? 1 : 0;
    for (int j = threadIdx.x; j < c.L_out; j += 256) {
      const long long r = j - tl;
      a.img_mask_tgt[(size_t)b * c.L_out + j] = (r >= 0 && r < n && (forced >= 0 ? r == forced : region_drawn<MRC>(a, s, (int)r))) ? 1 : 0;
    }
    if (b == c.B - 1) {
      int cnt = 0;
      for (int bp = threadIdx.x; bp < c.B; bp += 256) cnt += region_count_serial<MRC>(a, sample_of(c, bp));
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if (lane == 0) sh[wave] = cnt;
      __syncthreads();
      if (threadIdx.x == 0) *a.n_masked = sh[0] + sh[1] + sh[2] + sh[3];
    }
  }
}

// the draw fields of a from a checked mask configuration: the Philox key and counter word, prob as a threshold on a 32-bit word
int mask_draw(const char* who, PretrainArgs& a, const uniter_mask_cfg_t* cfg) {
  UCHECK_ARG(cfg, "%s: null mask configuration", who);
  UCHECK_ARG(cfg->prob >= 0.0f && cfg->prob <= 1.0f, "%s: prob = %g is outside [0, 1]", who, (double)cfg->prob);
  a.k0 = (uint32_t)(cfg->seed & 0xffffffffu); a.k1 = (uint32_t)(cfg->seed >> 32); a.draw = cfg->draw;
  const double t = (double)cfg->prob * 4294967296.0;         // make_drop's floor and clamp (philox.h)
  a.always = cfg->prob >= 1.0f;
  a.thresh = t >= 4294967295.0 ? 0xffffffffu : (t <= 0.0 ? 0u : (uint32_t)t);
  return 0;
}

}  // namespace

extern "C" int uniter_collate_pretrain_batch(const uniter_dataset_t* ds, const int64_t* sel, const int64_t* txt_sel, int task,
                                             const uniter_mask_cfg_t* cfg, int B, int R, int L_out, int flags, float* img_feat,
                                             float* img_pos_feat, int64_t* input_ids, int64_t* position_ids, int64_t* token_type_ids,
                                             float* attn_mask, int64_t* gather_index, int64_t* labels, int64_t* ids,
                                             int64_t* txt_labels, int64_t* img_masks, unsigned char* img_mask_tgt, float* feat_targets,
                                             int64_t* targets, int64_t* masked_positions, int32_t* n_masked, void* stream) {
  UCHECK_ARG(task == UNITER_TASK_MLM || task == UNITER_TASK_MRFR || task == UNITER_TASK_ITM,
             "collate_pretrain_batch: unknown task %d", task);
  PretrainArgs a = {};                                       // (what a task does not use stays null / 0)
  UCHECK_RC(fill_args("collate_pretrain_batch", a.c, ds, sel, B, R, L_out, flags, img_feat, img_pos_feat, input_ids, position_ids,
                      token_type_ids, attn_mask, gather_index, labels, ids));
  if (task != UNITER_TASK_ITM) {
    UCHECK_RC(mask_draw("collate_pretrain_batch", a, cfg));
    // (MRFR with R == 0: no region can be selected, masked_positions has no rows)
    UCHECK_ARG((masked_positions || (task == UNITER_TASK_MRFR && R == 0)) && n_masked,
               "collate_pretrain_batch: null masked_positions / n_masked");
  }
  if (task == UNITER_TASK_MLM) {
    UCHECK_ARG(txt_labels, "collate_pretrain_batch: null txt_labels");
    UCHECK_ARG(cfg->vocab_hi > cfg->vocab_lo && (unsigned long long)(cfg->vocab_hi - cfg->vocab_lo) <= (1ull << 32),
               "collate_pretrain_batch: vocabulary range [%lld, %lld) is empty or holds more than 2^32 ids", (long long)cfg->vocab_lo,
               (long long)cfg->vocab_hi);
    UCHECK_SHAPE(ds->T >= 2, "collate_pretrain_batch: MLM needs T >= 2 (a sample without a drawn token takes position 1); T = %d", ds->T);
    a.cls = cfg->cls; a.sep = cfg->sep; a.pad = cfg->pad; a.mask_token = cfg->mask_token; a.vocab_lo = cfg->vocab_lo;
    a.vocab_span = (unsigned long long)(cfg->vocab_hi - cfg->vocab_lo);
  } else if (task == UNITER_TASK_MRFR) {
    UCHECK_ARG(img_mask_tgt && ((img_masks && feat_targets) || R == 0),
               "collate_pretrain_batch: null img_masks / img_mask_tgt / feat_targets with R = %d", R);
    UCHECK_ARG(((uintptr_t)feat_targets & 15) == 0, "collate_pretrain_batch: feat_targets is not 16-byte aligned");
  } else {
    UCHECK_ARG(targets, "collate_pretrain_batch: null targets");
  }
  a.txt_sel = txt_sel; a.task = task;
  a.txt_labels = txt_labels; a.img_masks = img_masks; a.img_mask_tgt = img_mask_tgt; a.feat_targets = feat_targets;
  a.targets = targets; a.masked_positions = masked_positions; a.n_masked = n_masked;
  hipLaunchKernelGGL(collate_pretrain_kernel<false>, dim3(a.c.region_blocks + (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  UCHECK_LAUNCH();
  return 0;
}

// ---- masked region classification: MRFR's batch on its own stream, soft labels and their classes in place of feat_targets ------
extern "C" int uniter_collate_mrc_batch(const uniter_dataset_t* ds, const float* soft, int C, int ld_soft, const int64_t* sel,
                                        const uniter_mask_cfg_t* cfg, int B, int R, int L_out, int flags, float* img_feat,
                                        float* img_pos_feat, int64_t* input_ids, int64_t* position_ids, int64_t* token_type_ids,
                                        float* attn_mask, int64_t* gather_index, int64_t* labels, int64_t* ids, int64_t* img_masks,
                                        unsigned char* img_mask_tgt, float* label_targets, int64_t* label_ids,
                                        int64_t* masked_positions, int32_t* n_masked, void* stream) {
  PretrainArgs a = {};
  UCHECK_RC(fill_args("collate_mrc_batch", a.c, ds, sel, B, R, L_out, flags, img_feat, img_pos_feat, input_ids, position_ids,
                      token_type_ids, attn_mask, gather_index, labels, ids));
  UCHECK_RC(mask_draw("collate_mrc_batch", a, cfg));
  UCHECK_ARG(soft || ds->pool_rows == 0, "collate_mrc_batch: null soft labels with %lld pool rows", (long long)ds->pool_rows);
  UCHECK_SHAPE(C >= 2 && ld_soft >= C, "collate_mrc_batch: C = %d, ld_soft = %d (C >= 2: a background and a class; ld_soft >= C)", C, ld_soft);
  UCHECK_ARG(((uintptr_t)soft & 3) == 0 && ((uintptr_t)label_targets & 3) == 0, "collate_mrc_batch: soft / label_targets is not 4-byte aligned");
  // (R == 0: both have no elements, and an empty tensor's pointer is null)
  UCHECK_ARG(label_targets || label_ids || R == 0, "collate_mrc_batch: label_targets and label_ids are both null with R = %d", R);
  UCHECK_ARG(n_masked && img_mask_tgt && ((masked_positions && img_masks) || R == 0),
             "collate_mrc_batch: null masked_positions / n_masked / img_masks / img_mask_tgt with R = %d", R);
  a.task = UNITER_TASK_MRFR;                                 // the dense outputs are MRFR's, on UNITER_STREAM_MRC
  a.img_masks = img_masks; a.img_mask_tgt = img_mask_tgt; a.masked_positions = masked_positions; a.n_masked = n_masked;
  a.soft = soft; a.C = C; a.ld_soft = ld_soft; a.soft4 = ((uintptr_t)soft & 15) == 0 && ld_soft % 4 == 0;
  a.label_targets = label_targets; a.label_ids = label_ids;
  hipLaunchKernelGGL(collate_pretrain_kernel<true>, dim3(a.c.region_blocks + (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  UCHECK_LAUNCH();
  return 0;
}
