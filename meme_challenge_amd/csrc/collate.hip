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

__global__ __launch_bounds__(256) void collate_batch_kernel(const CollateArgs a) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x < a.region_blocks) {
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.region_items) return;
    const long long row = item / a.pieces;             // b * R + r
    const int piece = (int)(item - row * a.pieces);
    const int b = (int)(row / a.R), r = (int)(row - (long long)b * a.R);
    const long long s = sample_of(a, b);
    const long long src_row = a.ds.row_start[s] + r;
    // a pool row outside the pool reads as padding (never dereferenced)
    const bool real = r < regions_of(a, s) && src_row >= 0 && src_row < a.ds.pool_rows;
    f32x4* dp = reinterpret_cast<f32x4*>(a.img_feat) + (size_t)row * a.D4;
    const int c0 = piece * PIECE4 + lane;
    f32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (real) {
      const f32x4* sp = reinterpret_cast<const f32x4*>(a.ds.feat) + (size_t)src_row * a.D4;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + 64 * k < a.D4) v[k] = sp[c0 + 64 * k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + 64 * k < a.D4) dp[c0 + 64 * k] = v[k];
    if (piece == 0 && lane < 7)
      a.img_pos_feat[(size_t)row * 7 + lane] = real ? a.ds.pos[(size_t)src_row * 7 + lane] : 0.f;
    return;
  }
  const int b = (int)(blockIdx.x - a.region_blocks);
  const long long s = sample_of(a, b);
  const int T = a.ds.T;
  const long long tl = a.ds.txt_len[s];
  const long long il = a.ragged ? regions_of(a, s) : a.R;
  for (int t = threadIdx.x; t < T; t += 256) {
    a.input_ids[(size_t)b * T + t] = a.ds.input_ids[(size_t)s * T + t];
    a.position_ids[(size_t)b * T + t] = t;
    if (a.token_type_ids) a.token_type_ids[(size_t)b * T + t] = a.ds.token_type_ids[(size_t)s * T + t];
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

}  // namespace

extern "C" int uniter_collate_batch(const uniter_dataset_t* ds, const int64_t* sel, int B, int R, int L_out, int flags,
                                    float* img_feat, float* img_pos_feat, int64_t* input_ids, int64_t* position_ids,
                                    int64_t* token_type_ids, float* attn_mask, int64_t* gather_index, int64_t* labels,
                                    int64_t* ids, void* stream) {
  UCHECK_ARG(ds && sel, "collate_batch: null dataset or selection");
  UCHECK_ARG(ds->row_start && ds->row_cnt && ds->input_ids && ds->txt_len && ds->labels && ds->ids,
             "collate_batch: null pointer in the dataset");
  UCHECK_ARG(input_ids && position_ids && attn_mask && gather_index && labels && ids, "collate_batch: null output pointer");
  UCHECK_ARG(ds->N > 0 && ds->pool_rows >= 0, "collate_batch: dataset of %lld samples, %lld pool rows", (long long)ds->N,
             (long long)ds->pool_rows);
  UCHECK_SHAPE(B > 0 && ds->T > 0 && L_out > 0 && R >= 0, "collate_batch: B = %d, T = %d, L_out = %d, R = %d (B, T, L_out > 0, R >= 0)", B,
               ds->T, L_out, R);
  UCHECK_SHAPE((long long)L_out <= (long long)ds->T + R, "collate_batch: L_out = %d exceeds T + R = %d + %d", L_out, ds->T, R);
  UCHECK_SHAPE(ds->D > 0 && ds->D % 4 == 0, "collate_batch: D = %d must be a positive multiple of 4 (rows move as 16-byte items)", ds->D);
  // an empty pool (every sample's confidence filter left nothing) has no rows to point at; R == 0 has no region output
  UCHECK_ARG((ds->feat && ds->pos) || ds->pool_rows == 0, "collate_batch: null feat / pos with %lld pool rows", (long long)ds->pool_rows);
  UCHECK_ARG((img_feat && img_pos_feat) || R == 0, "collate_batch: null img_feat / img_pos_feat with R = %d", R);
  UCHECK_ARG(((uintptr_t)ds->feat & 15) == 0, "collate_batch: feat is not 16-byte aligned");
  UCHECK_ARG(((uintptr_t)img_feat & 15) == 0, "collate_batch: img_feat is not 16-byte aligned");
  CollateArgs a;
  a.ds = *ds;
  if (!token_type_ids || !ds->token_type_ids) token_type_ids = nullptr;
  a.sel = sel; a.B = B; a.R = R; a.L_out = L_out; a.ragged = flags & 1;
  a.D4 = ds->D / 4;
  a.pieces = (a.D4 + PIECE4 - 1) / PIECE4;
  a.region_items = (long long)B * R * a.pieces;
  const long long region_blocks = (a.region_items + 3) / 4;
  UCHECK_SHAPE(region_blocks + B < 0x7fffffffLL, "collate_batch: %lld region items exceed one launch", a.region_items);
  a.region_blocks = (unsigned)region_blocks;
  a.img_feat = img_feat; a.img_pos_feat = img_pos_feat; a.input_ids = input_ids; a.position_ids = position_ids;
  a.token_type_ids = token_type_ids; a.attn_mask = attn_mask; a.gather_index = gather_index; a.labels = labels; a.ids = ids;
  hipLaunchKernelGGL(collate_batch_kernel, dim3(a.region_blocks + (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  UCHECK_LAUNCH();
  return 0;
}
