// Gradients with respect to the model's INPUTS:
//   uniter_txt_embed_bwd_rows  per-token gradient of the sum that enters the text embeddings' LayerNorm
//                              (autograd of model/model.py:232-245 with respect to words_embeddings)
//   uniter_pos_feat_dgrad      d_pos7 = d_posfc @ Wp (autograd of pos_linear, model/model.py:268, with respect to img_pos_feat)
// The region-feature gradient is the schedule's own dense product (model.cpp); the perturbed text forward is an instantiation of
// the text row kernel (embed.hip); the update of an adversarial perturbation from these gradients is adv.hip's.
//
// Row kernels in the style of embed.hip: one wave per row, 16-byte accesses, H % 4 == 0, H <= 1024.  No float atomics anywhere:
// every result is a function of the inputs alone, every output element has one writer and is overwritten.
#include "common.h"
#include "gemm_internal.h"
#include "philox.h"
#include "rowops.h"

namespace {

__device__ __forceinline__ int clampi(long long v, int hi) { return v < 0 ? 0 : (v >= hi ? hi - 1 : (int)v); }

struct RowsArgs {
  const float* dcat; const int64_t* ids; const int64_t* pos_ids; const int64_t* type_ids;
  const float* word; const float* pos; const float* type; const float* gamma; const float* delta;
  float* d_rows;
  int B, T, S, H, vocab, max_pos, type_vocab, pos_bcast;
  DropCfg drop;
};

// The row pass of txt_embed_bwd_kernel (embed.hip), statement for statement, with the row's gradient stored to d_rows[row] and
// nothing else kept: the same operations in the same order, so d_rows[row] is bit for bit what the deterministic backward adds to a
// table row that this row alone reads.
template <int NV>
__global__ __launch_bounds__(256) void txt_embed_bwd_rows_kernel(const RowsArgs a) {
  const int lane = threadIdx.x & 63, H4 = a.H >> 2;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.T) return;
  const int b = row / a.T, t = row - b * a.T;
  f32x4 g[NV], dg[NV], db[NV], d[NV], e[NV], w[NV];
  row_load<NV>(g, a.gamma, H4, lane);
#pragma unroll
  for (int k = 0; k < NV; ++k) { dg[k] = f32x4{0, 0, 0, 0}; db[k] = dg[k]; }
  row_load<NV>(d, a.dcat + ((size_t)b * a.S + t) * a.H, H4, lane);
  if (a.drop.active) row_dropout<NV>(d, a.drop, (uint64_t)row * H4, H4, lane);
  const int id = clampi(a.ids[row], a.vocab);
  const int pid = clampi(a.pos_ids[a.pos_bcast ? t : row], a.max_pos);
  const int tt = a.type_ids ? clampi(a.type_ids[row], a.type_vocab) : 0;
  row_load<NV>(e, a.word + (size_t)id * a.H, H4, lane);
  if (a.delta) {                                                  // (uniform per launch)
    row_load<NV>(w, a.delta + (size_t)row * a.H, H4, lane);
#pragma unroll
    for (int k = 0; k < NV; ++k) e[k] += w[k];
  }
  row_load<NV>(w, a.pos + (size_t)pid * a.H, H4, lane);
#pragma unroll
  for (int k = 0; k < NV; ++k) e[k] += w[k];
  row_load<NV>(w, a.type + (size_t)tt * a.H, H4, lane);
#pragma unroll
  for (int k = 0; k < NV; ++k) e[k] += w[k];
  float mean, rstd;
  row_stats<NV>(e, a.H, H4, lane, mean, rstd);
  row_ln_bwd<NV>(d, e, g, mean, rstd, dg, db, a.H, H4, lane);     // d <- d(sum of the lookups and the perturbation)
  row_store<NV>(d, a.d_rows + (size_t)row * a.H, H4, lane);
}

// d_pos7[row][k] = sum_c d_posfc[row][c] * Wp[c][k].  One wave per row; lane l owns the 16-byte chunks l, l + 64, ... of the row and
// the 7 x 4 weights that belong to each (112 contiguous bytes, seven 16-byte loads).  The chunk loop has NV trips for EVERY lane -- the
// bound is the template parameter, the row's end is a predicate inside -- and the seven wave sums follow it, outside any loop: no
// shuffle runs under a trip count that differs between lanes.
template <int NV>
__global__ __launch_bounds__(256) void pos_feat_dgrad_kernel(const float* __restrict__ d_posfc, const float* __restrict__ Wp,
                                                             float* __restrict__ d_pos7, int rows, int H) {
  const int lane = threadIdx.x & 63, H4 = H >> 2;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                        // (whole waves leave: the row index is uniform in a wave)
  f32x4 d[NV];
  row_load<NV>(d, d_posfc + (size_t)row * H, H4, lane);
  float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < NV; ++kk) {
    const int c4 = lane + 64 * kk;
    if (c4 < H4) {
      const f32x4* wp = reinterpret_cast<const f32x4*>(Wp + (size_t)c4 * 28);
      float w[28];
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        const f32x4 v = wp[q];
        w[4 * q] = v[0]; w[4 * q + 1] = v[1]; w[4 * q + 2] = v[2]; w[4 * q + 3] = v[3];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < 7; ++k) s[k] += d[kk][e] * w[e * 7 + k];
    }
  }
  float o = 0.f;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const float t = wave_sum(s[k]);
    if (lane == k) o = t;
  }
  if (lane < 7) d_pos7[(size_t)row * 7 + lane] = o;
}

}  // namespace

#define IG_NV_DISPATCH(KERNEL, GRID, ...)                                                      \
  switch ((H / 4 + 63) / 64) {                                                                 \
    case 1: hipLaunchKernelGGL((KERNEL<1>), GRID, dim3(256), 0, st, __VA_ARGS__); break;       \
    case 2: hipLaunchKernelGGL((KERNEL<2>), GRID, dim3(256), 0, st, __VA_ARGS__); break;       \
    case 3: hipLaunchKernelGGL((KERNEL<3>), GRID, dim3(256), 0, st, __VA_ARGS__); break;       \
    default: hipLaunchKernelGGL((KERNEL<4>), GRID, dim3(256), 0, st, __VA_ARGS__); break;      \
  }

// the per-token pass behind the text side's gradient pass: the same call (rowpass_internal.h), its d_rows written
int txt_embed_bwd_rows_run(const TxtEmbedCall& c) {
  const int H = c.H;
  UCHECK_ARG(c.dcat && c.ids && c.pos_ids && c.word && c.pos && c.type && c.gamma && c.d_rows, "txt_embed_bwd_rows: null pointer");
  UCHECK_ARG((((uintptr_t)c.delta | (uintptr_t)c.d_rows) & 15) == 0, "txt_embed_bwd_rows: delta and d_rows must be 16-byte aligned");
  UCHECK_SHAPE(H > 0 && H % 4 == 0 && H <= 1024 && c.T <= c.S, "txt_embed_bwd_rows: bad shape (H %% 4, H <= 1024, T <= S)");
  if (c.B * c.T <= 0) return 0;
  RowsArgs a = {};
  a.dcat = c.dcat; a.ids = c.ids; a.pos_ids = c.pos_ids; a.type_ids = c.type_ids; a.word = c.word; a.pos = c.pos; a.type = c.type;
  a.gamma = c.gamma; a.delta = c.delta; a.d_rows = c.d_rows; a.B = c.B; a.T = c.T; a.S = c.S; a.H = H; a.vocab = c.vocab;
  a.max_pos = c.max_pos; a.type_vocab = c.type_vocab; a.pos_bcast = c.pos_bcast; a.drop = make_drop(c.drop);
  hipStream_t st = (hipStream_t)c.stream;
  IG_NV_DISPATCH(txt_embed_bwd_rows_kernel, dim3((c.B * c.T + 3) / 4), a);
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_txt_embed_bwd_rows(const float* dcat, const int64_t* input_ids, const int64_t* position_ids, const int64_t* type_ids,
                                         const float* word, const float* pos, const float* type, const float* gamma, const float* delta,
                                         float* d_rows, int B, int T, int S, int H, int vocab, int max_pos, int type_vocab, int pos_bcast,
                                         float p_drop, uint64_t seed, uint32_t offset, void* stream) {
  TxtEmbedCall c;
  c.dcat = dcat; c.ids = input_ids; c.pos_ids = position_ids; c.type_ids = type_ids; c.word = word; c.pos = pos; c.type = type;
  c.gamma = gamma; c.delta = delta; c.d_rows = d_rows; c.B = B; c.T = T; c.S = S; c.H = H; c.vocab = vocab; c.max_pos = max_pos;
  c.type_vocab = type_vocab; c.pos_bcast = pos_bcast; c.drop = {p_drop, seed, offset, SITE_TXT_EMB}; c.stream = stream;
  return txt_embed_bwd_rows_run(c);
}

extern "C" int uniter_pos_feat_dgrad(const float* d_posfc, const float* Wp, float* d_pos7, int rows, int H, void* stream) {
  UCHECK_ARG(d_posfc && Wp && d_pos7, "pos_feat_dgrad: null pointer");
  UCHECK_ARG((((uintptr_t)d_posfc | (uintptr_t)Wp) & 15) == 0, "pos_feat_dgrad: d_posfc and Wp must be 16-byte aligned");
  UCHECK_SHAPE(H > 0 && H % 4 == 0 && H <= 1024, "pos_feat_dgrad: bad shape (H %% 4, H <= 1024)");
  if (rows <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  IG_NV_DISPATCH(pos_feat_dgrad_kernel, dim3((rows + 3) / 4), d_posfc, Wp, d_pos7, rows, H);
  UCHECK_LAUNCH();
  return 0;
}
