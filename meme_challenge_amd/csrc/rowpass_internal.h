// The row passes behind the C ABI (layernorm.hip, embed.hip, input_grads.hip) as the schedule (model.cpp) calls them: one description of
// a LayerNorm row pass (LnCall) and of an embedding pass per side (TxtEmbedCall, ImgEmbedCall), the launchers that take them, and the
// partial-sum helpers the files share.  An unset field means "absent".  Only the extern "C" functions turn positional lists into a call.
#pragma once
#include "common.h"
#include "philox.h"

// ---- partial sums and small row helpers ----
int launch_add_f32(float* out, const float* a, const float* b, size_t n, hipStream_t st);
struct PartialSums { const float* part; int nparts; size_t stride; };      // nparts rows of `stride` floats
// out[n] (+)= sum_p part[p*stride + n]
int finalize_partials(const PartialSums& p, float* out, int N, int beta, hipStream_t st);
// second pass of the order-fixed column sums (uniter_colsum_*_add_det): out[c] = out[c] + (((P0 + P1) + P2) + ...) over part[nblocks][cols]
int colsum_det_finish(const float* part, int nblocks, int cols, float* out, hipStream_t st);
// outs[j][c] += sum_p part[p*stride + j*H + c] for j < nout (<= 8); NULL outputs skipped
int finalize_partials_multi(const PartialSums& p, float* const* outs, int nout, int H, hipStream_t st);
// up to 4 jobs: job i accumulates nout[i] (<= 3) outputs of seg[i] columns each out of part[i] (nparts[i] rows of stride[i] floats)
struct PartialJobs {
  const float* const* part; const int* nparts; const size_t* stride;
  float* const (*outs)[3]; const int* nout; const int* seg;
};
int finalize_partials_jobs(int njobs, const PartialJobs& j, hipStream_t st);
int ln_bwd_partial_rows(int M);
int launch_masked_rowsum(const float* x, const int64_t* masks, float* out, int rows, int D, hipStream_t st);

// ---- LayerNorm row passes: layernorm.hip ----
// Forward (ln_fwd_run): y = LayerNorm(dropout(sum of the x slabs) + res); z takes the LayerNorm's input, out takes y, copy its operand
// format, mean / rstd (both or neither) the row statistics.  Backward (ln_bwd_rows_run): x = the dy slabs; z, mean, rstd, gamma are
// read; dz takes the gradient of the LayerNorm's input, out (dx) and copy that gradient through the dropout; ws takes the column
// partials that uniter_ln_bwd_finalize reduces (want_dbias: the third set, the bias gradient of the product in front).
struct LnCall {
  const float* x = nullptr;          // nslab slabs [M][H], slab s at x + s * slab_stride (one slab: any stride)
  int nslab = 1;
  size_t slab_stride = 0;
  const float *res = nullptr, *gamma = nullptr, *beta = nullptr;
  float *z = nullptr, *dz = nullptr, *out = nullptr;
  void* copy = nullptr;              // out as bf16 (pieces = 1) or as its three x3 pieces (pieces = 3: H % 8 == 0, 16-byte aligned)
  int pieces = 1;
  float *mean = nullptr, *rstd = nullptr;
  int want_dbias = 0;
  int M = 0, H = 0;
  DropSite drop;
  int drop_row_step = 1;             // row r draws the dropout of row r * drop_row_step of the site (a pass over every step-th row, compacted)
  void* ws = nullptr;
  size_t ws_bytes = 0;
  void* stream = nullptr;
};
int ln_fwd_run(const LnCall& c);
int ln_bwd_rows_run(const LnCall& c);

// ---- embeddings: embed.hip, input_grads.hip ----
// The text side, forward (cat) or backward (dcat and the gradients; d_rows: the per-token pass of input_grads.hip).  delta [B, T, H]: a
// perturbation of the word rows, NULL = none.  det: the order-fixed backward (uniter_txt_embed_bwd_det) and its workspace.
struct TxtEmbedCall {
  const int64_t *ids = nullptr, *pos_ids = nullptr, *type_ids = nullptr;
  const float *word = nullptr, *pos = nullptr, *type = nullptr, *gamma = nullptr, *beta = nullptr, *delta = nullptr;
  float* cat = nullptr;
  const float* dcat = nullptr;
  float *dword = nullptr, *dpos = nullptr, *dtype = nullptr, *dgamma = nullptr, *dbeta = nullptr, *d_rows = nullptr;
  int B = 0, T = 0, S = 0, H = 0, vocab = 0, max_pos = 0, type_vocab = 0, pos_bcast = 0;
  DropSite drop;                     // site: SITE_TXT_EMB
  int det = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  void* stream = nullptr;
};
int txt_embed_fwd_run(const TxtEmbedCall& c);
int txt_embed_bwd_run(const TxtEmbedCall& c);
int txt_embed_bwd_rows_run(const TxtEmbedCall& c);

// The image side behind the region projection imgfc [B * R, H]; stats: the three LayerNorms' row statistics a training forward saves.
struct ImgEmbedCall {
  const float *imgfc = nullptr, *pos7 = nullptr;
  const int64_t* type_ids = nullptr;
  const float *Wp = nullptr, *bp = nullptr, *type = nullptr;
  const float *g_i = nullptr, *b_i = nullptr, *g_p = nullptr, *b_p = nullptr, *g_f = nullptr, *b_f = nullptr;
  float *cat = nullptr, *stats = nullptr;
  const float* dcat = nullptr;
  float *d_imgfc = nullptr, *d_posfc = nullptr, *dWp = nullptr, *dbp = nullptr, *dtype = nullptr;
  float *dg_i = nullptr, *db_i = nullptr, *dg_p = nullptr, *db_p = nullptr, *dg_f = nullptr, *db_f = nullptr;
  int B = 0, R = 0, T0 = 0, S = 0, H = 0, type_vocab = 0;
  DropSite drop;                     // site: SITE_IMG_EMB
  int det = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  void* stream = nullptr;
};
int img_embed_fwd_run(const ImgEmbedCall& c);
int img_embed_bwd_run(const ImgEmbedCall& c);
