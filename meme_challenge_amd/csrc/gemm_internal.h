// Host-side declarations shared by the kernel files and the schedule (model.cpp), stated once: the internal entry points behind the
// C ABI, and the two rules every persistent launch shares (band height of the tile walk, grid cap).  The defining file and every
// user include this header, so a changed signature fails where it is defined, at compile time.
#pragma once
#include "common.h"

// ---- dense products: gemm_f32.hip, gemm_bf16.hip, gemm_bf16_dma.hip, gemm_bf16_p.hip, gemm_split3.hip ----
// no_sk (the three *_run below): never the stream-K form, whose partial tiles meet in float atomics in arrival order -- a C += then
// runs on whole tiles, one adder per element (the plans of uniter_model_set_deterministic).  gemm_bf16v2_run has no such form: its
// C += is one workgroup per tile (split-K with beta is refused).
// lo (every launcher below; no default: a forgotten argument does not compile): the stamp slot, wave priority and CU reserve of THIS
// launch (common.h).  A launcher that forwards to another hands lo on whole.  gemm_bf16_run / gemm_bf16res_run's own kernels and the
// grouped weight-gradient launches set no wave priority: they ignore lo.prio.
int gemm_f32_run(int cfg, int tag, int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda,
                 const float* B, int ldb, float* C, int ldc, int epilogue, const float* bias,
                 const float* aux_in, float* aux_out, int ld_aux, int beta, float* colsum_part, void* stream,
                 const LaunchOpts& lo, int no_sk = 0);
int gemm_bf16_run(int cfg, int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda,
                  const float* B, int ldb, float* C, int ldc, int epilogue, const float* bias,
                  const float* aux_in, float* aux_out, int ld_aux, int beta, float* colsum_part, void* stream,
                  const LaunchOpts& lo, int no_sk = 0);
int gemm_bf16res_run(int cfg, int a_kmajor, int b_kmajor, int M, int N, int K, const void* A, int lda, const void* B,
                     int ldb, float* C, int ldc, void* Cb, int ldcb, int epilogue, const float* bias,
                     const float* aux_in, float* aux_out, int ld_aux, int beta, float* colsum_part, void* stream,
                     const LaunchOpts& lo, int no_sk = 0);
int gemm_bf16v2_run(int cfg, int nsplit, int a_kmajor, int b_kmajor, int M, int N, int K, const void* A, int lda,
                    const void* B, int ldb, float* C, int ldc, long c_split_stride, void* Cb, int ldcb, int epilogue,
                    const float* bias, const void* aux_in, int aux_in_bf16, void* aux_out, int aux_out_bf16,
                    int ld_aux, int beta, void* stream, const LaunchOpts& lo);
int gemm_f32_wgrad_group(int n, const int* Mo, const int* No, int K, const float* const* A, const float* const* B,
                         float* const* dW, int overwrite, void* stream, const LaunchOpts& lo);
int gemm_x3_run(int cfg, int nsplit, int a_kmajor, int b_kmajor, int M, int N, int K, const void* A, int lda, int psa,
                const void* B, int ldb, int psb, float* C, int ldc, long c_split_stride, void* Cx, int ldcx, int pscx,
                int epilogue, const float* bias, const float* aux_in, float* aux_out, int ld_aux, void* stream,
                float* colsum_part, void* sk_ws, size_t sk_ws_bytes, const LaunchOpts& lo);
size_t gemm_x3_sk_ws_bytes();
int gemm_x3_wgrad_default_cfg();
int gemm_x3_pick_split(int M, int N, int K);
int gemm_x3_pick_split_on(int M, int N, int K, int avail, int cu_reserve);
int gemm_x3_wgrad_group(int cfg, int n, const int* Mo, const int* No, int K, const void* const* A, const void* const* B,
                        float* const* dW, void* stream, int overwrite, int max_wgs, uniter_x3_riders_t* riders,
                        void* sk_ws, size_t sk_ws_bytes, const LaunchOpts& lo);
int gemm_x3_wgrad_group_slots(int cfg, int n, const int* Mo, const int* No, int max_wgs, int K, size_t sk_ws_bytes, int cu_reserve);
int gemm_x3_wgrad_group_balanced_wgs(int cfg, int n, const int* Mo, const int* No, int cu_reserve);
int gemm_bf16v2_pick_split(int M, int N, int K);
int gemm_b1p_pick_split(int M, int N, int K, int avail, int cu_reserve);
int gemm_b1p_run(int cfg, int nsplit, int b_kmajor, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                 float* C, int ldc, long c_split_stride, void* Cb, int ldcb, int epilogue, const float* bias,
                 const void* aux_in, int aux_in_bf16, void* aux_out, int aux_out_bf16, int ld_aux, float* colpart, void* stream,
                 const LaunchOpts& lo);
int gemm_b1p_wgrad_group(int n, const int* Mo, const int* No, int K, const void* const* A, const void* const* B, float* const* dW,
                         void* stream, int overwrite, int max_wgs, uniter_x3_riders_t* riders, const LaunchOpts& lo);
int gemm_b1p_wgrad_group_slots(int n, const int* Mo, const int* No, int max_wgs, int cu_reserve);
int gemm_bf16v2_wgrad_pieces(int M, int N, int K);
int gemm_bf16v2_wgrad_group(int cfg, int n, const int* Mo, const int* No, int K, const void* const* A,
                            const void* const* B, float* const* dW, void* stream, int overwrite, int max_wgs,
                            uniter_x3_riders_t* riders, const LaunchOpts& lo);
int gemm_bf16v2_wgrad_group_slots(int n, const int* Mo, const int* No, int max_wgs, int cu_reserve);
int gemm_bf16v2_wgrad_group_balanced_wgs(int n, const int* Mo, const int* No, int cu_reserve);

// ---- row passes: layernorm.hip, embed.hip ----
int launch_add_f32(float* out, const float* a, const float* b, size_t n, hipStream_t st);
// out[n] (+)= sum_p part[p*stride + n]
int finalize_partials(const float* part, int nparts, size_t stride, float* out, int N, int beta, hipStream_t st);
// second pass of the order-fixed column sums (uniter_colsum_*_add_det): out[c] = out[c] + (((P0 + P1) + P2) + ...) over part[nblocks][cols]
int colsum_det_finish(const float* part, int nblocks, int cols, float* out, hipStream_t st);
// outs[j][c] += sum_p part[p*stride + j*H + c] for j < nout (<= 8); NULL outputs skipped
int finalize_partials_multi(const float* part, int nparts, size_t stride, float* const* outs, int nout, int H,
                            hipStream_t st);
int finalize_partials_jobs(int njobs, const float* const* part, const int* nparts, const size_t* stride,
                           float* const (*outs)[3], const int* nout, const int* seg, hipStream_t st);
int ln_bwd_partial_rows(int M);
// The LayerNorm row passes behind uniter_ln_fwd_slabs(_x3) / uniter_ln_bwd_rows_slabs(_x3): pieces = 1 (bf16 copy) or 3 (x3 copy, which needs
// H % 8 == 0 and a 16-byte aligned buffer: the caller checks), keep_bits = this pass's dropout keep flags drawn ahead or NULL = draw them
int ln_fwd_run(const float* x, int nslab, size_t slab_stride, const float* res, const float* gamma, const float* beta, float* z_out,
               float* y, void* y_copy, int pieces, float* mean, float* rstd, int M, int H, float p_drop, uint64_t seed, uint32_t offset,
               uint32_t site, const unsigned char* keep_bits, void* stream);
int ln_bwd_rows_run(const float* dy, int nslab, size_t slab_stride, const float* z, const float* mean, const float* rstd,
                    const float* gamma, float* dz, float* dx, void* dx_copy, int pieces, int want_dbias, int M, int H, float p_drop,
                    uint64_t seed, uint32_t offset, uint32_t site, const unsigned char* keep_bits, void* ws, size_t ws_bytes, void* stream);
// the text embedding backward (uniter_txt_embed_bwd / _det) behind a forward pass with a perturbation of the word rows: delta [B, T, H]
// as uniter_txt_embed_fwd_delta had it, NULL = none (the public entry points)
int txt_embed_bwd_run(const float* dcat, const int64_t* input_ids, const int64_t* position_ids, const int64_t* type_ids,
                      const float* word, const float* pos, const float* type, const float* gamma, const float* delta, float* dword,
                      float* dpos, float* dtype, float* dgamma, float* dbeta, int B, int T, int S, int H, int vocab, int max_pos,
                      int type_vocab, int pos_bcast, float p_drop, uint64_t seed, uint32_t offset, void* ws, size_t ws_bytes,
                      void* stream);
int txt_embed_bwd_det_run(const float* dcat, const int64_t* input_ids, const int64_t* position_ids, const int64_t* type_ids,
                          const float* word, const float* pos, const float* type, const float* gamma, const float* delta, float* dword,
                          float* dpos, float* dtype, float* dgamma, float* dbeta, int B, int T, int S, int H, int vocab, int max_pos,
                          int type_vocab, int pos_bcast, float p_drop, uint64_t seed, uint32_t offset, void* ws, size_t ws_bytes,
                          void* stream);
int launch_masked_rowsum(const float* x, const int64_t* masks, float* out, int rows, int D, hipStream_t st);

// ---- attention backward: attention_f32.hip, attention_x3.hip, attention_bf16.hip ----
// The entry points behind uniter_attn_bwd_ex(_x3) (pieces = 1 / 3), uniter_attn_x3_bwd, uniter_attn_b16x_bwd and uniter_attn_bf16_bwd with the
// order of their bias partials as an argument: det = the per-sample partials are summed in a fixed order.
int attn_bwd_ex_run(const float* qkv, const float* attn_mask, const int32_t* cu_seqlens, const float* ctx, const float* lse,
                    const float* dctx, float* dqkv, void* dqkv_copy, int pieces, float* bias_part, const void* keep_bits, float* delta,
                    int B, int L, int nh, float p_drop, uint64_t seed, uint32_t offset, uint32_t site, void* ws, size_t ws_bytes,
                    void* stream, bool det);
int attn_x3_bwd_run(const float* qkv, const float* attn_mask, const int32_t* cu_seqlens, const float* ctx, const float* lse,
                    const float* dctx, int dctx_slabs, size_t dctx_slab_stride, float* dqkv, void* dqkv_x3, float* bias_part,
                    const void* keep_bits, float* delta, int B, int L, int nh, float p_drop, void* stream, bool det);
int attn_b16x_bwd_run(const void* qkv, int qkv_is_bf16, const float* attn_mask, const int32_t* cu_seqlens, const float* ctx,
                      const float* lse, const float* dctx, float* dqkv, void* dqkv_bf16, float* bias_part, const void* keep_bits,
                      float* delta, int B, int L, int nh, float p_drop, void* stream, bool det);
int attn_bf16_bwd_run(const void* qkv, int qkv_is_bf16, const float* attn_mask, const int32_t* cu_seqlens, const float* ctx,
                      const float* lse, const float* dctx, float* dqkv, void* dqkv_bf16, float* bias_part, const void* keep_bits,
                      float* delta, int B, int L, int nh, float p_drop, uint64_t seed, uint32_t offset, uint32_t site, void* ws,
                      size_t ws_bytes, void* stream, bool det);
// api.cpp: the hand-over of uniter_attn_bwd_set_next_det, taken (and reset) by the PUBLIC attention-backward wrappers as their first statement
bool attn_bwd_take_next_det();

// ---- persistent launches ----
int gemm_chip_cus();      // gemm_split3.hip: CUs of the current device, a multiple of 8

// Band height of the tile walk (round 5): an XCD's workgroups run ~32 tiles of its chunk of the walk at a time -- a band_h x (32 / band_h)
// rectangle of the tile grid -- and its L2 fetches band_h row panels and 32 / band_h column panels for them: least for
// band_h = sqrt(32 BN / BM).  (Round 4 sized the band for L2 capacity, 1.5 MB of row panels: 2 rows at K = 768, every XCD then
// fetched EVERY weight panel -- 7.1 x the operand bytes on FFN-up forward.  The panels' k-tiles are consumed k-synchronously, so
// capacity is not the constraint.  Time is unchanged either way -- the re-fetches are Infinity-Cache hits -- but the fabric moves
// a third less: profiles/r05_pmc_traffic.json.)
static inline int tile_band_height(int BM, int BN) {
  long bh = 1;
  while ((bh + 1) * (bh + 1) * (long)BM <= 32l * BN) ++bh;
  return (int)(bh > 16 ? 16 : bh);
}

// workgroups of a persistent launch over `nwork` items: a multiple of 8 (one chunk of the work per XCD), one per CU at most (it
// owns the CU's LDS), max_wgs >= 8: the caller's cap; cu_reserve: CUs the launch leaves free (LaunchOpts::cu_reserve)
static inline int persistent_grid(int nwork, int max_wgs, int cu_reserve) {
  int grid = (nwork + 7) / 8 * 8;
  const int cus = gemm_chip_cus();
  int cap = max_wgs >= 8 ? max_wgs / 8 * 8 : cus;
  if (cu_reserve > 0) {                                   // CUs left to the data-parallel exchange's kernels
    const int room = (cus - cu_reserve) / 8 * 8;
    if (room >= 8 && cap > room) cap = room;
  }
  return grid > cap ? cap : grid;
}
