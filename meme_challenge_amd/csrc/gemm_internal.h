// Host-side declarations shared by the GEMM files and the schedule (model.cpp), stated once: the internal entry points behind the
// C ABI, and the two rules every persistent launch shares (band height of the tile walk, grid cap).  The defining file and every
// user include this header, so a changed signature fails where it is defined, at compile time.
#pragma once
#include "common.h"

// ---- dense products: gemm_f32.hip, gemm_bf16.hip, gemm_bf16_dma.hip, gemm_bf16_p.hip, gemm_split3.hip ----
// no_sk (the three *_run below): never the stream-K form, whose partial tiles meet in float atomics in arrival order -- a C += then
// runs on whole tiles, one adder per element (the plans of uniter_model_set_deterministic).  gemm_bf16v2_run has no such form: its
// C += is one workgroup per tile (split-K with beta is refused).
int gemm_f32_run(int cfg, int tag, int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda,
                 const float* B, int ldb, float* C, int ldc, int epilogue, const float* bias,
                 const float* aux_in, float* aux_out, int ld_aux, int beta, float* colsum_part, void* stream,
                 int no_sk = 0);
int gemm_bf16_run(int cfg, int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda,
                  const float* B, int ldb, float* C, int ldc, int epilogue, const float* bias,
                  const float* aux_in, float* aux_out, int ld_aux, int beta, float* colsum_part, void* stream,
                  int no_sk = 0);
int gemm_bf16res_run(int cfg, int a_kmajor, int b_kmajor, int M, int N, int K, const void* A, int lda, const void* B,
                     int ldb, float* C, int ldc, void* Cb, int ldcb, int epilogue, const float* bias,
                     const float* aux_in, float* aux_out, int ld_aux, int beta, float* colsum_part, void* stream,
                     int no_sk = 0);
int gemm_bf16v2_run(int cfg, int nsplit, int a_kmajor, int b_kmajor, int M, int N, int K, const void* A, int lda,
                    const void* B, int ldb, float* C, int ldc, long c_split_stride, void* Cb, int ldcb, int epilogue,
                    const float* bias, const void* aux_in, int aux_in_bf16, void* aux_out, int aux_out_bf16,
                    int ld_aux, int beta, void* stream);
int gemm_f32_wgrad_group(int n, const int* Mo, const int* No, int K, const float* const* A, const float* const* B,
                         float* const* dW, int overwrite, void* stream);
int gemm_x3_run(int cfg, int nsplit, int a_kmajor, int b_kmajor, int M, int N, int K, const void* A, int lda, int psa,
                const void* B, int ldb, int psb, float* C, int ldc, long c_split_stride, void* Cx, int ldcx, int pscx,
                int epilogue, const float* bias, const float* aux_in, float* aux_out, int ld_aux, void* stream,
                float* colsum_part, void* sk_ws, size_t sk_ws_bytes);
size_t gemm_x3_sk_ws_bytes();
int gemm_x3_wgrad_default_cfg();
int gemm_x3_pick_split(int M, int N, int K);
int gemm_x3_pick_split_on(int M, int N, int K, int avail);
int gemm_x3_wgrad_group(int cfg, int n, const int* Mo, const int* No, int K, const void* const* A, const void* const* B,
                        float* const* dW, void* stream, int overwrite, int max_wgs, uniter_x3_riders_t* riders,
                        void* sk_ws, size_t sk_ws_bytes);
int gemm_x3_wgrad_group_slots(int cfg, int n, const int* Mo, const int* No, int max_wgs, int K, size_t sk_ws_bytes);
int gemm_x3_wgrad_group_balanced_wgs(int cfg, int n, const int* Mo, const int* No);
int gemm_bf16v2_pick_split(int M, int N, int K);
int gemm_b1p_pick_split(int M, int N, int K, int avail);
int gemm_b1p_run(int cfg, int nsplit, int b_kmajor, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                 float* C, int ldc, long c_split_stride, void* Cb, int ldcb, int epilogue, const float* bias,
                 const void* aux_in, int aux_in_bf16, void* aux_out, int aux_out_bf16, int ld_aux, float* colpart, void* stream);
int gemm_b1p_wgrad_group(int n, const int* Mo, const int* No, int K, const void* const* A, const void* const* B, float* const* dW,
                         void* stream, int overwrite, int max_wgs, uniter_x3_riders_t* riders);
int gemm_b1p_wgrad_group_slots(int n, const int* Mo, const int* No, int max_wgs);
int gemm_bf16v2_wgrad_pieces(int M, int N, int K);
int gemm_bf16v2_wgrad_group(int cfg, int n, const int* Mo, const int* No, int K, const void* const* A,
                            const void* const* B, float* const* dW, void* stream, int overwrite, int max_wgs,
                            uniter_x3_riders_t* riders);
int gemm_bf16v2_wgrad_group_slots(int n, const int* Mo, const int* No, int max_wgs);
int gemm_bf16v2_wgrad_group_balanced_wgs(int n, const int* Mo, const int* No);

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
int launch_masked_rowsum(const float* x, const int64_t* masks, float* out, int rows, int D, hipStream_t st);

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
// owns the CU's LDS), max_wgs >= 8: the caller's cap
static inline int persistent_grid(int nwork, int max_wgs) {
  int grid = (nwork + 7) / 8 * 8;
  const int cus = gemm_chip_cus();
  int cap = max_wgs >= 8 ? max_wgs / 8 * 8 : cus;
  if (g_uniter_cu_reserve > 0) {                          // CUs left to the data-parallel exchange's kernels
    const int room = (cus - g_uniter_cu_reserve) / 8 * 8;
    if (room >= 8 && cap > room) cap = room;
  }
  return grid > cap ? cap : grid;
}
