// Host-side declarations shared by the kernel files and the schedule (model.cpp), stated once: the one description of a dense product
// every GEMM launcher takes (GemmCall, WgradGroupCall) with the argument rules the families share, the rules every persistent launch
// shares (band height of the tile walk, grid cap, rounds), and -- each in a header of its own, included here -- the row passes and
// embeddings (rowpass_internal.h) and the attention launchers (attn_internal.h).  The defining file and every user include this
// header, so a changed signature fails where it is defined, at compile time.
#pragma once
#include "common.h"

// ---- dense products: gemm_f32.hip, gemm_bf16.hip, gemm_bf16_dma.hip, gemm_bf16_p.hip, gemm_split3.hip ----
// One operand of a product: k-contiguous ([rows][K], kmajor = 0) or k-major ([K][rows]).  piece_stride: elements between the three
// pieces of an x3 operand; 0 in every other format.
struct GemmOperand {
  const void* p = nullptr;
  int ld = 0, piece_stride = 0, kmajor = 0;
};
// One product C (+)= epi(A . B): what a caller states, by name.  An unset field means "absent".  The C ABI's wrappers and
// model.cpp fill one per product; a launcher that forwards to another hands the same call on.  A launcher refuses (UNITER_E_ARG)
// a set field its kernels cannot honour -- piece strides or k-pieces on the fp32 kernels, an output copy on gemm_bf16_run, a
// workspace outside the x3 family -- rather than ignore it.
struct GemmCall {
  int M = 0, N = 0, K = 0;
  GemmOperand A, B;                  // fp32 (gemm_f32_run, gemm_bf16_run), bf16 (bf16res, bf16v2, b1p) or x3
  float* C = nullptr;                // fp32 output: nsplit k-piece slabs, slab s at C + s * c_split_stride
  int ldc = 0, nsplit = 1;
  long c_split_stride = 0;
  void* Ccopy = nullptr;             // the output in the operand format (bf16 or x3): row stride, piece stride (x3)
  int ld_copy = 0, ps_copy = 0;
  int epi = UNITER_EPI_NONE;
  const float* bias = nullptr;
  const void* aux_in = nullptr;      // [M][ld_aux] fp32, or bf16 where the flag says so (bf16v2, b1p)
  void* aux_out = nullptr;
  int aux_in_bf16 = 0, aux_out_bf16 = 0, ld_aux = 0;
  // beta = 1: C +=.  no_sk: never the stream-K form, whose partial tiles meet in float atomics in arrival order -- a C += then runs on
  // whole tiles, one adder per element (the plans of uniter_model_set_deterministic); the bf16v2, b1p and x3 kernels have no such form
  int beta = 0, no_sk = 0;
  float* colpart = nullptr;          // column partials of the stored output (f32: per 32 rows; b1p, x3: per 64 rows, x aux epilogue)
  void* sk_ws = nullptr;             // workspace of the balanced walk (x3)
  size_t sk_ws_bytes = 0;
  void* stream = nullptr;
};

// Which epilogue needs which operand, for every family.  built: bit e set = the family builds epilogue e (one it does not build
// is refused by its dispatch, with its own message, whatever operands came along).  gelu_needs_aux_out: the bias + GELU epilogues
// of the fp32 kernels and of gemm_bf16.hip skip the store of u / gelu'(u) when aux_out is NULL (a forward pass that saves nothing);
// the bf16v2, b1p and x3 entry points have always refused that call.
constexpr unsigned GEMM_EPI_ALL = (2u << UNITER_EPI_MUL) - 1;
constexpr unsigned GEMM_EPI_PERSISTENT = 1u << UNITER_EPI_NONE | 1u << UNITER_EPI_BIAS | 1u << UNITER_EPI_ADD |
                                         1u << UNITER_EPI_BIAS_GELU_D | 1u << UNITER_EPI_MUL;      // b1p and x3
static inline int gemm_check_epilogue(const char* who, const GemmCall& c, unsigned built, bool gelu_needs_aux_out) {
  const int e = c.epi;
  if (e < 0 || e > UNITER_EPI_MUL || !(built >> e & 1)) return 0;
  const bool gelu = e == UNITER_EPI_BIAS_GELU || e == UNITER_EPI_BIAS_GELU_D;
  UCHECK_ARG(!(e == UNITER_EPI_BIAS || gelu) || c.bias, "%s: epilogue needs bias", who);
  UCHECK_ARG(!(e == UNITER_EPI_DGELU || e == UNITER_EPI_ADD || e == UNITER_EPI_MUL) || c.aux_in, "%s: epilogue needs aux_in", who);
  UCHECK_ARG(!(gelu && gelu_needs_aux_out) || c.aux_out, "%s: epilogue needs aux_out", who);
  return 0;
}
// the checks the three LDS-DMA families (bf16v2, b1p, x3) state alike: every fp32-side buffer 16-byte aligned, fp32 leading
// dimensions % 4, the copy's % 8; and the fp32 output and aux operand within 31-bit offsets with the tile overhang of `pad` rows
static inline bool gemm_side_buffers_aligned(const GemmCall& c) {
  return c.ldc % 4 == 0 && c.ld_copy % 8 == 0 && c.ld_aux % 4 == 0 && ((uintptr_t)c.C & 15) == 0 && ((uintptr_t)c.Ccopy & 15) == 0 &&
         ((uintptr_t)c.aux_in & 15) == 0 && ((uintptr_t)c.aux_out & 15) == 0 && ((uintptr_t)c.bias & 15) == 0;
}
static inline bool gemm_f32_side_in_range(const GemmCall& c, int pad) {
  return ((size_t)c.M + pad) * (c.ldc > 0 ? c.ldc : 1) * 4 < (1ull << 31) && ((size_t)c.M + pad) * (c.ld_aux > 0 ? c.ld_aux : 1) * 4 < (1ull << 31);
}

// cfg: the family's tile geometry, 0 = choose (| 64: B in the paired-row layout, >> 8: lab bits where the family has them).
// lo (no default: a forgotten argument does not compile): the stamp slot, wave priority and CU reserve of THIS launch (common.h).
// A launcher that forwards to another hands lo on whole.  gemm_bf16_run / gemm_bf16res_run's own kernels and the grouped
// weight-gradient launches set no wave priority: they ignore lo.prio.
int gemm_f32_run(int cfg, int tag, const GemmCall& c, const LaunchOpts& lo);
int gemm_bf16_run(int cfg, const GemmCall& c, const LaunchOpts& lo);
int gemm_bf16res_run(int cfg, const GemmCall& c, const LaunchOpts& lo);
int gemm_bf16v2_run(int cfg, const GemmCall& c, const LaunchOpts& lo);
int gemm_b1p_run(int cfg, const GemmCall& c, const LaunchOpts& lo);
int gemm_x3_run(int cfg, const GemmCall& c, const LaunchOpts& lo);
size_t gemm_x3_sk_ws_bytes();
int gemm_x3_wgrad_default_cfg();
int gemm_x3_pick_split(int M, int N, int K);
int gemm_x3_pick_split_on(int M, int N, int K, int avail, int cu_reserve);
int gemm_bf16v2_pick_split(int M, int N, int K);
int gemm_b1p_pick_split(int M, int N, int K, int avail, int cu_reserve);
int gemm_bf16v2_wgrad_pieces(int M, int N, int K);

// Up to four weight gradients dW_p[Mo_p, No_p] (+)= A_p^T B_p of one reduction length K as ONE launch (A_p [K][Mo_p], B_p [K][No_p] in
// the family's operand format, dW_p fp32 with leading dimension No_p).  max_wgs: grid cap, 0 = the family's; riders: side work of
// the launch (include/uniter_hip.h), not on the fp32 kernel; sk_ws: the balanced walk's workspace (x3).  Kp (x3, without sk_ws): a
// reduction length per product -- rows Kp[p] of A_p and B_p, the tiles, grid and riders' slots of the launch unchanged.
struct WgradGroupCall {
  int n = 0, K = 0;
  const int* Kp = nullptr;           // optional: product p's own reduction length Kp[p] > 0 in place of K (x3 only)
  const int *Mo = nullptr, *No = nullptr;
  const void *const *A = nullptr, *const *B = nullptr;
  float* const* dW = nullptr;
  int overwrite = 0, max_wgs = 0;
  uniter_x3_riders_t* riders = nullptr;
  void *sk_ws = nullptr, *stream = nullptr;
  size_t sk_ws_bytes = 0;
};
int gemm_f32_wgrad_group(const WgradGroupCall& c, const LaunchOpts& lo);
int gemm_bf16v2_wgrad_group(int cfg, const WgradGroupCall& c, const LaunchOpts& lo);
int gemm_b1p_wgrad_group(const WgradGroupCall& c, const LaunchOpts& lo);
int gemm_x3_wgrad_group(int cfg, const WgradGroupCall& c, const LaunchOpts& lo);
int gemm_x3_wgrad_group_slots(int cfg, int n, const int* Mo, const int* No, int max_wgs, int K, size_t sk_ws_bytes, int cu_reserve);
int gemm_x3_wgrad_group_balanced_wgs(int cfg, int n, const int* Mo, const int* No, int cu_reserve);
int gemm_b1p_wgrad_group_slots(int n, const int* Mo, const int* No, int max_wgs, int cu_reserve);
int gemm_bf16v2_wgrad_group_slots(int n, const int* Mo, const int* No, int max_wgs, int cu_reserve);
int gemm_bf16v2_wgrad_group_balanced_wgs(int n, const int* Mo, const int* No, int cu_reserve);

static inline int wgrad_group_check(const char* who, const WgradGroupCall& c) {
  UCHECK_ARG(c.n >= 1 && c.n <= 4 && c.K > 0 && c.Mo && c.No && c.A && c.B && c.dW, "%s: bad argument", who);
  for (int p = 0; c.Kp && p < c.n; ++p) UCHECK_ARG(c.Kp[p] > 0, "%s: product %d: reduction length %d", who, p, c.Kp[p]);
  return 0;
}
// The walk over the products of a grouped launch, written once: product p < n is checked (UNITER_E_ARG: a null or empty product;
// UNITER_E_SHAPE: in_range(p) says the family's kernel does not take it) and handed to fill(p), which writes the family's
// per-product kernel argument and returns its tile count; the padding slots p >= n go to pad(p).  start[p] = first work item of
// product p, start[n .. 4] = the total.
template <class InRange, class Fill, class Pad>
int wgrad_group_walk(const char* who, const WgradGroupCall& c, int* start, InRange in_range, Fill fill, Pad pad) {
  UCHECK_RC(wgrad_group_check(who, c));
  int total = 0;
  for (int p = 0; p < 4; ++p) {
    start[p] = total;
    if (p >= c.n) { pad(p); continue; }
    UCHECK_ARG(c.Mo[p] > 0 && c.No[p] > 0 && c.A[p] && c.B[p] && c.dW[p], "%s: bad product %d", who, p);
    UCHECK_SHAPE(in_range(p), "%s: product %d (%d x %d, K = %d) outside the grouped kernel's range (M, N multiples of 8 -- fp32: 4 --, "
                 "16-byte aligned buffers, 31-bit offsets)", who, p, c.Mo[p], c.No[p], c.Kp ? c.Kp[p] : c.K);
    total += fill(p);
  }
  for (int p = c.n; p <= 4; ++p) start[p] = total;
  return 0;
}
// what the three bf16-pipe families ask of product p alike; each adds the 31-bit range of its own operand format
static inline bool wgrad_product_aligned8(const WgradGroupCall& c, int p) {
  return c.Mo[p] % 8 == 0 && c.No[p] % 8 == 0 && ((uintptr_t)c.A[p] & 15) == 0 && ((uintptr_t)c.B[p] & 15) == 0 &&
         ((uintptr_t)c.dW[p] & 15) == 0 && ((size_t)c.Mo[p] + 256) * c.No[p] * 4 < (1ull << 31);
}
// ... the two bf16 launches (gemm_bf16_dma.hip, gemm_bf16_p.hip): a k-tile of overhang on the longer operand
static inline bool wgrad_bf16_product_in_range(const WgradGroupCall& c, int p) {
  return wgrad_product_aligned8(c, p) && (size_t)(c.K + 64) * (c.Mo[p] > c.No[p] ? c.Mo[p] : c.No[p]) * 2 < (1ull << 31);
}
// tiles of 128 x BN of the products of a grouped launch (0: arguments no launch would take)
static inline int wgrad_group_tiles(int n, const int* Mo, const int* No, int BN) {
  if (!Mo || !No || n < 1 || n > 4) return 0;
  int total = 0;
  for (int p = 0; p < n; ++p) total += ((Mo[p] + 127) / 128) * ((No[p] + BN - 1) / BN);
  return total;
}
// the smallest grid (a multiple of 8) on which `total` work items take no more rounds than on `full` workgroups
static inline int balanced_grid(int total, int full) {
  if (total <= 0 || full <= 0) return 0;
  const int rounds = (total + full - 1) / full;
  const int wgs = ((total + rounds - 1) / rounds + 7) / 8 * 8;
  return wgs < full ? wgs : full;
}
// sum-of-squares slots a launch with riders writes: one per compute wave of each of its `grid` workgroups
static inline int rider_slots(int waves, int grid) { return waves * grid; }

// ---- row passes and embeddings: layernorm.hip, embed.hip, input_grads.hip ----
#include "rowpass_internal.h"

// ---- attention: attention_f32.hip, attention_x3.hip, attention_bf16.hip ----
#include "attn_internal.h"

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
// the band of the kernels that kept round 4's rule (fp32, gemm_bf16.hip, gemm_bf16_dma.hip): row panels of `panel` bytes in 1.5 MB
static inline int l2_band_height(long panel, int tiles_m) {
  const long bh = (3l << 19) / (panel > 0 ? panel : 1);
  const int b = (int)(bh < 1 ? 1 : (bh > 16 ? 16 : bh));
  return b > tiles_m ? tiles_m : b;
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
