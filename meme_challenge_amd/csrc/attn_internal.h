// Host-side declarations of the attention launchers (attention_f32.hip, attention_x3.hip, attention_bf16.hip), included through
// gemm_internal.h by the defining files and by every user: the one description of an attention launch they all take (AttnCall), the
// rules the three files share, and the dispatch of the model's schedule over the kernel families.
#pragma once
#include "common.h"

// One attention launch, forward or backward: what a caller states, by name.  An unset field means "absent".  The C ABI's wrappers
// and model.cpp fill one per launch.  A launcher refuses (UNITER_E_ARG) a set field its kernels cannot honour -- slabs or bf16
// Q|K|V on the fp32 kernels, copies / keep flags / bias partials / cu_seqlens beyond the L <= 192 kernels, a seed, a workspace or
// flags to draw on attention_x3.hip -- rather than ignore it.
struct AttnCall {
  int B = 0, L = 0, nh = 0;          // L: the joint length (packed batches: the longest sample's)
  const void* qkv = nullptr;         // [rows, 3H] fp32, or bf16 where qkv_is_bf16 (attention_bf16.hip, the b16x kernels)
  int qkv_is_bf16 = 0;
  const float* mask = nullptr;       // [B, L] additive mask XOR ...
  const int32_t* cu_seqlens = nullptr;      // ... [B + 1] row prefix sums of a packed batch
  float *ctx = nullptr, *lse = nullptr;     // forward outputs, backward inputs
  void* ctx_copy = nullptr;          // the context in the operand format: pieces = 1: bf16 [rows][H]; 3: x3 pieces [rows][3][H]
  int pieces = 1;                    // of ctx_copy and dqkv_copy
  float p_drop = 0.f;
  uint64_t seed = 0;                 // Philox stream of the kernels that draw the dropout themselves
  uint32_t offset = 0, site = 0;
  void* keep_bits = nullptr;         // dropout keep flags [B * nh, L, Lr / 32, 2].  Forward: read where keep_ready
  int keep_ready = 0;                // (uniter_attn_keep_bits_gen drew them), else drawn and written; backward: read
  const float* dctx = nullptr;       // [dctx_slabs][rows, H], slab s at dctx + s * dctx_slab_stride: summed while they are read
  int dctx_slabs = 1;
  size_t dctx_slab_stride = 0;
  float* dqkv = nullptr;             // fp32 [rows, 3H] and / or ...
  void* dqkv_copy = nullptr;         // ... its operand copy (pieces)
  float* bias_part = nullptr;        // [B, 3H] per-sample column sums of dqkv
  float* delta = nullptr;            // [B, nh, L]
  void* ws = nullptr;                // Pd / dS scratch of the two-kernel backward forms (attn_bwd_ws_bytes)
  size_t ws_bytes = 0;
  bool det = false;                  // bias_part summed in a fixed order (Plan::det; the C ABI: uniter_attn_bwd_set_next_det)
  void* stream = nullptr;
};

// who: the prefix of the refusal messages (the C entry point's, which the callers of the C ABI know).
// attention_f32.hip: any length behind a mask; L <= uniter_attn_varlen_max_len(): cu_seqlens, copies, keep flags, bias partials too
int attn_f32_fwd_run(const char* who, const AttnCall& c);
int attn_f32_bwd_run(const char* who, const AttnCall& c);
// attention_x3.hip: pieces = 3 (fp32 Q|K|V) or 1 (the b16x kernels, Q|K|V fp32 or bf16); dropout by reading keep flags only
int attn_x3_fwd_run(const char* who, const AttnCall& c);
int attn_x3_bwd_run(const char* who, const AttnCall& c);
// attention_bf16.hip: pieces = 1
int attn_bf16_fwd_run(const char* who, const AttnCall& c);
int attn_bf16_bwd_run(const char* who, const AttnCall& c);
// api.cpp: the hand-over of uniter_attn_bwd_set_next_det, taken (and reset) by the PUBLIC attention-backward wrappers as their first
// statement and handed on as AttnCall::det
bool attn_bwd_take_next_det();

// ---- the rules every file shares ----
// key / query rows of the L <= 192 kernels: whole 32-row blocks
static inline int attn_block_rows(int L) { return (L + 31) / 32 * 32; }
static inline bool attn_one_row_source(const AttnCall& c) { return (c.mask != nullptr) != (c.cu_seqlens != nullptr); }
static inline int attn_check_dims(const char* who, const AttnCall& c) {
  UCHECK_ARG(c.B > 0 && c.L > 0 && c.nh > 0, "%s: bad dims B=%d L=%d nh=%d", who, c.B, c.L, c.nh);
  UCHECK_ARG(c.p_drop >= 0.f && c.p_drop < 1.f, "%s: bad dropout p", who);
  return 0;
}
// the backward scratch: Pd and dS, [B * nh][Lr][Lr] each, fp32 (attention_f32.hip) or bf16 (attention_bf16.hip); 0: no launch takes it
static inline size_t attn_bwd_ws_elems(int B, int L, int nh) {
  const size_t Lr = (size_t)attn_block_rows(L);
  return B > 0 && nh > 0 ? (size_t)2 * B * nh * Lr * Lr : 0;
}
static inline size_t attn_f32_bwd_ws_bytes(int B, int L, int nh) { return attn_bwd_ws_elems(B, L, nh) * sizeof(float); }
static inline size_t attn_bf16_bwd_ws_bytes(int B, int L, int nh) { return attn_bwd_ws_elems(B, L, nh) * sizeof(unsigned short); }
// one launch with `lds` bytes of dynamic LDS: the attribute is set on every launch (another device's copy of the kernel has its own)
template <class K, class... A>
int launch_lds(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
  UCHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  UCHECK_LAUNCH();
  return 0;
}

// ---- the schedule's view (model.cpp) ----
// the attention kernel of a plan, by its forward entry point; the backward entry point follows from it
enum AttnKernel {
  ATTN_F32,          // uniter_attn_fwd / uniter_attn_bwd: any length, reads the padded mask
  ATTN_F32_PRE,      // uniter_attn_fwd_pre / uniter_attn_bwd_ex: the L <= 192 kernels (packed batches, saved plans)
  ATTN_F32_PRE_X3,   // uniter_attn_fwd_pre_x3 / uniter_attn_bwd_ex_x3: the same with x3 pieces out (precision 3)
  ATTN_X3,           // uniter_attn_x3_fwd / _bwd: precision 3, the attention's own products on the bf16 pipe
  ATTN_BF16_PRE,     // uniter_attn_bf16_fwd_pre / uniter_attn_bf16_bwd: precision 2 (attention_bf16.hip)
  ATTN_B16X          // uniter_attn_b16x_fwd / _bwd: precision 2 in attention_x3.hip's decomposition
};
static inline bool attn_is_b16(AttnKernel k) { return k == ATTN_BF16_PRE || k == ATTN_B16X; }
// attention_x3.hip's kernels read the dropout keep flags and draw none
static inline bool attn_reads_flags_only(AttnKernel k) { return k == ATTN_X3 || k == ATTN_B16X; }
static inline int attn_forward(AttnKernel k, const char* who, const AttnCall& c) {
  switch (k) {
  case ATTN_X3: case ATTN_B16X: return attn_x3_fwd_run(who, c);
  case ATTN_BF16_PRE: return attn_bf16_fwd_run(who, c);
  case ATTN_F32: case ATTN_F32_PRE: case ATTN_F32_PRE_X3: break;
  }
  return attn_f32_fwd_run(who, c);
}
static inline int attn_backward(AttnKernel k, const char* who, const AttnCall& c) {
  switch (k) {
  case ATTN_X3: case ATTN_B16X: return attn_x3_bwd_run(who, c);
  case ATTN_BF16_PRE: return attn_bf16_bwd_run(who, c);
  case ATTN_F32: case ATTN_F32_PRE: case ATTN_F32_PRE_X3: break;
  }
  return attn_f32_bwd_run(who, c);
}
