// Fused optimizer step over flat fp32 buffers.
//
// Replaces, in one HBM pass, TrainerTemplate.average_gradients
// (train_template.py:89-92), torch.nn.utils.clip_grad_norm_ (:104), the
// per-tensor torch.optim.Adam / AdamW step configured by get_optimizer
// (utils/optim_utils.py:9-46) and optimizer.zero_grad (:107): 212 tensors x ~5
// elementwise launches in the reference.  Algorithmic traffic: read p,g,m,v +
// write p,m,v (+ zeroed g) = 32 B per parameter.
//
// The global gradient norm is reduced on the device into a double and consumed
// by the step kernel from device memory: no host synchronisation.
// Per-64-element chunk flags carry the parameter-group split:
//   0 = parameter received no gradient this step (torch skips grad=None params),
//   1 = no weight decay ('bias' / 'LayerNorm.*' names), 2 = weight decay;
//   + 4 = leave the gradient as it is (zero_grads notwithstanding): the next backward pass OVERWRITES this chunk
//         (the encoder's weight gradients, uniter_model_set_wgrad_overwrite) -- 28 instead of 32 bytes per parameter.
// The kernels test the whole byte for "skip", so 4 alone is invalid (it would update and count the chunk): callers pass
// 0, 1, 2, 5 or 6 (include/uniter_hip.h).
// uniter_optim_step_groups alone reads bits 3-7: the chunk's parameter group, 0 .. 31, whose row of a table of hyper-parameters
// (lr, betas, eps, weight decay: utils/optim_utils.py:9-30 copies a group's own keys into its decay and no-decay halves) the chunk is
// updated with; its valid bytes are 0 and (group << 3) | {1, 2, 5, 6}, and a group the table does not hold is a skip.  A frozen
// tensor's chunks are 0 whatever gradient it received.  The clip coefficient stays one value per launch.
#include "common.h"
#include "bf16_tile.h"

namespace {

constexpr int CHUNK = 64;

__device__ __forceinline__ f32x4 widen4(const unsigned short* __restrict__ g16, size_t i) {
  const u32x2_t w = reinterpret_cast<const u32x2_t*>(g16)[i];
  return f32x4{__builtin_bit_cast(float, w[0] << 16), __builtin_bit_cast(float, w[0] & 0xffff0000u),
               __builtin_bit_cast(float, w[1] << 16), __builtin_bit_cast(float, w[1] & 0xffff0000u)};
}

// g16 (optional): the gradients as bf16 (the data-parallel exchange's reduced payload) instead of the fp32 buffer
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g,
                                                    const uint8_t* __restrict__ flags, size_t n4,
                                                    double* __restrict__ part,
                                                    const unsigned short* __restrict__ g16) {
  __shared__ double red[4];
  double acc = 0.0;
  // two 16-byte pieces per thread and iteration, both loads issued first (the pass is a pure HBM stream: 440 MB)
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += 2 * stride) {
    const size_t j = i + stride;
    const bool f0 = !flags || flags[(i * 4) / CHUNK] != 0, f1 = j < n4 && (!flags || flags[(j * 4) / CHUNK] != 0);
    f32x4 v = {0.f, 0.f, 0.f, 0.f}, w = v;
    if (f0) v = g16 ? widen4(g16, i) : reinterpret_cast<const f32x4*>(g)[i];
    if (f1) w = g16 ? widen4(g16, j) : reinterpret_cast<const f32x4*>(g)[j];
    acc += (double)(v[0] * v[0] + v[1] * v[1]) + (double)(v[2] * v[2] + v[3] * v[3]);
    acc += (double)(w[0] * w[0] + w[1] * w[1]) + (double)(w[2] * w[2] + w[3] * w[3]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// (round 5: the fp32x3 backward leaves ~1000 partial sums per layer -- 1024 threads, four independent loads in flight each; the
// order of the additions depends on n alone: bit-reproducible)
__global__ __launch_bounds__(1024) void sumsq_final_kernel(const double* __restrict__ part, int n,
                                                           double* __restrict__ out) {
  __shared__ double red[16];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int i = threadIdx.x;
  for (; i + 3 * 1024 < n; i += 4 * 1024) { a0 += part[i]; a1 += part[i + 1024]; a2 += part[i + 2048]; a3 += part[i + 3072]; }
  for (; i < n; i += 1024) a0 += part[i];
  double acc = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];
    out[0] = t;
  }
}

struct AdamArgs {
  float* p; float* g; float* m; float* v;
  const uint8_t* flags;
  size_t n4;
  const double* sumsq;
  float gscale, max_norm, lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2;
  int adamw, zero_grads;
  unsigned short* mirror;     // optional bf16 copy of the updated parameters (precision 'bf16' weight mirror)
  size_t mirror_ps;           // > 0: the mirror holds the THREE bf16 pieces of every parameter, piece p at mirror + p * mirror_ps (precision 'fp32x3')
  const unsigned short* g16;  // optional: read the gradient from this bf16 buffer (reduced data-parallel payload); g is still zeroed
  // row split of a table (round 6, uniter_adam_step_rows): chunk c belongs to row c / row_chunks; only the rows whose mask byte is
  // (!= 0) == (rows_want != 0) are updated.  rows_want == 0 also means "these rows received no gradient": g is taken as zero
  // without being read (and is not cleared)
  const uint8_t* rowmask;
  int row_chunks, rows_want;
  // paired-row weight mirror (round 6, uniter_adam_step_x3p): the launch walks the buffer in the MIRROR's order.  vsrc[c] = {s0, s1}
  // (elements from the flat buffers' start; s0 < 0 / no table: chunk c is its own source): the two 32-element units of chunk c of the
  // mirror are the parameters s0 .. s0 + 31 and s1 .. s1 + 31 -- one unit of row 2 q and the same unit of row 2 q + 1.  p, g, m, v are
  // then read and written in whole 128-byte lines (a unit is 32 floats) and the mirror in whole lines too (two neighbouring 64-byte
  // units); walking in the parameters' order instead left half-written mirror lines behind every wave (adam_kernel 76 -> 95 us).
  // The table pointer is that of this launch's first chunk; vsrc_base = the launch's first element (its offsets are absolute)
  const int2* vsrc;
  long vsrc_base;
};

#define NT_LOAD(base, idx) __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base) + (idx))
// The update rule is a compile-time parameter of the step kernel: the walk, the chunk flags, the gradient widening, the non-temporal
// accesses and the mirror writes are one skeleton (adam_kernel<RULE>), the arithmetic per element is the rule's (include/uniter_hip.h,
// uniter_optim_step).  RULE_ADAM is torch.optim.Adam / AdamW as before (the adamw flag stays a launch argument).
enum { RULE_ADAM = 0, RULE_ADAMAX = 1, RULE_SGD = 2 };
// Parameter groups (uniter_optim_step_groups): bits 3-7 of a chunk's flag byte name its group, and the hyper-parameters an element
// is updated with are its group's row of a table instead of the launch's scalars.  The rows reach the kernel by value (a kernel
// argument of MAX_GROUPS rows) and are staged into LDS once per workgroup, by ONE thread through compile-time indices -- a per-lane
// index into a by-value argument would make the compiler copy the table into private memory; per item a lane then reads its group's
// 32 bytes from LDS (the lanes of a group read one address: a broadcast).  GROUPED is a compile-time variant of the walk: the
// instantiations behind every other entry point are the code they were.
constexpr int MAX_GROUPS = 32;
struct GroupRow { float lr, b1, b2, eps, wd, step_size, inv_sqrt_bc2, pad; };
struct GroupTable { int n; GroupRow row[MAX_GROUPS]; };

// H: where lr, b1, b2, eps, step_size and inv_sqrt_bc2 come from -- the launch's arguments or the chunk's GroupRow
template <int RULE, class H>
__device__ __forceinline__ void adam_update4(const H& a, int adamw, float coef, float wd, f32x4& p, const f32x4& g, f32x4& m, f32x4& v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float gg = g[e] * coef;
    float pp = p[e];
    if constexpr (RULE == RULE_ADAM) {
      if (adamw) pp *= 1.0f - a.lr * wd;
      else gg += wd * pp;
      m[e] = a.b1 * m[e] + (1.0f - a.b1) * gg;
      v[e] = a.b2 * v[e] + (1.0f - a.b2) * gg * gg;
      const float denom = sqrtf(v[e]) * a.inv_sqrt_bc2 + a.eps;
      p[e] = pp - a.step_size * (m[e] / denom);
    } else if constexpr (RULE == RULE_ADAMAX) {
      // torch.optim.Adamax: v is the infinity norm u; eps inside the max, bias correction of the first moment only
      gg += wd * pp;
      m[e] = a.b1 * m[e] + (1.0f - a.b1) * gg;
      v[e] = fmaxf(a.b2 * v[e], fabsf(gg) + a.eps);
      p[e] = pp - a.step_size * (m[e] / v[e]);
    } else {
      // torch.optim.SGD, dampening 0, no Nesterov: m is the momentum buffer (b1 = the momentum); no second state
      gg += wd * pp;
      m[e] = a.b1 * m[e] + gg;
      p[e] = pp - a.lr * m[e];
    }
  }
}
template <int RULE>
__device__ __forceinline__ void adam_store4(const AdamArgs& a, size_t i, size_t si, const f32x4& p, const f32x4& m, const f32x4& v, bool clear) {
  // the update streams 34 bytes per parameter once: non-temporal accesses, so that it does not evict the operand panels of
  // the forward kernels that share the chip with it from the L2s.  si: the item's place in the parameter buffers, i: in the mirror
  __builtin_nontemporal_store(p, reinterpret_cast<f32x4*>(a.p) + si);
  if (a.mirror) {
    const bf16x4 o = {(__bf16)p[0], (__bf16)p[1], (__bf16)p[2], (__bf16)p[3]};
    bf16x4* m0 = reinterpret_cast<bf16x4*>(a.mirror) + i;      // (i: the item's place in the mirror's order)
    *m0 = o;
    if (a.mirror_ps) {      // x = x1 + x2 + x3 exactly (round-to-nearest residuals): the operands of csrc/gemm_split3.hip
      f32x4 r = {p[0] - (float)o[0], p[1] - (float)o[1], p[2] - (float)o[2], p[3] - (float)o[3]};
      const bf16x4 o2 = {(__bf16)r[0], (__bf16)r[1], (__bf16)r[2], (__bf16)r[3]};
      *reinterpret_cast<bf16x4*>(reinterpret_cast<unsigned short*>(m0) + a.mirror_ps) = o2;
      r = f32x4{r[0] - (float)o2[0], r[1] - (float)o2[1], r[2] - (float)o2[2], r[3] - (float)o2[3]};
      *reinterpret_cast<bf16x4*>(reinterpret_cast<unsigned short*>(m0) + 2 * a.mirror_ps) = bf16x4{(__bf16)r[0], (__bf16)r[1], (__bf16)r[2], (__bf16)r[3]};
    }
  }
  __builtin_nontemporal_store(m, reinterpret_cast<f32x4*>(a.m) + si);
  if constexpr (RULE != RULE_SGD) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(a.v) + si);
  // zero_grad: only where something was written -- four of five rows of the embeddings' block (the word table away from
  // the batch's tokens) hold zeros already
  if (clear) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(a.g) + si);
}
__device__ __forceinline__ bool any_nonzero(const f32x4& g) { return g[0] != 0.f || g[1] != 0.f || g[2] != 0.f || g[3] != 0.f; }

// Two 16-byte elements per thread and iteration, all eight loads issued before the arithmetic: a grid of one or two
// workgroups per CU (the launch that shares the chip with the next forward, see trainer.FusedAdam) still keeps
// 32-64 KB per CU in flight.  (RULE_SGD: six loads, a.v is never touched and may be NULL.)
// AVG (uniter_optim_step_avg / uniter_optim_step_groups_avg): an exponential moving average of the parameters as one more stream of
// the same walk.  Every item on the update path reads its 16 bytes of `avg` with the other loads and writes
//   a' = a + w (p' - a)         (three fp32 operations in this order; p' = the parameter the item has just computed, still in registers)
// behind the parameter's own stores: 8 bytes per parameter, where a separate pass reads p once more (12).  avg is indexed like p (si, the
// item's place in the parameter buffers, whatever order the mirror is walked in); a skipped item neither reads nor writes it.  The two
// arguments live in a part of WalkArgs that only the AVG instantiations have: AdamArgs, and with it the kernel arguments and the code
// of every other instantiation, stay what they were.
struct AvgArgs { float* avg; float w; };
template <bool GROUPED, bool AVG> struct WalkArgs { AdamArgs a; };
template <> struct WalkArgs<true, false> { AdamArgs a; GroupTable t; };
template <> struct WalkArgs<false, true> { AdamArgs a; AvgArgs e; };
template <> struct WalkArgs<true, true> { AdamArgs a; GroupTable t; AvgArgs e; };

__device__ __forceinline__ void avg_store4(const AvgArgs& e, size_t si, const f32x4& p, f32x4 x) {
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = x[k] + e.w * (p[k] - x[k]);
  __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(e.avg) + si);
}

template <int RULE, bool GROUPED, bool AVG>
__global__ __launch_bounds__(256) void adam_kernel(const WalkArgs<GROUPED, AVG> w) {
  const AdamArgs& a = w.a;
  __shared__ GroupRow rows[GROUPED ? MAX_GROUPS : 1];
  int n_groups = 0;
  if constexpr (GROUPED) {
    n_groups = w.t.n;
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < MAX_GROUPS; ++k)
        if (k < w.t.n) rows[k] = w.t.row[k];
    }
    __syncthreads();
  }
  float coef = a.gscale;
  if (a.max_norm > 0.f && a.sumsq) {
    const float total = (float)sqrt(a.sumsq[0]) * a.gscale;         // norm of the averaged grads
    const float c = a.max_norm / (total + 1e-6f);                   // clip_grad_norm_
    coef *= c < 1.0f ? c : 1.0f;
  }
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += 2 * stride) {
    const size_t j = i + stride;
    const bool two = j < a.n4;
    // where the item sits in the parameter buffers: its own place, or -- a chunk of a paired tensor, walked in the mirror's order --
    // one of the two source units the table names
    size_t si = i, sj = j;
    if (a.vsrc) {
      const int2 vi = a.vsrc[(i * 4) / CHUNK];
      if (vi.x >= 0) si = (size_t)((long)((((i * 4) >> 5) & 1) ? vi.y : vi.x) - a.vsrc_base + (long)((i * 4) & 31)) / 4;
      if (two) {
        const int2 vj = a.vsrc[(j * 4) / CHUNK];
        if (vj.x >= 0) sj = (size_t)((long)((((j * 4) >> 5) & 1) ? vj.y : vj.x) - a.vsrc_base + (long)((j * 4) & 31)) / 4;
      }
    }
    uint8_t f0 = a.flags[(si * 4) / CHUNK];
    uint8_t f1 = two ? a.flags[(sj * 4) / CHUNK] : 0;
    if constexpr (GROUPED) {      // a chunk off the update path, or of a group the table does not hold: a 0 byte
      if ((f0 & 3) == 0 || (f0 >> 3) >= n_groups) f0 = 0;
      if ((f1 & 3) == 0 || (f1 >> 3) >= n_groups) f1 = 0;
    } else if (a.rowmask) {      // (one table, split by rows: this launch takes the rows on its side of the mask)
      if (f0 && (a.rowmask[((si * 4) / CHUNK) / a.row_chunks] != 0) != (a.rows_want != 0)) f0 = 0;
      if (f1 && (a.rowmask[((sj * 4) / CHUNK) / a.row_chunks] != 0) != (a.rows_want != 0)) f1 = 0;
    }
    const bool no_g = !GROUPED && a.rowmask && a.rows_want == 0;      // rows without a gradient this step: g == 0, unread
    f32x4 p0, g0 = {0.f, 0.f, 0.f, 0.f}, m0, v0, p1, g1 = g0, m1, v1, e0, e1;
    if (f0) {
      p0 = NT_LOAD(a.p, si); if (!no_g) g0 = a.g16 ? widen4(a.g16, si) : NT_LOAD(a.g, si); m0 = NT_LOAD(a.m, si);
      if constexpr (RULE != RULE_SGD) v0 = NT_LOAD(a.v, si);
      if constexpr (AVG) e0 = NT_LOAD(w.e.avg, si);
    }
    if (f1) {
      p1 = NT_LOAD(a.p, sj); if (!no_g) g1 = a.g16 ? widen4(a.g16, sj) : NT_LOAD(a.g, sj); m1 = NT_LOAD(a.m, sj);
      if constexpr (RULE != RULE_SGD) v1 = NT_LOAD(a.v, sj);
      if constexpr (AVG) e1 = NT_LOAD(w.e.avg, sj);
    }
    // (gradients read from the bf16 payload: the fp32 buffer holds this rank's own sums, cleared whatever the payload says)
    if (f0) {
      const bool c0 = !no_g && a.zero_grads && !(f0 & 4) && (a.g16 != nullptr || any_nonzero(g0));
      if constexpr (GROUPED) { const GroupRow h = rows[f0 >> 3]; adam_update4<RULE>(h, a.adamw, coef, (f0 & 3) == 2 ? h.wd : 0.f, p0, g0, m0, v0); }
      else adam_update4<RULE>(a, a.adamw, coef, (f0 & 3) == 2 ? a.wd : 0.f, p0, g0, m0, v0);
      adam_store4<RULE>(a, i, si, p0, m0, v0, c0);
      if constexpr (AVG) avg_store4(w.e, si, p0, e0);
    }
    if (f1) {
      const bool c1 = !no_g && a.zero_grads && !(f1 & 4) && (a.g16 != nullptr || any_nonzero(g1));
      if constexpr (GROUPED) { const GroupRow h = rows[f1 >> 3]; adam_update4<RULE>(h, a.adamw, coef, (f1 & 3) == 2 ? h.wd : 0.f, p1, g1, m1, v1); }
      else adam_update4<RULE>(a, a.adamw, coef, (f1 & 3) == 2 ? a.wd : 0.f, p1, g1, m1, v1);
      adam_store4<RULE>(a, j, sj, p1, m1, v1, c1);
      if constexpr (AVG) avg_store4(w.e, sj, p1, e1);
    }
  }
}

inline int sumsq_blocks(size_t n) {
  size_t b = (n / 4 + 255) / 256;
  return (int)(b < 2048 ? (b < 1 ? 1 : b) : 2048);
}

}  // namespace

extern "C" size_t uniter_grad_sumsq_ws_bytes(size_t n) { return (size_t)sumsq_blocks(n) * sizeof(double); }

extern "C" int uniter_grad_sumsq(const float* grads, const uint8_t* chunk_flags, size_t n, double* sumsq,
                                 void* ws, size_t ws_bytes, void* stream) {
  UCHECK_ARG(grads && chunk_flags && sumsq && ws, "grad_sumsq: null pointer");
  UCHECK_SHAPE(n % CHUNK == 0, "grad_sumsq: n must be a multiple of 64");
  UCHECK_ARG(ws_bytes >= uniter_grad_sumsq_ws_bytes(n), "grad_sumsq: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nb = sumsq_blocks(n);
  hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, st, grads, chunk_flags, n / 4, (double*)ws, (const unsigned short*)nullptr);
  UCHECK_LAUNCH();
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(1024), 0, st, (const double*)ws, nb, sumsq);
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_grad_sumsq_bf16(const void* grads_bf16, const uint8_t* chunk_flags, size_t n, double* sumsq,
                                      void* ws, size_t ws_bytes, void* stream) {
  UCHECK_ARG(grads_bf16 && chunk_flags && sumsq && ws, "grad_sumsq_bf16: null pointer");
  UCHECK_SHAPE(n % CHUNK == 0 && ((uintptr_t)grads_bf16 & 7) == 0, "grad_sumsq_bf16: n must be a multiple of 64, 8-byte aligned");
  UCHECK_ARG(ws_bytes >= uniter_grad_sumsq_ws_bytes(n), "grad_sumsq_bf16: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nb = sumsq_blocks(n);
  hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, st, (const float*)nullptr, chunk_flags, n / 4, (double*)ws,
                     (const unsigned short*)grads_bf16);
  UCHECK_LAUNCH();
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(1024), 0, st, (const double*)ws, nb, sumsq);
  UCHECK_LAUNCH();
  return 0;
}

// One slice of the norm, unreduced: `nblocks` workgroups leave their partial sums in parts[0 .. nblocks); the caller joins
// the slices' partials with uniter_sumsq_combine.  chunk_flags NULL = every chunk counts (a parameter without a gradient
// this step holds zeros: the buffer is cleared by the optimizer step).
extern "C" int uniter_grad_sumsq_part(const float* grads, const uint8_t* chunk_flags, size_t n, double* parts, int nblocks,
                                      void* stream) {
  UCHECK_ARG(grads && parts && nblocks >= 1 && nblocks <= 2048, "grad_sumsq_part: bad argument");
  UCHECK_SHAPE(n % 4 == 0 && ((uintptr_t)grads & 15) == 0, "grad_sumsq_part: n must be a multiple of 4, 16-byte aligned");
  hipLaunchKernelGGL(sumsq_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, grads, chunk_flags, n / 4, parts,
                     (const unsigned short*)nullptr);
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_sumsq_combine(const double* parts, int n, double* out, void* stream) {
  UCHECK_ARG(parts && out && n >= 1, "sumsq_combine: bad argument");
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, parts, n, out);
  UCHECK_LAUNCH();
  return 0;
}

namespace {

// One optimizer step over a flat buffer: what an entry point states, by name.  An unset field means "absent".  The eleven entry points
// below fill one from their positional lists and hand it to step_run, which holds every check and the one launch.
struct StepCall {
  const char* who = "adam_step";      // prefix of the messages of the checks only some entry points have
  int rule = RULE_ADAM;               // rule_of(kind); < 0 = a kind outside 0 .. 3
  float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;      // (RULE_SGD neither reads nor writes v: it may be NULL and is dropped)
  const void* g16 = nullptr;          // the gradients as bf16 instead (AdamArgs::g16)
  const uint8_t* flags = nullptr;
  size_t n = 0;
  const double* sumsq = nullptr;
  float grad_scale = 1.f, max_norm = 0.f;
  uniter_optim_group_t hp = {};       // the launch's hyper-parameters, or (grouped) a table of n_groups rows of them in host memory
  bool grouped = false;
  const uniter_optim_group_t* groups = nullptr;
  int n_groups = 0, step = 0, adamw = 0, zero_grads = 0;
  void* mirror = nullptr;             // bf16 copy of the updated parameters; piece_stride > 0: its three x3 pieces
  size_t piece_stride = 0, first_element = 0;      // first_element: the flat-buffer offset of p, which pair_src's entries are relative to
  const int* pair_src = nullptr;      // the paired-row source table of this launch's first chunk (AdamArgs::vsrc)
  bool by_rows = false;               // one table split by rows (uniter_adam_step_rows): row_mask one byte per row of row_len elements
  const uint8_t* row_mask = nullptr;
  int row_len = 0, rows_touched = 0;
  bool averaged = false;              // an exponential moving average of the parameters in the same walk (AvgArgs)
  float* avg = nullptr;
  float avg_weight = 0.f;
  int max_workgroups = 0;
  void* stream = nullptr;
};

inline int rule_of(int kind) { return kind == 0 || kind == 1 ? RULE_ADAM : kind == 2 ? RULE_ADAMAX : kind == 3 ? RULE_SGD : -1; }

// a group's hyper-parameters with its bias corrections at `step`, formed in double once per group (and once per launch for the scalars)
GroupRow group_row(const uniter_optim_group_t& g, int step) {
  const double bc1 = 1.0 - pow((double)g.beta1, (double)step);
  const double bc2 = 1.0 - pow((double)g.beta2, (double)step);
  return GroupRow{g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, (float)((double)g.lr / bc1), (float)(1.0 / sqrt(bc2)), 0.f};
}
GroupTable group_table(const uniter_optim_group_t* groups, int n_groups, int step) {
  GroupTable t;
  t.n = n_groups;
  for (int k = 0; k < MAX_GROUPS; ++k) t.row[k] = group_row(groups[k < n_groups ? k : 0], step);
  return t;
}

template <bool GROUPED, bool AVG>
void step_launch(int rule, int nb, hipStream_t st, const WalkArgs<GROUPED, AVG>& w) {
  switch (rule) {
    case RULE_ADAMAX: hipLaunchKernelGGL((adam_kernel<RULE_ADAMAX, GROUPED, AVG>), dim3(nb), dim3(256), 0, st, w); break;
    case RULE_SGD: hipLaunchKernelGGL((adam_kernel<RULE_SGD, GROUPED, AVG>), dim3(nb), dim3(256), 0, st, w); break;
    default: hipLaunchKernelGGL((adam_kernel<RULE_ADAM, GROUPED, AVG>), dim3(nb), dim3(256), 0, st, w); break;
  }
}

int step_run(const StepCall& c) {
  // what only some forms state: every argument is checked HERE, before anything is launched
  UCHECK_ARG(c.rule >= 0, "%s: kind must be 0 (Adam), 1 (AdamW), 2 (Adamax) or 3 (SGD with momentum)", c.who);
  UCHECK_ARG(!c.averaged || c.avg, "%s: avg is NULL", c.who);
  UCHECK_ARG(!c.averaged || (c.avg_weight >= 0.f && c.avg_weight <= 1.f), "%s: avg_weight must lie in [0, 1] (got %g)", c.who, (double)c.avg_weight);
  UCHECK_SHAPE(!c.averaged || ((uintptr_t)c.avg & 15) == 0, "%s: avg must be 16-byte aligned", c.who);
  UCHECK_ARG(!c.by_rows || (c.row_mask && c.row_len > 0 && c.row_len % CHUNK == 0 && c.n % (size_t)c.row_len == 0),
             "%s: row_len must be a multiple of 64 dividing n", c.who);
  UCHECK_ARG(!c.pair_src || (c.mirror && c.piece_stride > 0 && c.first_element % CHUNK == 0 && ((uintptr_t)c.pair_src & 7) == 0),
             "%s: a source table needs the x3 mirror, a launch that starts on a chunk and an 8-byte aligned table", c.who);
  UCHECK_ARG(!c.grouped || (c.groups && c.n_groups >= 1 && c.n_groups <= MAX_GROUPS), "%s: n_groups must be 1 .. 32 (got %d) with a table", c.who,
             c.n_groups);
  UCHECK_ARG(!c.grouped || c.step >= 1, "%s: step must be >= 1", c.who);
  // what every form states
  UCHECK_SHAPE(c.piece_stride % 4 == 0 && (c.piece_stride == 0 || c.mirror), "adam_step: bad mirror piece stride");
  UCHECK_ARG(c.p && c.g && c.m && (c.v || c.rule == RULE_SGD) && c.flags, "adam_step: null pointer");
  UCHECK_SHAPE(((uintptr_t)c.g16 & 7) == 0, "adam_step: bf16 gradients must be 8-byte aligned");
  UCHECK_SHAPE(c.n % CHUNK == 0, "adam_step: n must be a multiple of 64");
  UCHECK_ARG(c.step >= 1, "adam_step: step must be >= 1");
  UCHECK_ARG(c.max_norm <= 0.f || c.sumsq, "adam_step: clipping needs sumsq");
  const GroupRow h = group_row(c.hp, c.step);      // (grouped: zeros, unused -- every chunk reads its group's row)
  AdamArgs a;
  a.p = c.p; a.g = c.g; a.m = c.m; a.v = c.rule == RULE_SGD ? nullptr : c.v; a.flags = c.flags; a.n4 = c.n / 4;
  a.sumsq = c.sumsq; a.gscale = c.grad_scale; a.max_norm = c.max_norm; a.lr = h.lr; a.b1 = h.b1; a.b2 = h.b2;
  a.eps = h.eps; a.wd = h.wd; a.step_size = h.step_size; a.inv_sqrt_bc2 = h.inv_sqrt_bc2; a.adamw = c.adamw; a.zero_grads = c.zero_grads;
  a.mirror = (unsigned short*)c.mirror; a.mirror_ps = c.piece_stride; a.g16 = (const unsigned short*)c.g16;
  a.rowmask = c.by_rows ? c.row_mask : nullptr; a.row_chunks = c.by_rows ? c.row_len / CHUNK : 1; a.rows_want = c.by_rows && c.rows_touched ? 1 : 0;
  a.vsrc = (const int2*)c.pair_src; a.vsrc_base = (long)c.first_element;
  int nb = sumsq_blocks(c.n);
  if (c.max_workgroups > 0) {
    // an explicit grid: up to the one in which every thread takes its two items once (short-lived workgroups: what a persistent
    // product of the forward pass that wants the CU waits for is ONE workgroup's lifetime)
    const size_t full = (a.n4 + 511) / 512;
    nb = (int)(full < (size_t)c.max_workgroups ? (full < 1 ? 1 : full) : (size_t)c.max_workgroups);
  }
  hipStream_t st = (hipStream_t)c.stream;
  const AvgArgs e = {c.avg, c.avg_weight};
  if (c.averaged && c.grouped) step_launch(c.rule, nb, st, WalkArgs<true, true>{a, group_table(c.groups, c.n_groups, c.step), e});
  else if (c.averaged) step_launch(c.rule, nb, st, WalkArgs<false, true>{a, e});
  else if (c.grouped) step_launch(c.rule, nb, st, WalkArgs<true, false>{a, group_table(c.groups, c.n_groups, c.step)});
  else step_launch(c.rule, nb, st, WalkArgs<false, false>{a});
  UCHECK_LAUNCH();
  return 0;
}

}  // namespace

// what the entry points' positional lists share, by their parameters' names: the buffers and the step; the launch's own
// hyper-parameters; the x3 mirror with its pair source
#define STEP_IN(c)                                                                                                                      \
  StepCall c;                                                                                                                           \
  c.p = params; c.g = grads; c.m = exp_avg; c.v = exp_avg_sq; c.flags = chunk_flags; c.n = n; c.sumsq = sumsq; c.grad_scale = grad_scale; \
  c.max_norm = max_norm; c.step = step; c.zero_grads = zero_grads; c.stream = stream
#define STEP_SCALARS(c) c.hp = {lr, beta1, beta2, eps, weight_decay}; c.adamw = adamw
#define STEP_X3P(c)                                                                                                              \
  c.g16 = grads_bf16; c.mirror = mirror; c.piece_stride = mirror_piece_stride; c.pair_src = pair_src; c.first_element = first_element; \
  c.max_workgroups = max_workgroups

extern "C" int uniter_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* chunk_flags, size_t n,
                                const double* sumsq, float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps,
                                float weight_decay, int step, int adamw, int zero_grads, void* stream) {
  STEP_IN(c); STEP_SCALARS(c);
  return step_run(c);
}

extern "C" int uniter_adam_step_mirror(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* chunk_flags, size_t n,
                                       const double* sumsq, float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps,
                                       float weight_decay, int step, int adamw, int zero_grads, void* mirror_bf16, void* stream) {
  STEP_IN(c); STEP_SCALARS(c); c.mirror = mirror_bf16;
  return step_run(c);
}

extern "C" int uniter_adam_step_ex(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* chunk_flags, size_t n,
                                   const double* sumsq, float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int step, int adamw, int zero_grads, void* mirror_bf16, int max_workgroups,
                                   void* stream) {
  STEP_IN(c); STEP_SCALARS(c); c.mirror = mirror_bf16; c.max_workgroups = max_workgroups;
  return step_run(c);
}

extern "C" int uniter_adam_step_g16(float* params, float* grads, const void* grads_bf16, float* exp_avg, float* exp_avg_sq,
                                    const uint8_t* chunk_flags, size_t n, const double* sumsq, float grad_scale, float max_norm, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int step, int adamw, int zero_grads,
                                    void* mirror_bf16, int max_workgroups, void* stream) {
  STEP_IN(c); STEP_SCALARS(c); c.g16 = grads_bf16; c.mirror = mirror_bf16; c.max_workgroups = max_workgroups;
  return step_run(c);
}

extern "C" int uniter_adam_step_x3(float* params, float* grads, const void* grads_bf16, float* exp_avg, float* exp_avg_sq,
                                   const uint8_t* chunk_flags, size_t n, const double* sumsq, float grad_scale, float max_norm, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int step, int adamw, int zero_grads,
                                   void* mirror_bf16, size_t mirror_piece_stride, int max_workgroups, void* stream) {
  STEP_IN(c); STEP_SCALARS(c); c.g16 = grads_bf16; c.mirror = mirror_bf16; c.piece_stride = mirror_piece_stride;
  c.max_workgroups = max_workgroups;
  return step_run(c);
}

// uniter_adam_step_x3 that writes the weight pieces in the PAIRED-ROW layout (round 6) by walking the buffer in the MIRROR's order:
// pair_src points at the source table's entry for this launch's first 64-element chunk -- two int32 per chunk, the flat-buffer
// element offsets of the chunk's two 32-element units ({s0 < 0, ..} = the chunk is its own source; ParamStore.pair_src);
// first_element = the flat-buffer offset of `params` (the table's offsets are absolute).
extern "C" int uniter_adam_step_x3p(float* params, float* grads, const void* grads_bf16, float* exp_avg, float* exp_avg_sq,
                                    const uint8_t* chunk_flags, size_t n, const double* sumsq, float grad_scale, float max_norm, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int step, int adamw, int zero_grads,
                                    void* mirror, size_t mirror_piece_stride, const int* pair_src, size_t first_element, int max_workgroups,
                                    void* stream) {
  STEP_IN(c); c.who = "adam_step_x3p"; STEP_SCALARS(c); STEP_X3P(c);
  return step_run(c);
}

// The update of ONE table split by rows (round 6): a fine-tuning step touches at most B x T of the word-embedding table's 28996 rows
// (model/model.py:220-221), yet torch.optim.Adam with weight_decay updates every row (utils/optim_utils.py:33-40: g += wd p) -- 0.62 of
// the step's 3.18 GB -- and the next forward's text branch waits for all of it.  A row WITHOUT a gradient is updated from g = 0, which
// neither the clip coefficient nor the gradient exchange can change (0 x c = 0): its update does not depend on this step's backward
// pass at all.  So the table's launch is two: rows_touched = 0 -- the rows whose mask byte is 0, g taken as zero (never read), any
// time after the previous step's update, e.g. beside the backward pass; rows_touched = 1 -- the masked rows with their gradients,
// clipped, behind the backward pass as before (a few per cent of the table).  Same arithmetic per element: bit-identical parameters.
// params .. chunk_flags point at the TABLE (row 0); n = rows x row_len with row_len % 64 == 0; row_mask one byte per row.
extern "C" int uniter_adam_step_rows(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* chunk_flags, size_t n,
                                     const double* sumsq, float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps,
                                     float weight_decay, int step, int adamw, int zero_grads, const uint8_t* row_mask, int row_len,
                                     int rows_touched, int max_workgroups, void* stream) {
  STEP_IN(c); c.who = "adam_step_rows"; STEP_SCALARS(c); c.max_workgroups = max_workgroups;
  c.by_rows = true; c.row_mask = row_mask; c.row_len = row_len; c.rows_touched = rows_touched;
  // the untouched rows' g is zero whatever the norm: their launch neither reads sumsq nor clips (and may run before the norm exists)
  if (!rows_touched) { c.sumsq = nullptr; c.max_norm = 0.f; }
  return step_run(c);
}

// The optimizer family behind one entry point (include/uniter_hip.h): kind 0 / 1 = uniter_adam_step_x3p with adamw = 0 / 1 (and its
// message prefix), kind 2 = torch.optim.Adamax, kind 3 = torch.optim.SGD with momentum beta1 (exp_avg_sq may be NULL and is neither
// read nor written).  The adamw argument is not read: the kind says it.
extern "C" int uniter_optim_step(int kind, float* params, float* grads, const void* grads_bf16, float* exp_avg, float* exp_avg_sq,
                                 const uint8_t* chunk_flags, size_t n, const double* sumsq, float grad_scale, float max_norm, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int step, int adamw, int zero_grads, void* mirror,
                                 size_t mirror_piece_stride, const int* pair_src, size_t first_element, int max_workgroups, void* stream) {
  STEP_IN(c); c.rule = rule_of(kind);
  c.who = c.rule == RULE_ADAM ? "adam_step_x3p" : "optim_step";
  STEP_SCALARS(c); STEP_X3P(c); c.adamw = kind == 1;
  return step_run(c);
}

// uniter_optim_step with the hyper-parameters PER PARAMETER GROUP (include/uniter_hip.h): bits 3-7 of a chunk's flag name its row of
// `groups` (host memory, copied into the launch's arguments); the clip coefficient stays one value for the launch.
extern "C" int uniter_optim_step_groups(int kind, float* params, float* grads, const void* grads_bf16, float* exp_avg, float* exp_avg_sq,
                                        const uint8_t* chunk_flags, size_t n, const double* sumsq, float grad_scale, float max_norm,
                                        const uniter_optim_group_t* groups, int n_groups, int step, int zero_grads, void* mirror,
                                        size_t mirror_piece_stride, const int* pair_src, size_t first_element, int max_workgroups,
                                        void* stream) {
  STEP_IN(c); c.who = "optim_step_groups"; c.rule = rule_of(kind);
  STEP_X3P(c); c.adamw = kind == 1; c.grouped = true; c.groups = groups; c.n_groups = n_groups;
  return step_run(c);
}

// uniter_optim_step / uniter_optim_step_groups with an exponential moving average of the parameters updated by the same launch
// (include/uniter_hip.h): avg points at the element `params` points at; a' = a + avg_weight (p' - a) on every updated element.
extern "C" int uniter_optim_step_avg(int kind, float* params, float* grads, const void* grads_bf16, float* exp_avg, float* exp_avg_sq,
                                     const uint8_t* chunk_flags, size_t n, const double* sumsq, float grad_scale, float max_norm, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int step, int adamw, int zero_grads,
                                     void* mirror, size_t mirror_piece_stride, const int* pair_src, size_t first_element, float* avg,
                                     float avg_weight, int max_workgroups, void* stream) {
  STEP_IN(c); c.who = "optim_step_avg"; c.rule = rule_of(kind);
  STEP_SCALARS(c); STEP_X3P(c); c.adamw = kind == 1; c.averaged = true; c.avg = avg; c.avg_weight = avg_weight;
  return step_run(c);
}

extern "C" int uniter_optim_step_groups_avg(int kind, float* params, float* grads, const void* grads_bf16, float* exp_avg,
                                            float* exp_avg_sq, const uint8_t* chunk_flags, size_t n, const double* sumsq, float grad_scale,
                                            float max_norm, const uniter_optim_group_t* groups, int n_groups, int step, int zero_grads,
                                            void* mirror, size_t mirror_piece_stride, const int* pair_src, size_t first_element, float* avg,
                                            float avg_weight, int max_workgroups, void* stream) {
  STEP_IN(c); c.who = "optim_step_groups_avg"; c.rule = rule_of(kind);
  STEP_X3P(c); c.adamw = kind == 1; c.grouped = true; c.groups = groups; c.n_groups = n_groups;
  c.averaged = true; c.avg = avg; c.avg_weight = avg_weight;
  return step_run(c);
}
