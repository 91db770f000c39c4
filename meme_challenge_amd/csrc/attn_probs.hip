// The attention probabilities as an OUTPUT, and attention rollout on them:
//   uniter_attn_probs    p_ij = exp(s_ij - lse_i), s_ij = q_i . k_j / 8 + (1 - mask_j) * -10000   (BertSelfAttention.forward,
//                        model/layer.py:85-95, before the dropout), per head [B, nh, L, L] or as the mean over heads [B, L, L]
//   uniter_attn_rollout  R_0 = A~_0, R_l = A~_l R_{l-1} with A~_l = residual I + (1 - residual) A_l per sample
//                        (Abnar & Zuidema, "Quantifying Attention Flow in Transformers", 2020)
// The attention kernels (attention_f32.hip, attention_x3.hip, attention_bf16.hip) keep the probabilities in registers; this file
// recomputes them from the query|key|value buffer those kernels read, so it changes nothing in them.
//
// fp32 arithmetic on the vector pipe throughout -- 0.66 GFLOP per layer at B 16, L 164, 12 heads against 20.7 MB of stores -- with
// every sum in a fixed order and no atomics: each output element has one writer, is written once, and is a function of qkv and the
// mask alone.  Any L >= 1: the keys pass in chunks of 64, twice (row maximum and sum, then the probabilities).
#include "common.h"

namespace {

constexpr int PRMAX = 16;    // query rows of a workgroup: 4 waves x RW rows, RW = 4 per head, RW = 1 for the head mean
constexpr int PK = 64;       // keys of a chunk: one per lane
constexpr int PLD = 68;      // floats per LDS row: 16-byte reads of 16 lanes with consecutive rows fall on 16 different slots
constexpr int PMAXH = 64;    // heads whose row statistics a workgroup keeps (head_mean = 1)

struct ProbsArgs {
  const void* qkv; const float* mask; const int32_t* cu; float* out;
  int B, L, nh, head_mean;
};

template <bool B16>
__device__ __forceinline__ f32x4 load4(const void* base, size_t elem) {      // elem % 4 == 0
  if (B16) {
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(base) + elem);
    f32x4 r;
    r[0] = __uint_as_float(v.x << 16); r[1] = __uint_as_float(v.x & 0xffff0000u);
    r[2] = __uint_as_float(v.y << 16); r[3] = __uint_as_float(v.y & 0xffff0000u);
    return r;
  }
  return *reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + elem);
}

// ROWS x 64 values of one head into dst[ROWS][PLD]; rows at or beyond `valid` are zeros and are not read
template <bool B16, int ROWS>
__device__ __forceinline__ void stage_rows(float* dst, const void* src, size_t first_row, int valid, size_t ld, size_t col) {
#pragma unroll
  for (int it = 0; it < (ROWS + 15) / 16; ++it) {
    const int r = it * 16 + ((int)threadIdx.x >> 4), c4 = (int)threadIdx.x & 15;
    if (ROWS % 16 != 0 && r >= ROWS) break;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < valid) v = load4<B16>(src, (first_row + r) * ld + col + c4 * 4);
    *reinterpret_cast<f32x4*>(dst + r * PLD + c4 * 4) = v;
  }
}

// s[r] = q_(RW wave + r) . k_lane: 64 terms added in ascending order
template <int RW>
__device__ __forceinline__ void dots(const float* Qs, const float* Ks, int wave, int lane, float s[RW]) {
  const f32x4* kr = reinterpret_cast<const f32x4*>(Ks + lane * PLD);
  const f32x4* qr = reinterpret_cast<const f32x4*>(Qs + wave * RW * PLD);
#pragma unroll
  for (int r = 0; r < RW; ++r) s[r] = 0.f;
#pragma unroll 4
  for (int d4 = 0; d4 < 16; ++d4) {
    const f32x4 kv = kr[d4];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const f32x4 qv = qr[r * (PLD / 4) + d4];      // (one address per wave: a broadcast)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[r] = fmaf(qv[e], kv[e], s[r]);
    }
  }
}

// grid (ceil(L / (4 RW)), head_mean ? 1 : nh, B), 256 threads.  Wave w owns the query rows i0 + RW w .. + RW - 1, lane the key
// j0 + lane of every chunk.  Pass 1, per head: lse of the workgroup's rows (an online softmax per lane over its keys, then the lanes
// joined by the shuffle tree) into LDS.  Pass 2, per chunk of keys: the heads in ascending order, p = exp(s - lse) added up in a
// register, one store.  RW = 4 rows per wave where every head has workgroups of its own; the head mean, whose workgroups walk all
// the heads, takes RW = 1: four times the workgroups (656 instead of 176 at B 16, L 164) for 256 CUs.
template <bool B16, int RW>
__global__ __launch_bounds__(256, 4) void attn_probs_kernel(const ProbsArgs a) {
  constexpr int PR = 4 * RW;
  __shared__ __attribute__((aligned(16))) float Qs[PR * PLD];
  __shared__ __attribute__((aligned(16))) float Ks[PK * PLD];
  __shared__ float lse_s[PMAXH][PR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z, i0 = blockIdx.x * PR;
  const int L = a.L, nh = a.nh;
  const size_t ld = (size_t)3 * nh * 64;
  // the sample's rows of qkv and its length: in the packed form rows and keys at or beyond n do not exist
  size_t r0 = (size_t)b * L;
  int n = L;
  if (a.cu) {
    const int c0 = a.cu[b], c1 = a.cu[b + 1];
    r0 = (size_t)c0;
    n = c1 - c0;
    n = n < 0 ? 0 : (n > L ? L : n);
  }
  const int h0 = a.head_mean ? 0 : (int)blockIdx.y, nhead = a.head_mean ? nh : 1;
  const int qvalid = n - i0;      // (rows of this workgroup that exist; <= 0: none)

  // ---- pass 1 ----
  for (int hh = 0; hh < nhead && qvalid > 0; ++hh) {      // (uniform)
    const int h = h0 + hh;
    float m[RW], l[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
    for (int j0 = 0; j0 < n; j0 += PK) {
      __syncthreads();
      if (j0 == 0) stage_rows<B16, PR>(Qs, a.qkv, r0 + i0, qvalid, ld, (size_t)h * 64);
      stage_rows<B16, PK>(Ks, a.qkv, r0 + j0, n - j0, ld, (size_t)(nh + h) * 64);
      __syncthreads();
      float s[RW];
      dots<RW>(Qs, Ks, wave, lane, s);
      const int j = j0 + lane;
      if (j < n) {
        const float bias = a.mask ? (1.0f - a.mask[(size_t)b * L + j]) * -10000.0f : 0.f;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          const float x = s[r] * 0.125f + bias;
          const float mn = fmaxf(m[r], x);
          l[r] = l[r] * expf(m[r] - mn) + expf(x - mn);
          m[r] = mn;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const float M = wave_max(m[r]);                      // (finite: lane 0 has a key, and the mask's bias is finite)
      const float lsum = wave_sum(l[r] * expf(m[r] - M));  // (a lane without a key: 0 * exp(-inf) = 0)
      if (lane == 0) lse_s[hh][wave * RW + r] = M + logf(lsum);
    }
  }

  // ---- pass 2 ----
  const float div = (float)nhead;
  for (int j0 = 0; j0 < L; j0 += PK) {
    const int j = j0 + lane;
    float acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = 0.f;
    if (j0 < n && qvalid > 0) {      // (uniform)
      const float bias = (a.mask && j < n) ? (1.0f - a.mask[(size_t)b * L + j]) * -10000.0f : 0.f;
      for (int hh = 0; hh < nhead; ++hh) {
        const int h = h0 + hh;
        __syncthreads();
        stage_rows<B16, PR>(Qs, a.qkv, r0 + i0, qvalid, ld, (size_t)h * 64);
        stage_rows<B16, PK>(Ks, a.qkv, r0 + j0, n - j0, ld, (size_t)(nh + h) * 64);
        __syncthreads();
        float s[RW];
        dots<RW>(Qs, Ks, wave, lane, s);
        if (j < n) {
#pragma unroll
          for (int r = 0; r < RW; ++r) {
            const int row = wave * RW + r;
            if (row < qvalid) acc[r] += expf((s[r] * 0.125f + bias) - lse_s[hh][row]);
          }
        }
      }
    }
    if (j < L) {
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int i = i0 + wave * RW + r;
        if (i < L) {
          const size_t plane = a.head_mean ? (size_t)b : (size_t)b * nh + h0;
          a.out[(plane * L + i) * L + j] = acc[r] / div;      // (rows and keys beyond a packed sample's length: 0)
        }
      }
    }
  }
}

// ---- rollout ----
constexpr int RT = 32;      // output tile and k-chunk

__device__ __forceinline__ float with_residual(float a, bool diag, float res, float omr) { return omr * a + (diag ? res : 0.f); }

// grid (ceil(L L / 256), B): R_0 = A~_0
__global__ __launch_bounds__(256) void rollout_first_kernel(const float* __restrict__ A, float* __restrict__ out, int L, float res, float omr) {
  const size_t LL = (size_t)L * L, e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LL) return;
  const size_t base = (size_t)blockIdx.y * LL;
  const int i = (int)(e / L), k = (int)(e - (size_t)i * L);
  out[base + e] = with_residual(A[base + e], i == k, res, omr);
}

// grid (ceil(L / 32), ceil(L / 32), B), 256 threads: out = A~ Rin, a 32 x 32 tile per workgroup, thread (tx, ty) the rows ty, ty + 8,
// ty + 16, ty + 24 of column tx; the L terms of every element added in ascending k
__global__ __launch_bounds__(256) void rollout_step_kernel(const float* __restrict__ A, const float* __restrict__ Rin,
                                                           float* __restrict__ Rout, int L, float res, float omr) {
  __shared__ float As[RT][RT + 1];
  __shared__ float Bs[RT][RT + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int row0 = blockIdx.y * RT, col0 = blockIdx.x * RT;
  const size_t base = (size_t)blockIdx.z * L * L;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < L; k0 += RT) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rr = ty + 8 * q;
      const int i = row0 + rr, k = k0 + tx;
      As[rr][tx] = (i < L && k < L) ? with_residual(A[base + (size_t)i * L + k], i == k, res, omr) : 0.f;
      const int kk = k0 + rr, j = col0 + tx;
      Bs[rr][tx] = (kk < L && j < L) ? Rin[base + (size_t)kk * L + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RT; ++k) {
      const float bv = Bs[k][tx];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = fmaf(As[ty + 8 * q][k], bv, acc[q]);
    }
  }
  const int j = col0 + tx;
  if (j < L) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = row0 + ty + 8 * q;
      if (i < L) Rout[base + (size_t)i * L + j] = acc[q];
    }
  }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int uniter_attn_probs(const void* qkv, int qkv_is_bf16, const float* attn_mask, const int32_t* cu_seqlens, float* probs,
                                 int B, int L, int nh, int head_mean, void* stream) {
  UCHECK_ARG(qkv && probs, "attn_probs: null pointer");
  UCHECK_ARG((attn_mask != nullptr) != (cu_seqlens != nullptr), "attn_probs: exactly one of attn_mask / cu_seqlens");
  UCHECK_ARG(((uintptr_t)qkv & 15) == 0, "attn_probs: qkv must be 16-byte aligned");
  UCHECK_ARG(((uintptr_t)probs & 3) == 0, "attn_probs: probs must be 4-byte aligned");
  UCHECK_SHAPE(B >= 1 && L >= 1 && nh >= 1, "attn_probs: bad shape B %d L %d nh %d (heads of 64)", B, L, nh);
  UCHECK_SHAPE(B <= 65535 && nh <= 65535, "attn_probs: at most 65535 samples and heads (B %d nh %d)", B, nh);
  UCHECK_SHAPE(!head_mean || nh <= PMAXH, "attn_probs: the mean over heads takes at most %d heads (got %d)", PMAXH, nh);
  ProbsArgs a = {};
  a.qkv = qkv; a.mask = attn_mask; a.cu = cu_seqlens; a.out = probs; a.B = B; a.L = L; a.nh = nh; a.head_mean = head_mean ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (head_mean) {
    const dim3 grid((L + 3) / 4, 1, B);
    if (qkv_is_bf16) hipLaunchKernelGGL((attn_probs_kernel<true, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_probs_kernel<false, 1>), grid, dim3(256), 0, st, a);
  } else {
    const dim3 grid((L + PRMAX - 1) / PRMAX, nh, B);
    if (qkv_is_bf16) hipLaunchKernelGGL((attn_probs_kernel<true, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_probs_kernel<false, 4>), grid, dim3(256), 0, st, a);
  }
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_attn_rollout(const float* attn, float* rollout, float* tmp, int nl, int B, int L, float residual, void* stream) {
  UCHECK_ARG(attn && rollout && (tmp || nl == 1), "attn_rollout: null pointer");
  UCHECK_SHAPE(nl >= 1 && B >= 1 && L >= 1 && B <= 65535, "attn_rollout: bad shape nl %d B %d L %d", nl, B, L);
  UCHECK_ARG(residual >= 0.f && residual <= 1.f, "attn_rollout: residual must lie in [0, 1]");
  const size_t one = (size_t)B * L * L * sizeof(float);
  UCHECK_ARG(!overlap(attn, one * nl, rollout, one) && (!tmp || (!overlap(attn, one * nl, tmp, one) && !overlap(rollout, one, tmp, one))),
             "attn_rollout: attn, rollout and tmp must not overlap");
  hipStream_t st = (hipStream_t)stream;
  const float omr = 1.0f - residual;
  // the product of layer l lands in rollout when nl - 1 - l is even, so that the last one does
  auto dst = [&](int l) { return (nl - 1 - l) % 2 == 0 ? rollout : tmp; };
  const size_t LL = (size_t)L * L;
  UCHECK_SHAPE((LL + 255) / 256 <= 0x7fffffffu, "attn_rollout: L %d too long", L);
  hipLaunchKernelGGL(rollout_first_kernel, dim3((unsigned)((LL + 255) / 256), B), dim3(256), 0, st, attn, dst(0), L, residual, omr);
  UCHECK_LAUNCH();
  const dim3 grid((L + RT - 1) / RT, (L + RT - 1) / RT, B);
  for (int l = 1; l < nl; ++l) {
    hipLaunchKernelGGL(rollout_step_kernel, grid, dim3(256), 0, st, attn + (size_t)l * B * LL, (const float*)dst(l - 1), dst(l), L,
                       residual, omr);
    UCHECK_LAUNCH();
  }
  return 0;
}
