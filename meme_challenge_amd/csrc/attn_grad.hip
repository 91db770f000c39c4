// Gradient-weighted attention maps, the relevance they propagate, and the per-head sums that score a head's importance:
//   uniter_attn_grad       g_ij = p_ij dP_ij with p_ij = exp(s_ij - lse_i), s_ij = q_i . k_j / 8 + (1 - mask_j) * -10000 (the probabilities
//                          of csrc/attn_probs.hip, before the dropout) and dP_ij = dO_i . v_j, the gradient of the target with respect to
//                          p_ij given dO = d target / d context.  Per head [B, nh, L, L] (signed), or A^_ = (1 / nh) sum_h max(g, 0)
//                          [B, L, L] (Chefer, Gur & Wolf, "Generic Attention-model Explainability for Interpreting Bi-Modal and
//                          Encoder-Decoder Transformers", 2021); optionally head_sums [B, nh] = sum_ij g_ij = d target / d gate_h
//                          (Michel, Levy & Neubig, "Are Sixteen Heads Really Better than One?", 2019)
//   uniter_attn_relevance  R_0 = I + A^_0, R_l = R_{l-1} + A^_l R_{l-1} per sample
// The attention backward kernels keep p and dP in registers; this file recomputes both from the buffers those kernels read (the
// query|key|value buffer and the gradient of the context, the latter possibly as k-piece slabs that are summed here), so it changes
// nothing in them.
//
// fp32 arithmetic on the vector pipe, the staging and dot-product pattern of attn_probs.hip with twice its products.  Every sum in a
// fixed order and no atomics: each output element has one writer and is written once; head_sums goes through one partial per
// workgroup in the caller's workspace, added in ascending tile order by a second launch.  Any L >= 1.
#include "common.h"

namespace {

constexpr int GK = 64;       // keys of a chunk: one per lane
constexpr int GLD = 68;      // floats per LDS row: 16-byte reads of 16 lanes with consecutive rows fall on 16 different slots
constexpr int GMAXH = 64;    // heads a workgroup walks (reduce = 1)

struct GradArgs {
  const void* qkv; const float* mask; const int32_t* cu; const float* dctx; size_t slab_stride; float* out; float* part;
  int B, L, nh, reduce, n_slabs, ntiles;
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

// ROWS x 64 values of one head into dst[ROWS][GLD]; rows at or beyond `valid` are zeros and are not read.  n_slabs > 1 (fp32 only):
// the sum of the slabs at `stride` elements, added in ascending order
template <bool B16, int ROWS>
__device__ __forceinline__ void stage_rows(float* dst, const void* src, size_t first_row, int valid, size_t ld, size_t col,
                                           int n_slabs = 1, size_t stride = 0) {
#pragma unroll
  for (int it = 0; it < (ROWS + 15) / 16; ++it) {
    const int r = it * 16 + ((int)threadIdx.x >> 4), c4 = (int)threadIdx.x & 15;
    if (ROWS % 16 != 0 && r >= ROWS) break;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < valid) {
      const size_t e = (first_row + r) * ld + col + c4 * 4;
      v = load4<B16>(src, e);
      for (int s = 1; s < n_slabs; ++s) v += load4<false>(src, e + (size_t)s * stride);
    }
    *reinterpret_cast<f32x4*>(dst + r * GLD + c4 * 4) = v;
  }
}

// s[r] = a_(RW wave + r) . b_lane: 64 terms added in ascending order
template <int RW>
__device__ __forceinline__ void dots(const float* As, const float* Bs, int wave, int lane, float s[RW]) {
  const f32x4* br = reinterpret_cast<const f32x4*>(Bs + lane * GLD);
  const f32x4* ar = reinterpret_cast<const f32x4*>(As + wave * RW * GLD);
#pragma unroll
  for (int r = 0; r < RW; ++r) s[r] = 0.f;
#pragma unroll 4
  for (int d4 = 0; d4 < 16; ++d4) {
    const f32x4 bv = br[d4];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const f32x4 av = ar[r * (GLD / 4) + d4];      // (one address per wave: a broadcast)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[r] = fmaf(av[e], bv[e], s[r]);
    }
  }
}

// grid (ceil(L / (4 RW)), reduce ? 1 : nh, B), 256 threads.  Wave w owns the query rows i0 + RW w .. + RW - 1, lane the key j0 + lane
// of every chunk.  Pass 1, per head: lse of the workgroup's rows, as attn_probs.hip computes it.  Pass 2, per chunk of keys: the
// heads in ascending order, g = exp(s - lse) (dO_i . v_j), one store.  Per head RW = 4 and every head has workgroups of its own; the
// reduced form, whose workgroups walk all the heads, takes RW = 1 (656 workgroups at B 16, L 164; RW = 2 measured 279 us per layer
// against 243).  The sum of g over the workgroup's tile, per head: lane sums in chunk order, the shuffle tree, lane 0 of each wave
// adds to its own LDS word, the four waves joined in ascending order at the end.
template <bool B16, int RW>
__global__ __launch_bounds__(256, 2) void attn_grad_kernel(const GradArgs a) {
  constexpr int PR = 4 * RW;
  constexpr int NHS = RW == 1 ? GMAXH : 1;
  __shared__ __attribute__((aligned(16))) float Qs[PR * GLD];
  __shared__ __attribute__((aligned(16))) float Ds[PR * GLD];
  __shared__ __attribute__((aligned(16))) float Ks[GK * GLD];
  __shared__ __attribute__((aligned(16))) float Vs[GK * GLD];
  __shared__ float lse_s[NHS][PR];
  __shared__ float hs_s[NHS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z, i0 = blockIdx.x * PR;
  const int L = a.L, nh = a.nh;
  const size_t ld = (size_t)3 * nh * 64, ldd = (size_t)nh * 64;
  // the sample's rows of qkv / dctx and its length: in the packed form rows and keys at or beyond n do not exist
  size_t r0 = (size_t)b * L;
  int n = L;
  if (a.cu) {
    const int c0 = a.cu[b], c1 = a.cu[b + 1];
    r0 = (size_t)c0;
    n = c1 - c0;
    n = n < 0 ? 0 : (n > L ? L : n);
  }
  const int h0 = a.reduce ? 0 : (int)blockIdx.y, nhead = a.reduce ? nh : 1;
  const int qvalid = n - i0;      // (rows of this workgroup that exist; <= 0: none)
  if ((int)threadIdx.x < NHS * 4) (&hs_s[0][0])[threadIdx.x] = 0.f;
  __syncthreads();

  // ---- pass 1 ----
  for (int hh = 0; hh < nhead && qvalid > 0; ++hh) {      // (uniform)
    const int h = h0 + hh;
    float m[RW], l[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
    for (int j0 = 0; j0 < n; j0 += GK) {
      __syncthreads();
      if (j0 == 0) stage_rows<B16, PR>(Qs, a.qkv, r0 + i0, qvalid, ld, (size_t)h * 64);
      stage_rows<B16, GK>(Ks, a.qkv, r0 + j0, n - j0, ld, (size_t)(nh + h) * 64);
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
  for (int j0 = 0; j0 < L; j0 += GK) {
    const int j = j0 + lane;
    float acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = 0.f;
    if (j0 < n && qvalid > 0) {      // (uniform)
      const float bias = (a.mask && j < n) ? (1.0f - a.mask[(size_t)b * L + j]) * -10000.0f : 0.f;
      for (int hh = 0; hh < nhead; ++hh) {
        const int h = h0 + hh;
        __syncthreads();
        if (nhead > 1 || j0 == 0) {      // (one head: its query rows and their gradient stay for every chunk)
          stage_rows<B16, PR>(Qs, a.qkv, r0 + i0, qvalid, ld, (size_t)h * 64);
          stage_rows<false, PR>(Ds, a.dctx, r0 + i0, qvalid, ldd, (size_t)h * 64, a.n_slabs, a.slab_stride);
        }
        stage_rows<B16, GK>(Ks, a.qkv, r0 + j0, n - j0, ld, (size_t)(nh + h) * 64);
        stage_rows<B16, GK>(Vs, a.qkv, r0 + j0, n - j0, ld, (size_t)(2 * nh + h) * 64);
        __syncthreads();
        float s[RW], dp[RW];
        dots<RW>(Qs, Ks, wave, lane, s);
        dots<RW>(Ds, Vs, wave, lane, dp);
        float hsum = 0.f;
        if (j < n) {
#pragma unroll
          for (int r = 0; r < RW; ++r) {
            const int row = wave * RW + r;
            if (row < qvalid) {
              const float g = expf((s[r] * 0.125f + bias) - lse_s[hh][row]) * dp[r];
              hsum += g;
              acc[r] += a.reduce ? fmaxf(g, 0.f) : g;
            }
          }
        }
        if (a.part) {      // (uniform)
          hsum = wave_sum(hsum);
          if (lane == 0) hs_s[hh][wave] += hsum;
        }
      }
    }
    if (j < L) {
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int i = i0 + wave * RW + r;
        if (i < L) {
          const size_t plane = a.reduce ? (size_t)b : (size_t)b * nh + h0;
          a.out[(plane * L + i) * L + j] = acc[r] / div;      // (rows and keys beyond a packed sample's length: 0)
        }
      }
    }
  }
  if (a.part) {
    __syncthreads();
    if ((int)threadIdx.x < nhead) {
      const float* w = hs_s[threadIdx.x];
      a.part[((size_t)b * nh + h0 + threadIdx.x) * a.ntiles + blockIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
    }
  }
}

// one thread per (sample, head): the workgroups' partial sums in ascending tile order
__global__ __launch_bounds__(256) void head_sums_kernel(const float* __restrict__ part, float* __restrict__ out, int count, int ntiles) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float acc = 0.f;
  for (int t = 0; t < ntiles; ++t) acc += part[(size_t)e * ntiles + t];
  out[e] = acc;
}

// ---- relevance ----
constexpr int RT = 32;      // output tile and k-chunk

// grid (ceil(L L / 256), B): R_0 = I + A^_0
__global__ __launch_bounds__(256) void relevance_first_kernel(const float* __restrict__ A, float* __restrict__ out, int L) {
  const size_t LL = (size_t)L * L, e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LL) return;
  const size_t base = (size_t)blockIdx.y * LL;
  const int i = (int)(e / L), k = (int)(e - (size_t)i * L);
  out[base + e] = A[base + e] + (i == k ? 1.f : 0.f);
}

// grid (ceil(L / 32), ceil(L / 32), B), 256 threads: Rout = Rin + A Rin, a 32 x 32 tile per workgroup, thread (tx, ty) the rows ty,
// ty + 8, ty + 16, ty + 24 of column tx; the L terms of every element's product added in ascending k, then the element of Rin
__global__ __launch_bounds__(256) void relevance_step_kernel(const float* __restrict__ A, const float* __restrict__ Rin,
                                                             float* __restrict__ Rout, int L) {
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
      As[rr][tx] = (i < L && k < L) ? A[base + (size_t)i * L + k] : 0.f;
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
      if (i < L) Rout[base + (size_t)i * L + j] = Rin[base + (size_t)i * L + j] + acc[q];
    }
  }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

inline int tiles_of(int L, int reduce) { return reduce ? (L + 3) / 4 : (L + 15) / 16; }

}  // namespace

extern "C" size_t uniter_attn_grad_ws_bytes(int B, int L, int nh) {
  if (B < 1 || L < 1 || nh < 1) return 0;
  return (size_t)B * nh * tiles_of(L, 1) * sizeof(float);      // (the reduced form has the smaller tiles)
}

extern "C" int uniter_attn_grad(const void* qkv, int qkv_is_bf16, const float* attn_mask, const int32_t* cu_seqlens, const float* dctx,
                                int n_slabs, size_t slab_stride, float* out, float* head_sums, void* ws, size_t ws_bytes, int B, int L,
                                int nh, int reduce, void* stream) {
  UCHECK_ARG(qkv && dctx && out, "attn_grad: null pointer");
  UCHECK_ARG((attn_mask != nullptr) != (cu_seqlens != nullptr), "attn_grad: exactly one of attn_mask / cu_seqlens");
  UCHECK_ARG(n_slabs >= 1, "attn_grad: n_slabs must be >= 1 (got %d)", n_slabs);
  UCHECK_ARG((((uintptr_t)qkv | (uintptr_t)dctx) & 15) == 0 && (n_slabs == 1 || slab_stride % 4 == 0),
             "attn_grad: qkv, dctx and its slabs must be 16-byte aligned");
  UCHECK_ARG((((uintptr_t)out | (uintptr_t)head_sums | (uintptr_t)ws) & 3) == 0, "attn_grad: out, head_sums and ws must be 4-byte aligned");
  UCHECK_SHAPE(B >= 1 && L >= 1 && nh >= 1, "attn_grad: bad shape B %d L %d nh %d (heads of 64)", B, L, nh);
  UCHECK_SHAPE(B <= 65535 && nh <= 65535, "attn_grad: at most 65535 samples and heads (B %d nh %d)", B, nh);
  UCHECK_SHAPE(!reduce || nh <= GMAXH, "attn_grad: the reduction over heads takes at most %d heads (got %d)", GMAXH, nh);
  // (the packed form's row count is on the device: there the overlap checks cover the first row of qkv and of each slab of dctx)
  const size_t rows = attn_mask ? (size_t)B * L : 1, Hd = (size_t)nh * 64;
  const size_t n_qkv = rows * 3 * Hd * (qkv_is_bf16 ? 2 : 4);
  const size_t n_dctx = ((size_t)(n_slabs - 1) * slab_stride + rows * Hd) * sizeof(float);
  const size_t n_mask = attn_mask ? (size_t)B * L * sizeof(float) : (size_t)(B + 1) * sizeof(int32_t);
  const void* mk = attn_mask ? (const void*)attn_mask : (const void*)cu_seqlens;
  const size_t n_out = (size_t)B * (reduce ? 1 : nh) * L * L * sizeof(float), n_hs = (size_t)B * nh * sizeof(float);
  const int ntiles = tiles_of(L, reduce ? 1 : 0);
  const size_t n_ws = (size_t)B * nh * ntiles * sizeof(float);
  if (head_sums) {
    UCHECK_ARG(ws != nullptr, "attn_grad: head_sums needs a workspace (uniter_attn_grad_ws_bytes)");
    UCHECK_ARG(ws_bytes >= n_ws, "attn_grad: workspace too small (%zu < %zu)", ws_bytes, n_ws);
  }
  const void* outs[3] = {out, head_sums, head_sums ? ws : nullptr};
  const size_t n_outs[3] = {n_out, n_hs, n_ws};
  for (int o = 0; o < 3; ++o) {
    UCHECK_ARG(!overlap(outs[o], n_outs[o], qkv, n_qkv) && !overlap(outs[o], n_outs[o], dctx, n_dctx) && !overlap(outs[o], n_outs[o], mk, n_mask),
               "attn_grad: an output overlaps an input");
    for (int p = o + 1; p < 3; ++p) UCHECK_ARG(!overlap(outs[o], n_outs[o], outs[p], n_outs[p]), "attn_grad: outputs overlap");
  }
  GradArgs a = {};
  a.qkv = qkv; a.mask = attn_mask; a.cu = cu_seqlens; a.dctx = dctx; a.slab_stride = slab_stride; a.out = out;
  a.part = head_sums ? (float*)ws : nullptr;
  a.B = B; a.L = L; a.nh = nh; a.reduce = reduce ? 1 : 0; a.n_slabs = n_slabs; a.ntiles = ntiles;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ntiles, reduce ? 1 : nh, B);
  if (reduce) {
    if (qkv_is_bf16) hipLaunchKernelGGL((attn_grad_kernel<true, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_grad_kernel<false, 1>), grid, dim3(256), 0, st, a);
  } else {
    if (qkv_is_bf16) hipLaunchKernelGGL((attn_grad_kernel<true, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_grad_kernel<false, 4>), grid, dim3(256), 0, st, a);
  }
  UCHECK_LAUNCH();
  if (head_sums) {
    const int count = B * nh;
    UCHECK_SHAPE((size_t)B * nh <= 0x7fffffffu, "attn_grad: B nh too large");
    hipLaunchKernelGGL(head_sums_kernel, dim3((count + 255) / 256), dim3(256), 0, st, (const float*)ws, head_sums, count, ntiles);
    UCHECK_LAUNCH();
  }
  return 0;
}

extern "C" int uniter_attn_relevance(const float* maps, float* out, float* tmp, int nl, int B, int L, void* stream) {
  UCHECK_ARG(maps && out && (tmp || nl == 1), "attn_relevance: null pointer");
  UCHECK_SHAPE(nl >= 1 && B >= 1 && L >= 1 && B <= 65535, "attn_relevance: bad shape nl %d B %d L %d", nl, B, L);
  const size_t one = (size_t)B * L * L * sizeof(float);
  UCHECK_ARG(!overlap(maps, one * nl, out, one) && !overlap(maps, one * nl, tmp, one) && !overlap(out, one, tmp, one),
             "attn_relevance: maps, out and tmp must not overlap");
  hipStream_t st = (hipStream_t)stream;
  // the product of layer l lands in out when nl - 1 - l is even, so that the last one does
  auto dst = [&](int l) { return (nl - 1 - l) % 2 == 0 ? out : tmp; };
  const size_t LL = (size_t)L * L;
  UCHECK_SHAPE((LL + 255) / 256 <= 0x7fffffffu, "attn_relevance: L %d too long", L);
  hipLaunchKernelGGL(relevance_first_kernel, dim3((unsigned)((LL + 255) / 256), B), dim3(256), 0, st, maps, dst(0), L);
  UCHECK_LAUNCH();
  const dim3 grid((L + RT - 1) / RT, (L + RT - 1) / RT, B);
  for (int l = 1; l < nl; ++l) {
    hipLaunchKernelGGL(relevance_step_kernel, grid, dim3(256), 0, st, maps + (size_t)l * B * LL, (const float*)dst(l - 1), dst(l), L);
    UCHECK_LAUNCH();
  }
  return 0;
}
