// The ascent step of an adversarial perturbation (FreeLB, VILLA) between the encoder's passes, per sample, in both norms:
//   uniter_adv_delta_step       delta <- project(delta + step * g / |g|) onto the L2 ball of radius max_norm
//   uniter_adv_delta_step_linf  delta <- clamp(delta + step * g / max|g|, -max_norm, +max_norm)
// Both are two launches on one grid (partials per chunk of a sample, then the update) behind ONE launcher, delta_step_run: the
// argument checks, the grid and the launches are stated once, the norm chooses the kernels.  (The losses of the passes are
// uniter_bce_logits / uniter_bce_kl_logits in head.hip.)
// No float atomics: every result is a function of the inputs alone, every output element has one writer and is overwritten.
#include "common.h"

namespace {

constexpr int ADV_CHUNK = 4096;      // floats of a sample one workgroup owns: 256 threads x 4 x 16 bytes

// grid (P, B): body(i) for every 16-byte element i of sample blockIdx.y that workgroup blockIdx.x's chunk holds and this thread owns
template <class F>
__device__ __forceinline__ void chunk_walk(int n4, F&& body) {
#pragma unroll
  for (int j = 0; j < ADV_CHUNK / 1024; ++j) {
    const int i = blockIdx.x * (ADV_CHUNK / 4) + j * 256 + (int)threadIdx.x;
    if (i < n4) body(i);
  }
}

// sum of a double over the workgroup in a fixed order: lanes by the shuffle tree, then the four waves in ascending index
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- L2 ----
// part[b][p] = {g.g, delta.g, delta.delta} over the chunk, in double (a product of two floats is exact there)
__global__ __launch_bounds__(256) void adv_partials_kernel(const float* __restrict__ delta, const float* __restrict__ grad,
                                                           double* __restrict__ part, int n4) {
  __shared__ double red[4][3];
  const int p = blockIdx.x, b = blockIdx.y, P = gridDim.x;
  const f32x4* d4 = reinterpret_cast<const f32x4*>(delta) + (size_t)b * n4;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(grad) + (size_t)b * n4;
  double gg = 0.0, dg = 0.0, dd = 0.0;
  chunk_walk(n4, [&](int i) {
    const f32x4 dv = d4[i], gv = g4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double x = (double)dv[e], y = (double)gv[e];
      gg += y * y; dg += x * y; dd += x * x;
    }
  });
  gg = wave_sum_f64(gg); dg = wave_sum_f64(dg); dd = wave_sum_f64(dd);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = gg; red[wave][1] = dg; red[wave][2] = dd; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    part[((size_t)b * P + p) * 3 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// behind adv_partials_kernel: every thread folds the sample's P partials in ascending order (the same value in every thread and
// workgroup), forms the step and the projection's factor from them, and updates its elements of the chunk:
//   a = step / |g|;  |delta + a g|^2 = dd + 2 a dg + a^2 gg;  delta <- (delta + a g) * min(1, max_norm / |delta + a g|)
__global__ __launch_bounds__(256) void adv_update_kernel(float* __restrict__ delta, const float* __restrict__ grad,
                                                         const double* __restrict__ part, int n4, float step_size, float max_norm) {
  const int b = blockIdx.y, P = gridDim.x;
  const double* pp = part + (size_t)b * P * 3;
  double gg = 0.0, dg = 0.0, dd = 0.0;
  for (int q = 0; q < P; ++q) { gg += pp[3 * q]; dg += pp[3 * q + 1]; dd += pp[3 * q + 2]; }       // (P: uniform)
  const double a = gg > 0.0 ? (double)step_size / sqrt(gg) : 0.0;
  const float af = (float)a;
  const double ad = (double)af;                                   // (the factor the elements are stepped with)
  double n2 = dd + 2.0 * ad * dg + ad * ad * gg;
  n2 = n2 > 0.0 ? n2 : 0.0;
  const double nrm = sqrt(n2);
  const float sf = (max_norm > 0.f && nrm > (double)max_norm) ? (float)((double)max_norm / nrm) : 1.0f;
  if (af == 0.f && sf == 1.0f) return;                            // (uniform: the sample keeps its bits)
  f32x4* d4 = reinterpret_cast<f32x4*>(delta) + (size_t)b * n4;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(grad) + (size_t)b * n4;
  chunk_walk(n4, [&](int i) {
    f32x4 dv = d4[i];
    const f32x4 gv = g4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) dv[e] = (dv[e] + af * gv[e]) * sf;
    d4[i] = dv;
  });
}

// ---- L-infinity ----
// part[b][p] = max |g| over the chunk (exact, so any order gives the same bits)
__global__ __launch_bounds__(256) void linf_partials_kernel(const float* __restrict__ grad, float* __restrict__ part, int n4) {
  __shared__ float red[4];
  const int p = blockIdx.x, b = blockIdx.y, P = gridDim.x;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(grad) + (size_t)b * n4;
  float m = 0.f;
  chunk_walk(n4, [&](int i) {
    const f32x4 gv = g4[i];
    m = fmaxf(fmaxf(m, fabsf(gv[0])), fmaxf(fabsf(gv[1]), fmaxf(fabsf(gv[2]), fabsf(gv[3]))));
  });
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)b * P + p] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// behind linf_partials_kernel: every thread folds the sample's P partials in ascending order, forms the fp32 factor
// a = step / max|g| (0 where the gradient vanishes) and updates its elements of the chunk.  Without a step nothing is added (not even
// 0 * g), and the clamp is a pair of comparisons that hands an element inside the ball back as it is: a sample that neither steps
// nor clamps keeps its bits.
__global__ __launch_bounds__(256) void linf_update_kernel(float* __restrict__ delta, const float* __restrict__ grad,
                                                          const float* __restrict__ part, int n4, float step_size, float max_norm) {
  const int b = blockIdx.y, P = gridDim.x;
  const float* pp = part + (size_t)b * P;
  float gm = 0.f;
  for (int q = 0; q < P; ++q) gm = fmaxf(gm, pp[q]);               // (P: uniform)
  const float af = gm > 0.f ? step_size / gm : 0.f;
  const bool clamp = max_norm > 0.f;
  if (af == 0.f && !clamp) return;                                  // (uniform)
  f32x4* d4 = reinterpret_cast<f32x4*>(delta) + (size_t)b * n4;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(grad) + (size_t)b * n4;
  chunk_walk(n4, [&](int i) {
    f32x4 dv = d4[i];
    if (af != 0.f) {
      const f32x4 gv = g4[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) dv[e] = dv[e] + af * gv[e];
    }
    if (clamp) {
#pragma unroll
      for (int e = 0; e < 4; ++e) dv[e] = dv[e] > max_norm ? max_norm : (dv[e] < -max_norm ? -max_norm : dv[e]);
    }
    d4[i] = dv;
  });
}

inline int adv_parts(int n) { return (n + ADV_CHUNK - 1) / ADV_CHUNK; }

// both entry points: `linf` chooses the pair of kernels (and what the workspace holds), `who` opens every message
int delta_step_run(bool linf, const char* who, float* delta, const float* grad, int B, int n, float step_size, float max_norm, void* ws,
                   void* stream) {
  UCHECK_ARG(delta && grad && ws, "%s: null pointer", who);
  UCHECK_ARG((((uintptr_t)delta | (uintptr_t)grad) & 15) == 0 && ((uintptr_t)ws & 7) == 0,
             "%s: delta and grad must be 16-byte aligned, the workspace 8-byte", who);
  UCHECK_ARG(step_size == step_size && max_norm == max_norm, "%s: step_size / max_norm is NaN", who);
  UCHECK_SHAPE(B >= 0 && n >= 0 && n % 4 == 0, "%s: n must be a multiple of 4 (got %d)", who, n);
  UCHECK_SHAPE(B <= 65535, "%s: at most 65535 samples (got %d)", who, B);
  if (B == 0 || n == 0) return 0;
  const dim3 grid(adv_parts(n), B);
  hipStream_t st = (hipStream_t)stream;
  if (linf) hipLaunchKernelGGL(linf_partials_kernel, grid, dim3(256), 0, st, grad, (float*)ws, n / 4);
  else hipLaunchKernelGGL(adv_partials_kernel, grid, dim3(256), 0, st, delta, grad, (double*)ws, n / 4);
  UCHECK_LAUNCH();
  if (linf) hipLaunchKernelGGL(linf_update_kernel, grid, dim3(256), 0, st, delta, grad, (const float*)ws, n / 4, step_size, max_norm);
  else hipLaunchKernelGGL(adv_update_kernel, grid, dim3(256), 0, st, delta, grad, (const double*)ws, n / 4, step_size, max_norm);
  UCHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t uniter_adv_delta_ws_bytes(int B, int n) {
  if (B <= 0 || n <= 0) return 0;
  return (size_t)B * adv_parts(n) * 3 * sizeof(double);
}

extern "C" size_t uniter_adv_delta_linf_ws_bytes(int B, int n) {
  if (B <= 0 || n <= 0) return 0;
  return align_up((size_t)B * adv_parts(n) * sizeof(float), 8);
}

extern "C" int uniter_adv_delta_step(float* delta, const float* grad, int B, int n, float step_size, float max_norm, void* ws,
                                     void* stream) {
  return delta_step_run(false, "adv_delta_step", delta, grad, B, n, step_size, max_norm, ws, stream);
}

extern "C" int uniter_adv_delta_step_linf(float* delta, const float* grad, int B, int n, float step_size, float max_norm, void* ws,
                                          void* stream) {
  return delta_step_run(true, "adv_delta_step_linf", delta, grad, B, n, step_size, max_norm, ws, stream);
}
