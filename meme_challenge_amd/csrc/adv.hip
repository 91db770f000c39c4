// VILLA's pieces between the encoder's passes (the FreeLB ones are uniter_bce_logits in head.hip and uniter_adv_delta_step in
// input_grads.hip):
//   uniter_bce_kl_logits        loss of a perturbed pass = BCE + kl_weight * symmetric KL to the clean prediction, and its gradient
//                               with respect to the perturbed logits, ONE launch
//   uniter_adv_delta_step_linf  delta <- clamp(delta + step * g / max|g|, -max_norm, +max_norm) per sample
// No float atomics: every result is a function of the inputs alone, every output element has one writer and is overwritten.
#include "common.h"

namespace {

// single workgroup, bce_logits_kernel's decomposition (head.hip) and, statement for statement, its arithmetic for the BCE part: with
// klw = 0 the total, the probabilities and the gradient are that kernel's bits.  With z the perturbed logit, c the clean one,
// q = sigmoid(z), p = sigmoid(c):  KL(p||q) + KL(q||p) = (p - q)(c - z)  (the logarithms of the two divergences combine to the
// logit difference), d/dz = (q - p) + q (1 - q)(z - c).  Both vanish exactly where z == c: p and q are then one expression of one
// value.  q (1 - q) is formed as e / (1 + e)^2 with e = exp(-|z|), which keeps its relative accuracy where fp32 q rounds to 1.
__global__ __launch_bounds__(256) void bce_kl_logits_kernel(const float* __restrict__ logits, const float* __restrict__ clean,
                                                            const int64_t* __restrict__ labels, float pw, float klw,
                                                            float* __restrict__ terms, float* __restrict__ probs,
                                                            float* __restrict__ dlogits, float gscale, int B) {
  __shared__ float red[4][2];
  float acc = 0.f, kacc = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float x = logits[b];
    const float c = clean[b];
    const float y = (float)labels[b];
    const float lw = 1.0f + (pw - 1.0f) * y;
    const float sp = log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f);     // softplus(-x)
    acc += (1.0f - y) * x + lw * sp;
    const float sg = 1.0f / (1.0f + expf(-x));
    const float sc = 1.0f / (1.0f + expf(-c));
    kacc += (sc - sg) * (c - x);
    if (probs) probs[b] = sg;
    if (dlogits) {
      const float e = expf(-fabsf(x));
      const float qq = e / ((1.0f + e) * (1.0f + e));               // q (1 - q)
      const float kg = (sg - sc) + qq * (x - c);
      dlogits[b] = (((1.0f - y) - lw * (1.0f - sg)) + klw * kg) * (gscale / (float)B);
    }
  }
  acc = wave_sum(acc);
  kacc = wave_sum(kacc);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = acc; red[threadIdx.x >> 6][1] = kacc; }
  __syncthreads();
  if (threadIdx.x == 0 && terms) {
    const float bce = (red[0][0] + red[1][0] + red[2][0] + red[3][0]) / (float)B;
    const float kl = (red[0][1] + red[1][1] + red[2][1] + red[3][1]) / (float)B;
    terms[0] = bce + klw * kl;
    terms[1] = bce;
    terms[2] = kl;
  }
}

// ---- uniter_adv_delta_step_linf ----
constexpr int LINF_CHUNK = 4096;     // floats of a sample one workgroup owns (uniter_adv_delta_step's chunk): 256 threads x 4 x 16 bytes

// grid (P, B): part[b][p] = max |g| over the chunk (exact, so any order gives the same bits)
__global__ __launch_bounds__(256) void linf_partials_kernel(const float* __restrict__ grad, float* __restrict__ part, int n4) {
  __shared__ float red[4];
  const int p = blockIdx.x, b = blockIdx.y, P = gridDim.x;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(grad) + (size_t)b * n4;
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < LINF_CHUNK / 1024; ++j) {
    const int i = p * (LINF_CHUNK / 4) + j * 256 + (int)threadIdx.x;
    if (i < n4) {
      const f32x4 gv = g4[i];
      m = fmaxf(fmaxf(m, fabsf(gv[0])), fmaxf(fabsf(gv[1]), fmaxf(fabsf(gv[2]), fabsf(gv[3]))));
    }
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)b * P + p] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// grid (P, B), behind linf_partials_kernel: every thread folds the sample's P partials in ascending order, forms the fp32 factor
// a = step / max|g| (0 where the gradient vanishes) and updates its elements of the chunk.  Without a step nothing is added (not even
// 0 * g), and the clamp is a pair of comparisons that hands an element inside the ball back as it is: a sample that neither steps
// nor clamps keeps its bits.
__global__ __launch_bounds__(256) void linf_update_kernel(float* __restrict__ delta, const float* __restrict__ grad,
                                                          const float* __restrict__ part, int n4, float step_size, float max_norm) {
  const int p = blockIdx.x, b = blockIdx.y, P = gridDim.x;
  const float* pp = part + (size_t)b * P;
  float gm = 0.f;
  for (int q = 0; q < P; ++q) gm = fmaxf(gm, pp[q]);               // (P: uniform)
  const float af = gm > 0.f ? step_size / gm : 0.f;
  const bool clamp = max_norm > 0.f;
  if (af == 0.f && !clamp) return;                                  // (uniform)
  f32x4* d4 = reinterpret_cast<f32x4*>(delta) + (size_t)b * n4;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(grad) + (size_t)b * n4;
#pragma unroll
  for (int j = 0; j < LINF_CHUNK / 1024; ++j) {
    const int i = p * (LINF_CHUNK / 4) + j * 256 + (int)threadIdx.x;
    if (i < n4) {
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
    }
  }
}

inline int linf_parts(int n) { return (n + LINF_CHUNK - 1) / LINF_CHUNK; }

}  // namespace

extern "C" int uniter_bce_kl_logits(const float* logits, const float* clean_logits, const int64_t* labels, float pos_weight,
                                    float kl_weight, float* terms, float* probs, float* dlogits, float grad_scale, int B,
                                    void* stream) {
  UCHECK_ARG(logits && clean_logits && labels && B > 0, "bce_kl_logits: bad argument");
  UCHECK_ARG(kl_weight == kl_weight, "bce_kl_logits: kl_weight is NaN");
  hipLaunchKernelGGL(bce_kl_logits_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, clean_logits, labels, pos_weight,
                     kl_weight, terms, probs, dlogits, grad_scale, B);
  UCHECK_LAUNCH();
  return 0;
}

extern "C" size_t uniter_adv_delta_linf_ws_bytes(int B, int n) {
  if (B <= 0 || n <= 0) return 0;
  return align_up((size_t)B * linf_parts(n) * sizeof(float), 8);
}

extern "C" int uniter_adv_delta_step_linf(float* delta, const float* grad, int B, int n, float step_size, float max_norm, void* ws,
                                          void* stream) {
  UCHECK_ARG(delta && grad && ws, "adv_delta_step_linf: null pointer");
  UCHECK_ARG((((uintptr_t)delta | (uintptr_t)grad) & 15) == 0 && ((uintptr_t)ws & 7) == 0,
             "adv_delta_step_linf: delta and grad must be 16-byte aligned, the workspace 8-byte");
  UCHECK_ARG(step_size == step_size && max_norm == max_norm, "adv_delta_step_linf: step_size / max_norm is NaN");
  UCHECK_SHAPE(B >= 0 && n >= 0 && n % 4 == 0, "adv_delta_step_linf: n must be a multiple of 4 (got %d)", n);
  UCHECK_SHAPE(B <= 65535, "adv_delta_step_linf: at most 65535 samples (got %d)", B);
  if (B == 0 || n == 0) return 0;
  const dim3 grid(linf_parts(n), B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(linf_partials_kernel, grid, dim3(256), 0, st, grad, (float*)ws, n / 4);
  UCHECK_LAUNCH();
  hipLaunchKernelGGL(linf_update_kernel, grid, dim3(256), 0, st, delta, grad, (const float*)ws, n / 4, step_size, max_norm);
  UCHECK_LAUNCH();
  return 0;
}
