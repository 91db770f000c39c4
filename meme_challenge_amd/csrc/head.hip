// Pooler + classification head + loss.
//
// Replaces BertPooler.forward (model/layer.py:179-185: h[:,0] -> dense -> tanh),
// MemeUniter.linear (model/meme_uniter.py:19-20), nn.BCEWithLogitsLoss(pos_weight)
// (train_template.py:65,98-99) and their autograd.  B is small (16): these are
// latency-bound VALU kernels, one wave per output row of the weight.
#include "common.h"

namespace {

// pooled[b][n] = tanh(sum_k h0[b][k] W[n][k] + bias[n]); one wave per (n, group of 4 batch rows):
// the weight row is read once per wave and the four dot products reduce together
__global__ __launch_bounds__(256) void pooler_fwd_kernel(const float* __restrict__ hidden,
                                                         const float* __restrict__ W,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ pooled, int B, int L, int H) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b0 = blockIdx.y * 4;
  if (n >= H) return;
  const float* w = W + (size_t)n * H;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if ((H & 3) == 0) {        // 16-byte loads: 3 iterations instead of 12 at H = 768 (the kernel is a chain of load latencies)
    const int H4 = H >> 2;
    for (int k4 = lane; k4 < H4; k4 += 64) {
      const f32x4 wk = reinterpret_cast<const f32x4*>(w)[k4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (b0 + j < B) {
          const f32x4 x = reinterpret_cast<const f32x4*>(hidden + (size_t)(b0 + j) * L * H)[k4];
          s[j] += (x[0] * wk[0] + x[1] * wk[1]) + (x[2] * wk[2] + x[3] * wk[3]);
        }
    }
  } else {
    for (int k = lane; k < H; k += 64) {
      const float wk = w[k];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (b0 + j < B) s[j] += hidden[(size_t)(b0 + j) * L * H + k] * wk;
    }
  }
  const float bn = bias[n];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float t = wave_sum(s[j]);
    if (lane == 0 && b0 + j < B) pooled[(size_t)(b0 + j) * H + n] = tanhf(t + bn);
  }
}

// one wave per n: dbias[n] += sum_b dpre[b][n]; dW[n][:] += sum_b dpre[b][n] * h0[b][:]
// dpre[b][n] lives in lane b (chunks of 64 batch rows) and is broadcast by shuffles
__global__ __launch_bounds__(256) void pooler_bwd_w_kernel(const float* __restrict__ dpooled,
                                                           const float* __restrict__ pooled,
                                                           const float* __restrict__ hidden,
                                                           float* __restrict__ dW, float* __restrict__ dbias,
                                                           int B, int L, int H) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= H) return;
  float sb = 0.f;
  for (int bc = 0; bc < B; bc += 64) {
    const int nb = min(64, B - bc);
    float dpre = 0.f;
    if (lane < nb) {
      const float p = pooled[(size_t)(bc + lane) * H + n];
      dpre = dpooled[(size_t)(bc + lane) * H + n] * (1.0f - p * p);
    }
    sb += wave_sum(dpre);
    // (the loops' trip counts are wave-uniform: the shuffles below read lanes that a per-lane bound would have switched off --
    // H / 4 < 64 with more batch rows than that)
    if ((H & 3) == 0) {
      const int H4 = H >> 2;
      for (int k0 = 0; k0 < H4; k0 += 64) {
        const int k4 = k0 + lane;
        const bool on = k4 < H4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < nb; ++b) {
          const float d = __shfl(dpre, b, 64);
          if (on) {
            const f32x4 x = reinterpret_cast<const f32x4*>(hidden + (size_t)(bc + b) * L * H)[k4];
            acc[0] += d * x[0]; acc[1] += d * x[1]; acc[2] += d * x[2]; acc[3] += d * x[3];
          }
        }
        if (on) {
          f32x4* o = reinterpret_cast<f32x4*>(dW + (size_t)n * H) + k4;
          f32x4 t = *o;
          t[0] += acc[0]; t[1] += acc[1]; t[2] += acc[2]; t[3] += acc[3];
          *o = t;
        }
      }
    } else {
      for (int k0 = 0; k0 < H; k0 += 64) {
        const int k = k0 + lane;
        float s = 0.f;
        for (int b = 0; b < nb; ++b) {
          const float d = __shfl(dpre, b, 64);
          if (k < H) s += d * hidden[(size_t)(bc + b) * L * H + k];
        }
        if (k < H) dW[(size_t)n * H + k] += s;
      }
    }
  }
  if (lane == 0) dbias[n] += sb;
}

// dh0[b][k] (+)= sum_n dpre[b][n] W[n][k]: workgroup = (64 columns k, one b); its 4 waves split n
// 16 waves (was 4): the loop over n is a chain of dependent load latencies, 48 iterations instead of 192 at H = 768
constexpr int PBX_WAVES = 16;
__global__ __launch_bounds__(64 * PBX_WAVES) void pooler_bwd_x_kernel(const float* __restrict__ dpooled,
                                                           const float* __restrict__ pooled,
                                                           const float* __restrict__ W,
                                                           float* __restrict__ dhidden, int B, int L, int H,
                                                           int beta) {
  __shared__ float red[PBX_WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  const int b = blockIdx.y;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (k < H) {
    const float* dp = dpooled + (size_t)b * H;
    const float* pp = pooled + (size_t)b * H;
    constexpr int S = PBX_WAVES;
    int n = wv;
    for (; n + 3 * S < H; n += 4 * S) {
      const float p0 = pp[n], p1 = pp[n + S], p2 = pp[n + 2 * S], p3 = pp[n + 3 * S];
      s0 += dp[n] * (1.0f - p0 * p0) * W[(size_t)n * H + k];
      s1 += dp[n + S] * (1.0f - p1 * p1) * W[(size_t)(n + S) * H + k];
      s2 += dp[n + 2 * S] * (1.0f - p2 * p2) * W[(size_t)(n + 2 * S) * H + k];
      s3 += dp[n + 3 * S] * (1.0f - p3 * p3) * W[(size_t)(n + 3 * S) * H + k];
    }
    for (; n < H; n += S) {
      const float p0 = pp[n];
      s0 += dp[n] * (1.0f - p0 * p0) * W[(size_t)n * H + k];
    }
  }
  red[wv][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (wv == 0 && k < H) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < PBX_WAVES; ++w) s += red[w][lane];
    float* d = dhidden + (size_t)b * L * H + k;
    *d = beta ? *d + s : s;
  }
}

// y[b][c] = x[b] . W[c] + bias[c]; one wave per (b,c)
__global__ __launch_bounds__(256) void linear_small_fwd_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ W,
                                                               const float* __restrict__ bias,
                                                               float* __restrict__ y, int B, int H, int Cn) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= B * Cn) return;
  const int b = o / Cn, c = o - b * Cn;
  float s = 0.f;
  for (int k = lane; k < H; k += 64) s += x[(size_t)b * H + k] * W[(size_t)c * H + k];
  s = wave_sum(s);
  if (lane == 0) y[o] = s + bias[c];
}

// thread per k: dx[b][k] = sum_c dy[b][c] W[c][k] (all b);  dW[c][k] += sum_b dy[b][c] x[b][k];
// thread k < Cn additionally: db[k] += sum_b dy[b][k]
__global__ __launch_bounds__(256) void linear_small_bwd_kernel(const float* __restrict__ dy,
                                                               const float* __restrict__ x,
                                                               const float* __restrict__ W,
                                                               float* __restrict__ dx, float* __restrict__ dW,
                                                               float* __restrict__ db, int B, int H, int Cn) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < Cn && db) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dy[(size_t)b * Cn + k];
    db[k] += s;
  }
  if (k >= H) return;
  for (int b = 0; b < B && dx; ++b) {
    float s = 0.f;
    for (int c = 0; c < Cn; ++c) s += dy[(size_t)b * Cn + c] * W[(size_t)c * H + k];
    dx[(size_t)b * H + k] = s;
  }
  for (int c = 0; c < Cn && dW; ++c) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dy[(size_t)b * Cn + c] * x[(size_t)b * H + k];
    dW[(size_t)c * H + k] += s;
  }
}

// One element of the BCE sum, the arithmetic every logits loss below shares (the library is built without contraction, so one
// expression is one sequence of roundings wherever it is inlined): its term of the sum, sigmoid(x), and d term / dx
struct BceElem { float term, sg, dterm; };
__device__ __forceinline__ BceElem bce_elem(float x, float y, float pw) {
  const float lw = 1.0f + (pw - 1.0f) * y;
  const float sp = log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f);     // softplus(-x)
  const float sg = 1.0f / (1.0f + expf(-x));
  return {(1.0f - y) * x + lw * sp, sg, (1.0f - y) - lw * (1.0f - sg)};
}

// The logits loss, single workgroup: loss = mean_b [ (1-y) x + (1 + (pw-1) y) softplus(-x) ], and with KL the symmetric divergence to
// the clean prediction on top (a perturbed pass of VILLA).  One body for both kernels; without KL none of the KL arithmetic exists,
// and the BCE statements are the same ones in the same order either way, so with klw = 0 the total, the probabilities and the
// gradient of the KL kernel are the plain kernel's bits.  With z the perturbed logit, c the clean one, q = sigmoid(z),
// p = sigmoid(c):  KL(p||q) + KL(q||p) = (p - q)(c - z)  (the logarithms of the two divergences combine to the logit difference),
// d/dz = (q - p) + q (1 - q)(z - c).  Both vanish exactly where z == c: p and q are then one expression of one value.  q (1 - q) is
// formed as e / (1 + e)^2 with e = exp(-|z|), which keeps its relative accuracy where fp32 q rounds to 1.
// out: the loss, or with KL the terms [total, bce, kl].
template <bool KL>
__device__ __forceinline__ void bce_logits_body(const float* __restrict__ logits, const float* __restrict__ clean,
                                                const int64_t* __restrict__ labels, float pw, float klw, float* __restrict__ out,
                                                float* __restrict__ probs, float* __restrict__ dlogits, float gscale, int B) {
  __shared__ float red[4][KL ? 2 : 1];
  float acc = 0.f, kacc = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float x = logits[b];
    float c = 0.f;
    if constexpr (KL) c = clean[b];
    const BceElem el = bce_elem(x, (float)labels[b], pw);
    acc += el.term;
    const float sg = el.sg;
    if constexpr (KL) {
      const float sc = 1.0f / (1.0f + expf(-c));
      kacc += (sc - sg) * (c - x);
      if (probs) probs[b] = sg;
      if (dlogits) {
        const float e = expf(-fabsf(x));
        const float qq = e / ((1.0f + e) * (1.0f + e));               // q (1 - q)
        const float kg = (sg - sc) + qq * (x - c);
        dlogits[b] = (el.dterm + klw * kg) * (gscale / (float)B);
      }
    } else {
      if (probs) probs[b] = sg;
      if (dlogits) dlogits[b] = el.dterm * (gscale / (float)B);
    }
  }
  acc = wave_sum(acc);
  if constexpr (KL) kacc = wave_sum(kacc);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = acc;
    if constexpr (KL) red[threadIdx.x >> 6][1] = kacc;
  }
  __syncthreads();
  if (threadIdx.x == 0 && out) {
    const float bce = (red[0][0] + red[1][0] + red[2][0] + red[3][0]) / (float)B;
    if constexpr (KL) {
      const float kl = (red[0][1] + red[1][1] + red[2][1] + red[3][1]) / (float)B;
      out[0] = bce + klw * kl;
      out[1] = bce;
      out[2] = kl;
    } else {
      *out = bce;
    }
  }
}

// (the two instantiations under the kernel names every profile and trace of the step knows)
__global__ __launch_bounds__(256) void bce_logits_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ labels, float pw,
                                                         float* __restrict__ loss, float* __restrict__ probs,
                                                         float* __restrict__ dlogits, float gscale, int B) {
  bce_logits_body<false>(logits, nullptr, labels, pw, 0.f, loss, probs, dlogits, gscale, B);
}

__global__ __launch_bounds__(256) void bce_kl_logits_kernel(const float* __restrict__ logits, const float* __restrict__ clean,
                                                            const int64_t* __restrict__ labels, float pw, float klw,
                                                            float* __restrict__ terms, float* __restrict__ probs,
                                                            float* __restrict__ dlogits, float gscale, int B) {
  bce_logits_body<true>(logits, clean, labels, pw, klw, terms, probs, dlogits, gscale, B);
}

// ---- BCE + a pairwise AUROC surrogate over (batch) x (batch U bank of recent scores), and the bank's push: one launch ----------
// (contract: include/uniter_hip.h, uniter_bce_auc_logits).  One workgroup, in three stretches:
//   1. thread per element: the BCE element (bce_elem: uniter_bce_logits' statements in its order, so its bits), and the scores
//      and classes (1 positive, 0 negative, 2 takes no part) of the batch rows and of every bank slot into LDS -- a slot outside
//      the `fill` most recent ones is class 2 whatever it holds;
//   2. behind the barrier every read of the bank is done: the push (slots are distinct, N >= B) and the two state words;
//   3. wave per batch row (rows strided over the 4 waves), the row's opposite class strided over the 64 lanes.  A positive row
//      sums loss and slope over every negative (batch and bank); a negative row the slope over every positive and the loss over
//      the BANK's positives only -- its pairs with batch positives were counted from their side.  wave_sum's butterfly, the
//      serial sum over a wave's rows and the four waves' partial sums in index order: a fixed order.
// The surrogate's value and slope at d = s_positive - s_negative:
template <int KIND>
__device__ __forceinline__ void auc_pair(float d, float margin, float& l, float& dl) {
  if constexpr (KIND == 0) {            // softplus(-d), -sigmoid(-d): e <= 1 in both branches, nothing cancels
    const float e = expf(-fabsf(d));
    l = fmaxf(-d, 0.f) + log1pf(e);
    dl = -((d >= 0.f ? e : 1.0f) / (1.0f + e));
  } else {                              // max(0, margin - d)^2, exactly 0 (and flat) from d = margin on
    const float h = fmaxf(margin - d, 0.f);
    l = h * h;
    dl = -2.0f * h;
  }
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int AUC_MAX_B = 4096, AUC_MAX_N = 8192;       // (B + N) * 5 bytes of LDS: 60 KB at the limits

template <int KIND>
__global__ __launch_bounds__(256) void bce_auc_logits_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                             float pw, float aw, float margin, float* bank_scores,
                                                             int32_t* bank_labels, int32_t* bank_state, int N, int push,
                                                             float* __restrict__ terms, int32_t* __restrict__ n_pairs,
                                                             float* __restrict__ probs, float* __restrict__ dlogits, float gscale,
                                                             int B) {
  extern __shared__ float auc_lds[];
  __shared__ float red[4][2];
  __shared__ int cnt[4][4];
  const int M = B + N;
  float* sc = auc_lds;                                                   // [M] scores: the batch rows, then the bank's slots
  unsigned char* cls = reinterpret_cast<unsigned char*>(auc_lds + M);    // [M] classes
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool grad_pairs = dlogits != nullptr && aw != 0.f;               // else stretch 1 writes dlogits, as uniter_bce_logits does
  int head = 0, fill = 0;
  if (N > 0) {                                                           // (clamped for memory safety only)
    head = min(max(bank_state[0], 0), N - 1);
    fill = min(max(bank_state[1], 0), N);
  }
  float acc = 0.f;
  int nsp = 0, nsn = 0, nkp = 0, nkn = 0;
  for (int b = tid; b < B; b += 256) {
    const float x = logits[b];
    const int64_t lab = labels[b];
    const BceElem el = bce_elem(x, (float)lab, pw);
    acc += el.term;
    if (probs) probs[b] = el.sg;
    if (dlogits && !grad_pairs) dlogits[b] = el.dterm * (gscale / (float)B);
    const int c = lab == 1 ? 1 : (lab == 0 ? 0 : 2);
    sc[b] = x;
    cls[b] = (unsigned char)c;
    nsp += c == 1;
    nsn += c == 0;
  }
  for (int s = tid; s < N; s += 256) {
    int age = head - 1 - s;                                              // 0: the slot pushed last
    if (age < 0) age += N;
    const int32_t bl = bank_labels[s];
    const int c = age < fill ? (bl == 1 ? 1 : (bl == 0 ? 0 : 2)) : 2;
    sc[B + s] = bank_scores[s];
    cls[B + s] = (unsigned char)c;
    nkp += c == 1;
    nkn += c == 0;
  }
  acc = wave_sum(acc);
  nsp = wave_sum_int(nsp), nsn = wave_sum_int(nsn), nkp = wave_sum_int(nkp), nkn = wave_sum_int(nkn);
  if (lane == 0) {
    red[wv][0] = acc;
    cnt[wv][0] = nsp, cnt[wv][1] = nsn, cnt[wv][2] = nkp, cnt[wv][3] = nkn;
  }
  __syncthreads();
  if (push && N > 0) {
    for (int r = tid; r < B; r += 256) {
      int s = head + r;
      if (s >= N) s -= N;
      bank_scores[s] = sc[r];
      bank_labels[s] = (int32_t)labels[r];
    }
    if (tid == 0) {
      int h = head + B;
      if (h >= N) h -= N;
      bank_state[0] = h;
      bank_state[1] = min(fill + B, N);
    }
  }
  nsp = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
  nsn = cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
  nkp = cnt[0][2] + cnt[1][2] + cnt[2][2] + cnt[3][2];
  nkn = cnt[0][3] + cnt[1][3] + cnt[2][3] + cnt[3][3];
  const int n = nsp * (nsn + nkn) + nkp * nsn;                           // below AUC_MAX_B * (AUC_MAX_B + AUC_MAX_N) = 5.0e7
  const float inv_n = n > 0 ? 1.0f / (float)n : 0.f;
  float wl = 0.f;
  if (terms != nullptr || grad_pairs) {
    for (int b = wv; b < B; b += 4) {                                    // (b, c, z are wave-uniform: wave_sum sees every lane)
      const int c = cls[b];
      const float z = sc[b];
      float la = 0.f, ga = 0.f, l, dl;
      if (n > 0 && c == 1) {
        for (int j = lane; j < M; j += 64)
          if (cls[j] == 0) {
            auc_pair<KIND>(z - sc[j], margin, l, dl);
            la += l;
            ga += dl;
          }
      } else if (n > 0 && c == 0) {
        for (int j = lane; j < M; j += 64)
          if (cls[j] == 1) {
            auc_pair<KIND>(sc[j] - z, margin, l, dl);
            ga -= dl;
            if (j >= B) la += l;
          }
      }
      la = wave_sum(la);
      ga = wave_sum(ga);
      wl += la;
      if (grad_pairs && lane == 0) {
        const BceElem el = bce_elem(z, (float)labels[b], pw);
        dlogits[b] = el.dterm * (gscale / (float)B) + (gscale * aw) * (ga * inv_n);
      }
    }
  }
  if (lane == 0) red[wv][1] = wl;
  __syncthreads();
  if (tid == 0) {
    if (terms) {
      const float bce = (red[0][0] + red[1][0] + red[2][0] + red[3][0]) / (float)B;
      const float auc = (red[0][1] + red[1][1] + red[2][1] + red[3][1]) * inv_n;
      terms[0] = aw != 0.f ? bce + aw * auc : bce;
      terms[1] = bce;
      terms[2] = auc;
    }
    if (n_pairs) *n_pairs = n;
  }
}


// ---- round 6: pooler + classifier as ONE forward launch and ONE backward launch ------------------------------------------------
// Between the encoder's last LayerNorm and the backward pass's first one the step ran seven latency-sized launches (pooler, classifier,
// loss, classifier backward, a fill of the encoder output's gradient, pooler backward x 2: 67 us of a 9.1-ms step with nothing beside
// them, profiles/r06_timeline_f32x3.txt).  The loss stays the trainer's (train_template.py:98-99); the two modules of
// model/meme_uniter.py:19-21 become one launch each way.

// forward: pooler_fwd_kernel's waves, then the LAST workgroup to finish (a ticket counter) computes the logits from the pooled rows.
// The pooled values cross workgroups -- and XCDs, whose L2s are not coherent with each other inside a launch -- so they are stored and
// re-read device-coherently (sc1), the idiom of the balanced walk's partial sums (gemm_split3.hip).
__global__ __launch_bounds__(256) void pool_head_fwd_kernel(const float* __restrict__ hidden, const float* __restrict__ W,
                                                            const float* __restrict__ bias, const float* __restrict__ Wl,
                                                            const float* __restrict__ bl, float* __restrict__ pooled,
                                                            float* __restrict__ logits, unsigned* __restrict__ ticket, int B, int L,
                                                            int H, int Cn) {
  __shared__ unsigned last_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave;
  const int b0 = blockIdx.y * 4;
  if (n < H) {
    const float* w = W + (size_t)n * H;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if ((H & 3) == 0) {
      const int H4 = H >> 2;
      for (int k4 = lane; k4 < H4; k4 += 64) {
        const f32x4 wk = reinterpret_cast<const f32x4*>(w)[k4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (b0 + j < B) {
            const f32x4 x = reinterpret_cast<const f32x4*>(hidden + (size_t)(b0 + j) * L * H)[k4];
            s[j] += (x[0] * wk[0] + x[1] * wk[1]) + (x[2] * wk[2] + x[3] * wk[3]);
          }
      }
    } else {
      for (int k = lane; k < H; k += 64) {
        const float wk = w[k];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (b0 + j < B) s[j] += hidden[(size_t)(b0 + j) * L * H + k] * wk;
      }
    }
    const float bn = bias[n];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = wave_sum(s[j]);
      if (lane == 0 && b0 + j < B)
        __hip_atomic_store(pooled + (size_t)(b0 + j) * H + n, tanhf(t + bn), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's pooled values are in memory ...
  __syncthreads();                                        // ... and so are the other three waves'
  if (threadIdx.x == 0) {
    // Two levels of counters (16 groups 256 bytes apart, then one): 768 read-modify-writes of ONE address are served one after the other
    // (23 ns each: 18 us behind the pooler's own 10); 48 per group address in parallel, then 16.  Every counter is left zero.
    const unsigned total = gridDim.x * gridDim.y, id = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned g = id & 15u, gsize = (total + 15u - g) >> 4;          // workgroups whose id is g modulo 16
    unsigned* tg = ticket + g * 64u;
    unsigned last = 0u;
    if (__hip_atomic_fetch_add(tg, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1u) {
      __hip_atomic_store(tg, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unsigned* tt = ticket + 16u * 64u;
      if (__hip_atomic_fetch_add(tt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (total < 16u ? total : 16u) - 1u) {
        __hip_atomic_store(tt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = 1u;
      }
    }
    last_s = last;
  }
  __syncthreads();
  if (last_s == 0u) return;
  asm volatile("" ::: "memory");
  // logits[b][c] = pooled[b] . Wl[c] + bl[c]: one wave per (b, c), the accumulation order of linear_small_fwd_kernel.  The pooled rows
  // come through a buffer descriptor with the sc1 bit (device-coherent loads the compiler is free to issue back to back: the per-element
  // atomic loads of a first version were a chain of 48 memory latencies, 34 us for the launch)
  constexpr int AUX_SC1 = 16;
  const __amdgpu_buffer_rsrc_t rsP = __builtin_amdgcn_make_buffer_rsrc(pooled, 0, (int)((size_t)B * H * 4), 0x00020000);
  // every task's loads are issued before the first is waited for: two tasks (2 x up to 16 loads per lane) at a time
  constexpr int PF = 16;
  for (int o0 = wave; o0 < B * Cn; o0 += 8) {
    float pv[2][PF], acc[2] = {0.f, 0.f};
    for (int k0 = 0; k0 < H; k0 += 64 * PF) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int o = o0 + 4 * t;
        const int b = o < B * Cn ? o / Cn : 0;
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          const int k = k0 + lane + 64 * j;
          // (a column beyond H: an offset beyond the descriptor's range reads as zero)
          pv[t][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsP, k < H ? (b * H + k) * 4 : 0x7ffffff0, 0, AUX_SC1));
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int o = o0 + 4 * t;
        if (o < B * Cn) {
          const int c = o - (o / Cn) * Cn;
#pragma unroll
          for (int j = 0; j < PF; ++j) {
            const int k = k0 + lane + 64 * j;
            if (k < H) acc[t] += pv[t][j] * Wl[(size_t)c * H + k];
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int o = o0 + 4 * t;
      const float a = wave_sum(acc[t]);
      if (lane == 0 && o < B * Cn) logits[o] = a + bl[o - (o / Cn) * Cn];
    }
  }
}

// backward: one launch of 16-wave workgroups in three roles (by blockIdx.x):
//   [0, nW)          one wave (of four) per pooler output n: dWp[n][:] += sum_b dpre[b][n] h0[b][:], dbp[n] += sum_b dpre[b][n]   (pooler_bwd_w_kernel)
//   [nW, nW + nX)    (64 columns k, one sample b): dh0[b][k] = sum_n dpre[b][n] Wp[n][k]                                  (pooler_bwd_x_kernel)
//   nW + nX ..       thread per k: dWl[c][k] += sum_b dlogits[b][c] pooled[b][k]; dbl[c] += sum_b dlogits[b][c]           (linear_small_bwd_kernel)
// every role recomputes the pooled rows' gradient it needs from the logits' gradient on the fly (Cn multiply-adds per element):
//   dpooled[b][n] = sum_c dlogits[b][c] Wl[c][n],  dpre[b][n] = dpooled[b][n] (1 - pooled[b][n]^2)
constexpr int PHB_WAVES = 16;
constexpr int PHB_MAX_H = 4096;     // (the X role keeps one sample's row of H gradients in LDS)
// the forward's descriptor over `pooled` takes its size as an int, and the offset 0x7ffffff0 it hands a column beyond H must lie
// outside it: both launchers refuse a pooled tensor of that many bytes or more
constexpr size_t PH_MAX_POOLED_BYTES = 0x7ffffff0u;
__device__ __forceinline__ float phb_dpre(const float* __restrict__ dlogits, const float* __restrict__ Wl,
                                          const float* __restrict__ pooled, int b, int n, int H, int Cn) {
  float s = 0.f;
  for (int c = 0; c < Cn; ++c) s += dlogits[(size_t)b * Cn + c] * Wl[(size_t)c * H + n];
  const float p = pooled[(size_t)b * H + n];
  return s * (1.0f - p * p);
}

__global__ __launch_bounds__(64 * PHB_WAVES) void pool_head_bwd_kernel(const float* __restrict__ dlogits,
                                                                       const float* __restrict__ pooled,
                                                                       const float* __restrict__ hidden,
                                                                       const float* __restrict__ Wp, const float* __restrict__ Wl,
                                                                       float* __restrict__ dWp, float* __restrict__ dbp,
                                                                       float* __restrict__ dWl, float* __restrict__ dbl,
                                                                       float* __restrict__ dhidden, int B, int L, int H, int Cn,
                                                                       int nW, int nX, int beta) {
  __shared__ float red[PHB_WAVES][64];
  __shared__ float dpre_s[PHB_MAX_H];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int blk = blockIdx.x;
  if (blk < nW) {
    // (four of the sixteen waves: one pooler output each, spread over H / 4 workgroups -- the wave's loop over the batch rows of
    // hidden is a chain of load latencies that sixteen waves on one CU only queue behind each other)
    if (wv >= 4) return;
    const int n = blk * 4 + wv;
    if (n >= H) return;
    float sb = 0.f;
    for (int bc = 0; bc < B; bc += 64) {
      const int nb = min(64, B - bc);
      const float dpre = lane < nb ? phb_dpre(dlogits, Wl, pooled, bc + lane, n, H, Cn) : 0.f;
      sb += wave_sum(dpre);
      if ((H & 3) == 0) {                     // (wave-uniform trip counts around the shuffles, as in pooler_bwd_w_kernel)
        const int H4 = H >> 2;
        for (int k0 = 0; k0 < H4; k0 += 64) {
          const int k4 = k0 + lane;
          const bool on = k4 < H4;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          for (int b = 0; b < nb; ++b) {
            const float d = __shfl(dpre, b, 64);
            if (on) {
              const f32x4 x = reinterpret_cast<const f32x4*>(hidden + (size_t)(bc + b) * L * H)[k4];
              acc[0] += d * x[0]; acc[1] += d * x[1]; acc[2] += d * x[2]; acc[3] += d * x[3];
            }
          }
          if (on) {
            f32x4* o = reinterpret_cast<f32x4*>(dWp + (size_t)n * H) + k4;
            f32x4 t = *o;
            t[0] += acc[0]; t[1] += acc[1]; t[2] += acc[2]; t[3] += acc[3];
            *o = t;
          }
        }
      } else {
        for (int k0 = 0; k0 < H; k0 += 64) {
          const int k = k0 + lane;
          float s = 0.f;
          for (int b = 0; b < nb; ++b) {
            const float d = __shfl(dpre, b, 64);
            if (k < H) s += d * hidden[(size_t)(bc + b) * L * H + k];
          }
          if (k < H) dWp[(size_t)n * H + k] += s;
        }
      }
    }
    if (lane == 0) dbp[n] += sb;
    return;
  }
  blk -= nW;
  if (blk < nX) {
    // the sample's 'dpre' row once per workgroup through LDS (every thread one or a few n), then sixteen waves split the sum over n:
    // the loop is a stream of Wp loads with nothing to wait for in between
    const int kb = (H + 63) / 64;
    const int b = blk / kb;
    const int k = (blk - b * kb) * 64 + lane;
    for (int n = threadIdx.x; n < H; n += 64 * PHB_WAVES) dpre_s[n] = phb_dpre(dlogits, Wl, pooled, b, n, H, Cn);
    __syncthreads();
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (k < H) {
      constexpr int S = PHB_WAVES;
      int n = wv;
      for (; n + 3 * S < H; n += 4 * S) {        // (the summation order of pooler_bwd_x_kernel)
        s0 += dpre_s[n] * Wp[(size_t)n * H + k];
        s1 += dpre_s[n + S] * Wp[(size_t)(n + S) * H + k];
        s2 += dpre_s[n + 2 * S] * Wp[(size_t)(n + 2 * S) * H + k];
        s3 += dpre_s[n + 3 * S] * Wp[(size_t)(n + 3 * S) * H + k];
      }
      for (; n < H; n += S) s0 += dpre_s[n] * Wp[(size_t)n * H + k];
    }
    red[wv][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (wv == 0 && k < H) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < PHB_WAVES; ++w) s += red[w][lane];
      float* d = dhidden + (size_t)b * L * H + k;
      *d = beta ? *d + s : s;
    }
    return;
  }
  blk -= nX;
  const int k = blk * 64 * PHB_WAVES + threadIdx.x;
  if (k < Cn) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dlogits[(size_t)b * Cn + k];
    dbl[k] += s;
  }
  if (k >= H) return;
  for (int c = 0; c < Cn; ++c) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dlogits[(size_t)b * Cn + c] * pooled[(size_t)b * H + k];
    dWl[(size_t)c * H + k] += s;
  }
}

}  // namespace

extern "C" int uniter_pooler_fwd(const float* hidden, const float* Wp, const float* bp, float* pooled, int B,
                                 int L, int H, void* stream) {
  UCHECK_ARG(hidden && Wp && bp && pooled && B > 0 && L > 0 && H > 0, "pooler_fwd: bad argument");
  hipLaunchKernelGGL(pooler_fwd_kernel, dim3((H + 3) / 4, (B + 3) / 4), dim3(256), 0, (hipStream_t)stream, hidden, Wp, bp,
                     pooled, B, L, H);
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_pooler_bwd(const float* dpooled, const float* pooled, const float* hidden,
                                 const float* Wp, float* dWp, float* dbp, float* dhidden, int B, int L, int H,
                                 int beta_dhidden, void* stream) {
  UCHECK_ARG(dpooled && pooled && hidden && Wp && dWp && dbp && B > 0 && L > 0 && H > 0,
             "pooler_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pooler_bwd_w_kernel, dim3((H + 3) / 4), dim3(256), 0, st, dpooled, pooled, hidden, dWp,
                     dbp, B, L, H);
  UCHECK_LAUNCH();
  if (dhidden) {
    hipLaunchKernelGGL(pooler_bwd_x_kernel, dim3((H + 63) / 64, B), dim3(64 * PBX_WAVES), 0, st, dpooled, pooled, Wp,
                       dhidden, B, L, H, beta_dhidden);
    UCHECK_LAUNCH();
  }
  return 0;
}

extern "C" int uniter_linear_small_fwd(const float* x, const float* W, const float* b, float* y, int B, int H,
                                       int Cn, void* stream) {
  UCHECK_ARG(x && W && b && y && B > 0 && H > 0 && Cn > 0, "linear_small_fwd: bad argument");
  hipLaunchKernelGGL(linear_small_fwd_kernel, dim3((B * Cn + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, W,
                     b, y, B, H, Cn);
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_linear_small_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW,
                                       float* db, int B, int H, int Cn, void* stream) {
  UCHECK_ARG(dy && x && W && B > 0 && H > 0 && Cn > 0 && Cn <= H, "linear_small_bwd: bad argument");
  hipLaunchKernelGGL(linear_small_bwd_kernel, dim3((H + 255) / 256), dim3(256), 0, (hipStream_t)stream, dy, x,
                     W, dx, dW, db, B, H, Cn);
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_bce_logits(const float* logits, const int64_t* labels, float pos_weight, float* loss,
                                 float* probs, float* dlogits, float grad_scale, int B, void* stream) {
  UCHECK_ARG(logits && labels && B > 0, "bce_logits: bad argument");
  hipLaunchKernelGGL(bce_logits_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, labels,
                     pos_weight, loss, probs, dlogits, grad_scale, B);
  UCHECK_LAUNCH();
  return 0;
}

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

extern "C" int uniter_bce_auc_logits(const float* logits, const int64_t* labels, float pos_weight, float auc_weight, int kind,
                                     float margin, float* bank_scores, int32_t* bank_labels, int32_t* bank_state, int N, int push,
                                     float* terms, int32_t* n_pairs, float* probs, float* dlogits, float grad_scale, int B,
                                     void* stream) {
  UCHECK_ARG(logits && labels, "bce_auc_logits: null logits or labels");
  UCHECK_ARG(B > 0 && B <= AUC_MAX_B, "bce_auc_logits: B must lie in [1, %d] (got %d)", AUC_MAX_B, B);
  const bool bank = bank_scores != nullptr && N != 0;
  if (bank) {
    UCHECK_ARG(N >= B && N <= AUC_MAX_N, "bce_auc_logits: the bank's capacity must lie in [B, %d] (got N = %d, B = %d)", AUC_MAX_N, N, B);
    UCHECK_ARG(bank_labels && bank_state, "bce_auc_logits: a bank needs bank_labels and bank_state");
  }
  UCHECK_ARG(auc_weight >= 0.f, "bce_auc_logits: auc_weight is negative or NaN");
  UCHECK_ARG(kind == 0 || kind == 1, "bce_auc_logits: kind must be 0 (logistic) or 1 (squared hinge), got %d", kind);
  UCHECK_ARG(margin == margin, "bce_auc_logits: margin is NaN");
  const int Nk = bank ? N : 0;
  const size_t lds = (size_t)(B + Nk) * 5;
  auto kernel = kind == 0 ? bce_auc_logits_kernel<0> : bce_auc_logits_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(256), align_up(lds, 16), (hipStream_t)stream, logits, labels, pos_weight, auc_weight, margin,
                     bank_scores, bank_labels, bank_state, Nk, push, terms, n_pairs, probs, dlogits, grad_scale, B);
  UCHECK_LAUNCH();
  return 0;
}

// Pooler + classifier, one launch: pooled = tanh(hidden[:, 0] Wp^T + bp) (model/layer.py:179-185), logits = pooled Wl^T + bl
// (model/meme_uniter.py:19-21).  `ticket`: UNITER_POOL_HEAD_TICKET_WORDS zero-initialised unsigneds the launch leaves zero again (its last
// workgroup computes the logits).  Results equal uniter_pooler_fwd followed by uniter_linear_small_fwd.  H <= 4096 and
// B * H * 4 < 0x7ffffff0, as the backward launch.
extern "C" int uniter_pool_head_fwd(const float* hidden, const float* Wp, const float* bp, const float* Wl, const float* bl,
                                    float* pooled, float* logits, unsigned* ticket, int B, int L, int H, int Cn, void* stream) {
  UCHECK_ARG(hidden && Wp && bp && Wl && bl && pooled && logits && ticket && B > 0 && L > 0 && H > 0 && Cn > 0,
             "pool_head_fwd: bad argument");
  UCHECK_ARG(H <= PHB_MAX_H, "pool_head_fwd: hidden size up to %d (got %d)", PHB_MAX_H, H);
  UCHECK_ARG((size_t)B * H * 4 < PH_MAX_POOLED_BYTES, "pool_head_fwd: B * H * 4 must stay below 0x7ffffff0 (got B = %d, H = %d)", B, H);
  hipLaunchKernelGGL(pool_head_fwd_kernel, dim3((H + 3) / 4, (B + 3) / 4), dim3(256), 0, (hipStream_t)stream, hidden, Wp, bp, Wl,
                     bl, pooled, logits, ticket, B, L, H, Cn);
  UCHECK_LAUNCH();
  return 0;
}

// Backward of uniter_pool_head_fwd from the logits' gradient, one launch: dWp, dbp, dWl, dbl are ACCUMULATED into, dhidden (optional) gets
// the pooler's input gradient in the first row of every sample (assigned, or added with beta_dhidden != 0; the other rows are not touched).
// Results equal uniter_linear_small_bwd followed by uniter_pooler_bwd.
extern "C" int uniter_pool_head_bwd(const float* dlogits, const float* pooled, const float* hidden, const float* Wp,
                                    const float* Wl, float* dWp, float* dbp, float* dWl, float* dbl, float* dhidden, int B, int L,
                                    int H, int Cn, int beta_dhidden, void* stream) {
  UCHECK_ARG(dlogits && pooled && hidden && Wp && Wl && dWp && dbp && dWl && dbl && B > 0 && L > 0 && H > 0 && Cn > 0 && Cn <= H &&
                 H <= PHB_MAX_H, "pool_head_bwd: bad argument (hidden size up to 4096)");
  UCHECK_ARG((size_t)B * H * 4 < PH_MAX_POOLED_BYTES, "pool_head_bwd: B * H * 4 must stay below 0x7ffffff0 (got B = %d, H = %d)", B, H);
  const int nW = (H + 3) / 4;
  const int nX = dhidden ? ((H + 63) / 64) * B : 0;
  const int nL = (H + 64 * PHB_WAVES - 1) / (64 * PHB_WAVES);
  hipLaunchKernelGGL(pool_head_bwd_kernel, dim3(nW + nX + nL), dim3(64 * PHB_WAVES), 0, (hipStream_t)stream, dlogits, pooled, hidden,
                     Wp, Wl, dWp, dbp, dWl, dbl, dhidden, B, L, H, Cn, nW, nX, beta_dhidden);
  UCHECK_LAUNCH();
  return 0;
}
