// Ensemble weight search: the AUROC pair counts of C weight vectors against one prediction matrix, in ONE launch.  The scoring
// contract (operands, the order of the double arithmetic, the count) is in include/uniter_hip.h and is restated there only.
//
// Decomposition.  A candidate is independent of every other, its N mixed scores fit in LDS, and its result is one
// integer, so a workgroup takes a candidate (grid-stride over candidates):
//   * mix     thread i forms s_i from column i of x (and of present): M coalesced 8-byte loads per plane, the candidate's
//             weights at wave-uniform addresses; x and present are the same for every candidate and stay in L2.
//   * count   the columns are positives first.  A wave owns a contiguous share of the negatives and walks it at a wave-uniform LDS
//             address (identical addresses broadcast: no bank conflict); a lane holds KPOS positives in registers, so one 8-byte
//             LDS read serves 64 * KPOS comparisons.  (s_p > s_n) + (s_p >= s_n) is 2 * greater + equal.  A register slot past
//             n_pos holds a NaN, which compares false both times.
//   * reduce  32-bit partial counts per lane (2 * ceil(n_pos / 64) * ceil(negatives / waves) < 2^19), 64-bit across the wave and
//             the workgroup, one store by thread 0.
// No atomics, no workspace; the count does not depend on the grid or on which wave saw which pair.
#include "common.h"

namespace {

constexpr int KPOS = 4;                  // positives per lane and trip
constexpr int SMALL_N = 2048;            // up to here: 16 KB of scores, 256 threads, several workgroups per CU

struct EnsembleArgs {
  const double* x;
  const double* present;
  const double* w;
  int64_t* counts;
  int M, N, n_pos, C;
};

template <int NMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void ensemble_auc_kernel(const EnsembleArgs a) {
  constexpr int WAVES = THREADS / 64;
  __shared__ double s[NMAX];
  __shared__ unsigned long long part[WAVES];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nneg = a.N - a.n_pos;
  const int share = (nneg + WAVES - 1) / WAVES;
  const int j0 = min(wave * share, nneg), j1 = min(j0 + share, nneg);       // this wave's negatives
  const double* neg = s + a.n_pos;
  for (int c = blockIdx.x; c < a.C; c += gridDim.x) {
    const double* w = a.w + (size_t)c * a.M;
    for (int i = threadIdx.x; i < a.N; i += THREADS) {
      double num = 0.0, ws = 0.0;
      if (a.present) {
        for (int m = 0; m < a.M; ++m) {
          const double wm = w[m], pr = a.present[(size_t)m * a.N + i];
          num = num + (wm * a.x[(size_t)m * a.N + i]) * pr;
          ws = ws + wm * pr;
        }
      } else {                            // present == 1.0: the two products by it are exact
        for (int m = 0; m < a.M; ++m) {
          const double wm = w[m];
          num = num + wm * a.x[(size_t)m * a.N + i];
          ws = ws + wm;
        }
      }
      const double q = num / fmin(fmax(ws, 1e-4), 1e5);
      s[i] = ws == 0.0 ? 0.5 : q;
    }
    __syncthreads();
    unsigned cnt = 0;
    for (int p0 = 0; p0 < a.n_pos; p0 += 64 * KPOS) {
      double sp[KPOS];
#pragma unroll
      for (int k = 0; k < KPOS; ++k) {
        const int p = p0 + 64 * k + lane;
        sp[k] = p < a.n_pos ? s[p] : __builtin_nan("");
      }
#pragma unroll 4
      for (int j = j0; j < j1; ++j) {
        const double sn = neg[j];
#pragma unroll
        for (int k = 0; k < KPOS; ++k) cnt += (unsigned)(sp[k] > sn) + (unsigned)(sp[k] >= sn);
      }
    }
    unsigned long long total = cnt;
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    if (lane == 0) part[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long sum = 0;
#pragma unroll
      for (int k = 0; k < WAVES; ++k) sum += part[k];
      a.counts[c] = (int64_t)sum;
    }
    __syncthreads();                      // s and part are the next candidate's
  }
}

}  // namespace

extern "C" int uniter_ensemble_auc_counts(const double* x, const double* present, const double* w, int64_t* counts, int M, int N,
                                          int n_pos, int C, void* stream) {
  UCHECK_ARG(x && w && counts, "ensemble_auc_counts: null pointer");
  UCHECK_ARG((((uintptr_t)x | (uintptr_t)present | (uintptr_t)w | (uintptr_t)counts) & 7) == 0,
             "ensemble_auc_counts: x, present, w and counts must be 8-byte aligned");
  UCHECK_SHAPE(N >= 1 && N <= UNITER_ENSEMBLE_MAX_N, "ensemble_auc_counts: N = %d is outside [1, %d] (the scores of one candidate stay in LDS)",
               N, UNITER_ENSEMBLE_MAX_N);
  UCHECK_SHAPE(M >= 1 && M <= UNITER_ENSEMBLE_MAX_M, "ensemble_auc_counts: M = %d is outside [1, %d]", M, UNITER_ENSEMBLE_MAX_M);
  UCHECK_SHAPE(C >= 1, "ensemble_auc_counts: C = %d (at least one candidate)", C);
  UCHECK_ARG(n_pos >= 0 && n_pos <= N, "ensemble_auc_counts: n_pos = %d is outside [0, N = %d]", n_pos, N);
  EnsembleArgs a;
  a.x = x; a.present = present; a.w = w; a.counts = counts; a.M = M; a.N = N; a.n_pos = n_pos; a.C = C;
  const unsigned grid = (unsigned)(C < (1 << 20) ? C : (1 << 20));
  if (N <= SMALL_N)
    hipLaunchKernelGGL((ensemble_auc_kernel<SMALL_N, 256>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((ensemble_auc_kernel<UNITER_ENSEMBLE_MAX_N, 1024>), dim3(grid), dim3(1024), 0, (hipStream_t)stream, a);
  UCHECK_LAUNCH();
  return 0;
}
