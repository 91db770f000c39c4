// Embedding kernels: text (3 table lookups + LN + dropout), image-region
// epilogue (3 LayerNorms + 7-d position projection + type embedding + dropout),
// the gather that compacts [text|regions] per sample, and their backward.
//
// Replaces UniterTextEmbeddings.forward (model/model.py:232-245),
// UniterImageEmbeddings.forward after img_linear (:261-272), the type-embedding
// lookup of _compute_img_embeddings (:311-319) and cat + torch.gather
// (:330-333), plus their autograd.
//
// HBM/latency-bound row kernels: one wave per row of H floats, 16-byte accesses,
// all three LayerNorms of an image row stay in registers.  Backward recomputes
// the cheap forward pieces instead of saving them; embedding-table gradients are
// scattered with fp32 atomics issued as 256-B contiguous wave transactions (the
// fast shape, MI355X_MICROARCH.md "Global float atomics"); affine / type grads use
// deterministic two-stage column reductions.  The opt-in deterministic backward (uniter_*_embed_bwd_det, below the atomic
// kernels' entry points) sums the same table gradients in an order fixed by the inputs: per-row gradients to a workspace, a stable
// rank of the rows by table key, chunk sums, one plain read-modify-write per key.
#include <type_traits>
#include "common.h"
#include "gemm_internal.h"
#include "philox.h"
#include "rowops.h"

namespace {

__device__ __forceinline__ int clampi(long long v, int hi) { return v < 0 ? 0 : (v >= hi ? hi - 1 : (int)v); }

template <int NV>
__device__ __forceinline__ void row_add(f32x4 (&v)[NV], const f32x4 (&w)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] += w[k];
}

// p[c] = sum_k pos7[k] * Wp[c*7+k] + bp[c] for the lane's columns
template <int NV>
__device__ __forceinline__ void pos_linear(f32x4 (&p)[NV], const float* __restrict__ pos7,
                                           const float* __restrict__ Wp, const float* __restrict__ bp,
                                           int H4, int lane) {
  float x[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) x[k] = pos7[k];
#pragma unroll
  for (int kk = 0; kk < NV; ++kk) {
    const int c4 = lane + 64 * kk;
    if (c4 < H4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c4 * 4 + e;
        float s = bp[c];
#pragma unroll
        for (int k = 0; k < 7; ++k) s += x[k] * Wp[c * 7 + k];
        p[kk][e] = s;
      }
    } else {
      p[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

struct TxtArgs {
  const int64_t* ids; const int64_t* pos_ids; const int64_t* type_ids;
  const float* word; const float* pos; const float* type;
  const float* gamma; const float* beta;
  float* cat; const float* dcat;
  float* dword; float* dpos; float* dtype; float* part;
  int B, T, S, H, vocab, max_pos, type_vocab, pos_bcast;
  DropCfg drop;
};

// DELTA: an additive perturbation of the word row, delta[row][H] (uniter_txt_embed_fwd_delta, and the backward pass of such a forward,
// which recomputes the LayerNorm's input): (word + delta) + pos + type
struct TxtDeltaArgs : TxtArgs { const float* delta; };

template <int NV, bool DELTA = false>
__device__ __forceinline__ void txt_row_sum(const TxtArgs& a, const float* __restrict__ delta, int row, int t, f32x4 (&e)[NV],
                                            int& id, int& pid, int& tt, int H4, int lane) {
  id = clampi(a.ids[row], a.vocab);
  pid = clampi(a.pos_ids[a.pos_bcast ? t : row], a.max_pos);
  tt = a.type_ids ? clampi(a.type_ids[row], a.type_vocab) : 0;
  f32x4 w[NV];
  row_load<NV>(e, a.word + (size_t)id * a.H, H4, lane);
  if constexpr (DELTA) {
    row_load<NV>(w, delta + (size_t)row * a.H, H4, lane);
    row_add<NV>(e, w);
  }
  row_load<NV>(w, a.pos + (size_t)pid * a.H, H4, lane);
  row_add<NV>(e, w);
  row_load<NV>(w, a.type + (size_t)tt * a.H, H4, lane);
  row_add<NV>(e, w);
}

template <int NV, bool DELTA = false>
__global__ __launch_bounds__(256) void txt_embed_fwd_kernel(const std::conditional_t<DELTA, TxtDeltaArgs, TxtArgs> a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.T) return;
  const int b = row / a.T, t = row - b * a.T, H4 = a.H >> 2;
  f32x4 e[NV];
  int id, pid, tt;
  const float* delta = nullptr;
  if constexpr (DELTA) delta = a.delta;
  txt_row_sum<NV, DELTA>(a, delta, row, t, e, id, pid, tt, H4, lane);
  float mean, rstd;
  row_stats<NV>(e, a.H, H4, lane, mean, rstd);
  row_affine<NV>(e, a.gamma, a.beta, mean, rstd, H4, lane);
  if (a.drop.active) row_dropout<NV>(e, a.drop, (uint64_t)row * H4, H4, lane);
  row_store<NV>(e, a.cat + ((size_t)b * a.S + t) * a.H, H4, lane);
}

// scatter-add one row (held as float4 chunks) as contiguous 256-B atomic transactions via LDS
template <int NV>
__device__ __forceinline__ void row_atomic_add(const f32x4 (&v)[NV], float* buf, float* __restrict__ dst,
                                               int H, int H4, int lane) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = lane + 64 * k;
    if (c < H4) *reinterpret_cast<f32x4*>(buf + c * 4) = v[k];
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
  for (int c = lane; c < H; c += 64) atomicAdd(dst + c, buf[c]);
  __builtin_amdgcn_wave_barrier();
}

// DET: the row's table gradient goes to the workspace drow[row][H] with plain 16-byte stores instead of the atomic scatter
struct TxtDetArgs : TxtArgs { float* drow; };
struct TxtDetDeltaArgs : TxtDetArgs { const float* delta; };
template <bool DET, bool DELTA>
using TxtBwdArgs = std::conditional_t<DELTA, std::conditional_t<DET, TxtDetDeltaArgs, TxtDeltaArgs>, std::conditional_t<DET, TxtDetArgs, TxtArgs>>;

template <int NV, bool DET = false, bool DELTA = false>
__global__ __launch_bounds__(256) void txt_embed_bwd_kernel(const TxtBwdArgs<DET, DELTA> a) {
  __shared__ __attribute__((aligned(16))) float red[4 * NV * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, H4 = a.H >> 2;
  float* abuf = red + wave * NV * 256;   // per-wave staging for atomics (reused for the reduce)
  f32x4 g[NV], dg[NV], db[NV], dt0[NV];
  row_load<NV>(g, a.gamma, H4, lane);
#pragma unroll
  for (int k = 0; k < NV; ++k) { dg[k] = f32x4{0, 0, 0, 0}; db[k] = dg[k]; dt0[k] = dg[k]; }
  const int rows = a.B * a.T;
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const int b = row / a.T, t = row - b * a.T;
    f32x4 d[NV], e[NV];
    row_load<NV>(d, a.dcat + ((size_t)b * a.S + t) * a.H, H4, lane);
    if (a.drop.active) row_dropout<NV>(d, a.drop, (uint64_t)row * H4, H4, lane);
    int id, pid, tt;
    const float* delta = nullptr;
    if constexpr (DELTA) delta = a.delta;
    txt_row_sum<NV, DELTA>(a, delta, row, t, e, id, pid, tt, H4, lane);
    float mean, rstd;
    row_stats<NV>(e, a.H, H4, lane, mean, rstd);
    row_ln_bwd<NV>(d, e, g, mean, rstd, dg, db, a.H, H4, lane);     // d <- d(sum of the three lookups)
    if constexpr (DET) {
      row_store<NV>(d, a.drow + (size_t)row * a.H, H4, lane);
      if (!a.type_ids) row_add<NV>(dt0, d);
    } else {
    if (id != 0) row_atomic_add<NV>(d, abuf, a.dword + (size_t)id * a.H, a.H, H4, lane);  // padding_idx=0
    row_atomic_add<NV>(d, abuf, a.dpos + (size_t)pid * a.H, a.H, H4, lane);
    if (a.type_ids) row_atomic_add<NV>(d, abuf, a.dtype + (size_t)tt * a.H, a.H, H4, lane);
    else row_add<NV>(dt0, d);
    }
  }
  float* part = a.part + (size_t)blockIdx.x * 3 * a.H;
  block_col_reduce_store<NV>(dg, red, part, H4, lane, wave);
  block_col_reduce_store<NV>(db, red, part + a.H, H4, lane, wave);
  block_col_reduce_store<NV>(dt0, red, part + 2 * a.H, H4, lane, wave);
}

struct ImgArgs {
  const float* imgfc; const float* pos7; const int64_t* type_ids;
  const float* Wp; const float* bp; const float* type;
  const float* g_i; const float* b_i; const float* g_p; const float* b_p; const float* g_f; const float* b_f;
  float* cat; float* stats; const float* dcat;
  float* d_imgfc; float* d_posfc; float* dtype; float* part;
  int B, R, T0, S, H, type_vocab;
  DropCfg drop;
};

template <int NV>
__global__ __launch_bounds__(256) void img_embed_fwd_kernel(const ImgArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.R) return;
  const int b = row / a.R, r = row - b * a.R, H4 = a.H >> 2;
  f32x4 x[NV], p[NV];
  float st[6];
  row_load<NV>(x, a.imgfc + (size_t)row * a.H, H4, lane);
  row_stats<NV>(x, a.H, H4, lane, st[0], st[1]);
  row_affine<NV>(x, a.g_i, a.b_i, st[0], st[1], H4, lane);
  pos_linear<NV>(p, a.pos7 + (size_t)row * 7, a.Wp, a.bp, H4, lane);
  row_stats<NV>(p, a.H, H4, lane, st[2], st[3]);
  row_affine<NV>(p, a.g_p, a.b_p, st[2], st[3], H4, lane);
  row_add<NV>(x, p);
  const int tid = a.type_ids ? clampi(a.type_ids[row], a.type_vocab) : 1;
  row_load<NV>(p, a.type + (size_t)tid * a.H, H4, lane);
  row_add<NV>(x, p);
  // lanes beyond H4 hold garbage-free zeros only if every addend was zero there: enforce
#pragma unroll
  for (int k = 0; k < NV; ++k) if (lane + 64 * k >= H4) x[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  row_stats<NV>(x, a.H, H4, lane, st[4], st[5]);
  row_affine<NV>(x, a.g_f, a.b_f, st[4], st[5], H4, lane);
  if (a.drop.active) row_dropout<NV>(x, a.drop, (uint64_t)row * H4, H4, lane);
  row_store<NV>(x, a.cat + ((size_t)b * a.S + a.T0 + r) * a.H, H4, lane);
  if (a.stats && lane < 6) a.stats[(size_t)row * 6 + lane] = st[lane];
}

struct ImgDetArgs : ImgArgs { float* drow; };

template <int NV, bool DET = false>
__global__ __launch_bounds__(256) void img_embed_bwd_kernel(const std::conditional_t<DET, ImgDetArgs, ImgArgs> a) {
  __shared__ __attribute__((aligned(16))) float red[4 * NV * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, H4 = a.H >> 2;
  float* abuf = red + wave * NV * 256;
  f32x4 acc[7][NV];      // dg_f, db_f, dg_i, db_i, dg_p, db_p, dtype[1]
#pragma unroll
  for (int s = 0; s < 7; ++s)
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[s][k] = f32x4{0, 0, 0, 0};
  f32x4 gf[NV], gi[NV], gp[NV];
  row_load<NV>(gf, a.g_f, H4, lane);
  row_load<NV>(gi, a.g_i, H4, lane);
  row_load<NV>(gp, a.g_p, H4, lane);
  const int rows = a.B * a.R;
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const int b = row / a.R, r = row - b * a.R;
    const float* st = a.stats + (size_t)row * 6;
    f32x4 d[NV], x[NV], p[NV], f[NV];
    row_load<NV>(d, a.dcat + ((size_t)b * a.S + a.T0 + r) * a.H, H4, lane);
    if (a.drop.active) row_dropout<NV>(d, a.drop, (uint64_t)row * H4, H4, lane);
    // recompute f = LN_i(imgfc) + LN_p(pos proj) + type
    row_load<NV>(x, a.imgfc + (size_t)row * a.H, H4, lane);
    pos_linear<NV>(p, a.pos7 + (size_t)row * 7, a.Wp, a.bp, H4, lane);
    const int tid = a.type_ids ? clampi(a.type_ids[row], a.type_vocab) : 1;
    row_load<NV>(f, a.type + (size_t)tid * a.H, H4, lane);
    {
      f32x4 t[NV];
#pragma unroll
      for (int k = 0; k < NV; ++k) t[k] = x[k];
      row_affine<NV>(t, a.g_i, a.b_i, st[0], st[1], H4, lane);
      row_add<NV>(f, t);
#pragma unroll
      for (int k = 0; k < NV; ++k) t[k] = p[k];
      row_affine<NV>(t, a.g_p, a.b_p, st[2], st[3], H4, lane);
      row_add<NV>(f, t);
    }
    row_ln_bwd<NV>(d, f, gf, st[4], st[5], acc[0], acc[1], a.H, H4, lane);      // d <- df
    if constexpr (DET) {
      if (a.type_ids) row_store<NV>(d, a.drow + (size_t)row * a.H, H4, lane);
      else row_add<NV>(acc[6], d);
    } else {
    if (a.type_ids) row_atomic_add<NV>(d, abuf, a.dtype + (size_t)tid * a.H, a.H, H4, lane);
    else row_add<NV>(acc[6], d);
    }
    f32x4 d2[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) d2[k] = d[k];
    row_ln_bwd<NV>(d, x, gi, st[0], st[1], acc[2], acc[3], a.H, H4, lane);      // d <- d_imgfc
    row_store<NV>(d, a.d_imgfc + (size_t)row * a.H, H4, lane);
    row_ln_bwd<NV>(d2, p, gp, st[2], st[3], acc[4], acc[5], a.H, H4, lane);     // d2 <- d_posfc
    row_store<NV>(d2, a.d_posfc + (size_t)row * a.H, H4, lane);
  }
  float* part = a.part + (size_t)blockIdx.x * 7 * a.H;
#pragma unroll
  for (int s = 0; s < 7; ++s) block_col_reduce_store<NV>(acc[s], red, part + (size_t)s * a.H, H4, lane, wave);
}

// dWp[c][k] += sum_rows d_posfc[row][c] * pos7[row][k];  dbp[c] += sum_rows d_posfc[row][c]
__global__ __launch_bounds__(256) void pos_linear_wgrad_kernel(const float* __restrict__ d_posfc,
                                                               const float* __restrict__ pos7,
                                                               float* __restrict__ dWp, float* __restrict__ dbp,
                                                               int rows, int H) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * 32, r1 = min(rows, r0 + 32);
  if (c >= H) return;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = r0; r < r1; ++r) {
    const float dv = d_posfc[(size_t)r * H + c];
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k] += dv * pos7[(size_t)r * 7 + k];
    s[7] += dv;
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) atomicAdd(dWp + (size_t)c * 7 + k, s[k]);
  atomicAdd(dbp + c, s[7]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Deterministic table gradients (uniter_txt_embed_bwd_det / uniter_img_embed_bwd_det): no float atomics, the order of every sum
// fixed by the ids alone.
//   1. the row pass (DET above) leaves row r's table gradient in drow[r][H];
//   2. det_rank_kernel gives every row its stable rank by table key, rank(r) = #{r' : key[r'] < key[r] or (key[r'] == key[r] and
//      r' < r)} -- a permutation, so order[rank] = r and skey[rank] = key[r] are plain stores with one writer each.  A run of
//      equal keys in rank order is a segment: the rows that read one table row, in ascending row index;
//   3. det_chunk_kernel: the ranks are cut into chunks of DET_CHUNK; one wave per chunk sums each run of equal keys inside its
//      chunk in rank order (ascending row index).  A run that is a whole segment is added to its table row there and then; a run
//      whose segment goes on beyond the chunk is left as a piece: slot 0 of the chunk when the segment began in an earlier
//      chunk, slot 1 when it begins in this chunk (at most one run of each kind per chunk);
//   4. det_owner_kernel: the chunk a multi-chunk segment begins in owns it: its wave adds the pieces in ascending chunk order
//      (slot 1 of its own chunk, then slot 0 of the following ones) and adds the total to the table row.
// So table[key] <- table[key] + (((p_0 + p_1) + p_2) + ...), p_i = ((d[r_0] + d[r_1]) + ...) over the chunk's rows of that key in
// ascending row index; one owner per key and launch, one plain read-modify-write.  `skip` names the key whose table row stays
// as it is (the word table's padding_idx 0).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int DET_RANK_WG = 256;     // rows one workgroup ranks (one per thread)
constexpr int DET_RANK_TILE = 1024;  // keys staged through LDS at a time
constexpr int DET_CHUNK = 32;        // ranked rows per chunk
constexpr int DET_WG_ROWS = 32;      // rows per partial of the position projection's weight gradient (pos_linear_wgrad_kernel's)

struct DetTable {
  const int64_t* ids;   // the table's ids, as the forward reads them
  float* grad;          // [hi][H]
  int* order;           // [rows]: order[rank] = row
  int* skey;            // [rows]: skey[rank] = key
  float* piece;         // [chunks][2][H]
  int hi;               // keys are clamped to 0 .. hi - 1 (clampi, as txt_row_sum / the image kernels)
  int bcast_T;          // > 0: row r reads ids[r % bcast_T] (pos_bcast)
  int skip;             // key whose table row receives nothing; -1: none
};
struct DetArgs {
  DetTable t[3];
  const float* drow;
  int rows, H;
};

__device__ __forceinline__ int det_key(const DetTable& t, int row) {
  return clampi(t.ids[t.bcast_T > 0 ? row % t.bcast_T : row], t.hi);
}

// grid (ceil(rows / DET_RANK_WG), tables)
__global__ __launch_bounds__(DET_RANK_WG) void det_rank_kernel(const DetArgs a) {
  __shared__ int keys[DET_RANK_TILE];
  const DetTable t = a.t[blockIdx.y];
  const int r = blockIdx.x * DET_RANK_WG + threadIdx.x;
  const int mine = r < a.rows ? det_key(t, r) : 0;
  int rank = 0;
  for (int base = 0; base < a.rows; base += DET_RANK_TILE) {
    const int n = min(DET_RANK_TILE, a.rows - base);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += DET_RANK_WG) keys[i] = det_key(t, base + i);
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const int k = keys[i];
      rank += (k < mine || (k == mine && base + i < r)) ? 1 : 0;
    }
  }
  if (r < a.rows) { t.order[rank] = r; t.skey[rank] = mine; }
}

template <int NV>
__device__ __forceinline__ void det_table_add(const f32x4 (&acc)[NV], float* g, int H4, int lane) {
  f32x4 v[NV];
  row_load<NV>(v, g, H4, lane);
  row_add<NV>(v, acc);
  row_store<NV>(v, g, H4, lane);
}

// grid (ceil(chunks / 4), tables): one wave per chunk
template <int NV>
__global__ __launch_bounds__(256) void det_chunk_kernel(const DetArgs a) {
  const DetTable t = a.t[blockIdx.y];
  const int lane = threadIdx.x & 63, H4 = a.H >> 2;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int r0 = c * DET_CHUNK;
  if (r0 >= a.rows) return;
  const int r1 = min(a.rows, r0 + DET_CHUNK);
  const int prev = r0 > 0 ? t.skey[r0 - 1] : -1, next = r1 < a.rows ? t.skey[r1] : -1;     // (keys are >= 0)
  int i = r0;
  while (i < r1) {
    const int k = t.skey[i];
    f32x4 acc[NV];
    row_load<NV>(acc, a.drow + (size_t)t.order[i] * a.H, H4, lane);
    int j = i + 1;
    for (; j < r1 && t.skey[j] == k; ++j) {
      f32x4 v[NV];
      row_load<NV>(v, a.drow + (size_t)t.order[j] * a.H, H4, lane);
      row_add<NV>(acc, v);
    }
    const bool open_l = i == r0 && k == prev, open_r = j == r1 && k == next;
    if (open_l || open_r) row_store<NV>(acc, t.piece + ((size_t)c * 2 + (open_l ? 0 : 1)) * a.H, H4, lane);
    else if (k != t.skip) det_table_add<NV>(acc, t.grad + (size_t)k * a.H, H4, lane);
    i = j;
  }
}

// grid as det_chunk_kernel, behind it: the chunk whose last run begins a segment that goes on owns that segment
template <int NV>
__global__ __launch_bounds__(256) void det_owner_kernel(const DetArgs a) {
  const DetTable t = a.t[blockIdx.y];
  const int lane = threadIdx.x & 63, H4 = a.H >> 2;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int r0 = c * DET_CHUNK, r1 = min(a.rows, r0 + DET_CHUNK);
  if (r1 >= a.rows) return;                                            // (the last chunk, or none: nothing goes on behind it)
  const int k = t.skey[r1 - 1];
  if (t.skey[r1] != k || k == t.skip) return;
  if (r0 > 0 && t.skey[r0] == k && t.skey[r0 - 1] == k) return;        // the whole chunk lies inside a segment an earlier chunk owns
  f32x4 acc[NV];
  row_load<NV>(acc, t.piece + ((size_t)c * 2 + 1) * a.H, H4, lane);
  const int chunks = (a.rows + DET_CHUNK - 1) / DET_CHUNK;
  for (int cc = c + 1; cc < chunks && t.skey[cc * DET_CHUNK] == k; ++cc) {
    f32x4 v[NV];
    row_load<NV>(v, t.piece + (size_t)cc * 2 * a.H, H4, lane);
    row_add<NV>(acc, v);
  }
  det_table_add<NV>(acc, t.grad + (size_t)k * a.H, H4, lane);
}

// pos_linear_wgrad_kernel with the chunk's eight sums stored to part[chunk][c][8] instead of added atomically ...
__global__ __launch_bounds__(256) void pos_linear_wgrad_part_kernel(const float* __restrict__ d_posfc,
                                                                    const float* __restrict__ pos7, float* __restrict__ part,
                                                                    int rows, int H) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * DET_WG_ROWS, r1 = min(rows, r0 + DET_WG_ROWS);
  if (c >= H) return;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = r0; r < r1; ++r) {
    const float dv = d_posfc[(size_t)r * H + c];
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k] += dv * pos7[(size_t)r * 7 + k];
    s[7] += dv;
  }
  f32x4* o = reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.y * H + c) * 8);
  o[0] = f32x4{s[0], s[1], s[2], s[3]};
  o[1] = f32x4{s[4], s[5], s[6], s[7]};
}

// ... and folded over the chunks in ascending order: thread (c, k) owns dWp[c][k] (k < 7) or dbp[c] (k = 7)
__global__ __launch_bounds__(256) void pos_linear_wgrad_fold_kernel(const float* __restrict__ part, float* __restrict__ dWp,
                                                                    float* __restrict__ dbp, int chunks, int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * 8) return;
  const int c = i >> 3, k = i & 7;
  float s = part[i];
  for (int ch = 1; ch < chunks; ++ch) s += part[(size_t)ch * H * 8 + i];
  if (k < 7) dWp[(size_t)c * 7 + k] += s;
  else dbp[c] += s;
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ cat,
                                                          const int64_t* __restrict__ gi, float* __restrict__ out,
                                                          int B, int S, int Lout, int H) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * Lout) return;
  const int b = row / Lout, j = row - b * Lout;
  const int s = gi ? clampi(gi[row], S) : j;
  const f32x4* src = reinterpret_cast<const f32x4*>(cat + ((size_t)b * S + s) * H);
  f32x4* dst = reinterpret_cast<f32x4*>(out + (size_t)row * H);
  for (int c = lane; c < (H >> 2); c += 64) dst[c] = src[c];
}

// the same gather with the operand copies of layer 0's first product written in the same pass (round 6: the gather and the split were
// two launches of the chain that keeps the first encoder product waiting behind the optimizer -- 11 + 8 us): MODE 1 = the three bf16
// pieces of the fp32x3 mode ([row][3][H], what uniter_split3 writes), MODE 2 = the bf16 copy of the bf16 mode (uniter_cast_bf16)
template <int NV, int MODE>
__global__ __launch_bounds__(256) void gather_rows_ex_kernel(const float* __restrict__ cat, const int64_t* __restrict__ gi,
                                                             float* __restrict__ out, unsigned short* __restrict__ outb, int B, int S,
                                                             int Lout, int H) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * Lout) return;
  const int b = row / Lout, j = row - b * Lout;
  const int s = gi ? clampi(gi[row], S) : j;
  const int H4 = H >> 2;
  f32x4 v[NV];
  row_load<NV>(v, cat + ((size_t)b * S + s) * H, H4, lane);
  row_store<NV>(v, out + (size_t)row * H, H4, lane);
  if constexpr (MODE == 1) row_store_x3<NV>(v, outb + (size_t)row * 3 * H, H, H4, lane);
  else row_store_bf16<NV>(v, outb + (size_t)row * H, H4, lane);
}

// source-indexed: dcat[b,s] = sum over j with clamp(gi[b,j]) == s of dout[b,j]  (no atomics, deterministic; the adjoint of the
// clamped forward, so an out-of-range index sends its gradient to the row it read)
__global__ __launch_bounds__(256) void gather_rows_bwd_kernel(const float* __restrict__ dout,
                                                              const int64_t* __restrict__ gi,
                                                              float* __restrict__ dcat, int B, int S, int Lout, int H) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * S) return;
  const int b = row / S, s = row - b * S;
  f32x4* dst = reinterpret_cast<f32x4*>(dcat + (size_t)row * H);
  const int H4 = H >> 2;
  if (!gi) {
    const f32x4* src = reinterpret_cast<const f32x4*>(dout + ((size_t)b * Lout + s) * H);
    for (int c = lane; c < H4; c += 64) dst[c] = s < Lout ? src[c] : f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  for (int c0 = 0; c0 < H4; c0 += 64) {
    const int c = c0 + lane;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < Lout; j0 += 64) {
      const int j = j0 + lane;
      const bool hit = j < Lout && clampi(gi[(size_t)b * Lout + j], S) == s;     // the row the forward read (gather_rows_kernel)
      unsigned long long m = __ballot(hit);
      while (m) {
        const int jj = j0 + __builtin_ctzll(m);
        m &= m - 1;
        if (c < H4) acc += reinterpret_cast<const f32x4*>(dout + ((size_t)b * Lout + jj) * H)[c];
      }
    }
    if (c < H4) dst[c] = acc;
  }
}

__global__ void img_mask_add_kernel(const float* __restrict__ feat, const int64_t* __restrict__ masks,
                                    const float* __restrict__ mask_emb, float* __restrict__ out, int rows, int D4) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)rows * D4) return;
  const int row = (int)(idx / D4), c = (int)(idx - (size_t)row * D4);
  f32x4 v = reinterpret_cast<const f32x4*>(feat)[idx];
  // any non-zero mask adds row 1 (row 0 is zero in the reference); the same test as masked_rowsum_kernel, its gradient -- a
  // negative mask used to index before the table
  if (masks[row] != 0) v += reinterpret_cast<const f32x4*>(mask_emb + (size_t)D4 * 4)[c];
  reinterpret_cast<f32x4*>(out)[idx] = v;
}

// out[c] += sum over rows with masks[row] != 0 of x[row][c]   (gradient of mask_embedding row 1)
__global__ void masked_rowsum_kernel(const float* __restrict__ x, const int64_t* __restrict__ masks,
                                     float* __restrict__ out, int rows, int D) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= D) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r)
    if (masks[r] != 0) s += x[(size_t)r * D + c];
  out[c] += s;
}

inline int bwd_blocks(int rows) {
  int b = (rows + 3) / 4;
  return b < 256 ? (b < 1 ? 1 : b) : 256;
}

}  // namespace

int launch_masked_rowsum(const float* x, const int64_t* masks, float* out, int rows, int D, hipStream_t st) {
  hipLaunchKernelGGL(masked_rowsum_kernel, dim3((D + 255) / 256), dim3(256), 0, st, x, masks, out, rows, D);
  UCHECK_LAUNCH();
  return 0;
}

// KERNEL<NV, further template arguments>(ARG) for the NV 16-byte pieces per lane that H takes
#define NV_DISPATCH(KERNEL, GRID, ARG, ...)                                                             \
  switch ((H / 4 + 63) / 64) {                                                                          \
    case 1: hipLaunchKernelGGL((KERNEL<1, ##__VA_ARGS__>), GRID, dim3(256), 0, st, ARG); break;         \
    case 2: hipLaunchKernelGGL((KERNEL<2, ##__VA_ARGS__>), GRID, dim3(256), 0, st, ARG); break;         \
    case 3: hipLaunchKernelGGL((KERNEL<3, ##__VA_ARGS__>), GRID, dim3(256), 0, st, ARG); break;         \
    case 4: hipLaunchKernelGGL((KERNEL<4, ##__VA_ARGS__>), GRID, dim3(256), 0, st, ARG); break;         \
    default: uniter_set_error("embed: hidden size %d unsupported (max 1024)", H);                       \
             return UNITER_E_SHAPE;                                                                     \
  }

// A code object holds its kernel templates' instantiations in the order the host code first names them.  This list names them in the
// order the launchers named them while the plain, _delta and _det forms were separate functions, so the device code stays byte for
// byte what it was under the merged launchers below; nothing reads it.
#define NV4(K) (const void*)K<1>, (const void*)K<2>, (const void*)K<3>, (const void*)K<4>
#define NV4_T(K, ...) (const void*)K<1, __VA_ARGS__>, (const void*)K<2, __VA_ARGS__>, (const void*)K<3, __VA_ARGS__>, (const void*)K<4, __VA_ARGS__>
[[maybe_unused]] static const void* const kernel_order[] = {
    NV4(txt_embed_fwd_kernel), NV4_T(txt_embed_bwd_kernel, false, true), NV4(txt_embed_bwd_kernel), NV4(img_embed_fwd_kernel),
    NV4(img_embed_bwd_kernel), NV4_T(txt_embed_fwd_kernel, true), NV4(det_chunk_kernel), NV4(det_owner_kernel),
    NV4_T(txt_embed_bwd_kernel, true, true), NV4_T(txt_embed_bwd_kernel, true), NV4_T(img_embed_bwd_kernel, true)};
#undef NV4
#undef NV4_T

extern "C" size_t uniter_embed_bwd_ws_bytes(int rows, int H) {
  return (size_t)bwd_blocks(rows) * 7 * H * sizeof(float);
}

// ---- the deterministic backward (include/uniter_hip.h): its workspace and its fold ----
namespace {

// the workspace of one _det call: column partials | drow | per table: order, skey, pieces | position-projection partials
struct DetWs {
  float* part; float* drow; int* order[3]; int* skey[3]; float* piece[3]; float* wpart;
  size_t bytes;
};
DetWs det_carve(void* ws, int rows, int H, int ncol, int ntab, bool wgrad) {
  DetWs w = {};
  char* base = (char*)ws;
  size_t off = 0;
  auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += align_up(n * 4, 16); return p; };
  const size_t chunks = ((size_t)rows + DET_CHUNK - 1) / DET_CHUNK;
  w.part = (float*)take((size_t)bwd_blocks(rows) * ncol * H);
  w.drow = (float*)take((size_t)rows * H);
  for (int i = 0; i < ntab; ++i) {
    w.order[i] = (int*)take(rows);
    w.skey[i] = (int*)take(rows);
    w.piece[i] = (float*)take(chunks * 2 * H);
  }
  if (wgrad) w.wpart = (float*)take((((size_t)rows + DET_WG_ROWS - 1) / DET_WG_ROWS) * H * 8);
  w.bytes = off;
  return w;
}

// rank, chunk sums and owners of `ntab` tables over the same drow
int det_fold(DetArgs& d, int ntab, hipStream_t st) {
  const int H = d.H, chunks = (d.rows + DET_CHUNK - 1) / DET_CHUNK;
  hipLaunchKernelGGL(det_rank_kernel, dim3((d.rows + DET_RANK_WG - 1) / DET_RANK_WG, ntab), dim3(DET_RANK_WG), 0, st, d);
  UCHECK_LAUNCH();
  const dim3 grid((chunks + 3) / 4, ntab);
  NV_DISPATCH(det_chunk_kernel, grid, d);
  UCHECK_LAUNCH();
  if (chunks > 1) {
    NV_DISPATCH(det_owner_kernel, grid, d);
    UCHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" size_t uniter_embed_bwd_det_ws_bytes(int txt_rows, int img_rows, int H) {
  const size_t t = txt_rows > 0 ? det_carve(nullptr, txt_rows, H, 3, 3, false).bytes : 0;
  const size_t i = img_rows > 0 ? det_carve(nullptr, img_rows, H, 7, 1, true).bytes : 0;
  return t > i ? t : i;
}

// ---- the launchers: one call per side (rowpass_internal.h) ----
static void fill(TxtArgs& a, const TxtEmbedCall& c) {
  a.ids = c.ids; a.pos_ids = c.pos_ids; a.type_ids = c.type_ids; a.word = c.word; a.pos = c.pos; a.type = c.type;
  a.gamma = c.gamma; a.beta = c.beta; a.cat = c.cat; a.dcat = c.dcat; a.dword = c.dword; a.dpos = c.dpos; a.dtype = c.dtype;
  a.part = (float*)c.ws; a.B = c.B; a.T = c.T; a.S = c.S; a.H = c.H; a.vocab = c.vocab; a.max_pos = c.max_pos;
  a.type_vocab = c.type_vocab; a.pos_bcast = c.pos_bcast; a.drop = make_drop(c.drop);
}
static void fill(ImgArgs& a, const ImgEmbedCall& c) {
  a.imgfc = c.imgfc; a.pos7 = c.pos7; a.type_ids = c.type_ids; a.Wp = c.Wp; a.bp = c.bp; a.type = c.type;
  a.g_i = c.g_i; a.b_i = c.b_i; a.g_p = c.g_p; a.b_p = c.b_p; a.g_f = c.g_f; a.b_f = c.b_f; a.cat = c.cat; a.stats = c.stats;
  a.dcat = c.dcat; a.d_imgfc = c.d_imgfc; a.d_posfc = c.d_posfc; a.dtype = c.dtype; a.part = (float*)c.ws;
  a.B = c.B; a.R = c.R; a.T0 = c.T0; a.S = c.S; a.H = c.H; a.type_vocab = c.type_vocab; a.drop = make_drop(c.drop);
}

// c.delta: [B][T][H] added to the word rows (uniter_txt_embed_fwd_delta), 16-byte aligned; NULL = uniter_txt_embed_fwd itself
int txt_embed_fwd_run(const TxtEmbedCall& c) {
  const char* who = c.delta ? "txt_embed_fwd_delta" : "txt_embed_fwd";
  const int H = c.H;
  UCHECK_ARG(c.ids && c.pos_ids && c.word && c.pos && c.type && c.gamma && c.beta && c.cat, "%s: null pointer", who);
  if (c.delta) {
    UCHECK_ARG(((uintptr_t)c.delta & 15) == 0, "txt_embed_fwd_delta: delta must be 16-byte aligned");
    UCHECK_SHAPE(H % 4 == 0 && H <= 1024 && c.T <= c.S, "txt_embed_fwd_delta: bad shape (H %% 4, H <= 1024, T <= S)");
  } else {
    UCHECK_SHAPE(H % 4 == 0 && c.T <= c.S, "txt_embed_fwd: bad shape");
  }
  if (c.B * c.T <= 0) return 0;
  TxtDeltaArgs a = {};
  fill(a, c); a.delta = c.delta;
  hipStream_t st = (hipStream_t)c.stream;
  const dim3 grid((c.B * c.T + 3) / 4);
  if (c.delta) {
    NV_DISPATCH(txt_embed_fwd_kernel, grid, a, true);
  } else {
    const TxtArgs& plain = a;
    NV_DISPATCH(txt_embed_fwd_kernel, grid, plain);
  }
  UCHECK_LAUNCH();
  return 0;
}

// The text side's backward pass; c.delta: the forward pass's perturbation, with which the LayerNorm's input is recomputed.  c.det: the
// order-fixed form (uniter_txt_embed_bwd_det) -- the row gradients go to the carved workspace and are folded into the tables by rank
int txt_embed_bwd_run(const TxtEmbedCall& c) {
  const char* who = c.det ? "txt_embed_bwd_det" : "txt_embed_bwd";
  const int H = c.H, rows = c.B * c.T;
  UCHECK_ARG(c.dcat && c.ids && c.pos_ids && c.word && c.pos && c.type && c.gamma && c.dword && c.dpos && c.dtype &&
             c.dgamma && c.dbeta && c.ws, "%s: null pointer", who);
  if (c.det) {
    UCHECK_SHAPE(H % 4 == 0 && H <= 1024 && c.T <= c.S, "txt_embed_bwd_det: bad shape (H %% 4, H <= 1024, T <= S)");
    UCHECK_SHAPE((long long)c.B * c.T <= UNITER_EMBED_DET_MAX_ROWS, "txt_embed_bwd_det: %lld rows, the stable rank covers at most %d",
                 (long long)c.B * c.T, UNITER_EMBED_DET_MAX_ROWS);
  } else {
    UCHECK_SHAPE(H % 4 == 0 && c.T <= c.S, "txt_embed_bwd: bad shape");
    UCHECK_ARG(c.ws_bytes >= uniter_embed_bwd_ws_bytes(rows, H), "txt_embed_bwd: workspace too small");
  }
  if (rows <= 0) return 0;
  if (c.det) UCHECK_ARG(c.ws_bytes >= uniter_embed_bwd_det_ws_bytes(rows, 0, H), "txt_embed_bwd_det: workspace too small");
  const DetWs w = c.det ? det_carve(c.ws, rows, H, 3, 3, false) : DetWs{};
  TxtDetDeltaArgs a = {};
  fill(a, c); a.delta = c.delta;
  if (c.det) { a.part = w.part; a.drow = w.drow; }
  hipStream_t st = (hipStream_t)c.stream;
  const int nblk = bwd_blocks(rows);
  if (c.det && c.delta) {
    NV_DISPATCH(txt_embed_bwd_kernel, dim3(nblk), a, true, true);
  } else if (c.det) {
    const TxtDetArgs& plain = a;
    NV_DISPATCH(txt_embed_bwd_kernel, dim3(nblk), plain, true);
  } else if (c.delta) {
    const TxtDeltaArgs d = {a, c.delta};
    NV_DISPATCH(txt_embed_bwd_kernel, dim3(nblk), d, false, true);
  } else {
    const TxtArgs& plain = a;
    NV_DISPATCH(txt_embed_bwd_kernel, dim3(nblk), plain);
  }
  UCHECK_LAUNCH();
  float* outs[3] = {c.dgamma, c.dbeta, c.type_ids ? nullptr : c.dtype};
  UCHECK_RC(finalize_partials_multi({a.part, nblk, (size_t)3 * H}, outs, 3, H, st));
  if (!c.det) return 0;
  DetArgs d = {};
  d.drow = w.drow; d.rows = rows; d.H = H;
  const int64_t* src[3] = {c.ids, c.pos_ids, c.type_ids};
  float* grad[3] = {c.dword, c.dpos, c.dtype};
  const int hi[3] = {c.vocab, c.max_pos, c.type_vocab};
  const int ntab = c.type_ids ? 3 : 2;
  for (int i = 0; i < ntab; ++i) {
    DetTable& t = d.t[i];
    t.ids = src[i]; t.grad = grad[i]; t.order = w.order[i]; t.skey = w.skey[i]; t.piece = w.piece[i]; t.hi = hi[i];
    t.bcast_T = (i == 1 && c.pos_bcast) ? c.T : 0;
    t.skip = i == 0 ? 0 : -1;                           // padding_idx = 0
  }
  return det_fold(d, ntab, st);
}

int img_embed_fwd_run(const ImgEmbedCall& c) {
  const int H = c.H;
  UCHECK_ARG(c.imgfc && c.pos7 && c.Wp && c.bp && c.type && c.g_i && c.b_i && c.g_p && c.b_p && c.g_f && c.b_f && c.cat,
             "img_embed_fwd: null pointer");
  UCHECK_SHAPE(H % 4 == 0 && c.T0 + c.R <= c.S && c.type_vocab >= 2, "img_embed_fwd: bad shape");
  if (c.B * c.R <= 0) return 0;
  ImgArgs a = {};
  fill(a, c);
  hipStream_t st = (hipStream_t)c.stream;
  NV_DISPATCH(img_embed_fwd_kernel, dim3((c.B * c.R + 3) / 4), a);
  UCHECK_LAUNCH();
  return 0;
}

// The image side's backward pass; c.det: the order-fixed form (uniter_img_embed_bwd_det), whose token-type gradient of explicit ids is
// folded by rank and whose position-projection gradient is summed in two passes
int img_embed_bwd_run(const ImgEmbedCall& c) {
  const char* who = c.det ? "img_embed_bwd_det" : "img_embed_bwd";
  const int H = c.H, rows = c.B * c.R;
  UCHECK_ARG(c.dcat && c.imgfc && c.pos7 && c.Wp && c.bp && c.type && c.g_i && c.b_i && c.g_p && c.b_p && c.g_f && c.stats &&
             c.d_imgfc && c.d_posfc && c.dWp && c.dbp && c.dtype && c.dg_i && c.db_i && c.dg_p && c.db_p && c.dg_f && c.db_f && c.ws,
             "%s: null pointer", who);
  if (c.det) {
    UCHECK_SHAPE(H % 4 == 0 && H <= 1024 && c.T0 + c.R <= c.S && c.type_vocab >= 2,
                 "img_embed_bwd_det: bad shape (H %% 4, H <= 1024, T0 + R <= S, type_vocab >= 2)");
    UCHECK_SHAPE((long long)c.B * c.R <= UNITER_EMBED_DET_MAX_ROWS, "img_embed_bwd_det: %lld rows, the stable rank covers at most %d",
                 (long long)c.B * c.R, UNITER_EMBED_DET_MAX_ROWS);
  } else {
    UCHECK_SHAPE(H % 4 == 0 && c.T0 + c.R <= c.S && c.type_vocab >= 2, "img_embed_bwd: bad shape");
    UCHECK_ARG(c.ws_bytes >= uniter_embed_bwd_ws_bytes(rows, H), "img_embed_bwd: workspace too small");
  }
  if (rows <= 0) return 0;
  if (c.det) UCHECK_ARG(c.ws_bytes >= uniter_embed_bwd_det_ws_bytes(0, rows, H), "img_embed_bwd_det: workspace too small");
  const DetWs w = c.det ? det_carve(c.ws, rows, H, 7, 1, true) : DetWs{};
  ImgDetArgs a = {};
  fill(a, c);
  if (c.det) { a.part = w.part; a.drow = w.drow; }
  hipStream_t st = (hipStream_t)c.stream;
  const int nblk = bwd_blocks(rows);
  if (c.det) {
    NV_DISPATCH(img_embed_bwd_kernel, dim3(nblk), a, true);
  } else {
    const ImgArgs& plain = a;
    NV_DISPATCH(img_embed_bwd_kernel, dim3(nblk), plain);
  }
  UCHECK_LAUNCH();
  float* outs[7] = {c.dg_f, c.db_f, c.dg_i, c.db_i, c.dg_p, c.db_p, c.type_ids ? nullptr : c.dtype + H};
  UCHECK_RC(finalize_partials_multi({a.part, nblk, (size_t)7 * H}, outs, 7, H, st));
  if (!c.det) {
    hipLaunchKernelGGL(pos_linear_wgrad_kernel, dim3((H + 255) / 256, (rows + 31) / 32), dim3(256), 0, st,
                       c.d_posfc, c.pos7, c.dWp, c.dbp, rows, H);
    UCHECK_LAUNCH();
    return 0;
  }
  if (c.type_ids) {
    DetArgs d = {};
    d.drow = w.drow; d.rows = rows; d.H = H;
    DetTable& t = d.t[0];
    t.ids = c.type_ids; t.grad = c.dtype; t.order = w.order[0]; t.skey = w.skey[0]; t.piece = w.piece[0];
    t.hi = c.type_vocab; t.bcast_T = 0; t.skip = -1;
    UCHECK_RC(det_fold(d, 1, st));
  }
  const int wchunks = (rows + DET_WG_ROWS - 1) / DET_WG_ROWS;
  hipLaunchKernelGGL(pos_linear_wgrad_part_kernel, dim3((H + 255) / 256, wchunks), dim3(256), 0, st, c.d_posfc, c.pos7, w.wpart,
                     rows, H);
  UCHECK_LAUNCH();
  hipLaunchKernelGGL(pos_linear_wgrad_fold_kernel, dim3((H * 8 + 255) / 256), dim3(256), 0, st, w.wpart, c.dWp, c.dbp, wchunks, H);
  UCHECK_LAUNCH();
  return 0;
}

// ---- the C ABI: each entry point fills a call ----
#define TXT_IN(c)                                                                                                                  \
  TxtEmbedCall c;                                                                                                                  \
  c.ids = input_ids; c.pos_ids = position_ids; c.type_ids = type_ids; c.word = word; c.pos = pos; c.type = type; c.gamma = gamma;  \
  c.B = B; c.T = T; c.S = S; c.H = H; c.vocab = vocab; c.max_pos = max_pos; c.type_vocab = type_vocab; c.pos_bcast = pos_bcast;    \
  c.drop = {p_drop, seed, offset, SITE_TXT_EMB}; c.stream = stream
#define TXT_GRADS(c) \
  c.dcat = dcat; c.dword = dword; c.dpos = dpos; c.dtype = dtype; c.dgamma = dgamma; c.dbeta = dbeta; c.ws = ws; c.ws_bytes = ws_bytes

extern "C" int uniter_txt_embed_fwd(const int64_t* input_ids, const int64_t* position_ids, const int64_t* type_ids, const float* word,
                                    const float* pos, const float* type, const float* gamma, const float* beta, float* cat, int B, int T,
                                    int S, int H, int vocab, int max_pos, int type_vocab, int pos_bcast, float p_drop, uint64_t seed,
                                    uint32_t offset, void* stream) {
  TXT_IN(c); c.beta = beta; c.cat = cat;
  return txt_embed_fwd_run(c);
}

// uniter_txt_embed_fwd with delta[B][T][H] added to the word rows (include/uniter_hip.h); delta == NULL is that call itself
extern "C" int uniter_txt_embed_fwd_delta(const int64_t* input_ids, const int64_t* position_ids, const int64_t* type_ids, const float* word,
                                          const float* pos, const float* type, const float* gamma, const float* beta, const float* delta,
                                          float* cat, int B, int T, int S, int H, int vocab, int max_pos, int type_vocab, int pos_bcast,
                                          float p_drop, uint64_t seed, uint32_t offset, void* stream) {
  TXT_IN(c); c.beta = beta; c.delta = delta; c.cat = cat;
  return txt_embed_fwd_run(c);
}

extern "C" int uniter_txt_embed_bwd(const float* dcat, const int64_t* input_ids, const int64_t* position_ids, const int64_t* type_ids,
                                    const float* word, const float* pos, const float* type, const float* gamma, float* dword, float* dpos,
                                    float* dtype, float* dgamma, float* dbeta, int B, int T, int S, int H, int vocab, int max_pos,
                                    int type_vocab, int pos_bcast, float p_drop, uint64_t seed, uint32_t offset, void* ws, size_t ws_bytes,
                                    void* stream) {
  TXT_IN(c); TXT_GRADS(c);
  return txt_embed_bwd_run(c);
}

extern "C" int uniter_txt_embed_bwd_det(const float* dcat, const int64_t* input_ids, const int64_t* position_ids, const int64_t* type_ids,
                                        const float* word, const float* pos, const float* type, const float* gamma, float* dword,
                                        float* dpos, float* dtype, float* dgamma, float* dbeta, int B, int T, int S, int H, int vocab,
                                        int max_pos, int type_vocab, int pos_bcast, float p_drop, uint64_t seed, uint32_t offset, void* ws,
                                        size_t ws_bytes, void* stream) {
  TXT_IN(c); TXT_GRADS(c); c.det = 1;
  return txt_embed_bwd_run(c);
}
#undef TXT_IN
#undef TXT_GRADS

#define IMG_IN(c)                                                                                                              \
  ImgEmbedCall c;                                                                                                              \
  c.imgfc = imgfc; c.pos7 = pos7; c.type_ids = img_type_ids; c.Wp = Wp; c.bp = bp; c.type = type; c.g_i = g_i; c.b_i = b_i;    \
  c.g_p = g_p; c.b_p = b_p; c.g_f = g_f; c.B = B; c.R = R; c.T0 = T0; c.S = S; c.H = H; c.type_vocab = type_vocab;            \
  c.drop = {p_drop, seed, offset, SITE_IMG_EMB}; c.stream = stream
#define IMG_GRADS(c)                                                                                                           \
  c.dcat = dcat; c.stats = const_cast<float*>(stats); c.d_imgfc = d_imgfc; c.d_posfc = d_posfc; c.dWp = dWp; c.dbp = dbp;      \
  c.dtype = dtype; c.dg_i = dg_i; c.db_i = db_i; c.dg_p = dg_p; c.db_p = db_p; c.dg_f = dg_f; c.db_f = db_f; c.ws = ws;       \
  c.ws_bytes = ws_bytes

extern "C" int uniter_img_embed_fwd(const float* imgfc, const float* pos7, const int64_t* img_type_ids, const float* Wp, const float* bp,
                                    const float* type, const float* g_i, const float* b_i, const float* g_p, const float* b_p,
                                    const float* g_f, const float* b_f, float* cat, float* stats, int B, int R, int T0, int S, int H,
                                    int type_vocab, float p_drop, uint64_t seed, uint32_t offset, void* stream) {
  IMG_IN(c); c.b_f = b_f; c.cat = cat; c.stats = stats;
  return img_embed_fwd_run(c);
}

extern "C" int uniter_img_embed_bwd(const float* dcat, const float* imgfc, const float* pos7, const int64_t* img_type_ids, const float* Wp,
                                    const float* bp, const float* type, const float* g_i, const float* b_i, const float* g_p,
                                    const float* b_p, const float* g_f, const float* stats, float* d_imgfc, float* d_posfc, float* dWp,
                                    float* dbp, float* dtype, float* dg_i, float* db_i, float* dg_p, float* db_p, float* dg_f, float* db_f,
                                    int B, int R, int T0, int S, int H, int type_vocab, float p_drop, uint64_t seed, uint32_t offset,
                                    void* ws, size_t ws_bytes, void* stream) {
  IMG_IN(c); IMG_GRADS(c);
  return img_embed_bwd_run(c);
}

extern "C" int uniter_img_embed_bwd_det(const float* dcat, const float* imgfc, const float* pos7, const int64_t* img_type_ids,
                                        const float* Wp, const float* bp, const float* type, const float* g_i, const float* b_i,
                                        const float* g_p, const float* b_p, const float* g_f, const float* stats, float* d_imgfc,
                                        float* d_posfc, float* dWp, float* dbp, float* dtype, float* dg_i, float* db_i, float* dg_p,
                                        float* db_p, float* dg_f, float* db_f, int B, int R, int T0, int S, int H, int type_vocab,
                                        float p_drop, uint64_t seed, uint32_t offset, void* ws, size_t ws_bytes, void* stream) {
  IMG_IN(c); IMG_GRADS(c); c.det = 1;
  return img_embed_bwd_run(c);
}
#undef IMG_IN
#undef IMG_GRADS

extern "C" int uniter_gather_rows(const float* cat, const int64_t* gather_index, float* out, int B, int S,
                                  int Lout, int H, void* stream) {
  UCHECK_ARG(cat && out, "gather_rows: null pointer");
  UCHECK_SHAPE(H % 4 == 0 && (gather_index || Lout <= S), "gather_rows: bad shape");
  if (B * Lout <= 0) return 0;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((B * Lout + 3) / 4), dim3(256), 0, (hipStream_t)stream, cat,
                     gather_index, out, B, S, Lout, H);
  UCHECK_LAUNCH();
  return 0;
}

// uniter_gather_rows with the joint rows' operand copy in the same launch: mode 1 = three bf16 pieces per row ([row][3][H], as
// uniter_split3 with row stride 3 H and piece stride H), mode 2 = one bf16 copy ([row][H], as uniter_cast_bf16).  H up to 1024;
// UNITER_E_SHAPE beyond (the caller then runs the two launches).
extern "C" int uniter_gather_rows_ex(const float* cat, const int64_t* gather_index, float* out, void* out_b16, int mode, int B, int S,
                                     int Lout, int H, void* stream) {
  UCHECK_ARG(cat && out && out_b16 && (mode == 1 || mode == 2), "gather_rows_ex: bad argument");
  UCHECK_SHAPE(H % 4 == 0 && H <= 1024 && (gather_index || Lout <= S), "gather_rows_ex: bad shape (H %% 4, H <= 1024)");
  if (B * Lout <= 0) return 0;
  const dim3 grid((B * Lout + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  unsigned short* ob = (unsigned short*)out_b16;
  const int nv = (H / 4 + 63) / 64;
#define UNITER_GRX(NV_)                                                                                                       \
  if (mode == 1) hipLaunchKernelGGL((gather_rows_ex_kernel<NV_, 1>), grid, block, 0, st, cat, gather_index, out, ob, B, S, Lout, H); \
  else hipLaunchKernelGGL((gather_rows_ex_kernel<NV_, 2>), grid, block, 0, st, cat, gather_index, out, ob, B, S, Lout, H);
  if (nv == 1) { UNITER_GRX(1) } else if (nv == 2) { UNITER_GRX(2) } else if (nv == 3) { UNITER_GRX(3) } else { UNITER_GRX(4) }
#undef UNITER_GRX
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_gather_rows_bwd(const float* dout, const int64_t* gather_index, float* dcat, int B,
                                      int S, int Lout, int H, void* stream) {
  UCHECK_ARG(dout && dcat, "gather_rows_bwd: null pointer");
  UCHECK_SHAPE(H % 4 == 0 && (gather_index || Lout <= S), "gather_rows_bwd: bad shape");
  if (B * S <= 0) return 0;
  hipLaunchKernelGGL(gather_rows_bwd_kernel, dim3((B * S + 3) / 4), dim3(256), 0, (hipStream_t)stream, dout,
                     gather_index, dcat, B, S, Lout, H);
  UCHECK_LAUNCH();
  return 0;
}

// out[m][:] = bias for m < M: the starting value of a product that is then ACCUMULATED on top (C += x W^T by the stream-K
// form of the GEMM, which has no bias epilogue)
__global__ __launch_bounds__(256) void bias_rows_kernel(const float* __restrict__ bias, float* __restrict__ out, int M, int N4) {
  const size_t n = (size_t)M * N4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(bias)[i % N4];
}

extern "C" int uniter_bias_rows(const float* bias, float* out, int M, int N, void* stream) {
  UCHECK_ARG(bias && out && M > 0 && N > 0, "bias_rows: bad argument");
  UCHECK_SHAPE(N % 4 == 0, "bias_rows: N must be a multiple of 4");
  const size_t n = (size_t)M * (N / 4);
  const int nb = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  hipLaunchKernelGGL(bias_rows_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, bias, out, M, N / 4);
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_img_mask_add(const float* feat, const int64_t* img_masks, const float* mask_emb,
                                   float* feat_out, int rows, int D, void* stream) {
  UCHECK_ARG(feat && img_masks && mask_emb && feat_out, "img_mask_add: null pointer");
  UCHECK_SHAPE(D % 4 == 0, "img_mask_add: D must be a multiple of 4");
  const size_t n = (size_t)rows * (D / 4);
  if (n == 0) return 0;
  hipLaunchKernelGGL(img_mask_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, feat, img_masks, mask_emb, feat_out, rows, D / 4);
  UCHECK_LAUNCH();
  return 0;
}
