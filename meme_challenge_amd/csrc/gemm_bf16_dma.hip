// bf16-resident GEMM for gfx950, second generation: operands go global -> LDS by LDS-DMA
// (buffer_load_dwordx4 ... lds), no staging registers and no ds_write traffic; a ring of LDS stages with
// counted s_waitcnt vmcnt(N) and one raw s_barrier per 64-deep k-tile keeps two k-tiles of loads in flight
// across the barrier; the accumulator is held TRANSPOSED (MFMA A operand = the weight rows, B operand = the
// activation rows) so that each lane owns one output row and 4 consecutive columns per register group:
// fp32 outputs leave as 16-byte stores, bf16 outputs as 16-byte stores after a v_permlane32_swap of
// neighbouring groups, the bias / residual / gelu' operands arrive as 16- or 8-byte loads.
//
// Replaces cuBLAS behind nn.Linear forward and input-gradient products of model/layer.py:76-78 (query / key /
// value), :112 (attention output), :140 (intermediate) and :153 (output) in the bf16 mode.
//
// LDS images (per operand and stage, 64 k per k-tile): bf16_tile.h, Dma.
//
// Split-K: a tile's k-range may be cut into `nsplit` pieces computed by different workgroups; piece s
// stores its fp32 partial tile to C + s * c_split_stride (piece 0 applies the epilogue); the CONSUMER
// (LayerNorm forward / backward row pass) adds the slabs -- no atomics, no in-kernel hand-off.
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "bf16_tile.h"
#include "gemm_internal.h"
#include "switches.h"
#include "riders.h"

namespace {

typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));

struct GArgsD {
  int M, N, K;
  const void* A; int lda;      // bf16
  const void* B; int ldb;      // bf16
  float* C; int ldc;           // fp32 output (optional); slab s of a split-K launch at C + s * c_split_stride
  long c_split_stride;
  unsigned short* Cb; int ldcb;   // bf16 output (optional)
  int epi;
  const float* bias;
  const void* aux_in; int aux_in_bf16;
  void* aux_out; int aux_out_bf16;
  int ld_aux;
  int tiles_m, tiles_n, band_h, nsplit;
  unsigned long long* stamp;    // optional {first start, last end} slot (common.h)
  int prio;      // wave priority (common.h: LaunchOpts::prio)
  int dbg;       // measurement builds only (tests/tools/gemm_v2_lab.py): 1 = drop every output store, 2 = skip the k-loop
};

constexpr int KT = 64;                 // k-tile depth

// ---- MFMA operand fragments ---------------------------------------------------------------------------
// 8 consecutive k (k16-step ks, lane half h) of row / column 32 blk + i5 of the operand image.
// k-contiguous images are read by plain 16-byte LDS loads (the compiler schedules and counts them).
// k-major images are read by ds_read_b64_tr_b16 as inline assembly with hand-counted lgkmcnt waits (bf16_tile.h says why).
// Differs from Frag3 / Frag16 / FragP: 32-row blocks of a 64-deep image, four k16-steps, two blocks per wave.
template <int R, bool KM>
struct Frag {
  int o0, o1;         // k-contiguous: row byte offset, swizzle key
  unsigned ka[4];     // k-contiguous, asm form: image-relative byte address of k16-step ks (first block of the wave)
  unsigned tr[2][2];  // k-major: image-relative byte address of the (first, second) read of the wave's two blocks
  __device__ __forceinline__ void init(int i5, int h, int blk0) {
    if constexpr (!KM) {
      o0 = i5 * 128; o1 = (h ^ ((i5 >> 1) & 7));      // (xor with 2 ks below)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) ka[ks] = o0 + blk0 * 32 * 128 + (((2 * ks) ^ o1) << 4);
    } else {
      const int l16 = i5 & 15, q = l16 >> 2, p = l16 & 3;
      const int s1 = (q << 2) | (2 * h), s2 = s1 | 1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int r0 = (blk0 + t) * 32;
        const int seg = r0 >> 7;
        const int c = ((r0 & 127) >> 3) + 2 * (i5 >> 4) + (p >> 1);
        const int base = (8 * h + q) * (R * 2) + 8 * (p & 1) + seg * 256;
        tr[t][0] = base + ((c ^ s1) << 4);
        tr[t][1] = base + 4 * (R * 2) + ((c ^ s2) << 4);
      }
    }
  }
  __device__ __forceinline__ bf16x8 read(const unsigned char* img, int blk, int ks) const {
    static_assert(!KM, "k-major images are read through read_tr");
    const int off = o0 + blk * 32 * 128 + (((2 * ks) ^ o1) << 4);
    return *reinterpret_cast<const bf16x8*>(img + off);
  }
  // asm form of read() for the kernels whose other operand is k-major: one kind of LDS read per loop, all counted by hand
  template <int KS, int T>
  __device__ __forceinline__ void read_asm(unsigned img_addr, u32x4_t& out) const {
    lds_read_b128<T * 32 * 128>(out, img_addr + ka[KS]);
  }
  // raw halves of the fragment of block t, k16-step KS; complete only after the caller's lgkmcnt wait
  template <int KS>
  __device__ __forceinline__ void read_tr(unsigned img_addr, int t, u32x2_t& lo, u32x2_t& hi) const {
    lds_read_tr<KS * 16 * R * 2>(lo, img_addr + tr[t][0]);
    lds_read_tr<KS * 16 * R * 2>(hi, img_addr + tr[t][1]);
  }
};

// differs from bf16_tile.h's lgkm_wait + tie: the wait names its destinations itself
template <int N>
__device__ __forceinline__ void wait_lgkm(u32x2_t& a, u32x2_t& b, u32x2_t& c, u32x2_t& d, u32x4_t& e, u32x4_t& f) {
#if defined(__HIP_DEVICE_COMPILE__)
  // naming every destination "+v" ties their first use to this wait (and keeps register-only MFMAs below it)
  asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f) : "n"(N) : "memory");
#endif
}

// BM x BN tile, one 64 x 64 sub-tile (2 x 2 accumulator blocks of 32 x 32) per wave, ST LDS stages.
// SWAP: accumulator transposed (lane = output row); !SWAP: lane = output column (fp32 atomics for C +=).
template <int N>
__device__ __forceinline__ void wait_lgkm8(u32x2_t& a, u32x2_t& b, u32x2_t& c, u32x2_t& d, u32x2_t& e, u32x2_t& f,
                                           u32x2_t& g, u32x2_t& h) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : "n"(N) : "memory");
#endif
}

// one work item w = (tile, k-piece) of the product g
// what a tile of a launch with riders hands back / is asked for (gemm_dma_wgrad_group_kernel<.., XTR = true>)
struct TileRider {
  float* colsum_out;   // non-null: also sum this tile's A operand (k-major) over k, out[m] += .. (the tile's first 64-column strip only)
  int colsum_M;
  float ss;            // out: this lane's sum of squares of what the tile stored (and of the column sums it wrote)
};

template <int BM, int BN, bool AKM, bool BKM, bool SWAP, int ST, int EPI, bool XTR = false>
__device__ __forceinline__ void gemm_dma_tile(const GArgsD& g, const int w, unsigned char* smem, TileRider* rt = nullptr) {
#if defined(__HIP_DEVICE_COMPILE__)      // device-only builtins / asm: the host pass gets an empty body (it only needs the launch stub)
  constexpr int WNN = BN / 64, NW = (BM / 64) * WNN;
  constexpr int IMG_A = BM * 128, IMG_B = BN * 128, STAGE = IMG_A + IMG_B;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i5 = lane & 31, h = lane >> 5;
  const int wm = wave / WNN, wn = wave % WNN;

  const int tile = w / g.nsplit, piece = w - tile * g.nsplit;
  int tmi, tni;
  tile_coords(tile, g.tiles_m, g.tiles_n, g.band_h, tmi, tni);
  const int m0 = tmi * BM, n0 = tni * BN;
  const int nk = (g.K + KT - 1) / KT;
  const int kb = (int)((long)nk * piece / g.nsplit), ke = (g.dbg & 2) ? kb : (int)((long)nk * (piece + 1) / g.nsplit);

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(g.A), 0, (AKM ? g.K : g.M) * g.lda * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(g.B), 0, (BKM ? g.K : g.N) * g.ldb * 2, 0x00020000);
  Dma<BM, AKM, NW, KT> da;
  Dma<BN, BKM, NW, KT> db;
  da.offsets(g.lda, m0, wave, lane);
  db.offsets(g.ldb, n0, wave, lane);
  const int kstepA = Dma<BM, AKM, NW, KT>::kstep(g.lda), kstepB = Dma<BN, BKM, NW, KT>::kstep(g.ldb);
  constexpr int NDMA = Dma<BM, AKM, NW, KT>::NI + Dma<BN, BKM, NW, KT>::NI;

  Frag<BM, AKM> fa;
  Frag<BN, BKM> fb;
  fa.init(i5, h, wm * 2);
  fb.init(i5, h, wn * 2);
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) acc[a][b][rr] = 0.f;
  // riders: the column sums of the k-major A operand over k, as ones . A on the matrix pipe (two more MFMAs per k16-step for
  // the waves that hold the tile's first 64 columns, in the tiles of the first tile column)
  f32x16 acc1[XTR ? 2 : 1];
  bool colsum = false;
  if constexpr (XTR) {
    colsum = rt->colsum_out != nullptr && n0 == 0 && wn == 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) acc1[a][rr] = 0.f;
  }
  const bf16x8 ones8 = __builtin_bit_cast(bf16x8, u32x4_t{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u});

#define ISSUE(KTILE, STG)                                                        \
  do {                                                                           \
    da.issue(rsA, smem + (STG) * STAGE, (KTILE) * kstepA, wave);                 \
    db.issue(rsB, smem + (STG) * STAGE + IMG_A, (KTILE) * kstepB, wave);         \
  } while (0)

// One k-tile: four k16-steps, fragments of step s+1 read while step s multiplies.  LDS instructions per step
// of a k-major B: 2 + 4 asm reads and no compiler-counted LDS read at all (a compiler read between them would be
// waited for with a count that ignores the asm reads, i.e. far too early in the queue); every asm statement
// clobbers "memory", so the issue order is the program order and lgkmcnt(6) at step s leaves exactly step
// s+1's six reads outstanding.
#define RD_STEP(KS, BUF)                                                                                 \
  {                                                                                                      \
    if constexpr (AKM && BKM) {           /* weight gradients: both operands k-major, 8 transposed reads per step */ \
      fa.template read_tr<KS>(sAaddr, 0, rA[BUF][0][0], rA[BUF][0][1]);                                  \
      fa.template read_tr<KS>(sAaddr, 1, rA[BUF][1][0], rA[BUF][1][1]);                                  \
      fb.template read_tr<KS>(sBaddr, 0, rb[BUF][0][0], rb[BUF][0][1]);                                  \
      fb.template read_tr<KS>(sBaddr, 1, rb[BUF][1][0], rb[BUF][1][1]);                                  \
    } else if constexpr (BKM) {                                                                          \
      fa.template read_asm<KS, 0>(sAaddr, ra[BUF][0]);                                                   \
      fa.template read_asm<KS, 1>(sAaddr, ra[BUF][1]);                                                   \
      fb.template read_tr<KS>(sBaddr, 0, rb[BUF][0][0], rb[BUF][0][1]);                                  \
      fb.template read_tr<KS>(sBaddr, 1, rb[BUF][1][0], rb[BUF][1][1]);                                  \
    } else {                                                                                             \
      xa[BUF][0] = fa.read(sA, wm * 2, KS); xa[BUF][1] = fa.read(sA, wm * 2 + 1, KS);                    \
      xb[BUF][0] = fb.read(sB, wn * 2, KS); xb[BUF][1] = fb.read(sB, wn * 2 + 1, KS);                    \
    }                                                                                                    \
  }
#define MM_STEP(BUF, NLATER)                                                                             \
  {                                                                                                      \
    if constexpr (AKM && BKM) {                                                                          \
      wait_lgkm8<(NLATER) ? 8 : 0>(rA[BUF][0][0], rA[BUF][0][1], rA[BUF][1][0], rA[BUF][1][1],           \
                                   rb[BUF][0][0], rb[BUF][0][1], rb[BUF][1][0], rb[BUF][1][1]);          \
      xa[BUF][0] = join_halves(rA[BUF][0][0], rA[BUF][0][1]);                                            \
      xa[BUF][1] = join_halves(rA[BUF][1][0], rA[BUF][1][1]);                                            \
      xb[BUF][0] = join_halves(rb[BUF][0][0], rb[BUF][0][1]);                                            \
      xb[BUF][1] = join_halves(rb[BUF][1][0], rb[BUF][1][1]);                                            \
    } else if constexpr (BKM) {                                                                          \
      wait_lgkm<NLATER>(rb[BUF][0][0], rb[BUF][0][1], rb[BUF][1][0], rb[BUF][1][1], ra[BUF][0], ra[BUF][1]); \
      xa[BUF][0] = __builtin_bit_cast(bf16x8, ra[BUF][0]);                                               \
      xa[BUF][1] = __builtin_bit_cast(bf16x8, ra[BUF][1]);                                               \
      xb[BUF][0] = join_halves(rb[BUF][0][0], rb[BUF][0][1]);                                            \
      xb[BUF][1] = join_halves(rb[BUF][1][0], rb[BUF][1][1]);                                            \
    }                                                                                                    \
    _Pragma("unroll") for (int a = 0; a < 2; ++a)                                                        \
    _Pragma("unroll") for (int b = 0; b < 2; ++b)                                                        \
      acc[a][b] = SWAP ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(xb[BUF][b], xa[BUF][a], acc[a][b], 0, 0, 0) \
                       : __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[BUF][a], xb[BUF][b], acc[a][b], 0, 0, 0); \
    if constexpr (XTR && AKM && BKM && SWAP) {                                                           \
      if (colsum) {                                                                                      \
        acc1[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones8, xa[BUF][0], acc1[0], 0, 0, 0);          \
        acc1[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones8, xa[BUF][1], acc1[1], 0, 0, 0);          \
      }                                                                                                  \
    }                                                                                                    \
  }
#define COMPUTE(STG)                                                                                     \
  {                                                                                                      \
    const unsigned char* sA = smem + (STG) * STAGE;                                                      \
    const unsigned char* sB = sA + IMG_A;                                                                \
    const unsigned sAaddr = lds0 + (STG) * STAGE, sBaddr = sAaddr + IMG_A;                               \
    (void)sA; (void)sB; (void)sAaddr; (void)sBaddr;                                                      \
    bf16x8 xa[2][2], xb[2][2];                                                                           \
    u32x2_t rb[2][2][2], rA[2][2][2];                                                                    \
    u32x4_t ra[2][2];                                                                                    \
    RD_STEP(0, 0)                                                                                        \
    RD_STEP(1, 1) MM_STEP(0, 6)                                                                          \
    RD_STEP(2, 0) MM_STEP(1, 6)                                                                          \
    RD_STEP(3, 1) MM_STEP(0, 6)                                                                          \
    MM_STEP(1, 0)                                                                                        \
  }

  if (kb < ke) {
    if constexpr (ST == 3) {
      ISSUE(kb, 0);
      if (kb + 1 < ke) ISSUE(kb + 1, 1);
      int kt = kb;
#define STEP3(STG)                                                               \
  {                                                                              \
    if (kt + 1 < ke) wait_vm<NDMA>(); else wait_vm<0>();                         \
    __builtin_amdgcn_s_barrier();                                                \
    __builtin_amdgcn_sched_barrier(0);                                           \
    if (kt + 2 < ke) ISSUE(kt + 2, ((STG) + 2) % 3);                             \
    COMPUTE(STG)                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                           \
  }
      while (true) {
        STEP3(0) if (++kt == ke) break;
        STEP3(1) if (++kt == ke) break;
        STEP3(2) if (++kt == ke) break;
      }
#undef STEP3
    } else {
      ISSUE(kb, 0);
      int kt = kb;
#define STEP2(STG)                                                               \
  {                                                                              \
    wait_vm<0>();                                                                \
    __builtin_amdgcn_s_barrier();                                                \
    __builtin_amdgcn_sched_barrier(0);                                           \
    if (kt + 1 < ke) ISSUE(kt + 1, 1 - (STG));                                   \
    COMPUTE(STG)                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                           \
  }
      while (true) {
        STEP2(0) if (++kt == ke) break;
        STEP2(1) if (++kt == ke) break;
      }
#undef STEP2
    }
  }
#undef ISSUE
#undef COMPUTE
#undef RD_STEP
#undef MM_STEP

  // ---------------------------------------------------------------- epilogue ----
  // The epilogue kind is a template parameter (one code path per kernel: the unrolled blocks are long), and every
  // load of the tile (bias, aux operand of all four blocks) is issued before the first store: loads and stores share
  // vmcnt, so a load result needed behind stores in flight would drain them (s_waitcnt vmcnt(0)).
  float* Cp = g.C ? g.C + (size_t)piece * g.c_split_stride : nullptr;
  const int keep = (g.dbg & 1) ? 0 : 1;     // zero records: the range check drops the stores, the instruction stream stays
  const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(Cp, 0, Cp ? keep * g.M * g.ldc * 4 : 0, 0x00020000);
  if constexpr (SWAP) {
    const bool first = piece == 0;          // the other k-pieces store plain partial sums
    const __amdgpu_buffer_rsrc_t rsCb = __builtin_amdgcn_make_buffer_rsrc(g.Cb, 0, g.Cb ? keep * g.M * g.ldcb * 2 : 0, 0x00020000);
    const int axe_i = g.aux_in_bf16 ? 2 : 4, axe_o = g.aux_out_bf16 ? 2 : 4;
    const __amdgpu_buffer_rsrc_t rsI = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(g.aux_in), 0, g.aux_in ? g.M * g.ld_aux * axe_i : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(
        g.aux_out, 0, g.aux_out ? keep * g.M * g.ld_aux * axe_o : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsBias = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(g.bias), 0, g.bias ? g.N * 4 : 0, 0x00020000);
    constexpr bool HAS_BIAS = EPI == UNITER_EPI_BIAS || EPI == UNITER_EPI_BIAS_GELU || EPI == UNITER_EPI_BIAS_GELU_D;
    constexpr bool HAS_AUX = EPI == UNITER_EPI_DGELU || EPI == UNITER_EPI_ADD || EPI == UNITER_EPI_MUL;
    constexpr bool TWO = EPI == UNITER_EPI_BIAS_GELU_D || EPI == UNITER_EPI_BIAS_GELU;
    // register group gq of block (a, b) holds columns nb(b) + 8 gq + 4 h .. + 3 of row m(a)
    f32x4 bv[HAS_BIAS ? 2 : 1][4], ax[HAS_AUX ? 2 : 1][HAS_AUX ? 2 : 1][4];
    if (HAS_BIAS && first) {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int n = n0 + wn * 64 + b * 32 + 8 * gq + 4 * h;
          bv[b][gq] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsBias, n < g.N ? n * 4 : OOB, 0, 0));
        }
    }
    if (HAS_AUX && first) {
      // one uniform branch around ALL loads (a per-load branch makes hipcc wait vmcnt(0) after each of them)
      if (g.aux_in_bf16) {
        u32x2_t raw[2][2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const int m = m0 + wm * 64 + a * 32 + i5;
              const int n = n0 + wn * 64 + b * 32 + 8 * gq + 4 * h;
              raw[a][b][gq] = __builtin_amdgcn_raw_buffer_load_b64(rsI, n < g.N ? (m * g.ld_aux + n) * 2 : OOB, 0, 0);
            }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const u32x2_t t = raw[a][b][gq];
              ax[a][b][gq] = f32x4{bf_lo(t[0]), bf_hi(t[0]), bf_lo(t[1]), bf_hi(t[1])};
            }
      } else {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const int m = m0 + wm * 64 + a * 32 + i5;
              const int n = n0 + wn * 64 + b * 32 + 8 * gq + 4 * h;
              ax[a][b][gq] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsI, n < g.N ? (m * g.ld_aux + n) * 4 : OOB, 0, 0));
            }
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int m = m0 + wm * 64 + a * 32 + i5;                 // this lane's output row
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int nb = n0 + wn * 64 + b * 32;                   // first column of the block
        f32x16& v = acc[a][b];
        f32x16 x2;     // second output (gelu' or the pre-activation)
        if (first) {
          if constexpr (HAS_BIAS) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) v[rr] += bv[b][rr >> 2][rr & 3];
          }
          if constexpr (EPI == UNITER_EPI_BIAS_GELU_D) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) { float y_, d_; gelu_pair_fast(v[rr], y_, d_); v[rr] = y_; x2[rr] = d_; }
          } else if constexpr (EPI == UNITER_EPI_BIAS_GELU) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) { x2[rr] = v[rr]; v[rr] = gelu_erf(v[rr]); }
          } else if constexpr (EPI == UNITER_EPI_MUL) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) v[rr] *= ax[a][b][rr >> 2][rr & 3];
          } else if constexpr (EPI == UNITER_EPI_ADD) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) v[rr] += ax[a][b][rr >> 2][rr & 3];
          } else if constexpr (EPI == UNITER_EPI_DGELU) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) v[rr] *= dgelu_erf(ax[a][b][rr >> 2][rr & 3]);
          }
        }
        // fp32 outputs: one 16-byte store per register group
        if (Cp) {
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            const int n = nb + 8 * gq + 4 * h;
            const f32x4 o = {v[4 * gq], v[4 * gq + 1], v[4 * gq + 2], v[4 * gq + 3]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, o), rsC, n < g.N ? (m * g.ldc + n) * 4 : OOB, 0, 0);
            if constexpr (XTR) {      // only what was stored counts (a k-major operand's overhang columns read the next row, not zeros)
              const float s4 = (o[0] * o[0] + o[1] * o[1]) + (o[2] * o[2] + o[3] * o[3]);
              rt->ss += (m < g.M && n < g.N) ? s4 : 0.f;
            }
          }
        }
        if (TWO && !g.aux_out_bf16) {
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            const int n = nb + 8 * gq + 4 * h;
            const f32x4 o = {x2[4 * gq], x2[4 * gq + 1], x2[4 * gq + 2], x2[4 * gq + 3]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, o), rsX, n < g.N ? (m * g.ld_aux + n) * 4 : OOB, 0, 0);
          }
        }
        // bf16 outputs: groups (gq, gq + 1) exchanged between the lane halves -> 8 consecutive columns per lane
        if (g.Cb || (TWO && g.aux_out_bf16)) {
#pragma unroll
          for (int gp = 0; gp < 4; gp += 2) {
            const int n8 = nb + 8 * (gp + h);
            const bool ok = n8 < g.N;
            if (g.Cb) {
              unsigned a0 = pack2(v[4 * gp], v[4 * gp + 1]), a1 = pack2(v[4 * gp + 2], v[4 * gp + 3]);
              unsigned b0 = pack2(v[4 * gp + 4], v[4 * gp + 5]), b1 = pack2(v[4 * gp + 6], v[4 * gp + 7]);
              const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
              const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
              const u32x4_t o = {r0[0], r1[0], r0[1], r1[1]};
              __builtin_amdgcn_raw_buffer_store_b128(o, rsCb, ok ? (m * g.ldcb + n8) * 2 : OOB, 0, 0);
            }
            if (TWO && g.aux_out_bf16) {
              unsigned a0 = pack2(x2[4 * gp], x2[4 * gp + 1]), a1 = pack2(x2[4 * gp + 2], x2[4 * gp + 3]);
              unsigned b0 = pack2(x2[4 * gp + 4], x2[4 * gp + 5]), b1 = pack2(x2[4 * gp + 6], x2[4 * gp + 7]);
              const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
              const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
              const u32x4_t o = {r0[0], r1[0], r0[1], r1[1]};
              __builtin_amdgcn_raw_buffer_store_b128(o, rsX, ok ? (m * g.ld_aux + n8) * 2 : OOB, 0, 0);
            }
          }
        }
      }
    }
    if constexpr (XTR) {
      if (colsum && h == 0) {
        // every accumulator row of the ones-product holds the same sums: lanes 0..31 own column m of row block a
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const int m = m0 + wm * 64 + a * 32 + i5;
          if (m < rt->colsum_M) {
            const float o = rt->colsum_out[m] + acc1[a][0];
            rt->colsum_out[m] = o;
            rt->ss = __builtin_fmaf(o, o, rt->ss);
          }
        }
      }
    }
  } else {
    // lane = output column: C += by fp32 atomics (two 128-byte row segments per wave-instruction)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = n0 + wn * 64 + b * 32 + i5;
        const int r0 = m0 + wm * 64 + a * 32 + 4 * h;
        int p_ = col < g.N ? (r0 * g.ldc + col) * 4 : OOB;
        const int stC = g.ldc * 4;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc[a][b][rr], rsC, p_, 0, 0);
          p_ += ((rr & 3) == 3 ? 5 : 1) * stC;
        }
      }
  }
#endif
}

template <int BM, int BN, bool AKM, bool BKM, bool SWAP, int ST, int EPI>
__global__ __launch_bounds__(64 * (BM / 64) * (BN / 64), (ST * (BM + BN) * 128 <= 80 * 1024 ? 2 : 1)) void gemm_dma_kernel(const GArgsD g) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[ST * (BM + BN) * 128];
  // work item -> (tile, k-piece), banded tile order inside an XCD's chunk
  const int w = xcd_work_item(g.tiles_m * g.tiles_n * g.nsplit);
  if (w < 0) return;
  set_wave_prio(g.prio);
  stamp_begin(g.stamp);
  gemm_dma_tile<BM, BN, AKM, BKM, SWAP, ST, EPI>(g, w, smem);
  stamp_end(g.stamp);
}

// The weight gradients of one encoder layer as ONE launch: up to four products dW_p[M_p, N_p] += A_p^T B_p (both
// operands k-major, K = rows of the batch) whose 128 x 128 tiles are numbered through.  A layer of UNITER-base has
// 144 + 144 + 108 + 36 = 432 tiles for the chip's 512 workgroup slots: every tile is owned by one workgroup over
// the whole K, so there are no partial sums to exchange (no atomics, no slabs) and dW += is a plain
// read-modify-write in the epilogue (UNITER_EPI_ADD with the output as its own aux operand).
struct GGroupD {
  GArgsD p[4];
  int start[5];     // first work item of product p; start[n..4] = total
  uniter_x3_riders_t x;   // riders (kernels instantiated with XTR only): include/uniter_hip.h
};

template <int ST, bool ACC, bool XTR = false>
__global__ __launch_bounds__(256, (ST == 2 ? 2 : 1)) void gemm_dma_wgrad_group_kernel(const GGroupD G) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[ST * 256 * 128];
  // riders (XTR, round 5): the column-reduction items of this workgroup first -- dealt from the END of the grid, where the
  // workgroups with one tile less sit -- then, per tile, the sum of squares of what it stored (and, for product 0's first
  // tile column, the column sums of its A operand)
  double wss = 0.0;
  if constexpr (XTR) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = (int)gridDim.x - 1 - (int)blockIdx.x; r < G.x.nred; r += (int)gridDim.x)
      wss += (double)riders_reduce_item(G.x, r, wave, lane);
  }
  // a grid smaller than the tile count (G.max_wgs): the workgroup walks its XCD's chunk in strides of the grid -- fewer
  // workgroups of this launch resident per CU, so the input-gradient chain on the other stream finds free slots
  bool any = false;
  for (int round = 0;; ++round) {
    const int w = xcd_work_item(G.start[4], round);
    if (w < 0) break;
    if (!any) stamp_begin(G.p[0].stamp);
    else __syncthreads();                 // the slowest wave has left the previous tile's last LDS stage
    any = true;
    const int p = (w >= G.start[1]) + (w >= G.start[2]) + (w >= G.start[3]);
    // ACC: dW += (the output is its own aux operand); !ACC: dW = (the first backward pass after an optimizer step that left
    // the gradient uncleared: no read of dW, and the optimizer wrote no zeros -- uniter_model_set_wgrad_overwrite)
    if constexpr (XTR) {
      TileRider rt;
      rt.colsum_out = p == 0 ? G.x.colsum_out : nullptr; rt.colsum_M = G.p[0].M; rt.ss = 0.f;
      gemm_dma_tile<128, 128, true, true, true, ST, ACC ? UNITER_EPI_ADD : UNITER_EPI_NONE, true>(G.p[p], w - G.start[p], smem, &rt);
      wss += (double)rt.ss;
    } else {
      gemm_dma_tile<128, 128, true, true, true, ST, ACC ? UNITER_EPI_ADD : UNITER_EPI_NONE>(G.p[p], w - G.start[p], smem);
    }
  }
  if constexpr (XTR) riders_store_ssq(G.x, wss, threadIdx.x >> 6, threadIdx.x & 63);
  if (any) stamp_end(G.p[0].stamp);
}

template <int BM>
void plan_tiles(GArgsD& g, int BN) {
  g.tiles_m = (g.M + BM - 1) / BM;
  g.tiles_n = (g.N + BN - 1) / BN;
  g.band_h = l2_band_height((long)BM * g.K * 2, g.tiles_m);
}

template <int BM, int BN, bool AKM, bool BKM, bool SWAP, int ST, int EPI>
int launch_d(GArgsD g, hipStream_t st) {
  plan_tiles<BM>(g, BN);
  const int nwork = g.tiles_m * g.tiles_n * g.nsplit;
  const int grid = (nwork + 7) / 8 * 8;
  hipLaunchKernelGGL((gemm_dma_kernel<BM, BN, AKM, BKM, SWAP, ST, EPI>), dim3(grid), dim3(64 * (BM / 64) * (BN / 64)), 0, st, g);
  UCHECK_LAUNCH();
  return 0;
}

// weight gradients (both operands k-major): 128 x 128 tiles only
template <bool SWAP>
int dispatch_wgrad(int cfg, const GArgsD& g, hipStream_t st) {
  switch (cfg) {
    case 1: return launch_d<128, 128, true, true, SWAP, 2, UNITER_EPI_NONE>(g, st);
    case 4: return launch_d<128, 128, true, true, SWAP, 3, UNITER_EPI_NONE>(g, st);
    default: uniter_set_error("gemm_bf16v2: weight-gradient layout runs cfg 1 or 4 (got %d)", cfg); return UNITER_E_ARG;
  }
}

template <bool BKM, bool SWAP, int EPI>
int dispatch_cfg(int cfg, const GArgsD& g, hipStream_t st) {
  switch (cfg) {
    case 1: return launch_d<128, 128, false, BKM, SWAP, 2, EPI>(g, st);     // 4 waves, two workgroups per CU
    case 2: return launch_d<128, 256, false, BKM, SWAP, 3, EPI>(g, st);     // 8 waves, one workgroup per CU
    case 3: return launch_d<256, 128, false, BKM, SWAP, 3, EPI>(g, st);
    case 4: return launch_d<128, 128, false, BKM, SWAP, 3, EPI>(g, st);     // 4 waves, one workgroup per CU, deeper ring
    case 5: return launch_d<64, 128, false, BKM, SWAP, 2, EPI>(g, st);      // 2 waves: twice the tiles for the few-tile shapes (N = hidden)
    default: uniter_set_error("gemm_bf16v2: bad cfg %d (1..5)", cfg); return UNITER_E_ARG;
  }
}

template <bool BKM>
int dispatch_epi(int cfg, const GArgsD& g, hipStream_t st) {
  switch (g.epi) {
    case UNITER_EPI_NONE: return dispatch_cfg<BKM, true, UNITER_EPI_NONE>(cfg, g, st);
    case UNITER_EPI_BIAS: return dispatch_cfg<BKM, true, UNITER_EPI_BIAS>(cfg, g, st);
    case UNITER_EPI_BIAS_GELU: return dispatch_cfg<BKM, true, UNITER_EPI_BIAS_GELU>(cfg, g, st);
    case UNITER_EPI_DGELU: return dispatch_cfg<BKM, true, UNITER_EPI_DGELU>(cfg, g, st);
    case UNITER_EPI_ADD: return dispatch_cfg<BKM, true, UNITER_EPI_ADD>(cfg, g, st);
    case UNITER_EPI_BIAS_GELU_D: return dispatch_cfg<BKM, true, UNITER_EPI_BIAS_GELU_D>(cfg, g, st);
    case UNITER_EPI_MUL: return dispatch_cfg<BKM, true, UNITER_EPI_MUL>(cfg, g, st);
    default: uniter_set_error("gemm_bf16v2: bad epilogue %d", g.epi); return UNITER_E_ARG;
  }
}

}  // namespace

// cfg: 1 = 128x128 (2 stages), 2 = 128x256, 3 = 256x128, 4 = 128x128 (3 stages), 5 = 64x128 (2 waves); 0 = choose;
// 6 / 7 / 8 = the persistent loader / compute kernels of gemm_bf16_p.hip (128 x 128 / 128 x 256 / 128 x 192 tiles).
// beta = 1: C += A.B through fp32 atomics (lane = column orientation; no epilogue, no bf16 output).
int gemm_bf16v2_run(int cfg, const GemmCall& c, const LaunchOpts& lo) {
  const int M = c.M, N = c.N, K = c.K, a_kmajor = c.A.kmajor, b_kmajor = c.B.kmajor, nsplit = c.nsplit, beta = c.beta;
  UCHECK_RC(gemm_check_epilogue("gemm_bf16v2", c, GEMM_EPI_ALL, true));
  UCHECK_ARG(M > 0 && N > 0 && K > 0 && c.A.p && c.B.p && (c.C || c.Ccopy), "gemm_bf16v2: bad argument");
  UCHECK_ARG(!c.A.piece_stride && !c.B.piece_stride && !c.ps_copy && !c.sk_ws, "gemm_bf16v2: bf16 operands have no pieces, and no launch of this family takes a workspace");
  UCHECK_ARG(c.epi >= 0 && c.epi <= UNITER_EPI_MUL, "gemm_bf16v2: bad epilogue %d", c.epi);
  UCHECK_ARG(!a_kmajor || (b_kmajor && c.epi == UNITER_EPI_NONE && !c.Ccopy),
             "gemm_bf16v2: A k-major only as the weight-gradient layout (both operands k-major, no epilogue, fp32 output)");
  UCHECK_ARG(nsplit >= 1 && nsplit <= 8 && (nsplit == 1 || (c.C && !c.Ccopy && !beta && c.c_split_stride >= (long)M * c.ldc)),
             "gemm_bf16v2: split-K needs fp32 slabs (no bf16 output, no accumulate)");
  UCHECK_ARG(!beta || (c.C && !c.Ccopy && c.epi == UNITER_EPI_NONE), "gemm_bf16v2: C += has no epilogue and no bf16 copy");
  UCHECK_SHAPE((K % KT == 0 || (a_kmajor && b_kmajor)) && c.A.ld % 8 == 0 && c.B.ld % 8 == 0 && N % 8 == 0 && (!a_kmajor || M % 8 == 0) &&
               ((uintptr_t)c.A.p & 15) == 0 && ((uintptr_t)c.B.p & 15) == 0 && gemm_side_buffers_aligned(c),
               "gemm_bf16v2: K %% 64, N %% 8, leading dimensions %% 8 (bf16) / %% 4 (fp32) and 16-byte aligned "
               "buffers required (M=%d N=%d K=%d)", M, N, K);
  UCHECK_SHAPE((size_t)(a_kmajor ? K : M + 256) * c.A.ld * 2 < (1ull << 31) && (size_t)(b_kmajor ? K + 64 : N + 256) * c.B.ld * 2 < (1ull << 31) &&
               gemm_f32_side_in_range(c, 256), "gemm_bf16v2: operand beyond 31-bit offsets");
  if ((cfg & 0xff) >= 6) {
    UCHECK_ARG(!a_kmajor && !beta, "gemm_bf16v2: cfg %d (persistent kernels) runs forward / input-gradient layouts without accumulate "
               "(weight gradients: uniter_wgrad_bf16_group, cfg 7)", cfg & 0xff);
    return gemm_b1p_run(cfg & 0xff, c, lo);
  }
  UCHECK_ARG(!c.colpart, "gemm_bf16v2: column partials ride on the persistent kernels (cfg 7)");
  GArgsD g = {M, N, K, c.A.p, c.A.ld, c.B.p, c.B.ld, c.C, c.ldc, c.c_split_stride, (unsigned short*)c.Ccopy, c.ld_copy, c.epi, c.bias,
              c.aux_in, c.aux_in_bf16, c.aux_out, c.aux_out_bf16, c.ld_aux, /*tiles_m, tiles_n*/ 0, 0, /*band_h*/ 1, nsplit,
              lo.stamp, lo.prio, /*dbg*/ cfg >> 8};
  cfg &= 0xff;
  if (cfg == 0) {
    // few tiles and one k-piece (the attention-output products: 126 tiles of 128 x 128 for 256 CUs): 64 x 128 tiles,
    // twice the workgroups (12.0 -> 10.6 us forward, 11.7 -> 10.0 us input gradient; profiles/r02_gemm_bf16_v2.txt)
    const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
    cfg = (!a_kmajor && nsplit == 1 && tiles <= 160) ? 5 : 1;
  }
  hipStream_t st = (hipStream_t)c.stream;
  if (a_kmajor) return beta ? dispatch_wgrad<false>(cfg, g, st) : dispatch_wgrad<true>(cfg, g, st);
  if (beta) return b_kmajor ? dispatch_cfg<true, false, UNITER_EPI_NONE>(cfg, g, st) : dispatch_cfg<false, false, UNITER_EPI_NONE>(cfg, g, st);
  return b_kmajor ? dispatch_epi<true>(cfg, g, st) : dispatch_epi<false>(cfg, g, st);
}

// dW_p[M_p, N_p] += A_p^T B_p for up to four products of one reduction length K (A_p [K, M_p], B_p [K, N_p] bf16,
// dW_p fp32 with leading dimension N_p), one launch; cfg 1 = two LDS stages (two workgroups per CU), 4 = three.
// lo: the stamp slot and the reserve; this launch runs at the default wave priority whatever lo.prio says (cfg 7 is handed lo whole).
// workgroups of the grouped launch over `total` tiles: a multiple of 8, capped (max_wgs > 0: by the caller; else
// UNITER_WGRAD_GROUP_WGS, default 256 = one workgroup per CU walking its tiles: switches.h).  Not persistent_grid
// (gemm_internal.h): the default cap is the switch, not the chip's CUs, and a cap below 8 leaves the grid uncapped
static int wgrad_group_grid(int total, int max_wgs, int cu_reserve) {
  int grid = (total + 7) / 8 * 8;
  int cap = max_wgs >= 8 ? max_wgs / 8 * 8 : uniter_switches().wgrad_group_wgs;
  if (cu_reserve > 0 && cap >= 8) {                       // CUs left to the data-parallel exchange's kernels (LaunchOpts::cu_reserve)
    const int room = (gemm_chip_cus() - cu_reserve) / 8 * 8;
    if (room >= 8 && cap > room) cap = room;
  }
  if (cap >= 8 && grid > cap) grid = cap;
  return grid;
}
// sum-of-squares slots a launch with riders writes (4 compute waves per workgroup)
int gemm_bf16v2_wgrad_group_slots(int n, const int* Mo, const int* No, int max_wgs, int cu_reserve) {
  return rider_slots(4, wgrad_group_grid(wgrad_group_tiles(n, Mo, No, 128), max_wgs, cu_reserve));
}
// the smallest grid on which the tiles take no more rounds than on one workgroup per CU
int gemm_bf16v2_wgrad_group_balanced_wgs(int n, const int* Mo, const int* No, int cu_reserve) {
  const int total = wgrad_group_tiles(n, Mo, No, 128);
  return balanced_grid(total, wgrad_group_grid(total, 0, cu_reserve));
}

int gemm_bf16v2_wgrad_group(int cfg, const WgradGroupCall& c, const LaunchOpts& lo) {
  static const char* const who = "wgrad_group";
  UCHECK_RC(wgrad_group_check(who, c));
  if (cfg == 7) return gemm_b1p_wgrad_group(c, lo);      // 128 x 256 tiles, persistent
  UCHECK_ARG(!c.sk_ws && !c.Kp, "%s: no launch of the bf16 family takes a workspace or per-product reduction lengths", who);
  GGroupD G;
  memset(&G.x, 0, sizeof(G.x));
  UCHECK_RC(wgrad_group_walk(who, c, G.start, [&](int p) { return wgrad_bf16_product_in_range(c, p); },
    [&](int p) {
      const int Mo = c.Mo[p], No = c.No[p];
      float* const dW = c.dW[p];
      GArgsD& g = G.p[p];
      g = {Mo, No, c.K, c.A[p], Mo, c.B[p], No, dW, No, /*c_split_stride*/ 0, /*Cb*/ nullptr, 0,
           c.overwrite ? UNITER_EPI_NONE : UNITER_EPI_ADD, /*bias*/ nullptr, /*aux_in*/ c.overwrite ? nullptr : dW, 0, /*aux_out*/ nullptr, 0,
           /*ld_aux*/ No, /*tiles_m, tiles_n, band_h*/ 0, 0, 1, /*nsplit*/ 1, lo.stamp, /*prio*/ 0, /*dbg*/ 0};
      plan_tiles<128>(g, 128);
      return g.tiles_m * g.tiles_n;
    },
    [&](int p) { G.p[p] = G.p[0]; }));
  const int grid = wgrad_group_grid(G.start[4], c.max_wgs, lo.cu_reserve);
  hipStream_t st = (hipStream_t)c.stream;
  const int overwrite = c.overwrite;
  if (uniter_x3_riders_t* riders = c.riders) {
    UCHECK_ARG(cfg != 4, "wgrad_group: riders ride on the two-stage form (cfg 1)");
    riders->grid = grid;
    UCHECK_RC(riders_prepare(*riders, "wgrad_bf16_group"));
    G.x = *riders;
    if (overwrite) hipLaunchKernelGGL((gemm_dma_wgrad_group_kernel<2, false, true>), dim3(grid), dim3(256), 0, st, G);
    else hipLaunchKernelGGL((gemm_dma_wgrad_group_kernel<2, true, true>), dim3(grid), dim3(256), 0, st, G);
    UCHECK_LAUNCH();
    return 0;
  }
  if (cfg == 4) {
    if (overwrite) hipLaunchKernelGGL((gemm_dma_wgrad_group_kernel<3, false>), dim3(grid), dim3(256), 0, st, G);
    else hipLaunchKernelGGL((gemm_dma_wgrad_group_kernel<3, true>), dim3(grid), dim3(256), 0, st, G);
  } else {
    if (overwrite) hipLaunchKernelGGL((gemm_dma_wgrad_group_kernel<2, false>), dim3(grid), dim3(256), 0, st, G);
    else hipLaunchKernelGGL((gemm_dma_wgrad_group_kernel<2, true>), dim3(grid), dim3(256), 0, st, G);
  }
  UCHECK_LAUNCH();
  return 0;
}

extern "C" int uniter_wgrad_bf16_group_riders(int cfg, int n, const int* M, const int* N, int K, const void* const* A,
                                              const void* const* B, float* const* dW, int overwrite, int max_wgs,
                                              uniter_x3_riders_t* riders, void* stream) {
  WgradGroupCall c;
  c.n = n; c.Mo = M; c.No = N; c.K = K; c.A = A; c.B = B; c.dW = dW; c.overwrite = overwrite; c.max_wgs = max_wgs; c.riders = riders;
  c.stream = stream;
  return gemm_bf16v2_wgrad_group(cfg, c, LaunchOpts{});
}
extern "C" int uniter_wgrad_bf16_group(int cfg, int n, const int* M, const int* N, int K, const void* const* A,
                                       const void* const* B, float* const* dW, void* stream) {
  return uniter_wgrad_bf16_group_riders(cfg, n, M, N, K, A, B, dW, 0, 0, nullptr, stream);
}
extern "C" int uniter_wgrad_bf16_group_slots(int n, const int* M, const int* N, int max_wgs) {
  return gemm_bf16v2_wgrad_group_slots(n, M, N, max_wgs, 0);
}
// the same for a given geometry of the grouped launch: cfg 7 (persistent 128 x 256 tiles, gemm_bf16_p.hip) writes 8 slots per workgroup
extern "C" int uniter_wgrad_bf16_group_slots_cfg(int cfg, int n, const int* M, const int* N, int max_wgs) {
  return cfg == 7 ? gemm_b1p_wgrad_group_slots(n, M, N, max_wgs, 0) : gemm_bf16v2_wgrad_group_slots(n, M, N, max_wgs, 0);
}

// Split-K choice for the GEMMs whose N is the hidden size (measured on MI355X, tests/tools/gemm_v2_lab.py,
// profiles/r02_gemm_bf16_v2.txt): with 128 x 128 tiles M = 2624, N = 768 gives 126 tiles for 256 CUs x 2 resident
// workgroups; two k-pieces per tile fill the chip (FFN-down 33.7 -> 22.3 us).  Four pieces are faster still in the
// GEMM (21.0 us) but every extra slab costs the consumer an 8 MB read, so four only where two leave half the slots
// empty.  Pieces shorter than 12 k-tiles do not pay for their prologue.
int gemm_bf16v2_pick_split(int M, int N, int K) {
  const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
  const int nk = (K + KT - 1) / KT;
  if (tiles <= 128 && nk >= 48) return 4;
  if (tiles <= 320 && nk >= 24) return 2;
  return 1;
}

// Weight gradients dW[M, N] += dY^T X (both operands k-major, K = rows of the batch): pieces of the split-K slab form,
// or 0 = keep the stream-K + float-atomics kernel of gemm_bf16.hip (the default: the slab form is the opt-in
// UNITER_WGRAD_SLABS=1, switches.h)
int gemm_bf16v2_wgrad_pieces(int M, int N, int K) {
  if (!uniter_switches().wgrad_slabs || K < 1024 || M % 8 || N % 8) return 0;
  const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
  if (tiles <= 48) return 4;
  if (M <= N || tiles <= 128) return 2;
  return 0;
}

extern "C" int uniter_gemm_bf16v2_cfg(int cfg, int nsplit, int a_kmajor, int b_kmajor, int M, int N, int K,
                                      const void* A, int lda, const void* B, int ldb, float* C, int ldc,
                                      long c_split_stride, void* C_bf16, int ldcb, int epilogue, const float* bias,
                                      const void* aux_in, int aux_in_bf16, void* aux_out, int aux_out_bf16,
                                      int ld_aux, int beta, void* stream) {
  GemmCall c;
  c.M = M; c.N = N; c.K = K; c.A = {A, lda, 0, a_kmajor}; c.B = {B, ldb, 0, b_kmajor};
  c.C = C; c.ldc = ldc; c.c_split_stride = c_split_stride; c.nsplit = nsplit; c.Ccopy = C_bf16; c.ld_copy = ldcb;
  c.epi = epilogue; c.bias = bias; c.aux_in = aux_in; c.aux_in_bf16 = aux_in_bf16; c.aux_out = aux_out; c.aux_out_bf16 = aux_out_bf16;
  c.ld_aux = ld_aux; c.beta = beta; c.stream = stream;
  return gemm_bf16v2_run(cfg, c, LaunchOpts{});
}
