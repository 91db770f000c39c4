// Device vocabulary of the kernels on the bf16 matrix pipe (gemm_bf16*.hip, gemm_split3.hip, attention_*.hip), stated once:
// vector types, the banded tile walk, the XCD-chunked work item, bf16 packing, the inline-assembly LDS reads with their
// register ties and waits, and the LDS-DMA fill of a two-byte operand image.  What differs between the kernels on purpose --
// fragments (Frag / Frag3 / Frag16 / FragP), epilogues, Dma3's three piece images -- stays in their files.
#pragma once
#include <type_traits>
#include "common.h"

#ifdef __HIPCC__
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int OOB = 0x7ffffff0;        // buffer offset beyond every descriptor: load returns 0, store is dropped

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// L2-aware tile order.  The workgroups of one XCD run a window of consecutive tiles of the linear order at once.  Row-major order
// makes that window a few tile rows x all tile columns: the whole B operand streams through the 4 MiB L2 again for every few rows
// (measured on the fp32 FFN-up: 68 % L2 hit rate, ~250 MB fetched beyond L2 for 17 MB of operands).  Banded order: bands of
// `band_h` tile rows, tile columns swept inside a band with the row index fastest, so the window is band_h rows high.
__device__ __forceinline__ void tile_coords(int t, int tiles_m, int tiles_n, int band_h, int& tm, int& tn) {
  const int full = band_h * tiles_n;
  const int band = t / full;
  const int rem = t - band * full;
  const int bh = min(band_h, tiles_m - band * band_h);
  tn = rem / bh;
  tm = band * band_h + (rem - tn * bh);
}

// work item of this workgroup, XCD-chunked (blocks b and b + 8 share an XCD's L2: consecutive items go to one XCD);
// -1 for the padding blocks of the grid.  round > 0: the items a workgroup of a grid SMALLER than the work takes after
// its first one (a persistent or capped launch), still inside its XCD's chunk
__device__ __forceinline__ int xcd_work_item(int nwork, int round = 0) {
  const int xcd = blockIdx.x & 7, idx = (blockIdx.x >> 3) + round * (int)(gridDim.x >> 3);
  const int q8 = nwork >> 3, r8 = nwork & 7;
  const int chunk0 = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  const int chunk_n = q8 + (xcd < r8 ? 1 : 0);
  return idx < chunk_n ? chunk0 + idx : -1;
}

__device__ __forceinline__ unsigned pack2(float lo, float hi) {
  bf16x2 v = {(__bf16)lo, (__bf16)hi};      // v_cvt_pk_bf16_f32: round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float bf_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

// the three bf16 pieces of two fp32 values (exact: every residual is representable)
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& w1, unsigned& w2, unsigned& w3) {
  w1 = pack2(x0, x1);
  float r0 = x0 - bf_lo(w1), r1 = x1 - bf_hi(w1);
  w2 = pack2(r0, r1);
  r0 -= bf_lo(w2); r1 -= bf_hi(w2);
  w3 = pack2(r0, r1);
}

// the two halves of a transposed fragment read as one MFMA operand
__device__ __forceinline__ bf16x8 join_halves(u32x2_t lo, u32x2_t hi) {
  const u32x4_t v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(bf16x8, v);
}

// ---- LDS reads, register ties and waits ---------------------------------------------------------------------------------
// The fragment reads of the kernels that fill LDS by LDS-DMA are INLINE ASSEMBLY with hand-counted lgkmcnt waits: behind the
// builtin form of ds_read_b64_tr_b16 (and before compiler-visible LDS reads in general) hipcc (ROCm 7.2) waits
// s_waitcnt vmcnt(0) whenever an LDS-DMA is in flight, which would drain the prefetched k-tiles every k-tile (checked in the
// .s).  A loop uses ONE kind of LDS read: a compiler read between the asm ones would be waited for with a count that ignores
// them.  Every statement clobbers "memory", so the issue order is the program order.  (__HIP_DEVICE_COMPILE__: the host pass
// parses these bodies too and knows no "v" constraint.)
template <int OFF>
__device__ __forceinline__ void lds_read_b128(u32x4_t& out, unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(out) : "v"(addr), "n"(OFF) : "memory");
#endif
}
template <int OFF>
__device__ __forceinline__ void lds_read_tr(u32x2_t& out, unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(out) : "v"(addr), "n"(OFF) : "memory");
#endif
}
// ties a fragment's first use to the statements above it (the wait): an empty volatile asm that "rewrites" the register
__device__ __forceinline__ void tie(u32x4_t& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v)::"memory");
#endif
}
__device__ __forceinline__ void tie2(u32x2_t& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v)::"memory");
#endif
}
template <int N> __device__ __forceinline__ void lgkm_wait() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
#endif
}
template <int N> __device__ __forceinline__ void wait_vm() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}

// ---- LDS-DMA fill of one two-byte operand image (buffer_load_dwordx4 ... lds) -------------------------------------------------
// Images per operand and stage (R = rows of the tile, KT = 64 k per k-tile, no padding: LDS-DMA writes 1 KiB = 64 lanes x 16 B
// contiguously, so the swizzle sits on the per-lane SOURCE address and on the read):
//   k-contiguous operand ([rows][K] in memory): [R][64] bf16, 128-B rows, 16-B chunk c of row r stored at chunk
//     c ^ ((r >> 1) & 7): 16 consecutive rows x one k-chunk cover all 64 banks (ds_read_b128).  Eight rows x one 128-byte
//     line per instruction: the eight lanes of a row fetch the whole line.
//   k-major operand ([K][cols] in memory: the weight of an input-gradient product): [64 k][R] bf16 as 256-B segments, chunk c
//     (0..15) of k-row k stored at c ^ (((k & 3) << 2) | ((k >> 2) & 3)); the MFMA operand is gathered by ds_read_b64_tr_b16
//     (4 k-rows x 16 columns per 16-lane group), whose 32 lanes per half then touch 32 distinct 8-byte units.
// NW waves share the image's R / 8 wave-instructions; KT is the user's k-tile depth.
template <int R, bool KM, int NW, int KT>
struct Dma {
  static constexpr int NI = R / 8 / NW;          // 1-KiB wave-instructions per wave and k-tile
  static_assert(NI >= 1 && NI * 8 * NW == R, "tile rows must be a multiple of 8 x waves");
  static_assert(!KM || R == 128 || R == 256, "k-major tiles are 128 or 256 wide");
  int voff[NI];
  static __device__ __forceinline__ int kstep(int ld) { return (KM ? KT * ld : KT) * 2; }
  __device__ __forceinline__ void offsets(int ld, int rc0, int wave, int lane) {
#pragma unroll
    for (int t = 0; t < NI; ++t) {
      const int j = wave + NW * t;
      if constexpr (!KM) {
        const int row = 8 * j + (lane >> 3);
        const int c = (lane & 7) ^ ((4 * (j & 1) + (lane >> 4)) & 7);
        voff[t] = (rc0 + row) * ld * 2 + c * 16;
      } else if constexpr (R == 128) {
        const int k = 4 * j + (lane >> 4);
        const int c = (lane & 15) ^ (((lane >> 4) << 2) | (j & 3));
        voff[t] = (k * ld + rc0) * 2 + c * 16;
      } else {
        const int k = 2 * j + (lane >> 5);
        const int sw = (((2 * (j & 1) + (lane >> 5)) & 3) << 2) | ((j >> 1) & 3);
        const int c = (lane & 15) ^ sw;
        voff[t] = (k * ld + rc0) * 2 + ((lane >> 4) & 1) * 256 + c * 16;
      }
    }
  }
  // every wave-instruction of this wave
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rs, unsigned char* img, int soff, int wave) const {
#pragma unroll
    for (int t = 0; t < NI; ++t)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(img + (wave + NW * t) * 1024), 16, voff[t], soff, 0, 0);
  }
  // wave-instruction T of this wave
  template <int T>
  __device__ __forceinline__ void issue1(__amdgpu_buffer_rsrc_t rs, unsigned char* img, int soff, int wave) const {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(img + (wave + NW * T) * 1024), 16, voff[T], soff, 0, 0);
  }
};

}  // namespace
#endif
