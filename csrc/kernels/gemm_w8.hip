// FP8-weight decode GEMM (W8A16):  Y[M, N] = (X[M, K] · Wq[N, K]ᵀ) * scale[N],  1 <= M <= 64.
//
// The weight is one e4m3 byte per element in the byte form of the tiled layout (api.h kTileChunkF8) plus one fp32
// power-of-two scale per output row (ops/reference.py quantize_weight_f8).  The kernel keeps gemm_ring_kernel's
// discipline (gemm_stream.hip; docs/kernels.md "Decode GEMMs") and halves the bytes it streams:
//   * for K-chunk c (128 columns) every wave issues its share of the chunk's X rows (global_load_lds, L2-resident)
//     and its own 2 KiB weight chunk (two buffer_load ... lds of 1 KiB, non-temporal, through a descriptor that
//     covers exactly its K range) into LDS slot c % D, D - 1 chunks ahead of the MFMAs;
//   * one counted vmcnt + barrier per chunk publishes chunk c while chunks c+1 .. c+D-2 stay in flight; look-ahead
//     issues past the last chunk keep the per-wave load count uniform (weights fail the range check: no traffic; X
//     re-reads the last chunk into a slot nobody reads);
//   * a lane reads its 16 weight bytes of a half chunk with one ds_read_b128 (two k-steps), widens them to bf16 in
//     registers (every e4m3 value is exact in bf16) and feeds the same v_mfma_f32_16x16x32_bf16 as the bf16 kernels;
//   * slots are half as large per wave as the bf16 ring's, so the ring is about twice as deep in chunks and the
//     weight bytes in flight per CU stay at 36-64 KiB.
// Epilogue: the accumulator of column n is multiplied by scale[n] in fp32 before anything else; then the shared
// epilogues of gemm_epilogue.h run unchanged (the fp32 split-K slabs are therefore already scaled).
// Slot = [X image: 16 MT rows x 256 B, 16-B pieces XOR-swizzled by swz() on the source address][NW x 2 KiB weight
// chunks in the byte layout, read back lane-linearly].
#include "gemm_epilogue.h"

#include <type_traits>

#ifndef DSSE_XCD_SPLITK
#define DSSE_XCD_SPLITK 1  // XCD-grouped split-K workgroup mapping (as gemm_stream.hip)
#endif

namespace dsse {

template <int MT, int NW, int D>
struct W8Geom {
  static constexpr int SLOTX = 16 * MT * 256, SLOT = SLOTX + NW * kTileChunkF8;
  static constexpr size_t LDS = (size_t)D * SLOT;
};

// As many chunks as the LDS holds, 8 at most (beyond ~64 KiB of weight bytes in flight per CU nothing is gained).
constexpr int w8_depth(int mt, int nw) {
  const int d = (160 * 1024) / (16 * mt * 256 + nw * kTileChunkF8);
  return d > 8 ? 8 : d;
}

// XCD-grouped split-K numbering (gemm_stream.hip xcd_split_shift / xcd_split): bijective, speed only.
static inline int w8_xcd_shift(int gx, int S) {
  if (!DSSE_XCD_SPLITK || S <= 1 || 8 % S != 0 || (gx * S) % 8 != 0) return -1;
  return S == 2 ? 2 : (S == 4 ? 1 : 0);
}

DEV void w8_glds16(const void* src, char* lds_base) {
  __builtin_amdgcn_global_load_lds(const_cast<void*>(src),
                                   reinterpret_cast<__attribute__((address_space(3))) void*>(
                                       reinterpret_cast<uintptr_t>(lds_base)),
                                   16, 0, 0);
}

template <int MT, int NW, int D, int MODE>
__global__ void __launch_bounds__(64 * NW)
gemm_w8_kernel(const bf16* __restrict__ X, int ldx, int M, const f8* __restrict__ W, int K, int N, int Kr, int gx,
               int xs, int S, float* __restrict__ part, const float* __restrict__ scale, GemmEpi ep) {
  // Argument order (docs/kernels.md "Kernel entry"): the 14 dwords up to `part` are all the first DMA burst needs.
  using G = W8Geom<MT, NW, D>;
  constexpr int MP = 16 * MT;
  constexpr int XN = MP / 4;              // 1 KiB X DMA instructions per chunk (4 rows each)
  constexpr int XI = (XN + NW - 1) / NW;  // per wave; surplus instructions repeat the last one (a benign duplicate)
  static_assert(D >= 3 && G::LDS <= 160 * 1024, "ring of >= 3 slots within the CU's LDS");
  constexpr int PER = XI + 2;             // VMEM instructions per wave per chunk
  static_assert((D - 2) * PER <= 62, "the counted vmcnt is a 6-bit field (one more load may be in flight: scale)");
  extern __shared__ __attribute__((aligned(1024))) char smem[];

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  int wg = blockIdx.x, ks = blockIdx.y;
  if (xs >= 0) {
    const int lin = blockIdx.y * gx + blockIdx.x, xcd = lin & 7, slot = lin >> 3;
    ks = xcd >> xs;
    wg = (slot << xs) + (xcd & ((1 << xs) - 1));
  }
  const int tgi = wg * NW + w;  // this wave's 16-column tile (host: N / 16 % NW == 0, so tgi < N / 16)
  const int k0 = ks * Kr;
  const int nch = Kr >> 7;
  const int KC = K >> 7;

  const int tgu = __builtin_amdgcn_readfirstlane(tgi), k0u = __builtin_amdgcn_readfirstlane(k0);
  const __amdgpu_buffer_rsrc_t wrs =
      make_rsrc(W + ((size_t)tgu * KC + (k0u >> 7)) * kTileChunkF8, (uint32_t)nch * kTileChunkF8);

  // this lane's X source per DMA instruction: row 4 (w XI + i) + g, logical piece r ^ swz(row & 15)
  const bf16* xsrc[XI];
  int xdst[XI];
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    xdst[i] = __builtin_amdgcn_readfirstlane(min(w * XI + i, XN - 1));
    const int row = 4 * xdst[i] + g;
    xsrc[i] = X + (size_t)min(row, M - 1) * ldx + k0 + 8 * (r ^ swz(row & 15));
  }
  auto issue = [&](int c, int slot) {
    const int cc = min(c, nch - 1);
    char* base = smem + slot * G::SLOT;
#pragma unroll
    for (int i = 0; i < XI; ++i) w8_glds16(xsrc[i] + cc * 128, base + xdst[i] * 1024);
    char* wb = base + G::SLOTX + w * kTileChunkF8;
#pragma unroll
    for (int h = 0; h < 2; ++h)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wrs, reinterpret_cast<__attribute__((address_space(3))) void*>(reinterpret_cast<uintptr_t>(wb + 1024 * h)),
          16, (uint32_t)c * kTileChunkF8 + 1024 * h + lane * 16, 0, 0, kAuxNT);
  };

#pragma unroll
  for (int d = 0; d < D - 1; ++d) issue(d, d);

  // This lane's column scale, fetched behind the first DMA burst.  Issued as an instruction the compiler does not
  // count, so it places no wait of its own inside the ring; VMEM returns in order, so the counted waits below are
  // at most one load stricter until it lands, and the final vmcnt(0) (which names `sc`) covers it.
  float sc;
  {
    const float* sp = scale + tgi * 16 + r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(sc) : "v"(sp) : "memory");
  }

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < nch; c0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      if (u > 0 && c0 + u >= nch) break;
      // chunk c0 + u landed for every wave, chunks up to c0 + u + D - 2 still in flight
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((D - 2) * PER) : "memory");
      const char* xb = smem + u * G::SLOT;
      const char* wb = xb + G::SLOTX + w * kTileChunkF8 + lane * 16;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32x4 wq = *reinterpret_cast<const u32x4*>(wb + 1024 * h);
        bf16x8 xf[2][MT];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int ch = ((4 * g + 2 * h + s) ^ swz(r)) << 4;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            xf[s][mt] = *reinterpret_cast<const bf16x8*>(xb + (16 * mt + r) * 256 + ch);
        }
        const bf16x8 wf0 = widen_f8x8(make_uint2(wq[0], wq[1])), wf1 = widen_f8x8(make_uint2(wq[2], wq[3]));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16x16x32(xf[0][mt], wf0, acc[mt]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16x16x32(xf[1][mt], wf1, acc[mt]);
      }
      // refill the slot of chunk c - 1 (every wave finished it before the barrier above)
      issue(c0 + u + D - 1, (u + D - 1) % D);
    }
  }
  // no LDS-DMA may still be landing when the workgroup's LDS is handed to the next workgroup; `sc` landed too
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(sc)::"memory");

#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[mt][i] *= sc;

  float* part_ks = part ? part + (size_t)ks * M * N : nullptr;
  if constexpr (MODE == kSiluMul) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) silu_epilogue4(ep, M, 16 * mt + 4 * g, tgi, r, acc[mt]);
    return;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = acc[mt][i];
      const float partner = MODE == kQkvRope ? __shfl_xor(v, 8) : 0.f;
      epilogue<MODE>(ep, part_ks, M, N, 16 * mt + 4 * g + i, tgi, r, v, partner);
    }
}

template <int MT, int NW, int MODE>
static hipError_t launch_w8(const bf16* X, int ldx, int M, const f8* W, const float* scale, int K, int N, int S,
                            const GemmEpi& ep, float* part, hipStream_t st) {
  constexpr int D = w8_depth(MT, NW);
  const size_t lds = W8Geom<MT, NW, D>::LDS;
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_w8_kernel<MT, NW, D, MODE>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  dim3 grid(N / 16 / NW, S), block(64 * NW);
  hipLaunchKernelGGL((gemm_w8_kernel<MT, NW, D, MODE>), grid, block, lds, st, X, ldx, M, W, K, N, K / S, (int)grid.x,
                     w8_xcd_shift((int)grid.x, S), S, part, scale, ep);
  return hipGetLastError();
}

template <int MODE>
static hipError_t launch_w8_mode(int nw, const bf16* X, int ldx, int M, const f8* W, const float* scale, int K, int N,
                                 int S, const GemmEpi& ep, float* part, hipStream_t st) {
  const int mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
#define K_W8_CASE(MT_, NW_) \
  if (mt == MT_ && nw == NW_) return launch_w8<MT_, NW_, MODE>(X, ldx, M, W, scale, K, N, S, ep, part, st);
#define K_W8_MT(MT_) K_W8_CASE(MT_, 3) K_W8_CASE(MT_, 4) K_W8_CASE(MT_, 7) K_W8_CASE(MT_, 8)
  K_W8_MT(1) K_W8_MT(2) K_W8_MT(4)
#undef K_W8_MT
#undef K_W8_CASE
  return hipErrorInvalidValue;
}

}  // namespace dsse

// 1 <= M <= 64 rows (16-row MFMA tiles: 1 / 2 / 4 by M), nw in {3, 4, 7, 8} waves of one 16-column tile each.
// Shape contract (checked here and by the caller): K % (128 S) == 0, (N / 16) % nw == 0.  W: N x K bytes in the
// kTileChunkF8 layout, scale: fp32 [N].  part: fp32 [S, M, N] when S > 1; partial_only: leave the (scaled) slabs for
// the consumer (the folded decode attention, the fused residual + RMSNorm) instead of reducing them here.
extern "C" hipError_t dsse_gemm_w8(int mode, int nw, int S, int partial_only, const void* X, int ldx, int M,
                                   const void* W, const float* scale, int K, int N, const dsse::GemmEpi* ep,
                                   float* part, hipStream_t st) {
  using namespace dsse;
  const bf16* x = reinterpret_cast<const bf16*>(X);
  const f8* w = reinterpret_cast<const f8*>(W);
  if (M < 1 || M > 64 || S < 1 || K % (128 * S) != 0 || N % 16 != 0 || (N / 16) % nw != 0 || ldx < K)
    return hipErrorInvalidValue;
  if ((S > 1 || partial_only) && part == nullptr) return hipErrorInvalidValue;
  if (S == 1 && !partial_only) {
    switch (mode) {
      case kStoreBf16: return launch_w8_mode<kStoreBf16>(nw, x, ldx, M, w, scale, K, N, 1, *ep, nullptr, st);
      case kStoreF32: return launch_w8_mode<kStoreF32>(nw, x, ldx, M, w, scale, K, N, 1, *ep, nullptr, st);
      case kResidAdd: return launch_w8_mode<kResidAdd>(nw, x, ldx, M, w, scale, K, N, 1, *ep, nullptr, st);
      case kSiluMul: return launch_w8_mode<kSiluMul>(nw, x, ldx, M, w, scale, K, N, 1, *ep, nullptr, st);
      case kQkvRope: return launch_w8_mode<kQkvRope>(nw, x, ldx, M, w, scale, K, N, 1, *ep, nullptr, st);
    }
    return hipErrorInvalidValue;
  }
  hipError_t e = launch_w8_mode<kPartial>(nw, x, ldx, M, w, scale, K, N, S, *ep, part, st);
  if (e != hipSuccess || partial_only) return e;
  return launch_splitk_reduce(mode, part, S, M, N, *ep, st);
}

DSSE_CHECK_READER(dsse_check_gemm_w8)
