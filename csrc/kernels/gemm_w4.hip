// MXFP4-weight decode GEMM (W4A16):  Y[M, N] = X[M, K] · widen(Wq, E)[N, K]ᵀ,  1 <= M <= 64.
//
// The weight is OCP MXFP4: one e2m1 nibble per element and one e8m0 scale byte per 32 consecutive K, both in the tiled
// device layout of api.h (kTileChunkF4 / kTileScaleF4; ops/reference.py quantize_weight_mxfp4 / tile_weight_mxfp4).
// The kernel is gemm_w8_kernel's structure (gemm_w8.hip; docs/kernels.md "Decode GEMMs") with a quarter of the bf16
// weight bytes:
//   * for K-chunk c (128 columns) every wave issues its share of the chunk's X rows (global_load_lds, L2-resident),
//     its own 1 KiB of nibbles (one buffer_load ... lds of 16 B per lane, non-temporal) and its own 64 scale bytes
//     (one buffer_load ... lds of 4 B per lane: lanes 0-15 bring the chunk's scales, the other lanes the next three
//     chunks', which nobody reads) into LDS slot c % D, D - 1 chunks ahead of the MFMAs.  Both weight streams go
//     through descriptors that cover exactly the wave's K range;
//   * one counted vmcnt + barrier per chunk publishes chunk c while chunks c+1 .. c+D-2 stay in flight; look-ahead
//     issues past the last chunk keep the per-wave load count uniform (weights and scales fail the range check: no
//     traffic; X re-reads the last chunk into a slot nobody reads);
//   * lane r + 16 g owns one MX block per chunk, W[16T + r][128c + 32g .. 32g + 31]: one ds_read_b128 (32 nibbles,
//     four k-steps) and one ds_read_u8 (its scale).  v_cvt_scalef32_pk_bf16_fp4 turns a byte and the fp32 scale
//     2^(e - 127) into two bf16 values, exact, so the MFMA B operand is already scaled and the epilogues of
//     gemm_epilogue.h run on the accumulator as it is.  16 converts beside 4 MT MFMAs per chunk.
// Slot = [X image: 16 MT rows x 256 B, 16-B pieces XOR-swizzled by swz() on the source address][NW x 1 KiB nibbles,
// read back lane-linearly][NW x 256 B scale landing zones, byte [lane] of the first 64 used].
#include "gemm_epilogue.h"

#include <type_traits>

#ifndef DSSE_XCD_SPLITK
#define DSSE_XCD_SPLITK 1  // XCD-grouped split-K workgroup mapping (as gemm_stream.hip)
#endif

namespace dsse {

constexpr int kW4ScaleZone = 256;  // LDS bytes one 4-B-per-lane scale DMA writes

template <int MT, int NW, int D>
struct W4Geom {
  static constexpr int SLOTX = 16 * MT * 256, SLOTW = SLOTX + NW * kTileChunkF4;
  static constexpr int SLOT = SLOTW + NW * kW4ScaleZone;
  static constexpr size_t LDS = (size_t)D * SLOT;
};

// As many chunks as the LDS holds, 8 at most (as gemm_w8.hip: the X image, not the weight, fills the slots).
constexpr int w4_depth(int mt, int nw) {
  const int d = (160 * 1024) / (16 * mt * 256 + nw * (kTileChunkF4 + kW4ScaleZone));
  return d > 8 ? 8 : d;
}

// XCD-grouped split-K numbering (gemm_stream.hip xcd_split_shift / xcd_split): bijective, speed only.
static inline int w4_xcd_shift(int gx, int S) {
  if (!DSSE_XCD_SPLITK || S <= 1 || 8 % S != 0 || (gx * S) % 8 != 0) return -1;
  return S == 2 ? 2 : (S == 4 ? 1 : 0);
}

DEV void w4_glds16(const void* src, char* lds_base) {
  __builtin_amdgcn_global_load_lds(const_cast<void*>(src),
                                   reinterpret_cast<__attribute__((address_space(3))) void*>(
                                       reinterpret_cast<uintptr_t>(lds_base)),
                                   16, 0, 0);
}

// Four bytes = eight e2m1 nibbles (element 2j in the low nibble of byte j, element 2j + 1 in the high one) times the
// block scale -> the bf16x8 MFMA B fragment of one k-step (exact).
DEV bf16x8 widen_f4x8(unsigned d, float scale) {
  u32x4 o;
  o[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0));
  o[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1));
  o[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2));
  o[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3));
  return __builtin_bit_cast(bf16x8, o);
}

template <int MT, int NW, int D, int MODE>
__global__ void __launch_bounds__(64 * NW)
gemm_w4_kernel(const bf16* __restrict__ X, int ldx, int M, const unsigned char* __restrict__ W,
               const unsigned char* __restrict__ E, int K, int Kr, int gx, int xs, int N, int S,
               float* __restrict__ part, GemmEpi ep) {
  // Argument order (docs/kernels.md "Kernel entry"): the 12 dwords up to `xs` are all the first DMA burst needs.
  using G = W4Geom<MT, NW, D>;
  constexpr int MP = 16 * MT;
  constexpr int XN = MP / 4;              // 1 KiB X DMA instructions per chunk (4 rows each)
  constexpr int XI = (XN + NW - 1) / NW;  // per wave; surplus instructions repeat the last one (a benign duplicate)
  static_assert(D >= 3 && G::LDS <= 160 * 1024, "ring of >= 3 slots within the CU's LDS");
  constexpr int PER = XI + 2;             // VMEM instructions per wave per chunk: X, nibbles, scales
  static_assert((D - 2) * PER <= 63, "the counted vmcnt is a 6-bit field");
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
  const size_t blk0 = (size_t)tgu * KC + (k0u >> 7);  // this wave's first (tile, chunk) block
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(W + blk0 * kTileChunkF4, (uint32_t)nch * kTileChunkF4);
  const __amdgpu_buffer_rsrc_t ers = make_rsrc(E + blk0 * kTileScaleF4, (uint32_t)nch * kTileScaleF4);

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
    for (int i = 0; i < XI; ++i) w4_glds16(xsrc[i] + cc * 128, base + xdst[i] * 1024);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        wrs,
        reinterpret_cast<__attribute__((address_space(3))) void*>(
            reinterpret_cast<uintptr_t>(base + G::SLOTX + w * kTileChunkF4)),
        16, (uint32_t)c * kTileChunkF4 + lane * 16, 0, 0, kAuxNT);
    // scales: temporal, the 128-B line holds two chunks' worth and the lanes past 15 touch the lines that follow
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        ers,
        reinterpret_cast<__attribute__((address_space(3))) void*>(
            reinterpret_cast<uintptr_t>(base + G::SLOTW + w * kW4ScaleZone)),
        4, (uint32_t)c * kTileScaleF4 + lane * 4, 0, 0, 0);
  };

#pragma unroll
  for (int d = 0; d < D - 1; ++d) issue(d, d);

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
      const u32x4 wq = *reinterpret_cast<const u32x4*>(xb + G::SLOTX + w * kTileChunkF4 + lane * 16);
      const unsigned eb = *reinterpret_cast<const unsigned char*>(xb + G::SLOTW + w * kW4ScaleZone + lane);
      const float sc = __builtin_bit_cast(float, eb << 23);  // e8m0, bias 127: 2^(eb - 127), eb in [63, 191]
#pragma unroll
      for (int t = 0; t < 4; ++t) {  // k-step t: k = 32 g + 8 t + j, the X piece 4 g + t
        const int ch = ((4 * g + t) ^ swz(r)) << 4;
        bf16x8 xf[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xf[mt] = *reinterpret_cast<const bf16x8*>(xb + (16 * mt + r) * 256 + ch);
        const bf16x8 wf = widen_f4x8(wq[t], sc);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16x16x32(xf[mt], wf, acc[mt]);
      }
      // refill the slot of chunk c - 1 (every wave finished it before the barrier above)
      issue(c0 + u + D - 1, (u + D - 1) % D);
    }
  }
  // no LDS-DMA may still be landing when the workgroup's LDS is handed to the next workgroup
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

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
static hipError_t launch_w4(const bf16* X, int ldx, int M, const unsigned char* W, const unsigned char* E, int K, int N,
                            int S, const GemmEpi& ep, float* part, hipStream_t st) {
  constexpr int D = w4_depth(MT, NW);
  const size_t lds = W4Geom<MT, NW, D>::LDS;
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_w4_kernel<MT, NW, D, MODE>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  dim3 grid(N / 16 / NW, S), block(64 * NW);
  hipLaunchKernelGGL((gemm_w4_kernel<MT, NW, D, MODE>), grid, block, lds, st, X, ldx, M, W, E, K, K / S, (int)grid.x,
                     w4_xcd_shift((int)grid.x, S), N, S, part, ep);
  return hipGetLastError();
}

template <int MODE>
static hipError_t launch_w4_mode(int nw, const bf16* X, int ldx, int M, const unsigned char* W, const unsigned char* E,
                                 int K, int N, int S, const GemmEpi& ep, float* part, hipStream_t st) {
  const int mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
#define K_W4_CASE(MT_, NW_) \
  if (mt == MT_ && nw == NW_) return launch_w4<MT_, NW_, MODE>(X, ldx, M, W, E, K, N, S, ep, part, st);
#define K_W4_MT(MT_) K_W4_CASE(MT_, 3) K_W4_CASE(MT_, 4) K_W4_CASE(MT_, 6) K_W4_CASE(MT_, 7) K_W4_CASE(MT_, 8)
  K_W4_MT(1) K_W4_MT(2) K_W4_MT(4)
#undef K_W4_MT
#undef K_W4_CASE
  return hipErrorInvalidValue;
}

}  // namespace dsse

// 1 <= M <= 64 rows (16-row MFMA tiles: 1 / 2 / 4 by M), nw in {3, 4, 6, 7, 8} waves of one 16-column tile each.
// Shape contract (checked here and by the caller): K % (128 S) == 0, (N / 16) % nw == 0.  W: N x K / 2 nibble bytes in
// the kTileChunkF4 layout, E: N x K / 32 scale bytes in the kTileScaleF4 layout.  part: fp32 [S, M, N] when S > 1;
// partial_only: leave the slabs for the consumer (the folded decode attention, the fused residual + RMSNorm) instead
// of reducing them here.
extern "C" hipError_t dsse_gemm_w4(int mode, int nw, int S, int partial_only, const void* X, int ldx, int M,
                                   const void* W, const void* E, int K, int N, const dsse::GemmEpi* ep, float* part,
                                   hipStream_t st) {
  using namespace dsse;
  const bf16* x = reinterpret_cast<const bf16*>(X);
  const unsigned char* w = reinterpret_cast<const unsigned char*>(W);
  const unsigned char* e = reinterpret_cast<const unsigned char*>(E);
  if (M < 1 || M > 64 || S < 1 || K % (128 * S) != 0 || N % 16 != 0 || (N / 16) % nw != 0 || ldx < K)
    return hipErrorInvalidValue;
  if ((S > 1 || partial_only) && part == nullptr) return hipErrorInvalidValue;
  if (S == 1 && !partial_only) {
    switch (mode) {
      case kStoreBf16: return launch_w4_mode<kStoreBf16>(nw, x, ldx, M, w, e, K, N, 1, *ep, nullptr, st);
      case kStoreF32: return launch_w4_mode<kStoreF32>(nw, x, ldx, M, w, e, K, N, 1, *ep, nullptr, st);
      case kResidAdd: return launch_w4_mode<kResidAdd>(nw, x, ldx, M, w, e, K, N, 1, *ep, nullptr, st);
      case kSiluMul: return launch_w4_mode<kSiluMul>(nw, x, ldx, M, w, e, K, N, 1, *ep, nullptr, st);
      case kQkvRope: return launch_w4_mode<kQkvRope>(nw, x, ldx, M, w, e, K, N, 1, *ep, nullptr, st);
    }
    return hipErrorInvalidValue;
  }
  hipError_t err = launch_w4_mode<kPartial>(nw, x, ldx, M, w, e, K, N, S, *ep, part, st);
  if (err != hipSuccess || partial_only) return err;
  return launch_splitk_reduce(mode, part, S, M, N, *ep, st);
}

DSSE_CHECK_READER(dsse_check_gemm_w4)
