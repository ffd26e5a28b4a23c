// Memory-bound helper kernels of the decode/prefill step (K1, K2, K4, K11 of SURVEY.md §2.4).
// All bf16 traffic is vectorised to 8-16 bytes per lane (guide Guideline 13).
#include <algorithm>
#include "api.h"

namespace dsse {

constexpr int kPageTok = 32;

DEV int vperm_tok(int off) { return ((off & 15) >> 2) * 8 + ((off >> 4) & 1) * 4 + (off & 3); }

// ---- K1 + K2: (embedding gather | residual add) + RMSNorm ------------------------------------
// MODE 0: y = rmsnorm(resid)            MODE 1: resid += delta; y = rmsnorm(resid)
// MODE 2: resid = embed[ids[m]]; y = rmsnorm(resid)
// MODE 3: resid += sum_s part[s, m, :] (fp32 split-K slabs of the O / down projection, fusing the
//         split-K reduction into the norm that consumes it); y = rmsnorm(resid)
// The residual stream is fp32 [M, H]; y is the bf16 input of the next GEMM.  One workgroup of
// min(1024, H/4) threads per row (a decode batch has only M <= 64 rows, so the row is spread over
// as many waves as possible to keep enough loads in flight); each thread owns H / (4·threads) float4s.
template <int MODE>
__global__ void __launch_bounds__(1024)
rmsnorm_kernel(float* __restrict__ resid, const float* __restrict__ part, const bf16* __restrict__ w,
               const int* __restrict__ ids, const bf16* __restrict__ embed, int nt, int nit, int nsplit, int M,
               const bf16* __restrict__ delta, bf16* __restrict__ y, float eps, int vocab) {
  // Argument order (docs/kernels.md "Kernel entry"): the 14 dwords up to M arrive preloaded in SGPRs and address every
  // load of the row.  nt = the block size (blockDim is a hidden kernel argument: a round trip before the first load)
  // and nit = float4s per thread, both from the host: H = 4 nt nit exactly, so no division on the way to the loads.
  const int m = blockIdx.x, tid = threadIdx.x, H = 4 * nt * nit;
  const unsigned long long st0 = stamps::now();
  float* rrow = resid + (size_t)m * H;
  constexpr int kMaxIt = 2;  // H <= 8192
  float4 v[kMaxIt];
  float ss = 0.f;
  // the norm weights are loaded with the row, not after the block reduction: one dependent round trip fewer
  bf16x4 wv[kMaxIt];
#pragma unroll
  for (int it = 0; it < kMaxIt; ++it)
    if (it < nit) wv[it] = *reinterpret_cast<const bf16x4*>(w + (it * nt + tid) * 4);
#pragma unroll
  for (int it = 0; it < kMaxIt; ++it) {
    if (it < nit) {
      const int i = (it * nt + tid) * 4;
      float4 x;
      if constexpr (MODE == 2) {
        const bf16x4 e = *reinterpret_cast<const bf16x4*>(embed + (size_t)DSSE_IDX(ids[m], vocab, 0) * H + i);
        x = make_float4(bf2f(e[0]), bf2f(e[1]), bf2f(e[2]), bf2f(e[3]));
      } else {
        x = *reinterpret_cast<const float4*>(rrow + i);
        if constexpr (MODE == 1) {
          const bf16x4 d = *reinterpret_cast<const bf16x4*>(delta + (size_t)m * H + i);
          x.x += bf2f(d[0]); x.y += bf2f(d[1]); x.z += bf2f(d[2]); x.w += bf2f(d[3]);
        }
        if constexpr (MODE == 3) {
          const float* p = part + (size_t)m * H + i;
          const size_t slab = (size_t)M * H;
          int s = 0;
          for (; s + 4 <= nsplit; s += 4) {  // four independent loads in flight per step
            const float4 d0 = *reinterpret_cast<const float4*>(p + (s + 0) * slab);
            const float4 d1 = *reinterpret_cast<const float4*>(p + (s + 1) * slab);
            const float4 d2 = *reinterpret_cast<const float4*>(p + (s + 2) * slab);
            const float4 d3 = *reinterpret_cast<const float4*>(p + (s + 3) * slab);
            x.x += (d0.x + d1.x) + (d2.x + d3.x);
            x.y += (d0.y + d1.y) + (d2.y + d3.y);
            x.z += (d0.z + d1.z) + (d2.z + d3.z);
            x.w += (d0.w + d1.w) + (d2.w + d3.w);
          }
          for (; s < nsplit; ++s) {
            const float4 d = *reinterpret_cast<const float4*>(p + s * slab);
            x.x += d.x; x.y += d.y; x.z += d.z; x.w += d.w;
          }
        }
      }
      if constexpr (MODE != 0) *reinterpret_cast<float4*>(rrow + i) = x;
      v[it] = x;
      ss += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
    }
  }
  if (DSSE_PIPE_STAMPS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long st1 = stamps::now();  // the row's values (and slab sums) landed
  ss = wave_sum(ss);
  __shared__ float red[16];
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  float tot = 0.f;
  for (int i = 0; i < (nt >> 6); ++i) tot += red[i];
  const float inv = rsqrtf(tot / (float)H + eps);
  const unsigned long long st2 = stamps::now();
#pragma unroll
  for (int it = 0; it < kMaxIt; ++it) {
    if (it < nit) {
      const int i = (it * nt + tid) * 4;
      bf16x4 o;
      o[0] = f2bf(v[it].x * inv * bf2f(wv[it][0]));
      o[1] = f2bf(v[it].y * inv * bf2f(wv[it][1]));
      o[2] = f2bf(v[it].z * inv * bf2f(wv[it][2]));
      o[3] = f2bf(v[it].w * inv * bf2f(wv[it][3]));
      *reinterpret_cast<bf16x4*>(y + (size_t)m * H + i) = o;
    }
  }
  stamps::record(stamps::kNorm | MODE << 8, st0, st1, st2);
}

// ---- K4 (prefill side): RoPE on q/k + paged KV write from a library-GEMM QKV output ----------
// qkv: [T, (hq + 2 hkv) * 128] bf16 in the engine's permuted column order (inside each 16-column
// tile j of a head: columns 0..7 = dims 8j..8j+7, columns 8..15 = dims 64+8j..64+8j+7).
// A token's rows: each thread rotates 8 pairs of one (unit, tile j) with 16-byte loads and stores.
// KV = bf16, or f8 (FP8 cache: K rows are quantised from the rotated fp32 value with 1 / k_scale, 8-byte stores).
template <typename KV>
DEV void rope_kv_rows(const bf16* __restrict__ qkv, int hq, int hkv, const int* __restrict__ positions,
                      const int* __restrict__ slots, const float2* __restrict__ rope, bf16* __restrict__ q_out,
                      KV* __restrict__ k_cache, int num_slots, int rope_len, int t, float k_inv) {
  constexpr bool F8 = sizeof(KV) == 1;
  const int ncols = (hq + 2 * hkv) * 128;
  const bf16* row = qkv + (size_t)t * ncols;
  const int pos = DSSE_IDX(positions[t], rope_len, 0);
  const int slot = slots[t] < 0 ? -1 : DSSE_IDX(slots[t], num_slots, -1);
  const int blk = slot >= 0 ? slot / kPageTok : 0, off = slot >= 0 ? slot % kPageTok : 0;
  const int nrot = (hq + hkv) * 8;  // q and k heads x 8 column tiles (V: v_page_write)
  for (int idx = threadIdx.x; idx < nrot; idx += blockDim.x) {
    const int u = idx >> 3, j = idx & 7;
    bf16* dst = nullptr;
    KV* kdst = nullptr;  // F8: the key row (q rows stay bf16)
    if constexpr (F8) {
      if (u < hq) dst = q_out + ((size_t)t * hq + u) * 128;
      else if (slot >= 0) kdst = k_cache + (((size_t)blk * hkv + (u - hq)) * kPageTok + off) * 128;
      if (dst == nullptr && kdst == nullptr) continue;
    } else {
      dst = u < hq ? q_out + ((size_t)t * hq + u) * 128
                   : (slot >= 0 ? k_cache + (((size_t)blk * hkv + (u - hq)) * kPageTok + off) * 128 : nullptr);
      if (dst == nullptr) continue;
    }
    const bf16x8 x1 = ld_bf16x8(row + u * 128 + 16 * j);
    const bf16x8 x2 = ld_bf16x8(row + u * 128 + 16 * j + 8);
    const float4* cs4 = reinterpret_cast<const float4*>(rope + (size_t)pos * 64 + 8 * j);
    if constexpr (F8) {
      if (kdst != nullptr) {
        float f1[8], f2[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float4 cs = cs4[e];
          const float a0 = bf2f(x1[2 * e]), b0 = bf2f(x2[2 * e]), a1 = bf2f(x1[2 * e + 1]), b1 = bf2f(x2[2 * e + 1]);
          f1[2 * e] = a0 * cs.x - b0 * cs.y;
          f2[2 * e] = b0 * cs.x + a0 * cs.y;
          f1[2 * e + 1] = a1 * cs.z - b1 * cs.w;
          f2[2 * e + 1] = b1 * cs.z + a1 * cs.w;
        }
        *reinterpret_cast<uint2*>(kdst + 8 * j) = quant_f8x8(f1, k_inv);
        *reinterpret_cast<uint2*>(kdst + 64 + 8 * j) = quant_f8x8(f2, k_inv);
        continue;
      }
    }
    bf16x8 o1, o2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float4 cs = cs4[e];  // (cos, sin) of pairs 2e and 2e + 1
      const float a0 = bf2f(x1[2 * e]), b0 = bf2f(x2[2 * e]), a1 = bf2f(x1[2 * e + 1]), b1 = bf2f(x2[2 * e + 1]);
      o1[2 * e] = f2bf(a0 * cs.x - b0 * cs.y);
      o2[2 * e] = f2bf(b0 * cs.x + a0 * cs.y);
      o1[2 * e + 1] = f2bf(a1 * cs.z - b1 * cs.w);
      o2[2 * e + 1] = f2bf(b1 * cs.z + a1 * cs.w);
    }
    *reinterpret_cast<bf16x8*>(dst + 8 * j) = o1;
    *reinterpret_cast<bf16x8*>(dst + 64 + 8 * j) = o2;
  }
}

// ---- V into the transposed, token-permuted pages, a page row at a time -----------------------------------------
// A per-token form writes 2 bytes per (token, d): 128 scattered stores per head per token.  Here 128 threads take
// 32 consecutive rows x one kv head; thread d gathers its 32 values (coalesced
// over d) and, when the 32 rows fill one whole page in order (prefill of a page-aligned run), writes the page's row
// d as 4 x 16-byte stores in the vperm token order.  Other groups (page boundaries, padding, scattered slots) fall
// back to per-element stores.
// (rows t0 .. t0 + 31, kv head h, dim d = the thread's index in its 128-thread half; a wave never spans two heads)
// FP8 cache (KV = f8): the page row is 32 bytes, written as 4 x 8-byte runs; values quantised with 1 / v_scale.
template <typename KV>
DEV void v_page_write(const bf16* __restrict__ qkv, int T, int hq, int hkv, const int* __restrict__ slots,
                      KV* __restrict__ v_cache, int num_slots, int t0, int h, int d, float v_inv) {
  constexpr bool F8 = sizeof(KV) == 1;
  const int ncols = (hq + 2 * hkv) * 128;
  const int lane = threadIdx.x & 63;
  const int tl = t0 + (lane & 31);
  const int my_slot = tl < T ? (slots[tl] < 0 ? -1 : DSSE_IDX(slots[tl], num_slots, -1)) : -1;
  const int s0 = __shfl(my_slot, 0);
  const bool whole = __all(s0 >= 0 && s0 % kPageTok == 0 && my_slot == s0 + (lane & 31));
  // qkv columns are in the engine's permuted order: inside 16-column tile j, columns 0-7 = dims 8j..8j+7 and columns
  // 8-15 = dims 64 + 8j .. 64 + 8j + 7
  const int col = d < 64 ? 16 * (d >> 3) + (d & 7) : 16 * ((d - 64) >> 3) + 8 + (d & 7);
  const bf16* src = qkv + (size_t)t0 * ncols + (hq + hkv + h) * 128 + col;
  if (whole) {
    bf16 v[kPageTok];
#pragma unroll
    for (int i = 0; i < kPageTok; ++i) v[i] = src[(size_t)i * ncols];
    KV* dst = v_cache + (((size_t)(s0 / kPageTok) * hkv + h) * 128 + d) * kPageTok;
    if constexpr (F8) {
      float o[4][8];
#pragma unroll
      for (int i = 0; i < kPageTok; ++i) o[vperm_tok(i) >> 3][vperm_tok(i) & 7] = bf2f(v[i]);
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<uint2*>(dst + 8 * q) = quant_f8x8(o[q], v_inv);
    } else {
      bf16x8 o[4];
#pragma unroll
      for (int i = 0; i < kPageTok; ++i) o[vperm_tok(i) >> 3][vperm_tok(i) & 7] = v[i];
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<bf16x8*>(dst + 8 * q) = o[q];
    }
    return;
  }
  for (int i = 0; i < kPageTok && t0 + i < T; ++i) {
    const int sl = __shfl(my_slot, i);
    if (sl < 0) continue;
    KV* vd = v_cache + (((size_t)(sl / kPageTok) * hkv + h) * 128 + d) * kPageTok + vperm_tok(sl % kPageTok);
    if constexpr (F8) *vd = quant_f8(bf2f(src[(size_t)i * ncols]), v_inv);
    else *vd = src[(size_t)i * ncols];
  }
}

// One launch for both: blocks [0, T) rotate q / k of one token each (rope_kv_rows), the blocks after
// them write V page rows, two kv heads per 256-thread block.
template <typename KV>
__global__ void __launch_bounds__(256)
rope_kv_v_kernel(const bf16* __restrict__ qkv, int T, int hq, int hkv, const int* __restrict__ positions,
                 const int* __restrict__ slots, const float2* __restrict__ rope, bf16* __restrict__ q_out,
                 KV* __restrict__ k_cache, KV* __restrict__ v_cache, int num_slots, int rope_len, float k_inv,
                 float v_inv) {
  if ((int)blockIdx.x < T) {
    rope_kv_rows<KV>(qkv, hq, hkv, positions, slots, rope, q_out, k_cache, num_slots, rope_len, blockIdx.x, k_inv);
    return;
  }
  const int vb = blockIdx.x - T, hpairs = (hkv + 1) / 2;
  const int h = 2 * (vb % hpairs) + (threadIdx.x >> 7);
  if (h >= hkv) return;  // wave-uniform (128-thread halves)
  v_page_write<KV>(qkv, T, hq, hkv, slots, v_cache, num_slots, (vb / hpairs) * kPageTok, h, threadIdx.x & 127, v_inv);
}

// ---- FP8 cache: RoPE + q store + quantised paged KV write from the QKV projection's fp32 output ----------------
// y: [M, (hq + 2 hkv) * 128] fp32 sums in the engine's permuted column order (any decode / tiled GEMM in its fp32
// store mode).  K and V are quantised from the fp32 rotated / summed value -- one rounding, as ops/reference.py
// defines it.  One thread per (row, 16-column tile, j < 8): columns 16 tile + j and + 8 (the rotary partners).
__global__ void __launch_bounds__(256)
qkv_rope_f32_kernel(const float* __restrict__ y, int M, int hq, int hkv, const int* __restrict__ positions,
                    const int* __restrict__ slots, const float2* __restrict__ rope, bf16* __restrict__ q_out,
                    f8* __restrict__ k_cache, f8* __restrict__ v_cache, int num_slots, int rope_len, float k_inv,
                    float v_inv) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int tiles = (hq + 2 * hkv) * 8;
  if (idx >= M * tiles * 8) return;
  const int j = idx & 7, tile = (idx >> 3) % tiles, m = (idx >> 3) / tiles;
  const size_t base = (size_t)m * tiles * 16 + tile * 16 + j;
  const float a = y[base], b = y[base + 8];
  const int unit = tile >> 3, tj = tile & 7;
  const int d = 8 * tj + j;  // a: head dim d, b: d + 64
  const int s = slots[m] < 0 ? -1 : DSSE_IDX(slots[m], num_slots, -1);
  const int blk = s >= 0 ? s / kPageTok : 0, off = s >= 0 ? s % kPageTok : 0;
  if (unit < hq + hkv) {
    const float2 cs = rope[(size_t)DSSE_IDX(positions[m], rope_len, 0) * 64 + d];
    const float r1 = a * cs.x - b * cs.y, r2 = b * cs.x + a * cs.y;
    if (unit < hq) {
      bf16* q = q_out + ((size_t)m * hq + unit) * 128;
      q[d] = f2bf(r1);
      q[64 + d] = f2bf(r2);
    } else if (s >= 0) {
      f8* k = k_cache + (((size_t)blk * hkv + (unit - hq)) * kPageTok + off) * 128;
      store_kv(k + d, r1, k_inv);
      store_kv(k + 64 + d, r2, k_inv);
    }
  } else if (s >= 0) {
    f8* v = v_cache + ((size_t)blk * hkv + (unit - hq - hkv)) * 128 * kPageTok + vperm_tok(off);
    store_kv(v + (size_t)d * kPageTok, a, v_inv);
    store_kv(v + (size_t)(64 + d) * kPageTok, b, v_inv);
  }
}

// ---- SiLU·mul over the interleaved gate/up output of a library GEMM (prefill) ---------------
// gu: [T, 2F] with 16-column tiles (0..7 gate[8t..8t+7], 8..15 up[8t..8t+7]) -> h: [T, F]
// Block (x, y) takes 1024 tiles of row y (grid-strided over rows past 65535): each thread loads its four tiles'
// gate and up halves (8 x 16 B in flight) before it computes -- the one-tile-per-iteration form with a 64-bit
// division per tile ran the 8k-row pass at 5.9 TB/s.
__global__ void __launch_bounds__(256)
silu_mul_kernel(const bf16* __restrict__ gu, bf16* __restrict__ h, int F, int T) {
  const int tiles = F / 8;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    const bf16* src = gu + (size_t)t * 2 * F;
    bf16* dst = h + (size_t)t * F;
    const int tile0 = blockIdx.x * 1024 + threadIdx.x;
    bf16x8 gv[4], uv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int tile = tile0 + 256 * u;
      if (tile < tiles) {
        gv[u] = *reinterpret_cast<const bf16x8*>(src + tile * 16);
        uv[u] = *reinterpret_cast<const bf16x8*>(src + tile * 16 + 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int tile = tile0 + 256 * u;
      if (tile < tiles) {
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf(silu(bf2f(gv[u][j])) * bf2f(uv[u][j]));
        *reinterpret_cast<bf16x8*>(dst + tile * 8) = o;
      }
    }
  }
}

// ---- decode-step metadata (runs first inside the captured graph) -----------------------------
// For slot b: live sequences process the token at positions[b]; dead slots write nothing.
constexpr int kPrepThreads = 256;
__global__ void __launch_bounds__(kPrepThreads) decode_prep_kernel(int B, const int* __restrict__ active, const int* __restrict__ positions,
                                   const int* __restrict__ block_tables, int max_blocks, int num_blocks,
                                   int* __restrict__ slots, int* __restrict__ ctx_len,
                                   int* __restrict__ q_len) {
  const int b = blockIdx.x * kPrepThreads + threadIdx.x;  // (blockDim is a hidden kernel argument)
  if (b >= B) return;
  if (active[b]) {
    const int pos = positions[b];
    const int page = DSSE_IDX(block_tables[(size_t)b * max_blocks + DSSE_IDX(pos / kPageTok, max_blocks, 0)],
                              num_blocks, 0);
    slots[b] = page * kPageTok + pos % kPageTok;
    ctx_len[b] = pos + 1;
    q_len[b] = 1;
  } else {
    slots[b] = -1;
    ctx_len[b] = 0;
    q_len[b] = 0;
  }
}

// Token-ring head advance (one thread), the last node of a step.
__global__ void ring_advance_kernel(int* counter) { counter[0] += 1; }

}  // namespace dsse

using namespace dsse;

extern "C" hipError_t dsse_rmsnorm(int mode, int M, float* resid, int H, const void* delta,
                                   const void* embed, const int* ids, const void* w, void* y,
                                   float eps, const float* part, int nsplit, int vocab, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  const bf16* d = reinterpret_cast<const bf16*>(delta);
  const bf16* e = reinterpret_cast<const bf16*>(embed);
  const bf16* wp = reinterpret_cast<const bf16*>(w);
  bf16* yp = reinterpret_cast<bf16*>(y);
  // nit float4s per thread, nt threads: H == 4 nt nit exactly (H = 5120: 640 threads x 2), nt whole waves
  const int nit = (H / 4 + 1023) / 1024, nt = H / 4 / nit;
  if (nit > 2 || 4 * nt * nit != H || nt % 64 != 0) return hipErrorInvalidValue;
  switch (mode) {
    case 0: hipLaunchKernelGGL(rmsnorm_kernel<0>, dim3(M), dim3(nt), 0, st, resid, part, wp, ids, e, nt, nit, nsplit, M, d, yp, eps, vocab); break;
    case 1: hipLaunchKernelGGL(rmsnorm_kernel<1>, dim3(M), dim3(nt), 0, st, resid, part, wp, ids, e, nt, nit, nsplit, M, d, yp, eps, vocab); break;
    case 2: hipLaunchKernelGGL(rmsnorm_kernel<2>, dim3(M), dim3(nt), 0, st, resid, part, wp, ids, e, nt, nit, nsplit, M, d, yp, eps, vocab); break;
    case 3: hipLaunchKernelGGL(rmsnorm_kernel<3>, dim3(M), dim3(nt), 0, st, resid, part, wp, ids, e, nt, nit, nsplit, M, d, yp, eps, vocab); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

extern "C" hipError_t dsse_rope_kv_write(int T, const void* qkv, int hq, int hkv, const int* positions,
                                         const int* slots, const float2* rope, void* q_out,
                                         void* k_cache, void* v_cache, int num_slots, int rope_len,
                                         hipStream_t st) {
  if (T <= 0) return hipSuccess;
  const int vblocks = (T + kPageTok - 1) / kPageTok * ((hkv + 1) / 2);
  hipLaunchKernelGGL(rope_kv_v_kernel<bf16>, dim3(T + vblocks), dim3(256), 0, st, reinterpret_cast<const bf16*>(qkv), T,
                     hq, hkv, positions, slots, rope, reinterpret_cast<bf16*>(q_out), reinterpret_cast<bf16*>(k_cache),
                     reinterpret_cast<bf16*>(v_cache), num_slots, rope_len, 1.f, 1.f);
  return hipGetLastError();
}

// FP8 (e4m3) cache form of dsse_rope_kv_write: k_inv = 1 / k_scale, v_inv = 1 / v_scale.
extern "C" hipError_t dsse_rope_kv_write_f8(int T, const void* qkv, int hq, int hkv, const int* positions,
                                            const int* slots, const float2* rope, void* q_out, void* k_cache,
                                            void* v_cache, int num_slots, int rope_len, float k_inv, float v_inv,
                                            hipStream_t st) {
  if (T <= 0) return hipSuccess;
  const int vblocks = (T + kPageTok - 1) / kPageTok * ((hkv + 1) / 2);
  hipLaunchKernelGGL(rope_kv_v_kernel<f8>, dim3(T + vblocks), dim3(256), 0, st, reinterpret_cast<const bf16*>(qkv), T,
                     hq, hkv, positions, slots, rope, reinterpret_cast<bf16*>(q_out), reinterpret_cast<f8*>(k_cache),
                     reinterpret_cast<f8*>(v_cache), num_slots, rope_len, k_inv, v_inv);
  return hipGetLastError();
}

// FP8 cache: the QKV projection's epilogue from its fp32 output y [M, (hq + 2 hkv) * 128] (qkv_rope_f32_kernel).
extern "C" hipError_t dsse_qkv_rope_f8(int M, const float* y, int hq, int hkv, const int* positions, const int* slots,
                                       const float2* rope, void* q_out, void* k_cache, void* v_cache, int num_slots,
                                       int rope_len, float k_inv, float v_inv, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  const long threads = (long)M * (hq + 2 * hkv) * 64;
  hipLaunchKernelGGL(qkv_rope_f32_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, y, M, hq, hkv,
                     positions, slots, rope, reinterpret_cast<bf16*>(q_out), reinterpret_cast<f8*>(k_cache),
                     reinterpret_cast<f8*>(v_cache), num_slots, rope_len, k_inv, v_inv);
  return hipGetLastError();
}

extern "C" hipError_t dsse_silu_mul(int T, int F, const void* gu, void* h, hipStream_t st) {
  if (T <= 0) return hipSuccess;
  const dim3 grid((F / 8 + 1023) / 1024, std::min(T, 65535));
  hipLaunchKernelGGL(silu_mul_kernel, grid, dim3(256), 0, st,
                     reinterpret_cast<const bf16*>(gu), reinterpret_cast<bf16*>(h), F, T);
  return hipGetLastError();
}

extern "C" hipError_t dsse_decode_prep(int B, const int* active, const int* positions,
                                       const int* block_tables, int max_blocks, int num_blocks, int* slots,
                                       int* ctx_len, int* q_len, hipStream_t st) {
  hipLaunchKernelGGL(decode_prep_kernel, dim3((B + kPrepThreads - 1) / kPrepThreads), dim3(kPrepThreads), 0, st, B, active,
                     positions, block_tables, max_blocks, num_blocks, slots, ctx_len, q_len);
  return hipGetLastError();
}

extern "C" hipError_t dsse_ring_advance(int* counter, hipStream_t st) {
  hipLaunchKernelGGL(ring_advance_kernel, dim3(1), dim3(1), 0, st, counter);
  return hipGetLastError();
}

DSSE_CHECK_READER(dsse_check_elementwise)
DSSE_STAMPS_BINDER(dsse_stamps_bind_elementwise)
