// Multi-LoRA low-rank products for mixed batches (docs/kernels.md, "LoRA"): every row of a step names its own
// adapter slot (row_adapter[i], -1 = none), so the two products are per-row dot products ("bgmv") over 16-byte
// vector loads, not one GEMM:
//
//   lora_shrink      t[i, j]    = sum_k A_a[j, k] * x[i, k]                        a = row_adapter[i], j < S*R
//   lora_expand_add  out[i, n] += scale[a] * sum_{j < R} B_a[n, j] * t[i, slice(n)*R + j]
//
// A_a is the adapter's stacked A matrices [S*R, K] (S = 3 for qkv, 2 for gate_up, 1 for o / down: one shrink reads x
// once), B_a is [N, R] in the engine's output-row order, and slice(n) = slice_of_row[n] says which R columns of t
// output row n reads.  A and B of one projection are at most 1.8 MB and live in L2: the kernels are bound by launches
// and L2 traffic.  A workgroup covers kLoraRows consecutive rows and reloads its A / B fragment only where the adapter
// changes from one row to the next, so a prompt chunk's run of rows under one adapter loads the fragment once.
//
// Each (i, j) and (i, n) sum has one fixed order that does not depend on the other rows of the batch: a row's result
// is bit-identical whatever rides beside it.  Rows with adapter -1 (and, defensively, with an adapter past the pool)
// write zeros to t and leave `out` untouched.
#include "api.h"
#include "common.h"

namespace dsse {

constexpr int kLoraRows = 8;  // rows per workgroup (both kernels)
constexpr int kLoraJ = 4;     // shrink: outputs per wave (a workgroup of 4 waves: 16 outputs)
constexpr int kLoraCols = 256;  // expand: output columns per workgroup (one per thread)

// The adapter slot of row `row` as a wave-uniform value: -1 for rows past M, rows without an adapter, and slots past
// the pool (recorded by the checked build).
DEV int lora_row_adapter(const int* __restrict__ row_adapter, int row, int M, int nslots) {
  int a = row < M ? row_adapter[row] : -1;
  a = a < 0 ? -1 : DSSE_IDX(a, nslots, -1);
  if (a >= nslots) a = -1;
  return __builtin_amdgcn_readfirstlane(a);
}

// grid (ceil(M / kLoraRows), ceil(SR / 16)), 256 threads.  Wave w of workgroup (bx, by) owns outputs
// [j0, j0 + kLoraJ), j0 = (4 by + w) kLoraJ, of rows [kLoraRows bx, +kLoraRows): lane l sums k = 8 l + 512 m, then
// the 64 partial sums are added across the wave.  K % 8 == 0, SR % 4 == 0.
__global__ __launch_bounds__(256) void lora_shrink_kernel(const bf16* __restrict__ x, const bf16* __restrict__ A,
                                                          const int* __restrict__ row_adapter, float* __restrict__ t,
                                                          int M, int K, int SR, int nslots) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * kLoraRows;
  const int j0 = (blockIdx.y * 4 + wave) * kLoraJ;
  if (j0 >= SR) return;  // (no barrier in this kernel)
  int adp[kLoraRows];
#pragma unroll
  for (int r = 0; r < kLoraRows; ++r) adp[r] = lora_row_adapter(row_adapter, row0 + r, M, nslots);
  float acc[kLoraRows][kLoraJ];
#pragma unroll
  for (int r = 0; r < kLoraRows; ++r)
#pragma unroll
    for (int jj = 0; jj < kLoraJ; ++jj) acc[r][jj] = 0.f;
  for (int k = lane * 8; k < K; k += kWave * 8) {
    int prev = -1;
    bf16x8 af[kLoraJ];
#pragma unroll
    for (int r = 0; r < kLoraRows; ++r) {
      const int a = adp[r];
      if (a < 0) continue;
      if (a != prev) {  // the run's fragment: loaded once per adapter change
#pragma unroll
        for (int jj = 0; jj < kLoraJ; ++jj) af[jj] = ld_bf16x8(A + ((size_t)a * SR + j0 + jj) * K + k);
        prev = a;
      }
      const bf16x8 xv = ld_bf16x8(x + (size_t)(row0 + r) * K + k);
#pragma unroll
      for (int jj = 0; jj < kLoraJ; ++jj)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r][jj] += bf2f(af[jj][e]) * bf2f(xv[e]);
    }
  }
#pragma unroll
  for (int r = 0; r < kLoraRows; ++r) {
    if (row0 + r >= M) break;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (adp[r] >= 0) {
#pragma unroll
      for (int jj = 0; jj < kLoraJ; ++jj) v[jj] = wave_sum(acc[r][jj]);
    }
    if (lane == 0) *reinterpret_cast<f32x4*>(t + (size_t)(row0 + r) * SR + j0) = v;
  }
}

DEV float lora_ld(const float* p) { return *p; }
DEV float lora_ld(const bf16* p) { return bf2f(*p); }
DEV void lora_st(float* p, float v) { *p = v; }
DEV void lora_st(bf16* p, float v) { *p = f2bf(v); }

// grid (ceil(M / kLoraRows), ceil(N / kLoraCols)), 256 threads.  The workgroup stages its rows' t in LDS (S R floats
// per row), then thread c owns output column n = kLoraCols by + c of every row: B_a[n, :] in registers (R bf16),
// reloaded where the adapter changes, R fused multiply-adds per row against its slice of t (LDS broadcast reads).
template <int R, typename OutT>
__global__ __launch_bounds__(256) void lora_expand_kernel(const float* __restrict__ t, const bf16* __restrict__ B,
                                                          const float* __restrict__ scale,
                                                          const int* __restrict__ row_adapter,
                                                          const int* __restrict__ slice_of_row, OutT* __restrict__ out,
                                                          int M, int N, int S, int nslots) {
  __shared__ __attribute__((aligned(16))) float ts[kLoraRows][3 * R];
  const int row0 = blockIdx.x * kLoraRows;
  const int SR = S * R;  // S <= 3 (the host checks)
  for (int i = threadIdx.x; i < kLoraRows * SR; i += 256) {
    const int r = i / SR, c = i - r * SR;
    ts[r][c] = row0 + r < M ? t[(size_t)(row0 + r) * SR + c] : 0.f;
  }
  int adp[kLoraRows];
#pragma unroll
  for (int r = 0; r < kLoraRows; ++r) adp[r] = lora_row_adapter(row_adapter, row0 + r, M, nslots);
  __syncthreads();
  const int n = blockIdx.y * kLoraCols + threadIdx.x;
  if (n >= N) return;
  int s = DSSE_IDX(slice_of_row[n], S, 0);
  s = s < 0 ? 0 : (s >= S ? S - 1 : s);
  int prev = -1;
  bf16x8 bfr[R / 8];
  float sc = 0.f;
#pragma unroll
  for (int r = 0; r < kLoraRows; ++r) {
    const int a = adp[r];
    if (a < 0) continue;  // the row keeps its bits
    if (a != prev) {
#pragma unroll
      for (int c = 0; c < R / 8; ++c) bfr[c] = ld_bf16x8(B + ((size_t)a * N + n) * R + c * 8);
      sc = scale[a];
      prev = a;
    }
    const float* tp = &ts[r][s * R];
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < R / 8; ++c) {
      const f32x4 t0 = *reinterpret_cast<const f32x4*>(tp + c * 8);
      const f32x4 t1 = *reinterpret_cast<const f32x4*>(tp + c * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += bf2f(bfr[c][e]) * t0[e];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += bf2f(bfr[c][4 + e]) * t1[e];
    }
    OutT* o = out + (size_t)(row0 + r) * N + n;
    lora_st(o, lora_ld(o) + sc * acc);  // the scale multiplies the fp32 sum, B stays unscaled bf16
  }
}

template <int R>
void lora_expand_launch(dim3 grid, hipStream_t st, bool f32, const float* t, const bf16* B, const float* scale,
                        const int* row_adapter, const int* slice_of_row, void* out, int M, int N, int S, int nslots) {
  if (f32)
    hipLaunchKernelGGL((lora_expand_kernel<R, float>), grid, dim3(256), 0, st, t, B, scale, row_adapter, slice_of_row,
                       reinterpret_cast<float*>(out), M, N, S, nslots);
  else
    hipLaunchKernelGGL((lora_expand_kernel<R, bf16>), grid, dim3(256), 0, st, t, B, scale, row_adapter, slice_of_row,
                       reinterpret_cast<bf16*>(out), M, N, S, nslots);
}

}  // namespace dsse

using namespace dsse;

extern "C" hipError_t dsse_lora_shrink(int M, int K, int SR, int nslots, const void* x, const void* A,
                                       const int* row_adapter, float* t, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  if (K % 8 != 0 || SR % kLoraJ != 0 || SR <= 0 || nslots <= 0) return hipErrorInvalidValue;
  const dim3 grid((M + kLoraRows - 1) / kLoraRows, (SR + 4 * kLoraJ - 1) / (4 * kLoraJ));
  hipLaunchKernelGGL(lora_shrink_kernel, grid, dim3(256), 0, st, reinterpret_cast<const bf16*>(x),
                     reinterpret_cast<const bf16*>(A), row_adapter, t, M, K, SR, nslots);
  return hipGetLastError();
}

extern "C" hipError_t dsse_lora_expand(int M, int N, int R, int S, int nslots, int out_f32, const float* t,
                                       const void* B, const float* scale, const int* row_adapter,
                                       const int* slice_of_row, void* out, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  if (S < 1 || S > 3 || N <= 0 || nslots <= 0) return hipErrorInvalidValue;
  const dim3 grid((M + kLoraRows - 1) / kLoraRows, (N + kLoraCols - 1) / kLoraCols);
  const bf16* b = reinterpret_cast<const bf16*>(B);
  switch (R) {
    case 8: lora_expand_launch<8>(grid, st, out_f32, t, b, scale, row_adapter, slice_of_row, out, M, N, S, nslots); break;
    case 16: lora_expand_launch<16>(grid, st, out_f32, t, b, scale, row_adapter, slice_of_row, out, M, N, S, nslots); break;
    case 32: lora_expand_launch<32>(grid, st, out_f32, t, b, scale, row_adapter, slice_of_row, out, M, N, S, nslots); break;
    case 64: lora_expand_launch<64>(grid, st, out_f32, t, b, scale, row_adapter, slice_of_row, out, M, N, S, nslots); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

DSSE_CHECK_READER(dsse_check_lora)
