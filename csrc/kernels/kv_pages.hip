// KV page movers of the prefix cache's host tier (engine/kv_cache.py HostPageStore, engine/model_runner.py
// KVOffload): gather whole pages of the paged cache into contiguous staging records, and scatter records back.
//
// The cache is K [L, blocks, Hkv, 32, 128] and V [L, blocks, Hkv, 128, 32], so one page is 2 L segments of
// seg = Hkv * 4096 * itemsize bytes (one per layer and per K / V), blocks * seg bytes apart.  A staging record is the
// page's segments back to back: [K layer 0 .. K layer L-1 | V layer 0 .. V layer L-1] = 2 L seg bytes.
//
// Pure byte movers: one instantiation serves bf16 and fp8 caches.  Grid (2 L, n): workgroup (s, i) copies the whole
// segment s of listed page i, 16 bytes per lane per access, four accesses in flight per lane.  The block list is read
// from device memory.  Loads are non-temporal (every byte is read once; they bypass the vector L1 and cost nothing
// against plain loads at 16 bytes per lane), stores are plain: a scattered page is read by the next step's attention,
// and a gathered record by the copy engine right after the launch, so neither wants to leave the L2 early.
//
// The host validates the block list before the launch (ops.kv_pages_gather / kv_pages_scatter); a workgroup whose
// index is out of range nevertheless copies nothing, in every build, and the checked build records it (DSSE_IDX).
#include "api.h"

namespace dsse {

constexpr int kPageThreads = 256;
constexpr int kPageUnroll = 4;

template <bool GATHER>
__global__ void __launch_bounds__(kPageThreads)
kv_pages_kernel(char* __restrict__ k_cache, char* __restrict__ v_cache, const int* __restrict__ blocks,
                char* __restrict__ staging, int L, int num_blocks, unsigned seg_bytes) {
  const int seg = blockIdx.x, page = blockIdx.y;
  const int b = DSSE_IDX(blocks[page], num_blocks, -1);
  if ((unsigned)b >= (unsigned)num_blocks) return;  // (wave-uniform: nothing is touched for a bad index)
  const bool is_v = seg >= L;
  const int layer = is_v ? seg - L : seg;
  char* cache = (is_v ? v_cache : k_cache) + ((size_t)layer * num_blocks + b) * seg_bytes;
  char* rec = staging + ((size_t)page * 2 * L + seg) * seg_bytes;
  const u32x4* src = reinterpret_cast<const u32x4*>(GATHER ? cache : rec);
  u32x4* dst = reinterpret_cast<u32x4*>(GATHER ? rec : cache);
  const unsigned n = seg_bytes / 16;
  for (unsigned i = threadIdx.x; i < n; i += kPageThreads * kPageUnroll) {
    u32x4 v[kPageUnroll];
#pragma unroll
    for (int j = 0; j < kPageUnroll; ++j)
      if (i + j * kPageThreads < n) v[j] = __builtin_nontemporal_load(src + i + j * kPageThreads);
#pragma unroll
    for (int j = 0; j < kPageUnroll; ++j)
      if (i + j * kPageThreads < n) dst[i + j * kPageThreads] = v[j];
  }
}

}  // namespace dsse

extern "C" hipError_t dsse_kv_pages(int gather, int n, void* k_cache, void* v_cache, const int* blocks, void* staging,
                                    int L, int num_blocks, unsigned seg_bytes, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const dim3 grid(2 * L, n), block(dsse::kPageThreads);
  if (gather)
    hipLaunchKernelGGL(dsse::kv_pages_kernel<true>, grid, block, 0, st, (char*)k_cache, (char*)v_cache, blocks,
                       (char*)staging, L, num_blocks, seg_bytes);
  else
    hipLaunchKernelGGL(dsse::kv_pages_kernel<false>, grid, block, 0, st, (char*)k_cache, (char*)v_cache, blocks,
                       (char*)staging, L, num_blocks, seg_bytes);
  return hipGetLastError();
}

DSSE_CHECK_READER(dsse_check_kv_pages)
