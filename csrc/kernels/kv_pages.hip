// KV page movers.  For the prefix cache's host tier (engine/kv_cache.py HostPageStore, engine/model_runner.py
// KVOffload): gather whole pages of the paged cache into contiguous staging records, and scatter records back.  For
// parallel sampling (engine/engine.py _admit): copy pages onto pages inside the cache (kv_pages_copy_kernel below).
//
// The cache is K [L, blocks, Hkv, 32, 128] and V [L, blocks, Hkv, 128, 32], so one page is 2 L segments of
// seg = Hkv * 4096 * itemsize bytes (one per layer and per K / V), blocks * seg bytes apart.  A staging record is the
// page's segments back to back: [K layer 0 .. K layer L-1 | V layer 0 .. V layer L-1] = 2 L seg bytes.
//
// Pure byte movers: one instantiation serves bf16 and fp8 caches.  Grid (2 L, n): workgroup (s, i) copies the whole
// segment s of listed page (or pair) i, 16 bytes per lane per access, four accesses in flight per lane.  The block
// list is read from device memory.  Gather / scatter loads are non-temporal (every byte is read once; they bypass the
// vector L1 and cost nothing against plain loads at 16 bytes per lane), stores are plain: a scattered page is read by
// the next step's attention, and a gathered record by the copy engine right after the launch, so neither wants to
// leave the L2 early.  The page-to-page copy loads plainly (see its kernel).
//
// The host validates the block list before the launch (ops.kv_pages_gather / kv_pages_scatter / kv_pages_copy); a
// workgroup whose index is out of range nevertheless copies nothing, in every build, and the checked build records it
// (DSSE_IDX).
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

// Page-to-page copy inside the cache (parallel sampling, the fork branch of engine/engine.py _admit: a sibling choice
// gets a private copy of its parent's partial last prompt page).  pairs = [n, 2] int32 (src_block, dst_block);
// workgroup (s, i) copies segment s of page pairs[i][0] onto the same segment of page pairs[i][1].  One source may
// feed several destinations;
// the host guarantees (ops.kv_pages_copy) that destinations are distinct and that none is also a source, so no
// workgroup reads what another writes.  The whole page moves, written slots or not: slots past the copied prefix are
// overwritten by their new owner before any attention reads them (context lengths bound every read).  Plain loads here:
// the source page was just written by the parent's prompt pass and its lines are likely still in the L2.
__global__ void __launch_bounds__(kPageThreads)
kv_pages_copy_kernel(char* __restrict__ k_cache, char* __restrict__ v_cache, const int* __restrict__ pairs, int L,
                     int num_blocks, unsigned seg_bytes) {
  const int seg = blockIdx.x, pair = blockIdx.y;
  const int sb = DSSE_IDX(pairs[2 * pair], num_blocks, -1);
  const int db = DSSE_IDX(pairs[2 * pair + 1], num_blocks, -1);
  // (wave-uniform: nothing is touched for a bad index or a page copied onto itself)
  if ((unsigned)sb >= (unsigned)num_blocks || (unsigned)db >= (unsigned)num_blocks || sb == db) return;
  const bool is_v = seg >= L;
  const int layer = is_v ? seg - L : seg;
  char* base = (is_v ? v_cache : k_cache) + (size_t)layer * num_blocks * seg_bytes;
  const u32x4* src = reinterpret_cast<const u32x4*>(base + (size_t)sb * seg_bytes);
  u32x4* dst = reinterpret_cast<u32x4*>(base + (size_t)db * seg_bytes);
  const unsigned n = seg_bytes / 16;
  for (unsigned i = threadIdx.x; i < n; i += kPageThreads * kPageUnroll) {
    u32x4 v[kPageUnroll];
#pragma unroll
    for (int j = 0; j < kPageUnroll; ++j)
      if (i + j * kPageThreads < n) v[j] = src[i + j * kPageThreads];
#pragma unroll
    for (int j = 0; j < kPageUnroll; ++j)
      if (i + j * kPageThreads < n) dst[i + j * kPageThreads] = v[j];
  }
}

}  // namespace dsse

extern "C" hipError_t dsse_kv_pages_copy(int n, void* k_cache, void* v_cache, const int* pairs, int L, int num_blocks,
                                         unsigned seg_bytes, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(dsse::kv_pages_copy_kernel, dim3(2 * L, n), dim3(dsse::kPageThreads), 0, st, (char*)k_cache,
                     (char*)v_cache, pairs, L, num_blocks, seg_bytes);
  return hipGetLastError();
}

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
