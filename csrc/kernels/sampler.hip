// K10 sampler: greedy / temperature / top-k / top-p with a counter-based Philox RNG.
//
// One 1024-thread workgroup per batch row; the row (<= 32768 logits) stays in registers
// (<= 32 per thread).  Sampling is exact Gumbel-max: argmax_i (x_i / T + G_i) with
// G_i = -log(-log(U_i)), U_i = Philox(seed, counter = (global vocab index, position)).  The
// noise depends only on (seed, position, global index), so a vocab-sharded (tensor-parallel)
// run draws the same token as TP = 1: each rank reports its (score, index) candidate and the
// candidates are merged by max (sample_pick_kernel).  top-k / top-p thresholds are found by an
// MSB-first 8-bit radix select over order-preserving float keys — counts for top-k, softmax
// mass for top-p — four passes each, no sort.
#include "api.h"

namespace dsse {


DEV uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr int kSThreads = 1024;   // filtered path: one workgroup per row
constexpr int kSMaxV = 32768;     // per-rank vocab limit (row staged in 128 KiB of LDS)
constexpr int kCThreads = 256;    // unfiltered path: one workgroup per (row, vocab chunk)

// min_p of row b (0 = off): slot-indexed, through row_slot where the rows are not the slots.
DEV float row_min_p(const SampleParams& p, int b) {
  if (!p.min_p) return 0.f;
  const int slot = DSSE_IDX(p.row_slot ? p.row_slot[b] : b, p.ctl_slots, -1);
  if ((unsigned)slot >= (unsigned)p.ctl_slots) return 0.f;
  const float mp = p.min_p[slot];
  return mp > 0.f ? fminf(mp, 1.f) : 0.f;
}

DEV bool row_filtered(const SampleParams& p, int b) {
  return p.temperature[b] > 0.f &&
         ((p.top_k[b] > 0 && p.top_k[b] < p.V) || p.top_p[b] < 1.f || row_min_p(p, b) > 0.f);
}

// Score of one logit: greedy -> the logit itself; sampling -> logit/T + Gumbel(seed, pos, gidx).
DEV float score(float logit, float inv_t, bool greedy, uint2 seed, uint32_t pos, int gidx) {
  if (greedy) return logit;
  const uint4 rv = philox4x32(make_uint4((uint32_t)gidx, pos, 0x5353u, 0u), seed);
  return logit * inv_t - __logf(-__logf(u01(rv.x)));
}

DEV void better(float& best, int& bidx, float s, int i) {
  if (s > best || (s == best && i < bidx)) { best = s; bidx = i; }
}

template <int NT>
DEV void block_argmax(float& best, int& bidx, float* s_best, int* s_bidx) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) better(best, bidx, __shfl_xor(best, o), __shfl_xor(bidx, o));
  if ((threadIdx.x & 63) == 0) { s_best[threadIdx.x >> 6] = best; s_bidx[threadIdx.x >> 6] = bidx; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < NT / 64; ++i) better(best, bidx, s_best[i], s_bidx[i]);
}

// Unfiltered rows (greedy or pure temperature): Gumbel-max is separable, so each (row, chunk)
// workgroup proposes the best (score, index) of its vocab slice.
// Both candidate kernels open by reading the row's switches (active, temperature, top-k / top-p / min_p): those
// pointers and the logits row's address lead the argument list (14 dwords, preloaded in SGPRs), so the first loads
// do not wait for a trip to the kernarg segment; the rest of SampleParams arrives under them.
#define DSSE_SAMPLE_LEAD const int *__restrict__ active, const float *__restrict__ temperature,                     \
                         const int *__restrict__ top_k, const float *__restrict__ top_p,                          \
                         const float *__restrict__ logits, const float *__restrict__ min_p, int ld, int V
#define DSSE_SAMPLE_ARGS(P) (P).active, (P).temperature, (P).top_k, (P).top_p, (P).logits, (P).min_p, (P).ld, (P).V, (P)
DEV SampleParams sample_params(DSSE_SAMPLE_LEAD, const SampleParams& rest) {
  SampleParams p = rest;  // the leading arguments are the same values
  p.active = active;
  p.temperature = temperature;
  p.top_k = top_k;
  p.top_p = top_p;
  p.logits = logits;
  p.min_p = min_p;
  p.ld = ld;
  p.V = V;
  return p;
}

__global__ void __launch_bounds__(kCThreads) sample_chunk_kernel(DSSE_SAMPLE_LEAD, SampleParams p_rest) {
  const SampleParams p = sample_params(active, temperature, top_k, top_p, logits, min_p, ld, V, p_rest);
  const int c = blockIdx.x, b = blockIdx.y;
  if ((p.active && !p.active[b]) || row_filtered(p, b)) return;
  __shared__ float s_best[kCThreads / 64];
  __shared__ int s_bidx[kCThreads / 64];
  const float temp = p.temperature[b];
  const bool greedy = !(temp > 0.f);
  const float inv_t = greedy ? 1.f : 1.f / temp;
  const uint2 seed = p.seeds[b];
  const uint32_t pos = (uint32_t)p.positions[b];
  const int chunk = (p.V + p.nchunks - 1) / p.nchunks;
  const int lo = c * chunk, hi = min(p.V, lo + chunk);
  const float* row = p.logits + (size_t)b * p.ld;
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  for (int i = lo + threadIdx.x; i < hi; i += kCThreads)
    better(best, bidx, score(row[i], inv_t, greedy, seed, pos, i + p.vocab_offset), i + p.vocab_offset);
  block_argmax<kCThreads>(best, bidx, s_best, s_bidx);
  if (threadIdx.x == 0) p.cand[(size_t)b * p.nchunks + c] = make_float2(best, __int_as_float(bidx));
}

// MSB-first radix select over LDS-resident base-2 logits.  Returns the key `thr` such that the
// elements with key >= thr form the smallest top set whose weight (count or softmax mass) reaches
// `target`; elements with key < floor_key are ignored.
template <bool MASS>
DEV uint32_t radix_select(const float* xs, int V, float xmax, uint32_t floor_key, float target, float* hist) {
  uint32_t prefix = 0, mask = 0;
  float remaining = target;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += kSThreads) hist[i] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < V; i += kSThreads) {
      const uint32_t k = fkey(xs[i]);
      if (k >= floor_key && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255], MASS ? exp2f(xs[i] - xmax) : 1.f);
    }
    __syncthreads();
    float cum = 0.f;
    int digit = 0;
    for (int d = 255; d >= 0; --d) {  // every thread scans the 256 bins (no extra barrier round)
      const float hv = hist[d];
      if (cum + hv >= remaining) { digit = d; break; }
      cum += hv;
    }
    remaining -= cum;
    prefix |= (uint32_t)digit << shift;
    mask |= 255u << shift;
    __syncthreads();
  }
  return prefix;
}

template <typename T>
DEV T block_sum(T v, T* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T tot = 0;
  for (int i = 0; i < kSThreads / 64; ++i) tot += sh[i];
  __syncthreads();
  return tot;
}
DEV float block_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float tot = -INFINITY;
  for (int i = 0; i < kSThreads / 64; ++i) tot = fmaxf(tot, sh[i]);
  __syncthreads();
  return tot;
}

// Rows with top-k / top-p: one workgroup per row, the whole (local) row staged in LDS.
__global__ void __launch_bounds__(kSThreads) sample_filtered_kernel(DSSE_SAMPLE_LEAD, SampleParams p_rest) {
  const SampleParams p = sample_params(active, temperature, top_k, top_p, logits, min_p, ld, V, p_rest);
  const int b = blockIdx.x;
  if ((p.active && !p.active[b]) || !row_filtered(p, b)) return;
  __shared__ float xs[kSMaxV];
  __shared__ float hist[256];
  __shared__ float sh[kSThreads / 64];
  __shared__ int shi[kSThreads / 64];
  const float inv_t = 1.f / p.temperature[b];
  const float* row = p.logits + (size_t)b * p.ld;
  float lmax = -INFINITY;
  for (int i = threadIdx.x; i < p.V; i += kSThreads) {
    const float x = row[i] * inv_t * 1.4426950408889634f;  // base-2 scaled
    xs[i] = x;
    lmax = fmaxf(lmax, x);
  }
  const float xmax = block_max(lmax, sh);
  uint32_t thr = 0;
  const int tk = p.top_k[b];
  const float tp = p.top_p[b];
  if (tk > 0 && tk < p.V) thr = radix_select<false>(xs, p.V, xmax, 0u, (float)tk, hist);
  // min_p: keep x_i / T - max_j x_j / T >= ln(min_p), one more top set of the same ordering -> one more key threshold
  // (this rank's shard under TP, like top-k / top-p); the top-p mass select below then works on the survivors
  const float mp = row_min_p(p, b);
  if (mp > 0.f) thr = max(thr, fkey(xmax + log2f(mp)));
  if (tp < 1.f) {
    float z = 0.f;
    for (int i = threadIdx.x; i < p.V; i += kSThreads)
      if (fkey(xs[i]) >= thr) z += exp2f(xs[i] - xmax);
    z = block_sum(z, sh);
    thr = radix_select<true>(xs, p.V, xmax, thr, tp * z, hist);
  }
  const uint2 seed = p.seeds[b];
  const uint32_t pos = (uint32_t)p.positions[b];
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  for (int i = threadIdx.x; i < p.V; i += kSThreads) {
    if (fkey(xs[i]) < thr) continue;
    const int gidx = i + p.vocab_offset;
    const uint4 rv = philox4x32(make_uint4((uint32_t)gidx, pos, 0x5353u, 0u), seed);
    better(best, bidx, xs[i] * 0.6931471805599453f - __logf(-__logf(u01(rv.x))), gidx);
  }
  block_argmax<kSThreads>(best, bidx, sh, shi);
  if (threadIdx.x == 0) {
    p.cand[(size_t)b * p.nchunks] = make_float2(best, __int_as_float(bidx));
    for (int c = 1; c < p.nchunks; ++c)
      p.cand[(size_t)b * p.nchunks + c] = make_float2(-INFINITY, __int_as_float(0x7fffffff));
  }
}

// ---- presence / frequency / repetition penalties -------------------------------------------------------------
// Per-slot state (slot-indexed like slot_meta, device resident): pen_meta = [presence | frequency | repetition |
// n_prompt] (host-owned, uploaded with the slot metadata) and the token history hist[slot] = [len | prompt tokens |
// generated tokens] (the engine uploads a row when it places a penalised sequence in the slot; afterwards the device
// owns it: the pick / commit passes append every sampled token in stream order, so steps enqueued ahead of the host
// see the right history).  vLLM's order, before temperature / top-k / top-p and under greedy, with c[v] = the
// occurrences of v among the generated tokens:
//   v in prompt or generated: x = x > 0 ? x / r : x * r;   x -= f c[v];   c[v] > 0: x -= p.
constexpr uint32_t kPenPrompt = 0x80000000u;  // count word: bit 31 = the prompt names the token, bits 0-30 = c[v]

DEV bool penalties_on(const int* __restrict__ pm, int Bm, int slot) {
  return __int_as_float(pm[slot]) != 0.f || __int_as_float(pm[Bm + slot]) != 0.f ||
         __int_as_float(pm[2 * Bm + slot]) != 1.f;
}

// One workgroup per logits row.  A row that is inactive or whose parameters are neutral returns at once (its logits
// stay bit-identical).  Otherwise: zero a per-vocab count word in LDS, walk the history with LDS atomics (prompt
// tokens set the flag bit, generated ones count; ids outside this rank's vocab shard are skipped), then rewrite the
// logits whose word is nonzero, in fp32.  The counts are 32-bit words (V <= kSMaxV: 128 KiB of LDS), so they are
// exact for every history the int32 row stride can describe (< 2^31 tokens): nothing saturates or wraps into the
// flag bit.
__global__ void __launch_bounds__(kSThreads) sample_penalty_kernel(float* __restrict__ logits, SampleParams p) {
  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int slot = DSSE_IDX(p.row_slot ? p.row_slot[b] : b, p.pen_slots, 0);
  const int Bm = p.pen_slots;
  if (!penalties_on(p.pen_meta, Bm, slot)) return;
  __shared__ uint32_t cnt[kSMaxV];
  for (int i = threadIdx.x; i < p.V; i += kSThreads) cnt[i] = 0u;
  __syncthreads();
  const float pres = __int_as_float(p.pen_meta[slot]), freq = __int_as_float(p.pen_meta[Bm + slot]);
  const float rep = __int_as_float(p.pen_meta[2 * Bm + slot]);
  const int n_prompt = p.pen_meta[3 * Bm + slot];
  const int* h = p.hist + (size_t)slot * p.hist_ld;
  const int n = min(max(DSSE_IDX(h[0], p.hist_ld, 0), 0), p.hist_ld - 1);
  for (int j = threadIdx.x; j < n; j += kSThreads) {
    const int v = DSSE_IDX(h[1 + j], p.v_global, -1) - p.vocab_offset;
    if ((unsigned)v >= (unsigned)p.V) continue;  // another shard's token (or, checked build, a bad id)
    if (j < n_prompt) atomicOr(&cnt[v], kPenPrompt);
    else atomicAdd(&cnt[v], 1u);
  }
  __syncthreads();
  float* row = logits + (size_t)b * p.ld;
  for (int i = threadIdx.x; i < p.V; i += kSThreads) {
    const uint32_t w = cnt[i];
    if (w == 0u) continue;
    const uint32_t c = w & ~kPenPrompt;
    float x = row[i];
    if (rep != 1.f) x = x > 0.f ? x / rep : x * rep;
    x -= freq * (float)c;
    if (c > 0u) x -= pres;
    row[i] = x;
  }
}

// ---- logit_bias / min_tokens / stop_token_ids: the bias and ban pass ------------------------------------------
// One workgroup per logits row, after the raw logprob statistics and before the penalties (vLLM's order).  The
// slot's record (api.h: ctl_meta / ctl_body) is host-owned.  A row that is inactive, or whose slot has no bias entry
// and no ban in force, returns at once (its logits stay bit-identical).  Otherwise x[id] += bias for every entry
// (fp32; ids distinct), then, while the sampled token's position is below ban_until (generated tokens so far <
// min_tokens; derived here because steps are enqueued ahead of the host), x[id] = -inf for every banned id.  Ids
// outside this rank's vocab shard are skipped, so every TP rank runs the same launch.
constexpr int kCtlThreads = 256;

__global__ void __launch_bounds__(kCtlThreads) sample_bias_ban_kernel(float* __restrict__ logits, SampleParams p) {
  const int b = blockIdx.x;
  if (p.active && !p.active[b]) return;
  const int Bm = p.ctl_slots;
  const int slot = DSSE_IDX(p.row_slot ? p.row_slot[b] : b, Bm, -1);
  if ((unsigned)slot >= (unsigned)Bm) return;
  const int nb = min(max(DSSE_IDX(p.ctl_meta[slot], kCtlBias + 1, 0), 0), kCtlBias);
  int nban = min(max(DSSE_IDX(p.ctl_meta[Bm + slot], kCtlBan + 1, 0), 0), kCtlBan);
  if (p.positions[b] + 1 >= p.ctl_meta[2 * Bm + slot]) nban = 0;  // min_tokens reached (or never set)
  if (nb == 0 && nban == 0) return;
  const int* body = p.ctl_body + (size_t)slot * kCtlBody;
  float* row = logits + (size_t)b * p.ld;
  for (int j = threadIdx.x; j < nb; j += kCtlThreads) {
    const int v = DSSE_IDX(body[2 * j], p.v_global, -1) - p.vocab_offset;
    if ((unsigned)v >= (unsigned)p.V) continue;  // another shard's token (or, checked build, a bad id)
    row[v] += __int_as_float(body[2 * j + 1]);
  }
  if (nban == 0) return;  // (uniform over the workgroup)
  __syncthreads();        // a banned id may also carry a bias: the ban is written last
  for (int j = threadIdx.x; j < nban; j += kCtlThreads) {
    const int v = DSSE_IDX(body[2 * kCtlBias + j], p.v_global, -1) - p.vocab_offset;
    if ((unsigned)v >= (unsigned)p.V) continue;
    row[v] = -INFINITY;
  }
}

// ---- guided decoding: DFA token masking (api.h GuideParams) ------------------------------------------------------
// The walk of one token's bytes from `state`: the state reached, kGuideDead where a byte has no transition.  Length 0
// (or above kGuideTokBytes) = a token no guide allows.  Table entries are read through the vector L1 / L2: a used
// table is at most 256 KiB (a wide one 2 MiB) and the rows of the few states a step visits stay resident
// (profiles/r10/guided_decoding.md, profiles/guided_json.md).  `bound` = the states of the table's class.
DEV int guide_walk(const GuideParams& p, const unsigned short* __restrict__ tab, int bound, int state, int g) {
  const int len = p.tok_len[g];
  if (len < 1 || len > kGuideTokBytes) return kGuideDead;
  const uint4* src = reinterpret_cast<const uint4*>(p.tok_bytes + (size_t)g * kGuideTokBytes);
  const uint4 lo = src[0], hi = src[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int j = 0; j < kGuideTokBytes; ++j) {  // (unrolled: w[] stays in registers)
    if (j >= len) break;
    const int byte = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
    state = tab[(size_t)state * 256 + byte];
    if (state >= bound) return kGuideDead;  // dead (or, never written by the host, an entry out of range)
  }
  return state;
}

// The table of one entry word: the narrow pool below kGuidePool, the wide pool (schema guides) from there on.
struct GuideTable {
  const unsigned short* tab;
  int* flags;
  int bound;  // states of the class: a state at or above it is dead
};
DEV GuideTable guide_table(const GuideParams& p, int entry) {
  if (entry >= kGuidePool) {
    const size_t e = (size_t)(entry - kGuidePool);
    return {p.tab_wide + e * kGuideWideStates * 256, p.flags_wide + e * kGuideWideStates, kGuideWideStates};
  }
  return {p.tab + (size_t)entry * kGuideStates * 256, p.flags + (size_t)entry * kGuideStates, kGuideStates};
}

// The guide of row b: false = nothing to do (inactive row, guide off, dead state).  A JSON-mode slot comes back with
// entry = kGuideJson and its lexical state (json_load reads the rest), a wide-pool slot with its entry word
// (kGuidePool + the wide entry; off where no wide pool is given or the entry is outside it).
DEV bool guide_row(const GuideParams& p, int b, int* slot_out, int* entry_out, int* state_out) {
  if (p.active && !p.active[b]) return false;
  const int slot = DSSE_IDX(p.row_slot ? p.row_slot[b] : b, p.slots, -1);
  if ((unsigned)slot >= (unsigned)p.slots) return false;
  const int raw = p.meta[slot];
  if (raw == kGuideJson) {
    if (!p.json_state || !p.json_tab) return false;
    *slot_out = slot;
    *entry_out = kGuideJson;
    *state_out = p.json_state[slot];
    return true;
  }
  int entry = raw;
  if (raw >= kGuidePool) {
    if (!p.tab_wide || raw - kGuidePool >= p.pool_wide) return false;
  } else {
    entry = DSSE_IDX(raw, p.pool, -1);
    if ((unsigned)entry >= (unsigned)p.pool) return false;
  }
  *slot_out = slot;
  *entry_out = entry;
  *state_out = p.meta[p.slots + slot];
  return true;
}

// ---- JSON mode: the pushdown walk (api.h: json_tab / json_state) ---------------------------------------------------
struct JsonState {
  int q, depth;
  unsigned long long stack;  // one bit per open container, innermost at bit 0: 0 = object, 1 = array
};

// The slot's state; false = dead or out of range (a state no host write or advance produces).
DEV bool json_load(const GuideParams& p, int slot, JsonState* s) {
  const int* w = p.json_state + slot;
  s->q = w[0];
  s->depth = w[p.slots];
  s->stack = (unsigned long long)(unsigned)w[2 * (size_t)p.slots] |
             ((unsigned long long)(unsigned)w[3 * (size_t)p.slots] << 32);
  return (unsigned)s->q < (unsigned)p.json_states && (unsigned)s->depth <= (unsigned)kJsonDepth;
}

// One byte per step, as guide_walk: a dependent chain of 2-byte table reads (85 x 512 B, resident in the vector L1 /
// L2).  False = the walk died: no transition, a push at depth kJsonDepth, a token of length 0 or above kGuideTokBytes.
DEV bool json_walk(const GuideParams& p, JsonState& s, int g) {
  const int len = p.tok_len[g];
  if (len < 1 || len > kGuideTokBytes) return false;
  const uint4* src = reinterpret_cast<const uint4*>(p.tok_bytes + (size_t)g * kGuideTokBytes);
  const uint4 lo = src[0], hi = src[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  int q = s.q, depth = s.depth;
  unsigned long long stack = s.stack;
#pragma unroll
  for (int j = 0; j < kGuideTokBytes; ++j) {
    if (j >= len) break;
    const int byte = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
    const int e = p.json_tab[(size_t)q * 256 + byte];
    if (e == kGuideDead) return false;
    const int act = e >> 14;
    q = e & 0x3fff;
    if (act == 3) {  // pop: the next state is what the pop uncovers
      if (depth < 1) return false;
      --depth;
      stack >>= 1;
      q = depth == 0 ? kJsonDone : (stack & 1) ? kJsonAfterArr : kJsonAfterObj;
    } else if (act) {  // push: 1 = object, 2 = array
      if (depth >= kJsonDepth) return false;
      ++depth;
      stack = (stack << 1) | (unsigned long long)(act == 2);
    }
    if (q >= p.json_states) return false;  // (never written by the host: an entry out of range)
  }
  s.q = q;
  s.depth = depth;
  s.stack = stack;
  return true;
}

constexpr int kGuideThreads = 1024;

// Once per table upload, one workgroup per used state: bit 1 of its flag = no token of the global vocabulary other
// than EOS survives from it (the same on every TP rank: the table walked is the global one).  p.entry is an entry
// word: a wide entry runs up to kGuideWideStates workgroups.
__global__ void __launch_bounds__(kGuideThreads) guide_live_kernel(GuideParams p) {
  const int s = blockIdx.x;
  const GuideTable t = guide_table(p, p.entry);
  int any = 0;
  for (int g = threadIdx.x; g < p.v_global && !any; g += kGuideThreads)
    if (g != p.eos && guide_walk(p, t.tab, t.bound, s, g) != kGuideDead) any = 1;
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) {
    int* f = t.flags + s;
    *f = (*f & 1) | (any ? 0 : 2);
  }
}

// One workgroup per logits row, after the penalties and immediately before the candidate pass.  An inactive row, a
// slot with the guide off and a slot whose state is dead (steps enqueued past the stream's end) return at once, the
// row bit-identical.  Otherwise column v (global id g = v + vocab_offset) keeps its bits iff g is allowed: EOS iff the
// state is accepting or stuck, any other token iff its bytes walk from the state without meeting dead; the rest
// become -inf.  At a stuck state EOS is written 0.0f, which overrides a min_tokens ban: no row is ever all -inf.
//
// A JSON-mode row (entry kGuideJson) walks the pushdown automaton instead: a non-EOS token keeps its bits iff its bytes
// walk from the slot's (state, depth, stack) without dying.  EOS is 0.0f iff the row is stuck = no other token of the
// GLOBAL vocabulary survives (always so at kJsonDone), else -inf.  Survival can depend on the stack below its top
// ("}}" against "]}"), so there is no per-state flag: the rank that owns EOS, when none of its own columns survives,
// scans the rest of the vocabulary here.  Every other rank's columns are right without the answer.
DEV void json_mask_row(const GuideParams& p, int b, int slot) {
  JsonState s0;
  if (!json_load(p, slot, &s0)) return;  // dead: the row stays bit-identical
  float* row = p.logits + (size_t)b * p.ld;
  const int e = p.eos - p.vocab_offset;  // EOS's column here, if this rank owns it
  const bool own_eos = p.eos >= 0 && p.eos < p.v_global && (unsigned)e < (unsigned)p.V;
  int any = 0;
  for (int v = threadIdx.x; v < p.V; v += kGuideThreads) {
    const int g = v + p.vocab_offset;
    if (g >= p.v_global) { row[v] = -INFINITY; continue; }
    if (g == p.eos) continue;  // written below, once the row knows whether it is stuck
    JsonState s = s0;
    if (json_walk(p, s, g)) any = 1;
    else row[v] = -INFINITY;
  }
  if (!own_eos) return;  // (block-uniform)
  any = __syncthreads_or(any);
  if (!any && s0.q != kJsonDone) {  // (block-uniform) the other shards' tokens: [0, vocab_offset) and [offset + V, v_global)
    const int rest = p.vocab_offset + max(0, p.v_global - p.vocab_offset - p.V);
    for (int i = threadIdx.x; i < rest && !any; i += kGuideThreads) {
      const int g = i < p.vocab_offset ? i : i + p.V;
      if (g >= p.v_global || g == p.eos) continue;
      JsonState s = s0;
      if (json_walk(p, s, g)) any = 1;
    }
    any = __syncthreads_or(any);
  }
  if (threadIdx.x == 0) row[e] = any ? -INFINITY : 0.0f;
}

__global__ void __launch_bounds__(kGuideThreads) sample_guide_mask_kernel(GuideParams p) {
  const int b = blockIdx.x;
  int slot, entry, state;
  if (!guide_row(p, b, &slot, &entry, &state)) return;
  if (entry == kGuideJson) { json_mask_row(p, b, slot); return; }
  const GuideTable t = guide_table(p, entry);
  if ((unsigned)state >= (unsigned)t.bound) return;
  const int flags = t.flags[state];
  float* row = p.logits + (size_t)b * p.ld;
  for (int v = threadIdx.x; v < p.V; v += kGuideThreads) {
    const int g = v + p.vocab_offset;
    if (g >= p.v_global) { row[v] = -INFINITY; continue; }
    if (g == p.eos) {
      if (flags & 2) row[v] = 0.0f;
      else if (!(flags & 1)) row[v] = -INFINITY;
    } else if (guide_walk(p, t.tab, t.bound, state, g) == kGuideDead) {
      row[v] = -INFINITY;
    }
  }
}

// After each commit site: state = walk(state, bytes(committed id)).  EOS leaves the state unchanged; a dead walk, or
// a token of length 0, makes it dead.
__global__ void sample_guide_advance_kernel(int B, GuideParams p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int slot, entry, state;
  if (!guide_row(p, b, &slot, &entry, &state)) return;
  const int id = DSSE_IDX(p.ids[b], p.v_global, -1);
  if (id == p.eos) return;
  if (entry == kGuideJson) {  // JSON mode: (state, depth, stack) move together; a dead walk leaves only state = dead
    JsonState s;
    int* w = p.json_state + slot;
    if (json_load(p, slot, &s) && (unsigned)id < (unsigned)p.v_global && json_walk(p, s, id)) {
      w[0] = s.q;
      w[p.slots] = s.depth;
      w[2 * (size_t)p.slots] = (int)(unsigned)s.stack;
      w[3 * (size_t)p.slots] = (int)(unsigned)(s.stack >> 32);
    } else {
      w[0] = kGuideDead;
    }
    return;
  }
  int next = kGuideDead;
  const GuideTable t = guide_table(p, entry);
  if ((unsigned)state < (unsigned)t.bound && (unsigned)id < (unsigned)p.v_global)
    next = guide_walk(p, t.tab, t.bound, state, id);
  p.meta[p.slots + slot] = next;
}

// The sampled token joins its slot's history (slots with penalties only; a full row drops it: the engine sizes the
// rows for every token a sequence can sample, max_model_len + 1).
DEV void hist_append(const int* __restrict__ pen_meta, int Bm, int* __restrict__ hist, int hist_ld, int slot, int id) {
  if (!penalties_on(pen_meta, Bm, slot)) return;
  int* h = hist + (size_t)slot * hist_ld;
  const int n = DSSE_IDX(h[0], hist_ld - 1, -1);
  if ((unsigned)n >= (unsigned)(hist_ld - 1)) return;
  h[1 + n] = id;
  h[0] = n + 1;
}

// Eager first-token path: new_ids[i] joins the history of slot row_slot[i] (else i).
__global__ void sample_hist_append_kernel(const int* __restrict__ new_ids, int n, SampleParams p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (p.active && !p.active[i])) return;
  const int slot = DSSE_IDX(p.row_slot ? p.row_slot[i] : i, p.pen_slots, -1);
  if (slot < 0) return;
  hist_append(p.pen_meta, p.pen_slots, p.hist, p.hist_ld, slot, new_ids[i]);
}

// Merge candidates [world, B, nchunks] (vocab chunks x tensor-parallel shards) and commit the token:
// next_ids[b], ring[head][b], positions[b] += 1 (and, with p.hist, the history append of slot b).
constexpr int kPickThreads = 64;
__global__ void __launch_bounds__(kPickThreads)
sample_pick_kernel(const float2* __restrict__ cand, int world, int B, int nchunks, const int* __restrict__ active,
                   SampleParams p_rest) {
  // cand, the loop bounds and `active` lead (preloaded); the block size is a constant (blockDim is a hidden argument)
  SampleParams p = p_rest;
  p.nchunks = nchunks;
  p.active = active;
  const int b = blockIdx.x * kPickThreads + threadIdx.x;
  if (b >= B) return;
  if (p.active && !p.active[b]) return;
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  for (int w = 0; w < world; ++w)
    for (int c = 0; c < p.nchunks; ++c) {
      const float2 v = cand[((size_t)w * B + b) * p.nchunks + c];
      better(best, bidx, v.x, __float_as_int(v.y));
    }
  bidx = DSSE_IDX(bidx, p.v_global, 0);  // no candidate (all logits NaN / -inf) is a bug upstream
  p.next_ids[b] = bidx;
  if (p.ring) p.ring[(size_t)(p.ring_counter[0] % p.ring_size) * p.ring_stride + b] = bidx;
  if (p.positions_inc) p.positions_inc[b] += 1;
  if (p.hist && b < p.pen_slots) hist_append(p.pen_meta, p.pen_slots, p.hist, p.hist_ld, b, bidx);
}

// First-token sampling of the prompts a captured prefill / mixed graph finishes (round 6: inside the graph, no torch
// index kernels).  meta = [rows[NS] | slots[NS] | last_pos[NS] | n | ring_row] (uploaded with the graph's other
// metadata); slot_meta = the runner's per-slot sampling state [active | temperature | top_k | top_p | seeds x 2]
// (Bm each).  Gather: row i < n of xl = x[rows[i]] (zeros for i >= n) and the sampling parameters of slots[i] into
// smeta = [active | temperature | top_k | top_p | seeds x 2 | position] (NS each; active = i < n).
__global__ void __launch_bounds__(256)
prefill_sample_gather_kernel(const bf16* __restrict__ x, int T, int H, const int* __restrict__ meta, int NS,
                             const int* __restrict__ slot_meta, int Bm, bf16* __restrict__ xl, int* __restrict__ smeta) {
  const int i = blockIdx.x;
  const int n = meta[3 * NS];
  const bool on = i < n;
  const int row = on ? DSSE_IDX(meta[i], T, 0) : 0;
  const int H8 = H / 8;
  for (int c = threadIdx.x; c < H8; c += blockDim.x) {
    const bf16x8 v = on ? *reinterpret_cast<const bf16x8*>(x + (size_t)row * H + 8 * c) : zero_bf16x8();
    *reinterpret_cast<bf16x8*>(xl + (size_t)i * H + 8 * c) = v;
  }
  if (threadIdx.x == 0) {
    const int slot = on ? DSSE_IDX(meta[NS + i], Bm, 0) : 0;
    smeta[i] = on ? 1 : 0;
    smeta[NS + i] = slot_meta[Bm + slot];          // temperature (bits)
    smeta[2 * NS + i] = slot_meta[2 * Bm + slot];  // top_k
    smeta[3 * NS + i] = slot_meta[3 * Bm + slot];  // top_p (bits)
    smeta[4 * NS + 2 * i] = slot_meta[4 * Bm + 2 * slot];
    smeta[4 * NS + 2 * i + 1] = slot_meta[4 * Bm + 2 * slot + 1];
    smeta[6 * NS + i] = on ? meta[2 * NS + i] : 0;  // the sampled token's predecessor position (RNG counter)
  }
}

// Commit the picked first tokens: ids[slot], ring[ring_row][slot], positions[slot] = last_pos + 1 (and, with hist,
// the history append of the slots that have penalties; pen_meta / hist are [.., Bm] like ids).
__global__ void prefill_sample_commit_kernel(const int* __restrict__ meta, int NS, const int* __restrict__ new_ids,
                                             int* __restrict__ ids, int Bm, int* __restrict__ ring, int R,
                                             int* __restrict__ positions, const int* __restrict__ pen_meta,
                                             int* __restrict__ hist, int hist_ld) {
  const int i = threadIdx.x;
  if (i >= NS || i >= meta[3 * NS]) return;
  const int slot = DSSE_IDX(meta[NS + i], Bm, -1);
  if (slot < 0) return;
  const int row = DSSE_IDX(meta[3 * NS + 1], R, 0);
  ids[slot] = new_ids[i];
  ring[(size_t)row * Bm + slot] = new_ids[i];
  positions[slot] = meta[2 * NS + i] + 1;
  if (hist) hist_append(pen_meta, Bm, hist, hist_ld, slot, new_ids[i]);
}

// ---- logprobs / top_logprobs ---------------------------------------------------------------------------------
// Raw logprobs (vLLM's default): lp[v] = x[v] - logsumexp(x) over the full vocabulary of the fp32 logits as the LM
// head wrote them.  Per-slot state lp_meta[slot] (host-owned, uploaded with the slot metadata): -1 = off, 0..kLpTop
// = N.  top-N order: logit descending, equal logits by ascending global id -- `better` on the stored fp32 values,
// so the ids are the same under every vocab sharding.
DEV int lp_rows_n(const LogprobParams& p, int b, int* slot_out) {
  if (p.active && !p.active[b]) return -1;
  const int slot = DSSE_IDX(p.row_slot ? p.row_slot[b] : b, p.slots, -1);
  if (slot < 0) return -1;
  *slot_out = slot;
  return min(p.lp_meta[slot], kLpTop);
}

DEV int block_min_int(int v, int* sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int tot = 0x7fffffff;
  for (int i = 0; i < kSThreads / 64; ++i) tot = min(tot, sh[i]);
  __syncthreads();
  return tot;
}

// One workgroup per logits row of this rank's shard; a row that is inactive or off returns at once.  The row is
// staged once in LDS (and copied to p.raw when given: the penalty pass that follows rewrites logits in place), then:
// m = max, s = sum exp(x - m), and the shard's top-N: the radix select gives the N-th key, everything above it is
// taken, and the entries equal to it are admitted lowest id first (a tie across the N boundary resolves the same
// way on every rank layout); the <= kLpTop survivors are ordered by counting.  Record: [m | s | kLpTop x (logit,
// global id bits)], unused entries (-inf, 0x7fffffff).
__global__ void __launch_bounds__(kSThreads) logprob_stats_kernel(LogprobParams p) {
  const int b = blockIdx.x;
  int slot = 0;
  const int N = lp_rows_n(p, b, &slot);
  if (N < 0) return;
  __shared__ float xs[kSMaxV];
  __shared__ float hist[256];
  __shared__ float sh[kSThreads / 64];
  __shared__ int shi[kSThreads / 64];
  __shared__ float tl[kLpTop];
  __shared__ int ti[kLpTop];
  __shared__ int s_n;
  const float* row = p.logits + (size_t)b * p.ld;
  float* raw = p.raw ? p.raw + (size_t)b * p.V : nullptr;
  float lmax = -INFINITY;
  for (int i = threadIdx.x; i < p.V; i += kSThreads) {
    const float x = row[i];
    if (raw) raw[i] = x;
    xs[i] = x + 0.f;  // -0 -> +0: the radix keys then order exactly as the float compare of the merge does
    lmax = fmaxf(lmax, x);
  }
  if (threadIdx.x == 0) s_n = 0;
  const float m = block_max(lmax, sh);  // (barriers: xs and s_n are visible)
  float z = 0.f;
  if (m > -INFINITY)
    for (int i = threadIdx.x; i < p.V; i += kSThreads) z += expf(xs[i] - m);
  z = block_sum(z, sh);
  float* rec = p.rec + (size_t)b * kLpRec;
  const int n_take = min(N, p.V);
  int cnt = 0;
  if (n_take > 0) {
    const uint32_t thr = radix_select<false>(xs, p.V, m, 0u, (float)n_take, hist);
    for (int i = threadIdx.x; i < p.V; i += kSThreads)
      if (fkey(xs[i]) > thr) {
        const int j = atomicAdd(&s_n, 1);  // fewer than n_take by the select's definition
        if (j < kLpTop) { tl[j] = xs[i]; ti[j] = i + p.vocab_offset; }
      }
    __syncthreads();
    cnt = min(s_n, n_take);
    int last = -1;
    while (cnt < n_take) {  // the ties at the threshold, lowest id first (usually one entry, one round)
      int mn = 0x7fffffff;
      for (int i = threadIdx.x; i < p.V; i += kSThreads)
        if (i > last && fkey(xs[i]) == thr) { mn = i; break; }
      mn = block_min_int(mn, shi);
      if (mn == 0x7fffffff) break;
      if (threadIdx.x == 0) { tl[cnt] = xs[mn]; ti[cnt] = mn + p.vocab_offset; }
      last = mn;
      ++cnt;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { rec[0] = m; rec[1] = z; }
  if (threadIdx.x < kLpTop) {
    const int t = threadIdx.x;
    if (t < cnt) {
      const float l = tl[t];
      const int id = ti[t];
      int rank = 0;
      for (int j = 0; j < cnt; ++j) rank += (tl[j] > l || (tl[j] == l && ti[j] < id)) ? 1 : 0;
      rec[2 + 2 * rank] = l;
      rec[3 + 2 * rank] = __int_as_float(id);
    } else {
      rec[2 + 2 * t] = -INFINITY;
      rec[3 + 2 * t] = __int_as_float(0x7fffffff);
    }
  }
}

// chosen[b] = this shard's raw logit of the sampled token next_ids[b], -inf when another shard owns it (TP: one 4 B
// all-gather per row, then the finish pass takes the max).  `logits` is p.raw's copy where the penalty pass ran.
__global__ void logprob_chosen_kernel(int B, LogprobParams p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int slot = 0;
  if (lp_rows_n(p, b, &slot) < 0) return;
  const int v = DSSE_IDX(p.next_ids[b], p.v_global, -1) - p.vocab_offset;
  p.chosen[b] = (unsigned)v < (unsigned)p.V ? p.logits[(size_t)b * p.ld + v] : -INFINITY;
}

// One 64-thread workgroup per row: merge the `world` records -- M = max m_w, lse = M + log sum s_w exp(m_w - M)
// (an empty or all -inf shard has s_w = 0 and m_w = -inf: it adds nothing and is skipped, so no inf - inf), the
// world x kLpTop candidates ranked by counting in the same order -- subtract lse and write [logprob of the sampled
// token | kLpTop ids | kLpTop logprobs] to lp_ring[ring row][slot], where the token itself went; entries past
// min(N, vocab) are (-1, -inf).
__global__ void __launch_bounds__(64) logprob_finish_kernel(int B, LogprobParams p) {
  const int b = blockIdx.x;
  int slot = 0;
  const int N = lp_rows_n(p, b, &slot);
  if (N < 0) return;
  constexpr int kMaxWorld = 8;
  __shared__ float cl[kMaxWorld * kLpTop];
  __shared__ int ci[kMaxWorld * kLpTop];
  const int nc = p.world * kLpTop;
  float M = -INFINITY, chosen = -INFINITY;
  for (int w = 0; w < p.world; ++w) {
    M = fmaxf(M, p.rec[((size_t)w * B + b) * kLpRec]);
    chosen = fmaxf(chosen, p.chosen[(size_t)w * B + b]);
  }
  float s = 0.f;
  for (int w = 0; w < p.world; ++w) {
    const float* r = p.rec + ((size_t)w * B + b) * kLpRec;
    if (r[0] > -INFINITY && r[1] > 0.f) s += r[1] * expf(r[0] - M);
  }
  const float lse = s > 0.f ? M + logf(s) : -INFINITY;
  for (int c = threadIdx.x; c < nc; c += 64) {
    const float* r = p.rec + ((size_t)(c / kLpTop) * B + b) * kLpRec + 2 + 2 * (c % kLpTop);
    cl[c] = r[0];
    ci[c] = __float_as_int(r[1]);
  }
  __syncthreads();
  int row = p.ring_counter ? p.ring_counter[0] % p.ring_size : (p.ring_row_dev ? p.ring_row_dev[0] : p.ring_row);
  row = DSSE_IDX(row, p.ring_size, 0);
  float* out = p.lp_ring + ((size_t)row * p.slots + slot) * kLpOut;
  if (threadIdx.x == 0) out[0] = chosen > -INFINITY ? chosen - lse : -INFINITY;
  for (int c = threadIdx.x; c < nc; c += 64) {
    const float l = cl[c];
    const int id = ci[c];
    int rank = 0;
    for (int j = 0; j < nc; ++j)
      rank += (cl[j] > l || (cl[j] == l && (ci[j] < id || (ci[j] == id && j < c)))) ? 1 : 0;
    if (rank >= kLpTop) continue;
    const bool used = rank < N && id != 0x7fffffff;
    out[1 + rank] = __int_as_float(used ? DSSE_IDX(id, p.v_global, 0) : -1);
    out[1 + kLpTop + rank] = used && l > -INFINITY ? l - lse : -INFINITY;
  }
}

}  // namespace dsse

extern "C" hipError_t dsse_logprob_stats(int B, const dsse::LogprobParams* p, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (p->V > dsse::kSMaxV || p->V < 1 || p->ld < p->V || !p->logits || !p->lp_meta || !p->rec || p->slots < 1 ||
      (!p->row_slot && B > p->slots))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::logprob_stats_kernel, dim3(B), dim3(dsse::kSThreads), 0, st, *p);
  return hipGetLastError();
}

extern "C" hipError_t dsse_logprob_chosen(int B, const dsse::LogprobParams* p, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (p->V < 1 || p->ld < p->V || !p->logits || !p->lp_meta || !p->next_ids || !p->chosen || p->slots < 1 ||
      (!p->row_slot && B > p->slots))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::logprob_chosen_kernel, dim3((B + 63) / 64), dim3(64), 0, st, B, *p);
  return hipGetLastError();
}

extern "C" hipError_t dsse_logprob_finish(int B, const dsse::LogprobParams* p, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (p->world < 1 || p->world > 8 || !p->lp_meta || !p->rec || !p->chosen || !p->lp_ring || p->slots < 1 ||
      p->ring_size < 1 || (!p->row_slot && B > p->slots) ||
      (!p->ring_counter && !p->ring_row_dev && (p->ring_row < 0 || p->ring_row >= p->ring_size)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::logprob_finish_kernel, dim3(B), dim3(64), 0, st, B, *p);
  return hipGetLastError();
}

extern "C" hipError_t dsse_prefill_sample_gather(const void* x, int T, int H, const int* meta, int NS,
                                                 const int* slot_meta, int Bm, void* xl, int* smeta, hipStream_t st) {
  if (NS <= 0 || H % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::prefill_sample_gather_kernel, dim3(NS), dim3(256), 0, st,
                     reinterpret_cast<const bf16*>(x), T, H, meta, NS, slot_meta, Bm, reinterpret_cast<bf16*>(xl),
                     smeta);
  return hipGetLastError();
}

extern "C" hipError_t dsse_prefill_sample_commit(const int* meta, int NS, const int* new_ids, int* ids, int Bm,
                                                 int* ring, int R, int* positions, const int* pen_meta, int* hist,
                                                 int hist_ld, hipStream_t st) {
  if (NS <= 0 || NS > 64 || (hist && (!pen_meta || hist_ld < 2))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::prefill_sample_commit_kernel, dim3(1), dim3(64), 0, st, meta, NS, new_ids, ids, Bm, ring,
                     R, positions, pen_meta, hist, hist_ld);
  return hipGetLastError();
}

// Penalty pass over logits [B, p->ld] in place (p: active, V, ld, vocab_offset, v_global, pen_meta, hist, hist_ld,
// pen_slots, row_slot).
extern "C" hipError_t dsse_sample_penalties(int B, float* logits, const dsse::SampleParams* p, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (p->V > dsse::kSMaxV || p->V < 1 || p->ld < p->V || !p->pen_meta || !p->hist || p->hist_ld < 2 ||
      p->pen_slots < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::sample_penalty_kernel, dim3(B), dim3(dsse::kSThreads), 0, st, logits, *p);
  return hipGetLastError();
}

// Bias and ban pass over logits [B, p->ld] in place (p: active, positions, V, ld, vocab_offset, v_global, ctl_meta,
// ctl_body, ctl_slots, row_slot).
extern "C" hipError_t dsse_sample_bias_ban(int B, float* logits, const dsse::SampleParams* p, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (p->V < 1 || p->ld < p->V || !logits || !p->ctl_meta || !p->ctl_body || !p->positions || p->ctl_slots < 1 ||
      (!p->row_slot && B > p->ctl_slots))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::sample_bias_ban_kernel, dim3(B), dim3(dsse::kCtlThreads), 0, st, logits, *p);
  return hipGetLastError();
}

static bool guide_ok(const dsse::GuideParams* p) {
  return p->tok_bytes && p->tok_len && p->tab && p->flags && p->meta && p->slots >= 1 && p->pool >= 1 &&
         p->pool <= dsse::kGuidePool && p->v_global >= 1 && !p->json_tab == !p->json_state &&
         (!p->json_tab || (p->json_states > dsse::kJsonAfterArr && p->json_states <= dsse::kJsonStates)) &&
         !p->tab_wide == !p->flags_wide && (p->tab_wide ? p->pool_wide >= 1 && p->pool_wide <= dsse::kGuideWidePool
                                                        : p->pool_wide == 0);
}

// The stuck bits of the states [0, p->n_states) of the entry word p->entry (narrow: [0, pool); wide: kGuidePool +
// [0, pool_wide)).
extern "C" hipError_t dsse_guide_live(const dsse::GuideParams* p, hipStream_t st) {
  if (!guide_ok(p) || p->n_states < 1) return hipErrorInvalidValue;
  const bool wide = p->entry >= dsse::kGuidePool;
  if (wide ? p->entry - dsse::kGuidePool >= p->pool_wide || p->n_states > dsse::kGuideWideStates
           : p->entry < 0 || p->entry >= p->pool || p->n_states > dsse::kGuideStates)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::guide_live_kernel, dim3(p->n_states), dim3(dsse::kGuideThreads), 0, st, *p);
  return hipGetLastError();
}

// Guide mask over logits [B, p->ld] in place.
extern "C" hipError_t dsse_sample_guide_mask(int B, const dsse::GuideParams* p, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (!guide_ok(p) || !p->logits || p->V < 1 || p->ld < p->V || p->vocab_offset < 0 || (!p->row_slot && B > p->slots))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::sample_guide_mask_kernel, dim3(B), dim3(dsse::kGuideThreads), 0, st, *p);
  return hipGetLastError();
}

// Guide states of the slots of rows [0, B) advanced by p->ids.
extern "C" hipError_t dsse_sample_guide_advance(int B, const dsse::GuideParams* p, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (!guide_ok(p) || !p->ids || (!p->row_slot && B > p->slots)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::sample_guide_advance_kernel, dim3((B + 63) / 64), dim3(64), 0, st, B, *p);
  return hipGetLastError();
}

extern "C" hipError_t dsse_sample_hist_append(int n, const int* new_ids, const dsse::SampleParams* p,
                                              hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!p->pen_meta || !p->hist || p->hist_ld < 2 || p->pen_slots < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::sample_hist_append_kernel, dim3((n + 63) / 64), dim3(64), 0, st, new_ids, n, *p);
  return hipGetLastError();
}

// Per-rank candidate pass: fills p->cand[B, nchunks].
extern "C" hipError_t dsse_sample(int B, const dsse::SampleParams* p, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (p->V > dsse::kSMaxV || p->nchunks < 1 || (p->min_p && p->ctl_slots < 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dsse::sample_chunk_kernel, dim3(p->nchunks, B), dim3(dsse::kCThreads), 0, st,
                     DSSE_SAMPLE_ARGS(*p));
  hipLaunchKernelGGL(dsse::sample_filtered_kernel, dim3(B), dim3(dsse::kSThreads), 0, st, DSSE_SAMPLE_ARGS(*p));
  return hipGetLastError();
}

// Merge pass over cand [world, B, nchunks].
extern "C" hipError_t dsse_sample_pick(int B, int world, const void* cand, const dsse::SampleParams* p,
                                       hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(dsse::sample_pick_kernel, dim3((B + dsse::kPickThreads - 1) / dsse::kPickThreads),
                     dim3(dsse::kPickThreads), 0, st, reinterpret_cast<const float2*>(cand), world, B, p->nchunks,
                     p->active, *p);
  return hipGetLastError();
}

DSSE_CHECK_READER(dsse_check_sampler)
