// Host-visible kernel API of the engine: parameter structs and the extern "C" launchers that the
// torch bindings (bindings.cpp) call with raw pointers and torch's current HIP stream.
#pragma once
#include "common.h"

namespace dsse {

constexpr int kBS = 32;  // KV-cache page size in tokens (fixed for every kernel)

enum GemmMode { kStoreBf16 = 0, kStoreF32 = 1, kResidAdd = 2, kSiluMul = 3, kQkvRope = 4 };

// Decode-GEMM weight layout ("tiled"): W[N, K] is stored as blocks of (16-row tile T, 128-column
// K-chunk c), block-major (T, c), each block [s = 0..3][lane = 0..63][j = 0..7] where lane l = r + 16g
// holds W[16T + r][128c + 32g + 8s + j] — exactly the MFMA B-operand fragment of k-step s.  A wave
// therefore loads every block as four fully contiguous 1 KiB runs (see ops/reference.py tile_weight).
constexpr int kTileChunk = 16 * 128;  // elements per (tile, chunk) block

// FP8 weights (gemm_w8.hip; ops/reference.py quantize_weight_f8 / tile_weight_f8): Wq[N, K] holds one e4m3fn byte per
// element, value = bf16(byte) * scale[row] with one fp32 power-of-two scale per row.  Byte form of the tiled layout:
// the same (16-row tile T, 128-column K-chunk c) blocks, block-major (T, c), 2 KiB each; inside a block
// [h = 0..1][lane = 0..63][b = 0..15] where lane l = r + 16g holds Wq[16T + r][128c + 32g + 16h + b] -- 16 contiguous
// bytes per lane: bytes 0-7 widen to the MFMA B-operand fragment of k-step 2h, bytes 8-15 to that of k-step 2h + 1
// (the same k = 32g + 8s + j as the bf16 layout).  A wave loads every block as two fully contiguous 1 KiB runs.
constexpr int kTileChunkF8 = 16 * 128;  // bytes per (tile, chunk) block

// MXFP4 weights (gemm_w4.hip; ops/reference.py quantize_weight_mxfp4 / tile_weight_mxfp4): OCP e2m1 elements with one
// e8m0 scale byte per 32 consecutive K, value = e2m1(nibble) * 2^(scale byte - 127), exact in bf16.  Nibble code: bit 3
// sign, bits 2-1 exponent, bit 0 mantissa ({0, 0.5, 1, 1.5, 2, 3, 4, 6}; a zero is always code 0); a byte holds element
// k (even) in its low nibble and element k + 1 in its high nibble.  Device layout, two tensors over the same
// (16-row tile T, 128-column K-chunk c) blocks, block-major (T, c):
//   Wq [N, K / 2] bytes, 1 KiB per block: [lane = 0..63][b = 0..15] where lane l = r + 16g holds the 16 contiguous
//     bytes of W[16T + r][128c + 32g .. 32g + 31] -- one MX block; dword t of them widens to the MFMA B-operand
//     fragment of k-step t (k = 32g + 8t + j).  A wave loads every block as one contiguous 1 KiB run.
//   E  [N, K / 32] bytes, 64 B per block: byte [lane] is the scale of that lane's MX block, W's row 16T + r, columns
//     128c + 32g .. 32g + 31.  A wave's scales over its K range are one contiguous run.
constexpr int kTileChunkF4 = 16 * 128 / 2;  // nibble bytes per (tile, chunk) block
constexpr int kTileScaleF4 = 16 * 128 / 32;  // scale bytes per (tile, chunk) block

struct GemmEpi {
  void* out;          // bf16 / f32 output (modes 0, 1, 3)
  int ldo;
  float* resid;       // mode 2
  int ldr;
  const int* positions;   // mode 4: per-row absolute position
  const int* slots;       // mode 4: per-row KV slot (-1 = do not write)
  const float2* rope;     // mode 4: [max_pos][64] (cos, sin)
  bf16* q_out;            // mode 4: [M, nh*128]
  bf16* k_cache;          // [blocks, nkv, kBS, 128]
  bf16* v_cache;          // [blocks, nkv, 128, kBS] (token-permuted inside a page)
  int nh, nkv;
  int num_slots;          // mode 4: KV slots in the cache (pages * kBS); checked build only
  int rope_len;           // mode 4: rows of the rope table; checked build only
  // split-K fix-up inside the launch (gemm_pipe.hip, partial_only = 2): [4 + 2 * kFixTiles] ints -- word 0 counts
  // timed-out waits, then the per-tile ticket and done counters (zero between launches: each tile's last arriver
  // resets its pair); null when unused
  int* fix_cnt;
};
constexpr int kFixTiles = 8192;  // tiles of one fix-up launch at most
// the per-device counter block (bindings.cpp fix_state): [4 words][2 kFixTiles GEMM fix-up counters]
// [kFixTiles decode-attention combine tickets][stamps build: per-workgroup stamps]
constexpr int kAttnCntOff = 4 + 2 * kFixTiles;
constexpr int kStampOff = 4 + 3 * kFixTiles;


struct AttnParams {
  const bf16* q;            // [T, Hq, 128]
  const bf16* k_cache;
  const bf16* v_cache;
  const int* block_tables;  // [B, max_blocks]
  int max_blocks;
  int num_blocks;           // pages in the KV cache (checked build: block-table entries must be below)
  const int* q_start;       // [B] first query row of the sequence in q / out
  const int* q_len;         // [B] number of query tokens (0 = inactive)
  const int* ctx_len;       // [B] number of keys in the cache including the queries
  const int* work_seq;      // [num_work] sequence of work item
  const int* work_tile;     // [num_work] query-tile block (in units of QW tiles)
  bf16* out;                // [T, Hq, 128]
  float* part_o;            // [num_work, Hkv, nparts, QW, 16, 128]
  float2* part_ml;          // [num_work, Hkv, nparts, QW, 16]
  int hq, hkv, group;       // group = hq / hkv; 16 % group == 0
  int part;                 // keys per partition (multiple of 32 * KWV); 0 = each item's keys split evenly over nparts
  int nparts;               // grid.z
  float scale_log2;         // log2(e) / sqrt(128)
  int kwv;                  // decode: waves per workgroup splitting the keys (0 = by grid size)
  int pd;                   // mode 3: KV pages in flight per wave (0 = by occupancy, 1 = no look-ahead)
  // mode 3 (decode with the QKV epilogue folded in): q comes from the QKV GEMM's fp32 split-K slabs instead
  // of `q`; the workgroup holding a sequence's newest key also writes that token's K / V into the cache.
  const float* qkv_part;    // [qkv_S, qkv_M, (hq + 2 hkv) * 128], columns in the engine's rotary-pair order
  int qkv_S, qkv_M;
  const int* positions;     // [qkv_M] absolute position of row m (RoPE)
  const int* slots;         // [qkv_M] KV slot of row m (-1 = do not write)
  const float2* rope;       // [rope_len, 64] (cos, sin)
  int rope_len, num_slots;
  bf16* k_out;              // = k_cache, writable
  bf16* v_out;              // = v_cache, writable
  // flash prefill key split (mode 2, round 6; nullptr = every item walks all its key blocks and writes `out`):
  // item i walks key blocks [work_kb[2i], work_kb[2i + 1]) and, when work_slot[i] >= 0, leaves its unnormalised O
  // and (max, sum) in partial slot work_slot[i] ([slot][Hkv][G][64 queries] of part_o / part_ml) for the combine:
  // comb[4c ..] = (sequence, 64-query tile, first slot, slots) of split tile c, ncomb of them
  const int* work_kb;
  const int* work_slot;
  const int* comb;
  int ncomb;
  // decode partitions (nparts > 1, one query tile per workgroup) combined by the last partition of each (item, kv
  // head) to finish instead of attn_combine_kernel (round 6): [num_work * hkv] arrival tickets, zero between
  // launches (the last arriver resets its ticket); null = the combine kernel
  int* comb_cnt;
  // FP8 (e4m3) KV cache: k_cache / v_cache (k_out / v_out) point at bytes, same shapes and element order.  Stored
  // value = x / scale.  The host folds k_scale into scale_log2; v_scale multiplies the final 1 / l normalisation;
  // k_inv = 1 / k_scale and v_inv = 1 / v_scale quantise the folded write (mode 3).  All four are read by the f8
  // instantiations only.  The flash prefill kernels (attention_prefill.hip) have no f8 form and refuse kv_f8.
  int kv_f8;
  float v_scale, k_inv, v_inv;
};

struct SampleParams {
  const float* logits;  // [B, ld]
  int ld, V;            // row stride, local vocab size
  int vocab_offset;     // global index of local column 0
  const float* temperature;  // [B]; <= 0 -> greedy
  const int* top_k;          // [B]; <= 0 -> off
  const float* top_p;        // [B]; >= 1 -> off
  const uint2* seeds;        // [B]
  const int* positions;      // [B] position of the sampled token's predecessor (RNG counter)
  const int* active;         // [B] or null (all active)
  int* next_ids;             // [B] (pick pass)
  int* ring;                 // [ring_size, ring_stride] or null
  const int* ring_counter;
  int ring_size, ring_stride;
  int* positions_inc;        // [B] or null: positions[b] += 1 for active rows
  float2* cand;              // [B, nchunks] (score, index-as-bits) candidates
  int nchunks;               // vocab chunks per row (unfiltered path)
  int v_global;              // full vocabulary (all TP shards); checked build: sampled ids below it
  // presence / frequency / repetition penalties (sample_penalty_kernel, the history append of the pick / commit
  // passes); null = off, what every launcher without penalties passes
  const int* pen_meta;       // [4, pen_slots]: presence | frequency | repetition (float bits) | n_prompt, per slot
  int* hist;                 // [pen_slots, hist_ld]: word 0 = tokens held, then the prompt and the generated tokens
  int hist_ld, pen_slots;
  const int* row_slot;       // [B] slot of logits row b, or null (row b = slot b)
  // logit_bias / min_tokens / stop_token_ids (sample_bias_ban_kernel) and min_p (sample_filtered_kernel); null =
  // off, what every launcher without them passes.  All slot-indexed (row b -> slot row_slot[b], else b).
  const int* ctl_meta;       // [4, ctl_slots]: bias entries | banned ids | ban-until position | min_p (float bits)
  const int* ctl_body;       // [ctl_slots, kCtlBody]: kCtlBias x (global id, bias float bits), then kCtlBan banned ids
  int ctl_slots;
  const float* min_p;        // [ctl_slots] (= ctl_meta's fourth column) or null; <= 0 -> off
};

// Per-slot record of the bias and ban pass, host-owned.  ctl_meta (uploaded with the slot metadata, neutral = all
// zero): word [slot] = n_bias in 0..kCtlBias, [ctl_slots + slot] = n_ban in 0..kCtlBan, [2 ctl_slots + slot] =
// ban_until = prompt length as submitted + min_tokens (the ban is in force while the sampled token's position,
// positions[b] + 1, is below it), [3 ctl_slots + slot] = min_p.  ctl_body[slot] (uploaded when a sequence that uses
// it takes the slot): words [2j, 2j + 1] = (global token id, bias as float bits) for j < n_bias, ids distinct; words
// [2 kCtlBias + j] = banned global id j < n_ban (EOS unless ignore_eos, then the stop_token_ids).
constexpr int kCtlBias = 300;
constexpr int kCtlBan = 17;
constexpr int kCtlBody = 2 * kCtlBias + kCtlBan + 3;  // 620 words (row start 16 B aligned)

// Log-probabilities of the sampled token and the top-N (sampler.hip logprob_*_kernel): raw logprobs, x - logsumexp(x)
// over the full vocabulary of the fp32 logits as the LM head wrote them (before penalties / temperature / filters).
constexpr int kLpTop = 20;               // top_logprobs at most
constexpr int kLpRec = 2 + 2 * kLpTop;   // per-(rank, row) record: [max | sum exp(x - max) | kLpTop x (logit, id bits)]
constexpr int kLpOut = 1 + 2 * kLpTop;   // per-token result: [logprob of the sampled token | kLpTop ids | kLpTop logprobs]
struct LogprobParams {
  const float* logits;    // [B, ld] this rank's shard (stats / chosen passes)
  int ld, V, vocab_offset, v_global;
  const int* active;      // [B] or null
  const int* lp_meta;     // [slots]: -1 = off, 0..kLpTop = N
  int slots;
  const int* row_slot;    // [B] slot of row b, or null (row b = slot b)
  float* rec;             // stats: [B, kLpRec] out;  finish: [world, B, kLpRec] in
  float* raw;             // stats: [B, V] copy of the rows with logprobs on (the penalty pass rewrites logits), or null
  const int* next_ids;    // chosen: [B] sampled (global) ids
  float* chosen;          // chosen: [B] out;  finish: [world, B] in
  int world;
  float* lp_ring;         // finish: [ring_size, slots, kLpOut]
  int ring_size;
  const int* ring_counter;  // ring row = ring_counter[0] % ring_size, else ring_row_dev[0], else ring_row
  const int* ring_row_dev;
  int ring_row;
};

// Guided decoding (sampler.hip guide_live_kernel / sample_guide_mask_kernel / sample_guide_advance_kernel): a byte-level
// DFA per pattern, walked on the device so that no step waits for the host to look at a token.
//   tok_bytes [v_global, kGuideTokBytes] / tok_len [v_global] (uint8): the UTF-8 bytes of every piece of the global
//     vocabulary, whole on every TP rank, built once from the tokenizer.  Length 0 = never allowed under a guide
//     (<unk>, <s>, </s>, empty pieces, pieces longer than kGuideTokBytes).
//   guide_tab [kGuidePool, kGuideStates, 256] (uint16): the transition tables of the resident patterns, start state 0,
//     kGuideDead = dead; every entry is a state below kGuideStates or kGuideDead (the kernels treat anything else as
//     dead).  guide_flags [kGuidePool, kGuideStates] (int32): bit 0 = accepting (host, with the table), bit 1 = stuck
//     = no token of the global vocabulary other than EOS survives from the state (guide_live_kernel, once per upload).
//   guide_meta [2, slots] (int32): word [slot] = pool index of the slot's pattern, -1 = guide off (the neutral value);
//     word [slots + slot] = the current DFA state, kGuideDead = dead.  The host writes both words when a sequence takes
//     the slot (state = the walk over the tokens already published), stream-ordered; from then on only the advance
//     kernel writes the state.  Pool entries are host-owned and reference-counted by live sequences.
//
// JSON mode (response_format json_object; the language J: docs/kernels.md, "Sampler") is a pushdown walk inside the
// same two launches.  A slot whose guide_meta entry word is kGuideJson uses no pool entry; its state lives in
//   json_state [4, slots] (int32): [lexical state q | depth 0..kJsonDepth | stack bits 0..31 | stack bits 32..63],
//     q = kGuideDead = dead.  The stack holds one bit per open container (0 = object, 1 = array), innermost at bit 0.
//   json_tab [n <= kJsonStates, 256] (uint16): entry = next state | action << 14, kGuideDead = no transition.  Action
//     1 / 2 pushes an object / array bit (dead at depth kJsonDepth); action 3 pops, and the next state then comes from
//     what the pop uncovers: kJsonDone at depth 0, else kJsonAfterObj / kJsonAfterArr by the new innermost bit.  The
//     lexical states are split by context (in an object / in an array), so a closing byte always matches the top bit.
//
// Schema guides (guided_json / response_format json_schema) need more states than kGuideStates, so they live in a
// second, wide class of the same shape and semantics:
//   guide_tab_wide [kGuideWidePool, kGuideWideStates, 256] (uint16) / guide_flags_wide [kGuideWidePool,
//     kGuideWideStates] (int32), allocated when the first schema guide arrives (until then both pointers are null
//     and pool_wide is 0).  A slot whose guide_meta entry word lies in [kGuidePool, kGuidePool + pool_wide) uses
//     wide entry word - kGuidePool; its state is valid below kGuideWideStates.  An entry word or a state outside
//     its class's range is dead: the row and the state stay untouched.  One launch mixes rows of every kind.
constexpr int kGuideStates = 512;
constexpr int kGuidePool = 32;     // resident patterns (32 x 512 x 256 x 2 B = 8 MiB)
constexpr int kGuideWideStates = 4096;
constexpr int kGuideWidePool = 4;  // resident schema guides (4 x 4096 x 256 x 2 B = 8 MiB)
constexpr int kGuideTokBytes = 32;
constexpr int kGuideDead = 0xFFFF;
constexpr int kGuideJson = -2;     // guide_meta entry word of a JSON-mode slot
constexpr int kJsonDepth = 64;
constexpr int kJsonStates = 128;   // (the table built by ops/reference.py json_table has 85)
constexpr int kJsonStart = 0, kJsonDone = 1, kJsonAfterObj = 2, kJsonAfterArr = 3;
struct GuideParams {
  const unsigned char* tok_bytes;
  const unsigned char* tok_len;
  const unsigned short* tab;
  int* flags;
  int* meta;               // [2, slots]
  int slots, pool;
  int v_global, eos;       // EOS's global id (< 0: none)
  const int* active;       // [B] or null
  const int* row_slot;     // [B] slot of row b, or null (row b = slot b)
  // mask pass
  float* logits;           // [B, ld], this rank's shard
  int ld, V, vocab_offset;
  // advance pass
  const int* ids;          // [B] committed (global) ids
  // live pass
  int entry, n_states;     // the entry word just uploaded (wide: kGuidePool + its wide entry) and its used states
  // JSON mode (both null: a kGuideJson slot is treated as guide off)
  const unsigned short* json_tab;  // [json_states, 256]
  int* json_state;                 // [4, slots]
  int json_states;
  // the wide class (both null and pool_wide 0: an entry word at or above kGuidePool is treated as guide off)
  const unsigned short* tab_wide;  // [pool_wide, kGuideWideStates, 256]
  int* flags_wide;                 // [pool_wide, kGuideWideStates]
  int pool_wide;
};

}  // namespace dsse

extern "C" {
hipError_t dsse_skinny_gemm(int mode, int mt, int nt, int kw, const void* X, int ldx, int M,
                            const void* W, int K, int N, const dsse::GemmEpi* ep, hipStream_t st);
hipError_t dsse_gemm_stream(int mode, int mt, int nt, int nw, int rd, int S, int partial_only, const void* X, int ldx, int M,
                            const void* W, int K, int N, const dsse::GemmEpi* ep, float* part, hipStream_t st);
hipError_t dsse_gemm_ring(int mode, int nw, int S, int partial_only, int ring2, const void* X, int ldx, int M,
                          const void* W, int K, int N, const dsse::GemmEpi* ep, float* part, hipStream_t st);
hipError_t dsse_gemm_w8(int mode, int nw, int S, int partial_only, const void* X, int ldx, int M, const void* W,
                        const float* scale, int K, int N, const dsse::GemmEpi* ep, float* part, hipStream_t st);
hipError_t dsse_gemm_w4(int mode, int nw, int S, int partial_only, const void* X, int ldx, int M, const void* W,
                        const void* E, int K, int N, const dsse::GemmEpi* ep, float* part, hipStream_t st);
hipError_t dsse_gemm_wide(int mode, int mb, int rd, int S, int partial_only, const void* X, int ldx, int M, const void* W,
                          int K, int N, const dsse::GemmEpi* ep, float* part, hipStream_t st);
hipError_t dsse_gemm_tiled(int mode, int cfg, int S, int partial_only, const void* X, int ldx, int M, const void* W,
                           int K, int N, const dsse::GemmEpi* ep, float* part, hipStream_t st);
hipError_t dsse_gemm_pipe(int mode, int bm, int S, int partial_only, const void* X, int ldx, int M, const void* W,
                          int K, int N, const dsse::GemmEpi* ep, float* part, hipStream_t st);
size_t dsse_gemm_pipe_fix_floats(int bm, int S, int M, int N);
size_t dsse_gemm_ring_fix_floats(int nw, int S, int M, int N);
hipError_t dsse_paged_attention(int mode, int num_work, const dsse::AttnParams* p, hipStream_t st);
hipError_t dsse_flash_prefill(int num_work, const dsse::AttnParams* p, hipStream_t st);
hipError_t dsse_sample(int B, const dsse::SampleParams* p, hipStream_t st);
hipError_t dsse_sample_pick(int B, int world, const void* cand, const dsse::SampleParams* p,
                            hipStream_t st);
hipError_t dsse_prefill_sample_gather(const void* x, int T, int H, const int* meta, int NS, const int* slot_meta, int Bm,
                                      void* xl, int* smeta, hipStream_t st);
hipError_t dsse_prefill_sample_commit(const int* meta, int NS, const int* new_ids, int* ids, int Bm, int* ring, int R,
                                      int* positions, const int* pen_meta, int* hist, int hist_ld, hipStream_t st);
hipError_t dsse_sample_penalties(int B, float* logits, const dsse::SampleParams* p, hipStream_t st);
hipError_t dsse_sample_bias_ban(int B, float* logits, const dsse::SampleParams* p, hipStream_t st);
hipError_t dsse_guide_live(const dsse::GuideParams* p, hipStream_t st);
hipError_t dsse_sample_guide_mask(int B, const dsse::GuideParams* p, hipStream_t st);
hipError_t dsse_sample_guide_advance(int B, const dsse::GuideParams* p, hipStream_t st);
hipError_t dsse_sample_hist_append(int n, const int* new_ids, const dsse::SampleParams* p, hipStream_t st);
hipError_t dsse_logprob_stats(int B, const dsse::LogprobParams* p, hipStream_t st);
hipError_t dsse_logprob_chosen(int B, const dsse::LogprobParams* p, hipStream_t st);
hipError_t dsse_logprob_finish(int B, const dsse::LogprobParams* p, hipStream_t st);
hipError_t dsse_rmsnorm(int mode, int M, float* resid, int H, const void* delta, const void* embed,
                        const int* ids, const void* w, void* y, float eps, const float* part, int nsplit,
                        int vocab, hipStream_t st);
hipError_t dsse_rope_kv_write(int T, const void* qkv, int hq, int hkv, const int* positions,
                              const int* slots, const float2* rope, void* q_out, void* k_cache,
                              void* v_cache, int num_slots, int rope_len, hipStream_t st);
// FP8 (e4m3) cache writers: k_inv = 1 / k_scale, v_inv = 1 / v_scale; y = the QKV projection's fp32 output
hipError_t dsse_rope_kv_write_f8(int T, const void* qkv, int hq, int hkv, const int* positions, const int* slots,
                                 const float2* rope, void* q_out, void* k_cache, void* v_cache, int num_slots,
                                 int rope_len, float k_inv, float v_inv, hipStream_t st);
hipError_t dsse_qkv_rope_f8(int M, const float* y, int hq, int hkv, const int* positions, const int* slots,
                            const float2* rope, void* q_out, void* k_cache, void* v_cache, int num_slots,
                            int rope_len, float k_inv, float v_inv, hipStream_t st);
hipError_t dsse_silu_mul(int T, int F, const void* gu, void* h, hipStream_t st);
hipError_t dsse_decode_prep(int B, const int* active, const int* positions, const int* block_tables,
                            int max_blocks, int num_blocks, int* slots, int* ctx_len, int* q_len, hipStream_t st);
hipError_t dsse_ring_advance(int* counter, hipStream_t st);
// KV page movers of the prefix cache's host tier (kv_pages.hip): gather = 1 copies the n pages listed in `blocks`
// (device memory) into staging records [K layer 0 .. L-1 | V layer 0 .. L-1] of 2 L seg_bytes each; gather = 0 copies
// the records back into the listed pages.  seg_bytes = Hkv * 4096 * itemsize (a multiple of 16); n = 0 launches nothing.
hipError_t dsse_kv_pages(int gather, int n, void* k_cache, void* v_cache, const int* blocks, void* staging, int L,
                         int num_blocks, unsigned seg_bytes, hipStream_t st);
// Page-to-page copy inside the cache (parallel sampling): pairs = [n, 2] (src_block, dst_block) in device memory; all
// 2 L segments of page src are copied onto page dst.  Destinations are distinct and none is a source (the host checks).
hipError_t dsse_kv_pages_copy(int n, void* k_cache, void* v_cache, const int* pairs, int L, int num_blocks,
                              unsigned seg_bytes, hipStream_t st);
// Multi-LoRA products (lora.hip): row i uses adapter slot row_adapter[i] (-1: none).  A = [nslots, SR, K] bf16,
// t = [M, SR] fp32; B = [nslots, N, R] bf16 (R in 8 / 16 / 32 / 64), scale = [nslots] fp32, slice_of_row = [N] in
// [0, S), S <= 3, SR = S R; out = [M, N] fp32 (out_f32) or bf16, rows with -1 untouched.
hipError_t dsse_lora_shrink(int M, int K, int SR, int nslots, const void* x, const void* A, const int* row_adapter,
                            float* t, hipStream_t st);
hipError_t dsse_lora_expand(int M, int N, int R, int S, int nslots, int out_f32, const float* t, const void* B,
                            const float* scale, const int* row_adapter, const int* slice_of_row, void* out,
                            hipStream_t st);
// TP all-reduce + residual + RMSNorm over IPC peer buffers (allreduce.hip)
size_t dsse_ar_buffer_bytes(int rows, int H);
hipError_t dsse_ar_alloc(size_t bytes, void** ptr, void* handle64, int* uncached);
hipError_t dsse_ar_open(const void* handle64, void** ptr);
hipError_t dsse_ar_close(void* ptr, int opened);
hipError_t dsse_ar_rmsnorm(int M, const void* tmp, float* resid, const void* w, void* y, int H, float eps,
                           const unsigned long long* peers, int rank, int world, int rows, unsigned int* epoch,
                           unsigned int* err, const float* part, int nsplit, hipStream_t st);
hipError_t dsse_ar_gather(int M, const void* in, void* out, const unsigned long long* peers, int rank, int world,
                          int rows, int H, unsigned int* gepoch, unsigned int* err, hipStream_t st);
// Checked build: first out-of-range index per kernel file (line, value, bound, count); zeros otherwise.
hipError_t dsse_check_gemm_skinny(int* out, int clear);
hipError_t dsse_check_gemm_stream(int* out, int clear);
hipError_t dsse_check_attention(int* out, int clear);
hipError_t dsse_check_attention_prefill(int* out, int clear);
hipError_t dsse_check_elementwise(int* out, int clear);
hipError_t dsse_check_sampler(int* out, int clear);
hipError_t dsse_check_gemm_tiled(int* out, int clear);
hipError_t dsse_check_kv_pages(int* out, int clear);
hipError_t dsse_check_gemm_w8(int* out, int clear);
hipError_t dsse_check_gemm_w4(int* out, int clear);
hipError_t dsse_check_lora(int* out, int clear);
// Stamps build: bind the step-anatomy record buffer (common.h stamps::) of a kernel file; no-ops otherwise.
hipError_t dsse_stamps_bind_gemm_stream(void* rec);
hipError_t dsse_stamps_bind_elementwise(void* rec);
}
