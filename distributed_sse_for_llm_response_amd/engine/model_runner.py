"""Mistral forward passes on the engine's kernels: hipGraph-captured decode step + chunked prefill.

Decode step for a batch bucket of B slots (all device-resident, no host round trip):

    decode_prep          slots / ctx_len / q_len from positions + block tables
    embed+rmsnorm        resid = E[ids]; x = norm(resid)
    per layer:
      qkv GEMM           x·Wqkvᵀ as fp32 split-K slabs
      paged_attention    sums the slabs, RoPE, writes this token's K/V into the paged cache, then
                         flash-decoding over the pages (+ partition combine)
      gemm_resid         resid += attn·Woᵀ          (TP>1: gemm_out + one fused IPC all-reduce + add + norm kernel)
      rmsnorm            x = norm(resid)
      gemm_silu          h = silu(x·Wgᵀ)·(x·Wuᵀ)
      gemm_resid         resid += h·Wdᵀ             (TP>1: gemm_out + all-reduce + add)
      rmsnorm            x = norm(resid) with the next layer's (or the final) weight
    gemm_out (fp32)      logits = x·Wlmᵀ (vocab shard)

    sample               Gumbel-max / greedy; ids[b] <- token, ring[head][b] <- token, positions += 1
    ring_advance         head += 1

The sampled token becomes the next step's input in place, so consecutive steps need no host sync;
the host drains the token ring asynchronously (engine.py).  The whole step is captured once per
batch bucket into a torch.cuda.CUDAGraph (a hipGraph on ROCm).
"""
from __future__ import annotations

import contextlib
import gc
import math
import os
import time
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from .. import ops
from ..ops.reference import rope_table
from ..parallel.comm import TPComm
from .kv_cache import PAGE, KVCache
from .weights import EngineWeights, parse_quantization, quantize_engine_weights

RING_SIZE = 64
SAMPLE_CHUNKS = 16  # vocab chunks per row in the candidate pass (B x 16 workgroups)
@contextlib.contextmanager
def _capture(graph, **kw):
    """torch.cuda.graph with the garbage collector off for the capture: a collection inside it could run a finaliser
    that destroys another object's graph or event (a HIP call that stream capture forbids: the process aborts)."""
    enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **kw):
            yield
    finally:
        if enabled:
            gc.enable()


PREFILL_TILE = 64   # query tokens per flash-prefill workgroup (attention_prefill.hip)
# Prefill batches of up to 2048 tokens replay a captured graph per row bucket (padded rows: slot -1, no K/V write,
# no attention work); larger batches (long prompts at an idle budget) run eagerly.  DSSE_PREFILL_GRAPHS=0 disables.
PREFILL_GRAPH_BUCKETS = (128, 256, 512, 1024, 2048)
PREFILL_GRAPH_SEQS = 16  # sequences per captured prefill batch (more: eager)
# Largest decode bucket on the fused-norm decode step (gemm_skinny / gemm_stream, split-K slabs reduced in the
# norms); larger buckets take the wide path (_decode_layers_wide), whose projections the kernel library routes to
# gemm_wide / gemm_tiled by row count (bindings.cpp gemm_impl).  Round 1 measured the split at 128 rows
# (profiles/bucket_ab_r1.md).
DECODE_GEMM_MAX_M = 128
# Health words (runner.health, int32 on the device, copied to the host with every drained step; nonzero = the step's
# outputs cannot be trusted and the engine fails: engine.py EngineFault).
HEALTH_TP_PEER = 0      # a TP peer's all-reduce row did not arrive in time (allreduce.hip)
HEALTH_WORDS = ("TP peer all-reduce wait timed out",)


# TP prefill: the row-independent post-attention half of each layer (O -> all-reduce -> norm -> gate_up -> down ->
# all-reduce -> norm) runs in row chunks so that each chunk's all-reduce (RCCL, a side stream) overlaps the next chunk's
# GEMMs (64 MiB all-reduces at 8k tokens, VERDICT r3 missing 1).  Chunked from
# DSSE_TP_PREFILL_OVERLAP_MIN rows, in DSSE_TP_PREFILL_CHUNKS chunks of whole 64-row tiles.
def flash_split_plan(tiles: list, hkv: int, min_blocks: int = 32, fill: int = 256, min_target: int = 16,
                     one_round: bool = True):
    """Key split of the flash prefill for an under-filled grid (round 6).  `tiles`: [(seq, tile, key blocks)]
    heaviest first.  With fewer than `fill` (tile, kv head) workgroups and a tile of >= `min_blocks` 64-key blocks (a
    TP = 8 rank has ONE kv head: an 8k prompt is 128 workgroups for 256 CUs, and the last tile walks 128 blocks
    alone), every tile longer than `target` blocks is cut into even key ranges: target = max(16, blocks x Hkv / fill),
    raised (one_round) until the ranges fit one round of `fill` workgroups.  Each range leaves partial O in its own
    slot and flash_combine_kernel merges a tile's slots.  Returns None (no split)
    or (work int32 [seq | tile | (kb0, kb1) pairs | slot], comb int32 [(seq, tile, first slot, slots)], slots), the
    work list heaviest range first."""
    if not tiles or len(tiles) * hkv >= fill or max(n for _, _, n in tiles) < min_blocks:
        return None
    # the smallest range length whose parts still fit one round of `fill` workgroups (one flash workgroup per CU):
    # a second round of leftover ranges would cost a whole range's time again
    nmax = max(n for _, _, n in tiles)
    target = max(min_target, -(-sum(n for _, _, n in tiles) * hkv // fill))
    if one_round:  # the smallest fitting length (the part count falls as the length grows): binary search
        ns = [n for _, _, n in tiles]
        lo, hi = target, max(target, nmax)
        while lo < hi:
            mid = (lo + hi) // 2
            if sum(-(-n // mid) for n in ns) * hkv > fill:
                lo = mid + 1
            else:
                hi = mid
        target = lo
    work, comb, nslots = [], [], 0
    for b, t, n in tiles:
        parts = -(-n // target)
        if parts == 1:
            work.append((n, b, t, 0, n, -1))
            continue
        per = -(-n // parts)
        comb.append((b, t, nslots, parts))
        for k in range(parts):
            work.append((min(n, (k + 1) * per) - k * per, b, t, k * per, min(n, (k + 1) * per), nslots + k))
        nslots += parts
    if not comb:
        return None
    work.sort(key=lambda x: -x[0])
    cols = list(zip(*work))
    kb = [v for a, e in zip(cols[3], cols[4]) for v in (a, e)]
    w = np.asarray(list(cols[1]) + list(cols[2]) + kb + list(cols[5]), dtype=np.int32)
    return w, np.asarray([v for c in comb for v in c], dtype=np.int32), nslots


def prefill_row_chunks(T: int, tp: int) -> list:
    """[(row0, row1)] of the overlapped TP prefill (one chunk when it does not apply)."""
    lo = int(os.environ.get("DSSE_TP_PREFILL_OVERLAP_MIN", "1024"))
    n = int(os.environ.get("DSSE_TP_PREFILL_CHUNKS", "4")) if tp > 1 and T >= lo else 1
    step = max(64, -(-T // max(1, n) // 64) * 64)
    return [(a, min(T, a + step)) for a in range(0, T, step)]


# prompt passes up to this many rows send the residual projections' split-K slabs to the norm (_prefill_resid)
PREFILL_SLAB_ROWS = 512


# Prompt-chunk sizes of the captured mixed steps: one graph per (decode bucket, C).  The engine sizes each step's
# chunk from the measured step costs (engine.PassCost.mixed_chunk); a prompt longer than the chunk is split evenly.
# B + C stays within MIXED_MAX_ROWS.  Round 5 set 512 because of a GEMM cliff at 576 rows; the round-6 cost-model
# dispatch removed that cliff (profiles/r6/gemm_model_r6.md), and 768 was re-measured with the serving bench at
# 40 req/s: TTFT p50 29.5 vs 29.8 ms, ITL p99 13.4 vs 10.7 ms (profiles/r6/serving_r6.md).  The bigger chunks buy no
# TTFT and cost ITL, so 512 stays.
MIXED_CHUNKS = (128, 256, 384, 512)
MIXED_MAX_ROWS = 512


def mixed_mode() -> str:
    """DSSE_MIXED: "1" (default) = prompt chunks ride in the decode step whenever streams decode (mixed prefill +
    decode steps, chunk sized per step from measured cost), "0" = separate prefill passes.  Separate passes keep
    TTFT lower but every pass is a whole extra weight stream between two decode tokens: ITL p99 ~3x the step
    (profiles/r4/serving_r4.md, profiles/r5/serving_r5.md)."""
    return os.environ.get("DSSE_MIXED", "1")


def batch_buckets(max_batch: int):
    """Captured decode batch sizes: powers of two up to 64, then every 64 (less padding at 65-256 streams)."""
    out, b = [], 1
    while b < max_batch:
        out.append(b)
        b = b * 2 if b < 64 else b + 64
    out.append(max_batch)
    return sorted(set(out))


def decode_partitioning(B: int, nkv: int, max_ctx: int, target_wgs: int = 512, max_parts: int = 32):
    """(part, nparts) for flash-decoding so that B·Hkv·nparts workgroups fill the chip.

    512 = two 256-thread workgroups per CU; at B·Hkv >= 512 (e.g. 64 streams x 8 KV heads) there is a
    single partition and the combine kernel is skipped.
    """
    want = max(1, min(max_parts, math.ceil(target_wgs / max(1, B * nkv))))
    part = max(128, math.ceil(max_ctx / want / 128) * 128)
    nparts = math.ceil(max_ctx / part)
    # several partitions: part 0 = each sequence's keys split evenly over them (attention.hip part_keys), so the
    # partitions stay busy at the served contexts, not only at max_ctx (TP = 8, 64 streams: 19 -> ~? us per layer,
    # profiles/r6/tp8_rank_decode_kernels_r6.md)
    return (0 if nparts > 1 else part), nparts


@dataclass
class PrefillSeq:
    slot: int               # decode slot the sequence occupies
    tokens: list            # token ids of this chunk
    start_pos: int          # absolute position of tokens[0]
    block_table: list       # the sequence's full block table
    last_chunk: bool        # sample a token after this chunk
    adapter: int = -1       # LoRA pool slot of the sequence (-1: the base model)


class SampleSite(NamedTuple):
    """The operands in which the three sampling sites differ (ModelRunner._sample runs the passes over them)."""
    logits: torch.Tensor        # fp32 [rows, local vocab]; the bias, penalty and guide passes rewrite it in place
    active: object              # int32 [rows], or None: every row samples
    row_slot: object            # int32 [rows]: row i samples for slot row_slot[i]; None: row i is slot i
    temperature: torch.Tensor   # the rows' sampling parameters ...
    top_k: torch.Tensor
    top_p: torch.Tensor
    seeds: torch.Tensor
    positions: torch.Tensor     # ... and the position of each row's predecessor token
    cand: torch.Tensor          # fp32 [rows, chunks, 2]: this rank's candidates
    cand_all: object            # fp32 [TP, rows, chunks, 2]: their all-gathered form (read when TP > 1)
    lp_bufs: object             # _lp_alloc's buffers for these rows (read once logprobs are in use)
    ids: torch.Tensor           # int32 [rows]: where the commit writes the sampled tokens
    ring: dict                  # logprob_finish's ring_* keyword: the ring row the tokens go to
    commit: str                 # "decode" | "graph" | "eager": the commit ops of the site (_sample)


class ModelRunner:
    def __init__(self, w: EngineWeights, num_blocks: int, max_batch: int = 64, max_model_len: int = 4096,
                 max_prefill_tokens: int = 8192, device="cuda", comm: TPComm | None = None, use_graphs=None,
                 kv_cache_dtype="auto", quantization=None, lora=None):
        # quantization "fp8": FP8 (e4m3) weights beside a widened bf16 copy (engine/weights.py).  Decode buckets of
        # W8_MAX_M rows or fewer run every projection and the LM head on the FP8 kernels over *_q; wider buckets,
        # prefill, mixed steps and the first-token head use the existing kernels over the widened *_t -- identical
        # weight values on both paths.  "mxfp4": the same arrangement with OCP MXFP4 weights (*_q nibbles, *_e block
        # scale bytes), W4_MAX_M and the MXFP4 kernels.  None = as the weights were loaded.
        if quantization is not None and parse_quantization(quantization) != "none":
            if (comm.size if comm is not None else 1) > 1:
                raise ValueError(f"quantization={parse_quantization(quantization)} is not supported with tensor "
                                 "parallelism (tp > 1)")
            quantize_engine_weights(w, quantization)
        self.quantization = {"fp8": "fp8_e4m3", "mxfp4": "mxfp4"}.get(w.quantization, "none")
        self.w8 = w.quantization == "fp8"
        self.w4 = w.quantization == "mxfp4"
        self.w, self.cfg = w, w.cfg
        self.device = torch.device(device)
        self.comm = comm or TPComm()
        # lora: an engine.lora.LoraPool on this device.  Until the first request that names an adapter nothing
        # changes; from then on every step runs the LoRA layer body (_lora_layers) in twins of the captured graphs
        if lora is not None:
            if self.comm.size > 1:
                raise ValueError("LoRA is not supported with tensor parallelism (tp > 1)")
            if self.w8:
                raise ValueError("LoRA is not supported with quantization=fp8")
            if self.w4:
                raise ValueError("LoRA is not supported with quantization=mxfp4")
        self.lora = lora
        self.lora_used = False  # a request ever named an adapter (then the LoRA body is launched / captured)
        self.max_batch = max_batch
        self.max_model_len = max_model_len
        self.max_blocks = math.ceil(max_model_len / PAGE) + 1
        self.max_prefill_tokens = max_prefill_tokens
        self.use_graphs = (self.device.type == "cuda") if use_graphs is None else use_graphs
        cfg, dev = self.cfg, self.device
        H = cfg.hidden_size
        nh, nkv, F, V = w.nh, w.nkv, w.ffn, w.vocab_local
        # kv_cache_dtype "fp8": float8_e4m3fn pages (half the bytes per token), quantised with the layers' k_scale /
        # v_scale by the cache writers and widened in registers by the attention kernels (every captured graph then
        # holds the fp8 ops, the scales as constants).  Prompt attention then runs on the paged prefill kernel (mode
        # 1): the flash kernel has no fp8 form.  Its work items are 64 / G query tokens (4 tiles of 16 / G).
        self.kv = KVCache(cfg.num_layers, num_blocks, nkv, dev, dtype=kv_cache_dtype)
        for li, L in enumerate(w.layers):
            self.kv.k_scale[li], self.kv.v_scale[li] = float(L.k_scale), float(L.v_scale)
        self.attn_tile = PREFILL_TILE if not self.kv.is_fp8 else 64 // (nh // nkv)
        self.rope = rope_table(max(cfg.max_position, max_model_len + 1), cfg.rope_theta, dev)
        Bm = max_batch
        i32 = dict(device=dev, dtype=torch.int32)
        # ---- decode state (slot-indexed, device resident) ----
        self.ids = torch.zeros(Bm, **i32)
        self.positions = torch.zeros(Bm, **i32)
        # per-slot sampling state in ONE int32 buffer [active | temperature | top_k | top_p | seeds (Bm x 2)] (the
        # float fields are views of their words): the engine uploads a changed slot set with one pinned copy
        # (LLMEngine._upload)
        self.slot_meta = torch.zeros(6 * Bm, **i32)
        self.active = self.slot_meta[:Bm]
        self.block_tables = torch.zeros(Bm, self.max_blocks, **i32)
        self.slots = torch.full((Bm,), -1, **i32)
        # LoRA pool slot per decode slot (-1: none), host-owned and uploaded like lp_meta (LLMEngine._upload)
        self.slot_adapter = torch.full((Bm,), -1, **i32)
        self.ctx_len = torch.zeros(Bm, **i32)
        self.q_len = torch.zeros(Bm, **i32)
        self.q_start = torch.arange(Bm, **i32)
        self.work_seq = torch.arange(Bm, **i32)
        self.work_tile = torch.zeros(Bm, **i32)
        self.temperature = self.slot_meta[Bm:2 * Bm].view(torch.float32)
        self.top_k = self.slot_meta[2 * Bm:3 * Bm]
        self.top_p = self.slot_meta[3 * Bm:4 * Bm].view(torch.float32)
        self.top_p.fill_(1.0)
        self.seeds = self.slot_meta[4 * Bm:].view(Bm, 2)
        # presence / frequency / repetition penalties (sampler.hip sample_penalty_kernel): pen_meta = [presence |
        # frequency | repetition (float32 views) | n_prompt] per slot, host-owned and uploaded like slot_meta;
        # hist_state[slot] = [tokens held | prompt, then generated tokens], written by the engine when a penalised
        # sequence takes the slot (set_history) and device-owned afterwards: every sampled token is appended in
        # stream order by the pick / commit kernels.  max_model_len + 1 tokens hold everything a sequence can sample.
        self.pen_meta = torch.zeros(4 * Bm, **i32)
        self.presence = self.pen_meta[:Bm].view(torch.float32)
        self.frequency = self.pen_meta[Bm:2 * Bm].view(torch.float32)
        self.repetition = self.pen_meta[2 * Bm:3 * Bm].view(torch.float32)
        self.repetition.fill_(1.0)
        self.n_prompt = self.pen_meta[3 * Bm:]
        self.hist_state = torch.zeros(Bm, max_model_len + 2, **i32)
        self.hist_len = self.hist_state[:, 0]
        self.hist = self.hist_state[:, 1:]
        self.hist_used = False  # a history was ever uploaded (move_slots then moves the rows too)
        self.ring = torch.zeros(RING_SIZE, Bm, **i32)
        self.ring_counter = torch.zeros(1, **i32)
        # logprobs / top_logprobs (sampler.hip logprob_*_kernel): lp_meta[slot] = -1 (off) or N in 0..20, host-owned
        # and uploaded like slot_meta; lp_ring[ring row, slot] = [logprob of the sampled token | 20 ids | 20 logprobs]
        # is written where the token itself goes and drained with it (LLMEngine._Drain)
        self.lp_meta = torch.full((Bm,), -1, **i32)
        self.lp_ring = torch.zeros(RING_SIZE, Bm, ops.LP_OUT, device=dev, dtype=torch.float32)
        self.lp_used = False  # a request ever asked for logprobs (then the passes are launched / captured)
        self._lp_raw = None   # [rows, V] raw copy of the logprob rows, allocated once penalties AND logprobs are in use
        # logit_bias / min_tokens / stop_token_ids / min_p (sampler.hip sample_bias_ban_kernel, row_min_p): ctl_meta =
        # [bias entries | banned ids | ban-until position | min_p (float32 view)] per slot, host-owned and uploaded
        # like slot_meta (all zero = neutral); ctl_body[slot] = [300 x (global id, bias bits) | 17 banned ids],
        # written by the engine when a sequence that uses it takes the slot (set_controls)
        self.ctl_meta = torch.zeros(4 * Bm, **i32)
        self.min_p = self.ctl_meta[3 * Bm:].view(torch.float32)
        self.ctl_body = torch.zeros(Bm, ops.CTL_BODY, **i32)
        self.ctl_used = False  # a request ever used one of them (then the pass is launched / captured)
        # guided decoding (sampler.hip sample_guide_mask_kernel / sample_guide_advance_kernel; records: api.h): the
        # token byte table, the pool of transition tables and guide_meta = [pool index (-1 = off) | DFA state] per slot
        # are allocated by the first guided request (enable_guides), like the twins' buffers
        self.guide_used = False
        self.guide_eos = -1
        self.guide_pieces = None  # the vocabulary's pieces (set_guide_vocab): what the byte table is built from
        self.tok_bytes = self.tok_len = self.guide_tab = self.guide_flags = self.guide_meta = self.guide_host = None
        # the wide pool of schema guides (guided_json / response_format json_schema): allocated by the first schema
        # guide (enable_wide_guides), entry words ops.GUIDE_POOL + e
        self.guide_tab_wide = self.guide_flags_wide = None
        # JSON mode (response_format json_object): the pushdown automaton's table and json_state = [lexical state |
        # depth | stack bits 0..31 | stack bits 32..63] per slot, for the slots whose guide_meta pool index is
        # ops.JSON_ENTRY; allocated with the rest by enable_guides
        self.json_tab = self.json_state = None
        # ---- decode activations ----
        bf = dict(device=dev, dtype=torch.bfloat16)
        self.resid = torch.zeros(Bm, H, device=dev, dtype=torch.float32)
        self.x = torch.zeros(Bm, H, **bf)
        self.q = torch.zeros(Bm, nh * 128, **bf)
        self.attn = torch.zeros(Bm, nh * 128, **bf)
        self.h = torch.zeros(Bm, F, **bf)
        self.tmp = torch.zeros(Bm, H, **bf)
        if lora is not None:
            # the LoRA body's unfused outputs (decode rows) and the shrink result t [rows, S·R] of any pass
            self.lora_qkv = torch.zeros(Bm, (nh + 2 * nkv) * 128, **bf)
            self.lora_gu = torch.zeros(Bm, 2 * F, **bf)
            self._lora_t = torch.zeros(max(Bm, min(max(PREFILL_GRAPH_BUCKETS), max_prefill_tokens)) * 3 * lora.R,
                                       device=dev, dtype=torch.float32)
        # fp32 split-K slabs of the residual projections (reduced inside the next RMSNorm)
        # (on a GPU also large enough for the 8 slabs of a PREFILL_SLAB_ROWS-row prompt pass: _prefill_resid)
        slab_floats = 32 * Bm * H
        if torch.device(dev).type == "cuda":
            slab_floats = max(slab_floats, 8 * min(PREFILL_SLAB_ROWS, max_prefill_tokens) * H)
        self.split_part = torch.zeros(slab_floats, device=dev, dtype=torch.float32)
        self.health = torch.zeros(4, device=dev, dtype=torch.int32)
        self.logits = torch.zeros(Bm, V, device=dev, dtype=torch.float32)
        nch = SAMPLE_CHUNKS if dev.type == "cuda" else 1
        self._cand = {b: torch.zeros(b, nch, 2, device=dev, dtype=torch.float32) for b in batch_buckets(Bm)}
        self._cand_all = {b: torch.zeros(self.comm.size, b, nch, 2, device=dev, dtype=torch.float32)
                          for b in batch_buckets(Bm)}
        self._lp_bufs = {b: self._lp_alloc(b) for b in batch_buckets(Bm)}
        self._lp_pf = self._lp_alloc(PREFILL_GRAPH_SEQS)
        self._lp_eager = None  # the eager first-token path's buffers (max_batch rows, allocated at its first use)
        part, nparts = decode_partitioning(1, nkv, max_model_len)
        ws = max(decode_partitioning(b, nkv, max_model_len)[1] * b for b in batch_buckets(Bm))
        self.part_o = torch.zeros(max(1, ws) * nkv * 16 * 128, device=dev, dtype=torch.float32)
        self.part_ml = torch.zeros(max(1, ws) * nkv * 16 * 2, device=dev, dtype=torch.float32)
        # TP decode: the residual all-reduces on the fused IPC kernel (parallel/comm.py IpcAllReduce), RCCL otherwise
        self.fast_ar_reason = self.comm.enable_ipc_allreduce(dev, Bm, H) if self.comm.size > 1 else "tp=1"
        if self.comm.fast_ar is not None:
            # a timed-out peer wait now marks this runner's health word (checked at every drained step)
            self.comm.fast_ar.err = self.health[HEALTH_TP_PEER:HEALTH_TP_PEER + 1]
        if self.comm.size > 1 and self.comm.rank == 0:
            print(f"[engine] TP={self.comm.size} decode all-reduce + candidate all-gather: "
                  f"{'IPC kernels' if not self.fast_ar_reason else 'RCCL (' + self.fast_ar_reason + ')'}", flush=True)
        self.graphs = {}
        self.graph_pool = None
        self.pf_graphs = {}   # row bucket -> captured prefill graph
        self.pf = None        # static prefill buffers (allocated by capture)
        self.mx_graphs = {}   # decode bucket B -> [(chunk rows C, captured mixed prefill + decode graph)], C ascending
        # their twins per pass set (_twin_key: penalties, logprobs, the bias and ban pass / min_p, guides in use), each
        # captured the first time that combination is needed (_capture_twins); pen_* = the (True, False, False, False)
        # set: the penalty pass and nothing else new
        self.pen_graphs, self.pen_pf_graphs, self.pen_mx_graphs = {}, {}, {}
        self._twins = {(True, False, False, False): (self.pen_graphs, self.pen_pf_graphs, self.pen_mx_graphs)}
        self._captured_key = (False, False, False, False)  # the passes the graphs of capture() hold (set there)
        self.host_trace = None  # a list: host seconds of each graph-replayed mixed step (upload, replay, sampling)

    # ------------------------------------------------------------------ decode
    def decode_forward(self, B: int) -> None:
        """One decode step over slots [0, B) (graph-capturable: fixed shapes, no host sync)."""
        w, cfg, comm = self.w, self.cfg, self.comm
        nh, nkv = w.nh, w.nkv
        r = slice(0, B)
        eps = cfg.rms_eps
        ops.decode_prep(self.active[r], self.positions[r], self.block_tables[r], self.slots[r], self.ctx_len[r],
                        self.q_len[r], self.kv.num_blocks)
        resid, x = self.resid[r], self.x[r]
        ops.rmsnorm(resid, w.layers[0].attn_norm, x, eps, embed=w.embed, ids=self.ids[r])
        part, nparts = decode_partitioning(B, nkv, self.max_model_len)
        nl = len(w.layers)
        if self.lora_used:  # every bucket: the unfused body with the low-rank deltas
            d = dict(resid=resid, x=x, q=self.q[r].view(B, nh, 128), attn=self.attn[r].view(B, nh, 128), h=self.h[r],
                     tmp=self.tmp[r], qkv=self.lora_qkv[r], gu=self.lora_gu[r])
            self._lora_layers(B, d, self.positions[r], self.slots[r], self.slot_adapter[r])
            for b0 in range(0, B, 256):
                ops.gemm_out(x[b0:b0 + 256], w.lm_head_t, self.logits[b0:min(B, b0 + 256)])
            self._sample_commit(B)
            ops.ring_advance(self.ring_counter)
            return
        if B > DECODE_GEMM_MAX_M:
            self._decode_layers_wide(B, resid, x, part, nparts)
            return
        if self.w8 and B <= ops.W8_MAX_M:
            for li, L in enumerate(w.layers):
                self._qkv_attention(li, L, B, x, part, nparts)
                self._resid_proj_w8(self.attn[r], L.wo_q, L.wo_scale, resid, L.ffn_norm, x)
                ops.gemm_silu_w8(x, L.wgu_q, L.wgu_scale, self.h[r])
                w_next = w.layers[li + 1].attn_norm if li + 1 < nl else w.final_norm
                self._resid_proj_w8(self.h[r], L.wd_q, L.wd_scale, resid, w_next, x)
            ops.gemm_out_w8(x, w.lm_head_q, w.lm_head_scale, self.logits[r])
            self._sample_commit(B)
            ops.ring_advance(self.ring_counter)
            return
        if self.w4 and B <= ops.W4_MAX_M:
            for li, L in enumerate(w.layers):
                self._qkv_attention(li, L, B, x, part, nparts)
                self._resid_proj_w4(self.attn[r], L.wo_q, L.wo_e, resid, L.ffn_norm, x)
                ops.gemm_silu_w4(x, L.wgu_q, L.wgu_e, self.h[r])
                w_next = w.layers[li + 1].attn_norm if li + 1 < nl else w.final_norm
                self._resid_proj_w4(self.h[r], L.wd_q, L.wd_e, resid, w_next, x)
            ops.gemm_out_w4(x, w.lm_head_q, w.lm_head_e, self.logits[r])
            self._sample_commit(B)
            ops.ring_advance(self.ring_counter)
            return
        for li, L in enumerate(w.layers):
            self._qkv_attention(li, L, B, x, part, nparts)
            self._resid_proj(self.attn[r], L.wo_t, resid, L.ffn_norm, x, self.tmp[r])
            ops.gemm_silu(x, L.wgu_t, self.h[r])
            w_next = w.layers[li + 1].attn_norm if li + 1 < nl else w.final_norm
            self._resid_proj(self.h[r], L.wd_t, resid, w_next, x, self.tmp[r])
        ops.gemm_out(x, w.lm_head_t, self.logits[r])
        self._sample_commit(B)
        ops.ring_advance(self.ring_counter)

    def _decode_layers_wide(self, B: int, resid, x, part: int, nparts: int) -> None:
        """Decode step for buckets above DECODE_GEMM_MAX_M sequences (256 streams per GPU, BASELINE config 3).

        At B > 128 a weight byte feeds > 128 rows and the projections become compute-heavy skinny GEMMs; they run
        on the engine's tiled-layout GEMMs with fused epilogues (QKV + RoPE + KV write, residual + split-K norm,
        SiLU·mul) -- gemm_wide or the register-blocked gemm_tiled, chosen per shape by the kernel library.  The
        LM head stays on the fp32-output GEMM in 256-row blocks (sampling wants fp32 logits).  One captured graph
        per bucket.
        """
        w, cfg, comm = self.w, self.cfg, self.comm
        nh, nkv = w.nh, w.nkv
        r = slice(0, B)
        eps = cfg.rms_eps
        nl = len(w.layers)
        for li, L in enumerate(w.layers):
            self._qkv_attention(li, L, B, x, part, nparts)
            self._resid_proj(self.attn[r], L.wo_t, resid, L.ffn_norm, x, self.tmp[r])
            self._gate_up(x, L, self.h[r])
            w_next = w.layers[li + 1].attn_norm if li + 1 < nl else w.final_norm
            self._resid_proj(self.h[r], L.wd_t, resid, w_next, x, self.tmp[r])
        step = 256 if DECODE_GEMM_MAX_M > 2 else DECODE_GEMM_MAX_M  # one 256-row call streams the head once
        for b0 in range(0, B, step):
            b1 = min(B, b0 + step)
            ops.gemm_out(x[b0:b1], w.lm_head_t, self.logits[b0:b1])
        self._sample_commit(B)
        ops.ring_advance(self.ring_counter)

    def _qkv_attention(self, li: int, L, B: int, x, part: int, nparts: int) -> None:
        """QKV projection + RoPE + KV write + decode attention of layer li.  The projection's split-K slabs go
        to split_part (free here: the previous norm consumed it) and the attention kernel folds their reduction,
        RoPE and the K/V write in (ops.qkv_attention_decode)."""
        r = slice(0, B)
        nh, nkv = self.w.nh, self.w.nkv
        if self.w8 and B <= ops.W8_MAX_M:
            ops.qkv_attention_decode_w8(x, L.wqkv_q, L.wqkv_scale, self.positions[r], self.slots[r], self.rope,
                                        self.q[r], self.kv.k[li], self.kv.v[li], nh, nkv, self.split_part,
                                        self.block_tables[r], self.q_start[r], self.q_len[r], self.ctx_len[r],
                                        self.work_seq[r], self.work_tile[r], self.attn[r], self.part_o, self.part_ml,
                                        part, nparts, *self._kv_scales(li))
            return
        if self.w4 and B <= ops.W4_MAX_M:
            ops.qkv_attention_decode_w4(x, L.wqkv_q, L.wqkv_e, self.positions[r], self.slots[r], self.rope,
                                        self.q[r], self.kv.k[li], self.kv.v[li], nh, nkv, self.split_part,
                                        self.block_tables[r], self.q_start[r], self.q_len[r], self.ctx_len[r],
                                        self.work_seq[r], self.work_tile[r], self.attn[r], self.part_o, self.part_ml,
                                        part, nparts, *self._kv_scales(li))
            return
        ops.qkv_attention_decode(x, L.wqkv_t, self.positions[r], self.slots[r], self.rope, self.q[r], self.kv.k[li],
                                 self.kv.v[li], nh, nkv, self.split_part, self.block_tables[r], self.q_start[r],
                                 self.q_len[r], self.ctx_len[r], self.work_seq[r], self.work_tile[r], self.attn[r],
                                 self.part_o, self.part_ml, part, nparts, *self._kv_scales(li))

    # ------------------------------------------------------------------ LoRA
    def enable_lora(self) -> None:
        """The first request that names an adapter: from now on every step (decode, prefill, mixed) runs the LoRA
        layer body, in graph twins captured here; base-model rows ride in them with adapter -1."""
        if self.lora is None:
            raise ValueError("this engine was started without a LoRA pool (--enable-lora)")
        if not self.lora_used:
            if self.device.type == "cuda":
                # the two kernels' first launch (code object load) happens here, eagerly, not inside the capture:
                # one row without an adapter writes zeros to the t scratch and leaves the output untouched
                none = torch.full((1,), -1, device=self.device, dtype=torch.int32)
                self._lora_delta("qkv", 0, self.x[:1], self.lora_qkv[:1], none)
                # and the unfused projections at every captured row count, into scratch buffers only (as capture()
                # warms its shapes: kernel attributes and the dispatch's state are set outside the capture)
                L, nh = self.w.layers[0], self.w.nh
                rows = set(self.graphs) | set(self.pf_graphs) | {B + C for B, lst in self.mx_graphs.items() for C, _ in lst}
                for m in sorted(rows):
                    b = self.pf if self.pf is not None and m <= self.pf.tmax else None
                    if b is None and m > self.max_batch:
                        continue
                    x, attn, h, tmp = ((b.x, b.attn, b.h, b.tmp) if b is not None else
                                       (self.x, self.attn, self.h, self.tmp))
                    qkv, gu = (b.qkv, b.gu) if b is not None else (self.lora_qkv, self.lora_gu)
                    ops.gemm_out(x[:m], L.wqkv_t, qkv[:m])
                    ops.gemm_out(attn[:m].view(m, nh * 128), L.wo_t, tmp[:m])
                    ops.gemm_out(x[:m], L.wgu_t, gu[:m])
                    ops.gemm_out(h[:m], L.wd_t, tmp[:m])
                torch.cuda.synchronize(self.device)
            self.lora_used = True
            self._capture_twins()

    def _lora_delta(self, p: str, li: int, x, out, ra) -> None:
        """out += the rows' adapter deltas of projection p (qkv / o / gu / d) of layer li: one shrink over x for all
        of the projection's slices, then the expand-add with the slice id of each output row."""
        P = self.lora
        M, SR = x.shape[0], P.A[p].shape[2]
        t = self._lora_t[:M * SR].view(M, SR) if M * SR <= self._lora_t.numel() else \
            torch.empty(M, SR, device=self.device, dtype=torch.float32)  # (an eager prompt pass above the buckets)
        ops.lora_shrink(x, P.A[p][li], ra, t)
        ops.lora_expand_add(t, P.B[p][li], P.scale, ra, P.slice_of_row[p], out)

    def _lora_layers(self, B: int, d: dict, pos, slots, ra, split: bool = False) -> None:
        """Every layer over M rows with per-row adapters `ra` (int32 [M], -1 = none): rows [0, B) are decode rows,
        the rest the packed prompt rows that d's prefill metadata describes.  The fused kernels cannot take a delta
        (they fold RoPE and the KV write into attention, SiLU·mul into the epilogue, the split-K sum into the norm), so
        this body is built from the unfused ops: each projection's bf16 output, the delta added to it in place
        (before RoPE / SiLU / the residual add), then the consumer.  One body for decode, prefill and mixed steps."""
        w, eps = self.w, self.cfg.rms_eps
        nh, nkv = w.nh, w.nkv
        resid, x, q, attn, h, tmp, qkv, gu = (d[k] for k in ("resid", "x", "q", "attn", "h", "tmp", "qkv", "gu"))
        M = x.shape[0]
        r = slice(0, B)
        dpart, dnparts = decode_partitioning(max(B, 1), nkv, self.max_model_len)
        nl = len(w.layers)
        for li, L in enumerate(w.layers):
            kc, vc = self.kv.k[li], self.kv.v[li]
            ops.gemm_out(x, L.wqkv_t, qkv)
            self._lora_delta("qkv", li, x, qkv, ra)
            ops.rope_kv_write(qkv, pos, slots, self.rope, q, kc, vc, nh, nkv, *self._kv_scales(li))
            if B:
                ops.paged_attention(0, q[r], kc, vc, self.block_tables[r], self.q_start[r], self.q_len[r],
                                    self.ctx_len[r], self.work_seq[r], self.work_tile[r], attn[r], self.part_o,
                                    self.part_ml, dpart, dnparts, *self._kv_scales(li))
            if M > B:
                self._prefill_attention(li, q, attn, d, split=split)
            a2 = attn.view(M, nh * 128)
            ops.gemm_out(a2, L.wo_t, tmp)
            self._lora_delta("o", li, a2, tmp, ra)
            ops.rmsnorm(resid, L.ffn_norm, x, eps, delta=tmp)
            ops.gemm_out(x, L.wgu_t, gu)
            self._lora_delta("gu", li, x, gu, ra)
            ops.silu_mul(gu, h)
            ops.gemm_out(h, L.wd_t, tmp)
            self._lora_delta("d", li, h, tmp, ra)
            w_next = w.layers[li + 1].attn_norm if li + 1 < nl else w.final_norm
            ops.rmsnorm(resid, w_next, x, eps, delta=tmp)

    def _kv_scales(self, li: int) -> tuple:
        """(k_scale, v_scale) of layer li's cache: trailing arguments of the cache ops (1.0, 1.0 for bf16)."""
        return (self.kv.k_scale[li], self.kv.v_scale[li]) if self.kv.is_fp8 else (1.0, 1.0)

    def _prefill_attention(self, li: int, q, attn, d: dict, split: bool = False) -> None:
        """Prompt attention of layer li over the packed chunk rows: the flash kernel (64-query tiles; its key split
        when the plan has slots), or -- fp8 cache -- the paged prefill kernel on work items of attn_tile queries."""
        kc, vc = self.kv.k[li], self.kv.v[li]
        if self.kv.is_fp8:
            ops.paged_attention(1, q, kc, vc, d["bt"], d["qs"], d["ql"], d["ctx"], d["ws"], d["wt"], attn,
                                self.part_o, self.part_ml, d["part"], 1, *self._kv_scales(li))
        elif split and d.get("fslots"):
            ops.flash_prefill_split(q, kc, vc, d["bt"], d["qs"], d["ql"], d["ctx"], d["fw"], d["fc"], attn, d["fpo"],
                                    d["fpm"], d["fslots"])
        else:
            ops.paged_attention(2, q, kc, vc, d["bt"], d["qs"], d["ql"], d["ctx"], d["ws"], d["wt"], attn,
                                self.part_o, self.part_ml, d["part"], 1)

    def _resid_proj(self, a, wt, resid, norm_w, x, tmp) -> None:
        """resid += a·wᵀ (TP: all-reduced), then x = RMSNorm(resid)·norm_w.  TP = 1: split-K slabs (if the GEMM
        splits) are reduced inside the norm; TP > 1: the bf16 partial product is all-reduced first."""
        eps = self.cfg.rms_eps
        if self.comm.size == 1:
            ns = ops.gemm_resid_split(a, wt, resid, self.split_part)
            ops.rmsnorm(resid, norm_w, x, eps, part=self.split_part, nsplit=ns)
        elif self.comm.ipc_rows(a.shape[0]) and a.is_cuda:
            # the IPC all-reduce kernel sums the GEMM's split-K slabs itself (no splitk_reduce launch)
            ns = ops.gemm_out_split(a, wt, tmp, self.split_part)
            self.comm.all_reduce_rmsnorm(tmp, resid, norm_w, x, eps, part=self.split_part, nsplit=ns)
        else:
            ops.gemm_out(a, wt, tmp)
            self.comm.all_reduce_rmsnorm(tmp, resid, norm_w, x, eps)

    def _resid_proj_w8(self, a, wq, ws, resid, norm_w, x) -> None:
        """_resid_proj over an FP8 weight (TP = 1): the scaled split-K slabs are reduced inside the norm."""
        ns = ops.gemm_resid_split_w8(a, wq, ws, resid, self.split_part)
        ops.rmsnorm(resid, norm_w, x, self.cfg.rms_eps, part=self.split_part, nsplit=ns)

    def _resid_proj_w4(self, a, wq, we, resid, norm_w, x) -> None:
        """_resid_proj over an MXFP4 weight (TP = 1): the split-K slabs are reduced inside the norm."""
        ns = ops.gemm_resid_split_w4(a, wq, we, resid, self.split_part)
        ops.rmsnorm(resid, norm_w, x, self.cfg.rms_eps, part=self.split_part, nsplit=ns)

    def _sample_commit(self, B: int) -> None:
        """The decode step's sampling (decode and mixed graphs): row b is slot b, the pick commits ids / ring row /
        positions itself."""
        r = slice(0, B)
        self._sample(SampleSite(self.logits[r], self.active[r], None, self.temperature[r], self.top_k[r],
                                self.top_p[r], self.seeds[r], self.positions[r], self._cand[B], self._cand_all[B],
                                self._lp_bufs[B], self.ids[r], dict(ring_counter=self.ring_counter), "decode"))

    def _sample(self, s: SampleSite) -> None:
        """Every sampling site's passes, in the one order they have (docs/kernels.md, "Sampler"):

            logprob stats -> bias / ban -> penalties -> guide mask -> candidates (with min_p once the bias and ban
            pass is in use) -> (TP: all-gather, 8 B per candidate) -> the site's commit -> guide advance -> logprob
            chosen / finish

        The statistics come first because the next three passes rewrite the logits in place; the guide mask is last
        before the candidates so that nothing un-masks a token; the two passes after the commit read the committed
        ids only.  Each optional pass is launched (and captured: _capture_twins) only once a request has asked for
        its feature; rows with neutral parameters return at once."""
        w, cfg, comm = self.w, self.cfg, self.comm
        if self.lp_used:
            raw = self._logprob_stats(s.logits, s.active, s.row_slot, s.lp_bufs)
        if self.ctl_used:  # logit_bias and the min_tokens ban
            ops.sample_bias_ban(s.logits, s.active, self.ctl_meta, self.ctl_body, s.positions, s.row_slot,
                                w.vocab_offset, cfg.vocab_size)
        if self.hist_used:
            # (first-token sites after a re-prefill: the tokens already published count, the engine uploaded them
            # with the history)
            ops.sample_penalties(s.logits, s.active, self.pen_meta, self.hist_state, s.row_slot, w.vocab_offset,
                                 cfg.vocab_size)
        if self.guide_used:
            self._guide_mask(s.logits, s.active, s.row_slot)
        rows = (s.logits, s.temperature, s.top_k, s.top_p, s.seeds, s.positions, s.active, s.cand)
        if self.ctl_used:  # min_p: ctl_meta's fourth column, slot-indexed
            ops.sample_candidates_min_p(*rows, self.ctl_meta, s.row_slot, w.vocab_offset)
        else:
            ops.sample_candidates(*rows, w.vocab_offset)
        if comm.size == 1:
            cand_all = s.cand.unsqueeze(0)
        else:
            cand_all = s.cand_all
            comm.all_gather_into(cand_all, s.cand)
        if s.commit == "decode":  # the pick also writes the ring row, positions += 1 and the penalised histories
            ops.sample_pick_hist(cand_all, s.active, s.ids, self.ring, self.ring_counter, s.positions, self.pen_meta,
                                 self.hist_state, vocab=cfg.vocab_size)
        else:
            ops.sample_pick(cand_all, s.active, s.ids, vocab=cfg.vocab_size)
            if s.commit == "graph":
                ops.prefill_sample_commit_hist(self.pf.samp_meta(), s.ids, self.ids, self.ring, self.positions,
                                               self.pen_meta, self.hist_state)
            elif self.hist_used:  # "eager": the site copies ids / ring row / positions itself
                ops.sample_hist_append(s.ids, s.row_slot, None, self.pen_meta, self.hist_state)
        if self.guide_used:  # the committed token advances its slot's DFA state
            self._guide_advance(s.ids, s.active, s.row_slot)
        if self.lp_used:  # (decode: before ring_advance, the same ring row the pick wrote)
            self._logprob_finish(s.logits, raw, s.ids, s.active, s.row_slot, s.lp_bufs, **s.ring)

    # ------------------------------------------------------------------ logprobs
    def _lp_alloc(self, n: int) -> dict:
        """Record / chosen-logit buffers of an n-row sampling site (and their all-gathered forms under TP)."""
        f32 = dict(device=self.device, dtype=torch.float32)
        d = dict(rec=torch.zeros(n, ops.LP_REC, **f32), chosen=torch.zeros(n, **f32))
        if self.comm.size > 1:
            d.update(rec_all=torch.zeros(self.comm.size, n, ops.LP_REC, **f32),
                     chosen_all=torch.zeros(self.comm.size, n, **f32))
        return d

    def _lp_eager_bufs(self, n: int) -> dict:
        """Buffers of an n-row eager first-token sampling (n <= max_batch): contiguous views of one cached set."""
        if self._lp_eager is None:
            self._lp_eager = {k: v.view(-1) for k, v in self._lp_alloc(self.max_batch).items()}
        e, W = self._lp_eager, self.comm.size
        d = dict(rec=e["rec"][:n * ops.LP_REC].view(n, ops.LP_REC), chosen=e["chosen"][:n])
        if W > 1:
            d.update(rec_all=e["rec_all"][:W * n * ops.LP_REC].view(W, n, ops.LP_REC),
                     chosen_all=e["chosen_all"][:W * n].view(W, n))
        return d

    def _logprob_stats(self, logits, active, row_slot, bufs):
        """Per-rank (max, sum, top-N) records of the rows whose slot has logprobs on, from the logits as the LM head
        wrote them.  Returns the raw copy of those rows when a penalty pass follows (else None)."""
        raw = self._lp_raw[:logits.shape[0]] if self.hist_used else None
        ops.logprob_stats(logits, active, self.lp_meta, row_slot, bufs["rec"], raw, self.w.vocab_offset)
        return raw

    def _logprob_finish(self, logits, raw, ids, active, row_slot, bufs, **ring) -> None:
        """After the pick / commit: this shard's raw logit of each sampled token, (TP: the records and those 4 B per
        row all-gathered,) then the merge into lp_ring at the token's own (ring row, slot)."""
        ops.logprob_chosen(logits if raw is None else raw, ids, active, self.lp_meta, row_slot, bufs["chosen"],
                           self.w.vocab_offset, self.cfg.vocab_size)
        if self.comm.size == 1:
            rec_all, chosen_all = bufs["rec"].unsqueeze(0), bufs["chosen"].unsqueeze(0)
        else:
            rec_all, chosen_all = bufs["rec_all"], bufs["chosen_all"]
            self.comm.all_gather_into(rec_all, bufs["rec"])
            self.comm.all_gather_into(chosen_all, bufs["chosen"])
        ops.logprob_finish(rec_all, chosen_all, active, self.lp_meta, row_slot, self.lp_ring,
                           vocab=self.cfg.vocab_size, **ring)

    def enable_logprobs(self) -> None:
        """The first request with logprobs: from now on every sampling site runs the logprob passes (rows whose slot
        is off return at once) and the graph twins that hold them are replayed."""
        if not self.lp_used:
            self.lp_used = True
            self._capture_twins()

    def set_history(self, slot: int, tokens: list, n_prompt: int) -> None:
        """A penalised sequence takes `slot`: its tokens so far (the submitted prompt, then what it has published)
        and their count become the slot's history, with one pinned non-blocking copy ordered after every step
        already enqueued.  The device owns the row afterwards.  (n_prompt itself travels in pen_meta.)"""
        row = torch.tensor([len(tokens)] + list(tokens), dtype=torch.int32)
        if row.numel() > self.hist_state.shape[1]:
            raise ValueError(f"history of {len(tokens)} tokens exceeds max_model_len + 1")
        if self.device.type == "cuda":
            row = row.pin_memory()
        self.hist_state[slot, :row.numel()].copy_(row, non_blocking=True)
        if not self.hist_used:
            self.hist_used = True
            self._capture_twins()

    def enable_controls(self) -> None:
        """The first request with logit_bias, min_tokens, stop_token_ids or min_p: from now on every sampling site
        runs the bias and ban pass (rows with nothing to do return at once) and the candidates read min_p; the graph
        twins that hold them are replayed."""
        if not self.ctl_used:
            self.ctl_used = True
            self._capture_twins()

    def set_controls(self, slot: int, bias: dict, ban_ids: list) -> None:
        """A sequence with logit_bias entries {global id: bias} and / or banned ids (min_tokens: EOS, stop_token_ids)
        takes `slot`: they become the slot's ctl_body row, with one pinned non-blocking copy ordered after every step
        already enqueued.  (The counts, ban_until and min_p travel in ctl_meta.)"""
        if len(bias) > ops.CTL_BIAS or len(ban_ids) > ops.CTL_BAN:
            raise ValueError(f"at most {ops.CTL_BIAS} logit_bias entries and {ops.CTL_BAN} banned ids per sequence")
        row = np.zeros(ops.CTL_BODY, dtype=np.int32)
        if bias:
            row[0:2 * len(bias):2] = list(bias.keys())
            row[1:2 * len(bias):2] = np.asarray(list(bias.values()), dtype=np.float32).view(np.int32)
        row[2 * ops.CTL_BIAS:2 * ops.CTL_BIAS + len(ban_ids)] = ban_ids
        row = torch.from_numpy(row)
        if self.device.type == "cuda":
            row = row.pin_memory()
        self.ctl_body[slot].copy_(row, non_blocking=True)
        self.enable_controls()

    # ------------------------------------------------------------------ guided decoding
    def set_guide_vocab(self, pieces, eos_id: int) -> None:
        """The text of every token id (tokenizer.pieces()) and EOS's id: what a guide constrains is the concatenation
        of piece(id), so the byte table is built from these (at the first guided request)."""
        self.guide_pieces, self.guide_eos = list(pieces), int(eos_id)

    def enable_guides(self) -> None:
        """The first guided request: allocate the token byte table (whole on every TP rank), the table pool and
        guide_meta; from now on every sampling site runs the mask pass before the candidates and the advance pass
        after the commit (rows without a guide return at once), in graph twins captured here."""
        if self.guide_used:
            return
        if self.guide_pieces is None:
            raise ValueError("guided decoding needs the vocabulary's pieces (ModelRunner.set_guide_vocab)")
        V = self.cfg.vocab_size
        pieces = (self.guide_pieces + [""] * V)[:V]
        never = {i for i in (0, self.guide_eos) if i >= 0}
        tb, tl = ops.guide_token_table(pieces, never=never)
        dev = self.device
        self.guide_host = (tb, tl)  # (host copies: the engine walks a re-admitted sequence's published tokens)
        self.tok_bytes, self.tok_len = tb.to(dev), tl.to(dev)
        self.guide_tab = torch.full((ops.GUIDE_POOL, ops.GUIDE_STATES, 256), -1, device=dev, dtype=torch.int16)
        self.guide_flags = torch.zeros(ops.GUIDE_POOL, ops.GUIDE_STATES, device=dev, dtype=torch.int32)
        self.guide_meta = torch.zeros(2 * self.max_batch, device=dev, dtype=torch.int32)
        self.guide_meta[:self.max_batch] = -1
        self.json_tab = torch.from_numpy(ops.json_table()[0].view(np.int16).copy()).to(dev)
        self.json_state = torch.zeros(4 * self.max_batch, device=dev, dtype=torch.int32)
        ops.guide_attach_json(self.guide_meta, self.json_tab, self.json_state)  # (they ride with guide_meta)
        self.guide_used = True
        self._capture_twins()

    def enable_wide_guides(self) -> None:
        """The first schema guide: allocate the wide pool (8 MiB, as large as the narrow one) and attach it to
        guide_meta.  Graphs captured with the guide passes hold the launch records of before, whose wide pointers are
        null, so they are dropped and the pass set in use is captured again, once; the pass set itself is the same."""
        if self.guide_tab_wide is not None:
            return
        self.enable_guides()
        dev = self.device
        self.guide_tab_wide = torch.full((ops.GUIDE_WIDE_POOL, ops.GUIDE_WIDE_STATES, 256), -1, device=dev,
                                         dtype=torch.int16)
        self.guide_flags_wide = torch.zeros(ops.GUIDE_WIDE_POOL, ops.GUIDE_WIDE_STATES, device=dev, dtype=torch.int32)
        ops.guide_attach_wide(self.guide_meta, self.guide_tab_wide, self.guide_flags_wide)
        for key, twins in self._twins.items():
            if key[3]:
                for d in twins:
                    d.clear()
        if self._captured_key[3]:  # capture() ran with the guides on: its graphs are stale too, twins replace them
            self._captured_key = (None, None, None, True)
        self._capture_twins()

    def upload_guide(self, entry: int, table: np.ndarray, accept: np.ndarray) -> None:
        """Pattern table uint16 [n, 256] (n <= 512) and its accepting flags become pool entry `entry`, stream-ordered
        after every step already enqueued; then the live pass marks its stuck states.  entry >= ops.GUIDE_POOL: a
        schema guide's table (n <= 4096) becomes wide entry entry - ops.GUIDE_POOL."""
        n = int(table.shape[0])
        if entry >= ops.GUIDE_POOL:
            if not (1 <= n <= ops.GUIDE_WIDE_STATES and table.shape[1] == 256 and
                    entry < ops.GUIDE_POOL + ops.GUIDE_WIDE_POOL):
                raise ValueError("wide guide table must be [1..4096, 256]")
            self.enable_wide_guides()
            tabs, flgs, e = self.guide_tab_wide, self.guide_flags_wide, entry - ops.GUIDE_POOL
        else:
            if not (1 <= n <= ops.GUIDE_STATES and table.shape[1] == 256 and 0 <= entry):
                raise ValueError("guide table must be [1..512, 256]")
            self.enable_guides()
            tabs, flgs, e = self.guide_tab, self.guide_flags, entry
        tab = torch.from_numpy(np.array(table, dtype=np.uint16).view(np.int16))
        flg = torch.from_numpy(np.ascontiguousarray(accept, dtype=np.int32) & 1)
        if self.device.type == "cuda":
            tab, flg = tab.pin_memory(), flg.pin_memory()
        tabs[e, :n].copy_(tab, non_blocking=True)
        flgs[e, :n].copy_(flg, non_blocking=True)
        ops.guide_live(self.tok_bytes, self.tok_len, self.guide_tab, self.guide_flags, self.guide_meta, entry, n,
                       self.guide_eos)

    def set_guide(self, slot: int, entry: int, state) -> None:
        """A sequence takes `slot`: its pool entry (-1: no guide) and the DFA state after the tokens it has already
        published, stream-ordered; from then on the advance pass owns the state.  JSON mode: entry = ops.JSON_ENTRY
        and state = the (lexical state, depth, stack) after those tokens, which goes to the slot's json_state words
        (zeroed for every other sequence)."""
        if not self.guide_used:
            return
        js = [0, 0, 0, 0]
        if entry == ops.JSON_ENTRY:
            js, state = ops.json_state_words(state), 0
        m = torch.tensor([entry, state] + js, dtype=torch.int32)
        if self.device.type == "cuda":
            m = m.pin_memory()
        self.guide_meta.view(2, -1)[:, slot].copy_(m[:2], non_blocking=True)
        self.json_state.view(4, -1)[:, slot].copy_(m[2:], non_blocking=True)

    def _guide_mask(self, logits, active, row_slot) -> None:
        ops.guide_mask(logits, active, self.tok_bytes, self.tok_len, self.guide_tab, self.guide_flags, self.guide_meta,
                       row_slot, self.w.vocab_offset, self.guide_eos)

    def _guide_advance(self, ids, active, row_slot) -> None:
        ops.guide_advance(ids, active, self.tok_bytes, self.tok_len, self.guide_tab, self.guide_flags, self.guide_meta,
                          row_slot, self.guide_eos)

    def _twin_key(self) -> tuple:
        """The pass set in use: (penalties, logprobs, the bias and ban pass / min_p, the guide passes), and a fifth
        component, True, once the LoRA body is in use.  It is absent before, not False: the tests of the earlier
        features pin the four-component values (tests/test_guided_cpu.py, test_guided_json_gpu.py, test_logprobs_gpu.py
        and their kin compare _twin_key() and index _twins with 4-tuples).  A further component must follow the same
        rule, appended after this one, and readers of the first four slice them (_slot_arrays)."""
        return (self.hist_used, self.lp_used, self.ctl_used, self.guide_used) + ((True,) if self.lora_used else ())

    def _capture_graphs(self, shapes, body) -> list:
        """Capture body(shape) into a new graph in the shared pool, largest shape first (the first graph ever
        captured hands its pool to the rest).  Returns [(shape, graph)] in capture order."""
        out = []
        for shape in sorted(shapes, reverse=True):
            g = torch.cuda.CUDAGraph()
            with _capture(g, pool=self.graph_pool):
                body(shape)
            if self.graph_pool is None:
                self.graph_pool = g.pool()
            out.append((shape, g))
        return out

    def _prefill_graph_body(self, tb: int) -> None:
        self._prefill_layers(tb, self.pf.views(tb))
        self._graph_sample()

    def _mixed_graph_body(self, shape: tuple) -> None:
        self._mixed_layers(*shape)
        self._graph_sample()

    def _capture_mixed_graphs(self, pairs, out: dict) -> None:
        """out[B] = [(C, graph), ...] by ascending C for the (B, C) in `pairs`."""
        for (B, C), g in self._capture_graphs(pairs, self._mixed_graph_body):
            out.setdefault(B, []).insert(0, (C, g))

    def _capture_twins(self) -> None:
        """The first request that needs a new pass set (_twin_key): every captured graph gets a twin with the passes
        in use (_sample), replayed from now on; until then the graphs captured at startup run, which hold no such
        launch and no extra collective (an early-exit launch per step measured +8 us on the 4.23 ms 64-stream step:
        profiles/r7/penalties.md).  The key names 15 pass sets besides the empty one (31 with a LoRA pool: each set
        with and without the LoRA body), each captured at most once
        between two capture() calls.  Stream capture executes nothing, so no decode state changes; the shapes and
        buffers are the ones the startup capture warmed, and the logprob all-gathers run once eagerly first.
        Deterministic across a TP group: every rank admits the same request in the same step."""
        key = self._twin_key()
        if key[:2] == (True, True) and self._lp_raw is None:
            self._lp_raw = torch.zeros(max(self.max_batch, PREFILL_GRAPH_SEQS), self.w.vocab_local,
                                       device=self.device, dtype=torch.float32)
        if key == self._captured_key or any(self._twins.get(key, ())) or \
                not (self.graphs or self.pf_graphs or self.mx_graphs):
            return
        dec, pfg, mxg = self._twins.setdefault(key, ({}, {}, {}))
        if self.lp_used and self.comm.size > 1:
            for bufs in (self._lp_bufs[max(self._lp_bufs)], self._lp_pf):
                self.comm.all_gather_into(bufs["rec_all"], bufs["rec"])
                self.comm.all_gather_into(bufs["chosen_all"], bufs["chosen"])
        t0 = time.perf_counter()
        dec.update(self._capture_graphs(self.graphs, self.decode_forward))
        pfg.update(self._capture_graphs(self.pf_graphs, self._prefill_graph_body))
        self._capture_mixed_graphs([(B, C) for B, lst in self.mx_graphs.items() for C, _ in lst], mxg)
        torch.cuda.synchronize(self.device)
        self.twin_capture_s = time.perf_counter() - t0
        if self.comm.rank == 0:
            what = " and ".join(n for n, on in zip(("the penalty pass", "the logprob passes",
                                                    "the bias and ban pass / min_p", "the guide passes",
                                                    "the LoRA layer body"), key) if on)
            print(f"[engine] first request with this combination: captured the graphs with {what} "
                  f"({self.twin_capture_s:.2f} s)", flush=True)

    def _graph_set(self):
        """(decode, prefill, mixed) graphs to replay: the twins that hold the passes in use (penalties, logprobs, the
        bias and ban pass / min_p)."""
        key = self._twin_key()
        if key == self._captured_key:
            return self.graphs, self.pf_graphs, self.mx_graphs
        return self._twins.get(key) or ({}, {}, {})

    def health_faults(self, words) -> list:
        """Descriptions of the nonzero health words in `words` (a host copy of self.health)."""
        return [HEALTH_WORDS[i] for i in range(min(len(HEALTH_WORDS), len(words))) if int(words[i]) != 0]

    def close(self) -> None:
        """Release the TP all-reduce's IPC mappings and buffer.  Collective over the TP group: the device is
        synchronised, then every rank passes a barrier, so no peer's kernel can still be reading this rank's buffer
        (the IPC kernels pull peer rows) when it is unmapped and freed."""
        if self.comm.fast_ar is not None:
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            try:
                self.comm.barrier()
            except Exception as e:  # noqa: BLE001 - a dead peer cannot be reading any more either
                print(f"[engine] TP rank {self.comm.rank}: barrier before the IPC teardown failed ({e})", flush=True)
            self.comm.fast_ar.close()
            self.comm.fast_ar = None

    def bucket_for(self, n_active_max_slot: int) -> int:
        for b in batch_buckets(self.max_batch):
            if b >= n_active_max_slot:
                return b
        return self.max_batch

    def _collectives_capturable(self) -> tuple:
        """TP>1 startup self-check: an all-reduce captured into a graph and replayed must produce the sum on
        every rank.  Decided by all ranks together (an eager MIN of the local verdicts), so either every rank
        captures its decode step or every rank runs it eagerly -- the collectives stay matched."""
        import torch.distributed as dist

        ok, why = True, ""
        if dist.get_backend(self.comm.group) == "gloo":
            ok, why = False, "gloo backend (host-staged collectives cannot be captured)"
        try:
            if not ok:
                raise StopIteration
            t = torch.ones(8, device=self.device, dtype=torch.float32)
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                self.comm.all_reduce(t)  # warm the communicator outside capture
            torch.cuda.current_stream(self.device).wait_stream(s)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with _capture(g):
                self.comm.all_reduce(t)
            t.fill_(1.0)
            g.replay()
            torch.cuda.synchronize(self.device)
            if not torch.all(t == float(self.comm.size)):
                ok, why = False, f"replayed all-reduce gave {t.tolist()}"
        except StopIteration:
            pass
        except Exception as e:  # noqa: BLE001 - the reason is logged, decode then runs eagerly
            ok, why = False, f"{type(e).__name__}: {e}"
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device)
        if dist.get_backend(self.comm.group) == "gloo":
            flag = flag.cpu()
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.comm.group)
        if ok and int(flag.item()) == 0:
            why = "another rank of the TP group cannot capture its collectives"
        return int(flag.item()) == 1, why

    def ipc_decode(self) -> bool:
        """TP > 1 with the IPC context up for every decode row: the decode step's collectives are the hand-written
        IPC all-reduce (both per layer) and candidate all-gather kernels only -- no RCCL call in the step."""
        ar = self.comm.fast_ar
        return self.comm.size > 1 and ar is not None and ar.rows >= self.max_batch

    def capture(self, buckets=None) -> None:
        """Capture the decode step of each batch bucket into its own graph (shared memory pool).  TP > 1: the decode
        graphs hold the IPC collective kernels when that context is up (ipc_decode), else the RCCL collectives after
        a capture self-check; the prefill / mixed graphs (their all-reduces are RCCL) only when RCCL captures.
        Neither: eager decode (reason logged)."""
        if not self.use_graphs:
            return
        self._captured_key = self._twin_key()
        for twins in self._twins.values():  # recorded against the previous capture's graphs and buffers
            for d in twins:
                d.clear()
        prefill_graphs = True
        if self.comm.size > 1:
            ipc = self.ipc_decode()
            rccl_ok, why = self._collectives_capturable()
            if not ipc and not rccl_ok:
                print(f"[engine] TP rank {self.comm.rank}: decode graphs disabled, collectives not capturable "
                      f"({why}); decoding eagerly", flush=True)
                self.use_graphs = False
                return
            prefill_graphs = rccl_ok
            if self.comm.rank == 0:
                print(f"[engine] TP={self.comm.size} decode graphs captured with "
                      f"{'the IPC all-reduce + all-gather kernels (no RCCL in the step)' if ipc else 'RCCL collectives'}"
                      f"; prefill graphs {'captured' if rccl_ok else 'off (' + why + ')'}", flush=True)
        buckets = buckets or batch_buckets(self.max_batch)
        # Warm up on a side stream (allocator + library init) before capture.
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        saved = self._snapshot_state()
        with torch.cuda.stream(s):
            for B in buckets:
                self.decode_forward(B)
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        self.graphs.update(self._capture_graphs(buckets, self.decode_forward))
        torch.cuda.synchronize(self.device)
        self._restore_state(saved)
        if prefill_graphs:
            self._capture_prefill(buckets)

    def _capture_prefill(self, decode_buckets) -> None:
        """One graph per prefill row bucket over static buffers (_PrefillStatic); the metadata of a batch is
        uploaded into them before the replay.  Captured with all-padding metadata (every row slot -1: no K/V
        write; every work item on the empty sequence)."""
        if os.environ.get("DSSE_PREFILL_GRAPHS", "1") == "0":
            return
        buckets = [t for t in PREFILL_GRAPH_BUCKETS if t <= self.max_prefill_tokens]
        if not buckets:
            return
        self.pf = _PrefillStatic(self, max(buckets))
        self.pf.upload_padding()
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for tb in buckets:
                self._prefill_graph_body(tb)  # padding metadata: no prompt finishes, nothing is committed
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        self.pf_graphs.update(self._capture_graphs(buckets, self._prefill_graph_body))
        torch.cuda.synchronize(self.device)
        if mixed_mode() != "0" and os.environ.get("DSSE_MIXED_GRAPHS", "1") != "0":
            self._capture_mixed(list(decode_buckets))

    def mixed_chunk(self, B: int) -> int:
        """The prompt rows of a mixed step before its cost is measured: DSSE_MIXED_CHUNK when set (then the only
        captured chunk size), else 256; whole 64-row flash-prefill tiles."""
        fixed = int(os.environ.get("DSSE_MIXED_CHUNK", "0"))
        return -(-fixed // PREFILL_TILE) * PREFILL_TILE if fixed > 0 else 256

    def mixed_chunks(self, B: int) -> list:
        """The chunk sizes C captured for decode bucket B (B + C rows fit the static prefill buffers)."""
        fixed = int(os.environ.get("DSSE_MIXED_CHUNK", "0"))
        tmax = self.pf.tmax if self.pf is not None else 0
        if fixed > 0:
            return [c for c in [self.mixed_chunk(B)] if B + c <= tmax]
        top = (MIXED_MAX_ROWS - B) // PREFILL_TILE * PREFILL_TILE
        sizes = sorted({c for c in MIXED_CHUNKS if c <= top} | ({top} if top >= MIXED_CHUNKS[0] else set()))
        return [c for c in sizes if B + c <= tmax]

    def _capture_mixed(self, decode_buckets) -> None:
        """One graph per (decode bucket B, chunk size C in mixed_chunks(B)) for the mixed step (ModelRunner.mixed;
        captured like the decode step: the decode state restored afterwards).  mx_graphs[B] = [(C, graph), ...]
        by ascending C."""
        pairs = [(B, C) for B in decode_buckets for C in self.mixed_chunks(B)]
        if not pairs:
            return
        saved = self._snapshot_state()
        self.pf.upload_padding()
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for pair in pairs:  # eager warm-up of every shape (kernel attributes, library state)
                self._mixed_graph_body(pair)
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        self._capture_mixed_graphs(pairs, self.mx_graphs)
        torch.cuda.synchronize(self.device)
        self._restore_state(saved)

    def mixed_graph_rows(self, B: int, T: int):
        """C of the captured mixed graph that a step of bucket B with T prompt rows replays (the smallest C >= T),
        or None (the step runs eagerly)."""
        return next((c for c, _ in self.mx_graphs.get(B, ()) if c >= T), None)

    def _snapshot_state(self):
        # hist_len: a warm-up or capture run over a penalised active slot appends to its history (the token written
        # past the restored length is never read)
        return [t.clone() for t in (self.ids, self.positions, self.ring, self.ring_counter, self.hist_len)]

    def _restore_state(self, saved):
        for t, s in zip((self.ids, self.positions, self.ring, self.ring_counter, self.hist_len), saved):
            t.copy_(s)

    def move_slots(self, src: list, dst: list) -> None:
        """Slot compaction: decode state (last token, position) of slot src[i] -> dst[i], gathered before it
        is scattered so swaps work; stream-ordered after every decode step already enqueued."""
        idx = torch.tensor([src, dst], dtype=torch.long)
        if self.device.type == "cuda":  # pinned + non_blocking: no host wait for the decode steps already queued
            idx = idx.pin_memory().to(self.device, non_blocking=True)
        si, di = idx[0], idx[1]
        for t, dim in self._slot_arrays():
            t.index_copy_(dim, di, t.index_select(dim, si))

    def _slot_arrays(self) -> list:
        """[(tensor, the dimension that indexes slots)]: the device state that travels with a sequence when its slot
        moves (the host-owned slot_meta / pen_meta are re-uploaded by the engine).  A feature's arrays travel once a
        request has used it; a new per-slot array needs one line here."""
        hist, lp, ctl, guide = self._twin_key()[:4]
        arrays = [(self.ids, 0), (self.positions, 0)]
        arrays += [(self.slot_adapter, 0)] if self.lora_used else []
        arrays += [(self.hist_state, 0)] if hist else []  # the token histories: length word + tokens
        arrays += [(self.lp_meta, 0)] if lp else []
        arrays += [(self.ctl_body, 0), (self.ctl_meta.view(4, -1), 1)] if ctl else []  # bias / ban records + columns
        arrays += [(self.guide_meta.view(2, -1), 1)] if guide else []  # the pool index and the device-owned DFA state
        arrays += [(self.json_state.view(4, -1), 1)] if guide else []  # JSON mode's lexical state, depth and stack
        return arrays

    def decode(self, B: int) -> None:
        g = self._graph_set()[0].get(B)
        if g is not None:
            g.replay()
        else:
            self.decode_forward(B)

    # ------------------------------------------------------------------ prefill
    def _proj(self, a, wt, out) -> None:
        """out = a·wᵀ in bf16 on the engine's tiled-layout GEMMs (every row count: no library GEMM)."""
        ops.gemm_out(a, wt, out)

    def _gate_up(self, x, L, h) -> None:
        """h = SiLU(x·W_gateᵀ)·(x·W_upᵀ) with the fused SiLU·mul epilogue (gate / up rows interleaved by 8)."""
        ops.gemm_silu(x, L.wgu_t, h)

    def _seq_sharded_norm(self, tmp, resid, norm_w, x) -> None:
        """TP prefill residual step in its sequence-sharded form: reduce-scatter the partial products over the rows
        (rank r gets the summed rows [r n, (r + 1) n)), add + RMSNorm those n = T / t rows only, all-gather the normed
        bf16 rows.  Same bytes on the wire as the all-reduce it replaces (a ring all-reduce IS reduce-scatter +
        all-gather), 1 / t of the norm work, and each rank's residual stream is authoritative for its own rows only
        (the next residual step adds into the same rows; nothing else reads resid)."""
        t, r = self.comm.size, self.comm.rank
        n = tmp.shape[0] // t
        own = slice(r * n, (r + 1) * n)
        # one reduce-scatter target per shape, reused: every use of it is ordered on one stream (the side stream in
        # the chunked path, the current one otherwise, and the two paths are ordered against each other by the
        # chunked path's events); no allocation on the host's per-chunk path
        key = (n, tmp.shape[1], tmp.dtype, tmp.device)
        cache = self.__dict__.setdefault("_rs_bufs", {})
        summed = cache.get(key)
        if summed is None:
            summed = cache[key] = torch.empty(n, tmp.shape[1], device=tmp.device, dtype=tmp.dtype)
        self.comm.reduce_scatter_rows(summed, tmp)
        ops.rmsnorm(resid[own], norm_w, x[own], self.cfg.rms_eps, delta=summed)
        self.comm.all_gather_rows(x, x[own])

    def _resid_async(self, tmp, resid, norm_w, x):
        """Residual step of one row chunk on the communication side stream, ordered after everything queued on the
        current stream: the sequence-sharded reduce-scatter -> add + RMSNorm of this rank's rows -> all-gather when
        the chunk's rows divide by the TP degree, else all-reduce -> replicated norm.  Returns the event the consumer
        of x waits for (None: done synchronously, CPU / gloo)."""
        sharded = tmp.shape[0] % self.comm.size == 0
        if not tmp.is_cuda:
            if sharded:
                self._seq_sharded_norm(tmp, resid, norm_w, x)
            else:
                self.comm.all_reduce(tmp)
                ops.rmsnorm(resid, norm_w, x, self.cfg.rms_eps, delta=tmp)
            return None
        main = torch.cuda.current_stream(self.device)
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(self.device)
            # a ring of event pairs, reused: every wait on an event is enqueued before the event is recorded again
            # (the ring outlasts a layer's 2 x chunks residual steps)
            self._side_evs = [(torch.cuda.Event(), torch.cuda.Event()) for _ in range(32)]
            self._side_ev_i = 0
        ready, done = self._side_evs[self._side_ev_i]
        self._side_ev_i = (self._side_ev_i + 1) % len(self._side_evs)
        ready.record(main)
        self._side.wait_event(ready)
        with torch.cuda.stream(self._side):
            if sharded:
                self._seq_sharded_norm(tmp, resid, norm_w, x)
            else:
                self.comm.all_reduce(tmp)
                ops.rmsnorm(resid, norm_w, x, self.cfg.rms_eps, delta=tmp)
        done.record(self._side)
        return done

    def _prefill_post_attention(self, T: int, attn, L, w_next, resid, x, h, tmp) -> None:
        """resid += all_reduce(attn·Woᵀ); x = norm(resid); resid += all_reduce(silu-mlp(x)); x = norm(resid)·w_next.

        TP: whenever the rows divide by the TP degree, each all-reduce + replicated norm is the sequence-sharded
        reduce-scatter -> norm on T / t rows -> all-gather (_seq_sharded_norm; VERDICT r5 missing 3): the same bytes
        on the wire as the all-reduce (a ring all-reduce is reduce-scatter + all-gather), 1 / t of the norm work.

        TP prefill of >= DSSE_TP_PREFILL_OVERLAP_MIN rows: these ops are row-independent, so they run in row chunks and
        every chunk's residual step (collectives + its 1 / t of the norm) is issued on a side stream the moment its
        GEMM is done -- the O steps of chunk i under the O GEMM of chunk i + 1 and the MLP of chunk i - 1, the down
        steps under the next chunks' MLP; only the last chunk's second step is exposed (1 / 2n of the layer's
        communication, n chunks).  Each rank's residual rows are then updated on the side stream only (nothing on the
        main stream reads resid).  Every rank issues the collectives in the same order.  TP = 1 or short prompts: the
        unchunked chain."""
        chunks = prefill_row_chunks(T, self.comm.size)
        if len(chunks) == 1:
            self._prefill_resid(attn, L.wo_t, resid, L.ffn_norm, x, tmp)
            self._gate_up(x, L, h)
            self._prefill_resid(h, L.wd_t, resid, w_next, x, tmp)
            return
        main = torch.cuda.current_stream(self.device) if tmp.is_cuda else None
        ev1 = []
        for a, b in chunks:
            self._proj(attn[a:b], L.wo_t, tmp[a:b])
            ev1.append(self._resid_async(tmp[a:b], resid[a:b], L.ffn_norm, x[a:b]))
        ev2 = []
        for (a, b), ev in zip(chunks, ev1):
            if ev is not None:
                main.wait_event(ev)
            self._gate_up(x[a:b], L, h[a:b])
            self._proj(h[a:b], L.wd_t, tmp[a:b])  # tmp rows [a, b) are free: their O step was waited for
            ev2.append(self._resid_async(tmp[a:b], resid[a:b], w_next, x[a:b]))
        for ev in ev2:
            if ev is not None:
                main.wait_event(ev)

    def _prefill_resid(self, a, wt, resid, norm_w, x, tmp) -> None:
        """resid += a·wᵀ, x = RMSNorm(resid).  Thousands of rows: the product goes out as a bf16 tile (row-contiguous
        stores) and the norm kernel adds it -- the fused fp32 read-modify-write epilogue measured +120 us per
        8192-row projection (profiles/r2/prefill_kernels_8k.md).  Up to PREFILL_SLAB_ROWS rows on the tiled kernels
        (split K) the norm reduces the fp32 split-K slabs itself, as in decode: no reduce launch, no bf16 round trip."""
        rows = a.shape[0]
        if self.comm.size == 1 and rows <= PREFILL_SLAB_ROWS and self.split_part.numel() >= 8 * rows * wt.shape[0]:
            ns = ops.gemm_resid_split(a, wt, resid, self.split_part)
            ops.rmsnorm(resid, norm_w, x, self.cfg.rms_eps, part=self.split_part, nsplit=ns)
            return
        self._proj(a, wt, tmp)
        if self.comm.size > 1 and rows % self.comm.size == 0:
            self._seq_sharded_norm(tmp, resid, norm_w, x)
            return
        self.comm.all_reduce(tmp)
        ops.rmsnorm(resid, norm_w, x, self.cfg.rms_eps, delta=tmp)

    def _prefill_meta(self, seqs: list, row0: int = 0, split: bool = False):
        """Packed metadata of prefill chunks whose rows start at `row0` of the activations (0 for a prefill-only
        batch, B for the prefill rows of a mixed step): host lists + device tensors (one pinned upload).  split: add
        the flash key-split plan when the grid is under-filled (flash_split_plan: d["fw"], d["fc"], d["fslots"])."""
        dev = self.device
        n = len(seqs)
        # vectorised per sequence (an 8k-token chunk was ~25k Python list appends on the TTFT path)
        ids_l, pos_l, slots_l, adp_l = [], [], [], []
        q_start, q_len, ctx_len, items = [], [], [], []
        bt = torch.zeros(n, self.max_blocks, dtype=torch.int32)
        row = 0
        for i, s in enumerate(seqs):
            m = len(s.tokens)
            q_start.append(row0 + row)
            p = s.start_pos + np.arange(m, dtype=np.int64)
            table = np.asarray(s.block_table, dtype=np.int64)
            ids_l.append(np.asarray(s.tokens, dtype=np.int64))
            pos_l.append(p)
            slots_l.append(table[p // PAGE] * PAGE + p % PAGE)
            adp_l.append(np.full(m, s.adapter, dtype=np.int64))
            q_len.append(m)
            ctx_len.append(s.start_pos + m)
            bt[i, : len(s.block_table)] = torch.from_numpy(table.astype(np.int32))
            # flash prefill: heaviest (most keys) 64-query tiles first, so the causal tail balances over the CUs
            tile = self.attn_tile
            items += [(-(s.start_pos + min(m, (t + 1) * tile)), i, t) for t in range(math.ceil(m / tile))]
            row += m
        items.sort()
        work_seq = [i for _, i, _ in items]
        work_tile = [t for _, _, t in items]
        T = row
        plan = None
        if split and not self.kv.is_fp8:
            plan = flash_split_plan([(i, t, -(-(-k) // PREFILL_TILE)) for k, i, t in items], self.w.nkv)
        fw, fc = (plan[0], plan[1]) if plan else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        empty = np.zeros(0, dtype=np.int64)
        meta = torch.from_numpy(np.concatenate(
            [np.concatenate(ids_l) if ids_l else empty, np.concatenate(pos_l) if pos_l else empty,
             np.concatenate(slots_l) if slots_l else empty,
             np.asarray(q_start + q_len + ctx_len + work_seq + work_tile, dtype=np.int64),
             fw.astype(np.int64), fc.astype(np.int64),
             np.concatenate(adp_l) if adp_l and self.lora_used else empty]).astype(np.int32))
        if dev.type == "cuda":
            meta = meta.pin_memory().to(dev, non_blocking=True)
            bt = bt.pin_memory().to(dev, non_blocking=True)
        d, o = {}, 0
        for name, k in (("ids", T), ("pos", T), ("slots", T), ("qs", n), ("ql", n), ("ctx", n),
                        ("ws", len(work_seq)), ("wt", len(work_seq)), ("fw", len(fw)), ("fc", len(fc)),
                        ("adp", T if self.lora_used else 0)):
            d[name], o = meta[o:o + k], o + k
        d["bt"] = bt
        d["fslots"] = plan[2] if plan else 0
        return T, q_start, q_len, ctx_len, d

    def _prefill_sample(self, seqs: list, x, q_start: list, q_len: list, ring_row: int) -> None:
        """Sequences whose last chunk this is sample their first token (rows q_start + q_len - 1 of `x`) into
        ids[slot] and ring[ring_row, slot]; positions[slot] is set on the device."""
        w, comm, dev = self.w, self.comm, self.device
        last = [i for i, s in enumerate(seqs) if s.last_chunk]
        if not last:
            return
        f32 = dict(device=dev, dtype=torch.float32)
        nL = len(last)
        # one pinned, non-blocking upload of the three index vectors: a pageable torch.tensor(..., device=dev) is a
        # synchronous copy that waits for every step already queued (the prefill graph and the pipelined decode
        # steps) -- 27-30 ms of host stall per prompt at ~120 streams (profiles/r3/serving_trace.md)
        idx = torch.tensor([q_start[i] + q_len[i] - 1 for i in last] + [seqs[i].slot for i in last] +
                           [seqs[i].start_pos + len(seqs[i].tokens) - 1 for i in last], dtype=torch.long)
        if dev.type == "cuda":
            idx = idx.pin_memory().to(dev, non_blocking=True)
        rows, slot_idx, last_pos = idx[:nL], idx[nL:2 * nL], idx[2 * nL:].to(torch.int32)
        xl = x.index_select(0, rows)
        logits = torch.empty(nL, w.vocab_local, **f32)
        ops.gemm_out(xl, w.lm_head_t, logits)
        new_ids = torch.zeros(nL, dtype=torch.int32, device=dev)
        nch = SAMPLE_CHUNKS if dev.type == "cuda" else 1
        slot_i32 = slot_idx.to(torch.int32) if any(self._twin_key()) else None
        # (eager passes: nothing is launched or allocated until a request has asked for its feature)
        self._sample(SampleSite(logits, None, slot_i32, self.temperature.index_select(0, slot_idx),
                                self.top_k.index_select(0, slot_idx), self.top_p.index_select(0, slot_idx),
                                self.seeds.index_select(0, slot_idx).contiguous(), last_pos,
                                torch.zeros(nL, nch, 2, **f32),
                                torch.zeros(comm.size, nL, nch, 2, **f32) if comm.size > 1 else None,
                                self._lp_eager_bufs(nL) if self.lp_used else None, new_ids,
                                dict(ring_row=ring_row), "eager"))
        self.ids.index_copy_(0, slot_idx, new_ids)
        self.ring[ring_row].index_copy_(0, slot_idx, new_ids)
        self.positions.index_copy_(0, slot_idx, last_pos + 1)

    def prefill(self, seqs: list, ring_row: int) -> None:
        """Run one packed prefill batch: a captured graph of the smallest row bucket that holds it (metadata
        uploaded into the static buffers first), else eagerly.  Sequences whose last chunk this is sample their
        first token into ids[slot] and ring[ring_row, slot] and get positions[slot] set on device."""
        if not seqs:
            return
        T = sum(len(s.tokens) for s in seqs)
        tb = next((t for t in sorted(self.pf_graphs) if t >= T), None) if len(seqs) <= PREFILL_GRAPH_SEQS else None
        if tb is not None:
            self.pf.upload(seqs, tb, ring_row=ring_row)
            self._graph_set()[1][tb].replay()  # first tokens sampled inside the graph (_graph_sample)
            return
        w, dev = self.w, self.device
        nh, nkv, F, H = w.nh, w.nkv, w.ffn, self.cfg.hidden_size
        T, q_start, q_len, ctx_len, d = self._prefill_meta(seqs, split=True)
        f32 = dict(device=dev, dtype=torch.float32)
        bf = dict(device=dev, dtype=torch.bfloat16)
        if d["fslots"]:  # partial slots of the flash key split: [slots][Hkv][G][64 queries] x (128 dims | (m, l))
            d.update(fpo=torch.empty(d["fslots"] * nh * PREFILL_TILE * 128, **f32),
                     fpm=torch.empty(d["fslots"] * nh * PREFILL_TILE * 2, **f32))
        d.update(resid=torch.empty(T, H, **f32), x=torch.empty(T, H, **bf), q=torch.empty(T, nh, 128, **bf),
                 attn=torch.empty(T, nh, 128, **bf), h=torch.empty(T, F, **bf), tmp=torch.empty(T, H, **bf),
                 qkv=torch.empty(T, (nh + 2 * nkv) * 128, **bf), part=math.ceil(max(ctx_len) / 32) * 32)
        if self.lora_used:
            d.update(gu=torch.empty(T, 2 * F, **bf))
        self._prefill_layers(T, d)
        self._prefill_sample(seqs, d["x"], q_start, q_len, ring_row)

    def _prefill_layers(self, T: int, d: dict) -> None:
        """Embedding + every layer over T packed prompt rows (buffers and metadata in `d`; graph-capturable)."""
        w, eps = self.w, self.cfg.rms_eps
        nh, nkv = w.nh, w.nkv
        resid, x, q, attn, h, tmp, qkv = (d[k] for k in ("resid", "x", "q", "attn", "h", "tmp", "qkv"))
        ops.rmsnorm(resid, w.layers[0].attn_norm, x, eps, embed=w.embed, ids=d["ids"])
        nl = len(w.layers)
        if self.lora_used:
            self._lora_layers(0, d, d["pos"], d["slots"], d["adp"], split=True)
            return
        # projections on the engine's tiled-layout GEMMs (gemm_pipe.hip / gemm_tiled.hip for T > 128 rows; gate_up with
        # its fused SiLU·mul epilogue): no library GEMM
        for li, L in enumerate(w.layers):
            # QKV out as a plain bf16 tile, then the vectorised RoPE + paged-KV-write kernel: the fused
            # per-element RoPE epilogue measured +200 us per 8192-row layer (profiles/r2/prefill_kernels_8k.md), and
            # at 512 rows (gemm_qkv_rope, one launch fewer) 9.21-9.37 vs 9.15-9.33 ms TTFT, alternating
            # (profiles/r6/ttft512_qkv_fused_ab_r6.log)
            self._proj(x, L.wqkv_t, qkv)
            ops.rope_kv_write(qkv, d["pos"], d["slots"], self.rope, q, self.kv.k[li], self.kv.v[li], nh, nkv,
                              *self._kv_scales(li))
            self._prefill_attention(li, q, attn, d, split=True)
            w_next = w.layers[li + 1].attn_norm if li + 1 < nl else w.final_norm
            self._prefill_post_attention(T, attn.view(T, nh * 128), L, w_next, resid, x, h, tmp)

    # ------------------------------------------------------------------ mixed prefill + decode
    def _graph_sample(self) -> None:
        """The first-token sampling of the prompts a captured prefill / mixed batch finishes, inside the graph
        (VERDICT r5 item 5): gather their last rows of the static x and their slots' sampling parameters
        (prefill_sample_gather), LM head, candidates (TP: all-gathered), pick, commit ids / ring row / positions
        (prefill_sample_commit) -- static shapes of PREFILL_GRAPH_SEQS rows, rows past the batch's count inactive.
        Replaces _prefill_sample's torch index kernels and per-call index upload on the graph paths."""
        pf, ns = self.pf, self.pf.ns
        meta, sm = pf.samp_meta(), pf.s_meta
        ops.prefill_sample_gather(pf.x, meta, self.slot_meta, pf.s_xl, sm)
        ops.gemm_out(pf.s_xl, self.w.lm_head_t, pf.s_logits)
        # gathered row i samples for slot meta[ns + i]: its bias / ban record, penalties, history, guide, logprobs
        self._sample(SampleSite(pf.s_logits, sm[:ns], meta[ns:2 * ns], sm[ns:2 * ns].view(torch.float32),
                                sm[2 * ns:3 * ns], sm[3 * ns:4 * ns].view(torch.float32),
                                sm[4 * ns:6 * ns].view(ns, 2), sm[6 * ns:7 * ns], pf.s_cand, pf.s_cand_all,
                                self._lp_pf, pf.s_new, dict(ring_row_dev=meta[3 * ns + 1:3 * ns + 2]), "graph"))

    def mixed(self, B: int, seqs: list, ring_row: int) -> None:
        """ONE forward over the decode slots [0, B) and the prefill chunks `seqs` (rows B .. B+T-1): every weight
        byte streams once for both, so prompt tokens absorbed while streams decode cost the in-flight streams a
        bigger GEMM (M = B + T rows) instead of a whole extra prefill pass (decode-priority
        chunked prefill).  The captured graph of bucket B with the smallest chunk size C >= the chunks' rows (metadata
        uploaded into the static prefill buffers first), else eagerly.  Decode rows: QKV as a bf16 tile ->
        vectorised RoPE + K/V write for all rows -> decode attention (partitioned flash-decoding) for the B decode
        rows and flash prefill for the chunk rows -> shared o / gate_up / down / norms -> the B decode rows sample
        and commit exactly as the captured decode step does (ids, ring row, positions), the chunks that finish a
        prompt sample their first token as prefill() does.  Same tokens as prefill() + decode() (greedy:
        tests/test_mixed_step.py)."""
        T = sum(len(s.tokens) for s in seqs)
        entry = next(((c, g) for c, g in self._graph_set()[2].get(B, ()) if c >= T), None)
        if entry is not None and len(seqs) <= PREFILL_GRAPH_SEQS:
            t0 = time.perf_counter()
            self.pf.upload(seqs, entry[0], row0=B, ring_row=ring_row)
            t1 = time.perf_counter()
            entry[1].replay()  # the finishing prompts' first tokens are sampled inside (_graph_sample)
            t2 = time.perf_counter()
            if self.host_trace is not None:  # host seconds: metadata upload, graph launch, (in-graph sampling: 0)
                self.host_trace.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
            return
        w, dev = self.w, self.device
        nh, nkv, F, H = w.nh, w.nkv, w.ffn, self.cfg.hidden_size
        T, q_start, q_len, ctx_len, d = self._prefill_meta(seqs, row0=B)
        M = B + T
        f32 = dict(device=dev, dtype=torch.float32)
        bf = dict(device=dev, dtype=torch.bfloat16)
        d.update(resid=torch.empty(M, H, **f32), x=torch.empty(M, H, **bf), q=torch.empty(M, nh, 128, **bf),
                 attn=torch.empty(M, nh, 128, **bf), h=torch.empty(M, F, **bf), tmp=torch.empty(M, H, **bf),
                 qkv=torch.empty(M, (nh + 2 * nkv) * 128, **bf), part=math.ceil(max(ctx_len) / 32) * 32,
                 mx_ids=torch.empty(M, dtype=torch.int32, device=dev),
                 mx_pos=torch.empty(M, dtype=torch.int32, device=dev),
                 mx_slots=torch.empty(M, dtype=torch.int32, device=dev))
        if self.lora_used:
            d.update(gu=torch.empty(M, 2 * F, **bf), mx_adp=torch.empty(M, dtype=torch.int32, device=dev))
        self._mixed_body(B, T, d)
        self._prefill_sample(seqs, d["x"], q_start, q_len, ring_row)

    def _mixed_layers(self, B: int, C: int) -> None:
        """The graph body of a mixed step: bucket B decode rows + C static prompt rows (_PrefillStatic)."""
        d = self.pf.views(C)
        M = B + C
        for k in ("resid", "x", "q", "attn", "h", "tmp", "qkv") + (("gu",) if self.lora_used else ()):
            d[k] = getattr(self.pf, k)[:M]
        d.update(mx_ids=self.pf.mx_ids[:M], mx_pos=self.pf.mx_pos[:M], mx_slots=self.pf.mx_slots[:M])
        if self.lora_used:
            d.update(mx_adp=self.pf.mx_adp[:M])
        self._mixed_body(B, C, d)

    def _mixed_body(self, B: int, T: int, d: dict) -> None:
        """Decode prep, the forward over B + T rows, the decode rows' sampling and the ring advance (graph-capturable
        when `d` holds static buffers)."""
        w, cfg = self.w, self.cfg
        nh, nkv = w.nh, w.nkv
        eps = cfg.rms_eps
        r = slice(0, B)
        M = B + T
        ops.decode_prep(self.active[r], self.positions[r], self.block_tables[r], self.slots[r], self.ctx_len[r],
                        self.q_len[r], self.kv.num_blocks)
        ids, pos, slots = d["mx_ids"], d["mx_pos"], d["mx_slots"]
        ids[:B].copy_(self.ids[r])
        ids[B:].copy_(d["ids"][:T])
        pos[:B].copy_(self.positions[r])
        pos[B:].copy_(d["pos"][:T])
        slots[:B].copy_(self.slots[r])
        slots[B:].copy_(d["slots"][:T])
        resid, x, q, attn, h, tmp, qkv = (d[k] for k in ("resid", "x", "q", "attn", "h", "tmp", "qkv"))
        ops.rmsnorm(resid, w.layers[0].attn_norm, x, eps, embed=w.embed, ids=ids)
        dpart, dnparts = decode_partitioning(B, nkv, self.max_model_len)
        nl = len(w.layers)
        if self.lora_used:  # decode rows: their slots' adapters; prompt rows: the uploaded per-row adapters
            ra = d["mx_adp"]
            ra[:B].copy_(self.slot_adapter[r])
            ra[B:].copy_(d["adp"][:T])
            self._lora_layers(B, d, pos, slots, ra)
        else:
            for li, L in enumerate(w.layers):
                kc, vc = self.kv.k[li], self.kv.v[li]
                self._proj(x, L.wqkv_t, qkv)
                ops.rope_kv_write(qkv, pos, slots, self.rope, q, kc, vc, nh, nkv, *self._kv_scales(li))
                ops.paged_attention(0, q[r], kc, vc, self.block_tables[r], self.q_start[r], self.q_len[r],
                                    self.ctx_len[r], self.work_seq[r], self.work_tile[r], attn[r], self.part_o,
                                    self.part_ml, dpart, dnparts, *self._kv_scales(li))
                self._prefill_attention(li, q, attn, d)
                self._resid_proj(attn.view(M, nh * 128), L.wo_t, resid, L.ffn_norm, x, tmp)
                self._gate_up(x, L, h)
                w_next = w.layers[li + 1].attn_norm if li + 1 < nl else w.final_norm
                self._resid_proj(h, L.wd_t, resid, w_next, x, tmp)
        ops.gemm_out(x[r], w.lm_head_t, self.logits[r])
        self._sample_commit(B)
        ops.ring_advance(self.ring_counter)


class _PrefillStatic:
    """Static buffers of the captured prefill graphs (sized for the largest bucket Tmax; a bucket's graph uses
    the first tb rows) and their metadata upload: one int32 image [ids | pos | slots | q_start | q_len | ctx_len |
    work_seq | work_tile | block tables] filled on the host (two pinned buffers, alternating; an event guards
    reuse) and copied with one non-blocking H2D before the replay.  Padding: rows >= T have slot -1 (no K/V
    write) and token 0; sequence index NS is the empty sequence (q_len 0) that padded work items point at."""

    def __init__(self, runner: ModelRunner, tmax: int):
        # no back-reference to the runner: a runner <-> buffers cycle kept captured graphs alive until a garbage
        # collection, which could then run inside ANOTHER runner's capture and free a graph pool mid-capture (abort)
        self.tmax = tmax
        w, cfg, dev = runner.w, runner.cfg, runner.device
        nh, nkv, F, H = w.nh, w.nkv, w.ffn, cfg.hidden_size
        self.ns = PREFILL_GRAPH_SEQS
        self.tile = runner.attn_tile  # query tokens per prompt-attention work item (64; fp8 cache: 64 / G)
        self.nw = tmax // self.tile + self.ns  # work items: sum of ceil(q_len / tile) <= T / tile + seqs
        self.mb = runner.max_blocks
        self.lora = runner.lora is not None  # then the image carries the rows' adapter slots ("adp")
        n1 = self.ns + 1
        self.off = {}
        o = 0
        for name, k in (("ids", tmax), ("pos", tmax), ("slots", tmax), ("qs", n1), ("ql", n1), ("ctx", n1),
                        ("ws", self.nw), ("wt", self.nw), ("bt", n1 * self.mb), ("samp", 3 * self.ns + 2),
                        ("adp", tmax if self.lora else 0)):
            self.off[name] = (o, k)
            o += k
        self.words = o
        self.dev_meta = torch.zeros(o, dtype=torch.int32, device=dev)
        pin = dev.type == "cuda"
        self.host = [torch.zeros(o, dtype=torch.int32).pin_memory() if pin else torch.zeros(o, dtype=torch.int32)
                     for _ in range(2)]
        self.events = [None, None]
        self.flip = 0
        f32 = dict(device=dev, dtype=torch.float32)
        bf = dict(device=dev, dtype=torch.bfloat16)
        self.resid = torch.zeros(tmax, H, **f32)
        self.x = torch.zeros(tmax, H, **bf)
        self.q = torch.zeros(tmax, nh, 128, **bf)
        self.attn = torch.zeros(tmax, nh, 128, **bf)
        self.h = torch.zeros(tmax, F, **bf)
        self.tmp = torch.zeros(tmax, H, **bf)
        self.qkv = torch.zeros(tmax, (nh + 2 * nkv) * 128, **bf)
        self.part = math.ceil(runner.max_model_len / 32) * 32
        # mixed steps: ids / positions / slots of the B decode rows followed by the chunk rows
        i32 = dict(device=dev, dtype=torch.int32)
        self.mx_ids, self.mx_pos, self.mx_slots = (torch.zeros(tmax, **i32) for _ in range(3))
        if self.lora:  # the LoRA body's gate / up tile and the mixed step's per-row adapters
            self.gu = torch.zeros(tmax, 2 * F, **bf)
            self.mx_adp = torch.full((tmax,), -1, **i32)
        # first-token sampling inside the graph (ModelRunner._graph_sample): the finishing prompts' last rows, their
        # sampling parameters, logits, candidates and picks, ns rows each
        ns, V = self.ns, w.vocab_local
        nch = SAMPLE_CHUNKS if dev.type == "cuda" else 1
        self.s_xl = torch.zeros(ns, H, **bf)
        self.s_meta = torch.zeros(7 * ns, **i32)
        self.s_logits = torch.zeros(ns, V, **f32)
        self.s_cand = torch.zeros(ns, nch, 2, **f32)
        self.s_cand_all = torch.zeros(runner.comm.size, ns, nch, 2, **f32)
        self.s_new = torch.zeros(ns, **i32)

    def _meta(self, name):
        o, k = self.off[name]
        return self.dev_meta[o:o + k]

    def samp_meta(self):
        """[rows | slots | last_pos (ns each) | n | ring_row] of the prompts the uploaded batch finishes."""
        return self._meta("samp")

    def views(self, tb: int) -> dict:
        nwb = tb // self.tile + self.ns
        d = {"ids": self._meta("ids")[:tb], "pos": self._meta("pos")[:tb], "slots": self._meta("slots")[:tb],
             "qs": self._meta("qs"), "ql": self._meta("ql"), "ctx": self._meta("ctx"),
             "ws": self._meta("ws")[:nwb], "wt": self._meta("wt")[:nwb],
             "bt": self._meta("bt").view(self.ns + 1, self.mb), "part": self.part}
        if self.lora:
            d.update(adp=self._meta("adp")[:tb], gu=self.gu[:tb])
        d.update(resid=self.resid[:tb], x=self.x[:tb], q=self.q[:tb], attn=self.attn[:tb], h=self.h[:tb],
                 tmp=self.tmp[:tb], qkv=self.qkv[:tb])
        return d

    def _fill(self, buf: torch.Tensor, seqs: list, tb: int, row0: int = 0, ring_row: int = 0):
        a = buf.numpy()
        a[:] = 0
        o = self.off
        sm = a[o["samp"][0]:o["samp"][0] + o["samp"][1]]
        ns, row = self.ns, row0
        n = 0
        for s in seqs:
            row += len(s.tokens)
            if s.last_chunk:  # the chunk's last row samples the prompt's first token (as _prefill_sample)
                sm[n], sm[ns + n], sm[2 * ns + n] = row - 1, s.slot, s.start_pos + len(s.tokens) - 1
                n += 1
        sm[3 * ns], sm[3 * ns + 1] = n, ring_row
        ids, pos, slots = (a[o[k][0]:o[k][0] + o[k][1]] for k in ("ids", "pos", "slots"))
        qs, ql, ctx = (a[o[k][0]:o[k][0] + o[k][1]] for k in ("qs", "ql", "ctx"))
        ws, wt = (a[o[k][0]:o[k][0] + o[k][1]] for k in ("ws", "wt"))
        bt = a[o["bt"][0]:o["bt"][0] + o["bt"][1]].reshape(self.ns + 1, self.mb)
        slots[:] = -1
        adp = a[o["adp"][0]:o["adp"][0] + o["adp"][1]]
        adp[:] = -1
        q_start, q_len, items = [], [], []
        row = 0
        for i, s in enumerate(seqs):
            n = len(s.tokens)
            q_start.append(row0 + row)
            q_len.append(n)
            p = s.start_pos + np.arange(n)
            ids[row:row + n] = s.tokens
            pos[row:row + n] = p
            table = np.asarray(s.block_table, dtype=np.int64)
            slots[row:row + n] = table[p // PAGE] * PAGE + p % PAGE
            if self.lora:
                adp[row:row + n] = s.adapter
            bt[i, :len(s.block_table)] = s.block_table
            qs[i], ql[i], ctx[i] = row0 + row, n, s.start_pos + n
            # flash prefill: heaviest (most keys) 64-query tiles first (as _prefill_meta)
            items += [(-(s.start_pos + min(n, (t + 1) * self.tile)), i, t)
                      for t in range(math.ceil(n / self.tile))]
            row += n
        items.sort()
        ws[:] = self.ns  # padded items -> the empty sequence
        for k, (_key, i, t) in enumerate(items):
            ws[k], wt[k] = i, t
        return q_start, q_len

    def upload(self, seqs: list, tb: int, row0: int = 0, ring_row: int = 0):
        """Metadata of `seqs` into the static buffers (stream-ordered before the replay that follows); the rows of
        the chunks start at `row0` of the activations (a mixed step: after the B decode rows); the prompts finishing
        in this batch commit their first token to ring row `ring_row` inside the graph."""
        k = self.flip
        self.flip ^= 1
        if self.events[k] is not None:
            self.events[k].synchronize()  # that pinned buffer's previous copy has been consumed
        q_start, q_len = self._fill(self.host[k], seqs, tb, row0, ring_row)
        self.dev_meta.copy_(self.host[k], non_blocking=True)
        if self.dev_meta.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
            self.events[k] = ev
        return q_start, q_len

    def upload_padding(self):
        self.upload([], self.tmax)


# Device staging records of the host KV tier (KVOffload): what one engine step can spill plus restore.  64 pages are
# 256 MiB of HBM for the full model in bf16 (128 MiB in fp8) and 2048 tokens of prefix per admission; pages evicted
# beyond the free records in one step are dropped, and a host-tier hit longer than them is cut to what fits (the rest
# of that prompt is prefilled as if it had missed).
OFFLOAD_RING_PAGES = 64


class KVOffload:
    """Device side of the prefix cache's host tier: moves whole KV pages between the paged cache and a HostPageStore
    through a ring of contiguous staging records on the device (ops.kv_pages_gather / kv_pages_scatter), with the
    PCIe copies on a side stream behind events, as engine._Drain does for tokens.  The ops run eagerly on the compute
    stream between graph replays; nothing here is captured.

    Ordering rules (the engine holds (a) and the first half of (d), this class the rest):
      (a) the gather of block b is enqueued before any kernel that writes b for its new owner: the engine drains the
          allocator's spill list right after the allocations of a step, before the step (or a restore) is enqueued;
      (b) a host slot is ``filling``, invisible to lookup, until its D2H event has completed (poll -> store.commit);
      (c) a staging record is not reused before its copy is done: records return to the free set only in poll(),
          once the event recorded behind their last use (a spill's D2H, a restore's scatter) has completed;
      (d) H2D happens before the scatter (the compute stream waits for the copy's event), and the scatter before the
          first step that reads the block (same stream, enqueued at admission, before the prompt's chunks);
      (e) a host slot in ``reading`` is not recycled before its H2D event has completed: it is released in poll()
          behind the restore's scatter event, which the H2D precedes.
    Events are only ever polled (``query``): no call here waits on the device."""

    def __init__(self, runner: ModelRunner, store, ring_pages: int | None = None):
        kv = runner.kv
        self.r, self.store = runner, store
        self.R = int(ring_pages or OFFLOAD_RING_PAGES)
        self.bytes_per_block = KVCache.bytes_per_block(kv.num_layers, kv.nkv, kv.dtype)
        if self.R < 1:
            raise ValueError("the host KV tier needs at least one staging record")
        if store.bytes_per_block != self.bytes_per_block:
            raise ValueError(f"host store records are {store.bytes_per_block} bytes, a KV page is {self.bytes_per_block}")
        self.cuda = runner.device.type == "cuda"
        self.staging = torch.zeros(self.R, self.bytes_per_block // kv.dtype.itemsize, dtype=kv.dtype,
                                   device=runner.device)
        self._busy = [False] * self.R
        self._ops: list = []  # in flight: (kind, first record, count, host slots, event | None)
        # block lists, one pinned row per possible first record: a row is rewritten only once its record is free again
        self._idx = torch.zeros(self.R, self.R, dtype=torch.int32)
        if self.cuda:
            self._idx = self._idx.pin_memory()
            self.stream = torch.cuda.Stream(runner.device)

    def free_records(self) -> int:
        return self._busy.count(False)

    def _runs(self, n: int) -> list:
        """Free records for n pages as contiguous runs [(first, count)] (a launch's records are one slice)."""
        runs, i = [], 0
        while n > 0 and i < self.R:
            if self._busy[i]:
                i += 1
                continue
            j = i
            while j < self.R and not self._busy[j] and j - i < n:
                self._busy[j] = True
                j += 1
            runs.append((i, j - i))
            n -= j - i
            i = j
        assert n == 0, "more pages than free staging records (the caller asks free_records() first)"
        return runs

    def _rows(self, first: int, blocks: list):
        row = self._idx[first, :len(blocks)]
        row.copy_(torch.tensor(blocks, dtype=torch.int32))
        return row

    def spill(self, pairs: list) -> None:
        """pairs = [(block, host slot)]: copy the blocks' pages into the (``filling``) host slots.  Enqueued now, on
        the compute stream, so the pages are read before their new owners' kernels write them (rule a)."""
        kv, at = self.r.kv, 0
        for first, m in self._runs(len(pairs)):
            part = pairs[at:at + m]
            at += m
            rec = self.staging[first:first + m]
            ops.kv_pages_gather(kv.k, kv.v, self._rows(first, [b for b, _ in part]), rec)
            ev = None
            if self.cuda:
                done = torch.cuda.Event()
                done.record()
                self.stream.wait_event(done)
                with torch.cuda.stream(self.stream):
                    for j, (_, slot) in enumerate(part):
                        self.store.buf[slot].copy_(rec[j].view(torch.uint8), non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
            else:
                for j, (_, slot) in enumerate(part):
                    self.store.buf[slot].copy_(rec[j].view(torch.uint8))
            self._ops.append(("spill", first, m, [s for _, s in part], ev))

    def restore(self, pairs: list) -> None:
        """pairs = [(host slot, block)]: copy the (``reading``) host slots into the blocks, which the caller has just
        allocated.  H2D on the side stream into free records, then one scatter per run on the compute stream behind
        the copy's event (rule d)."""
        kv, at = self.r.kv, 0
        for first, m in self._runs(len(pairs)):
            part = pairs[at:at + m]
            at += m
            rec = self.staging[first:first + m]
            if self.cuda:
                with torch.cuda.stream(self.stream):
                    for j, (slot, _) in enumerate(part):
                        rec[j].view(torch.uint8).copy_(self.store.buf[slot], non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(self.stream)
                torch.cuda.current_stream(self.r.device).wait_event(copied)
            else:
                for j, (slot, _) in enumerate(part):
                    rec[j].view(torch.uint8).copy_(self.store.buf[slot])
            ops.kv_pages_scatter(rec, self._rows(first, [b for _, b in part]), kv.k, kv.v)
            ev = None
            if self.cuda:
                ev = torch.cuda.Event()
                ev.record()
            self._ops.append(("restore", first, m, [s for s, _ in part], ev))

    def poll(self) -> None:
        """Retire the operations whose events have completed (never waits): a spill's host slots become visible, a
        restore's host slots recyclable, and their staging records free.  On the CPU every copy is done when issued;
        it is still retired here, at the next poll, so both devices walk through the same states."""
        if not self._ops:
            return
        live = []
        for op in self._ops:
            kind, first, m, slots, ev = op
            if ev is not None and not ev.query():
                live.append(op)
                continue
            for s in slots:
                (self.store.commit if kind == "spill" else self.store.release)(s)
            for i in range(first, first + m):
                self._busy[i] = False
        self._ops = live
