"""Continuous-batching LLM engine: scheduler + pipelined decode + asynchronous token-ring drain.

Replaces vLLM's scheduler/worker loop behind the reference's proxy (reference
``src/llm-stream-proxy/main.go:148-228`` consumed vLLM's OpenAI SSE stream; here the engine emits
token events directly).  One engine per GPU (DP replica) or per TP group.

Per ``step()`` (host, a few hundred microseconds of Python):

1. give every sequence about to decode the KV page its next position lands in (pages are allocated
   lazily, one at a time; when the pool runs dry the newest sequence -- paused ones first -- is
   *preempted*: its pages are freed and it is requeued at the head of the queue to be re-prefilled
   from prompt + the tokens it already published, so its stream resumes where it stopped);
2. admit waiting requests into free decode slots (lowest index first so live slots stay packed and
   the smallest captured batch bucket applies), allocating KV pages for the prompt only; when the
   queue is empty, *compact*: decoding sequences above the bucket their count needs move down into
   free slots or swap with paused ones (ids / positions move on the device), so holes left by
   finished or paused streams do not keep the step on a bigger captured graph;
3. upload slot metadata that changed (block tables, sampling params, active mask) with pinned,
   non-blocking copies on the compute stream;
4. absorb prompt work.  Default (``DSSE_MIXED=1``): the prompt chunk rides in the decode step itself
   (``ModelRunner.mixed``: one forward over the B decode rows + the chunk's rows, every weight byte streamed once,
   replayed from the graph of (B, chunk size)).  The chunk starts at 256 rows and grows to the largest captured
   size whose measured step cost stays within ``DSSE_PREFILL_ITL_RATIO`` x the bucket's decode step
   (``PassCost``); a longer backlog is split into even shares, shortest prompt first; a prompt queued for more
   than 40 steps gets the full PREFILL_BUDGET (the TTFT guard; counted in steps, so TP ranks agree).
   ``DSSE_MIXED=0``: separate prefill passes within a per-step token budget (decode-priority chunked prefill);
5. replay the captured decode graph of the batch bucket (sampled ids stay on the device and feed the
   next step; token ring row ``t`` receives every token produced in step ``t``);
6. start the device->host copy of ring row ``t`` on a side stream, then process the drained rows of
   earlier steps: sequence numbers, EOS / max_tokens stops, TTFT / ITL accounting.

Flow control: a sequence whose subscribers all fall behind is *paused* (``set_paused``): its slot stays
in the batch with ``active = 0``, so the decode graph neither advances its position nor writes its KV,
and it resumes exactly where it stopped.  Everyone else keeps decoding.  The reference instead dropped
frames once a subscriber's 100-slot channel filled (``src/sse-adapter/sse_handler.go:147-156``).

The GPU is never idle waiting for the host: step ``t+1`` is enqueued before row ``t`` is read.  Stops
discovered late (EOS) cost at most one wasted decode step for that slot, and the slot's pages are
only reused by work enqueued after the stop, so stream order makes reuse safe.
"""
from __future__ import annotations

import hashlib
import itertools
import math
import os
import time
from collections import deque
from dataclasses import dataclass, field

import numpy as np
import torch

from .. import ops
from .kv_cache import PAGE, BlockAllocator, HostPageStore, KVCache, blocks_needed, page_hashes
from .model_runner import PREFILL_GRAPH_SEQS, RING_SIZE, KVOffload, ModelRunner, PrefillSeq, batch_buckets, mixed_mode


@dataclass
class SamplingParams:
    temperature: float = 1.0   # vLLM OpenAI-server defaults (the proxy sets none: main.go:155-163)
    top_p: float = 1.0
    top_k: int = 0
    max_tokens: int = 256
    seed: int | None = None
    ignore_eos: bool = False
    # vLLM's token-history penalties, applied in this order before temperature / top-k / top-p (and under greedy);
    # c[v] = occurrences of v among the generated tokens (sampler.hip sample_penalty_kernel)
    presence_penalty: float = 0.0    # x[v] -= p where c[v] > 0
    frequency_penalty: float = 0.0   # x[v] -= f * c[v]
    repetition_penalty: float = 1.0  # v in the prompt or generated: x[v] = x[v] / r if x[v] > 0 else x[v] * r

    # raw logprobs (x - logsumexp(x) of the logits before penalties / temperature / filters) of every sampled token
    # and of the top N tokens: -1 = off, 0..20 = N (sampler.hip logprob_stats_kernel / logprob_finish_kernel)
    logprobs: int = -1
    # vLLM's remaining controls.  logit_bias {token id: bias in [-100, 100]} (<= 300 entries) is added to the fp32
    # logits after the raw logprob statistics and before the penalties, also under greedy; while fewer than
    # min_tokens tokens are generated, EOS (unless ignore_eos) and every stop_token_ids entry get -inf
    # (sampler.hip sample_bias_ban_kernel); a sampled stop_token_ids entry (<= 16) ends the stream as EOS does,
    # ignore_eos or not; min_p in [0, 1] keeps, after temperature, the tokens with p_i >= min_p max_j p_j
    # (sample_filtered_kernel).  `stop` strings are matched on the decoded text by the serving loop
    # (serving/stop_strings.py): the engine itself only carries them.
    logit_bias: dict | None = None
    min_tokens: int = 0
    stop_token_ids: tuple = ()
    min_p: float = 0.0
    stop: tuple = ()
    # guided decoding: one canonical pattern (guided_regex as given, guided_choice lowered to an alternation of escaped
    # literals) whose full match the delivered text must be, or a prefix of one when max_tokens ends the stream first.
    # The pattern is compiled to a byte-level DFA (csrc/runtime/guide.cpp) that lives on the device: a mask pass before
    # the candidates keeps the tokens whose bytes the DFA accepts from the slot's state, an advance pass after the
    # commit moves the state (sampler.hip sample_guide_mask_kernel / sample_guide_advance_kernel)
    guide: str | None = None
    # the guide is a JSON Schema lowered to a pattern (guided_json / response_format json_schema; guide.h
    # schema_pattern): it compiles under the wide caps (compile_wide) and lives in the device's wide pool
    guide_schema: bool = False
    # JSON mode (response_format {"type": "json_object"}): the delivered text is a JSON object of the language J
    # (docs/kernels.md, "Sampler"), or a viable prefix of one when max_tokens ends the stream first.  A pushdown walk
    # inside the same two guide passes; it takes no pattern pool entry.  Mutually exclusive with `guide`.
    json_object: bool = False
    # the name of a loaded LoRA adapter (engine/lora.py; None: the base model).  The adapter travels with the
    # params: through preemption and re-prefill, and to the siblings of an n > 1 request
    lora: str | None = None

    def penalised(self) -> bool:
        return self.presence_penalty != 0.0 or self.frequency_penalty != 0.0 or self.repetition_penalty != 1.0

    def controlled(self) -> bool:
        """Needs the device's bias and ban pass or min_p (stop_token_ids alone are the host's business)."""
        return bool(self.logit_bias) or self.min_tokens > 0 or self.min_p > 0.0


FINISH_CODES = {"": 0, "stop": 1, "length": 2, "abort": 3}  # runtime FinishReason (csrc/runtime/json.h)


@dataclass(slots=True)
class TokenEvent:
    conversation_id: str
    token_id: int
    sequence: int
    done: bool
    text: str = ""          # overrides the vocabulary piece ("[DONE]", "[ERROR]")
    timestamp_ns: int = 0
    finish: str = ""        # terminal events: "stop" (EOS), "length" (max_tokens / context), "abort"
    prompt_tokens: int = -1  # terminal events: prompt length (OpenAI usage)
    logprob: float | None = None  # streams that asked for logprobs: the sampled token's raw logprob ...
    top: list | None = None       # ... and the top N as [(token id, logprob)], logit descending, ties by ascending id
    cached_tokens: int = -1  # terminal events, prefix caching on: prompt tokens whose KV was reused (else -1)


@dataclass
class Sequence:
    rid: int
    conversation_id: str
    prompt: list
    params: SamplingParams
    arrival_ns: int = 0
    slot: int = -1
    blocks: list = field(default_factory=list)
    prefilled: int = 0
    state: str = "waiting"      # waiting | prefill | decode | finished | preempted (replaced by a requeued copy)
    decode_enqueued: int = 0    # decode steps enqueued (tokens 2..n)
    produced: int = 0           # tokens drained and published
    first_token_ns: int = 0
    last_token_ns: int = 0
    queued_ns: int = 0          # add_request (after the serving loop polled and tokenized it)
    admit_ns: int = 0           # first prompt chunk planned into a step (0: prefilled by the separate-pass path)
    aborted: bool = False
    stop_after_enqueue: bool = False
    paused: bool = False        # flow control: held out of the decode batch (KV and position kept)
    paused_at: float = 0.0
    orig_len: int = 0           # prompt length as submitted (after a preemption `prompt` also holds out_ids)
    out_ids: list = field(default_factory=list)  # tokens published so far (re-prefilled after a preemption)
    base: int = 0               # tokens published before the latest (re-)admission
    enq_step: int = 0           # engine step at which it was queued (the mixed-step TTFT boost counts steps)
    guide_entry: int = -1       # pool entry of its pattern while it holds a slot (a reference; -1: none)
    stamped: bool = False       # admit_ns was taken (its first chunk was planned; a cache hit never has prefilled == 0)
    cached_tokens: int = -1     # prefix caching: prompt tokens served from resident pages at its FIRST admission
    hashes: list = field(default_factory=list)  # prefix caching: chain hashes of its full pages, prompt pages first
    published: int = 0          # prefix caching: its leading pages that are shared or were offered to the index
    parent: object = None       # parallel sampling: choice 0 of its request, whose prompt pages it forks at its first
                                # admission (choices 1..n-1 only; cleared once used or once it took the plain path)


class EngineFault(RuntimeError):
    """A device-side health word was set (a bounded in-kernel wait timed out: persistent decode kernel, TP peer):
    the step's tokens cannot be trusted.  The serving loop ends every live stream with [ERROR], drops readiness
    and exits non-zero (no re-exec of a process that has touched the GPU)."""


class _Drain:
    def __init__(self, runner: ModelRunner):
        self.r = runner
        self.cuda = runner.device.type == "cuda"
        B = runner.max_batch
        # the runner's health words ride along with every ring row (same side stream, same event)
        nh = runner.health.numel()
        self.health = torch.zeros(RING_SIZE, nh, dtype=torch.int32)
        self.pf_health = torch.zeros(RING_SIZE, nh, dtype=torch.int32)
        if self.cuda:
            self.health, self.pf_health = self.health.pin_memory(), self.pf_health.pin_memory()
        if self.cuda:
            self.host = torch.zeros(RING_SIZE, B, dtype=torch.int32).pin_memory()
            self.stream = torch.cuda.Stream(runner.device)
            self.events = [torch.cuda.Event() for _ in range(RING_SIZE)]
        else:
            self.host = torch.zeros(RING_SIZE, B, dtype=torch.int32)

        # first tokens of prompts whose prefill pass precedes a decode step in the same engine step: drained as
        # soon as the prefill pass is done, not after the decode step (their own buffers and events per ring row)
        self.pf_host = torch.zeros_like(self.host)
        if self.cuda:
            self.pf_host = self.pf_host.pin_memory()
            self.pf_events = [torch.cuda.Event() for _ in range(RING_SIZE)]
        self.lp_host = self.pf_lp_host = None  # host rows of the runner's lp_ring, once logprobs are in use

    def _lp_hosts(self):
        if self.lp_host is None:
            shape = (RING_SIZE,) + tuple(self.r.lp_ring.shape[1:])
            self.lp_host, self.pf_lp_host = torch.zeros(shape), torch.zeros(shape)
            if self.cuda:
                self.lp_host, self.pf_lp_host = self.lp_host.pin_memory(), self.pf_lp_host.pin_memory()
        return self.lp_host, self.pf_lp_host

    def issue(self, row: int, width: int, first: bool = False):
        host = self.pf_host if first else self.host
        health = self.pf_health if first else self.health
        # the logprob rows ride along (same stream, same event, the drained width) once a request has asked for them
        lp = self._lp_hosts()[1 if first else 0] if self.r.lp_used else None
        if not self.cuda:
            host[row, :width] = self.r.ring[row, :width]
            health[row].copy_(self.r.health)
            if lp is not None:
                lp[row, :width] = self.r.lp_ring[row, :width]
            return
        self.stream.wait_stream(torch.cuda.current_stream(self.r.device))
        with torch.cuda.stream(self.stream):
            host[row, :width].copy_(self.r.ring[row, :width], non_blocking=True)
            health[row].copy_(self.r.health, non_blocking=True)
            if lp is not None:
                lp[row, :width].copy_(self.r.lp_ring[row, :width], non_blocking=True)
            (self.pf_events if first else self.events)[row].record(self.stream)

    def logprobs(self, row: int, first: bool = False):
        """Host copy of lp_ring[row] (after wait()), or None while no request has asked for logprobs."""
        return None if self.lp_host is None else (self.pf_lp_host if first else self.lp_host)[row]

    def faults(self, row: int, first: bool = False) -> list:
        """Health faults recorded with ring row `row` (after wait())."""
        return self.r.health_faults((self.pf_health if first else self.health)[row].tolist())

    def ready(self, row: int, first: bool = False) -> bool:
        return (not self.cuda) or (self.pf_events if first else self.events)[row].query()

    def wait(self, row: int, first: bool = False):
        if self.cuda:
            (self.pf_events if first else self.events)[row].synchronize()
        return (self.pf_host if first else self.host)[row]


class PassCost:
    """Measured GPU cost of the engine's step kinds, for sizing prompt work from measured cost instead of a fixed
    size.  Timing events bracket every decode step, every mixed step and every
    separate prefill pass; they are read once they have completed (no host wait).  Decode: an EMA of the step per
    bucket.  Prefill passes: an exponentially weighted least-squares line ms = a + b * tokens.  Mixed steps: the
    same kind of line for the extra over the bucket's decode step, extra = a + b * C (C = the replayed graph's
    prompt rows).

    budget(B): the largest multiple of 64 prompt tokens whose separate pass costs at most (ratio - 1) x step(B);
    mixed_chunk(B, sizes): the largest captured chunk size whose mixed step costs at most ratio x step(B).  Either
    way a stream's token gap stays within `ratio` x the occupied bucket's steady step.  Until the costs are measured
    both return None (the caller keeps its configured size)."""

    def __init__(self, ratio: float, decay: float = 0.9):
        self.ratio = ratio
        self.decay = decay
        self.step_ms: dict = {}
        self._fit = [0.0] * 5  # weighted sums: w, w t, w t^2, w y, w t y
        self._mfit = [0.0] * 5  # the same for mixed steps' extra cost over the decode step
        self._mixed_seen: set = set()
        self._pending: deque = deque()

    def record(self, kind: str, key: int):
        """(start event, end-record callable) around one enqueued pass; kind 'decode' (key = bucket) or 'prefill'
        (key = tokens)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        return lambda: (e1.record(), self._pending.append((kind, key, e0, e1)))

    def observe(self, kind: str, key, ms: float) -> None:
        if kind == "decode":
            old = self.step_ms.get(key)
            self.step_ms[key] = ms if old is None else 0.8 * old + 0.2 * ms
            return
        if kind == "mixed":  # key = (B, C)
            B, C = key
            step = self.step_ms.get(B)
            if step is None:
                return
            self._mixed_seen.add(C)
            f, t, ms = self._mfit, float(C), ms - step
        else:
            f, t = self._fit, float(key)
        d = self.decay
        for i, v in enumerate((1.0, t, t * t, ms, t * ms)):
            f[i] = d * f[i] + v

    def poll(self) -> None:
        while self._pending and self._pending[0][3].query():
            kind, key, e0, e1 = self._pending.popleft()
            self.observe(kind, key, e0.elapsed_time(e1))

    def line(self, fit=None):
        """(a, b) of the pass-cost line (`fit`: the mixed-step sums), or None before two sizes were seen."""
        w, st, stt, sy, sty = self._fit if fit is None else fit
        den = w * stt - st * st
        if w <= 0 or den <= 1e-6 * max(1.0, w * stt):
            return None
        b = (w * sty - st * sy) / den
        a = (sy - b * st) / w
        return (max(0.0, a), b) if b > 0 else None

    def mixed_line(self):
        """(a, b) of extra = a + b * C for mixed steps: the fitted line once two chunk sizes were seen; with one
        size, the proportional line through its mean (b = extra / C, a = 0: it over-predicts larger chunks, so the
        first choice is conservative and the next size measured turns on the fit); None before any."""
        if len(self._mixed_seen) >= 2:
            line = self.line(self._mfit)
            if line is not None:
                return line
        w, st, _, sy, _ = self._mfit
        return (0.0, sy / st) if w > 0 and st > 0 and sy > 0 else None

    def mixed_ms(self, B: int, C: int):
        """Predicted GPU time of a mixed step (bucket B, C prompt rows), or None before it can be predicted."""
        step = self.step_ms.get(B)
        line = self.mixed_line()
        return None if step is None or line is None else step + line[0] + line[1] * C

    def mixed_chunk(self, B: int, sizes: list):
        """The largest of `sizes` whose predicted mixed step stays within ratio x step(B) (the smallest when none
        does), or None until the decode step of bucket B and a mixed step were measured."""
        step = self.step_ms.get(B)
        line = self.mixed_line()
        if step is None or line is None or not sizes:
            return None
        a, b = line
        fit = [c for c in sizes if a + b * c <= (self.ratio - 1.0) * step]
        return max(fit) if fit else min(sizes)

    def budget(self, B: int, cap: int):
        step = self.step_ms.get(B)
        line = self.line()
        if step is None or line is None:
            return None
        a, b = line
        room = (self.ratio - 1.0) * step - a
        return max(64, min(cap, int(room / b) // 64 * 64)) if room > 0 else 64


class LLMEngine:
    def __init__(self, runner: ModelRunner, eos_id: int = 2, prefill_budget: int = 512,
                 idle_prefill_budget: int | None = None, default_params: SamplingParams | None = None,
                 pipeline_depth: int | None = None, max_pause_s: float = 30.0, deterministic: bool | None = None,
                 prefix_cache: bool = False, kv_offload_pages: int = 0, offload_ring_pages: int | None = None):
        self.r = runner
        self.eos_id = eos_id
        # automatic prefix caching (off by default): full KV pages are indexed by the hash of the token prefix they
        # end, and a prompt that starts with resident pages shares them and prefills only the rest (_admit).  Every
        # rank of a TP group runs this same allocator on the same inputs in the same order (the plan carries requests,
        # not pages; drained steps are consumed by count), so block tables and start positions agree without
        # travelling.
        self.prefix_cache = bool(prefix_cache)
        # host tier behind the prefix cache (off by default): kv_offload_pages > 0 keeps that many evicted pages in
        # (pinned) host memory; a later prompt whose hash chain runs past the resident pages continues into them, and
        # the hit pages are copied back into fresh HBM pages at admission (_admit, _drain_spills; the device side and
        # the ordering rules are model_runner.KVOffload's).  Not under TP: the followers' fixed-size step plan has no
        # room for spill and restore lists.
        self.offload = None
        store = None
        if kv_offload_pages:
            if kv_offload_pages < 0:
                raise ValueError("kv_offload_pages must be >= 0")
            if not self.prefix_cache:
                raise ValueError("the host KV tier (kv_offload_pages) needs prefix_cache=True: it holds evicted "
                                 "prefix-cache pages")
            if runner.comm.size > 1:
                raise ValueError("the host KV tier (kv_offload_pages) is not supported with tensor parallelism")
            kv = runner.kv
            store = HostPageStore(kv_offload_pages, KVCache.bytes_per_block(kv.num_layers, kv.nkv, kv.dtype),
                                  pinned=runner.device.type == "cuda")
            self.offload = KVOffload(runner, store, offload_ring_pages)
        self.alloc = BlockAllocator(runner.kv.num_blocks, prefix_cache=self.prefix_cache, host_store=store)
        # the runner's KV cache element type ("bf16" | "fp8_e4m3": ModelRunner(kv_cache_dtype=)); nothing the engine
        # schedules -- pages, block tables, slots, prefix hashes -- depends on it
        self.kv_cache_dtype = "fp8_e4m3" if runner.kv.is_fp8 else "bf16"
        # the runner's weight quantisation ("none" | "fp8_e4m3" | "mxfp4": ModelRunner(quantization=)); it changes which GEMM
        # kernels a decode bucket runs and nothing the engine schedules
        self.quantization = getattr(runner, "quantization", "none")
        self.shared_write_violations = 0  # a step's write slots named a shared page (checked when debug_shared_writes)
        self.debug_shared_writes = runner.device.type != "cuda" or os.environ.get("DSSE_DEBUG_PREFIX_CACHE", "0") == "1"
        self.prefill_budget = prefill_budget
        self.idle_prefill_budget = idle_prefill_budget or runner.max_prefill_tokens
        self.default_params = default_params or SamplingParams()
        # decode steps kept enqueued ahead of the host's token processing.  1 (one step queued while the host
        # consumes the previous one): a new prompt's prefill pass waits behind one decode step instead of two --
        # TTFT p50 31.7 -> 23.8 ms at 13 req/s, 39.3 -> 30.4 ms at 40 req/s, same ITL, steady 64-stream step
        # within 0.5 % (profiles/r3/pipeline_depth.md).  A depth that changes with the load was measured too: each
        # change is one doubled token gap for every stream (64-stream p99 ITL 7.2 ms), so it stays fixed.
        self.depth = pipeline_depth if pipeline_depth is not None else int(os.environ.get("DSSE_PIPELINE_DEPTH", "1"))
        self.max_pause_s = max_pause_s
        # TP groups (serving/tp.py): every rank must consume drained steps at the same engine step, so the
        # count decides (len(inflight) - depth), never whether this rank's copy event has completed yet
        self.deterministic = runner.comm.size > 1 if deterministic is None else deterministic
        self.waiting: deque = deque()
        self.slots: list = [None] * runner.max_batch
        self.by_conv: dict = {}
        self.step_no = 0
        # (step, ring_row, producers [(slot, seq)], t_enqueue, first): first = an early first-token drain entry
        # (Drain.issue(first=True)); the pipeline depth counts the other entries only
        self.inflight: deque = deque()
        self.drain = _Drain(runner)
        self._rid = itertools.count(1)
        self._dirty_slots: set = set()
        self._pen_live = False  # the device's penalty block holds a non-neutral slot (then _upload rewrites it)
        self._lp_live = False   # the device's lp_meta holds a slot that is on (likewise)
        self._ctl_live = False  # the device's ctl_meta holds a non-neutral slot (likewise)
        self._lora_live = False  # the device's slot_adapter holds a slot with an adapter (likewise)
        self.lora_requests: dict = {}  # adapter name -> sequences queued under it
        # guided decoding: compiled patterns (pattern -> (table uint16 [n, 256], accept uint8 [n])), and the device
        # pool's entries: pattern -> index, references by live sequences per index, and the resident pattern per index
        # (an entry without references stays resident until another pattern needs it)
        # Entries are entry words: [0, GUIDE_POOL) the narrow pool, [GUIDE_POOL, GUIDE_POOL + GUIDE_WIDE_POOL) the
        # wide pool of schema guides; a key is (pattern, schema-derived), and each kind waits for its own pool.
        self._guide_dfa: dict = {}
        self._guide_idx: dict = {}
        self._guide_refs = [0] * (ops.GUIDE_POOL + ops.GUIDE_WIDE_POOL)
        self._guide_pat = [None] * (ops.GUIDE_POOL + ops.GUIDE_WIDE_POOL)
        self._guide_lru = 0
        self._guide_used_at = [0] * (ops.GUIDE_POOL + ops.GUIDE_WIDE_POOL)
        self.ring_head = int(runner.ring_counter.item()) if runner.device.type == "cuda" else int(runner.ring_counter[0])
        self.stats = {"steps": 0, "decode_steps": 0, "mixed_steps": 0, "prefill_tokens": 0, "tokens": 0,
                      "last_step_s": 0.0, "pauses": 0, "preemptions": 0, "compactions": 0, "host_s": 0.0, "wait_s": 0.0,
                      # prefix caching: prompt tokens looked up / served from resident pages (admissions), pages evicted
                      "prefix_queries": 0, "prefix_hit_tokens": 0, "prefix_evictions": 0,
                      # parallel sampling (add_request n > 1): requests / prompt tokens the siblings did not prefill
                      # again / partial last prompt pages copied for them (kv_pages_copy)
                      "fork_requests": 0, "fork_shared_tokens": 0, "fork_tail_copies": 0}
        if self.offload is not None:
            # host tier: pages copied out at eviction / evicted with their content already there / evicted with no
            # free staging record or host slot (content lost) / copied back at admission, and the tokens those held
            self.stats.update(offload_spilled_pages=0, offload_spill_skipped=0, offload_dropped_pages=0,
                              offload_restored_pages=0, offload_hit_tokens=0)
        # admission keeps this many pages free for running sequences to grow into (vLLM's 1% watermark)
        self.watermark = max(1, runner.kv.num_blocks // 100)
        self._bt_new: list = []  # (sequence, page index, block) appended since the last upload
        # parallel sampling: conversation id of choice 0 -> ids of its request's choices that are still alive (abort
        # by that id ends them all), and each of those ids -> choice 0's; (src, dst) tail-page copies of the siblings
        # admitted in this step, launched together before the step's passes
        self._groups: dict = {}
        self._group_of: dict = {}
        self._fork_pairs: list = []
        self._pending: list = []  # events raised between steps (aborts of queued requests), returned by the next
        self.on_ttft = None
        self.ttft_trace = None  # a list: (arrival, queued, admitted, first token) ns per sequence
        self.enq_trace = None   # a list: (step kind, host seconds from step start to enqueue)
        self.on_itl = None
        # on_flush(events): called with the events gathered so far before the step blocks on a drain that is not
        # ready yet (the serving loop publishes them at once: early-drained first tokens do not wait for the
        # decode step behind them); what is left is returned by step() as usual
        self.on_flush = None
        # mixed prefill + decode steps (ModelRunner.mixed); DSSE_MIXED=0 runs chunks as separate prefill passes
        self.mixed = mixed_mode() != "0" and hasattr(runner, "mixed")
        self.mixed_min_tokens = 64
        # a prompt queued longer than this many steps gets the full prefill budget (TTFT guard, counted in steps:
        # identical on every TP rank)
        self.mixed_boost_steps = 40
        # two or more prompts pending: mixed steps take the largest captured chunk (_mixed_budget)
        self.mixed_queue_boost = True
        # adaptive prefill budget (separate passes while streams decode): DSSE_PREFILL_ITL_RATIO = r > 1 sizes each
        # pass so that a token gap spanning a decode step and a pass stays <= r x the occupied bucket's step
        # (PassCost), up to prefill_budget; a prompt that has waited DSSE_PREFILL_BOOST_STEPS steps gets the full
        # budget (TTFT guard).  Unset / 0: the fixed prefill_budget.
        # Mixed steps (the default): the ratio is on by default (1.85: a mixed step within ~2x the bucket's step,
        # VERDICT r4 item 2's ITL p99 target, with margin) and sizes each step's prompt chunk.
        # TP groups (deterministic): no PassCost -- its fit comes from this rank's own GPU event timings, so ranks
        # would pick different chunk sizes and replay graphs of different row counts (mismatched collectives)
        ratio = float(os.environ.get("DSSE_PREFILL_ITL_RATIO", "1.85" if self.mixed else "0") or 0)
        self.cost = PassCost(ratio) if ratio > 1.0 and runner.device.type == "cuda" and not self.deterministic \
            else None
        self.boost_steps = int(os.environ.get("DSSE_PREFILL_BOOST_STEPS", "8"))
        self._jit = None  # (host time the newest step started, its expected ms): jit_delay

    def jit_delay(self, margin_s: float = 0.0015) -> float:
        """Seconds the host can still wait before enqueueing the next step without leaving the GPU idle: the
        in-flight step's expected end (PassCost) minus `margin_s` for the host's own step work.  A prompt that
        arrives meanwhile then rides in the very next step instead of the one after the step already queued
        (pipeline depth 1 alone makes a new prompt wait ~1.5 steps).  0 without a cost estimate, in
        deterministic (TP) mode, or with no step in flight."""
        if self.deterministic or self.cost is None or not self.inflight or self._jit is None:
            return 0.0
        start, est_ms = self._jit
        if est_ms is None:
            return 0.0
        return max(0.0, start + est_ms / 1e3 - margin_s - time.perf_counter())

    # ------------------------------------------------------------------ requests
    def next_rid(self) -> int:
        return next(self._rid)

    def add_request(self, conversation_id: str, prompt: list, params: SamplingParams | None = None,
                    arrival_ns: int | None = None, rid: int | None = None, n: int = 1, choice_ids=None):
        """Queue a request.  `rid` (a TP leader's request id, replayed on its followers) seeds the sampling RNG
        when the params carry no seed, so it must be the same on every rank of a TP group.

        n > 1 (parallel sampling) queues n sequences, the choices of one request, and returns them as a list: choice 0
        under `conversation_id`, choice i under f"{conversation_id}-c{i}" (or `choice_ids[i]`), with consecutive rids
        rid .. rid + n - 1.  With a seed, choice i samples with seed + i (the draw is per (seed, position): equal seeds
        would give equal siblings), so choice 0 is the same request with n = 1; without one the rid-derived seeds
        differ already.  Choices 1.. wait behind choice 0 and fork its prompt's KV pages once its whole prompt is
        enqueued (_admit); when choice 0 is gone by then they prefill on their own."""
        n = int(n)
        if n != 1:
            if not 1 <= n <= self.r.max_batch:
                raise ValueError(f"n must be in [1, {self.r.max_batch}] (the engine's max_batch), got {n}")
            ids = [conversation_id] + [f"{conversation_id}-c{i}" for i in range(1, n)] if choice_ids is None \
                else list(choice_ids)
            if len(ids) != n or ids[0] != conversation_id or len(set(ids)) != n:
                raise ValueError("choice_ids must be n distinct ids, the first the conversation id")
            p = params or self.default_params
            first = rid if rid is not None else next(self._rid)
            seqs = []
            for i, cid in enumerate(ids):
                pi = p if p.seed is None or i == 0 else SamplingParams(**{**p.__dict__, "seed": int(p.seed) + i})
                r_i = first + i if rid is not None or i == 0 else next(self._rid)
                s = self.add_request(cid, prompt, pi, arrival_ns=arrival_ns, rid=r_i)
                if i:
                    s.parent = seqs[0]
                seqs.append(s)
            assert [s.rid for s in seqs] == list(range(first, first + n)), "parallel sampling: rids must be consecutive"
            self._groups[conversation_id] = set(ids)
            for cid in ids:
                self._group_of[cid] = conversation_id
            self.stats["fork_requests"] += 1
            return seqs
        p = params or self.default_params
        if p.json_object:
            if p.guide is not None:
                raise ValueError("json_object cannot be combined with a guide (guided_regex / guided_choice)")
            if self.r.guide_pieces is None:
                raise ValueError("JSON mode needs the vocabulary's pieces (ModelRunner.set_guide_vocab)")
        if p.lora is not None:
            if self.r.lora is None:
                raise ValueError(f"LoRA adapter {p.lora!r} requested, but the engine was started without LoRA")
            self.r.lora.slot_of(p.lora)  # (LoraError, a ValueError, for a name that is not loaded: nothing is queued)
            self.lora_requests[p.lora] = self.lora_requests.get(p.lora, 0) + 1
        if p.guide_schema and p.guide is None:
            raise ValueError("guide_schema needs the lowered pattern in guide")
        if p.guide is not None:
            self._guide_compiled(p.guide, p.guide_schema)  # (ValueError for a pattern the compiler rejects: nothing is queued)
            if self.r.guide_pieces is None:
                raise ValueError("guided decoding needs the vocabulary's pieces (ModelRunner.set_guide_vocab)")
        max_prompt = self.r.max_model_len - 1
        if len(prompt) > max_prompt:
            prompt = prompt[-max_prompt:]  # keep the tail (most recent context)
        s = Sequence(rid=next(self._rid) if rid is None else rid, conversation_id=conversation_id,
                     prompt=list(prompt), params=p, arrival_ns=arrival_ns or time.time_ns(), orig_len=len(prompt),
                     enq_step=self.step_no, queued_ns=time.time_ns())
        self.waiting.append(s)
        self.by_conv[conversation_id] = s
        return s

    def abort(self, conversation_id: str, choices: bool = True) -> bool:
        """Abort a conversation.  The id of a request with n > 1 (its choice 0's) ends every choice still alive;
        choices=False ends that one sequence only (a stop string matched in choice 0's text)."""
        group = self._groups.get(conversation_id) if choices else None
        if group is not None:
            hit = [self._abort_one(c) for c in sorted(group)]
            return any(hit)
        return self._abort_one(conversation_id)

    def _abort_one(self, conversation_id: str) -> bool:
        s = self.by_conv.get(conversation_id)
        if s is None or s.state == "finished":
            return False
        s.aborted = True
        if s.state == "waiting":  # never admitted, or preempted: its terminal event goes out with the next step
            self.waiting.remove(s)
            self._finish(s, self._pending, reason="abort")
        return True

    def set_paused(self, conversation_id: str, paused: bool) -> bool:
        """Flow control: hold (or release) one sequence's decode.  Returns whether anything changed."""
        s = self.by_conv.get(conversation_id)
        if s is None or s.state == "finished" or s.paused == paused:
            return False
        s.paused = paused
        s.paused_at = time.monotonic()
        if paused:
            self.stats["pauses"] += 1
        else:
            s.last_token_ns = 0  # the held interval is not an inter-token latency sample
        if s.slot >= 0:
            self._dirty_slots.add(s.slot)
        return True

    def expired_pauses(self, now: float | None = None) -> list:
        """Conversations paused for longer than ``max_pause_s`` (the caller resumes them)."""
        now = time.monotonic() if now is None else now
        return [c for c, s in self.by_conv.items() if s.paused and now - s.paused_at > self.max_pause_s]

    def has_work(self) -> bool:
        return bool(self.waiting or self.inflight or self._pending) or any(s is not None for s in self.slots)

    def runnable(self) -> bool:
        """Work a step would make progress on (paused decode sequences are not)."""
        if self.waiting or self.inflight or self._pending:
            return True
        return any(s is not None and (not s.paused or s.aborted or s.state != "decode") for s in self.slots)

    def num_running(self) -> int:
        return sum(1 for s in self.slots if s is not None)

    # ------------------------------------------------------------------ helpers
    def _upload(self):
        """Push host-side slot metadata changes to the device (pinned, non-blocking)."""
        if self._bt_new:
            self._upload_pages()
        if not self._dirty_slots:
            return
        r = self.r
        Bm = r.max_batch
        # built in numpy (one element write ~0.1 us; on torch CPU tensors ~1 us each: with ~130 live slots the
        # element loop cost ~1 ms of host time per step that changed a slot, on the JIT enqueue's critical path)
        meta = np.zeros(6 * Bm, dtype=np.int32)  # ModelRunner.slot_meta's layout
        active, topk = meta[:Bm], meta[2 * Bm:3 * Bm]
        temp, topp = meta[Bm:2 * Bm].view(np.float32), meta[3 * Bm:4 * Bm].view(np.float32)
        seeds = meta[4 * Bm:].reshape(Bm, 2)
        topp[:] = 1.0
        for i, s in enumerate(self.slots):
            if s is None:
                continue
            if s.state == "decode" and not s.aborted and not s.stop_after_enqueue and not s.paused:
                active[i] = 1
            p = s.params
            temp[i] = p.temperature
            topk[i] = p.top_k
            topp[i] = p.top_p
            sd = p.seed if p.seed is not None else (s.rid * 2654435761) & 0x7FFFFFFF
            seeds[i, 0] = sd & 0x7FFFFFFF
            seeds[i, 1] = (sd >> 31) & 0x7FFFFFFF
        # the penalty block [presence | frequency | repetition | n_prompt] (ModelRunner.pen_meta): built and sent only
        # while a penalised sequence holds a slot, and once more after the last one left (back to neutral).  The
        # token histories and their lengths are device-owned (ModelRunner.set_history at admission): not touched here
        pen = None
        live = [(i, s) for i, s in enumerate(self.slots) if s is not None and s.params.penalised()]
        if live or self._pen_live:
            pen = np.zeros(4 * Bm, dtype=np.int32)
            pf = pen[:3 * Bm].view(np.float32)
            pf[2 * Bm:] = 1.0
            for i, s in live:
                p = s.params
                pf[i], pf[Bm + i], pf[2 * Bm + i] = p.presence_penalty, p.frequency_penalty, p.repetition_penalty
                pen[3 * Bm + i] = s.orig_len
            self._pen_live = bool(live)
        # lp_meta (-1 = off, else N): likewise only while a sequence with logprobs holds a slot, and once after
        lpm = None
        live = [(i, s) for i, s in enumerate(self.slots) if s is not None and s.params.logprobs >= 0]
        if live or self._lp_live:
            lpm = np.full(Bm, -1, dtype=np.int32)
            for i, s in live:
                lpm[i] = min(int(s.params.logprobs), 20)
            self._lp_live = bool(live)
        # ctl_meta [bias entries | banned ids | ban-until position | min_p]: likewise (the entries and ids themselves
        # were uploaded at admission: ModelRunner.set_controls).  ban_until = orig_len + min_tokens does not change
        # over a preemption and re-prefill.
        ctl = None
        live = [(i, s) for i, s in enumerate(self.slots) if s is not None and s.params.controlled()]
        if live or self._ctl_live:
            ctl = np.zeros(4 * Bm, dtype=np.int32)
            for i, s in live:
                p = s.params
                bans = self._ban_ids(p)
                ctl[i] = len(self._bias(p))
                ctl[Bm + i] = len(bans)
                ctl[2 * Bm + i] = s.orig_len + p.min_tokens if bans else 0
                ctl[3 * Bm:].view(np.float32)[i] = min(max(float(p.min_p), 0.0), 1.0)
            self._ctl_live = bool(live)
        # slot_adapter (-1 = the base model, else the pool slot): likewise, from the first sequence with an adapter
        adp = None
        live = [(i, s) for i, s in enumerate(self.slots) if s is not None and s.params.lora is not None]
        if live or self._lora_live:
            adp = np.full(Bm, -1, dtype=np.int32)
            for i, s in live:
                adp[i] = self._adapter_slot(s)
            self._lora_live = bool(live)
        bt_rows = {}
        for i in self._dirty_slots:
            s = self.slots[i]
            if s is not None and s.blocks:
                row = np.zeros(r.max_blocks, dtype=np.int32)
                row[: len(s.blocks)] = s.blocks
                bt_rows[i] = torch.from_numpy(row)
        cuda = r.device.type == "cuda"

        def put(dst, src):
            if cuda:
                dst.copy_(src.pin_memory(), non_blocking=True)
            else:
                dst.copy_(src)

        put(r.slot_meta, torch.from_numpy(meta))
        if pen is not None:
            put(r.pen_meta, torch.from_numpy(pen))
        if lpm is not None:
            put(r.lp_meta, torch.from_numpy(lpm))
        if ctl is not None:
            put(r.ctl_meta, torch.from_numpy(ctl))
        if adp is not None:
            put(r.slot_adapter, torch.from_numpy(adp))
        for i, row in bt_rows.items():
            put(r.block_tables[i], row)
        self._dirty_slots.clear()

    def _upload_pages(self):
        """Write the block-table entries of pages appended by ``_grow`` (one small copy, whatever the count).
        Slots whose whole row is re-uploaded this step, or that changed hands, are skipped."""
        r = self.r
        idx, val = [], []
        for s, j, blk in self._bt_new:
            if s.slot >= 0 and self.slots[s.slot] is s and s.slot not in self._dirty_slots:
                idx.append(s.slot * r.max_blocks + j)
                val.append(blk)
        self._bt_new.clear()
        if not idx:
            return
        packed = torch.tensor(idx + val, dtype=torch.int32)
        if r.device.type == "cuda":
            packed = packed.pin_memory().to(r.device, non_blocking=True)
        n = len(idx)
        r.block_tables.view(-1).index_copy_(0, packed[:n].long(), packed[n:])

    def _adapter_slot(self, s: Sequence) -> int:
        """The LoRA pool slot of s's adapter (-1: the base model)."""
        return -1 if s.params.lora is None else self.r.lora.slot_of(s.params.lora)

    @staticmethod
    def _hash_salt(s: Sequence) -> bytes:
        """h_{-1} of s's page-hash chain: empty for the base model, a digest of the adapter's NAME otherwise (K and V
        depend on the adapter, so its pages must never serve another adapter or the base model; the name, not the
        slot, so the identity survives slot numbering).  The host tier sits behind the same hashes."""
        if s.params.lora is None:
            return b""
        return hashlib.blake2b(b"lora:" + s.params.lora.encode(), digest_size=16).digest()

    def _bias(self, p: SamplingParams) -> dict:
        """logit_bias as {id: bias} over the ids the vocabulary has (ids distinct: the kernel's contract)."""
        V = self.r.cfg.vocab_size
        return {int(k): float(v) for k, v in (p.logit_bias or {}).items() if 0 <= int(k) < V}

    def _ban_ids(self, p: SamplingParams) -> list:
        """The ids min_tokens keeps from being sampled: EOS unless ignore_eos, then the stop_token_ids."""
        if p.min_tokens <= 0:
            return []
        V = self.r.cfg.vocab_size
        ids = ([] if p.ignore_eos else [int(self.eos_id)]) + [int(t) for t in p.stop_token_ids]
        return [t for t in dict.fromkeys(ids) if 0 <= t < V]

    def _guide_compiled(self, pattern: str, schema: bool = False):
        """(table, accept) of `pattern`, compiled once (the same compiler the HTTP routes validate with; a
        schema-derived pattern under the wide caps)."""
        hit = self._guide_dfa.get((pattern, schema))
        if hit is None:
            from .. import runtime

            rt = runtime.load()
            n, tab, acc = rt.guide_compile_wide(pattern) if schema else rt.guide_compile(pattern)
            hit = (np.frombuffer(tab, dtype=np.uint16).reshape(n, 256), np.frombuffer(acc, dtype=np.uint8))
            if len(self._guide_dfa) >= 4 * ops.GUIDE_POOL:  # bounded: drop the oldest
                self._guide_dfa.pop(next(iter(self._guide_dfa)))
            self._guide_dfa[(pattern, schema)] = hit
        return hit

    @staticmethod
    def _guide_pool(schema: bool) -> range:
        """The entry words of a guide's pool."""
        return range(ops.GUIDE_POOL, ops.GUIDE_POOL + ops.GUIDE_WIDE_POOL) if schema else range(ops.GUIDE_POOL)

    def _guide_acquire(self, pattern: str, schema: bool = False) -> int:
        """A reference to the pool entry that holds `pattern`, uploading its table into a free entry of its pool (one
        without references, the least recently used) when it is not resident; -1 = every entry is referenced: wait."""
        e = self._guide_idx.get((pattern, schema), -1)
        if e < 0:
            free = [i for i in self._guide_pool(schema) if self._guide_refs[i] == 0]
            if not free:
                return -1
            e = min(free, key=lambda i: (self._guide_pat[i] is not None, self._guide_used_at[i]))
            if self._guide_pat[e] is not None:
                del self._guide_idx[self._guide_pat[e]]
            tab, acc = self._guide_compiled(pattern, schema)
            self.r.upload_guide(e, tab, acc)  # (the first one allocates the pool and captures the graph twins)
            self._guide_pat[e], self._guide_idx[(pattern, schema)] = (pattern, schema), e
        self._guide_refs[e] += 1
        self._guide_lru += 1
        self._guide_used_at[e] = self._guide_lru
        return e

    def _guide_release(self, s: Sequence) -> None:
        if s.guide_entry >= 0:
            self._guide_refs[s.guide_entry] -= 1
            s.guide_entry = -1

    def _victim(self):
        """The sequence to preempt: paused ones first, then the most recent request (FCFS keeps the oldest)."""
        cands = [s for s in self.slots if s is not None and s.state in ("prefill", "decode") and not s.aborted
                 and not s.stop_after_enqueue]
        return max(cands, key=lambda s: (s.paused, s.rid))

    def _preempt(self, v: Sequence):
        """Free a sequence's slot and pages and requeue it (head of the queue) to be re-prefilled from its
        prompt plus the tokens it already published.  Tokens of its steps still in flight are discarded
        (``_consume`` skips the preempted object) and regenerated at the same positions -- with the same
        per-(seed, position) sampling draw.  Stream order keeps the freed pages safe: their in-flight
        writes precede anything a new owner enqueues."""
        self.stats["preemptions"] += 1
        n = Sequence(rid=v.rid, conversation_id=v.conversation_id, prompt=v.prompt[:v.orig_len] + v.out_ids,
                     params=v.params, arrival_ns=v.arrival_ns, produced=v.produced, first_token_ns=v.first_token_ns,
                     last_token_ns=v.last_token_ns, paused=v.paused, paused_at=v.paused_at, orig_len=v.orig_len,
                     out_ids=v.out_ids, base=v.produced, cached_tokens=v.cached_tokens)
        # prefix caching: no special case.  Its full pages are published, fall into the evictable pool as the most
        # recently used, and if they survive until it is readmitted its re-prefill is skipped
        self._publish_written(v)
        v.state = "preempted"
        self._guide_release(v)
        self.slots[v.slot] = None
        self._dirty_slots.add(v.slot)
        self.alloc.free(v.blocks)
        v.blocks = []
        if self.by_conv.get(v.conversation_id) is v:
            self.by_conv[v.conversation_id] = n
        self.waiting.appendleft(n)

    # ------------------------------------------------------------------ prefix cache
    # Invariant the publishing rests on: every K/V write lands on the stream all later steps run on.  Prompt rows are
    # written by rope_kv_write of the prefill / mixed pass, decode rows by the folded QKV write in
    # paged_attention_kernel, both on the compute stream (the TP prefill's side stream carries only the residual
    # collectives and norms, and the main stream waits for it before the pass ends).  So a page may be published as
    # soon as the step that writes its last position is ENQUEUED: whoever looks it up later enqueues behind it.
    # Positions whose writes are enqueued: a prompt chunk writes [start_pos, start_pos + n), so s.prefilled prompt
    # positions; a decode step writes the position of the token it consumes as input, so a decoding sequence has
    # len(s.prompt) + s.decode_enqueued positions written, and the token sampled last has no K/V yet.
    def _publish_pages(self, s: Sequence, upto: int) -> None:
        for i in range(s.published, upto):
            self.alloc.publish(s.blocks[i], s.hashes[i])
        s.published = max(s.published, upto)

    def _publish_prompt(self, s: Sequence) -> None:
        """Right after the step that carries s's latest prompt chunk was enqueued: its wholly written prompt pages."""
        if self.prefix_cache and s.blocks:
            self._publish_pages(s, min(s.prefilled // PAGE, len(s.hashes)))

    def _publish_written(self, s: Sequence) -> None:
        """When a decoding sequence leaves (finish, abort, preemption): the full pages that generated tokens
        completed.  The host learns those ids only from the drain, so the count is the smaller of the positions
        written (above) and the tokens known, prompt[:orig_len] + out_ids; a late stop's wasted step wrote a position
        past the known tokens, which is never counted.  A prompt that leaves mid-prefill publishes nothing more."""
        if not self.prefix_cache or s.state != "decode" or not s.blocks:
            return
        full = s.prompt[:s.orig_len] + s.out_ids
        pages = min(min(len(s.prompt) + s.decode_enqueued, len(full)) // PAGE, len(s.blocks))
        if pages > len(s.hashes):
            s.hashes = s.hashes + page_hashes(full[:pages * PAGE], s.hashes[-1] if s.hashes else self._hash_salt(s),
                                              len(s.hashes))
        self._publish_pages(s, pages)

    def _check_write_pages(self, chunks: list, dec: list) -> None:
        """No shared page (more than one owner, or published) may be in a step's write slots (CPU engines, or
        DSSE_DEBUG_PREFIX_CACHE=1): a hit writes only at positions >= its cached length, on its private pages."""
        bad = []
        for c in chunks:
            pages = range(c.start_pos // PAGE, (c.start_pos + len(c.tokens) - 1) // PAGE + 1)
            bad += [(c.slot, c.block_table[i]) for i in pages if self.alloc.is_shared(c.block_table[i])]
        for s in dec:
            b = s.blocks[(len(s.prompt) + s.decode_enqueued) // PAGE]
            if self.alloc.is_shared(b):
                bad.append((s.slot, b))
        if bad:
            self.shared_write_violations += len(bad)
            raise AssertionError(f"prefix cache: step {self.step_no} would write shared KV pages (slot, block): {bad}")

    def _drain_spills(self, reserve: int = 0) -> None:
        """Copy the pages evicted since the last call out to the host tier.  Called after the allocations of a step
        (and of an admission that restores) and BEFORE anything that writes the evicted blocks is enqueued, so the
        gather reads the old content (KVOffload rule a).  Never waits: what exceeds the free staging records (less
        `reserve`, kept for the caller's restore) or finds no host slot is dropped, least recently used first, and a
        page whose content the store already holds is not copied again."""
        off = self.offload
        if off is None:
            return
        off.poll()
        spills = self.alloc.take_spills()
        if not spills:
            return
        st = self.alloc.host_store
        todo = [(b, h) for b, h in spills if not st.has(h)]
        self.stats["offload_spill_skipped"] += len(spills) - len(todo)
        room = max(0, off.free_records() - reserve)
        pairs = []
        for b, h in todo[max(0, len(todo) - room):]:  # (the list is in eviction order: its head is dropped first)
            slot = st.reserve(h)
            if slot is not None:
                pairs.append((b, slot))
        self.stats["offload_dropped_pages"] += len(todo) - len(pairs)
        self.stats["offload_spilled_pages"] += len(pairs)
        if pairs:
            off.spill(pairs)

    def _grow(self):
        """Before the decode step: every sequence in it needs the page its write position falls in."""
        need = [s for s in self.slots if s is not None and s.state == "decode" and not s.aborted
                and not s.stop_after_enqueue and not s.paused
                and (len(s.prompt) + s.decode_enqueued) // PAGE >= len(s.blocks)]
        for s in sorted(need, key=lambda s: s.rid):  # oldest first: the newest are the ones preempted
            while self.alloc.num_free == 0 and s.state == "decode":
                self._preempt(self._victim())
            if s.state != "decode":
                continue
            blk = self.alloc.allocate(1)[0]
            self._bt_new.append((s, len(s.blocks), blk))
            s.blocks.append(blk)

    def _admit(self):
        r = self.r
        while self.waiting:
            s = self.waiting[0]
            free = next((i for i, x in enumerate(self.slots) if x is None), -1)
            if free < 0:
                return
            if s.base == 0:  # first admission: clamp max_tokens to the context and to the whole pool
                cap = self.alloc.num_blocks * PAGE - s.orig_len
                max_new = max(1, min(s.params.max_tokens, r.max_model_len - s.orig_len, cap))
                s.params = SamplingParams(**{**s.params.__dict__, "max_tokens": max_new,
                                             "min_tokens": max(0, min(int(s.params.min_tokens), max_new))})
            if s.params.guide is not None and (s.params.guide, s.params.guide_schema) not in self._guide_idx and \
                    all(self._guide_refs[i] > 0 for i in self._guide_pool(s.params.guide_schema)):
                return  # its pattern is not resident and every pool entry is in use: it waits, as for KV pages
            # parallel sampling: a sibling whose parent (choice 0) holds a slot with its whole prompt enqueued is
            # admitted like a prefix hit of len(prompt) - 1 tokens on the parent's own pages; it waits while the parent
            # is still prefilling, and takes the plain path below when the parent is gone (finished, aborted, preempted)
            par, s.parent = s.parent, None
            if par is not None:
                if par.state == "prefill" and not par.aborted and par.prefilled < len(par.prompt):
                    s.parent = par
                    return
                if not (par.state in ("prefill", "decode") and par.slot >= 0 and self.slots[par.slot] is par
                        and not par.aborted and par.base == 0 and par.prefilled == len(par.prompt)
                        and len(par.prompt) == len(s.prompt) and len(par.blocks) >= blocks_needed(len(s.prompt))):
                    par = None
            nshared = (len(s.prompt) - 1) // PAGE if par is not None else 0
            hits, run, host = [], None, []
            if par is not None:
                if self.prefix_cache and not s.hashes:
                    s.hashes = page_hashes(s.prompt, self._hash_salt(s))
            elif self.prefix_cache:
                # the resident leading pages of the prompt minus its last token: at least one token is always
                # prefilled, so the first token is sampled by the ordinary last-chunk path.  (Hashed once; looked up
                # on every attempt while it waits: the index changes between steps.)
                if not s.hashes:
                    s.hashes = page_hashes(s.prompt, self._hash_salt(s))
                chain = s.hashes[:(len(s.prompt) - 1) // PAGE]
                if self.offload is None:
                    hits = self.alloc.lookup(chain)
                else:
                    # both tiers: run[i] is page i's resident block, or None for a page to copy back from the host
                    # slot in `host` (at most as many as there are free staging records: a longer hit is cut there)
                    self.offload.poll()
                    run, host = self.alloc.lookup_tiers(chain, max_host=self.offload.free_records())
                    hits = [b for b in run if b is not None]
            # pages to allocate: everything that is not resident, the host-tier hits' new HBM pages included
            need = blocks_needed(len(s.prompt)) - (len(hits) if par is None else nshared)
            idle = not any(x is not None for x in self.slots)
            if need > self.alloc.num_free - (0 if idle else self.watermark):
                s.parent = par  # (a sibling that waits for pages still forks when they come)
                if hits:
                    self.alloc.free(hits)  # it waits: the references go back (the pages stay indexed)
                for _, slot in host:
                    self.alloc.host_store.release(slot)
                if idle and need + len(hits) > self.alloc.num_blocks:  # can never fit: fail it rather than wait forever
                    self.waiting.popleft()
                    self._finish(s, self._early, reason="length")
                    continue
                return
            self.waiting.popleft()
            if par is not None:
                # fork: one more reference on the parent's full prompt pages (never written again by anyone), one
                # private page for the rest.  When the last prompt token is not the first of its page, that page starts
                # as a copy of the parent's: the copy is enqueued with this step's others, before its passes, so stream
                # order puts it behind the parent's prompt writes and ahead of this sibling's first chunk.
                hits = self.alloc.fork(par.blocks[:nshared])
                new = self.alloc.allocate(need)
                s.blocks = hits + new
                if (len(s.prompt) - 1) % PAGE:
                    self._fork_pairs.append((par.blocks[nshared], new[0]))
                    self.stats["fork_tail_copies"] += 1
                self.stats["fork_shared_tokens"] += len(s.prompt) - 1
            elif not host:
                s.blocks = hits + self.alloc.allocate(need)
            else:
                # restore: the first new pages take the host-tier hits' places.  The allocation may have evicted
                # pages (those very blocks among them): their gathers are enqueued first, then H2D + scatter, all
                # before this prompt's first chunk -- the compute stream orders them (KVOffload rules a and d).
                # The restored blocks are then published under their hashes like any prefilled page.
                new = self.alloc.allocate(need)
                self._drain_spills(reserve=len(host))
                pairs = [(slot, new[j]) for j, (_, slot) in enumerate(host)]
                self.offload.restore(pairs)
                for (i, _), (_, b) in zip(host, pairs):
                    run[i] = b
                    self.alloc.publish(b, s.hashes[i])
                s.blocks = run + new[len(host):]
                hits = run
                self.stats["offload_restored_pages"] += len(host)
                self.stats["offload_hit_tokens"] += PAGE * len(host)
            s.slot = free
            s.state = "prefill"
            # its chunks start here: it writes private pages only (a forked sibling: its last prompt token alone)
            s.prefilled = PAGE * len(hits) if par is None else len(s.prompt) - 1
            s.published = len(hits)
            s.decode_enqueued = 0
            if self.prefix_cache:
                if s.cached_tokens < 0:  # what the client is told: the first admission's hit, not a re-prefill's
                    s.cached_tokens = min(s.prefilled, s.orig_len)
                if par is None:  # (a fork is not a lookup: it has its own counters)
                    self.stats["prefix_queries"] += len(s.prompt)
                    self.stats["prefix_hit_tokens"] += s.prefilled
                self.stats["prefix_evictions"] = self.alloc.evictions
            self.slots[s.slot] = s
            self._dirty_slots.add(s.slot)
            if s.params.penalised():
                # its history: the prompt as submitted, then (after a preemption) everything it has published
                # (`prompt` is exactly that); the device appends every token sampled from here on
                r.set_history(s.slot, s.prompt, s.orig_len)
            if s.params.logprobs >= 0:
                r.enable_logprobs()  # (the first such request captures the graph twins with the logprob passes)
            if s.params.lora is not None:
                r.enable_lora()  # (the first such request captures the graph twins with the LoRA layer body)
            if s.params.controlled():
                # its bias entries and banned ids (again after a preemption: the slot may be another one); the first
                # such request captures the graph twins with the bias and ban pass and min_p
                r.set_controls(s.slot, self._bias(s.params), self._ban_ids(s.params))
            if s.params.guide is not None:
                # its pattern's pool entry, and the DFA state after the tokens it has already published (after a
                # preemption the regenerated tokens continue the same match); the device advances it from here on
                wide = s.params.guide_schema
                s.guide_entry = self._guide_acquire(s.params.guide, wide)
                r.set_guide(s.slot, s.guide_entry,
                            ops.guide_walk(self._guide_compiled(s.params.guide, wide)[0], 0, s.out_ids, *r.guide_host,
                                           r.guide_eos, ops.GUIDE_WIDE_STATES if wide else ops.GUIDE_STATES))
            elif s.params.json_object:
                # JSON mode holds no pool entry (it never waits for one, and _guide_release has nothing to give
                # back): the slot gets the marker and the pushdown state after the tokens already published
                r.enable_guides()
                r.set_guide(s.slot, ops.JSON_ENTRY, ops.json_walk_ids(ops.JSON_START_STATE, s.out_ids, *r.guide_host,
                                                                      r.guide_eos))
            else:
                r.set_guide(s.slot, -1, 0)  # (a no-op until a guided request has been seen)

    def _copy_fork_tails(self):
        """The tail pages of the siblings admitted in this step, in one launch on the compute stream (after the step's
        spills were read out of the blocks it allocated, before its passes)."""
        pairs, self._fork_pairs = self._fork_pairs, []
        ops.kv_pages_copy(self.r.kv.k, self.r.kv.v, pairs)

    def _compact(self):
        """Move decoding sequences above the bucket their count needs into lower free / paused slots."""
        dec = [s for s in self.slots if s is not None and s.state == "decode" and not s.aborted
               and not s.stop_after_enqueue and not s.paused]
        if not dec:
            return
        buckets = batch_buckets(self.r.max_batch)
        hi = max(s.slot for s in dec) + 1
        want = next(b for b in buckets if b >= len(dec))
        if next(b for b in buckets if b >= hi) <= want:
            return
        holes = [i for i in range(want) if self.slots[i] is None or (
            self.slots[i].state == "decode" and self.slots[i].paused and not self.slots[i].stop_after_enqueue)]
        movers = sorted((s for s in dec if s.slot >= want), key=lambda s: -s.slot)
        src, dst = [], []
        for s, j in zip(movers, holes):
            i, p = s.slot, self.slots[j]
            src.append(i)
            dst.append(j)
            self.slots[j], s.slot = s, j
            self.slots[i] = p
            if p is not None:  # swap with a paused sequence: its device state goes the other way
                p.slot = i
                src.append(j)
                dst.append(i)
            self._dirty_slots.update((i, j))
        if src:
            self.r.move_slots(src, dst)
            self.stats["compactions"] += 1

    def _decode_bucket(self) -> int:
        hi = max((s.slot for s in self.slots if s is not None and s.state == "decode"), default=-1) + 1
        return next(b for b in batch_buckets(self.r.max_batch) if b >= hi) if hi > 0 else 0

    def _mixed_fits(self, B: int, chunks: list) -> bool:
        graphs = getattr(self.r, "mx_graphs", None)
        if not graphs:  # no captured mixed steps (CPU, or DSSE_MIXED_GRAPHS=0): the eager mixed step takes any size
            return True
        T = sum(len(c.tokens) for c in chunks)
        return self.r.mixed_graph_rows(B, T) is not None and len(chunks) <= PREFILL_GRAPH_SEQS

    def _mixed_budget(self, B: int) -> int:
        """Prompt rows for this mixed step of bucket B: the runner's default chunk (256), raised to the largest
        captured size whose measured-cost step stays within the ratio (PassCost.mixed_chunk) -- never lowered
        below the default: chunks cut to the ratio at small buckets (128 rows at 64 streams) halve the prompt
        throughput, and at 40 req/s the queue then grows without bound (TTFT p50 0.39 s, profiles/r5/serving_r5.md).
        A backlog longer than the chunk is split into even shares (two 256-row steps instead of 384 + 128: the
        longest step, which sets the ITL tail, is shorter)."""
        sizes = self.r.mixed_chunks(B) if hasattr(self.r, "mixed_chunks") and getattr(self.r, "mx_graphs", None) \
            else []
        cap = self.r.mixed_chunk(B)
        if self.cost is not None and sizes and not self.deterministic:
            self.cost.poll()
            fit = self.cost.mixed_chunk(B, sizes)
            if fit is not None:
                cap = max(cap, fit)
        pending = [s for s in self.slots if s is not None and s.state == "prefill" and not s.aborted]
        backlog = sum(len(s.prompt) - s.prefilled for s in pending)
        if self.mixed_queue_boost and sizes and len(pending) + len(self.waiting) >= 2:
            # prompts queue: the largest captured chunk, so the weights stream once for more prompt rows (the
            # step's length then matches a bucket-128 mixed step's, the ITL tail the serving mix already has)
            cap = max(cap, max(sizes))
        if backlog > cap:
            n = -(-backlog // cap)  # steps the backlog needs at the cap
            per = -(-backlog // n)  # their even share
            cap = min(cap, -(-per // 64) * 64)
        return max(self.mixed_min_tokens, cap)

    def set_itl_ratio(self, ratio: float) -> None:
        """Adaptive prefill budget on (ratio > 1) or off (bench_serving sweeps both in one process)."""
        self.cost = PassCost(ratio) if ratio > 1.0 and self.r.device.type == "cuda" and not self.deterministic \
            else None

    def _oldest_prefill_step(self) -> int:
        oldest = min((s.enq_step for s in self.slots if s is not None and s.state == "prefill"), default=self.step_no)
        if self.waiting:
            oldest = min(oldest, self.waiting[0].enq_step)
        return oldest

    def _schedule_prefill(self, t: int):
        running_decode = any(s is not None and s.state == "decode" for s in self.slots)
        budget = self.prefill_budget if running_decode else self.idle_prefill_budget
        if running_decode and self.cost is not None and not self.mixed and not self.deterministic:
            self.cost.poll()
            adaptive = self.cost.budget(self._decode_bucket(), self.prefill_budget)
            if adaptive is not None and self.step_no - self._oldest_prefill_step() <= self.boost_steps:
                budget = adaptive
        if running_decode and self.mixed:
            # the chunk rides in the decode step: keep B + chunk near the next row bucket, unless a prompt has
            # waited too long (counted in steps: identical on every TP rank)
            hi = max((s.slot for s in self.slots if s is not None and s.state == "decode"), default=-1) + 1
            B = next(b for b in batch_buckets(self.r.max_batch) if b >= hi)
            oldest = min((s.enq_step for s in self.slots if s is not None and s.state == "prefill"),
                         default=self.step_no)
            if self.waiting:
                oldest = min(oldest, self.waiting[0].enq_step)
            if self.step_no - oldest <= self.mixed_boost_steps:
                budget = min(budget, self._mixed_budget(B))
        chunks, finished = [], []
        # shortest remaining prompt first (then arrival order): a prompt already half prefilled finishes before a
        # new one starts, which minimises the mean time to first token
        pending = sorted((s for s in self.slots if s is not None and s.state == "prefill" and not s.aborted),
                         key=lambda s: (len(s.prompt) - s.prefilled, s.rid))
        for s in pending:
            if budget <= 0:
                continue
            n = min(len(s.prompt) - s.prefilled, budget)
            if not s.stamped:  # (not `prefilled == 0`: a prefix-cache hit starts past 0)
                s.stamped = True
                s.admit_ns = time.time_ns()
            last = s.prefilled + n == len(s.prompt)
            chunks.append(PrefillSeq(slot=s.slot, tokens=s.prompt[s.prefilled:s.prefilled + n], start_pos=s.prefilled,
                                     block_table=s.blocks, last_chunk=last, adapter=self._adapter_slot(s)))
            s.prefilled += n
            budget -= n
            if last:
                finished.append(s)
        return chunks, finished

    def _finish(self, s: Sequence, events: list, reason: str = "stop", text: str = "[DONE]", publish: bool = True):
        if s.state == "finished":
            return
        if publish:
            self._publish_written(s)  # (before its pages are freed: published ones stay indexed, evictable)
        s.state = "finished"
        self._guide_release(s)
        now = time.time_ns()
        events.append(TokenEvent(s.conversation_id, -1, s.produced + 1, True, text=text, timestamp_ns=now,
                                 finish=reason, prompt_tokens=s.orig_len,
                                 cached_tokens=max(0, s.cached_tokens) if self.prefix_cache else -1))
        if s.slot >= 0 and self.slots[s.slot] is s:
            self.slots[s.slot] = None
            self._dirty_slots.add(s.slot)
        if s.blocks:
            self.alloc.free(s.blocks)
            s.blocks = []
        if self.by_conv.get(s.conversation_id) is s:
            del self.by_conv[s.conversation_id]
        root = self._group_of.pop(s.conversation_id, None)
        if root is not None:
            live = self._groups.get(root)
            if live is not None:
                live.discard(s.conversation_id)
                if not live:
                    del self._groups[root]

    # ------------------------------------------------------------------ step
    def step(self, block: bool = True) -> list:
        """Enqueue one engine step and return the token events of completed earlier steps."""
        t0 = time.perf_counter()
        events, self._pending = self._pending, []
        self._early = events
        r = self.r
        # sequences whose max_tokens budget is fully enqueued stop decoding now
        for s in self.slots:
            if s is not None and s.state == "decode" and s.base + s.decode_enqueued + 1 >= s.params.max_tokens:
                if not s.stop_after_enqueue:
                    s.stop_after_enqueue = True
                    self._dirty_slots.add(s.slot)
            if s is not None and s.aborted and s.state != "finished":
                self._dirty_slots.add(s.slot)
        self._grow()
        self._admit()
        # host tier: the pages this step's allocations evicted are copied out before the step that writes them
        self._drain_spills()
        if self._fork_pairs:
            self._copy_fork_tails()
        if not self.waiting:
            self._compact()
        t_a = time.perf_counter()
        row = self.ring_head % RING_SIZE
        chunks, prefill_done = self._schedule_prefill(self.step_no)
        t_b = time.perf_counter()
        self._upload()
        t_c = time.perf_counter()
        producers = []
        ran = False
        dec = [s for s in self.slots if s is not None and s.state == "decode" and not s.aborted
               and not s.stop_after_enqueue and not s.paused]
        B = next(b for b in batch_buckets(r.max_batch) if b >= max(s.slot for s in dec) + 1) if dec else 0
        # a mixed step only when the chunks fit its captured graph (a starved prompt's big budget: separate passes)
        mixed = bool(chunks) and bool(dec) and self.mixed and self._mixed_fits(B, chunks)
        if (self.prefix_cache or self.alloc.has_forks) and self.debug_shared_writes:
            self._check_write_pages(chunks, dec)
        if chunks:
            if not mixed:
                done = (self.cost.record("prefill", sum(len(c.tokens) for c in chunks))
                        if self.cost is not None and r.device.type == "cuda" else None)
                r.prefill(chunks, ring_row=row)
                if done:
                    done()
            self.stats["prefill_tokens"] += sum(len(c.tokens) for c in chunks)
            if not mixed and dec and prefill_done:
                # a decode step follows on the stream: drain the first tokens now (TTFT minus one decode step)
                self.drain.issue(row, max(s.slot for s in prefill_done) + 1, first=True)
                self.inflight.append((self.step_no, row, [(s.slot, s) for s in prefill_done], t0, True))
            else:
                producers += [(s.slot, s) for s in prefill_done]
            ran = True
        est_ms = None  # expected GPU time of the step enqueued now (just-in-time enqueue: jit_delay)
        if dec:
            if mixed:
                C = r.mixed_graph_rows(B, sum(len(c.tokens) for c in chunks)) if hasattr(r, "mixed_graph_rows") \
                    else None
                done = (self.cost.record("mixed", (B, C)) if self.cost is not None and C is not None
                        and r.device.type == "cuda" else None)
                r.mixed(B, chunks, ring_row=row)
                if done:
                    done()
                    est_ms = self.cost.mixed_ms(B, C)
                self.stats["mixed_steps"] += 1
                hist = self.stats.setdefault("mixed_graph_rows", {})
                hist[C] = hist.get(C, 0) + 1
            else:
                done = self.cost.record("decode", B) if self.cost is not None and r.device.type == "cuda" else None
                r.decode(B)
                if done:
                    done()
                    est_ms = None if chunks else self.cost.step_ms.get(B)
            for s in dec:
                s.decode_enqueued += 1
                producers.append((s.slot, s))
            self.stats["decode_steps"] += 1
            ran = True
        elif ran:
            from .. import ops
            ops.ring_advance(r.ring_counter)
        if self.prefix_cache:
            # the pass that writes these chunks' K/V is enqueued (separately or inside the mixed step): the prompt
            # pages it completed may be shared by anything admitted from now on
            for c in chunks:
                self._publish_prompt(self.slots[c.slot])
        for s in prefill_done:
            s.state = "decode"
            self._dirty_slots.add(s.slot)
        t_enq = time.perf_counter()
        if self.enq_trace is not None and ran:  # host time from the step's start to its enqueue (bench_serving.py)
            self.enq_trace.append(("mixed" if chunks and dec and mixed else ("prefill" if chunks else "decode"),
                                   t_enq - t0, (t_a - t0, t_b - t_a, t_c - t_b, t_enq - t_c)))
        if ran:
            width = max(sl for sl, _ in producers) + 1 if producers else 1
            self.drain.issue(row, width)
            self.inflight.append((self.step_no, row, producers, t0, False))
            self.ring_head += 1
            self.step_no += 1
        # ---- consume drained steps: keep `depth` steps in flight, process everything that is ready
        wait = 0.0  # blocked on a drain event (GPU time, not host work)
        t_done = None
        n_main = sum(1 for e in self.inflight if not e[4])
        depth = self.depth
        while self.inflight:
            st, rrow, prods, tq, first = self.inflight[0]
            must = n_main > depth or not ran
            if not must and (self.deterministic or not block or not self.drain.ready(rrow, first)):
                break
            if self.on_flush is not None and events and not self.drain.ready(rrow, first):
                self.on_flush(list(events))
                events.clear()
            tw = time.perf_counter()
            toks = self.drain.wait(rrow, first)
            bad = self.drain.faults(rrow, first)
            if bad:
                raise EngineFault("; ".join(bad))
            n_main -= 0 if first else 1
            t_done = time.perf_counter()
            wait += t_done - tw
            self.inflight.popleft()
            self._consume(toks, prods, events, self.drain.logprobs(rrow, first))
        # the newest step started when its predecessor finished (the wait above) or, on an idle GPU, when enqueued
        if ran:
            self._jit = (max(t_enq, t_done), est_ms) if n_main == 1 and t_done is not None else (t_enq, est_ms)
        # aborted sequences leave at this boundary
        for s in list(self.slots):
            if s is not None and s.aborted and s.state != "finished" and not any(
                    s is p for _, _, prods, _, _ in self.inflight for _, p in prods):
                self._finish(s, events, reason="abort")
        self.stats["steps"] += 1
        if self.prefix_cache:
            self.stats["prefix_evictions"] = self.alloc.evictions
        dt = time.perf_counter() - t0
        self.stats["last_step_s"] = dt
        self.stats["wait_s"] = wait
        self.stats["host_s"] = dt - wait
        return events

    def _consume(self, toks, prods, events, lps=None):
        now = time.time_ns()
        tl = toks.tolist()
        lp_ids = lps.view(torch.int32) if lps is not None else None
        for slot, s in prods:
            if s.state == "finished" or s.state == "preempted" or s.aborted:
                continue
            tok = int(tl[slot])
            s.produced += 1
            if s.produced == 1:
                s.first_token_ns = now
                if self.on_ttft:
                    self.on_ttft((now - s.arrival_ns) / 1e9)
                if self.ttft_trace is not None:  # TTFT split (tools/bench_serving.py): arrival, queued, admitted, token
                    self.ttft_trace.append((s.arrival_ns, s.queued_ns, s.admit_ns, now))
            elif self.on_itl and s.last_token_ns:
                self.on_itl((now - s.last_token_ns) / 1e9)
            s.last_token_ns = now
            # a stop_token_ids entry ends the stream as EOS does (undelivered), whatever ignore_eos says
            is_eos = (tok == self.eos_id and not s.params.ignore_eos) or tok in s.params.stop_token_ids
            if not is_eos:
                ev = TokenEvent(s.conversation_id, tok, s.produced, False, timestamp_ns=now)
                if s.params.logprobs >= 0 and lps is not None:
                    n = min(int(s.params.logprobs), 20)
                    row, ids = lps[slot].tolist(), lp_ids[slot, 1:1 + n].tolist()
                    ev.logprob = row[0]
                    ev.top = [(t, row[21 + j]) for j, t in enumerate(ids) if t >= 0]
                events.append(ev)
                s.out_ids.append(tok)
                self.stats["tokens"] += 1
            else:
                s.produced -= 1
            if is_eos:
                self._finish(s, events, reason="stop")
            elif s.produced >= s.params.max_tokens or s.orig_len + s.produced >= self.r.max_model_len:
                self._finish(s, events, reason="length")

    def fail_all(self, text: str = "[ERROR]") -> list:
        """Terminal `text` events for every live conversation (running, paused, queued), after an EngineFault: the
        clients see the reference's upstream-error token (llm-stream-proxy main.go:166-186) instead of a hang or
        tokens computed from untrusted state.  Nothing else is enqueued on the device."""
        events = []
        self.inflight.clear()
        for s in list(self.slots) + list(self.waiting):
            if s is not None and s.state != "finished":
                self._finish(s, events, reason="abort", text=text, publish=False)  # (untrusted KV is never indexed)
        self.waiting.clear()
        return events

    def error_events(self, text: str = "[ERROR]") -> list:
        """Terminal `text` events for every live conversation WITHOUT touching engine state (the watchdog's view of a
        loop blocked inside a step: the loop may still resume, so only it may mutate the engine)."""
        now = time.time_ns()
        live = [s for s in list(self.slots) + list(self.waiting) if s is not None and s.state != "finished"]
        return [TokenEvent(s.conversation_id, -1, s.produced + 1, True, text=text, timestamp_ns=now, finish="abort",
                           prompt_tokens=s.orig_len) for s in live]

    def run_until_idle(self, max_steps: int = 100000) -> list:
        out = []
        for _ in range(max_steps):
            if not self.has_work():
                break
            out += self.step()
        return out
