"""The serving process: native runtime (HTTP/SSE/bus) + one engine loop per GPU replica.

Data path of one token (compare reference README.md:59-68, six network hops and four JSON
round trips): sampled on the GPU into the HBM token ring -> side-stream copy into pinned host memory
-> engine loop publishes the step's tokens in one call -> C++ bus formats one SSE frame per token
and fans it out to the subscribed connections' I/O threads -> epoll writer.  No network hop inside
the node.

Engine kinds:
* ``gpu``  Mistral on the gfx950 kernels (TP group of this process, captured hipGraphs);
* ``cpu``  the same engine on the fp32 reference ops with a tiny model (plumbing tests, no GPU);
* ``stub`` the C++ stub token generator (BASELINE config 1: delivery plumbing only).
"""
from __future__ import annotations

import threading
import json
import os
import time

import torch

from .. import runtime as rt_mod
from ..engine.engine import FINISH_CODES, EngineFault, LLMEngine, SamplingParams, TokenEvent
from ..engine.kv_cache import KVCache, kv_cache_torch_dtype
from ..engine.model_runner import ModelRunner
from ..models.mistral import TINY, get_config, init_standard_weights
from ..models.tokenizer import get_tokenizer, prompt_for_request
from .config import ServeConfig
from .faults import FaultPlan, StepTracer, Watchdog
from .stop_strings import StopMatcher


def build_engine(cfg: ServeConfig, device=None, comm=None):
    """Weights + KV cache + runner + engine for this process (one DP replica / TP rank)."""
    from ..engine.weights import convert_standard, load_safetensors, random_engine_weights

    cfg.validate()  # option combinations (quantization with tp > 1, ...) fail here, before any weight is loaded
    quant = cfg.quantization

    def lora_pool(mcfg, dev):
        """--enable-lora: every --lora-modules entry loaded into the device pool (None with LoRA off).  A refused
        adapter (rank above --max-lora-rank, DoRA, a foreign shape, ...) is a start-up error that names its file."""
        if not cfg.enable_lora:
            return None
        from ..engine.lora import build_pool
        from .config import parse_lora_modules

        pool = build_pool(mcfg, parse_lora_modules(cfg.lora_modules), cfg.max_loras, cfg.max_lora_rank, dev)
        if comm is None or comm.rank == 0:
            print(f"[engine] LoRA: {pool.slots} slots of rank {pool.R} ({pool.nbytes() / 1e6:.1f} MB), adapters "
                  f"{[n for n in pool.names if n is not None]}", flush=True)
        return pool

    if cfg.engine == "cpu":
        mcfg = TINY if cfg.model.startswith("mistral-7b") else get_config(cfg.model)
        tp_rank, tp = (comm.rank, comm.size) if comm is not None else (0, 1)
        w = convert_standard(mcfg, init_standard_weights(mcfg, seed=cfg.seed), tp_rank=tp_rank, tp_size=tp,
                             quantization=quant)
        runner = ModelRunner(w, num_blocks=256, max_batch=min(cfg.max_batch, 8),
                             max_model_len=min(cfg.max_model_len, 1024), device="cpu", comm=comm, use_graphs=False,
                             kv_cache_dtype=cfg.kv_cache_dtype, lora=lora_pool(mcfg, "cpu"))
    else:
        device = device or torch.device("cuda", torch.cuda.current_device())
        mcfg = get_config(cfg.model)
        tp_rank, tp = (comm.rank, comm.size) if comm is not None else (0, 1)
        if cfg.weights_path:
            w = load_safetensors(mcfg, cfg.weights_path, tp_rank, tp, device, quantization=quant)
        else:
            w = random_engine_weights(mcfg, tp_rank=tp_rank, tp_size=tp, device=device, seed=cfg.seed,
                                      quantization=quant)
        pool = lora_pool(mcfg, device)  # resident before the page budget below is sized, so its bytes are counted
        # the page budget below is what is free once the weights are resident: under quantization both copies (the
        # widened bf16 one, 14.5 GB for Mistral-7B, and the FP8 one, 7.2 GB, or the MXFP4 one, 3.8 GB) are already
        # allocated here
        free, total = torch.cuda.mem_get_info(device)
        budget = int(total * cfg.gpu_memory_utilization) - (total - free) - (2 << 30)
        nkv = mcfg.num_kv_heads // tp
        nblk = max(64, min(KVCache.blocks_for_budget(budget, mcfg.num_layers, nkv, kv_cache_torch_dtype(cfg.kv_cache_dtype)),
                           cfg.max_batch * (cfg.max_model_len // 32 + 2) * 4))
        runner = ModelRunner(w, num_blocks=nblk, max_batch=cfg.max_batch, max_model_len=cfg.max_model_len,
                             device=device, comm=comm, kv_cache_dtype=cfg.kv_cache_dtype, lora=pool)
        runner.capture()
    kv = runner.kv
    if comm is None or comm.rank == 0:
        f8, f4 = w.nbytes_fp8(), w.nbytes_fp4()
        print(f"[engine] weights: quantization {runner.quantization}, bf16 copy {(w.nbytes() - f8 - f4) / 1e9:.2f} GB"
              + (f" (widened from fp8), fp8 copy {f8 / 1e9:.2f} GB (decode buckets of 64 rows or fewer)"
                 if f8 else "")
              + (f" (widened from mxfp4), mxfp4 copy {f4 / 1e9:.2f} GB (decode buckets of 64 rows or fewer)"
                 if f4 else ""), flush=True)
        print(f"[engine] KV cache: {'fp8_e4m3' if kv.is_fp8 else 'bf16'} ({cfg.kv_cache_dtype}), "
              f"{KVCache.bytes_per_block(kv.num_layers, kv.nkv, kv.dtype) // 32 // 1024} KiB per token"
              f"{' per rank' if comm is not None and comm.size > 1 else ''}, {kv.num_blocks} pages of 32 tokens",
              flush=True)
    tok = get_tokenizer(mcfg.vocab_size, cfg.tokenizer_path or None)
    runner.set_guide_vocab(tok.pieces(), tok.eos_id)  # guided decoding constrains the text: the pieces' bytes
    engine = LLMEngine(runner, eos_id=tok.eos_id, prefill_budget=cfg.prefill_budget, max_pause_s=cfg.max_pause_s,
                       default_params=SamplingParams(temperature=cfg.temperature, max_tokens=cfg.max_tokens),
                       prefix_cache=cfg.enable_prefix_caching, kv_offload_pages=kv_offload_pages(cfg, runner))
    if engine.offload is not None and (comm is None or comm.rank == 0):
        st = engine.alloc.host_store
        print(f"[engine] host KV tier: {st.capacity} pages of {st.bytes_per_block >> 10} KiB "
              f"({st.capacity * st.bytes_per_block / 2**30:.2f} GiB {'pinned ' if runner.device.type == 'cuda' else ''}"
              "host memory)", flush=True)
    return engine, tok


def kv_offload_pages(cfg: ServeConfig, runner) -> int:
    """Pages of the host KV tier for --kv-offload-gb / KV_OFFLOAD_GB (0 = off); start-up errors name the fix."""
    cfg.validate()
    if cfg.kv_offload_gb <= 0:
        return 0
    kv = runner.kv
    per = KVCache.bytes_per_block(kv.num_layers, kv.nkv, kv.dtype)
    pages = int(cfg.kv_offload_gb * 2**30) // per
    if pages < 1:
        raise ValueError(f"--kv-offload-gb {cfg.kv_offload_gb} holds less than one KV page ({per} bytes = "
                         f"{per / 2**30:.6f} GiB): raise it to at least that, or set it to 0 to turn the host tier off")
    return pages


class EngineLoop(threading.Thread):
    """Pulls chat requests from the runtime, steps the engine, publishes token events.

    `runtime` is either the in-process ``Runtime`` (single replica, TP leader) or a ``DpWorker`` channel
    to a data-parallel router (``serving/dp.py``); both expose poll_requests / pop_cancellations /
    publish_tokens / set_ready.  A DP worker ships its engine metrics to the router (``observe``).
    """

    halted = False
    pub_lock = threading.Lock()  # class default (a loop built without __init__); each loop sets its own
    stops = None                 # (likewise: no stop-string matching)
    _prefix_cache = False        # (likewise: no cached_tokens on the terminal events, no prefix-cache counters)
    _offload = False             # (likewise: no host-tier counters)

    def __init__(self, runtime, engine: LLMEngine, tokenizer, cfg: ServeConfig):
        super().__init__(daemon=True, name="engine-loop")
        self.rt, self.engine, self.tok, self.cfg = runtime, engine, tokenizer, cfg
        self.stop_flag = threading.Event()
        self.error = None
        self.halted = False  # set by the watchdog after it failed every stream: the loop must not touch the engine
        # publish() and the watchdog's halt + [ERROR] publish serialise on this lock, so no token frame of the loop
        # thread can follow a stream's terminal [ERROR] (the loop may be inside publish() when the watchdog fires)
        self.pub_lock = threading.Lock()
        rt = rt_mod.load()
        self._rt = rt
        self._remote = hasattr(runtime, "observe")
        self._ttft, self._itl, self._host = [], [], []
        self._last_obs = 0.0
        # prefix caching (a TP leader wraps the engine): its counters reach /metrics as deltas, the way the TTFT
        # samples do -- straight into the in-process runtime, or with a DP worker's stats message
        self._prefix_cache = bool(getattr(getattr(engine, "engine", engine), "prefix_cache", False))
        self._prefix_seen = [0, 0, 0]
        # host KV tier: its counters travel the same way, and /metrics names them only when the tier is on
        self._offload = getattr(getattr(engine, "engine", engine), "offload", None) is not None
        self._offload_seen = [0, 0, 0, 0]
        # parallel sampling (n > 1): its counters travel the same way, and /metrics names them only once a request
        # with n > 1 was seen (a server that never sees one shows what it always showed)
        self._fork_seen = [0, 0, 0]
        if self._offload and not self._remote:
            rt.observe_kv_offload(0, 0, 0, 0)
        if self._prefix_cache and not self._remote:
            rt.observe_prefix_cache(0, 0, 0)  # /metrics shows the counters from the start
        self.faults = FaultPlan.from_env()
        self.tracer = StepTracer()
        self.last_progress = time.monotonic()
        self.steps = 0
        self.tokenize_errors = 0
        # stop strings are matched where the text exists: on the events this loop publishes (serving/stop_strings.py)
        self.stops = StopMatcher(tokenizer.piece)
        # just-in-time enqueue (LLMEngine.jit_delay): the host work that must fit between polling the requests and
        # the in-flight step's end; DSSE_JIT_MARGIN_MS=0 enqueues every step at once (one queued ahead)
        self.jit_margin_s = float(os.environ.get("DSSE_JIT_MARGIN_MS", "1.5")) / 1e3
        if self._remote:
            engine.on_ttft = self._ttft.append
            engine.on_itl = self._itl.append
        else:
            engine.on_ttft = rt.observe_ttft
            engine.on_itl = rt.observe_itl
        if isinstance(engine, LLMEngine):  # (a TP leader post-processes the events of its step itself)
            engine.on_flush = self._flush

    def _params(self, req) -> SamplingParams:
        d = self.engine.default_params
        return SamplingParams(
            temperature=req["temperature"] if req["temperature"] >= 0 else d.temperature,
            top_p=req["top_p"] if 0 < req["top_p"] <= 1 else d.top_p,
            top_k=req["top_k"] if req["top_k"] > 0 else d.top_k,
            max_tokens=req["max_tokens"] if req["max_tokens"] > 0 else d.max_tokens,
            seed=req["seed"] if req["seed"] >= 0 else None, ignore_eos=bool(req.get("ignore_eos", False)),
            # (range-checked by the HTTP server; a request without them carries the neutral values)
            presence_penalty=float(req.get("presence_penalty", d.presence_penalty)),
            frequency_penalty=float(req.get("frequency_penalty", d.frequency_penalty)),
            repetition_penalty=float(req.get("repetition_penalty", d.repetition_penalty)),
            # -1 = off, else top_logprobs (0..20) of an OpenAI request with logprobs: true
            logprobs=int(req.get("logprobs", -1)),
            # (validated by the HTTP server: <= 300 (id, bias) pairs, <= 16 ids, <= 4 strings)
            logit_bias={int(t): float(b) for t, b in req.get("logit_bias") or ()} or None,
            min_tokens=int(req.get("min_tokens", 0)), stop_token_ids=tuple(int(t) for t in req.get("stop_token_ids") or ()),
            min_p=float(req.get("min_p", 0.0)), stop=tuple(req.get("stop") or ()),
            # guided_regex, or guided_choice lowered to a pattern (compiled once by the HTTP server to validate it)
            guide=req.get("guide") or None,
            guide_schema=bool(req.get("guide_schema")),  # guided_json / response_format json_schema, lowered
            json_object=bool(req.get("guide_json")),  # response_format {"type": "json_object"}
            lora=req.get("lora") or None)  # the adapter "model" named (checked against the loaded names by the server)

    @staticmethod
    def choice_ids(req) -> list:
        """The conversation ids of a request's choices (parallel sampling, n > 1): the id itself for choice 0, then
        f"{id}-c{i}" -- the subjects the HTTP server subscribed to, and the ids the engine derives."""
        conv = req["conversation_id"]
        return [conv] + [f"{conv}-c{i}" for i in range(1, max(1, int(req.get("n", 1))))]

    def _watch_stop(self, req, prompt, params: SamplingParams) -> None:
        """A request with stop strings: its events pass through the matcher from now on (every choice on its own: the
        matcher's state is keyed by conversation id)."""
        if self.stops is not None and params is not None and params.stop:
            n = min(len(prompt), self.engine.r.max_model_len - 1)  # (what the engine keeps of the prompt)
            for conv in self.choice_ids(req):
                self.stops.register(conv, params.stop, min(params.min_tokens, params.max_tokens), n)

    def stop_aborts(self) -> list:
        """Conversations a stop string ended since the last call: the loop aborts them in the engine."""
        if self.stops is None:
            return []
        with self.pub_lock:
            return self.stops.pop_aborts()

    def flow_events(self) -> list:
        """Flow-control transitions from the runtime plus pauses that outlived ``max_pause_s``."""
        ev = list(self.rt.pop_flow_events())
        return ev + [(c, False) for c in self.engine.expired_pauses()]

    def _flush(self, events):
        """Events the engine hands over before it blocks on a drain (LLMEngine.on_flush)."""
        if self.faults.active:
            events = self.faults.filter_events(events)
        self.publish(events)

    def publish(self, events, final: bool = False):
        """Hand events to the runtime.  After the watchdog halted the loop only its own `final` batch goes out."""
        if not events:
            return
        with self.pub_lock:
            if self.halted and not final:
                return
            if self.stops is not None:
                events = self.stops.filter(events)
            if events:
                self._publish(events)

    def _lp_item(self, token_id: int, logprob: float) -> str:
        """{"token": piece, "logprob": f, "bytes": [the piece's UTF-8 bytes]} without the closing brace.  %.9g
        round-trips every fp32; JSON has no -inf: -9999.0, as vLLM writes it."""
        piece = self.tok.piece(token_id)
        lp = format(logprob, ".9g") if logprob > -9999.0 else "-9999.0"
        return f'{{"token":{json.dumps(piece)},"logprob":{lp},"bytes":{json.dumps(list(piece.encode("utf-8")), separators=(",", ":"))}'

    def logprobs_entry(self, e) -> str:
        """The OpenAI `logprobs.content` entry of a token event that carries logprobs ("" otherwise)."""
        if e.logprob is None or e.done:
            return ""
        tops = ",".join(self._lp_item(t, v) + "}" for t, v in (e.top or ()))
        return self._lp_item(e.token_id, e.logprob) + f',"top_logprobs":[{tops}]}}'

    def _publish(self, events):
        args = ([e.conversation_id for e in events], [e.token_id for e in events],
                [e.sequence for e in events], [e.done for e in events], 0,
                [e.text for e in events], [FINISH_CODES.get(e.finish, 0) for e in events],
                [e.prompt_tokens for e in events])
        lps = [self.logprobs_entry(e) for e in events] if any(e.logprob is not None for e in events) else []
        if self._prefix_cache:  # cached_tokens rides beside prompt_tokens on the terminal events
            self.rt.publish_tokens(*args, lps, [getattr(e, "cached_tokens", -1) for e in events])
        elif lps:
            self.rt.publish_tokens(*args, lps)
        else:
            self.rt.publish_tokens(*args)

    def tokenize(self, req):
        """Prompt ids of a queued request, or None after publishing a terminal [ERROR] event for it: a
        conversation the tokenizer / chat template rejects must fail alone, not stop the loop (every other
        live stream of this replica depends on it)."""
        try:
            return prompt_for_request(self.tok, req)
        except Exception as e:  # noqa: BLE001 - any tokenizer / template failure is this request's error
            self.tokenize_errors += 1
            self.publish([TokenEvent(conv, -1, 1, True, text="[ERROR]", timestamp_ns=time.time_ns(),
                                     finish="abort", prompt_tokens=0) for conv in self.choice_ids(req)])
            print(f"[engine] request {req['conversation_id']} rejected by the tokenizer: {e!r}", flush=True)
            return None

    def _take(self, reqs):
        for req in reqs:
            prompt = self.tokenize(req)
            if prompt is not None:
                params = self._params(req)
                self._watch_stop(req, prompt, params)
                n = int(req.get("n", 1))
                if n > 1:  # the choices of one request: one prefill, forked KV pages (LLMEngine.add_request)
                    self.engine.add_request(req["conversation_id"], prompt, params, arrival_ns=req["arrival_ns"], n=n)
                else:
                    self.engine.add_request(req["conversation_id"], prompt, params, arrival_ns=req["arrival_ns"])

    def _jit_wait(self):
        """Wait until the just-in-time deadline (LLMEngine.jit_delay), taking in the requests that arrive meanwhile
        -- tokenized and queued as they come, so the host work left at the deadline is the step's plan and enqueue
        and a prompt that arrives during the wait still rides in the next step."""
        if self.jit_margin_s <= 0:
            return
        t_end = time.perf_counter() + min(self.engine.jit_delay(self.jit_margin_s), 0.05)
        while True:
            left = t_end - time.perf_counter()
            if left < 1e-3:  # the poll's timeout has millisecond granularity
                if left > 0:
                    time.sleep(left)
                return
            self._take(self.rt.poll_requests(256, int(left * 1e3)))

    def _observe(self):
        e = self.engine
        running, free = float(e.num_running()), float(e.alloc.num_free)
        host = e.stats.get("host_s", -1.0)
        if not self._remote:
            self._rt.engine_observe(e.stats["last_step_s"], running, free, host)
            self._rt.set_active_chats(running + len(e.waiting))
            if self._prefix_cache:
                d = self._prefix_delta()
                if any(d):
                    self._rt.observe_prefix_cache(*d)
            if self._offload:
                d = self._offload_delta()
                if any(d):
                    self._rt.observe_kv_offload(*d)
            d = self._fork_delta()
            if any(d):
                self._rt.observe_parallel_sampling(*d)
            return
        if host >= 0:
            self._host.append(host)
        now = time.monotonic()
        if now - self._last_obs < 0.05 and len(self._itl) < 4096 and len(self._host) < 4096:
            return  # batch the observations: one stats message per ~50 ms
        self._last_obs = now
        ttft, itl, hs = self._ttft[:], self._itl[:], self._host[:]
        self._ttft.clear()
        self._itl.clear()
        self._host.clear()
        prefix = self._prefix_delta() + (self._offload_delta() if self._offload else []) if self._prefix_cache else []
        fork = self._fork_delta()
        if any(fork):  # (a replica that has seen a request with n > 1: its counters ride behind the prefix cache's)
            self.rt.observe(e.stats["last_step_s"], running, free, running + len(e.waiting), ttft, itl, hs, prefix, fork)
        elif self._prefix_cache:
            self.rt.observe(e.stats["last_step_s"], running, free, running + len(e.waiting), ttft, itl, hs, prefix)
        else:
            self.rt.observe(e.stats["last_step_s"], running, free, running + len(e.waiting), ttft, itl, hs)

    def _prefix_delta(self) -> list:
        """[queries, hits (prompt tokens), evictions (pages)] of the engine's prefix cache since the last call."""
        st = self.engine.stats
        now = [st.get("prefix_queries", 0), st.get("prefix_hit_tokens", 0), st.get("prefix_evictions", 0)]
        d = [float(a - b) for a, b in zip(now, self._prefix_seen)]
        self._prefix_seen = now
        return d

    def _fork_delta(self) -> list:
        """[requests with n > 1, prompt tokens their siblings did not prefill, tail pages copied] since the last call."""
        st = self.engine.stats
        now = [st.get("fork_requests", 0), st.get("fork_shared_tokens", 0), st.get("fork_tail_copies", 0)]
        d = [float(a - b) for a, b in zip(now, self._fork_seen)]
        self._fork_seen = now
        return d

    def _offload_delta(self) -> list:
        """[spilled, restored, dropped (pages), host-tier hit tokens] of the engine's host KV tier since the last call."""
        st = self.engine.stats
        now = [st.get(k, 0) for k in ("offload_spilled_pages", "offload_restored_pages", "offload_dropped_pages",
                                      "offload_hit_tokens")]
        d = [float(a - b) for a, b in zip(now, self._offload_seen)]
        self._offload_seen = now
        return d

    def _shutdown(self) -> bool:
        f = getattr(self.rt, "shutdown_requested", None)
        return bool(f and f())

    def run(self):
        # Everything allocated so far (weights, graphs, runtime objects) moves to the permanent generation:
        # the per-step objects of the loop then never make a full collection walk the whole heap (those
        # pauses showed up as 0.5 ms gaps between decode graphs at 256 streams).
        import gc

        gc.collect()
        gc.freeze()
        try:
            while not self.stop_flag.is_set() and not self._shutdown() and not self.halted:
                busy = self.engine.runnable()
                # only paused streams left: wait briefly so their resume events get through
                wait = 0 if busy else (2 if self.engine.has_work() else 20)
                self._take(self.rt.poll_requests(256, wait))
                for conv in self.rt.pop_cancellations():
                    self.engine.abort(conv)
                for conv in self.stop_aborts():  # a stop string ends the choice it matched in, not its siblings
                    self.engine.abort(conv, choices=False)
                for conv, paused in self.flow_events():
                    self.engine.set_paused(conv, paused)
                if not self.engine.runnable():
                    self.last_progress = time.monotonic()
                    continue
                self.tracer.begin(self.steps)
                t0 = time.perf_counter()
                events = self.engine.step()
                if self.halted:  # the watchdog ended every stream while this step was blocked
                    break
                if self.faults.active:
                    events = self.faults.filter_events(events)
                self.publish(events)
                self.tracer.end(self.steps, self.engine, events, time.perf_counter() - t0)
                self.steps += 1
                self.last_progress = time.monotonic()
                self._observe()
                if self.faults.active:
                    self.faults.after_step(self.engine)
                # just-in-time enqueue: plan the next step as late as the in-flight step allows (TTFT)
                self._jit_wait()
        except EngineFault as e:
            # untrusted device state: every live stream ends with [ERROR] now, readiness drops, the process exits
            # non-zero through serve_forever (the orchestrator restarts it; nothing re-execs in this process)
            self.error = e
            self.rt.set_ready(False)
            print(f"[engine] FAULT: {e}; ending {self.engine.num_running() + len(self.engine.waiting)} streams",
                  flush=True)
            self.publish(self.engine.fail_all())
            raise
        except Exception as e:  # noqa: BLE001 - surfaced to the operator, readiness drops
            self.error = e
            self.rt.set_ready(False)
            raise
        finally:
            self.tracer.close()


class ServingApp:
    def __init__(self, cfg: ServeConfig, device=None, comm=None):
        self.cfg = cfg
        mod = rt_mod.load()
        rd = cfg.runtime_dict()
        rd["local_engine"] = cfg.engine in ("gpu", "cpu", "stub")
        self.rt = mod.Runtime(rd)
        self.loop = None
        self.watchdog = None
        self.engine = None
        self.tok = None
        if cfg.engine in ("gpu", "cpu"):
            self.rt.set_ready(False)
            self.engine, self.tok = build_engine(cfg, device=device, comm=comm)
            self.rt.set_vocab(self.tok.pieces())

    def start(self):
        self.rt.start()
        if self.cfg.engine == "stub":
            self.rt.start_stub(self.cfg.stub_tokens, self.cfg.stub_token_delay_ms, 2)
        elif self.engine is not None:
            self.loop = EngineLoop(self.rt, self.engine, self.tok, self.cfg)
            self.loop.start()
            self.rt.set_ready(True)
            self.watchdog = Watchdog(self.loop, self.rt.set_ready)
            self.watchdog.start()
        return self

    def port(self, role: str) -> int:
        return self.rt.bound_port(role)

    def stop(self):
        if self.watchdog is not None:
            self.watchdog.stop()
        if self.loop is not None:
            self.loop.stop_flag.set()
            self.loop.join(timeout=10)
        self.rt.stop()
        if self.engine is not None and (self.loop is None or not self.loop.is_alive()):
            self.engine.r.close()  # TP: unmap the IPC all-reduce peers' buffers

    def serve_forever(self):
        try:
            while True:
                time.sleep(0.5)
                if self.loop is not None and not self.loop.is_alive():
                    if isinstance(self.loop.error, EngineFault):
                        time.sleep(0.5)  # let the I/O threads write the [ERROR] frames already on the bus
                    raise RuntimeError(f"engine loop died: {self.loop.error!r}")
        except KeyboardInterrupt:
            pass
        finally:
            self.stop()
