"""Typed configuration honouring the reference's environment variables.

Reference keys (same names, same defaults where they apply here):
  SSE_PORT=8080 METRICS_PORT=9090 (sse-adapter, src/sse-adapter/main.go:29-40), PORT / ORIGIN_PORT
  (llm-stream-proxy, src/llm-stream-proxy/main.go:70-96; the origin gets its own port because both
  services default to 8080 and they now share a process), LLM_PROXY_URL, INSPECTION_MODE,
  INSPECTION_BUFFER_MS, LOG_LEVEL, MODEL_NAME, REDIS_ADDR (the RESP ingest port, e.g. ":6379").
Topology keys (new): UPSTREAM_URL (edge: relay conversations from the origin), UI_PATH.
Flow control (new): FLOW_HIGH_WATER (bytes queued for every subscriber of a conversation before its decode
  pauses; 0 = off), MAX_PAUSE_S (a paused stream resumes after this long regardless).
Engine keys (new): TP, DP, DP_PREFIX, DP_WORKER_TIMEOUT_MS, MAX_MODEL_LEN, MAX_BATCH, KV_BLOCK (fixed 32), GPU_MEMORY_UTILIZATION,
  SEED, MAX_TOKENS, PREFILL_BUDGET, TOKENIZER_PATH, WEIGHTS_PATH, ENABLE_PREFIX_CACHING (default 0),
  DP_PREFIX_AFFINITY_SLACK (default 4, unmeasured), KV_CACHE_DTYPE (auto | bf16 | fp8 | fp8_e4m3; default auto = bf16),
  KV_OFFLOAD_GB (GiB of pinned host memory per engine process behind the prefix cache; default 0 = off),
  QUANTIZATION (none | fp8 | mxfp4; default none; fp8 = FP8 e4m3 weights, mxfp4 = OCP MXFP4 weights, either for decode
  buckets of 64 rows or fewer, TP = 1),
  ENABLE_LORA (default 0), LORA_MODULES (comma-separated NAME=PATH of PEFT directories), MAX_LORAS (slots, default 4,
  at most 8), MAX_LORA_RANK (8 | 16 | 32 | 64, default 16); TP = 1 and bf16 weights only.
"""
from __future__ import annotations

import argparse
import os
from dataclasses import asdict, dataclass, fields


# the one list of KV cache element types (engine/kv_cache.py imports it; kept here: no torch import at parse time)
KV_CACHE_DTYPES = ("auto", "bf16", "fp8", "fp8_e4m3")


def parse_kv_cache_dtype(v) -> str:
    """The option as typed (lower-cased); a value outside the choices is a start-up error that names them."""
    key = str(v).strip().lower()
    if key not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache_dtype / KV_CACHE_DTYPE must be one of {', '.join(KV_CACHE_DTYPES)}; got {v!r}")
    return key


# weight quantisation at load (engine/weights.py keeps its own copy of the list: no torch import at parse time)
QUANTIZATIONS = ("none", "fp8", "mxfp4")


def parse_quantization(v) -> str:
    """The option as typed (lower-cased); a value outside the choices is a start-up error that names them."""
    key = str(v).strip().lower()
    if key not in QUANTIZATIONS:
        raise ValueError(f"quantization / QUANTIZATION must be one of {', '.join(QUANTIZATIONS)}; got {v!r}")
    return key


# LoRA pool limits (engine/lora.py and ops keep their own copies: no torch import at parse time)
LORA_RANKS = (8, 16, 32, 64)
LORA_MAX_SLOTS = 8


def parse_lora_modules(v) -> dict:
    """"NAME=PATH,NAME=PATH" (or a list of NAME=PATH) -> {name: path} in order; a malformed or repeated entry is a
    start-up error."""
    items = [s.strip() for s in v.split(",")] if isinstance(v, str) else [str(s).strip() for s in (v or ())]
    out = {}
    for it in items:
        if not it:
            continue
        name, sep, path = it.partition("=")
        if not sep or not name or not path:
            raise ValueError(f"--lora-modules / LORA_MODULES entries are NAME=PATH; got {it!r}")
        if name in out:
            raise ValueError(f"--lora-modules / LORA_MODULES names adapter {name!r} twice")
        out[name] = path
    return out


def _env(name, default, cast=str):
    v = os.environ.get(name)
    if v is None or v == "":
        return default
    if cast is bool:
        return v.lower() in ("1", "true", "yes", "on")
    return cast(v)


@dataclass
class ServeConfig:
    # delivery (reference sse-adapter / proxy)
    host: str = "0.0.0.0"
    sse_port: int = 8080
    origin_port: int = 8081
    metrics_port: int = 9090
    resp_port: int = -1
    io_threads: int = 4
    llm_proxy_url: str = ""
    upstream_url: str = ""       # edge: origin SSE endpoint to relay conversations from (csrc/runtime/relay.h)
    ui_path: str = ""            # chat page served at GET / ("" = the built-in page, "none" = off)
    inspection_mode: str = "disabled"
    inspection_buffer_ms: int = 150
    inspection_endpoint: str = ""  # remote inspector URL (POST /inspect of the reference's Spin function)
    inspection_timeout_ms: int = 250
    inspection_fail_open: int = 0  # 1: a failed / overloaded inline inspector delivers uninspected (default: [ERROR])
    dedupe_window_s: int = 30      # bus duplicate window (the bridge's DEDUPE_WINDOW_SEC; 0 = off)
    log_level: str = "info"
    model_name: str = "mistralai/Mistral-7B-Instruct-v0.3"
    keepalive_ms: int = 15000
    first_token_timeout_ms: int = 30000
    flow_high_water: int = 256 << 10   # per-conversation backpressure (csrc/runtime/server.h)
    max_pause_s: float = 30.0
    # engine
    engine: str = "gpu"          # gpu | cpu (tiny reference-op model) | stub (C++ token generator)
    model: str = "mistral-7b-v0.3"
    tp: int = 1
    dp: int = 1
    max_model_len: int = 4096
    max_batch: int = 256  # decode slots (captured buckets 1..64 by powers of two, then every 64); KV pages are lazy
    gpu_memory_utilization: float = 0.85
    seed: int = 0
    max_tokens: int = 256
    temperature: float = 1.0
    prefill_budget: int = 512
    tokenizer_path: str = ""
    weights_path: str = ""
    stub_tokens: int = 50
    stub_token_delay_ms: int = 50
    dp_prefix: str = ""          # shared-memory ring name prefix of a DP group (default from MASTER_PORT)
    dp_worker_timeout_ms: int = 10000
    # automatic prefix caching (engine/kv_cache.py): off by default; passed to every engine replica
    enable_prefix_caching: bool = False
    # DP router: a chat's affine replica wins while its outstanding count is at most the least one plus this slack
    # (only with prefix caching on; the default is a guess nobody has measured)
    dp_prefix_affinity_slack: int = 4
    # KV cache element type: auto = bf16 (128 KiB per token at TP = 1), fp8 = fp8_e4m3 (64 KiB per token, twice the
    # pages in the same budget); passed to every engine replica / TP rank
    kv_cache_dtype: str = "auto"
    # host tier of the prefix cache: GiB of pinned host memory per engine process that keep evicted KV pages (0 = off;
    # needs enable_prefix_caching, not available with tp > 1); passed to every engine replica
    kv_offload_gb: float = 0.0
    # weight quantisation at load: none, fp8 = W8A16 e4m3 weights or mxfp4 = W4A16 OCP MXFP4 weights (e2m1 elements,
    # one e8m0 scale per 32 K), either for decode buckets of 64 rows or fewer beside a widened bf16 copy for everything
    # else (not available with tp > 1); passed to every engine replica
    quantization: str = "none"
    # LoRA serving (engine/lora.py): every NAME=PATH of lora_modules (comma-separated) is loaded into one of max_loras
    # pool slots of rank max_lora_rank at start-up; "model": NAME of a chat request then selects it.  TP = 1, bf16
    # weights; passed to every engine replica
    enable_lora: bool = False
    lora_modules: str = ""
    max_loras: int = 4
    max_lora_rank: int = 16

    @classmethod
    def from_env(cls) -> "ServeConfig":
        c = cls()
        c.sse_port = _env("SSE_PORT", c.sse_port, int)
        c.metrics_port = _env("METRICS_PORT", c.metrics_port, int)
        c.origin_port = _env("ORIGIN_PORT", _env("PORT", c.origin_port, int), int)
        redis = _env("REDIS_ADDR", "")
        if redis and ":" in redis and redis.rsplit(":", 1)[0] in ("", "0.0.0.0", "localhost", "127.0.0.1"):
            c.resp_port = int(redis.rsplit(":", 1)[1])
        c.resp_port = _env("RESP_PORT", c.resp_port, int)
        c.io_threads = _env("IO_THREADS", c.io_threads, int)
        c.llm_proxy_url = _env("LLM_PROXY_URL", c.llm_proxy_url)
        c.upstream_url = _env("UPSTREAM_URL", c.upstream_url)
        c.ui_path = _env("UI_PATH", c.ui_path)
        c.flow_high_water = _env("FLOW_HIGH_WATER", c.flow_high_water, int)
        c.max_pause_s = _env("MAX_PAUSE_S", c.max_pause_s, float)
        c.inspection_mode = _env("INSPECTION_MODE", c.inspection_mode)
        c.inspection_buffer_ms = _env("INSPECTION_BUFFER_MS", c.inspection_buffer_ms, int)
        c.inspection_endpoint = _env("INSPECTION_ENDPOINT", c.inspection_endpoint)
        c.inspection_timeout_ms = _env("INSPECTION_TIMEOUT_MS", c.inspection_timeout_ms, int)
        c.inspection_fail_open = _env("INSPECTION_FAIL_OPEN", c.inspection_fail_open, int)
        c.dedupe_window_s = _env("DEDUPE_WINDOW_SEC", c.dedupe_window_s, int)
        c.log_level = _env("LOG_LEVEL", c.log_level)
        c.model_name = _env("MODEL_NAME", c.model_name)
        c.engine = _env("ENGINE", c.engine)
        c.model = _env("MODEL", c.model)
        c.tp = _env("TP", c.tp, int)
        c.dp = _env("DP", c.dp, int)
        c.max_model_len = _env("MAX_MODEL_LEN", c.max_model_len, int)
        c.max_batch = _env("MAX_BATCH", c.max_batch, int)
        c.gpu_memory_utilization = _env("GPU_MEMORY_UTILIZATION", c.gpu_memory_utilization, float)
        c.seed = _env("SEED", c.seed, int)
        c.max_tokens = _env("MAX_TOKENS", c.max_tokens, int)
        c.temperature = _env("TEMPERATURE", c.temperature, float)
        c.prefill_budget = _env("PREFILL_BUDGET", c.prefill_budget, int)
        c.tokenizer_path = _env("TOKENIZER_PATH", c.tokenizer_path)
        c.weights_path = _env("WEIGHTS_PATH", c.weights_path)
        c.stub_tokens = _env("STUB_TOKENS", c.stub_tokens, int)
        c.stub_token_delay_ms = _env("STUB_TOKEN_DELAY_MS", c.stub_token_delay_ms, int)
        c.dp_prefix = _env("DP_PREFIX", c.dp_prefix)
        c.dp_worker_timeout_ms = _env("DP_WORKER_TIMEOUT_MS", c.dp_worker_timeout_ms, int)
        c.enable_prefix_caching = _env("ENABLE_PREFIX_CACHING", c.enable_prefix_caching, bool)
        c.dp_prefix_affinity_slack = _env("DP_PREFIX_AFFINITY_SLACK", c.dp_prefix_affinity_slack, int)
        c.kv_cache_dtype = _env("KV_CACHE_DTYPE", c.kv_cache_dtype, parse_kv_cache_dtype)
        c.kv_offload_gb = _env("KV_OFFLOAD_GB", c.kv_offload_gb, float)
        c.quantization = _env("QUANTIZATION", c.quantization, parse_quantization)
        c.enable_lora = _env("ENABLE_LORA", c.enable_lora, bool)
        c.lora_modules = _env("LORA_MODULES", c.lora_modules)
        c.max_loras = _env("MAX_LORAS", c.max_loras, int)
        c.max_lora_rank = _env("MAX_LORA_RANK", c.max_lora_rank, int)
        return c

    @classmethod
    def add_args(cls, ap: argparse.ArgumentParser):
        for f in fields(cls):
            if isinstance(f.default, bool):  # a switch: --enable-prefix-caching
                ap.add_argument("--" + f.name.replace("_", "-"), action="store_const", const=True, default=None)
                continue
            if f.name == "kv_cache_dtype":  # --help lists the choices; a bad value is a usage error that names them
                ap.add_argument("--kv-cache-dtype", type=str.lower, choices=KV_CACHE_DTYPES, default=None)
                continue
            if f.name == "quantization":
                ap.add_argument("--quantization", type=str.lower, choices=QUANTIZATIONS, default=None)
                continue
            if f.name == "lora_modules":  # --lora-modules a=/path/a b=/path/b
                ap.add_argument("--lora-modules", nargs="+", metavar="NAME=PATH", default=None)
                continue
            ap.add_argument("--" + f.name.replace("_", "-"), type=type(f.default) if f.default is not None else str,
                            default=None)

    def update_from_args(self, ns: argparse.Namespace) -> "ServeConfig":
        for f in fields(self):
            v = getattr(ns, f.name, None)
            if v is not None:
                setattr(self, f.name, ",".join(v) if f.name == "lora_modules" and not isinstance(v, str) else v)
        self.kv_cache_dtype = parse_kv_cache_dtype(self.kv_cache_dtype)
        self.quantization = parse_quantization(self.quantization)
        return self.validate()

    def validate(self) -> "ServeConfig":
        """Start-up errors of option combinations, each naming the fix (the CLI calls it once flags and environment
        are merged; build_engine calls it again for configs built in code)."""
        if self.kv_offload_gb < 0:
            raise ValueError(f"--kv-offload-gb / KV_OFFLOAD_GB must be >= 0 (0 = off), got {self.kv_offload_gb}")
        if self.kv_offload_gb > 0:
            if not self.enable_prefix_caching:
                raise ValueError("--kv-offload-gb / KV_OFFLOAD_GB needs the prefix cache: add --enable-prefix-caching "
                                 "(ENABLE_PREFIX_CACHING=1), or set it to 0")
            if self.tp > 1:
                raise ValueError(f"--kv-offload-gb / KV_OFFLOAD_GB is not supported with tensor parallelism (tp = "
                                 f"{self.tp}): run with --tp 1 (data parallelism, --dp N, works: every replica has its "
                                 "own host tier), or set it to 0")
        if parse_quantization(self.quantization) != "none" and self.tp > 1:
            raise ValueError(f"--quantization {self.quantization} / QUANTIZATION is not supported with tensor "
                             f"parallelism (tp = {self.tp}): the {'block' if self.quantization == 'mxfp4' else 'row'} "
                             "scales are not sharded; run with --tp 1 (data parallelism, --dp N, works), or set it "
                             "to none")
        mods = parse_lora_modules(self.lora_modules)
        if mods and not self.enable_lora:
            raise ValueError("--lora-modules / LORA_MODULES needs --enable-lora (ENABLE_LORA=1)")
        if self.enable_lora:
            if self.tp > 1:
                raise ValueError(f"--enable-lora / ENABLE_LORA is not supported with tensor parallelism (tp = {self.tp}): "
                                 "the adapters are not sharded; run with --tp 1 (data parallelism, --dp N, works)")
            if parse_quantization(self.quantization) != "none":
                raise ValueError(f"--enable-lora / ENABLE_LORA is not supported with --quantization "
                                 f"{self.quantization}: the {'MXFP4' if self.quantization == 'mxfp4' else 'FP8'} decode kernels "
                                 "cannot take a delta; set it to none")
            if not 1 <= int(self.max_loras) <= LORA_MAX_SLOTS:
                raise ValueError(f"--max-loras / MAX_LORAS must be in [1, {LORA_MAX_SLOTS}], got {self.max_loras}")
            if int(self.max_lora_rank) not in LORA_RANKS:
                raise ValueError(f"--max-lora-rank / MAX_LORA_RANK must be one of {', '.join(map(str, LORA_RANKS))}, "
                                 f"got {self.max_lora_rank}")
            if len(mods) > int(self.max_loras):
                raise ValueError(f"{len(mods)} --lora-modules for --max-loras {self.max_loras} slots: every adapter is "
                                 f"loaded at start-up (no eviction); raise --max-loras (at most {LORA_MAX_SLOTS})")
            if self.model_name in mods:
                raise ValueError(f"--lora-modules names an adapter {self.model_name!r}, the served model's own name")
        return self

    def lora_names(self) -> list:
        """The adapters' names, in slot order ([] with LoRA off)."""
        return list(parse_lora_modules(self.lora_modules)) if self.enable_lora else []

    def to_json(self) -> str:
        import json

        return json.dumps(asdict(self))

    @classmethod
    def from_json(cls, s: str) -> "ServeConfig":
        import json

        return cls(**json.loads(s))

    def runtime_dict(self) -> dict:
        d = asdict(self)
        keys = ("host", "sse_port", "origin_port", "metrics_port", "resp_port", "io_threads", "llm_proxy_url",
                "upstream_url", "inspection_mode", "inspection_buffer_ms", "inspection_endpoint",
                "inspection_timeout_ms", "inspection_fail_open", "dedupe_window_s", "model_name", "keepalive_ms",
                "first_token_timeout_ms", "flow_high_water")
        out = {k: d[k] for k in keys}
        # `n` of POST /v1/chat/completions: at most 16 choices, and no more than the engine has decode slots (the CPU
        # engine is built with min(MAX_BATCH, 8): serving/app.py build_engine)
        slots = min(self.max_batch, 8) if self.engine == "cpu" else self.max_batch
        out["max_choices"] = max(1, min(16, int(slots)))
        out["enable_lora"] = bool(self.enable_lora)
        out["lora_names"] = self.lora_names()
        if self.ui_path != "none":
            from pathlib import Path

            p = Path(self.ui_path) if self.ui_path else Path(__file__).with_name("static") / "chat.html"
            if p.exists():
                out["ui_html"] = p.read_text()
        return out
