"""--kv-cache-dtype / KV_CACHE_DTYPE through the serving stack on CPU: the option reaches the engine of the process,
both chat routes stream to [DONE] on an fp8 cache, and nothing of it shows on /metrics or /health -- with ``auto``
the serving surface is what it was."""
import json
from pathlib import Path

from distributed_sse_for_llm_response_amd.serving.app import ServingApp
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from distributed_sse_for_llm_response_amd.utils.sse_client import request

H = "127.0.0.1"
# The parent commit's /metrics after this file's traffic on the CPU engine (`_traffic`, ServeConfig of `_cfg`), recorded
# by serving it there: every series (name + label set; values differ from run to run), the # HELP / # TYPE lines
# and the /health body.
PARENT = json.loads((Path(__file__).parent / "golden" / "kv_fp8_parent_metrics.json").read_text())


def _cfg(**kw):
    c = ServeConfig(host=H, sse_port=0, origin_port=0, metrics_port=0, resp_port=0, io_threads=2, engine="cpu",
                    max_tokens=8, temperature=0.0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _traffic(app):
    r = request(H, app.port("edge"), "POST", "/chat", {"message": "Why stream tokens?", "max_tokens": 6}, timeout=60)
    assert r.status == 200
    toks = [e.json() for e in r.events if e.event == "token"]
    assert toks[-1]["done"] and toks[-1]["token"] == "[DONE]" and 1 <= len(toks) - 1 <= 6
    s = request(H, app.port("origin"), "POST", "/v1/chat/completions",
                {"messages": [{"role": "user", "content": "and fp8?"}], "max_tokens": 5, "stream": True}, timeout=60)
    assert s.status == 200
    lines = [ln for ln in s.body.decode().splitlines() if ln.startswith("data: ")]
    assert lines[-1] == "data: [DONE]"
    chunks = [json.loads(ln[6:]) for ln in lines[:-1]]
    assert chunks[-1]["choices"][0]["finish_reason"] in ("length", "stop")
    return len(toks) - 1


def _metric_names(app):
    """/metrics as the parent's record holds it: (series without values, # lines), and the raw text."""
    text = request(H, app.port("metrics"), "GET", "/metrics").body.decode()
    series = sorted({ln.rsplit(" ", 1)[0] for ln in text.splitlines() if ln and not ln.startswith("#")})
    return (series, sorted(ln for ln in text.splitlines() if ln.startswith("#"))), text


def test_auto_serves_on_bf16_and_fp8_adds_nothing_to_metrics_or_health(monkeypatch, capsys):
    monkeypatch.delenv("KV_CACHE_DTYPE", raising=False)
    assert ServeConfig.from_env().kv_cache_dtype == "auto"
    app = ServingApp(_cfg()).start()
    try:
        assert app.engine.kv_cache_dtype == "bf16"
        _traffic(app)
        names_auto, text = _metric_names(app)
        health_auto = request(H, app.port("origin"), "GET", "/health").body
        # with auto, /metrics is the parent's for the same traffic: the same series, HELP and TYPE lines; /health too
        assert names_auto[0] == PARENT["series"] and names_auto[1] == PARENT["meta"]
        assert health_auto.decode() == PARENT["health_body"]
        assert "kv_cache" not in text and "fp8" not in text and b"fp8" not in health_auto
    finally:
        app.stop()
    assert "[engine] KV cache: bf16 (auto), " in capsys.readouterr().out

    monkeypatch.setenv("KV_CACHE_DTYPE", "fp8")
    cfg = ServeConfig.from_env()
    assert cfg.kv_cache_dtype == "fp8"
    app = ServingApp(_cfg(kv_cache_dtype=cfg.kv_cache_dtype)).start()
    try:
        assert app.engine.kv_cache_dtype == "fp8_e4m3" and app.engine.r.kv.is_fp8
        _traffic(app)
        names_fp8, _ = _metric_names(app)
        assert names_fp8 == names_auto  # the same lines for the same traffic: the dtype is not a metric
        assert request(H, app.port("origin"), "GET", "/health").body == health_auto
    finally:
        app.stop()
    out = capsys.readouterr().out
    assert "[engine] KV cache: fp8_e4m3 (fp8), " in out and "KiB per token" in out and "pages of 32 tokens" in out
