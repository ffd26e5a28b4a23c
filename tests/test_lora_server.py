"""LoRA through the real server on the CPU engine: /v1/models lists the adapters, "model" selects one and is echoed,
an unknown model is vLLM's 404, /chat takes "model", concurrent streams on different adapters equal their solo runs,
n = 2 under an adapter, the per-adapter metric, and the start-up refusals.  Without LoRA any model string is echoed."""
import json
import threading

import pytest

from lora_common import write_adapter

from distributed_sse_for_llm_response_amd.models.mistral import TINY
from distributed_sse_for_llm_response_amd.serving.app import ServingApp
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from distributed_sse_for_llm_response_amd.utils.sse_client import request

H = "127.0.0.1"
MSG = [{"role": "user", "content": "Why stream tokens one by one?"}]
BASE = "mistralai/Mistral-7B-Instruct-v0.3"


def _cfg(**kw):
    return ServeConfig(host=H, sse_port=0, origin_port=0, metrics_port=0, resp_port=0, io_threads=2, engine="cpu",
                       max_tokens=8, temperature=0.0, **kw)


@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapters")
    # b_std 0.05 at alpha = 2 r: deltas about 0.4 of a weight's scale, so the greedy streams differ from the base's
    return {"a": write_adapter(d / "a", TINY, 40, r=4), "b": write_adapter(d / "b", TINY, 41, r=8)}


@pytest.fixture(scope="module")
def app(adapters):
    mods = ",".join(f"{k}={v}" for k, v in adapters.items())
    a = ServingApp(_cfg(enable_lora=True, lora_modules=mods, max_loras=2, max_lora_rank=8)).start()
    try:
        yield a
    finally:
        a.stop()


def _post(app, body, path="/v1/chat/completions", role="origin"):
    return request(H, app.port(role), "POST", path, body, timeout=120)


def _text(app, model, **kw):
    body = {"messages": MSG, "max_tokens": 8, "temperature": 0.0, **kw}
    if model is not None:
        body["model"] = model
    r = _post(app, body)
    assert r.status == 200, r.body
    return json.loads(r.body)


def test_models_lists_the_adapters_with_their_parent(app):
    d = json.loads(request(H, app.port("origin"), "GET", "/v1/models").body)
    assert [(m["id"], m["parent"]) for m in d["data"]] == [(BASE, None), ("a", BASE), ("b", BASE)]
    assert all(m["object"] == "model" for m in d["data"])


def test_model_selects_the_adapter_and_is_echoed(app):
    base, none = _text(app, BASE), _text(app, None)
    a, b = _text(app, "a"), _text(app, "b")
    assert (base["model"], none["model"], a["model"], b["model"]) == (BASE, BASE, "a", "b")
    texts = [d["choices"][0]["message"]["content"] for d in (base, none, a, b)]
    assert texts[0] == texts[1] and len({texts[0], texts[2], texts[3]}) == 3
    assert app.engine.r.lora_used
    assert _text(app, "a")["choices"][0]["message"]["content"] == texts[2]  # and base rows after it are unchanged:
    assert _text(app, BASE)["choices"][0]["message"]["content"] == texts[0]
    s = _post(app, {"messages": MSG, "max_tokens": 4, "temperature": 0.0, "model": "b", "stream": True})
    chunks = [json.loads(ln[6:]) for ln in s.body.decode().splitlines() if ln.startswith("data: {")]
    assert chunks and all(c["model"] == "b" for c in chunks)


def test_unknown_model_is_404_model_not_found(app):
    r = _post(app, {"messages": MSG, "model": "nope"})
    assert r.status == 404
    d = json.loads(r.body)
    assert d["message"] == "The model `nope` does not exist." and d["code"] == "model_not_found"
    assert d["object"] == "error" and d["type"] == "NotFoundError"


def test_chat_route_accepts_model(app):
    before = app.engine.lora_requests.get("b", 0)
    r = _post(app, {"message": "hello", "model": "b", "max_tokens": 3}, path="/chat")
    assert r.status == 200 and json.loads(r.body)["status"] == "streaming"
    assert _post(app, {"message": "hello", "model": "nope"}, path="/chat").status == 404
    assert _post(app, {"message": "hello", "model": BASE, "max_tokens": 2}, path="/chat").status == 200
    for _ in range(200):
        if app.engine.lora_requests.get("b", 0) > before and not app.engine.has_work():
            break
        threading.Event().wait(0.05)
    assert app.engine.lora_requests["b"] == before + 1  # the engine saw the adapter
    text = request(H, app.port("metrics"), "GET", "/metrics").body.decode()
    assert 'lora_requests_total{adapter="b"}' in text and 'adapter="nope"' not in text


def test_concurrent_streams_on_different_adapters_equal_their_solo_runs(app):
    solo = {m: _text(app, m, max_tokens=12)["choices"][0]["message"]["content"] for m in ("a", "b", BASE)}
    got = {}

    def run(m):
        got[m] = _text(app, m, max_tokens=12)["choices"][0]["message"]["content"]

    ts = [threading.Thread(target=run, args=(m,)) for m in solo]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert got == solo and len(set(solo.values())) == 3


_N2 = """
import json, sys
from distributed_sse_for_llm_response_amd.serving.app import ServingApp
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from distributed_sse_for_llm_response_amd.utils.sse_client import request
a = ServingApp(ServeConfig(host="127.0.0.1", sse_port=0, origin_port=0, metrics_port=0, resp_port=0, io_threads=2,
                           engine="cpu", max_tokens=8, temperature=0.0, enable_lora=True, lora_modules=sys.argv[1],
                           max_loras=2, max_lora_rank=8)).start()
try:
    out = []
    for n in (2, 1):
        r = request("127.0.0.1", a.port("origin"), "POST", "/v1/chat/completions",
                    {"messages": [{"role": "user", "content": "Why stream tokens one by one?"}], "max_tokens": 8,
                     "temperature": 0.0, "model": "a", "n": n}, timeout=120)
        assert r.status == 200, r.body
        out.append(json.loads(r.body))
    print("RESULT " + json.dumps(out))
finally:
    a.stop()
"""


def test_n2_under_an_adapter(adapters):
    """In a process of its own: the runtime's metrics are one per process, and tests/test_parallel_sampling_server.py
    compares the n > 1 counters of /metrics with its own engine's."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mods = ",".join(f"{k}={v}" for k, v in adapters.items())
    r = subprocess.run([sys.executable, "-c", _N2, mods], capture_output=True, text=True, timeout=300, cwd=root,
                       env={**os.environ, "PYTHONPATH": root})
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
    d, one = json.loads(line[7:])
    one = one["choices"][0]["message"]["content"]
    assert d["model"] == "a" and [c["index"] for c in d["choices"]] == [0, 1]
    assert [c["message"]["content"] for c in d["choices"]] == [one, one]  # greedy: both are the adapter's stream


def test_without_lora_any_model_string_is_echoed():
    a = ServingApp(_cfg()).start()
    try:
        d = _text(a, "whatever-you-like")
        assert d["model"] == "whatever-you-like"
        assert _text(a, None)["model"] == BASE and not a.engine.r.lora_used and a.engine.r.lora is None
        m = json.loads(request(H, a.port("origin"), "GET", "/v1/models").body)
        assert [x["id"] for x in m["data"]] == [BASE]
    finally:
        a.stop()


def test_start_up_refusals(adapters, tmp_path):
    mods = ",".join(f"{k}={v}" for k, v in adapters.items())
    with pytest.raises(ValueError, match="tensor parallelism"):
        _cfg(enable_lora=True, lora_modules=mods, tp=2).validate()
    with pytest.raises(ValueError, match="quantization"):
        _cfg(enable_lora=True, lora_modules=mods, quantization="fp8").validate()
    with pytest.raises(ValueError, match="2 --lora-modules for --max-loras 1"):
        _cfg(enable_lora=True, lora_modules=mods, max_loras=1).validate()
    with pytest.raises(ValueError, match="needs --enable-lora"):
        _cfg(lora_modules=mods).validate()
    with pytest.raises(ValueError, match="MAX_LORA_RANK"):
        _cfg(enable_lora=True, max_lora_rank=12).validate()
    big = write_adapter(tmp_path / "big", TINY, 9, r=16)
    with pytest.raises(ValueError, match=r"adapter_config\.json: rank r = 16 exceeds max_lora_rank = 8"):
        ServingApp(_cfg(enable_lora=True, lora_modules=f"big={big}", max_lora_rank=8))


def test_flags_and_environment(monkeypatch, adapters):
    import argparse

    ap = argparse.ArgumentParser()
    ServeConfig.add_args(ap)
    ns = ap.parse_args(["--enable-lora", "--lora-modules", f"a={adapters['a']}", f"b={adapters['b']}", "--max-loras",
                        "3", "--max-lora-rank", "32"])
    c = ServeConfig().update_from_args(ns)
    assert c.enable_lora and c.lora_names() == ["a", "b"] and (c.max_loras, c.max_lora_rank) == (3, 32)
    assert ServeConfig.from_json(c.to_json()).lora_names() == ["a", "b"]
    monkeypatch.setenv("ENABLE_LORA", "1")
    monkeypatch.setenv("LORA_MODULES", f"x={adapters['a']},y={adapters['b']}")
    monkeypatch.setenv("MAX_LORAS", "2")
    monkeypatch.setenv("MAX_LORA_RANK", "8")
    e = ServeConfig.from_env().validate()
    assert e.enable_lora and e.lora_names() == ["x", "y"] and (e.max_loras, e.max_lora_rank) == (2, 8)
    assert e.runtime_dict()["lora_names"] == ["x", "y"] and e.runtime_dict()["enable_lora"] is True
