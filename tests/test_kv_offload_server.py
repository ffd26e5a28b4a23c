"""The host KV tier through the serving stack on CPU: KV_OFFLOAD_GB reaches the engine, a second turn whose pages were
evicted in between is served from the host tier (cached_tokens in usage, as for any prefix-cache hit), and the tier's
counters reach /metrics -- only when it is on.

The runtime's metrics are process-wide and have no reset: once an engine with prefix caching (or the tier) on has
reported, its counters stay on /metrics, and tests/test_prefix_cache_server.py, which runs after this file, asserts
their absence in a process that never turned the feature on.  So each scenario here runs in a fresh child process
(this file as a script), which is also the only way "off" can be shown on a /metrics nobody has touched."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from distributed_sse_for_llm_response_amd.engine.kv_cache import KVCache  # noqa: E402
from distributed_sse_for_llm_response_amd.serving.app import ServingApp  # noqa: E402
from test_prefix_cache_server import _cfg, _complete, _metrics  # noqa: E402

NAMES = ("engine_prefix_cache_offload_spilled_pages_total", "engine_prefix_cache_offload_restored_pages_total",
         "engine_prefix_cache_offload_dropped_pages_total", "engine_prefix_cache_offload_hit_tokens_total")
FREE_PAGES = 8  # of the CPU serving engine's 256: the tests hold the rest, so a few requests turn the pool over
LONG = " ".join(f"word{i}" for i in range(120))  # a first user turn of three full KV pages and a bit


def _two_turns_with_evicting_traffic(app):
    held = app.engine.alloc.allocate(app.engine.alloc.num_free - FREE_PAGES)  # (before any request: the loop is idle)
    first = [{"role": "user", "content": LONG}]
    d1 = json.loads(_complete(app, first).body)
    for i in range(4):  # other conversations, each of several pages
        other = " ".join(f"other{i}x{j}" for j in range(120))
        _complete(app, [{"role": "user", "content": other}])
    second = first + [{"role": "assistant", "content": d1["choices"][0]["message"]["content"]},
                      {"role": "user", "content": "and then?"}]
    d2 = json.loads(_complete(app, second).body)
    return d1, d2, held


def tier_off_metrics_have_none_of_the_new_names():
    app = ServingApp(_cfg(enable_prefix_caching=True)).start()
    try:
        assert app.engine.offload is None
        d1, d2, _ = _two_turns_with_evicting_traffic(app)
        assert app.engine.stats["prefix_evictions"] > 0
        assert d2["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}  # evicted: the second turn is a miss
        text = _metrics(app)
        assert not any(n in text for n in NAMES) and not any("offload" in k for k in text)
    finally:
        app.stop()


def second_turn_is_served_from_the_host_tier():
    cfg = _cfg(enable_prefix_caching=True, kv_offload_gb=0.001)
    app = ServingApp(cfg).start()
    try:
        e = app.engine
        kv = e.r.kv
        per = KVCache.bytes_per_block(kv.num_layers, kv.nkv, kv.dtype)
        assert e.offload is not None and e.alloc.host_store.capacity == int(0.001 * 2**30) // per == 16
        m0 = _metrics(app)
        assert all(m0[n] == 0 for n in NAMES)  # shown from the start when the tier is on
        d1, d2, _ = _two_turns_with_evicting_traffic(app)
        assert d1["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
        cached = d2["usage"]["prompt_tokens_details"]["cached_tokens"]
        assert cached > 0 and cached % 32 == 0 and cached < d2["usage"]["prompt_tokens"]
        assert sorted(d2["usage"]["prompt_tokens_details"]) == ["cached_tokens"]  # no new response field
        assert e.stats["offload_restored_pages"] * 32 == e.stats["offload_hit_tokens"] > 0
        deadline = time.time() + 5
        while time.time() < deadline and _metrics(app)[NAMES[1]] < e.stats["offload_restored_pages"]:
            time.sleep(0.05)
        m = _metrics(app)
        assert m[NAMES[1]] == e.stats["offload_restored_pages"] > 0
        assert m[NAMES[0]] == e.stats["offload_spilled_pages"] > 0
        assert m[NAMES[3]] == e.stats["offload_hit_tokens"] and m[NAMES[2]] == e.stats["offload_dropped_pages"]
    finally:
        app.stop()


def _child(scenario):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), scenario], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and f"ok {scenario}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_tier_off_metrics_have_none_of_the_new_names():
    _child("tier_off_metrics_have_none_of_the_new_names")


def test_second_turn_is_served_from_the_host_tier():
    _child("second_turn_is_served_from_the_host_tier")


if __name__ == "__main__":
    globals()[sys.argv[1]]()
    print("ok", sys.argv[1])
