"""Prefix caching through the serving stack on CPU: ENABLE_PREFIX_CACHING reaches the engine, cached_tokens rides
from the engine's terminal event to usage.prompt_tokens_details of the OpenAI route, the three counters reach
/metrics, and the DP router keeps the turns of one conversation on one replica while its load allows.

The runtime's metrics are process-wide, so the feature-off test runs first (definition order): once an engine with
the feature on has reported, the counters stay on /metrics."""
import json
import threading
import time
import uuid

from distributed_sse_for_llm_response_amd import runtime as rtmod
from distributed_sse_for_llm_response_amd.serving.app import ServingApp
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from distributed_sse_for_llm_response_amd.utils.sse_client import request

H = "127.0.0.1"
COUNTERS = ("engine_prefix_cache_queries_total", "engine_prefix_cache_hits_total",
            "engine_prefix_cache_evictions_total")
LONG = " ".join(f"word{i}" for i in range(60))  # a first user turn of well over two KV pages


def _cfg(**kw):
    c = ServeConfig(host=H, sse_port=0, origin_port=0, metrics_port=0, resp_port=0, io_threads=2, engine="cpu",
                    max_tokens=8, temperature=0.0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _complete(app, messages, **kw):
    r = request(H, app.port("origin"), "POST", "/v1/chat/completions", {"messages": messages, "max_tokens": 6, **kw},
                timeout=60)
    assert r.status == 200, r.body
    return r


def _metrics(app_or_rt):
    port = app_or_rt.port("metrics") if hasattr(app_or_rt, "port") else app_or_rt.bound_port("metrics")
    text = request(H, port, "GET", "/metrics").body.decode()
    return {ln.split()[0]: float(ln.split()[1]) for ln in text.splitlines() if ln and not ln.startswith("#")
            and "{" not in ln}


def _two_turns(app):
    first = [{"role": "user", "content": LONG}]
    d1 = json.loads(_complete(app, first).body)
    second = first + [{"role": "assistant", "content": d1["choices"][0]["message"]["content"]},
                      {"role": "user", "content": "and then?"}]
    return d1, json.loads(_complete(app, second).body), second


def test_feature_off_bodies_and_metrics_are_unchanged():
    assert ServeConfig().enable_prefix_caching is False
    app = ServingApp(_cfg()).start()
    try:
        assert not app.engine.prefix_cache
        d1, d2, second = _two_turns(app)
        for d in (d1, d2):
            assert sorted(d["usage"]) == ["completion_tokens", "prompt_tokens", "total_tokens"]
        s = request(H, app.port("origin"), "POST", "/v1/chat/completions",
                    {"messages": second, "max_tokens": 4, "stream": True}, timeout=60)
        assert b"usage" not in s.body and b"prompt_tokens_details" not in s.body
        m = _metrics(app)
        assert not any(k in m for k in COUNTERS)
    finally:
        app.stop()


def test_env_and_cli_switch(monkeypatch):
    import argparse

    monkeypatch.setenv("ENABLE_PREFIX_CACHING", "1")
    monkeypatch.setenv("DP_PREFIX_AFFINITY_SLACK", "7")
    c = ServeConfig.from_env()
    assert c.enable_prefix_caching is True and c.dp_prefix_affinity_slack == 7
    monkeypatch.delenv("ENABLE_PREFIX_CACHING")
    monkeypatch.delenv("DP_PREFIX_AFFINITY_SLACK")
    ap = argparse.ArgumentParser()
    ServeConfig.add_args(ap)
    assert ServeConfig.from_env().update_from_args(ap.parse_args([])).enable_prefix_caching is False
    c = ServeConfig.from_env().update_from_args(ap.parse_args(["--enable-prefix-caching"]))
    assert c.enable_prefix_caching is True and c.dp_prefix_affinity_slack == 4
    assert ServeConfig.from_json(c.to_json()).enable_prefix_caching is True  # (how DP worker processes get it)


def test_second_turn_reports_cached_tokens_and_counters(monkeypatch):
    monkeypatch.setenv("ENABLE_PREFIX_CACHING", "1")
    cfg = ServeConfig.from_env()
    app = ServingApp(_cfg(enable_prefix_caching=cfg.enable_prefix_caching)).start()
    try:
        assert app.engine.prefix_cache
        m0 = _metrics(app)
        assert all(k in m0 for k in COUNTERS)  # shown from the start when the feature is on
        d1, d2, second = _two_turns(app)
        assert d1["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
        cached = d2["usage"]["prompt_tokens_details"]["cached_tokens"]
        assert cached > 0 and cached % 32 == 0 and cached < d2["usage"]["prompt_tokens"]
        assert d2["usage"]["total_tokens"] == d2["usage"]["prompt_tokens"] + d2["usage"]["completion_tokens"]
        # the final chunk of a stream carries the same usage
        s = request(H, app.port("origin"), "POST", "/v1/chat/completions",
                    {"messages": second, "max_tokens": 4, "stream": True}, timeout=60)
        last = [json.loads(ln[6:]) for ln in s.body.decode().splitlines()
                if ln.startswith("data: {")][-1]
        assert last["usage"]["prompt_tokens_details"]["cached_tokens"] >= cached
        deadline = time.time() + 5
        while time.time() < deadline and _metrics(app)[COUNTERS[1]] - m0[COUNTERS[1]] < 2 * cached:
            time.sleep(0.05)
        m = _metrics(app)
        sent = d1["usage"]["prompt_tokens"] + 2 * d2["usage"]["prompt_tokens"]
        assert m[COUNTERS[0]] - m0[COUNTERS[0]] == sent  # queries: every prompt token of the three requests
        assert m[COUNTERS[1]] - m0[COUNTERS[1]] >= 2 * cached  # hits: prompt tokens served from resident pages
        assert m[COUNTERS[2]] - m0[COUNTERS[2]] == 0
    finally:
        app.stop()


# ------------------------------------------------------------------------------------------------ DP router
class _HoldingWorker(threading.Thread):
    """A stub replica: records what it is routed and answers (two tokens, [DONE]) once `release` is set."""

    def __init__(self, prefix, rank):
        super().__init__(daemon=True)
        self.chan = rtmod.load().DpWorker(prefix, rank, 5000)
        self.served, self.held = [], []
        self.release, self.stop = threading.Event(), threading.Event()

    def run(self):
        self.chan.set_ready(True)
        while not self.stop.is_set() and not self.chan.shutdown_requested():
            for req in self.chan.poll_requests(16, 20):
                self.served.append(req["messages"])
                self.held.append(req["conversation_id"])
            if self.release.is_set():
                for c in self.held:
                    self.chan.publish_tokens([c, c], [10, -1], [1, 2], [False, True], 0, ["", "[DONE]"], [0, 1], [-1, 3],
                                             [], [-1, 0])
                self.held = []


def _router(slack):
    rt = rtmod.load().Runtime({"sse_port": 0, "origin_port": 0, "metrics_port": 0, "resp_port": -1, "io_threads": 2,
                               "host": H, "local_engine": True})
    rt.set_vocab([f"tok{i}" for i in range(100)])
    prefix = f"/dsse-test-{uuid.uuid4().hex[:8]}"
    rt.start_dp_router(prefix, 2, 1, 10000, slack)
    rt.start()
    ws = [_HoldingWorker(prefix, k) for k in range(2)]
    for w in ws:
        w.start()
    deadline = time.time() + 10
    while time.time() < deadline and not all(i["ready"] for i in rt.dp_workers()):
        time.sleep(0.02)
    return rt, ws


def _norm(messages):
    return json.dumps(messages, separators=(",", ":"), ensure_ascii=False)


def _post(rt, messages, out=None):
    r = request(H, rt.bound_port("origin"), "POST", "/v1/chat/completions", {"messages": messages, "max_tokens": 4},
                timeout=30)
    if out is not None:
        out.append(r.status)
    return r


def test_affinity_key_covers_the_messages_up_to_the_first_user_turn():
    key = rtmod.load().dp_affinity_key
    sys_ = {"role": "system", "content": 'be "brief" \\ ok'}
    t1 = [sys_, {"role": "user", "content": "hello } there"}]
    t2 = t1 + [{"role": "assistant", "content": "hi"}, {"role": "user", "content": "more"}]
    assert key(_norm(t1)) == key(_norm(t2))
    assert key(_norm(t1)) != key(_norm([sys_, {"role": "user", "content": "hello } there!"}]))
    assert key(_norm(t1)) != key(_norm(t1[1:]))  # the system prompt is part of it


def test_router_keeps_a_conversation_on_its_replica_until_it_is_overloaded():
    key = rtmod.load().dp_affinity_key
    rt, ws = _router(slack=1)
    try:
        for w in ws:
            w.release.set()
        # two turns of one conversation land on the same worker, key % 2 -- for conversations of either worker (the
        # least-outstanding policy alone alternates between idle workers)
        for i in range(4):
            t1 = [{"role": "user", "content": f"conversation {i}"}]
            t2 = t1 + [{"role": "assistant", "content": "tok10"}, {"role": "user", "content": "go on"}]
            a = key(_norm(t1)) % 2
            for turn in (t1, t2):
                before = len(ws[a].served)
                assert _post(rt, turn).status == 200
                assert len(ws[a].served) == before + 1 and json.loads(ws[a].served[-1]) == turn
        assert all(len(w.served) > 0 for w in ws)  # (the four conversations cover both replicas)
        # the affine worker loaded past the slack: the request goes to the least loaded one
        for w in ws:
            w.release.clear()
        convs = [[{"role": "user", "content": f"busy {i}"}] for i in range(64)]
        mine = [c for c in convs if key(_norm(c)) % 2 == 0][:3]
        served = [len(w.served) for w in ws]
        status, threads = [], []
        for n, c in enumerate(mine):
            threads.append(threading.Thread(target=_post, args=(rt, c, status)))
            threads[-1].start()
            deadline = time.time() + 10
            while time.time() < deadline and sum(len(w.served) for w in ws) < sum(served) + n + 1:
                time.sleep(0.01)
        # outstanding on worker 0 was 0, then 1 (<= 0 + slack: still worker 0), then 2 (> 0 + 1: worker 1)
        assert [len(w.served) - s for w, s in zip(ws, served)] == [2, 1]
        assert json.loads(ws[1].served[-1]) == mine[2]
        for w in ws:
            w.release.set()
        for t in threads:
            t.join(30)
        assert status == [200, 200, 200]
    finally:
        for w in ws:
            w.stop.set()
        rt.stop()


def test_router_without_the_feature_ignores_the_key():
    rt, ws = _router(slack=-1)
    try:
        for w in ws:
            w.release.set()
        t1 = [{"role": "user", "content": "conversation 0"}]
        for _ in range(4):  # idle workers, ties rotate: the same first turn alternates between the replicas
            assert _post(rt, t1).status == 200
        assert [len(w.served) for w in ws] == [2, 2]
    finally:
        for w in ws:
            w.stop.set()
        rt.stop()
