"""`n` of POST /v1/chat/completions through the real server on the CPU engine: several choices in one response or one
stream, per-choice logprobs and stop strings, the 400s, /chat untouched, and the DP router with two CPU replicas."""
import json
import os
import socket
import subprocess
import sys
import threading
import time

import pytest

from distributed_sse_for_llm_response_amd import runtime as rtmod
from distributed_sse_for_llm_response_amd.serving.app import ServingApp
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from distributed_sse_for_llm_response_amd.utils.sse_client import request

H = "127.0.0.1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSG = [{"role": "user", "content": "Why stream tokens one by one?"}]


@pytest.fixture(scope="module")
def app():
    c = ServeConfig(host=H, sse_port=0, origin_port=0, metrics_port=0, resp_port=0, io_threads=2, engine="cpu",
                    max_tokens=8, temperature=0.0)
    a = ServingApp(c).start()
    try:
        yield a
    finally:
        a.stop()


def _post(app, body, path="/v1/chat/completions", role="origin"):
    return request(H, app.port(role), "POST", path, body, timeout=120)


def _chunks(r):
    lines = [ln for ln in r.body.decode().splitlines() if ln.startswith("data: ")]
    return lines, [json.loads(ln[6:]) for ln in lines if ln != "data: [DONE]"]


def test_two_choices_buffered_with_summed_usage(app):
    body = {"messages": MSG, "max_tokens": 6, "temperature": 1.0, "seed": 5, "n": 2}
    before = dict(app.engine.stats)
    r = _post(app, body)
    assert r.status == 200, r.body
    d = json.loads(r.body)
    assert [c["index"] for c in d["choices"]] == [0, 1]
    for c in d["choices"]:
        assert c["finish_reason"] in ("length", "stop") and c["message"]["role"] == "assistant"
    u = d["usage"]
    assert u["prompt_tokens"] > 0 and 2 <= u["completion_tokens"] <= 12
    assert u["total_tokens"] == u["prompt_tokens"] + u["completion_tokens"]  # the prompt is counted once
    assert app.engine.stats["fork_requests"] == before["fork_requests"] + 1
    assert app.engine.stats["fork_shared_tokens"] == before["fork_shared_tokens"] + u["prompt_tokens"] - 1
    # choice 0 is the same request with n = 1; choice 1 the one with seed + 1
    for i, c in enumerate(d["choices"]):
        solo = json.loads(_post(app, {**body, "n": 1, "seed": 5 + i}).body)
        assert solo["choices"][0]["message"]["content"] == c["message"]["content"], i
        assert len(solo["choices"]) == 1
    # the completion tokens are the sum over the choices
    counts = [json.loads(_post(app, {**body, "n": 1, "seed": 5 + i}).body)["usage"]["completion_tokens"]
              for i in range(2)]
    assert u["completion_tokens"] == sum(counts)


def test_three_choices_streamed(app):
    r = _post(app, {"messages": MSG, "max_tokens": 5, "temperature": 1.0, "seed": 9, "n": 3, "stream": True})
    assert r.status == 200
    lines, chunks = _chunks(r)
    assert lines[-1] == "data: [DONE]" and lines.count("data: [DONE]") == 1
    assert len({c["id"] for c in chunks}) == 1
    per = {0: [], 1: [], 2: []}
    for c in chunks:
        assert len(c["choices"]) == 1
        per[c["choices"][0]["index"]].append(c["choices"][0])
    for i, cs in per.items():
        assert cs[0]["delta"] == {"role": "assistant", "content": ""}, i  # the role chunk comes first
        fins = [c for c in cs if c["finish_reason"] is not None]
        assert len(fins) == 1 and fins[0] is cs[-1] and fins[0]["delta"] == {}, i
        toks = cs[1:-1]
        assert 1 <= len(toks) <= 5 and all(isinstance(t["delta"]["content"], str) for t in toks), i
    # the role chunks of every index precede the first token chunk
    first_tok = next(k for k, c in enumerate(chunks) if c["choices"][0]["delta"].get("role") is None)
    assert sorted(c["choices"][0]["index"] for c in chunks[:first_tok]) == [0, 1, 2]


def test_logprobs_per_choice(app):
    body = {"messages": MSG, "max_tokens": 4, "temperature": 1.0, "seed": 3, "n": 2, "logprobs": True,
            "top_logprobs": 2}
    d = json.loads(_post(app, body).body)
    for i, c in enumerate(d["choices"]):
        ent = c["logprobs"]["content"]
        assert "".join(e["token"] for e in ent) == c["message"]["content"]
        assert all(len(e["top_logprobs"]) == 2 and e["logprob"] <= 0 for e in ent)
        # the same tokens as the n = 1 request of seed + i.  The values agree to bf16 rounding only: the choices decode
        # in one batch, the lone request in a batch of one, and the bf16 weights' matmuls round differently per batch
        # shape (one bf16 ulp, 2^-8, of logits of magnitude <= 8: 0.03 -- also for choice 0, which forks nothing)
        solo = json.loads(_post(app, {**body, "n": 1, "seed": 3 + i}).body)["choices"][0]["logprobs"]["content"]
        assert [e["token"] for e in solo] == [e["token"] for e in ent], i
        assert all(abs(x["logprob"] - y["logprob"]) < 0.03 for x, y in zip(solo, ent)), i
    s = _post(app, {**body, "stream": True})
    _, chunks = _chunks(s)
    for i in range(2):
        got = [c["choices"][0]["logprobs"]["content"][0] for c in chunks
               if c["choices"][0]["index"] == i and c["choices"][0]["delta"].get("content") is not None
               and c["choices"][0]["delta"].get("role") is None and c["choices"][0]["finish_reason"] is None]
        assert got == d["choices"][i]["logprobs"]["content"], i


def test_stop_string_ends_one_choice_while_the_others_run_on(app):
    body = {"messages": MSG, "max_tokens": 8, "temperature": 1.0, "seed": 21, "n": 3}
    free = [c["message"]["content"] for c in json.loads(_post(app, body).body)["choices"]]
    # a stop string that occurs in exactly one choice's text, past its first character
    pick = None
    for i, t in enumerate(free):
        for a in range(1, len(t) - 1):
            for ln in (3, 2):
                s = t[a:a + ln]
                if len(s) == ln and all(s not in o for j, o in enumerate(free) if j != i):
                    pick = pick or (i, s)
    assert pick is not None, free
    i, s = pick
    d = json.loads(_post(app, {**body, "stop": [s]}).body)
    for j, c in enumerate(d["choices"]):
        if j == i:
            assert c["finish_reason"] == "stop" and c["message"]["content"] == free[i][:free[i].index(s)]
        else:
            assert c["message"]["content"] == free[j] and c["finish_reason"] == "length", (j, c)


@pytest.mark.parametrize("n", [0, 17, 1.5, -1, "2"])
def test_n_outside_the_range_is_a_400(app, n):
    r = _post(app, {"messages": MSG, "max_tokens": 2, "n": n})
    assert r.status == 400
    assert "n must be an integer in [1, 16]" in json.loads(r.body)["message"]


def test_n_above_the_engines_slots_is_a_400(app):
    assert app.engine.r.max_batch == 8  # the CPU engine's decode slots
    r = _post(app, {"messages": MSG, "max_tokens": 2, "n": 9})
    assert r.status == 400 and "MAX_BATCH" in json.loads(r.body)["message"]
    assert _post(app, {"messages": MSG, "max_tokens": 2, "n": 8}).status == 200


def test_chat_route_ignores_n(app):
    before = app.engine.stats["fork_requests"]
    r = _post(app, {"message": "Why stream tokens?", "max_tokens": 4, "n": 3}, path="/chat", role="edge")
    assert r.status == 200
    toks = [e.json() for e in r.events if e.event == "token"]
    assert toks[-1]["done"] and len({t["conversation_id"] for t in toks}) == 1
    assert [t["sequence"] for t in toks] == list(range(1, len(toks) + 1))
    assert app.engine.stats["fork_requests"] == before


def test_fork_counters_reach_metrics(app):
    """After the n > 1 traffic of this file /metrics names the engine's fork counters (a server that never saw such a
    request does not: tests/test_kv_fp8_server.py pins that surface)."""
    body = {"messages": MSG, "max_tokens": 3, "temperature": 1.0, "seed": 2, "n": 3}

    def read():
        text = request(H, app.port("metrics"), "GET", "/metrics").body.decode()
        vals = {ln.split()[0]: float(ln.split()[1]) for ln in text.splitlines()
                if ln.startswith("engine_parallel_sampling_")}
        return vals, text

    assert _post(app, body).status == 200
    want = {"engine_parallel_sampling_requests_total": app.engine.stats["fork_requests"],
            "engine_parallel_sampling_shared_tokens_total": app.engine.stats["fork_shared_tokens"],
            "engine_parallel_sampling_tail_copies_total": app.engine.stats["fork_tail_copies"]}
    assert want["engine_parallel_sampling_requests_total"] >= 1
    deadline = time.time() + 10
    while time.time() < deadline and read()[0] != want:  # (the loop reports after the step that finished the request)
        _post(app, {"messages": MSG, "max_tokens": 1})
    vals, text = read()
    assert vals == want, (vals, want)
    assert "# TYPE engine_parallel_sampling_requests_total counter" in text


# ---------------------------------------------------------------- connection events (a runtime without an engine:
# the test is the producer, so what has ended when is exact)
def _bare(**kw):
    cfg = {"sse_port": 0, "origin_port": 0, "metrics_port": 0, "resp_port": 0, "io_threads": 2, "host": H,
           "local_engine": True}
    cfg.update(kw)
    r = rtmod.load().Runtime(cfg)
    r.start()
    return r


def _submit(rt, body):
    """POST the request in a thread; returns (thread, [response], the queued request as the engine would see it)."""
    got = []
    th = threading.Thread(target=lambda: got.append(
        request(H, rt.bound_port("origin"), "POST", "/v1/chat/completions", body, timeout=20)))
    th.start()
    reqs = []
    deadline = time.time() + 10
    while not reqs and time.time() < deadline:
        reqs = list(rt.poll_requests(4, 100))
    assert len(reqs) == 1
    return th, got, reqs[0]


@pytest.mark.parametrize("stream", [False, True])
def test_kill_after_choice_0_ended_ends_the_siblings(stream):
    rt = _bare()
    try:
        th, got, req = _submit(rt, {"messages": MSG, "n": 3, "stream": stream})
        conv = req["conversation_id"]
        assert req["n"] == 3 and rt.subscriber_count(conv + "-c1") == 1 and rt.subscriber_count(conv + "-c2") == 1
        rt.publish(conv, "a", 1, False, 0)
        rt.publish(conv, "[DONE]", 2, True, 0)  # choice 0 is over; its siblings run on
        rt.publish(conv + "-c1", "b", 1, False, 0)
        rt.publish(conv + "-c2", "c", 1, False, 0)
        time.sleep(0.1)
        r = request(H, rt.bound_port("edge"), "POST", f"/publish/chat.{conv}.control", {"action": "kill"})
        assert r.status == 200 and json.loads(r.body)["status"] == "killed"
        rt.publish(conv + "-c1", "late", 2, False, 0)  # the producer had not seen the kill yet
        th.join(10)
        assert got and got[0].status == 200
        if stream:
            lines, chunks = _chunks(got[0])
            assert lines[-1] == "data: [DONE]"
            fins = {c["choices"][0]["index"]: c["choices"][0]["finish_reason"] for c in chunks
                    if c["choices"][0]["finish_reason"]}
            text = "".join(c["choices"][0]["delta"].get("content") or "" for c in chunks)
        else:
            d = json.loads(got[0].body)
            fins = {c["index"]: c["finish_reason"] for c in d["choices"]}
            text = "".join(c["message"]["content"] for c in d["choices"])
        assert fins == {0: "stop", 1: "abort", 2: "abort"} and "late" not in text
        assert sorted(rt.pop_cancellations()) == [conv + "-c1", conv + "-c2"]
        assert rt.subscriber_count(conv + "-c1") == 0
    finally:
        rt.stop()


def test_kill_of_a_plain_conversation_spares_a_lookalike_id():
    rt = _bare()
    try:
        outs = {}

        def stream(c):
            outs[c] = request(H, rt.bound_port("edge"), "GET", f"/stream/{c}", timeout=3)

        ths = [threading.Thread(target=stream, args=(c,)) for c in ("abc", "abc-c1")]
        for t in ths:
            t.start()
        time.sleep(0.3)
        rt.publish("abc", "x", 1, False, 0)
        rt.publish("abc-c1", "y", 1, False, 0)
        request(H, rt.bound_port("edge"), "POST", "/publish/chat.abc.control", {"action": "kill"})
        rt.publish("abc-c1", "z", 2, False, 0)
        rt.publish("abc-c1", "[DONE]", 3, True, 0)
        for t in ths:
            t.join(5)
        toks = {c: [e.json()["token"] for e in outs[c].events if e.event == "token"] for c in outs}
        assert toks == {"abc": ["x", "[KILLED]"], "abc-c1": ["y", "z", "[DONE]"]}
    finally:
        rt.stop()


def test_disconnect_cancels_every_choice():
    rt = _bare()
    try:
        body = json.dumps({"messages": MSG, "n": 3, "stream": True}).encode()
        s = socket.create_connection((H, rt.bound_port("origin")))
        s.sendall(b"POST /v1/chat/completions HTTP/1.1\r\nHost: x\r\nContent-Type: application/json\r\n"
                  b"Content-Length: " + str(len(body)).encode() + b"\r\n\r\n" + body)
        reqs = []
        deadline = time.time() + 10
        while not reqs and time.time() < deadline:
            reqs = list(rt.poll_requests(4, 100))
        conv = reqs[0]["conversation_id"]
        rt.publish(conv, "a", 1, False, 0)
        s.close()
        cancels = []
        deadline = time.time() + 10
        while len(cancels) < 3 and time.time() < deadline:
            cancels += list(rt.pop_cancellations())
            time.sleep(0.02)
        assert sorted(cancels) == [conv, conv + "-c1", conv + "-c2"]
        assert rt.subscriber_count(conv + "-c2") == 0
    finally:
        rt.stop()


def test_first_token_timeout_ends_every_choice():
    rt = _bare(first_token_timeout_ms=300)
    try:
        th, got, req = _submit(rt, {"messages": MSG, "n": 2})
        th.join(10)
        d = json.loads(got[0].body)
        assert [(c["index"], c["finish_reason"], c["message"]["content"]) for c in d["choices"]] == \
            [(0, "abort", ""), (1, "abort", "")]
        conv = req["conversation_id"]
        assert sorted(rt.pop_cancellations()) == [conv, conv + "-c1"]
    finally:
        rt.stop()


def _free_port():
    s = socket.socket()
    s.bind((H, 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(300)
def test_choices_through_the_dp_router():
    """Two CPU replicas behind the router: every choice of a request comes back through one front door, and equals
    the n = 1 requests of seed + i (whichever replica served those)."""
    sse, met = _free_port(), _free_port()
    env = dict(os.environ, MASTER_PORT=str(_free_port()), PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    p = subprocess.Popen([sys.executable, "-m", "distributed_sse_for_llm_response_amd", "serve", "--dp", "2",
                          "--engine", "cpu", "--host", H, "--sse-port", str(sse), "--origin-port", "-1",
                          "--metrics-port", str(met), "--max-tokens", "6", "--temperature", "0"],
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        deadline = time.time() + 240
        ready = False
        while time.time() < deadline and p.poll() is None:
            try:
                ready = request(H, met, "GET", "/metrics", timeout=2).body.decode().count("dp_workers_alive 2") == 1
            except OSError:
                ready = False
            if ready:
                break
            time.sleep(0.5)
        assert ready, p.stdout.read() if p.poll() is not None else "router never saw 2 workers"
        body = {"messages": MSG, "max_tokens": 5, "temperature": 1.0, "seed": 13, "n": 3}
        for _ in range(2):  # (twice: the rotation sends the second request to the other replica)
            r = request(H, sse, "POST", "/v1/chat/completions", body, timeout=120)
            assert r.status == 200, r.body
            d = json.loads(r.body)
            assert [c["index"] for c in d["choices"]] == [0, 1, 2]
            for i, c in enumerate(d["choices"]):
                solo = json.loads(request(H, sse, "POST", "/v1/chat/completions", {**body, "n": 1, "seed": 13 + i},
                                          timeout=120).body)
                assert solo["choices"][0]["message"]["content"] == c["message"]["content"], i
        s = request(H, sse, "POST", "/v1/chat/completions", {**body, "stream": True}, timeout=120)
        lines = [ln for ln in s.body.decode().splitlines() if ln.startswith("data: ")]
        assert lines[-1] == "data: [DONE]"
        fins = [json.loads(ln[6:])["choices"][0] for ln in lines[:-1]]
        assert sorted(c["index"] for c in fins if c["finish_reason"]) == [0, 1, 2]
        # the replicas' fork counters reach the router's /metrics with their stats messages (sent while they step)
        want, seen = "engine_parallel_sampling_requests_total 3", ""
        deadline = time.time() + 20
        while time.time() < deadline and want not in seen:
            request(H, sse, "POST", "/v1/chat/completions", {"messages": MSG, "max_tokens": 1}, timeout=120)
            seen = request(H, met, "GET", "/metrics", timeout=5).body.decode()
        assert want in seen, [ln for ln in seen.splitlines() if "parallel_sampling" in ln]
    finally:
        p.terminate()
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()
