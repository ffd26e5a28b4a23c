"""stop / stop_token_ids / min_tokens / min_p / logit_bias without a GPU: the CPU twins against float64, the CPU
engine (bias, ban, stop tokens, preemption), the stop-string matcher, both HTTP routes, the DP ring, the TP plan and
TP = 2 over gloo."""
import json
import math
import os
import socket
import threading
import time
import uuid

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd import runtime as rtmod
from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams, TokenEvent
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as ref
from distributed_sse_for_llm_response_amd.parallel.comm import TPComm
from distributed_sse_for_llm_response_amd.serving import tp as tpmod
from distributed_sse_for_llm_response_amd.serving.app import ServingApp
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from distributed_sse_for_llm_response_amd.serving.stop_strings import StopMatcher
from distributed_sse_for_llm_response_amd.utils.sse_client import request

H = "127.0.0.1"


# ------------------------------------------------------------------------------------------------ twins
def _ctl(Bm):
    return torch.zeros(4 * Bm, dtype=torch.int32), torch.zeros(Bm, ops.CTL_BODY, dtype=torch.int32)


def _set(meta, body, slot, bias=(), bans=(), until=0, min_p=0.0):
    Bm = meta.numel() // 4
    meta[slot], meta[Bm + slot], meta[2 * Bm + slot] = len(bias), len(bans), until
    meta[3 * Bm:].view(torch.float32)[slot] = min_p
    for j, (t, b) in enumerate(bias):
        body[slot, 2 * j] = t
        body[slot, 2 * j + 1:2 * j + 2].view(torch.float32)[0] = b
    for j, t in enumerate(bans):
        body[slot, 2 * ops.CTL_BIAS + j] = t


def test_bias_and_ban_twin_against_float64():
    V, Bm = 64, 4
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(3, V, generator=g)
    meta, body = _ctl(Bm)
    bias = [(3, 1.25), (10, -100.0), (63, 100.0), (200, 5.0)]  # 200: outside the vocabulary slice, skipped
    _set(meta, body, 2, bias=bias, bans=(7, 3), until=12)
    _set(meta, body, 1, bans=(5,), until=12)
    row_slot = torch.tensor([2, 1, 0], dtype=torch.int32)
    pos = torch.tensor([10, 11, 3], dtype=torch.int32)  # row 0: 11 < 12 ban in force; row 1: 12 >= 12 expired
    x = x0.clone()
    ref.sample_bias_ban(x, None, meta, body, pos, row_slot)
    want = x0.double().clone()
    for t, b in bias[:3]:
        want[0, t] = float((x0[0, t].double() + b).float())  # (the fp32 sum)
    want[0, 7] = want[0, 3] = -math.inf
    assert torch.equal(x.double(), want)
    assert torch.equal(x[1], x0[1]) and torch.equal(x[2], x0[2])  # expired ban / neutral slot: bit-identical
    # an inactive row stays; the second shard of a 32 + 32 split sees id 63 only
    y = x0.clone()
    ref.sample_bias_ban(y, torch.tensor([0, 1, 1], dtype=torch.int32), meta, body, pos, row_slot)
    assert torch.equal(y, x0)
    z = x0[:, 32:].clone()
    ref.sample_bias_ban(z, None, meta, body, pos, row_slot, vocab_offset=32)
    assert float(z[0, 31]) == float(x0[0, 63] + 100.0) and torch.equal(z[0, :31], x0[0, 32:63])


def test_min_p_twin_against_float64():
    x = torch.tensor([2.0, 1.0, 0.0, -1.0, -3.0, 1.9])
    T = 0.5
    for mp_, k, p in ((0.1, 0, 1.0), (0.5, 0, 1.0), (0.1, 2, 1.0), (0.01, 0, 0.6), (1.0, 0, 1.0)):
        xs = x.double() / T
        keep = xs - xs.max() >= math.log(mp_) - 1e-12
        if k:
            keep &= xs >= xs.topk(k).values[-1]
        if p < 1.0:
            pr = torch.where(keep, torch.exp(xs - xs.max()), torch.zeros_like(xs))
            pr /= pr.sum()
            order = torch.argsort(pr, descending=True)
            n = int(torch.searchsorted(torch.cumsum(pr[order], 0), torch.tensor(p, dtype=torch.float64))) + 1
            keep2 = torch.zeros_like(keep)
            keep2[order[:n]] = True
            keep &= keep2
        got = ref._kept_mask(xs / math.log(2.0), k, p, mp_)
        assert got.tolist() == keep.tolist(), (mp_, k, p)
    # through the op: every sample of a min_p row lies in the kept set; a greedy row ignores min_p
    meta, _ = _ctl(2)
    meta[6:].view(torch.float32)[:] = torch.tensor([0.5, 0.5])
    logits = torch.stack([x, x])
    cand = torch.zeros(2, 1, 2)
    seen = set()
    for s in range(64):
        ops.sample_candidates_min_p(logits, torch.tensor([T, 0.0]), torch.zeros(2, dtype=torch.int32), torch.ones(2),
                                    torch.tensor([[s, 1], [s, 1]], dtype=torch.int32),
                                    torch.tensor([s, s], dtype=torch.int32), None, cand, meta)
        seen.add(int(cand[0, 0, 1]))
        assert int(cand[1, 0, 1]) == 0
    assert seen == {0, 5}  # exp((1.9 - 2) / 0.5) = 0.82 >= 0.5 > exp(-2) = 0.14


# ------------------------------------------------------------------------------------------------ CPU engine
_W = {}
EOS = 2


def _engine(num_blocks=256, max_batch=4, eos_id=EOS):
    if "w" not in _W:
        _W["w"] = convert_standard(TINY, init_standard_weights(TINY, seed=11))
    r = ModelRunner(_W["w"], num_blocks=num_blocks, max_batch=max_batch, max_model_len=512, device="cpu",
                    use_graphs=False)
    return LLMEngine(r, eos_id=eos_id, prefill_budget=256)


def _prompt(i, n):
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randint(3, TINY.vocab_size, (n,), generator=g).tolist()


def _run(e, reqs, max_steps=4000):
    """reqs = [(conv, prompt, SamplingParams, step_to_add)] -> (conv -> [token ids], conv -> finish reason)."""
    out, fin = {c: [] for c, *_ in reqs}, {}
    for step in range(max_steps):
        for c, p, sp, at in reqs:
            if at == step:
                e.add_request(c, p, sp)
        for ev in e.step():
            if ev.done:
                fin[ev.conversation_id] = ev.finish
            else:
                out[ev.conversation_id].append(ev.token_id)
        if step > max(at for *_, at in reqs) and not e.has_work():
            break
    assert not e.has_work(), "engine did not drain"
    return out, fin


def _greedy(mt, **kw):
    return SamplingParams(temperature=0.0, max_tokens=mt, **kw)


def test_bias_forces_and_bans_a_token():
    p = _prompt(0, 20)
    plain, _ = _run(_engine(eos_id=-1), [("a", p, _greedy(12), 0)])
    e = _engine(eos_id=-1)
    forced, _ = _run(e, [("a", p, _greedy(12, logit_bias={77: 100.0}), 0)])
    assert forced["a"] == [77] * 12 and e.r.ctl_used
    first = plain["a"][0]
    banned, _ = _run(_engine(eos_id=-1), [("a", p, _greedy(12, logit_bias={first: -100.0}), 0)])
    assert first not in banned["a"] and len(banned["a"]) == 12
    sampled, _ = _run(_engine(eos_id=-1), [("a", p, SamplingParams(temperature=1.0, seed=3, max_tokens=12,
                                                                     logit_bias={77: 100.0}), 0)])
    assert sampled["a"] == [77] * 12  # +100 wins under sampling as well
    # no field: nothing is uploaded and the pass is never enabled
    e = _engine(eos_id=-1)
    again, _ = _run(e, [("a", p, _greedy(12), 0)])
    assert again == plain and not e.r.ctl_used and not e._ctl_live


def test_min_tokens_holds_eos_back_for_exactly_that_many_tokens():
    p = _prompt(1, 33)  # (33 tokens: the prefill ends off a page boundary)
    e = _engine()
    out, fin = _run(e, [("a", p, _greedy(40, logit_bias={EOS: 100.0}, min_tokens=7), 0)])
    assert len(out["a"]) == 7 and EOS not in out["a"] and fin["a"] == "stop"
    out, fin = _run(_engine(), [("a", p, _greedy(40, logit_bias={EOS: 100.0}), 0)])
    assert out["a"] == [] and fin["a"] == "stop"  # without min_tokens EOS comes at once
    # stop_token_ids are banned with EOS, and end the stream afterwards
    out, fin = _run(_engine(), [("a", p, _greedy(40, logit_bias={90: 100.0}, min_tokens=3, stop_token_ids=(90,)), 0)])
    assert len(out["a"]) == 3 and 90 not in out["a"] and fin["a"] == "stop"


def test_stop_token_ends_the_stream_undelivered():
    p = _prompt(2, 20)
    plain, _ = _run(_engine(eos_id=-1), [("a", p, _greedy(12), 0)])
    t = plain["a"][4]
    k = plain["a"].index(t)
    for ignore_eos in (False, True):
        out, fin = _run(_engine(eos_id=-1), [("a", p, _greedy(12, stop_token_ids=(t,), ignore_eos=ignore_eos), 0)])
        assert out["a"] == plain["a"][:k] and fin["a"] == "stop"


def test_preempted_biased_streams_resume_token_exact():
    bias = {5: 3.0, 9: -100.0, 700: 2.0}
    reqs = [(f"c{i}", _prompt(i, 20 + 7 * i), _greedy(50 + 5 * i, logit_bias=bias, min_tokens=20 + i, ignore_eos=True,
                                                      stop_token_ids=(11,)), i // 2) for i in range(5)]
    want, _ = _run(_engine(num_blocks=256), reqs)
    e = _engine(num_blocks=10)
    got, _ = _run(e, reqs)
    assert e.stats["preemptions"] > 0 and got == want
    plain, _ = _run(_engine(num_blocks=256), [(c, p, _greedy(sp.max_tokens, ignore_eos=True), at)
                                              for c, p, sp, at in reqs])
    assert plain != want


# ------------------------------------------------------------------------------------------------ stop strings
PIECES = ["<0>", "ab", "cd", "e", "fgh", " ", "xy", "bcd"]


def _ev(conv, toks, done=None, start=1):
    out = [TokenEvent(conv, t, start + i, False) for i, t in enumerate(toks)]
    if done:
        out.append(TokenEvent(conv, -1, start + len(toks), True, text="[DONE]", finish=done, prompt_tokens=3))
    return out


def _text(m, events):
    return "".join(e.text or m.piece(e.token_id) for e in events if not e.done)


def _matcher(stops, min_tokens=0):
    m = StopMatcher(PIECES.__getitem__)
    m.register("c", stops, min_tokens, prompt_tokens=3)
    return m


@pytest.mark.parametrize("stop", ["b", "bc", "de", "ab", "dx", "cde", "fgh", "h"])
@pytest.mark.parametrize("batch", [1, 2, 100])
def test_matcher_truncates_at_the_earliest_match(stop, batch):
    toks = [1, 2, 3, 4, 5, 6]  # "abcdefgh xy"
    text = "".join(PIECES[t] for t in toks)
    m = _matcher([stop, "zzz"])
    evs, out = _ev("c", toks, "length"), []
    for i in range(0, len(evs), batch):
        out += m.filter(evs[i:i + batch])
    cut = text.find(stop)
    want = text[:cut] if cut >= 0 else text
    assert _text(m, out) == want
    assert [e.sequence for e in out] == list(range(1, len(out) + 1)) and out[-1].done and sum(e.done for e in out) == 1
    if cut >= 0:
        assert out[-1].finish == "stop" and out[-1].prompt_tokens == 3 and m.pop_aborts() == ["c"]
        assert not m.closed  # the engine's leftovers, its terminal frame included, were dropped on the way
    else:
        assert out[-1].finish == "length" and m.pop_aborts() == []
    assert not m.streams


def test_matcher_holds_only_while_a_match_can_still_begin():
    m = _matcher(["bcdx", "hq"])
    a, b, c = _ev("c", [1, 2, 3])
    assert m.filter([a]) == []            # "ab": "b" may begin "bcdx"
    assert m.filter([b]) == []            # "abcd": "bcd" still may
    out = m.filter([c])                   # "abcde": ruled out -> everything goes, complete and in order
    assert [e.sequence for e in out] == [1, 2, 3] and _text(m, out) == "abcde"
    (d,) = _ev("c", [4], start=4)
    assert m.filter([d]) == []            # "fgh": "h" may begin "hq"
    out = m.filter(_ev("c", [], "length", start=5))
    assert [e.sequence for e in out] == [4, 5] and out[-1].finish == "length"  # the held tail is flushed
    # min_tokens: nothing is matched, or held, in the first tokens
    m = _matcher(["ab", "e"], min_tokens=2)
    out = m.filter(_ev("c", [1, 2, 3, 4]))
    assert _text(m, out) == "abcd" and out[-1].done and out[-1].sequence == 3
    # other conversations pass untouched
    other = _ev("d", [1, 2], "stop")
    assert m.filter(other) == other


# ------------------------------------------------------------------------------------------------ HTTP
@pytest.fixture
def rt():
    r = rtmod.load().Runtime({"sse_port": 0, "origin_port": 0, "metrics_port": 0, "resp_port": 0, "io_threads": 2,
                              "host": H, "first_token_timeout_ms": 200})
    r.start()
    r.set_local_engine(True)  # requests queue up, nothing generates
    r.set_vocab([f"tok{i}" for i in range(1000)])
    yield r
    r.stop()


def _post(rt, route, extra, role="origin"):
    body = {"message": "hi"} if route == "/chat" else {"messages": [{"role": "user", "content": "hi"}]}
    return request(H, rt.bound_port(role), "POST", route, json.dumps({**body, **extra}).encode(), timeout=10)


@pytest.mark.parametrize("route", ["/chat", "/v1/chat/completions"])
def test_fields_reach_the_queued_request(rt, route):
    _post(rt, route, {"logit_bias": {"5": 1.5, "999": -100}, "min_tokens": 3, "max_tokens": 3, "min_p": 0.25,
                      "stop_token_ids": [7, 0], "stop": ["a", "b\n"]})
    (q,) = rt.poll_requests(10, 1000)
    assert q["logit_bias"] == [(5, 1.5), (999, -100.0)] and q["min_tokens"] == 3 and q["min_p"] == 0.25
    assert q["stop_token_ids"] == [7, 0] and q["stop"] == ["a", "b\n"]
    _post(rt, route, {"stop": "END"})
    (q,) = rt.poll_requests(10, 1000)
    assert q["stop"] == ["END"]
    _post(rt, route, {"logit_bias": None, "min_tokens": None, "min_p": None, "stop_token_ids": None, "stop": None})
    (q,) = rt.poll_requests(10, 1000)
    assert (q["logit_bias"], q["min_tokens"], q["min_p"], q["stop_token_ids"], q["stop"]) == ([], 0, 0.0, [], [])


BAD = [({"logit_bias": [1]}, "logit_bias"), ({"logit_bias": {"a": 1}}, "logit_bias"),
       ({"logit_bias": {"1.5": 1}}, "logit_bias"), ({"logit_bias": {"-1": 1}}, "logit_bias"),
       ({"logit_bias": {"1000": 1}}, "logit_bias"), ({"logit_bias": {"1": 100.5}}, "logit_bias"),
       ({"logit_bias": {"1": -101}}, "logit_bias"), ({"logit_bias": {"1": "2"}}, "logit_bias"),
       ({"logit_bias": {str(i): 1 for i in range(301)}}, "logit_bias"),
       ({"stop_token_ids": 5}, "stop_token_ids"), ({"stop_token_ids": [1.5]}, "stop_token_ids"),
       ({"stop_token_ids": [-1]}, "stop_token_ids"), ({"stop_token_ids": [1000]}, "stop_token_ids"),
       ({"stop_token_ids": ["1"]}, "stop_token_ids"), ({"stop_token_ids": list(range(17))}, "stop_token_ids"),
       ({"stop": 5}, "stop must"), ({"stop": ""}, "stop must"), ({"stop": ["a", ""]}, "stop must"),
       ({"stop": ["a", 1]}, "stop must"), ({"stop": ["a", "b", "c", "d", "e"]}, "stop must"),
       ({"min_p": -0.1}, "min_p"), ({"min_p": 1.5}, "min_p"), ({"min_p": "0.5"}, "min_p"),
       ({"min_tokens": 1.5}, "min_tokens"), ({"min_tokens": -1}, "min_tokens"), ({"min_tokens": "3"}, "min_tokens"),
       ({"min_tokens": 5, "max_tokens": 4}, "min_tokens")]


@pytest.mark.parametrize("extra, field", BAD)
def test_bad_fields_are_a_400_that_names_the_field(rt, extra, field):
    for role in ("edge", "origin"):
        r = _post(rt, "/chat", extra, role)
        assert r.status == 400 and r.body.decode().startswith(field)
    r = _post(rt, "/v1/chat/completions", extra)
    assert r.status == 400 and json.loads(r.body)["message"].startswith(field)
    assert rt.poll_requests(10, 0) == []


@pytest.fixture(scope="module")
def cpu_app():
    c = ServeConfig(host=H, sse_port=0, origin_port=0, metrics_port=0, resp_port=0, io_threads=2)
    c.engine, c.max_tokens, c.temperature = "cpu", 8, 0.0
    app = ServingApp(c).start()
    yield app
    app.stop()


MSGS = [{"role": "user", "content": "Why stream tokens?"}]


def _oa(app, extra, stream=False):
    r = request(H, app.port("origin"), "POST", "/v1/chat/completions", {"messages": MSGS, "stream": stream, **extra},
                timeout=60, stop_on_done=False)
    if not stream:
        d = json.loads(r.body)
        return d["choices"][0]["message"]["content"], d["choices"][0]["finish_reason"], d["usage"]["completion_tokens"]
    chunks = [json.loads(e.data)["choices"][0] for e in r.events if e.data != "[DONE]"]
    parts = [c["delta"]["content"] for c in chunks[1:-1]]
    return parts, chunks[-1]["finish_reason"], len(parts)


def _idle(app):
    deadline = time.time() + 10
    while time.time() < deadline and (app.engine.has_work() or app.engine.alloc.num_free != app.engine.alloc.num_blocks):
        time.sleep(0.01)
    return not app.engine.has_work() and app.engine.alloc.num_free == app.engine.alloc.num_blocks


def test_stop_strings_on_the_openai_route(cpu_app):
    """This test fails where the field is ignored: the completion then runs to max_tokens."""
    parts, fin, n = _oa(cpu_app, {"max_tokens": 10}, stream=True)
    text = "".join(parts)
    assert n == 10 and fin == "length" and all(len(p) >= 2 for p in parts[:4])
    mid = parts[1][1:]                       # starts mid-token
    span = parts[1][-1] + parts[2][:1]       # spans two tokens
    head = parts[0][:1]                      # at the very start
    for stop in (mid, span, head, [span, mid], "no such text\n"):
        stops = [stop] if isinstance(stop, str) else stop
        cut = min((text.find(s) for s in stops if s in text), default=-1)
        want, reason = (text[:cut], "stop") if cut >= 0 else (text, "length")
        got, fin, n = _oa(cpu_app, {"max_tokens": 10, "stop": stop})
        assert (got, fin) == (want, reason)
        sp, fin, ns = _oa(cpu_app, {"max_tokens": 10, "stop": stop}, stream=True)
        assert ("".join(sp), fin, ns) == (want, reason, n)
        assert _idle(cpu_app)  # the aborted sequence's slot and pages are free again
    # /chat: the same text, contiguous sequence numbers, a terminal frame
    c = request(H, cpu_app.port("edge"), "POST", "/chat", {"message": "Why stream tokens?", "max_tokens": 10,
                                                           "stop": "no such text\n"}, timeout=60)
    full = [e.json() for e in c.events if e.event == "token"]
    ctext = "".join(t["token"] for t in full[:-1])
    stop = ctext[len(full[0]["token"]) + 1:len(full[0]["token"]) + 3]
    c = request(H, cpu_app.port("edge"), "POST", "/chat", {"message": "Why stream tokens?", "max_tokens": 10,
                                                           "stop": [stop]}, timeout=60)
    toks = [e.json() for e in c.events if e.event == "token"]
    assert "".join(t["token"] for t in toks[:-1]) == ctext[:ctext.find(stop)] and toks[-1]["done"]
    assert [t["sequence"] for t in toks] == list(range(1, len(toks) + 1)) and len(toks) < len(full)
    assert _idle(cpu_app)


def test_other_fields_take_effect_over_http(cpu_app):
    piece = cpu_app.tok.piece(77)
    for stream in (False, True):
        got, fin, n = _oa(cpu_app, {"max_tokens": 4, "logit_bias": {"77": 100}}, stream)
        assert "".join(got) == piece * 4 and n == 4
        eos = cpu_app.tok.eos_id
        got, fin, n = _oa(cpu_app, {"max_tokens": 9, "logit_bias": {str(eos): 100}, "min_tokens": 3}, stream)
        assert (n, fin) == (3, "stop")
        got, fin, n = _oa(cpu_app, {"max_tokens": 9, "logit_bias": {"77": 100}, "stop_token_ids": [77]}, stream)
        assert (n, fin) == (0, "stop")
        a = _oa(cpu_app, {"max_tokens": 6, "temperature": 1.0, "seed": 5, "min_p": 1.0}, stream)
        b = _oa(cpu_app, {"max_tokens": 6, "temperature": 0.0}, stream)
        assert a == b  # min_p = 1 keeps the most likely token only: sampling becomes greedy
    c = request(H, cpu_app.port("edge"), "POST", "/chat", {"message": "hi", "max_tokens": 3, "logit_bias": {"77": 100}},
                timeout=60)
    toks = [e.json() for e in c.events if e.event == "token"]
    assert [t["token"] for t in toks[:-1]] == [piece] * 3


# ------------------------------------------------------------------------------------------------ DP ring, TP plan
def test_dp_ring_delivers_the_fields_and_truncated_text():
    mod = rtmod.load()
    r = mod.Runtime({"sse_port": 0, "origin_port": 0, "metrics_port": 0, "resp_port": -1, "io_threads": 2,
                     "host": H, "local_engine": True})
    r.set_vocab([f"tok{i}" for i in range(100)])
    prefix = f"/dsse-test-{uuid.uuid4().hex[:8]}"
    r.start_dp_router(prefix, 1, 1, 10000)
    r.start()
    seen, stop = [], threading.Event()

    def worker():
        chan = mod.DpWorker(prefix, 0, 5000)
        chan.set_ready(True)
        m = StopMatcher(lambda t: f"tok{t}")
        while not stop.is_set() and not chan.shutdown_requested():
            for req in chan.poll_requests(16, 50):
                seen.append(req)
                c = req["conversation_id"]
                m.register(c, req["stop"], req["min_tokens"], 1)
                evs = m.filter([TokenEvent(c, 10, 1, False), TokenEvent(c, 21, 2, False), TokenEvent(c, 33, 3, False),
                                TokenEvent(c, -1, 4, True, text="[DONE]", finish="length", prompt_tokens=1)])
                chan.publish_tokens([e.conversation_id for e in evs], [e.token_id for e in evs],
                                    [e.sequence for e in evs], [e.done for e in evs], 0, [e.text for e in evs])

    t = threading.Thread(target=worker, daemon=True)
    t.start()
    try:
        deadline = time.time() + 10
        while time.time() < deadline and not all(i["ready"] for i in r.dp_workers()):
            time.sleep(0.02)
        a = request(H, r.bound_port("edge"), "POST", "/chat",
                    {"message": "hi", "conversation_id": "p1", "logit_bias": {"5": -2.5}, "min_tokens": 1, "min_p": 0.5,
                     "stop_token_ids": [3, 4], "stop": ["k21t", "zz"]}, timeout=30)
        b = request(H, r.bound_port("edge"), "POST", "/chat", {"message": "hi", "conversation_id": "p2"}, timeout=30)
        assert a.status == 200 and b.status == 200
        by = {q["conversation_id"]: q for q in seen}
        q = by["p1"]
        assert (q["logit_bias"], q["min_tokens"], q["min_p"], q["stop_token_ids"], q["stop"]) == \
               ([(5, -2.5)], 1, 0.5, [3, 4], ["k21t", "zz"])
        q = by["p2"]
        assert (q["logit_bias"], q["min_tokens"], q["min_p"], q["stop_token_ids"], q["stop"]) == ([], 0, 0.0, [], [])
        ta = [e.json() for e in a.events if e.event == "token"]
        assert [(x["token"], x["sequence"], x["done"]) for x in ta] == [("tok10", 1, False), ("to", 2, False),
                                                                        ("[DONE]", 3, True)]
        tb = [e.json() for e in b.events if e.event == "token"]
        assert [x["token"] for x in tb] == ["tok10", "tok21", "tok33", "[DONE]"]
    finally:
        stop.set()
        t.join(5)
        r.stop()


def test_plan_carries_the_fields_bit_exactly():
    sp = SamplingParams(temperature=0.7, max_tokens=9, logit_bias={5: 0.1, 31999: -100.0}, min_tokens=4,
                        stop_token_ids=(7, 8, 9), min_p=0.05, stop=("only the leader has text",))
    plan = tpmod.Plan(step=True, adds=[(7, [1, 2, 3], sp, 123456789), (8, [4], SamplingParams(), 5)], aborts=[3])
    once = plan.roundtrip()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    got = once.adds[0][2]
    assert got.logit_bias == {5: f32(0.1), 31999: -100.0} and got.min_tokens == 4 and got.stop_token_ids == (7, 8, 9)
    assert got.min_p == f32(0.05) and got.stop == ()
    dflt = once.adds[1][2]
    assert (dflt.logit_bias, dflt.min_tokens, dflt.stop_token_ids, dflt.min_p) == (None, 0, (), 0.0)
    assert once.adds[0][1] == [1, 2, 3] and once.adds[1][1] == [4] and once.aborts == [3]
    twice = once.roundtrip()
    assert twice.encode() == once.encode() and twice.adds == once.adds


# ------------------------------------------------------------------------------------------------ TP over gloo
TP_PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 150)), [11] * 20]
TP_TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]


def _tp_generate(rank, world, use=True, steps=10):
    std = init_standard_weights(TINY, seed=3)
    comm = TPComm(rank=rank, size=world, group=None) if world > 1 else TPComm()
    w = convert_standard(TINY, std, tp_rank=rank, tp_size=world)
    r = ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device="cpu", comm=comm, use_graphs=False)
    V = TINY.vocab_size
    for i, bt in enumerate(TP_TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
    if use:
        # slot 1: ids in both shards biased; slot 2: token V - 3 forced but banned for the first 4 tokens
        r.set_controls(1, {3: 50.0, V - 2: 49.0, 40: -100.0}, [])
        r.set_controls(2, {V - 3: 100.0}, [V - 3, 1])
        Bm = 4
        r.ctl_meta[1], r.ctl_meta[2], r.ctl_meta[Bm + 2], r.ctl_meta[2 * Bm + 2] = 3, 1, 2, len(TP_PROMPTS[2]) + 4
    r.prefill([PrefillSeq(i, p, 0, TP_TABLES[i], True) for i, p in enumerate(TP_PROMPTS)], ring_row=0)
    r.active[:3] = 1
    gen = [[int(r.ids[i])] for i in range(3)]
    for _ in range(steps):
        r.decode(4)
        for i in range(3):
            gen[i].append(int(r.ids[i]))
    return gen


def _tp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out[rank] = _tp_generate(rank, world)
    finally:
        dist.destroy_process_group()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(600)
def test_tp2_with_bias_and_min_tokens_matches_tp1():
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_tp_worker, args=(2, _port(), out), nprocs=2, join=True)
        res = [out[r] for r in range(2)]
    assert res[0] == res[1], "TP ranks disagree on the sampled tokens"
    one = _tp_generate(0, 1)
    assert res[0] == one
    V = TINY.vocab_size
    assert set(one[1]) == {3}                                   # +50 beats +49 in the other shard
    assert V - 3 not in one[2][:4] and one[2][4:] == [V - 3] * (len(one[2]) - 4)  # banned for 4 tokens, then forced
    plain = _tp_generate(0, 1, use=False)
    assert plain[0] == one[0] and plain[1:] != one[1:]
