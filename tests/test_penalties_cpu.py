"""Presence / frequency / repetition penalties without a GPU: the reference semantics, the CPU engine (greedy,
preemption, compaction, TP over gloo), the TP plan's wire form, and the HTTP / DP request plumbing."""
import json
import os
import socket
import threading
import time
import uuid

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_sse_for_llm_response_amd import runtime as rtmod
from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as ref
from distributed_sse_for_llm_response_amd.parallel.comm import TPComm
from distributed_sse_for_llm_response_amd.serving import tp as tpmod
from distributed_sse_for_llm_response_amd.utils.sse_client import request

H = "127.0.0.1"


# ------------------------------------------------------------------------------------------------ semantics
def _state(Bm, cap):
    pen = torch.zeros(4 * Bm, dtype=torch.int32)
    pen[2 * Bm:3 * Bm].view(torch.float32).fill_(1.0)
    return pen, torch.zeros(Bm, cap + 1, dtype=torch.int32)


def test_reference_semantics_by_hand():
    """V = 8, prompt [1, 3], generated [3, 3, 4, 5], p = 0.5, f = 0.25, r = 2: repetition first (divide positive,
    multiply negative; the prompt-only token 1 gets nothing else), then frequency, then presence."""
    pen, hist = _state(2, 8)
    f = pen.view(torch.float32)
    f[1], f[2 + 1], f[4 + 1] = 0.5, 0.25, 2.0
    pen[6 + 1] = 2
    hist[1, :7] = torch.tensor([6, 1, 3, 3, 3, 4, 5], dtype=torch.int32)
    hist[0, :3] = torch.tensor([2, 0, 7], dtype=torch.int32)  # slot 0: neutral parameters, ignored
    x = torch.tensor([[2.0, -1.0, 0.5, 4.0, -3.0, 1.0, 0.0, -2.0]] * 2)
    ref.sample_penalties(x, None, pen, hist)
    assert x[0].tolist() == [2.0, -1.0, 0.5, 4.0, -3.0, 1.0, 0.0, -2.0]
    # token 3: 4 / 2 = 2, - 0.25 * 2 = 1.5, - 0.5 = 1.0 (presence / frequency first would give 1.5)
    assert x[1].tolist() == [2.0, -2.0, 0.5, 1.0, -6.75, -0.25, 0.0, -2.0]
    # an inactive row and a shard that holds none of the tokens stay as they are
    y = torch.tensor([[2.0, -1.0, 0.5, 4.0, -3.0, 1.0, 0.0, -2.0]] * 2)
    ref.sample_penalties(y, torch.tensor([1, 0], dtype=torch.int32), pen, hist)
    ref.sample_penalties(y, None, pen, hist, vocab_offset=8)
    assert y[1].tolist() == [2.0, -1.0, 0.5, 4.0, -3.0, 1.0, 0.0, -2.0]
    # the second shard of a 4 + 4 split sees tokens 4 and 5 only
    z = torch.tensor([[-3.0, 1.0, 0.0, -2.0]] * 2)
    ref.sample_penalties(z, None, pen, hist, vocab_offset=4)
    assert z[1].tolist() == [-6.75, -0.25, 0.0, -2.0]
    # the append: penalised slots only
    ref.sample_hist_append(torch.tensor([7, 7], dtype=torch.int32), None, None, pen, hist)
    assert hist[1, :8].tolist() == [7, 1, 3, 3, 3, 4, 5, 7] and hist[0, :3].tolist() == [2, 0, 7]


# ------------------------------------------------------------------------------------------------ CPU engine
_W = {}


def _engine(num_blocks=256, max_batch=4, compact=True):
    if "w" not in _W:
        _W["w"] = convert_standard(TINY, init_standard_weights(TINY, seed=11))
    r = ModelRunner(_W["w"], num_blocks=num_blocks, max_batch=max_batch, max_model_len=512, device="cpu",
                    use_graphs=False)
    e = LLMEngine(r, eos_id=-1, prefill_budget=256)
    if not compact:
        e._compact = lambda: None
    return e


def _prompt(i, n):
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randint(3, TINY.vocab_size, (n,), generator=g).tolist()


def _streams(e, reqs, max_steps=4000):
    """reqs = [(conv, prompt, SamplingParams, step_to_add)] -> conv -> [token ids]."""
    out = {c: [] for c, *_ in reqs}
    for step in range(max_steps):
        for c, p, sp, at in reqs:
            if at == step:
                e.add_request(c, p, sp)
        for ev in e.step():
            if not ev.done:
                out[ev.conversation_id].append(ev.token_id)
        if step > max(at for *_, at in reqs) and not e.has_work():
            break
    assert not e.has_work(), "engine did not drain"
    return out


def _greedy(mt, **kw):
    return SamplingParams(temperature=0.0, max_tokens=mt, ignore_eos=True, **kw)


def test_neutral_values_change_nothing():
    p = _prompt(0, 24)
    want = _streams(_engine(), [("a", p, _greedy(24), 0)])["a"]
    e = _engine()
    got = _streams(e, [("a", p, _greedy(24, presence_penalty=0.0, frequency_penalty=0.0, repetition_penalty=1.0), 0)])
    assert got["a"] == want
    assert not e.r.hist_used and not e._pen_live  # nothing was uploaded for it


def test_huge_presence_penalty_never_repeats_a_token():
    p, n = [7] * 33, 40
    plain = _streams(_engine(), [("a", p, _greedy(n), 0)])["a"]
    assert len(plain) == n and len(set(plain)) < n  # the unpenalised greedy stream does repeat a token
    got = _streams(_engine(), [("a", p, _greedy(n, presence_penalty=1e4), 0)])["a"]
    assert len(got) == n and len(set(got)) == n


PEN = dict(presence_penalty=0.6, frequency_penalty=0.4, repetition_penalty=1.3)


def test_preempted_streams_resume_token_exact():
    reqs = [(f"c{i}", _prompt(i, 20 + 7 * i), _greedy(50 + 5 * i, **PEN), i // 2) for i in range(5)]
    want = _streams(_engine(num_blocks=256), reqs)
    e = _engine(num_blocks=10)
    got = _streams(e, reqs)
    assert e.stats["preemptions"] > 0
    assert got == want
    assert want != _streams(_engine(num_blocks=256), [(c, p, _greedy(sp.max_tokens), at) for c, p, sp, at in reqs])


def test_compaction_keeps_penalised_streams():
    reqs = [(f"c{i}", _prompt(i, 12), _greedy(6 if i < 6 else 40, **PEN), 0) for i in range(8)]
    e = _engine(num_blocks=128, max_batch=8)
    got = _streams(e, reqs)
    assert e.stats["compactions"] > 0
    assert got == _streams(_engine(num_blocks=128, max_batch=8, compact=False), reqs)


# ------------------------------------------------------------------------------------------------ TP over gloo
TP_PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 150)), [11] * 20]
TP_TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]
TP_PENS = [(0.0, 0.0, 1.0), (1.5, 0.5, 1.4), (0.5, 0.0, 1.8)]


def _tp_generate(rank, world, pens=TP_PENS, steps=12):
    std = init_standard_weights(TINY, seed=3)
    comm = TPComm(rank=rank, size=world, group=None) if world > 1 else TPComm()
    w = convert_standard(TINY, std, tp_rank=rank, tp_size=world)
    r = ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device="cpu", comm=comm, use_graphs=False)
    for i, bt in enumerate(TP_TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
        r.presence[i], r.frequency[i], r.repetition[i] = pens[i]
        r.n_prompt[i] = len(TP_PROMPTS[i])
        if pens[i] != (0.0, 0.0, 1.0):
            r.set_history(i, TP_PROMPTS[i], len(TP_PROMPTS[i]))
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
def test_tp2_with_penalties_matches_tp1():
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_tp_worker, args=(2, _port(), out), nprocs=2, join=True)
        res = [out[r] for r in range(2)]
    assert res[0] == res[1], "TP ranks disagree on the sampled tokens"
    one = _tp_generate(0, 1)
    assert res[0] == one
    plain = _tp_generate(0, 1, pens=[(0.0, 0.0, 1.0)] * 3)
    assert plain[0] == one[0] and plain[1:] != one[1:]  # the penalties did steer the penalised streams


def test_plan_carries_the_penalties_bit_exactly():
    sp = SamplingParams(temperature=0.7, top_p=0.9, max_tokens=5, presence_penalty=0.1, frequency_penalty=-1.7,
                        repetition_penalty=1.3)
    plan = tpmod.Plan(step=True, adds=[(7, [1, 2, 3], sp, 123456789), (8, [4], SamplingParams(), 5)])
    once = plan.roundtrip()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    got = once.adds[0][2]
    assert (got.presence_penalty, got.frequency_penalty, got.repetition_penalty) == (f32(0.1), f32(-1.7), f32(1.3))
    dflt = once.adds[1][2]
    assert (dflt.presence_penalty, dflt.frequency_penalty, dflt.repetition_penalty) == (0.0, 0.0, 1.0)
    assert once.adds[0][1] == [1, 2, 3] and once.adds[1][1] == [4]
    twice = once.roundtrip()
    assert twice.encode() == once.encode() and twice.adds == once.adds  # a fixed point
    msgs = tpmod._messages(tpmod.Plan(step=True), 1024)
    assert len(msgs) == 1 and len(msgs[0]) == 6  # the idle step is still the 6-word header


# ------------------------------------------------------------------------------------------------ HTTP / DP
@pytest.fixture
def rt():
    r = rtmod.load().Runtime({"sse_port": 0, "origin_port": 0, "metrics_port": 0, "resp_port": 0, "io_threads": 2,
                              "host": H, "first_token_timeout_ms": 200})
    r.start()
    r.set_local_engine(True)  # requests queue up, nothing generates
    yield r
    r.stop()


def _post(rt, route, extra, role="origin"):
    body = {"message": "hi"} if route == "/chat" else {"messages": [{"role": "user", "content": "hi"}]}
    raw = extra if isinstance(extra, bytes) else json.dumps({**body, **extra}).encode()
    return request(H, rt.bound_port(role), "POST", route, raw, timeout=10)


def _pens(q):
    return q["presence_penalty"], q["frequency_penalty"], q["repetition_penalty"]


@pytest.mark.parametrize("route", ["/chat", "/v1/chat/completions"])
def test_penalty_fields_reach_the_queued_request(rt, route):
    _post(rt, route, {"presence_penalty": 1.5, "frequency_penalty": -2, "repetition_penalty": 0.25})
    (q,) = rt.poll_requests(10, 1000)
    assert _pens(q) == (1.5, -2.0, 0.25)
    _post(rt, route, {"max_tokens": 3})
    (q,) = rt.poll_requests(10, 1000)
    assert _pens(q) == (0.0, 0.0, 1.0)  # absent: the neutral values
    _post(rt, route, {"presence_penalty": 2, "frequency_penalty": 2.0, "repetition_penalty": 2})  # the bounds
    (q,) = rt.poll_requests(10, 1000)
    assert _pens(q) == (2.0, 2.0, 2.0)


BAD = [({"presence_penalty": 2.5}, "presence_penalty must be a number in [-2, 2]"),
       ({"presence_penalty": -2.01}, "presence_penalty must be a number in [-2, 2]"),
       ({"presence_penalty": "1"}, "presence_penalty must be a number in [-2, 2]"),
       ({"frequency_penalty": 3}, "frequency_penalty must be a number in [-2, 2]"),
       ({"frequency_penalty": None}, "frequency_penalty must be a number in [-2, 2]"),
       ({"frequency_penalty": True}, "frequency_penalty must be a number in [-2, 2]"),
       ({"repetition_penalty": 0}, "repetition_penalty must be a number in (0, 2]"),
       ({"repetition_penalty": -1}, "repetition_penalty must be a number in (0, 2]"),
       ({"repetition_penalty": 2.5}, "repetition_penalty must be a number in (0, 2]"),
       ({"repetition_penalty": [1]}, "repetition_penalty must be a number in (0, 2]")]


@pytest.mark.parametrize("extra, msg", BAD)
def test_bad_penalty_fields_are_a_400(rt, extra, msg):
    for role in ("edge", "origin"):
        r = _post(rt, "/chat", extra, role)
        assert r.status == 400 and r.body == (msg + "\n").encode()
    r = _post(rt, "/v1/chat/completions", extra)
    assert r.status == 400 and json.loads(r.body)["message"] == msg
    assert rt.poll_requests(10, 0) == []


def test_non_finite_penalty_is_a_400(rt):
    r = _post(rt, "/chat", b'{"message":"hi","presence_penalty":1e400}')
    assert r.status == 400 and r.body == b"presence_penalty must be a number in [-2, 2]\n"
    r = _post(rt, "/v1/chat/completions",
              b'{"messages":[{"role":"user","content":"hi"}],"repetition_penalty":1e400}')
    assert r.status == 400 and json.loads(r.body)["message"] == "repetition_penalty must be a number in (0, 2]"
    assert rt.poll_requests(10, 0) == []


def test_serving_loop_maps_the_request_to_sampling_params():
    from distributed_sse_for_llm_response_amd.serving.app import EngineLoop

    class _E:
        default_params = SamplingParams()

    loop = EngineLoop.__new__(EngineLoop)
    loop.engine = _E()
    base = {"temperature": -1, "top_p": -1, "top_k": -1, "max_tokens": -1, "seed": -1}
    sp = loop._params({**base, "presence_penalty": 0.5, "frequency_penalty": -0.25, "repetition_penalty": 1.5})
    assert (sp.presence_penalty, sp.frequency_penalty, sp.repetition_penalty) == (0.5, -0.25, 1.5)
    assert sp.penalised() and not loop._params(base).penalised()


def test_dp_ring_delivers_the_penalties():
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
        while not stop.is_set() and not chan.shutdown_requested():
            for req in chan.poll_requests(16, 50):
                seen.append(req)
                c = req["conversation_id"]
                chan.publish_tokens([c], [10], [1], [False], 0, [])
                chan.publish_tokens([c], [-1], [2], [True], 0, ["[DONE]"])

    t = threading.Thread(target=worker, daemon=True)
    t.start()
    try:
        deadline = time.time() + 10
        while time.time() < deadline and not all(i["ready"] for i in r.dp_workers()):
            time.sleep(0.02)
        a = request(H, r.bound_port("edge"), "POST", "/chat",
                    {"message": "hi", "conversation_id": "p1", "presence_penalty": -0.5, "frequency_penalty": 0.75,
                     "repetition_penalty": 1.25}, timeout=30)
        b = request(H, r.bound_port("edge"), "POST", "/chat", {"message": "hi", "conversation_id": "p2"}, timeout=30)
        assert a.status == 200 and b.status == 200
        by = {q["conversation_id"]: q for q in seen}
        assert _pens(by["p1"]) == (-0.5, 0.75, 1.25) and _pens(by["p2"]) == (0.0, 0.0, 1.0)
        assert by["p1"]["message"] == "hi"  # the fields after the new ones still decode
    finally:
        stop.set()
        t.join(5)
        r.stop()
