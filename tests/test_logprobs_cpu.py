"""logprobs / top_logprobs without a GPU: the reference semantics by hand, the CPU engine (neighbours, preemption,
TP over gloo), the TP plan's wire form, the DP ring, the HTTP validation and the OpenAI responses end to end."""
import json
import math
import os
import socket
import threading
import time
import uuid

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd import runtime as rtmod
from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as ref
from distributed_sse_for_llm_response_amd.parallel.comm import TPComm
from distributed_sse_for_llm_response_amd.serving import tp as tpmod
from distributed_sse_for_llm_response_amd.serving.app import EngineLoop, ServingApp
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from distributed_sse_for_llm_response_amd.utils.sse_client import request

H = "127.0.0.1"
TOL = 2e-5  # the bound of tests/test_logprobs_gpu.py


# ------------------------------------------------------------------------------------------------ semantics
def test_reference_semantics_by_hand():
    """V = 6, x = [0, ln 2, ln 2, -inf, ln 4, 0]: sum exp = 1 + 2 + 2 + 0 + 4 + 1 = 10, so lp = x - ln 10.  Order:
    4 (ln 4), then the tie 1, 2 (ln 2) by ascending id, then the tie 0, 5, then 3."""
    ln = math.log
    x = torch.tensor([[0.0, ln(2), ln(2), float("-inf"), ln(4), 0.0]] * 4)
    lp_meta = torch.tensor([2, -1, 6, 20], dtype=torch.int32)  # N = 2 cuts the tie 1 | 2; off; N = V; N > V
    rec = torch.full((1, 4, ops.LP_REC), 7.0)
    chosen = torch.full((1, 4), 7.0)
    ring = torch.full((2, 4, ops.LP_OUT), 7.0)
    ref.logprob_stats(x, None, lp_meta, None, rec[0])
    ref.logprob_chosen(x, torch.tensor([2, 2, 3, 5], dtype=torch.int32), None, lp_meta, None, chosen[0])
    ref.logprob_finish(rec, chosen, None, lp_meta, None, ring, ring_row=1)
    assert bool((ring[0] == 7.0).all()) and bool((ring[1, 1] == 7.0).all()) and bool((rec[0, 1] == 7.0).all())
    ids = ring.view(torch.int32)[1, :, 1:21]
    assert ids[0].tolist() == [4, 1] + [-1] * 18
    assert ids[2].tolist() == [4, 1, 2, 0, 5, 3] + [-1] * 14 and ids[3].tolist() == ids[2].tolist()
    assert float(ring[1, 0, 0]) == pytest.approx(ln(2) - ln(10), abs=1e-6)  # the sampled token 2 is not in the top 2
    assert ring[1, 0, 21:23].tolist() == pytest.approx([ln(4) - ln(10), ln(2) - ln(10)], abs=1e-6)
    assert float(ring[1, 2, 0]) == float("-inf") and float(ring[1, 2, 26]) == float("-inf")  # token 3: -inf
    assert float(ring[1, 3, 0]) == pytest.approx(-ln(10), abs=1e-6)
    assert float(rec[0, 0, 0]) == pytest.approx(ln(4)) and float(rec[0, 0, 1]) == pytest.approx(2.5)
    # two shards of 3 (the tie 1 | 2 inside shard 0, the tie 0 | 5 across the shards) and an all -inf third shard
    rec3, ch3 = torch.zeros(3, 4, ops.LP_REC), torch.zeros(3, 4)
    xs = [x[:, :3].contiguous(), x[:, 3:].contiguous(), torch.full((4, 3), float("-inf"))]
    nid = torch.tensor([2, 2, 3, 5], dtype=torch.int32)
    for w in range(3):
        ref.logprob_stats(xs[w], None, lp_meta, None, rec3[w], None, 3 * w)
        ref.logprob_chosen(xs[w], nid, None, lp_meta, None, ch3[w], 3 * w)
    ring3 = torch.full((2, 4, ops.LP_OUT), 7.0)
    ref.logprob_finish(rec3, ch3, None, lp_meta, None, ring3, ring_row=1)
    assert ring3.view(torch.int32)[1, 0, 1:21].tolist() == ids[0].tolist()
    assert ring3.view(torch.int32)[1, 2, 1:7].tolist() == [4, 1, 2, 0, 5, 3]
    assert ring3.view(torch.int32)[1, 3, 1:10].tolist() == [4, 1, 2, 0, 5, 3, 6, 7, 8]  # N > V: the -inf ids follow
    fin = torch.isfinite(ring[1])
    assert float((ring3[1][fin] - ring[1][fin]).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ CPU engine
_W = {}


def _engine(num_blocks=256, max_batch=4):
    if "w" not in _W:
        _W["w"] = convert_standard(TINY, init_standard_weights(TINY, seed=11))
    r = ModelRunner(_W["w"], num_blocks=num_blocks, max_batch=max_batch, max_model_len=512, device="cpu",
                    use_graphs=False)
    return LLMEngine(r, eos_id=-1, prefill_budget=256)


def _prompt(i, n):
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randint(3, TINY.vocab_size, (n,), generator=g).tolist()


def _streams(e, reqs, max_steps=4000):
    """reqs = [(conv, prompt, SamplingParams, step_to_add)] -> conv -> [token events]."""
    out = {c: [] for c, *_ in reqs}
    for step in range(max_steps):
        for c, p, sp, at in reqs:
            if at == step:
                e.add_request(c, p, sp)
        for ev in e.step():
            if not ev.done:
                out[ev.conversation_id].append(ev)
        if step > max(at for *_, at in reqs) and not e.has_work():
            break
    assert not e.has_work(), "engine did not drain"
    return out


def _sp(mt, **kw):
    return SamplingParams(temperature=kw.pop("temperature", 0.0), max_tokens=mt, ignore_eos=True, **kw)


def _well_formed(ev, n):
    assert ev.logprob is not None and ev.logprob <= 0.0 and len(ev.top) == n
    vals = [v for _, v in ev.top]
    assert all(a > b or (a == b and i < j) for (i, a), (j, b) in zip(ev.top, ev.top[1:]))  # the order rule
    assert sum(math.exp(v) for v in vals) <= 1.0 + 1e-5
    for t, v in ev.top:
        if t == ev.token_id:
            assert v == ev.logprob


def test_engine_attaches_logprobs_to_requesting_streams_only():
    p = [_prompt(i, 20 + 3 * i) for i in range(3)]
    plain = _streams(_engine(), [("a", p[0], _sp(12), 0), ("b", p[1], _sp(12), 0), ("c", p[2], _sp(12), 2)])
    e = _engine()
    got = _streams(e, [("a", p[0], _sp(12, logprobs=5), 0), ("b", p[1], _sp(12), 0),
                       ("c", p[2], _sp(12, logprobs=0, temperature=0.9, top_k=1, seed=5), 2)])
    for c in "abc":  # the same tokens as without the feature (top_k = 1 sampling is the argmax too)
        assert [ev.token_id for ev in got[c]] == [ev.token_id for ev in plain[c]] and len(got[c]) == 12
    assert all(ev.logprob is None and ev.top is None for ev in got["b"] + plain["a"])
    for ev in got["a"]:
        _well_formed(ev, 5)
        assert ev.top[0][0] == ev.token_id  # greedy: the sampled token is top entry 0
    for ev in got["c"]:
        _well_formed(ev, 0)
    # with top_k = 1 sampling and N >= 1 the sampled token is top entry 0
    e2 = _engine()
    evs = _streams(e2, [("k", p[0], _sp(6, logprobs=2, temperature=0.8, top_k=1, seed=9), 0)])["k"]
    assert all(ev.top[0][0] == ev.token_id for ev in evs)
    # against float64 on the step's own logits: the lone stream's last decode step's row is still in the runner
    lp = torch.log_softmax(e2.r.logits[0].double(), dim=0)
    assert abs(float(lp[evs[-1].token_id]) - evs[-1].logprob) <= TOL
    assert abs(float(lp[evs[-1].top[1][0]]) - evs[-1].top[1][1]) <= TOL
    assert _engine().r.lp_used is False and e.r.lp_used


def test_logprobs_with_penalties_report_the_raw_distribution():
    """A stream with both: its tokens are the penalised stream's, its logprobs come from the un-penalised logits
    (rank 0 is the raw argmax, which a huge presence penalty stops it from sampling twice)."""
    p, n = [7] * 33, 24
    pen = _streams(_engine(), [("a", p, _sp(n, presence_penalty=1e4), 0)])["a"]
    got = _streams(_engine(), [("a", p, _sp(n, presence_penalty=1e4, logprobs=3), 0)])["a"]
    assert [ev.token_id for ev in got] == [ev.token_id for ev in pen] and len({ev.token_id for ev in got}) == n
    for ev in got:
        _well_formed(ev, 3)
    assert any(ev.top[0][0] != ev.token_id for ev in got)  # the raw argmax was penalised away at least once
    assert all(ev.logprob > -50.0 for ev in got)  # raw values: a penalised logit (x - 1e4) would be < -1e3


def _check_every_sampling_call(r):
    """Wrap the runner's finish pass: after every call (decode step or first-token sampling, a re-prefill's too),
    each row that is on must hold at its own (ring row, slot) the ids of the stable descending sort and the float64
    log-softmax of THAT call's logits within the bound.  Returns the list of (sampled id, its logprob) it checked."""
    orig, seen = r._logprob_finish, []

    def wrapped(logits, raw, ids, active, row_slot, bufs, **ring):
        orig(logits, raw, ids, active, row_slot, bufs, **ring)
        assert raw is None  # (no penalties here: `logits` are the raw values)
        row = int(ring["ring_counter"][0]) % r.lp_ring.shape[0] if "ring_counter" in ring else int(ring["ring_row"])
        for b in range(logits.shape[0]):
            if active is not None and not int(active[b]):
                continue
            slot = int(row_slot[b]) if row_slot is not None else b
            n = int(r.lp_meta[slot])
            if n < 0:
                continue
            lp = torch.log_softmax(logits[b].double(), dim=0)
            w = r.lp_ring[row, slot]
            want = torch.sort(logits[b], descending=True, stable=True).indices[:n].tolist()
            assert w.view(torch.int32)[1:1 + n].tolist() == want
            assert abs(float(w[0]) - float(lp[int(ids[b])])) <= TOL
            assert all(abs(float(w[21 + j]) - float(lp[t])) <= TOL for j, t in enumerate(want))
            seen.append((int(ids[b]), float(w[0])))

    r._logprob_finish = wrapped
    return seen


def test_preempted_stream_resumes_with_logprobs_on_new_tokens_only():
    reqs = [(f"c{i}", _prompt(i, 20 + 7 * i), _sp(50 + 5 * i, logprobs=2), i // 2) for i in range(5)]
    want = _streams(_engine(num_blocks=256), reqs)
    e = _engine(num_blocks=10)
    checked = _check_every_sampling_call(e.r)
    got = _streams(e, reqs)
    assert e.stats["preemptions"] > 0
    checked = set(checked)
    for c in want:  # every published token exactly once, in order, each with its own logprobs
        assert [ev.sequence for ev in got[c]] == list(range(1, len(want[c]) + 1))
        assert [ev.token_id for ev in got[c]] == [ev.token_id for ev in want[c]]
        for a in got[c]:
            _well_formed(a, 2)
            # the event carries a row that was checked against float64 on its own step's logits (a re-prefilled
            # context runs the prompt kernels' arithmetic, so the un-preempted run's values are no reference)
            assert a.top[0][0] == a.token_id and (a.token_id, a.logprob) in checked


# ------------------------------------------------------------------------------------------------ TP over gloo
TP_PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 150)), [11] * 20]
TP_TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]
TP_LPS = [-1, 20, 4]


def _tp_logits():
    """Global logits [3, V] shared by every TP degree: randn * 4 with a tie planted across the shard boundary at
    rank 4 of row 2 (ids 7 and V/2 + 7) and inside a shard at rank 20 of row 1."""
    g = torch.Generator().manual_seed(21)
    x = torch.randn(3, TINY.vocab_size, generator=g) * 4.0
    V = TINY.vocab_size
    o = torch.sort(x[2], descending=True, stable=True).indices
    v = float(x[2, o[3]])
    x[2, o[3]] = -40.0
    x[2, 7], x[2, V // 2 + 7] = v, v
    o = torch.sort(x[1], descending=True, stable=True).indices
    x[1, o[20]] = x[1, o[19]]
    return x


def _tp_generate(rank, world, steps=4):
    """(a) The sampling site on GIVEN logits: every rank gets its column slice of _tp_logits() in runner.logits and
    runs the decode step's sampling (_sample_commit: stats, candidates, all-gathers, pick, chosen, finish).  The
    model's own logits differ between TP degrees (the bf16 all-reduce order: up to 1.6e-2 on TINY, more than the
    gaps between neighbouring ranks), so equal ids and the 2e-5 bound against TP = 1 are only defined on equal
    logits.  (b) The model end to end: prefill + decode steps, returning the tokens and each step's own logits."""
    std = init_standard_weights(TINY, seed=3)
    comm = TPComm(rank=rank, size=world, group=None) if world > 1 else TPComm()
    w = convert_standard(TINY, std, tp_rank=rank, tp_size=world)
    r = ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device="cpu", comm=comm, use_graphs=False)
    for i, bt in enumerate(TP_TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
        r.lp_meta[i] = TP_LPS[i]
    r.enable_logprobs()
    r.active[:3] = 1
    r.logits[:3] = _tp_logits()[:, w.vocab_offset:w.vocab_offset + w.vocab_local]
    r._sample_commit(4)
    given = (r.ids[:3].tolist(), r.lp_ring[0, :3].clone())
    r.active[:3] = 0
    r.positions.zero_()
    r.prefill([PrefillSeq(i, p, 0, TP_TABLES[i], True) for i, p in enumerate(TP_PROMPTS)], ring_row=0)
    r.active[:3] = 1
    gen = [[int(r.ids[i])] for i in range(3)]
    rows = []
    for step in range(steps):
        r.decode(4)
        for i in range(3):
            gen[i].append(int(r.ids[i]))
        rows.append((r.logits[:3].clone(), r.lp_ring[step % r.lp_ring.shape[0], :3].clone()))
    return given, gen, rows


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


def _ids(row):
    return row.view(torch.int32)[1:21].tolist()


@pytest.mark.timeout(600)
def test_tp2_logprobs_match_tp1():
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_tp_worker, args=(2, _port(), out), nprocs=2, join=True)
        res = [out[r] for r in range(2)]
    one = _tp_generate(0, 1)
    # (a) the same logits: the same sampled ids, the same top ids, values within the bound; and against float64
    x = _tp_logits()
    V = TINY.vocab_size
    assert res[0][0][0] == res[1][0][0] == one[0][0] == x.argmax(dim=1).tolist()
    for i in range(3):
        r0, r1, r = res[0][0][1][i], res[1][0][1][i], one[0][1][i]
        assert torch.equal(r0.view(torch.int32), r1.view(torch.int32))  # the ranks agree bit for bit
        if TP_LPS[i] < 0:
            assert bool((r0 == 0).all()) and bool((r == 0).all())  # never written
            continue
        n = TP_LPS[i]
        want = torch.sort(x[i], descending=True, stable=True).indices[:n].tolist()
        assert _ids(r0)[:n] == _ids(r)[:n] == want and _ids(r0)[n:] == [-1] * (20 - n)
        lp = torch.log_softmax(x[i].double(), dim=0)
        for got in (r0, r):
            assert abs(float(got[0]) - float(lp[one[0][0][i]])) <= TOL
            assert max(abs(float(got[21 + j]) - float(lp[t])) for j, t in enumerate(want)) <= TOL
        assert float((r0[21:21 + n] - r[21:21 + n]).abs().max()) <= TOL and abs(float(r0[0] - r[0])) <= TOL
    assert 7 in _ids(one[0][1][2])[:4] and V // 2 + 7 not in _ids(one[0][1][2])[:4]  # the cross-shard tie: lower id
    # (b) the model: the ranks agree, sample TP = 1's tokens, and report the float64 log-softmax of their own logits
    assert res[0][1] == res[1][1] == one[1]
    for step, ((l0, w0), (l1, w1)) in enumerate(zip(res[0][2], res[1][2])):
        assert torch.equal(w0.view(torch.int32), w1.view(torch.int32))
        full = torch.cat([l0, l1], dim=1)
        for i in (1, 2):
            n = TP_LPS[i]
            lp = torch.log_softmax(full[i].double(), dim=0)
            want = torch.sort(full[i], descending=True, stable=True).indices[:n].tolist()
            assert _ids(w0[i])[:n] == want and want[0] == res[0][1][i][step + 1]
            assert max(abs(float(w0[i, 21 + j]) - float(lp[t])) for j, t in enumerate(want)) <= TOL
            assert abs(float(w0[i, 0]) - float(lp[want[0]])) <= TOL


def test_plan_carries_logprobs_and_is_a_fixed_point():
    plan = tpmod.Plan(step=True, adds=[(7, [1, 2, 3], SamplingParams(logprobs=20), 123456789),
                                       (8, [4], SamplingParams(), 5), (9, [5, 6], SamplingParams(logprobs=0), 6)])
    once = plan.roundtrip()
    assert [a[2].logprobs for a in once.adds] == [20, -1, 0]
    assert [a[1] for a in once.adds] == [[1, 2, 3], [4], [5, 6]]
    twice = once.roundtrip()
    assert twice.encode() == once.encode() and twice.adds == once.adds
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
    return request(H, rt.bound_port(role), "POST", route, json.dumps({**body, **extra}).encode(), timeout=10)


def test_logprob_fields_reach_the_queued_request(rt):
    for extra, want in (({"logprobs": True, "top_logprobs": 5}, 5), ({"logprobs": True}, 0), ({"max_tokens": 3}, -1),
                        ({"logprobs": None, "top_logprobs": None}, -1), ({"logprobs": True, "top_logprobs": None}, 0),
                        ({"logprobs": None}, -1),
                        ({"logprobs": False}, -1), ({"logprobs": True, "top_logprobs": 20}, 20),
                        ({"logprobs": True, "top_logprobs": 0}, 0)):
        _post(rt, "/v1/chat/completions", extra)
        (q,) = rt.poll_requests(10, 1000)
        assert q["logprobs"] == want, extra
    _post(rt, "/chat", {"logprobs": True, "top_logprobs": 5})  # /chat keeps the reference's contract: ignored
    (q,) = rt.poll_requests(10, 1000)
    assert q["logprobs"] == -1


BAD = [({"top_logprobs": 3}, "top_logprobs requires logprobs to be true"),
       ({"logprobs": None, "top_logprobs": 3}, "top_logprobs requires logprobs to be true"),
       ({"logprobs": False, "top_logprobs": 3}, "top_logprobs requires logprobs to be true"),
       ({"logprobs": True, "top_logprobs": 21}, "top_logprobs must be an integer in [0, 20]"),
       ({"logprobs": True, "top_logprobs": -1}, "top_logprobs must be an integer in [0, 20]"),
       ({"logprobs": True, "top_logprobs": 2.5}, "top_logprobs must be an integer in [0, 20]"),
       ({"logprobs": True, "top_logprobs": "3"}, "top_logprobs must be an integer in [0, 20]"),
       ({"logprobs": True, "top_logprobs": True}, "top_logprobs must be an integer in [0, 20]"),
       ({"logprobs": True, "top_logprobs": 1e20}, "top_logprobs must be an integer in [0, 20]"),
       ({"logprobs": 1}, "logprobs must be a boolean"),
       ({"logprobs": "true"}, "logprobs must be a boolean")]


@pytest.mark.parametrize("extra, msg", BAD)
def test_bad_logprob_fields_are_a_400_on_the_openai_route_only(rt, extra, msg):
    r = _post(rt, "/v1/chat/completions", extra)
    assert r.status == 400 and json.loads(r.body)["message"] == msg and json.loads(r.body)["object"] == "error"
    assert rt.poll_requests(10, 0) == []
    assert _post(rt, "/chat", extra).status != 400  # /chat neither accepts nor validates them
    (q,) = rt.poll_requests(10, 1000)
    assert q["logprobs"] == -1


def test_chat_route_sse_bytes_do_not_change_with_a_logprobs_entry(rt):
    """A token published with an entry string: the /chat SSE frame is byte-for-byte the frame without one."""
    frames = []
    for conv, lp in (("lp-a", ['{"token":"x","logprob":-1.5,"bytes":[120],"top_logprobs":[]}', ""]), ("lp-b", [])):
        rt.publish_tokens([conv, conv], [-1, -1], [1, 2], [False, True], 1234, ["x", "[DONE]"], [0, 1], [-1, 3], lp)
        s = request(H, rt.bound_port("edge"), "GET", f"/stream/{conv}?replay=1", timeout=10)
        frames.append([(e.event, e.data.replace(conv, "C")) for e in s.events if e.event == "token"])
    assert frames[0] == frames[1] and "logprob" not in json.dumps(frames[0])
    assert json.loads(frames[0][0][1]) == {"conversation_id": "C", "token": "x", "sequence": 1, "done": False,
                                           "timestamp": 1234}


def test_serving_loop_maps_the_request_and_builds_the_entry():
    class _E:
        default_params = SamplingParams()

    class _Tok:
        def piece(self, i):
            return {1: "é", 2: ' "q"', 3: "z"}[i]

    loop = EngineLoop.__new__(EngineLoop)
    loop.engine, loop.tok = _E(), _Tok()
    base = {"temperature": -1, "top_p": -1, "top_k": -1, "max_tokens": -1, "seed": -1}
    assert loop._params(base).logprobs == -1 and loop._params({**base, "logprobs": 7}).logprobs == 7
    from distributed_sse_for_llm_response_amd.engine.engine import TokenEvent
    f32 = float(torch.tensor(-0.1, dtype=torch.float32))
    ev = TokenEvent("c", 1, 1, False, logprob=f32, top=[(2, f32), (3, float("-inf"))])
    d = json.loads(loop.logprobs_entry(ev))
    assert d["token"] == "é" and d["bytes"] == [0xC3, 0xA9]
    assert float(torch.tensor(d["logprob"], dtype=torch.float32)) == f32  # the digits round-trip the fp32 value
    assert d["top_logprobs"] == [{"token": ' "q"', "logprob": d["logprob"], "bytes": list(b' "q"')},
                                 {"token": "z", "logprob": -9999.0, "bytes": [122]}]
    assert loop.logprobs_entry(TokenEvent("c", 1, 1, False)) == ""
    assert loop.logprobs_entry(TokenEvent("c", -1, 2, True, text="[DONE]", logprob=-1.0)) == ""


def test_dp_ring_delivers_the_field_and_the_entry():
    mod = rtmod.load()
    r = mod.Runtime({"sse_port": 0, "origin_port": 0, "metrics_port": 0, "resp_port": -1, "io_threads": 2,
                     "host": H, "local_engine": True})
    r.set_vocab([f"tok{i}" for i in range(100)])
    prefix = f"/dsse-test-{uuid.uuid4().hex[:8]}"
    r.start_dp_router(prefix, 1, 1, 10000)
    r.start()
    seen, stop = [], threading.Event()
    entry = '{"token":"tok10","logprob":-0.25,"bytes":[116,111,107,49,48],"top_logprobs":[]}'

    def worker():
        chan = mod.DpWorker(prefix, 0, 5000)
        chan.set_ready(True)
        while not stop.is_set() and not chan.shutdown_requested():
            for req in chan.poll_requests(16, 50):
                seen.append(req)
                c = req["conversation_id"]
                chan.publish_tokens([c], [10], [1], [False], 0, [], [], [], [entry] if req["logprobs"] >= 0 else [])
                chan.publish_tokens([c], [-1], [2], [True], 0, ["[DONE]"], [2], [4])

    t = threading.Thread(target=worker, daemon=True)
    t.start()
    try:
        deadline = time.time() + 10
        while time.time() < deadline and not all(i["ready"] for i in r.dp_workers()):
            time.sleep(0.02)
        msgs = [{"role": "user", "content": "hi"}]
        a = request(H, r.bound_port("origin"), "POST", "/v1/chat/completions",
                    {"messages": msgs, "logprobs": True, "top_logprobs": 7, "repetition_penalty": 1.25}, timeout=30)
        b = request(H, r.bound_port("origin"), "POST", "/v1/chat/completions", {"messages": msgs}, timeout=30)
        assert a.status == 200 and b.status == 200
        assert sorted(q["logprobs"] for q in seen) == [-1, 7]
        assert all(q["message"] == "hi" for q in seen) and {q["repetition_penalty"] for q in seen} == {1.0, 1.25}
        da, db = json.loads(a.body), json.loads(b.body)
        assert da["choices"][0]["logprobs"] == {"content": [json.loads(entry)]} and da["usage"]["prompt_tokens"] == 4
        assert db["choices"][0]["logprobs"] is None and b'"logprobs":null' in b.body
    finally:
        stop.set()
        t.join(5)
        r.stop()


# ------------------------------------------------------------------------------------------------ inspection gate
class _Inspector:
    """POST /inspect stand-in: text containing "pw" -> redact to "[REDACTED]", else allow."""

    def __init__(self):
        import http.server

        class Handler(http.server.BaseHTTPRequestHandler):
            protocol_version = "HTTP/1.1"

            def log_message(self, *a):
                pass

            def do_POST(self):
                body = json.loads(self.rfile.read(int(self.headers["Content-Length"])))
                red = "pw" in body["data"].lower()
                out = json.dumps({"action": "redact" if red else "allow", "reason": "pw" if red else None,
                                  "redacted_content": "[REDACTED]" if red else None}).encode()
                self.send_response(200)
                self.send_header("Content-Type", "application/json")
                self.send_header("Content-Length", str(len(out)))
                self.end_headers()
                self.wfile.write(out)

        self.srv = http.server.ThreadingHTTPServer((H, 0), Handler)
        self.url = f"http://{H}:{self.srv.server_address[1]}/inspect"
        threading.Thread(target=self.srv.serve_forever, daemon=True).start()

    def close(self):
        self.srv.shutdown()


SECRET = "my pw is x"


def _entry(piece):
    return json.dumps({"token": piece, "logprob": -0.5, "bytes": list(piece.encode()),
                       "top_logprobs": [{"token": piece, "logprob": -0.5, "bytes": list(piece.encode())}]},
                      separators=(",", ":"))


@pytest.mark.parametrize("mode", ["inline", "hybrid"])
@pytest.mark.parametrize("stream", [True, False])
def test_a_redacted_token_takes_its_logprobs_entry_with_it(mode, stream):
    """The inspection gate replaces a token: neither the OpenAI stream chunks nor the non-stream body may show the
    original piece, its bytes or its alternatives through `logprobs`.  inline: the one redacted token loses its
    entry; hybrid: the held text becomes one replacement frame without one."""
    insp = _Inspector()
    r = rtmod.load().Runtime({"sse_port": 0, "origin_port": 0, "metrics_port": 0, "resp_port": -1, "io_threads": 2,
                              "host": H, "inspection_mode": mode, "inspection_endpoint": insp.url,
                              "inspection_buffer_ms": 60000})
    r.start()
    r.set_local_engine(True)
    got = []
    body = {"messages": [{"role": "user", "content": "hi"}], "logprobs": True, "top_logprobs": 1, "stream": stream}
    th = threading.Thread(target=lambda: got.append(request(H, r.bound_port("origin"), "POST", "/v1/chat/completions",
                                                            body, timeout=20, stop_on_done=False)))
    th.start()
    try:
        (q,) = r.poll_requests(10, 5000)
        conv, toks = q["conversation_id"], ["hello", SECRET, "bye"]
        assert q["logprobs"] == 1
        r.publish_tokens([conv] * 3, [-1] * 3, [1, 2, 3], [False] * 3, 0, toks, [], [], [_entry(t) for t in toks])
        r.publish_tokens([conv], [-1], [4], [True], 0, ["[DONE]"], [1], [2])  # (hybrid: the held text is judged now)
        th.join(20)
        resp = got[0]
        raw = resp.body if not stream else "".join(e.data for e in resp.events).encode()
        leaks = [SECRET.encode(), json.dumps(list(SECRET.encode()), separators=(",", ":")).encode()]
        assert resp.status == 200 and b"[REDACTED]" in raw and not any(x in raw for x in leaks)
        if stream:
            content = [json.loads(e.data)["choices"][0] for e in resp.events if e.data != "[DONE]"][1:-1]
            if mode == "inline":
                assert [c["delta"]["content"] for c in content] == ["hello", "[REDACTED]", "bye"]
                assert content[1]["logprobs"] is None
                assert [c["logprobs"]["content"][0]["token"] for c in (content[0], content[2])] == ["hello", "bye"]
            else:
                assert [(c["delta"]["content"], c["logprobs"]) for c in content] == [("[REDACTED]", None)]
        else:
            d = json.loads(raw)
            assert d["choices"][0]["message"]["content"] == ("hello[REDACTED]bye" if mode == "inline" else "[REDACTED]")
            assert d["choices"][0]["logprobs"] is None  # not one entry per completion token: none at all
            assert d["usage"]["completion_tokens"] == (3 if mode == "inline" else 1)
    finally:
        th.join(1)
        r.stop()
        insp.close()


def test_non_stream_body_without_entries_says_null(rt):
    """A request with logprobs whose frames carry no entry (the stub generator, an engine behind a relay edge): the
    non-stream body keeps null, as the stream chunks do."""
    got = []
    body = {"messages": [{"role": "user", "content": "hi"}], "logprobs": True}
    th = threading.Thread(target=lambda: got.append(request(H, rt.bound_port("origin"), "POST", "/v1/chat/completions",
                                                            body, timeout=20)))
    th.start()
    (q,) = rt.poll_requests(10, 5000)
    rt.publish_tokens([q["conversation_id"]] * 2, [-1, -1], [1, 2], [False, True], 0, ["x", "[DONE]"], [0, 1], [-1, 2])
    th.join(20)
    d = json.loads(got[0].body)
    assert d["choices"][0]["message"]["content"] == "x" and d["choices"][0]["logprobs"] is None
    assert b'"logprobs":null' in got[0].body


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def cpu_app():
    c = ServeConfig(host=H, sse_port=0, origin_port=0, metrics_port=0, resp_port=0, io_threads=2)
    c.engine, c.max_tokens, c.temperature = "cpu", 8, 0.0
    app = ServingApp(c).start()
    yield app
    app.stop()


def _check_entries(app, entries, text, n):
    assert "".join(e["token"] for e in entries) == text
    pieces = app.tok.pieces()
    for e in entries:
        assert e["token"] in pieces and e["bytes"] == list(e["token"].encode("utf-8"))
        assert e["logprob"] <= 0 and len(e["top_logprobs"]) == n
        vals = [t["logprob"] for t in e["top_logprobs"]]
        assert vals == sorted(vals, reverse=True) and vals[0] == e["logprob"]  # greedy: the sampled token is rank 0
        assert e["top_logprobs"][0]["token"] == e["token"]
        assert all(t["bytes"] == list(t["token"].encode("utf-8")) and set(t) == {"token", "logprob", "bytes"}
                   for t in e["top_logprobs"])


def test_openai_responses_carry_logprobs_end_to_end(cpu_app):
    msgs = [{"role": "user", "content": "Why stream tokens?"}]
    body = {"messages": msgs, "max_tokens": 5, "logprobs": True, "top_logprobs": 3}
    r = request(H, cpu_app.port("origin"), "POST", "/v1/chat/completions", body, timeout=60)
    d = json.loads(r.body)
    entries = d["choices"][0]["logprobs"]["content"]
    assert len(entries) == d["usage"]["completion_tokens"] == 5
    _check_entries(cpu_app, entries, d["choices"][0]["message"]["content"], 3)
    s = request(H, cpu_app.port("origin"), "POST", "/v1/chat/completions", {**body, "stream": True}, timeout=60,
                stop_on_done=False)
    chunks = [json.loads(e.data) for e in s.events if e.data != "[DONE]"]
    assert s.events[-1].data == "[DONE]"
    assert chunks[0]["choices"][0]["logprobs"] is None and chunks[-1]["choices"][0]["logprobs"] is None  # role, finish
    content = chunks[1:-1]
    assert len(content) == 5 and all(len(c["choices"][0]["logprobs"]["content"]) == 1 for c in content)
    streamed = [c["choices"][0]["logprobs"]["content"][0] for c in content]
    _check_entries(cpu_app, streamed, "".join(c["choices"][0]["delta"]["content"] for c in content), 3)
    assert streamed == entries  # greedy, the same conversation: the same entries either way
    # without the fields: null everywhere, and the same completion
    p = request(H, cpu_app.port("origin"), "POST", "/v1/chat/completions", {"messages": msgs, "max_tokens": 5},
                timeout=60)
    assert b'"logprobs":null' in p.body and json.loads(p.body)["choices"][0]["message"] == d["choices"][0]["message"]
    ps = request(H, cpu_app.port("origin"), "POST", "/v1/chat/completions",
                 {"messages": msgs, "max_tokens": 5, "stream": True}, timeout=60, stop_on_done=False)
    assert all(json.loads(e.data)["choices"][0]["logprobs"] is None for e in ps.events if e.data != "[DONE]")
    # /chat ignores the fields: the reference's token events, nothing else
    c = request(H, cpu_app.port("edge"), "POST", "/chat", {"message": "Why stream tokens?", "max_tokens": 3,
                                                            "logprobs": True, "top_logprobs": 3}, timeout=60)
    toks = [e.json() for e in c.events if e.event == "token"]
    assert toks[-1]["done"] and all(set(t) <= {"conversation_id", "token", "sequence", "done", "timestamp"} for t in toks)
