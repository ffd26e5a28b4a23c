"""guided_regex / guided_choice on the CPU: the reference ops on a hand-built table, the engine end to end with the
synthetic tokenizer (matches, prefixes, stuck patterns, preemption, unguided neighbours, pool pressure), both HTTP
routes, the DP ring and the TP plan."""
import json
import os
import re
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
from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.models.tokenizer import SyntheticTokenizer
from distributed_sse_for_llm_response_amd.parallel.comm import TPComm
from distributed_sse_for_llm_response_amd.serving import tp as tpmod
from distributed_sse_for_llm_response_amd.serving.app import ServingApp
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from distributed_sse_for_llm_response_amd.utils.sse_client import request

H = "127.0.0.1"
DEAD = ops.GUIDE_DEAD
NEG = float("-inf")


def compile_(pattern):
    n, tab, acc = rtmod.load().guide_compile(pattern)
    return np.frombuffer(tab, dtype=np.uint16).reshape(n, 256), np.frombuffer(acc, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ reference ops
PIECES = ["<unk>", "<s>", "</s>", "a", "b", "c", "ab", "bc", "abc", "x", "", "bbbc", "ca", "é"]
EOS3 = 2


def _hand_table():
    """0 -a-> 1; 1 -b-> 1, 1 -c-> 2; state 2 accepts and has no way on: the language ab*c."""
    tab = np.full((3, 256), DEAD, dtype=np.uint16)
    tab[0, ord("a")] = 1
    tab[1, ord("b")] = 1
    tab[1, ord("c")] = 2
    return tab, np.array([0, 0, 1], dtype=np.uint8)


def _pool(tab, acc, entry=1, slots=4):
    tb, tl = ops.guide_token_table(PIECES, never={0, EOS3})
    gt = torch.full((3, ops.GUIDE_STATES, 256), -1, dtype=torch.int16)
    gf = torch.zeros(3, ops.GUIDE_STATES, dtype=torch.int32)
    gt[entry, :tab.shape[0]] = torch.from_numpy(tab.view(np.int16))
    gf[entry, :tab.shape[0]] = torch.from_numpy(acc.astype(np.int32))
    meta = torch.zeros(2 * slots, dtype=torch.int32)
    meta[:slots] = -1
    return tb, tl, gt, gf, meta


def test_token_table_marks_what_no_guide_allows():
    tb, tl = ops.guide_token_table(PIECES + ["y" * 32, "y" * 33], never={0, EOS3})
    assert tl.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 3, 1, 0, 4, 2, 2, 32, 0]
    assert bytes(tb[13, :2].tolist()) == "é".encode() and bytes(tb[8, :3].tolist()) == b"abc"


def test_reference_ops_on_a_hand_built_table():
    tab, acc = _hand_table()
    tb, tl, gt, gf, meta = _pool(tab, acc)
    ops.guide_live(tb, tl, gt, gf, meta, 1, 3, EOS3)
    assert gf[1, :3].tolist() == [0, 0, 1 | 2]  # only the accepting end state is stuck
    # rows -> slots 3, 2, 1, 0: slot 3 at state 0, slot 2 guide off, slot 1 at state 1 (inactive row), slot 0 dead
    meta[3], meta[4 + 3] = 1, 0
    meta[1], meta[4 + 1] = 1, 1
    meta[0], meta[4 + 0] = 1, DEAD
    row_slot = torch.tensor([3, 2, 1, 0], dtype=torch.int32)
    active = torch.tensor([1, 1, 0, 1], dtype=torch.int32)
    x0 = torch.randn(4, len(PIECES))
    x = x0.clone()
    ops.guide_mask(x, active, tb, tl, gt, gf, meta, row_slot, 0, EOS3)
    assert torch.equal(x[1:], x0[1:])
    allowed = {3, 6, 8}  # from state 0: "a", "ab", "abc"
    for v in range(len(PIECES)):
        assert (x[0, v] == x0[0, v]) if v in allowed else (x[0, v] == NEG), v
    active[2] = 1
    x = x0.clone()
    ops.guide_mask(x, active, tb, tl, gt, gf, meta, row_slot, 0, EOS3)
    assert [v for v in range(len(PIECES)) if x[2, v] != NEG] == [4, 5, 7, 11]  # from state 1: b, c, bc, bbbc
    meta[4 + 1] = 2  # accepting and stuck: EOS only, written 0.0 whatever it held (a min_tokens ban's -inf)
    x = x0.clone()
    x[2, EOS3] = NEG
    ops.guide_mask(x, active, tb, tl, gt, gf, meta, row_slot, 0, EOS3)
    assert x[2, EOS3] == 0.0 and (x[2, :EOS3] == NEG).all() and (x[2, EOS3 + 1:] == NEG).all()
    # a vocabulary shard that does not own EOS: columns 4.. as local 0..
    x = x0[:, 4:].clone()
    ops.guide_mask(x, active, tb, tl, gt, gf, meta, row_slot, 4, EOS3)
    assert (x[2] == NEG).all() and [v + 4 for v in range(x.shape[1]) if x[0, v] != NEG] == [6, 8]
    # advance: "ab" from 0 -> 1; EOS leaves a state; "x" kills; a piece of length 0 kills; off / inactive rows skipped
    meta[4 + 1] = 1
    ids = torch.tensor([6, 3, EOS3, 3], dtype=torch.int32)
    active[3] = 0
    ops.guide_advance(ids, active, tb, tl, gt, gf, meta, row_slot, EOS3)
    assert meta[4:].tolist() == [DEAD, 1, 0, 1] and meta[:4].tolist() == [1, 1, -1, 1]
    ops.guide_advance(torch.tensor([9, 0, 10, 0], dtype=torch.int32), None, tb, tl, gt, gf, meta, row_slot, EOS3)
    assert meta[4:].tolist() == [DEAD, DEAD, 0, DEAD]
    assert ops.guide_walk(tab, 0, [3, 4, EOS3, 7], tb, tl, EOS3) == 2 and ops.guide_walk(tab, 0, [4], tb, tl) == DEAD
    assert ops.guide_walk(tab, 0, [10], tb, tl) == DEAD and ops.guide_walk(tab, 0, [], tb, tl) == 0


# ------------------------------------------------------------------------------------------------ CPU engine
_W = {}
TOK = SyntheticTokenizer(TINY.vocab_size)
EOS = TOK.eos_id


def _engine(num_blocks=256, max_batch=4):
    if "w" not in _W:
        _W["w"] = convert_standard(TINY, init_standard_weights(TINY, seed=11))
    r = ModelRunner(_W["w"], num_blocks=num_blocks, max_batch=max_batch, max_model_len=512, device="cpu",
                    use_graphs=False)
    r.set_guide_vocab(TOK.pieces(), EOS)
    return LLMEngine(r, eos_id=EOS, prefill_budget=256)


def _prompt(i, n):
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randint(3, TINY.vocab_size, (n,), generator=g).tolist()


def _run(e, reqs, max_steps=4000, watch=None):
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
        if watch is not None:
            watch(step, fin)
        if step > max(at for *_, at in reqs) and not e.has_work():
            break
    assert not e.has_work(), "engine did not drain"
    return out, fin


def _text(ids):
    return "".join(TOK.piece(t) for t in ids)


def _is_prefix(pattern, text):
    tab, _ = compile_(pattern)
    s = 0
    for b in text.encode():
        s = int(tab[s, b])
        if s == DEAD:
            return False
    return True


PHONE = "[0-9]{3}-[0-9]{4}"
LABELS = [TOK.piece(40) + TOK.piece(44), "12", "7-3", TOK.piece(48) + TOK.piece(49)]


def test_guided_streams_deliver_matches_and_prefixes():
    choice = rtmod.load().guide_choice_pattern(LABELS)
    reqs = [("phone", _prompt(0, 20), SamplingParams(temperature=0.0, max_tokens=20, guide=PHONE), 0),
            ("label", _prompt(1, 33), SamplingParams(temperature=1.0, seed=7, max_tokens=20, guide=choice), 0),
            ("label2", _prompt(2, 9), SamplingParams(temperature=0.0, max_tokens=20, guide=choice), 1),
            ("cut", _prompt(3, 12), SamplingParams(temperature=1.0, seed=3, max_tokens=3, guide=PHONE), 2)]
    e = _engine()
    out, fin = _run(e, reqs)
    assert e.r.guide_used and e.r._twin_key() == (False, False, False, True)
    assert fin["phone"] == "stop" and re.fullmatch(PHONE, _text(out["phone"])), _text(out["phone"])
    for c in ("label", "label2"):
        assert fin[c] == "stop" and _text(out[c]) in LABELS, _text(out[c])
    assert fin["cut"] == "length" and len(out["cut"]) == 3
    assert _is_prefix(PHONE, _text(out["cut"])) and not re.fullmatch(PHONE, _text(out["cut"]))
    assert all(EOS not in v for v in out.values()) and sum(e._guide_refs) == 0


def test_a_stuck_pattern_ends_with_stop():
    """'#' is in no piece: after "1" nothing but EOS survives, and from the start state of '#' nothing at all."""
    e = _engine()
    out, fin = _run(e, [("a", _prompt(0, 20), SamplingParams(temperature=0.0, max_tokens=30, guide="1#2"), 0),
                        ("b", _prompt(1, 20), SamplingParams(temperature=1.0, seed=1, max_tokens=30, guide="#+"), 0),
                        # min_tokens bans EOS, the stuck state overrides it: no row is ever all -inf
                        ("c", _prompt(2, 20), SamplingParams(temperature=0.0, max_tokens=30, min_tokens=5,
                                                            guide="1#2"), 0)])
    assert fin == {"a": "stop", "b": "stop", "c": "stop"}
    assert _text(out["a"]) == "1" and out["b"] == [] and _text(out["c"]) == "1"


LONG = "(?:[0-9a-z]| |-){200}"


def test_preempted_guided_streams_resume_token_exact():
    reqs = [(f"c{i}", _prompt(i, 20 + 7 * i), SamplingParams(temperature=1.0, seed=40 + i, max_tokens=50 + 5 * i,
                                                             guide=LONG), i // 2) for i in range(5)]
    want, fin = _run(_engine(num_blocks=256), reqs)
    e = _engine(num_blocks=10)
    got, _ = _run(e, reqs)
    assert e.stats["preemptions"] > 0 and got == want
    for c, v in want.items():  # cut by max_tokens: a prefix of a match; 200 bytes reached: the match itself
        assert (fin[c] == "length" and _is_prefix(LONG, _text(v))) or (fin[c] == "stop" and re.fullmatch(LONG, _text(v)))
    plain, _ = _run(_engine(), [(c, p, SamplingParams(temperature=1.0, seed=sp.seed, max_tokens=sp.max_tokens), at)
                                for c, p, sp, at in reqs])
    assert plain != want


def test_unguided_streams_in_the_batch_are_unchanged():
    """Against the same batch with no guided request (the neighbours' fields dropped): a row's numerics depend on the
    batch it shares, so that is the run to compare with."""
    free = [("u0", _prompt(5, 17), SamplingParams(temperature=0.0, max_tokens=24, ignore_eos=True), 0),
            ("u1", _prompt(6, 40), SamplingParams(temperature=0.9, seed=5, top_k=50, max_tokens=24, ignore_eos=True), 1)]

    def others(guided):
        return [("g0", _prompt(7, 11), SamplingParams(temperature=0.0, max_tokens=24, guide=PHONE if guided else None), 0),
                ("g1", _prompt(8, 30), SamplingParams(temperature=1.0, seed=2, max_tokens=24,
                                                      guide=LONG if guided else None), 2)]

    e = _engine()
    plain, _ = _run(e, free + others(False))
    assert not e.r.guide_used and e.r.guide_tab is None  # nothing is allocated before the first guided request
    mixed, _ = _run(_engine(), free + others(True))
    assert {c: mixed[c] for c, *_ in free} == {c: plain[c] for c, *_ in free}
    assert re.fullmatch(PHONE, _text(mixed["g0"])) and mixed["g0"] != plain["g0"]


def test_a_pattern_waits_for_a_pool_entry():
    n = ops.GUIDE_POOL + 1
    reqs = [(f"p{i}", _prompt(i, 5), SamplingParams(temperature=0.0, max_tokens=12, guide=f"{i:02d}[0-9]{{{2 + i % 3}}}"), 0)
            for i in range(n)]
    e = _engine(num_blocks=256, max_batch=n + 3)
    seen = {}

    def watch(step, fin):
        live = [s for s in e.slots if s is not None]
        assert len(live) <= ops.GUIDE_POOL and all(r >= 0 for r in e._guide_refs)
        if step == 0:
            seen["waiting"] = [s.conversation_id for s in e.waiting]
            assert len(live) == ops.GUIDE_POOL and sum(e._guide_refs) == ops.GUIDE_POOL
        if f"p{n - 1}" in [s.conversation_id for s in live] and "admitted_after" not in seen:
            seen["admitted_after"] = len(fin)

    out, fin = _run(e, reqs, watch=watch)
    assert seen["waiting"] == [f"p{n - 1}"] and seen["admitted_after"] >= 1  # served once an entry was freed
    for i, (c, _, sp, _) in enumerate(reqs):
        assert fin[c] == "stop" and re.fullmatch(sp.guide, _text(out[c])), (c, _text(out[c]))
    assert sum(e._guide_refs) == 0


def test_bad_pattern_is_refused_at_add_request():
    e = _engine()
    with pytest.raises(ValueError, match="anchor"):
        e.add_request("x", _prompt(0, 5), SamplingParams(guide="^a"))
    assert not e.has_work()


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
    _post(rt, route, {"guided_regex": PHONE})
    (q,) = rt.poll_requests(10, 1000)
    assert q["guide"] == PHONE
    _post(rt, route, {"guided_choice": ["a.b", "yes", "(no)"], "guided_regex": None, "ignore_eos": False})
    (q,) = rt.poll_requests(10, 1000)
    assert q["guide"] == r"a\.b|yes|\(no\)"
    _post(rt, route, {"guided_choice": None, "guided_regex": None})
    (q,) = rt.poll_requests(10, 1000)
    assert q["guide"] == ""


BAD = [({"guided_regex": "a", "guided_choice": ["a"]}, "guided_regex and guided_choice", ""),
       ({"guided_regex": "a", "ignore_eos": True}, "guided_regex", "ignore_eos"),
       ({"guided_choice": ["a"], "ignore_eos": True}, "guided_choice", "ignore_eos"),
       ({"guided_regex": 5}, "guided_regex must", ""), ({"guided_regex": ["a"]}, "guided_regex must", ""),
       ({"guided_regex": "a" * 2049}, "guided_regex must", "2048"),
       ({"guided_choice": "a"}, "guided_choice must", ""), ({"guided_choice": []}, "guided_choice must", ""),
       ({"guided_choice": ["a", 1]}, "guided_choice must", ""), ({"guided_choice": ["a", ""]}, "guided_choice must", ""),
       ({"guided_choice": ["a", "a"]}, "guided_choice must", "distinct"),
       ({"guided_choice": ["a" * 65]}, "guided_choice must", "64"),
       ({"guided_choice": [str(i) for i in range(65)]}, "guided_choice must", "64"),
       ({"guided_regex": "^a$"}, "guided_regex: guide pattern: anchor ^", "offset 0"),
       ({"guided_regex": "a*?"}, "guided_regex: guide pattern: lazy quantifier", "offset 2"),
       ({"guided_regex": "a{255}a{255}aa"}, "guided_regex: guide pattern: needs more than 512 DFA states", ""),
       ({"guided_choice": [chr(97 + i) * 60 for i in range(10)]},  # a 600-state trie
        "guided_choice: guide pattern: needs more than 512 DFA states", "")]


@pytest.mark.parametrize("extra, field, also", BAD)
def test_bad_fields_are_a_400_that_names_the_field(rt, extra, field, also):
    for role in ("edge", "origin"):
        r = _post(rt, "/chat", extra, role)
        assert r.status == 400 and r.body.decode().startswith(field) and also in r.body.decode(), r.body
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


def test_guides_take_effect_over_http(cpu_app):
    msgs = [{"role": "user", "content": "Pick one."}]
    for stream in (False, True):
        r = request(H, cpu_app.port("origin"), "POST", "/v1/chat/completions",
                    {"messages": msgs, "stream": stream, "max_tokens": 20, "guided_choice": LABELS}, timeout=60,
                    stop_on_done=False)
        if stream:
            chunks = [json.loads(e.data)["choices"][0] for e in r.events if e.data != "[DONE]"]
            text, fin = "".join(c["delta"]["content"] for c in chunks[1:-1]), chunks[-1]["finish_reason"]
        else:
            d = json.loads(r.body)["choices"][0]
            text, fin = d["message"]["content"], d["finish_reason"]
        assert text in LABELS and fin == "stop"
    c = request(H, cpu_app.port("edge"), "POST", "/chat", {"message": "A number?", "max_tokens": 20,
                                                           "temperature": 1.0, "seed": 4, "guided_regex": PHONE}, timeout=60)
    toks = [e.json() for e in c.events if e.event == "token"]
    assert re.fullmatch(PHONE, "".join(t["token"] for t in toks[:-1])) and toks[-1]["done"]


def test_the_stub_engine_validates_and_ignores_the_guide():
    c = ServeConfig(host=H, sse_port=0, origin_port=0, metrics_port=0, resp_port=0, io_threads=2)
    c.engine, c.stub_tokens, c.stub_token_delay_ms = "stub", 5, 0
    app = ServingApp(c).start()
    try:
        r = request(H, app.port("edge"), "POST", "/chat", {"message": "hi", "guided_regex": "(?=a)"}, timeout=30)
        assert r.status == 400 and r.body.decode().startswith("guided_regex: guide pattern: look-around")
        r = request(H, app.port("edge"), "POST", "/chat", {"message": "hi", "guided_regex": PHONE}, timeout=30)
        toks = [e.json() for e in r.events if e.event == "token"]
        assert r.status == 200 and len(toks) >= 2 and toks[-1]["done"]
    finally:
        app.stop()


# ------------------------------------------------------------------------------------------------ DP ring, TP plan
def test_dp_ring_delivers_the_guide():
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
                chan.publish_tokens([c, c], [10, -1], [1, 2], [False, True], 0, ["", "[DONE]"])

    t = threading.Thread(target=worker, daemon=True)
    t.start()
    try:
        deadline = time.time() + 10
        while time.time() < deadline and not all(i["ready"] for i in r.dp_workers()):
            time.sleep(0.02)
        long = "(?:é|[a-z]{1,200}|" + "|".join(["x"] * 900) + ")+"  # (long as carried, small as a DFA)
        a = request(H, r.bound_port("edge"), "POST", "/chat", {"message": "hi", "conversation_id": "p1",
                                                               "guided_regex": long}, timeout=30)
        b = request(H, r.bound_port("edge"), "POST", "/chat", {"message": "hi", "conversation_id": "p2"}, timeout=30)
        c = request(H, r.bound_port("edge"), "POST", "/chat", {"message": "hi", "conversation_id": "p3",
                                                               "guided_choice": ["a|b", "c"]}, timeout=30)
        assert a.status == 200 and b.status == 200 and c.status == 200
        by = {q["conversation_id"]: q["guide"] for q in seen}
        assert by == {"p1": long, "p2": "", "p3": r"a\|b|c"}
    finally:
        stop.set()
        t.join(5)
        r.stop()


def test_plan_carries_the_guide_bit_exactly():
    for guide in (PHONE, "é|日本+", "a", "abcd", "x" * 8191, ""):
        sp = SamplingParams(temperature=0.7, max_tokens=9, logit_bias={5: 0.5}, stop_token_ids=(7, 8), guide=guide)
        plan = tpmod.Plan(step=True, adds=[(7, [1, 2, 3], sp, 123456789), (8, [4], SamplingParams(), 5)], aborts=[3])
        once = plan.roundtrip()
        assert once.adds[0][2].guide == guide and once.adds[1][2].guide is None
        assert once.adds[0][2].logit_bias == {5: 0.5} and once.adds[0][2].stop_token_ids == (7, 8)
        assert once.adds[0][1] == [1, 2, 3] and once.adds[1][1] == [4] and once.aborts == [3]
        assert once.roundtrip().encode() == once.encode()


# ------------------------------------------------------------------------------------------------ TP over gloo
TP_PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 150)), [11] * 20]
TP_TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]
TP_GUIDES = [(1, PHONE), (2, "(?:[a-z]| )+")]  # (slot, pattern): digits and EOS live in shard 0, most words in shard 1


def _tp_generate(rank, world, use=True, steps=10):
    std = init_standard_weights(TINY, seed=3)
    comm = TPComm(rank=rank, size=world, group=None) if world > 1 else TPComm()
    w = convert_standard(TINY, std, tp_rank=rank, tp_size=world)
    r = ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device="cpu", comm=comm, use_graphs=False)
    r.set_guide_vocab(TOK.pieces(), EOS)
    for i, bt in enumerate(TP_TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
    if use:
        for e, (slot, pattern) in enumerate(TP_GUIDES):
            r.upload_guide(e, *compile_(pattern))
            r.set_guide(slot, e, 0)
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
def test_tp2_guided_matches_tp1():
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_tp_worker, args=(2, _port(), out), nprocs=2, join=True)
        res = [out[r] for r in range(2)]
    assert res[0] == res[1], "TP ranks disagree on the sampled tokens"
    one = _tp_generate(0, 1)
    assert res[0] == one
    phone = _text(one[1][:one[1].index(EOS)] if EOS in one[1] else one[1])
    assert re.fullmatch(PHONE, phone) and re.fullmatch(TP_GUIDES[1][1], _text([t for t in one[2] if t != EOS]))
    plain = _tp_generate(0, 1, use=False)
    assert plain[0] == one[0] and plain[1:] != one[1:]
