"""JSON mode (response_format json_object) on the CPU: the byte walker against json.loads, the mask / advance twins
against a per-token scalar walk on a crafted vocabulary, the engine end to end on a tiny model whose pieces can spell
JSON (deterministic, sampled, mixed batch, preemption, a vocabulary without braces), and TP = 2 over gloo."""
import json
import os
import random
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.models.tokenizer import SyntheticTokenizer
from distributed_sse_for_llm_response_amd.parallel.comm import TPComm
from distributed_sse_for_llm_response_amd.serving import tp as tpmod

import json_mode_common as jc
from json_mode_common import DEAD, EOS, NEG, VG, is_done, is_viable, oracle

DONE = ops.JSON_DONE


# ------------------------------------------------------------------------------------------------ 1. the walker
def _value(rng, depth):
    kind = rng.randrange(10 if depth > 0 else 6)
    if kind == 0:
        return rng.choice([0, -1, 7, 10 ** 12, -(2 ** 40), 123456789])
    if kind == 1:
        return rng.choice([0.5, -2.25, 1e-7, 3.5e+20, -0.0, 6.02e23, 1e300])
    if kind == 2:
        return rng.choice([True, False, None])
    if kind == 3:
        return _string(rng)
    if kind == 4:
        return rng.choice([{}, [], "", [[]], [{}]])
    if kind == 5:
        return rng.randrange(-1000, 1000)
    if kind < 8:
        return {_string(rng): _value(rng, depth - 1) for _ in range(rng.randrange(4))}
    return [_value(rng, depth - 1) for _ in range(rng.randrange(4))]


def _string(rng):
    alphabet = ["a", "Z", " ", "é", "日", "😀", "\\", '"', "/", "\n", "\t", "\x01", "\x1f", "\x7f", " ", "ß", "0", "{", "]"]
    return "".join(rng.choice(alphabet) for _ in range(rng.randrange(6)))


@pytest.fixture(scope="module")
def documents():
    rng = random.Random(20240)
    docs = []
    for i in range(300):
        top = {_string(rng): _value(rng, rng.randrange(1, 6)) for _ in range(rng.randrange(4))}
        indent = rng.choice([None, None, 0, 1, 2, "\t"])
        seps = rng.choice([None, (",", ":"), (", ", ": "), (" ,\n", " :\r ")])
        docs.append(json.dumps(top, indent=indent, separators=seps, ensure_ascii=bool(i % 2)).encode("utf-8"))
    assert max(len(d) for d in docs) > 200 and any(b"\\u" in d for d in docs) and any(max(d) >= 0x80 for d in docs)
    return docs


def test_walker_accepts_documents_and_keeps_every_prefix_alive(documents):
    for d in documents:
        assert oracle(d)
        s = ops.JSON_START_STATE
        for i, byte in enumerate(d):
            assert s[0] not in (DEAD, DONE), (d, i)  # every proper prefix: live and not DONE
            s = ops.json_walk(bytes([byte]), s)
        assert s == (DONE, 0, 0), d


def test_walker_agrees_with_the_oracle_on_one_byte_mutations(documents):
    rng = random.Random(99)
    pool = list(b'{}[]",:0123456789.-+eE \n\tnulltrufasx\\') + [0x00, 0x1f, 0x7f, 0x80, 0xbf, 0xc0, 0xc3, 0xe0, 0xed, 0xf4,
                                                               0xf5, 0xff]
    n = accepted = 0
    for d in documents:
        for _ in range(10):
            i, op = rng.randrange(len(d)), rng.randrange(3)
            b = bytes([rng.choice(pool)])
            m = d[:i] + d[i + 1:] if op == 0 else d[:i] + b + d[i:] if op == 1 else d[:i] + b + d[i + 1:]
            want = oracle(m)
            assert is_done(m) == want, (m, want)
            n, accepted = n + 1, accepted + want
    assert n == 3000 and 100 < accepted < 2900  # (both answers are exercised)


# (prefix, next byte, dead?)
TABLE = [
    (b'{"a":0', b"1", True), (b'{"a":0', b"0", True), (b'{"a":-0', b"5", True), (b'{"a":0', b".", False),
    (b'{"a":-', b"}", True), (b'{"a":-', b" ", True), (b'{"a":-', b"-", True), (b'{"a":-', b"7", False),
    (b'{"a":1.', b"}", True), (b'{"a":1.', b"e", True), (b'{"a":1.', b"0", False),
    (b'{"a":1e', b"}", True), (b'{"a":1e', b",", True), (b'{"a":1e', b"+", False), (b'{"a":1e+', b"}", True),
    (b'{"a":1e+', b"3", False), (b'{"a":1E5', b"}", False), (b'{"a":1.5', b".", True), (b'{"a":1', b"a", True),
    (b'{"a":"\\u12', b"g", True), (b'{"a":"\\u12', b'"', True), (b'{"a":"\\u12', b"F", False), (b'{"a":"\\', b"x", True),
    (b'{"a":"\\', b"/", False), (b'{"a":"', b"\x1f", True), (b'{"a":"', b"\n", True), (b'{"a":"', b"\x7f", False),
    (b'{"a":"', b"\xc0", True), (b'{"a":"', b"\xc1", True), (b'{"a":"\xe0', b"\x80", True),  # (C0 80: dead at C0)
    (b'{"a":"\xe0\xa0', b"\x80", False), (b'{"a":"\xed', b"\xa0", True), (b'{"a":"\xed\x9f', b"\xbf", False),
    (b'{"a":"\xf4', b"\x90", True), (b'{"a":"\xf4\x8f\xbf', b"\xbf", False), (b'{"a":"\xf0', b"\x8f", True),
    (b'{"a":"', b"\xf5", True), (b'{"a":"', b"\x80", True), (b'{"a":"\xc3', b'"', True),
    (b'{"a":1,', b"}", True), (b'{"a":[', b",", True), (b'{"a":[1,', b"]", True), (b'{"a" ', b"1", True),
    (b'{"a" ', b":", False), (b"{", b",", True), (b"{", b"1", True), (b'{"a":[1', b"}", True), (b'{"a":{', b"]", True),
    (b'{"a":1', b"]", True), (b'{"a":tru', b"}", True), (b'{"a":', b"N", True), (b'{"a":', b"I", True),
    (b'{"a":', b"T", True), (b'{"a":nul', b"l", False),
    (jc.DEEP, b"{", True), (jc.DEEP, b"[", True), (jc.DEEP, b"1", False), (b'{"a":' * 63, b"[", False),
    (b"", b"[", True), (b"", b"1", True), (b"", b'"', True), (b"", b" ", True), (b"", b"{", False),
    (b"{}", b" ", True), (b"{}", b"\n", True), (b"{}", b"}", True), (b'{"a":{}}', b"}", True),
]


@pytest.mark.parametrize("prefix, byte, dead", TABLE)
def test_walker_hand_table(prefix, byte, dead):
    s = ops.json_walk(prefix)
    assert s[0] != DEAD, prefix
    assert (ops.json_walk(byte, s)[0] == DEAD) == dead
    assert ops.json_walk(byte, ops.JSON_DEAD_STATE)[0] == DEAD  # dead stays dead


def test_depth_and_stack_words():
    q, depth, stack = ops.json_walk(jc.DEEP)
    assert depth == 64 and stack == 0 and is_done(jc.DEEP + b"1" + b"}" * 64)
    deep_arr = b'{"a":' + b"[" * 63
    q, depth, stack = ops.json_walk(deep_arr)
    assert depth == 64 and stack == (1 << 63) - 1 and is_done(deep_arr + b"]" * 63 + b"}")
    assert ops.json_state_words((q, depth, stack)) == [q, 64, -1, 0x7FFFFFFF]
    assert not is_viable(deep_arr + b"[") and not is_viable(b'{"a":[}') and is_viable(b'{"a":[{"b":[')


# ------------------------------------------------------------------------------------------------ 2. mask / advance
@pytest.fixture(scope="module")
def vocab():
    return jc.vocabulary()


def _scalar_kept(state, tb, tl):
    """The per-token scalar walk: ids that survive from `state` (EOS aside)."""
    keep = []
    for g in range(tl.shape[0]):
        n = int(tl[g])
        if g != EOS and 1 <= n <= 32 and ops.json_walk(bytes(tb[g, :n].tolist()), state)[0] != DEAD:
            keep.append(g)
    return keep


def _pool():
    gt = torch.full((1, ops.GUIDE_STATES, 256), -1, dtype=torch.int16)
    gf = torch.zeros(1, ops.GUIDE_STATES, dtype=torch.int32)
    return gt, gf


@pytest.mark.parametrize("name", list(jc.PREFIXES) + ["dead"])
def test_mask_twin_keeps_what_the_scalar_walk_keeps(vocab, name):
    tb, tl = vocab
    state = jc.states()[name]
    gt, gf = _pool()
    meta = torch.tensor([-1, ops.JSON_ENTRY, -1, 0, 0, 0], dtype=torch.int32)
    js = jc.json_state_tensor(3, {1: state})
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, VG, generator=g)
    x0[:, EOS] = NEG  # banned, as by min_tokens
    x = x0.clone()
    ops.guide_attach_json(meta, jc.json_tab_tensor(), js)
    ops.guide_mask(x, None, tb, tl, gt, gf, meta, torch.tensor([0, 1], dtype=torch.int32), 0, EOS)
    assert torch.equal(x[0], x0[0])
    if name == "dead":
        assert torch.equal(x[1], x0[1])
        return
    keep = _scalar_kept(state, tb.numpy(), tl.numpy())
    got = [v for v in range(VG) if x[1, v] != NEG and v != EOS]
    assert got == keep
    assert torch.equal(x[1, keep], x0[1, keep])
    assert x[1, EOS] == (NEG if keep else 0.0)
    assert bool(keep) == (name != "done") and jc.LEN0 not in keep and jc.LEN33 not in keep
    frag = {f: jc.token_id(tb, tl, f) for f in (b"}}", b"]}", b"{", b"[", b" " * 32)}
    if name == "after a value, stack obj obj":
        assert frag[b"}}"] in keep and frag[b"]}"] not in keep
    if name == "after a value, stack obj arr":
        assert frag[b"]}"] in keep and frag[b"}}"] not in keep
    if name == "depth 64":
        assert frag[b"{"] not in keep and frag[b"["] not in keep and jc.token_id(tb, tl, b'"') in keep
    if name == "depth 1 before the closing brace":
        assert frag[b" " * 32] in keep and frag[b"}}"] not in keep and jc.token_id(tb, tl, b"}") in keep
    if name == "nul":
        assert keep == [jc.BYTE0 + ord("l")]
    if name == "dot":
        assert keep and max(keep) < 1000


def test_mask_twin_on_a_shard_decides_stuck_over_the_global_vocabulary(vocab):
    tb, tl = vocab
    st = jc.states()
    gt, gf = _pool()
    meta = torch.tensor([ops.JSON_ENTRY, ops.JSON_ENTRY, 0, 0], dtype=torch.int32)
    js = jc.json_state_tensor(2, {0: st["nul"], 1: st["done"]})
    x = torch.zeros(2, 1000)
    ops.guide_mask(x, None, tb, tl, gt, gf, ops.guide_attach_json(meta, jc.json_tab_tensor(), js), None, 0, EOS)
    assert (x[0] == NEG).all()                     # the survivor lives in the other shard: not stuck, EOS stays banned
    assert x[1, EOS] == 0.0 and (x[1] == NEG).sum() == 999
    js = jc.json_state_tensor(2, {0: st["dot"], 1: st["nul"]})
    x = torch.zeros(2, 1000)
    ops.guide_mask(x, None, tb, tl, gt, gf, ops.guide_attach_json(meta, jc.json_tab_tensor(), js), None, 1000, EOS)
    assert (x[0] == NEG).all() and [v for v in range(1000) if x[1, v] != NEG] == [jc.BYTE0 + ord("l") - 1000]


def test_advance_twin_moves_the_state_words(vocab):
    tb, tl = vocab
    st = jc.states()
    gt, gf = _pool()
    tid = lambda raw: jc.token_id(tb, tl, raw)  # noqa: E731
    # slot: state, committed token, the text the state then stands for (None: dead)
    cases = [(st["start"], tid(b'{"a":{"b":['), b'{"a":{"b":['), (st["number in an array"], tid(b","), b'{"k":[12,'),
             (st["number in an object"], tid(b","), b'{"k":12,'), (st["after a value, stack obj obj"], tid(b"}}"), b"{}"),
             (st["after a value, stack obj arr"], tid(b"}}"), None), (st["after a value, stack obj arr"], tid(b"]}"), b"{}"),
             (st["depth 64"], tid(b"{"), None), (st["done"], EOS, b"{}"), (st["done"], tid(b" "), None),
             (st["key string"], jc.LEN0, None), (st["key string"], jc.LEN33, None), (st["dead"], tid(b"{"), None),
             (st["mid a 3-byte character"], tid("日".encode()[2:]), b'{"k":"\xe6\x97\xa5'),
             (st["start"], EOS, b"")]
    n = len(cases)
    meta = torch.tensor([ops.JSON_ENTRY] * n + [7] * n, dtype=torch.int32)
    js = jc.json_state_tensor(n, {i: c[0] for i, c in enumerate(cases)})
    before = js.clone()
    perm = list(reversed(range(n)))
    ids = torch.tensor([cases[s][1] for s in perm], dtype=torch.int32)
    active = torch.ones(n, dtype=torch.int32)
    active[0] = 0  # the row of the last slot: skipped
    ops.guide_attach_json(meta, jc.json_tab_tensor(), js)
    ops.guide_advance(ids, active, tb, tl, gt, gf, meta, torch.tensor(perm, dtype=torch.int32), EOS)
    assert meta.tolist() == [ops.JSON_ENTRY] * n + [7] * n  # guide_meta is not JSON mode's to write
    for i, (_, _, text) in enumerate(cases[:-1]):
        got = js.view(4, -1)[:, i].tolist()
        if text is None:
            assert got[0] == DEAD and got[1:] == before.view(4, -1)[1:, i].tolist(), i
        else:
            assert got == ops.json_state_words(ops.json_walk(text)), i
    assert torch.equal(js.view(4, -1)[:, n - 1], before.view(4, -1)[:, n - 1])
    assert ops.json_walk_ids(ops.JSON_START_STATE, [tid(b'{"'), tid(b"a"), EOS, tid(b'":'), tid(b"true"), tid(b"}")],
                             tb, tl, EOS) == (DONE, 0, 0)
    assert ops.json_walk_ids(ops.JSON_START_STATE, [tid(b'{"'), jc.LEN0], tb, tl, EOS) == ops.JSON_DEAD_STATE
    assert ops.json_walk_ids(ops.JSON_START_STATE, [VG], tb, tl, EOS) == ops.JSON_DEAD_STATE


# ------------------------------------------------------------------------------------------------ 3. the engine
_W = {}
PIECES = jc.json_pieces(TINY.vocab_size)
PID = lambda text: jc.piece_id(PIECES, text)  # noqa: E731


def _engine(num_blocks=256, max_batch=4, pieces=PIECES):
    if "w" not in _W:
        _W["w"] = convert_standard(TINY, init_standard_weights(TINY, seed=11))
    r = ModelRunner(_W["w"], num_blocks=num_blocks, max_batch=max_batch, max_model_len=512, device="cpu",
                    use_graphs=False)
    r.set_guide_vocab(pieces, EOS)
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


def _text(ids, pieces=PIECES):
    return "".join(pieces[t] for t in ids).encode("utf-8")


def test_json_object_excludes_a_guide():
    e = _engine()
    with pytest.raises(ValueError, match="json_object"):
        e.add_request("x", _prompt(0, 5), SamplingParams(json_object=True, guide="a"))
    assert not e.has_work() and not SamplingParams().json_object


def test_deterministic_empty_object():
    e = _engine()
    sp = SamplingParams(temperature=0.0, max_tokens=20, json_object=True, logit_bias={PID("}"): 100.0})
    out, fin = _run(e, [("a", _prompt(0, 20), sp, 0)])
    assert _text(out["a"]) == b"{}" and len(out["a"]) == 2 and fin["a"] == "stop"
    assert e.r.guide_used and e.r._twin_key()[3] and e.r.json_state is not None and sum(e._guide_refs) == 0


BIAS = 12.0  # on one id each of " } ] , and : (the condition below is met with it on the CPU twin engine)


def test_sampled_streams_are_objects_or_viable_prefixes():
    bias = {PID(p): BIAS for p in ('"', "}", "]", ",", ":")}
    reqs = [(f"s{i}", _prompt(i, 8 + i), SamplingParams(temperature=1.0, seed=100 + i, max_tokens=64, json_object=True,
                                                        logit_bias=bias), i // 4) for i in range(16)]
    out, fin = _run(_engine(max_batch=8), reqs)
    stops = 0
    for c, ids in out.items():
        text = _text(ids)
        print(c, fin[c], text)
        assert EOS not in ids
        if fin[c] == "stop":
            stops += 1
            assert oracle(text), text
        else:
            assert fin[c] == "length" and len(ids) == 64 and is_viable(text) and not is_done(text), text
    assert stops >= 4, stops


def test_mixed_batch_leaves_the_neighbours_alone_and_takes_no_pool_entry():
    def reqs(js):
        return [("j", _prompt(7, 11), SamplingParams(temperature=1.0, seed=9, max_tokens=24, json_object=js), 0),
                ("g", _prompt(8, 30), SamplingParams(temperature=1.0, seed=2, max_tokens=24, guide="(?:[a-z0-9]| )+"), 0),
                ("u", _prompt(6, 40), SamplingParams(temperature=0.9, seed=5, top_k=50, max_tokens=24, ignore_eos=True), 1)]

    plain, _ = _run(_engine(), reqs(False))
    e = _engine()
    seen = []

    def watch(step, fin):
        live = [s for s in e.slots if s is not None]
        seen.append(sum(e._guide_refs))
        assert sum(e._guide_refs) == sum(1 for s in live if s.params.guide is not None)
        assert all(s.guide_entry == -1 for s in live if s.params.json_object)

    mixed, fin = _run(e, reqs(True), watch=watch)
    assert max(seen) == 1 and sum(e._guide_refs) == 0
    assert mixed["g"] == plain["g"] and mixed["u"] == plain["u"] and mixed["j"] != plain["j"]
    text = _text(mixed["j"])
    assert oracle(text) if fin["j"] == "stop" else is_viable(text), text


def test_preempted_json_streams_resume_token_exact():
    # an opening {" and long keys: every stream is mid-object, several levels deep, when the pool runs out.  The
    # biases also keep the winner of every draw clear of the runner-up: a re-prefill rounds the KV differently from
    # the decode steps it replaces, and a near-tie among the few tokens a mask leaves would then flip
    bias = {PID('{"'): 12.0, PID("a"): 10.0, PID("key"): 9.0, PID(":"): 10.0, PID(","): 10.0, PID('"'): 7.0}
    reqs = [(f"c{i}", _prompt(i, 20 + 7 * i), SamplingParams(temperature=1.0, seed=40 + i, max_tokens=50 + 5 * i,
                                                             json_object=True, logit_bias=bias), i // 2) for i in range(5)]
    want, fin = _run(_engine(num_blocks=256), reqs)
    e = _engine(num_blocks=8)
    got, fin2 = _run(e, reqs)
    assert e.stats["preemptions"] > 0 and got == want and fin2 == fin
    assert all(len(v) >= 50 for v in want.values())
    for c, v in want.items():
        assert oracle(_text(v)) if fin[c] == "stop" else is_viable(_text(v)), _text(v)


def test_a_vocabulary_without_braces_is_stuck_at_once():
    tok = SyntheticTokenizer(TINY.vocab_size)
    assert not any("{" in p for p in tok.pieces())
    e = _engine(pieces=tok.pieces())
    steps = []
    out, fin = _run(e, [("a", _prompt(0, 20), SamplingParams(temperature=1.0, seed=3, max_tokens=30, min_tokens=4,
                                                             json_object=True), 0)],
                    watch=lambda step, fin: steps.append(step))
    assert out["a"] == [] and fin["a"] == "stop" and len(steps) <= 3


def test_plan_carries_json_object():
    sp = SamplingParams(temperature=0.7, max_tokens=9, json_object=True)
    plan = tpmod.Plan(step=True, adds=[(7, [1, 2, 3], sp, 123456789), (8, [4], SamplingParams(ignore_eos=True), 5)])
    once = plan.roundtrip()
    assert once.adds[0][2].json_object and not once.adds[0][2].ignore_eos
    assert not once.adds[1][2].json_object and once.adds[1][2].ignore_eos
    assert once.roundtrip().encode() == once.encode()


# ------------------------------------------------------------------------------------------------ 4. TP over gloo
TP_PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 150)), [11] * 20]
TP_TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]


def _tp_generate(rank, world, use=True, steps=14):
    std = init_standard_weights(TINY, seed=3)
    comm = TPComm(rank=rank, size=world, group=None) if world > 1 else TPComm()
    w = convert_standard(TINY, std, tp_rank=rank, tp_size=world)
    r = ModelRunner(w, num_blocks=64, max_batch=4, max_model_len=512, device="cpu", comm=comm, use_graphs=False)
    r.set_guide_vocab(PIECES, EOS)
    for i, bt in enumerate(TP_TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
    if use:
        r.enable_guides()
        for slot in (1, 2):
            r.set_guide(slot, ops.JSON_ENTRY, ops.JSON_START_STATE)
    r.temperature[:3] = torch.tensor([1.0, 1.0, 0.0])
    r.seeds[:3, 0] = torch.tensor([11, 22, 33], dtype=torch.int32)
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
def test_tp2_json_matches_tp1():
    assert EOS < TINY.vocab_size // 2  # the second shard does not own EOS
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_tp_worker, args=(2, _port(), out), nprocs=2, join=True)
        res = [out[r] for r in range(2)]
    assert res[0] == res[1], "TP ranks disagree on the sampled tokens"
    one = _tp_generate(0, 1)
    assert res[0] == one
    for row in one[1:]:
        text = _text(row[:row.index(EOS)] if EOS in row else row)
        assert text.startswith(b"{") and (oracle(text) if EOS in row else is_viable(text)), text
    plain = _tp_generate(0, 1, use=False)
    assert plain[0] == one[0] and plain[1:] != one[1:]
