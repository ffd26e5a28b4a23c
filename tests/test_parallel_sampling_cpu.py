"""Parallel sampling (add_request n > 1) on the CPU engine: the allocator's fork, the scheduler's use of it (a sibling
admitted on its parent's pages with one token left to prefill, a copied partial last page), the fallbacks, and the
TP plan.  The oracle is the same engine serving independent n = 1 requests of seed + i: on the CPU the streams are
exactly equal."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
from distributed_sse_for_llm_response_amd.engine.kv_cache import PAGE, BlockAllocator
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as ref
from distributed_sse_for_llm_response_amd.parallel.comm import TPComm
from distributed_sse_for_llm_response_amd.serving.tp import Plan, TPLeader, apply_plan
from test_prefix_cache_cpu import _engine, _prompt, _spy_prefill

IDS = ["a", "a-c1", "a-c2"]


def _sp(seed=40, mt=10, temp=0.9):
    return SamplingParams(temperature=temp, top_p=0.95, max_tokens=mt, seed=seed)


def _drive(e, hooks=None, max_steps=600):
    """Step until idle; conv -> [(token, sequence, done, finish)]."""
    out = {}
    for step in range(max_steps):
        if hooks and step in hooks:
            hooks[step](e)
        for ev in e.step():
            out.setdefault(ev.conversation_id, []).append((ev.token_id, ev.sequence, ev.done, ev.finish))
        if not e.has_work():
            break
    assert not e.has_work(), "engine did not drain"
    return out


def _solo(blocks, cache, prompt, i, seed=40, mt=10, temp=0.9):
    e = _engine(blocks, cache)
    e.add_request("x", prompt, _sp(seed + i, mt, temp))
    return _drive(e)["x"]


def _clean(e, blocks):
    """Every reference is back: all pages free, no fork left, no count above zero."""
    assert e.alloc.num_free == blocks and not e.alloc.has_forks
    if e.alloc.prefix_cache:
        assert all(r == 0 for r in e.alloc._ref)


# ---------------------------------------------------------------------------------------------- allocator
@pytest.mark.parametrize("cache", [False, True])
def test_fork_shares_blocks_until_the_last_owner_frees_them(cache):
    al = BlockAllocator(8, prefix_cache=cache)
    a = al.allocate(3)
    assert not any(al.is_shared(b) for b in a)
    assert al.fork(a[:2]) == a[:2] and al.fork(a[:1]) == a[:1]
    assert [al.is_shared(b) for b in a] == [True, True, False] and al.num_free == 5
    al.free(a)  # the first owner: only the private page comes back
    assert al.num_free == 6 and al.is_shared(a[0]) and not al.is_shared(a[1])
    al.free(a[:2])
    assert al.num_free == 7 and not al.is_shared(a[0])
    al.free(a[:1])
    assert al.num_free == 8 and not al.has_forks
    assert sorted(al.allocate(8)) == list(range(8))


def test_reference_copy_moves_whole_pages_and_nothing_else():
    g = torch.Generator().manual_seed(0)
    k = torch.randn(2, 8, 1, 32, 128, generator=g).bfloat16()
    v = torch.randn(2, 8, 1, 128, 32, generator=g).bfloat16()
    k0, v0 = k.clone(), v.clone()
    ops.kv_pages_copy(k, v, [(3, 6), (3, 1), (0, 7)])
    for b in range(8):
        src = {6: 3, 1: 3, 7: 0}.get(b, b)
        assert torch.equal(k[:, b], k0[:, src]) and torch.equal(v[:, b], v0[:, src])
    for bad in ([(0, 8)], [(-1, 0)], [(0, 1), (2, 1)], [(0, 1), (1, 2)]):
        with pytest.raises(ValueError):
            ops.kv_pages_copy(k, v, bad)
    ref.kv_pages_copy(k, v, torch.zeros(0, 2, dtype=torch.int32))  # n = 0


# ---------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("cache", [False, True], ids=["plain", "prefix-cache"])
@pytest.mark.parametrize("length,copies", [(2 * PAGE + 5, 2), (2 * PAGE + 1, 0), (2 * PAGE, 2), (7, 2)])
def test_choices_equal_independent_requests_of_seed_plus_i(cache, length, copies):
    prompt = _prompt(300 + length, length)
    e = _engine(32, cache)
    seen = _spy_prefill(e)
    seqs = e.add_request("a", prompt, _sp(), n=3)
    assert [s.conversation_id for s in seqs] == IDS
    assert [s.rid for s in seqs] == list(range(seqs[0].rid, seqs[0].rid + 3))
    assert [s.params.seed for s in seqs] == [40, 41, 42]
    got = _drive(e)
    # one prompt pass; each sibling prefills its last prompt token alone, on forked pages
    assert sorted(seen) == sorted([("a", 0, length), ("a-c1", length - 1, 1), ("a-c2", length - 1, 1)])
    assert e.stats["fork_requests"] == 1 and e.stats["fork_shared_tokens"] == 2 * (length - 1)
    assert e.stats["fork_tail_copies"] == copies and e.shared_write_violations == 0
    for i, c in enumerate(IDS):
        assert got[c] == _solo(32, cache, prompt, i), c
    assert len({tuple(got[c]) for c in IDS}) == 3  # different seeds: different streams
    _clean(e, 32)


def test_greedy_siblings_are_identical_and_seedless_ones_differ():
    prompt = _prompt(1, 50)
    e = _engine(32, False)
    e.add_request("a", prompt, SamplingParams(temperature=0.0, max_tokens=8), n=3)
    got = _drive(e)
    assert got["a"] == got["a-c1"] == got["a-c2"] and len(got["a"]) == 9
    e.add_request("a", prompt, SamplingParams(temperature=1.0, max_tokens=8), n=3)  # no seed: rid-derived ones
    got = _drive(e)
    assert len({tuple(got[c]) for c in IDS}) == 3
    _clean(e, 32)


def test_n_1_is_the_call_without_n():
    prompt = _prompt(2, 40)
    a, b = _engine(32, True), _engine(32, True)
    sa = a.add_request("a", prompt, _sp())
    sb = b.add_request("a", prompt, _sp(), n=1)
    assert type(sb) is type(sa) and sb.rid == sa.rid and sb.parent is None
    ga, gb = _drive(a), _drive(b)
    drop = ("last_step_s", "host_s", "wait_s")
    assert ga == gb and {k: v for k, v in a.stats.items() if k not in drop} == \
        {k: v for k, v in b.stats.items() if k not in drop}
    assert b.stats["fork_requests"] == 0
    with pytest.raises(ValueError):
        a.add_request("z", prompt, _sp(), n=0)
    with pytest.raises(ValueError):
        a.add_request("z", prompt, _sp(), n=a.r.max_batch + 1)


@pytest.mark.parametrize("cache", [False, True])
def test_parent_gone_before_admission_falls_back_to_a_full_prefill(cache):
    """Two slots, one taken by another stream: the parent finishes (max_tokens = 1) before its sibling can get a slot;
    the sibling then prefills on its own (the prefix index, when on, still spares it the full pages)."""
    prompt = _prompt(3, 2 * PAGE + 5)
    e = _engine(32, cache, max_batch=2)
    seen = _spy_prefill(e)
    e.add_request("b", _prompt(33, 20), SamplingParams(temperature=0.0, max_tokens=30))
    e.add_request("a", prompt, _sp(mt=1), n=2)
    got = _drive(e)
    assert e.stats["fork_requests"] == 1 and e.stats["fork_shared_tokens"] == 0 and e.stats["fork_tail_copies"] == 0
    start = 2 * PAGE if cache else 0
    assert [x for x in seen if x[0] != "b"] == [("a", 0, len(prompt)), ("a-c1", start, len(prompt) - start)]
    for i, c in enumerate(IDS[:2]):
        assert got[c] == _solo(32, cache, prompt, i, mt=1), c
    assert len(got["b"]) == 31
    _clean(e, 32)


def test_a_small_pool_makes_siblings_wait_without_preempting_the_parent():
    """5 pages, watermark 1: beside the parent's 3-page prompt there is room for one sibling's private page; the
    other waits for pages (and, its parent gone by then, prefills on its own).  Nobody is preempted for an admission,
    and everyone finishes with the right tokens."""
    prompt = _prompt(4, 2 * PAGE + 5)
    e = _engine(5, False)
    e.add_request("a", prompt, _sp(mt=6), n=3)
    waited = []
    hooks = {k: (lambda e: waited.append(len(e.waiting))) for k in range(1, 40)}
    got = _drive(e, hooks)
    assert max(waited) >= 1  # a sibling sat in the queue while the parent ran
    assert e.stats["preemptions"] == 0 and e.stats["fork_tail_copies"] == 1
    for i, c in enumerate(IDS):
        assert got[c] == _solo(32, False, prompt, i, mt=6), c
    _clean(e, 5)


@pytest.mark.parametrize("cache", [False, True])
def test_abort_ends_every_choice(cache):
    prompt = _prompt(5, 2 * PAGE + 5)
    e = _engine(32, cache)
    e.add_request("a", prompt, _sp(mt=40), n=3)
    got = _drive(e, {4: lambda e: e.abort("a")})
    for c in IDS:
        assert got[c][-1][2] and got[c][-1][3] == "abort" and len(got[c]) < 41, c
    _clean(e, 32)
    # one choice alone: the others run on (what a stop string match does)
    e.add_request("a", prompt, _sp(mt=12), n=3)
    got = _drive(e, {4: lambda e: (e.abort("a", choices=False), e.abort("a-c2"))})
    assert got["a"][-1][3] == "abort" and got["a-c2"][-1][3] == "abort"
    assert got["a-c1"] == _solo(32, cache, prompt, 1, mt=12)
    _clean(e, 32)
    assert not e._groups and not e._group_of


@pytest.mark.parametrize("cache", [False, True])
def test_a_preempted_sibling_resumes_with_the_same_tokens(cache):
    prompt = _prompt(6, 2 * PAGE + 5)
    e = _engine(32, cache)
    e.add_request("a", prompt, _sp(mt=14), n=3)

    def kick(e):
        v = next(s for s in e.slots if s is not None and s.conversation_id == "a-c1")
        assert v.state == "decode" and e.alloc.is_shared(v.blocks[0])
        e._preempt(v)

    got = _drive(e, {5: kick})
    assert e.stats["preemptions"] == 1
    for i, c in enumerate(IDS):
        assert got[c] == _solo(32, cache, prompt, i, mt=14), c
    _clean(e, 32)


# ---------------------------------------------------------------------------------------------- TP plan
def test_plan_carries_n_and_single_choice_aborts():
    p = Plan(step=True, adds=[(7, [1, 2, 3], _sp(), 123, 4), (11, [4, 5], _sp(), 456)], aborts=[7, -9])
    q = p.roundtrip()
    assert [a[4] if len(a) > 4 else 1 for a in q.adds] == [4, 1] and q.aborts == [7, -9]
    assert q.adds[1] == (11, [4, 5], q.adds[1][2], 456)
    one = Plan(adds=[(11, [4, 5], _sp(), 456)])
    assert one.encode() == Plan(adds=[(11, [4, 5], _sp(), 456, 1)]).encode()  # n = 1 encodes as ever


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        std = init_standard_weights(TINY, seed=3)
        w = convert_standard(TINY, std, tp_rank=rank, tp_size=world)
        r = ModelRunner(w, num_blocks=32, max_batch=4, max_model_len=256, device="cpu",
                        comm=TPComm(rank=rank, size=world, group=None), use_graphs=False)
        e = LLMEngine(r, eos_id=-1, prefill_budget=128)
        # every rank applies the plan the leader would broadcast (the leader's own ids on rank 0, rids elsewhere)
        lead = TPLeader(e, None)
        lead.add("a", _prompt(7, 2 * PAGE + 5), _sp(mt=6), 1, n=3)
        plan = lead.plan.roundtrip()
        apply_plan(e, plan, lead._conv.__getitem__) if rank == 0 else apply_plan(e, plan)
        rids = sorted(s.rid for s in e.waiting)
        toks = {}
        for _ in range(200):
            for ev in e.step():
                rid = lead._rid[ev.conversation_id] if rank == 0 else \
                    next(k for k in lead._conv if ev.conversation_id in (f"tp-rid-{k}",))
                toks.setdefault(rid, []).append((ev.token_id, ev.done))
            if not e.has_work():
                break
        out[rank] = (rids, toks, e.stats["fork_shared_tokens"], e.stats["fork_tail_copies"])
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_tp2_ranks_make_the_same_rids_and_tokens():
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_tp_worker, args=(2, _port(), out), nprocs=2, join=True)
        a, b = out[0], out[1]
    assert a[0] == b[0] == list(range(a[0][0], a[0][0] + 3))
    assert a[1] == b[1] and len(a[1]) == 3 and all(len(v) == 7 and v[-1][1] for v in a[1].values())
    assert a[2] == b[2] == 2 * (2 * PAGE + 4) and a[3] == b[3] == 2
    assert len({tuple(v) for v in a[1].values()}) == 3
