"""Host-memory tier of the prefix cache on the CPU engine: the allocator's spill list, HostPageStore's slot states and
LRU, the lookup across both tiers, and the engine's spill at eviction / restore at admission (through the reference
kv_pages ops and the same KVOffload ring as on the GPU, with every copy synchronous).

The oracle for a restored prefix is the same request on an engine whose pool keeps the prefix resident: a restored
page is the evicted page's bytes, so on the CPU the greedy streams are equal, not merely equal up to ties."""
import argparse

import pytest
import torch

from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine
from distributed_sse_for_llm_response_amd.engine.kv_cache import PAGE, BlockAllocator, HostPageStore, page_hashes
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
from distributed_sse_for_llm_response_amd.serving.config import ServeConfig
from test_prefix_cache_cpu import _engine, _prompt, _same_up_to_ties, _streams, _toks, _W


def offload_engine(num_blocks, kv_cache_dtype="auto", device="cpu", use_graphs=False, prefix_cache=True, **kw):
    """test_prefix_cache_cpu._engine with a KV cache dtype (same weights, same defaults)."""
    _engine(1, False, device=device)  # (fills the shared weight cache for this device)
    r = ModelRunner(_W[str(device)], num_blocks=num_blocks, max_batch=4, max_model_len=512, device=device,
                    use_graphs=use_graphs, kv_cache_dtype=kv_cache_dtype)
    if use_graphs:
        r.capture()
    kw.setdefault("prefill_budget", 256)
    return LLMEngine(r, eos_id=-1, prefix_cache=prefix_cache, **kw)


# ---------------------------------------------------------------------------------------------- allocator
def _trace(al):
    """A recorded sequence of allocate / free / publish / lookup calls on a pool of 4 (publish and lookup only where
    the prefix cache is on; the frees are ordered so that the evictable pool's least recently used page is also the
    plain free list's last one).  Returns (the blocks every allocate returned, the publish / lookup results)."""
    h = page_hashes(_prompt(300, 2 * PAGE))
    allocs, others = [], []
    a = al.allocate(4)
    allocs.append(a)
    if al.prefix_cache:
        others.append(al.publish(a[0], h[0]))
    al.free(a[:1])
    al.free(a[1:])
    if al.prefix_cache:
        others.append(al.lookup(h[:1]))  # revived from the evictable pool ...
        al.free(a[:1])                   # ... and back in it
    b = al.allocate(4)  # three plain pages, then the published one is evicted
    allocs.append(b)
    if al.prefix_cache:
        others.append(al.publish(b[1], h[1]))
        others.append(al.lookup(h[:1]))  # evicted: a miss
    al.free(b[1:2])
    al.free([b[0], b[2], b[3]])
    allocs.append(al.allocate(3))
    allocs.append(al.allocate(1))  # the second eviction
    return allocs, others


def test_allocator_trace_is_the_same_in_all_three_arms():
    plain = BlockAllocator(4, prefix_cache=False)
    cached = BlockAllocator(4, prefix_cache=True)
    store = HostPageStore(8, 64)
    tiered = BlockAllocator(4, prefix_cache=True, host_store=store)
    t_plain, t_cached, t_tiered = _trace(plain), _trace(cached), _trace(tiered)
    assert t_plain[0] == t_cached[0] == t_tiered[0] == [[0, 1, 2, 3], [1, 2, 3, 0], [1, 3, 0], [2]]
    assert t_cached[1] == t_tiered[1] == [True, [0], True, []]  # (publish / lookup results too)
    assert t_plain[1] == []
    # only the store arm yields a spill list: exactly the evicted pages, in eviction order
    assert plain.take_spills() == [] and cached.take_spills() == []
    h = page_hashes(_prompt(300, 2 * PAGE))
    assert cached.evictions == tiered.evictions == 2
    assert tiered.take_spills() == [(0, h[0]), (2, h[1])]
    assert tiered.take_spills() == []
    assert len(store) == 0  # (the allocator only lists them: the engine decides what is copied)
    with pytest.raises(ValueError, match="prefix_cache"):
        BlockAllocator(4, prefix_cache=False, host_store=store)


# ---------------------------------------------------------------------------------------------- host store
def test_host_store_states_and_lru():
    st = HostPageStore(3, 32)
    assert st.buf.shape == (3, 32) and st.buf.dtype == torch.uint8
    h = [bytes([i]) * 16 for i in range(6)]
    s0 = st.reserve(h[0])
    assert st.state[s0] == "filling" and st.find(h[0]) is None and st.has(h[0])  # invisible until its copy is done
    assert st.reserve(h[0]) is None  # a duplicate hash is not stored twice, whatever its state
    st.commit(s0)
    assert st.find(h[0]) == s0 and st.reserve(h[0]) is None and len(st) == 1
    s1, s2 = st.reserve(h[1]), st.reserve(h[2])
    st.commit(s1)
    st.commit(s2)
    assert sorted((s0, s1, s2)) == [0, 1, 2]
    # at capacity the least recently used ready slot is recycled: h0's
    s3 = st.reserve(h[3])
    assert s3 == s0 and st.find(h[0]) is None and not st.has(h[0]) and st.recycled == 1
    st.commit(s3)
    # a slot being read is never recycled, and reading makes it the most recently used once released
    st.acquire(s1)
    st.acquire(s1)  # (two restores may read one slot)
    assert st.state[s1] == "reading" and st.find(h[1]) == s1
    s4 = st.reserve(h[4])
    assert s4 == s2 and st.find(h[2]) is None  # h1 is older than h2 but being read: h2 goes
    s5 = st.reserve(h[5])
    assert s5 == s3  # next oldest ready slot (h3); s4 is filling, s1 reading
    assert st.reserve(h[0]) is None  # every slot is filling or being read: nothing to recycle, no exception
    st.release(s1)
    assert st.state[s1] == "reading"
    st.release(s1)
    assert st.state[s1] == "ready"
    st.cancel(s5)  # a reservation whose copy was never issued
    assert st.state[s5] == "free" and not st.has(h[5])
    assert st.reserve(h[0]) == s5
    with pytest.raises(ValueError):
        HostPageStore(0, 32)


def test_lookup_walks_both_tiers_and_stops_at_the_first_miss():
    st = HostPageStore(4, 16)
    al = BlockAllocator(8, prefix_cache=True, host_store=st)
    h = page_hashes(_prompt(301, 6 * PAGE))
    blocks = al.allocate(2)
    for i in (0, 1):
        al.publish(blocks[i], h[i])
    slots = {}
    for i in (2, 3, 5):
        slots[i] = st.reserve(h[i])
        st.commit(slots[i])
    run, host = al.lookup_tiers(h)
    assert run == [blocks[0], blocks[1], None, None] and host == [(2, slots[2]), (3, slots[3])]
    assert st.state[slots[2]] == st.state[slots[3]] == "reading" and st.state[slots[5]] == "ready"  # 5: not touched
    assert al._ref[blocks[0]] == 2
    al.free(blocks)
    for _, s in host:
        st.release(s)
    # mixed runs (HBM, host, HBM) are legal, a filling slot ends the run, and max_host cuts it
    b4 = al.allocate(1)[0]
    al.publish(b4, h[4])
    assert al.lookup_tiers(h)[0] == [blocks[0], blocks[1], None, None, b4, None]
    run, host = al.lookup_tiers(h, max_host=1)
    assert run == [blocks[0], blocks[1], None] and host == [(2, slots[2])]
    filling = HostPageStore(2, 16)
    al2 = BlockAllocator(4, prefix_cache=True, host_store=filling)
    filling.reserve(h[0])
    assert al2.lookup_tiers(h) == ([], [])
    # no store attached: the resident run, no host pages
    al3 = BlockAllocator(4, prefix_cache=True)
    b = al3.allocate(1)
    al3.publish(b[0], h[0])
    assert al3.lookup_tiers(h) == ([b[0]], [])


# ---------------------------------------------------------------------------------------------- engine
def _page_bytes(e, blocks):
    kv = e.r.kv
    return [torch.cat([kv.k[:, b].reshape(-1).view(torch.uint8).cpu(), kv.v[:, b].reshape(-1).view(torch.uint8).cpu()])
            for b in blocks]


def restored_prefix(mk, same, settle=lambda e: e.offload.poll()):
    """Scenario 4 (shared with the GPU test): A (96 tokens) is served, four distinct prompts evict all its pages
    from a pool of 8, then A plus one turn is served from the host tier.  `mk(num_blocks, **engine kwargs)` builds an
    engine; `same(got, want, reqs)` compares the second turn with the run whose pool keeps A resident; `settle(e)`
    retires the tier's finished copies (the GPU test waits for the device first)."""
    A = _prompt(500, 96)
    first = [("a", A, 4, 0)]
    evictors = [[(f"e{i}", _prompt(510 + i, 96), 4, 0)] for i in range(4)]
    second = [("a2", A + _prompt(600, 20), 8, 0)]
    hs = page_hashes(A)
    e = mk(8, kv_offload_pages=16)
    assert e.offload is not None and e.alloc.host_store.capacity == 16
    _streams(e, first)
    before = _page_bytes(e, [e.alloc._index[h] for h in hs])
    for r in evictors:
        _streams(e, r)
    assert not any(h in e.alloc._index for h in hs)  # every page of A left HBM ...
    settle(e)
    assert all(e.alloc.host_store.find(h) is not None for h in hs)  # ... for the host tier
    assert e.stats["offload_restored_pages"] == 0 and e.stats["offload_spilled_pages"] >= 3
    cached = {}
    got = _streams(e, second, cached=cached)
    assert cached == {"a2": 96}
    assert e.stats["offload_restored_pages"] == 3 and e.stats["offload_hit_tokens"] == 96
    assert e.stats["offload_dropped_pages"] == 0
    after = _page_bytes(e, [e.alloc._index[h] for h in hs])
    for x, y in zip(before, after):
        assert torch.equal(x, y)  # the restored pages are the evicted pages, byte for byte
    assert all(e.alloc.host_store.find(h) is not None for h in hs)  # (the host copy stays)
    settle(e)
    assert e.offload.free_records() == e.offload.R and e.alloc.num_free == 8
    assert "reading" not in e.alloc.host_store.state and "filling" not in e.alloc.host_store.state
    big = mk(64)
    assert big.offload is None and "offload_restored_pages" not in big.stats
    _streams(big, first)
    for r in evictors:
        _streams(big, r)
    cached = {}
    want = _streams(big, second, cached=cached)
    assert cached == {"a2": 96} and big.stats["prefix_evictions"] == 0  # the resident-prefix run
    same(got, want, second)
    return e


def _equal(got, want, reqs):
    assert got == want


@pytest.mark.parametrize("kv_cache_dtype", ["bf16", "fp8"])
def test_evicted_prefix_comes_back_from_the_host_tier(kv_cache_dtype):
    restored_prefix(lambda n, **kw: offload_engine(n, kv_cache_dtype, **kw), _equal)


def test_a_page_already_in_the_store_is_not_copied_again():
    e = offload_engine(8, kv_offload_pages=16)
    A = _prompt(500, 96)
    evictors = [[(f"e{i}", _prompt(510 + i, 96), 4, 0)] for i in range(4)]
    _streams(e, [("a", A, 4, 0)])
    for r in evictors:
        _streams(e, r)
    _streams(e, [("a2", A + _prompt(600, 20), 8, 0)])  # restored: A's pages are in both tiers now
    spilled = e.stats["offload_spilled_pages"]
    for r in evictors:
        _streams(e, r)  # evicts them again
    assert not any(h in e.alloc._index for h in page_hashes(A))
    assert e.stats["offload_spill_skipped"] >= 3
    assert e.stats["offload_spilled_pages"] + e.stats["offload_spill_skipped"] - spilled >= 3


def test_preempted_stream_restores_from_the_host_tier():
    """Two streams whose KV outgrows a pool of 8 pages: the newer one is preempted, its published pages are evicted by
    the survivor's growth, and its re-admission finds them in the host tier.

    The oracle is the same run with the tier off, where the re-admission prefills those pages again.  The two runs
    are not bit-identical by construction: a restored page holds the K/V its decode steps wrote, the tier-off run
    recomputes the same positions in one prefill pass, and the two differ in bf16 rounding -- exactly the situation
    of test_prefix_cache_cpu.test_preemption_with_the_cache_on, whose comparison is used here: equal streams, or a
    first difference that is a near-tie of the fp32 reference (< 0.02 of its largest logit), after which the
    continuations legitimately differ.  Measured on four prompt pairs: two give identical streams, two (this one
    among them) differ first at s1's token 77 / 79 of 100, each time within that near-tie bound."""
    reqs = [("s0", _prompt(700, 60), 150, 0), ("s1", _prompt(701, 70), 100, 1)]
    off = offload_engine(8)
    want = _streams(off, reqs)
    assert off.stats["preemptions"] > 0
    on = offload_engine(8, kv_offload_pages=16)
    got = _streams(on, reqs)
    assert on.stats["preemptions"] > 0
    assert on.stats["offload_restored_pages"] >= 1, on.stats
    assert on.shared_write_violations == 0
    for c, _, mt, _ in reqs:
        assert len(_toks(got[c])) == mt and got[c][-1][3] == "length"
        assert [s for _, s, d, _ in got[c] if not d] == list(range(1, mt + 1))
    assert got["s0"] == want["s0"]  # the stream that was never preempted
    _same_up_to_ties(got, want, reqs)
    assert on.alloc.num_free == 8


def test_more_evictions_than_staging_records_drop_the_rest():
    e = offload_engine(8, kv_offload_pages=16, offload_ring_pages=2)
    assert e.offload.R == 2
    p = _prompt(800, 160)  # five full pages
    _streams(e, [("p", p, 4, 0)])
    assert len(e.alloc._lru) == 5
    hs = page_hashes(p)[:5]
    spy = []
    orig = e.offload.spill
    e.offload.spill = lambda pairs: (spy.append(len(pairs)), orig(pairs))[1]
    _streams(e, [("q", _prompt(801, 250), 4, 0)])  # eight pages at once: one step evicts all five
    assert e.stats["prefix_evictions"] == 5
    assert spy and max(spy) <= 2  # never more in one call than the ring has records
    spilled, dropped = e.stats["offload_spilled_pages"], e.stats["offload_dropped_pages"]
    assert spilled >= 2 and spilled + dropped == 5 and dropped >= 1, e.stats
    e.offload.poll()
    st = e.alloc.host_store
    kept = [h for h in hs if st.find(h) is not None]
    assert len(kept) == spilled
    # the dropped ones were the least recently used (the prompt's tail pages go first): later lookups miss them,
    # and a lookup of the whole chain stops at the first dropped page
    assert kept == hs[:len(kept)]
    run, host = e.alloc.lookup_tiers(hs)
    assert len(run) == len(kept) and [i for i, _ in host] == list(range(len(kept)))
    for _, s in host:
        st.release(s)


# ---------------------------------------------------------------------------------------------- configuration
def test_config_errors_and_the_cli_flag(monkeypatch):
    assert ServeConfig().kv_offload_gb == 0 and ServeConfig().validate().kv_offload_gb == 0  # 0 is off
    ap = argparse.ArgumentParser()
    ServeConfig.add_args(ap)
    monkeypatch.setenv("KV_OFFLOAD_GB", "1")
    assert ServeConfig.from_env().kv_offload_gb == 1.0
    with pytest.raises(ValueError, match="enable-prefix-caching"):
        ServeConfig.from_env().update_from_args(ap.parse_args([]))
    monkeypatch.setenv("ENABLE_PREFIX_CACHING", "1")
    assert ServeConfig.from_env().update_from_args(ap.parse_args([])).kv_offload_gb == 1.0
    monkeypatch.setenv("TP", "2")
    with pytest.raises(ValueError, match="tensor parallelism"):
        ServeConfig.from_env().update_from_args(ap.parse_args([]))
    for k in ("KV_OFFLOAD_GB", "ENABLE_PREFIX_CACHING", "TP"):
        monkeypatch.delenv(k)
    c = ServeConfig.from_env().update_from_args(ap.parse_args(["--enable-prefix-caching", "--kv-offload-gb", "0.5"]))
    assert c.kv_offload_gb == 0.5 and c.enable_prefix_caching
    assert ServeConfig.from_json(c.to_json()).kv_offload_gb == 0.5  # (how DP worker processes get it)
    assert ServeConfig.from_env().update_from_args(ap.parse_args([])).kv_offload_gb == 0
    with pytest.raises(ValueError, match=">= 0"):
        ServeConfig(kv_offload_gb=-1.0).validate()


def test_config_reaches_the_engine_and_a_value_below_one_page_raises():
    from distributed_sse_for_llm_response_amd.engine.kv_cache import KVCache
    from distributed_sse_for_llm_response_amd.serving.app import build_engine, kv_offload_pages

    def cfg(**kw):
        return ServeConfig(engine="cpu", max_tokens=4, temperature=0.0, **kw)

    e, _ = build_engine(cfg())
    assert e.offload is None and e.alloc.host_store is None
    kv = e.r.kv
    per = KVCache.bytes_per_block(kv.num_layers, kv.nkv, kv.dtype)
    e, _ = build_engine(cfg(enable_prefix_caching=True, kv_offload_gb=10.5 * per / 2**30))
    assert e.offload is not None and e.alloc.host_store.capacity == 10 and e.alloc.host_store.bytes_per_block == per
    with pytest.raises(ValueError, match="less than one KV page"):
        kv_offload_pages(cfg(enable_prefix_caching=True, kv_offload_gb=0.5 * per / 2**30), e.r)
    with pytest.raises(ValueError, match="enable-prefix-caching"):
        build_engine(cfg(kv_offload_gb=1.0))
    # the engine's own guards (an engine built in code)
    with pytest.raises(ValueError, match="prefix_cache"):
        offload_engine(8, prefix_cache=False, kv_offload_pages=4)
