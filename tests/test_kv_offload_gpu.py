"""Host-memory tier of the prefix cache on the GPU: the kv_pages_gather / kv_pages_scatter HIP kernels against the
reference ops (bit-exact, on integer views), the wrapper's refusals before any launch, and the engine's spill and
restore through the kernels, a side stream and pinned host memory."""
import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.kv_cache import page_hashes
from distributed_sse_for_llm_response_amd.ops import reference as ref
from test_kv_offload_cpu import offload_engine, restored_prefix
from test_prefix_cache_cpu import _prompt, _same_up_to_ties, _streams, _toks

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 2), (3, 16, 8)]  # (L, blocks, Hkv)
DTYPES = [torch.bfloat16, torch.float8_e4m3fn]


def _lists(blocks):
    return [[5], [7, 0, 3], list(range(blocks - 1, -1, -1))]  # one page; unsorted, both ends; every page, reversed


def _caches(L, blocks, hkv, dtype, seed, device):
    """K and V of random BYTES (every bit pattern, NaNs included: the kernels move bytes), and the same on the CPU."""
    g = torch.Generator().manual_seed(seed)
    nb = dtype.itemsize
    k8 = torch.randint(0, 256, (L, blocks, hkv, 32, 128 * nb), generator=g, dtype=torch.uint8)
    v8 = torch.randint(0, 256, (L, blocks, hkv, 128, 32 * nb), generator=g, dtype=torch.uint8)
    return (k8.to(device).view(dtype), v8.to(device).view(dtype)), (k8.view(dtype), v8.view(dtype))


def _staging(n, L, hkv, dtype, device, fill=0x5A):
    elems = 2 * L * hkv * 4096
    return torch.full((n, elems * dtype.itemsize), fill, dtype=torch.uint8, device=device).view(dtype)


def _i(t):
    return t.cpu().contiguous().view(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp8"])
@pytest.mark.parametrize("shape", SHAPES, ids=["L2b8h2", "L3b16h8"])
def test_gather_matches_the_reference_bit_for_bit(gpu, shape, dtype):
    L, blocks, hkv = shape
    (k, v), (kc, vc) = _caches(L, blocks, hkv, dtype, 1, gpu)
    for lst in _lists(blocks):
        n = len(lst)
        st = _staging(n + 1, L, hkv, dtype, gpu)  # one record more than listed: it must stay untouched
        want = _staging(n + 1, L, hkv, dtype, "cpu")
        ops.kv_pages_gather(k, v, lst, st)
        ref.kv_pages_gather(kc, vc, torch.tensor(lst, dtype=torch.int32), want)
        assert torch.equal(_i(st), _i(want)), lst
        # and record i really is [K layer 0 .. L-1 | V layer 0 .. L-1] of page lst[i]
        rec = _i(st)[0].view(2, L, -1)
        assert torch.equal(rec[0, L - 1], _i(kc[L - 1, lst[0]]).reshape(-1))
        assert torch.equal(rec[1, 0], _i(vc[0, lst[0]]).reshape(-1))
    assert torch.equal(_i(k), _i(kc)) and torch.equal(_i(v), _i(vc))  # a gather writes no cache byte
    st = _staging(2, L, hkv, dtype, gpu)
    ops.kv_pages_gather(k, v, [], st)  # n = 0: nothing is launched, staging untouched
    assert bool((_i(st) == 0x5A).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp8"])
@pytest.mark.parametrize("shape", SHAPES, ids=["L2b8h2", "L3b16h8"])
def test_scatter_writes_the_listed_pages_and_nothing_else(gpu, shape, dtype):
    L, blocks, hkv = shape
    for lst in _lists(blocks):
        (k, v), (kc, vc) = _caches(L, blocks, hkv, dtype, 2, gpu)
        n = len(lst)
        g = torch.Generator().manual_seed(3)
        rec8 = torch.randint(0, 256, (n, 2 * L * hkv * 4096 * dtype.itemsize), generator=g, dtype=torch.uint8)
        ops.kv_pages_scatter(rec8.to(gpu).view(dtype), lst, k, v)
        ref.kv_pages_scatter(rec8.view(dtype), torch.tensor(lst, dtype=torch.int32), kc, vc)
        # against the reference: the listed pages hold the records, every other page is the clone's
        assert torch.equal(_i(k), _i(kc)) and torch.equal(_i(v), _i(vc)), lst
        seg = hkv * 4096 * dtype.itemsize
        for i, b in enumerate(lst[:3]):
            r = rec8[i].view(2, L, seg)
            assert torch.equal(_i(k[:, b]).reshape(L, seg), r[0]) and torch.equal(_i(v[:, b]).reshape(L, seg), r[1])
    # gather -> scatter into different blocks -> gather reproduces the records
    (k, v), _ = _caches(L, blocks, hkv, dtype, 4, gpu)
    src, dst = [7, 0, 3], [1, 6, 2]
    a, b = _staging(3, L, hkv, dtype, gpu), _staging(3, L, hkv, dtype, gpu, fill=0)
    ops.kv_pages_gather(k, v, src, a)
    ops.kv_pages_scatter(a, dst, k, v)
    ops.kv_pages_gather(k, v, dst, b)
    assert torch.equal(_i(a), _i(b))
    before = (_i(k), _i(v))
    ops.kv_pages_scatter(a, [], k, v)  # n = 0
    assert torch.equal(_i(k), before[0]) and torch.equal(_i(v), before[1])


def test_wrapper_refuses_bad_arguments_before_any_launch(gpu, monkeypatch):
    L, blocks, hkv = 2, 8, 2
    (k, v), _ = _caches(L, blocks, hkv, torch.bfloat16, 5, gpu)
    st = _staging(2, L, hkv, torch.bfloat16, gpu)
    launched = []
    monkeypatch.setattr(ops, "_hip", lambda t: launched.append(1) or True)  # reached only past the validation
    k0, v0, s0 = _i(k), _i(v), _i(st)
    cases = [
        (lambda: ops.kv_pages_gather(k, v, [blocks], st), "blocks"),            # out of range
        (lambda: ops.kv_pages_scatter(st, [0, blocks + 3], k, v), "blocks"),
        (lambda: ops.kv_pages_gather(k, v, [-1], st), "blocks"),                # negative
        (lambda: ops.kv_pages_scatter(st, [-2], k, v), "blocks"),
        (lambda: ops.kv_pages_scatter(st, [3, 3], k, v), "blocks"),             # a duplicate in scatter
        (lambda: ops.kv_pages_gather(k, v, [0, 1, 2], st), "staging"),          # n above the staging capacity
        (lambda: ops.kv_pages_scatter(st, [0, 1, 2], k, v), "staging"),
        (lambda: ops.kv_pages_gather(k, v, [0], st.view(torch.float8_e4m3fn)), "staging"),  # bf16 cache, fp8 staging
        (lambda: ops.kv_pages_scatter(st.view(torch.float8_e4m3fn), [0], k, v), "staging"),
    ]
    for call, arg in cases:
        with pytest.raises((ValueError, RuntimeError), match=arg):
            call()
    assert not launched
    monkeypatch.undo()
    # the bindings' own checks (shapes, dtypes, contiguity), for a caller that goes past the wrapper
    idx = torch.tensor([0], dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match="staging has dtype"):
        torch.ops.dsse.kv_pages_gather(k, v, idx, st.view(torch.float8_e4m3fn))
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.dsse.kv_pages_gather(k.transpose(3, 4), v, idx, st)
    with pytest.raises(RuntimeError, match="staging holds"):
        torch.ops.dsse.kv_pages_scatter(st, torch.zeros(3, dtype=torch.int32, device=gpu), k, v)
    with pytest.raises(RuntimeError, match="blocks has dtype"):
        torch.ops.dsse.kv_pages_gather(k, v, idx.long(), st)
    torch.cuda.synchronize()
    assert torch.equal(_i(k), k0) and torch.equal(_i(v), v0) and torch.equal(_i(st), s0)  # nothing was written


def _drained(e):
    """The test's own wait for the host tier's copies (the engine never waits: it polls)."""
    torch.cuda.synchronize()
    e.offload.poll()


@pytest.mark.parametrize("kv_cache_dtype", ["bf16", "fp8"])
def test_evicted_prefix_comes_back_through_the_kernels(gpu, kv_cache_dtype):
    def mk(n, **kw):
        e = offload_engine(n, kv_cache_dtype, device=gpu, **kw)
        if e.offload is not None:
            assert e.alloc.host_store.buf.is_pinned() and e.offload.staging.is_cuda
        return e

    # (the scenario reads the store's state between requests: _drained lets the copies land first)
    restored_prefix(mk, _same_up_to_ties, settle=_drained)


def test_restored_prefix_chunk_rides_in_a_mixed_step(gpu):
    """test_prefix_cache_gpu.test_cached_prefix_chunk_rides_in_a_mixed_step with the prefix in the host tier: the
    prompt's two full pages are evicted, then the repeat is admitted while another stream decodes; its pages are
    restored and its remaining chunk (start_pos = 64 of 90) rides in that stream's decode step."""
    p, other = _prompt(80, 90), _prompt(81, 40)
    warm = [("w", p, 4, 0)]
    evict = [("x", _prompt(82, 250), 4, 0)]  # eight pages: the whole pool
    reqs = [("o", other, 40, 0), ("p", p, 20, 5)]
    want_e = offload_engine(64, device=gpu, use_graphs=True)  # the resident-prefix run
    _streams(want_e, warm)
    cached = {}
    want = _streams(want_e, reqs, cached=cached)
    assert cached == {"o": 0, "p": 64}
    on = offload_engine(8, device=gpu, use_graphs=True, kv_offload_pages=16)
    assert on.mixed
    _streams(on, warm)
    _streams(on, evict)
    _drained(on)
    assert on.alloc.lookup(page_hashes(p)) == []  # (gone from HBM)
    rode = []
    orig = on.r.mixed
    on.r.mixed = lambda B, chunks, **kw: (rode.extend((c.start_pos, len(c.tokens)) for c in chunks),
                                          orig(B, chunks, **kw))[1]
    cached = {}
    got = _streams(on, reqs, cached=cached)
    assert cached == {"o": 0, "p": 64}
    assert on.stats["offload_restored_pages"] == 2 and rode == [(64, 26)], (on.stats, rode)
    assert len(_toks(got["p"])) == 20 and len(_toks(got["o"])) == 40
    _same_up_to_ties(got, want, reqs)
    _drained(on)
    assert on.alloc.num_free == 8 and on.offload.free_records() == on.offload.R
