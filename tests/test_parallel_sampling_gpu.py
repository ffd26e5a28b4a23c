"""Parallel sampling (n > 1) on the GPU: the kv_pages_copy HIP kernel against the reference op (bit-exact, on integer
views), the wrapper's refusals before any launch, and the engine's fork -- shared full prompt pages, a copied partial
last page, a one-token chunk -- against independent n = 1 requests, on captured graphs and eagerly, bf16 and fp8 KV.

The engine comparison is the one tests/test_prefix_cache_gpu.py makes between a prefix hit and a cold prefill
(test_prefix_cache_cpu._same_up_to_ties): identical streams, or a first difference that is a near-tie of the fp32
reference's logits.  That bound is about an argmax, so the streams here are greedy; the request still carries a seed,
and choice i is compared with the independent request of seed + i.  (Seeded sampling at temperature > 0, where the
tokens are exactly equal, is pinned on the CPU engine: tests/test_parallel_sampling_cpu.py.)"""
import pytest
import torch

import test_prefix_cache_cpu as tpc
from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams
from distributed_sse_for_llm_response_amd.engine.kv_cache import PAGE
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as ref
from test_prefix_cache_cpu import _prompt, _same_up_to_ties, _toks

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float8_e4m3fn]
PAIRS = [[], [(5, 2)], [(7, 0), (1, 3), (6, 4)], [(3, 6), (3, 1)]]  # none; one; three; one source, two destinations


def _caches(L, blocks, hkv, dtype, seed, device):
    """K and V of random BYTES (every bit pattern, NaNs included: the kernel moves bytes), and the same on the CPU."""
    g = torch.Generator().manual_seed(seed)
    nb = dtype.itemsize
    k8 = torch.randint(0, 256, (L, blocks, hkv, 32, 128 * nb), generator=g, dtype=torch.uint8)
    v8 = torch.randint(0, 256, (L, blocks, hkv, 128, 32 * nb), generator=g, dtype=torch.uint8)
    return (k8.to(device).view(dtype), v8.to(device).view(dtype)), (k8.clone().view(dtype), v8.clone().view(dtype))


def _i(t):
    return t.cpu().contiguous().view(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp8"])
@pytest.mark.parametrize("hkv", [1, 2])
def test_copy_matches_the_reference_byte_for_byte(gpu, hkv, dtype):
    L, blocks = 2, 8
    for seed, pairs in enumerate(PAIRS):
        (k, v), (kc, vc) = _caches(L, blocks, hkv, dtype, 10 + seed, gpu)
        k0, v0 = _i(kc).clone(), _i(vc).clone()
        ops.kv_pages_copy(k, v, pairs)
        ref.kv_pages_copy(kc, vc, torch.tensor(pairs, dtype=torch.int32).view(-1, 2))
        assert torch.equal(_i(k), _i(kc)) and torch.equal(_i(v), _i(vc)), pairs
        dsts = {d for _, d in pairs}
        for b in range(blocks):
            if b in dsts:
                src = next(s for s, d in pairs if d == b)
                assert torch.equal(_i(k)[:, b], k0[:, src]) and torch.equal(_i(v)[:, b], v0[:, src]), (pairs, b)
            else:  # every page that is not a destination is unchanged
                assert torch.equal(_i(k)[:, b], k0[:, b]) and torch.equal(_i(v)[:, b], v0[:, b]), (pairs, b)


def test_copy_refuses_bad_pairs_before_any_launch(gpu):
    L, blocks, hkv = 2, 8, 2
    (k, v), (kc, vc) = _caches(L, blocks, hkv, torch.bfloat16, 3, gpu)
    for bad, what in (([(0, blocks)], "outside"), ([(blocks + 3, 1)], "outside"), ([(-1, 2)], "outside"),
                      ([(0, 1), (2, 1)], "duplicate destination"),
                      ([(0, 1), (1, 2)], "both a destination and a source"), ([(4, 4)], "both a destination")):
        with pytest.raises(ValueError, match=what):
            ops.kv_pages_copy(k, v, bad)
    torch.cuda.synchronize()
    assert torch.equal(_i(k), _i(kc)) and torch.equal(_i(v), _i(vc))  # nothing was launched
    idx = torch.tensor([[0, 1]], dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match="pairs"):  # the raw op checks what it can without a device sync
        torch.ops.dsse.kv_pages_copy(k, v, idx.long())
    with pytest.raises(RuntimeError, match="pairs"):
        torch.ops.dsse.kv_pages_copy(k, v, idx.view(-1))
    with pytest.raises(RuntimeError, match="v_cache"):
        torch.ops.dsse.kv_pages_copy(k, v.view(torch.float8_e4m3fn), idx)


# ------------------------------------------------------------------------------------------------ engine
_ENGINES = {}


def _engine(gpu, graphs, dtype):
    """One engine of 64 pages per (graphs, KV dtype), shared by the cases of this file (capturing is most of its
    cost); every case leaves it idle.  The weights are the ones _same_up_to_ties judges near-ties with."""
    key = (graphs, dtype)
    if key not in _ENGINES:
        if str(gpu) not in tpc._W:
            tpc._W[str(gpu)] = convert_standard(TINY, init_standard_weights(TINY, seed=11), device=gpu)
        r = ModelRunner(tpc._W[str(gpu)], num_blocks=64, max_batch=4, max_model_len=512, device=gpu,
                        use_graphs=graphs, kv_cache_dtype=dtype)
        if graphs:
            r.capture()
        _ENGINES[key] = LLMEngine(r, eos_id=-1, prefill_budget=256)
    e = _ENGINES[key]
    assert not e.has_work() and e.alloc.num_free == 64
    return e


def _run(e, conv, prompt, params, n=1):
    e.add_request(conv, prompt, params, n=n)
    out = {}
    for _ in range(400):
        for ev in e.step():
            out.setdefault(ev.conversation_id, []).append((ev.token_id, ev.sequence, ev.done, ev.finish))
        if not e.has_work():
            break
    assert not e.has_work(), "engine did not drain"
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_forked_choices_match_independent_requests(gpu, graphs, dtype):
    e = _engine(gpu, graphs, dtype)
    seed, n, new = 77, 3, 12
    for k, (length, copies) in enumerate(((2 * PAGE + 5, 2), (2 * PAGE + 1, 0))):
        prompt = _prompt(200 + k, length)
        before = dict(e.stats)
        got = _run(e, "g", prompt, SamplingParams(temperature=0.0, max_tokens=new, seed=seed), n=n)
        ids = ["g", "g-c1", "g-c2"]
        assert sorted(got) == sorted(ids)
        # two siblings, each spared len - 1 prompt tokens; the partial last page is copied only when there is one
        assert e.stats["fork_requests"] - before["fork_requests"] == 1
        assert e.stats["fork_shared_tokens"] - before["fork_shared_tokens"] == (n - 1) * (length - 1)
        assert e.stats["fork_tail_copies"] - before["fork_tail_copies"] == copies
        assert e.stats["prefill_tokens"] - before["prefill_tokens"] == length + (n - 1)
        assert e.alloc.num_free == 64 and not e.alloc.has_forks
        want, reqs = {}, []
        for i, c in enumerate(ids):
            solo = _run(e, f"s{i}", prompt, SamplingParams(temperature=0.0, max_tokens=new, seed=seed + i))
            want[c] = [(t, s, d, f) for t, s, d, f in solo[f"s{i}"]]
            reqs.append((c, prompt, new, 0))
            assert len(_toks(got[c])) == new and got[c][-1][2:] == (True, "length")
        print(f"graphs={graphs} kv={dtype} len={length}:",
              {c: ("same" if got[c] == want[c] else "differs") for c in ids})
        _same_up_to_ties(got, want, reqs)
    assert e.alloc.num_free == 64


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_seeded_siblings_sample_different_streams_on_captured_graphs(gpu, dtype):
    """Temperature 1 with a seed through the device sampler of the captured graphs: choice i draws with seed + i, so
    the three streams differ from one another; lengths, counters and pages hold as for the greedy runs.  (No
    comparison with separate requests here: at temperature > 0 a rounding difference between two passes moves a draw
    across a CDF boundary, which no logit near-tie bounds; that equality is exact on the CPU engine and pinned there.)"""
    e = _engine(gpu, True, dtype)
    length, n, new = 2 * PAGE + 5, 3, 12
    prompt = _prompt(210, length)
    sp = SamplingParams(temperature=1.0, max_tokens=new, seed=31)
    before = dict(e.stats)
    a = _run(e, "t", prompt, sp, n=n)
    ids = ["t", "t-c1", "t-c2"]
    assert sorted(a) == sorted(ids)
    for c in ids:
        assert len(_toks(a[c])) == new and a[c][-1][2:] == (True, "length")
    assert len({tuple(_toks(a[c])) for c in ids}) == n, a
    assert e.stats["fork_requests"] - before["fork_requests"] == 1
    assert e.stats["fork_shared_tokens"] - before["fork_shared_tokens"] == (n - 1) * (length - 1)
    assert e.stats["fork_tail_copies"] - before["fork_tail_copies"] == n - 1
    assert e.alloc.num_free == 64 and not e.alloc.has_forks
