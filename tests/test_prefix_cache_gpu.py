"""Automatic prefix caching on the GPU.  The feature adds no kernel: a hit runs the existing prompt-chunk path at
start_pos > 0 over the paged cache and then ordinary decode.  What is new for the kernels is the regime, pinned here:
block tables of different sequences that name the same physical pages in one launch, and a short query run against a
longer context that starts at a page boundary which is not a 64-key block boundary."""
import functools

import pytest
import torch

from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights, reference_forward
from test_prefix_cache_cpu import _engine, _prompt, _same_up_to_ties, _streams, _toks, second_turn, \
    shared_live

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _mk(gpu):
    """Captured-graph engines of 64 pages, one with the cache on and one with it off, shared by the tests of this
    file (capturing is most of an engine's cost; every test uses prompts of its own and leaves its engines idle)."""
    def mk(cache):
        if cache not in _ENGINES:
            _ENGINES[cache] = _engine(64, cache, device=gpu, use_graphs=True)
        e = _ENGINES[cache]
        assert not e.has_work() and e.alloc.num_free == 64
        return e
    return mk


@pytest.mark.parametrize("split", [False, True])
def test_prefill_chunks_over_shared_pages_match_the_reference(gpu, monkeypatch, split):
    """X (96 tokens, 3 pages) is prefilled; then ONE prefill call runs two chunks whose block tables both start
    with X's three physical pages and go on in private pages, both at start_pos = 96 (a page boundary, not a 64-key
    block boundary): 5 tokens (less than a tile) and 70 tokens (more than one).  Each sampled token must be the
    fp32 reference's argmax on the full token list, within the bound tests/test_model_runner.py puts on the same
    quantity (reference logit gap < 0.1).  split: the flash key split is forced through its plan's parameters (every
    64-key block a range of its own), so partial slots exist whose keys a wave cannot see at all."""
    from distributed_sse_for_llm_response_amd.engine import model_runner as mr

    calls = []
    if split:
        monkeypatch.setattr(mr, "flash_split_plan",
                            functools.partial(mr.flash_split_plan, min_blocks=1, fill=1 << 20, min_target=1))
        orig = mr.ops.flash_prefill_split
        monkeypatch.setattr(mr.ops, "flash_prefill_split", lambda *a: (calls.append(a[-1]), orig(*a))[1])
    std = init_standard_weights(TINY, seed=1)
    w = convert_standard(TINY, std, device=gpu)
    r = ModelRunner(w, num_blocks=16, max_batch=4, max_model_len=512, device=gpu, use_graphs=False)
    x = _prompt(70, 96)
    tails = [_prompt(71, 5), _prompt(72, 70)]
    shared = [3, 7, 5]
    bts = [shared + [10], shared + [11, 12, 13]]
    r.prefill([PrefillSeq(0, x, 0, shared, False)], ring_row=0)
    r.prefill([PrefillSeq(1 + i, t, 96, bts[i], True) for i, t in enumerate(tails)], ring_row=0)
    ids = r.ids.cpu().tolist()
    if split:
        assert len(calls) == 2 * TINY.num_layers and all(n > 0 for n in calls), calls  # (the prefill of X splits too)
    for i, t in enumerate(tails):
        logits, _ = reference_forward(TINY, std, torch.tensor(x + t))
        row = logits[-1]
        gap = float(row.max() - row[ids[1 + i]])
        print(f"split={split} tail {len(t)}: sampled {ids[1 + i]}, reference gap {gap:.4f}")
        assert gap < 0.1, (len(t), gap)


def test_second_turn_on_captured_graphs(gpu):
    on = second_turn(_mk(gpu))  # asserts cached_tokens == 128, start_pos == 128 and the stream up to ties
    assert on.r.pf_graphs  # (the hit's chunk replayed a captured prefill graph)


def test_shared_live_pages_on_captured_graphs(gpu):
    shared_live(_mk(gpu))


def test_cached_prefix_chunk_rides_in_a_mixed_step(gpu):
    """A repeat of a finished prompt is admitted while another stream decodes: its chunk (start_pos = 64 of 90) rides
    in that stream's decode step (ModelRunner.mixed)."""
    mk = _mk(gpu)
    p, other = _prompt(80, 90), _prompt(81, 40)
    warm = [("w", p, 4, 0)]
    reqs = [("o", other, 40, 0), ("p", p, 20, 5)]
    off = mk(False)
    _streams(off, warm)
    want = _streams(off, reqs)
    on = mk(True)
    assert on.mixed
    _streams(on, warm)
    mixed_before = on.stats["mixed_steps"]
    rode = []
    orig = on.r.mixed
    on.r.mixed = lambda B, chunks, **kw: (rode.extend((c.start_pos, len(c.tokens)) for c in chunks),
                                          orig(B, chunks, **kw))[1]
    cached = {}
    try:
        got = _streams(on, reqs, cached=cached)
    finally:
        on.r.mixed = orig
    assert cached == {"o": 0, "p": 64}
    assert rode == [(64, 26)] and on.stats["mixed_steps"] > mixed_before, rode
    assert len(_toks(got["p"])) == 20 and len(_toks(got["o"])) == 40
    _same_up_to_ties(got, want, reqs)
    assert on.alloc.num_free == 64
