"""logit_bias / min_tokens / stop_token_ids / min_p on the GPU: the bias and ban pass bit for bit against its CPU
twin, min_p in the filtered sampler against the float64 kept set, and the runner's captured / eager / compacted
decode and the engine's lazily captured graph twins."""
import math

import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ bias and ban pass
def _ctl(Bm):
    return torch.zeros(4 * Bm, dtype=torch.int32), torch.zeros(Bm, ops.CTL_BODY, dtype=torch.int32)


def _set(meta, body, slot, bias=(), bans=(), until=0):
    Bm = meta.numel() // 4
    meta[slot], meta[Bm + slot], meta[2 * Bm + slot] = len(bias), len(bans), until
    if bias:
        ids, vals = zip(*bias)
        body[slot, 0:2 * len(bias):2] = torch.tensor(ids, dtype=torch.int32)
        body[slot, 1:2 * len(bias):2] = torch.tensor(vals, dtype=torch.float32).view(torch.int32)
    body[slot, 2 * ops.CTL_BIAS:2 * ops.CTL_BIAS + len(bans)] = torch.tensor(list(bans), dtype=torch.int32)


def _entries(n, vocab, gen):
    ids = torch.randperm(vocab, generator=gen)[:n].tolist()
    vals = (torch.rand(n, generator=gen) * 200 - 100).tolist()
    return list(zip(ids, vals))


@pytest.mark.parametrize("V, offset, vocab", [(1000, 0, 1000), (32768, 0, 32768), (16384, 0, 32768),
                                              (16384, 16384, 32768)])
def test_bias_ban_kernel_matches_the_twin_bit_for_bit(gpu, V, offset, vocab):
    """3 rows (row 1 inactive) over 4 slots through a row_slot permutation; slot 3: 300 entries and a ban in force,
    slot 2: 1 entry and an expired ban, slot 1: 300 entries but its row is inactive, slot 0: nothing.  With two
    shards of 16384 the ids of the other shard are skipped."""
    g = torch.Generator().manual_seed(V + offset)
    x0 = torch.randn(3, V, generator=g) * 3
    meta, body = _ctl(4)
    bans = [2, vocab - 1, 5, vocab // 2 - 1, vocab // 2] + list(range(100, 112))  # 17 ids, in both shards
    _set(meta, body, 3, _entries(300, vocab, g), bans, until=41)
    _set(meta, body, 2, [(offset + 7, 3.5)], [offset + 9], until=30)
    _set(meta, body, 1, _entries(300, vocab, g), bans, until=41)
    row_slot = torch.tensor([3, 1, 2], dtype=torch.int32)
    active = torch.tensor([1, 0, 1], dtype=torch.int32)
    pos = torch.tensor([39, 39, 29], dtype=torch.int32)  # row 0: 40 < 41 in force; row 2: 30 >= 30 expired
    want = x0.clone()
    ref.sample_bias_ban(want, active, meta, body, pos, row_slot, offset, vocab)
    got = x0.to(gpu)
    ops.sample_bias_ban(got, active.to(gpu), meta.to(gpu), body.to(gpu), pos.to(gpu), row_slot.to(gpu), offset, vocab)
    got = got.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[1], x0[1])                                    # inactive: bit-identical
    changed = (got[2].view(torch.int32) != x0[2].view(torch.int32)).nonzero().flatten().tolist()
    assert changed == [7] and float(got[2, 7]) == float(x0[2, 7] + torch.tensor(3.5))  # the expired ban wrote nothing
    n_inf = int(torch.isinf(got[0]).sum())
    assert n_inf == sum(1 for t in set(bans) if offset <= t < offset + V) and n_inf > 0
    # 0 entries and no ban anywhere: the whole tensor stays bit-identical (row = slot, no map)
    meta0, body0 = _ctl(4)
    y = x0.to(gpu)
    ops.sample_bias_ban(y, None, meta0.to(gpu), body0.to(gpu), pos.to(gpu), None, offset, vocab)
    assert torch.equal(y.cpu().view(torch.int32), x0.view(torch.int32))


# ------------------------------------------------------------------------------------------------ min_p
def _kept64(x, T, min_p, top_k, top_p):
    """The float64 kept set of one row, with the distance of every decision from its threshold asserted."""
    d = x.double() / T
    d = d - d.max()
    thr = math.log(min_p)
    assert float((d - thr).abs().min()) > 1e-4 * abs(thr), "a logit sits on the min_p threshold"
    keep = d >= thr
    if top_k:
        kth = torch.topk(d, top_k + 1).values
        assert float(kth[-2] - kth[-1]) > 1e-4
        keep &= d >= kth[-2]
    if top_p < 1.0:
        pr = torch.where(keep, torch.exp(d), torch.zeros_like(d))
        pr = pr / pr.sum()
        vals, order = torch.sort(pr, descending=True)
        cum = torch.cumsum(vals, 0)
        n = int(torch.searchsorted(cum, torch.tensor(top_p, dtype=torch.float64))) + 1
        assert float((cum[:n + 1] - top_p).abs().min()) > 1e-4, "the top-p mass sits on its boundary"
        k2 = torch.zeros_like(keep)
        k2[order[:n]] = True
        keep &= k2
    return keep


CASES = [(0.8, 0.05, 0, 1.0), (1.0, 0.02, 20, 1.0), (0.7, 0.01, 0, 0.9)]  # (T, min_p, top_k, top_p)


@pytest.mark.parametrize("V", [1000, 32768])
def test_min_p_token_equals_the_twin(gpu, V):
    """64 seeds per case: min_p alone, with top-k, with top-p.  Rows are not slots here (row_slot)."""
    g = torch.Generator().manual_seed(V)
    S = 64
    base = torch.randn(len(CASES), V, generator=g) * 3
    meta, _ = _ctl(4)
    rows = len(CASES) * S
    logits = base.repeat_interleave(S, 0).contiguous()
    row_slot = torch.arange(len(CASES), dtype=torch.int32).repeat_interleave(S) + 1  # slots 1..3
    t = torch.zeros(rows)
    k = torch.zeros(rows, dtype=torch.int32)
    p = torch.ones(rows)
    for c, (T, mp, tk, tp) in enumerate(CASES):
        meta[3 * 4 + 1 + c:3 * 4 + 2 + c].view(torch.float32)[0] = mp
        t[c * S:(c + 1) * S], k[c * S:(c + 1) * S], p[c * S:(c + 1) * S] = T, tk, tp
        keep = _kept64(base[c], T, mp, tk, tp)
        assert 1 < int(keep.sum()) < V
    seeds = torch.stack([torch.arange(rows, dtype=torch.int32), torch.full((rows,), 3, dtype=torch.int32)], 1)
    pos = torch.arange(rows, dtype=torch.int32)
    cand_r = torch.zeros(rows, 1, 2)
    ops.sample_candidates_min_p(logits, t, k, p, seeds, pos, None, cand_r, meta, row_slot, 0)
    cand = torch.zeros(rows, 16, 2, device=gpu)
    ops.sample_candidates_min_p(logits.to(gpu), t.to(gpu), k.to(gpu), p.to(gpu), seeds.to(gpu), pos.to(gpu), None,
                                cand, meta.to(gpu), row_slot.to(gpu), 0)
    ids = torch.zeros(rows, dtype=torch.int32, device=gpu)
    ops.sample_pick(cand.unsqueeze(0), None, ids, vocab=V)
    want = cand_r[:, 0, 1].to(torch.int32)
    assert torch.equal(ids.cpu(), want)
    for c, (T, mp, tk, tp) in enumerate(CASES):
        keep = _kept64(base[c], T, mp, tk, tp)
        assert bool(keep[ids.cpu()[c * S:(c + 1) * S].long()].all())


def test_min_p_samples_cover_the_kept_set(gpu):
    """2,000 seeds on one row whose only filter is min_p: every sample lies in the float64 kept set and every kept
    token of mass >= 5 % appears."""
    V, N, T, mp = 1000, 2000, 1.0, 0.1
    g = torch.Generator().manual_seed(77)
    x = torch.randn(V, generator=g) * 2
    keep = _kept64(x, T, mp, 0, 1.0)
    meta, _ = _ctl(1)
    meta[3:].view(torch.float32)[0] = mp
    logits = x.repeat(N, 1).to(gpu)
    seeds = torch.stack([torch.arange(N, dtype=torch.int32), torch.full((N,), 9, dtype=torch.int32)], 1).to(gpu)
    cand = torch.zeros(N, 16, 2, device=gpu)
    i32 = dict(dtype=torch.int32, device=gpu)
    ops.sample_candidates_min_p(logits, torch.full((N,), T, device=gpu), torch.zeros(N, **i32),
                                torch.ones(N, device=gpu), seeds, torch.zeros(N, **i32), None, cand, meta.to(gpu),
                                torch.zeros(N, **i32), 0)
    ids = torch.zeros(N, **i32)
    ops.sample_pick(cand.unsqueeze(0), None, ids, vocab=V)
    ids = ids.cpu().long()
    assert bool(keep[ids].all())
    pr = torch.where(keep, torch.exp(x.double() - x.double().max()), torch.zeros(V, dtype=torch.float64))
    pr = pr / pr.sum()
    must = (pr >= 0.05).nonzero().flatten().tolist()
    assert must and set(must) <= set(ids.tolist())  # (0.95 ** 2000: a miss is out of the question)
    # a greedy row with min_p set is the plain argmax
    ops.sample_candidates_min_p(logits[:2], torch.zeros(2, device=gpu), torch.zeros(2, **i32),
                                torch.ones(2, device=gpu), seeds[:2], torch.zeros(2, **i32), None, cand[:2],
                                meta.to(gpu), torch.zeros(2, **i32), 0)
    ids2 = torch.zeros(2, **i32)
    ops.sample_pick(cand[:2].unsqueeze(0), None, ids2, vocab=V)
    assert ids2.cpu().tolist() == [int(x.argmax())] * 2


# ------------------------------------------------------------------------------------------------ runner
PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 170)), [7] * 33]
TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]
STEPS = 16
V = TINY.vocab_size
# slot 0 neutral; slot 1: bias entries in the vocabulary's both halves; slot 2: token V - 3 forced, banned 6 tokens long
CTL = [None, ({3: 6.0, V - 2: 5.5, 40: -100.0, 41: -100.0}, [], 0), ({V - 3: 100.0}, [V - 3, 1], 6)]


@pytest.fixture(scope="module")
def weights(gpu):
    return convert_standard(TINY, init_standard_weights(TINY, seed=1), device=gpu)


def _meta(r, slot, ctl, n_prompt):
    Bm = r.max_batch
    bias, bans, mn = ctl
    r.ctl_meta[slot], r.ctl_meta[Bm + slot], r.ctl_meta[2 * Bm + slot] = len(bias), len(bans), n_prompt + mn


def _run(weights, gpu, graphs, ctl=CTL, swap_at=None):
    r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=graphs)
    if graphs:
        r.capture([4])
    for i, bt in enumerate(TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
        if ctl[i] is not None:
            r.set_controls(i, ctl[i][0], ctl[i][1])
            _meta(r, i, ctl[i], len(PROMPTS[i]))
    r.prefill([PrefillSeq(i, p, 0, TABLES[i], True) for i, p in enumerate(PROMPTS)], ring_row=0)
    r.active[:3] = 1
    where = [0, 1, 2]
    first = r.ids.cpu().tolist()
    toks = [[first[i]] for i in range(3)]
    for step in range(STEPS):
        if step == swap_at:  # slots 1 <-> 2: records and ctl_meta through move_slots, the block tables by hand
            r.move_slots([1, 2], [2, 1])
            r.block_tables[[1, 2]] = r.block_tables[[2, 1]]
            where = [0, 2, 1]
        r.decode(4)
        row = r.ring.cpu()[step]
        for i in range(3):
            toks[i].append(int(row[where[i]]))
    torch.cuda.synchronize()
    return toks, r


@pytest.fixture(scope="module")
def eager_run(weights, gpu):
    return _run(weights, gpu, False)


def test_runner_obeys_bias_and_ban(eager_run):
    toks, _ = eager_run
    assert not {40, 41} & set(toks[1])
    assert V - 3 not in toks[2][:6] and toks[2][6:] == [V - 3] * (len(toks[2]) - 6)  # first token included: 6 banned


def test_runner_graph_replay_equals_eager(weights, gpu, eager_run):
    toks, r = _run(weights, gpu, True)
    key = (False, False, True, False)
    assert r.graphs and r.pf_graphs and set(r._twins[key][0]) == set(r.graphs)
    assert set(r._twins[key][1]) == set(r.pf_graphs) and not r.pen_graphs
    assert r._graph_set()[0] is r._twins[key][0] and r._graph_set()[0] is not r.graphs
    assert toks == eager_run[0]


def test_runner_neutral_slot_ignores_its_neighbours(weights, gpu, eager_run):
    plain, r = _run(weights, gpu, False, ctl=[None] * 3)
    assert not r.ctl_used
    assert plain[0] == eager_run[0][0]
    assert plain[1] != eager_run[0][1] and plain[2] != eager_run[0][2]


def test_runner_streams_continue_across_a_slot_swap(weights, gpu, eager_run):
    toks, _ = _run(weights, gpu, False, swap_at=STEPS // 2)
    assert toks == eager_run[0]


def test_runner_without_the_fields_replays_the_startup_graphs(weights, gpu):
    toks, r = _run(weights, gpu, True, ctl=[None] * 3)
    dec, pfg, mxg = r._graph_set()
    assert dec is r.graphs and pfg is r.pf_graphs and mxg is r.mx_graphs
    assert not r.ctl_used and not any(any(t) for t in r._twins.values())


def test_engine_first_biased_request_arrives_mid_stream(weights, gpu):
    """Captured graphs, a plain stream decoding when the first request with a bias arrives: the twins with the bias
    and ban pass are captured then, the running stream's tokens are unchanged, the biased stream obeys the bias."""
    from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams

    def run(with_bias):
        r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=True)
        r.capture()
        e = LLMEngine(r, eos_id=-1, prefill_budget=256)
        out = {"a": [], "b": []}
        for step in range(400):
            if step == 0:
                e.add_request("a", PROMPTS[1], SamplingParams(temperature=0.0, max_tokens=30, ignore_eos=True))
            if step == 8:
                e.add_request("b", PROMPTS[2], SamplingParams(
                    temperature=0.0, max_tokens=16, ignore_eos=True, stop_token_ids=(1,),
                    logit_bias={V - 3: 100.0} if with_bias else None, min_tokens=5 if with_bias else 0))
            for ev in e.step():
                if not ev.done:
                    out[ev.conversation_id].append(ev.token_id)
            if step > 8 and not e.has_work():
                break
        assert not e.has_work()
        return out, r

    plain, r0 = run(False)
    got, r1 = run(True)
    key = (False, False, True, False)
    assert not r0.ctl_used and key not in r0._twins and r0._graph_set()[0] is r0.graphs
    assert set(r1._twins[key][0]) == set(r1.graphs) and not r1.pen_graphs
    assert len(plain["a"]) == 30 and got["a"] == plain["a"]
    assert got["b"] == [V - 3] * 16 and plain["b"] != got["b"]
