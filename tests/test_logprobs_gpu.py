"""logprobs / top_logprobs on the GPU: the statistics, chosen-logit and finish passes against torch.log_softmax in
float64 of the same fp32 logits, vocab shards, the row -> slot map, a row with penalties too, and the runner's
captured / eager / lazily captured paths.

Bound: |logprob - float64 reference| <= 2e-5.  For |x| <= 32 and V <= 32768 the kernel's error is a few 2^-23
relative in each exponential and in the sum (tree depth 15), about 1e-6 in log s, plus the final rounding of
|lp| <~ 45 (2^-18 ~ 4e-6); a dropped shard, a wrong max or an off-by-one N misses by >= 1e-2.  Measured maxima are in
profiles/r8/logprobs.md."""
import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

TOL = 2e-5
SENT = 777.0  # sentinel of untouched record / ring words
NS = [-1, 0, 5, 20]  # the four rows: off, N = 0, N = 5, N = 20


def _logits(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * 4.0).clamp_(-32.0, 32.0)


def _plant_tie(x, b, n):
    """Make the values ranked n-1, n, n+1 (1-based) of row b equal: a tie that straddles rank n."""
    V = x.shape[1]
    order = torch.sort(x[b], descending=True, stable=True).indices
    for k in (n - 2, n - 1, n):
        if 0 <= k < V:
            x[b, order[k]] = x[b, order[min(max(n - 1, 0), V - 1)]]


def _want(x_row, n):
    """float64 log-softmax of the row and the first n ids of the stable descending sort."""
    lp = torch.log_softmax(x_row.double(), dim=0)
    order = torch.sort(x_row, descending=True, stable=True).indices
    return lp, order[:min(n, x_row.numel())].tolist()


def _check_ring_row(out, x_row, n, tok):
    """out = the 41 ring words of one token: sampled logprob, ids and top logprobs against float64."""
    lp, ids = _want(x_row, n)
    got_ids = out.view(torch.int32)[1:1 + ops.LP_TOP].tolist()
    got_lp = out[1 + ops.LP_TOP:]
    assert got_ids[:len(ids)] == ids
    assert got_ids[len(ids):] == [-1] * (ops.LP_TOP - len(ids))
    assert bool(torch.isinf(got_lp[len(ids):]).all())
    err = [abs(float(out[0]) - float(lp[tok]))]
    err += [abs(float(got_lp[j]) - float(lp[i])) for j, i in enumerate(ids)]
    assert max(err) <= TOL, max(err)
    return max(err)


def _pipeline(gpu, shards, lp_meta, active, row_slot, next_ids, slots, ring_kw, R=4, raw=False):
    """stats per shard (one call each, as TP ranks would) -> chosen per shard -> finish with world = len(shards).
    shards = [(device logits view, vocab_offset)].  Returns (rec_all, lp_ring) on the host."""
    B = shards[0][0].shape[0]
    world = len(shards)
    rec_all = torch.full((world, B, ops.LP_REC), SENT, device=gpu)
    chosen_all = torch.full((world, B), SENT, device=gpu)
    ring = torch.full((R, slots, ops.LP_OUT), SENT, device=gpu)
    for w, (x, off) in enumerate(shards):
        rw = torch.zeros(B, x.shape[1], device=gpu) if raw else None
        ops.logprob_stats(x, active, lp_meta, row_slot, rec_all[w], rw, off)
        ops.logprob_chosen(rw if raw else x, next_ids, active, lp_meta, row_slot, chosen_all[w], off)
    ops.logprob_finish(rec_all, chosen_all, active, lp_meta, row_slot, ring, **ring_kw)
    return rec_all.cpu(), ring.cpu()


@pytest.mark.parametrize("V", [16, 1000, 32768])
def test_stats_and_finish_match_float64_log_softmax(gpu, V):
    B, ld = 4, V + 24
    buf = torch.zeros(B, ld)
    buf[:, :V] = _logits(B, V, V)
    for b, n in enumerate(NS):
        if n > 0:
            _plant_tie(buf[:, :V], b, n)  # (at V = 16 row 3 has N = 20 > V: all 16 come back, no rank 20 to straddle)
    x0 = buf[:, :V].clone()
    i32 = dict(dtype=torch.int32, device=gpu)
    lp_meta = torch.tensor(NS, **i32)
    toks = [3, V - 1, 7 % V, V // 2]
    counter = torch.tensor([6], **i32)  # ring row 6 % 4 = 2
    dbuf = buf.to(gpu)
    rec, ring = _pipeline(gpu, [(dbuf[:, :V], 0)], lp_meta, None, None, torch.tensor(toks, **i32), B,
                          dict(ring_counter=counter))
    assert torch.equal(dbuf.cpu(), buf)  # the logits themselves are only read
    assert bool((rec[0, 0] == SENT).all()) and bool((ring[:, 0] == SENT).all())  # the off row: nothing written
    assert bool((ring[[0, 1, 3]] == SENT).all())  # the other ring rows
    worst = max(_check_ring_row(ring[2, b], x0[b], NS[b], toks[b]) for b in (1, 2, 3))
    print(f"V={V}: max |logprob - float64| = {worst:.3e}")
    # the record: max, sum and the unused entries
    for b in (1, 2, 3):
        assert float(rec[0, b, 0]) == float(x0[b].max())
        s = float(torch.exp(x0[b].double() - x0[b].double().max()).sum())
        assert abs(float(rec[0, b, 1]) - s) <= 4e-6 * s
        n = min(NS[b], V)
        assert bool(torch.isinf(rec[0, b, 2 + 2 * n::2]).all())
        assert rec[0, b].view(torch.int32)[3 + 2 * n::2].tolist() == [0x7FFFFFFF] * (ops.LP_TOP - n)
    # the CPU twin writes the same ids and values within the bound
    rec_c = torch.full((1, B, ops.LP_REC), SENT)
    ch_c, ring_c = torch.full((1, B), SENT), torch.full((4, B, ops.LP_OUT), SENT)
    ref.logprob_stats(x0, None, lp_meta.cpu(), None, rec_c[0], None, 0)
    ref.logprob_chosen(x0, torch.tensor(toks, dtype=torch.int32), None, lp_meta.cpu(), None, ch_c[0], 0)
    ref.logprob_finish(rec_c, ch_c, None, lp_meta.cpu(), None, ring_c, ring_counter=counter.cpu())
    assert torch.equal(ring_c.view(torch.int32)[:, :, 1:21], ring.view(torch.int32)[:, :, 1:21])
    fin = torch.isfinite(ring_c)
    assert torch.equal(fin, torch.isfinite(ring)) and float((ring_c[fin] - ring[fin]).abs().max()) <= TOL


def test_vocab_shards_merge_to_the_unsharded_result(gpu):
    """V = 4096 as 4 shards of 1024 (four calls, then the finish with world = 4) = world 1: same ids, same bound.
    Shard 2 is all -inf; a tie across rank N has its members in shards 0 and 3; an inactive row stays untouched."""
    B, V, S = 4, 4096, 1024
    x0 = _logits(B, V, 77)
    x0[:, 2 * S:3 * S] = float("-inf")
    ns = [5, 20, 3, 0]
    for b, n in enumerate(ns[:2]):
        order = torch.sort(x0[b], descending=True, stable=True).indices
        v = float(x0[b, order[n - 1]])
        x0[b, order[n - 1]] = -33.0  # (moved out of the way, then the tie is planted in two shards)
        x0[b, 100 + b], x0[b, 3 * S + 50 + b] = v, v
    i32 = dict(dtype=torch.int32, device=gpu)
    lp_meta = torch.tensor(ns, **i32)
    active = torch.tensor([1, 1, 0, 1], **i32)
    toks = [100, 3 * S + 5, 9, 2 * S + 1]  # row 3 sampled a -inf token of the empty shard: logprob -inf
    nid = torch.tensor(toks, **i32)
    d = x0.to(gpu)
    kw = dict(ring_row=1)
    _, one = _pipeline(gpu, [(d, 0)], lp_meta, active, None, nid, B, kw)
    rec4, four = _pipeline(gpu, [(d[:, k * S:(k + 1) * S], k * S) for k in range(4)], lp_meta, active, None, nid, B, kw)
    assert torch.equal(one.view(torch.int32)[:, :, 1:21], four.view(torch.int32)[:, :, 1:21])
    assert bool(torch.isinf(rec4[2, [0, 1, 3], 0]).all()) and bool((rec4[2, [0, 1, 3], 1] == 0).all())
    assert bool((four[1, 2] == SENT).all()) and bool((rec4[:, 2] == SENT).all())  # the inactive row
    for ring in (one, four):
        for b in (0, 1):
            _check_ring_row(ring[1, b], x0[b], ns[b], toks[b])
            ids = ring[1, b].view(torch.int32)[1:1 + ns[b]].tolist()
            assert 100 + b in ids and 3 * S + 50 + b not in ids  # the tie's lower id won rank N
        assert float(ring[1, 3, 0]) == float("-inf") and ring[1, 3].view(torch.int32)[1:21].tolist() == [-1] * 20
    fin = torch.isfinite(one)
    assert float((one[fin] - four[fin]).abs().max()) <= TOL


def test_row_slot_map_lands_in_the_right_slot_and_ring_row(gpu):
    """4 gathered first-token rows of slots [11, 2, 7, 14] of a 16-slot state; the ring row comes from the device
    word the captured graphs read (meta's ring row), then from the eager path's host integer."""
    Bm, V = 16, 1000
    slots = [11, 2, 7, 14]
    ns = {11: 4, 2: -1, 7: 20, 14: 0}
    x0 = _logits(4, V, 5)
    i32 = dict(dtype=torch.int32, device=gpu)
    meta = torch.full((Bm,), -1, dtype=torch.int32)
    for s, n in ns.items():
        meta[s] = n
    meta[3] = 9  # a slot no row maps to
    toks = [1, 2, 3, 4]
    for kw, row in ((dict(ring_row_dev=torch.tensor([3], **i32)), 3), (dict(ring_row=0), 0)):
        _, ring = _pipeline(gpu, [(x0.to(gpu), 0)], meta.to(gpu), torch.tensor([1, 1, 1, 1], **i32),
                            torch.tensor(slots, **i32), torch.tensor(toks, **i32), Bm, kw)
        for b, s in enumerate(slots):
            if ns[s] >= 0:
                _check_ring_row(ring[row, s], x0[b], ns[s], toks[b])
        untouched = torch.ones(4, Bm, dtype=torch.bool)
        untouched[row, [11, 7, 14]] = False
        assert bool((ring[untouched] == SENT).all())


def test_row_with_penalties_reports_the_unpenalised_logprobs(gpu):
    """Greedy rows whose penalties move the argmax: the sampled token is the penalised reference's, its logprob and
    the top-N are the log-softmax of the logits BEFORE the penalty pass."""
    B, V, cap = 3, 1000, 16
    g = torch.Generator().manual_seed(3)
    x0 = torch.stack([torch.randperm(V, generator=g).float() * 0.03125 for _ in range(B)])  # distinct, |x| < 32
    top = [int(x0[b].argmax()) for b in range(B)]
    pen = torch.zeros(4 * B, dtype=torch.int32)
    fl = pen.view(torch.float32)
    fl[2 * B:3 * B] = 1.0
    hist = torch.zeros(B, cap + 1, dtype=torch.int32)
    fl[0] = 2.0        # row 0: presence 2 on its top token (generated once)
    hist[0, :2] = torch.tensor([1, top[0]])
    fl[2 * B + 2] = 2.0  # row 2: repetition 2 on its top token (a prompt token)
    hist[2, :2] = torch.tensor([1, top[2]])
    pen[3 * B + 2] = 1
    want = x0.double().clone()
    ref.sample_penalties(want, None, pen, hist)
    want_ids = want.argmax(dim=1).tolist()
    assert want_ids[0] != top[0] and want_ids[1] == top[1] and want_ids[2] != top[2]
    i32 = dict(dtype=torch.int32, device=gpu)
    ns = [5, 5, 2]
    lp_meta = torch.tensor(ns, **i32)
    logits, dp, dh = x0.clone().to(gpu), pen.clone().to(gpu), hist.clone().to(gpu)
    rec = torch.zeros(1, B, ops.LP_REC, device=gpu)
    raw = torch.zeros(B, V, device=gpu)
    chosen = torch.zeros(1, B, device=gpu)
    ring = torch.full((2, B, ops.LP_OUT), SENT, device=gpu)
    next_ids, positions = torch.full((B,), -1, **i32), torch.full((B,), 10, **i32)
    cand = torch.zeros(B, 16, 2, device=gpu)
    ops.logprob_stats(logits, None, lp_meta, None, rec[0], raw, 0)
    ops.sample_penalties(logits, None, dp, dh, None, 0, V)
    ops.sample_candidates(logits, torch.zeros(B, device=gpu), torch.zeros(B, **i32), torch.ones(B, device=gpu),
                          torch.zeros(B, 2, **i32), positions, None, cand, 0)
    ops.sample_pick_hist(cand.unsqueeze(0), None, next_ids, None, None, None, dp, dh, vocab=V)
    ops.logprob_chosen(raw, next_ids, None, lp_meta, None, chosen[0], 0, V)
    ops.logprob_finish(rec, chosen, None, lp_meta, None, ring, ring_row=1, vocab=V)
    assert next_ids.cpu().tolist() == want_ids
    assert not torch.equal(logits.cpu(), x0) and torch.equal(raw.cpu(), x0)
    out = ring.cpu()
    for b in range(B):
        _check_ring_row(out[1, b], x0[b], ns[b], want_ids[b])
        assert int(out[1, b].view(torch.int32)[1]) == top[b]  # rank 0 is the unpenalised argmax


# ------------------------------------------------------------------------------------------------ runner
PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 170)), [7] * 33]
TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]
LPS = [-1, 20, 3]  # slot 0 off
STEPS = 12


@pytest.fixture(scope="module")
def weights(gpu):
    return convert_standard(TINY, init_standard_weights(TINY, seed=1), device=gpu)


def _run(weights, gpu, graphs, swap_at=None):
    """First token + STEPS greedy decode tokens of the three prompts; per sequence [(token, 41 ring words)]; every
    decode step's row is also checked against float64 on that step's own logits."""
    r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=graphs)
    if graphs:
        r.capture([4])
    for i, bt in enumerate(TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
        r.lp_meta[i] = LPS[i]
    r.enable_logprobs()
    r.prefill([PrefillSeq(i, p, 0, TABLES[i], True) for i, p in enumerate(PROMPTS)], ring_row=0)
    r.active[:3] = 1
    where = [0, 1, 2]
    out = [[(int(r.ids[i]), r.lp_ring[0, i].cpu())] for i in range(3)]
    worst = 0.0
    for step in range(STEPS):
        if step == swap_at:
            r.move_slots([1, 2], [2, 1])
            r.block_tables[[1, 2]] = r.block_tables[[2, 1]]
            where = [0, 2, 1]
        r.decode(4)
        row = step % r.ring.shape[0]  # (the first decode step reuses ring row 0, read above)
        ring, lp, logits = r.ring[row].cpu(), r.lp_ring[row].cpu(), r.logits[:4].cpu()
        for i in range(3):
            s = where[i]
            out[i].append((int(ring[s]), lp[s]))
            if LPS[i] >= 0:
                worst = max(worst, _check_ring_row(lp[s], logits[s], LPS[i], int(ring[s])))
    torch.cuda.synchronize()
    print(f"runner graphs={graphs}: max |logprob - float64| over {STEPS} decode steps = {worst:.3e}")
    return out, r, where


def _same(a, b):
    for sa, sb in zip(a, b):
        assert [t for t, _ in sa] == [t for t, _ in sb]
        for (_, x), (_, y) in zip(sa, sb):
            assert torch.equal(x.view(torch.int32)[1:21], y.view(torch.int32)[1:21])
            fin = torch.isfinite(x)
            assert torch.equal(fin, torch.isfinite(y)) and float((x[fin] - y[fin]).abs().max()) <= TOL


@pytest.fixture(scope="module")
def eager_run(weights, gpu):
    return _run(weights, gpu, False)


def test_runner_graph_replay_equals_eager(weights, gpu, eager_run):
    out, r, _ = _run(weights, gpu, True)
    dec, pfg, mxg = r._graph_set()
    assert dec is not r.graphs and set(dec) == set(r.graphs) and set(pfg) == set(r.pf_graphs)
    assert {B: [c for c, _ in v] for B, v in mxg.items()} == {B: [c for c, _ in v] for B, v in r.mx_graphs.items()}
    assert not r.pen_graphs  # the penalty-only twins were never needed
    _same(out, eager_run[0])
    for i in (1, 2):  # greedy: the sampled token is rank 0 and its logprob is the first top entry
        for tok, w in out[i]:
            assert int(w.view(torch.int32)[1]) == tok and float(w[0]) == float(w[21]) and float(w[0]) <= 0.0
    assert all(bool((w == 0).all()) for _, w in out[0])  # the off slot's ring words were never written


def test_runner_setting_moves_with_its_slot(weights, gpu, eager_run):
    out, r, where = _run(weights, gpu, False, swap_at=STEPS // 2)
    _same(out, eager_run[0])
    assert r.lp_meta.cpu().tolist()[:3] == [-1, 3, 20]


def test_engine_first_logprobs_request_arrives_mid_stream(weights, gpu):
    """Captured graphs, a stream decoding when the first logprobs request arrives (its prompt rides in a mixed
    step): the twins are captured then, the neighbour's tokens stay bit-identical, and the new stream's tokens
    are the ones it samples without logprobs; every one of its tokens carries a logprob and N sorted tops."""
    from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams

    def run(n, graphs=True):
        r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=graphs)
        if graphs:
            r.capture()
        e = LLMEngine(r, eos_id=-1, prefill_budget=256)
        out = {"a": [], "b": []}
        for step in range(400):
            if step == 0:
                e.add_request("a", PROMPTS[1], SamplingParams(temperature=0.0, max_tokens=30, ignore_eos=True))
            if step == 8:
                e.add_request("b", PROMPTS[2], SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True,
                                                              logprobs=n))
            for ev in e.step():
                if not ev.done:
                    out[ev.conversation_id].append(ev)
            if step > 8 and not e.has_work():
                break
        assert not e.has_work()
        return out, r, e

    plain, r0, _ = run(-1)
    got, r1, e1 = run(4)
    assert not r0._twins.get((False, True, False, False)) and not r0.lp_used
    assert set(r1._twins[(False, True, False, False)][0]) == set(r1.graphs) and not r1.pen_graphs
    assert e1.stats["mixed_steps"] > 0
    for c in "ab":
        assert [ev.token_id for ev in got[c]] == [ev.token_id for ev in plain[c]]
    assert len(got["a"]) == 30 and all(ev.logprob is None and ev.top is None for ev in got["a"] + plain["b"])
    assert len(got["b"]) == 16
    for ev in got["b"]:
        assert len(ev.top) == 4 and ev.top[0][0] == ev.token_id and ev.logprob == ev.top[0][1] <= 0.0
        vals = [v for _, v in ev.top]
        assert vals == sorted(vals, reverse=True) and sum(torch.tensor(vals).exp().tolist()) <= 1.0 + 1e-5
    # the eager engine (no graphs; separate prefill and decode passes) reports the same ids and values within the bound
    eager, _, _ = run(4, graphs=False)
    assert [ev.token_id for ev in eager["b"]] == [ev.token_id for ev in got["b"]]
    for x, y in zip(eager["b"], got["b"]):
        assert [t for t, _ in x.top] == [t for t, _ in y.top]
        assert max(abs(u - v) for (_, u), (_, v) in zip(x.top, y.top)) <= TOL and abs(x.logprob - y.logprob) <= TOL
