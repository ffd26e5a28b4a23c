"""Presence / frequency / repetition penalties on the GPU: the penalty pass, the history append of the pick and
first-token commit passes, and the runner's captured / eager / compacted decode, all against ops/reference.py
evaluated in float64."""
import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights
from distributed_sse_for_llm_response_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _state(Bm, cap):
    """Neutral host-side state: pen_meta [4 Bm] and hist [Bm, cap + 1]."""
    pen = torch.zeros(4 * Bm, dtype=torch.int32)
    pen[2 * Bm:3 * Bm].view(torch.float32).fill_(1.0)
    return pen, torch.zeros(Bm, cap + 1, dtype=torch.int32)


def _set(pen, hist, slot, p, f, r, n_prompt, tokens):
    Bm = hist.shape[0]
    fl = pen.view(torch.float32)
    fl[slot], fl[Bm + slot], fl[2 * Bm + slot] = p, f, r
    pen[3 * Bm + slot] = n_prompt
    hist[slot, 0] = len(tokens)
    hist[slot, 1:1 + len(tokens)] = torch.tensor(tokens, dtype=torch.int32)


def _check(got, x0, pen, hist, active, row_slot=None, vocab_offset=0):
    """got (device result, on the host) against the float64 reference on x0: every touched value within three fp32
    roundings, |got - ref| <= 1e-6 (|x| + |f| c + |p|); everything else bit-identical.  Returns the touched mask."""
    B, V = x0.shape
    want = x0.double().clone()
    ref.sample_penalties(want, active, pen, hist, row_slot, vocab_offset)
    touched = torch.zeros(B, V, dtype=torch.bool)
    bound = torch.zeros(B, V, dtype=torch.float64)
    Bm = hist.shape[0]
    fl = pen.view(torch.float32)
    for b in range(B):
        slot = int(row_slot[b]) if row_slot is not None else b
        if (active is not None and not int(active[b])) or not ref.penalties_on(pen, slot):
            continue
        p, f, n_prompt = float(fl[slot]), float(fl[Bm + slot]), int(pen[3 * Bm + slot])
        toks = hist[slot, 1:1 + int(hist[slot, 0])].tolist()
        for j, t in enumerate(toks):
            v = t - vocab_offset
            if 0 <= v < V:
                touched[b, v] = True
                bound[b, v] += abs(f) if j >= n_prompt else 0.0
        gen = {t - vocab_offset for t in toks[n_prompt:]}
        for v in gen:
            if 0 <= v < V:
                bound[b, v] += abs(p)
    bound = 1e-6 * (bound + x0.double().abs())
    err = (got.double() - want).abs()
    worst = float((err - bound)[touched].max()) if touched.any() else 0.0
    print(f"touched {int(touched.sum())}, worst |got - ref| {float(err.max()):.3e}, worst margin {worst:.3e}")
    assert bool((err[touched] <= bound[touched]).all())
    assert torch.equal(got.view(torch.int32)[~touched], x0.view(torch.int32)[~touched])  # bit-identical
    return touched


@pytest.mark.parametrize("V", [1000, 32768])
def test_penalty_pass(gpu, V):
    cap, B, ld = 512, 6, V + 24
    g = torch.Generator().manual_seed(V)
    pen, hist = _state(B, cap)
    pool = torch.randint(0, V, (40,), generator=g).tolist()  # few distinct tokens: they repeat in a long history
    long = [pool[i] for i in torch.randint(0, 40, (cap,), generator=g).tolist()]
    _set(pen, hist, 0, 0.5, 0.3, 1.3, 0, [])                       # empty history: nothing to do
    _set(pen, hist, 1, 0.7, 0.2, 1.5, 1, [V - 1])                  # a prompt-only token: repetition alone
    _set(pen, hist, 2, 0.0, 0.0, 1.0, 3, [3, 9, 3, 5, 9, 9, 1])    # neutral parameters
    _set(pen, hist, 3, 0.0, 0.01, 1.0, 0, [17] * 300)              # 300 repeats (an 8-bit count would wrap)
    _set(pen, hist, 4, -1.25, 0.4, 0.8, 200, long)                 # the full capacity, all three, r < 1
    _set(pen, hist, 5, 1.0, 1.0, 2.0, 2, [3, 9, 3, 5, 9, 9, 1])    # penalised but inactive
    active = torch.tensor([1, 1, 1, 1, 1, 0], dtype=torch.int32)
    buf = torch.randn(B, ld, generator=g) * 4.0
    x0 = buf[:, :V].clone()
    # both signs on penalised tokens of the long row (the repetition branch), and on the prompt-only token's row
    assert (x0[4, long] > 0).any() and (x0[4, long] < 0).any()
    dbuf = buf.to(gpu)
    ops.sample_penalties(dbuf[:, :V], active.to(gpu), pen.to(gpu), hist.to(gpu), None, 0, V)
    out = dbuf.cpu()
    assert torch.equal(out[:, V:].view(torch.int32), buf[:, V:].view(torch.int32))  # the row padding
    got = out[:, :V].contiguous()
    touched = _check(got, x0, pen, hist, active)
    assert not touched[0].any() and not touched[2].any() and not touched[5].any()
    # the prompt-only token got repetition, not frequency or presence
    x = float(x0[1, V - 1])
    assert float(got[1, V - 1]) == pytest.approx(x / 1.5 if x > 0 else x * 1.5, rel=1e-6)
    # 300 exact counts
    assert float(got[3, 17]) == pytest.approx(float(x0[3, 17]) - 3.0, abs=1e-5)


def test_penalty_pass_vocab_shards(gpu):
    """Two 512-wide shards of 1024-wide logits, same histories (global ids, some outside each shard, some outside
    both) = the unsharded pass."""
    B, V, cap = 4, 1024, 64
    g = torch.Generator().manual_seed(5)
    pen, hist = _state(B, cap)
    for b in range(B):
        toks = torch.randint(0, V, (40 + b,), generator=g).tolist() + [V + 7, 2000]
        _set(pen, hist, b, 0.5 * b, 0.25, 1.0 + 0.2 * b, 10 * b, toks)
    x0 = torch.randn(B, V, generator=g) * 3.0
    dp, dh = pen.to(gpu), hist.to(gpu)
    whole = x0.to(gpu)
    ops.sample_penalties(whole, None, dp, dh, None, 0, 4096)
    sharded = x0.to(gpu)
    ops.sample_penalties(sharded[:, :512], None, dp, dh, None, 0, 4096)
    ops.sample_penalties(sharded[:, 512:], None, dp, dh, None, 512, 4096)
    assert torch.equal(whole.view(torch.int32), sharded.view(torch.int32))
    _check(whole.cpu(), x0, pen, hist, None)
    lo = x0[:, :512].contiguous()
    _check(sharded.cpu()[:, 512:].contiguous(), x0[:, 512:].contiguous(), pen, hist, None, vocab_offset=512)
    _check(sharded.cpu()[:, :512].contiguous(), lo, pen, hist, None)


def test_penalty_pass_row_slot_map(gpu):
    """4 gathered rows of non-contiguous slots of a 16-slot state = the identity-mapped pass on those slots."""
    Bm, V, cap = 16, 1000, 48
    g = torch.Generator().manual_seed(9)
    pen, hist = _state(Bm, cap)
    slots = [11, 2, 7, 14]
    for k, s in enumerate(slots):
        _set(pen, hist, s, 0.4 + k, 0.1 * k, 1.0 + 0.25 * k, 5, torch.randint(0, V, (20 + 7 * k,), generator=g).tolist())
    rows = torch.randn(4, V, generator=g) * 3.0
    full = torch.randn(Bm, V, generator=g)
    full[slots] = rows
    dp, dh = pen.to(gpu), hist.to(gpu)
    mapped = rows.to(gpu)
    row_slot = torch.tensor(slots, dtype=torch.int32)
    ops.sample_penalties(mapped, None, dp, dh, row_slot.to(gpu), 0, V)
    ident = full.to(gpu)
    ops.sample_penalties(ident, None, dp, dh, None, 0, V)
    assert torch.equal(mapped.view(torch.int32), ident[slots].view(torch.int32))
    touched = _check(mapped.cpu(), rows, pen, hist, None, row_slot=row_slot)
    assert touched.any(dim=1).all()


def _pick_case():
    """5 greedy rows over V = 1000 logits with gaps of 1 (a permutation of 0 .. V-1); slot b's history names its top
    tokens so that the penalties move the argmax by a clear margin (never a tie)."""
    B, V, cap = 5, 1000, 32
    g = torch.Generator().manual_seed(3)
    x0 = torch.stack([torch.randperm(V, generator=g).float() for _ in range(B)])
    top = [int(x0[b].argmax()) for b in range(B)]
    pen, hist = _state(B, cap)
    _set(pen, hist, 0, 0.0, 0.0, 1.0, 0, [top[0]] * 4)              # unpenalised: keeps its argmax
    _set(pen, hist, 1, 2.5, 0.0, 1.0, 1, [5, top[1]])               # presence: 999 -> 996.5
    _set(pen, hist, 2, 0.0, 1.5, 1.0, 0, [top[2]] * 3)              # frequency: 999 -> 994.5
    _set(pen, hist, 3, 0.0, 0.0, 2.0, 1, [top[3]])                  # repetition on a prompt token: 999 -> 499.5
    _set(pen, hist, 4, 2.5, 0.0, 1.0, 0, [top[4]])                  # penalised but inactive
    active = torch.tensor([1, 1, 1, 1, 0], dtype=torch.int32)
    return B, V, x0, top, pen, hist, active


def test_pick_through_penalties_and_append(gpu):
    B, V, x0, top, pen, hist, active = _pick_case()
    want = x0.double().clone()
    ref.sample_penalties(want, active, pen, hist)
    want_ids = want.argmax(dim=1).tolist()
    srt = want.sort(dim=1, descending=True).values
    assert bool((srt[:, 0] - srt[:, 1] >= 0.5).all())  # the reference pick is unambiguous
    i32 = dict(dtype=torch.int32, device=gpu)
    logits, dp, dh, dact = x0.to(gpu), pen.to(gpu), hist.to(gpu), active.to(gpu)
    next_ids = torch.full((B,), -1, **i32)
    ring, counter, positions = torch.full((4, B), -1, **i32), torch.tensor([2], **i32), torch.full((B,), 10, **i32)
    cand = torch.zeros(B, 16, 2, device=gpu)
    ops.sample_penalties(logits, dact, dp, dh, None, 0, V)
    ops.sample_candidates(logits, torch.zeros(B, device=gpu), torch.zeros(B, **i32), torch.ones(B, device=gpu),
                          torch.zeros(B, 2, **i32), positions, dact, cand, 0)
    ops.sample_pick_hist(cand.unsqueeze(0), dact, next_ids, ring, counter, positions, dp, dh, vocab=V)
    got = next_ids.cpu().tolist()
    assert got[:4] == want_ids[:4] and got[4] == -1
    assert got[0] == top[0] and all(got[b] != top[b] for b in (1, 2, 3))  # the penalties moved the argmax
    assert ring.cpu()[2].tolist() == got and positions.cpu().tolist() == [11, 11, 11, 11, 10]
    after = dh.cpu()
    for b in (1, 2, 3):  # penalised and active: the pick joined the history
        n = int(hist[b, 0])
        assert int(after[b, 0]) == n + 1 and int(after[b, 1 + n]) == got[b]
        assert torch.equal(after[b, 1:1 + n], hist[b, 1:1 + n])
    for b in (0, 4):  # unpenalised / inactive: untouched
        assert torch.equal(after[b], hist[b])


def test_prefill_commit_appends_history(gpu):
    """The first-token commit with n = 2 of NS = 4 rows: slot 6 (penalised) gets its token appended, slot 1
    (unpenalised) does not, and the slots named by rows >= n are left alone."""
    NS, Bm, cap = 4, 8, 16
    pen, hist = _state(Bm, cap)
    _set(pen, hist, 6, 0.5, 0.0, 1.0, 3, [4, 5, 6])
    _set(pen, hist, 1, 0.0, 0.0, 1.0, 2, [8, 9])
    _set(pen, hist, 3, 0.0, 0.7, 1.0, 1, [2])  # named by row 2, which is past n
    i32 = dict(dtype=torch.int32, device=gpu)
    meta = torch.tensor([0, 1, 2, 3] + [6, 1, 3, 0] + [30, 40, 50, 0] + [2, 1], **i32)
    new_ids = torch.tensor([101, 102, 103, 104], **i32)
    ids, ring, positions = torch.zeros(Bm, **i32), torch.zeros(3, Bm, **i32), torch.zeros(Bm, **i32)
    dp, dh = pen.to(gpu), hist.to(gpu)
    ops.prefill_sample_commit_hist(meta, new_ids, ids, ring, positions, dp, dh)
    assert ids.cpu().tolist() == [0, 102, 0, 0, 0, 0, 101, 0]
    assert ring.cpu()[1].tolist() == [0, 102, 0, 0, 0, 0, 101, 0]
    assert positions.cpu().tolist() == [0, 41, 0, 0, 0, 0, 31, 0]
    after = dh.cpu()
    assert after[6, :5].tolist() == [4, 4, 5, 6, 101]
    for s in (0, 1, 2, 3, 4, 5, 7):
        assert torch.equal(after[s], hist[s])
    # the eager first-token path's append: rows -> slots
    ops.sample_hist_append(torch.tensor([7, 8], **i32), torch.tensor([6, 1], **i32), None, dp, dh)
    after = dh.cpu()
    assert after[6, :6].tolist() == [5, 4, 5, 6, 101, 7] and torch.equal(after[1], hist[1])


# ------------------------------------------------------------------------------------------------ runner
PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 170)), [7] * 33]
TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22]]
PENS = [(0.0, 0.0, 1.0), (2.0, 2.0, 1.0), (0.0, 0.0, 2.0)]  # slot 0 unpenalised, slot 1 p + f, slot 2 r
STEPS = 20


@pytest.fixture(scope="module")
def weights(gpu):
    return convert_standard(TINY, init_standard_weights(TINY, seed=1), device=gpu)


def _run(weights, gpu, graphs, pens=PENS, swap_at=None):
    """First token + STEPS greedy decode tokens of the three prompts (per sequence) and the runner."""
    r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=graphs)
    if graphs:
        r.capture([4])  # the prefill below then replays a captured graph: first tokens sampled inside it
    for i, bt in enumerate(TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
        r.presence[i], r.frequency[i], r.repetition[i] = pens[i]
        r.n_prompt[i] = len(PROMPTS[i])
        if pens[i] != (0.0, 0.0, 1.0):
            r.set_history(i, PROMPTS[i], len(PROMPTS[i]))
    r.prefill([PrefillSeq(i, p, 0, TABLES[i], True) for i, p in enumerate(PROMPTS)], ring_row=0)
    r.active[:3] = 1
    where = [0, 1, 2]  # slot of sequence i
    first = r.ids.cpu().tolist()
    toks = [[first[i]] for i in range(3)]
    for step in range(STEPS):
        if step == swap_at:  # slots 1 <-> 2: the device state through move_slots, the host-owned state by hand
            r.move_slots([1, 2], [2, 1])
            for t in (r.block_tables, r.presence, r.frequency, r.repetition, r.n_prompt):
                t[[1, 2]] = t[[2, 1]]
            where = [0, 2, 1]
        r.decode(4)
        row = r.ring.cpu()[step]
        for i in range(3):
            toks[i].append(int(row[where[i]]))
    torch.cuda.synchronize()
    return toks, r, where


@pytest.fixture(scope="module")
def eager_run(weights, gpu):
    return _run(weights, gpu, False)


def test_runner_graph_replay_equals_eager(weights, gpu, eager_run):
    toks, r, _ = _run(weights, gpu, True)
    # the first penalised slot captured the twins of every graph with the penalty pass; they were replayed
    assert r.graphs and r.pf_graphs and set(r.pen_graphs) == set(r.graphs) and set(r.pen_pf_graphs) == set(r.pf_graphs)
    assert {B: [c for c, _ in v] for B, v in r.pen_mx_graphs.items()} == \
        {B: [c for c, _ in v] for B, v in r.mx_graphs.items()}
    assert r._graph_set()[0] is r.pen_graphs
    assert toks == eager_run[0]


def test_runner_history_holds_prompt_and_drained_tokens(eager_run):
    toks, r, where = eager_run
    state = r.hist_state.cpu()
    for i in (1, 2):
        n = int(state[where[i], 0])
        assert n == len(PROMPTS[i]) + 1 + STEPS
        assert state[where[i], 1:1 + n].tolist() == PROMPTS[i] + toks[i]
    assert int(state[0, 0]) == 0  # the unpenalised slot keeps no history


def test_runner_unpenalised_slot_ignores_its_neighbours(weights, gpu, eager_run):
    plain, _, _ = _run(weights, gpu, False, pens=[(0.0, 0.0, 1.0)] * 3)
    assert plain[0] == eager_run[0][0]
    assert plain[1] != eager_run[0][1] or plain[2] != eager_run[0][2]  # the penalties do change a stream


def test_runner_streams_continue_across_a_slot_swap(weights, gpu, eager_run):
    toks, r, where = _run(weights, gpu, False, swap_at=STEPS // 2)
    assert toks == eager_run[0]
    state = r.hist_state.cpu()
    for i in (1, 2):
        n = int(state[where[i], 0])
        assert state[where[i], 1:1 + n].tolist() == PROMPTS[i] + toks[i]


def test_engine_first_penalised_request_arrives_mid_stream(weights, gpu):
    """Captured graphs, an unpenalised stream decoding when the first penalised request arrives: the graph twins with
    the penalty pass are captured then (nothing executes during a capture), the prompt rides in a mixed step, the
    running stream's tokens are unchanged and the penalised stream (p = 1e4) never repeats a token."""
    from distributed_sse_for_llm_response_amd.engine.engine import LLMEngine, SamplingParams

    def run(with_pen):
        r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=True)
        r.capture()
        e = LLMEngine(r, eos_id=-1, prefill_budget=256)
        out = {"a": [], "b": []}
        for step in range(400):
            if step == 0:
                e.add_request("a", PROMPTS[1], SamplingParams(temperature=0.0, max_tokens=30, ignore_eos=True))
            if step == 8:  # (unpenalised in the comparison run: the same mixed step, the same arithmetic for "a")
                e.add_request("b", PROMPTS[2], SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True,
                                                              presence_penalty=1e4 if with_pen else 0.0))
            for ev in e.step():
                if not ev.done:
                    out[ev.conversation_id].append(ev.token_id)
            if step > 8 and not e.has_work():
                break
        assert not e.has_work()
        return out, r

    plain, r0 = run(False)
    got, r1 = run(True)
    assert not r0.pen_graphs and set(r1.pen_graphs) == set(r1.graphs)
    assert len(plain["a"]) == 30 and got["a"] == plain["a"]
    assert len(got["b"]) == 16 and len(set(got["b"])) == 16
