"""JSON mode on the GPU: the pushdown rows of the mask and advance kernels bit for bit against their CPU twins (whole
vocabulary and shards), the runner's captured decode against eager with an unguided neighbour and a slot move, and
the first token of a JSON stream at the captured-prefill, mixed-step and eager first-token sites."""
import numpy as np
import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd import runtime as rtmod
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights

import json_mode_common as jc
from json_mode_common import DEAD, EOS, NEG, VG, is_viable, oracle

pytestmark = pytest.mark.gpu
SLOTS = 8


@pytest.fixture(scope="module")
def pool(gpu):
    """The crafted vocabulary, one resident pattern ([a-z ]*, one state) and the JSON table, on the CPU and the GPU."""
    tb, tl = jc.vocabulary()
    n, tab, acc = rtmod.load().guide_compile("[a-z ]*")
    tab = np.frombuffer(tab, dtype=np.uint16).reshape(n, 256)
    gt = torch.full((1, ops.GUIDE_STATES, 256), -1, dtype=torch.int16)
    gf = torch.zeros(1, ops.GUIDE_STATES, dtype=torch.int32)
    gt[0, :n] = torch.from_numpy(tab.copy().view(np.int16))
    gf[0, :n] = torch.from_numpy(np.frombuffer(acc, dtype=np.uint8).astype(np.int32))
    ops.guide_live(tb, tl, gt, gf, None, 0, n, EOS)
    cpu = (tb, tl, gt, gf, jc.json_tab_tensor())
    return cpu, tuple(t.to(gpu) for t in cpu)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# the two JSON rows of a launch
PAIRS = [("start", "key string"), ("value string after a backslash", "mid \\u, 2 digits seen"),
         ("mid a 3-byte character", "number in an array"), ("number in an object", "after a value, stack obj obj"),
         ("after a value, stack obj arr", "depth 64"), ("depth 1 before the closing brace", "done"), ("dead", "nul"),
         ("dot", "nul")]
# rows 0..4 -> slots: inactive (a JSON slot) | unguided | regex-guided | JSON a | JSON b
ROW_SLOT = [6, 2, 7, 0, 5]


@pytest.mark.parametrize("V, offset", [(VG, 0), (1000, 1000), (1000, 0)])
@pytest.mark.parametrize("a, b", PAIRS)
def test_mask_and_advance_match_the_twin_bit_for_bit(pool, gpu, a, b, V, offset):
    (tb, tl, gt, gf, jt), (dtb, dtl, dgt, dgf, djt) = pool
    st = jc.states()
    meta = torch.zeros(2 * SLOTS, dtype=torch.int32)
    meta[:SLOTS] = -1
    meta[6], meta[0], meta[5] = ops.JSON_ENTRY, ops.JSON_ENTRY, ops.JSON_ENTRY
    meta[7], meta[SLOTS + 7] = 0, 0
    meta[SLOTS + 0], meta[SLOTS + 5] = 123, DEAD  # (the state word of a JSON slot means nothing)
    js = jc.json_state_tensor(SLOTS, {6: st["key string"], 0: st[a], 5: st[b]})
    row_slot = torch.tensor(ROW_SLOT, dtype=torch.int32)
    active = torch.tensor([0, 1, 1, 1, 1], dtype=torch.int32)
    g = torch.Generator().manual_seed(len(a) * 31 + len(b))
    x0 = (torch.randn(5, V + 3, generator=g) * 4)[:, :V]  # (a row stride above V)
    e = EOS - offset
    if 0 <= e < V:
        x0[:, e] = NEG  # EOS banned, as by min_tokens
    x, dx = x0.clone(), x0.clone().to(gpu)
    dmeta, djs = meta.clone().to(gpu), js.clone().to(gpu)
    ops.guide_attach_json(meta, jt, js)
    ops.guide_attach_json(dmeta, djt, djs)
    dev = (active.to(gpu), dtb, dtl, dgt, dgf, dmeta, row_slot.to(gpu))
    ops.guide_mask(x, active, tb, tl, gt, gf, meta, row_slot, offset, EOS)
    ops.guide_mask(dx, *dev, offset, EOS)
    got = dx.cpu()
    assert _same_bits(got[:2], x0[:2])                    # the inactive and the unguided row
    assert torch.equal(got == NEG, x == NEG)              # the -inf set, row by row
    assert _same_bits(got, x)                             # and every column
    keep = x != NEG
    if 0 <= e < V:
        keep[:, e] = False
    assert _same_bits(got[keep], x0[keep])                # kept columns keep their bits
    assert not _same_bits(got[2], x0[2])                  # (the regex row was masked too)
    for row, name in ((3, a), (4, b)):
        if name == "dead":
            assert _same_bits(got[row], x0[row])
            continue
        alive = ops.json_walk_all(st[name], tb.numpy(), tl.numpy())[0] != DEAD  # over the global vocabulary
        alive[EOS] = False
        kept = got[row] != NEG
        if 0 <= e < V:
            kept[e] = False
        assert torch.equal(kept, torch.from_numpy(alive[offset:offset + V]))
        if 0 <= e < V:  # stuck iff nothing survives anywhere in the global vocabulary
            assert got[row, e] == (NEG if alive.any() else 0.0), name
            if name == "nul" and offset == 0 and V < VG:
                assert (got[row] == NEG).all()            # its one survivor is in the other shard: not stuck
            if name == "done":
                assert (got[row] == NEG).sum() == V - 1
    assert torch.equal(dmeta.cpu(), meta) and torch.equal(djs.cpu(), js)  # the mask writes no state
    # advance: each JSON row commits its first surviving token of the global vocabulary (EOS where none), then "}}"
    ids = []
    for name in ("key string", None, None, a, b):
        if name is None:
            ids.append(jc.token_id(tb, tl, b"a"))
            continue
        alive = ops.json_walk_all(st[name], tb.numpy(), tl.numpy())[0] != DEAD
        alive[EOS] = False
        ids.append(int(np.argmax(alive)) if alive.any() else EOS)
    for step_ids in (ids, [jc.token_id(tb, tl, b"}}")] * 5, [jc.LEN0, jc.LEN33, 3, jc.LEN33, jc.LEN0]):
        t = torch.tensor(step_ids, dtype=torch.int32)
        ops.guide_advance(t, active, tb, tl, gt, gf, meta, row_slot, EOS)
        ops.guide_advance(t.to(gpu), *dev, EOS)
        assert torch.equal(djs.cpu(), js) and torch.equal(dmeta.cpu(), meta)
    assert meta[:SLOTS].tolist() == [ops.JSON_ENTRY, -1, -1, -1, -1, ops.JSON_ENTRY, ops.JSON_ENTRY, 0]
    assert meta[SLOTS + 0] == 123 and meta[SLOTS + 5] == DEAD and meta[SLOTS + 7] == DEAD  # only the DFA row's word moved
    assert js.view(4, -1)[:, 6].tolist() == ops.json_state_words(st["key string"])       # the inactive row's slot
    assert js.view(4, -1)[0, 0] == DEAD and js.view(4, -1)[0, 5] == DEAD                    # a token of length 0 kills


def test_json_slots_without_the_json_tensors_are_guide_off(pool, gpu):
    _, (dtb, dtl, dgt, dgf, _) = pool
    meta = torch.tensor([ops.JSON_ENTRY, -1, 0, 0], device=gpu, dtype=torch.int32)
    x = torch.randn(2, VG)
    dx = x.clone().to(gpu)
    ops.guide_mask(dx, None, dtb, dtl, dgt, dgf, meta, None, 0, EOS)
    ops.guide_advance(torch.tensor([5, 5], device=gpu, dtype=torch.int32), None, dtb, dtl, dgt, dgf, meta, None, EOS)
    assert _same_bits(dx.cpu(), x) and meta.tolist() == [ops.JSON_ENTRY, -1, 0, 0]


# ------------------------------------------------------------------------------------------------ the runner
PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 150)), [11] * 20, [7, 9, 400, 1200]]
TABLES = [[0, 1, 2], [10, 4, 5, 6], [20, 21, 22], [30, 31]]
STEPS = 23  # 24 tokens with the first
PIECES = jc.json_pieces(TINY.vocab_size)


@pytest.fixture(scope="module")
def weights(gpu):
    return convert_standard(TINY, init_standard_weights(TINY, seed=1), device=gpu)


def _text(ids):
    return "".join(PIECES[t] for t in ids if t != EOS).encode("utf-8")


def _run(weights, gpu, graphs, json_slots=(1, 3), swap_at=None):
    r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=graphs)
    r.set_guide_vocab(PIECES, EOS)
    if graphs:
        r.capture([4])
    for i, bt in enumerate(TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
    before = (r.guide_used, r.json_state, r._graph_set()[0] is r.graphs)
    if json_slots:
        r.enable_guides()
        for slot in json_slots:
            r.set_guide(slot, ops.JSON_ENTRY, ops.JSON_START_STATE)
    r.temperature[:] = torch.tensor([0.0, 1.0, 0.8, 0.0])
    r.seeds[:] = torch.arange(8, dtype=torch.int32).view(4, 2) + 11
    r.prefill([PrefillSeq(i, p, 0, TABLES[i], True) for i, p in enumerate(PROMPTS)], ring_row=0)
    r.active[:4] = 1
    where = [0, 1, 2, 3]
    first = r.ids.cpu().tolist()
    toks = [[first[i]] for i in range(4)]
    for step in range(STEPS):
        if step == swap_at:  # slots 1 <-> 2: the device state through move_slots, the host-owned state by hand
            r.move_slots([1, 2], [2, 1])
            for t in (r.block_tables, r.temperature, r.seeds):
                t[[1, 2]] = t[[2, 1]]
            where = [0, 2, 1, 3]
        r.decode(4)
        row = r.ring.cpu()[step]
        for i in range(4):
            toks[i].append(int(row[where[i]]))
    torch.cuda.synchronize()
    return toks, r, before


def test_captured_decode_equals_eager_and_unused_costs_nothing(weights, gpu):
    plain, r0, _ = _run(weights, gpu, True, json_slots=())  # no JSON request: the startup graphs, nothing allocated
    assert not r0.guide_used and r0.json_state is None and r0.json_tab is None and r0._graph_set()[0] is r0.graphs
    assert not any(any(t) for t in r0._twins.values())
    eager, _, _ = _run(weights, gpu, False)
    toks, r, before = _run(weights, gpu, True)
    assert before == (False, None, True)  # (also in this runner, until enable_guides)
    key = (False, False, False, True)
    assert r._twin_key() == key and r._graph_set()[0] is r._twins[key][0] and set(r._twins[key][0]) == set(r.graphs)
    assert set(r._twins[key][1]) == set(r.pf_graphs) and r.json_state.numel() == 4 * r.max_batch
    assert toks == eager
    assert toks[0] == plain[0] and toks[2] == plain[2] and toks[1] != plain[1] and toks[3] != plain[3]
    for i in (1, 3):
        cut = toks[i][:toks[i].index(EOS)] if EOS in toks[i] else toks[i]
        text = _text(cut)
        assert text.startswith(b"{") and (oracle(text) if EOS in toks[i] else is_viable(text)), text
        # the device's state words are the host walk over the tokens it committed
        want = ops.json_walk_ids(ops.JSON_START_STATE, toks[i], *r.guide_host, EOS)
        assert r.json_state.view(4, -1)[:, i].cpu().tolist() == ops.json_state_words(want)
    moved, rm, _ = _run(weights, gpu, False, swap_at=STEPS // 2)
    assert moved == eager  # the stream continues in its new slot: json_state travelled with guide_meta
    assert rm.guide_meta[:4].cpu().tolist() == [-1, -1, ops.JSON_ENTRY, ops.JSON_ENTRY]


LATE = (list(range(40, 77)), [40, 41, 42])  # a prompt absorbed by a mixed step (slot 3)


@pytest.mark.parametrize("graphs", [True, False])
def test_first_token_sites_open_the_object(weights, gpu, graphs):
    """Slot 1's first token comes out of the prefill pass (the captured prefill graph, or the eager first-token site),
    slot 3's out of a mixed step (captured or eager): both must start with '{', and the decode steps go on from the
    state the first token left."""
    r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=graphs)
    r.set_guide_vocab(PIECES, EOS)
    if graphs:
        r.capture([4])
        assert r.graphs and r.pf_graphs and r.mx_graphs
    for i, bt in enumerate(TABLES[:3] + [LATE[1]]):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
    r.enable_guides()
    r.set_guide(1, ops.JSON_ENTRY, ops.JSON_START_STATE)
    r.set_guide(3, ops.JSON_ENTRY, ops.JSON_START_STATE)
    r.temperature[:] = torch.tensor([0.0, 1.0, 0.8, 1.0])
    r.seeds[:] = torch.arange(8, dtype=torch.int32).view(4, 2) + 3
    r.prefill([PrefillSeq(i, p, 0, TABLES[i], True) for i, p in enumerate(PROMPTS[:3])], ring_row=0)
    r.active[:3] = 1
    toks = {1: [int(r.ids[1])], 3: []}
    for step in range(6):
        if step == 2:
            r.mixed(4, [PrefillSeq(3, LATE[0], 0, LATE[1], True)], ring_row=int(r.ring_counter[0]))
            r.active[3] = 1
            toks[3].append(int(r.ids[3]))
        else:
            r.decode(4)
            if step > 2:
                toks[3].append(int(r.ids[3]))
        toks[1].append(int(r.ids[1]))
    torch.cuda.synchronize()
    for slot, ids in toks.items():
        assert PIECES[ids[0]].startswith("{"), (slot, PIECES[ids[0]])
        cut = ids[:ids.index(EOS)] if EOS in ids else ids
        assert is_viable(_text(cut)), _text(cut)
        want = ops.json_walk_ids(ops.JSON_START_STATE, ids, *r.guide_host, EOS)
        assert r.json_state.view(4, -1)[:, slot].cpu().tolist() == ops.json_state_words(want)
