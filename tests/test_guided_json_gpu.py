"""Schema guides on the device: the guide kernels walk a wide-pool row bit for bit like the CPU reference in a launch
that also holds narrow, JSON-mode, off and inactive rows (whole vocabulary and a 2-shard split), guide_live marks a
table of more than 512 states, and the tiny model decodes under a schema through the captured graph."""
import json

import numpy as np
import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd import runtime as rtmod
from distributed_sse_for_llm_response_amd.engine.model_runner import ModelRunner, PrefillSeq
from distributed_sse_for_llm_response_amd.engine.weights import convert_standard
from distributed_sse_for_llm_response_amd.models.mistral import TINY, init_standard_weights

import guided_json_common as gj
import json_mode_common as jc
from guided_json_common import DEAD, EOS, VG

pytestmark = pytest.mark.gpu
NEG = float("-inf")
SLOTS = 8
WIDE = ops.GUIDE_POOL  # the first wide entry word
ROW_SLOT = [7, 1, 4, 2, 6]  # rows: narrow | wide | JSON mode | guide off | inactive (a wide slot)


@pytest.fixture(scope="module")
def pool(gpu):
    """The 512-piece vocabulary; narrow entry 0 = [a-z ]*; wide entry 0 = integer or null (small, with a stuck state
    after "nu": no piece holds an 'l'), wide entry 1 = the three strings of 64 (more than 512 states); JSON's table.
    The flags come from the reference's live pass."""
    (tb, tl), pieces = gj.vocabulary()
    n, t, a = rtmod.load().guide_compile("[a-z ]*")
    gt = torch.full((1, ops.GUIDE_STATES, 256), -1, dtype=torch.int16)
    gf = torch.zeros(1, ops.GUIDE_STATES, dtype=torch.int32)
    gt[0, :n] = torch.from_numpy(np.frombuffer(t, dtype=np.uint16).reshape(n, 256).view(np.int16).copy())
    gf[0, :n] = torch.from_numpy(np.frombuffer(a, dtype=np.uint8).astype(np.int32))
    wt = torch.full((2, ops.GUIDE_WIDE_STATES, 256), -1, dtype=torch.int16)
    wf = torch.zeros(2, ops.GUIDE_WIDE_STATES, dtype=torch.int32)
    small = gj.compile_wide(gj.lower({"type": ["integer", "null"]}))
    big = gj.compiled("three strings of 64")[1:]
    for e, (tab, acc) in enumerate((small, big)):
        wt[e, :tab.shape[0]] = torch.from_numpy(tab.view(np.int16).copy())
        wf[e, :tab.shape[0]] = torch.from_numpy(acc.astype(np.int32))
    meta = ops.guide_attach_wide(torch.zeros(2, dtype=torch.int32), wt, wf)
    ops.guide_live(tb, tl, gt, gf, meta, 0, n, EOS)
    accept_only = wf.clone()
    for e, (tab, _) in enumerate((small, big)):
        ops.guide_live(tb, tl, gt, gf, meta, WIDE + e, tab.shape[0], EOS)
    cpu = (tb, tl, gt, gf, wt, wf, jc.json_tab_tensor())
    return cpu, tuple(x.to(gpu) for x in cpu), (small, big, pieces, accept_only)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_live_kernel_marks_a_wide_entry_like_the_reference(pool, gpu):
    (tb, tl, gt, gf, wt, wf, _), (dtb, dtl, dgt, dgf, dwt, _, _), (small, big, _, accept_only) = pool
    n = big[0].shape[0]
    assert n > ops.GUIDE_STATES
    dwf = accept_only.clone().to(gpu)
    dwf[1, n:] = 5  # (states past the used ones are not the kernel's to write)
    dmeta = ops.guide_attach_wide(torch.zeros(2, device=gpu, dtype=torch.int32), dwt, dwf)
    narrow = dgf.clone()
    ops.guide_live(dtb, dtl, dgt, narrow, dmeta, WIDE + 1, n, EOS)
    ops.guide_live(dtb, dtl, dgt, narrow, dmeta, WIDE + 0, small[0].shape[0], EOS)
    got = dwf.cpu()
    assert torch.equal(got[1, :n], wf[1, :n]) and (got[1, n:] == 5).all() and torch.equal(got[0], wf[0])
    assert torch.equal(narrow.cpu(), gf)  # the narrow flags are another pool's
    stuck = (wf[1, :n] & 2) != 0
    assert stuck.any() and not stuck.all() and int(wf[0, gj.walk(small[0], b"nu")]) == 2  # stuck, not accepting


def _states(small, big):
    deep = gj.walk(big[0], b'{"a":"","b":"\\u00e9","c":"' + b"x" * 62)
    assert deep >= ops.GUIDE_STATES
    return {"deep in the third string": (1, deep), "the highest used state": (1, big[0].shape[0] - 1),
            "mid a 3-byte character": (1, gj.walk(big[0], '{"a":"日'.encode()[:-1])),
            "after a backslash": (1, gj.walk(big[0], b'{"a":"x","b":"\\')),
            "string at its bound": (1, gj.walk(big[0], b'{"a":"' + b"x" * 64)),
            "accepting and stuck": (1, gj.walk(big[0], b'{"a":"","b":"","c":""}')),
            "start": (1, 0), "accepting, not stuck": (0, gj.walk(small[0], b"-12")),
            "stuck, not accepting": (0, gj.walk(small[0], b"nu")),
            "state out of range": (1, ops.GUIDE_WIDE_STATES), "dead": (1, DEAD),
            "entry out of range": (2, 3), "entry past the wide class": (ops.GUIDE_WIDE_POOL, 0)}


CASES = ["deep in the third string", "the highest used state", "mid a 3-byte character", "after a backslash",
         "string at its bound", "accepting and stuck", "start", "accepting, not stuck", "stuck, not accepting",
         "state out of range", "dead", "entry out of range", "entry past the wide class"]


@pytest.mark.parametrize("V, offset", [(VG, 0), (256, 0), (256, 256)])
@pytest.mark.parametrize("case", CASES)
def test_mask_and_advance_match_the_reference_bit_for_bit(pool, gpu, case, V, offset):
    (tb, tl, gt, gf, wt, wf, jt), (dtb, dtl, dgt, dgf, dwt, dwf, djt), (small, big, pieces, _) = pool
    entry, state = _states(small, big)[case]
    tab = (small, big)[entry][0] if entry < 2 else None
    meta = torch.zeros(2 * SLOTS, dtype=torch.int32)
    meta[:SLOTS] = -1
    meta[7], meta[1], meta[4], meta[6] = 0, WIDE + entry, ops.JSON_ENTRY, WIDE + 1
    meta[SLOTS + 1], meta[SLOTS + 6] = state, 600
    js = jc.json_state_tensor(SLOTS, {4: ops.json_walk(b'{"k":"a')})
    row_slot = torch.tensor(ROW_SLOT, dtype=torch.int32)
    active = torch.tensor([1, 1, 1, 1, 0], dtype=torch.int32)
    g = torch.Generator().manual_seed(len(case) * 7 + offset)
    x0 = (torch.randn(5, V + 3, generator=g) * 4)[:, :V]  # (a row stride above V)
    e = EOS - offset
    if 0 <= e < V:
        x0[:, e] = NEG  # EOS banned, as by min_tokens
    x, y, dx, dy = x0.clone(), x0.clone(), x0.clone().to(gpu), x0.clone().to(gpu)
    dmeta, djs, meta0, js0 = meta.clone().to(gpu), js.clone().to(gpu), meta.clone(), js.clone()
    dmeta0, djs0 = meta.clone().to(gpu), js.clone().to(gpu)
    ops.guide_attach_wide(ops.guide_attach_json(meta, jt, js), wt, wf)
    ops.guide_attach_wide(ops.guide_attach_json(dmeta, djt, djs), dwt, dwf)
    ops.guide_attach_json(meta0, jt, js0)     # the same launch without the wide pool: today's behaviour
    ops.guide_attach_json(dmeta0, djt, djs0)
    dev = (active.to(gpu), dtb, dtl, dgt, dgf)
    ops.guide_mask(x, active, tb, tl, gt, gf, meta, row_slot, offset, EOS)
    ops.guide_mask(y, active, tb, tl, gt, gf, meta0, row_slot, offset, EOS)
    ops.guide_mask(dx, *dev, dmeta, row_slot.to(gpu), offset, EOS)
    ops.guide_mask(dy, *dev, dmeta0, row_slot.to(gpu), offset, EOS)
    got, got0 = dx.cpu(), dy.cpu()
    assert _same_bits(got, x) and _same_bits(got0, y)
    for row in (0, 2, 3, 4):  # the narrow, JSON, off and inactive rows do not see the wide pool
        assert _same_bits(got[row], got0[row])
    assert _same_bits(got0[1], x0[1]) and _same_bits(got[3], x0[3]) and _same_bits(got[4], x0[4])
    assert not _same_bits(got[0], x0[0]) and not _same_bits(got[2], x0[2])
    keep = got[1] != NEG
    if tab is None or not 0 <= state < ops.GUIDE_WIDE_STATES:
        assert _same_bits(got[1], x0[1])  # dead: the row untouched
    else:
        want = torch.tensor([i != EOS and 0 < len(p) and i not in (0, gj.LEN0) and gj.walk(tab, p, state) != DEAD
                             for i, p in enumerate(pieces)])
        flags = int(wf[entry, state])
        stuck, accepting = not bool(want.any()), bool((small, big)[entry][1][state])
        assert flags == (1 if accepting else 0) | (2 if stuck else 0)
        if 0 <= e < V:
            assert got[1, e] == (0.0 if stuck else x0[1, e] if accepting else NEG)
            keep[e] = False
        assert torch.equal(keep, want[offset:offset + V])
        assert _same_bits(got[1][keep], x0[1][keep])
    assert torch.equal(dmeta.cpu(), meta) and torch.equal(djs.cpu(), js)  # the mask writes no state
    # advance: a surviving token, EOS (unchanged), a token that dies, a zero-length piece
    alive = [i for i, p in enumerate(pieces) if tab is not None and state < tab.shape[0] and p and i not in (0, gj.LEN0)
             and gj.walk(tab, p, state) != DEAD]
    dies = next(i for i, p in enumerate(pieces) if p[:1] == b"\x01")
    for wide_id in ([alive[len(alive) // 2]] if alive else []) + [EOS, dies, gj.LEN0]:
        before = int(meta[SLOTS + 1])
        ids = torch.tensor([jc.token_id(tb, tl, b"a"), wide_id, jc.token_id(tb, tl, b'"'), 9, wide_id], dtype=torch.int32)
        for m, dm in ((meta, dmeta), (meta0, dmeta0)):
            ops.guide_advance(ids, active, tb, tl, gt, gf, m, row_slot, EOS)
            ops.guide_advance(ids.to(gpu), *dev, dm, row_slot.to(gpu), EOS)
        assert torch.equal(dmeta.cpu(), meta) and torch.equal(djs.cpu(), js)
        assert torch.equal(dmeta0.cpu(), meta0) and torch.equal(djs0.cpu(), js0)
        after = int(meta[SLOTS + 1])
        if tab is None:
            assert after == before
        elif wide_id == EOS:
            assert after == before
        elif wide_id in (dies, gj.LEN0) or not 0 <= before < ops.GUIDE_WIDE_STATES:
            assert after == DEAD
        else:
            assert after == gj.walk(tab, pieces[wide_id], before) != DEAD
        assert int(meta[SLOTS + 6]) == 600 and int(meta0[SLOTS + 1]) == state  # inactive; off without the pool
        assert torch.equal(meta0[SLOTS + 7], meta[SLOTS + 7]) and torch.equal(js0, js)


# ------------------------------------------------------------------------------------------------ the runner
PROMPTS = [[5, 17, 99, 3, 8, 1000, 42], list(range(100, 150)), [11] * 20, [7, 9, 400, 1200]]
TABLES = [[0, 1, 2, 3], [10, 4, 5, 6], [20, 21, 22], [30, 31, 32]]
STEPS = 39  # 40 tokens with the first
PIECES = jc.json_pieces(TINY.vocab_size)
# (keys the pieces can spell)
SCHEMA = {"type": "object", "required": ["a", "b", "name"], "additionalProperties": False,
          "properties": {"a": {"type": "string", "maxLength": 64}, "b": {"type": "string", "maxLength": 64},
                         "name": {"type": "string", "maxLength": 64}, "id": {"type": "integer"}}}


@pytest.fixture(scope="module")
def weights(gpu):
    return convert_standard(TINY, init_standard_weights(TINY, seed=1), device=gpu)


@pytest.fixture(scope="module")
def dfa():
    tab, acc = gj.compile_wide(gj.lower(SCHEMA))
    assert tab.shape[0] > ops.GUIDE_STATES
    return tab, acc


def _text(ids):
    return "".join(PIECES[t] for t in ids if t != jc.EOS).encode("utf-8")


def _run(weights, gpu, dfa, graphs, slots=(1, 3), resume=None):
    """Slots 1 (seeded) and 3 (greedy) decode under SCHEMA.  resume = (k, tokens): slot 3 is a sequence preempted
    after k tokens and prefilled again with them, its state the host walk over what it has published."""
    r = ModelRunner(weights, num_blocks=64, max_batch=4, max_model_len=512, device=gpu, use_graphs=graphs)
    r.set_guide_vocab(PIECES, jc.EOS)
    if graphs:
        r.capture([4])
    for i, bt in enumerate(TABLES):
        r.block_tables[i, :len(bt)] = torch.tensor(bt, dtype=torch.int32)
    before = (r.guide_tab_wide, r._graph_set()[0] is r.graphs)
    prompts = list(PROMPTS)
    if slots:
        r.enable_guides()  # (a narrow guide was seen first: the wide pool then arrives with twins already captured)
        narrow_twin = r._graph_set()[0]
        r.upload_guide(WIDE + 2, *dfa)
        assert not graphs or (r._graph_set()[0] is narrow_twin and set(narrow_twin) == set(r.graphs))
        for slot in slots:
            r.set_guide(slot, WIDE + 2, 0)
        if resume:
            k, toks = resume
            prompts[3] = PROMPTS[3] + toks[:k]
            r.set_guide(3, WIDE + 2, ops.guide_walk(dfa[0], 0, toks[:k], *r.guide_host, jc.EOS, ops.GUIDE_WIDE_STATES))
    r.temperature[:] = torch.tensor([0.0, 1.0, 0.8, 0.0])
    r.seeds[:] = torch.arange(8, dtype=torch.int32).view(4, 2) + 11
    r.prefill([PrefillSeq(i, p, 0, TABLES[i], True) for i, p in enumerate(prompts)], ring_row=0)
    r.active[:4] = 1
    first = r.ids.cpu().tolist()
    toks = [[first[i]] for i in range(4)]
    for step in range(STEPS):
        r.decode(4)
        row = r.ring.cpu()[step]
        for i in range(4):
            toks[i].append(int(row[i]))
    torch.cuda.synchronize()
    return toks, r, before


def test_schema_guide_through_the_captured_graph(weights, gpu, dfa):
    tab, acc = dfa
    plain, r0, _ = _run(weights, gpu, dfa, True, slots=())
    assert r0.guide_tab_wide is None and not r0.guide_used and r0._graph_set()[0] is r0.graphs  # unused: nothing
    eager, _, _ = _run(weights, gpu, dfa, False)
    toks, r, before = _run(weights, gpu, dfa, True)
    assert before == (None, True) and tuple(r.guide_tab_wide.shape) == (ops.GUIDE_WIDE_POOL, ops.GUIDE_WIDE_STATES, 256)
    assert r._twin_key() == (False, False, False, True)  # the same pass set: no new graph variant
    assert toks == eager
    assert toks[0] == plain[0] and toks[2] == plain[2] and toks[1] != plain[1] and toks[3] != plain[3]
    for i in (1, 3):
        ended = jc.EOS in toks[i]
        cut = toks[i][:toks[i].index(jc.EOS)] if ended else toks[i]
        text = _text(cut)
        assert text.startswith(b'{"a":"') and all(gj.walk(tab, _text(cut[:k])) != DEAD for k in range(len(cut) + 1)), text
        if ended:
            assert gj.accepts(tab, acc, text) and gj.valid(json.loads(text.decode("utf-8")), SCHEMA), text
        # the device's state is the host walk over the tokens it committed
        want = ops.guide_walk(tab, 0, toks[i], *r.guide_host, jc.EOS, ops.GUIDE_WIDE_STATES)
        assert r.guide_meta.view(2, -1)[:, i].cpu().tolist() == [WIDE + 2, want]
    # preempted after 9 tokens, mid-object, and prefilled again with them: the stream resumes in the state of what
    # it has published (from any other state, the start included, its next tokens would kill the walk below)
    k = 9
    assert gj.walk(tab, _text(eager[3][:k])) not in (0, DEAD) and jc.EOS not in eager[3][:k]
    again, ra, _ = _run(weights, gpu, dfa, False, resume=(k, eager[3]))
    whole = eager[3][:k] + again[3]
    cut = whole[:whole.index(jc.EOS)] if jc.EOS in whole else whole
    assert all(gj.walk(tab, _text(cut[:j])) != DEAD for j in range(len(cut) + 1)), _text(cut)
    assert jc.EOS not in whole or gj.accepts(tab, acc, _text(cut))
    want = ops.guide_walk(tab, 0, whole, *ra.guide_host, jc.EOS, ops.GUIDE_WIDE_STATES)
    assert ra.guide_meta.view(2, -1)[:, 3].cpu().tolist() == [WIDE + 2, want] and want != DEAD
