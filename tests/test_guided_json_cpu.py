"""guided_json / response_format json_schema on the host: the schema lowering (guide.h schema_pattern) is sound and
covers the compact serialisation, refuses what it does not support by name, agrees with Python's re on ASCII, and the
reference ops walk narrow, wide, JSON-mode, off and inactive rows in one launch."""
import json
import random
import re

import numpy as np
import pytest
import torch

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd import runtime as rtmod
from distributed_sse_for_llm_response_amd.ops import reference as ref

import guided_json_common as gj
from guided_json_common import DEAD, FIXTURES

NEG = float("-inf")


def test_three_bounded_strings_need_the_wide_class():
    pattern, tab, acc = gj.compiled("three strings of 64")
    assert 512 < tab.shape[0] <= ops.GUIDE_WIDE_STATES and len(pattern) <= rtmod.load().GUIDE_PATTERN_BYTES
    with pytest.raises(ValueError, match="needs more than 512 DFA states"):
        rtmod.load().guide_compile("[a-z]{200}[a-z]{200}[a-z]{200}")  # (the narrow caps stay what they were)
    with pytest.raises(ValueError, match=r"unsupported escape \\x"):  # (and \x is the wide entry point's alone)
        rtmod.load().guide_compile(pattern)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_every_accepted_string_is_json_that_validates(name):
    schema = FIXTURES[name][0]
    _, tab, acc = gj.compiled(name)
    dist = gj.distance_to_accept(tab, acc)
    rng = random.Random(len(name) * 1009)
    seen = set()
    for _ in range(200):
        raw = gj.draw(tab, acc, dist, rng, turn=rng.choice((8, 48, 160)))
        seen.add(raw)
        text = raw.decode("utf-8")  # (strict: the string bodies are valid UTF-8)
        assert gj.valid(json.loads(text), schema), text
        assert not re.search(r"[\x00-\x1f]", text)
    assert len(seen) > 20


@pytest.mark.parametrize("name", list(FIXTURES))
def test_compact_instances_are_accepted_and_invalid_ones_rejected(name):
    schema, good, bad = FIXTURES[name]
    pattern, tab, acc = gj.compiled(name)
    for x in good:
        assert gj.valid(x, schema), x  # (the fixture itself)
        assert gj.accepts(tab, acc, gj.compact(x).encode("utf-8")), x
    for text in bad:
        assert not gj.accepts(tab, acc, text.encode("utf-8")), text
    # the lowered pattern means the same to Python's re on ASCII subjects
    for text in [gj.compact(x) for x in good] + bad:
        if text.isascii():
            assert bool(re.fullmatch(pattern, text)) == gj.accepts(tab, acc, text.encode()), text
    # every proper prefix of an accepted text keeps the DFA alive and is not accepted twice over
    raw = gj.compact(good[-1]).encode("utf-8")
    assert all(gj.walk(tab, raw[:k]) != DEAD for k in range(len(raw)))


@pytest.mark.parametrize("schema, names", gj.REFUSED)
def test_unsupported_schemas_are_refused_by_name(schema, names):
    with pytest.raises(ValueError) as e:
        gj.lower(schema)
    assert str(e.value).startswith("json schema: ") and names in str(e.value), str(e.value)


def test_limits_are_errors_that_name_the_cap():
    rt = rtmod.load()
    big = {"type": "string", "description": "d" * rt.GUIDE_SCHEMA_BYTES}
    with pytest.raises(ValueError, match="longer than 8192 bytes"):
        gj.lower(big)
    with pytest.raises(ValueError, match="malformed JSON"):
        gj.lower('{"type": "string",}')
    with pytest.raises(ValueError, match="must be an object"):
        gj.lower("true")
    five = {"type": "object", "required": list("abcde"),
            "properties": {k: {"type": "string", "maxLength": 64} for k in "abcde"}}
    with pytest.raises(ValueError, match="needs more than 4096 DFA states"):
        rt.guide_compile_wide(gj.lower(five))
    item = {"type": "object", "required": ["s"], "properties": {"s": {"type": "string"}}}
    for _ in range(6):  # (each level writes its item twice)
        item = {"type": "array", "items": item}
    with pytest.raises(ValueError, match=r"8192.*kGuidePatternBytes"):
        gj.lower(item)
    # the narrow entry point compiles what it did: same states, same table, and no minimisation
    assert rt.guide_compile("ad|bd")[0] == 4 and rt.guide_compile_wide("ad|bd")[0] == 3


def test_ignored_annotations_and_canonical_scalars():
    plain = gj.lower({"type": "integer"})
    assert plain == gj.lower({"type": "integer", "title": "t", "description": "d", "default": 1, "examples": [1],
                              "$schema": "s", "$id": "i"}) == "-?(?:0|[1-9][0-9]*)"
    tab, acc = gj.compile_wide(gj.lower({"enum": [1.0, 2.50, 1e3, "a.b", None, False]}))
    for text, want in [("1", True), ("1.0", False), ("2.5", True), ("1000", True), ('"a.b"', True), ('"aXb"', False),
                       ("null", True), ("false", True), ("true", False)]:
        assert gj.accepts(tab, acc, text.encode()) is want, text
    tab, acc = gj.compile_wide(gj.lower({"type": "string", "enum": ["a", 1, None]}))  # type and enum: both must hold
    assert gj.accepts(tab, acc, b'"a"') and not gj.accepts(tab, acc, b"1") and not gj.accepts(tab, acc, b"null")
    tab, acc = gj.compile_wide(gj.lower({"type": "string"}))
    for raw, want in [(b'"\\ud83d"', False), (b'"\\u00e9\\n\\/"', True), (b'"\xed\xa0\x80"', False), (b'"\xc0\x80"', False),
                      ('"日本"'.encode(), True), (b'"a\x01"', False), (b'"\\x"', False), (b'"\x7f"', True)]:
        assert gj.accepts(tab, acc, raw) is want, raw


# ------------------------------------------------------------------------------------------------ the reference ops
SLOTS = 8
ROW_SLOT = [7, 1, 4, 2, 6]  # rows: narrow | wide | JSON mode | guide off | inactive (a wide slot)


def _launch(wide: bool):
    (tb, tl), _ = gj.vocabulary()
    n, t, a = rtmod.load().guide_compile("[a-z ]*")
    gt = torch.full((1, ops.GUIDE_STATES, 256), -1, dtype=torch.int16)
    gf = torch.zeros(1, ops.GUIDE_STATES, dtype=torch.int32)
    gt[0, :n] = torch.from_numpy(np.frombuffer(t, dtype=np.uint16).reshape(n, 256).view(np.int16).copy())
    gf[0, :n] = torch.from_numpy(np.frombuffer(a, dtype=np.uint8).astype(np.int32))
    ops.guide_live(tb, tl, gt, gf, torch.zeros(2, dtype=torch.int32), 0, n, gj.EOS)
    _, wtab, wacc = gj.compiled("three strings of 64")
    wt = torch.full((2, ops.GUIDE_WIDE_STATES, 256), -1, dtype=torch.int16)
    wf = torch.zeros(2, ops.GUIDE_WIDE_STATES, dtype=torch.int32)
    wt[1, :wtab.shape[0]] = torch.from_numpy(wtab.view(np.int16).copy())
    wf[1, :wtab.shape[0]] = torch.from_numpy(wacc.astype(np.int32))
    state = gj.walk(wtab, b'{"a":"","b":"","c":"' + b"x" * 40)
    assert state >= ops.GUIDE_STATES
    meta = torch.zeros(2 * SLOTS, dtype=torch.int32)
    meta[:SLOTS] = -1
    meta[7], meta[1], meta[4], meta[6] = 0, ops.GUIDE_POOL + 1, ops.JSON_ENTRY, ops.GUIDE_POOL + 1
    meta[SLOTS + 1], meta[SLOTS + 6] = state, state
    js = torch.zeros(4 * SLOTS, dtype=torch.int32)
    js.view(4, -1)[:, 4] = torch.tensor(ops.json_state_words(ops.json_walk(b'{"k":"a')), dtype=torch.int32)
    ops.guide_attach_json(meta, torch.from_numpy(ops.json_table()[0].view(np.int16).copy()), js)
    if wide:
        ops.guide_attach_wide(meta, wt, wf)
        ops.guide_live(tb, tl, gt, gf, meta, ops.GUIDE_POOL + 1, wtab.shape[0], gj.EOS)
    return (tb, tl, gt, gf, meta), js, (wtab, wacc, state)


def test_reference_ops_mix_the_row_kinds_in_one_launch():
    (tb, tl, gt, gf, meta), js, (wtab, wacc, state) = _launch(True)
    (_, _, _, _, meta0), js0, _ = _launch(False)
    active = torch.tensor([1, 1, 1, 1, 0], dtype=torch.int32)
    row_slot = torch.tensor(ROW_SLOT, dtype=torch.int32)
    x0 = torch.randn(5, gj.VG, generator=torch.Generator().manual_seed(3)) * 4
    x, y = x0.clone(), x0.clone()
    ops.guide_mask(x, active, tb, tl, gt, gf, meta, row_slot, 0, gj.EOS)
    ops.guide_mask(y, active, tb, tl, gt, gf, meta0, row_slot, 0, gj.EOS)  # the wide arguments absent
    for row in (0, 2, 3, 4):  # the pre-existing kinds: what the functions give without the wide pool
        assert torch.equal(x[row].view(torch.int32), y[row].view(torch.int32))
    assert torch.equal(y[1], x0[1]) and torch.equal(x[3], x0[3]) and torch.equal(x[4], x0[4])
    (_, pieces) = gj.vocabulary()
    want = [i != gj.EOS and len(p) > 0 and i not in (0, gj.LEN0) and gj.walk(wtab, p, state) != DEAD
            for i, p in enumerate(pieces)]
    assert (x[1] != NEG).tolist() == want and any(want) and not all(want)
    assert torch.equal(x[1][x[1] != NEG], x0[1][x[1] != NEG])
    ids = torch.tensor([5, want.index(True), 9, 9, want.index(True)], dtype=torch.int32)
    ops.guide_advance(ids, active, tb, tl, gt, gf, meta, row_slot, gj.EOS)
    ops.guide_advance(ids, active, tb, tl, gt, gf, meta0, row_slot, gj.EOS)
    assert int(meta[SLOTS + 1]) == gj.walk(wtab, pieces[want.index(True)], state) != DEAD
    assert int(meta0[SLOTS + 1]) == state and int(meta[SLOTS + 6]) == state  # off without the pool; the inactive row
    assert int(meta[SLOTS + 7]) == int(meta0[SLOTS + 7]) and torch.equal(js, js0)
    for bad_state, bad_entry in ((ops.GUIDE_WIDE_STATES, ops.GUIDE_POOL + 1), (DEAD, ops.GUIDE_POOL + 1),
                                 (state, ops.GUIDE_POOL + 2), (state, ops.GUIDE_POOL + ops.GUIDE_WIDE_POOL)):
        meta[1], meta[SLOTS + 1] = bad_entry, bad_state
        z = x0.clone()
        ops.guide_mask(z, active, tb, tl, gt, gf, meta, row_slot, 0, gj.EOS)
        assert torch.equal(z[1], x0[1])  # out of range: dead, the row untouched


def test_engine_carries_the_schema_flag_over_the_tp_plan():
    from distributed_sse_for_llm_response_amd.engine.engine import SamplingParams
    from distributed_sse_for_llm_response_amd.serving.tp import Plan

    pattern = gj.compiled("flat")[0]
    p = Plan(step=True)
    p.adds.append((7, [1, 2, 3], SamplingParams(guide=pattern, guide_schema=True), 5))
    p.adds.append((8, [4], SamplingParams(guide="a+"), 6))
    q = Plan.decode(1, 2, 0, 0, p.encode())
    assert [(sp.guide, sp.guide_schema) for _, _, sp, _ in q.adds] == [(pattern, True), ("a+", False)]
