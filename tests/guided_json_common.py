"""Shared by the guided_json tests: the fixture schemas with hand-written valid and invalid instances, a validator for
the supported subset (used when the jsonschema package does not import), host walkers of a compiled DFA and the
512-piece vocabulary of the kernel tests."""
import json
import random

import numpy as np

from distributed_sse_for_llm_response_amd import ops
from distributed_sse_for_llm_response_amd import runtime as rtmod

DEAD = ops.GUIDE_DEAD
S64 = "x" * 64
U64 = "é日😀" + "y" * 61  # 64 code points, 70 bytes

_PT = {"type": "object", "properties": {"x": {"type": "integer"}, "y": {"type": "integer"}}, "required": ["x", "y"]}

# name -> (schema, valid instances, invalid texts)
FIXTURES = {
    "flat": (
        {"type": "object", "additionalProperties": False, "required": ["name", "age", "ok"],
         "properties": {"name": {"type": "string", "maxLength": 8}, "age": {"type": "integer"}, "ok": {"type": "boolean"}}},
        [{"name": "ann", "age": 7, "ok": True}, {"name": "", "age": -12, "ok": False},
         {"name": "12345678", "age": 0, "ok": True}, {"name": "é日😀\"\\\n", "age": 10, "ok": False}],
        ['{"name":"ann","ok":true}', '{"name":"ann","age":7,"ok":true,"z":1}', '{"name":"ann","age":"7","ok":true}',
         '{"name":"123456789","age":7,"ok":true}', '{"name":"ann","age":07,"ok":true}',
         '{"name":"ann", "age":7,"ok":true}', '{"name":"ann","age":7,"ok":true} ', '{"age":7,"name":"ann","ok":true}',
         '{"name":"ann","age":7.5,"ok":true}', '{"name":"ann","age":-,"ok":true}']),
    "nested": (
        {"type": "object", "required": ["id", "pos"],
         "properties": {"id": {"type": "integer"},
                        "pos": {"type": "object", "required": ["x", "y"],
                                "properties": {"x": {"type": "number"}, "y": {"type": "number"}}}}},
        [{"id": 1, "pos": {"x": 0.5, "y": -2}}, {"id": 0, "pos": {"x": 1e-07, "y": 100}}],
        ['{"id":1,"pos":{"x":0.5}}', '{"id":1,"pos":{"x":0.5,"y":1,"z":2}}', '{"id":1,"pos":[0.5,1]}',
         '{"id":1,"pos":{"x":00.5,"y":1}}', '{"id":1,"pos":{"x":.5,"y":1}}', '{"id":1,"pos":{ "x":0.5,"y":1}}']),
    "optional": (
        {"type": "object", "required": ["b"],
         "properties": {"a": {"type": "string", "maxLength": 4}, "b": {"type": "integer"}, "c": {"type": "boolean"},
                        "d": {"type": "null"}}},
        [{"b": 1}, {"a": "xy", "b": 1}, {"b": 1, "d": None}, {"a": "abcd", "b": 2, "c": True, "d": None},
         {"b": 3, "c": False}],
        ['{}', '{"a":"xy"}', '{"b":1,}', '{"b":1,"a":"xy"}', '{"a":"abcde","b":1}', '{"b":1,"c":null}', '{,"b":1}']),
    "all optional": (
        {"type": "object", "properties": {"p": {"type": "integer"}, "q": {"type": "integer"}, "r": {"type": "integer"}}},
        [{}, {"p": 1}, {"q": 2}, {"r": 3}, {"p": 1, "r": 3}, {"p": 1, "q": 2, "r": 3}],
        ['{,}', '{"q":2,"p":1}', '{"p":1,,"r":3}', '{"p":1 }', '{"s":1}']),
    "enums": (
        {"type": "object", "required": ["color", "level"],
         "properties": {"color": {"enum": ["red", "green", "bl\"ue", "é"]}, "level": {"enum": [1, 2.5, -3]},
                        "k": {"const": "x"}, "flag": {"enum": [True, None]}}},
        [{"color": "red", "level": 1}, {"color": "bl\"ue", "level": 2.5, "k": "x"}, {"color": "é", "level": -3, "flag": None},
         {"color": "green", "level": 1, "flag": True}],
        ['{"color":"blue","level":1}', '{"color":"red","level":2}', '{"color":"red","level":1,"k":"y"}',
         '{"color":"red","level":1.0}', '{"color":red,"level":1}', '{"color":"red","level":1,"flag":false}']),
    "anyOf with null": (
        {"type": "object", "required": ["v"],
         "properties": {"v": {"anyOf": [{"type": "string", "maxLength": 3}, {"type": "null"}]},
                        "w": {"type": ["integer", "null"]},
                        "u": {"oneOf": [{"type": "boolean"}, {"type": "integer"}]}}},
        [{"v": None}, {"v": "abc"}, {"v": "", "w": None}, {"v": None, "w": 5, "u": True}, {"v": "日", "u": 3}],
        ['{"v":1}', '{"v":"abcd"}', '{"v":null,"w":"x"}', '{"w":5}', '{"v":null,"u":"t"}', '{"v": null}']),
    "$ref": (
        {"$defs": {"pt": _PT}, "type": "object", "required": ["a"],
         "properties": {"a": {"$ref": "#/$defs/pt"}, "b": {"$ref": "#/$defs/pt"}}},
        [{"a": {"x": 1, "y": 2}}, {"a": {"x": -1, "y": 0}, "b": {"x": 10, "y": 20}}],
        ['{"a":{"x":1}}', '{"b":{"x":1,"y":2}}', '{"a":{"x":1,"y":2,"z":3}}', '{"a":{"y":2,"x":1}}',
         '{"a":{"x":1,"y":02}}']),
    "array of objects": (
        {"type": "array", "minItems": 1, "maxItems": 3,
         "items": {"type": "object", "required": ["t"],
                   "properties": {"t": {"type": "string", "minLength": 1, "maxLength": 2}, "n": {"type": "integer"}}}},
        [[{"t": "a"}], [{"t": "ab", "n": 1}, {"t": "é"}], [{"t": "a"}, {"t": "b"}, {"t": "cc", "n": 0}]],
        ['[]', '[{"t":"a"},{"t":"a"},{"t":"a"},{"t":"a"}]', '[{"t":""}]', '[{"t":"abc"}]', '[{"t":"a"},]',
         '[{"t":"a"}, {"t":"b"}]', '{"t":"a"}', '[{"n":1}]']),
    "three strings of 64": (
        {"type": "object", "required": ["a", "b", "c"],
         "properties": {k: {"type": "string", "maxLength": 64} for k in "abc"}},
        [{"a": "", "b": "", "c": ""}, {"a": S64, "b": U64, "c": S64}, {"a": "hi", "b": "\t\u0001", "c": "é"}],
        ['{"a":"' + S64 + 'x","b":"","c":""}', '{"a":"","b":"' + U64 + 'y","c":""}', '{"a":"","b":""}',
         '{"a":"","b":"","c":"","d":""}', '{"a":"","b":"","c":5}', '{"a":"", "b":"","c":""}']),
}

# (schema, what the error names): everything outside the subset is refused, never ignored
REFUSED = [
    ({"type": "string", "pattern": "a+"}, "'pattern' at #"), ({"type": "string", "format": "date"}, "'format' at #"),
    ({"type": "integer", "minimum": 0}, "'minimum' at #"), ({"type": "number", "maximum": 1}, "'maximum' at #"),
    ({"type": "number", "multipleOf": 2}, "'multipleOf' at #"), ({"type": "object"}, "'type' at #"),
    ({"type": "object", "properties": {}, "additionalProperties": True}, "'additionalProperties' at #"),
    ({"type": "object", "properties": {}, "additionalProperties": {"type": "integer"}}, "'additionalProperties' at #"),
    ({"type": "object", "properties": {"a": {"type": "object", "properties": {"b": {"type": "string", "pattern": "x"}}}}},
     "'pattern' at #/properties/a/properties/b"),
    ({"type": "object", "properties": {}, "patternProperties": {}}, "'patternProperties' at #"),
    ({"type": "array", "items": {"type": "integer"}, "uniqueItems": True}, "'uniqueItems' at #"),
    ({"type": "array", "prefixItems": [{"type": "integer"}]}, "'prefixItems' at #"),
    ({"type": "array", "items": {"type": "integer"}, "maxItems": 17}, "'maxItems' at # must be an integer in [0, 16]"),
    ({"type": "string", "maxLength": 65}, "'maxLength' at # must be an integer in [0, 64]"),
    ({"type": "array"}, "'type' at #"), ({}, "'type' at #"), ({"not": {"type": "null"}}, "'not' at #"),
    ({"allOf": [{"type": "integer"}]}, "'allOf' at #"), ({"type": "integer", "minLength": 1}, "'minLength' at #"),
    ({"if": {"type": "integer"}}, "'if' at #"), ({"enum": [[1]]}, "'enum' at #"), ({"const": {"a": 1}}, "'const' at #"),
    ({"oneOf": [{"type": "integer"}, {"type": "number"}]}, "'oneOf' at #"),
    ({"oneOf": [{"type": "string", "maxLength": 1}, {"type": "string"}]}, "'oneOf' at #"),
    ({"$ref": "http://example.com/s.json"}, "'$ref' at #"),
    ({"$ref": "#/$defs/a", "$defs": {"a": {"type": "array", "items": {"$ref": "#/$defs/a"}}}}, "recursive $ref"),
    ({"$defs": {"a": {"$ref": "#/$defs/b"}, "b": {"$ref": "#/$defs/a"}}, "$ref": "#/$defs/a"}, "recursive $ref"),
    ({"$ref": "#/$defs/nope"}, "names no definition"),
]


def lower(schema) -> str:
    return rtmod.load().guide_schema_pattern(schema if isinstance(schema, str) else json.dumps(schema))


_COMPILED = {}


def compiled(name):
    """(pattern, table uint16 [n, 256], accept uint8 [n]) of a fixture, compiled once."""
    if name not in _COMPILED:
        pattern = lower(FIXTURES[name][0])
        _COMPILED[name] = (pattern, *compile_wide(pattern))
    return _COMPILED[name]


def compile_wide(pattern):
    n, tab, acc = rtmod.load().guide_compile_wide(pattern)
    return np.frombuffer(tab, dtype=np.uint16).reshape(n, 256), np.frombuffer(acc, dtype=np.uint8)


def compact(x) -> str:
    return json.dumps(x, separators=(",", ":"), ensure_ascii=False)


def walk(tab, raw: bytes, state: int = 0) -> int:
    for b in raw:
        if state == DEAD:
            return DEAD
        state = int(tab[state, b])
    return state


def accepts(tab, acc, raw: bytes) -> bool:
    s = walk(tab, raw)
    return s != DEAD and bool(acc[s])


def distance_to_accept(tab, acc):
    """Bytes still needed from each state to reach an accepting one (every state of a trimmed DFA reaches one)."""
    n = tab.shape[0]
    nxt = np.where(tab == DEAD, n, tab).astype(np.int64)
    dist = np.full(n + 1, 1 << 30, dtype=np.int64)
    dist[:n][acc != 0] = 0
    while True:
        new = np.minimum(dist[:n], dist[nxt].min(axis=1) + 1)
        if (new == dist[:n]).all():
            return dist[:n]
        dist[:n] = new


def draw(tab, acc, dist, rng: random.Random, turn: int = 48) -> bytes:
    """One accepted string: uniform among the live bytes of each state; once longer than `turn` bytes it stops at the
    first accepting state and otherwise takes a byte that brings acceptance nearer."""
    out, s = bytearray(), 0
    while True:
        live = np.nonzero(tab[s] != DEAD)[0]
        if acc[s] and (len(out) > turn or live.size == 0 or rng.random() < 0.15):
            return bytes(out)
        if len(out) > turn:
            live = [b for b in live if dist[tab[s, b]] < dist[s]]
        b = int(rng.choice(list(live)))
        out.append(b)
        s = int(tab[s, b])


# ------------------------------------------------------------------------------------------------ the validator
def _type_ok(t, x) -> bool:
    if t == "null":
        return x is None
    if t == "boolean":
        return isinstance(x, bool)
    if t == "integer":
        return isinstance(x, int) and not isinstance(x, bool) or isinstance(x, float) and x == int(x)
    if t == "number":
        return isinstance(x, (int, float)) and not isinstance(x, bool)
    return isinstance(x, {"string": str, "array": list, "object": dict}[t])


def _same(a, b) -> bool:
    return type(a) is type(b) and a == b or \
        all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in (a, b)) and a == b


def _valid_subset(x, s, root) -> bool:
    if "$ref" in s:
        return _valid_subset(x, root[s["$ref"].split("/")[1]][s["$ref"].split("/")[2]], root)
    for key in ("anyOf", "oneOf"):
        if key in s:
            n = sum(_valid_subset(x, b, root) for b in s[key])
            if n == 0 or (key == "oneOf" and n != 1):
                return False
    if "enum" in s and not any(_same(x, v) for v in s["enum"]):
        return False
    if "const" in s and not _same(x, s["const"]):
        return False
    if "type" in s:
        ts = s["type"] if isinstance(s["type"], list) else [s["type"]]
        if not any(_type_ok(t, x) for t in ts):
            return False
    if isinstance(x, str):
        if not s.get("minLength", 0) <= len(x) <= s.get("maxLength", 1 << 30):
            return False
    if isinstance(x, list):
        if not s.get("minItems", 0) <= len(x) <= s.get("maxItems", 1 << 30):
            return False
        if "items" in s and not all(_valid_subset(v, s["items"], root) for v in x):
            return False
    if isinstance(x, dict):
        props = s.get("properties", {})
        if any(k not in x for k in s.get("required", ())):
            return False
        if s.get("additionalProperties") is False and any(k not in props for k in x):
            return False
        if not all(_valid_subset(v, props[k], root) for k, v in x.items() if k in props):
            return False
    return True


def valid(x, schema) -> bool:
    """x validates against schema: by the jsonschema package where it imports, else by the validator above (the
    supported subset only, which is all the fixtures use)."""
    try:
        import jsonschema
    except ImportError:
        return _valid_subset(x, schema, schema)
    try:
        jsonschema.validate(x, schema)
        return True
    except jsonschema.ValidationError:
        return False


# ------------------------------------------------------------------------------------------------ the kernel vocabulary
VG, EOS = 512, 300   # EOS on the second shard of the 2-shard split
LEN0 = 7             # a zero-length piece


def vocabulary():
    """512 pieces of 0 to 4 bytes: every printable ASCII byte but 'l', pieces that cross a string's closing quote,
    multi-byte UTF-8 characters whole and split, escapes, and seeded filler.  No piece holds an 'l': after "nu" of null
    a guide is stuck.  (tok_bytes, tok_len) as torch tensors; ids 0, LEN0 and EOS have length 0."""
    fixed = [bytes([c]) for c in range(0x20, 0x7f) if c != ord("l")]
    fixed += [b'",', b'"}', b'":', b'{"', b'":"', b'a"', b'x"}', b'","', b'"a":', b'"b":', b'"c":', b'{"a"', b"xx", b"xxxx",
              "é".encode(), "日".encode(), "😀".encode(), b"\xc3", b"\xa9", "日".encode()[:2], "日".encode()[2:],
              "😀".encode()[:3], "😀".encode()[3:], b"\xc0\x80", b"\xed\xa0", b"\\n", b"\\u", b"00e9", b"d800", b"\\\"", b"\\\\",
              b"true", b"fa", b"se", b"nu", b"12", b"0.5", b"e+3", b"-1", b"00", b"},{", b"[{", b"}]", b"\x01", b"\n"]
    rng = random.Random(5)
    alphabet = b'abcdefxyz0123456789"{}:,\\ '
    pieces = [b""] * VG
    free = [i for i in range(1, VG) if i not in (LEN0, EOS)]
    rng.shuffle(free)
    for i in free:
        pieces[i] = fixed.pop() if fixed else bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 4)))
    return ops.guide_token_table(pieces, never={0, LEN0, EOS}), pieces
