"""The pattern compiler of guided decoding (csrc/runtime/guide.cpp) against Python's re.fullmatch: the language of every
supported construct, trimming, every rejected construct and limit, and the guided_choice lowering.  CPU only."""
import itertools
import re
import time

import numpy as np
import pytest

from distributed_sse_for_llm_response_amd import runtime as rtmod

DEAD = 0xFFFF


def compile_(pattern):
    n, tab, acc = rtmod.load().guide_compile(pattern)
    tab = np.frombuffer(tab, dtype=np.uint16).reshape(n, 256)
    acc = np.frombuffer(acc, dtype=np.uint8)
    assert tab.shape == (n, 256) and acc.shape == (n,) and 1 <= n <= 512
    assert ((tab < n) | (tab == DEAD)).all()
    return tab, acc


def accepts(tab, acc, data: bytes) -> bool:
    s = 0
    for b in data:
        s = int(tab[s, b])
        if s == DEAD:
            return False
    return bool(acc[s])


# (pattern, alphabet): every string over the alphabet up to length 6 is checked against re.fullmatch
CASES = [
    ("abc", "abcd"), ("", "ab"), ("a|b|cd", "abcd"), ("a*", "ab"), ("a+b?", "abc"), ("(ab)*c", "abc"),
    ("(?:ab|c)+", "abc"), ("a{3}", "ab"), ("a{2,}", "ab"), ("a{1,3}b", "abc"), ("a{0}b", "ab"), ("a{0,2}", "ab"),
    ("(a|b){2,4}c", "abc"), (".", "a\nb."), (".*a", "a\nbc"), (r"\d+", "09a-"), (r"\D\d", "0a9-"), (r"\w+", "a_0-Z"),
    (r"\W", "a_0- "), (r"\s*x", " \tx\n"), (r"\Sx", " ax\t"), (r"a\nb|\t\r", "ab\n\t\r"), (r"\.\*\+\?", ".*+?a"),
    (r"\(\)\[\]\{\}\|\\", "()[]{"), (r"\^\$\-\/", "^$-/a"), ("[abc]+", "abcd"), ("[^ab]", "abc\n"), ("[a-c]x", "abcdx"),
    ("[a-cx-z0]+", "axz0b"), (r"[\d\-x]+", "0-x9a"), (r"[^\w]", "a_-. "), (r"[\s,]+", " ,a\n"), ("[]a]+", "]ab["),
    ("[^]a]", "]ab["), ("[a-]+", "a-b"), (r"[\]\\]", "]\\a"), ("[.*+?(){}|^$]+", ".*(^a"), ("(a(b(c)?)?)?d", "abcd"),
    ("(|a)b", "ab"), ("(a*)*b", "ab"), ("(a|ab)(c|bcd)", "abcd"), ("[0-9]{3}-[0-9]{4}", "019-"), ("x(?:a|b)*", "xab"),
    ("a]b}", "ab]}"), ("(yes|no|maybe)", "yesno"),
]


@pytest.mark.parametrize("pattern, alphabet", CASES)
def test_language_equals_re_fullmatch(pattern, alphabet):
    tab, acc = compile_(pattern)
    want = re.compile(pattern)
    n = 0
    for L in range(0 if len(alphabet) <= 5 else 1, 7):
        for tup in itertools.product(alphabet, repeat=L):
            s = "".join(tup)
            assert accepts(tab, acc, s.encode()) == (want.fullmatch(s) is not None), (pattern, s)
            n += 1
    assert n > 100


def test_non_ascii_literals_are_byte_sequences():
    tab, acc = compile_("é+|日本")
    for s in ("é", "éé", "日本"):
        assert accepts(tab, acc, s.encode())
    for s in ("", "日", "é日本", "\xc3"):
        assert not accepts(tab, acc, s.encode())
    assert not accepts(tab, acc, "é".encode()[:1])


@pytest.mark.parametrize("pattern", [c[0] for c in CASES] + ["(a|b)*abb", "a{255}a{255}a", "(ab|ac|ad){0,40}"])
def test_every_state_reaches_acceptance(pattern):
    tab, acc = compile_(pattern)
    n = tab.shape[0]
    live = acc.astype(bool).copy()
    for _ in range(n):
        nxt = np.where(tab == DEAD, 0, tab)
        live |= ((tab != DEAD) & live[nxt]).any(axis=1)
    assert live.all()
    seen, todo = {0}, [0]  # and every state is reachable from the start
    while todo:
        for t in set(tab[todo.pop()].tolist()) - {DEAD}:
            if t not in seen:
                seen.add(t)
                todo.append(t)
    assert len(seen) == n


REJECTED = [
    ("^a", "anchor ^", 0), ("a$", "anchor $", 1), (r"a\b", "anchor \\b", 1), (r"\Aa", "anchor \\A", 0),
    (r"(a)\1", "back-reference", 3), ("(?=a)b", "look-around", 0), ("(?!a)b", "look-around", 0),
    ("(?<=a)b", "look-around", 0), ("(?<!a)b", "look-around", 0), ("a*?", "lazy quantifier", 2),
    ("a+?", "lazy quantifier", 2), ("a??", "lazy quantifier", 2), ("a{2}?", "lazy quantifier", 4),
    ("a*+", "possessive quantifier", 2), ("a++", "possessive quantifier", 2), ("(?P<n>a)", "named group", 0),
    ("(?<n>a)", "named group", 0), ("(?i)a", "inline flag", 0), ("(?#c)a", "comment group", 0),
    ("a**", "quantifier on a quantifier", 2), ("*a", "nothing to repeat", 0), ("(|+)", "nothing to repeat", 2),
    ("a{256}", "bound above 255", 1), ("a{1,256}", "bound above 255", 1), ("a{3,2}", "n < m", 1),
    ("a{,3}", "without a lower bound", 1), ("a{2", "malformed quantifier", 1), ("a{", "without a lower bound", 1), ("{", "unescaped {", 0),
    ("(a", "unterminated group", 0), ("a)", "unbalanced )", 1), ("[a", "unterminated class", 0),
    ("[é]", "non-ASCII class member", 1), ("[a-é]", "non-ASCII class member", 3), ("[z-a]", "reversed class range", 1),
    (r"[a-\d]", "range end", 3), ("[[:alpha:]]", "POSIX class", 1), (r"\x41", "unsupported escape \\x", 0),
    (r"\pL", "unsupported escape \\p", 0), ("a\\", "trailing backslash", 1), ("(" * 101 + ")" * 101, "nested deeper", 100),
]


@pytest.mark.parametrize("pattern, construct, offset", REJECTED)
def test_rejected_constructs_are_named_with_their_offset(pattern, construct, offset):
    with pytest.raises(ValueError) as e:
        compile_(pattern)
    assert construct in str(e.value) and str(e.value).endswith(f"at offset {offset}"), str(e.value)


def test_limits_are_errors():
    tab, _ = compile_("a{255}a{255}a")       # 512 states: the limit itself
    assert tab.shape[0] == 512
    with pytest.raises(ValueError, match="more than 512 DFA states"):
        compile_("a{255}a{255}aa")           # 513
    compile_("a" * 300 + "|" + "b" * 200)    # (a long pattern within the limits)
    with pytest.raises(ValueError, match="longer than 8192 bytes"):
        compile_("(?:a|b)*" * 1024 + "c")    # 8193 bytes
    with pytest.raises(ValueError, match="more than 16384 NFA states.*quantifier at offset 8"):
        compile_("(a{255}){255}")
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="work cap"):
        compile_("(?:(?:a?){255}){12}b")     # nested quantifiers: ~15k NFA states in every closure
    assert time.perf_counter() - t0 < 5.0


def test_choice_lowering_round_trips_every_metacharacter():
    mod = rtmod.load()
    choices = ["a.b", "a*b", "x+y?", "(z)", "[q]", "{1}", "a|b", "back\\slash", "^start$", "tab\there", "plain", "é-ü",
               "-#&~", "\\d\\w", "]}"]
    pattern = mod.guide_choice_pattern(choices)
    tab, acc = compile_(pattern)
    want = re.compile(pattern)
    for c in choices:
        assert accepts(tab, acc, c.encode()) and want.fullmatch(c)
    for c in ["axb", "ab", "aab", "xy", "xyy", "z", "q", "1", "a", "b", "backslash", "start", "", "plainplain", "5a",
              "a.b|a*b"]:
        assert not accepts(tab, acc, c.encode()) and not want.fullmatch(c)
    assert mod.guide_choice_pattern(["only"]) == "only"
