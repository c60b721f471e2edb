"""No GPU: the host side of regular-expression grammars (whisperlive_amd/pattern.py) — the compiler against re.fullmatch on every short
string over a small alphabet, trimming, the refusals and the limits by name, the vocabulary's bytes against the tokenizer's decode,
dead_states on a hand-made vocabulary."""
import itertools
import re

import numpy as np
import pytest

from whisperlive_amd import pattern as P
from whisperlive_amd.tokenizer import synthetic_tokenizer

# (regex, ignore_case, alphabet): \d \w \s are ASCII sets here, so the reference compiles with re.ASCII
PATTERNS = [(r"\d{3}", False, "019a"), (r"\d{2,4}-\d", False, "12-"), (r"yes|no|maybe", False, "yesnomab"), (r"(ab|a)(c|bc)*", False, "abc"),
            (r"(a(b|c){1,2}d?){2}", False, "abcd"), (r"[^ab]c+", False, "abcé"), (r"[a-c_]+x?", False, "abc_xd"), (r"Yes|No", True, "yesnoYN"),
            (r"[a-b]{2}", True, "abAB"), (r"né+e", False, "neé"), (r"a{2,}b*", False, "ab"), (r"\w+\.\s?\W", False, "a_. é!"),
            (r"(?:x|yz)?\\", False, "xyz\\")]


@pytest.mark.parametrize("regex,ignore_case,alphabet", PATTERNS)
def test_the_compiled_dfa_matches_what_re_fullmatch_matches(regex, ignore_case, alphabet):
    p = P.compile_pattern(regex, ignore_case=ignore_case, leading_space=False)
    spaced = P.compile_pattern(regex, ignore_case=ignore_case)
    flags = re.ASCII | (re.IGNORECASE if ignore_case else 0)
    ref, ref_spaced = re.compile(regex, flags), re.compile(f" ?(?:{regex})", flags)             # leading_space: " ?(regex)"
    n = 0
    for length in range(7 if len(alphabet) <= 4 else 6):
        for chars in itertools.product(alphabet, repeat=length):
            text = "".join(chars)
            want = ref.fullmatch(text) is not None
            assert p.accepts(text) == want, text
            for t in (text, " " + text):
                assert spaced.accepts(t) == (ref_spaced.fullmatch(t) is not None), t
            n += want
    assert n > 0                                # (the alphabet reaches the language)
    # trimming: every live state has a path to an accepting state, every state is reachable, and state 0 is the start state
    for q in (p, spaced):
        nxt = [set(int(t) for t in row if t != P.DEAD) for row in q.trans]
        good = {s for s in range(q.n_states) if q.accept[s]}
        while True:
            more = {s for s in range(q.n_states) if nxt[s] & good} | good
            if more == good:
                break
            good = more
        assert good == set(range(q.n_states))
        assert q.byte_class.dtype == np.uint8 and q.trans.dtype == np.uint16 and int(q.byte_class.max()) == q.n_classes - 1


def test_a_digit_string_is_a_state_per_digit():
    p = P.compile_pattern(r"\d{8}")
    assert (p.n_states, p.n_classes) == (10, 3) and p.accepts(" 12345678") and p.accepts("12345678") and not p.accepts("1234567")
    assert p.step(0, b" 1") == 2 and p.step(0, b"x") == -1 and p.step(2, ord("5")) == 3


REFUSED = [(r"^a", "anchor"), (r"a$", "anchor"), (r"a\b", "anchor"), (r"(a)\1", "back-reference"), (r"(?=a)b", "look-around"),
           (r"(?<!a)b", "look-around"), (r"a*?", "lazy"), (r"a{2,3}?", "lazy"), (r"a++", "possessive"), (r"[aé]", "non-ASCII character inside a class"),
           (r"(?P<n>a)", "named group"), (r"(?i)a", "inline flag"), (r"(a", "without its ')'"), (r"a)", "unmatched ')'"), (r"[ab", "without its ']'"),
           (r"*a", "nothing to repeat"), (r"a{3,2}", "count"), (r"a{1001}", "count"), (r"\p", "escape"), ("", "non-empty"),
           (r"(\d{1000}){5}", "4096 states"), (r"[ab]*a[ab]{12}", "4096 states"),
           (r"[a-z]{40}" + "".join(chr(97 + k) + "{60}" for k in range(26)), "24576 cells")]


@pytest.mark.parametrize("regex,names", REFUSED)
def test_a_refusal_names_its_construct_or_limit(regex, names):
    with pytest.raises(ValueError, match=re.escape(names)):
        P.compile_pattern(regex)


def test_token_bytes_inverts_decode():
    tk = synthetic_tokenizer(2310)              # (the smallest vocabularies of the special-token layout start near 1900 ids)
    eot = tk.token_to_id("<|endoftext|>")
    off, by = P.token_bytes(tk, eot)
    assert off.dtype == np.int32 and off.shape == (eot + 1,) and off[0] == 0 and by.dtype == np.uint8 and by.shape == (off[-1],)
    assert sorted(bytes(by[off[t]:off[t + 1]]) for t in range(256)) == [bytes([b]) for b in range(256)]     # the byte alphabet, once each
    for t in range(256, eot):
        assert bytes(by[off[t]:off[t + 1]]).decode("utf-8") == tk.decode([t]) == f" w{t}"
    ids = tk.encode(" w300 é7").ids
    assert b"".join(bytes(by[off[t]:off[t + 1]]) for t in ids) == " w300 é7".encode("utf-8")
    assert P.token_bytes(tk, eot)[1] is by      # cached per tokenizer: the same arrays


def test_dead_states_on_a_hand_made_vocabulary():
    # tokens: 0 `a`, 1 `b`, 2 `ab`, 3 `c`, 4 empty, 5 ` `
    parts = [b"a", b"b", b"ab", b"c", b"", b" "]
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int32)
    by = np.frombuffer(b"".join(parts), np.uint8)
    p = P.compile_pattern("abc", leading_space=False)           # states 0 -a-> 1 -b-> 2 -c-> 3 (accepting)
    assert [p.allowed(s, off, by).tolist() for s in range(4)] == [[0, 2], [1], [3], []]
    assert p.dead_states(off, by, []) == []                     # state 3 allows nothing but accepts
    assert p.dead_states(off, by, [1]) == [1] and p.dead_states(off, by, [0]) == [] and p.dead_states(off, by, [0, 2, 3]) == [0, 2]
    assert p.dead_states(off, by, [2], blank=0) == [0] and p.dead_states(off, by, [2], blank=1) == []       # the blank counts in state 0 only
    assert p.dead_states(off[:4], by[:4], []) == [2]            # a vocabulary without `c`: nothing to emit and no acceptance
    q = P.compile_pattern("abc")                                # " ?abc": the space token alone leads on
    assert q.allowed(0, off, by).tolist() == [0, 2, 5] and q.dead_states(off, by, [0, 2]) == [1] and q.dead_states(off, by, [0, 2], blank=5) == [0, 1]
