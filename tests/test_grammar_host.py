"""CPU, no library: latex_ocr_amd.grammar.Grammar -- the host statement of the delimiter grammar and the tests' reference for the device
kernels.  The constructors, `check`, and the guarantee itself proved for the host model by exhaustive enumeration: from every reachable
state the set is non-empty, the invariant depth <= steps left holds, and every complete walk ends balanced with END by step max_iter."""
import numpy as np
import pytest

from latex_ocr_amd.grammar import Grammar

TOKS = ["a", "{", "}", "\\left(", "\\left[", "\\right)", "\\right]", "\\begin{array}", "\\end{array}", "\\begin{matrix}", "\\leftarrow",
        "\\rightarrow", "b", "_UNK", "_PAD", "_END"]


class Voc(object):
    tok_to_id = {t: i for i, t in enumerate(TOKS)}
    n_tok = len(TOKS)
    id_end = len(TOKS) - 1


def test_from_pairs_by_string_and_by_id():
    g = Grammar.from_pairs(Voc, [("{", "}"), (["\\left(", "\\left["], ["\\right)", 6])], max_depth=4)
    assert g.cls.dtype == np.int8 and g.cls.tolist() == [0, 1, -1, 2, 2, -2, -2] + [0] * 9
    assert (g.n_kinds, g.max_depth, g.budget, g.id_end, g.n_tok) == (2, 4, True, Voc.id_end, len(TOKS))
    h = Grammar.from_pairs(len(TOKS), [(1, 2)], budget=False)
    assert h.cls.tolist() == [0, 1, -1] + [0] * 13 and h.id_end is None and not h.budget
    for bad in ([("{", "nope")], [("{", "}"), ("{", "\\right)")], [(1, 99)], [], [(i, i) for i in range(16)]):
        with pytest.raises(ValueError):
            Grammar.from_pairs(Voc, bad)
    with pytest.raises(ValueError):
        Grammar.from_pairs(len(TOKS), [("{", "}")])                         # strings without a vocabulary
    with pytest.raises(ValueError):
        Grammar(np.zeros(4, np.int8), max_depth=33)
    with pytest.raises(ValueError):
        Grammar(np.array([0, 16], np.int64))
    with pytest.raises(ValueError):
        Grammar(np.array([0, 1, -1], np.int8), id_end=1)                    # END must be plain


def test_latex_reads_the_token_strings():
    g = Grammar.latex(Voc)
    c = dict(zip(TOKS, g.cls.tolist()))
    assert c["{"] == -c["}"] > 0
    assert c["\\left("] == c["\\left["] == -c["\\right)"] == -c["\\right]"] > 0
    assert c["\\begin{array}"] == -c["\\end{array}"] > 0
    assert len({c["{"], c["\\left("], c["\\begin{array}"]}) == 3 and g.n_kinds == 3
    assert c["\\begin{matrix}"] == 0                                        # no \end{matrix} in the vocabulary: the kind is dropped
    assert c["\\leftarrow"] == 0 and c["\\rightarrow"] == 0                 # arrows are no delimiters
    assert c["a"] == c["_END"] == 0 and g.id_end == Voc.id_end
    with pytest.raises(ValueError):
        Grammar.latex(["a", "b", "_END"])


def test_check_is_balanced_and_ended():
    g = Grammar.latex(Voc)
    i = Voc.tok_to_id
    E = Voc.id_end
    seq = lambda *t: [i[x] for x in t]
    assert g.check(seq("a", "{", "\\left(", "b", "\\right]", "}", "_END"))
    assert g.check(seq("_END")) and g.check(seq("a", "_END", "}", "}"))      # what follows END does not count
    assert not g.check(seq("a", "{", "_END"))                                # open at END
    assert not g.check(seq("}", "_END"))                                     # closer with nothing open
    assert not g.check(seq("{", "\\left(", "}", "\\right)", "_END"))         # crossed
    assert not g.check(seq("{", "}"))                                        # no END
    assert not g.check([])
    assert g.check(np.array(seq("{", "}", "_END"), np.int32), E)
    with pytest.raises(ValueError):
        Grammar(g.cls).check(seq("_END"))                                    # no id_end bound, none passed


def test_apply_leaves_the_state_on_what_the_grammar_bans():
    g = Grammar(np.array([0, 1, -1, 2, -2, 0], np.int8), max_depth=2, id_end=5)
    assert g.apply((), 1) == (1,) and g.apply((1,), 3) == (1, 2) and g.apply((1, 2), 4) == (1,)
    assert g.apply((1, 2), 1) == (1, 2)                                      # an opener at max_depth
    assert g.apply((1, 2), 2) == (1, 2)                                      # a mismatched closer
    assert g.apply((), 2) == ()                                              # a closer at depth 0
    assert g.apply((1,), 0) == (1,) and g.apply((1,), 5) == (1,) and g.apply((1,), 77) == (1,)


# tokens: 0 plain, 1 / 2 open / close kind 1, 3 / 4 open / close kind 2, 5 END
CLS = np.array([0, 1, -1, 3 - 1, -2, 0], np.int8)


@pytest.mark.parametrize("max_iter", range(7))
def test_guarantee_by_exhaustive_enumeration(max_iter):
    """every reachable (state, t) at max_iter <= 6, D = 2, two kinds: the set is non-empty, depth <= r before every step, at r == d only the
    matching closer (or END at depth 0) is left, and every walk reaches END at or before step max_iter, balanced"""
    g = Grammar(CLS, max_depth=2, budget=True, id_end=5)
    seen, walks = set(), [0]

    def walk(state, t, toks):
        r = max_iter - t
        assert len(state) <= r, (state, t)
        ok = g.allowed_at(state, t, max_iter)
        assert ok.any(), (state, t)
        seen.add((len(state), r))
        if r == len(state):
            assert np.nonzero(ok)[0].tolist() == ([5] if not state else [2 * state[-1]])
        if r == len(state) + 1:
            assert not ok[1] and not ok[3]                                   # no room left to open
        for tok in np.nonzero(ok)[0].tolist():
            if tok == 5:
                assert not state and g.check(toks + [5]) and len(toks) + 1 <= max_iter + 1
                walks[0] += 1
                continue
            assert t < max_iter                                              # something other than END: a step must be left
            walk(g.apply(state, tok), t + 1, toks + [tok])

    walk((), 0, [])
    assert walks[0] >= 1
    assert {d for d, _ in seen} == set(range(min(2, max_iter // 2) + 1))      # the depths the budget and D leave reachable
    if max_iter >= 4:
        assert (2, 2) in seen and (0, 0) in seen
    if max_iter >= 5:
        assert (2, 3) in seen


def test_without_budget_only_the_order_rules_bind():
    g = Grammar(CLS, max_depth=2, budget=False, id_end=5)
    for t in (0, 6):
        assert g.allowed_at((), t, 6).tolist() == [True, True, False, True, False, True]
        assert g.allowed_at((1,), t, 6).tolist() == [True, True, True, True, False, False]
        assert g.allowed_at((1, 2), t, 6).tolist() == [True, False, False, False, True, False]
    b = Grammar(CLS, max_depth=2, budget=True, id_end=5)
    assert b.allowed_at((1,), 5, 6).tolist() == [False, False, True, False, False, False]     # r == d
    assert b.allowed_at((1,), 4, 6).tolist() == [True, False, True, False, False, False]      # r == d + 1
    assert b.allowed_at((), 6, 6).tolist() == [False] * 5 + [True]
