"""CPU: Img2SeqModel._token_sets -- banned / allowed token lists (strings or ids, one list for all images or one per image) to the boolean sets
Engine.greedy_decode / beam_decode take as allowed=."""
import types

import numpy as np
import pytest

from latex_ocr_amd.model.img2seq import Img2SeqModel

TOKS = ["a", "b", "\\frac", "{", "}", "_UNK", "_PAD", "_END"]
STUB = types.SimpleNamespace(_vocab=types.SimpleNamespace(tok_to_id={t: i for i, t in enumerate(TOKS)}, n_tok=len(TOKS), id_end=7))
sets = lambda n, **kw: Img2SeqModel._token_sets(STUB, n, kw.get("banned"), kw.get("allowed"))


def test_no_lists_no_constraint():
    assert sets(3) is None


def test_banned_is_the_complement_form():
    m = sets(3, banned=["_UNK", "_PAD"])
    assert m.shape == (8,) and m.dtype == bool and m.tolist() == [True] * 5 + [False, False, True]
    assert np.array_equal(sets(3, banned=[5, 6]), m)                         # ids or strings
    assert sets(3, banned=[]).all()


def test_allowed_one_list_and_per_image():
    m = sets(2, allowed=["a", "{", 7])
    assert m.tolist() == [True, False, False, True, False, False, False, True]
    m = sets(2, allowed=[["a", "_END"], ["b", "_END"]])
    assert m.shape == (2, 8) and m[0].tolist() == [True] + [False] * 6 + [True] and m[1].tolist() == [False, True] + [False] * 5 + [True]
    m = sets(2, allowed=[["a", "b", "_END"], ["b", "_END"]], banned=["b"])    # both: allowed and not banned
    assert m[:, 1].tolist() == [False, False] and m[:, 0].tolist() == [True, False]
    m = sets(2, banned=[["a"], []])
    assert m.shape == (2, 8) and not m[0, 0] and m[1].all()


def test_unknown_tokens_and_wrong_counts_raise():
    with pytest.raises(ValueError):
        sets(2, banned=["\\no_such_token"])
    with pytest.raises(ValueError):
        sets(2, allowed=[8])
    with pytest.raises(ValueError):
        sets(3, allowed=[["a"], ["b"]])
