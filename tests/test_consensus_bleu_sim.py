"""CPU (hipsim): lxo_consensus_bleu -- the consensus under the cost 1 - sentence BLEU, csrc/seqcost.hip -- against the float64 reference of
tests/sentence_bleu_ref.py: the clipped matches as integers in both directions, the exact cases and the diagonal on their bytes, costs and risks
within the derived bounds, the arg-min exactly; weights, permuted draws, layouts, repeat runs and the -1 returns.  The same cases run on the
MI355X in tests/test_gpu_sentence_bleu.py."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from simlib import SIM_SO, build_sim
from sentence_bleu_ref import LIMIT, MAX_N, RISK_BOUND, check_cons_case, cons_cases, cons_weight_cases, make_cons, run_cons


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


def test_case_matrix(lib):
    cases = cons_cases()
    assert {c["n"] for c in cases} >= {1, 2, 3, 5, MAX_N} and {c["B"] for c in cases} >= {1, 3}
    for c in cases:
        check_cons_case(lib, c)


def test_named_equal_draw_cases(lib):
    by = {c["name"]: c for c in cons_cases()}
    _, cost, risk, best = check_cons_case(lib, by["all draws equal"])
    assert not cost.any() and not risk.any() and not best.any()
    _, cost, risk, best = check_cons_case(lib, by["all draws empty"])
    assert not cost.any() and not risk.any() and not best.any()
    c = by["two equal draws tie"]
    _, cost, risk, best = check_cons_case(lib, c)
    assert best.tolist() == [1, 1] and risk[:, 1].tobytes() == risk[:, 2].tobytes() and (risk[:, 0] > risk[:, 1]).all()


def test_weights(lib):
    cases = cons_weight_cases()
    assert [c["name"] for c in cases] == ["weights: %s" % k for k in ("none", "positive", "with zeros", "one-hot", "a row of zeros", "negative, NaN, inf")]
    for c in cases:
        check_cons_case(lib, c)


def test_permuted_draws_permute_the_outputs(lib):
    c = [x for x in cons_cases() if x["n"] == 5 and x["B"] == 3][0]
    B, n, T = c["B"], c["n"], c["T"]
    ids = c["ids"].reshape(B, -1, n)
    match, cost, risk, best = check_cons_case(lib, c)
    perm = np.array([3, 0, 4, 2, 1])
    pc = make_cons("permuted", ids[:, :, perm], T, c["id_end"])
    m2, c2, r2, b2 = check_cons_case(lib, pc)
    assert np.array_equal(m2, match[:, perm][:, :, perm]) and c2.tobytes() == np.ascontiguousarray(cost[:, perm][:, :, perm]).tobytes()
    assert np.abs(r2.astype(np.float64) - risk[:, perm]).max() <= 2 * RISK_BOUND          # (the sums run in another order)
    assert perm[b2].tolist() == best.tolist()


def test_layouts_without_match_and_runs_repeat(lib):
    c = [x for x in cons_cases() if x["name"].endswith("BnT")][0]
    B, n, T = c["B"], c["n"], c["T"]
    rows = c["ids"].reshape(B, n, T)
    first = check_cons_case(lib, c)
    other = make_cons("as [B, T, n]", np.ascontiguousarray(rows.transpose(0, 2, 1)), T, c["id_end"])
    second = check_cons_case(lib, other)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    rc, none, cost, risk, best = run_cons(lib, c, want_match=False)
    assert rc == 0 and none is None and all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], (cost, risk, best)))
    # no image: nothing launches, nothing is written
    rc, _, cost, risk, best = run_cons(lib, c, B=0)
    assert rc == 0 and (cost == -7).all() and (risk == -7).all()


def test_refusals(lib):
    c = [x for x in cons_cases() if x["n"] == 3][0]
    z = ctypes.c_void_p(0)
    assert run_cons(lib, c)[0] == 0
    for kw in (dict(ids=z), dict(cost=z), dict(risk=z), dict(best=z), dict(B=-1), dict(n=0), dict(n=MAX_N + 1), dict(T=-1), dict(T=LIMIT + 1),
               dict(image_stride=-1), dict(draw_stride=-1), dict(tok_stride=-1), dict(B=1 << 21, n=MAX_N)):
        rc, match, cost, risk, best = run_cons(lib, c, **kw)
        assert rc == -1 and lib.lxo_last_error(), kw
        assert (match == -7).all() and (cost == -7).all() and (risk == -7).all() and (best == -7).all(), kw
    assert run_cons(lib, c, T=LIMIT + 1)[0] == -1 and b"staging limit" in lib.lxo_last_error()
    assert run_cons(lib, c, n=MAX_N + 1)[0] == -1 and b"LXO_CONSENSUS_MAX_N" in lib.lxo_last_error()
