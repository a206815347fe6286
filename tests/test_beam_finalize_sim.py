"""CPU (hipsim): lxo_beam_finalize and lxo_beam_rerank -- the kernels of csrc/beamfin.hip -- against include/lxo.h's definitions as
tests/beam_finalize_ref.py restates them: the back-trace bit for bit on the case matrix (integers, and the f32 outputs as bytes), the rerank's scores
and posterior against float64 within bounds derived from its stated arithmetic, its order exactly.  The same runners go through the MI355X in
tests/test_gpu_beam_finalize.py."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from latex_ocr_amd.model.utils.text import beam_backtrace, beam_parent_rows
from simlib import SIM_SO, build_sim
from beam_finalize_ref import (END, MAX_K, MAX_STEPS, OUTPUTS, all_cases, check_case, check_finalize, check_rerank, finalize_reference, make_case,
                               make_rerank_case, preconditions, rerank_cases, rerank_reference, run_finalize, run_rerank, special_cases, stable_order)


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


# ------------------------------------------------------------------------------------------------------------------ finalize --
def test_the_matrix_holds_what_it_claims():
    preconditions(all_cases())


@pytest.mark.parametrize("i", range(len(all_cases())), ids=[c["name"] for c in all_cases()])
def test_finalize_matches_the_definition(lib, i):
    check_case(lib, all_cases()[i])


def test_each_output_alone_and_without_scores(lib):
    """a nullable argument changes nothing about the others"""
    for c in special_cases()[:3] + [x for x in all_cases() if x["steps"] == 65 and x["k"] == 5][:2]:
        for n in OUTPUTS:
            rc, got = run_finalize(lib, c, outputs=(n,))
            assert rc == 0 and list(got) == [n], (c["name"], n, lib.lxo_last_error())
            check_finalize(c, got)
        rc, got = run_finalize(lib, c, outputs=("hyp", "len", "src"), with_scores=False)
        assert rc == 0 and len(got) == 3, c["name"]
        check_finalize(c, got)


def test_the_clamp_is_the_reference_s(lib):
    c = special_cases()[0]
    p = c["parents"][:, :c["steps"]]
    assert [int(((p[b] < 0) | (p[b] >= c["k"])).sum()) for b in range(c["B"])] == [1] * c["B"]
    check_case(lib, c)


def test_against_the_host_back_trace(lib):
    """on decodes where a finished path only extends with END (what the beam kernels produce): hyp is beam_backtrace, src beam_parent_rows
    transposed, seq_logp the last step's scores"""
    rng = np.random.default_rng(11)
    B, k, steps = 3, 5, 20
    c = make_case("decode-like", B, k, steps, steps + 2, "random", "none", 12)
    ids, par, sc = c["ids"], c["parents"], c["scores"]
    fin = np.zeros((B, k), bool)
    for t in range(steps):                                           # a slot whose parent has finished carries END on and keeps its score
        if t:
            fin = np.take_along_axis(fin, par[:, t], axis=1)
            keep = np.take_along_axis(sc[:, t - 1], par[:, t], axis=1)
            sc[:, t] = np.where(fin, keep, sc[:, t])
        ids[:, t] = np.where(fin, END, ids[:, t])
        new = rng.random(size=(B, k)) < 0.08
        ids[:, t] = np.where(new & ~fin, END, ids[:, t])
        fin |= new
    c["want"] = finalize_reference(ids, par, sc, steps, k, END)
    got = check_case(lib, c)
    assert (got["len"] < steps).any() and (got["len"] == steps).any()
    assert np.array_equal(got["hyp"], beam_backtrace(ids[:, :steps], par[:, :steps]))
    assert np.array_equal(got["src"].reshape(steps, B, k).transpose(1, 0, 2), beam_parent_rows(par[:, :steps]))
    assert got["seq_logp"].tobytes() == np.ascontiguousarray(sc[:, steps - 1]).tobytes()
    run = beam_backtrace(sc[:, :steps], par[:, :steps])
    assert np.array_equal(got["tok_logp"], np.where(np.arange(steps)[None, :, None] < got["len"][:, None, :], np.diff(run, axis=1, prepend=np.float32(0)), 0))


def test_finalize_repeats_and_refuses(lib):
    c = special_cases()[1]
    a, b = run_finalize(lib, c)[1], run_finalize(lib, c)[1]
    assert all(a[n].tobytes() == b[n].tobytes() for n in OUTPUTS)
    rc, got = run_finalize(lib, c, B=0)
    assert rc == 0 and all((v == -7).all() for v in got.values())
    z = ctypes.c_void_p(0)
    for kw, code in ((dict(ids=z), -1), (dict(parents=z), -1), (dict(scores=z), -1), (dict(B=-1), -1), (dict(id_end=-1), -1), (dict(ld_t=c["steps"] - 1), -1),
                     (dict(k=0), -5), (dict(k=MAX_K + 1), -5), (dict(steps=0), -5), (dict(steps=MAX_STEPS + 1, ld_t=MAX_STEPS + 1), -5)):
        rc, got = run_finalize(lib, c, **kw)
        assert rc == code and lib.lxo_last_error().startswith(b"lxo_beam_finalize") and all((v == -7).all() for v in got.values()), kw
    assert run_finalize(lib, c, outputs=())[0] == -1
    assert run_finalize(lib, c, outputs=("hyp",), with_scores=False)[0] == 0


# -------------------------------------------------------------------------------------------------------------------- rerank --
def test_rerank_matches_the_definition(lib):
    worst_s = worst_p = 0.0
    sep = tot = 0
    for c in rerank_cases():
        rc, got = run_rerank(lib, c)
        assert rc == 0, (c["name"], lib.lxo_last_error())
        s, p, a, b = check_rerank(c, got)
        worst_s, worst_p, sep, tot = max(worst_s, s), max(worst_p, p), sep + a, tot + b
    print("rerank: largest score deviation %.3f of its bound, posterior %.3f of its bound; %d of %d images separated" % (worst_s, worst_p, sep, tot))
    assert sep >= 0.9 * tot, (sep, tot)


def test_the_cases_are_separated_under_the_reference_alone():
    """at least 90 % of the images have adjacent float64 scores more than twice the bound apart: the order check is not vacuous"""
    from beam_finalize_ref import score_bound
    sep = tot = 0
    for c in rerank_cases():
        ref, _, cp = rerank_reference(c["len"], c["seq"], c["cov"], c["R"], c["alpha"], c["beta"], c["floor"])
        sb = score_bound(c["seq"], c["len"], cp, c["alpha"], c["beta"])
        ro = np.argsort(-ref, axis=1, kind="stable")
        rs, rb = np.take_along_axis(ref, ro, axis=1), np.take_along_axis(sb, ro, axis=1)
        ok = (rs[:, :-1] - rs[:, 1:] > 2 * np.maximum(rb[:, :-1], rb[:, 1:])).all(axis=1)
        sep, tot = sep + int(ok.sum()), tot + len(ok)
    assert sep >= 0.9 * tot, (sep, tot)


def test_alpha_zero_without_coverage_is_seq_logp_bit_for_bit(lib):
    c = make_rerank_case("alpha 0", 9, 5, 0.0, 0.7, 0.5, 3)         # beta without coverage adds nothing
    c["seq"][0, 0], c["seq"][1, 2] = -0.0, np.float32(-1e-38)
    rc, got = run_rerank(lib, c)
    assert rc == 0 and got["score"].tobytes() == c["seq"].tobytes()
    assert np.array_equal(got["order"], stable_order(c["seq"]))


def test_ties_go_to_the_lower_slot(lib):
    c = make_rerank_case("ties", 4, 5, 0.6, 0.0, 0.5, 4)
    c["seq"][:, 3], c["len"][:, 3] = c["seq"][:, 1], c["len"][:, 1]
    c["seq"][2], c["len"][2] = np.float32(-3.25), 17                 # a whole image of equal hypotheses
    rc, got = run_rerank(lib, c)
    assert rc == 0 and got["score"][:, 1].tobytes() == got["score"][:, 3].tobytes()
    for b in (0, 1, 3):
        o = got["order"][b].tolist()
        assert o.index(1) + 1 == o.index(3), o
    assert got["order"][2].tolist() == [0, 1, 2, 3, 4] and got["post"][2].tobytes() == np.full(5, 0.2, np.float32).tobytes()
    check_rerank(c, got)


def test_a_length_penalty_changes_the_winner(lib):
    c = make_rerank_case("winner", 1, 2, 0.0, 0.0, 0.5, 5)
    c["seq"][0], c["len"][0] = (-10.0, -11.0), (5, 20)
    assert run_rerank(lib, c)[1]["order"].tolist() == [[0, 1]]
    c["alpha"] = 1.0                                                 # -10 / (10 / 6) = -6 against -11 / (25 / 6) = -2.64
    rc, got = run_rerank(lib, c)
    assert got["order"].tolist() == [[1, 0]] and got["post"][0, 0] > got["post"][0, 1]      # the posterior is the search's, not the rerank's
    check_rerank(c, got)


def test_padding_cells_shift_an_image_s_scores_together(lib):
    c = [x for x in rerank_cases() if x["R"] == 35 and x["k"] == 5][0]
    wide = dict(c, cov=np.concatenate([c["cov"][:, :35], np.zeros((c["cov"].shape[0], 5), np.float32)], axis=1), R=40)
    a, b = run_rerank(lib, c)[1], run_rerank(lib, wide)[1]
    assert np.array_equal(a["order"], b["order"]) and a["post"].tobytes() == b["post"].tobytes()
    shift = b["score"].astype(np.float64) - a["score"]
    want = float(np.float32(c["beta"])) * 5 * np.log(float(np.float32(c["floor"])))
    assert np.abs(shift - want).max() <= 2.0 ** -22 * np.abs(a["score"]).max()


def test_rerank_nullable_outputs_repeat_and_refusals(lib):
    c = rerank_cases()[2]
    rc, full = run_rerank(lib, c)
    assert rc == 0 and run_rerank(lib, c)[1]["score"].tobytes() == full["score"].tobytes()
    for n in ("score", "post", "order"):
        rc, got = run_rerank(lib, c, outputs=(n,))
        assert rc == 0 and list(got) == [n] and got[n].tobytes() == full[n].tobytes()
    rc, got = run_rerank(lib, c, B=0)
    assert rc == 0 and all((v == -7).all() for v in got.values())
    z = ctypes.c_void_p(0)
    for kw, code in ((dict(len=z), -1), (dict(seq=z), -1), (dict(B=-1), -1), (dict(k=0), -5), (dict(k=MAX_K + 1), -5), (dict(alpha=-0.1), -1),
                     (dict(alpha=float("nan")), -1), (dict(beta=-1.0), -1), (dict(beta=float("inf")), -1), (dict(floor=0.0), -1), (dict(floor=1.5), -1),
                     (dict(R=-1), -1), (dict(cov_ld=c["R"] - 1), -1)):
        rc, got = run_rerank(lib, c, **kw)
        assert rc == code and lib.lxo_last_error().startswith(b"lxo_beam_rerank") and all((v == -7).all() for v in got.values()), kw
    assert run_rerank(lib, c, outputs=())[0] == -1
