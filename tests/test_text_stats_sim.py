"""CPU (hipsim): lxo_text_stats -- the text-metric counts of csrc/seqcost.hip -- against the project's own _ngrams / levenshtein / truncate_end on the
case matrix of tests/text_stats_ref.py, as integers; its distance column against lxo_edit_distance on the same arguments; the corpus row, accumulate,
either output alone, repeat runs, scores_from_counts against the host metrics, and the -1 returns.  The same matrix runs on the MI355X in
tests/test_gpu_text_stats.py."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from latex_ocr_amd.model.evaluation.text import bleu_score, edit_distance, exact_match_score, scores_from_counts
from simlib import SIM_SO, build_sim
from edit_distance_ref import Host, run_edit
from text_stats_ref import CASE_NAMES, LIMIT, NC, NS, check_text_case, corpus_of, named, run_text, text_cases


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_stats_match_the_host_functions(lib, name):
    c = named(name)
    stats, _ = check_text_case(lib, c)
    rc, dist, _ = run_edit(lib, c, want_cost=False)                 # the same arguments through lxo_edit_distance
    assert rc == 0 and np.array_equal(stats[:, 10], dist)


def test_corpus_accumulates_and_overwrites(lib):
    c = named("END, lengths")
    half = c["pairs"] // 2
    rc, s1, co = run_text(lib, c, corpus=np.full(NC, 99, np.int64), accumulate=0, hi=half)      # overwrites what was there
    assert rc == 0 and co.tolist() == corpus_of(c["stats"][:half]).tolist() and np.array_equal(s1, c["stats"][:half])
    rc, s2, co = run_text(lib, c, corpus=co, accumulate=1, lo=half)
    assert rc == 0 and co.tolist() == c["corpus"].tolist() and np.array_equal(s2, c["stats"][half:])
    rc, _, co2 = run_text(lib, c, corpus=co, accumulate=1)          # and once more on top: twice the sums
    assert rc == 0 and co2.tolist() == (2 * c["corpus"]).tolist()
    # the same without the rows (the waves add into the corpus themselves)
    rc, none, co = run_text(lib, c, want_stats=False, corpus=np.full(NC, 99, np.int64), accumulate=0, hi=half)
    assert rc == 0 and none is None and co.tolist() == corpus_of(c["stats"][:half]).tolist()
    rc, _, co = run_text(lib, c, want_stats=False, corpus=co, accumulate=1, lo=half)
    assert rc == 0 and co.tolist() == c["corpus"].tolist()
    # no pair: the corpus is zeroed or left alone, nothing else is written
    rc, s0, co0 = run_text(lib, c, corpus=np.full(NC, 5, np.int64), accumulate=0, hi=0)
    assert rc == 0 and s0.size == 0 and not co0.any()
    rc, _, co0 = run_text(lib, c, corpus=np.full(NC, 5, np.int64), accumulate=1, hi=0)
    assert rc == 0 and (co0 == 5).all()


def test_either_output_alone_and_runs_repeat(lib):
    for name in ("wave, ref 129", "strided [B, T, n]"):
        c = named(name)
        rc, s1, none = run_text(lib, c)
        assert rc == 0 and none is None and np.array_equal(s1, c["stats"])
        rc, none, co = run_text(lib, c, want_stats=False, corpus=np.full(NC, -7, np.int64))
        assert rc == 0 and none is None and co.tolist() == c["corpus"].tolist()
        rc, s2, co2 = run_text(lib, c, corpus=np.full(NC, -7, np.int64))
        assert rc == 0 and s2.tobytes() == s1.tobytes() and co2.tobytes() == co.tobytes()


def test_scores_from_counts_equal_the_host_metrics(lib):
    # (the host metrics run the Python levenshtein once more: the pairs of the widest references are left to the integer checks above)
    cases = [c for c in text_cases() if c["ref"].shape[1] <= 152]
    assert len(cases) >= 20
    for c in cases:
        _, _, co = run_text(lib, c, want_stats=False, corpus=np.zeros(NC, np.int64))
        hyps, refs = [h for h, _ in c["cut"]], [r for _, r in c["cut"]]
        got = scores_from_counts(co)
        want = {"BLEU-4": bleu_score(refs, hyps) * 100, "ExactMatchScore": exact_match_score(refs, hyps) * 100, "EditDistance": edit_distance(refs, hyps) * 100}
        assert got == want, (c["name"], got, want)
    # the whole matrix as one corpus, accumulated call by call
    co = np.zeros(NC, np.int64)
    hyps, refs = [], []
    for c in cases:
        _, _, co = run_text(lib, c, want_stats=False, corpus=co, accumulate=1)
        hyps += [h for h, _ in c["cut"]]
        refs += [r for _, r in c["cut"]]
    got = scores_from_counts(co)
    assert got["BLEU-4"] == bleu_score(refs, hyps) * 100 > 0.0 and got["EditDistance"] == edit_distance(refs, hyps) * 100
    assert got["ExactMatchScore"] == exact_match_score(refs, hyps) * 100 > 0.0
    assert scores_from_counts([0] * NC) == {"BLEU-4": 0.0, "ExactMatchScore": 0.0, "EditDistance": 100.0}      # no pair: the host functions' values
    with pytest.raises(ValueError):
        scores_from_counts([0] * 12)


def test_refusals(lib):
    c = named("short")
    p, z = Host.ptr, ctypes.c_void_p(0)
    hyp, ref, hl, rl = c["hyp"], c["ref"], c["hyp_len"], c["ref_len"]
    stats, corpus = np.full((c["pairs"], NS), -7, np.int32), np.full(NC, -7, np.int64)
    T = c["T"]

    def call(hyp_p=p(hyp), ref_p=p(ref), stats_p=p(stats), corpus_p=p(corpus), block=1, bs=T, rs=0, ts=1, T=T, G=c["pairs"], ref_ld=ref.shape[1], per_ref=1,
             pairs=c["pairs"], acc=0):
        return lib.lxo_text_stats(hyp_p, block, bs, rs, ts, T, p(hl), ref_p, G, ref_ld, p(rl), z, per_ref, pairs, -1, stats_p, corpus_p, acc, None)

    assert call() == 0 and np.array_equal(stats, c["stats"])
    for kw in (dict(hyp_p=z), dict(ref_p=z), dict(stats_p=z, corpus_p=z), dict(pairs=-1), dict(T=-1), dict(T=LIMIT + 1), dict(G=-1), dict(G=0), dict(bs=-1),
               dict(ts=-1), dict(rs=-1), dict(block=0), dict(per_ref=0), dict(ref_ld=0), dict(ref_ld=LIMIT + 1), dict(acc=2), dict(acc=-1)):
        stats[:] = -7
        corpus[:] = -7
        assert call(**kw) == -1, kw
        assert lib.lxo_last_error() and (stats == -7).all() and (corpus == -7).all(), kw
    assert call(T=LIMIT + 1) == -1 and b"staging limit" in lib.lxo_last_error()
    assert call(ref_ld=LIMIT + 1) == -1 and b"column limit" in lib.lxo_last_error()
