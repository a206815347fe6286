"""CPU (hipsim): lxo_sentence_bleu -- the sentence-level BLEU of csrc/seqcost.hip -- against the float64 definition of tests/sentence_bleu_ref.py on
its case matrix: the counts as integers (and against lxo_text_stats on the same arguments), the exact cases on their bytes, the floats within the
derived 1e-5; the host restatement sentence_bleu; lxo_mrt_candidates_cost with either cost; repeat runs and the -1 returns.  The same matrix
runs on the MI355X in tests/test_gpu_sentence_bleu.py."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from latex_ocr_amd.model.evaluation.text import sentence_bleu, sentence_bleu_cost
from simlib import SIM_SO, build_sim
from edit_distance_ref import CAND_END, CAND_PAD, CAND_REFS, Host, cand_calls, constructed_ids, host_candidates, run_candidates
from sentence_bleu_ref import BOUND, CASE_NAMES, LIMIT, NCNT, bleu_of, check_pair_case, named, pair_cases, run_bleu


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_pairs_match_the_definition(lib, name):
    check_pair_case(lib, named(name))


def test_host_restatement_is_the_definition():
    """sentence_bleu (model/evaluation/text.py, Python floats) against the reference module's own statement, and the named values"""
    for c in pair_cases():
        for (h, r), b in zip(c["cut"], c["bleu"]):
            got = sentence_bleu(h, r)
            assert abs(got - b) <= 1e-12 and sentence_bleu_cost(h, r) == 1.0 - got, (c["name"], h, r)
            assert (got == 1.0) == (h == r)
    assert sentence_bleu([], []) == 1.0 and sentence_bleu([], [1]) == 0.0 and sentence_bleu([1], []) == 0.0
    assert sentence_bleu([1, 2], [1, 2]) == 1.0 and sentence_bleu_cost([3, 4], [1, 2]) == 1.0
    # worked by hand: h = a b against r = a b c: m = (2, 1, 0, 0), t = (2, 1, 1, 1), p = (1, 1, 1/2, 1/2), BP = exp(1 - 3/2)
    assert abs(sentence_bleu([1, 2], [1, 2, 3]) - np.exp(-0.5) * 0.25 ** 0.25) < 1e-15
    assert bleu_of([1, 2], [1, 2, 3]) == sentence_bleu([1, 2], [1, 2, 3])


def test_either_output_alone_and_runs_repeat(lib):
    for name in ("wave, ref 129", "strided [B, T, n]", "END, lengths clamped"):
        c = named(name)
        rc, counts, bleu, cost = run_bleu(lib, c)
        assert rc == 0
        for k, want in enumerate(((True, False, False), (False, True, False), (False, False, True))):
            out = run_bleu(lib, c, want=want)
            assert out[0] == 0 and [o is None for o in out[1:]] == [not w for w in want]
            assert out[1 + k].tobytes() == (counts, bleu, cost)[k].tobytes()
        again = run_bleu(lib, c)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[1:], (counts, bleu, cost)))
    # no pair: nothing runs, nothing is written
    c = dict(named("clipping"), pairs=0)
    rc, counts, bleu, cost = run_bleu(lib, c)
    assert rc == 0 and counts.shape == (0, NCNT) and bleu.size == 0


def _run_cand_cost(lib, ids, steps, refs, inc, kind):
    """run_candidates through lxo_mrt_candidates_cost: the same outputs"""
    class Shim(object):
        def __getattr__(self, k):
            return getattr(lib, k)

        def lxo_mrt_candidates(self, *a):
            return lib.lxo_mrt_candidates_cost(*(a[:-1] + (kind, a[-1])))
    return run_candidates(Shim(), ids, steps, refs, CAND_END, CAND_PAD, inc)


@pytest.mark.parametrize("steps,inc", cand_calls())
def test_mrt_candidates_cost(lib, steps, inc):
    ids = constructed_ids()
    base = run_candidates(lib, ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc)
    edit = _run_cand_cost(lib, ids, steps, CAND_REFS, inc, _abi.LXO_COST_EDIT)
    assert base[0] == 0 and edit[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(base[1:], edit[1:]))       # the existing call, byte for byte
    bleu = _run_cand_cost(lib, ids, steps, CAND_REFS, inc, _abi.LXO_COST_BLEU)
    assert bleu[0] == 0
    for k in (1, 2, 4, 5):                                          # cand, cand_len, group_off, row_image
        assert bleu[k].tobytes() == base[k].tobytes()
    cand, cand_len, cost, group_off = bleu[1], bleu[2], bleu[3], bleu[4]
    live = int(group_off[-1])
    f, ln, sizes, _ = host_candidates(ids[:, :steps], CAND_REFS, CAND_END, CAND_PAD, bool(inc))
    assert live == int(sizes.sum())
    want = np.array([sentence_bleu_cost([int(x) for x in f[r, :ln[r] - 1]], CAND_REFS[int(bleu[5][r])]) for r in range(live)])
    assert np.abs(cost[:live].astype(np.float64) - want).max() <= BOUND
    assert cost[live:].tobytes() == np.zeros(len(cost) - live, np.float32).tobytes()                 # dead rows
    if inc:
        assert all(cost[int(o)].tobytes() == np.float32(0).tobytes() for o in group_off[:-1])       # the reference's own row
    assert (want > 0).any() and (cost[:live] != base[3][:live]).any()


def test_refusals(lib):
    c = named("clipping")
    p, z = Host.ptr, ctypes.c_void_p(0)
    hyp, ref, hl, rl = c["hyp"], c["ref"], c["hyp_len"], c["ref_len"]
    counts, bleu, cost = np.full((c["pairs"], NCNT), -7, np.int32), np.full(c["pairs"], -7, np.float32), np.full(c["pairs"], -7, np.float32)
    T = c["T"]

    def call(hyp_p=p(hyp), ref_p=p(ref), outs=(p(counts), p(bleu), p(cost)), block=1, bs=T, rs=0, ts=1, T=T, G=c["pairs"], ref_ld=ref.shape[1], per_ref=1,
             pairs=c["pairs"]):
        return lib.lxo_sentence_bleu(hyp_p, block, bs, rs, ts, T, p(hl), ref_p, G, ref_ld, p(rl), z, per_ref, pairs, -1, outs[0], outs[1], outs[2], None)

    assert call() == 0 and np.array_equal(counts, c["counts"])
    for kw in (dict(hyp_p=z), dict(ref_p=z), dict(outs=(z, z, z)), dict(pairs=-1), dict(T=-1), dict(T=LIMIT + 1), dict(G=-1), dict(G=0), dict(bs=-1),
               dict(ts=-1), dict(rs=-1), dict(block=0), dict(per_ref=0), dict(ref_ld=0), dict(ref_ld=LIMIT + 1)):
        counts[:], bleu[:], cost[:] = -7, -7, -7
        assert call(**kw) == -1, kw
        assert lib.lxo_last_error() and (counts == -7).all() and (bleu == -7).all() and (cost == -7).all(), kw
    assert call(outs=(z, z, z)) == -1 and b"all NULL" in lib.lxo_last_error()
    assert call(T=LIMIT + 1) == -1 and b"staging limit" in lib.lxo_last_error()
    # lxo_mrt_candidates_cost: another cost_kind, and rows wider than the kernel takes under LXO_COST_BLEU
    ids = constructed_ids()
    for kind in (2, -1):
        out = _run_cand_cost(lib, ids, 6, CAND_REFS, 1, kind)
        assert out[0] == -1 and b"cost_kind" in lib.lxo_last_error() and all((o == -7).all() for o in out[1:])
    wide = np.zeros((1, LIMIT, 1), np.int32)
    assert _run_cand_cost(lib, wide, LIMIT, [[1]], 1, _abi.LXO_COST_BLEU)[0] == -1 and b"steps + 1" in lib.lxo_last_error()
    assert _run_cand_cost(lib, wide, LIMIT, [[1]], 1, _abi.LXO_COST_EDIT)[0] == 0
