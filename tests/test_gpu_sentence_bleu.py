"""-m gpu: the sentence-level BLEU cost on the MI355X, through liblxo.so.

1. lxo_sentence_bleu on the pair matrix of tests/sentence_bleu_ref.py, as the hipsim file: counts as integers (and against lxo_text_stats), the exact
   cases on their bytes, floats against float64 within the derived 1e-5; twice the same bytes.
2. lxo_consensus_bleu on the consensus cases and the weight cases: matches, costs, risks, the arg-min.
3. lxo_mrt_candidates_cost with either cost on the constructed ids.
4. Both calls captured into one graph (one stream, one branch) and replayed, also on other ids.
5. Engine.mrt_sample_step(cost="bleu") in f32 against the host candidates, the host sentence_bleu_cost and the oracle's q and risk."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from latex_ocr_amd import _abi
from latex_ocr_amd.engine import _p
from latex_ocr_amd.model.evaluation.text import sentence_bleu_cost
import mrt_oracle
from edit_distance_ref import CAND_END, CAND_PAD, CAND_REFS, cand_calls, constructed_ids, host_candidates, run_candidates
from sentence_bleu_ref import (BOUND, CASE_NAMES, WORST, bleu_of, check_cons_case, check_pair_case, cons_cases, cons_weight_cases, counts_of, host_consensus,
                               named, run_bleu, run_cons, RISK_BOUND)


class Dev(object):
    """numpy <-> the GPU for the shared runners of tests/sentence_bleu_ref.py"""
    stream = None

    @staticmethod
    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def ptr(a):
        return _p(a)

    @staticmethod
    def down(a):
        return a.cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


# ------------------------------------------------------------------------------------------------------------------ 1. the pair kernel --
@pytest.mark.parametrize("name", CASE_NAMES)
def test_pair_matrix(lib, name):
    c = named(name)
    counts, bleu, cost = check_pair_case(lib, c, Dev)
    again = run_bleu(lib, c, Dev)
    assert again[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(again[1:], (counts, bleu, cost)))
    alone = run_bleu(lib, c, Dev, want=(False, False, True))
    assert alone[0] == 0 and alone[1] is None and alone[3].tobytes() == cost.tobytes()
    print("largest deviation of a bleu / cost so far: %.3g" % WORST.get("bleu", 0.0))


# ------------------------------------------------------------------------------------------------------------------ 2. the consensus --
def test_consensus_matrix(lib):
    for c in cons_cases() + cons_weight_cases():
        first = check_cons_case(lib, c, Dev)
        again = run_cons(lib, c, Dev)
        assert again[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(again[1:], first)), c["name"]
    print("largest deviations: cost %.3g (bound %.0e), risk %.3g (bound %.0e)" % (WORST["bleu"], BOUND, WORST["risk"], RISK_BOUND))


# ------------------------------------------------------------------------------------------------------------------ 3. the candidates --
@pytest.mark.parametrize("steps,inc", cand_calls())
def test_mrt_candidates_cost(lib, steps, inc):
    class Shim(object):
        def __init__(self, kind):
            self.kind = kind

        def lxo_mrt_candidates(self, *a):
            return lib.lxo_mrt_candidates_cost(*(a[:-1] + (self.kind, a[-1])))
    ids = constructed_ids()
    base = run_candidates(lib, ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc, Dev)
    edit = run_candidates(Shim(_abi.LXO_COST_EDIT), ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc, Dev)
    assert base[0] == 0 and edit[0] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(base[1:], edit[1:]))
    bleu = run_candidates(Shim(_abi.LXO_COST_BLEU), ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc, Dev)
    assert bleu[0] == 0 and all(bleu[k].tobytes() == base[k].tobytes() for k in (1, 2, 4, 5))
    cost, group_off, row_image = bleu[3], bleu[4], bleu[5]
    f, ln, sizes, _ = host_candidates(ids[:, :steps], CAND_REFS, CAND_END, CAND_PAD, bool(inc))
    live = int(group_off[-1])
    want = np.array([sentence_bleu_cost([int(x) for x in f[r, :ln[r] - 1]], CAND_REFS[int(row_image[r])]) for r in range(live)])
    assert live == int(sizes.sum()) and np.abs(cost[:live].astype(np.float64) - want).max() <= BOUND
    assert cost[live:].tobytes() == np.zeros(len(cost) - live, np.float32).tobytes()
    if inc:
        assert all(cost[int(o)].tobytes() == np.float32(0).tobytes() for o in group_off[:-1])


# ------------------------------------------------------------------------------------------------------------------ 4. a graph --
def test_both_calls_are_captured_into_a_graph(lib):
    """lxo_sentence_bleu and lxo_consensus_bleu on the capturing stream, one behind the other: a replay gives the eager calls' bytes, and on other
    ids what the definition gives on them"""
    rng = np.random.default_rng(6)
    B, T, n = 3, 70, 4
    first = rng.integers(0, 3, size=(B, T, n)).astype(np.int32)
    refs = torch.from_numpy(rng.integers(0, 3, size=(B, 66)).astype(np.int32)).cuda()
    ids = torch.from_numpy(first).cuda()
    pairs = B * n
    counts, bleu, pcost = (torch.empty(pairs, 10, dtype=torch.int32, device="cuda"), torch.empty(pairs, dtype=torch.float32, device="cuda"),
                           torch.empty(pairs, dtype=torch.float32, device="cuda"))
    match, cost, risk, best = (torch.empty(B, n, n, 4, dtype=torch.int32, device="cuda"), torch.empty(B, n, n, dtype=torch.float32, device="cuda"),
                               torch.empty(B, n, dtype=torch.float32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))
    outs = (counts, bleu, pcost, match, cost, risk, best)

    def both():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.lxo_sentence_bleu(_p(ids), n, T * n, 1, n, T, None, _p(refs), B, 66, None, None, n, pairs, 2, _p(counts), _p(bleu), _p(pcost), st) == 0
        assert lib.lxo_consensus_bleu(_p(ids), T * n, 1, n, B, n, T, 2, None, _p(match), _p(cost), _p(risk), _p(best), st) == 0

    def host(a):
        cut = lambda s: [int(x) for x in s[:list(s).index(2)]] if 2 in s else [int(x) for x in s]
        r = refs.cpu().numpy()
        want_b = np.array([bleu_of(cut(a[g, :, j]), cut(r[g])) for g in range(B) for j in range(n)])
        want_c = np.array([counts_of(cut(a[g, :, j]), cut(r[g])) for g in range(B) for j in range(n)], np.int32)
        return want_b, want_c, host_consensus(a, 2)

    both()
    torch.cuda.synchronize()
    eager = [o.cpu().numpy().copy() for o in outs]
    wb, wc, (c_ref, r_ref, _) = host(first)
    assert np.array_equal(eager[0], wc) and np.abs(eager[1] - wb).max() <= BOUND and np.abs(eager[4] - c_ref).max() <= BOUND
    for o in outs:
        o.fill_(-7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    g.replay()
    torch.cuda.synchronize()
    assert all(o.cpu().numpy().tobytes() == e.tobytes() for o, e in zip(outs, eager))
    other = rng.integers(0, 3, size=(B, T, n)).astype(np.int32)
    ids.copy_(torch.from_numpy(other).cuda())
    g.replay()
    torch.cuda.synchronize()
    wb, wc, (c_ref, r_ref, _) = host(other)
    assert np.array_equal(counts.cpu().numpy(), wc) and np.abs(bleu.cpu().numpy() - wb).max() <= BOUND
    assert np.abs(cost.cpu().numpy() - c_ref).max() <= BOUND and np.abs(risk.cpu().numpy() - r_ref).max() <= RISK_BOUND
    assert best.cpu().tolist() == np.argmin(risk.cpu().numpy(), axis=1).tolist()


# ------------------------------------------------------------------------------------------------------------------ 5. the step --
H, W, V = 32, 128, 50
ID_END, ID_PAD = V - 1, V - 2
N, ALPHA, MAX_ITER = 3, 1.0, 6
SAMPLING = dict(temperature=0.5, top_k=2, seed=7)                   # tests/test_gpu_mrt_device.py's: few likely tokens per step, draws repeat


def test_mrt_sample_step_with_the_bleu_cost():
    imgs, forms = synthetic.make_set(2, H, W, V, 3, 5, seed=13)
    ref, rl = pad_batch_formulas(forms, ID_PAD, ID_END)
    img, refs = pad_batch_images(imgs), [list(f) for f in forms]
    eng = with_env("LXO_ENC_OVERLAP", "0", lambda: Engine(V, dtype="f32", seed=3))
    ids = eng.sample_decode(img, ID_END, n=N, max_iter=MAX_ITER, **SAMPLING)
    f, ln, sizes, edit_costs = host_candidates(ids, refs, ID_END, ID_PAD, True)
    rows = np.repeat(np.arange(len(sizes)), sizes)
    costs64 = np.array([sentence_bleu_cost([int(x) for x in f[r, :ln[r] - 1]], refs[rows[r]]) for r in range(len(ln))])
    P = oracle_params(eng)
    risk_ref, _, q_ref = mrt_oracle.mrt_grads(P, img, f, ln, sizes, costs64.astype(np.float32), ALPHA)
    risk, info = eng.mrt_sample_step(img, ref, rl, ID_END, ID_PAD, 0.0, ALPHA, n=N, max_iter=MAX_ITER, cost="bleu", **SAMPLING)
    assert info["group_sizes"].tolist() == sizes.tolist() and info["cand_lengths"].tolist() == ln.tolist()
    for r in range(len(ln)):
        assert info["cand"][r, :ln[r]].tolist() == f[r, :ln[r]].tolist() and (info["cand"][r, ln[r]:] == ID_PAD).all(), r
    err = np.abs(info["cost"].astype(np.float64) - costs64).max()
    print("f32: group sizes %s, risk %.7f oracle %.7f, q max err %.2e, cost max err %.2e" % (sizes.tolist(), risk, risk_ref, np.abs(info["q"] - q_ref).max(), err))
    assert err <= BOUND and (info["cost"] != edit_costs).any()
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert all(info["cost"][o].tobytes() == np.float32(0).tobytes() for o in off[:-1])
    assert abs(risk - risk_ref) <= 1e-5 and np.abs(info["q"] - q_ref).max() <= 1e-5
