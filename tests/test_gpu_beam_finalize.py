"""-m gpu: lxo_beam_finalize and lxo_beam_rerank on the MI355X through liblxo.so, with the runners of tests/beam_finalize_ref.py exactly as the hipsim
file drives them: the back-trace bit for bit on the case matrix (steps = 1024 at k = 16 on one case), every output alone, the rerank's scores and
posterior within their derived bounds and its order exactly; a call made twice gives the same bytes; both calls captured into one graph and replayed
on another decode.  The largest deviations met, as fractions of their bounds, are printed for profiles/beam_finalize.txt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from latex_ocr_amd import _abi
from latex_ocr_amd.engine import _p
from beam_finalize_ref import (MAX_K, MAX_STEPS, OUTPUTS, all_cases, check_case, check_finalize, check_rerank, make_case, make_rerank_case, rerank_cases,
                               run_finalize, run_rerank, special_cases, stable_order)


class Dev(object):
    """numpy <-> the GPU for the shared runners of tests/beam_finalize_ref.py"""
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


def test_finalize_matrix(lib):
    cases = all_cases()
    assert sum(c["steps"] == MAX_STEPS and c["k"] == MAX_K for c in cases) == 1
    for c in cases:
        check_case(lib, c, Dev)


def test_each_output_alone_and_runs_repeat(lib):
    for c in special_cases()[:3] + [x for x in all_cases() if x["steps"] in (65, MAX_STEPS) and x["k"] in (5, MAX_K)][:4]:
        rc, full = run_finalize(lib, c, Dev)
        assert rc == 0
        for n in OUTPUTS:
            rc, got = run_finalize(lib, c, Dev, outputs=(n,))
            assert rc == 0 and list(got) == [n] and got[n].tobytes() == full[n].tobytes(), (c["name"], n)
        rc, got = run_finalize(lib, c, Dev, outputs=("hyp", "len", "src"), with_scores=False)
        assert rc == 0
        check_finalize(c, got)
        rc, again = run_finalize(lib, c, Dev)
        assert rc == 0 and all(again[n].tobytes() == full[n].tobytes() for n in OUTPUTS), c["name"]


def test_refusals_launch_nothing(lib):
    c = special_cases()[1]
    for kw, code in ((dict(ids=None), -1), (dict(scores=None), -1), (dict(B=-1), -1), (dict(id_end=-1), -1), (dict(ld_t=c["steps"] - 1), -1), (dict(k=0), -5),
                     (dict(k=MAX_K + 1), -5), (dict(steps=0), -5), (dict(steps=MAX_STEPS + 1, ld_t=MAX_STEPS + 1), -5)):
        rc, got = run_finalize(lib, c, Dev, **kw)
        torch.cuda.synchronize()
        assert rc == code and lib.lxo_last_error() and all((v == -7).all() for v in got.values()), kw
    r = rerank_cases()[2]
    for kw, code in ((dict(len=None), -1), (dict(k=MAX_K + 1), -5), (dict(alpha=-0.5), -1), (dict(beta=float("nan")), -1), (dict(floor=0.0), -1),
                     (dict(cov_ld=r["R"] - 1), -1)):
        rc, got = run_rerank(lib, r, Dev, **kw)
        torch.cuda.synchronize()
        assert rc == code and all((v == -7).all() for v in got.values()), kw


def test_rerank_cases(lib):
    worst_s = worst_p = 0.0
    sep = tot = 0
    for c in rerank_cases():
        rc, got = run_rerank(lib, c, Dev)
        assert rc == 0, (c["name"], lib.lxo_last_error())
        s, p, a, b = check_rerank(c, got)
        worst_s, worst_p, sep, tot = max(worst_s, s), max(worst_p, p), sep + a, tot + b
        rc, again = run_rerank(lib, c, Dev)
        assert all(again[n].tobytes() == got[n].tobytes() for n in got), c["name"]
    print("rerank on the MI355X: largest score deviation %.3f of its bound, posterior %.3f of its bound; %d of %d images separated" % (worst_s, worst_p, sep, tot))
    assert sep >= 0.9 * tot
    c = make_rerank_case("alpha 0", 9, 5, 0.0, 0.7, 0.5, 3)
    got = run_rerank(lib, c, Dev)[1]
    assert got["score"].tobytes() == c["seq"].tobytes() and np.array_equal(got["order"], stable_order(c["seq"]))
    c = make_rerank_case("ties", 4, 5, 0.6, 0.0, 0.5, 4)
    c["seq"][:, 3], c["len"][:, 3] = c["seq"][:, 1], c["len"][:, 1]
    got = run_rerank(lib, c, Dev)[1]
    assert got["score"][:, 1].tobytes() == got["score"][:, 3].tobytes() and all(o.index(1) + 1 == o.index(3) for o in got["order"].tolist())


def test_both_calls_are_captured_into_one_graph(lib):
    """finalize and the rerank of its outputs on the capturing stream, one behind the other: a replay gives the eager bytes, and on another decode in
    the same buffers what the definition gives on it"""
    a, b = make_case("graph a", 3, 5, 40, 44, "random", "mixed", 31), make_case("graph b", 3, 5, 40, 44, "collapse", "mixed", 32)
    B, k, steps, ld = a["B"], a["k"], a["steps"], a["ld_t"]
    ids, par, sc = (torch.from_numpy(a[n]).cuda() for n in ("ids", "parents", "scores"))
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.full(s, -7, dtype=torch.float32, device="cuda")
    out = dict(hyp=i32(B, steps, k), len=i32(B, k), src=i32(steps, B * k), tok_logp=f32(B, steps, k), seq_logp=f32(B, k))
    score, post, order = f32(B, k), f32(B, k), i32(B, k)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        assert lib.lxo_beam_finalize(_p(ids), _p(par), _p(sc), B, ld, steps, k, a["id_end"], *([_p(out[n]) for n in OUTPUTS] + [st])) == 0
        assert lib.lxo_beam_rerank(_p(out["len"]), _p(out["seq_logp"]), None, 0, 0, B, k, 0.6, 0.0, 0.5, _p(score), _p(post), _p(order), st) == 0
    for c in (a, b):
        ids.copy_(torch.from_numpy(c["ids"]).cuda())
        par.copy_(torch.from_numpy(c["parents"]).cuda())
        sc.copy_(torch.from_numpy(c["scores"]).cuda())
        g.replay()
        torch.cuda.synchronize()
        check_finalize(c, {n: out[n].cpu().numpy() for n in OUTPUTS})
        r = dict(name=c["name"], B=B, k=k, len=c["want"]["len"], seq=c["want"]["seq_logp"], cov=None, R=0, cov_ld=0, alpha=0.6, beta=0.0, floor=0.5)
        got = dict(score=score.cpu().numpy(), post=post.cpu().numpy(), order=order.cpu().numpy())
        check_rerank(r, got)
        eager = run_rerank(lib, r, Dev)[1]
        assert all(eager[n].tobytes() == got[n].tobytes() for n in got)
    assert not np.array_equal(a["want"]["hyp"], b["want"]["hyp"])
