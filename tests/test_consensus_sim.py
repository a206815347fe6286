"""CPU (hipsim): lxo_consensus -- the pairs and select kernels of csrc/seqcost.hip -- against the project's own levenshtein / truncate_end and the
risk of include/lxo.h's definition in float64, on the case matrix of tests/consensus_ref.py: the distances and the arg-min exactly, the risk bit for
bit where the definition makes it exact and within the derived bound elsewhere; its properties and its -1 returns.  The same matrix runs on the
MI355X in tests/test_gpu_consensus.py."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from simlib import SIM_SO, build_sim
from consensus_ref import LIMIT, MAX_N, all_cases, bound, check_case, end_cases, make_case, matrix_cases, run_consensus, weight_cases, with_options


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.mark.parametrize("i", range(len(all_cases())), ids=[c["name"] for c in all_cases()])
def test_consensus_matches_the_definition(lib, i):
    check_case(lib, all_cases()[i])


def test_named_outcomes(lib):
    by = {c["name"]: c for c in all_cases()}
    for name in ("all draws empty", "all draws equal"):
        _, dist, risk, best = run_consensus(lib, by[name])
        assert not dist.any() and risk.tobytes() == np.zeros_like(risk).tobytes() and not best.any(), name
    _, dist, risk, best = run_consensus(lib, by["two equal draws tie"])
    assert best.tolist() == [1, 1] and (risk[:, 1].tobytes() == risk[:, 2].tobytes()) and (risk[:, 1] < risk[:, 0]).all() and (dist[:, 1, 2] == 0).all()
    for nm in (0, 1):
        # the weight on one draw: that draw costs nothing, nor does its copy (draws 1 and 3 are equal), and the first of them is chosen
        _, _, risk, best = run_consensus(lib, by["weights: one-hot norm%d" % nm])
        assert best.tolist() == [1, 0, 1] and risk[0, 1] == risk[0, 3] == risk[1, 0] == risk[2, 1] == risk[2, 3] == 0.0
        assert np.count_nonzero(risk) == risk.size - 5
        # a row of zero weights is the row of ones; a negative, NaN or infinite weight is a zero: bit for bit
        z, pos = by["weights: a row of zeros norm%d" % nm], by["weights: positive norm%d" % nm]
        _, _, rz, bz = run_consensus(lib, z)
        _, _, rp, _ = run_consensus(lib, pos)
        _, _, ru, bu = run_consensus(lib, by["weights: none norm%d" % nm])
        assert rz[1].tobytes() == ru[1].tobytes() and bz[1] == bu[1] and rz[[0, 2]].tobytes() == rp[[0, 2]].tobytes()
        bad = by["weights: negative, NaN, inf norm%d" % nm]
        w0 = bad["weights"].copy()
        w0[~(np.isfinite(w0) & (w0 > 0))] = 0.0
        assert (w0 == 0).sum() == 4
        _, _, rb, bb = run_consensus(lib, bad)
        _, _, r0, b0 = run_consensus(lib, with_options(bad, w0))
        assert rb.tobytes() == r0.tobytes() and bb.tolist() == b0.tolist()


def test_a_permutation_of_the_draws_permutes_the_outputs(lib):
    c = weight_cases()[1]                                            # positive weights, normalised
    B, n, T = c["B"], c["n"], c["T"]
    ids = c["ids"].reshape(B, -1, n)
    perm = np.array([3, 0, 4, 2, 1])
    p = make_case("permuted", ids[:, :, perm], T, c["id_end"], weights=c["weights"][:, perm], normalize=c["normalize"])
    _, dist, risk, _ = run_consensus(lib, c)
    dist_p, risk_p, _ = check_case(lib, p)
    assert np.array_equal(dist_p, dist[:, perm][:, :, perm])
    # the same terms in another order: the risks agree within twice the bound of one of them, and exactly without weights or normalisation
    assert (np.abs(risk_p.astype(np.float64) - risk[:, perm]) <= 2 * bound(n) * c["risk"][:, perm]).all()
    u = with_options(c, None, 0)
    _, _, ru, _ = run_consensus(lib, u)
    _, _, rpu, _ = run_consensus(lib, with_options(p, None, 0))
    assert rpu.tobytes() == np.ascontiguousarray(ru[:, perm]).tobytes()


def test_runs_repeat_and_the_edge_sizes(lib):
    c = matrix_cases()[-3]
    a, b = run_consensus(lib, c), run_consensus(lib, c)
    assert a[0] == b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    # B == 0: nothing launched, nothing written
    rc, dist, risk, best = run_consensus(lib, c, B=0)
    assert rc == 0 and (dist == -7).all() and (risk == -7).all()
    # T == 0 and n == 1: zeros
    for cc in (x for x in matrix_cases() if x["T"] == 0 or x["n"] == 1):
        rc, dist, risk, best = run_consensus(lib, cc)
        assert rc == 0 and not dist.any() and risk.tobytes() == np.zeros_like(risk).tobytes() and not best.any(), cc["name"]


def test_refusals(lib):
    c = end_cases()[0]
    z = ctypes.c_void_p(0)
    assert run_consensus(lib, c)[0] == 0
    for kw in (dict(ids=z), dict(dist=z), dict(risk=z), dict(best=z), dict(B=-1), dict(n=0), dict(n=-1), dict(n=MAX_N + 1), dict(T=-1), dict(T=LIMIT + 1),
               dict(image_stride=-1), dict(draw_stride=-1), dict(tok_stride=-1), dict(normalize=2), dict(normalize=-1)):
        outs = {}

        def call():
            rc, dist, risk, best = run_consensus(lib, c, **kw)
            outs.update(dist=dist, risk=risk, best=best)
            return rc
        assert call() == -1, kw
        assert lib.lxo_last_error().startswith(b"lxo_consensus") and all((v == -7).all() for v in outs.values()), kw
    assert run_consensus(lib, c, T=LIMIT + 1)[0] == -1 and b"column limit" in lib.lxo_last_error()
    # the limits themselves are taken: n = MAX_N and T = LIMIT run in the matrix
    assert any(x["n"] == MAX_N for x in matrix_cases()) and any(x["T"] == LIMIT for x in matrix_cases())
