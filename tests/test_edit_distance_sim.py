"""CPU (hipsim): lxo_edit_distance -- the batched Levenshtein kernel of csrc/seqcost.hip -- against the project's own levenshtein / truncate_end on the
case matrix of tests/edit_distance_ref.py, exactly (the distances as ints, the costs as bytes), and its -1 returns.  The same matrix runs on the
MI355X in tests/test_gpu_mrt_device.py."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from simlib import SIM_SO, build_sim
from edit_distance_ref import Host, LIMIT, check_edit_case, edit_cases, run_edit


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.mark.parametrize("i", range(len(edit_cases())), ids=[c["name"] for c in edit_cases()])
def test_edit_distance_matches_levenshtein(lib, i):
    check_edit_case(lib, edit_cases()[i])


def test_cost_is_optional_and_runs_repeat(lib):
    c = edit_cases()[4]
    _, d1, c1 = run_edit(lib, c)
    rc, d2, none = run_edit(lib, c, want_cost=False)
    assert rc == 0 and none is None and np.array_equal(d1, d2) and c1.tobytes() == c["cost"].tobytes()
    empty = dict(c, pairs=0)
    rc, d0, _ = run_edit(lib, empty)                                # no pair: nothing launched, nothing written
    assert rc == 0 and d0.size == 0


def test_refusals(lib):
    c = edit_cases()[1]
    p, z = Host.ptr, ctypes.c_void_p(0)
    hyp, ref, hl = c["hyp"], c["ref"], c["hyp_len"]
    dist = np.full(c["pairs"], -7, np.int32)
    T = c["T"]

    def call(hyp_p=p(hyp), ref_p=p(ref), dist_p=p(dist), block=1, bs=T, rs=0, ts=1, T=T, G=1, ref_ld=ref.shape[1], per_ref=c["per_ref"], pairs=c["pairs"]):
        return lib.lxo_edit_distance(hyp_p, block, bs, rs, ts, T, p(hl), ref_p, G, ref_ld, z, z, per_ref, pairs, -1, dist_p, z, None)

    assert call() == 0
    for kw in (dict(hyp_p=z), dict(ref_p=z), dict(dist_p=z), dict(pairs=-1), dict(T=-1), dict(G=-1), dict(G=0), dict(bs=-1), dict(ts=-1), dict(rs=-1),
               dict(block=0), dict(per_ref=0), dict(ref_ld=0), dict(ref_ld=LIMIT + 1)):
        dist[:] = -7
        assert call(**kw) == -1, kw
        assert lib.lxo_last_error() and (dist == -7).all(), kw
    # the limit itself is taken (the matrix runs it); one beyond is refused with the reason
    assert call(ref_ld=LIMIT + 1) == -1 and b"column limit" in lib.lxo_last_error()
    assert LIMIT >= 511
