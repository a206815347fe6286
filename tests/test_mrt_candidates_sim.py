"""CPU (hipsim): lxo_mrt_candidates -- the candidate rows of a minimum-risk step built on the device -- on CONSTRUCTED ids, so that every case is
certain to occur (tests/edit_distance_ref.py: constructed_ids), against the host construction of Img2SeqModel.mrt_batch, exactly."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from simlib import SIM_SO, build_sim
from edit_distance_ref import CAND_END, CAND_PAD, CAND_REFS, Host, LIMIT, cand_calls, check_candidates, constructed_ids, run_candidates


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.mark.parametrize("steps,inc", cand_calls())
def test_candidates_match_the_host_construction(lib, steps, inc):
    ids = constructed_ids()
    out = run_candidates(lib, ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc)
    assert out[0] == 0, lib.lxo_last_error()
    sizes = check_candidates(ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc, *out[1:])
    if steps == 6:
        # image 0: two equal draws are one, the draw equal to the reference joins it (or stands alone without it), the draw without END stays whole;
        # image 1: all draws equal; image 2: the two empty draws are one candidate of length 1 (its END)
        assert sizes.tolist() == ([3, 2, 3] if inc else [3, 1, 3])
        cand, cand_len = out[1], out[2]
        assert cand_len[2] == 7 and CAND_END not in cand[2, :6].tolist()          # six tokens, then the END the row gets
        first_empty = int(np.cumsum(sizes)[1]) + inc
        assert cand_len[first_empty] == 1 and cand[first_empty, 0] == CAND_END
    # the same bytes again: integer kernels, no atomics
    again = run_candidates(lib, ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[1:], again[1:]))


def test_a_single_image_and_no_image(lib):
    ids = constructed_ids()[2:3]
    out = run_candidates(lib, ids, 6, CAND_REFS[2:3], CAND_END, CAND_PAD, 1)
    assert out[0] == 0
    assert check_candidates(ids, 6, CAND_REFS[2:3], CAND_END, CAND_PAD, 1, *out[1:]).tolist() == [3]
    off = np.full(1, -7, np.int32)
    one = np.zeros(8, np.int32)
    assert lib.lxo_mrt_candidates(Host.ptr(one), 0, 8, 4, 6, Host.ptr(one), 6, Host.ptr(one), CAND_END, CAND_PAD, 1, Host.ptr(one), Host.ptr(one),
                                  Host.ptr(one.view(np.float32)), Host.ptr(off), Host.ptr(one), None) == 0
    assert off[0] == 0


def test_refusals(lib):
    a = np.zeros(64, np.int32)
    p, z = Host.ptr(a), ctypes.c_void_p(0)
    good = [p, 1, 8, 4, 6, p, 6, p, CAND_END, CAND_PAD, 1, p, p, p, p, p, None]
    for i, v in ((0, z), (5, z), (7, z), (11, z), (12, z), (13, z), (14, z), (15, z), (1, -1), (3, 0), (3, 17), (4, -1), (4, 9), (6, 0), (6, LIMIT + 1), (8, -1)):
        bad = list(good)
        bad[i] = v
        assert lib.lxo_mrt_candidates(*bad) == -1, (i, v)
        assert lib.lxo_last_error()
    assert not a.any()
