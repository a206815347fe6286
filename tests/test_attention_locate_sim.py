"""CPU (hipsim): lxo_attention_locate -- csrc/attloc.hip -- against the float64 definition of tests/attention_locate_ref.py on its case matrix: peak,
box and S exact on the dyadic maps, edges valid within the f32 summation bound elsewhere, the stats within their derived bounds, the coverage bit
for bit; every output alone, a wider cov_ld, runs repeated, the refusals.  The same matrix runs on the MI355X in tests/test_gpu_attention_locate.py."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from simlib import SIM_SO, build_sim
from edit_distance_ref import Host
from attention_locate_ref import CASE_NAMES, LIMIT, MASSES, check_locate_case, coverage_ref, decided_share, named, run_locate


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


def test_the_reference_decides_the_random_edges():
    """the seeds of the matrix: at least 95 % of the non-dyadic maps' edges have a margin above the summation bound, so they are held to equality"""
    share = decided_share()
    print("edges decided by more than TOL: %.4f" % share)
    assert share >= 0.95


@pytest.mark.parametrize("name", CASE_NAMES)
def test_locations_match_the_definition(lib, name):
    check_locate_case(lib, named(name))


def test_each_output_alone_and_runs_repeat(lib):
    for name in ("3x5 TBR", "2x65 BTR", "14x62 BTR"):
        c = named(name)
        rc, full = run_locate(lib, c, 0.9)
        assert rc == 0
        for k in ("peak", "box", "stats", "coverage"):
            rc, one = run_locate(lib, c, 0.9, want=(k,))
            assert rc == 0 and list(one) == [k] and one[k].tobytes() == full[k].tobytes(), (name, k)
        for want in (("box", "coverage"), ("stats", "coverage")):    # the coverage launch reads "has a map" off whichever output there is
            rc, two = run_locate(lib, c, 0.9, want=want)
            assert rc == 0 and all(two[k].tobytes() == full[k].tobytes() for k in want), (name, want)
        rc, again = run_locate(lib, c, 0.9)
        assert rc == 0 and all(again[k].tobytes() == full[k].tobytes() for k in full), name
        rc, wide = run_locate(lib, c, 0.9, want=("coverage",), cov_ld=c["R"] + 5)      # cells behind R keep what they held
        assert rc == 0 and np.array_equal(wide["coverage"][:, :c["R"]], coverage_ref(c)) and (wide["coverage"][:, c["R"]:] == -7).all()


def test_no_rows_and_no_steps(lib):
    c = named("3x5 TBR")
    rc, got = run_locate(lib, c, 0.9, rows=0)
    assert rc == 0 and all((v == -7).all() for v in got.values())
    rc, got = run_locate(lib, c, 0.9, steps=0)                      # nothing per position; the coverage of a row without steps is zeros
    assert rc == 0 and all((got[k] == -7).all() for k in ("peak", "box", "stats")) and not got["coverage"].any()


def test_refusals_write_nothing(lib):
    c = named("3x5 BTR")
    z = None
    cases = [(-1, dict(alpha=z)), (-1, dict(mass=0.0)), (-1, dict(mass=-0.5)), (-1, dict(mass=1.0000001)), (-1, dict(mass=float("nan"))),
             (-1, dict(mass=float("inf"))), (-1, dict(ss=-1)), (-1, dict(rs=-1)), (-1, dict(rows=-1)), (-1, dict(steps=-1)), (-1, dict(alpha_rows=-1)),
             (-1, dict(cov_ld=c["R"] - 1)), (-1, dict(cov_ld=0)), (-5, dict(Hp=0)), (-5, dict(Wp=0)), (-5, dict(Hp=-3)), (-5, dict(Hp=LIMIT + 1, Wp=1)),
             (-5, dict(Hp=1 << 20, Wp=1 << 20)), (-5, dict(Hp=98, Wp=100))]
    for code, kw in cases:
        cov_ld = kw.pop("cov_ld", None)
        rc, got = run_locate(lib, c, kw.pop("mass", 0.9), cov_ld=cov_ld, **kw)
        assert rc == code and lib.lxo_last_error(), (code, kw)
        assert all((v == -7).all() for v in got.values()), kw        # nothing launched: every output as it was
    rc, got = run_locate(lib, c, 0.9, want=())
    assert rc == -1 and b"all NULL" in lib.lxo_last_error()
    assert run_locate(lib, c, 0.9, Hp=LIMIT + 1, Wp=1)[0] == -5 and b"staging limit" in lib.lxo_last_error()
    rc, got = run_locate(lib, c, 0.9, want=("peak",), cov_ld=0)     # cov_ld is not read without a coverage
    assert rc == 0
    assert LIMIT >= 98 * 98 and LIMIT == _abi.LXO_LOCATE_MAX_CELLS
    assert set(MASSES) == {1.0, 0.9, 0.5, 2.0 ** -20}
