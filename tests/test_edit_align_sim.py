"""CPU (hipsim): lxo_edit_align -- the edit alignment of csrc/seqcost.hip -- against the full-table reference of tests/edit_align_ref.py on its case
matrix, as integers: maps, counts, corpus row, confusion matrix; the tie-break-independent validity checks on the kernel's output; its S + I + D
against lxo_edit_distance on the same arguments; accumulate, every output alone, repeat runs, guard words, the -1 returns and the size function.  The
same matrix runs on the MI355X in tests/test_gpu_edit_align.py."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from simlib import SIM_SO, build_sim
from edit_distance_ref import Host, run_edit
from edit_align_ref import CASE_NAMES, LIMIT, NA, NC, check_align_case, confusion_of, corpus_of, named, run_align


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_alignment_matches_the_table_reference(lib, name):
    c = named(name)
    got = check_align_case(lib, c)
    rc, dist, _ = run_edit(lib, c, want_cost=False)                 # the same arguments through lxo_edit_distance
    assert rc == 0 and np.array_equal(got["counts"][:, 1:4].sum(1), dist)


def _half_confusion(c, lo, hi):
    conf, out = confusion_of(c["cut"][lo:hi], c["maps"][lo:hi], c["V"])
    return conf, corpus_of(c["counts"][lo:hi], out)


@pytest.mark.parametrize("per_pair", [True, False])
def test_accumulate_over_two_halves_equals_one_call(lib, per_pair):
    c = named("END, lengths")
    half, nconf = c["pairs"] // 2, (c["V"] + 1) ** 2
    want = ("hyp_align", "ref_align", "counts") if per_pair else ()
    conf1, corp1 = _half_confusion(c, 0, half)
    rc, a = run_align(lib, c, want=want, corpus=np.full(NC, 99, np.int64), confusion=np.full(nconf, 99, np.int64), accumulate=0, hi=half)      # overwrites
    assert rc == 0 and a["corpus"].tolist() == corp1.tolist() and a["confusion"].tolist() == conf1.tolist()
    rc, b = run_align(lib, c, want=want, corpus=a["corpus"], confusion=a["confusion"], accumulate=1, lo=half)
    assert rc == 0 and b["corpus"].tolist() == c["corpus"].tolist() and b["confusion"].tolist() == c["confusion"].tolist()
    if per_pair:
        for k in want:
            assert np.array_equal(np.concatenate([a[k], b[k]]), c[k]), k
    rc, d = run_align(lib, c, want=want, corpus=b["corpus"], confusion=b["confusion"], accumulate=1)          # and once more on top: twice the sums
    assert rc == 0 and d["corpus"].tolist() == (2 * c["corpus"]).tolist() and d["confusion"].tolist() == (2 * c["confusion"]).tolist()
    # no pair: zeroed or left alone, nothing else written
    rc, z = run_align(lib, c, want=want, corpus=np.full(NC, 5, np.int64), confusion=np.full(nconf, 5, np.int64), accumulate=0, hi=0)
    assert rc == 0 and not z["corpus"].any() and not z["confusion"].any()
    rc, z = run_align(lib, c, want=want, corpus=np.full(NC, 5, np.int64), confusion=np.full(nconf, 5, np.int64), accumulate=1, hi=0)
    assert rc == 0 and (z["corpus"] == 5).all() and (z["confusion"] == 5).all()


def test_each_output_alone_and_runs_repeat(lib):
    for name in ("ref 129", "strided [B, T, n]", "tokens outside [0, V)"):
        c = named(name)
        nconf = (c["V"] + 1) ** 2
        rc, full = run_align(lib, c, corpus=np.zeros(NC, np.int64), confusion=np.zeros(nconf, np.int64))
        assert rc == 0
        for k in ("hyp_align", "ref_align", "counts"):
            rc, one = run_align(lib, c, want=(k,))
            assert rc == 0 and list(one) == [k] and np.array_equal(one[k], c[k]), (name, k)
        rc, one = run_align(lib, c, want=(), corpus=np.full(NC, -7, np.int64))
        # (without a matrix nothing is left out of one)
        assert rc == 0 and list(one) == ["corpus"] and one["corpus"].tolist() == c["corpus"][:7].tolist() + [0]
        rc, one = run_align(lib, c, want=(), confusion=np.full(nconf, -7, np.int64))
        assert rc == 0 and list(one) == ["confusion"] and one["confusion"].tolist() == c["confusion"].tolist()
        rc, again = run_align(lib, c, corpus=np.zeros(NC, np.int64), confusion=np.zeros(nconf, np.int64))
        assert rc == 0 and all(again[k].tobytes() == full[k].tobytes() for k in full), name


def test_refusals_write_nothing(lib):
    c = named("V = 1")
    p, z = Host.ptr, ctypes.c_void_p(0)
    hyp, ref, hl, rl = c["hyp"], c["ref"], c["hyp_len"], c["ref_len"]
    T, ld, n = c["T"], ref.shape[1], c["pairs"]
    outs = [np.full((n, T), -7, np.int32), np.full((n, ld), -7, np.int32), np.full((n, NA), -7, np.int32), np.full(NC, -7, np.int64), np.full(4, -7, np.int64)]
    need = lib.lxo_edit_align_scratch_bytes(n, T, ld)
    sc = np.full(need, 0xF9, np.uint8)
    none = dict(ha=z, ra=z, cn=z, co=z, cf=z)

    def call(hyp_p=p(hyp), ref_p=p(ref), ha=p(outs[0]), ra=p(outs[1]), cn=p(outs[2]), co=p(outs[3]), cf=p(outs[4]), block=1, bs=T, rs=0, ts=1, T=T, G=n, ref_ld=ld,
             per_ref=1, pairs=n, V=1, acc=0, sc_p=p(sc), sc_n=need):
        return lib.lxo_edit_align(hyp_p, block, bs, rs, ts, T, p(hl), ref_p, G, ref_ld, p(rl), z, per_ref, pairs, -1, ha, ra, cn, co, cf, V, acc, sc_p, sc_n, None)

    assert call() == 0 and np.array_equal(outs[0], c["hyp_align"]) and np.array_equal(outs[2], c["counts"]) and outs[4].tolist() == c["confusion"].tolist()
    for kw in (dict(hyp_p=z), dict(ref_p=z), none, dict(pairs=-1), dict(T=-1), dict(T=LIMIT + 1), dict(G=-1), dict(G=0), dict(bs=-1), dict(ts=-1), dict(rs=-1),
               dict(block=0), dict(per_ref=0), dict(ref_ld=0), dict(ref_ld=LIMIT + 1), dict(acc=2), dict(acc=-1), dict(V=0), dict(V=-3), dict(sc_p=z),
               dict(sc_n=need - 1), dict(sc_n=0)):
        for o in outs:
            o[...] = -7
        sc[:] = 0xF9
        assert call(**kw) == -1, kw
        assert lib.lxo_last_error() and all((o == -7).all() for o in outs) and (sc == 0xF9).all(), kw
    assert call(T=LIMIT + 1) == -1 and b"staging limit" in lib.lxo_last_error()
    assert call(ref_ld=LIMIT + 1) == -1 and b"column limit" in lib.lxo_last_error()
    assert call(sc_n=need - 1) == -1 and b"scratch" in lib.lxo_last_error()
    # V is not read without a matrix, the scratch not without a row of the table
    assert call(cf=z, V=0) == 0
    assert call(pairs=0, sc_p=z, sc_n=0) == 0
    h0 = np.zeros(1, np.int32)
    assert call(hyp_p=p(h0), T=0, bs=0, sc_p=z, sc_n=0, ha=z) == 0 and outs[2][:, 4].tolist() == [0] * n and np.array_equal(outs[2][:, 3], outs[2][:, 5])


def test_the_size_function(lib):
    f = lib.lxo_edit_align_scratch_bytes
    assert f(0, 10, 10) == 0 and f(10, 0, 10) == 0
    grid = [(pairs, T, ld) for pairs in (1, 2, 7, 320) for T in (1, 2, 63, 64, 65, 152, LIMIT) for ld in (1, 64, 65, 128, 129, 256, 257, 512, 513, LIMIT)]
    for pairs, T, ld in grid:
        v = f(pairs, T, ld)
        assert 0 < v <= pairs * T * 256, (pairs, T, ld, v)
        assert f(pairs + 1, T, ld) >= v and f(pairs, T + 1 if T < LIMIT else T, ld) >= v and f(pairs, T, min(ld + 1, LIMIT)) >= v
