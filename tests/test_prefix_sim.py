"""CPU (hipsim): lxo_greedy_decode_prefix / lxo_beam_decode_prefix -- decode from a given prefix -- against tests/prefix_ref.py (the oracle's
decode with forced steps), from the features the Sim's own decoder read (ws region "img"), as test_decode_scores_sim.py does.  Per-row
prefix lengths {0, 1, mid, max_iter}; with every length 0 the calls are bit-identical to lxo_greedy_decode_scores / lxo_beam_decode_scores."""
import ctypes
import os

import numpy as np
import pytest

from simharness import Sim, ptr
import prefix_ref

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_small.npz"))
SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, END, MAX_ITER, MS = 11, 10, 8, 9
B = 4
TOL = 1e-5
IMG = np.concatenate([GOLD["img"], GOLD["img"][::-1]], axis=0)          # 4 images (two distinct pairs)
LENS = np.array([0, 1, 4, MAX_ITER], np.int32)                          # none, one token, mid, the whole decode


def _torch_params(S):
    import torch
    return {k: torch.from_numpy(np.asarray(v)) for k, v in S.P.items()}


def _sim(beam=1, gamma=1.0, prob=0.0):
    S = Sim(B, 32, 48, 1, V, dtype=0, seed=0, beam=beam, max_steps=MS, dims=SMALL)
    if beam > 1:
        S.shape.div_gamma, S.shape.div_prob, S.shape.div_seed = gamma, prob, 4
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(IMG), None), "enc")
    from latex_ocr_amd.model.utils.image import encoder_out_hw
    Hp, Wp = encoder_out_hw(32, 48)
    S.enc = S.region("img", np.float32)[:B * Hp * Wp * SMALL["C"]].reshape(B, Hp * Wp, SMALL["C"]).copy()
    return S


def _prefix(seed=0):
    """ids in [0, V) without END; the forced tokens differ from the rows' greedy picks often enough to leave the greedy path"""
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray(rs.randint(0, END, size=(B, MAX_ITER)), np.int32)


def _greedy(S, pf, ln):
    ids = np.zeros((B, MS), np.int32); lp = np.zeros((B, MS), np.float32); steps = ctypes.c_int(0)
    S.ck(S.L.lxo_greedy_decode_prefix(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(pf), pf.shape[1], ptr(ln),
                                      ptr(ids), ptr(lp), None, ctypes.byref(steps), None), "greedy_prefix")
    return ids[:, :steps.value], lp[:, :steps.value]


def _beam(S, k, pf, ln):
    ids = np.zeros((B, MS, k), np.int32); par = np.zeros((B, MS, k), np.int32); sc = np.zeros((B, MS, k), np.float32)
    steps = ctypes.c_int(0)
    S.ck(S.L.lxo_beam_decode_prefix(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(pf), pf.shape[1], ptr(ln),
                                    ptr(ids), ptr(par), ptr(sc), None, ctypes.byref(steps), None), "beam_prefix")
    n = steps.value
    return ids[:, :n], par[:, :n], sc[:, :n]


def test_greedy_prefix_matches_the_reference():
    S = _sim()
    pf = _prefix()
    ids, lp = _greedy(S, pf, LENS)
    rid, rlp = prefix_ref.greedy_prefix(_torch_params(S), S.enc, END, pf, LENS, MAX_ITER)
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    for b in range(B):
        assert np.array_equal(ids[b, :LENS[b]], pf[b, :LENS[b]])
    assert ids.shape[1] == MAX_ITER + 1                                 # the row forced for max_iter steps keeps the loop to its bound
    assert np.abs(lp - rlp).max() < TOL, np.abs(lp - rlp).max()


@pytest.mark.parametrize("k,gamma,prob", [(2, 1.0, 0.0), (3, 0.5, 1.0), (4, 1.0, 0.0)])
def test_beam_prefix_matches_the_reference(k, gamma, prob):
    S = _sim(k, gamma, prob)
    pf = _prefix(1)
    ids, par, sc = _beam(S, k, pf, LENS)
    rid, rpar, rsc = prefix_ref.beam_prefix(_torch_params(S), S.enc, END, k, pf, LENS, MAX_ITER, gamma, prob, 4)
    assert ids.shape == rid.shape and np.array_equal(ids, rid) and np.array_equal(par, rpar), (ids, rid, par, rpar)
    for b in range(B):
        assert (ids[b, :LENS[b]] == pf[b, :LENS[b], None]).all()
        assert (par[b, :LENS[b]] == np.arange(k)).all()
    assert np.abs(sc - rsc).max() < TOL * max(1.0, np.abs(rsc).max()), np.abs(sc - rsc).max()


def test_greedy_empty_prefixes_are_bit_identical_to_the_scores_call():
    S = _sim()
    ids, lp = _greedy(S, _prefix(), np.zeros(B, np.int32))
    ids0 = np.zeros((B, MS), np.int32); lp0 = np.zeros((B, MS), np.float32); steps = ctypes.c_int(0)
    S.ck(S.L.lxo_greedy_decode_scores(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(ids0), ptr(lp0), None,
                                      ctypes.byref(steps), None), "greedy_scores")
    n = steps.value
    assert ids.shape[1] == n and np.array_equal(ids, ids0[:, :n]) and np.array_equal(lp.view(np.uint32), lp0[:, :n].view(np.uint32))


@pytest.mark.parametrize("k,gamma,prob", [(2, 1.0, 0.0), (3, 0.5, 1.0)])
def test_beam_empty_prefixes_are_bit_identical_to_the_scores_call(k, gamma, prob):
    S = _sim(k, gamma, prob)
    ids, par, sc = _beam(S, k, _prefix(), np.zeros(B, np.int32))
    ids0 = np.zeros((B, MS, k), np.int32); par0 = np.zeros((B, MS, k), np.int32); sc0 = np.zeros((B, MS, k), np.float32)
    steps = ctypes.c_int(0)
    S.ck(S.L.lxo_beam_decode_scores(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(ids0), ptr(par0), ptr(sc0), None,
                                    ctypes.byref(steps), None), "beam_scores")
    n = steps.value
    assert ids.shape[1] == n and np.array_equal(ids, ids0[:, :n]) and np.array_equal(par, par0[:, :n])
    assert np.array_equal(sc.view(np.uint32), sc0[:, :n].view(np.uint32))


def test_out_of_range_device_values_are_read_defensively():
    """a length beyond min(ld, max_iter) is clamped there, a negative one to 0, an id outside [0, V) reads as 0: nothing faults"""
    S = _sim()
    pf = _prefix(2)
    bad = pf.copy(); bad[0, 1] = -7; bad[2, 0] = V + 5
    ln = np.array([3, -4, 2, 1000], np.int32)
    ids, lp = _greedy(S, bad, ln)
    fixed = pf.copy(); fixed[0, 1] = 0; fixed[2, 0] = 0
    rid, rlp = prefix_ref.greedy_prefix(_torch_params(S), S.enc, END, fixed, np.array([3, 0, 2, MAX_ITER]), MAX_ITER)
    assert np.array_equal(ids, rid) and np.abs(lp - rlp).max() < TOL


def test_null_prefix_or_bad_ld_is_refused():
    S = _sim()
    pf, ln = _prefix(), LENS.copy()
    ids = np.zeros((B, MS), np.int32); steps = ctypes.c_int(0)
    args = lambda p, ld, l: (S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, p, ld, l, ptr(ids), None, None, ctypes.byref(steps), None)
    assert S.L.lxo_greedy_decode_prefix(*args(None, MAX_ITER, ptr(ln))) == -1
    assert S.L.lxo_greedy_decode_prefix(*args(ptr(pf), MAX_ITER, None)) == -1
    assert S.L.lxo_greedy_decode_prefix(*args(ptr(pf), 0, ptr(ln))) == -1
