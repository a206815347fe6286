"""CPU (hipsim): lxo_greedy_decode_constrained / lxo_beam_decode_constrained -- decode under per-image allowed-token sets -- against
tests/constraint_ref.py (the oracle's decode with banned columns at -inf), from the features the Sim's own decoder read (ws region "img"), as
test_prefix_sim.py does.  The sets bite: row 0 allows everything, every other row bans its own unconstrained first pick.  With every token
allowed the calls are bit-identical to lxo_*_decode_prefix / lxo_*_decode_scores."""
import ctypes
import os

import numpy as np
import pytest

from simharness import Sim, ptr
import constraint_ref
import prefix_ref

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_small.npz"))
SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, END, MAX_ITER, MS = 11, 10, 8, 9
B = 4
TOL = 1e-5                                                              # test_prefix_sim.py's bound
IMG = np.concatenate([GOLD["img"], GOLD["img"][::-1]], axis=0)          # 4 images (two distinct pairs)
LENS = np.array([0, 1, 4, MAX_ITER], np.int32)                          # none, one token, mid, the whole decode
FULL = np.ones((B, V), bool)


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


def _greedy(S, bits, ld, pf=None, ln=None):
    """-> (return code, ids, logp); bits None / ld as given: the refusals"""
    ids = np.zeros((B, MS), np.int32); lp = np.zeros((B, MS), np.float32); steps = ctypes.c_int(0)
    pa = (ptr(pf), pf.shape[1], ptr(ln)) if pf is not None else (None, 0, None)
    rc = S.L.lxo_greedy_decode_constrained(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER,
                                           ptr(bits) if bits is not None else None, ld, *pa,
                                           ptr(ids), ptr(lp), None, ctypes.byref(steps), None)
    return rc, ids[:, :steps.value], lp[:, :steps.value]


def _beam(S, k, bits, ld, pf=None, ln=None):
    ids = np.zeros((B, MS, k), np.int32); par = np.zeros((B, MS, k), np.int32); sc = np.zeros((B, MS, k), np.float32)
    steps = ctypes.c_int(0)
    pa = (ptr(pf), pf.shape[1], ptr(ln)) if pf is not None else (None, 0, None)
    rc = S.L.lxo_beam_decode_constrained(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER,
                                         ptr(bits) if bits is not None else None, ld, *pa,
                                         ptr(ids), ptr(par), ptr(sc), None, ctypes.byref(steps), None)
    n = steps.value
    return rc, ids[:, :n], par[:, :n], sc[:, :n]


def _sets(first, seed=0, banned_extra=()):
    """Row 0: everything allowed.  Every other row: a random subset with its own unconstrained first pick `first[b]` banned, END allowed and at
    least 4 tokens allowed.  banned_extra: ids kept allowed in every row (a prefix's tokens)."""
    rs = np.random.RandomState(seed)
    al = rs.rand(B, V) < 0.6
    for b in range(B):
        al[b, list(banned_extra)] = True
        al[b, first[b]] = False
        al[b, END] = True
        free = [v for v in range(V) if not al[b, v] and v != first[b]]
        while al[b].sum() < 4:
            al[b, free.pop()] = True
    al[0] = True
    assert (al.sum(1) >= 4).all() and al[:, END].all() and not al[np.arange(1, B), first[1:]].any()
    return al


def _all_allowed(ids, al):
    """every emitted id lies in its row's set (ids [B, T] or [B, T, k])"""
    return all(al[b][ids[b].reshape(-1)].all() for b in range(B))


def test_greedy_constrained_matches_the_reference():
    S = _sim()
    rc, ids0, _ = _greedy(S, constraint_ref.pack_bits(FULL), 1)
    assert rc == 0
    al = _sets(ids0[:, 0])
    bits = constraint_ref.pack_bits(al)
    rc, ids, lp = _greedy(S, bits, bits.shape[1])
    assert rc == 0
    rid, rlp, _ = constraint_ref.greedy_constrained(_torch_params(S), S.enc, END, al, MAX_ITER)
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    assert _all_allowed(ids, al)
    for b in range(1, B):                                               # the constraint binds: otherwise the comparison shows nothing
        n = min(ids.shape[1], ids0.shape[1])
        assert ids.shape[1] != ids0.shape[1] or not np.array_equal(ids[b, :n], ids0[b, :n]), b
        assert ids[b, 0] != ids0[b, 0]
    assert np.isfinite(lp).all() and np.abs(lp - rlp).max() < TOL, np.abs(lp - rlp).max()


@pytest.mark.parametrize("k,gamma,prob", [(2, 1.0, 0.0), (3, 0.5, 1.0), (4, 1.0, 0.0)])
def test_beam_constrained_matches_the_reference(k, gamma, prob):
    S = _sim(k, gamma, prob)
    rc, ids0, par0, _ = _beam(S, k, constraint_ref.pack_bits(FULL), 1)
    assert rc == 0
    al = _sets(ids0[:, 0, 0])                                           # slot 0's first token: the image's best first pick
    bits = constraint_ref.pack_bits(al)
    rc, ids, par, sc = _beam(S, k, bits, bits.shape[1])
    assert rc == 0
    rid, rpar, rsc = constraint_ref.beam_constrained(_torch_params(S), S.enc, END, k, al, MAX_ITER, gamma, prob, 4)
    assert ids.shape == rid.shape and np.array_equal(ids, rid) and np.array_equal(par, rpar), (ids, rid, par, rpar)
    assert _all_allowed(ids, al)
    for b in range(1, B):
        assert ids.shape[1] != ids0.shape[1] or not np.array_equal(ids[b], ids0[b]), b
        assert (ids[b, 0] != ids0[b, 0, 0]).all()
    assert np.isfinite(sc).all()
    assert np.abs(sc - rsc).max() < TOL * max(1.0, np.abs(rsc).max()), np.abs(sc - rsc).max()


def _prefix(seed=0):
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray(rs.randint(0, END, size=(B, MAX_ITER)), np.int32)


def test_sets_combine_with_prefix_lengths():
    """sets + prefix lengths {0, 1, mid, max_iter}: no forced token is banned in its row; the first FREE pick of the unconstrained completion is"""
    S = _sim()
    pf = _prefix()
    P = _torch_params(S)
    uid, _ = prefix_ref.greedy_prefix(P, S.enc, END, pf, LENS, MAX_ITER)
    first_free = np.array([uid[b, min(LENS[b], uid.shape[1] - 1)] for b in range(B)])
    al = np.ones((B, V), bool)
    for b in (1, 2):                                                    # rows 0 (no prefix) and 3 (forced to the bound) stay unconstrained
        al[b, first_free[b]] = False
        al[b, END] = True
        al[b, pf[b, :LENS[b]]] = True
    bits = constraint_ref.pack_bits(al)
    rc, ids, lp = _greedy(S, bits, bits.shape[1], pf, LENS)
    assert rc == 0
    rid, rlp, _ = constraint_ref.greedy_constrained(P, S.enc, END, al, MAX_ITER, pf, LENS)
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    assert _all_allowed(ids, al)
    for b in range(B):
        assert np.array_equal(ids[b, :LENS[b]], pf[b, :LENS[b]])
    for b in (1, 2):
        if first_free[b] != END and not (pf[b, :LENS[b]] == first_free[b]).any():
            assert ids[b, LENS[b]] != uid[b, LENS[b]], b
    assert np.abs(lp - rlp).max() < TOL, np.abs(lp - rlp).max()
    k = 3
    Sb = _sim(k, 0.5, 1.0)
    alb = al.copy()
    rc, bid, bpar, bsc = _beam(Sb, k, constraint_ref.pack_bits(alb), bits.shape[1], pf, LENS)
    assert rc == 0
    rid, rpar, rsc = constraint_ref.beam_constrained(_torch_params(Sb), Sb.enc, END, k, alb, MAX_ITER, 0.5, 1.0, 4, pf, LENS)
    assert np.array_equal(bid, rid) and np.array_equal(bpar, rpar) and _all_allowed(bid, alb)
    assert np.abs(bsc - rsc).max() < TOL * max(1.0, np.abs(rsc).max())


def test_reference_with_every_token_allowed_equals_prefix_ref():
    S = _sim()
    P = _torch_params(S)
    pf, zero = _prefix(), np.zeros(B, np.int32)
    i0, l0, _ = constraint_ref.greedy_constrained(P, S.enc, END, FULL, MAX_ITER)
    i1, l1 = prefix_ref.greedy_prefix(P, S.enc, END, pf, zero, MAX_ITER)
    assert np.array_equal(i0, i1) and np.array_equal(l0, l1)
    for k, g, pr in [(2, 1.0, 0.0), (3, 0.5, 1.0), (3, 4.0, 1.0)]:
        a = constraint_ref.beam_constrained(P, S.enc, END, k, FULL, MAX_ITER, g, pr, 4)
        b = prefix_ref.beam_prefix(P, S.enc, END, k, pf, zero, MAX_ITER, g, pr, 4)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_greedy_every_token_allowed_is_bit_identical():
    S = _sim()
    full = constraint_ref.pack_bits(FULL)
    rc, ids, lp = _greedy(S, full, full.shape[1])
    assert rc == 0
    ids0 = np.zeros((B, MS), np.int32); lp0 = np.zeros((B, MS), np.float32); steps = ctypes.c_int(0)
    S.ck(S.L.lxo_greedy_decode_scores(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(ids0), ptr(lp0), None,
                                      ctypes.byref(steps), None), "greedy_scores")
    n = steps.value
    assert ids.shape[1] == n and np.array_equal(ids, ids0[:, :n]) and np.array_equal(lp.view(np.uint32), lp0[:, :n].view(np.uint32))
    pf = _prefix()
    rc, ids, lp = _greedy(S, full, full.shape[1], pf, LENS)
    assert rc == 0
    ids0[:] = 0; lp0[:] = 0
    S.ck(S.L.lxo_greedy_decode_prefix(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(pf), pf.shape[1], ptr(LENS),
                                      ptr(ids0), ptr(lp0), None, ctypes.byref(steps), None), "greedy_prefix")
    n = steps.value
    assert ids.shape[1] == n and np.array_equal(ids, ids0[:, :n]) and np.array_equal(lp.view(np.uint32), lp0[:, :n].view(np.uint32))


@pytest.mark.parametrize("k,gamma,prob", [(2, 1.0, 0.0), (3, 0.5, 1.0)])
def test_beam_every_token_allowed_is_bit_identical(k, gamma, prob):
    S = _sim(k, gamma, prob)
    full = constraint_ref.pack_bits(FULL)
    pf = _prefix(1)
    for with_prefix in (False, True):
        rc, ids, par, sc = _beam(S, k, full, full.shape[1], *((pf, LENS) if with_prefix else ()))
        assert rc == 0
        ids0 = np.zeros((B, MS, k), np.int32); par0 = np.zeros((B, MS, k), np.int32); sc0 = np.zeros((B, MS, k), np.float32)
        steps = ctypes.c_int(0)
        if with_prefix:
            S.ck(S.L.lxo_beam_decode_prefix(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(pf), pf.shape[1], ptr(LENS),
                                            ptr(ids0), ptr(par0), ptr(sc0), None, ctypes.byref(steps), None), "beam_prefix")
        else:
            S.ck(S.L.lxo_beam_decode_scores(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(ids0), ptr(par0), ptr(sc0), None,
                                            ctypes.byref(steps), None), "beam_scores")
        n = steps.value
        assert ids.shape[1] == n and np.array_equal(ids, ids0[:, :n]) and np.array_equal(par, par0[:, :n])
        assert np.array_equal(sc.view(np.uint32), sc0[:, :n].view(np.uint32))


def test_shared_set_equals_copies_of_the_row():
    """allow_ld = 0: one set for every image = B copies of the same row"""
    S = _sim()
    row = np.ones(V, bool); row[[1, 4, 7]] = False
    one = constraint_ref.pack_bits(row)
    rc, ids, lp = _greedy(S, one, 0)
    rc2, ids2, lp2 = _greedy(S, np.ascontiguousarray(np.repeat(one, B, axis=0)), one.shape[1])
    assert rc == 0 and rc2 == 0
    assert np.array_equal(ids, ids2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32))
    assert not np.isin(ids, [1, 4, 7]).any()
    Sb = _sim(2)
    a = _beam(Sb, 2, one, 0)
    b = _beam(Sb, 2, np.ascontiguousarray(np.repeat(one, B, axis=0)), one.shape[1])
    assert a[0] == 0 and b[0] == 0 and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[1:], b[1:]))
    assert not np.isin(a[1], [1, 4, 7]).any()


def test_a_wider_row_stride_and_bits_beyond_v_are_ignored():
    S = _sim()
    al = _sets(np.zeros(B, np.int64), seed=3)
    tight = constraint_ref.pack_bits(al)
    wide = constraint_ref.pack_bits(al, ld=3)
    wide[:, 0] |= np.uint32(0xFFFFFFFF) << np.uint32(V)                 # bits at or beyond V
    wide[:, 1:] = 0xFFFFFFFF
    a = _greedy(S, tight, 1)
    b = _greedy(S, wide, 3)
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def test_null_set_or_short_ld_is_refused():
    S = _sim()
    full = constraint_ref.pack_bits(FULL)
    assert _greedy(S, None, 1)[0] == -1
    assert _greedy(S, None, 0)[0] == -1
    assert _greedy(S, full, -1)[0] == -1
    Sb = _sim(2)
    assert _beam(Sb, 2, None, 1)[0] == -1
    pf = _prefix()
    ids = np.zeros((B, MS), np.int32); steps = ctypes.c_int(0)                # half a prefix: refused
    assert S.L.lxo_greedy_decode_constrained(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(full), 1, ptr(pf), MAX_ITER, None,
                                             ptr(ids), None, None, ctypes.byref(steps), None) == -1
    # 0 < allow_ld < (V + 31) / 32 needs V > 32
    S2 = Sim(B, 32, 48, 1, 40, dtype=0, seed=0, beam=1, max_steps=MS, dims=SMALL)
    S2.ck(S2.L.lxo_encoder_fwd(S2.sref(), ptr(S2.params), ptr(S2.wpack), ptr(S2.ws), ptr(IMG), None), "enc")
    bits = np.full((B, 2), 0xFFFFFFFF, np.uint32)
    args = lambda ld: (S2.sref(), ptr(S2.params), ptr(S2.wpack), ptr(S2.ws), 39, MAX_ITER, ptr(bits), ld, None, 0, None,
                       ptr(ids), None, None, ctypes.byref(steps), None)
    assert S2.L.lxo_greedy_decode_constrained(*args(1)) == -1
    assert S2.L.lxo_greedy_decode_constrained(*args(2)) == 0


def test_an_empty_set_returns_without_a_fault():
    """a row that breaks the contract (nothing allowed) must not fault or hang; the other rows decode as the reference does"""
    S = _sim()
    al = FULL.copy(); al[2] = False
    bits = constraint_ref.pack_bits(al)
    rc, ids, lp = _greedy(S, bits, 1)
    assert rc == 0 and ids.shape[1] >= 1 and ((ids >= 0) & (ids < V)).all()
    rc0, ids0, lp0 = _greedy(S, constraint_ref.pack_bits(FULL), 1)
    n = min(ids.shape[1], ids0.shape[1])
    for b in (0, 1, 3):
        assert np.array_equal(ids[b, :n], ids0[b, :n])
    Sb = _sim(2)
    rc, bid, bpar, bsc = _beam(Sb, 2, bits, 1)
    assert rc == 0 and ((bid >= 0) & (bid < V)).all() and ((bpar >= 0) & (bpar < 2)).all()
