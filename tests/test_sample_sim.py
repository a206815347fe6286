"""CPU (hipsim): lxo_sample_tokens / lxo_sample_decode -- temperature, top-k and top-p draws -- against tests/sample_ref.py (the float64
restatement of the definition in head_kernels.h).  One criterion everywhere: a kernel token that differs from the reference's must have a reference
perturbed score within the reference's near-tie bound of the reference's best; at most 0.1 % of the compared draws may differ at all."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from latex_ocr_amd import _abi
from simharness import Sim, lib, ptr
import constraint_ref
import sample_ref

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_small.npz"))
SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, END, MAX_ITER, MS = 11, 10, 8, 9
B = 4
TOL = 1e-5
IMG = np.concatenate([GOLD["img"], GOLD["img"][::-1]], axis=0)
LENS = np.array([0, 1, 4, MAX_ITER], np.int32)

# (V, ld): ld % 4 == 0 and ld <= 1024 takes the register row (KV = 4 up to 256, 8 up to 512, 16 up to 1024), anything else the strided row
SHAPES = [(5, 8), (5, 5), (11, 12), (11, 11), (64, 64), (65, 68), (65, 65), (500, 512), (500, 500), (501, 501),
          (256, 256), (258, 260), (512, 512), (514, 516), (1024, 1024), (1026, 1028), (1026, 1026)]
TAUS, PS = (0.5, 1.0, 2.0), (1.0, 0.9, 0.5)


def opts(tau=1.0, top_k=0, top_p=1.0, seed=0):
    return _abi.LxoSampleOpts(tau, top_k, top_p, seed)


def tokens(lg, Vn, n, t, o, allow=None, want=(True, True)):
    """lxo_sample_tokens on logits [rows, ld] -> (rc, ids, logp, logq)"""
    rows = lg.shape[0]
    ids = np.full(rows, -7, np.int32); lp = np.zeros(rows, np.float32); lq = np.zeros(rows, np.float32)
    bits = constraint_ref.pack_bits(allow) if allow is not None else None
    rc = lib().lxo_sample_tokens(ptr(lg), lg.shape[1], rows, n, Vn, t, ctypes.byref(o), ptr(bits), 0 if bits is None or bits.shape[0] == 1 else bits.shape[1],
                                 ptr(ids), ptr(lp) if want[0] else None, ptr(lq) if want[1] else None, None)
    return rc, ids, lp, lq


def logits_for(Vn, ld, rows, scale, seed):
    rs = np.random.RandomState(seed)
    lg = np.full((rows, ld), 1.0e30, np.float32)                           # the padding must never be read as a column
    lg[:, :Vn] = (rs.randn(rows, Vn) * scale).astype(np.float32)
    return lg


def sets_for(Vn, images, seed):
    """image 0: everything, image 1: only END = V - 1, the others: random sets of at least two tokens with END"""
    rs = np.random.RandomState(seed)
    al = rs.rand(images, Vn) < 0.6
    al[:, Vn - 1] = True; al[:, 0] = True
    al[0] = True
    if images > 1:
        al[1] = False; al[1, Vn - 1] = True
    return al


def case_for(Vn, ld, rows, scale, lseed, n, t, tau, K, p, seed, allow):
    """logits and their reference picks; with top-p on, logits whose cumulative mass stays clear of p at every column (the next seed until it does)"""
    lg = logits_for(Vn, ld, rows, scale, lseed)
    for k in range(200):
        ref = sample_ref.sample_tokens(lg[:, :Vn], n, t, tau, K, p, seed, allow)
        close = [r for r, q in enumerate(ref) if q.margin <= 2e-4]
        if not close:
            return lg, ref
        for r in close:                                                    # another row in its place
            lg[r, :Vn] = (np.random.RandomState(lseed + 1000 * (k + 1) + r).randn(Vn) * scale).astype(np.float32)
    raise AssertionError("no logits clear of p")


def check_rows(Vn, p, ref, got, stats):
    """the criterion, logp / logq on the agreeing draws, and -- with top-p on -- the reference's margin"""
    rc, ids, lp, lq = got
    assert rc == 0
    for r, q in enumerate(ref):
        assert 0 <= ids[r] < Vn
        if p < 1.0:
            assert q.margin > 1e-4, ("the test's own case: cumulative mass too close to p", r, q.margin)
        assert q.cand[ids[r]], ("token outside the reference set", r, ids[r], np.nonzero(q.cand)[0])
        stats[0] += 1
        if ids[r] != q.id:
            stats[1] += 1
            assert sample_ref.flip_ok(q, int(ids[r])), (r, ids[r], q.id, q.score[ids[r]], q.score[q.id], q.tol)
            continue
        assert abs(lp[r] - q.logp) < TOL * max(1.0, abs(q.logp)), (r, lp[r], q.logp)
        assert abs(lq[r] - q.logq) < TOL, (r, lq[r], q.logq)


@pytest.mark.parametrize("Vn,ld", SHAPES)
def test_tokens_match_the_reference(Vn, ld):
    n, images = 3, 3
    rows = n * images
    stats = [0, 0]
    Ks = (0, 1, 3, Vn)
    full = Vn <= 65                                                        # the whole option grid on the small rows, one option varied at a time on the wide ones
    combos = list(itertools.product(TAUS, Ks, PS)) if full else \
        [(1.0, 0, 1.0)] + [(t, 0, 1.0) for t in TAUS[::2]] + [(1.0, k, 1.0) for k in Ks[1:]] + [(1.0, 0, p) for p in PS[1:]] + [(2.0, Vn // 3, 0.9), (0.5, 3, 0.5)]
    for ci, (tau, K, p) in enumerate(combos):
        for with_sets in (False, True):
            al = sets_for(Vn, images, ci) if with_sets else None
            lg, ref = case_for(Vn, ld, rows, (1.0, 5.0, 30.0)[ci % 3], 100 + ci, n, 3 + ci, tau, K, p, 7 + ci, al)
            got = tokens(lg, Vn, n, 3 + ci, opts(tau, K, p, 7 + ci), al)
            check_rows(Vn, p, ref, got, stats)
            if with_sets:
                assert (got[1][n:2 * n] == Vn - 1).all()                   # the image that allows only END
    print("draws compared %d, differing %d" % tuple(stats))
    assert stats[1] <= 1e-3 * stats[0]


def test_a_base_that_is_not_16_byte_aligned_takes_the_strided_row():
    """ld % 4 == 0 but the logits start 4 bytes into a 16-byte line: the launcher must not take the register row's 16-byte loads; same results"""
    for Vn, ld in [(11, 12), (500, 512)]:
        lg = logits_for(Vn, ld, 6, 2.0, 9)
        flat = np.zeros(lg.size + 8, np.float32)
        off = next(o for o in range(1, 5) if (flat.ctypes.data + 4 * o) % 16 == 4)
        shifted = flat[off:off + lg.size].reshape(lg.shape)
        shifted[:] = lg
        assert shifted.ctypes.data % 16 == 4 and lg.ctypes.data % 16 == 0
        al = sets_for(Vn, 2, 3)
        for o in (opts(1.0, 0, 1.0, 5), opts(0.5, 4, 0.9, 5)):
            a = tokens(lg, Vn, 3, 2, o, al); b = tokens(shifted, Vn, 3, 2, o, al)
            assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1])
            assert np.abs(a[2] - b[2]).max() < TOL and np.abs(a[3] - b[3]).max() < TOL


def test_top_k_1_is_the_arg_max():
    for Vn, ld in SHAPES:
        lg = logits_for(Vn, ld, 6, 3.0, Vn)
        lg[0, 1] = lg[0, 3] = lg[0, :Vn].max() + 1.0                       # a tie: the lower column
        al = sets_for(Vn, 2, 5)
        for tau in TAUS:
            rc, ids, lp, lq = tokens(lg, Vn, 3, 0, opts(tau, 1, 1.0, 3))
            assert rc == 0 and np.array_equal(ids, lg[:, :Vn].argmax(1)) and ids[0] == 1 and (lq == 0).all()
            rc, ids, _, _ = tokens(lg, Vn, 3, 0, opts(tau, 1, 0.5, 3), al)
            masked = np.where(np.repeat(al, 3, axis=0), lg[:, :Vn], -np.inf)
            assert rc == 0 and np.array_equal(ids, masked.argmax(1))


_SIMS = {}


def _sim(n=1):
    """one Sim per n for the module (the encoder runs once; every decode call sets its own state up)"""
    if n not in _SIMS:
        _SIMS[n] = _new_sim(n)
    return _SIMS[n]


def _new_sim(n):
    S = Sim(B, 32, 48, 1, V, dtype=0, seed=0, beam=n, max_steps=MS, dims=SMALL)
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(IMG), None), "enc")
    from latex_ocr_amd.model.utils.image import encoder_out_hw
    Hp, Wp = encoder_out_hw(32, 48)
    S.enc = S.region("img", np.float32)[:B * Hp * Wp * SMALL["C"]].reshape(B, Hp * Wp, SMALL["C"]).copy()
    return S


def _torch_params(S):
    import torch
    return {k: torch.from_numpy(np.asarray(v)) for k, v in S.P.items()}


def _greedy(S, al, pf=None, ln=None):
    bits = constraint_ref.pack_bits(al)
    ids = np.zeros((B, MS), np.int32); lp = np.zeros((B, MS), np.float32); steps = ctypes.c_int(0)
    pa = (ptr(pf), pf.shape[1], ptr(ln)) if pf is not None else (None, 0, None)
    S.ck(S.L.lxo_greedy_decode_constrained(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(bits), bits.shape[1], *pa,
                                           ptr(ids), ptr(lp), None, ctypes.byref(steps), None), "greedy")
    return ids[:, :steps.value], lp[:, :steps.value]


def test_top_k_1_has_the_arg_max_kernels_ids_and_logp_bits():
    """lxo_sample_tokens(K = 1) on the decoder's own step-0 logits against lxo_k_argmax, reached through lxo_greedy_decode_constrained"""
    S = _sim()
    for al in (np.ones((B, V), bool), sets_for(V, B, 2)):
        gid, glp = _greedy(S, al)
        S.ck(S.L.lxo_decode_begin(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), None), "begin")
        S.ck(S.L.lxo_decode_cell_step(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), 0, 1, None), "cell")
        lg = S.region("dec_logits", np.float32, (B, 32)).copy()
        for tau in (1.0, 0.5):
            rc, ids, lp, _ = tokens(lg, V, 1, 0, opts(tau, 1, 1.0, 9), al)
            assert rc == 0 and np.array_equal(ids, gid[:, 0])
            assert np.array_equal(lp.view(np.uint32), glp[:, 0].view(np.uint32))


def test_a_draw_depends_on_neither_n_nor_the_other_rows():
    for Vn, ld in [(11, 12), (65, 65), (500, 512)]:
        lg = logits_for(Vn, ld, 10, 2.0, 1)
        al = sets_for(Vn, 2, 1); al[1] = al[0]
        for o, a in ((opts(1.0, 0, 1.0, 4), None), (opts(2.0, 5, 0.9, 4), al)):
            rc5, i5, p5, q5 = tokens(lg, Vn, 5, 2, o, a)
            pick = np.array([0, 1, 5, 6])
            rc2, i2, p2, q2 = tokens(np.ascontiguousarray(lg[pick]), Vn, 2, 2, o, a)
            assert rc5 == 0 and rc2 == 0
            assert np.array_equal(i5[pick], i2) and np.array_equal(p5[pick].view(np.uint32), p2.view(np.uint32))
            assert np.array_equal(q5[pick].view(np.uint32), q2.view(np.uint32))


def test_a_seed_repeats_bit_for_bit_and_seeds_differ():
    lg = logits_for(65, 68, 48, 1.0, 2)
    a = tokens(lg, 65, 16, 1, opts(1.0, 0, 1.0, 11))
    b = tokens(lg, 65, 16, 1, opts(1.0, 0, 1.0, 11))
    c = tokens(lg, 65, 16, 1, opts(1.0, 0, 1.0, 12))
    d = tokens(lg, 65, 16, 2, opts(1.0, 0, 1.0, 11))
    assert a[0] == 0 and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[1:], b[1:]))
    assert not np.array_equal(a[1], c[1]) and not np.array_equal(a[1], d[1])
    assert len(set(a[1][:16].tolist())) > 1                               # the draws of one image differ among themselves
    e = tokens(lg, 65, 16, 1, opts(1.0, 0, 1.0, 11), want=(False, False))  # nullable logp / logq
    assert e[0] == 0 and np.array_equal(e[1], a[1])


def test_an_empty_set_emits_zero_without_a_fault():
    lg = logits_for(11, 12, 4, 1.0, 3)
    al = np.ones((2, 11), bool); al[1] = False
    for o in (opts(), opts(0.7, 3, 0.8, 1)):
        rc, ids, _, _ = tokens(lg, 11, 2, 0, o, al)
        assert rc == 0 and (ids[2:] == 0).all() and ((ids >= 0) & (ids < 11)).all()
    lg2 = logits_for(70, 70, 4, 1.0, 3)                                    # the strided row
    al2 = np.ones((2, 70), bool); al2[1] = False
    rc, ids, _, _ = tokens(lg2, 70, 2, 0, opts(0.7, 3, 0.8, 1), al2)
    assert rc == 0 and (ids[2:] == 0).all()


def test_refusals():
    lg = logits_for(11, 12, 4, 1.0, 0)
    for o in (opts(0.0), opts(-1.0), opts(1e-39), opts(float("inf")), opts(float("nan")), opts(1.0, -1), opts(1.0, 0, 0.0), opts(1.0, 0, 1.5), opts(1.0, 0, float("nan"))):
        assert tokens(lg, 11, 2, 0, o)[0] == -1
    ids = np.zeros(4, np.int32); o = opts()
    L = lib()
    assert L.lxo_sample_tokens(ptr(lg), 12, 4, 2, 11, 0, None, None, 0, ptr(ids), None, None, None) == -1
    assert L.lxo_sample_tokens(None, 12, 4, 2, 11, 0, ctypes.byref(o), None, 0, ptr(ids), None, None, None) == -1
    assert L.lxo_sample_tokens(ptr(lg), 12, 4, 2, 11, 0, ctypes.byref(o), None, 1, ptr(ids), None, None, None) == -1
    assert L.lxo_sample_tokens(ptr(lg), 12, 4, 17, 11, 0, ctypes.byref(o), None, 0, ptr(ids), None, None, None) == -5
    assert L.lxo_sample_tokens(ptr(lg), 10, 4, 2, 11, 0, ctypes.byref(o), None, 0, ptr(ids), None, None, None) == -5
    assert L.lxo_sample_tokens(ptr(lg), 12, 4, 2, 11, -1, ctypes.byref(o), None, 0, ptr(ids), None, None, None) == -5
    assert (ids == 0).all()                                               # refused before any launch
    S = _sim(3)
    out = np.zeros((B, MS, 3), np.int32); steps = ctypes.c_int(0)
    call = lambda o, mi=MAX_ITER, al=None, ld=0, pf=None, pld=0, pln=None: S.L.lxo_sample_decode(
        S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, mi, ctypes.byref(o) if o is not None else None, ptr(al), ld, ptr(pf), pld, ptr(pln),
        ptr(out), None, None, None, ctypes.byref(steps), None)
    for o in (None, opts(0.0), opts(float("nan")), opts(1.0, -2), opts(1.0, 0, 0.0), opts(1.0, 0, 1.0001)):
        assert call(o) == -1
    assert call(opts(), MS) == -5                                         # fewer record columns than steps
    assert call(opts(), al=None, ld=1) == -1                              # half a set, half a prefix
    assert call(opts(), pf=np.zeros((B, 2), np.int32), pld=2) == -1
    S.shape.beam = 12                                                     # more rows per image than tokens
    try:
        assert call(opts()) == -5
    finally:
        S.shape.beam = 3
    assert (out == 0).all()


def _decode(S, n, o, al=None, pf=None, ln=None):
    ids = np.zeros((B, MS, n), np.int32); lp = np.zeros((B, MS, n), np.float32); lq = np.zeros((B, MS, n), np.float32); steps = ctypes.c_int(0)
    bits = constraint_ref.pack_bits(al) if al is not None else None
    pa = (ptr(pf), pf.shape[1], ptr(ln)) if pf is not None else (None, 0, None)
    rc = S.L.lxo_sample_decode(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ctypes.byref(o), ptr(bits), 0 if bits is None else bits.shape[1],
                               *pa, ptr(ids), ptr(lp), ptr(lq), None, ctypes.byref(steps), None)
    assert rc == 0, S.L.lxo_last_error()
    t = steps.value
    return ids[:, :t], lp[:, :t], lq[:, :t]


def _against_reference(S, n, tau, K, p, seed, al=None, pf=None, ln=None):
    ids, lp, lq = _decode(S, n, opts(tau, K, p, seed), al, pf, ln)
    rid, rlp, rlq, picks, _ = sample_ref.sample_decode(_torch_params(S), S.enc, END, n, MAX_ITER, tau, K, p, seed, al, pf, ln)
    compared, differ, agree = sample_ref.compare_decode(ids, rid, picks)
    print("n = %d: draws compared %d, differing %d" % (n, compared, differ))
    assert differ <= 1e-3 * compared
    if differ == 0:
        assert ids.shape == rid.shape
    T = agree.shape[1]
    assert np.abs(lp[:, :T] - rlp[:, :T])[agree].max() < TOL and np.abs(lq[:, :T] - rlq[:, :T])[agree].max() < TOL
    return ids, lp, lq


@pytest.mark.parametrize("n", [1, 3])
def test_decode_matches_the_reference(n):
    S = _sim(n)
    ids, _, _ = _against_reference(S, n, 1.0, 0, 1.0, 5)
    _against_reference(S, n, 2.0, 4, 0.9, 6)
    if n > 1:
        assert any(not np.array_equal(ids[b, :, 0], ids[b, :, j]) for b in range(B) for j in range(1, n))      # the draws of an image differ


@pytest.mark.parametrize("n", [1, 3])
def test_decode_with_prefix_lengths_and_sets(n):
    S = _sim(n)
    pf = np.ascontiguousarray(np.random.RandomState(0).randint(0, END, size=(B, MAX_ITER)), np.int32)
    ids, lp, lq = _against_reference(S, n, 1.5, 0, 1.0, 2, None, pf, LENS)
    for b in range(B):
        assert (ids[b, :LENS[b]] == pf[b, :LENS[b], None]).all() and (lq[b, :LENS[b]] == 0).all()
    al = np.ones((B, V), bool)
    al[1, [2, 3, 7]] = False; al[2, :5] = False; al[3, 1::2] = False; al[:, END] = True
    ids, _, _ = _against_reference(S, n, 1.5, 0, 0.9, 3, al)
    assert all(al[b][ids[b].reshape(-1)].all() for b in range(B))
    al2 = al.copy()
    for b in range(B):
        al2[b, pf[b, :LENS[b]]] = True
    ids, _, _ = _against_reference(S, n, 1.5, 5, 1.0, 4, al2, pf, LENS)
    assert all(al2[b][ids[b].reshape(-1)].all() for b in range(B))


@pytest.mark.parametrize("n", [1, 3])
def test_decode_with_top_k_1_equals_greedy(n):
    S1 = _sim(1)
    full = np.ones((B, V), bool)
    gid, glp = _greedy(S1, full)
    S = _sim(n)
    ids, lp, lq = _decode(S, n, opts(0.7, 1, 1.0, 8))
    assert ids.shape[1] == gid.shape[1]
    for j in range(n):
        assert np.array_equal(ids[:, :, j], gid) and np.abs(lp[:, :, j] - glp).max() < TOL
    assert (lq == 0).all()
    a = _decode(S, n, opts(1.3, 0, 1.0, 8)); b = _decode(S, n, opts(1.3, 0, 1.0, 8))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
