"""CPU (hipsim): Engine.greedy_decode / beam_decode / sample_decode with grammar= -- the host-side contract check, the staging and the choice
of entry point -- bit for bit against direct lxo_*_decode_grammar calls on a Sim with the same parameters and images, and token for token
against tests/grammar_ref.py (the oracle's decode with the per-step sets of latex_ocr_amd.grammar.Grammar), log-probs inside the 1e-5 the
f32 constrained tests use.  Two delimiter kinds over tokens 0 .. 5 of an 11-token vocabulary, so that random weights run into the order rules
and, at max_iter = 8, into the budget; every test that compares also shows that the grammar changed the decode."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.grammar import Grammar
from latex_ocr_amd.model.utils.image import pad_batch_images, encoder_out_hw
from simharness import Sim, ptr
from simlib import SIM_SO, build_sim
import constraint_ref
import grammar_ref
import sample_ref

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, END, MAX_ITER, MS = 11, 10, 8, 9
B, H, W = 2, 32, 48
TOL = 1e-5
CLS = np.array([1, -1, 2, -2, 1, -1, 0, 0, 0, 0, 0], np.int8)          # 0, 4 open kind 1; 1, 5 close it; 2 / 3 open / close kind 2
PREFIX = np.array([[0, 2, 3, 0, 0, 0, 0, 0], [0] * 8], np.int32)         # row 0: open 1, open 2, close 2 -- then the decode is at depth 1
LENS = np.array([3, 0], np.int32)
SMP = dict(temperature=1.3, top_k=6, top_p=0.9, seed=11)


def gram(**kw):
    return Grammar(CLS, **dict(dict(max_depth=2, budget=True, id_end=END), **kw))


@pytest.fixture(scope="module")
def setup():
    build_sim()
    eng = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=_abi.bind(ctypes.CDLL(SIM_SO)))
    imgs, _ = synthetic.make_set(B, H, W, V, 2, 4, seed=5)
    img = pad_batch_images(imgs)
    eng.greedy_decode(img, END, max_iter=MAX_ITER)
    Hp, Wp = encoder_out_hw(H, W)
    enc = eng.region("img", "f32")[:B * Hp * Wp * SMALL["C"]].reshape(B, Hp * Wp, SMALL["C"]).cpu().numpy().copy()      # the features the decoder reads
    P = {k: torch.from_numpy(np.asarray(v).copy()) for k, v in eng.get_params().items()}
    return eng, img, P, enc


def _allowed():
    """a static set that bans two plain tokens in row 0 and one in row 1; END and every closer stay (the contract)"""
    al = np.ones((B, V), bool)
    al[0, [6, 8]] = False
    al[1, 7] = False
    return al


def _direct(eng, img, kind, k, g, al, prefix):
    """the C call itself: -> the outputs cut to the steps run, the depths last"""
    S = Sim(B, H, W, 1, V, dtype=0, beam=max(k, 1), max_steps=MS, dims=SMALL, params=eng.get_params())
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(np.ascontiguousarray(img, np.uint8)), None), "enc")
    bits = constraint_ref.pack_bits(al) if al is not None else None
    cls = np.ascontiguousarray(g.cls)
    gs = _abi.LxoGrammar(ptr(cls), g.n_kinds, g.max_depth, 1 if g.budget else 0)
    rows = B * max(k, 1)
    scratch = np.zeros(S.L.lxo_grammar_scratch_bytes(rows, V) // 4, np.uint32)
    steps = ctypes.c_int(0)
    pa = (ptr(PREFIX), PREFIX.shape[1], ptr(LENS)) if prefix else (None, 0, None)
    aa = (ptr(bits), bits.shape[1]) if bits is not None else (None, 0)
    head = (S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER)
    shp = (B, MS) if kind == "greedy" else (B, MS, k)
    ids = np.zeros(shp, np.int32); dep = np.zeros(shp, np.int32); lp = np.zeros(shp, np.float32)
    if kind == "greedy":
        S.ck(S.L.lxo_greedy_decode_grammar(*head, *aa, *pa, ctypes.byref(gs), ptr(ids), ptr(lp), None, ptr(dep), ptr(scratch),
                                           ctypes.byref(steps), None), "greedy_grammar")
        out = (ids, lp, dep)
    elif kind == "beam":
        par = np.zeros(shp, np.int32)
        S.ck(S.L.lxo_beam_decode_grammar(*head, *aa, *pa, ctypes.byref(gs), ptr(ids), ptr(par), ptr(lp), None, ptr(dep), ptr(scratch),
                                         ctypes.byref(steps), None), "beam_grammar")
        out = (ids, par, lp, dep)
    else:
        lq = np.zeros(shp, np.float32)
        so = _abi.LxoSampleOpts(SMP["temperature"], SMP["top_k"], SMP["top_p"], SMP["seed"])
        S.ck(S.L.lxo_sample_decode_grammar(*head, ctypes.byref(so), *aa, *pa, ctypes.byref(gs), ptr(ids), ptr(lp), ptr(lq), None, ptr(dep),
                                           ptr(scratch), ctypes.byref(steps), None), "sample_grammar")
        out = (ids, lp, lq, dep)
    return tuple(a[:, :steps.value] for a in out)


def _same(got, want):
    assert len(got) == len(want)
    for a, r in zip(got, want):
        assert a.dtype == r.dtype and a.shape == r.shape and np.array_equal(a.view(np.uint32), r.view(np.uint32))


def _guarantee(g, seqs, depths, forced):
    """every sequence reaches END balanced, lies in its sets at the free steps, and the returned depths are the host replay's"""
    for seq, dep, nf in zip(seqs, depths, forced):
        assert g.check(seq, END), seq
        want, ok = g.replay(seq, MAX_ITER, END, nf)
        assert ok, seq
        if dep is not None:
            assert list(dep) == want, (seq, list(dep), want)


CASES = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("prefix,allowed", CASES)
def test_greedy_grammar(setup, prefix, allowed):
    eng, img, P, enc = setup
    g = gram()
    al = _allowed() if allowed else None
    kw = dict(prefix=PREFIX, prefix_lengths=LENS) if prefix else {}
    if allowed:
        kw["allowed"] = al
    free = eng.greedy_decode(img, END, max_iter=MAX_ITER, **kw)
    ids, lp, dep = eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True, **kw)
    _same((ids, lp, dep), _direct(eng, img, "greedy", 0, g, al, prefix))
    rid, rlp, rdep, _ = grammar_ref.greedy_grammar(P, enc, END, g, MAX_ITER, al, PREFIX if prefix else None, LENS if prefix else None)
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    assert np.array_equal(dep, rdep)
    assert np.isfinite(lp).all() and np.abs(lp - rlp).max() < TOL, np.abs(lp - rlp).max()
    _guarantee(g, ids, dep, LENS if prefix else [0] * B)
    n = min(ids.shape[1], free.shape[1])
    assert ids.shape[1] != free.shape[1] or not np.array_equal(ids[:, :n], free[:, :n])      # the grammar binds
    assert not all(g.check(free[b], END) for b in range(B))                                   # ... because the free decode is not balanced
    if not prefix and not allowed:
        assert np.array_equal(eng.greedy_decode(img, END, max_iter=MAX_ITER, grammar=g), ids)      # ids alone
        i2, alpha, l2, d2 = eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, return_attention=True, grammar=g, return_depth=True)
        _same((i2, l2, d2), (ids, lp, dep))
        assert alpha.shape[:2] == ids.shape


@pytest.mark.parametrize("k,prefix,allowed", [(2, False, False), (3, True, True), (3, False, True), (2, True, False)])
def test_beam_grammar(setup, k, prefix, allowed):
    eng, img, P, enc = setup
    g = gram()
    al = _allowed() if allowed else None
    kw = dict(prefix=PREFIX, prefix_lengths=LENS) if prefix else {}
    if allowed:
        kw["allowed"] = al
    free, fpar = eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_parents=True, **kw)
    ids, par, sc, dep = eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True, **kw)
    _same((ids, par, sc, dep), _direct(eng, img, "beam", k, g, al, prefix))
    rid, rpar, rsc, rdep = grammar_ref.beam_grammar(P, enc, END, k, g, MAX_ITER, al, PREFIX if prefix else None, LENS if prefix else None)
    assert ids.shape == rid.shape and np.array_equal(ids, rid) and np.array_equal(par, rpar), (ids, rid, par, rpar)
    assert np.array_equal(dep, rdep)
    assert np.isfinite(sc).all() and np.abs(sc - rsc).max() < TOL * max(1.0, np.abs(rsc).max())
    unbalanced = 0
    for b in range(B):
        hyps = grammar_ref.backtrace(ids[b], par[b])
        _guarantee(g, hyps, [None] * k, [LENS[b] if prefix else 0] * k)
        # depth [t][j] belongs to the hypothesis that sits in slot j at step t: replay every back-traced prefix
        for t in range(ids.shape[1]):
            for j, seq in enumerate(grammar_ref.backtrace(ids[b, :t + 1], par[b, :t + 1])):
                assert dep[b, t, j] == g.replay(seq, MAX_ITER, END, LENS[b] if prefix else 0)[0][-1], (b, t, j)
        unbalanced += sum(not g.check(s, END) for s in grammar_ref.backtrace(free[b], fpar[b]))
    assert unbalanced > 0 and not np.array_equal(ids[:, :min(ids.shape[1], free.shape[1])], free[:, :min(ids.shape[1], free.shape[1])])


@pytest.mark.parametrize("prefix,allowed", CASES)
def test_sample_grammar(setup, prefix, allowed):
    eng, img, P, enc = setup
    g, n = gram(), 3
    al = _allowed() if allowed else None
    kw = dict(prefix=PREFIX, prefix_lengths=LENS) if prefix else {}
    if allowed:
        kw["allowed"] = al
    free = eng.sample_decode(img, END, n, max_iter=MAX_ITER, **SMP, **kw)
    ids, lp, lq, dep = eng.sample_decode(img, END, n, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True, **SMP, **kw)
    _same((ids, lp, lq, dep), _direct(eng, img, "sample", n, g, al, prefix))
    rid, rlp, rlq, rdep, _, _ = grammar_ref.sample_grammar(P, enc, END, n, g, MAX_ITER, SMP["temperature"], SMP["top_k"], SMP["top_p"], SMP["seed"],
                                                           al, PREFIX if prefix else None, LENS if prefix else None)
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    assert np.array_equal(dep, rdep)
    assert np.abs(lp - rlp).max() < TOL and np.abs(lq - rlq).max() < TOL
    for b in range(B):
        _guarantee(g, ids[b].T, dep[b].T, [LENS[b] if prefix else 0] * n)
    assert not all(g.check(free[b, :, j], END) for b in range(B) for j in range(n))
    assert ids.shape != free.shape or not np.array_equal(ids, free)


def test_an_all_plain_table_without_budget_is_the_call_without_a_grammar(setup):
    eng, img, _, _ = setup
    g = Grammar(np.zeros(V, np.int8), budget=False, id_end=END)
    al = _allowed()
    for kw in (dict(prefix=PREFIX, prefix_lengths=LENS, allowed=al),):
        _same(eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, grammar=g, **kw),
              eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, **kw))
        _same(eng.beam_decode(img, END, 3, max_iter=MAX_ITER, return_scores=True, grammar=g, **kw),
              eng.beam_decode(img, END, 3, max_iter=MAX_ITER, return_scores=True, **kw))
        _same(eng.sample_decode(img, END, 3, max_iter=MAX_ITER, return_scores=True, grammar=g, **SMP, **kw),
              eng.sample_decode(img, END, 3, max_iter=MAX_ITER, return_scores=True, **SMP, **kw))
    dep = eng.greedy_decode(img, END, max_iter=MAX_ITER, grammar=g, return_depth=True)[1]
    assert not dep.any()


def test_engine_refuses_a_broken_contract_before_any_launch(setup):
    _, img, _, _ = setup
    eng = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=setup[0].lib)
    g = gram()
    no_closer = np.ones((B, V), bool); no_closer[1, 3] = False                 # bans the closer of kind 2
    few = np.zeros((B, V), bool); few[:, [1, 3, 5, END, 6]] = True             # step 0 leaves END and one plain token: not enough for a beam of 3
    bad_pf = np.array([[1, 0, 0], [0, 0, 0]], np.int32)                         # row 0 starts with a closer
    calls = [dict(grammar="latex"), dict(grammar=Grammar(np.zeros(V + 1, np.int8), id_end=END)), dict(grammar=Grammar(CLS)),
             dict(grammar=g, allowed=no_closer), dict(grammar=g, prefix=bad_pf, prefix_lengths=np.array([1, 0], np.int32)),
             dict(grammar=g, prefix=PREFIX, prefix_lengths=np.array([2, 0], np.int32), max_iter=2),      # depth 2 with one step left
             dict(return_depth=True)]
    for kw in calls:
        kw = dict(dict(max_iter=MAX_ITER), **kw)
        end = 0 if kw.get("grammar") is not None and isinstance(kw["grammar"], Grammar) and kw["grammar"].id_end is None else END      # END = 0 is an opener
        with pytest.raises(ValueError):
            eng.greedy_decode(img, end, **kw)
        with pytest.raises(ValueError):
            eng.beam_decode(img, end, 2, **kw)
        with pytest.raises(ValueError):
            eng.sample_decode(img, end, 2, **kw)
    with pytest.raises(ValueError):
        eng.beam_decode(img, END, 3, max_iter=MAX_ITER, grammar=g, allowed=few)
    assert eng.ws is None and not hasattr(eng, "_img")                         # nothing was staged or launched
    ids = eng.greedy_decode(img, END, max_iter=MAX_ITER, grammar=g, allowed=few)
    assert np.isin(ids, [6, END]).all()
