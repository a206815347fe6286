"""CPU (hipsim): Engine.greedy_decode / Engine.beam_decode with allowed= -- the host-side check, the bit packing and the choice of entry point --
bit for bit against a direct lxo_*_decode_constrained call on a Sim with the same parameters and images and the sets packed by
tests/constraint_ref.pack_bits (tests/test_constraint_sim.py holds those C calls to the reference).  And every ValueError the Engine
raises before a launch."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
from simharness import Sim, ptr
from simlib import SIM_SO, build_sim
import constraint_ref

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, END, MAX_ITER, MS = 11, 10, 8, 9
B, H, W = 2, 32, 48
PREFIX = np.ascontiguousarray(np.random.RandomState(0).randint(0, END, size=(B, MAX_ITER)), np.int32)
LENS = np.array([3, 0], np.int32)


@pytest.fixture(scope="module")
def setup():
    build_sim()
    eng = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=_abi.bind(ctypes.CDLL(SIM_SO)))
    imgs, _ = synthetic.make_set(B, H, W, V, 2, 4, seed=5)
    return eng, pad_batch_images(imgs)


def _sets(eng, img):
    """row 0 bans its own unconstrained first pick, row 1 its second token; END and the prefix tokens stay allowed"""
    ids = eng.greedy_decode(img, END, max_iter=MAX_ITER)
    al = np.ones((B, V), bool)
    al[0, ids[0, 0]] = False
    al[1, ids[1, min(1, ids.shape[1] - 1)]] = False
    al[:, END] = True
    al[0, PREFIX[0, :LENS[0]]] = True
    return al, ids


def _direct(eng, img, k, al, ld, prefix):
    S = Sim(B, H, W, 1, V, dtype=0, beam=max(k, 1), max_steps=MS, dims=SMALL, params=eng.get_params())
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(np.ascontiguousarray(img, np.uint8)), None), "enc")
    bits = constraint_ref.pack_bits(al)
    steps = ctypes.c_int(0)
    pa = (ptr(PREFIX), PREFIX.shape[1], ptr(LENS)) if prefix else (None, 0, None)
    head = (S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(bits), ld) + pa
    if k == 0:
        ids = np.zeros((B, MS), np.int32); lp = np.zeros((B, MS), np.float32)
        S.ck(S.L.lxo_greedy_decode_constrained(*head, ptr(ids), ptr(lp), None, ctypes.byref(steps), None), "greedy_constrained")
        return ids[:, :steps.value], lp[:, :steps.value]
    ids = np.zeros((B, MS, k), np.int32); par = np.zeros((B, MS, k), np.int32); sc = np.zeros((B, MS, k), np.float32)
    S.ck(S.L.lxo_beam_decode_constrained(*head, ptr(ids), ptr(par), ptr(sc), None, ctypes.byref(steps), None), "beam_constrained")
    n = steps.value
    return ids[:, :n], par[:, :n], sc[:, :n]


def _same(got, want):
    assert len(got) == len(want)
    for a, r in zip(got, want):
        assert a.dtype == r.dtype and a.shape == r.shape and np.array_equal(a.view(np.uint32), r.view(np.uint32))


@pytest.mark.parametrize("prefix", [False, True])
def test_engine_greedy_allowed_equals_the_c_call(setup, prefix):
    eng, img = setup
    al, free = _sets(eng, img)
    kw = dict(prefix=PREFIX, prefix_lengths=LENS) if prefix else {}
    got = eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, allowed=al, **kw)
    _same(got, _direct(eng, img, 0, al, 1, prefix))
    assert all(al[b][got[0][b]].all() for b in range(B))
    if not prefix:
        assert got[0][0, 0] != free[0, 0]                                   # the constraint binds
        assert np.array_equal(eng.greedy_decode(img, END, max_iter=MAX_ITER, allowed=al), got[0])                # ids alone
        ids, alpha, lp = eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, return_attention=True, allowed=al)
        _same((ids, lp), got)
        assert alpha.shape[:2] == ids.shape
    # [V]: one set for the batch (allow_ld = 0)
    _same(eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, allowed=al[0], **kw), _direct(eng, img, 0, al[0], 0, prefix))
    # every token allowed: the call without a set, bit for bit
    _same(eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, allowed=np.ones(V, np.int64), **kw),
          eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, **kw))


@pytest.mark.parametrize("k,prefix", [(2, False), (3, True)])
def test_engine_beam_allowed_equals_the_c_call(setup, k, prefix):
    eng, img = setup
    al, _ = _sets(eng, img)
    kw = dict(prefix=PREFIX, prefix_lengths=LENS) if prefix else {}
    got = eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_scores=True, allowed=al, **kw)
    _same(got, _direct(eng, img, k, al, 1, prefix))
    assert all(al[b][got[0][b].reshape(-1)].all() for b in range(B))
    _same(eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_scores=True, allowed=np.ones((B, V), bool), **kw),
          eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_scores=True, **kw))


def test_engine_refuses_bad_sets_before_any_launch(setup):
    _, img = setup
    eng = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=setup[0].lib)
    ok = np.ones((B, V), bool)
    no_end = ok.copy(); no_end[1, END] = False
    few = np.zeros((B, V), bool); few[:, END] = True; few[:, 2] = True        # two tokens: enough for greedy, not for a beam of 3
    ban = ok.copy(); ban[0, PREFIX[0, 1]] = False                              # row 0 forces PREFIX[0, :3]
    bad = [dict(allowed=np.ones((B + 1, V), bool)), dict(allowed=np.ones((B, V + 1), bool)), dict(allowed=np.ones((1, B, V), bool)),
           dict(allowed=no_end), dict(allowed=np.zeros(V, bool)), dict(allowed=ban, prefix=PREFIX, prefix_lengths=LENS)]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.greedy_decode(img, END, max_iter=MAX_ITER, **kw)
        with pytest.raises(ValueError):
            eng.beam_decode(img, END, 3, max_iter=MAX_ITER, **kw)
    with pytest.raises(ValueError):
        eng.beam_decode(img, END, 3, max_iter=MAX_ITER, allowed=few)
    assert eng.ws is None and not hasattr(eng, "_img")                         # nothing was staged or launched
    ids = eng.greedy_decode(img, END, max_iter=MAX_ITER, allowed=few)
    assert np.isin(ids, [2, END]).all()
    ids = eng.greedy_decode(img, END, max_iter=MAX_ITER, allowed=ban, prefix=PREFIX, prefix_lengths=np.array([1, 0], np.int32))   # the banned position is dead
    assert ids[0, 0] == PREFIX[0, 0]
