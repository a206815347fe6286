"""CPU (hipsim): what Engine.greedy_decode / Engine.beam_decode return for every combination of return_attention x return_scores x prefix
(x return_parents) -- the tuple's type, length and order, every array's shape and dtype -- and every array bit for bit against a direct
C-ABI call on a Sim with the same parameters and images: the most general entry point of the kind (lxo_greedy_decode_prefix /
lxo_beam_decode_prefix with every output; all prefix lengths 0 for "no prefix"), sliced to `steps`.  tests/test_prefix_sim.py and
tests/test_decode_scores_sim.py hold those C calls to the oracle and to each other."""
import ctypes
import itertools

import numpy as np
import pytest

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import encoder_out_hw, pad_batch_images
from simharness import Sim, ptr
from simlib import SIM_SO, build_sim

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, END, MAX_ITER, MS = 11, 10, 8, 9
B, H, W = 2, 32, 48
HP, WP = encoder_out_hw(H, W)
R = HP * WP
RP = (R + 7) // 8 * 8
PREFIX = np.ascontiguousarray(np.random.RandomState(0).randint(0, END, size=(B, MAX_ITER)), np.int32)      # ids in [0, V) without END
LENS = np.array([0, MAX_ITER], np.int32)             # greedy and beam 2: no forced token / the whole decode
LENS_MID = np.array([4, 1], np.int32)                # beam 3
DIV = dict(div_gamma=0.5, div_prob=1.0, div_seed=4)


@pytest.fixture(scope="module")
def setup():
    build_sim()
    eng = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=_abi.bind(ctypes.CDLL(SIM_SO)))
    imgs, _ = synthetic.make_set(B, H, W, V, 2, 4, seed=5)
    return eng, pad_batch_images(imgs)


def _reference(eng, img, k, lens, div=None):
    """{name: array} of the direct C call with every output, sliced to steps and laid out as the Engine documents its results"""
    S = Sim(B, H, W, 1, V, dtype=0, beam=max(k, 1), max_steps=MS, dims=SMALL, params=eng.get_params())
    if div:
        S.shape.div_gamma, S.shape.div_prob, S.shape.div_seed = div["div_gamma"], div["div_prob"], div["div_seed"]
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(np.ascontiguousarray(img, np.uint8)), None), "enc")
    steps = ctypes.c_int(0)
    head = (S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(PREFIX), PREFIX.shape[1], ptr(lens))
    if k == 0:
        ids = np.zeros((B, MS), np.int32); lp = np.zeros((B, MS), np.float32); al = np.zeros((MS, B, RP), np.float32)
        S.ck(S.L.lxo_greedy_decode_prefix(*head, ptr(ids), ptr(lp), ptr(al), ctypes.byref(steps), None), "greedy_prefix")
        n = steps.value
        return {"ids": ids[:, :n], "logp": lp[:, :n], "alpha": al[:n, :, :R].transpose(1, 0, 2).reshape(B, n, HP, WP)}
    ids = np.zeros((B, MS, k), np.int32); par = np.zeros((B, MS, k), np.int32); sc = np.zeros((B, MS, k), np.float32)
    al = np.zeros((MS, B * k, RP), np.float32)
    S.ck(S.L.lxo_beam_decode_prefix(*head, ptr(ids), ptr(par), ptr(sc), ptr(al), ctypes.byref(steps), None), "beam_prefix")
    n = steps.value
    return {"ids": ids[:, :n], "parents": par[:, :n], "scores": sc[:, :n],
            "alpha": al[:n, :, :R].reshape(n, B, k, HP, WP).transpose(1, 0, 2, 3, 4)}


def _check(what, got, names, ref):
    """the tuple (a bare array when only ids are returned) in `names` order; each array's shape, dtype and bits are the reference's"""
    if len(names) == 1:
        assert isinstance(got, np.ndarray), (what, type(got))
        got = (got,)
    assert isinstance(got, tuple) and len(got) == len(names), (what, type(got), len(got), names)
    for name, a in zip(names, got):
        r = ref[name]
        assert isinstance(a, np.ndarray) and a.dtype == r.dtype and a.shape == r.shape, (what, name, getattr(a, "dtype", None), getattr(a, "shape", None), r.shape)
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(r).view(np.uint32)), (what, name)
    assert ref["ids"].dtype == np.int32 and ref["alpha"].dtype == np.float32


def test_greedy_every_combination(setup):
    eng, img = setup
    refs = {False: _reference(eng, img, 0, np.zeros(B, np.int32)), True: _reference(eng, img, 0, LENS)}
    assert refs[True]["ids"].shape == (B, MS) and np.array_equal(refs[True]["ids"][1, :MAX_ITER], PREFIX[1])
    for attn, scores, pfx in itertools.product((False, True), repeat=3):
        kw = dict(prefix=PREFIX, prefix_lengths=LENS) if pfx else {}
        got = eng.greedy_decode(img, END, max_iter=MAX_ITER, return_attention=attn, return_scores=scores, **kw)
        names = ["ids"] + ["alpha"] * attn + ["logp"] * scores
        _check(("greedy", attn, scores, pfx), got, names, refs[pfx])


def _beam_combination(eng, img, k, refs, lens, combo, div):
    par, attn, scores, pfx = combo
    kw = dict(prefix=PREFIX, prefix_lengths=lens) if pfx else {}
    got = eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_parents=par, return_attention=attn, return_scores=scores, **dict(kw, **div))
    names = ["ids"] + ["parents"] * (par or attn or scores) + ["alpha"] * attn + ["scores"] * scores
    _check(("beam", k) + combo, got, names, refs[pfx])


def test_beam_every_combination(setup):
    eng, img = setup
    refs = {False: _reference(eng, img, 2, np.zeros(B, np.int32)), True: _reference(eng, img, 2, LENS)}
    assert (refs[True]["ids"][1, :MAX_ITER] == PREFIX[1][:, None]).all()
    for combo in itertools.product((False, True), repeat=4):
        _beam_combination(eng, img, 2, refs, LENS, combo, {})


def test_beam_3_with_the_diversity_penalty_corners(setup):
    eng, img = setup
    refs = {False: _reference(eng, img, 3, np.zeros(B, np.int32), DIV), True: _reference(eng, img, 3, LENS_MID, DIV)}
    for combo in ((False, False, False, False), (True, False, False, False), (False, True, True, False), (False, True, True, True)):
        _beam_combination(eng, img, 3, refs, LENS_MID, combo, DIV)
