"""CPU (hipsim): Engine.sample_decode / Engine.sample_tokens -- the host-side checks, the staging of sets and prefixes and the output assembly --
bit for bit against a direct lxo_sample_decode / lxo_sample_tokens call on a Sim with the same parameters and images (tests/test_sample_sim.py holds
those C calls to the reference).  And every ValueError the Engine raises before a launch."""
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


_SIMS = {}


def _direct(eng, img, n, o, al=None, prefix=False):
    if n not in _SIMS:                                                     # one Sim per n: the encoder runs once, every call sets its own state up
        S = Sim(B, H, W, 1, V, dtype=0, beam=n, max_steps=MS, dims=SMALL, params=eng.get_params())
        S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(np.ascontiguousarray(img, np.uint8)), None), "enc")
        _SIMS[n] = S
    S = _SIMS[n]
    bits = constraint_ref.pack_bits(al) if al is not None else None
    ids = np.zeros((B, MS, n), np.int32); lp = np.zeros((B, MS, n), np.float32); lq = np.zeros((B, MS, n), np.float32); steps = ctypes.c_int(0)
    pa = (ptr(PREFIX), PREFIX.shape[1], ptr(LENS)) if prefix else (None, 0, None)
    S.ck(S.L.lxo_sample_decode(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ctypes.byref(o), ptr(bits), 0 if bits is None else bits.shape[1],
                               *pa, ptr(ids), ptr(lp), ptr(lq), None, ctypes.byref(steps), None), "sample_decode")
    t = steps.value
    return ids[:, :t], lp[:, :t], lq[:, :t]


def _same(got, want):
    return all(a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))


def test_sample_decode_equals_the_direct_call(setup):
    eng, img = setup
    eng.max_steps, eng.ws = MS, None
    al = np.ones((B, V), bool); al[0, [1, 2]] = False; al[1, 5] = False
    al[0, PREFIX[0, :LENS[0]]] = True
    for n in (1, 3):
        got = eng.sample_decode(img, END, n=n, temperature=1.5, top_k=6, top_p=0.9, seed=4, max_iter=MAX_ITER, return_scores=True)
        assert got[0].shape[0] == B and got[0].shape[2] == n and _same(got, _direct(eng, img, n, _abi.LxoSampleOpts(1.5, 6, 0.9, 4)))
        ids = eng.sample_decode(img, END, n=n, temperature=1.5, top_k=6, top_p=0.9, seed=4, max_iter=MAX_ITER)
        assert np.array_equal(ids, got[0])
        got = eng.sample_decode(img, END, n=n, seed=5, max_iter=MAX_ITER, return_scores=True, allowed=al, prefix=PREFIX, prefix_lengths=LENS)
        assert _same(got, _direct(eng, img, n, _abi.LxoSampleOpts(1.0, 0, 1.0, 5), al, True))
        assert (got[0][0, :LENS[0]] == PREFIX[0, :LENS[0], None]).all() and all(al[b][got[0][b].reshape(-1)].all() for b in range(B))
    one = eng.sample_decode(img, END, n=3, seed=5, max_iter=MAX_ITER, allowed=al[0])                  # [V]: one set for the batch
    assert _same((one,), _direct(eng, img, 3, _abi.LxoSampleOpts(1.0, 0, 1.0, 5), np.repeat(al[:1], B, axis=0))[:1])
    ids, alpha, lp, lq = eng.sample_decode(img, END, n=3, seed=5, max_iter=MAX_ITER, return_scores=True, return_attention=True)
    assert alpha.shape[:3] == ids.shape and np.allclose(alpha.reshape(ids.shape + (-1,)).sum(-1), 1.0, atol=1e-4)
    assert _same((ids, lp, lq), eng.sample_decode(img, END, n=3, seed=5, max_iter=MAX_ITER, return_scores=True))


def test_temperature_zero_is_top_k_1_and_the_greedy_path(setup):
    eng, img = setup
    eng.max_steps, eng.ws = MS, None
    gid, glp = eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True)
    ids, lp, lq = eng.sample_decode(img, END, n=3, temperature=0, seed=9, max_iter=MAX_ITER, return_scores=True)
    assert _same((ids, lp, lq), eng.sample_decode(img, END, n=3, temperature=0.7, top_k=1, seed=1, max_iter=MAX_ITER, return_scores=True))
    for j in range(3):
        assert np.array_equal(ids[:, :, j], gid) and np.abs(lp[:, :, j] - glp).max() < 1e-5
    assert (lq == 0).all()


def test_sample_tokens_equals_the_direct_call(setup):
    eng, _ = setup
    lg = (np.random.RandomState(1).randn(6, V) * 2).astype(np.float32)
    al = np.ones((2, V), bool); al[1, :4] = False
    ids, lp, lq = eng.sample_tokens(lg, n=3, time=4, temperature=0.8, top_k=5, top_p=0.9, seed=2, allowed=al)
    bits = constraint_ref.pack_bits(al)
    o = _abi.LxoSampleOpts(0.8, 5, 0.9, 2)
    i2 = np.zeros(6, np.int32); p2 = np.zeros(6, np.float32); q2 = np.zeros(6, np.float32)
    assert eng.lib.lxo_sample_tokens(ptr(lg), V, 6, 3, V, 4, ctypes.byref(o), ptr(bits), 1, ptr(i2), ptr(p2), ptr(q2), None) == 0
    assert _same((ids, lp, lq), (i2, p2, q2)) and not np.isin(ids[3:], [0, 1, 2, 3]).any()
    big = eng.sample_tokens(np.tile(lg[:1], (32, 1)), n=16, time=0, seed=3)[0]                        # the select step alone: n up to 16 at any V
    assert big.shape == (32,) and len(set(big.tolist())) > 1
    import torch
    wide = torch.full((6, 12), 1.0e30); wide[:, :V] = torch.from_numpy(lg)                             # a view of padded rows is read in place
    assert _same(eng.sample_tokens(wide[:, :V], n=3, time=4, temperature=0.8, top_k=5, top_p=0.9, seed=2, allowed=al), (ids, lp, lq))


def test_refusals_before_any_launch():
    build_sim()
    eng = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=_abi.bind(ctypes.CDLL(SIM_SO)))
    img = pad_batch_images(synthetic.make_set(B, H, W, V, 2, 4, seed=5)[0])
    no_end = np.ones((B, V), bool); no_end[1, END] = False
    for kw in [dict(n=0), dict(n=17), dict(n=12), dict(temperature=-0.5), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature=1e-39), dict(temperature=1e-60), dict(top_k=-1),
               dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan")), dict(allowed=no_end), dict(allowed=np.ones((3, V), bool)),
               dict(prefix=np.full((B, 2), END, np.int32)), dict(prefix=PREFIX, prefix_lengths=np.array([MAX_ITER + 1, 0]))]:
        with pytest.raises(ValueError):
            eng.sample_decode(img, END, max_iter=MAX_ITER, **kw)
    assert not hasattr(eng, "_img") and eng.ws is None
    for kw in [dict(logits=np.zeros((4, V + 1), np.float32)), dict(logits=np.zeros(V, np.float32)), dict(logits=np.zeros((4, V), np.float32), time=-1),
               dict(logits=np.zeros((4, V), np.float32), n=2, allowed=np.ones((3, V), bool)), dict(logits=np.zeros((4, V), np.float32), top_p=2.0)]:
        with pytest.raises(ValueError):
            eng.sample_tokens(**kw)
