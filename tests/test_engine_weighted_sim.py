"""CPU (hipsim): Engine.loss(weights=, row_weights=), Engine.train_step(..., weights=, row_weights=, norm=) and Engine.mrt_step -- the weighted loss
and the minimum-risk step end to end -- against autograd through oracle/ref_model.py (tests/mrt_oracle.py): of sum w CE / norm for the first, of
the TRUE expected cost (1 / G) sum_g sum_c softmax_c(alpha seq_logp) cost for the second, which holds the weight formula itself.  And every
ValueError the three raise before a launch."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
from simlib import SIM_SO, build_sim
import mrt_oracle

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, T, H, W = 11, 5, 32, 48
LOSS_TOL, MIN_COS = 2e-5, 0.9999        # tests/test_gpu_parity.py's f32 bars; the cosine one decade looser: signed weights cancel signal, not rounding noise


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


def _engine(lib, seed=3):
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=seed, lib=lib)


def _batch(B, seed):
    imgs, _ = synthetic.make_set(B, H, W, V, 2, 4, seed=seed)
    rng = np.random.default_rng(seed)
    f = rng.integers(0, V, size=(B, T)).astype(np.int32)
    return pad_batch_images(imgs), f


def _oracle_params(eng):
    return {k: torch.from_numpy(v.copy()) for k, v in eng.get_params().items()}


def _report(what, loss, ref, cs):
    err = abs(loss - ref) / abs(ref)
    print("%s: loss %.7f oracle %.7f rel %.2e; lowest gradient cosines %s" % (what, loss, ref, err, ", ".join("%.7f %s" % (c, k.split("/", 1)[-1]) for c, k in cs[:3])))
    assert err < LOSS_TOL, (loss, ref)
    for c, k in cs:
        assert c > MIN_COS, (k, c)


def test_mixed_sign_token_weights_against_autograd(lib):
    eng = _engine(lib)
    img, f = _batch(3, seed=5)
    ln = np.array([5, 2, 4], np.int32)
    rng = np.random.default_rng(1)
    w = rng.uniform(-2.0, 2.0, size=(3, T)).astype(np.float32)
    w[0, 1] = 0.0
    norm = 7.0
    eng.forward(img, f)
    stats = eng.loss(ln, 1.0 / norm, weights=w).numpy().copy()
    eng.backward()
    ref, G = mrt_oracle.weighted_grads(_oracle_params(eng), img, f, ln, w, norm)
    assert stats.shape == (4,) and stats[1] == float(ln.sum())
    live = np.arange(T)[None, :] < ln[:, None]
    assert abs(stats[2] - float(w[live].sum(dtype=np.float64))) <= 2.0 ** -22 * float(np.abs(w[live]).sum())
    _report("weights [B, T]", float(stats[0]) / norm, ref, mrt_oracle.cosines(eng.grad_dict(), G))
    # the same weights split into a token and a row factor: the f32 product on the device
    wr = np.array([0.5, -2.0, 4.0], np.float32)
    eng.forward(img, f)
    s2 = eng.loss(ln, 1.0 / norm, weights=w, row_weights=torch.from_numpy(wr)).numpy().copy()
    eng.backward()
    ref2, G2 = mrt_oracle.weighted_grads(_oracle_params(eng), img, f, ln, w * wr[:, None], norm)
    _report("weights x row_weights", float(s2[0]) / norm, ref2, mrt_oracle.cosines(eng.grad_dict(), G2))
    # without weights the call is the one it was
    eng.forward(img, f)
    s3 = eng.loss(ln, 1.0 / float(ln.sum()))
    assert s3.shape == (2,) and abs(float(s3[0]) - float(s2[3])) <= 1e-6 * abs(float(s2[3]))


def test_train_step_weighted_returns_the_weighted_loss(lib):
    eng = _engine(lib)
    img, f = _batch(3, seed=6)
    ln = np.array([3, 5, 1], np.int32)
    wr = np.array([1.5, -0.5, 0.25], np.float32)
    P = _oracle_params(eng)
    ref, _ = mrt_oracle.weighted_grads(P, img, f, ln, np.repeat(wr[:, None], T, 1), 4.0)
    before = eng.params.clone()
    loss = eng.train_step(img, f, ln, 1e-3, row_weights=wr, norm=4.0)
    assert abs(loss - ref) / abs(ref) < LOSS_TOL, (loss, ref)
    assert not torch.equal(eng.params, before)
    # norm = None: the token count, as without weights
    eng2 = _engine(lib)
    ref2, _ = mrt_oracle.weighted_grads(P, img, f, ln, np.repeat(wr[:, None], T, 1), float(ln.sum()))
    loss2 = eng2.train_step(img, f, ln, 1e-3, row_weights=wr)
    assert abs(loss2 - ref2) / abs(ref2) < LOSS_TOL, (loss2, ref2)


def test_mrt_step_against_autograd_of_the_true_risk(lib):
    eng = _engine(lib, seed=4)
    img, _ = _batch(2, seed=7)
    gs = np.array([3, 2], np.int64)
    rng = np.random.default_rng(2)
    cand = rng.integers(0, V, size=(5, T)).astype(np.int32)
    ln = np.array([5, 3, 4, 2, 5], np.int32)
    cost = np.array([0.0, 0.8, 1.25, 0.5, 0.1], np.float32)
    alpha = 0.7
    P = _oracle_params(eng)
    risk_ref, G, q_ref = mrt_oracle.mrt_grads(P, img, cand, ln, gs, cost, alpha)
    # the gradient, read before the optimizer step
    risk_d, q_d, w_d = eng.mrt_grads(img, cand, ln, gs, cost, alpha)
    risk, q, w = float(risk_d[0]) / 2, q_d.numpy().copy(), w_d.numpy().copy()
    _report("mrt", risk, risk_ref, mrt_oracle.cosines(eng.grad_dict(), G))
    assert np.abs(q - q_ref).max() <= 1e-5, np.abs(q - q_ref).max()
    for lo, hi in ((0, 3), (3, 5)):
        assert abs(float(q[lo:hi].sum(dtype=np.float64)) - 1.0) <= 1e-5
        assert abs(float(w[lo:hi].sum(dtype=np.float64))) <= 1e-6 * alpha, w[lo:hi]
    # the whole step on a copy of the parameters: the same risk and q, and an update
    eng2 = _engine(lib, seed=4)
    eng2.load_params(copy.deepcopy(eng.get_params()))
    before = eng2.params.clone()
    risk2, q2 = eng2.mrt_step(img, cand, ln, gs, cost, 1e-3, alpha)
    assert abs(risk2 - risk_ref) <= 1e-5 and np.abs(q2 - q_ref).max() <= 1e-5 and q2.shape == (5,)
    assert risk2 == risk and q2.tobytes() == q.tobytes()
    assert not torch.equal(eng2.params, before) and eng2.adam_t == 1


def test_refusals_before_any_launch(lib):
    img, f = _batch(3, seed=5)
    ln = np.array([5, 2, 4], np.int32)
    ok_w, ok_r = np.ones((3, T), np.float32), np.ones(3, np.float32)
    nan_w = ok_w.copy(); nan_w[1, 2] = np.nan
    inf_r = ok_r.copy(); inf_r[0] = np.inf
    bad_weights = [dict(weights=np.ones((3, T + 1), np.float32)), dict(weights=np.ones((2, T), np.float32)), dict(weights=nan_w),
                   dict(row_weights=np.ones(4, np.float32)), dict(row_weights=np.ones((3, 1), np.float32)), dict(row_weights=inf_r),
                   dict(weights=ok_w, row_weights=inf_r), dict(weights=torch.ones(3, T + 1)), dict(row_weights=torch.ones(2)),
                   dict(row_weights=np.array(["a", "b", "c"]))]
    eng = _engine(lib)
    for kw in bad_weights + [dict(row_weights=ok_r, norm=0.0), dict(row_weights=ok_r, norm=float("nan")), dict(norm=float("inf"))]:
        with pytest.raises(ValueError):
            eng.train_step(img, f, ln, 1e-3, **kw)
    assert not hasattr(eng, "_img") and eng.ws is None and eng.adam_t == 0
    cand = np.zeros((5, T), np.int32)
    cl, cost, gs = np.full(5, 3, np.int32), np.zeros(5, np.float32), np.array([3, 2])
    nan_c = cost.copy(); nan_c[4] = np.nan
    for kw in [dict(group_sizes=np.array([3, 3])), dict(group_sizes=np.array([5, 0])), dict(group_sizes=np.array([5])), dict(cost=nan_c),
               dict(cost=np.array([0, 0, 0, 0, 1e39])), dict(cost=cost[:4]), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")),
               dict(alpha=float("inf")), dict(cand_lengths=np.full(5, T + 1, np.int32)), dict(cand_lengths=cl[:4])]:
        args = dict(cand_lengths=cl, group_sizes=gs, cost=cost, alpha=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.mrt_step(img[:2], cand, args["cand_lengths"], args["group_sizes"], args["cost"], 1e-3, args["alpha"])
    assert not hasattr(eng, "_img") and eng.ws is None and eng.adam_t == 0
    # loss(): after a forward, refused before its launch -- the workspace keeps every byte
    eng.forward(img, f)
    before = eng.ws.clone()
    for kw in bad_weights:
        with pytest.raises(ValueError):
            eng.loss(ln, 1.0, **kw)
    assert torch.equal(eng.ws, before)
