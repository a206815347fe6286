"""-m gpu: the weighted loss and the minimum-risk step on the MI355X.

1. lxo_ce_loss_weighted on CONSTRUCTED logits written into ws region "logits" against the float64 reference of tests/weighted_loss_ref.py (the
   hipsim file's matrix at V = 33, 500, 1025 and 48 rows), with its bit identities against lxo_ce_loss_fwd_bwd; lxo_mrt_weights against its own.
2. The weighted step end to end against autograd through the oracle (tests/mrt_oracle.py), at 6 rows -- in bf16 the chain batch of 8, so the
   zero weights of the dead rows ride the persistent chains.  bf16 with SIGNED weights is held at the d(logits) level in 1.: the backward is
   untouched and linear in d(logits).
3. Engine.mrt_step in bf16 on the chains, and a weighted step captured into a HIP graph."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from latex_ocr_amd.engine import _p
import mrt_oracle
from weighted_loss_ref import (MRT_ALPHAS, W_CASES, W_MODES, check_mrt, check_weighted, make_case, make_mrt_case, make_weights, padded, vpad,
                               weighted_reference)

H, W = 32, 128
B, T = 8, 6
INV_NORM = 1.0 / 7.0
_engines = {}


def _head_engine(V, dtype):
    eng = _engines.get((V, dtype))
    if eng is None:
        eng = _engines[(V, dtype)] = Engine(V, dtype=dtype, seed=0)
    eng.ensure(B, H, W, T)
    return eng


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outputs(eng, n, Vp):
    loss = eng.region("loss")[:4].cpu().numpy().copy()
    raw = eng.region("dlogits", "ct")[:n * Vp].clone()
    return loss, raw.float().cpu().numpy().reshape(n, Vp), raw.view(torch.uint8).cpu().numpy()


def run_weighted(eng, x_p, f, ln, w_tok, w_row, inv_norm=INV_NORM, norm_dev=None):
    n, Vp = x_p.shape
    eng.region("logits")[:n * Vp].copy_(torch.from_numpy(x_p.reshape(-1)))
    keep = [_dev(f), _dev(ln), _dev(w_tok), _dev(w_row), _dev(norm_dev)]
    eng._ck(eng.lib.lxo_ce_loss_weighted(eng.sref(), _p(eng.ws), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), ctypes.c_float(inv_norm),
                                         _p(keep[4]), eng._stream()), "ce_loss_weighted")
    return _outputs(eng, n, Vp)


def run_plain(eng, x_p, f, ln, inv_ntok):
    n, Vp = x_p.shape
    eng.region("logits")[:n * Vp].copy_(torch.from_numpy(x_p.reshape(-1)))
    fd, ld = _dev(f), _dev(ln)
    eng._ck(eng.lib.lxo_ce_loss_fwd_bwd(eng.sref(), _p(eng.ws), _p(fd), _p(ld), ctypes.c_float(inv_ntok), eng._stream()), "ce_loss")
    return _outputs(eng, n, Vp)


# ------------------------------------------------------------------------------------------------- 1. the kernels on constructed inputs --
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", [33, 500, 1025])
def test_weighted_loss_against_float64(V, dtype):
    eng = _head_engine(V, dtype)
    Vp = vpad(V)
    for case in W_CASES:
        x, f, ln = make_case(case, V, B, T, seed=1)
        w_tok, w_row = make_weights(ln, B, T, seed=2)
        for mode in W_MODES:
            wt, wr = {"tok": (w_tok, None), "row": (None, w_row), "both": (w_tok, w_row)}[mode]
            ref = weighted_reference(x, f, ln, wt, wr, INV_NORM)
            loss, dl, _ = run_weighted(eng, padded(x, Vp, None), f, ln, wt, wr)
            worst = check_weighted(ref, x, V, Vp, loss, dl, INV_NORM, bf16=dtype == "bf16")
            print("V=%d %s %s %s: d(logits) at %.2f of its bar, sum w CE %.2f, sum w %.2f, sum CE %.2f of theirs"
                  % (V, dtype, case, mode, worst["dlogits"], worst["loss0"], worst["loss2"], worst["loss3"]))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", [33, 500, 1025])
def test_bit_identities_with_the_unweighted_loss(V, dtype):
    eng = _head_engine(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=3)
    xp = padded(x, Vp, None)
    inv = np.float32(INV_NORM)
    base = run_plain(eng, xp, f, ln, inv)
    ones = run_weighted(eng, xp, f, ln, np.ones((B, T), np.float32), None, inv)
    assert ones[2].tobytes() == base[2].tobytes() and ones[0][:2].tobytes() == base[0][:2].tobytes()
    for c in (0.375, -3.0):
        got = run_weighted(eng, xp, f, ln, None, np.full(B, c, np.float32), inv)
        want = run_plain(eng, xp, f, ln, np.float32(c) * np.float32(inv))
        assert got[2].tobytes() == want[2].tobytes(), c
    w_tok, w_row = make_weights(ln, B, T, seed=4)
    a = run_weighted(eng, xp, f, ln, w_tok, w_row, np.float32(0.125))
    b = run_weighted(eng, xp, f, ln, w_tok, w_row, 123.0, np.array([8.0], np.float32))
    assert a[2].tobytes() == b[2].tobytes() and a[0].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("alpha", MRT_ALPHAS)
def test_mrt_weights_against_float64(alpha):
    eng = _head_engine(33, "f32")
    lp, cost, off, rows = make_mrt_case()
    d = [_dev(lp), _dev(cost), _dev(off)]

    def run(G=len(off) - 1, offs=d[2]):
        w = torch.full((rows,), 7.0, device="cuda"); q = torch.full((rows,), 7.0, device="cuda"); r = torch.full((1,), 7.0, device="cuda")
        eng._ck(eng.lib.lxo_mrt_weights(_p(d[0]), _p(d[1]), _p(offs), G, rows, ctypes.c_float(alpha), _p(w), _p(q), _p(r), eng._stream()), "mrt")
        return w.cpu().numpy(), q.cpu().numpy(), r.cpu().numpy()
    w, q, risk = run()
    worst = check_mrt(lp, cost, off, alpha, w, q, risk[0])
    print("alpha %g: w at %.2f, q at %.2f, risk at %.2f of their bars" % (alpha, worst["w"], worst["q"], worst["risk"]))
    w2, q2, risk2 = run()
    assert w2.tobytes() == w.tobytes() and q2.tobytes() == q.tobytes() and risk2.tobytes() == risk.tobytes()
    w0, q0, r0 = run(0, torch.zeros(1, dtype=torch.int32, device="cuda"))          # G == 0: every row weighs nothing
    assert (w0 == 0).all() and (q0 == 0).all() and r0[0] == 0
    for args in ((None, _p(d[1]), _p(d[2]), 6, rows, ctypes.c_float(alpha), _p(d[0])), (_p(d[0]), _p(d[1]), _p(d[2]), 6, rows, ctypes.c_float(alpha), None),
                 (_p(d[0]), _p(d[1]), _p(d[2]), -1, rows, ctypes.c_float(alpha), _p(d[0])), (_p(d[0]), _p(d[1]), _p(d[2]), 6, rows, ctypes.c_float(float("nan")), _p(d[0]))):
        assert eng.lib.lxo_mrt_weights(*args, None, None, eng._stream()) == -1 and eng.lib.lxo_last_error()


# ------------------------------------------------------------------------------------------------------------ 2. end to end vs autograd --
CONV1_BF16 = 0.998       # tests/test_gpu_parity.py: conv1's kernel / bias in bf16


def _weighted_grads_check(dtype, w, tol_loss, min_cos, norm=11.0):
    V, n = 50, 6
    img, f, l = batch(n, 32, 128, V, 5, 12, seed=7)
    eng = Engine(V, dtype=dtype, seed=3)
    P = oracle_params(eng)
    eng.forward(img, f)
    if dtype == "bf16":
        assert int(eng.shape.B) == 8 and int(eng.live_B) == 6       # the chain batch: two dead rows, whose weights loss() appends as zeros
    stats = eng.loss(l, 1.0 / norm, weights=w(f.shape)).cpu().numpy()
    eng.backward()
    torch.cuda.synchronize()
    ref, G = mrt_oracle.weighted_grads(P, img, f, l, w(f.shape), norm)
    loss = float(stats[0]) / norm
    assert stats[1] == float(l.sum())
    cs = mrt_oracle.cosines(eng.grad_dict(), G)
    print("%s: weighted loss %.6f oracle %.6f rel %.2e; lowest gradient cosines %s" % (
        dtype, loss, ref, abs(loss - ref) / abs(ref), ", ".join("%.6f %s" % (c, k.split("/", 1)[-1]) for c, k in cs[:3])))
    assert abs(loss - ref) / abs(ref) < tol_loss, (loss, ref)
    for c, k in cs:
        bar = CONV1_BF16 if (dtype == "bf16" and k.startswith("Encoder/convolutional_encoder/conv2d/")) else min_cos
        assert c > bar, (k, c)
    return eng


def test_weighted_step_f32_mixed_sign():
    _weighted_grads_check("f32", lambda s: np.random.default_rng(5).uniform(-2.0, 2.0, size=s).astype(np.float32), 2e-5, 0.9999)


def test_weighted_step_bf16_positive_weights():
    eng = _weighted_grads_check("bf16", lambda s: np.random.default_rng(6).uniform(0.25, 2.0, size=s).astype(np.float32), 1e-3, 0.999)
    assert eng.chain_used, "the forward chain did not run"


# ------------------------------------------------------------------------------------------------------- 3. mrt_step, graph capture --
def _mrt_inputs(V=50):
    img, f, l = batch(2, 32, 128, V, 5, 9, seed=13)
    rng = np.random.default_rng(3)
    cand = rng.integers(0, V - 2, size=(6, 8)).astype(np.int32)
    ln = np.array([8, 5, 6, 3, 8, 7], np.int32)
    cost = np.array([0.0, 0.5, 1.0, 0.25, 0.0, 2.0], np.float32)
    return img, cand, ln, np.array([3, 3]), cost


def test_mrt_step_bf16_on_the_chains():
    img, cand, ln, gs, cost = _mrt_inputs()
    out = []
    for _ in range(2):
        eng = Engine(50, dtype="bf16", seed=4, deterministic=True)
        risk, q = eng.mrt_step(img, cand, ln, gs, cost, 1e-3, 1.0)
        assert int(eng.shape.B) == 8 and int(eng.live_B) == 6
        print("mrt_step bf16: chain_used %s chain_used_bwd %s, risk %.6f, q %s" % (eng.chain_used, eng.chain_used_bwd, risk, q.tolist()))
        assert eng.chain_used and eng.chain_used_bwd
        assert np.isfinite(risk) and q.shape == (6,)
        assert abs(float(q[:3].sum(dtype=np.float64)) - 1.0) <= 1e-5 and abs(float(q[3:].sum(dtype=np.float64)) - 1.0) <= 1e-5
        out.append(q)
    assert out[0].tobytes() == out[1].tobytes()                   # deterministic mode: the same q bit for bit from a second engine


def test_weighted_step_captured_into_a_graph():
    V, Bg = 50, 16
    img, f, l = batch(Bg, 32, 128, V, 5, 20, seed=11)
    img, f, l = torch.from_numpy(img).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(l.astype(np.int32)).cuda()
    wr = torch.from_numpy(np.random.default_rng(7).uniform(-1.0, 2.0, size=Bg).astype(np.float32)).cuda()

    def fresh():
        e = Engine(V, dtype="bf16", seed=3, deterministic=True)
        e.set_optimizer("sgd")
        return e

    def body(e):
        e.forward(img, f)
        e.loss(l, 1.0 / 37.0, row_weights=wr)
        e.backward()
        e.optimizer_step(0.05)

    def stats(e):
        return e.region("loss")[:4].cpu().numpy().tobytes()
    ref, want = fresh(), []
    for _ in range(3):
        body(ref)
        want.append(stats(ref))
    eng = fresh()
    body(eng)
    got = [stats(eng)]
    assert eng.chain_used and eng.chain_used_bwd
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body(eng)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        got.append(stats(eng))
    assert got == want
    assert torch.equal(eng.params, ref.params)
