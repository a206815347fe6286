"""-m gpu: the label-smoothed loss on the MI355X.

1. lxo_ce_loss_smoothed on CONSTRUCTED logits written into ws region "logits" against the float64 reference of tests/smoothed_loss_ref.py -- the hipsim
   file's matrix (V = 33, 500, 1000, 1025, 48 rows, both dtypes, weights none / tok / row / both, eps 0.1 and 0.9, five cases, both padding poisons) --
   with its bit identities against lxo_ce_loss_weighted and lxo_ce_loss_fwd_bwd, what it refuses and what it may write.
2. The smoothed step end to end against autograd through the oracle (F.cross_entropy(label_smoothing=)), at tests/test_gpu_weighted_loss.py's 6 rows --
   in bf16 the chain batch of 8 on the persistent chains.
3. A smoothed step captured into a HIP graph, and the torch module's label_smoothing= (on while training, off in eval())."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from latex_ocr_amd import _abi
from latex_ocr_amd.engine import _p
import mrt_oracle
from smoothed_loss_ref import (POISONS, S_B as B, S_CASES, S_EPS, S_INV_NORM as INV_NORM, S_MODES, S_T as T, S_VOCABS, check_smoothed, make_case,
                               make_weights, mode_weights, padded, smoothed_grads, smoothed_reference, vpad)

H, W = 32, 128
EPS = 0.1
_engines = {}


def _head_engine(V, dtype):
    eng = _engines.get((V, dtype))
    if eng is None:
        eng = _engines[(V, dtype)] = Engine(V, dtype=dtype, seed=0)
    eng.ensure(B, H, W, T)
    return eng


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outputs(eng, n, Vp):
    loss = eng.region("loss")[:4].cpu().numpy().copy()
    raw = eng.region("dlogits", "ct")[:n * Vp].clone()
    return loss, raw.float().cpu().numpy().reshape(n, Vp), raw.view(torch.uint8).cpu().numpy()


def _write_logits(eng, x_p):
    eng.region("logits")[:x_p.size].copy_(torch.from_numpy(x_p.reshape(-1)))


def run_smoothed(eng, x_p, f, ln, eps, w_tok=None, w_row=None, inv_norm=INV_NORM, norm_dev=None):
    n, Vp = x_p.shape
    _write_logits(eng, x_p)
    keep = [_dev(f), _dev(ln), _dev(w_tok), _dev(w_row), _dev(norm_dev)]
    eng._ck(eng.lib.lxo_ce_loss_smoothed(eng.sref(), _p(eng.ws), _p(keep[0]), _p(keep[1]), ctypes.c_float(eps), _p(keep[2]), _p(keep[3]),
                                         ctypes.c_float(inv_norm), _p(keep[4]), eng._stream()), "ce_loss_smoothed")
    return _outputs(eng, n, Vp)


def run_weighted(eng, x_p, f, ln, w_tok, w_row, inv_norm=INV_NORM):
    n, Vp = x_p.shape
    _write_logits(eng, x_p)
    keep = [_dev(f), _dev(ln), _dev(w_tok), _dev(w_row)]
    eng._ck(eng.lib.lxo_ce_loss_weighted(eng.sref(), _p(eng.ws), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), ctypes.c_float(inv_norm),
                                         None, eng._stream()), "ce_loss_weighted")
    return _outputs(eng, n, Vp)


def run_plain(eng, x_p, f, ln, inv_ntok):
    n, Vp = x_p.shape
    _write_logits(eng, x_p)
    fd, ld = _dev(f), _dev(ln)
    eng._ck(eng.lib.lxo_ce_loss_fwd_bwd(eng.sref(), _p(eng.ws), _p(fd), _p(ld), ctypes.c_float(inv_ntok), eng._stream()), "ce_loss")
    return _outputs(eng, n, Vp)


# ------------------------------------------------------------------------------------------------- 1. the kernels on constructed inputs --
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", S_VOCABS)
def test_smoothed_loss_against_float64(V, dtype):
    eng = _head_engine(V, dtype)
    Vp = vpad(V)
    top = {}
    for case in S_CASES:
        x, f, ln = make_case(case, V, B, T, seed=1)
        w_tok, w_row = make_weights(ln, B, T, seed=2)
        xp = {poison: padded(x, Vp, poison) for poison in POISONS}
        for mode in S_MODES:
            wt, wr = mode_weights(mode, w_tok, w_row)
            # "loss"[1] and [3] are the weighted call's bytes with the same weights (no weights: every token weighing 1.f)
            base = run_weighted(eng, xp["nan"], f, ln, wt if mode != "none" else np.ones((B, T), np.float32), wr)[0]
            for eps in S_EPS:
                ref = smoothed_reference(x, f, ln, wt, wr, INV_NORM, eps)
                outs = [run_smoothed(eng, xp[poison], f, ln, eps, wt, wr) for poison in POISONS]
                loss, dl, raw = outs[0]
                worst = check_smoothed(ref, x, V, Vp, loss, dl, INV_NORM, bf16=dtype == "bf16")
                for k, v in worst.items():
                    if v > top.get(k, (-1.0, ""))[0]:
                        top[k] = (v, "%s %s eps=%g" % (case, mode, eps))
                assert outs[1][0].tobytes() == loss.tobytes() and outs[1][2].tobytes() == raw.tobytes(), (case, mode, eps)
                assert loss[1].tobytes() == base[1].tobytes() and loss[3].tobytes() == base[3].tobytes(), (case, mode, eps)
    print("V=%d %s, worst fractions of the bars: %s" % (V, dtype, ", ".join("%s %.3f (%s)" % (k, v, w) for k, (v, w) in sorted(top.items()))))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", S_VOCABS)
def test_eps_zero_is_the_weighted_and_the_plain_loss_bit_for_bit(V, dtype):
    eng = _head_engine(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=3)
    xp = padded(x, Vp, None)
    inv = np.float32(INV_NORM)
    w_tok, w_row = make_weights(ln, B, T, seed=4)
    for mode in S_MODES[1:]:
        wt, wr = mode_weights(mode, w_tok, w_row)
        want = run_weighted(eng, xp, f, ln, wt, wr, inv)
        got = run_smoothed(eng, xp, f, ln, 0.0, wt, wr, inv)
        assert got[2].tobytes() == want[2].tobytes() and got[0].tobytes() == want[0].tobytes(), mode
    base = run_plain(eng, xp, f, ln, inv)
    got = run_smoothed(eng, xp, f, ln, 0.0, None, None, inv)
    assert got[2].tobytes() == base[2].tobytes() and got[0][:2].tobytes() == base[0][:2].tobytes()
    assert got[0][2] == base[0][1] and got[0][3].tobytes() == base[0][0].tobytes()
    a = run_smoothed(eng, xp, f, ln, EPS, w_tok, w_row, np.float32(0.125))
    b = run_smoothed(eng, xp, f, ln, EPS, w_tok, w_row, 123.0, np.array([8.0], np.float32))
    assert a[2].tobytes() == b[2].tobytes() and a[0].tobytes() == b[0].tobytes()
    c = run_smoothed(eng, xp, f, ln, EPS, w_tok, w_row, np.float32(0.125))          # ordered slots: the same bytes in every run
    assert a[2].tobytes() == c[2].tobytes() and a[0].tobytes() == c[0].tobytes()


@pytest.mark.parametrize("V", (33, 1025))
def test_refusals_untouched_memory_and_the_chain_word(V):
    eng = _head_engine(V, "bf16")
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=5)
    w_tok, w_row = make_weights(ln, B, T, seed=6)
    xp = padded(x, Vp, None)
    clean = run_smoothed(eng, xp, f, ln, EPS, w_tok, w_row)
    # every -1 writes nothing
    fd, ld = _dev(f), _dev(ln)
    c = ctypes.c_float
    ok = dict(s=eng.sref(), ws=_p(eng.ws), f=_p(fd), ln=_p(ld), eps=c(EPS))
    torch.cuda.synchronize()
    before = eng.ws.clone()
    for kw in (dict(eps=c(1.0)), dict(eps=c(-0.1)), dict(eps=c(float("nan"))), dict(eps=c(float("inf"))), dict(ws=None), dict(f=None), dict(ln=None),
               dict(s=None)):
        a = dict(ok, **kw)
        assert eng.lib.lxo_ce_loss_smoothed(a["s"], a["ws"], a["f"], a["ln"], a["eps"], None, None, c(1.0), None, eng._stream()) == -1, kw
        assert eng.lib.lxo_last_error()
    torch.cuda.synchronize()
    assert torch.equal(eng.ws, before)
    # a call on a workspace full of 0xA5 outside what it reads: nothing but "dlogits", "loss" and "det_part" may change
    keep = {name: eng.region(name).clone() for name in ("logits", "xdec_sync")}
    eng.ws.fill_(0xA5)
    for name, raw in keep.items():
        eng.region(name).copy_(raw)
    before = eng.ws.clone()
    again = run_smoothed(eng, xp, f, ln, EPS, w_tok, w_row)
    assert again[0].tobytes() == clean[0].tobytes() and again[2].tobytes() == clean[2].tobytes()
    changed = (eng.ws != before).cpu().numpy()
    owned = np.zeros(changed.shape, bool)
    for name in ("dlogits", "loss", "det_part"):
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        eng._ck(eng.lib.lxo_ws_region(eng.sref(), name.encode(), ctypes.byref(off), ctypes.byref(nb)), "region")
        owned[off.value:off.value + nb.value] = True
    assert not (changed & ~owned).any(), np.flatnonzero(changed & ~owned)[:8]
    assert changed.any()
    eng.ws.zero_()
    # the forward chain's error word, set by hand and read by the loss kernel only: NaN in [0], the count as ever
    word = eng.region("xdec_sync", "i32")
    word[_abi.LXO_XDEC_ERR_WORD] = 3
    try:
        loss = run_smoothed(eng, xp, f, ln, EPS, w_tok, w_row)[0]
    finally:
        word[_abi.LXO_XDEC_ERR_WORD] = 0
    assert np.isnan(loss[0]) and loss[1] == clean[0][1] and loss[3].tobytes() == clean[0][3].tobytes()


# ------------------------------------------------------------------------------------------------------------ 2. end to end vs autograd --
CONV1_BF16 = 0.998       # tests/test_gpu_parity.py: conv1's kernel / bias in bf16


def _smoothed_grads_check(dtype, w, tol_loss, min_cos, norm=11.0):
    V, n = 50, 6
    img, f, l = batch(n, 32, 128, V, 5, 12, seed=7)
    eng = Engine(V, dtype=dtype, seed=3)
    P = oracle_params(eng)
    eng.forward(img, f)
    if dtype == "bf16":
        assert int(eng.shape.B) == 8 and int(eng.live_B) == 6       # the chain batch: two dead rows behind the six
    kw = dict(weights=w(f.shape)) if w is not None else {}
    stats = eng.loss(l, 1.0 / norm, label_smoothing=EPS, **kw).cpu().numpy()
    eng.backward()
    torch.cuda.synchronize()
    ref, G, ce = smoothed_grads(P, img, f, l, w(f.shape) if w is not None else np.ones(f.shape, np.float32), norm, EPS)
    loss = float(stats[0]) / norm
    assert stats.shape == (4,) and stats[1] == float(l.sum())
    assert abs(float(stats[3]) / float(stats[1]) - ce) / ce < tol_loss
    cs = mrt_oracle.cosines(eng.grad_dict(), G)
    print("%s%s: smoothed loss %.6f oracle %.6f rel %.2e; lowest gradient cosines %s" % (
        dtype, " weighted" if w is not None else "", loss, ref, abs(loss - ref) / abs(ref), ", ".join("%.6f %s" % (c, k.split("/", 1)[-1]) for c, k in cs[:3])))
    assert abs(loss - ref) / abs(ref) < tol_loss, (loss, ref)
    for c, k in cs:
        bar = CONV1_BF16 if (dtype == "bf16" and k.startswith("Encoder/convolutional_encoder/conv2d/")) else min_cos
        assert c > bar, (k, c)
    return eng


def test_smoothed_step_f32():
    _smoothed_grads_check("f32", None, 2e-5, 0.9999)


def test_smoothed_step_f32_mixed_sign_weights():
    _smoothed_grads_check("f32", lambda s: np.random.default_rng(5).uniform(-2.0, 2.0, size=s).astype(np.float32), 2e-5, 0.9999)


def test_smoothed_step_bf16_on_the_chain():
    eng = _smoothed_grads_check("bf16", None, 1e-3, 0.999)
    assert eng.chain_used, "the forward chain did not run"


def test_train_step_returns_the_smoothed_loss_and_keeps_the_plain_ce():
    V = 50
    img, f, l = batch(6, 32, 128, V, 5, 12, seed=7)
    eng = Engine(V, dtype="f32", seed=3)
    ref, _, ce = smoothed_grads(oracle_params(eng), img, f, l, np.ones(f.shape, np.float32), float(l.sum()), EPS)
    loss = eng.train_step(img, f, l, 1e-3, label_smoothing=EPS)
    assert abs(loss - ref) / abs(ref) < 2e-5 and abs(eng.last_ce - ce) / ce < 2e-5, (loss, ref, eng.last_ce, ce)
    a, b = Engine(V, dtype="f32", seed=3), Engine(V, dtype="f32", seed=3)
    la, lb = a.train_step(img, f, l, 1e-3), b.train_step(img, f, l, 1e-3, label_smoothing=0.0)
    assert la == lb and a.last_ce == b.last_ce == la and torch.equal(a.params, b.params)


# ------------------------------------------------------------------------------------------------- 3. graph capture, the torch module --
def test_smoothed_step_captured_into_a_graph():
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
        e.loss(l, 1.0 / 37.0, row_weights=wr, label_smoothing=EPS)
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


def test_torch_module_smooths_while_training_only():
    from latex_ocr_amd.model.img2seq_torch import Img2Seq
    V = 50
    img, f, l = batch(6, 32, 128, V, 5, 12, seed=7)
    ntok = float(l.sum())
    mod = Img2Seq(V, dtype="f32", seed=3, label_smoothing=EPS)
    eng = Engine(V, dtype="f32", seed=3)                            # the same initial weights
    eng.forward(img, f)
    st = eng.loss(l, 1.0 / ntok, label_smoothing=EPS).cpu().numpy()
    eng.backward()
    torch.cuda.synchronize()
    mod.train()
    loss = mod(img, f, l)
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss.detach()) == float(np.float32(st[0]) / np.float32(st[1]))          # (the module divides on the device, in f32)
    assert torch.equal(mod.flat.grad, eng.grads)
    # eval(): the plain loss, as a module without the argument
    eng.forward(img, f)
    plain = eng.loss(l, 1.0 / ntok).cpu().numpy()
    mod.eval()
    with torch.no_grad():
        le = mod(img, f, l)
    assert float(le) == float(np.float32(plain[0]) / np.float32(plain[1])) and float(le) != float(loss.detach())
    with pytest.raises(ValueError):
        Img2Seq(V, dtype="f32", seed=3, label_smoothing=1.0)
