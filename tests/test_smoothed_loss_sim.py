"""CPU (hipsim): the label-smoothed loss lxo_ce_loss_smoothed -- the <..., CeSmooth> and <..., CeWeights, CeSmooth> instantiations of
ce_loss_rows_kernel<KV = 4, 8, 16> and of the strided ce_loss_kernel -- on CONSTRUCTED logits against a float64 reference
(tests/smoothed_loss_ref.py), its bit identities with lxo_ce_loss_weighted and lxo_ce_loss_fwd_bwd, what it may write and what it refuses.  The
same checks run on the MI355X in tests/test_gpu_smoothed_loss.py."""
import ctypes

import numpy as np
import pytest

from simharness import Sim, ptr
from simlib import bf16_to_f32
from smoothed_loss_ref import (POISONS, S_B as B, S_CASES, S_EPS, S_INV_NORM as INV_NORM, S_MODES, S_T as T, S_VOCABS, check_smoothed, make_case,
                               make_weights, mode_weights, padded, smoothed_reference, vpad)

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
H, W = 32, 48

_sims = {}


def _sim(V, dtype):
    if (V, dtype) not in _sims:
        _sims[(V, dtype)] = Sim(B, H, W, T, V, dtype=dtype, seed=0, dims=SMALL)
    return _sims[(V, dtype)]


def _outputs(S, n, Vp):
    loss = S.region("loss", np.float32)[:4].copy()
    if S.dtype == 1:
        raw = S.region("dlogits", np.uint16)[:n * Vp].copy()
        dl = bf16_to_f32(raw).reshape(n, Vp)
    else:
        dl = S.region("dlogits", np.float32)[:n * Vp].reshape(n, Vp).copy()
        raw = dl.copy()
    return loss, dl, raw


def run_smoothed(S, logits_p, f, ln, eps, w_tok=None, w_row=None, inv_norm=INV_NORM, norm_dev=None):
    """write the padded logits into ws "logits", run the smoothed loss -> (loss [4], d(logits) f32 [n, Vp], its raw elements)"""
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    S.ck(S.L.lxo_ce_loss_smoothed(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ctypes.c_float(eps), ptr(w_tok), ptr(w_row), ctypes.c_float(inv_norm),
                                  ptr(norm_dev), None), "ce_s")
    return _outputs(S, n, Vp)


def run_weighted(S, logits_p, f, ln, w_tok, w_row, inv_norm=INV_NORM):
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    S.ck(S.L.lxo_ce_loss_weighted(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ptr(w_tok), ptr(w_row), ctypes.c_float(inv_norm), None, None), "ce_w")
    return _outputs(S, n, Vp)


def run_plain(S, logits_p, f, ln, inv_ntok):
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    S.ck(S.L.lxo_ce_loss_fwd_bwd(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ctypes.c_float(inv_ntok), None), "ce")
    return _outputs(S, n, Vp)


@pytest.mark.parametrize("case", S_CASES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", S_VOCABS)
def test_smoothed_loss_against_float64(V, dtype, case):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case(case, V, B, T, seed=1)
    w_tok, w_row = make_weights(ln, B, T, seed=2)
    xp = {poison: padded(x, Vp, poison) for poison in POISONS}
    for mode in S_MODES:
        wt, wr = mode_weights(mode, w_tok, w_row)
        # "loss"[1] and [3] are the weighted call's bytes with the same weights (no weights: every token weighing 1.f)
        base = run_weighted(S, xp["nan"], f, ln, wt if mode != "none" else np.ones((B, T), np.float32), wr)[0]
        for eps in S_EPS:
            ref = smoothed_reference(x, f, ln, wt, wr, INV_NORM, eps)
            outs = [run_smoothed(S, xp[poison], f, ln, eps, wt, wr) for poison in POISONS]
            loss, dl, raw = outs[0]
            worst = check_smoothed(ref, x, V, Vp, loss, dl, INV_NORM, bf16=dtype == 1)
            print("V=%d %s %s %s eps=%g: d(logits) at %.2f of its bar, row sums %.2f, sum w L %.2f, sum w %.2f, sum CE %.2f of theirs"
                  % (V, ("f32", "bf16")[dtype], case, mode, eps, worst["dlogits"], worst["rowsum"], worst["loss0"], worst["loss2"], worst["loss3"]))
            # either poison in [V, Vp): the same bytes (a NaN or 1e30 read into the logit sum would show in [0])
            assert outs[1][0].tobytes() == loss.tobytes() and outs[1][2].tobytes() == raw.tobytes()
            assert loss[1].tobytes() == base[1].tobytes() and loss[3].tobytes() == base[3].tobytes()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", S_VOCABS)
def test_eps_zero_is_the_weighted_and_the_plain_loss_bit_for_bit(V, dtype):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=3)
    xp = padded(x, Vp, None)
    inv = np.float32(INV_NORM)
    w_tok, w_row = make_weights(ln, B, T, seed=4)
    for mode in S_MODES[1:]:
        wt, wr = mode_weights(mode, w_tok, w_row)
        want = run_weighted(S, xp, f, ln, wt, wr, inv)
        got = run_smoothed(S, xp, f, ln, 0.0, wt, wr, inv)
        assert got[2].tobytes() == want[2].tobytes() and got[0].tobytes() == want[0].tobytes(), mode
    base = run_plain(S, xp, f, ln, inv)
    got = run_smoothed(S, xp, f, ln, 0.0, None, None, inv)
    assert got[2].tobytes() == base[2].tobytes() and got[0][:2].tobytes() == base[0][:2].tobytes()
    assert got[0][2] == base[0][1] and got[0][3].tobytes() == base[0][0].tobytes()          # sum w = the count, sum CE = sum 1 L
    # the normaliser read from device memory: 1 / norm_dev[0] replaces inv_norm (1 / 8 is exact)
    a = run_smoothed(S, xp, f, ln, 0.1, w_tok, w_row, np.float32(0.125))
    b = run_smoothed(S, xp, f, ln, 0.1, w_tok, w_row, 123.0, np.array([8.0], np.float32))
    assert a[2].tobytes() == b[2].tobytes() and a[0].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", (33, 1025))
def test_untouched_memory(V, dtype):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=5)
    w_tok, w_row = make_weights(ln, B, T, seed=6)
    for wt, wr in ((None, None), (w_tok, w_row)):
        clean = run_smoothed(S, padded(x, Vp, None), f, ln, 0.1, wt, wr)
        # a second call on a workspace full of 0xA5 outside what the call owns: nothing but "dlogits", "loss" and "det_part" may change
        keep = {name: S.region(name, np.uint8).copy() for name in ("logits", "xdec_sync")}        # what the call reads
        S.ws[:] = 0xA5
        for name, raw in keep.items():
            S.region(name, np.uint8)[:] = raw
        before = S.ws.copy()
        again = run_smoothed(S, padded(x, Vp, None), f, ln, 0.1, wt, wr)
        assert again[0].tobytes() == clean[0].tobytes() and again[2].tobytes() == clean[2].tobytes()
        changed = S.ws != before
        owned = np.zeros(S.ws.shape, bool)
        for name in ("dlogits", "loss", "det_part"):
            off, nb = ctypes.c_size_t(), ctypes.c_size_t()
            S.ck(S.L.lxo_ws_region(S.sref(), name.encode(), ctypes.byref(off), ctypes.byref(nb)), "region")
            owned[off.value:off.value + nb.value] = True
        assert not (changed & ~owned).any(), np.flatnonzero(changed & ~owned)[:8]
        assert changed.any()
        S.ws[:] = 0


def test_failed_chain_word_poisons_the_smoothed_loss():
    from latex_ocr_amd import _abi
    S = _sim(33, 1)
    x, f, ln = make_case("normal", 33, B, T, seed=7)
    S.region("xdec_sync", np.int32)[_abi.LXO_XDEC_ERR_WORD] = 3
    try:
        loss = run_smoothed(S, padded(x, vpad(33), None), f, ln, 0.1)[0]
    finally:
        S.region("xdec_sync", np.int32)[_abi.LXO_XDEC_ERR_WORD] = 0
    assert np.isnan(loss[0]) and loss[1] == float((np.arange(T)[None, :] < ln[:, None]).sum())


def test_refusals_write_nothing():
    S = _sim(33, 0)
    x, f, ln = make_case("normal", 33, B, T, seed=7)
    S.write_region("logits", padded(x, vpad(33), None))
    before = S.ws.copy()
    c = ctypes.c_float
    ok = dict(s=S.sref(), ws=ptr(S.ws), f=ptr(f), ln=ptr(ln), eps=c(0.1))
    bad = [dict(eps=c(1.0)), dict(eps=c(1.5)), dict(eps=c(-0.1)), dict(eps=c(-1e-30)), dict(eps=c(float("nan"))), dict(eps=c(float("inf"))),
           dict(eps=c(float("-inf"))), dict(ws=None), dict(f=None), dict(ln=None), dict(s=None)]
    for kw in bad:
        a = dict(ok, **kw)
        rc = S.L.lxo_ce_loss_smoothed(a["s"], a["ws"], a["f"], a["ln"], a["eps"], None, None, c(1.0), None, None)
        assert rc == -1 and S.L.lxo_last_error(), kw
        assert np.array_equal(S.ws, before), kw
    # the largest f32 below 1 is inside [0, 1)
    S.ck(S.L.lxo_ce_loss_smoothed(ok["s"], ok["ws"], ok["f"], ok["ln"], c(float(np.nextafter(np.float32(1), np.float32(0)))), None, None, c(1.0), None,
                                  None), "ce_s")
