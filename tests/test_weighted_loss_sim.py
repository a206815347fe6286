"""CPU (hipsim): the weighted loss lxo_ce_loss_weighted -- the W = CeWeights instantiations of ce_loss_rows_kernel<KV = 4, 8, 16> and of the strided
ce_loss_kernel -- on CONSTRUCTED logits against a float64 reference (tests/weighted_loss_ref.py), its bit identities with lxo_ce_loss_fwd_bwd, what
it may write, and the minimum-risk weights lxo_mrt_weights.  The same checks run on the MI355X in tests/test_gpu_weighted_loss.py."""
import ctypes

import numpy as np
import pytest

from simharness import Sim, ptr
from simlib import bf16_to_f32
from weighted_loss_ref import (MRT_ALPHAS, W_CASES, W_MODES, check_mrt, check_weighted, make_case, make_mrt_case, make_weights, padded, vpad,
                               weighted_reference)

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
H, W = 32, 48
B, T = 3, 4                        # 12 rows: three workgroups of four waves
W_VOCABS = (4, 33, 257, 513, 1025)          # KV = 4 (twice: the smallest shape, the worst padding), 8, 16, the strided kernel
INV_NORM = 1.0 / 7.0

_sims = {}


def _sim(V, dtype):
    if (V, dtype) not in _sims:
        _sims[(V, dtype)] = Sim(B, H, W, T, V, dtype=dtype, seed=0, dims=SMALL)
    return _sims[(V, dtype)]


def _outputs(S, n, Vp):
    loss = S.region("loss", np.float32)[:4].copy()
    if S.dtype == 1:
        dl = bf16_to_f32(S.region("dlogits", np.uint16)[:n * Vp].copy()).reshape(n, Vp)
        raw = S.region("dlogits", np.uint16)[:n * Vp].copy()
    else:
        dl = S.region("dlogits", np.float32)[:n * Vp].reshape(n, Vp).copy()
        raw = dl.copy()
    return loss, dl, raw


def run_weighted(S, logits_p, f, ln, w_tok, w_row, inv_norm=INV_NORM, norm_dev=None):
    """write the padded logits into ws "logits", run the weighted loss -> (loss [4], d(logits) f32 [n, Vp], its raw elements)"""
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    S.ck(S.L.lxo_ce_loss_weighted(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ptr(w_tok), ptr(w_row), ctypes.c_float(inv_norm), ptr(norm_dev), None), "ce_w")
    return _outputs(S, n, Vp)


def run_plain(S, logits_p, f, ln, inv_ntok):
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    S.ck(S.L.lxo_ce_loss_fwd_bwd(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ctypes.c_float(inv_ntok), None), "ce")
    return _outputs(S, n, Vp)


def _modes(w_tok, w_row):
    return {"tok": (w_tok, None), "row": (None, w_row), "both": (w_tok, w_row)}


@pytest.mark.parametrize("case", W_CASES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", W_VOCABS)
def test_weighted_loss_against_float64(V, dtype, case):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case(case, V, B, T, seed=1)
    w_tok, w_row = make_weights(ln, B, T, seed=2)
    live = np.arange(T)[None, :] < ln[:, None]
    assert (w_tok[live] == 0).any() and (w_row == 0).any() and (w_tok < 0).any() and (w_tok > 0).any()
    for mode in W_MODES:
        wt, wr = _modes(w_tok, w_row)[mode]
        ref = weighted_reference(x, f, ln, wt, wr, INV_NORM)
        loss, dl, _ = run_weighted(S, padded(x, Vp, None), f, ln, wt, wr)
        worst = check_weighted(ref, x, V, Vp, loss, dl, INV_NORM, bf16=dtype == 1)
        print("V=%d %s %s %s: d(logits) at %.2f of its bar, sum w CE %.2f, sum w %.2f, sum CE %.2f of theirs"
              % (V, ("f32", "bf16")[dtype], case, mode, worst["dlogits"], worst["loss0"], worst["loss2"], worst["loss3"]))


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", W_VOCABS)
def test_bit_identities_with_the_unweighted_loss(V, dtype):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=3)
    xp = padded(x, Vp, None)
    inv = np.float32(INV_NORM)
    base = run_plain(S, xp, f, ln, inv)
    # every token weighs 1.0f: the unweighted call's d(logits) and its two statistics
    ones = run_weighted(S, xp, f, ln, np.ones((B, T), np.float32), None, inv)
    assert ones[2].tobytes() == base[2].tobytes() and ones[0][:2].tobytes() == base[0][:2].tobytes()
    assert ones[0][2] == base[0][1] and ones[0][3].tobytes() == base[0][0].tobytes()        # sum w = the count, sum CE = sum 1 CE
    # every row weighs c: the unweighted call at inv_ntok = c * inv_norm, the f32 product (its loss[0] is sum CE, not c sum CE: not compared)
    for c in (0.375, -3.0):
        got = run_weighted(S, xp, f, ln, None, np.full(B, c, np.float32), inv)
        want = run_plain(S, xp, f, ln, np.float32(c) * np.float32(inv))
        assert got[2].tobytes() == want[2].tobytes(), c
        assert got[0][1] == want[0][1]
    # the normaliser read from device memory: 1 / norm_dev[0] replaces inv_norm
    w_tok, w_row = make_weights(ln, B, T, seed=4)
    norm = np.array([8.0], np.float32)                             # (1 / 8 is exact: the f32 quotient on the device is the host's constant)
    a = run_weighted(S, xp, f, ln, w_tok, w_row, np.float32(0.125))
    b = run_weighted(S, xp, f, ln, w_tok, w_row, 123.0, norm)
    assert a[2].tobytes() == b[2].tobytes() and a[0].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", (33, 1025))
def test_untouched_memory_and_poisoned_padding(V, dtype):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=5)
    w_tok, w_row = make_weights(ln, B, T, seed=6)
    clean = run_weighted(S, padded(x, Vp, None), f, ln, w_tok, w_row)
    # a second call on a workspace full of 0xA5 outside what the call owns: nothing but "dlogits", "loss" and "det_part" may change
    keep = {}
    for name in ("logits", "xdec_sync"):                           # what the call reads
        keep[name] = S.region(name, np.uint8).copy()
    S.ws[:] = 0xA5
    for name, raw in keep.items():
        S.region(name, np.uint8)[:] = raw
    before = S.ws.copy()
    again = run_weighted(S, padded(x, Vp, None), f, ln, w_tok, w_row)
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
    # poisoned padding columns [V, Vp): no output changes, and the poison is still there
    for poison in ("nan", "huge"):
        out = run_weighted(S, padded(x, Vp, poison), f, ln, w_tok, w_row)
        assert out[0].tobytes() == clean[0].tobytes() and out[2].tobytes() == clean[2].tobytes(), poison
        pad = S.region("logits", np.float32)[:x.shape[0] * Vp].reshape(-1, Vp)[:, V:Vp]
        assert (np.isnan(pad) if poison == "nan" else pad == np.float32(1e30)).all()


def test_failed_chain_word_poisons_the_weighted_loss():
    from latex_ocr_amd import _abi
    S = _sim(33, 1)
    x, f, ln = make_case("normal", 33, B, T, seed=7)
    w_tok, w_row = make_weights(ln, B, T, seed=8)
    S.region("xdec_sync", np.int32)[_abi.LXO_XDEC_ERR_WORD] = 3
    try:
        loss = run_weighted(S, padded(x, vpad(33), None), f, ln, w_tok, w_row)[0]
    finally:
        S.region("xdec_sync", np.int32)[_abi.LXO_XDEC_ERR_WORD] = 0
    assert np.isnan(loss[0]) and loss[1] == float((np.arange(T)[None, :] < ln[:, None]).sum())


def test_no_weights_is_refused():
    S = _sim(33, 0)
    x, f, ln = make_case("normal", 33, B, T, seed=7)
    before = S.ws.copy()
    rc = S.L.lxo_ce_loss_weighted(S.sref(), ptr(S.ws), ptr(f), ptr(ln), None, None, ctypes.c_float(1.0), None, None)
    assert rc == -1 and S.L.lxo_last_error() and np.array_equal(S.ws, before)


# ---------------------------------------------------------------------------------------------------------- minimum-risk weights --
def run_mrt(L, lp, cost, off, rows, alpha, q=True, risk=True):
    w = np.full(rows, 7.0, np.float32)
    qo = np.full(rows, 7.0, np.float32) if q else None
    ro = np.full(1, 7.0, np.float32) if risk else None
    rc = L.lxo_mrt_weights(ptr(lp), ptr(cost), ptr(off), len(off) - 1, rows, ctypes.c_float(alpha), ptr(w), ptr(qo), ptr(ro), None)
    assert rc == 0, L.lxo_last_error()
    return w, qo, ro


@pytest.mark.parametrize("alpha", MRT_ALPHAS)
def test_mrt_weights_against_float64(alpha):
    from simharness import lib
    L = lib()
    lp, cost, off, rows = make_mrt_case()
    w, q, risk = run_mrt(L, lp, cost, off, rows, alpha)
    worst = check_mrt(lp, cost, off, alpha, w, q, risk[0])
    print("alpha %g: w at %.2f, q at %.2f, risk at %.2f of their bars" % (alpha, worst["w"], worst["q"], worst["risk"]))
    w2, q2, risk2 = run_mrt(L, lp, cost, off, rows, alpha)         # no atomics: the same bytes in every run
    assert w2.tobytes() == w.tobytes() and q2.tobytes() == q.tobytes() and risk2.tobytes() == risk.tobytes()
    w3, _, _ = run_mrt(L, lp, cost, off, rows, alpha, q=False, risk=False)      # the optional outputs left out: the same weights
    assert w3.tobytes() == w.tobytes()
    # an empty group in the middle leaves its neighbours' weights as they were
    off_e = np.concatenate([off[:3], off[2:]]).astype(np.int32)
    we, qe, re_ = run_mrt(L, lp, cost, off_e, rows, alpha)
    assert we.tobytes() == w.tobytes() and qe.tobytes() == q.tobytes() and re_.tobytes() == risk.tobytes()


def test_mrt_weights_no_groups_and_refusals():
    from simharness import lib
    L = lib()
    lp, cost, off, rows = make_mrt_case()
    w, q, risk = run_mrt(L, lp, cost, np.zeros(1, np.int32), rows, 1.0)
    assert (w == 0).all() and (q == 0).all() and risk[0] == 0
    w = np.full(rows, 7.0, np.float32)
    G = len(off) - 1
    f = ctypes.c_float
    bad = [(ptr(lp), ptr(cost), ptr(off), G, rows, f(1.0), None),
           (None, ptr(cost), ptr(off), G, rows, f(1.0), ptr(w)),
           (ptr(lp), None, ptr(off), G, rows, f(1.0), ptr(w)),
           (ptr(lp), ptr(cost), None, G, rows, f(1.0), ptr(w)),
           (ptr(lp), ptr(cost), ptr(off), -1, rows, f(1.0), ptr(w)),
           (ptr(lp), ptr(cost), ptr(off), G, -1, f(1.0), ptr(w)),
           (ptr(lp), ptr(cost), ptr(off), G, rows, f(float("nan")), ptr(w)),
           (ptr(lp), ptr(cost), ptr(off), G, rows, f(float("inf")), ptr(w))]
    for args in bad:
        assert L.lxo_mrt_weights(*args, None, None, None) == -1
        assert L.lxo_last_error()
    assert (w == 7.0).all()
