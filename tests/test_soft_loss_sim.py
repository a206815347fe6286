"""CPU (hipsim): the soft-target loss lxo_ce_loss_soft -- the <..., CeSmooth, CeSoft> and <..., CeWeights, CeSmooth, CeSoft> instantiations of
ce_loss_rows_kernel<KV = 4, 8, 16> and of the strided ce_loss_kernel -- on CONSTRUCTED logits against a float64 reference (tests/soft_loss_ref.py),
its bit identities with lxo_ce_loss_smoothed and lxo_ce_loss_weighted, what it may write and what it refuses.  The same checks run on the MI355X
in tests/test_gpu_soft_loss.py."""
import ctypes

import numpy as np
import pytest

from simharness import Sim, ptr
from simlib import bf16_to_f32
from soft_loss_ref import (F_B as B, F_CASES, F_EPS, F_INV_NORM as INV_NORM, F_K, F_KINDS, F_LAMBDA, F_T as T, F_VOCABS, MASS_CAP, POISONS,
                           check_soft, counted_mass, make_case, make_slots, make_weights, padded, soft_reference, vpad, with_invalid_ids)

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


def run_soft(S, logits_p, f, ln, eps, lam, ids, p, w_tok=None, w_row=None, inv_norm=INV_NORM, norm_dev=None):
    """write the padded logits into ws "logits", run the soft loss -> (loss [4], d(logits) f32 [n, Vp], its raw elements)"""
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    S.ck(S.L.lxo_ce_loss_soft(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ctypes.c_float(eps), ctypes.c_float(lam), ids.shape[2], ptr(ids), ptr(p),
                              ptr(w_tok), ptr(w_row), ctypes.c_float(inv_norm), ptr(norm_dev), None), "ce_f")
    return _outputs(S, n, Vp)


def run_smoothed(S, logits_p, f, ln, eps, w_tok=None, w_row=None, inv_norm=INV_NORM):
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    S.ck(S.L.lxo_ce_loss_smoothed(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ctypes.c_float(eps), ptr(w_tok), ptr(w_row), ctypes.c_float(inv_norm),
                                  None, None), "ce_s")
    return _outputs(S, n, Vp)


def run_weighted(S, logits_p, f, ln, w_tok, w_row, inv_norm=INV_NORM):
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    S.ck(S.L.lxo_ce_loss_weighted(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ptr(w_tok), ptr(w_row), ctypes.c_float(inv_norm), None, None), "ce_w")
    return _outputs(S, n, Vp)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("case", F_CASES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", F_VOCABS)
def test_soft_loss_against_float64(V, dtype, case):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case(case, V, B, T, seed=1)
    w_tok, w_row = make_weights(ln, B, T, seed=2)
    xp = {poison: padded(x, Vp, poison) for poison in POISONS}
    ones = np.ones((B, T), np.float32)
    for k in F_K:
        # every kind of slot data in one call ("mix": taught rows beside rows of -1), and each kind alone at lambda 0.5 / eps 0.1
        slots = {"mix": make_slots("mix", x, f, ln, V, k, seed=3)}
        slots.update({kind: make_slots(kind, x, f, ln, V, k, seed=3) for kind in F_KINDS})
        for ids, p in slots.values():
            assert counted_mass(ids, p, ln, V).max(initial=0.0) <= MASS_CAP          # the CPU reference alone: inside the Engine's cap
        for wt, wr in ((None, None), (w_tok, w_row)):
            # "loss"[1] and [3] are the weighted call's bytes with the same weights (no weights: every token weighing 1.f)
            base = run_weighted(S, xp["nan"], f, ln, wt if wt is not None else ones, wr)[0]
            for name, (ids, p) in slots.items():
                for lam in F_LAMBDA:
                    for eps in F_EPS:
                        if name != "mix" and (lam, eps) != (0.5, 0.1):
                            continue
                        ref = soft_reference(x, f, ln, wt, wr, INV_NORM, eps, lam, ids, p)
                        outs = [run_soft(S, xp[poison], f, ln, eps, lam, ids, p, wt, wr) for poison in POISONS]
                        loss, dl, raw = outs[0]
                        worst = check_soft(ref, x, V, Vp, loss, dl, INV_NORM, bf16=dtype == 1)
                        print("V=%d %s %s k=%d %s w=%s lambda=%g eps=%g: d(logits) at %.2f of its bar, row sums %.2f, sum w L %.2f, sum w %.2f, "
                              "sum CE %.2f of theirs" % (V, ("f32", "bf16")[dtype], case, k, name, wt is not None, lam, eps, worst["dlogits"],
                                                         worst["rowsum"], worst["loss0"], worst["loss2"], worst["loss3"]))
                        assert _same(outs[1], outs[0])             # either poison in [V, Vp): the same bytes
                        assert loss[1].tobytes() == base[1].tobytes() and loss[3].tobytes() == base[3].tobytes()
                        if name == "mix":
                            assert _same(run_soft(S, xp["nan"], f, ln, eps, lam, ids, p, wt, wr), outs[0])          # a second run: the same bytes


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", F_VOCABS)
def test_identities_with_the_smoothed_and_the_weighted_loss(V, dtype):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=4)
    xp = padded(x, Vp, None)
    w_tok, w_row = make_weights(ln, B, T, seed=5)
    live_rows = [(t * B + b) for t in range(T) for b in range(B) if t < ln[b]]
    for k in F_K:
        mix_ids, mix_p = make_slots("mix", x, f, ln, V, k, seed=6)
        none_ids = np.where(np.arange(T)[None, :, None] < ln[:, None, None], -1, mix_ids).astype(np.int32)       # every live row: all slots -1
        untaught = [t * B + b for t in range(T) for b in range(B) if t < ln[b] and (mix_ids[b, t] < 0).all()]
        assert untaught and len(untaught) < len(live_rows)
        for wt, wr in ((None, None), (w_tok, w_row)):
            for eps in F_EPS:
                sm = run_smoothed(S, xp, f, ln, eps, wt, wr)
                for lam in F_LAMBDA:
                    # rows of -1 beside taught rows, lambda > 0: those rows carry the smoothed call's bytes
                    got = run_soft(S, xp, f, ln, eps, lam, mix_ids, mix_p, wt, wr)
                    sm_rows, got_rows = sm[2].reshape(-1, Vp), got[2].reshape(-1, Vp)
                    assert got_rows[untaught].tobytes() == sm_rows[untaught].tobytes(), (k, eps, lam)
                    # every row like that: the four statistics too
                    assert _same(run_soft(S, xp, f, ln, eps, lam, none_ids, mix_p, wt, wr), sm), (k, eps, lam)
                # lambda == 0 is the smoothed call, whatever the slots say
                assert _same(run_soft(S, xp, f, ln, eps, 0.0, mix_ids, mix_p, wt, wr), sm), (k, eps)
            if wt is not None:
                # eps == 0 on such rows: the weighted call's bytes
                wd = run_weighted(S, xp, f, ln, wt, wr)
                got = run_soft(S, xp, f, ln, 0.0, 0.5, mix_ids, mix_p, wt, wr)
                assert got[2].reshape(-1, Vp)[untaught].tobytes() == wd[2].reshape(-1, Vp)[untaught].tobytes(), k
                assert _same(run_soft(S, xp, f, ln, 0.0, 0.5, none_ids, mix_p, wt, wr), wd), k
        # a slot id >= V or < 0 changes nothing against the same call with that slot -1
        topk_ids, topk_p = make_slots("topk" if k == 1 else "dup", x, f, ln, V, k, seed=7)
        bad, minus = with_invalid_ids(topk_ids, V, seed=8)
        assert (bad != minus).any()
        assert _same(run_soft(S, xp, f, ln, 0.1, 0.5, bad, topk_p, w_tok, w_row), run_soft(S, xp, f, ln, 0.1, 0.5, minus, topk_p, w_tok, w_row)), k
    # the normaliser read from device memory: 1 / norm_dev[0] replaces inv_norm (1 / 8 is exact)
    ids, p = make_slots("mix", x, f, ln, V, 5, seed=6)
    a = run_soft(S, xp, f, ln, 0.1, 0.5, ids, p, w_tok, w_row, np.float32(0.125))
    b = run_soft(S, xp, f, ln, 0.1, 0.5, ids, p, w_tok, w_row, 123.0, np.array([8.0], np.float32))
    assert _same(a, b)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", (33, 1025))
def test_untouched_memory(V, dtype):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=9)
    w_tok, w_row = make_weights(ln, B, T, seed=10)
    ids, p = make_slots("mix", x, f, ln, V, 16, seed=11)
    for wt, wr in ((None, None), (w_tok, w_row)):
        clean = run_soft(S, padded(x, Vp, None), f, ln, 0.1, 0.5, ids, p, wt, wr)
        # a second call on a workspace full of 0xA5 outside what the call owns: nothing but "dlogits", "loss" and "det_part" may change
        keep = {name: S.region(name, np.uint8).copy() for name in ("logits", "xdec_sync")}        # what the call reads
        S.ws[:] = 0xA5
        for name, raw in keep.items():
            S.region(name, np.uint8)[:] = raw
        before = S.ws.copy()
        again = run_soft(S, padded(x, Vp, None), f, ln, 0.1, 0.5, ids, p, wt, wr)
        assert _same(again, clean)
        changed = S.ws != before
        owned = np.zeros(S.ws.shape, bool)
        for name in ("dlogits", "loss", "det_part"):
            off, nb = ctypes.c_size_t(), ctypes.c_size_t()
            S.ck(S.L.lxo_ws_region(S.sref(), name.encode(), ctypes.byref(off), ctypes.byref(nb)), "region")
            owned[off.value:off.value + nb.value] = True
        assert not (changed & ~owned).any(), np.flatnonzero(changed & ~owned)[:8]
        assert changed.any()
        S.ws[:] = 0


def test_failed_chain_word_poisons_the_soft_loss():
    from latex_ocr_amd import _abi
    S = _sim(33, 1)
    x, f, ln = make_case("normal", 33, B, T, seed=12)
    ids, p = make_slots("topk", x, f, ln, 33, 5, seed=13)
    S.region("xdec_sync", np.int32)[_abi.LXO_XDEC_ERR_WORD] = 3
    try:
        loss = run_soft(S, padded(x, vpad(33), None), f, ln, 0.1, 0.5, ids, p)[0]
    finally:
        S.region("xdec_sync", np.int32)[_abi.LXO_XDEC_ERR_WORD] = 0
    assert np.isnan(loss[0]) and loss[1] == float((np.arange(T)[None, :] < ln[:, None]).sum())


def test_refusals_write_nothing():
    S = _sim(33, 0)
    x, f, ln = make_case("normal", 33, B, T, seed=12)
    ids, p = make_slots("topk", x, f, ln, 33, 5, seed=13)
    S.write_region("logits", padded(x, vpad(33), None))
    before = S.ws.copy()
    c = ctypes.c_float
    ok = dict(s=S.sref(), ws=ptr(S.ws), f=ptr(f), ln=ptr(ln), eps=c(0.1), lam=c(0.5), k=5, ids=ptr(ids), p=ptr(p))
    nan, inf = float("nan"), float("inf")
    bad = [dict(eps=c(1.0)), dict(eps=c(1.5)), dict(eps=c(-0.1)), dict(eps=c(nan)), dict(eps=c(inf)), dict(eps=c(-inf)),
           dict(lam=c(-0.1)), dict(lam=c(-1e-30)), dict(lam=c(float(np.nextafter(np.float32(1), np.float32(2))))), dict(lam=c(1.5)), dict(lam=c(nan)),
           dict(lam=c(inf)), dict(lam=c(-inf)), dict(k=0), dict(k=-1), dict(k=17), dict(k=1 << 20),
           dict(ws=None), dict(f=None), dict(ln=None), dict(ids=None), dict(p=None), dict(s=None)]
    for kw in bad:
        a = dict(ok, **kw)
        rc = S.L.lxo_ce_loss_soft(a["s"], a["ws"], a["f"], a["ln"], a["eps"], a["lam"], a["k"], a["ids"], a["p"], None, None, c(1.0), None, None)
        assert rc == -1 and S.L.lxo_last_error(), kw
        assert np.array_equal(S.ws, before), kw
    # the ends of the two ranges are inside: eps 0 and the largest f32 below 1, lambda 0 and 1, k 1 and 16
    for kw in (dict(eps=c(0.0)), dict(eps=c(float(np.nextafter(np.float32(1), np.float32(0))))), dict(lam=c(0.0)), dict(lam=c(1.0))):
        a = dict(ok, **kw)
        S.ck(S.L.lxo_ce_loss_soft(a["s"], a["ws"], a["f"], a["ln"], a["eps"], a["lam"], a["k"], a["ids"], a["p"], None, None, c(1.0), None, None), "ce_f")
    for k in (1, 16):
        ids, p = make_slots("topk", x, f, ln, 33, k, seed=13)
        S.ck(S.L.lxo_ce_loss_soft(ok["s"], ok["ws"], ok["f"], ok["ln"], c(0.1), c(0.5), k, ptr(ids), ptr(p), None, None, c(1.0), None, None), "ce_f")
