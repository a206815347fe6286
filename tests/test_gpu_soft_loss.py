"""-m gpu: the soft-target loss on the MI355X.

1. lxo_ce_loss_soft on CONSTRUCTED logits written into ws region "logits" against the float64 reference of tests/soft_loss_ref.py -- the hipsim file's
   matrix (V = 33, 500, 1000, 1025, 48 rows, both dtypes, k = 1, 5, 16, lambda 0.5 and 1, eps 0 and 0.1, weights none / both, four cases, every kind
   of slot data, both padding poisons) -- with its bit identities against lxo_ce_loss_smoothed and lxo_ce_loss_weighted and what it refuses.
2. The soft step end to end against autograd through the oracle, at tests/test_gpu_smoothed_loss.py's 6 rows -- in bf16 the chain batch of 8 on the
   persistent chains.
3. A soft step captured into a HIP graph and replayed: the bytes of the eager steps, in the deterministic mode.
4. A teacher -> student round: 20 steps on one batch lower the student's cross-entropy against the teacher's sparse targets (the gradient's sign)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from latex_ocr_amd.engine import _p
import mrt_oracle
from soft_loss_ref import (F_B as B, F_CASES, F_EPS, F_INV_NORM as INV_NORM, F_K, F_KINDS, F_LAMBDA, F_T as T, F_VOCABS, MASS_CAP, POISONS, check_soft,
                           counted_mass, make_case, make_slots, make_weights, padded, soft_grads, soft_reference, vpad, with_invalid_ids)

H, W = 32, 128
EPS, LAM = 0.1, 0.5
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


def run_soft(eng, x_p, f, ln, eps, lam, ids, p, w_tok=None, w_row=None, inv_norm=INV_NORM, norm_dev=None):
    n, Vp = x_p.shape
    _write_logits(eng, x_p)
    keep = [_dev(f), _dev(ln), _dev(ids), _dev(p), _dev(w_tok), _dev(w_row), _dev(norm_dev)]
    eng._ck(eng.lib.lxo_ce_loss_soft(eng.sref(), _p(eng.ws), _p(keep[0]), _p(keep[1]), ctypes.c_float(eps), ctypes.c_float(lam), ids.shape[2],
                                     _p(keep[2]), _p(keep[3]), _p(keep[4]), _p(keep[5]), ctypes.c_float(inv_norm), _p(keep[6]), eng._stream()),
            "ce_loss_soft")
    return _outputs(eng, n, Vp)


def run_smoothed(eng, x_p, f, ln, eps, w_tok=None, w_row=None, inv_norm=INV_NORM):
    n, Vp = x_p.shape
    _write_logits(eng, x_p)
    keep = [_dev(f), _dev(ln), _dev(w_tok), _dev(w_row)]
    eng._ck(eng.lib.lxo_ce_loss_smoothed(eng.sref(), _p(eng.ws), _p(keep[0]), _p(keep[1]), ctypes.c_float(eps), _p(keep[2]), _p(keep[3]),
                                         ctypes.c_float(inv_norm), None, eng._stream()), "ce_loss_smoothed")
    return _outputs(eng, n, Vp)


def run_weighted(eng, x_p, f, ln, w_tok, w_row, inv_norm=INV_NORM):
    n, Vp = x_p.shape
    _write_logits(eng, x_p)
    keep = [_dev(f), _dev(ln), _dev(w_tok), _dev(w_row)]
    eng._ck(eng.lib.lxo_ce_loss_weighted(eng.sref(), _p(eng.ws), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), ctypes.c_float(inv_norm),
                                         None, eng._stream()), "ce_loss_weighted")
    return _outputs(eng, n, Vp)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()


# ------------------------------------------------------------------------------------------------- 1. the kernels on constructed inputs --
@pytest.mark.parametrize("case", F_CASES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", F_VOCABS)
def test_soft_loss_against_float64(V, dtype, case):
    eng = _head_engine(V, dtype)
    Vp = vpad(V)
    top = {}
    ones = np.ones((B, T), np.float32)
    x, f, ln = make_case(case, V, B, T, seed=1)
    w_tok, w_row = make_weights(ln, B, T, seed=2)
    xp = {poison: padded(x, Vp, poison) for poison in POISONS}
    for k in F_K:
        slots = {"mix": make_slots("mix", x, f, ln, V, k, seed=3)}
        slots.update({kind: make_slots(kind, x, f, ln, V, k, seed=3) for kind in F_KINDS})
        for ids, p in slots.values():
            assert counted_mass(ids, p, ln, V).max(initial=0.0) <= MASS_CAP
        for wt, wr in ((None, None), (w_tok, w_row)):
            base = run_weighted(eng, xp["nan"], f, ln, wt if wt is not None else ones, wr)[0]
            for name, (ids, p) in slots.items():
                for lam in F_LAMBDA:
                    for eps in F_EPS:
                        if name != "mix" and (lam, eps) != (0.5, 0.1):
                            continue
                        ref = soft_reference(x, f, ln, wt, wr, INV_NORM, eps, lam, ids, p)
                        outs = [run_soft(eng, xp[poison], f, ln, eps, lam, ids, p, wt, wr) for poison in POISONS]
                        loss, dl, raw = outs[0]
                        what = (case, k, name, wt is not None, lam, eps)
                        worst = check_soft(ref, x, V, Vp, loss, dl, INV_NORM, bf16=dtype == "bf16")
                        for key, v in worst.items():
                            if v > top.get(key, (-1.0, ""))[0]:
                                top[key] = (v, "%s k=%d %s w=%s lambda=%g eps=%g" % what)
                        assert _same(outs[1], outs[0]), what       # either poison in [V, Vp): the same bytes
                        assert loss[1].tobytes() == base[1].tobytes() and loss[3].tobytes() == base[3].tobytes(), what
                        if name == "mix":
                            assert _same(run_soft(eng, xp["nan"], f, ln, eps, lam, ids, p, wt, wr), outs[0]), what          # ordered slots: every run
    print("V=%d %s %s, worst fractions of the bars: %s" % (V, dtype, case, ", ".join("%s %.3f (%s)" % (k, v, w) for k, (v, w) in sorted(top.items()))))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", F_VOCABS)
def test_identities_with_the_smoothed_and_the_weighted_loss(V, dtype):
    eng = _head_engine(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case("normal", V, B, T, seed=4)
    xp = padded(x, Vp, None)
    w_tok, w_row = make_weights(ln, B, T, seed=5)
    live_rows = [(t * B + b) for t in range(T) for b in range(B) if t < ln[b]]

    def rows(out):
        return out[2].reshape(T * B, -1)
    for k in F_K:
        mix_ids, mix_p = make_slots("mix", x, f, ln, V, k, seed=6)
        none_ids = np.where(np.arange(T)[None, :, None] < ln[:, None, None], -1, mix_ids).astype(np.int32)
        untaught = [t * B + b for t in range(T) for b in range(B) if t < ln[b] and (mix_ids[b, t] < 0).all()]
        assert untaught and len(untaught) < len(live_rows)
        for wt, wr in ((None, None), (w_tok, w_row)):
            for eps in F_EPS:
                sm = run_smoothed(eng, xp, f, ln, eps, wt, wr)
                for lam in F_LAMBDA:
                    got = run_soft(eng, xp, f, ln, eps, lam, mix_ids, mix_p, wt, wr)
                    assert rows(got)[untaught].tobytes() == rows(sm)[untaught].tobytes(), (k, eps, lam)
                    assert _same(run_soft(eng, xp, f, ln, eps, lam, none_ids, mix_p, wt, wr), sm), (k, eps, lam)
                assert _same(run_soft(eng, xp, f, ln, eps, 0.0, mix_ids, mix_p, wt, wr), sm), (k, eps)
            if wt is not None:
                wd = run_weighted(eng, xp, f, ln, wt, wr)
                got = run_soft(eng, xp, f, ln, 0.0, 0.5, mix_ids, mix_p, wt, wr)
                assert rows(got)[untaught].tobytes() == rows(wd)[untaught].tobytes(), k
                assert _same(run_soft(eng, xp, f, ln, 0.0, 0.5, none_ids, mix_p, wt, wr), wd), k
        topk_ids, topk_p = make_slots("topk" if k == 1 else "dup", x, f, ln, V, k, seed=7)
        bad, minus = with_invalid_ids(topk_ids, V, seed=8)
        assert _same(run_soft(eng, xp, f, ln, 0.1, 0.5, bad, topk_p, w_tok, w_row), run_soft(eng, xp, f, ln, 0.1, 0.5, minus, topk_p, w_tok, w_row)), k
    ids, p = make_slots("mix", x, f, ln, V, 5, seed=6)
    a = run_soft(eng, xp, f, ln, 0.1, 0.5, ids, p, w_tok, w_row, np.float32(0.125))
    b = run_soft(eng, xp, f, ln, 0.1, 0.5, ids, p, w_tok, w_row, 123.0, np.array([8.0], np.float32))
    assert _same(a, b)


def test_refusals_write_nothing():
    V = 33
    eng = _head_engine(V, "bf16")
    x, f, ln = make_case("normal", V, B, T, seed=12)
    ids, p = make_slots("topk", x, f, ln, V, 5, seed=13)
    _write_logits(eng, padded(x, vpad(V), None))
    keep = [_dev(f), _dev(ln), _dev(ids), _dev(p)]
    c = ctypes.c_float
    ok = dict(s=eng.sref(), ws=_p(eng.ws), f=_p(keep[0]), ln=_p(keep[1]), eps=c(0.1), lam=c(0.5), k=5, ids=_p(keep[2]), p=_p(keep[3]))
    torch.cuda.synchronize()
    before = eng.ws.clone()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(eps=c(1.0)), dict(eps=c(-0.1)), dict(eps=c(nan)), dict(eps=c(inf)), dict(lam=c(-0.1)), dict(lam=c(1.5)), dict(lam=c(nan)), dict(lam=c(inf)),
               dict(k=0), dict(k=17), dict(ws=None), dict(f=None), dict(ln=None), dict(ids=None), dict(p=None), dict(s=None)):
        a = dict(ok, **kw)
        assert eng.lib.lxo_ce_loss_soft(a["s"], a["ws"], a["f"], a["ln"], a["eps"], a["lam"], a["k"], a["ids"], a["p"], None, None, c(1.0), None,
                                        eng._stream()) == -1, kw
        assert eng.lib.lxo_last_error()
    torch.cuda.synchronize()
    assert torch.equal(eng.ws, before)


# ------------------------------------------------------------------------------------------------------------ 2. end to end vs autograd --
CONV1_BF16 = 0.998       # tests/test_gpu_parity.py: conv1's kernel / bias in bf16


def _step_slots(f, l, V, k, seed):
    """k distinct tokens per position, masses adding up to 0.8; one live position without a teacher, one with two slots on one token"""
    rng = np.random.default_rng(seed)
    Bn, Tn = f.shape
    ids = np.stack([np.stack([rng.choice(V, size=k, replace=False) for _ in range(Tn)]) for _ in range(Bn)]).astype(np.int32)
    p = rng.dirichlet(np.ones(k), size=(Bn, Tn)).astype(np.float32) * np.float32(0.8)
    ids[0, 0, :] = -1
    ids[0, 1, 1] = ids[0, 1, 0]
    return ids, p


def _soft_grads_check(dtype, w, tol_loss, min_cos, norm=11.0):
    V, n = 50, 6
    img, f, l = batch(n, 32, 128, V, 5, 12, seed=7)
    ids, p = _step_slots(f, l, V, 5, seed=9)
    eng = Engine(V, dtype=dtype, seed=3)
    P = oracle_params(eng)
    eng.forward(img, f)
    if dtype == "bf16":
        assert int(eng.shape.B) == 8 and int(eng.live_B) == 6       # the chain batch: two dead rows behind the six
    kw = dict(weights=w(f.shape)) if w is not None else {}
    stats = eng.loss(l, 1.0 / norm, label_smoothing=EPS, soft_targets=(ids, p), soft_weight=LAM, **kw).cpu().numpy()
    eng.backward()
    torch.cuda.synchronize()
    ref, G, ce = soft_grads(P, img, f, l, w(f.shape) if w is not None else np.ones(f.shape, np.float32), norm, EPS, LAM, ids, p)
    loss = float(stats[0]) / norm
    assert stats.shape == (4,) and stats[1] == float(l.sum())
    assert abs(float(stats[3]) / float(stats[1]) - ce) / ce < tol_loss
    cs = mrt_oracle.cosines(eng.grad_dict(), G)
    print("%s%s: soft loss %.6f oracle %.6f rel %.2e; chain_used %s; lowest gradient cosines %s" % (
        dtype, " weighted" if w is not None else "", loss, ref, abs(loss - ref) / abs(ref), eng.chain_used,
        ", ".join("%.6f %s" % (c, k.split("/", 1)[-1]) for c, k in cs[:3])))
    assert abs(loss - ref) / abs(ref) < tol_loss, (loss, ref)
    for c, k in cs:
        bar = CONV1_BF16 if (dtype == "bf16" and k.startswith("Encoder/convolutional_encoder/conv2d/")) else min_cos
        assert c > bar, (k, c)
    return eng


def test_soft_step_f32():
    _soft_grads_check("f32", None, 2e-5, 0.9999)


def test_soft_step_f32_mixed_sign_weights():
    _soft_grads_check("f32", lambda s: np.random.default_rng(5).uniform(-2.0, 2.0, size=s).astype(np.float32), 2e-5, 0.9999)


def test_soft_step_bf16_on_the_chain():
    eng = _soft_grads_check("bf16", None, 1e-3, 0.999)
    assert eng.chain_used, "the forward chain did not run"


# ------------------------------------------------------------------------------------------------------------------- 3. graph capture --
def test_soft_step_captured_into_a_graph():
    V, Bg = 50, 16
    img, f, l = batch(Bg, 32, 128, V, 5, 20, seed=11)
    ids, p = _step_slots(f, l, V, 5, seed=12)
    img, f, l = torch.from_numpy(img).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(l.astype(np.int32)).cuda()
    ids, p = torch.from_numpy(ids).cuda(), torch.from_numpy(p).cuda()
    wr = torch.from_numpy(np.random.default_rng(7).uniform(-1.0, 2.0, size=Bg).astype(np.float32)).cuda()

    def fresh():
        e = Engine(V, dtype="bf16", seed=3, deterministic=True)
        e.set_optimizer("sgd")
        return e

    def body(e):
        e.forward(img, f)
        e.loss(l, 1.0 / 37.0, row_weights=wr, label_smoothing=EPS, soft_targets=(ids, p), soft_weight=LAM)
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


# ------------------------------------------------------------------------------------------------------------ 4. teacher -> student --
def test_student_moves_towards_the_teacher():
    V, k = 50, 5
    img, f, l = batch(8, 32, 128, V, 5, 12, seed=13)
    teacher, student = Engine(V, dtype="bf16", seed=21), Engine(V, dtype="bf16", seed=4)
    alt = teacher.score(img, f, l, alternatives=k)[-1]
    ids, p = alt.ids, np.exp(alt.logp.astype(np.float64)).astype(np.float32)

    def ce_against_teacher():
        """the student's mean cross-entropy against the teacher's sparse targets, by the float64 reference from the student's logits"""
        student.forward(img, f)
        Bp, Tn, Vp = int(student.shape.B), int(student.shape.T), vpad(V)
        x = student.region("logits")[:Tn * Bp * Vp].cpu().numpy().reshape(Tn, Bp, Vp)[:, :len(l), :V].reshape(-1, V)
        ref = soft_reference(np.ascontiguousarray(x), f, l, None, None, 1.0, 0.0, 1.0, ids, p)
        return float(ref["stats_f"][0] / ref["stats_f"][1])
    before = ce_against_teacher()
    for _ in range(20):
        student.train_step(img, f, l, 1e-3, soft_targets=alt, soft_weight=1.0, label_smoothing=0.0, sync_loss=False)
    after = ce_against_teacher()
    print("student's cross-entropy against the teacher's top-%d targets: %.4f -> %.4f after 20 steps" % (k, before, after))
    assert after < before
