"""CPU (hipsim): the decoder output head on CONSTRUCTED logits -- lxo_ce_loss_fwd_bwd (ce_loss_rows_kernel<KV = 4, 8, 16> and the strided
ce_loss_kernel) and lxo_score_tokens (score_rows_kernel<KV> / score_kernel, score_seq_kernel) -- against a float64 NumPy reference
(tests/output_head_ref.py), across vocabulary sizes that pick every code path, in f32 and bf16, on random, large, one-hot-like and tied
logits, with target ids at both edges and outside [0, V), and with rows past lengths[b].  The padding columns [V, Vp) of every logits row
are poisoned (NaN, +1e30): no output may change, d(logits) must be exactly 0 there, and the poison must still be there afterwards.
The same matrix runs on the MI355X in tests/test_gpu_output_head.py, with row counts the sim cannot afford."""
import ctypes

import numpy as np
import pytest

from output_head_ref import CASES, POISONS, VOCABS, check, make_case, padded, reference, vpad
from simharness import Sim, ptr
from simlib import bf16_to_f32

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
H, W = 32, 48
B, T = 3, 4                        # 12 rows: three workgroups of four waves


def run_head(S, logits_p, f, ln):
    """write the padded logits into ws "logits", run CE then scoring -> (loss [2], dlogits f32 [n, Vp], logp, top1, seq, logits after)"""
    n, Vp = logits_p.shape
    S.write_region("logits", logits_p)
    ntok = int((np.arange(T)[None, :] < ln[:, None]).sum())
    S.ck(S.L.lxo_ce_loss_fwd_bwd(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ctypes.c_float(1.0 / max(ntok, 1)), None), "ce")
    loss = S.region("loss", np.float32)[:2].copy()
    if S.dtype == 1:
        dl = bf16_to_f32(S.region("dlogits", np.uint16)[:n * Vp].copy()).reshape(n, Vp)
    else:
        dl = S.region("dlogits", np.float32)[:n * Vp].reshape(n, Vp).copy()
    lp = np.full((B, T), 7.0, np.float32)
    t1 = np.full((B, T), 77, np.int32)
    sq = np.full(B, 7.0, np.float32)
    S.ck(S.L.lxo_score_tokens(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ptr(lp), ptr(t1), ptr(sq), None), "score")
    after = S.region("logits", np.float32)[:n * Vp].reshape(n, Vp).copy()
    return loss, dl, lp, t1, sq, after


_sims = {}


def _sim(V, dtype):
    if (V, dtype) not in _sims:
        _sims[(V, dtype)] = Sim(B, H, W, T, V, dtype=dtype, seed=0, dims=SMALL)
    return _sims[(V, dtype)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", VOCABS)
def test_head(V, dtype, case):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case(case, V, B, T, seed=1)
    ref = reference(x, f, ln)
    clean = run_head(S, padded(x, Vp, None), f, ln)
    worst = check(ref, x, V, Vp, *clean[:5], bf16=dtype == 1)
    print("V=%d %s %s: worst |logp - ref| %.2e, |CE - ref| %.2e, d(logits) at %.2f of its bound"
          % (V, ("f32", "bf16")[dtype], case, worst["logp"], worst["ce"], worst["dlogits"]))
    for poison in POISONS:
        out = run_head(S, padded(x, Vp, poison), f, ln)
        for a, b in zip(clean[:5], out[:5]):
            assert a.tobytes() == b.tobytes(), poison                           # nothing read the padding
        pad = out[5][:, V:Vp]
        assert (np.isnan(pad) if poison == "nan" else pad == np.float32(1e30)).all()    # ... and it was there to be read


# ------------------------------------------------------------------------------------------------------------------- beam steps --
def _beam_sim(V, k):
    """a beam decode of GOLD's two images at vocabulary V (SMALL dims) -> (S, ids, par, scores, features)"""
    from test_decode_scores_sim import GOLD
    from latex_ocr_amd.model.utils.image import encoder_out_hw
    ms, max_iter = 5, 4
    S = Sim(2, 32, 48, 1, V, dtype=0, seed=0, beam=k, max_steps=ms, dims=SMALL)
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(GOLD["img"]), None), "enc")
    Hp, Wp = encoder_out_hw(32, 48)
    enc = S.region("img", np.float32)[:2 * Hp * Wp * SMALL["C"]].reshape(2, Hp * Wp, SMALL["C"]).copy()
    ids = np.zeros((2, ms, k), np.int32); par = np.zeros((2, ms, k), np.int32); sc = np.zeros((2, ms, k), np.float32)
    steps = ctypes.c_int(0)
    S.ck(S.L.lxo_beam_decode_scores(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), V - 1, max_iter, ptr(ids), ptr(par), ptr(sc), None,
                                    ctypes.byref(steps), None), "beam_scores")
    n = steps.value
    return S, ids[:, :n], par[:, :n], sc[:, :n], enc


@pytest.mark.parametrize("V,k", [(512, 8), (1000, 4), (1025, 3), (1025, 4)])
def test_beam_scores_large_vocabulary(V, k):
    """beam_step_fast_kernel's three log-sum-exp forms (V <= 512 with k * V = 4096; 512 < V <= 1024; V > 1024) and the general kernel at
    k * V = 4100: every final score = the teacher-forced log-prob of the path that back-traces from its slot (oracle.decoder_train on
    the features the Sim's decoder read)"""
    import torch
    from test_decode_scores_sim import backtrace_path, path_logprob
    S, ids, par, sc, enc = _beam_sim(V, k)
    P = {key: torch.from_numpy(np.asarray(v)) for key, v in S.P.items()}
    t = ids.shape[1] - 1
    assert ((ids >= 0) & (ids < V)).all() and ((par >= 0) & (par < k)).all()
    assert (np.diff(sc, axis=2) <= 0).all()
    worst = 0.0
    for b in range(2):
        for i in range(k):
            ref = path_logprob(P, enc[b], backtrace_path(ids, par, b, t, i), V - 1)
            worst = max(worst, abs(sc[b, t, i] - ref) / max(1.0, abs(ref)))
    print("beam V=%d k=%d: %d steps, |final score - teacher-forced path log-prob| / max(1, |score|) max %.2e" % (V, k, t + 1, worst))
    assert worst < 1e-5


def test_beam_wider_than_vocabulary_is_refused():
    """k > V: at time 0 only V candidates exist, so a k-th selection has no index (its parent would be 0x7fffffff / V, a row index for the
    next step).  lxo_beam_decode, lxo_decode_begin and lxo_decode_step refuse the shape with nothing written; the Engine says why"""
    V, k = 8, 9
    S = Sim(2, 32, 48, 1, V, dtype=0, seed=0, beam=k, max_steps=5, dims=SMALL)
    before = S.ws.copy()
    ids = np.full((2, 5, k), -3, np.int32); par = np.full((2, 5, k), -3, np.int32); steps = ctypes.c_int(-3)
    assert S.L.lxo_beam_decode(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), V - 1, 4, ptr(ids), ptr(par), ctypes.byref(steps), None) != 0
    assert S.L.lxo_decode_begin(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), None) != 0
    fin = np.zeros(2 * k, np.int32)
    assert S.L.lxo_decode_step(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), V - 1, 0, ptr(ids), ptr(par), ptr(fin), None, None) != 0
    assert np.array_equal(S.ws, before) and (ids == -3).all() and (par == -3).all() and steps.value == -3 and (fin == 0).all()
    from latex_ocr_amd.engine import Engine
    from simharness import lib
    eng = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=0, lib=lib())
    from test_decode_scores_sim import GOLD
    for call in (lambda: eng.beam_decode(GOLD["img"], V - 1, k, max_iter=4), lambda: eng.decode_begin(GOLD["img"], beam_size=k, max_steps=5)):
        with pytest.raises(ValueError, match="9.*8"):
            call()
        assert eng.ws is None and eng.beam == 1                                 # refused before any workspace or launch
