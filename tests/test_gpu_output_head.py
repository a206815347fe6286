"""-m gpu: the decoder output head across vocabulary sizes V and beam widths k -- every branch the kernels pick from V and k.

1. lxo_ce_loss_fwd_bwd and lxo_score_tokens on CONSTRUCTED logits written into ws region "logits" (tests/output_head_ref.py: float64
   reference, the case matrix, poisoned padding columns), including row counts above the grid caps of the row loops (2048 and 8192 rows).
2. Decode against the oracle: greedy ids and token log-probs at V up to 3000; bf16 greedy on both sides of the decode chain's V <= 512;
   beam ids, parents and scores at (V, k) pairs that run every branch of beam_step_fast_kernel and beam_step_kernel; the fast kernel
   against the general one (LXO_BEAM_FAST=0, a child process); NaN in the padding columns of "dec_logits" during decode.
3. One training step at large V against oracle.train_grads (the logits GEMM with N = V, y_W_o's weight gradient with J = V, the
   embedding scatter, the CE branches inside a real step); one decode step at V = 1000 (fused logits) and V = 1001 (the GEMM fallback).
4. predict_with_attention's maps along the back-traced beam path, and the refusal of a beam wider than the vocabulary."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from latex_ocr_amd.engine import _p
from latex_ocr_amd.model.utils.text import beam_slots
from output_head_ref import CASES, POISONS, VOCABS, check, make_case, padded, reference, vpad
from test_gpu_decode_scores import _restate

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H, W = 32, 128

# ------------------------------------------------------------------------------------------------ 1. the head on constructed logits --
_engines = {}


def _head_engine(V, dtype, B, T):
    eng = _engines.get((V, dtype))
    if eng is None:
        eng = _engines[(V, dtype)] = Engine(V, dtype=dtype, seed=0)
    eng.ensure(B, H, W, T)
    if dtype == "bf16":
        # the scoring / CE kernels read the forward chain's error word: a fresh (zeroed) workspace, or the word a forward left, is 0
        assert int(eng.region("xdec_sync", "i32")[512].item()) == 0
    return eng


def run_head(eng, x_p, f, ln):
    """padded logits -> ws "logits"; CE then scoring through the C ABI -> (loss [2], dlogits f32 [n, Vp], logp, top1, seq, logits after)"""
    B, T = f.shape
    n, Vp = x_p.shape
    eng.region("logits")[:n * Vp].copy_(torch.from_numpy(x_p.reshape(-1)))
    fd, ld = torch.from_numpy(f).to(eng.device), torch.from_numpy(ln).to(eng.device)
    ntok = int((np.arange(T)[None, :] < ln[:, None]).sum())
    st = eng._stream()
    eng._ck(eng.lib.lxo_ce_loss_fwd_bwd(eng.sref(), _p(eng.ws), _p(fd), _p(ld), ctypes.c_float(1.0 / max(ntok, 1)), st), "ce_loss")
    loss = eng.region("loss")[:2].cpu().numpy().copy()
    dl = eng.region("dlogits", "ct")[:n * Vp].float().cpu().numpy().reshape(n, Vp)
    lp = torch.full((B, T), 7.0, dtype=torch.float32, device=eng.device)
    t1 = torch.full((B, T), 77, dtype=torch.int32, device=eng.device)
    sq = torch.full((B,), 7.0, dtype=torch.float32, device=eng.device)
    eng._ck(eng.lib.lxo_score_tokens(eng.sref(), _p(eng.ws), _p(fd), _p(ld), _p(lp), _p(t1), _p(sq), st), "score_tokens")
    after = eng.region("logits")[:n * Vp].cpu().numpy().reshape(n, Vp)
    return loss, dl, lp.cpu().numpy(), t1.cpu().numpy(), sq.cpu().numpy(), after


def _head_case(V, dtype, case, B, T, poisons=POISONS):
    eng = _head_engine(V, dtype, B, T)
    Vp = vpad(V)
    x, f, ln = make_case(case, V, B, T, seed=2)
    ref = reference(x, f, ln)
    clean = run_head(eng, padded(x, Vp, None), f, ln)
    worst = check(ref, x, V, Vp, *clean[:5], bf16=dtype == "bf16")
    print("V=%d %s %s rows=%d: worst |logp - ref| %.2e, |CE - ref| %.2e, d(logits) at %.2f of its bound"
          % (V, dtype, case, B * T, worst["logp"], worst["ce"], worst["dlogits"]))
    for poison in poisons:
        out = run_head(eng, padded(x, Vp, poison), f, ln)
        for a, b in zip(clean[:5], out[:5]):
            assert a.tobytes() == b.tobytes(), poison                           # no output read the padding ...
        pad = out[5][:, V:Vp]
        assert (np.isnan(pad) if poison == "nan" else pad == np.float32(1e30)).all()    # ... which was there to be read


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", VOCABS)
def test_head(V, dtype, case):
    _head_case(V, dtype, case, 8, 16)                                           # 128 rows: 32 workgroups of four row-waves


@pytest.mark.parametrize("T", [40, 151])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", [33, 512, 1000, 3000])
def test_head_row_counts(V, dtype, T):
    """B = 64: 2560 rows (above the 512 workgroups x 4 rows of the CE row loop) and 9664 rows (above the scoring kernel's 2048 x 4)"""
    _head_case(V, dtype, "normal", 64, T, poisons=("nan",))


# --------------------------------------------------------------------------------------------------------- 2. decode vs the oracle --
def _img(V, seed, n=2):
    return batch(n, H, W, V, 5, 9, seed=seed)[0]


@pytest.mark.parametrize("V", [33, 513, 1025, 3000])
def test_greedy_f32_vs_oracle(V):
    img = _img(V, 3)
    eng = Engine(V, dtype="f32", seed=5)
    ids, lp = eng.greedy_decode(img, V - 1, max_iter=8, return_scores=True)
    rid, logits = R.greedy_decode(oracle_params(eng), torch.from_numpy(img), V - 1, max_iter=8, return_logits=True)
    assert np.array_equal(ids, rid.numpy()), (ids, rid.numpy())
    ref = F.log_softmax(logits.double(), dim=-1).gather(-1, rid.long()[..., None])[..., 0].numpy()
    err = np.abs(lp - ref).max()
    print("greedy f32 V=%d: %d steps, |logp - oracle| max %.2e" % (V, ids.shape[1], err))
    assert err < 1e-4


@pytest.mark.parametrize("V,chain", [(512, True), (513, False)])
def test_greedy_bf16_chain_cutoff(V, chain):
    img = _img(V, 4)
    eng = Engine(V, dtype="bf16", seed=5)
    ids, lp = eng.greedy_decode(img, V - 1, max_iter=8, return_scores=True)
    used, err = eng.chain_status()
    assert (used, err) == (chain, 0), (used, err)                               # the persistent decode chain takes V <= 512 only
    rid, logits = R.greedy_decode(oracle_params(eng), torch.from_numpy(img), V - 1, max_iter=8, return_logits=True)
    n_div = assert_flips_are_near_ties(ids, rid.numpy(), logits.numpy(), "greedy bf16 V=%d" % V)
    print("greedy bf16 V=%d: chain %s, %d of %d rows diverge from the oracle (at near-ties)" % (V, used, n_div, ids.shape[0]))
    assert np.isfinite(lp).all() and (lp <= 1e-6).all()


# (V, k, div_gamma, div_prob): which kernel each one runs is chosen by lxo_k_beam_step -- the fast one for k <= 8, k * V <= 4096 and no
# diversity penalty, else the general one (a kernel trace of these cases on the MI355X: beam_step_fast_kernel for exactly the five FAST
# ones, beam_step_kernel for the other six)
BEAM_CASES = [
    (512, 8, 1.0, 0.0),        # fast, k * V = 4096 exactly, row in registers (V <= 512)
    (513, 8, 1.0, 0.0),        # general, k * V = 4104
    (1000, 4, 1.0, 0.0),       # fast, middle log-sum-exp branch (512 < V <= 1024)
    (1024, 4, 1.0, 0.0),       # fast, middle branch at its edge
    (1025, 4, 1.0, 0.0),       # general, k * V = 4100
    (1025, 3, 1.0, 0.0),       # fast, strided log-sum-exp (V > 1024)
    (2000, 2, 1.0, 0.0),       # fast, strided
    (50, 9, 1.0, 0.0),         # general, k > 8
    (50, 16, 1.0, 0.0),        # general, the widest beam
    (1000, 16, 1.0, 0.0),      # general, k > 8 at a large V
    (1000, 5, 0.7, 1.0),       # general with the diversity penalty at a large V
]
FAST = [(V, k) for V, k, g, p in BEAM_CASES if k <= 8 and k * V <= 4096 and (g == 1.0 or p == 0.0)]


def _beam_run(V, k, g, p):
    img = _img(V, 10 + k)
    eng = Engine(V, dtype="f32", seed=1)
    ids, par, sc = eng.beam_decode(img, V - 1, k, max_iter=8, return_scores=True, div_gamma=g, div_prob=p, div_seed=3)
    return img, eng, ids, par, sc


@pytest.mark.parametrize("V,k,g,p", BEAM_CASES)
def test_beam_f32_vs_oracle(V, k, g, p):
    img, eng, ids, par, sc = _beam_run(V, k, g, p)
    P = oracle_params(eng)
    rid, rpar = R.beam_decode(P, torch.from_numpy(img), V - 1, k, max_iter=8, div_gamma=g, div_prob=p, div_seed=3)
    assert ids.shape == tuple(rid.shape)
    assert np.array_equal(ids, rid.numpy()) and np.array_equal(par, rpar.numpy())
    assert (np.diff(sc, axis=2) <= 0).all()
    if g == 1.0 or p == 0.0:                                                    # with a penalty the scores are not path log-probs
        t = ids.shape[1] - 1
        ref = _restate(P, img, ids, par, t, V - 1)
        err = (np.abs(sc[:, t] - ref) / np.maximum(1.0, np.abs(ref))).max()
        print("beam f32 V=%d k=%d: %d steps, |final score - teacher-forced restatement| / max(1, |score|) max %.2e" % (V, k, ids.shape[1], err))
        assert err < 1e-4


def _dump_fast_cases(out):
    """child process (LXO_BEAM_FAST=0 in its environment): the FAST cases' decodes -> npz"""
    res = {}
    for V, k in FAST:
        _, _, ids, par, sc = _beam_run(V, k, 1.0, 0.0)
        res["ids_%d_%d" % (V, k)], res["par_%d_%d" % (V, k)], res["sc_%d_%d" % (V, k)] = ids, par, sc
    np.savez(out, **res)


def test_beam_fast_kernel_vs_general_kernel(tmp_path):
    out = str(tmp_path / "general.npz")
    env = dict(os.environ, LXO_BEAM_FAST="0", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "dump-general", out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    gen = dict(np.load(out))
    for V, k in FAST:
        _, _, ids, par, sc = _beam_run(V, k, 1.0, 0.0)
        gi, gp, gs = gen["ids_%d_%d" % (V, k)], gen["par_%d_%d" % (V, k)], gen["sc_%d_%d" % (V, k)]
        assert np.array_equal(ids, gi) and np.array_equal(par, gp), (V, k)
        err = (np.abs(sc - gs) / np.maximum(1.0, np.abs(gs))).max()
        print("beam V=%d k=%d: fast vs general kernel: ids and parents identical, scores differ by %.2e (relative, max)" % (V, k, err))
        assert err < 1e-5                  # the log-sum-exp's summation order only (measured: 0, the scores were bit-identical at every case)


@pytest.mark.parametrize("V", [33, 1025])
@pytest.mark.parametrize("k", [1, 3])
def test_decode_ignores_padding_columns(V, k):
    """NaN in the padding columns of ws "dec_logits" [B * k, Vp] while decoding step by step (lxo_decode_step: argmax_kernel / the beam
    kernels): the same ids, parents and running log-probs as without; the logits GEMM leaves those columns alone, so the NaN is still
    there when the next selection reads the row"""
    img = _img(V, 6)
    Vp = vpad(V)

    def run(poison):
        eng = Engine(V, dtype="f32", seed=2)
        eng.decode_begin(img, beam_size=k, max_steps=8)
        rows = 2 * k
        out, kept = [], []
        for t in range(6):
            if poison:
                eng.region("dec_logits", "f32", (rows, Vp))[:, V:] = float("nan")
            ids, par, fin, _ = eng.decode_step(t, V - 1)
            lg = eng.region("dec_logits", "f32", (rows, Vp)).cpu().numpy()
            kept.append(bool(np.isnan(lg[:, V:]).all()) if poison else None)
            assert np.isfinite(lg[:, :V]).all()
            lp = eng.region("beam_lp", "f32")[:rows].cpu().numpy().copy() if k > 1 else None
            out.append((ids, par, fin, lp))
        return out, kept

    clean, _ = run(False)
    dirty, kept = run(True)
    print("V=%d k=%d: padding still NaN after each step's logits were produced: %s" % (V, k, kept))
    assert all(kept)                                                            # the producer did not overwrite the pad: the selection saw NaN
    for a, b in zip(clean, dirty):
        for x, y in zip(a, b):
            assert (x is None and y is None) or x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------------ 3. a training step at large V --
@pytest.mark.parametrize("V", [513, 1000, 1025, 3000])
def test_train_step_large_vocabulary(V):
    img, f, l = batch(6, H, W, V, 5, 12, seed=7)
    n = int(l.sum())
    eng = Engine(V, dtype="f32", seed=3)
    P = oracle_params(eng)
    eng.forward(img, f)
    stats = eng.loss(l, 1.0 / n).cpu().numpy()
    eng.backward()
    torch.cuda.synchronize()
    loss_ref, G, _, _ = R.train_grads(P, torch.from_numpy(img), torch.from_numpy(f), torch.from_numpy(l))
    loss = stats[0] / stats[1]
    assert stats[1] == n
    got = eng.grad_dict()
    cs = sorted((cosine(got[k], G[k].numpy()), k) for k in G)
    emb = rel(got["Decoder/embedding_table"], G["Decoder/embedding_table"].numpy())
    ywo = ["Decoder/AttentionCell/rnn/y_W_o"]
    print("f32 V=%d: loss rel %.2e; lowest gradient cosines %s; embedding table rel %.2e" % (
        V, abs(loss - float(loss_ref)) / float(loss_ref), ", ".join("%.7f %s" % (c, k.split("/", 1)[-1]) for c, k in cs[:3]), emb))
    assert abs(loss - float(loss_ref)) / float(loss_ref) < 2e-5, (loss, float(loss_ref))
    for c, k in cs:
        assert c > 0.99999, (k, c)
    for k in ywo + ["Decoder/embedding_table"]:
        assert rel(got[k], G[k].numpy()) < 1e-4, (k, rel(got[k], G[k].numpy()))
    e16 = Engine(V, dtype="bf16", seed=3)
    l16 = e16.train_step(img, f, l, 1e-3)
    print("bf16 V=%d: loss %.6f, oracle %.6f" % (V, l16, float(loss_ref)))
    assert abs(l16 - float(loss_ref)) / float(loss_ref) < 2e-3


@pytest.mark.parametrize("V", [1000, 1001])
def test_decode_step_logits_vs_oracle(V):
    """V % 4 == 0: the fused step kernel writes the logits (rstep); otherwise the dense GEMM does"""
    img = _img(V, 8)
    eng = Engine(V, dtype="f32", seed=4)
    eng.decode_begin(img, beam_size=1, max_steps=4)
    ids, _, _, lg = eng.decode_step(0, V - 1)
    rid, rl = R.greedy_decode(oracle_params(eng), torch.from_numpy(img), V - 1, max_iter=0, return_logits=True)
    ref = rl[:, 0].double().numpy()
    err = rel(lg, ref)
    print("decode step V=%d: logits rel %.2e" % (V, err))
    assert err < 1e-5
    assert np.array_equal(ids, rid[:, 0].numpy())


# ----------------------------------------------------------------------------------------------- 4. attention maps, beam width > V --
def test_predict_with_attention_backtraced_maps():
    """config.beam_backtrace: step t's map is that of the row the back-traced best hypothesis read its token off, against the oracle's
    beam alpha walked the same way -- on an image and weights where that path leaves slot 0 (asserted: else this proves nothing)"""
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    V = 50

    class Voc(object):
        id_end = V - 1
        id_to_tok = {i: "t%d" % i for i in range(V)}

    found, best = None, 0.0
    for seed in range(6):                       # the image / weights / k whose back-traced path reads maps furthest from slot 0's parents'
        for k in (3, 4, 5):
            img = _img(V, 30 + seed, n=1)[0]
            eng = Engine(V, dtype="f32", seed=seed)
            rid, rpar, ralpha = R.beam_decode(oracle_params(eng), torch.from_numpy(img[None]), V - 1, k, max_iter=9, return_alpha=True)
            rpar, ralpha = rpar.numpy(), ralpha.numpy()
            slot = beam_slots(rpar)[0, :, 0]
            steps = np.arange(len(slot))
            read = rpar[0, steps, slot]
            d = float(np.abs(ralpha[0, steps, read] - ralpha[0, steps, rpar[0, :, 0]]).max())
            if d > best:
                found, best = (eng, img, k, rid.numpy(), rpar, ralpha, read), d
    assert found is not None and best > 1e-4, "no image / weights whose back-traced best path leaves slot 0"
    eng, img, k, rid, rpar, ralpha, read = found
    m = Img2SeqModel.__new__(Img2SeqModel)
    m._config = Config({"decoding": "beam_search", "beam_size": k, "beam_backtrace": True, "max_length_formula": 8})     # max_iter 9
    m._vocab, m.engine = Voc(), eng
    text, maps = m.predict_with_attention(img)
    T = rid.shape[1]
    ref = np.stack([ralpha[0, t, read[t]] for t in range(T)])
    assert maps.shape[0] == T
    err = np.abs(maps.reshape(T, -1) - ref).max()
    print("k=%d: back-traced path reads rows %s (slot 0's parents %s); maps vs oracle max |diff| %.2e" % (k, read.tolist(), rpar[0, :, 0].tolist(), err))
    assert err < 1e-6
    old = np.stack([ralpha[0, t, rpar[0, t, 0]] for t in range(T)])
    d_old = np.abs(maps.reshape(T, -1) - old).max()
    print("k=%d: the old read-out (slot 0's parents) would differ by %.2e" % (k, d_old))
    assert d_old > 100 * max(err, 1e-6)                                         # ... it would have drawn another hypothesis' maps


def test_beam_wider_than_vocabulary_is_refused():
    V = 8
    eng = Engine(V, dtype="f32", seed=0)
    img = _img(V, 1)
    for call in (lambda: eng.beam_decode(img, V - 1, 9, max_iter=4), lambda: eng.decode_begin(img, beam_size=9, max_steps=6)):
        with pytest.raises(ValueError, match="9.*8"):
            call()
        assert eng.ws is None and eng.beam == 1                                 # refused before any workspace or launch
    ids, par = eng.beam_decode(img, V - 1, 8, max_iter=4, return_parents=True)     # k = V: every first-step candidate taken
    assert ids.shape[2] == 8 and (ids >= 0).all() and (ids < V).all() and (par >= 0).all() and (par < 8).all()
    assert sorted(ids[0, 0].tolist()) == list(range(V))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "dump-general":
    _dump_fast_cases(sys.argv[2])
