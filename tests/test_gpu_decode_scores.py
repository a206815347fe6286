"""-m gpu: token log-probs and hypothesis scores from the decode loops (lxo_greedy_decode_scores / lxo_beam_decode_scores, Engine
return_scores=True, Img2SeqModel.predict_batch(return_scores=True), predict.py --scores).

Greedy: log_softmax(logits)[id] per step, on the launch-per-step kernels (argmax_kernel) and inside the persistent bf16 chain
(xdec_dec_kernel<NB, true>: every workgroup hands its exponential sum over beside its arg-max word).  Beam: the running log-probs of
the hypotheses (beam_step_kernel / beam_step_fast_kernel).  Asking for scores must not change an id or a parent."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from test_gpu_benchcfg import count_set, V, H, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = V - 1


@pytest.fixture(scope="module")
def end_params():
    """weights that emit END at staggered steps (the recipe of tests/test_gpu_decchain.py)"""
    return train_end_params(V)


def _engine(dtype, params=None, step_kernels=0, seed=0):
    eng = Engine(V, dtype=dtype, seed=seed)
    if params is not None:
        eng.load_params(params)
    eng.step_kernels = step_kernels
    return eng


def _agree_prefix(a, b):
    """mask [B, T]: positions up to and including the first where a and b differ are excluded from there on"""
    same = np.cumprod(a == b, axis=1).astype(bool)
    return same


def test_greedy_f32_logp_vs_oracle():
    img = pad_batch_images(count_set(64, 7)[0])
    eng = _engine("f32", seed=3)
    ids0 = eng.greedy_decode(img, END, max_iter=20)
    ids, lp = eng.greedy_decode(img, END, max_iter=20, return_scores=True)
    assert np.array_equal(ids, ids0) and lp.shape == ids.shape and lp.dtype == np.float32
    rid, logits = R.greedy_decode(oracle_params(eng), torch.from_numpy(img), END, max_iter=20, return_logits=True)
    assert np.array_equal(ids, rid.numpy())
    ref = F.log_softmax(logits.double(), dim=-1).gather(-1, rid.long()[..., None])[..., 0].numpy()
    err = np.abs(lp - ref).max()
    print("greedy f32 B=64: |logp - oracle| max %.2e" % err)
    assert err < 1e-4


@pytest.mark.parametrize("B,chunk", [(64, None), (32, None), (16, None), (8, None), (64, "3"), (16, "3")])
def test_greedy_bf16_chain_scores(end_params, B, chunk):
    img = pad_batch_images(count_set(B, 300 + B)[0])
    eng = _engine("bf16", end_params)

    def run():
        a = eng.greedy_decode(img, END, max_iter=151)
        used0, err0 = eng.chain_status()
        b, lp = eng.greedy_decode(img, END, max_iter=151, return_scores=True)
        used, err = eng.chain_status()
        return a, (used0, err0), b, lp, (used, err)
    a, st0, b, lp, st = with_env("LXO_XDEC_DEC_CHUNK", chunk, run)
    assert st0 == (True, 0) and st == (True, 0), (st0, st)                  # both calls ran the chain, no hand-over timed out
    assert np.array_equal(a, b)                                             # ids bit-identical with and without scores
    c, lpc = _engine("bf16", end_params, step_kernels=2).greedy_decode(img, END, max_iter=151, return_scores=True)
    T = min(b.shape[1], c.shape[1])
    m = _agree_prefix(b[:, :T], c[:, :T])
    err = np.abs(lp[:, :T] - lpc[:, :T])[m].max()
    print("chain B=%d chunk=%s: %d steps, ids agree on %.4f of the columns, |logp chain - step kernels| max %.2e"
          % (B, chunk, b.shape[1], m.mean(), err))
    assert m.mean() > 0.99 and err < 1e-3
    assert np.all(lp[:, :T] <= 1e-6) and np.isfinite(lp).all()


def test_greedy_bf16_chain_scores_filled_up_batch(end_params):
    img = pad_batch_images(count_set(20, 77)[0])
    eng = _engine("bf16", end_params)
    ids, lp = eng.greedy_decode(img, END, max_iter=151, return_scores=True)
    assert ids.shape[0] == 20 and lp.shape == ids.shape
    assert eng.chain_status() == (True, 0)
    full, lpf = _engine("bf16", end_params).greedy_decode(img[np.arange(32) % 20], END, max_iter=151, return_scores=True)
    assert np.array_equal(ids, full[:20]) and np.array_equal(lp, lpf[:20])


@pytest.mark.parametrize("dtype,bar", [("f32", 1e-5), ("bf16", 2e-2)])
def test_sequence_logp_is_minus_the_training_ce(end_params, dtype, bar):
    """sum of a row's token log-probs through its first END = -CE of that formula under teacher forcing (Engine.evaluate_batch)"""
    imgs = count_set(6, 21)[0]
    eng = _engine(dtype, end_params)
    worst = 0.0
    for im in imgs:
        img = pad_batch_images([im])
        ids, lp = eng.greedy_decode(img, END, max_iter=151, return_scores=True)
        n = first_end(ids[0], END) + 1
        assert n > 0 and ids[0, n - 1] == END
        f, l = pad_batch_formulas([list(ids[0, :n - 1])], V - 2, V - 1)
        ce, nw = eng.evaluate_batch(img, f, l)
        assert nw == n
        seq = float(np.sum(lp[0, :n], dtype=np.float64))
        print("%s: %d tokens, sequence log-prob %.7f, CE %.7f" % (dtype, n, seq, ce))
        worst = max(worst, abs(seq + ce) / max(abs(ce), 1.0))          # relative, absolute below |CE| = 1 (a confident model: CE -> 0)
    print("%s: sequence log-prob vs -CE, worst difference %.2e" % (dtype, worst))
    assert worst < bar


def _restate(P, img, ids, par, t, id_end):
    """teacher-forced log-prob of every hypothesis that back-traces from step t (oracle.decoder_train, f64 log_softmax) -> [B, k]"""
    B, _, k = ids.shape
    paths = np.zeros((B, k, t + 1), np.int64)
    slot = np.tile(np.arange(k), (B, 1))
    rows = np.arange(B)[:, None]
    for s in range(t, -1, -1):
        paths[:, :, s] = ids[rows, s, slot]
        slot = par[rows, s, slot]
    enc = R.encoder(P, torch.from_numpy(img))
    enc = enc.repeat_interleave(k, dim=0)
    flat = torch.from_numpy(paths.reshape(B * k, t + 1))
    lg = R.decoder_train(P, enc, flat)
    lp = F.log_softmax(lg.double(), dim=-1).gather(-1, flat[..., None])[..., 0].numpy()
    alive = np.cumsum(np.concatenate([np.zeros((B * k, 1)), (paths.reshape(B * k, -1) == id_end)[:, :-1]], axis=1), axis=1) == 0
    return (lp * alive).sum(axis=1).reshape(B, k)


@pytest.mark.parametrize("k", [2, 5, 12])
def test_beam_f32_scores(k):
    img, _, _ = batch(4, 32, 128, 50, 5, 9, seed=k)
    eng = Engine(50, dtype="f32", seed=1)
    ids0, par0 = eng.beam_decode(img, 49, k, max_iter=12, return_parents=True)
    ids, par, sc = eng.beam_decode(img, 49, k, max_iter=12, return_scores=True)
    assert np.array_equal(ids, ids0) and np.array_equal(par, par0) and sc.shape == ids.shape
    assert (np.diff(sc, axis=2) <= 0).all()                                 # top_k order at every step
    t = ids.shape[1] - 1
    ref = _restate(oracle_params(eng), img, ids, par, t, 49)
    err = (np.abs(sc[:, t] - ref) / np.maximum(1.0, np.abs(ref))).max()
    print("beam f32 k=%d: |final score - teacher-forced restatement| / max(1, |score|) max %.2e" % (k, err))
    assert err < 1e-4


def test_beam_bf16_scores_invariants(end_params):
    img = pad_batch_images(count_set(64, 55)[0])
    eng = _engine("bf16", end_params)
    ids0, par0 = eng.beam_decode(img, END, 5, max_iter=151, return_parents=True)
    ids, par, sc = eng.beam_decode(img, END, 5, max_iter=151, return_scores=True)
    assert np.array_equal(ids, ids0) and np.array_equal(par, par0)
    assert (np.diff(sc, axis=2) <= 0).all()
    from latex_ocr_amd.model.utils.text import beam_backtrace
    B, T, k = ids.shape
    rows = np.arange(B)[:, None]
    fin = np.zeros((B, k), bool)
    frozen = 0
    for t in range(T):
        if t > 0:
            pf = fin[rows, par[:, t]]                                       # the parent had finished: END again, score unchanged
            assert (ids[:, t][pf] == END).all()
            assert np.array_equal(sc[:, t][pf], sc[:, t - 1][rows, par[:, t]][pf])
            frozen += int(pf.sum())
            fin = pf | (ids[:, t] == END)
        else:
            fin = ids[:, 0] == END
    run = beam_backtrace(sc, par)
    d = np.diff(run, axis=1, prepend=0.0)
    assert (d <= 1e-6).all()
    assert np.allclose(d.sum(axis=1), sc[:, -1], rtol=1e-5, atol=1e-4)
    assert frozen > 0


def _model(tmp, decoding, beam=2):
    from latex_ocr_amd import synthetic
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    os.chdir(tmp)
    if not os.path.exists("data/synthetic"):
        synthetic.write_dataset("data/synthetic", n_train=8, n_val=4, n_test=4)
    d = "results/%s/" % decoding
    os.makedirs(d, exist_ok=True)
    cfg = json.load(open(os.path.join(ROOT, "configs", "model.json")))
    cfg.update(decoding=decoding, beam_size=beam, max_length_formula=20)
    json.dump(cfg, open(d + "model.json", "w"))
    shutil.copy(os.path.join(ROOT, "configs", "vocab_small.json"), d + "vocab.json")
    m = Img2SeqModel(Config(d + "model.json"), d, Vocab(Config(d + "vocab.json")))
    m.build_pred()
    return m, d


@pytest.mark.parametrize("decoding", ["greedy", "beam_search"])
def test_predict_batch_scores(tmp_path, monkeypatch, decoding):
    from PIL import Image
    from latex_ocr_amd.model.utils.image import greyscale
    monkeypatch.chdir(tmp_path)
    m, d = _model(str(tmp_path), decoding)
    files = sorted(p for p in os.listdir("data/synthetic/test") if p.endswith(".png"))[:3]
    imgs = [greyscale(np.asarray(Image.open("data/synthetic/test/" + p).convert("RGB"))) for p in files]
    hyps, scores = m.predict_batch(imgs, return_scores=True)
    k = 2 if decoding == "beam_search" else 1
    assert len(hyps) == k and len(scores) == k and all(len(h) == len(imgs) for h in hyps)
    for i in range(k):
        for b in range(len(imgs)):
            seq, toks = scores[i][b]
            assert np.isfinite(seq) and seq <= 1e-5 and abs(seq - sum(toks)) <= 1e-5 * max(1.0, abs(seq))
            assert len(toks) >= len(hyps[i][b].split())
    if decoding == "greedy":
        assert hyps == m.predict_batch(imgs)
    else:
        from latex_ocr_amd.model.utils.text import beam_backtrace
        from latex_ocr_amd.model.evaluation.text import truncate_end
        fd = m._get_feed_dict(imgs, dropout=1)
        ids, par = m.engine.beam_decode(fd["img"], m._vocab.id_end, 2, max_iter=21, return_parents=True)
        bt = beam_backtrace(ids, par)
        for i in range(2):
            for b in range(len(imgs)):
                assert hyps[i][b] == " ".join(m._vocab.id_to_tok[int(x)] for x in truncate_end(bt[b, :, i], m._vocab.id_end))
        assert scores[0][0][0] >= scores[1][0][0]                           # slot order: best first
    if decoding == "beam_search":
        m.save_session(1)
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--scores",
                                       "data/synthetic/test/" + files[0]], cwd=str(tmp_path), timeout=600,
                                      env=dict(os.environ, PYTHONPATH=ROOT)).decode()
        line = [l for l in out.splitlines() if "=>" in l][-1]
        assert "logp" in line and "geo-mean p" in line, out
        assert float(line.split("logp")[1].split()[0]) == pytest.approx(scores[0][0][0], abs=1e-3)
