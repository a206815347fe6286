"""-m gpu: teacher-forced scoring of given formulas (lxo_score_tokens, Engine.score, Img2SeqModel.score_batch, predict.py --formula,
evaluate_txt.py --per-sample): log-probs against the oracle's log_softmax, against the decode loop's own token log-probs when the scored
formula is the greedy path, against evaluate_batch's CE; batches padded for the chains, split above 64; no effect on training."""
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
from test_gpu_decode_scores import end_params  # noqa: F401  (module fixture: weights that emit END at staggered steps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = V - 1
# bf16, greedy path re-scored under teacher forcing, both sides on the persistent chains (decode chain vs training forward chain):
# per-token |logp score - logp decode| (measured on the MI355X with the end_params weights: 7.7e-7 and 8.3e-7 in two runs; the two chains run the same step
# arithmetic -- the bound is the one expected of two different bf16 paths)
BF16_GREEDY_TOL = 2e-2
# bf16, a sample scored inside a padded / split batch against the same sample inside a batch of 64: the chains of different batch sizes
# split the attention over other chunk counts (other summation orders, then bf16 roundings; measured 1.2e-5 and 6.7e-6 over B = 3, 20, 100 in two runs)
BF16_BATCH_TOL = 2e-2


def _engine(dtype, params=None, seed=0, **kw):
    eng = Engine(V, dtype=dtype, seed=seed, **kw)
    if params is not None:
        eng.load_params(params)
    return eng


def _live(lengths, T):
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def test_f32_vs_oracle():
    img, f, l = batch(64, H, W, V, 5, 20, seed=11)
    eng = _engine("f32", seed=3)
    logp, top1, seq = eng.score(img, f, l, return_top1=True)
    assert logp.shape == f.shape and top1.shape == f.shape and seq.shape == (64,)
    P = oracle_params(eng)
    with torch.no_grad():
        lg = R.decoder_train(P, R.encoder(P, torch.from_numpy(img)), torch.from_numpy(f.astype(np.int64))).double()
    ref = F.log_softmax(lg, dim=-1).gather(-1, torch.from_numpy(f.astype(np.int64))[..., None])[..., 0].numpy()
    lg = lg.numpy()
    live = _live(l, f.shape[1])
    err = np.abs(logp - ref)[live].max()
    ref_top = lg.argmax(-1)
    flips = live & (top1 != ref_top)
    gaps = np.take_along_axis(lg, ref_top[..., None], -1)[..., 0] - np.take_along_axis(lg, np.maximum(top1, 0)[..., None], -1)[..., 0]
    print("f32 B=64: |logp - oracle| max %.2e; top1 differs at %d of %d positions, oracle gaps there max %.2e"
          % (err, int(flips.sum()), int(live.sum()), float(gaps[flips].max()) if flips.any() else 0.0))
    assert err < 1e-4
    assert (gaps[flips] <= 1e-4 * np.maximum(1.0, np.abs(lg).max(-1))[flips]).all()       # near-ties only
    assert (logp[~live] == 0).all() and (top1[~live] == -1).all()
    for b in range(64):
        s = np.float32(0)
        for x in logp[b, :l[b]]:
            s = np.float32(s + x)
        assert s == seq[b]


def _greedy_paths(eng, img):
    ids, lp = eng.greedy_decode(img, END, max_iter=151, return_scores=True)
    forms, ns = [], []
    for row in ids:
        e = np.flatnonzero(row == END)
        n = int(e[0]) + 1 if e.size else 0
        forms.append(list(row[:max(n - 1, 0)]))
        ns.append(n)
    return ids, lp, forms, np.array(ns)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_greedy_path_rescored(end_params, dtype):
    img = pad_batch_images(count_set(64, 404)[0])
    eng = _engine(dtype, end_params)
    ids, lp, forms, ns = _greedy_paths(eng, img)
    if dtype == "bf16":
        assert eng.chain_status() == (True, 0)
    ended = ns > 0
    assert ended.mean() > 0.9, ns
    sel = np.flatnonzero(ended)
    f, l = pad_batch_formulas([forms[i] for i in sel], V - 2, END)
    assert np.array_equal(l, ns[sel])
    imgs = img[sel]
    logp, top1, seq = eng.score(imgs, f, l, return_top1=True)
    if dtype == "bf16":
        assert eng.chain_used                                 # the training forward chain (a batch below 64 is padded up to one)
    live = _live(l, f.shape[1])
    err = np.abs(logp - lp[sel, :f.shape[1]])[live].max()
    same = (top1 == ids[sel, :f.shape[1]]) | ~live
    print("%s: %d greedy paths re-scored: |logp score - logp decode| max %.2e, top1 = the path at %.5f of the positions"
          % (dtype, len(sel), err, same[live].mean()))
    assert err < (1e-4 if dtype == "f32" else BF16_GREEDY_TOL)
    if dtype == "f32":
        P = oracle_params(eng)
        with torch.no_grad():
            ref = R.decoder_train(P, R.encoder(P, torch.from_numpy(imgs)), torch.from_numpy(f.astype(np.int64))).double().numpy()
        for b, t in zip(*np.nonzero(~same)):
            gap = ref[b, t].max() - ref[b, t, top1[b, t]]
            assert gap <= 1e-4 * max(1.0, np.abs(ref[b, t]).max()), (b, t, gap)
    else:
        assert same[live].mean() > 0.99


@pytest.mark.parametrize("dtype,bar", [("f32", 1e-5), ("bf16", 1e-4)])
def test_agrees_with_evaluate_batch(end_params, dtype, bar):
    imgs, forms = count_set(64, 505)
    img = pad_batch_images(imgs)
    f, l = pad_batch_formulas(forms, V - 2, END)
    eng = _engine(dtype, end_params)
    _, seq = eng.score(img, f, l)
    ce, n = eng.evaluate_batch(img, f, l)
    tot = -float(np.sum(seq, dtype=np.float64))
    print("%s: -sum seq %.6f, evaluate_batch CE %.6f (%d tokens)" % (dtype, tot, ce, n))
    assert abs(tot - ce) <= bar * abs(ce)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_sizes(end_params, dtype):
    imgs, forms = count_set(100, 606)
    img = pad_batch_images(imgs)
    f, l = pad_batch_formulas(forms, V - 2, END)
    eng = _engine(dtype, end_params)
    ref_lp, ref_seq = {}, {}
    for i in (0, 64):                                       # every sample inside a batch of 64 (rows 36..99 for the second)
        lo = min(i, 100 - 64)
        a, s = eng.score(img[lo:lo + 64], f[lo:lo + 64], l[lo:lo + 64])
        for b in range(64):
            ref_lp[lo + b], ref_seq[lo + b] = a[b], s[b]
    tol = 1e-5 if dtype == "f32" else BF16_BATCH_TOL
    worst = 0.0
    for B in (3, 20):
        lp, seq = eng.score(img[:B], f[:B], l[:B])
        assert lp.shape == (B, f.shape[1]) and seq.shape == (B,)
        if dtype == "bf16":
            assert eng.chain_used and eng.shape.B in (8, 32) and eng.shape.live_B == B         # padded with dead rows, on the chain
        for b in range(B):
            worst = max(worst, np.abs(lp[b] - ref_lp[b]).max())
    lp, seq = eng.score(img, f, l)                           # 64 + 36 (padded to 64)
    assert lp.shape == (100, f.shape[1]) and seq.shape == (100,)
    for b in range(100):
        worst = max(worst, np.abs(lp[b] - ref_lp[b]).max())
    print("%s: per-sample |logp - logp inside a batch of 64| max %.2e over B = 3, 20, 100" % (dtype, worst))
    assert worst <= tol


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_split_is_bit_identical_to_scoring_the_pieces(end_params, dtype):
    imgs, forms = count_set(100, 707)
    img = pad_batch_images(imgs)
    f, l = pad_batch_formulas(forms, V - 2, END)
    eng = _engine(dtype, end_params, deterministic=True)
    lp, top1, seq = eng.score(img, f, l, return_top1=True)
    a = eng.score(img[:64], f[:64], l[:64], return_top1=True)
    b = eng.score(img[64:], f[64:], l[64:], return_top1=True)
    for whole, p0, p1 in zip((lp, top1, seq), a, b):
        assert whole.tobytes() == np.concatenate([p0, p1]).tobytes()


def test_refuses_bad_ids():
    img, f, l = batch(4, 32, 128, V, 3, 6, seed=1)
    eng = _engine("bf16")
    for bad in (-1, V):
        g = f.copy(); g[2, 1] = bad
        with pytest.raises(ValueError):
            eng.score(img, g, l)


def test_no_side_effects_on_training():
    imgs, forms = count_set(16, 808)
    img = pad_batch_images(imgs)
    f, l = pad_batch_formulas(forms, V - 2, END)
    e1 = _engine("bf16", seed=4, deterministic=True)
    e2 = _engine("bf16", seed=4, deterministic=True)
    l1 = [e1.train_step(img, f, l, 1e-3)]
    e1.score(img, f, l, return_top1=True)
    l1.append(e1.train_step(img, f, l, 1e-3))
    l2 = [e2.train_step(img, f, l, 1e-3), e2.train_step(img, f, l, 1e-3)]
    assert l1 == l2, (l1, l2)
    assert torch.equal(e1.params, e2.params) and torch.equal(e1.adam_m, e2.adam_m) and torch.equal(e1.adam_v, e2.adam_v)
    # after a dropout step: the keep probability does not leak into the score
    e1.train_step(img, f, l, 1e-3, dropout=0.5)
    s1 = e1.score(img, f, l, return_top1=True)
    e3 = _engine("bf16", e1.get_params(), deterministic=True)
    s3 = e3.score(img, f, l, return_top1=True)
    for a, b in zip(s1, s3):
        assert a.tobytes() == b.tobytes()


def _results_dir(tmp):
    from latex_ocr_amd import synthetic
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    os.chdir(tmp)
    synthetic.write_dataset("data/synthetic", n_train=8, n_val=4, n_test=6)
    d = "results/score/"
    os.makedirs(d, exist_ok=True)
    cfg = json.load(open(os.path.join(ROOT, "configs", "model.json")))
    cfg.update(max_length_formula=20)
    json.dump(cfg, open(d + "model.json", "w"))
    shutil.copy(os.path.join(ROOT, "configs", "vocab_small.json"), d + "vocab.json")
    shutil.copy(os.path.join(ROOT, "configs", "data_small.json"), d + "data.json")
    m = Img2SeqModel(Config(d + "model.json"), d, Vocab(Config(d + "vocab.json")))
    m.build_pred()
    m.save_session(1)
    return m, d


def test_drivers(tmp_path, monkeypatch):
    from PIL import Image
    from latex_ocr_amd.model.utils.image import greyscale
    monkeypatch.chdir(tmp_path)
    m, d = _results_dir(str(tmp_path))
    png = sorted(p for p in os.listdir("data/synthetic/test") if p.endswith(".png"))[0]
    img = greyscale(np.asarray(Image.open("data/synthetic/test/" + png).convert("RGB")))
    formula = "t1 t2 t3 zz t4"
    lp, toks, first = m.score_batch([img], [formula])[0]
    assert len(toks) == 6 and -1 <= first < 6 and abs(lp - sum(toks)) <= 1e-4 * max(1.0, abs(lp))
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--formula", formula,
                                   "data/synthetic/test/" + png], cwd=str(tmp_path), timeout=600,
                                  env=dict(os.environ, PYTHONPATH=ROOT)).decode()
    line = [x for x in out.splitlines() if "<=" in x][-1]
    assert "logp" in line and "geo-mean p" in line and "first disagreement" in line, out
    assert float(line.split("logp")[1].split()[0]) == pytest.approx(lp, abs=1e-3)
    assert int(line.split("first disagreement")[1].split()[0]) == first
    sys.path.insert(0, ROOT)
    import evaluate_txt
    tsv = str(tmp_path / "per_sample.tsv")
    with_flag = evaluate_txt.main(["--results", d, "--per-sample", tsv])
    without = evaluate_txt.main(["--results", d])
    assert set(with_flag) == set(without)
    for k in without:
        assert with_flag[k] == pytest.approx(without[k], rel=1e-6), k
    rows = [x.split("\t") for x in open(tsv).read().splitlines()]
    n_test = len([x for x in open("data/synthetic/test.matching.txt").read().splitlines() if x.strip()])
    assert len(rows) == n_test and sorted(int(r[0]) for r in rows) == list(range(n_test))
    means = [float(r[3]) for r in rows]
    assert means == sorted(means)
    for r in rows:
        n = len(r[1].split()) + 1
        assert float(r[3]) == pytest.approx(float(r[2]) / n, rel=1e-5, abs=1e-6) and -1 <= int(r[4]) < n
