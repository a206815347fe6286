"""-m gpu: decode from a given prefix (lxo_greedy_decode_prefix / lxo_beam_decode_prefix, Engine greedy_decode / beam_decode with
prefix=, Img2SeqModel.complete_batch).

f32: against tests/prefix_ref.py (the oracle's decode with forced steps) token for token.  bf16: the persistent chain
(xdec_dec_kernel<NB, SC, true>: a forced row takes the prefix token at the boundary; with scores the workgroup owning the forced column
hands its logit over as a third tagged word) against the launch-per-step path, and the forced log-probs against Engine.score.  Weights
that emit END at staggered steps (the recipe of tests/test_gpu_decchain.py)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from test_gpu_benchcfg import count_set, V, H, W
import prefix_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = V - 1


@pytest.fixture(scope="module")
def end_params():
    return train_end_params(V)


def _engine(dtype, params, step_kernels=0):
    eng = Engine(V, dtype=dtype, seed=0)
    eng.load_params(params)
    eng.step_kernels = step_kernels
    return eng


def _prefix(B, T, seed):
    """ids in [0, END): mostly off the model's own path (it writes 7s)"""
    return np.random.RandomState(seed).randint(0, END, size=(B, T)).astype(np.int32)


def _oracle_enc(params, img):
    P = {k: torch.from_numpy(np.asarray(v).copy()) for k, v in params.items()}
    with torch.no_grad():
        return P, R.encoder(P, torch.from_numpy(img))


# ---------------------------------------------------------------------------------------------------------------- f32 vs the reference ----
def test_greedy_f32_prefix_vs_reference(end_params):
    """per-row lengths {0, 1, mid, long}: the long row keeps the loop alive past every other row's END; the step count is the reference's"""
    img = pad_batch_images(count_set(4, 41)[0])
    pf = _prefix(4, 16, 1)
    ln = np.array([0, 1, 5, 16], np.int32)
    eng = _engine("f32", end_params)
    ids, lp = eng.greedy_decode(img, END, max_iter=30, return_scores=True, prefix=pf, prefix_lengths=ln)
    P, enc = _oracle_enc(end_params, img)
    with torch.no_grad():
        rid, rlp = prefix_ref.greedy_prefix(P, enc, END, pf, ln, 30)
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    assert 17 <= ids.shape[1] < 31                                         # the 16-token row kept the loop alive, then finished
    err = np.abs(lp - rlp).max()
    print("greedy f32 prefix: %d steps, |logp - reference| max %.2e" % (ids.shape[1], err))
    assert err < 1e-5


@pytest.mark.parametrize("k,gamma,prob", [(2, 1.0, 0.0), (3, 0.5, 1.0), (5, 1.0, 0.0), (9, 1.0, 0.0)])
def test_beam_f32_prefix_vs_reference(end_params, k, gamma, prob):
    """k = 2, 5: beam_step_fast_kernel (k V <= 4096, k <= 8); k = 3 with the diversity penalty and k = 9: beam_step_kernel"""
    img = pad_batch_images(count_set(3, 43)[0])
    pf = _prefix(3, 6, 2)
    ln = np.array([0, 1, 6], np.int32)
    eng = _engine("f32", end_params)
    ids, par, sc = eng.beam_decode(img, END, k, max_iter=20, div_gamma=gamma, div_prob=prob, div_seed=5, return_scores=True,
                                   prefix=pf, prefix_lengths=ln)
    P, enc = _oracle_enc(end_params, img)
    with torch.no_grad():
        rid, rpar, rsc = prefix_ref.beam_prefix(P, enc, END, k, pf, ln, 20, gamma, prob, 5)
    assert ids.shape == rid.shape and np.array_equal(ids, rid) and np.array_equal(par, rpar)
    for b in range(3):
        assert (ids[b, :ln[b]] == pf[b, :ln[b], None]).all() and (par[b, :ln[b]] == np.arange(k)).all()
    err = np.abs(sc - rsc).max()
    print("beam %d f32 prefix: %d steps, |scores - reference| max %.2e" % (k, ids.shape[1], err))
    assert err < 1e-5 * max(1.0, float(np.abs(rsc).max()))


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
from test_gpu_benchcfg import count_set, V
d = np.load(sys.argv[2])
eng = Engine(V, dtype="f32", seed=0)
eng.load_params({k[2:]: d[k] for k in d.files if k.startswith("p:")})
ids, par, sc = eng.beam_decode(pad_batch_images(count_set(3, 43)[0]), V - 1, 5, max_iter=20, return_scores=True,
                               prefix=d["pf"], prefix_lengths=d["ln"])
np.savez(sys.argv[3], ids=ids, par=par, sc=sc)
"""


def test_beam_fast_kernel_prefix_equals_the_general_kernel(end_params, tmp_path):
    """k = 5 at V = 500 takes beam_step_fast_kernel; LXO_BEAM_FAST=0 (read once per process: a child) takes beam_step_kernel -- bit for bit"""
    pf = _prefix(3, 6, 2)
    ln = np.array([0, 1, 6], np.int32)
    eng = _engine("f32", end_params)
    ids, par, sc = eng.beam_decode(pad_batch_images(count_set(3, 43)[0]), END, 5, max_iter=20, return_scores=True, prefix=pf, prefix_lengths=ln)
    np.savez(str(tmp_path / "in.npz"), pf=pf, ln=ln, **{"p:" + k: np.asarray(v) for k, v in end_params.items()})
    subprocess.check_call([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], timeout=600,
                          env=dict(os.environ, LXO_BEAM_FAST="0"))
    o = np.load(str(tmp_path / "out.npz"))
    assert np.array_equal(ids, o["ids"]) and np.array_equal(par, o["par"]) and np.array_equal(sc.view(np.uint32), o["sc"].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- empty / own prefixes ----
@pytest.mark.parametrize("step_kernels", [0, 2])
@pytest.mark.parametrize("scores", [False, True])
def test_empty_prefixes_are_bit_identical(end_params, step_kernels, scores):
    img = pad_batch_images(count_set(16, 51)[0])
    eng = _engine("bf16", end_params, step_kernels)
    zero = np.zeros(16, np.int32)
    a = eng.greedy_decode(img, END, max_iter=151, return_scores=scores)
    b = eng.greedy_decode(img, END, max_iter=151, return_scores=scores, prefix=_prefix(16, 4, 3), prefix_lengths=zero)
    if step_kernels == 0:
        assert eng.chain_status() == (True, 0)
    for x, y in zip(a if scores else (a,), b if scores else (b,)):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
    img4 = img[:4]
    a = eng.beam_decode(img4, END, 3, max_iter=40, return_parents=True, return_scores=scores)
    b = eng.beam_decode(img4, END, 3, max_iter=40, return_parents=True, return_scores=scores, prefix=_prefix(4, 4, 3),
                        prefix_lengths=zero[:4])
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_own_greedy_prefix_gives_the_same_decode(end_params, dtype):
    """the first P tokens of the model's own greedy output as the prefix: the same ids (bf16: on the chain), and the same logp bit for bit
    (the forced logit is the row max: logits[f] - max = 0)"""
    img = pad_batch_images(count_set(16, 53)[0])
    eng = _engine(dtype, end_params)
    ids, lp = eng.greedy_decode(img, END, max_iter=151, return_scores=True)
    ends = [first_end(r, END) if (r == END).any() else ids.shape[1] for r in ids]
    ln = np.array([min(i % 5, ends[i]) for i in range(16)], np.int32)      # never END inside a prefix
    assert ln.max() > 0
    ids2, lp2 = eng.greedy_decode(img, END, max_iter=151, return_scores=True, prefix=ids[:, :4].copy(), prefix_lengths=ln)
    if dtype == "bf16":
        assert eng.chain_status() == (True, 0)
    assert ids2.shape == ids.shape and np.array_equal(ids2, ids)
    assert np.array_equal(lp2.view(np.uint32), lp.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- the bf16 chain ----
@pytest.mark.parametrize("B", [8, 16, 32, 64, 20])
def test_chain_prefix_equals_launch_per_step(end_params, B):
    imgs, _ = count_set(B, 600 + B)
    img = pad_batch_images(imgs)
    pf = _prefix(B, 12, B)
    ln = (np.arange(B) % 13).astype(np.int32)
    a, la = _engine("bf16", end_params).greedy_decode(img, END, max_iter=151, return_scores=True, prefix=pf, prefix_lengths=ln)
    eng = _engine("bf16", end_params)
    a2 = eng.greedy_decode(img, END, max_iter=151, prefix=pf, prefix_lengths=ln)
    assert eng.chain_status() == (True, 0)
    assert a.shape[0] == B and np.array_equal(a, a2)                       # ids with and without scores
    b, lb = _engine("bf16", end_params, step_kernels=2).greedy_decode(img, END, max_iter=151, return_scores=True, prefix=pf, prefix_lengths=ln)
    for r in range(B):
        assert np.array_equal(a[r, :ln[r]], pf[r, :ln[r]])
    assert a.shape == b.shape, (a.shape, b.shape)
    assert a.shape[1] > ln.max()                                           # the longest prefixes kept the loop alive
    agree = float((a == b).mean())
    forced = np.arange(a.shape[1])[None, :] < ln[:, None]
    err = np.abs(la - lb)[forced].max()
    print("chain B=%d prefix: %d steps, ids agree with the launch-per-step path on %.4f, |forced logp chain - step kernels| max %.2e"
          % (B, a.shape[1], agree, err))
    assert agree >= 0.999, np.argwhere(a != b)[:8]
    assert err < 2e-2                                                      # bf16 (test_gpu_score.py's bound): a forced logit is no row max
                                                                           # and its rounding does not cancel (measured: 1.1e-3 at B = 64)


@pytest.mark.parametrize("lens", [(2, 3, 4, 6), (3, 6, 9, 1)])
def test_chain_prefix_across_launches(end_params, lens):
    """launches of 3 steps: prefixes that end inside a launch (2, 4) and exactly at a launch boundary (3, 6, 9)"""
    img = pad_batch_images(count_set(16, 71)[0])
    pf = _prefix(16, 10, 9)
    ln = np.array([lens[i % 4] for i in range(16)], np.int32)

    def run():
        eng = _engine("bf16", end_params)
        out = eng.greedy_decode(img, END, max_iter=151, return_scores=True, prefix=pf, prefix_lengths=ln)
        return out, eng.chain_status()
    (a, la), st = with_env("LXO_XDEC_DEC_CHUNK", "3", run)
    assert st == (True, 0), st
    (c, lc), _ = run()
    b, lb = _engine("bf16", end_params, step_kernels=2).greedy_decode(img, END, max_iter=151, return_scores=True, prefix=pf, prefix_lengths=ln)
    assert np.array_equal(a, c) and np.array_equal(la.view(np.uint32), lc.view(np.uint32))      # launch boundaries change nothing
    assert a.shape == b.shape and (a == b).mean() >= 0.999


@pytest.mark.parametrize("B", [16, 64])
def test_chain_forced_logp_vs_score(end_params, B):
    """the chain's forced log-probs against teacher-forced Engine.score of the same tokens (the bf16 bound of test_gpu_score.py), one row
    forced onto its LEAST likely first token (the third hand-over word carries that logit itself: no exp-sum re-based on it)"""
    img = pad_batch_images(count_set(B, 81)[0])
    eng = _engine("bf16", end_params)
    eng.decode_begin(img, 1, max_steps=152)
    _, _, _, logits = eng.decode_step(0, END)
    worst = int(np.argmin(np.where(np.arange(V) == END, np.inf, logits[0])))
    pf = _prefix(B, 8, 11)
    pf[0, 0] = worst
    ln = np.array([8, 3, 1, 5] * (B // 4), np.int32)
    eng = _engine("bf16", end_params)
    ids, lp = eng.greedy_decode(img, END, max_iter=151, return_scores=True, prefix=pf, prefix_lengths=ln)
    assert eng.chain_status() == (True, 0)
    s_lp, _ = _engine("bf16", end_params).score(img, pf, ln)
    forced = np.arange(8)[None, :] < ln[:, None]
    err = np.abs(lp[:, :8] - s_lp)[forced].max()
    print("chain B=%d forced logp vs Engine.score: max |diff| %.2e; least likely token %d at logp %.2f (score %.2f)" % (B, err, worst, lp[0, 0], s_lp[0, 0]))
    assert lp[0, 0] <= lp[0, 1:][np.isfinite(lp[0, 1:])].min() + 1e-3 or lp[0, 0] < -10.0
    assert err < 2e-2


# ---------------------------------------------------------------------------------------------------------------- refusals ----
def test_prefix_refusals(end_params):
    eng = _engine("bf16", end_params)
    img = pad_batch_images(count_set(4, 91)[0])
    pf = _prefix(4, 5, 4)
    bad = [
        dict(prefix=pf[:3]),                                                          # shape: 3 rows for 4 images
        dict(prefix=pf, prefix_lengths=np.array([1, 2, 3], np.int32)),                # lengths shape
        dict(prefix=np.where(np.arange(5) == 2, V, pf)),                              # id >= V
        dict(prefix=np.where(np.arange(5) == 1, -1, pf)),                             # id < 0
        dict(prefix=np.where(np.arange(5) == 0, END, pf)),                            # END inside a prefix
        dict(prefix=pf, prefix_lengths=np.array([1, 6, 0, 0], np.int32)),             # length > T_prefix
        dict(prefix=pf, prefix_lengths=np.array([1, -1, 0, 0], np.int32)),            # length < 0
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.greedy_decode(img, END, max_iter=151, **kw)
        with pytest.raises(ValueError):
            eng.beam_decode(img, END, 2, max_iter=151, **kw)
    with pytest.raises(ValueError):
        eng.greedy_decode(img, END, max_iter=3, prefix=pf)                            # length > max_iter
    ok = np.where(np.arange(5) == 4, V + 3, pf)                                       # beyond every length: not read
    ids = eng.greedy_decode(img, END, max_iter=20, prefix=ok, prefix_lengths=np.array([4, 4, 0, 2], np.int32))
    assert np.array_equal(ids[0, :4], pf[0, :4])


# ---------------------------------------------------------------------------------------------------------------- the facade ----
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
def test_complete_batch(tmp_path, monkeypatch, decoding):
    from PIL import Image
    from latex_ocr_amd.model.utils.image import greyscale
    monkeypatch.chdir(tmp_path)
    m, d = _model(str(tmp_path), decoding)
    files = sorted(p for p in os.listdir("data/synthetic/test") if p.endswith(".png"))[:3]
    imgs = [greyscale(np.asarray(Image.open("data/synthetic/test/" + p).convert("RGB"))) for p in files]
    k = 2 if decoding == "beam_search" else 1
    toks = [t for t in m._vocab.tok_to_id if m._vocab.tok_to_id[t] not in (m._vocab.id_end, m._vocab.id_pad)][:3]
    given = [" ".join(toks[:2]), [m._vocab.tok_to_id[toks[2]]], ""]
    hyps, scores = m.complete_batch(imgs, given, return_scores=True)
    assert len(hyps) == k and all(len(h) == 3 for h in hyps)
    for i in range(k):
        assert hyps[i][0].split()[:2] == toks[:2] and hyps[i][1].split()[:1] == toks[2:3]
        for b in range(3):
            seq, tl = scores[i][b]
            assert np.isfinite(seq) and abs(seq - sum(tl)) <= 1e-5 * max(1.0, abs(seq))
    ref_h, ref_s = m.predict_batch(imgs, return_scores=True)
    if decoding == "greedy":
        ref = m.predict_batch(imgs)
        own = [" ".join(h.split()[:2]) for h in ref[0]]                  # the model's own first tokens as the prefix
        assert m.complete_batch(imgs, own) == ref == ref_h
    else:
        h0, s0 = m.complete_batch(imgs, ["", "", ""], return_scores=True)
        assert h0 == ref_h and s0 == ref_s                                 # empty prefixes: predict_batch(return_scores=True)'s hypotheses
    m.save_session(1)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--scores", "--prefix", given[0],
                                   "data/synthetic/test/" + files[0]], cwd=str(tmp_path), timeout=600,
                                  env=dict(os.environ, PYTHONPATH=ROOT)).decode()
    line = [l for l in out.splitlines() if "=>" in l][-1]
    assert line.split("=>")[1].split()[:2] == toks[:2] and "logp" in line, out
