"""-m gpu: sampled decode (lxo_sample_decode / lxo_sample_tokens, Engine.sample_decode / sample_tokens, Img2SeqModel.sample_batch,
predict.py --sample) against tests/sample_ref.py, the float64 restatement of the definition in head_kernels.h.

One criterion: a kernel token that differs from the reference's must lie in the reference's candidate set with a reference perturbed score
within the bound of the reference's best -- sample_ref's near-tie bound for given logits, plus the error of the logits where the kernel computed
them itself (f32: 2 * 1e-5 * max(1, max|x|) / tau, 1e-5 being the bound the sibling f32 tests hold; bf16: gpu_common.assert_flips_are_near_ties'
8 * 2^-8 * max|x|, scaled by 1 / tau).  At most 0.1 % of the compared draws may differ at all, on given logits and in the f32
end-to-end comparisons alike (bf16: the share of rows agreeing through step 5 instead, as the sibling bf16 tests)."""
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
from test_gpu_benchcfg import count_set, V
import sample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = V - 1
TAU, MAX_ITER = 1.5, 20
# (V, ld): both sides of every row-kind boundary, as tests/test_sample_sim.py's list; the options are a hand-picked list of 12 combinations in which
# every value the issue names occurs (the sim tests run the whole tau x K x p product on the small rows).  The register row at ld % 4 == 0 and ld <= 1024 (KV = 4, 8, 16), the strided row elsewhere
SHAPES = [(5, 8), (5, 5), (11, 12), (11, 11), (64, 64), (65, 68), (65, 65), (500, 512), (501, 501), (256, 256), (258, 260), (512, 512), (514, 516),
          (1024, 1024), (1026, 1028)]


@pytest.fixture(scope="module")
def end_params():
    return train_end_params(V)


@pytest.fixture(scope="module")
def images():
    return pad_batch_images(count_set(4, 41)[0])


@pytest.fixture(scope="module")
def oracle(end_params, images):
    """the oracle's parameters and its encoder features of the module's images, once"""
    P = {k: torch.from_numpy(np.asarray(v).copy()) for k, v in end_params.items()}
    with torch.no_grad():
        return P, R.encoder(P, torch.from_numpy(images))


_REF = {}


def _reference(oracle, n, seed, tau=TAU, **kw):
    """sample_ref.sample_decode of the module's images, computed once per argument set and left unchanged"""
    key = (n, seed, tau, json.dumps({k: np.asarray(v).tolist() for k, v in kw.items()}, sort_keys=True))
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = sample_ref.sample_decode(oracle[0], oracle[1], END, n, MAX_ITER, tau, 0, 1.0, seed, **kw)
    return _REF[key]


def _engine(dtype, params, step_kernels=0):
    eng = Engine(V, dtype=dtype, seed=0)
    eng.load_params(params)
    eng.step_kernels = step_kernels
    return eng


# ---------------------------------------------------------------------------------------------------------------- the select step on given logits ----
def _sets(Vn, images, seed):
    al = np.random.RandomState(seed).rand(images, Vn) < 0.6
    al[:, Vn - 1] = True; al[:, 0] = True
    al[0] = True
    al[1] = False; al[1, Vn - 1] = True                                       # a row that allows only END
    return al


def _case(Vn, rows, scale, lseed, n, t, tau, K, p, seed, allow):
    """logits [rows, Vn] and their reference picks; with top-p on, rows whose cumulative mass stays clear of p at every column"""
    lg = (np.random.RandomState(lseed).randn(rows, Vn) * scale).astype(np.float32)
    for k in range(200):
        ref = sample_ref.sample_tokens(lg, n, t, tau, K, p, seed, allow)
        close = [r for r, q in enumerate(ref) if q.margin <= 2e-4]
        if not close:
            return lg, ref
        for r in close:
            lg[r] = (np.random.RandomState(lseed + 1000 * (k + 1) + r).randn(Vn) * scale).astype(np.float32)
    raise AssertionError("no logits clear of p")


@pytest.mark.parametrize("Vn,ld", SHAPES)
def test_tokens_match_the_reference(Vn, ld):
    eng = Engine(Vn, dtype="f32", seed=0)
    n, images = 3, 3
    rows = n * images
    combos = [(1.0, 0, 1.0), (0.5, 0, 1.0), (2.0, 0, 1.0), (1.0, 1, 1.0), (1.0, 3, 1.0), (1.0, Vn, 1.0), (1.0, 0, 0.9), (1.0, 0, 0.5),
              (2.0, 3, 0.9), (0.5, Vn, 0.5), (2.0, max(1, Vn // 3), 0.5), (0.5, 3, 0.9)]
    compared = differ = 0
    for ci, (tau, K, p) in enumerate(combos):
        for with_sets in (False, True):
            al = _sets(Vn, images, ci) if with_sets else None
            lg, ref = _case(Vn, rows, (1.0, 5.0, 30.0)[ci % 3], 100 + ci, n, 3 + ci, tau, K, p, 7 + ci, al)
            dev = torch.full((rows, ld), 1.0e30, dtype=torch.float32, device=eng.device)      # the padding must never be read as a column
            dev[:, :Vn] = torch.from_numpy(lg)
            ids, lp, lq = eng.sample_tokens(dev[:, :Vn], n=n, time=3 + ci, temperature=tau, top_k=K, top_p=p, seed=7 + ci, allowed=al)
            for r, q in enumerate(ref):
                if p < 1.0:
                    assert q.margin > 1e-4
                assert 0 <= ids[r] < Vn and q.cand[ids[r]], (r, ids[r])
                compared += 1
                if ids[r] != q.id:
                    differ += 1
                    assert sample_ref.flip_ok(q, int(ids[r])), (r, ids[r], q.id, q.tol)
                    continue
                assert abs(lp[r] - q.logp) < 1e-5 * max(1.0, abs(q.logp)) and abs(lq[r] - q.logq) < 1e-5, (r, lp[r], q.logp, lq[r], q.logq)
                if K == 1:
                    assert ids[r] == np.where(al[r // n], lg[r], -np.inf).argmax() if with_sets else ids[r] == lg[r].argmax()
            if with_sets:
                assert (ids[n:2 * n] == Vn - 1).all()
    print("V = %d, ld = %d: draws compared %d, differing %d" % (Vn, ld, compared, differ))
    assert differ <= 1e-3 * compared


def test_frequencies_follow_the_softmax():
    row = np.array([2, 1, .5, 0, -.5, -1, 1.5, -2, .25, -.25, .75], np.float32)
    eng = Engine(11, dtype="f32", seed=0)
    lg = torch.from_numpy(np.tile(row, (64 * 16, 1))).to(eng.device)
    counts = np.zeros(11, np.int64); counts3 = np.zeros(11, np.int64)
    for t in range(32):
        counts += np.bincount(eng.sample_tokens(lg, n=16, time=t, temperature=1.0, seed=1)[0], minlength=11)
        counts3 += np.bincount(eng.sample_tokens(lg, n=16, time=t, temperature=1.0, top_k=3, seed=1)[0], minlength=11)
    assert counts.sum() == 32768
    e = np.exp(row.astype(np.float64)); e = e / e.sum() * counts.sum()
    chi2 = float(((counts - e) ** 2 / e).sum())
    print("chi^2 of 32768 draws against the softmax: %.2f (0.999 quantile at 10 degrees of freedom: 29.59)" % chi2)
    assert chi2 < 29.59
    assert counts3.sum() == 32768 and counts3[[0, 6, 1]].sum() == 32768 and (counts3[[0, 6, 1]] > 0).all()


# ---------------------------------------------------------------------------------------------------------------- f32 end to end ----
def _check_against_reference(ids, lp, lq, ref, what, tau=TAU):
    rid, rlp, rlq, picks, _ = ref
    compared, differ, agree = sample_ref.compare_decode(ids, rid, picks, lambda q: 2.0 * 1e-5 * max(1.0, q.xmax) / tau)
    T = agree.shape[1]
    err_p = np.abs(lp[:, :T] - rlp[:, :T])[agree] / np.maximum(1.0, np.abs(rlp[:, :T][agree]))
    err_q = np.abs(lq[:, :T] - rlq[:, :T])[agree] / np.maximum(1.0, np.abs(rlq[:, :T][agree]))
    print("%s: %d steps (reference %d), draws compared %d, differing %d, |logp - ref| max %.2e, |logq - ref| max %.2e"
          % (what, ids.shape[1], rid.shape[1], compared, differ, err_p.max(), err_q.max()))
    assert err_p.max() < 1e-5 and err_q.max() < 1e-5
    assert differ <= 1e-3 * compared


@pytest.mark.parametrize("n", [1, 5, 9])
def test_f32_decode_vs_reference(end_params, images, oracle, n):
    eng = _engine("f32", end_params)
    ids, lp, lq = eng.sample_decode(images, END, n=n, temperature=TAU, seed=3, max_iter=MAX_ITER, return_scores=True)
    assert ids.shape[0] == 4 and ids.shape[2] == n
    _check_against_reference(ids, lp, lq, _reference(oracle, n, 3), "sample f32 n = %d" % n)
    if n > 1:
        # These weights are so peaked that at tau = 1.5 the draws of ONE image all agree (measured: 3 distinct sequences over the 4 images, one per
        # image, at n = 5 and n = 9, the reference's too): distinct sequences occur across the images, and a flat temperature shows that the draws of
        # an image vary -- against the reference as well.
        seqs = {tuple(ids[b, :, j]) for b in range(4) for j in range(n)}
        print("n = %d, tau = %.1f: %d distinct sequences" % (n, TAU, len(seqs)))
        assert len(seqs) >= 2
        hot = eng.sample_decode(images, END, n=n, temperature=8.0, seed=3, max_iter=MAX_ITER, return_scores=True)
        _check_against_reference(hot[0], hot[1], hot[2], _reference(oracle, n, 3, tau=8.0), "sample f32 n = %d, tau = 8" % n, tau=8.0)
        per_image = [len({tuple(hot[0][b, :, j]) for j in range(n)}) for b in range(4)]
        print("n = %d, tau = 8: distinct sequences per image %s" % (n, per_image))
        assert min(per_image) >= 2
    again = eng.sample_decode(images, END, n=n, temperature=TAU, seed=3, max_iter=MAX_ITER, return_scores=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip((ids, lp, lq), again))


def test_f32_decode_with_sets_and_prefix(end_params, images, oracle):
    eng = _engine("f32", end_params)
    al = np.ones((4, V), bool); al[2, 7] = False
    ids, lp, lq = eng.sample_decode(images, END, n=5, temperature=TAU, seed=4, max_iter=MAX_ITER, return_scores=True, allowed=al)
    assert 7 not in ids[2]
    _check_against_reference(ids, lp, lq, _reference(oracle, 5, 4, allow=al), "sample f32 n = 5, 7 banned on image 2")
    pf = np.array([[7, 7, 3], [5, 0, 0], [9, 8, 7], [1, 2, 3]], np.int32); ln = np.array([3, 1, 0, 2], np.int32)
    ids, lp, lq = eng.sample_decode(images, END, n=5, temperature=TAU, seed=5, max_iter=MAX_ITER, return_scores=True, prefix=pf, prefix_lengths=ln)
    for b in range(4):
        assert (ids[b, :ln[b]] == pf[b, :ln[b], None]).all() and (lq[b, :ln[b]] == 0).all()
    _check_against_reference(ids, lp, lq, _reference(oracle, 5, 5, prefix=pf, lengths=ln), "sample f32 n = 5, prefixes")


@pytest.mark.parametrize("n", [1, 5])
def test_top_k_1_equals_greedy(end_params, images, n):
    gid, glp = _engine("f32", end_params, step_kernels=2).greedy_decode(images, END, max_iter=MAX_ITER, return_scores=True)
    eng = _engine("f32", end_params)
    ids, lp, lq = eng.sample_decode(images, END, n=n, temperature=0.8, top_k=1, seed=6, max_iter=MAX_ITER, return_scores=True)
    assert ids.shape[1] == gid.shape[1]
    for j in range(n):
        assert np.array_equal(ids[:, :, j], gid) and np.abs(lp[:, :, j] - glp).max() < 1e-5
    assert (lq == 0).all()
    zero = eng.sample_decode(images, END, n=n, temperature=0, seed=6, max_iter=MAX_ITER)       # temperature 0 means top_k = 1
    assert np.array_equal(zero, ids)


def test_refusals_before_any_launch(end_params, images):
    eng = _engine("f32", end_params)
    for kw in [dict(n=0), dict(n=17), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature=1e-39), dict(top_k=-1),
               dict(top_p=0.0), dict(top_p=1.5), dict(allowed=np.zeros(V, bool)), dict(prefix=np.full((4, 2), END, np.int32))]:
        with pytest.raises(ValueError):
            eng.sample_decode(images, END, max_iter=MAX_ITER, **kw)
    assert not hasattr(eng, "_img") and eng.ws is None
    with pytest.raises(ValueError):
        eng.sample_tokens(np.zeros((4, V + 1), np.float32))


# ---------------------------------------------------------------------------------------------------------------- bf16 ----
def test_bf16_decode_vs_the_f32_reference(end_params, images, oracle):
    n = 5
    eng = _engine("bf16", end_params)
    ids, lp, lq = eng.sample_decode(images, END, n=n, temperature=TAU, seed=3, max_iter=MAX_ITER, return_scores=True)
    rid, rlp, rlq, picks, _ = _reference(oracle, n, 3)
    # the differing token's reference perturbed score within 8 * 2^-8 * max|logit| / tau of the reference's best (flip_ok adds q.tol to extra)
    compared, differ, agree = sample_ref.compare_decode(ids, rid, picks, lambda q: 8.0 * 2.0 ** -8 * q.xmax / TAU - q.tol)
    T = agree.shape[1]
    through = min(6, T)
    share = float(agree[:, :through].all(axis=1).mean())
    print("sample bf16 n = %d: %d steps (reference %d), draws compared %d, rows diverging %d, share of rows agreeing through step 5: %.3f"
          % (n, ids.shape[1], rid.shape[1], compared, differ, share))
    assert share >= 0.70
    assert np.isfinite(lp).all() and np.isfinite(lq).all() and (lp <= 1e-6).all() and (lq <= 1e-6).all()
    again = eng.sample_decode(images, END, n=n, temperature=TAU, seed=3, max_iter=MAX_ITER, return_scores=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip((ids, lp, lq), again))


# ---------------------------------------------------------------------------------------------------------------- the model layer ----
def _model(tmp):
    from latex_ocr_amd import synthetic
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    if not os.path.exists("data/synthetic"):
        synthetic.write_dataset("data/synthetic", n_train=8, n_val=4, n_test=4)
    d = "results/greedy/"
    os.makedirs(d, exist_ok=True)
    cfg = json.load(open(os.path.join(ROOT, "configs", "model.json")))
    cfg.update(decoding="greedy", max_length_formula=20)
    json.dump(cfg, open(d + "model.json", "w"))
    shutil.copy(os.path.join(ROOT, "configs", "vocab_small.json"), d + "vocab.json")
    m = Img2SeqModel(Config(d + "model.json"), d, Vocab(Config(d + "vocab.json")))
    m.build_pred()
    return m, d


def test_sample_batch_and_predict_sample(tmp_path, monkeypatch):
    from PIL import Image
    from latex_ocr_amd.model.utils.image import greyscale
    monkeypatch.chdir(tmp_path)
    m, d = _model(str(tmp_path))
    files = sorted(p for p in os.listdir("data/synthetic/test") if p.endswith(".png"))[:3]
    imgs = [greyscale(np.asarray(Image.open("data/synthetic/test/" + p).convert("RGB"))) for p in files]
    res = m.sample_batch(imgs, 8, temperature=1.0, seed=2, banned=["_UNK", "_PAD"])
    assert len(res) == 3
    for r in res:
        hyps = r["hypotheses"]
        assert sum(h["count"] for h in hyps) == 8 and 0.0 < r["agreement"] <= 1.0 and r["agreement"] == hyps[0]["count"] / 8.0
        assert [(-h["count"], -h["logp"]) for h in hyps] == sorted((-h["count"], -h["logp"]) for h in hyps)
        assert len({h["text"] for h in hyps}) == len(hyps)
        assert all(np.isfinite(h["logp"]) and abs(h["logp"] - sum(h["token_logp"])) < 1e-4 for h in hyps)
        assert not any(t in ("_UNK", "_PAD") for h in hyps for t in h["text"].split())
    assert m.sample_batch(imgs, 8, temperature=1.0, seed=2, banned=["_UNK", "_PAD"]) == res
    one = m.sample_batch(imgs, 4, top_k=1)
    for r in one:
        assert len(r["hypotheses"]) == 1 and r["hypotheses"][0]["count"] == 4 and r["agreement"] == 1.0
    assert m.sample_batch(imgs, 4, temperature=0) == one
    m.save_session(1)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--sample", "4", "--temperature", "1.2", "--top-k", "20",
                                   "--top-p", "0.95", "--seed", "3", "data/synthetic/test/" + files[0]], cwd=str(tmp_path), timeout=600,
                                  env=dict(os.environ, PYTHONPATH=ROOT)).decode()
    head = [l for l in out.splitlines() if "~>" in l]
    rows = [l for l in out.splitlines() if " x  logp" in l]
    assert len(head) == 1 and "agreement" in head[0] and 1 <= len(rows) <= 4, out
    assert sum(int(l.split("x")[0]) for l in rows) == 4, out
