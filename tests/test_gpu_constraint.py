"""-m gpu: decode under per-image allowed-token sets (lxo_greedy_decode_constrained / lxo_beam_decode_constrained, Engine greedy_decode /
beam_decode with allowed=, Img2SeqModel.predict_batch with banned= / allowed=).

f32: against tests/constraint_ref.py (the oracle's decode with banned columns at -inf) token for token.  bf16: the persistent chain
(xdec_dec_kernel<NB, SC, PF, true>: a banned column is masked where a column >= V is) and the launch-per-step kernels, each against that
reference, and against each other.  Weights that write 7s and then END at staggered steps (the recipe of tests/test_gpu_decchain.py): a set
that keeps 7 and END leaves the model on its path with the constraint present, a set that bans 7 binds.

The bounds are the ones the unconstrained paths are held to (1e-5 for f32 against the reference, 1e-3 between the two bf16 paths on arg-max
tokens, near-tie flips only against the f32 reference); the 0.70 share of compared columns is derived (three quarters of the rows do not
bind, times the 0.99 measured for them without a constraint) and test_bf16_paths_vs_reference_and_each_other prints the measured share."""
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
import constraint_ref

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


def _sets(B, seed, bind=None):
    """A random half of the vocabulary banned per row; 7 and END kept, except that the rows `bind` (default: every fourth) ban 7 -- there the
    constraint takes the trained model's dominant token away"""
    al = np.random.RandomState(seed).rand(B, V) < 0.5
    al[:, END] = True
    al[:, 7] = True
    bind = list(range(3, B, 4)) if bind is None else list(bind)
    al[bind, 7] = False
    return al, bind


def _oracle_enc(params, img):
    P = {k: torch.from_numpy(np.asarray(v).copy()) for k, v in params.items()}
    with torch.no_grad():
        return P, R.encoder(P, torch.from_numpy(img))


def _allowed_everywhere(ids, al):
    """every emitted id lies in its row's set (ids [B, T] or [B, T, k])"""
    return all(al[b][ids[b].reshape(-1)].all() for b in range(ids.shape[0]))


def _agree_prefix(a, b):
    """mask [B, T]: the columns before a row's first divergence"""
    return np.cumprod(a == b, axis=1).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- f32 vs the reference ----
def test_greedy_f32_constrained_vs_reference(end_params):
    img = pad_batch_images(count_set(4, 41)[0])
    al, bind = _sets(4, 1)
    eng = _engine("f32", end_params)
    ids0 = eng.greedy_decode(img, END, max_iter=30)
    ids, lp = eng.greedy_decode(img, END, max_iter=30, return_scores=True, allowed=al)
    P, enc = _oracle_enc(end_params, img)
    with torch.no_grad():
        rid, rlp, _ = constraint_ref.greedy_constrained(P, enc, END, al, 30)
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    assert _allowed_everywhere(ids, al)
    n = min(ids.shape[1], ids0.shape[1])
    for b in bind:                                                          # the constraint binds: the row changed
        assert (ids0[b] == 7).any() and not np.array_equal(ids[b, :n], ids0[b, :n]), b
    err = np.abs(lp - rlp).max()
    print("greedy f32 constrained: %d steps (unconstrained %d), |logp - reference| max %.2e" % (ids.shape[1], ids0.shape[1], err))
    assert err < 1e-5


@pytest.mark.parametrize("k,gamma,prob", [(2, 1.0, 0.0), (3, 0.5, 1.0), (5, 1.0, 0.0), (9, 1.0, 0.0)])
def test_beam_f32_constrained_vs_reference(end_params, k, gamma, prob):
    """k = 2, 5: beam_step_fast_kernel (k V <= 4096, k <= 8); k = 3 with the diversity penalty and k = 9: beam_step_kernel"""
    img = pad_batch_images(count_set(3, 43)[0])
    al, bind = _sets(3, 2, bind=[2])
    eng = _engine("f32", end_params)
    ids0 = eng.beam_decode(img, END, k, max_iter=20, div_gamma=gamma, div_prob=prob, div_seed=5)
    ids, par, sc = eng.beam_decode(img, END, k, max_iter=20, div_gamma=gamma, div_prob=prob, div_seed=5, return_scores=True, allowed=al)
    P, enc = _oracle_enc(end_params, img)
    with torch.no_grad():
        rid, rpar, rsc = constraint_ref.beam_constrained(P, enc, END, k, al, 20, gamma, prob, 5)
    assert ids.shape == rid.shape and np.array_equal(ids, rid) and np.array_equal(par, rpar)
    assert _allowed_everywhere(ids, al)
    n = min(ids.shape[1], ids0.shape[1])
    for b in bind:
        assert (ids0[b] == 7).any() and not np.array_equal(ids[b, :n], ids0[b, :n]), b
    err = np.abs(sc - rsc).max()
    print("beam %d f32 constrained: %d steps, |scores - reference| max %.2e" % (k, ids.shape[1], err))
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
ids, par, sc = eng.beam_decode(pad_batch_images(count_set(3, 43)[0]), V - 1, 5, max_iter=20, return_scores=True, allowed=d["al"])
np.savez(sys.argv[3], ids=ids, par=par, sc=sc)
"""


def test_beam_fast_kernel_constrained_equals_the_general_kernel(end_params, tmp_path):
    """k = 5 at V = 500 takes beam_step_fast_kernel; LXO_BEAM_FAST=0 (read once per process: a child) takes beam_step_kernel -- bit for bit"""
    al, _ = _sets(3, 2, bind=[2])
    eng = _engine("f32", end_params)
    ids, par, sc = eng.beam_decode(pad_batch_images(count_set(3, 43)[0]), END, 5, max_iter=20, return_scores=True, allowed=al)
    np.savez(str(tmp_path / "in.npz"), al=al, **{"p:" + k: np.asarray(v) for k, v in end_params.items()})
    subprocess.check_call([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], timeout=600,
                          env=dict(os.environ, LXO_BEAM_FAST="0"))
    o = np.load(str(tmp_path / "out.npz"))
    assert np.array_equal(ids, o["ids"]) and np.array_equal(par, o["par"]) and np.array_equal(sc.view(np.uint32), o["sc"].view(np.uint32))


def test_beam_bf16_constrained_ids_are_allowed(end_params):
    img = pad_batch_images(count_set(64, 47)[0])
    al, _ = _sets(64, 5)
    ids, par, sc = _engine("bf16", end_params).beam_decode(img, END, 5, max_iter=151, return_scores=True, allowed=al)
    assert _allowed_everywhere(ids, al)
    assert np.isfinite(sc).all() and (np.diff(sc, axis=2) <= 0).all()         # descending within a step


# ---------------------------------------------------------------------------------------------------------------- the bf16 chain: no tolerance ----
@pytest.mark.parametrize("B,chunk", [(8, None), (16, None), (32, None), (64, None), (20, None), (64, "3"), (16, "3")])
def test_chain_constrained_exact_properties(end_params, B, chunk):
    img = pad_batch_images(count_set(B, 700 + B)[0])
    al, bind = _sets(B, B)
    full = np.ones((B, V), bool)

    def run():
        eng = _engine("bf16", end_params)
        st = []
        u = eng.greedy_decode(img, END, max_iter=151); st.append(eng.chain_status())
        u2, ulp = eng.greedy_decode(img, END, max_iter=151, return_scores=True); st.append(eng.chain_status())
        a = eng.greedy_decode(img, END, max_iter=151, allowed=al); st.append(eng.chain_status())
        a2, alp = eng.greedy_decode(img, END, max_iter=151, return_scores=True, allowed=al); st.append(eng.chain_status())
        f = eng.greedy_decode(img, END, max_iter=151, allowed=full); st.append(eng.chain_status())
        f2, flp = eng.greedy_decode(img, END, max_iter=151, return_scores=True, allowed=full); st.append(eng.chain_status())
        # a set that allows every token the unconstrained decode emitted in its row, and bans half of the others
        own = np.random.RandomState(B + 1).rand(B, V) < 0.5
        own[:, END] = True
        for b in range(B):
            own[b, u[b]] = True
        o2, olp = eng.greedy_decode(img, END, max_iter=151, return_scores=True, allowed=own); st.append(eng.chain_status())
        return st, u, u2, ulp, a, a2, alp, f, f2, flp, o2, olp
    st, u, u2, ulp, a, a2, alp, f, f2, flp, o2, olp = with_env("LXO_XDEC_DEC_CHUNK", chunk, run)
    assert all(s == (True, 0) for s in st), st                               # every call ran the chain, no hand-over timed out
    assert a.shape[0] == B and _allowed_everywhere(a, al)
    assert np.array_equal(a, a2)                                             # ids with and without scores
    assert np.isfinite(alp).all() and np.all(alp <= 1e-6)
    for b in bind:
        assert 7 not in a[b]
    assert np.array_equal(f, u) and np.array_equal(f2, u2) and np.array_equal(flp.view(np.uint32), ulp.view(np.uint32))      # every token allowed
    assert np.array_equal(o2, u2)
    low = float((olp - ulp).min())
    print("chain B=%d chunk=%s: %d steps constrained (%d unconstrained); own-token sets: min(logp constrained - unconstrained) %.2e"
          % (B, chunk, a.shape[1], u.shape[1], low))
    assert low >= -1e-3                                                      # renormalising over fewer columns cannot lower a log-prob (bf16 bound below)


def test_filled_up_batch_equals_the_full_batch(end_params):
    img = pad_batch_images(count_set(20, 77)[0])
    al, _ = _sets(20, 9)
    eng = _engine("bf16", end_params)
    ids, lp = eng.greedy_decode(img, END, max_iter=151, return_scores=True, allowed=al)
    assert ids.shape[0] == 20 and eng.chain_status() == (True, 0)
    rows = np.arange(32) % 20
    full, lpf = _engine("bf16", end_params).greedy_decode(img[rows], END, max_iter=151, return_scores=True, allowed=al[rows])
    assert np.array_equal(ids, full[:20]) and np.array_equal(lp.view(np.uint32), lpf[:20].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- bf16 vs the f32 reference ----
def test_bf16_paths_vs_reference_and_each_other(end_params):
    """B = 64: the chain and the launch-per-step kernels each against the f32 reference -- an arg-max flip only where the reference's logits,
    restricted to the allowed columns, leave a near-tie -- and their log-probs against each other on the columns before a row's first
    divergence: 1e-3, the bound tests/test_gpu_decode_scores.py holds the same two paths to.  That comparison must cover >= 0.70 of all
    columns (the rows whose set does not bind, three quarters, times the 0.99 measured for them without a constraint)."""
    B = 64
    img = pad_batch_images(count_set(B, 811)[0])
    al, bind = _sets(B, 13)
    eng = _engine("bf16", end_params)
    a, la = eng.greedy_decode(img, END, max_iter=151, return_scores=True, allowed=al)
    assert eng.chain_status() == (True, 0)
    b, lb = _engine("bf16", end_params, step_kernels=2).greedy_decode(img, END, max_iter=151, return_scores=True, allowed=al)
    assert _allowed_everywhere(a, al) and _allowed_everywhere(b, al)
    P, enc = _oracle_enc(end_params, img)
    with torch.no_grad():
        rid, rlp, rlogits = constraint_ref.greedy_constrained(P, enc, END, al, 151)
    # the reference's logits restricted to the allowed columns: every id compared is allowed (asserted above), so a banned column's value is
    # never a gap's operand; at 0 it does not widen the bar (max |logit| over the row) either
    rlogits = np.where(al[:, None, :], rlogits, 0.0)
    n_a = assert_flips_are_near_ties(a, rid, rlogits, "constrained greedy bf16 chain, B = 64")
    n_b = assert_flips_are_near_ties(b, rid, rlogits, "constrained greedy bf16 launch-per-step, B = 64")
    T = min(a.shape[1], b.shape[1])
    m = _agree_prefix(a[:, :T], b[:, :T])
    share = float(m.sum()) / float(B * max(a.shape[1], b.shape[1]))
    err = np.abs(la[:, :T] - lb[:, :T])[m].max()
    nb = np.ones(B, bool); nb[bind] = False
    print("constrained B=64: chain %d steps, step kernels %d, reference %d; rows diverging from the reference: chain %d, step kernels %d; "
          "chain vs step kernels: agreement before the first divergence on %.4f of all columns (rows that do not bind %.4f, rows that bind %.4f), "
          "|logp chain - step kernels| max %.2e there" % (a.shape[1], b.shape[1], rid.shape[1], n_a, n_b, share, m[nb].mean(), m[~nb].mean(), err))
    assert share >= 0.70
    assert err < 1e-3


# ---------------------------------------------------------------------------------------------------------------- refusals ----
def test_allowed_refusals(end_params):
    eng = _engine("bf16", end_params)
    img = pad_batch_images(count_set(4, 91)[0])
    ok = np.ones((4, V), bool)
    no_end = ok.copy(); no_end[2, END] = False
    few = np.zeros((4, V), bool); few[:, END] = True; few[:, 7] = True          # two tokens: enough for greedy, not for a beam of 3
    pf = np.full((4, 3), 7, np.int32)
    ban7 = ok.copy(); ban7[3, 7] = False
    for kw in [dict(allowed=ok[:3]), dict(allowed=ok[:, :V - 1]), dict(allowed=np.ones((2, 2, V), bool)), dict(allowed=no_end), dict(allowed=np.zeros(V, bool)),
               dict(allowed=ban7, prefix=pf)]:
        with pytest.raises(ValueError):
            eng.greedy_decode(img, END, max_iter=20, **kw)
        with pytest.raises(ValueError):
            eng.beam_decode(img, END, 3, max_iter=20, **kw)
    with pytest.raises(ValueError):
        eng.beam_decode(img, END, 3, max_iter=20, allowed=few)
    assert not hasattr(eng, "_img") and eng.ws is None                        # nothing was staged or launched
    ids = eng.greedy_decode(img, END, max_iter=20, allowed=few)              # greedy: two tokens are enough
    assert np.isin(ids, [7, END]).all()
    ids = eng.greedy_decode(img, END, max_iter=20, allowed=ban7, prefix=pf, prefix_lengths=np.array([3, 3, 3, 0], np.int32))      # dead prefix positions are not checked
    assert (ids[:3, :3] == 7).all() and 7 not in ids[3]
    one = eng.greedy_decode(img, END, max_iter=20, allowed=ban7[3])           # [V]: one set for the batch
    assert 7 not in one


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
def test_predict_batch_banned_and_allowed(tmp_path, monkeypatch, decoding):
    from PIL import Image
    from latex_ocr_amd.model.utils.image import greyscale
    monkeypatch.chdir(tmp_path)
    m, d = _model(str(tmp_path), decoding)
    vocab = m._vocab
    files = sorted(p for p in os.listdir("data/synthetic/test") if p.endswith(".png"))[:3]
    imgs = [greyscale(np.asarray(Image.open("data/synthetic/test/" + p).convert("RGB"))) for p in files]
    k = 2 if decoding == "beam_search" else 1
    free = m.predict_batch(imgs)
    emitted = sorted({t for h in free for s in h for t in s.split()})
    assert emitted                                                           # the randomly initialised model writes something
    ban = ["_UNK", "_PAD"] + emitted[:2]
    hyps, scores = m.predict_batch(imgs, return_scores=True, banned=ban)
    assert len(hyps) == k and all(len(h) == 3 for h in hyps)
    assert not any(t in ban for h in hyps for s in h for t in s.split())
    assert all(np.isfinite(scores[i][b][0]) for i in range(k) for b in range(3))
    assert m.predict_batch(imgs, banned=ban)[0] == hyps[0] or decoding == "beam_search"      # greedy: the unscored call's hypotheses
    assert m.predict_batch(imgs, banned=[vocab.tok_to_id[t] for t in ban]) == m.predict_batch(imgs, banned=ban)      # ids or strings
    some = [t for t in vocab.tok_to_id if vocab.tok_to_id[t] not in (vocab.id_pad, vocab.id_unk)][:6] + ["_END"]
    per_image = [some, some[2:], some[1:]]
    hyps = m.predict_batch(imgs, allowed=per_image)
    for i in range(k):
        for b in range(3):
            assert set(hyps[i][b].split()) <= set(per_image[b])
    with pytest.raises(ValueError):
        m.predict_batch(imgs, banned=["\\no_such_token"])
    with pytest.raises(ValueError):
        m.predict_batch(imgs, banned=["_END"])
    with pytest.raises(ValueError):
        m.predict_batch(imgs, allowed=[some, some])                          # two per-image lists for three images
    # a prefix token the model does not write by itself, and "not that token again" for one it does (a randomly initialised model may
    # write a single token over and over, so the banned token is its first and the prefix is another)
    given = next(t for t in vocab.tok_to_id if t not in emitted and vocab.tok_to_id[t] not in (vocab.id_end, vocab.id_pad, vocab.id_unk))
    done = m.complete_batch(imgs, [given, "", ""], banned=emitted[:1])
    assert len(done) == k and done[0][0].split()[:1] == [given]
    assert not any(emitted[0] in s.split() for h in done for s in h)
    with pytest.raises(ValueError):
        m.complete_batch(imgs, [given, "", ""], banned=[given])              # the prefix token is banned
    m.save_session(1)
    with open("allow.txt", "w") as f:
        f.write("\n".join(some[:-1]) + "\n")
    run = lambda *extra: subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, *extra,
                                                  "data/synthetic/test/" + files[0]], cwd=str(tmp_path), timeout=600,
                                                 env=dict(os.environ, PYTHONPATH=ROOT)).decode()
    line = [l for l in run("--ban", " ".join(ban)).splitlines() if "=>" in l][-1]
    assert not any(t in ban for t in line.split("=>")[1].split()), line
    line = [l for l in run("--scores", "--allow-file", "allow.txt").splitlines() if "=>" in l][-1]
    assert set(line.split("=>")[1].split("\t")[0].split()) <= set(some) and "logp" in line, line
