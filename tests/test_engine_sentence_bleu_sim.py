"""CPU (hipsim): the sentence-BLEU cost above the C ABI -- Engine.sentence_bleu, Engine.consensus(cost="bleu"), Engine.sample_decode(consensus_cost=),
Engine.mrt_sample_step(cost="bleu"), Img2SeqModel.mrt_batch(cost=) on both paths, sample_batch(consensus_cost=), the training config's "cost" key and
predict.py --consensus-cost -- against the float64 reference of tests/sentence_bleu_ref.py and the host sentence_bleu_cost; the gradient identity of
tests/test_engine_weighted_sim.py with the BLEU costs plugged in; and every default: the calls and the bytes they had."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.evaluation.text import sentence_bleu_cost
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import pad_batch_formulas
from simlib import SIM_SO, build_sim
from edit_distance_ref import host_candidates
from sentence_bleu_ref import BOUND, GAP, RISK_BOUND, bleu_of, counts_of, host_consensus
import mrt_oracle

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, H, W = 11, 32, 48
END, PAD = 10, 9
N, ALPHA, MAX_ITER = 3, 0.7, 4
SAMPLING = dict(temperature=0.5, top_k=3, seed=5)                   # tests/test_engine_mrt_device_sim.py's: a draw of image 0 repeats, others differ
SAMPLING2 = dict(temperature=0.5, top_k=2, seed=4)
REFS = [[0, 1, 2], [3, 4]]
LOSS_TOL, MIN_COS = 2e-5, 0.9999                                   # tests/test_engine_weighted_sim.py's bars
NEW = ("lxo_sentence_bleu", "lxo_consensus_bleu", "lxo_mrt_candidates_cost")


class Counting(object):
    """the library with its calls counted by name"""
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("lxo_"):
            return f

        def g(*a):
            self.calls.append(name)
            return f(*a)
        return g


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


def _engine(lib):
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=MAX_ITER + 1)


def _images():
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    return pad_batch_images(imgs)


def test_sentence_bleu_takes_arrays_tensors_and_views(lib):
    eng = _engine(lib)
    rng = np.random.default_rng(3)
    hyp = rng.integers(0, 3, size=(6, 12)).astype(np.int32)
    ref = rng.integers(0, 3, size=(3, 9)).astype(np.int32)
    hl, rl = np.array([12, 0, 5, 7, 12, 1]), np.array([9, 4, 0])
    pairs = [(list(hyp[p, :hl[p]]), list(ref[p // 2, :rl[p // 2]])) for p in range(6)]
    want = np.array([bleu_of(h, r) for h, r in pairs])
    b = eng.sentence_bleu(hyp, ref, hl, rl)
    assert b.dtype == np.float32 and b.shape == (6,) and np.abs(b - want).max() <= BOUND and (want > 0).any()
    b2, c2 = eng.sentence_bleu(torch.from_numpy(hyp), torch.from_numpy(ref), torch.from_numpy(hl), torch.from_numpy(rl), return_counts=True)
    assert b2.tobytes() == b.tobytes() and c2.dtype == np.int32 and c2.tolist() == [counts_of(h, r) for h, r in pairs]
    assert np.array_equal(c2, eng.text_stats(hyp, ref, hl, rl)[:, :_abi.LXO_BLEU_COUNTS])
    idx = np.array([2, 2, 0, 1, 0, 1])
    b3 = eng.sentence_bleu(hyp, ref, ref_index=idx)
    assert np.abs(b3 - [bleu_of(list(hyp[p]), list(ref[idx[p]])) for p in range(6)]).max() <= BOUND
    # an equal pair and a pair without a common token, cut at END: exactly 1 and 0
    f, fl = pad_batch_formulas([[0, 1], [2]], PAD, END)
    assert eng.sentence_bleu(f, f, fl, fl, id_end=END).tobytes() == np.ones(2, np.float32).tobytes()
    assert eng.sentence_bleu(f, f[::-1].copy(), id_end=END).tobytes() == np.zeros(2, np.float32).tobytes()
    # the [B, T, n] ids of a sampled decode, as a device tensor read in place, and a permuted view of rows [B, n, T]
    ids = rng.integers(0, 3, size=(2, 10, 3)).astype(np.int32)
    refs = rng.integers(0, 2, size=(2, 8)).astype(np.int32)
    w3 = np.array([bleu_of(list(ids[g, :, j][:list(ids[g, :, j]).index(2)] if 2 in ids[g, :, j] else ids[g, :, j]), list(refs[g])) for g in range(2) for j in range(3)])
    t = torch.from_numpy(np.concatenate([ids, np.full((2, 2, 3), 2, np.int32)], axis=1))[:, :10]
    b4 = eng.sentence_bleu(t, refs, id_end=2)
    assert np.abs(b4 - w3).max() <= BOUND
    view = torch.from_numpy(np.ascontiguousarray(ids.transpose(0, 2, 1))).permute(0, 2, 1)
    assert not view.is_contiguous() and eng.sentence_bleu(view, refs, id_end=2).tobytes() == b4.tobytes()
    # the edges: no pair, a side without a column
    assert eng.sentence_bleu(hyp[:0], ref).shape == (0,) and eng.sentence_bleu(hyp[:0], ref, return_counts=True)[1].shape == (0, 10)
    assert not eng.sentence_bleu(hyp[:, :0], ref).any() and not eng.sentence_bleu(hyp, ref[:, :0]).any()
    for bad in (dict(hyp=hyp[0]), dict(ref=ref[0]), dict(hyp=hyp[:5]), dict(hyp_lengths=hl[:5]), dict(ref_lengths=rl[:2]), dict(ref_index=idx[:5]),
                dict(ref_index=np.array([0, 1, 2, 3, 0, 0])), dict(ref=np.zeros((3, _abi.LXO_EDIT_MAX_REF + 1), np.int32)),
                dict(hyp=np.zeros((6, _abi.LXO_EDIT_MAX_REF + 1), np.int32)), dict(ref=ref[:0])):
        kw = dict(hyp=hyp, ref=ref, hyp_lengths=None, ref_lengths=None)
        kw.update(bad)
        with pytest.raises(ValueError, match="sentence_bleu"):
            eng.sentence_bleu(**kw)


def _check_consensus(ids, id_end, best, risk, cost=None, weights=None):
    c_ref, r_ref, seqs = host_consensus(ids, id_end, weights)
    assert best.dtype == np.int32 and risk.dtype == np.float32 and risk.shape == ids.shape[::2]
    if cost is not None:
        assert cost.dtype == np.float32 and np.abs(cost - c_ref).max() <= BOUND and not cost[:, np.arange(ids.shape[2]), np.arange(ids.shape[2])].any()
    assert np.abs(risk - r_ref).max() <= RISK_BOUND
    assert best.tolist() == np.argmin(risk, axis=1).tolist()
    for b in range(len(best)):
        assert r_ref[b, best[b]] - r_ref[b].min() <= GAP
    return c_ref, seqs


def test_consensus_with_the_bleu_cost(lib):
    eng = _engine(lib)
    rng = np.random.default_rng(4)
    B, T, n = 3, 12, 5
    ids = rng.integers(0, 3, size=(B, T, n)).astype(np.int32)
    w = rng.uniform(0.5, 2.0, size=(B, n)).astype(np.float32)
    best, risk, cost = eng.consensus(ids, 2, return_dist=True, cost="bleu")
    _check_consensus(ids, 2, best, risk, cost)
    be, re_, de = eng.consensus(ids, 2, return_dist=True)
    assert de.dtype == np.int32 and (re_ != risk).any()                  # another cost
    # rows [B, n, T] seen as [B, T, n] and a slice of a longer buffer, read in place: the contiguous call's bytes
    view = torch.from_numpy(np.ascontiguousarray(ids.transpose(0, 2, 1))).permute(0, 2, 1)
    assert not view.is_contiguous()
    b2, r2, c2 = eng.consensus(view, 2, return_dist=True, cost="bleu")
    assert b2.tobytes() == best.tobytes() and r2.tobytes() == risk.tobytes() and c2.tobytes() == cost.tobytes()
    buf = torch.from_numpy(np.concatenate([ids, np.full((B, 3, n), 2, np.int32)], axis=1))
    b3, r3 = eng.consensus(buf[:, :T], 2, cost="bleu")
    assert b3.tobytes() == best.tobytes() and r3.tobytes() == risk.tobytes()
    bw, rw = eng.consensus(ids, 2, weights=w, cost="bleu")
    _check_consensus(ids, 2, bw, rw, weights=w)
    bn, rn, cn = eng.consensus(ids, None, return_dist=True, cost="bleu")
    _check_consensus(ids, None, bn, rn, cn)
    # the edges: no image, no token, one draw
    e = eng.consensus(ids[:0], 2, return_dist=True, cost="bleu")
    assert [x.shape for x in e] == [(0,), (0, n), (0, n, n)] and e[2].dtype == np.float32
    z = eng.consensus(ids[:, :0], 2, return_dist=True, cost="bleu")
    assert not z[0].any() and not z[1].any() and not z[2].any()
    o = eng.consensus(ids[:, :, :1], 2, cost="bleu")
    assert not o[0].any() and not o[1].any() and o[1].shape == (B, 1)


def test_sample_decode_consensus_cost(lib):
    eng, img = _engine(lib), _images()
    ids = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, **SAMPLING)
    out = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, return_consensus=True, consensus_cost="bleu", **SAMPLING)
    assert len(out) == 3 and np.array_equal(out[0], ids)
    c_ref, seqs = _check_consensus(ids, END, out[1], out[2])
    off = ~np.eye(N, dtype=bool)
    assert (c_ref[:, off] == 0).any() and (c_ref > 0).any()         # somewhere two draws of an image are equal, somewhere two differ
    b2, r2 = eng.consensus(ids, END, cost="bleu")
    assert b2.tobytes() == out[1].tobytes() and r2.tobytes() == out[2].tobytes()


def test_mrt_sample_step_bleu_against_the_host_costs_and_the_oracle(lib):
    counted = Counting(lib)
    eng, img = _engine(counted), _images()
    ref, rl = pad_batch_formulas(REFS, PAD, END)
    ids = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, **SAMPLING)
    f, ln, sizes, edit_costs = host_candidates(ids, REFS, END, PAD, True)
    rows_ref = np.repeat(np.arange(len(sizes)), sizes)
    costs64 = np.array([sentence_bleu_cost([int(x) for x in f[r, :ln[r] - 1]], REFS[rows_ref[r]]) for r in range(len(ln))])
    costs = costs64.astype(np.float32)                              # rounded once, where f32 is needed
    P = {k: torch.from_numpy(v.copy()) for k, v in eng.get_params().items()}
    risk_ref, G, q_ref = mrt_oracle.mrt_grads(P, img, f, ln, sizes, costs, ALPHA)
    before = eng.params.clone()
    risk, info = eng.mrt_sample_step(img, ref, rl, END, PAD, 0.0, ALPHA, n=N, max_iter=MAX_ITER, cost="bleu", **SAMPLING)
    assert torch.equal(eng.params, before)
    assert counted.calls.count("lxo_mrt_candidates_cost") == 1 and "lxo_mrt_candidates" not in counted.calls and "lxo_edit_distance" not in counted.calls
    assert info["group_sizes"].tolist() == sizes.tolist() and info["cand_lengths"].tolist() == ln.tolist()
    for r in range(len(ln)):
        assert info["cand"][r, :ln[r]].tolist() == f[r, :ln[r]].tolist() and (info["cand"][r, ln[r]:] == PAD).all(), r
    err = np.abs(info["cost"].astype(np.float64) - costs64).max()
    print("largest |device cost - host sentence_bleu_cost| = %.3g" % err)
    assert err <= BOUND and (info["cost"] != edit_costs).any()
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert all(info["cost"][o].tobytes() == np.float32(0).tobytes() for o in off[:-1])               # the reference's own row
    cs = mrt_oracle.cosines(eng.grad_dict(), G)
    q = info["q"]
    print("risk %.7f oracle %.7f; q max err %.2e; lowest gradient cosines %s" % (risk, risk_ref, np.abs(q - q_ref).max(), cs[:3]))
    assert abs(risk - risk_ref) <= 1e-5 and np.abs(q - q_ref).max() <= 1e-5
    assert abs(risk - risk_ref) / abs(risk_ref) < LOSS_TOL
    for c, k in cs:
        assert c > MIN_COS, (k, c)


def test_defaults_run_the_calls_and_return_the_bytes_they_did(lib):
    """without the new keyword, and with "edit", no new entry point is called and the results are equal byte for byte"""
    counted = Counting(lib)
    eng, img = _engine(counted), _images()
    ref, rl = pad_batch_formulas(REFS, PAD, END)
    rng = np.random.default_rng(8)
    ids = rng.integers(0, 3, size=(2, 9, 4)).astype(np.int32)
    a, b = eng.consensus(ids, 2, return_dist=True), eng.consensus(ids, 2, return_dist=True, cost="edit")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[2].dtype == np.int32
    a = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, return_consensus=True, **SAMPLING)
    b = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, return_consensus=True, consensus_cost="edit", **SAMPLING)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    r1, i1 = eng.mrt_sample_step(img, ref, rl, END, PAD, 0.0, ALPHA, n=N, max_iter=MAX_ITER, **SAMPLING)
    g1 = {k: v.copy() for k, v in eng.grad_dict().items()}
    r2, i2 = eng.mrt_sample_step(img, ref, rl, END, PAD, 0.0, ALPHA, n=N, max_iter=MAX_ITER, cost="edit", **SAMPLING)
    assert r1 == r2 and all(i1[k].tobytes() == i2[k].tobytes() for k in i1)
    assert all(np.asarray(g1[k]).tobytes() == np.asarray(v).tobytes() for k, v in eng.grad_dict().items())
    assert "lxo_mrt_candidates" in counted.calls and "lxo_consensus" in counted.calls and not [c for c in counted.calls if c in NEW]
    eng.consensus(ids, 2, cost="bleu")
    assert counted.calls.count("lxo_consensus_bleu") == 1


def test_refusals_before_any_launch(lib, monkeypatch):
    eng, img = _engine(lib), _images()
    ref, rl = pad_batch_formulas(REFS, PAD, END)
    ids = np.zeros((2, 6, 3), np.int32)
    calls = []
    monkeypatch.setattr(eng, "_ck", lambda rc, what: calls.append(what))
    with pytest.raises(ValueError, match='cost must be "edit" or "bleu", got \'rouge\''):
        eng.consensus(ids, END, cost="rouge")
    with pytest.raises(ValueError, match="no normalisation"):
        eng.consensus(ids, END, normalize=False, cost="bleu")
    with pytest.raises(ValueError, match='cost must be "edit" or "bleu"'):
        eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, return_consensus=True, consensus_cost="rouge")
    with pytest.raises(ValueError, match="no normalisation"):
        eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, return_consensus=True, consensus_cost="bleu", consensus_normalize=False)
    with pytest.raises(ValueError, match='mrt_sample_step: cost must be "edit" or "bleu"'):
        eng.mrt_sample_step(img, ref, rl, END, PAD, 0.0, ALPHA, n=N, max_iter=MAX_ITER, cost="rouge")
    with pytest.raises(ValueError, match="max_iter"):
        eng.mrt_sample_step(img, ref, rl, END, PAD, 0.0, ALPHA, n=N, max_iter=_abi.LXO_EDIT_MAX_REF, cost="bleu")
    assert not calls and eng.ws is None and eng.adam_t == 0


# ------------------------------------------------------------------------------------------------------------------ the model --
def _model(tmp, lib):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    (tmp / "vocab.txt").write_text("\n".join(["a", "b", "c", "d", "e", "f", "g", "h"]) + "\n")          # + _UNK, _PAD, _END: 11 ids
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp / "vocab.txt")}))
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": MAX_ITER - 1, "decoding": "greedy"})
    return Img2SeqModel(cfg, str(tmp) + "/out/", vocab, lib=lib)


@pytest.fixture(scope="module")
def model(tmp_path_factory, lib):
    m = _model(tmp_path_factory.mktemp("sentence_bleu"), lib)
    m.build_pred()
    m.engine = _engine(lib)
    return m


def test_mrt_batch_with_the_bleu_cost_on_both_paths(model, monkeypatch):
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    refs = ["a b c", "d e"]
    kw = dict(n=2, alpha=ALPHA, **SAMPLING2)
    host = model.mrt_batch(imgs, refs, 0.0, cost="bleu", **kw)
    dev = model.mrt_batch(imgs, refs, 0.0, on_device=True, cost="bleu", **kw)
    texts = lambda out: [[c["text"] for c in g] for g in out["candidates"]]
    assert texts(dev) == texts(host) and [len(g) for g in dev["candidates"]] == [2, 3]
    ch, cd = [np.array([c["cost"] for g in out["candidates"] for c in g]) for out in (host, dev)]
    tok = {t: i for i, t in enumerate(model._vocab.id_to_tok[i] for i in range(V))}
    want = [sentence_bleu_cost([tok[t] for t in c["text"].split()], [tok[t] for t in refs[b].split()]) for b, g in enumerate(host["candidates"]) for c in g]
    assert ch.tolist() == want and np.abs(cd - ch).max() <= BOUND
    assert dev["candidates"][0][0]["text"] == "a b c" and dev["candidates"][0][0]["cost"] == 0.0 and host["candidates"][0][0]["cost"] == 0.0
    qd, qh = [c["q"] for g in dev["candidates"] for c in g], [c["q"] for g in host["candidates"] for c in g]
    assert np.abs(np.array(qd) - np.array(qh)).max() <= 1e-5 and abs(dev["risk"] - host["risk"]) <= 1e-5
    # the default and "edit" hand the engine what they handed it (the steps themselves are tests/test_engine_mrt_device_sim.py's): the same arrays
    # into mrt_step, edit-distance costs among them, and no cost keyword into mrt_sample_step
    seen = []

    class Stop(Exception):
        pass

    def grab(*a, **k):
        seen.append((a, k))
        raise Stop()
    monkeypatch.setattr(model.engine, "mrt_step", grab)
    monkeypatch.setattr(model.engine, "mrt_sample_step", grab)
    for on_device in (False, True):
        for more in ({}, {"cost": "edit"}):
            with pytest.raises(Stop):
                model.mrt_batch(imgs, refs, 0.0, on_device=on_device, **dict(kw, **more))
    (a0, k0), (a1, k1), (a2, k2), (a3, k3) = seen
    assert k0 == k1 and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a0[1:], a1[1:]))
    assert a0[4].dtype == np.float32 and a0[4].tobytes() != ch.astype(np.float32).tobytes() and a0[3].tolist() == [2, 3]
    assert k2 == k3 and "cost" not in k2 and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a2[1:], a3[1:]))
    with pytest.raises(ValueError, match='mrt_batch: cost must be "edit" or "bleu"'):
        model.mrt_batch(imgs, refs, 0.0, cost="rouge", **kw)


def test_sample_batch_consensus_cost(model):
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    plain = model.sample_batch(imgs, N, consensus=True, **SAMPLING)
    assert model.sample_batch(imgs, N, consensus=True, consensus_cost="edit", **SAMPLING) == plain
    res = model.sample_batch(imgs, N, consensus=True, consensus_cost="bleu", **SAMPLING)
    ids, best, risk = model.engine.sample_decode(model._get_feed_dict(imgs, dropout=1)["img"], END, n=N, max_iter=MAX_ITER, return_consensus=True,
                                                 consensus_cost="bleu", **SAMPLING)
    _, r_ref, seqs = host_consensus(ids, END)
    for b, (r, p) in enumerate(zip(res, plain)):
        assert [{k: v for k, v in h.items() if k != "risk"} for h in r["hypotheses"]] == [{k: v for k, v in h.items() if k != "risk"} for h in p["hypotheses"]]
        texts = [" ".join(model._vocab.id_to_tok[i] for i in s) for s in seqs[b]]
        assert r["hypotheses"][r["consensus"]]["text"] == texts[best[b]] and r["expected_cost"] == float(risk[b, best[b]])
        for h in r["hypotheses"]:
            assert abs(h["risk"] - r_ref[b, texts.index(h["text"])]) <= RISK_BOUND
    assert any(h["risk"] != q["risk"] for r, p in zip(res, plain) for h, q in zip(r["hypotheses"], p["hypotheses"]))
    with pytest.raises(ValueError, match='consensus_cost must be "edit" or "bleu"'):
        model.sample_batch(imgs, N, consensus=True, consensus_cost="rouge", **SAMPLING)


def test_config_key_names_the_cost(model, monkeypatch, tmp_path, lib):
    from latex_ocr_amd.model.utils.general import Config
    assert "cost" in model.MRT_KEYS
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    seen = []
    monkeypatch.setattr(model, "mrt_batch", lambda *a, **k: seen.append(k) or {"risk": 0.0})
    monkeypatch.setattr(model, "evaluate", lambda *a, **k: {"perplexity": 1.0})
    sched = type("Sched", (), {"lr": 1e-3, "update": lambda self, **k: None})()
    train = [(imgs[0], "a b"), (imgs[1], "c")]
    model._run_train(Config({"batch_size": 2, "mrt": {"n": 2, "on_device": True, "cost": "bleu"}}), train, [], 0, sched)
    assert len(seen) == 1 and seen[0]["cost"] == "bleu" and seen[0]["on_device"] is True
    # a cost that is neither string is refused when the model is built, before an engine exists
    fresh = _model(tmp_path, lib)
    for bad in (3, "rouge", None):
        with pytest.raises(ValueError, match='"mrt": "cost" must be "edit" or "bleu"'):
            fresh.build_train(Config({"lr_method": "adam", "mrt": {"cost": bad}}))
    assert getattr(fresh, "engine", None) is None


def test_predict_refuses_consensus_cost_without_consensus(capsys):
    import predict
    for argv in (["--consensus-cost", "bleu", "formula.png"], ["--sample", "3", "--consensus-cost", "bleu", "formula.png"],
                 ["--consensus-cost", "edit", "formula.png"]):
        with pytest.raises(SystemExit) as e:
            predict.main(argv)
        assert e.value.code == 2 and "--consensus-cost" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        predict.main(["--sample", "3", "--consensus", "--consensus-cost", "rouge", "formula.png"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
