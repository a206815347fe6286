"""CPU (hipsim): Engine.loss(label_smoothing=) + backward and Engine.train_step(label_smoothing=) against autograd through oracle/ref_model.py with
F.cross_entropy(..., label_smoothing=, reduction="none"), masked, weighted and divided by the norm; Engine.last_ce; every ValueError before a launch;
and the training config's "label_smoothing" key through Img2SeqModel.  The shapes are tests/test_engine_weighted_sim.py's."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
from simlib import SIM_SO, build_sim
import mrt_oracle
from smoothed_loss_ref import smoothed_grads

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, T, H, W = 11, 5, 32, 48
LOSS_TOL, MIN_COS = 2e-5, 0.9999        # tests/test_engine_weighted_sim.py's bars
EPS = 0.1


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


def _engine(lib, seed=3):
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=seed, lib=lib)


def _batch(B, seed):
    imgs, _ = synthetic.make_set(B, H, W, V, 2, 4, seed=seed)
    rng = np.random.default_rng(seed)
    f = rng.integers(0, V, size=(B, T)).astype(np.int32)
    return pad_batch_images(imgs), f


def _oracle_params(eng):
    return {k: torch.from_numpy(v.copy()) for k, v in eng.get_params().items()}


def _report(what, loss, ref, cs):
    err = abs(loss - ref) / abs(ref)
    print("%s: loss %.7f oracle %.7f rel %.2e; lowest gradient cosines %s" % (what, loss, ref, err, ", ".join("%.7f %s" % (c, k.split("/", 1)[-1]) for c, k in cs[:3])))
    assert err < LOSS_TOL, (loss, ref)
    for c, k in cs:
        assert c > MIN_COS, (k, c)


def test_smoothed_loss_and_backward_against_autograd(lib):
    eng = _engine(lib)
    img, f = _batch(3, seed=5)
    ln = np.array([5, 2, 4], np.int32)
    ntok = float(ln.sum())
    # smoothing alone, normalised by the token count
    eng.forward(img, f)
    stats = eng.loss(ln, 1.0 / ntok, label_smoothing=EPS).numpy().copy()
    eng.backward()
    ref, G, ce = smoothed_grads(_oracle_params(eng), img, f, ln, np.ones((3, T), np.float32), ntok, EPS)
    assert stats.shape == (4,) and stats[1] == ntok and stats[2] == ntok
    assert abs(float(stats[3]) / ntok - ce) <= LOSS_TOL * ce
    _report("label_smoothing", float(stats[0]) / ntok, ref, mrt_oracle.cosines(eng.grad_dict(), G))
    # with mixed-sign token weights and the caller's norm
    rng = np.random.default_rng(1)
    w = rng.uniform(-2.0, 2.0, size=(3, T)).astype(np.float32)
    w[0, 1] = 0.0
    norm = 7.0
    eng.forward(img, f)
    s2 = eng.loss(ln, 1.0 / norm, weights=w, label_smoothing=EPS).numpy().copy()
    eng.backward()
    ref2, G2, _ = smoothed_grads(_oracle_params(eng), img, f, ln, w, norm, EPS)
    assert s2[1] == ntok and s2[3].tobytes() == stats[3].tobytes()
    _report("label_smoothing x weights", float(s2[0]) / norm, ref2, mrt_oracle.cosines(eng.grad_dict(), G2))
    # the normaliser read from the device, as data parallelism passes it (the logits of the forward above are still in the workspace)
    s3 = eng.loss(ln, ntok_dev=torch.tensor([norm], dtype=torch.float32), weights=w, label_smoothing=EPS).numpy().copy()
    assert np.abs(s3 - s2).max() <= 1e-6 * np.abs(s2).max()
    # 0.0: the two-statistics call it was
    s0 = eng.loss(ln, 1.0 / ntok, label_smoothing=0.0)
    assert s0.shape == (2,) and abs(float(s0[0]) - float(stats[3])) <= 1e-6 * abs(float(stats[3]))


def test_train_step_returns_the_smoothed_loss_and_keeps_the_plain_ce(lib):
    img, f = _batch(3, seed=6)
    ln = np.array([3, 5, 1], np.int32)
    eng = _engine(lib)
    P = _oracle_params(eng)
    ref, _, ce = smoothed_grads(P, img, f, ln, np.ones((3, T), np.float32), float(ln.sum()), EPS)
    assert eng.last_ce is None
    before = eng.params.clone()
    loss = eng.train_step(img, f, ln, 1e-3, label_smoothing=EPS)
    assert abs(loss - ref) / abs(ref) < LOSS_TOL, (loss, ref)
    assert abs(eng.last_ce - ce) / ce < LOSS_TOL and abs(loss - eng.last_ce) > 1e-3          # two different numbers
    assert not torch.equal(eng.params, before)
    # 0.0 is the call without the argument, bit for bit: the loss, the plain CE and the updated parameters
    a, b = _engine(lib), _engine(lib)
    la = a.train_step(img, f, ln, 1e-3)
    lb = b.train_step(img, f, ln, 1e-3, label_smoothing=0.0)
    assert la == lb and a.last_ce == b.last_ce == la and torch.equal(a.params, b.params)
    assert abs(la - ce) / ce < LOSS_TOL


def test_refusals_before_any_launch(lib):
    img, f = _batch(3, seed=5)
    ln = np.array([5, 2, 4], np.int32)
    bad = [1.0, 1.5, -0.1, float("nan"), float("inf"), float("-inf"), "a", None, 1.0 - 1e-9]        # (the last: 1.0f once it is an f32)
    eng = _engine(lib)
    for eps in bad:
        with pytest.raises(ValueError):
            eng.train_step(img, f, ln, 1e-3, label_smoothing=eps)
    assert not hasattr(eng, "_img") and eng.ws is None and eng.adam_t == 0
    eng.forward(img, f)
    before = eng.ws.clone()
    for eps in bad:
        with pytest.raises(ValueError):
            eng.loss(ln, 1.0, label_smoothing=eps)
    assert torch.equal(eng.ws, before)
    # the minimum-risk steps do not take the argument
    with pytest.raises(TypeError):
        eng.mrt_step(img[:2], np.zeros((5, T), np.int32), np.full(5, 3, np.int32), np.array([3, 2]), np.zeros(5, np.float32), 1e-3, 1.0, label_smoothing=EPS)
    with pytest.raises(TypeError):
        eng.mrt_sample_step(img[:2], f[:2], ln[:2], V - 1, V - 2, 1e-3, 1.0, label_smoothing=EPS)


# ------------------------------------------------------------------------------------------------------------------ the model --
def _model(tmp, lib):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    (tmp / "vocab.txt").write_text("\n".join(["a", "b", "c", "d", "e", "f", "g", "h"]) + "\n")          # + _UNK, _PAD, _END: 11 ids
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp / "vocab.txt")}))
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": 6, "decoding": "greedy"})
    return Img2SeqModel(cfg, str(tmp) + "/out/", vocab, lib=lib)


def test_config_key_reaches_the_step(tmp_path, lib, monkeypatch):
    from latex_ocr_amd.model.utils.general import Config
    m = _model(tmp_path, lib)
    train_cfg = Config({"lr_method": "adam", "batch_size": 2, "prefetch_depth": 0, "label_smoothing": EPS})
    m.build_train(train_cfg)
    seen, logged = [], []
    real = m.engine.train_step
    monkeypatch.setattr(m.engine, "train_step", lambda *a, **k: seen.append(k) or real(*a, **k))
    monkeypatch.setattr(m, "evaluate", lambda *a, **k: {"perplexity": 1.0})
    import latex_ocr_amd.model.img2seq as mod

    class Bar(mod.Progbar):
        def update(self, i, values=(), **k):
            logged.append(dict(values))
            return super().update(i, values, **k)
    monkeypatch.setattr(mod, "Progbar", Bar)
    sched = type("Sched", (), {"lr": 1e-3, "update": lambda self, **k: None})()
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    train = [(imgs[0], [0, 1, 2]), (imgs[1], [3, 4])]
    m._run_train(train_cfg, train, [], 0, sched)
    assert len(seen) == 1 and seen[0]["label_smoothing"] == EPS and m.engine.adam_t == 1
    # the smoothed loss is logged; the perplexity is the plain cross-entropy's
    assert logged[0]["perplexity"] == np.exp(m.engine.last_ce) and abs(logged[0]["loss"] - m.engine.last_ce) > 1e-3
    # without the key the step is called as ever
    m2 = _model(tmp_path, lib)
    plain_cfg = Config({"lr_method": "adam", "batch_size": 2, "prefetch_depth": 0})
    m2.build_train(plain_cfg)
    seen2 = []
    monkeypatch.setattr(m2.engine, "train_step", lambda *a, **k: seen2.append(k) or 1.25)
    monkeypatch.setattr(m2, "evaluate", lambda *a, **k: {"perplexity": 1.0})
    m2._run_train(plain_cfg, train, [], 0, sched)
    assert len(seen2) == 1 and "label_smoothing" not in seen2[0]
    assert logged[1]["perplexity"] == np.exp(logged[1]["loss"])


def test_config_refusals(tmp_path, lib):
    from latex_ocr_amd.model.utils.general import Config
    m = _model(tmp_path, lib)
    with pytest.raises(ValueError, match="(?s)label_smoothing.*mrt|mrt.*label_smoothing"):
        m.build_train(Config({"lr_method": "adam", "batch_size": 2, "label_smoothing": EPS, "mrt": {"n": 2}}))
    for eps in (1.0, -0.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="label_smoothing"):
            m.build_train(Config({"lr_method": "adam", "batch_size": 2, "label_smoothing": eps}))
