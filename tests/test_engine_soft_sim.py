"""CPU (hipsim): Engine.loss(soft_targets=, soft_weight=) + backward and Engine.train_step(soft_targets=) against autograd through
oracle/ref_model.py with the target q of tests/soft_loss_ref.py (loss sum w (-sum_j q_j log_softmax_j) / norm); the Alternatives form of the
argument; every ValueError before a launch; Img2SeqModel.distill_batch with one and two teachers against the step with hand-built slots; and
the training config's "distill" key.  The shapes are tests/test_engine_smoothed_sim.py's."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Alternatives, Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
from simlib import SIM_SO, build_sim
import mrt_oracle
from soft_loss_ref import soft_grads

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, T, H, W = 11, 5, 32, 48
LOSS_TOL, MIN_COS = 2e-5, 0.9999        # tests/test_engine_weighted_sim.py's bars
EPS, LAM, K = 0.1, 0.5, 3


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


def _slots(B, ln, seed, k=K):
    """k distinct tokens per position with masses adding up to 0.8; one live position without a teacher, one with two slots on one token, and
    garbage behind the lengths (never read)"""
    rng = np.random.default_rng(seed)
    ids = np.stack([np.stack([rng.choice(V, size=k, replace=False) for _ in range(T)]) for _ in range(B)]).astype(np.int32)
    p = rng.dirichlet(np.ones(k), size=(B, T)).astype(np.float32) * np.float32(0.8)
    ids[0, 0, :] = -1
    if k > 1:
        ids[0, 1, 1] = ids[0, 1, 0]
    dead = np.arange(T)[None, :] >= np.asarray(ln)[:, None]
    ids[dead] = 1 << 20
    p[dead] = np.nan
    return ids, p


def _oracle_params(eng):
    return {k: torch.from_numpy(v.copy()) for k, v in eng.get_params().items()}


def _report(what, loss, ref, cs):
    err = abs(loss - ref) / abs(ref)
    print("%s: loss %.7f oracle %.7f rel %.2e; lowest gradient cosines %s" % (what, loss, ref, err, ", ".join("%.7f %s" % (c, k.split("/", 1)[-1]) for c, k in cs[:3])))
    assert err < LOSS_TOL, (loss, ref)
    for c, k in cs:
        assert c > MIN_COS, (k, c)


def test_soft_loss_and_backward_against_autograd(lib):
    eng = _engine(lib)
    img, f = _batch(3, seed=5)
    ln = np.array([5, 2, 4], np.int32)
    ntok = float(ln.sum())
    ids, p = _slots(3, ln, seed=1)
    ones = np.ones((3, T), np.float32)
    # soft targets alone (no smoothing), normalised by the token count
    eng.forward(img, f)
    stats = eng.loss(ln, 1.0 / ntok, soft_targets=(ids, p), soft_weight=LAM).numpy().copy()
    eng.backward()
    ref, G, ce = soft_grads(_oracle_params(eng), img, f, ln, ones, ntok, 0.0, LAM, ids, p)
    assert stats.shape == (4,) and stats[1] == ntok and stats[2] == ntok
    assert abs(float(stats[3]) / ntok - ce) <= LOSS_TOL * ce
    _report("soft_targets", float(stats[0]) / ntok, ref, mrt_oracle.cosines(eng.grad_dict(), G))
    # with smoothing, mixed-sign token weights, row weights and the caller's norm
    rng = np.random.default_rng(1)
    w = rng.uniform(-2.0, 2.0, size=(3, T)).astype(np.float32)
    w[0, 1] = 0.0
    wr = np.array([1.5, -0.5, 1.0], np.float32)
    norm = 7.0
    eng.forward(img, f)
    s2 = eng.loss(ln, 1.0 / norm, weights=w, row_weights=wr, label_smoothing=EPS, soft_targets=(ids, p), soft_weight=LAM).numpy().copy()
    eng.backward()
    ref2, G2, _ = soft_grads(_oracle_params(eng), img, f, ln, w * wr[:, None], norm, EPS, LAM, ids, p)
    assert s2[1] == ntok and s2[3].tobytes() == stats[3].tobytes()
    _report("soft_targets x label_smoothing x weights", float(s2[0]) / norm, ref2, mrt_oracle.cosines(eng.grad_dict(), G2))
    # the normaliser read from the device, as data parallelism passes it (the logits of the forward above are still in the workspace)
    s3 = eng.loss(ln, ntok_dev=torch.tensor([norm], dtype=torch.float32), weights=w, row_weights=wr, label_smoothing=EPS, soft_targets=(ids, p),
                  soft_weight=LAM).numpy().copy()
    assert np.abs(s3 - s2).max() <= 1e-6 * np.abs(s2).max()
    # device tensors are taken as they are
    s4 = eng.loss(ln, 1.0 / norm, weights=w, row_weights=wr, label_smoothing=EPS,
                  soft_targets=(torch.from_numpy(np.where(ids > V, -1, ids)), torch.from_numpy(np.nan_to_num(p))), soft_weight=LAM).numpy().copy()
    assert s4.tobytes() == s2.tobytes()
    # without the argument: the calls the engine made before
    s0 = eng.loss(ln, 1.0 / ntok)
    assert s0.shape == (2,) and abs(float(s0[0]) - float(stats[3])) <= 1e-6 * abs(float(stats[3]))
    # soft_weight 0 is the smoothed loss bit for bit
    a = eng.loss(ln, 1.0 / ntok, label_smoothing=EPS).numpy().copy()
    da = eng.region("dlogits").clone()
    b = eng.loss(ln, 1.0 / ntok, label_smoothing=EPS, soft_targets=(ids, p), soft_weight=0.0).numpy().copy()
    assert a.tobytes() == b.tobytes() and torch.equal(da, eng.region("dlogits"))
    # None is the call without the argument, bit for bit
    c = eng.loss(ln, 1.0 / ntok, label_smoothing=EPS, soft_targets=None, soft_weight=0.7).numpy().copy()
    assert a.tobytes() == c.tobytes() and torch.equal(da, eng.region("dlogits"))


def test_train_step_returns_the_soft_loss_and_keeps_the_plain_ce(lib):
    img, f = _batch(3, seed=6)
    ln = np.array([3, 5, 1], np.int32)
    ids, p = _slots(3, ln, seed=2)
    eng = _engine(lib)
    P = _oracle_params(eng)
    ref, _, ce = soft_grads(P, img, f, ln, np.ones((3, T), np.float32), float(ln.sum()), EPS, LAM, ids, p)
    before = eng.params.clone()
    loss = eng.train_step(img, f, ln, 1e-3, label_smoothing=EPS, soft_targets=(ids, p), soft_weight=LAM)
    assert abs(loss - ref) / abs(ref) < LOSS_TOL, (loss, ref)
    assert abs(eng.last_ce - ce) / ce < LOSS_TOL and abs(loss - eng.last_ce) > 1e-3          # two different numbers
    assert not torch.equal(eng.params, before)
    # None is the step without the argument: nothing of the soft targets reaches loss()
    seen = []
    real = eng.loss
    eng.loss = lambda *a, **k: seen.append(k) or real(*a, **k)
    eng.train_step(img, f, ln, 1e-3, soft_targets=None, soft_weight=0.7)
    assert len(seen) == 1 and "soft_targets" not in seen[0] and "soft_weight" not in seen[0] and "label_smoothing" not in seen[0]


def test_alternatives_are_the_pair_of_ids_and_exp_logp(lib):
    img, f = _batch(3, seed=6)
    ln = np.array([3, 5, 1], np.int32)
    teacher = _engine(lib, seed=8)
    alt = teacher.score(img, f, ln, alternatives=K)[-1]
    assert isinstance(alt, Alternatives) and alt.ids.shape == (3, T, K)
    # the device form of the scoring call holds the same ids and log-probs (the logits of score()'s forward are still in the workspace)
    di, dl = teacher.score_alternatives_dev(img, f, ln, K)
    assert np.array_equal(di.numpy(), alt.ids) and np.array_equal(dl.numpy(), alt.logp)
    pair = (alt.ids, torch.exp(torch.from_numpy(alt.logp)).numpy())
    eng = _engine(lib)
    eng.forward(img, f)

    def run(**kw):
        st = eng.loss(ln, 1.0 / float(ln.sum()), soft_weight=LAM, **kw).numpy().copy()
        return st.tobytes(), eng.region("dlogits").clone()
    a, b, c = run(soft_targets=alt), run(soft_targets=pair), run(soft_targets=(di, torch.exp(dl)))
    assert a[0] == b[0] == c[0] and torch.equal(a[1], b[1]) and torch.equal(a[1], c[1])
    # a log-prob of -inf is a mass of 0: the slot adds nothing
    lp = alt.logp.copy()
    lp[:, :, K - 1] = -np.inf
    cut = alt.ids.copy()
    cut[:, :, K - 1] = -1
    d, e = run(soft_targets=Alternatives(alt.ids, lp, alt.rank, alt.entropy)), run(soft_targets=(cut, pair[1]))
    assert d[0] == e[0] and torch.equal(d[1], e[1]) and d[0] != a[0]


def test_refusals_before_any_launch(lib):
    img, f = _batch(3, seed=5)
    ln = np.array([5, 2, 4], np.int32)
    ids, p = _slots(3, ln, seed=1)

    def masses(b, t, vals):
        q = p.copy()
        q[b, t, :len(vals)] = vals
        return q
    bad = [dict(soft_targets=(ids[:2], p[:2])),                                            # the batch
           dict(soft_targets=(ids[:, :4], p[:, :4])),                                      # the steps
           dict(soft_targets=(ids, p[:, :, :2])),                                          # ids and masses disagree
           dict(soft_targets=(ids[:, :, 0], p[:, :, 0])),                                  # no slot axis
           dict(soft_targets=(np.zeros((3, T, 17), np.int32), np.zeros((3, T, 17), np.float32))),          # k = 17
           dict(soft_targets=(np.zeros((3, T, 0), np.int32), np.zeros((3, T, 0), np.float32))),            # k = 0
           dict(soft_targets=(ids, masses(1, 1, [-0.1]))), dict(soft_targets=(ids, masses(1, 1, [np.nan]))),
           dict(soft_targets=(ids, masses(1, 1, [np.inf]))), dict(soft_targets=(ids, masses(2, 3, [0.5, 0.5, 0.0011]))),
           dict(soft_targets=(ids.astype(np.float32), p)), dict(soft_targets=ids), dict(soft_targets=(ids, p, p)),
           dict(soft_targets=(ids, p), soft_weight=-0.1), dict(soft_targets=(ids, p), soft_weight=1.5), dict(soft_targets=(ids, p), soft_weight=float("nan")),
           dict(soft_targets=(ids, p), soft_weight=float("inf")), dict(soft_targets=(ids, p), soft_weight="a"), dict(soft_targets=(ids, p), soft_weight=None)]
    eng = _engine(lib)
    for kw in bad:
        with pytest.raises(ValueError):
            eng.train_step(img, f, ln, 1e-3, **kw)
    assert not hasattr(eng, "_img") and eng.ws is None and eng.adam_t == 0
    eng.forward(img, f)
    before = eng.ws.clone()
    for kw in bad:
        with pytest.raises(ValueError):
            eng.loss(ln, 1.0, **kw)
    assert torch.equal(eng.ws, before)
    # inside: masses adding up to 1 + 1e-3 exactly at most, a bad mass behind a length or in a slot that does not count, the ends of soft_weight
    ok = masses(2, 3, [0.5, 0.5, 0.0009])
    ok[1, 4, :] = np.nan                                               # t = 4 >= ln[1] = 2
    skip = ids.copy()
    skip[2, 0, 0] = -1
    ok[2, 0, 0] = -5.0
    for lam in (0.0, 1.0):
        eng.loss(ln, 1.0, soft_targets=(skip, ok), soft_weight=lam)
    # the minimum-risk steps do not take the argument
    with pytest.raises(TypeError):
        eng.mrt_step(img[:2], np.zeros((5, T), np.int32), np.full(5, 3, np.int32), np.array([3, 2]), np.zeros(5, np.float32), 1e-3, 1.0, soft_targets=(ids, p))


# ------------------------------------------------------------------------------------------------------------------ the model --
def _model(tmp, lib, seed=0, words=8, name="out"):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    tmp.mkdir(parents=True, exist_ok=True)
    (tmp / "vocab.txt").write_text("\n".join("abcdefghijkl"[:words]) + "\n")          # + _UNK, _PAD, _END: 11 ids at 8 words
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp / "vocab.txt")}))
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": 6, "decoding": "greedy", "seed": seed})
    return Img2SeqModel(cfg, str(tmp) + "/" + name + "/", vocab, lib=lib)


def _train_cfg(**kw):
    from latex_ocr_amd.model.utils.general import Config
    return Config(dict({"lr_method": "adam", "batch_size": 2, "prefetch_depth": 0}, **kw))


def test_distill_batch_is_the_step_with_the_teachers_slots(tmp_path, lib):
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    forms = [[0, 1, 2], [3, 4]]
    teachers = [_model(tmp_path / ("t%d" % i), lib, seed=20 + i) for i in range(2)]
    for t in teachers:
        t.build_pred()
    a, b = _model(tmp_path / "a", lib), _model(tmp_path / "b", lib)
    for m in (a, b):
        m.build_train(_train_cfg(label_smoothing=EPS))
    assert torch.equal(a.engine.params, b.engine.params) and not torch.equal(a.engine.params, teachers[0].engine.params)
    fd = b._get_feed_dict(imgs, formula=forms)
    img, f, ln = fd["img"], fd["formula"], fd["formula_length"]
    alts = [t.engine.score(img, f, ln, alternatives=K)[-1] for t in teachers]
    # by hand: every teacher's host Alternatives, side by side, the probabilities divided by the number of teachers
    ids = np.concatenate([x.ids for x in alts], axis=2)
    p = torch.cat([torch.exp(torch.from_numpy(x.logp)) / 2.0 for x in alts], dim=2).numpy()
    assert ids.shape == (2, f.shape[1], K * 2)
    # one teacher (not in a list) and two: the step is train_step's with those slots
    la = a.distill_batch(imgs, forms, 1e-3, teachers, k=K, weight=0.75)
    lb = b.engine.train_step(img, f, ln, 1e-3, clip=b._clip, label_smoothing=EPS, soft_targets=(ids, p), soft_weight=0.75)
    assert la == lb and torch.equal(a.engine.params, b.engine.params) and a.engine.adam_t == 1
    seen = []
    a.engine.train_step = lambda *args, **k: seen.append(k) or 1.5
    assert a.distill_batch(imgs, forms, 1e-3, teachers[0], k=K) == 1.5
    ti, tp = seen[0]["soft_targets"]
    assert np.array_equal(ti.numpy(), alts[0].ids) and tp.numpy().tobytes() == torch.exp(torch.from_numpy(alts[0].logp)).numpy().tobytes()
    assert seen[0]["soft_weight"] == 0.5 and seen[0]["label_smoothing"] == EPS
    # k * M above 16, and a teacher with another vocabulary
    with pytest.raises(ValueError, match="16"):
        a.distill_batch(imgs, forms, 1e-3, teachers * 9, k=1)
    other = _model(tmp_path / "o", lib, words=10)
    other.build_pred()
    with pytest.raises(ValueError, match="vocabulary"):
        a.distill_batch(imgs, forms, 1e-3, other, k=K)
    assert len(seen) == 1


def test_config_key(tmp_path, lib, monkeypatch):
    teacher = _model(tmp_path / "t", lib, seed=21)
    teacher.build_train(_train_cfg())
    teacher.save_session(0)
    tdir = str(tmp_path / "t") + "/out/"
    cfg = _train_cfg(label_smoothing=EPS, distill={"teacher": tdir, "k": K, "weight": 0.25})
    m = _model(tmp_path / "s", lib)
    m.build_train(cfg)
    assert len(m._distill["teacher"]) == 1 and torch.equal(m._distill["teacher"][0].engine.params, teacher.engine.params)
    assert not torch.equal(m.engine.params, teacher.engine.params)
    seen = []
    real = m.engine.train_step
    monkeypatch.setattr(m.engine, "train_step", lambda *a, **k: seen.append(k) or real(*a, **k))
    monkeypatch.setattr(m, "evaluate", lambda *a, **k: {"perplexity": 1.0})
    sched = type("Sched", (), {"lr": 1e-3, "update": lambda self, **k: None})()
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    train = [(imgs[0], [0, 1, 2]), (imgs[1], [3, 4])]
    m._run_train(cfg, train, [], 0, sched)
    assert len(seen) == 1 and seen[0]["soft_weight"] == 0.25 and seen[0]["label_smoothing"] == EPS and m.engine.adam_t == 1
    ids, p = seen[0]["soft_targets"]
    assert tuple(ids.shape) == (2, 4, K) and tuple(p.shape) == (2, 4, K)
    # a list of two directories; without the key the step is called as ever
    m3 = _model(tmp_path / "s3", lib)
    m3.build_train(_train_cfg(distill={"teacher": [tdir, tdir], "k": 2}))
    assert len(m3._distill["teacher"]) == 2 and m3._distill["weight"] == 0.5
    m4 = _model(tmp_path / "s4", lib)
    m4.build_train(_train_cfg())
    seen4 = []
    monkeypatch.setattr(m4.engine, "train_step", lambda *a, **k: seen4.append(k) or 1.25)
    monkeypatch.setattr(m4, "evaluate", lambda *a, **k: {"perplexity": 1.0})
    m4._run_train(_train_cfg(), train, [], 0, sched)
    assert len(seen4) == 1 and "soft_targets" not in seen4[0] and "soft_weight" not in seen4[0]


def test_config_refusals(tmp_path, lib):
    teacher = _model(tmp_path / "t", lib, seed=21)
    teacher.build_train(_train_cfg())
    teacher.save_session(0)
    tdir = str(tmp_path / "t") + "/out/"
    m = _model(tmp_path / "s", lib)
    with pytest.raises(ValueError, match="(?s)distill.*mrt|mrt.*distill"):
        m.build_train(_train_cfg(distill={"teacher": tdir}, mrt={"n": 2}))
    for bad in ({"teacher": tdir, "k": 17}, {"teacher": [tdir] * 4, "k": 5}, {"teacher": tdir, "k": 0}, {"teacher": tdir, "weight": 1.5},
                {"teacher": tdir, "weight": "x"}, {"teacher": []}, {"k": 3}, {"teacher": tdir, "temperature": 2.0}):
        with pytest.raises(ValueError, match="distill"):
            m.build_train(_train_cfg(distill=bad))
    with pytest.raises(IOError):
        m.build_train(_train_cfg(distill={"teacher": str(tmp_path / "nowhere")}))
    # a teacher made for another vocabulary
    big = _model(tmp_path / "big", lib, words=10)
    with pytest.raises(ValueError, match="vocabulary"):
        big.build_train(_train_cfg(distill={"teacher": tdir}))
