"""CPU (hipsim): Engine.mrt_sample_step -- the sampled decode, the candidate kernels and the minimum-risk step without a host visit in between --
against the host path (Engine.sample_decode + the candidate loop of Img2SeqModel.mrt_batch, tests/edit_distance_ref.py: host_candidates) at the same
seed, exactly, and against autograd of the true risk on those candidates (tests/mrt_oracle.py) at tests/test_engine_weighted_sim.py's bars.
Img2SeqModel.mrt_batch(on_device=True) against the default, the config key, and Engine.edit_distance's surface."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.evaluation.text import levenshtein
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import pad_batch_formulas
from simlib import SIM_SO, build_sim
from edit_distance_ref import check_candidates, host_candidates, run_candidates
import mrt_oracle

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, H, W = 11, 32, 48
END, PAD = 10, 9
N, ALPHA, MAX_ITER = 3, 0.7, 4
# found on the CPU: at this seed, temperature and top_k the host path keeps 3 and 4 candidates for the two images (a draw of image 0 repeats), of
# 2 to 5 tokens; with n = 2 draws (the model tests) seed 4 at top_k 2 keeps 2 and 3
SAMPLING = dict(temperature=0.5, top_k=3, seed=5)
SAMPLING2 = dict(temperature=0.5, top_k=2, seed=4)
REFS = [[0, 1, 2], [3, 4]]
LOSS_TOL, MIN_COS = 2e-5, 0.9999                                   # tests/test_engine_weighted_sim.py's bars


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


def _engine(lib):
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=MAX_ITER + 1)


def _images():
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    return pad_batch_images(imgs)


def _same_rows(info, f, ln, sizes, costs):
    assert info["group_sizes"].tolist() == sizes.tolist() and info["cand_lengths"].tolist() == ln.tolist()
    assert info["cost"].tobytes() == costs.tobytes()
    assert info["cand"].shape[0] == len(ln)
    for r in range(len(ln)):
        assert info["cand"][r, :ln[r]].tolist() == f[r, :ln[r]].tolist() and (info["cand"][r, ln[r]:] == PAD).all(), r


def test_mrt_sample_step_against_the_host_path_and_the_oracle(lib):
    eng, img = _engine(lib), _images()
    ref, rl = pad_batch_formulas(REFS, PAD, END)
    ids = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, **SAMPLING)
    f, ln, sizes, costs = host_candidates(ids, REFS, END, PAD, True)
    assert (sizes < N + 1).any() and (sizes > 1).any(), sizes       # duplicates were dropped somewhere, and somewhere a draw stayed
    P = {k: torch.from_numpy(v.copy()) for k, v in eng.get_params().items()}
    risk_ref, G, q_ref = mrt_oracle.mrt_grads(P, img, f, ln, sizes, costs, ALPHA)
    before = eng.params.clone()
    risk, info = eng.mrt_sample_step(img, ref, rl, END, PAD, 0.0, ALPHA, n=N, max_iter=MAX_ITER, **SAMPLING)
    assert torch.equal(eng.params, before)                          # lr 0
    _same_rows(info, f, ln, sizes, costs)
    q = info["q"]
    cs = mrt_oracle.cosines(eng.grad_dict(), G)
    print("risk %.7f oracle %.7f; q max err %.2e; lowest gradient cosines %s" % (risk, risk_ref, np.abs(q - q_ref).max(), cs[:3]))
    assert abs(risk - risk_ref) <= 1e-5 and np.abs(q - q_ref).max() <= 1e-5
    assert abs(risk - risk_ref) / abs(risk_ref) < LOSS_TOL
    for c, k in cs:
        assert c > MIN_COS, (k, c)
    # per group: sum q = 1, sum w = 0; the dead rows (the dropped duplicates' and the chain batch's): w = q = 0
    Bp, live = int(eng.shape.B), int(sizes.sum())
    buf = eng._mrt_keep[-1]
    w_all, q_all = buf[Bp:2 * Bp].numpy(), buf[2 * Bp + 1:3 * Bp + 1].numpy()
    off = np.concatenate([[0], np.cumsum(sizes)])
    for lo, hi in zip(off[:-1], off[1:]):
        assert abs(float(q[lo:hi].sum(dtype=np.float64)) - 1.0) <= 1e-5
        assert abs(float(w_all[lo:hi].sum(dtype=np.float64))) <= 1e-6 * ALPHA
    assert live < 2 * (N + 1) <= Bp and not w_all[live:].any() and not q_all[live:].any()
    assert np.array_equal(q_all[:live], q)
    # without the reference: the candidate call alone on the same device ids (the step behind it is the one above)
    d_ids, _, _, _, steps, _ = eng._sample_device(img, END, N, SAMPLING["temperature"], SAMPLING["top_k"], 1.0, SAMPLING["seed"], MAX_ITER)
    out = run_candidates(lib, d_ids.numpy(), steps, REFS, END, PAD, 0)
    assert out[0] == 0 and steps == ids.shape[1]
    check_candidates(d_ids.numpy(), steps, REFS, END, PAD, 0, *out[1:])


def test_sample_decode_returns_what_it_returned(lib):
    """the device-side body factored out of sample_decode leaves its outputs as they were: ids, scores and maps of one call equal a direct
    lxo_sample_decode call's (tests/test_engine_sample_sim.py holds the full matrix; here the split itself)"""
    eng, img = _engine(lib), _images()
    ids, logp, logq = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, return_scores=True, **SAMPLING)
    d_ids, d_logp, d_logq, _, steps, geo = eng._sample_device(img, END, N, SAMPLING["temperature"], SAMPLING["top_k"], 1.0, SAMPLING["seed"], MAX_ITER, True)
    assert geo[:2] == (2, N) and ids.shape == (2, steps, N)
    assert np.array_equal(ids, d_ids[:, :steps].numpy()) and logp.tobytes() == d_logp[:, :steps].contiguous().numpy().tobytes()
    assert logq.tobytes() == d_logq[:, :steps].contiguous().numpy().tobytes()


def test_refusals_before_any_launch(lib):
    eng, img = _engine(lib), _images()
    ref, rl = pad_batch_formulas(REFS, PAD, END)
    ok = dict(n=N, max_iter=MAX_ITER)
    for args, kw in (((img, ref[:1], rl, END, PAD, 0.0, ALPHA), ok), ((img, ref, rl[:1], END, PAD, 0.0, ALPHA), ok), ((img, ref[0], rl, END, PAD, 0.0, ALPHA), ok),
                     ((img, ref, rl, V, PAD, 0.0, ALPHA), ok), ((img, ref, rl, END, -1, 0.0, ALPHA), ok), ((img, ref, rl, END, PAD, 0.0, 0.0), ok),
                     ((img, ref, rl, END, PAD, 0.0, float("nan")), ok), ((img, ref, rl, END, PAD, 0.0, ALPHA), dict(n=17, max_iter=MAX_ITER)),
                     ((img, ref, rl, END, PAD, 0.0, ALPHA), dict(n=N, max_iter=MAX_ITER, temperature=-1.0)),
                     ((img, np.zeros((2, _abi.LXO_EDIT_MAX_REF + 1), np.int32), rl, END, PAD, 0.0, ALPHA), ok)):
        with pytest.raises(ValueError):
            eng.mrt_sample_step(*args, **kw)
    assert not hasattr(eng, "_img") and eng.ws is None and eng.adam_t == 0


def test_edit_distance_takes_arrays_and_tensors(lib):
    eng = _engine(lib)
    rng = np.random.default_rng(3)
    hyp = rng.integers(0, 3, size=(6, 12)).astype(np.int32)
    ref = rng.integers(0, 3, size=(3, 9)).astype(np.int32)
    hl, rl = np.array([12, 0, 5, 7, 12, 1]), np.array([9, 4, 0])
    want = np.array([levenshtein(list(hyp[p, :hl[p]]), list(ref[p // 2, :rl[p // 2]])) for p in range(6)], np.int32)
    wcost = np.array([np.float32(want[p] / float(max(rl[p // 2], 1))) for p in range(6)], np.float32)
    d = eng.edit_distance(hyp, ref, hl, rl)
    assert d.dtype == np.int32 and np.array_equal(d, want)
    d2, c2 = eng.edit_distance(torch.from_numpy(hyp), torch.from_numpy(ref), torch.from_numpy(hl), torch.from_numpy(rl), return_cost=True)
    assert np.array_equal(d2, want) and c2.dtype == np.float32 and c2.tobytes() == wcost.tobytes()
    idx = np.array([2, 2, 0, 1, 0, 1])
    d3 = eng.edit_distance(hyp, ref, ref_index=idx)                  # whole rows, an explicit pairing
    assert np.array_equal(d3, [levenshtein(list(hyp[p]), list(ref[idx[p]])) for p in range(6)])
    f, fl = pad_batch_formulas([[0, 1, 1], [2]], PAD, END)            # pad_batch_formulas' layout, cut at END with and without the lengths
    assert eng.edit_distance(f, f, id_end=END).tolist() == [0, 0] and eng.edit_distance(f, f[::-1].copy(), fl, fl[::-1].copy(), id_end=END).tolist() == [3, 3]
    assert eng.edit_distance(f, f[::-1].copy()).tolist() == [4, 4]      # no cut: END and PAD are tokens
    assert eng.edit_distance(hyp[:0], ref).shape == (0,)
    assert eng.edit_distance(hyp[:, :0], ref).tolist() == [9] * 6 and eng.edit_distance(hyp, ref[:, :0]).tolist() == [12] * 6      # a side without a column
    for bad in (dict(hyp=hyp[0]), dict(ref=ref[0]), dict(hyp=hyp[:5]), dict(hyp_lengths=hl[:5]), dict(ref_lengths=rl[:2]), dict(ref_index=idx[:5]),
                dict(ref_index=np.array([0, 1, 2, 3, 0, 0])), dict(ref=np.zeros((3, _abi.LXO_EDIT_MAX_REF + 1), np.int32)), dict(ref=ref[:0])):
        kw = dict(hyp=hyp, ref=ref, hyp_lengths=None, ref_lengths=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.edit_distance(**kw)


# ------------------------------------------------------------------------------------------------------------------ the model --
@pytest.fixture(scope="module")
def model(tmp_path_factory, lib):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    tmp = tmp_path_factory.mktemp("mrt_device")
    (tmp / "vocab.txt").write_text("\n".join(["a", "b", "c", "d", "e", "f", "g", "h"]) + "\n")          # + _UNK, _PAD, _END: 11 ids
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp / "vocab.txt")}))
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": MAX_ITER - 1, "decoding": "greedy"})
    m = Img2SeqModel(cfg, str(tmp) + "/out/", vocab, lib=lib)
    m.build_pred()
    m.engine = _engine(lib)
    return m


def test_mrt_batch_on_device_equals_the_host_path(model):
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    refs = ["a b c", "d e"]
    kw = dict(n=2, alpha=ALPHA, **SAMPLING2)
    host = model.mrt_batch(imgs, refs, 0.0, **kw)
    dev = model.mrt_batch(imgs, refs, 0.0, on_device=True, **kw)
    assert [[c["text"] for c in g] for g in dev["candidates"]] == [[c["text"] for c in g] for g in host["candidates"]]
    # (the host path reports the float64 quotient and trains on its float32: the device's cost is that float32, bit for bit)
    cost32 = lambda out: np.array([c["cost"] for g in out["candidates"] for c in g], np.float32).tobytes()
    assert cost32(dev) == cost32(host)
    assert [len(g) for g in dev["candidates"]] == [2, 3] and dev["candidates"][0][0]["text"] == "a b c" and dev["candidates"][0][0]["cost"] == 0.0
    qd, qh = [c["q"] for g in dev["candidates"] for c in g], [c["q"] for g in host["candidates"] for c in g]
    assert np.abs(np.array(qd) - np.array(qh)).max() <= 1e-5 and abs(dev["risk"] - host["risk"]) <= 1e-5


def test_config_key_selects_the_device_path(model, monkeypatch):
    from latex_ocr_amd.model.utils.general import Config
    assert "on_device" in model.MRT_KEYS
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    seen = []
    real = model.mrt_batch
    monkeypatch.setattr(model, "mrt_batch", lambda *a, **k: seen.append(k) or real(*a, **k))
    monkeypatch.setattr(model, "evaluate", lambda *a, **k: {"perplexity": 1.0})
    sched = type("Sched", (), {"lr": 1e-3, "update": lambda self, **k: None})()
    train = [(imgs[0], "a b"), (imgs[1], "c")]
    before, t0 = model.engine.params.clone(), model.engine.adam_t
    model._run_train(Config({"batch_size": 2, "mrt": {"n": 2, "on_device": True}}), train, [], 0, sched)
    assert len(seen) == 1 and seen[0]["on_device"] is True and seen[0]["n"] == 2
    assert not torch.equal(model.engine.params, before) and model.engine.adam_t == t0 + 1          # the step was taken
