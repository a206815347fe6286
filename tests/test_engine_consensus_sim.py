"""CPU (hipsim): the consensus choice above the C ABI -- Engine.consensus, Engine.sample_decode(return_consensus=True) on the ids the decode leaves
on the device, and Img2SeqModel.sample_batch(consensus=True) -- against the host reference of tests/consensus_ref.py (the project's own levenshtein
and truncate_end, the risk in float64)."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
from simlib import SIM_SO, build_sim
from consensus_ref import check_against_host, check_sample_batch

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, H, W = 11, 32, 48
END = 10
N, MAX_ITER = 3, 4
# found on the CPU (tests/test_engine_mrt_device_sim.py's starting point): at this seed, temperature and top_k two draws of an image agree and
# others differ; the tests assert both
SAMPLING = dict(temperature=0.5, top_k=3, seed=5)


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


def _engine(lib):
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=MAX_ITER + 1)


def _images():
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    return pad_batch_images(imgs)


def test_sample_decode_returns_the_consensus_of_its_draws(lib):
    eng, img = _engine(lib), _images()
    ids = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, **SAMPLING)
    out = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, return_consensus=True, **SAMPLING)
    assert len(out) == 3 and np.array_equal(out[0], ids)
    best, risk = out[1:]
    d = check_against_host(ids, END, best, risk)
    # the preconditions: somewhere two draws of an image are equal, somewhere two differ
    off = ~np.eye(N, dtype=bool)
    assert (d[:, off] == 0).any() and (d > 0).any(), d.tolist()
    b2, r2, d2 = eng.consensus(ids, END, return_dist=True)
    assert b2.tolist() == best.tolist() and r2.tobytes() == risk.tobytes() and np.array_equal(d2, d)
    # with the scores in front, and without the normalisation
    full = eng.sample_decode(img, END, n=N, max_iter=MAX_ITER, return_scores=True, return_consensus=True, consensus_normalize=False, **SAMPLING)
    assert len(full) == 5 and np.array_equal(full[0], ids)
    check_against_host(ids, END, full[3], full[4], normalize=False)
    assert full[4].tobytes() == (d.sum(axis=2).astype(np.float32) / np.float32(N)).tobytes()


def test_consensus_takes_arrays_and_strided_tensors(lib):
    eng = _engine(lib)
    rng = np.random.default_rng(4)
    B, T, n = 3, 12, 5
    ids = rng.integers(0, 3, size=(B, T, n)).astype(np.int32)
    w = rng.uniform(0.5, 2.0, size=(B, n)).astype(np.float32)
    best, risk, dist = eng.consensus(ids, 2, return_dist=True)
    check_against_host(ids, 2, best, risk, dist)
    # rows [B, n, T] seen as [B, T, n], and a slice of a longer decode buffer: read in place through the tensor's strides
    rows = torch.from_numpy(np.ascontiguousarray(ids.transpose(0, 2, 1)))
    view = rows.permute(0, 2, 1)
    assert not view.is_contiguous()
    b2, r2 = eng.consensus(view, 2)
    assert b2.tolist() == best.tolist() and r2.tobytes() == risk.tobytes()
    buf = torch.from_numpy(np.concatenate([ids, np.full((B, 3, n), 2, np.int32)], axis=1))
    b3, r3 = eng.consensus(buf[:, :T], 2)
    assert b3.tolist() == best.tolist() and r3.tobytes() == risk.tobytes()
    # weights as an array and as a tensor; no cut; no normalisation
    bw, rw = eng.consensus(ids, 2, weights=w)
    check_against_host(ids, 2, bw, rw, weights=w)
    bt, rt = eng.consensus(torch.from_numpy(ids), 2, weights=torch.from_numpy(w))
    assert bt.tolist() == bw.tolist() and rt.tobytes() == rw.tobytes()
    bn, rn, dn = eng.consensus(ids, None, normalize=False, return_dist=True)
    check_against_host(ids, None, bn, rn, dn, normalize=False)
    assert (dn != dist).any()
    # the edges: no image, no token, one draw
    e = eng.consensus(ids[:0], 2, return_dist=True)
    assert [x.shape for x in e] == [(0,), (0, n), (0, n, n)]
    z = eng.consensus(ids[:, :0], 2, return_dist=True)
    assert not z[0].any() and not z[1].any() and not z[2].any() and z[2].shape == (B, n, n)
    o = eng.consensus(ids[:, :, :1], 2)
    assert not o[0].any() and not o[1].any() and o[1].shape == (B, 1)


def test_refusals_before_any_launch(lib, monkeypatch):
    eng = _engine(lib)
    ids = np.zeros((2, 6, 3), np.int32)
    w = np.ones((2, 3), np.float32)
    calls = []
    monkeypatch.setattr(eng, "_ck", lambda rc, what: calls.append(what))
    bad_w = [w[:1], w[:, :2], w.reshape(-1)]
    for k, v in ((0, -1.0), (1, float("nan")), (2, float("inf"))):
        x = w.copy()
        x[0, k] = v
        bad_w.append(x)
    x = w.copy()
    x[1] = 0.0
    bad_w.append(x)
    for kw in [dict(ids=ids[0]), dict(ids=ids[:, :, :0]), dict(ids=np.zeros((1, 2, _abi.LXO_CONSENSUS_MAX_N + 1), np.int32)),
               dict(ids=np.zeros((1, _abi.LXO_EDIT_MAX_REF + 1, 2), np.int32))] + [dict(weights=x) for x in bad_w]:
        a = dict(ids=ids, id_end=END)
        a.update(kw)
        with pytest.raises(ValueError):
            eng.consensus(**a)
    assert not calls
    eng.consensus(ids, END, weights=w)
    assert calls == ["consensus"]
    with pytest.raises(ValueError):
        eng.sample_decode(_images(), END, n=N, max_iter=_abi.LXO_EDIT_MAX_REF + 1, return_consensus=True)
    assert calls == ["consensus"] and eng.ws is None


# ------------------------------------------------------------------------------------------------------------------ the model --
@pytest.fixture(scope="module")
def model(tmp_path_factory, lib):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    tmp = tmp_path_factory.mktemp("consensus")
    (tmp / "vocab.txt").write_text("\n".join(["a", "b", "c", "d", "e", "f", "g", "h"]) + "\n")          # + _UNK, _PAD, _END: 11 ids
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp / "vocab.txt")}))
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": MAX_ITER - 1, "decoding": "greedy"})
    m = Img2SeqModel(cfg, str(tmp) + "/out/", vocab, lib=lib)
    m.build_pred()
    m.engine = _engine(lib)
    return m


def test_sample_batch_consensus(model):
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    res = check_sample_batch(model, imgs, N, END, **SAMPLING)
    assert any(len(r["hypotheses"]) < N for r in res) and any(len(r["hypotheses"]) > 1 for r in res)


def test_predict_refuses_consensus_without_sample(capsys):
    import predict
    with pytest.raises(SystemExit) as e:
        predict.main(["--consensus", "formula.png"])
    assert e.value.code == 2 and "--consensus" in capsys.readouterr().err
