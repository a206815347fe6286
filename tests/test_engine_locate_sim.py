"""CPU (hipsim): token locations through the Python layers -- Engine.attention_locate on arrays, tensors and strided views against the C call of
tests/attention_locate_ref.py; Engine.score(locate=True) against attention_locate on score(return_attention=True)'s maps, byte for byte;
greedy_decode / beam_decode / sample_decode(return_boxes=True) against attention_locate on return_attention's maps (beam: the host back-trace, and a
hand-built parents array); the other outputs byte-equal with and without the flags; feature_box_to_pixels; Img2SeqModel.locate_batch both ways.
B = 3 (fill-up rows present), T <= 8, a 32 x 64 image, V = 20."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine, Locations
from latex_ocr_amd.model.utils.image import encoder_out_hw, feature_box_to_pixels, pad_batch_images
from latex_ocr_amd.model.utils.text import beam_backtrace, beam_parent_rows, beam_slots, pad_batch_formulas
from simlib import SIM_SO, build_sim
from attention_locate_ref import named, run_locate

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, H, W, T = 20, 32, 64, 6
END, PAD = V - 1, V - 2
NAMES = ("peak", "box", "stats", "coverage")


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.fixture(scope="module", params=["f32", "bf16"])
def eng(lib, request):
    return Engine(V, dims=SMALL, dtype=request.param, device="cpu", seed=3, lib=lib, max_steps=T + 2)


def _batch(seed=7):
    imgs, forms = synthetic.make_set(3, H, W, V - 2, 2, T - 1, seed=seed)
    f, ln = pad_batch_formulas(forms, PAD, END)
    return pad_batch_images(imgs), f, ln


def same(a, b):
    """two Locations, byte for byte"""
    for k, x, y in zip(NAMES, a, b):
        assert (x is None) == (y is None) and (x is None or (x.shape == y.shape and x.tobytes() == y.tobytes())), k


def end_lengths(ids, n):
    hit = ids == END
    return np.where(hit.any(-1), hit.argmax(-1) + 1, n).astype(np.int32)


def test_attention_locate_takes_arrays_tensors_and_views(lib):
    eng = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib)
    c = named("3x5 BTR")                                            # rows + 1 alpha rows, len and src
    rc, want = run_locate(lib, c, 0.9)
    assert rc == 0
    maps = c["maps"].reshape(c["alpha_rows"], c["steps"], c["Hp"], c["Wp"])
    got = eng.attention_locate(maps, lengths=c["len"], src=c["src"], mass=0.9, coverage=True)
    assert isinstance(got, Locations)
    same(got, Locations(want["peak"], want["box"], want["stats"], want["coverage"].reshape(c["rows"], c["Hp"], c["Wp"])))
    t = named("3x5 TBR")                                            # the [steps][rows][Rp] buffer, NaN padding, as a permuted view: read in place
    rc, want = run_locate(lib, t, 0.5)
    view = torch.from_numpy(t["buf"])[:, :, :t["R"]].permute(1, 0, 2).unflatten(2, (t["Hp"], t["Wp"]))
    assert not view.is_contiguous()
    got = eng.attention_locate(view, mass=0.5, coverage=True)
    same(got, Locations(want["peak"], want["box"], want["stats"], want["coverage"].reshape(t["rows"], t["Hp"], t["Wp"])))
    assert eng.attention_locate(view, mass=0.5).coverage is None
    dev = eng.attention_locate_dev(view, mass=0.5)
    assert isinstance(dev.peak, torch.Tensor) and np.array_equal(dev.peak.numpy(), want["peak"])
    for bad in (dict(mass=0.0), dict(mass=1.5), dict(lengths=[1, 2]), dict(src=np.zeros((2, 3), np.int32))):
        with pytest.raises(ValueError):
            eng.attention_locate(view, **bad)
    with pytest.raises(ValueError):
        eng.attention_locate(np.zeros((2, 3, 5), np.float32))


def test_score_locates_the_given_formula(eng):
    img, f, ln = _batch()
    base = eng.score(img, f, ln, return_top1=True)
    out = eng.score(img, f, ln, return_top1=True, locate=True, mass=0.9, coverage=True, return_attention=True)
    assert len(out) == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(base, out[:3]))
    loc, maps = out[3], out[4]
    Hp, Wp = encoder_out_hw(H, W)
    assert isinstance(loc, Locations) and maps.shape == (3, f.shape[1], Hp, Wp) and maps.dtype == np.float32
    same(loc, eng.attention_locate(maps, lengths=ln, mass=0.9, coverage=True))
    live = np.arange(f.shape[1])[None, :] < ln[:, None]
    assert (loc.peak[live] >= 0).all() and (loc.peak[~live] == -1).all() and (loc.box[~live] == -1).all() and not loc.stats[~live].any()
    assert np.allclose(loc.stats[live][:, 0], 1.0, atol=1e-3)      # a soft-max sums to 1
    assert np.allclose(loc.coverage.sum((1, 2)), ln, atol=1e-2)
    two = eng.score(img, f, ln, locate=True, mass=0.5)
    assert len(two) == 3 and two[2].coverage is None and np.array_equal(two[2].peak, loc.peak)
    assert two[0].tobytes() == base[0].tobytes() and two[1].tobytes() == base[2].tobytes()
    for bad in (dict(locate=True, mass=0.0), dict(coverage=True)):
        with pytest.raises(ValueError):
            eng.score(img, f, ln, **bad)


def test_greedy_boxes(eng):
    img, _, _ = _batch()
    ids, alpha, logp = eng.greedy_decode(img, END, max_iter=T, return_attention=True, return_scores=True)
    out = eng.greedy_decode(img, END, max_iter=T, return_scores=True, return_boxes=True, mass=0.9, coverage=True)
    assert len(out) == 3 and out[0].tobytes() == ids.tobytes() and out[1].tobytes() == logp.tobytes()
    same(out[2], eng.attention_locate(alpha, lengths=end_lengths(ids, ids.shape[1]), mass=0.9, coverage=True))
    both = eng.greedy_decode(img, END, max_iter=T, return_attention=True, return_boxes=True)
    assert len(both) == 3 and both[0].tobytes() == ids.tobytes() and both[1].tobytes() == alpha.tobytes() and np.array_equal(both[2].peak, out[2].peak)


def test_beam_boxes_follow_the_back_trace(eng):
    img, _, _ = _batch()
    k = 3
    ids, par, alpha, sc = eng.beam_decode(img, END, k, max_iter=T, return_attention=True, return_scores=True)
    out = eng.beam_decode(img, END, k, max_iter=T, return_scores=True, return_boxes=True, mass=0.9, coverage=True)
    assert len(out) == 4 and all(a.tobytes() == b.tobytes() for a, b in zip(out[:3], (ids, par, sc)))
    B, n = ids.shape[:2]
    slots, hyp = beam_slots(par), beam_backtrace(ids, par)
    # predict_with_attention's rule, for every image and slot: the map of step t is the one of the parent of the path's slot at t
    traced = np.stack([np.stack([np.stack([alpha[b, t, par[b, t, slots[b, t, i]]] for t in range(n)]) for i in range(k)]) for b in range(B)])
    ln = end_lengths(hyp.transpose(0, 2, 1), n)                     # [B, k]
    want = eng.attention_locate(traced.reshape((B * k, n) + traced.shape[3:]), lengths=ln.reshape(-1), mass=0.9, coverage=True)
    same(out[3], Locations(*[a.reshape((B, k) + a.shape[1:]) for a in want]))


def test_parent_rows_of_a_hand_built_beam():
    par = np.array([[[0, 0, 0], [2, 0, 1]], [[0, 0, 0], [1, 1, 0]]], np.int32)       # B = 2, T = 2, k = 3
    rows = beam_parent_rows(par)
    # image 0: the hypotheses ending in slots 0, 1, 2 sat in slots 2, 0, 1 at step 0; their last tokens were read off rows 2, 0, 1, their first off row 0
    assert rows[0].tolist() == [[0, 0, 0], [2, 0, 1]] and beam_slots(par)[0].tolist() == [[2, 0, 1], [0, 1, 2]]
    assert rows[1].tolist() == [[3, 3, 3], [4, 4, 3]] and beam_slots(par)[1].tolist() == [[1, 1, 0], [0, 1, 2]]


def test_sample_boxes(eng):
    img, _, _ = _batch()
    n = 2
    ids, alpha, logp, logq = eng.sample_decode(img, END, n=n, seed=5, max_iter=T, return_attention=True, return_scores=True)
    out = eng.sample_decode(img, END, n=n, seed=5, max_iter=T, return_scores=True, return_boxes=True, mass=0.9, coverage=True)
    assert len(out) == 4 and all(a.tobytes() == b.tobytes() for a, b in zip(out[:3], (ids, logp, logq)))
    B, steps = ids.shape[:2]
    maps = alpha.transpose(0, 2, 1, 3, 4).reshape((B * n, steps) + alpha.shape[3:])
    want = eng.attention_locate(maps, lengths=end_lengths(ids.transpose(0, 2, 1), steps).reshape(-1), mass=0.9, coverage=True)
    same(out[3], Locations(*[a.reshape((B, n) + a.shape[1:]) for a in want]))


def test_feature_box_to_pixels():
    Hp, Wp = encoder_out_hw(H, W)                                   # 2 x 6 cells of a 32 x 64 image
    assert (Hp, Wp) == (2, 6)
    assert feature_box_to_pixels((0, 0, 0, 0), H, W) == (8, 8, 16, 16)
    assert feature_box_to_pixels((Wp - 1, 0, Wp - 1, 0), H, W) == (48, 8, 56, 16)
    assert feature_box_to_pixels((0, Hp - 1, 0, Hp - 1), H, W) == (8, 16, 16, 24)
    assert feature_box_to_pixels((Wp - 1, Hp - 1, Wp - 1, Hp - 1), H, W) == (48, 16, 56, 24)
    assert feature_box_to_pixels((0, 0, Wp - 1, Hp - 1), H, W) == (8, 8, 56, 24)
    assert feature_box_to_pixels((2, 0, 5, 1), 20, 50) == (24, 8, 50, 20)             # clipped to a smaller image
    assert feature_box_to_pixels(np.array([1, 1, 1, 1], np.int32), H, W) == (16, 16, 24, 24)
    with pytest.raises(ValueError):
        feature_box_to_pixels((0, 0, 0, 0), H, W, encoder_cnn="cnn")
    with pytest.raises(ValueError):
        feature_box_to_pixels((-1, -1, -1, -1), H, W)


def test_model_locate_batch(lib, tmp_path):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    toks = ["t%d" % i for i in range(V - 3)]                        # + _UNK, _PAD, _END
    (tmp_path / "vocab.txt").write_text("\n".join(toks) + "\n")
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp_path / "vocab.txt")}))
    assert vocab.n_tok == V
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": T - 1, "decoding": "greedy"})
    m = Img2SeqModel(cfg, str(tmp_path) + "/out/", vocab, lib=lib)
    m.build_pred()
    m.engine = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=T + 2)
    imgs, _ = synthetic.make_set(2, H, W, V - 3, 2, 4, seed=9)
    Hp, Wp = encoder_out_hw(H, W)
    given = m.locate_batch(imgs, ["t1 t2 t3", "t4"], mass=0.9)
    assert [len(r["tokens"]) for r in given] == [4, 2] and given[0]["tokens"][-1]["token"] == "_END" and given[1]["tokens"][0]["token"] == "t4"
    for r in given:
        assert r["coverage"].shape == (Hp, Wp) and 0 < r["max_coverage"] == float(r["coverage"].max()) and 0 <= r["uncovered"] <= 1
        assert abs(float(r["coverage"].sum()) - len(r["tokens"])) < 1e-2
        for e in r["tokens"]:
            l, t, rt, bt = e["box"]
            assert 8 <= l < rt <= W - 8 and 8 <= t < bt <= H - 8 and 0.8 - 1e-5 <= e["inside"] <= 1 + 1e-5 and 0 < e["peak_share"] <= 1
            assert l - 8 <= e["centre"][0] <= rt + 8 and e["spread"][0] >= 0
    dec = m.locate_batch(imgs)
    hyp = m.predict_batch(imgs)[0]
    for r, h in zip(dec, hyp):
        assert [e["token"] for e in r["tokens"]][:len(h.split())] == h.split() and len(r["tokens"]) in (len(h.split()), len(h.split()) + 1)
    with pytest.raises(ValueError):
        m.locate_batch(imgs, ["t1"])
    m._config.encoder_cnn = "cnn"
    with pytest.raises(ValueError):
        m.locate_batch(imgs)
