"""-m gpu: token locations through the Python layers on the MI355X -- the checks of tests/test_engine_locate_sim.py on a real engine in f32 and bf16
(B = 3: fill-up rows present; T <= 8; a 32 x 64 image; V = 20): Engine.score(locate=True) against attention_locate on score(return_attention=True)'s
maps byte for byte, greedy / beam (k = 3, the host back-trace) / sample (n = 2) with return_boxes=True against attention_locate on return_attention's
maps, every other output byte-equal with and without the flags; a strided device view read in place; Img2SeqModel.locate_batch both ways and
predict.py --boxes in a process of its own on the synthetic data set."""
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
from latex_ocr_amd.engine import Locations
from latex_ocr_amd.model.utils.image import encoder_out_hw
from test_engine_locate_sim import END, H, T, V, W, same
from test_engine_locate_sim import test_beam_boxes_follow_the_back_trace as _beam
from test_engine_locate_sim import test_greedy_boxes as _greedy
from test_engine_locate_sim import test_sample_boxes as _sample
from test_engine_locate_sim import test_score_locates_the_given_formula as _score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["f32", "bf16"])
def eng(request):
    return Engine(V, dtype=request.param, seed=3, max_steps=T + 2)


def test_score_locates_the_given_formula(eng):
    _score(eng)


def test_greedy_boxes(eng):
    _greedy(eng)


def test_beam_boxes_follow_the_back_trace(eng):
    _beam(eng)


def test_sample_boxes(eng):
    _sample(eng)


def test_a_strided_device_view_is_read_in_place(eng):
    """a decode's [max_steps][rows][Rp] buffer, steps it did not run and the row padding behind the view"""
    Hp, Wp = encoder_out_hw(H, W)
    R, Rp, rows, steps = Hp * Wp, (Hp * Wp + 7) // 8 * 8, 5, 4
    rng = np.random.default_rng(3)
    buf = torch.full((steps + 2, rows, Rp), float("nan"), device="cuda")
    maps = rng.random((rows, steps, R)).astype(np.float32)
    buf[:steps, :, :R] = torch.from_numpy(maps.transpose(1, 0, 2)).cuda()
    view = buf[:steps, :, :R].permute(1, 0, 2).unflatten(2, (Hp, Wp))
    assert not view.is_contiguous()
    ln = np.array([4, 0, 2, 4, 1], np.int32)
    got = eng.attention_locate(view, lengths=ln, mass=0.9, coverage=True)
    same(got, eng.attention_locate(maps.reshape(rows, steps, Hp, Wp), lengths=ln, mass=0.9, coverage=True))
    live = np.arange(steps)[None, :] < ln[:, None]
    assert (got.peak[live] == maps.argmax(2)[live]).all() and (got.peak[~live] == -1).all()
    assert isinstance(got, Locations) and got.coverage.shape == (rows, Hp, Wp)


def _results_dir(tmp):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    os.chdir(tmp)
    synthetic.write_dataset("data/synthetic", n_train=8, n_val=4, n_test=6)
    d = "results/locate/"
    os.makedirs(d, exist_ok=True)
    cfg = json.load(open(os.path.join(ROOT, "configs", "model.json")))
    cfg.update(max_length_formula=12)
    json.dump(cfg, open(d + "model.json", "w"))
    shutil.copy(os.path.join(ROOT, "configs", "vocab_small.json"), d + "vocab.json")
    shutil.copy(os.path.join(ROOT, "configs", "data_small.json"), d + "data.json")
    m = Img2SeqModel(Config(d + "model.json"), d, Vocab(Config(d + "vocab.json")))
    m.build_pred()
    m.save_session(1)
    return m, d


def test_locate_batch_and_the_driver(tmp_path, monkeypatch):
    from PIL import Image
    from latex_ocr_amd.model.utils.image import greyscale
    monkeypatch.chdir(tmp_path)
    m, d = _results_dir(str(tmp_path))
    png = sorted(p for p in os.listdir("data/synthetic/test") if p.endswith(".png"))[0]
    img = greyscale(np.asarray(Image.open("data/synthetic/test/" + png).convert("RGB")))
    formula = "t1 t2 t3 zz t4"
    given = m.locate_batch([img], [formula])[0]
    assert len(given["tokens"]) == 6 and given["tokens"][-1]["token"] == "_END" and abs(float(given["coverage"].sum()) - 6) < 1e-2
    dec = m.locate_batch([img])[0]                                  # the shipped config decodes with beam search: the back-traced best hypothesis
    assert dec["tokens"] and dec["coverage"].shape == given["coverage"].shape == encoder_out_hw(img.shape[0], img.shape[1])
    for e in given["tokens"] + dec["tokens"]:
        l, t, r, b = e["box"]
        assert 0 <= l < r <= img.shape[1] and 0 <= t < b <= img.shape[0] and 0.8 - 1e-5 <= e["inside"] <= 1 + 1e-5
    run = lambda *extra: subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--boxes", *extra,
                                                  "data/synthetic/test/" + png], cwd=str(tmp_path), timeout=600,
                                                 env=dict(os.environ, PYTHONPATH=ROOT)).decode().splitlines()
    out = run("--formula", formula)
    head = [k for k, x in enumerate(out) if "<=" in x][-1]
    assert "max coverage" in out[head] and len(out) - head - 1 == 6
    for line, e in zip(out[head + 1:], given["tokens"]):
        w = line.split()
        assert w[1] == e["token"] and tuple(int(v) for v in w[3:7]) == e["box"] and float(w[8]) == pytest.approx(e["inside"], abs=2e-3)
    out = run()
    head = [k for k, x in enumerate(out) if "=>" in x][-1]
    assert [line.split()[1] for line in out[head + 1:]] == [e["token"] for e in dec["tokens"]]
