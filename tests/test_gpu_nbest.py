"""-m gpu: the beam finished on the device, through the Python layers on the MI355X -- the checks of tests/test_engine_nbest_sim.py on a real engine
in f32 and bf16 (32 x 48, V = 11, beam 3, max_iter 4 .. 6): beam_decode(return_nbest=True) against the host route on the same ids / parents / scores,
its consensus with the posterior as weights, its coverage penalty against coverage summed on the host from the maps, the combinations with prefix /
allowed / grammar, Engine.beam_finalize on device views; a call made twice gives the same bytes; Img2SeqModel.nbest_batch and
predict.py --nbest --length-penalty 0.6 --consensus in a process of its own."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from test_engine_nbest_sim import END, H, K, V, W
from test_engine_nbest_sim import test_nbest_batch as _nbest_batch
from test_engine_nbest_sim import test_nbest_combines_with_prefix_allowed_and_grammar as _combines
from test_engine_nbest_sim import test_nbest_is_the_host_route_on_the_same_decode as _host_route
from test_engine_nbest_sim import test_the_consensus_over_the_beam as _consensus
from test_engine_nbest_sim import test_the_coverage_penalty_reads_the_back_traced_maps as _coverage
from beam_finalize_ref import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["f32", "bf16"])
def eng(request):
    return Engine(V, dtype=request.param, seed=3, max_steps=7)


@pytest.mark.parametrize("max_iter", [4, 6])
def test_nbest_is_the_host_route_on_the_same_decode(eng, max_iter):
    _host_route(eng, max_iter)


def test_the_consensus_over_the_beam(eng):
    _consensus(eng)


def test_the_coverage_penalty_reads_the_back_traced_maps(eng):
    _coverage(eng)


def test_nbest_combines_with_prefix_allowed_and_grammar(eng):
    _combines(eng)


def test_a_call_made_twice_gives_the_same_bytes(eng):
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    kw = dict(max_iter=6, return_nbest=True, length_penalty=0.6, coverage_penalty=0.2, return_consensus=True)
    a, b = eng.beam_decode(pad_batch_images(imgs), END, K, **kw), eng.beam_decode(pad_batch_images(imgs), END, K, **kw)
    assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2].tobytes() == b[2].tobytes()
    assert a[3].tobytes() == b[3].tobytes()


def test_beam_finalize_reads_device_views_in_place(eng):
    c = make_case("device views", 3, 5, 9, 12, "random", "mixed", 21)
    w, E = c["want"], c["id_end"]
    t = [torch.from_numpy(c[n].copy()).cuda() for n in ("ids", "parents", "scores")]
    views = [x[:, :9] for x in t]
    assert not views[0].is_contiguous()
    perm = [x[:, :9].permute(0, 2, 1).contiguous().permute(0, 2, 1) for x in t]
    for args in (views, perm, [views[0], perm[1], views[2]], [c["ids"][:, :9], c["parents"][:, :9], c["scores"][:, :9]]):
        got = eng.beam_finalize(*args, id_end=E)
        for name, a in zip(("hyp", "len", "src", "tok_logp", "seq_logp"), got):
            assert a.tobytes() == w[name].tobytes(), name
    dev = eng.beam_finalize_dev(*views, id_end=E)
    assert dev.hyp.is_cuda and np.array_equal(dev.lengths.cpu().numpy(), w["len"])
    with pytest.raises(ValueError):
        eng.beam_finalize(c["ids"], np.full_like(c["parents"], 5), id_end=E)


def _model(tmp, dtype):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    d = os.path.join(tmp, "results") + "/"
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(tmp, "vocab.txt"), "w") as f:
        f.write("\n".join(["a", "b", "c", "d", "e", "f", "g", "h"]) + "\n")          # + _UNK, _PAD, _END: 11 ids
    cfg = json.load(open(os.path.join(ROOT, "configs", "model.json")))
    cfg.update(decoding="beam_search", beam_size=K, max_length_formula=5, compute_dtype=dtype)
    json.dump(cfg, open(d + "model.json", "w"))
    json.dump({"export_name": "vocab.json", "unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": os.path.join(tmp, "vocab.txt"), "min_count_tok": 1},
              open(d + "vocab.json", "w"))
    m = Img2SeqModel(Config(d + "model.json"), d, Vocab(Config(d + "vocab.json")))
    m.build_pred()
    return m, d


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_nbest_batch(tmp_path, dtype):
    m, _ = _model(str(tmp_path), dtype)
    assert m._vocab.n_tok == V and m._vocab.id_end == END
    _nbest_batch(m)


def test_predict_nbest(tmp_path):
    from PIL import Image
    m, d = _model(str(tmp_path), "bf16")
    m.save_session(1)
    imgs, _ = synthetic.make_set(1, H, W, V, 2, 4, seed=9)
    path = os.path.join(str(tmp_path), "formula.png")
    Image.fromarray(np.asarray(imgs[0]).reshape(H, W)).save(path)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--nbest", "--length-penalty", "0.6", "--consensus", path],
                                  cwd=str(tmp_path), timeout=600, env=dict(os.environ, PYTHONPATH=ROOT)).decode()
    head = re.findall(r"=> consensus: (.*) \texpected cost ([0-9.]+)", out)
    rows = re.findall(r"^([* ]) slot +(\d+)  score +(\S+)  logp +(\S+)  post (\S+)  len +(\d+)  risk ([0-9.]+)  (.*)$", out, re.M)
    assert len(head) == 1 and len(rows) == K and sorted(int(r[1]) for r in rows) == list(range(K)), out
    scores = [float(r[2]) for r in rows]
    assert scores == sorted(scores, reverse=True) and abs(sum(float(r[4]) for r in rows) - 1.0) < 1e-3, out
    marked = [r for r in rows if r[0] == "*"]
    assert len(marked) == 1 and marked[0][7] == head[0][0] and marked[0][6] == head[0][1] and float(head[0][1]) == min(float(r[6]) for r in rows), out
