"""-m gpu: the consensus choice among sampled transcriptions, on the MI355X.

1. lxo_consensus on the case matrix of tests/consensus_ref.py, with the checks of the hipsim file: distances and arg-min exactly, the risk bit for
   bit where the definition makes it exact and within the derived bound elsewhere; twice the same bytes; captured into a graph.
2. Engine.sample_decode(return_consensus=True), Engine.consensus and Img2SeqModel.sample_batch(consensus=True) at 32 x 48, V = 11, in both dtypes,
   against the host reference (the checks tests/test_engine_consensus_sim.py runs under hipsim).
3. predict.py --sample 4 --consensus in a process of its own."""
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
from latex_ocr_amd import _abi
from latex_ocr_amd.engine import _p
from consensus_ref import all_cases, check_against_host, check_case, check_outputs, check_sample_batch, matrix_cases, run_consensus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, H, W = 11, 32, 48
END = V - 1
MAX_ITER = 6
SAMPLING = dict(temperature=0.5, top_k=2, seed=7)                   # few likely tokens per step: draws repeat


class Dev(object):
    """numpy <-> the GPU for the shared runners of tests/consensus_ref.py"""
    stream = None

    @staticmethod
    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def ptr(a):
        return _p(a)

    @staticmethod
    def down(a):
        return a.cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


# ------------------------------------------------------------------------------------------------------------------ 1. the kernels --
def test_consensus_matrix(lib):
    for c in all_cases():
        check_case(lib, c, Dev)


def test_runs_repeat(lib):
    for c in (matrix_cases()[-3], matrix_cases()[20]):
        a, b = run_consensus(lib, c, Dev), run_consensus(lib, c, Dev)
        assert a[0] == b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])), c["name"]


def test_the_call_is_captured_into_a_graph(lib):
    """two launches on the capturing stream, nothing that synchronises: a replay on other ids gives what the eager call gives on them"""
    a = [c for c in matrix_cases() if c["name"].startswith("B5 T20 n16")][0]
    B, n, T = a["B"], a["n"], a["T"]
    rng = np.random.default_rng(2)
    other = rng.integers(0, 3, size=a["ids"].shape).astype(np.int32)
    eng = Engine(V, dtype="f32", seed=0)
    ids = torch.from_numpy(a["ids"]).cuda().reshape(B, -1, n)
    eng._consensus_device(ids[:, :T], a["id_end"])                  # eager first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        best, risk, dist = eng._consensus_device(ids[:, :T], a["id_end"])
    g.replay()
    torch.cuda.synchronize()
    check_outputs(a, dist.cpu().numpy(), risk.cpu().numpy(), best.cpu().numpy())
    ids.copy_(torch.from_numpy(other).cuda().reshape(B, -1, n))
    g.replay()
    torch.cuda.synchronize()
    want = eng._consensus_device(ids[:, :T], a["id_end"])
    assert all(torch.equal(x, y) for x, y in zip((best, risk, dist), want))
    assert not np.array_equal(dist.cpu().numpy(), a["dist"])


# ------------------------------------------------------------------------------------------------------- 2. the engine and the model --
def _images(n=3):
    imgs, _ = synthetic.make_set(n, H, W, V, 2, 4, seed=9)
    return imgs


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sample_decode_returns_the_consensus_of_its_draws(dtype):
    eng, img, n = Engine(V, dtype=dtype, seed=3), pad_batch_images(_images()), 4
    ids = eng.sample_decode(img, END, n=n, max_iter=MAX_ITER, **SAMPLING)
    out = eng.sample_decode(img, END, n=n, max_iter=MAX_ITER, return_consensus=True, **SAMPLING)
    assert len(out) == 3 and np.array_equal(out[0], ids)
    best, risk = out[1:]
    d = check_against_host(ids, END, best, risk)
    print("%s: steps %d, distances %s, risk %s, best %s" % (dtype, ids.shape[1], d.tolist(), risk.tolist(), best.tolist()))
    b2, r2, d2 = eng.consensus(ids, END, return_dist=True)
    assert b2.tolist() == best.tolist() and r2.tobytes() == risk.tobytes() and np.array_equal(d2, d)
    # a strided device tensor: rows [B, n, T] seen as [B, T, n]
    view = torch.from_numpy(np.ascontiguousarray(ids.transpose(0, 2, 1))).cuda().permute(0, 2, 1)
    b3, r3 = eng.consensus(view, END, normalize=False)
    check_against_host(ids, END, b3, r3, normalize=False)
    assert r3.tobytes() == (d.sum(axis=2).astype(np.float32) / np.float32(n)).tobytes()
    with pytest.raises(ValueError):
        eng.consensus(ids, END, weights=np.zeros((ids.shape[0], n), np.float32))


def _model(tmp, dtype):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    d = os.path.join(tmp, "results") + "/"
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(tmp, "vocab.txt"), "w") as f:
        f.write("\n".join(["a", "b", "c", "d", "e", "f", "g", "h"]) + "\n")          # + _UNK, _PAD, _END: 11 ids
    cfg = json.load(open(os.path.join(ROOT, "configs", "model.json")))
    cfg.update(decoding="greedy", max_length_formula=MAX_ITER - 1, compute_dtype=dtype)
    json.dump(cfg, open(d + "model.json", "w"))
    json.dump({"export_name": "vocab.json", "unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": os.path.join(tmp, "vocab.txt"), "min_count_tok": 1},
              open(d + "vocab.json", "w"))
    m = Img2SeqModel(Config(d + "model.json"), d, Vocab(Config(d + "vocab.json")))
    m.build_pred()
    return m, d


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sample_batch_consensus(tmp_path, dtype):
    m, _ = _model(str(tmp_path), dtype)
    assert m._vocab.n_tok == V and m._vocab.id_end == END
    check_sample_batch(m, _images(), 4, END, **SAMPLING)
    one = check_sample_batch(m, _images(), 4, END, top_k=1)         # the arg-max four times: one hypothesis, no cost
    assert all(r["consensus"] == 0 and r["expected_cost"] == 0.0 and len(r["hypotheses"]) == 1 for r in one)


# ------------------------------------------------------------------------------------------------------------------ 3. the driver --
def test_predict_sample_consensus(tmp_path):
    from PIL import Image
    m, d = _model(str(tmp_path), "bf16")
    m.save_session(1)
    path = os.path.join(str(tmp_path), "formula.png")
    Image.fromarray(np.asarray(_images(1)[0]).reshape(H, W)).save(path)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--sample", "4", "--consensus", "--temperature", "1.2",
                                   "--seed", "3", path], cwd=str(tmp_path), timeout=600, env=dict(os.environ, PYTHONPATH=ROOT)).decode()
    head = re.findall(r"=> consensus: (.*) \texpected cost ([0-9.]+)", out)
    rows = re.findall(r"^([* ]) +(\d+) x  logp +\S+  risk ([0-9.]+)  (.*)$", out, re.M)
    assert len(head) == 1 and 1 <= len(rows) <= 4 and sum(int(r[1]) for r in rows) == 4, out
    marked = [r for r in rows if r[0] == "*"]
    assert len(marked) == 1 and marked[0][3] == head[0][0] and marked[0][2] == head[0][1], out
    assert head[0][0] in [r[3] for r in rows] and float(head[0][1]) == min(float(r[2]) for r in rows), out
