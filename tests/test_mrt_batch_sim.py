"""CPU (hipsim): Img2SeqModel.mrt_batch -- sampled candidates, their edit-distance costs, one Engine.mrt_step -- on a tiny vocabulary: what the
candidates are, what they cost, and the SIGN of the step: a few steps at one seed lower the expected cost of the same candidates."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.evaluation.text import levenshtein
from simlib import SIM_SO, build_sim

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, H, W = 11, 32, 48
SEED, N, ALPHA, LR = 3, 4, 1.0, 2e-3


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    build_sim()
    lib = _abi.bind(ctypes.CDLL(SIM_SO))
    tmp = tmp_path_factory.mktemp("mrt")
    (tmp / "vocab.txt").write_text("\n".join(["a", "b", "c", "d", "e", "f", "g", "h"]) + "\n")          # + _UNK, _PAD, _END: 11 ids
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp / "vocab.txt")}))
    assert vocab.n_tok == V
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": 5, "decoding": "greedy"})
    m = Img2SeqModel(cfg, str(tmp) + "/out/", vocab, lib=lib)
    m.build_pred()
    m.engine = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=7)      # C = 128, the width the sim tests interpret
    return m, vocab


def test_mrt_batch_candidates_costs_and_the_sign_of_the_step(model):
    m, vocab = model
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    refs = ["a b c", "d e"]
    kw = dict(n=N, alpha=ALPHA, temperature=1.0, seed=SEED)
    out = m.mrt_batch(imgs, refs, 0.0, **kw)                       # lr 0: the candidates and the risk of the initial weights
    assert len(out["candidates"]) == 2 and np.isfinite(out["risk"])
    for ref, cands in zip(refs, out["candidates"]):
        texts = [c["text"] for c in cands]
        assert len(set(texts)) == len(texts) and 1 <= len(texts) <= N + 1           # distinct
        assert texts[0] == ref                                                      # the reference, asked for
        for c in cands:
            want = levenshtein(c["text"].split(" ") if c["text"] else [], ref.split(" ")) / float(len(ref.split(" ")))
            assert c["cost"] == pytest.approx(want, abs=1e-7)
        assert cands[0]["cost"] == 0.0
        assert abs(sum(c["q"] for c in cands) - 1.0) <= 1e-5
    assert abs(out["risk"] - np.mean([sum(c["q"] * c["cost"] for c in cands) for cands in out["candidates"]])) <= 1e-5
    no_ref = m.mrt_batch(imgs, refs, 0.0, include_reference=False, **kw)
    for ref, a, b in zip(refs, out["candidates"], no_ref["candidates"]):       # the distinct draws alone; the reference joins them once
        assert set(c["text"] for c in b) | {ref} == set(c["text"] for c in a) and len(b) in (len(a), len(a) - 1)
    ids = [vocab.form_prepro(r) for r in refs]                     # token-id lists are taken as the strings are
    same = m.mrt_batch(imgs, ids, 0.0, **kw)
    assert same["risk"] == out["risk"]
    with pytest.raises(ValueError):
        m.mrt_batch(imgs, refs[:1], 0.0, **kw)
    # five steps at one seed and a small lr, then the same sampling again: the expected cost is lower.  A smoke test of the SIGN at this seed
    # (measured: 0.928 -> 0.609), not a convergence claim: the draws after the update are other draws, and another seed can go the other way
    before = out["risk"]
    for _ in range(5):
        m.mrt_batch(imgs, refs, LR, **kw)
    after = m.mrt_batch(imgs, refs, 0.0, **kw)["risk"]
    print("risk before %.6f, after five steps %.6f" % (before, after))
    assert after < before


def test_mrt_config_key_is_single_process(model):
    m, _ = model
    from latex_ocr_amd.model.utils.general import Config
    m.dist = type("FakeDist", (), {"world": 2, "rank": 0})()
    try:
        with pytest.raises(NotImplementedError, match="single process"):
            m._run_train(Config({"batch_size": 2, "mrt": {"n": 2}}), [], [], 0, None)
    finally:
        m.dist = None
    with pytest.raises(ValueError, match="unknown"):
        m._run_train(Config({"batch_size": 2, "mrt": {"n": 2, "beta": 1}}), [], [], 0, None)
