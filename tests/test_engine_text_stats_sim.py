"""CPU (hipsim): the text metrics through the Python layers -- Engine.text_stats / text_metrics (host and device inputs, views read in place, the
corpus accumulator, the ValueErrors), Img2SeqModel.score_ids against score_files on the files write_answers writes from the same ids (the empty-line
quirk included), and the opt-in wiring: _run_evaluate with metrics_on_device and evaluate_txt.py --on-device against their defaults."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.evaluation.text import (bleu_score, edit_distance, exact_match_score, score_files, scores_from_counts, truncate_end,
                                                 write_answers)
from latex_ocr_amd.model.utils.text import pad_batch_formulas
from simlib import SIM_SO, build_sim
from text_stats_ref import corpus_of, pair_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, H, W = 11, 32, 48
END, PAD = 10, 9
MAX_LEN = 3


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.fixture(scope="module")
def eng(lib):
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=MAX_LEN + 2)


def _host(h, r):
    return {"BLEU-4": bleu_score(r, h) * 100, "ExactMatchScore": exact_match_score(r, h) * 100, "EditDistance": edit_distance(r, h) * 100}


def test_text_stats_takes_arrays_tensors_and_views(eng):
    rng = np.random.default_rng(3)
    hyp = rng.integers(0, 3, size=(6, 12)).astype(np.int32)
    ref = rng.integers(0, 3, size=(3, 9)).astype(np.int32)
    hl, rl = np.array([12, 0, 5, 7, 12, 1]), np.array([9, 4, 0])
    cut = [(list(hyp[p, :hl[p]]), list(ref[p // 2, :rl[p // 2]])) for p in range(6)]
    want = np.array([pair_stats(h, r) for h, r in cut], np.int32)
    s = eng.text_stats(hyp, ref, hl, rl)
    assert s.dtype == np.int32 and s.shape == (6, 12) and np.array_equal(s, want)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    assert np.array_equal(eng.text_stats(t(hyp), t(ref), t(hl), t(rl)), want)
    assert eng.text_metrics(hyp, ref, hl, rl) == _host([h for h, _ in cut], [r for _, r in cut])
    # an explicit pairing, whole rows
    idx = np.array([2, 2, 0, 1, 0, 1])
    assert np.array_equal(eng.text_stats(hyp, ref, ref_index=idx), [pair_stats(hyp[p], ref[idx[p]]) for p in range(6)])
    # a transposed view of [T, pairs] rows, read in place through its strides
    tv = t(hyp.T.copy()).t()
    assert not tv.is_contiguous() and np.array_equal(eng.text_stats(tv, ref, hl, rl), want)
    # the [B, T, n] ids of a sampled decode: pair b * n + j is draw j of image b; and a permuted view of rows [B, n, T]
    ids = t(hyp.reshape(3, 2, 12).transpose(0, 2, 1))              # [B = 3, T = 12, n = 2]
    assert np.array_equal(eng.text_stats(ids, ref, hl, rl), want)
    pv = t(hyp.reshape(3, 2, 12)).permute(0, 2, 1)
    assert not pv.is_contiguous() and np.array_equal(eng.text_stats(pv, ref, hl, rl), want)
    # pad_batch_formulas' layout, cut at END with and without the lengths
    f, fl = pad_batch_formulas([[0, 1, 1], [2]], PAD, END)
    assert eng.text_stats(f, f, id_end=END)[:, 8:].tolist() == [[3, 3, 0, 1], [1, 1, 0, 1]]
    assert eng.text_stats(f, f[::-1].copy(), fl, fl[::-1].copy(), id_end=END)[:, 8:].tolist() == [[3, 1, 3, 0], [1, 3, 3, 0]]
    # no pair, no column
    assert eng.text_stats(hyp[:0], ref).shape == (0, 12)
    assert eng.text_stats(hyp[:, :0], ref)[:, 8:].tolist() == [[0, 9, 9, 0]] * 6 and eng.text_stats(hyp, ref[:, :0])[:, 8:].tolist() == [[12, 0, 12, 0]] * 6
    assert eng.text_metrics(hyp[:0], ref) == scores_from_counts([0] * 14)


def test_corpus_accumulates_across_calls(eng):
    rng = np.random.default_rng(4)
    hyp = rng.integers(0, 2, size=(7, 10)).astype(np.int32)
    ref = rng.integers(0, 2, size=(7, 8)).astype(np.int32)
    want = np.array([pair_stats(hyp[p], ref[p]) for p in range(7)], np.int32)
    corpus = torch.zeros(14, dtype=torch.int64)
    s1 = eng.text_stats(hyp[:3], ref[:3], corpus=corpus)
    assert corpus.tolist() == corpus_of(want[:3]).tolist()
    s2 = eng.text_stats(hyp[3:], ref[3:], corpus=corpus)
    assert np.array_equal(np.concatenate([s1, s2]), want) and corpus.tolist() == corpus_of(want).tolist()
    assert scores_from_counts(corpus.numpy()) == _host([list(h) for h in hyp], [list(r) for r in ref]) == eng.text_metrics(hyp, ref)
    eng.text_stats(hyp[:0], ref, corpus=corpus)                     # no pair: untouched
    assert corpus.tolist() == corpus_of(want).tolist()


def test_value_errors_before_any_launch(eng):
    hyp, ref = np.zeros((6, 12), np.int32), np.zeros((3, 9), np.int32)
    wide = np.zeros((3, _abi.LXO_EDIT_MAX_REF + 1), np.int32)
    for bad in (dict(hyp=hyp[0]), dict(ref=ref[0]), dict(hyp=hyp[:5]), dict(hyp_lengths=np.zeros(5)), dict(ref_lengths=np.zeros(2)), dict(ref_index=np.zeros(5)),
                dict(ref_index=np.array([0, 1, 2, 3, 0, 0])), dict(ref=wide), dict(hyp=wide), dict(ref=ref[:0]), dict(hyp=np.zeros((2, 2, 2, 2), np.int32)),
                dict(corpus=np.zeros(14, np.int64)), dict(corpus=torch.zeros(14, dtype=torch.int32)), dict(corpus=torch.zeros(13, dtype=torch.int64))):
        kw = dict(hyp=hyp, ref=ref)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.text_stats(**kw)
    with pytest.raises(ValueError):
        eng.text_metrics(wide, ref)


# ------------------------------------------------------------------------------------------------------------------ the model --
TOKS = ["a", "b", "c", "d", "e", "f", "g", "h"]                       # + _UNK, _PAD, _END: 11 ids


def _write_results_dir(tmp):
    """a results directory and a three-image test set in the reference's on-disk format, small enough for the interpreter"""
    from PIL import Image
    d = str(tmp) + "/results/"
    os.makedirs(d)
    os.makedirs(str(tmp) + "/data/test")
    (tmp / "data" / "vocab.txt").write_text("\n".join(TOKS) + "\n")
    imgs, forms = synthetic.make_set(3, H, W, V, 2, MAX_LEN + 1, seed=9)
    with open(str(tmp) + "/data/test.formulas.txt", "w") as ff, open(str(tmp) + "/data/test.matching.txt", "w") as fm:
        for i, (img, form) in enumerate(zip(imgs, forms)):
            Image.fromarray(np.repeat(img, 3, axis=2)).save(str(tmp) + "/data/test/%d.png" % i)
            ff.write(" ".join(TOKS[t] for t in form) + "\n")
            fm.write("%d.png %d\n" % (i, i))
    json.dump({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp) + "/data/vocab.txt", "min_count_tok": 1}, open(d + "vocab.json", "w"))
    json.dump({"dir_images_test": str(tmp) + "/data/test/", "path_matching_test": str(tmp) + "/data/test.matching.txt",
               "path_formulas_test": str(tmp) + "/data/test.formulas.txt", "max_iter": None, "max_length_formula": MAX_LEN, "bucket_test": True},
              open(d + "data.json", "w"))
    json.dump({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
               "compute_dtype": "f32", "device": "cpu", "max_length_formula": MAX_LEN, "decoding": "greedy"}, open(d + "model.json", "w"))
    return d


@pytest.fixture(scope="module")
def results(tmp_path_factory, lib):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    tmp = tmp_path_factory.mktemp("text_stats")
    d = _write_results_dir(tmp)
    vocab = Vocab(Config(d + "vocab.json"))
    m = Img2SeqModel(Config(d + "model.json"), d, vocab, lib=lib)
    m.build_pred()
    return m, vocab, d


def test_score_ids_equals_score_files_on_the_written_answers(results, tmp_path):
    m, vocab, _ = results
    assert vocab.n_tok == V and vocab.id_end == END
    rng = np.random.default_rng(6)
    seq = lambda n: [int(x) for x in rng.integers(0, 3, size=n)]
    refs = [seq(5), seq(4) + [END, 1, 1], [], [END, 0], seq(6), [], seq(3), seq(70), seq(2), [0, 1, 0, 1, 0, 1, 0]]
    hyps = [list(refs[0]), seq(4), seq(2), seq(3), [END], [], refs[6] + [END, 2], seq(66), [], [0, 1, 0, 1]]
    empties = [(len(truncate_end(r, END)) == 0, len(truncate_end(h, END)) == 0) for r, h in zip(refs, hyps)]
    assert {(True, False), (False, True), (True, True)} <= set(empties)             # an empty reference, an empty hypothesis, both
    files = write_answers(refs, [hyps], vocab.id_to_tok, str(tmp_path) + "/answers/", END)
    want = score_files(files[0], files[1])
    old = m.SCORE_IDS_BATCH
    try:
        for batch in (old, 4):                                      # one batch, and three with one accumulator
            m.SCORE_IDS_BATCH = batch
            got, rows = m.score_ids(refs, hyps, per_sample=True)
            assert got == want and m.score_ids(refs, hyps) == want, (got, want)
            assert rows.shape == (10, 12) and rows.dtype == np.int32
    finally:
        m.SCORE_IDS_BATCH = old
    assert want["ExactMatchScore"] == 30.0 and 0.0 < want["BLEU-4"] < 100.0        # pairs 0, 5 (both empty: one token each) and 6
    both = empties.index((True, True))
    assert rows[both].tolist() == [1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1]              # the quirk: an empty line is ONE token, equal on both sides
    tok = lambda ids: [vocab.id_to_tok[i] for i in truncate_end(ids, END)] or [""]
    assert [r.tolist() for r in rows] == [pair_stats([hash(x) for x in tok(h)], [hash(x) for x in tok(r)]) for r, h in zip(refs, hyps)]
    assert m.score_ids([], []) == scores_from_counts([0] * 14)
    with pytest.raises(ValueError):
        m.score_ids(refs, hyps[:3])


def _stub_the_network(monkeypatch):
    """The wiring is under test, not the network (tests/test_gpu_text_stats.py scores a real decode): the teacher-forced pass and the decode of
    write_prediction are replaced by cheap deterministic functions of the images -- the interpreter needs half a minute per real pass.  Per image
    the "decode" emits the ink-dependent start of a fixed token pattern and END: some hypotheses repeat n-grams, one may be empty."""
    from latex_ocr_amd.engine import Engine
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    calls = []

    def decode(self, img, allowed=None):
        calls.append(len(img))
        out = np.full((len(img), 1, MAX_LEN + 1), END, np.int32)
        for b, im in enumerate(img):
            n = int(np.asarray(im, np.int64).sum()) % (MAX_LEN + 1)
            out[b, 0, :n] = [0, 1, 0][:n]
        return out
    monkeypatch.setattr(Img2SeqModel, "_decode", decode)
    monkeypatch.setattr(Engine, "evaluate_batch", lambda self, img, formula, lengths: (0.5 * float(np.asarray(lengths).sum()), int(np.asarray(lengths).sum())))
    return calls


def test_run_evaluate_and_the_driver_with_and_without_the_flag(results, lib, monkeypatch):
    from latex_ocr_amd.model import img2seq
    from latex_ocr_amd.model.utils.general import Config
    m, vocab, d = results
    sys.path.insert(0, ROOT)
    import evaluate_txt
    from train import make_sets
    calls = _stub_the_network(monkeypatch)
    (test_set,) = make_sets(Config(d + "data.json"), vocab, names=("test",))
    base = {"dir_answers": d + "formulas_val/", "batch_size": 20}
    plain = m._run_evaluate(Config(dict(base)), test_set)
    seen = []
    real = img2seq.score_files
    monkeypatch.setattr(img2seq, "score_files", lambda *a: seen.append(a) or real(*a))
    assert m._run_evaluate(Config(dict(base)), test_set) == plain and len(seen) == 1
    on_dev = m._run_evaluate(Config(dict(base, metrics_on_device=True)), test_set)
    assert len(seen) == 1 and on_dev == plain and set(plain) == {"BLEU-4", "ExactMatchScore", "EditDistance", "perplexity"}      # not through the files
    assert os.path.exists(d + "formulas_val/ref.txt") and os.path.exists(d + "formulas_val/hyp_0.txt")      # which are still written
    assert plain == dict(real(d + "formulas_val/ref.txt", d + "formulas_val/hyp_0.txt"), perplexity=plain["perplexity"])
    # the driver: the same model class over the interpreter's library
    monkeypatch.setattr(evaluate_txt, "Img2SeqModel", lambda cfg, out, voc: img2seq.Img2SeqModel(cfg, out, voc, lib=lib))
    without = evaluate_txt.main(["--results", d])
    with_flag = evaluate_txt.main(["--results", d, "--on-device"])
    assert with_flag == without == plain and calls == [3] * 5
