"""CPU (hipsim): the edit alignment through the Python layers -- model/evaluation/text.py's align against the table reference of
tests/edit_align_ref.py on the whole matrix, error_report's rankings and tie rule on a hand-made matrix, Engine.edit_align (host and device inputs,
views read in place, the accumulators, the ValueErrors), Img2SeqModel.error_analysis against a host loop over align across two batches, and
evaluate_txt.py --errors."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi
from latex_ocr_amd.engine import Alignment, Engine
from latex_ocr_amd.model.evaluation.text import align, error_report, format_error_report, truncate_end
from latex_ocr_amd.model.utils.text import pad_batch_formulas
from simlib import SIM_SO, build_sim
from edit_align_ref import align_cases, align_ref, confusion_of, corpus_of
from test_engine_text_stats_sim import END, PAD, ROOT, SMALL, V, MAX_LEN, _stub_the_network, _write_results_dir


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.fixture(scope="module")
def eng(lib):
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=MAX_LEN + 2)


def test_host_align_equals_the_table_reference_on_the_matrix():
    n = 0
    for c in align_cases():
        for (h, r), (ha, ra), counts in zip(c["cut"], c["maps"], c["counts"]):
            if len(h) * len(r) > 200000:                            # (the plain-Python loop on limit x limit takes seconds; the kernel is held to it above)
                continue
            assert align(h, r) == (ha, ra, counts.tolist()), (c["name"], h, r)
            n += 1
    assert n > 1100
    assert align([], []) == ([], [], [0] * 6) and align([1], []) == ([-1], [], [0, 0, 1, 0, 1, 0]) and align(iter([1]), (1,)) == ([0], [0], [1, 0, 0, 0, 1, 1])
    # the rule on a tie: "ab" against "b" keeps b and inserts a; "a" against "aa" pairs the LAST a (the walk starts at the end)
    assert align([0, 1], [1]) == ([-1, 0], [1], [1, 0, 1, 0, 2, 1]) and align([0], [0, 0]) == ([1], [-1, 0], [1, 0, 0, 1, 1, 2])


def test_error_report_rankings_and_ties():
    Vr = 4
    C = np.zeros((Vr + 1, Vr + 1), np.int64)
    C[0, 0], C[1, 1], C[2, 2], C[3, 3] = 6, 3, 3, 0
    C[0, 1] = 2
    C[1, 0] = 2                                                     # ties with [0][1]: the lower reference id first
    C[2, 3] = 5
    C[1, 2] = 2                                                     # ties again: [1][0] before [1][2]
    C[3, 0] = 1
    C[0, Vr], C[2, Vr], C[1, Vr] = 1, 4, 1                          # deleted: 2 first, then 0 before 1
    C[Vr, 3], C[Vr, 1] = 2, 2                                       # inserted: 1 before 3
    corpus = [12, 12, 4, 6, 28, 30, 5, 3]
    rev = {0: "a", 1: "b", 2: "c"}                                  # id 3 has no name: shown as its number
    rep = error_report(corpus, C.reshape(-1), rev, top=3)
    assert rep["confusions"] == [("c", "3", 5), ("a", "b", 2), ("b", "a", 2)]
    assert rep["deleted"] == [("c", 4), ("a", 1), ("b", 1)] and rep["inserted"] == [("b", 2), ("3", 2)]
    assert rep["recall"] == [("3", 0.0, 1), ("c", 0.25, 12), ("b", 0.375, 8)]
    assert [rep[k] for k in ("matches", "substitutions", "insertions", "deletions", "hyp_tokens", "ref_tokens", "pairs", "left_out")] == corpus
    assert rep["SubRate"] == 40.0 and rep["InsRate"] == 100.0 * 4 / 30.0 and rep["DelRate"] == 20.0
    full = error_report(corpus, C, ["a", "b", "c"])                 # a list for a vocabulary, the matrix as [V + 1, V + 1], no cut
    assert full["confusions"] == [("c", "3", 5), ("a", "b", 2), ("b", "a", 2), ("b", "c", 2), ("3", "a", 1)] and len(full["recall"]) == 4
    assert error_report(corpus, C, rev, top=0)["confusions"] == []
    assert error_report([0] * 8, [0] * 4, {})["SubRate"] == 0.0
    text = format_error_report(rep)
    assert "SubRate 40.00" in text and "  c -> 3  5\n" in text and "  c  4\n" in text
    for bad in (dict(corpus=[0] * 7), dict(confusion=[0] * 5), dict(confusion=[0])):
        kw = dict(corpus=corpus, confusion=C, rev_vocab=rev)
        kw.update(bad)
        with pytest.raises(ValueError):
            error_report(**kw)


def _want(cut, Vc):
    maps = [align_ref(h, r) for h, r in cut]
    conf, out = confusion_of(cut, [(a, b) for a, b, _ in maps], Vc)
    counts = np.array([c for _, _, c in maps], np.int32).reshape(len(cut), 6)
    return maps, counts, corpus_of(counts, out), conf


def _maps_equal(al, maps, T, Tr):
    for p, (ha, ra, _) in enumerate(maps):
        assert al.hyp_align[p].tolist() == ha + [-2] * (T - len(ha)) and al.ref_align[p].tolist() == ra + [-2] * (Tr - len(ra)), p


def test_edit_align_takes_arrays_tensors_and_views(eng):
    rng = np.random.default_rng(3)
    hyp = rng.integers(0, 3, size=(6, 12)).astype(np.int32)
    ref = rng.integers(0, 3, size=(3, 9)).astype(np.int32)
    hl, rl = np.array([12, 0, 5, 7, 12, 1]), np.array([9, 4, 0])
    cut = [(list(hyp[p, :hl[p]]), list(ref[p // 2, :rl[p // 2]])) for p in range(6)]
    maps, counts, corpus, conf = _want(cut, V)
    al = eng.edit_align(hyp, ref, hl, rl, corpus=True, confusion=True)
    assert isinstance(al, Alignment) and al.hyp_align.dtype == al.ref_align.dtype == al.counts.dtype == np.int32
    assert al.hyp_align.shape == (6, 12) and al.ref_align.shape == (6, 9) and np.array_equal(al.counts, counts)
    _maps_equal(al, maps, 12, 9)
    assert al.corpus.dtype == torch.int64 and al.corpus.tolist() == corpus.tolist() and al.confusion.shape == (V + 1, V + 1)
    assert al.confusion.reshape(-1).tolist() == conf.tolist()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    al2 = eng.edit_align(t(hyp), t(ref), t(hl), t(rl))
    assert al2.corpus is None and al2.confusion is None and np.array_equal(al2.hyp_align, al.hyp_align) and np.array_equal(al2.ref_align, al.ref_align)
    # without the maps; a second call adds into the accumulators of the first
    al3 = eng.edit_align(hyp, ref, hl, rl, corpus=al.corpus, confusion=al.confusion, return_maps=False)
    assert al3.hyp_align is None and al3.ref_align is None and np.array_equal(al3.counts, counts)
    assert al3.corpus is al.corpus and al.corpus.tolist() == (2 * corpus).tolist() and al.confusion.reshape(-1).tolist() == (2 * conf).tolist()
    # a smaller matrix of the caller's: tokens outside it are counted, left out and reported
    small = torch.zeros(3, 3, dtype=torch.int64)
    al4 = eng.edit_align(hyp, ref, hl, rl, corpus=True, confusion=small)
    _, _, corpus2, conf2 = _want(cut, 2)
    assert small.reshape(-1).tolist() == conf2.tolist() and al4.corpus.tolist() == corpus2.tolist() and corpus2[7] > 0
    # an explicit pairing, whole rows
    idx = np.array([2, 2, 0, 1, 0, 1])
    maps5 = [align_ref(hyp[p], ref[idx[p]]) for p in range(6)]
    _maps_equal(eng.edit_align(hyp, ref, ref_index=idx), maps5, 12, 9)
    # a transposed view of [T, pairs] rows, the [B, T, n] ids of a sampled decode and a permuted view of rows [B, n, T]: read in place
    tv = t(hyp.T.copy()).t()
    assert not tv.is_contiguous()
    _maps_equal(eng.edit_align(tv, ref, hl, rl), maps, 12, 9)
    _maps_equal(eng.edit_align(t(hyp.reshape(3, 2, 12).transpose(0, 2, 1)), ref, hl, rl), maps, 12, 9)
    pv = t(hyp.reshape(3, 2, 12)).permute(0, 2, 1)
    assert not pv.is_contiguous()
    _maps_equal(eng.edit_align(pv, ref, hl, rl), maps, 12, 9)
    # pad_batch_formulas' layout, cut at END
    f, fl = pad_batch_formulas([[0, 1, 1], [2]], PAD, END)
    al6 = eng.edit_align(f, f[::-1].copy(), fl, fl[::-1].copy(), id_end=END)
    assert al6.counts.tolist() == [[0, 1, 2, 0, 3, 1], [0, 1, 0, 2, 1, 3]] and al6.hyp_align[0].tolist() == [-1, -1, 0, -2]
    # no pair, no column
    e = eng.edit_align(hyp[:0], ref)
    assert e.counts.shape == (0, 6) and e.hyp_align.shape == (0, 12) and e.ref_align.shape == (0, 9)
    e = eng.edit_align(hyp[:, :0], ref)
    assert e.counts.tolist() == [[0, 0, 0, 9, 0, 9]] * 6 and e.hyp_align.shape == (6, 0) and (e.ref_align == -1).all()
    e = eng.edit_align(hyp, ref[:, :0])
    assert e.counts.tolist() == [[0, 0, 12, 0, 12, 0]] * 6 and e.ref_align.shape == (6, 0) and (e.hyp_align == -1).all()


def test_value_errors_before_any_launch(eng):
    hyp, ref = np.zeros((6, 12), np.int32), np.zeros((3, 9), np.int32)
    wide = np.zeros((3, _abi.LXO_EDIT_MAX_REF + 1), np.int32)
    for bad in (dict(hyp=hyp[0]), dict(ref=ref[0]), dict(hyp=hyp[:5]), dict(hyp_lengths=np.zeros(5)), dict(ref_lengths=np.zeros(2)), dict(ref_index=np.zeros(5)),
                dict(ref_index=np.array([0, 1, 2, 3, 0, 0])), dict(ref=wide), dict(hyp=wide), dict(ref=ref[:0]), dict(corpus=np.zeros(8, np.int64)),
                dict(corpus=torch.zeros(8, dtype=torch.int32)), dict(corpus=torch.zeros(14, dtype=torch.int64)), dict(confusion=torch.zeros(4, 5, dtype=torch.int64)),
                dict(confusion=torch.zeros(1, 1, dtype=torch.int64)), dict(confusion=torch.zeros(4, 4, dtype=torch.int32)), dict(confusion=np.zeros((4, 4), np.int64))):
        kw = dict(hyp=hyp, ref=ref)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.edit_align(**kw)


# ------------------------------------------------------------------------------------------------------------------ the model --
@pytest.fixture(scope="module")
def results(tmp_path_factory, lib):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    tmp = tmp_path_factory.mktemp("edit_align")
    d = _write_results_dir(tmp)
    vocab = Vocab(Config(d + "vocab.json"))
    m = Img2SeqModel(Config(d + "model.json"), d, vocab, lib=lib)
    m.build_pred()
    return m, vocab, d


def _host_loop(vocab, refs, hyps, top=20):
    """error_analysis on the host: align pair by pair, the sums, error_report"""
    Vv = vocab.n_tok
    cut = [(truncate_end([int(x) for x in h], vocab.id_end), truncate_end([int(x) for x in r], vocab.id_end)) for r, h in zip(refs, hyps)]
    al = [align(h, r) for h, r in cut]
    conf, out = confusion_of(cut, [(a, b) for a, b, _ in al], Vv)
    counts = np.array([c for _, _, c in al], np.int32).reshape(len(cut), 6)
    return error_report(corpus_of(counts, out), conf, vocab.id_to_tok, top), counts, [a for a, _, _ in al], [b for _, b, _ in al]


def test_error_analysis_equals_the_host_loop_across_two_batches(results, monkeypatch):
    m, vocab, _ = results
    assert vocab.n_tok == V and vocab.id_end == END
    rng = np.random.default_rng(12)
    seq = lambda n: [int(x) for x in rng.integers(0, 4, size=n)]
    refs = [seq(int(rng.integers(0, 12))) for _ in range(37)] + [[], [END, 0], seq(70)]
    hyps = [(r[:] if k % 5 == 0 else seq(int(rng.integers(0, 12)))) for k, r in enumerate(refs[:37])] + [[], seq(3), seq(66)]
    hyps[3] = []                                                    # an empty hypothesis: its reference is all deletions
    refs[4], hyps[4] = refs[4] + [END, 1, 1], hyps[4] + [END, 2]    # what lies behind END is not aligned
    want = _host_loop(vocab, refs, hyps)
    calls = []
    real = Engine._edit_align_device
    monkeypatch.setattr(Engine, "_edit_align_device", lambda self, *a: calls.append(1) or real(self, *a))
    monkeypatch.setattr(type(m), "SCORE_IDS_BATCH", 25)
    got = m.error_analysis(refs, hyps, per_sample=True)
    assert len(calls) == 2                                          # 40 pairs: two batches, one accumulator
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3]
    assert m.error_analysis(refs, hyps) == want[0] and len(calls) == 4
    rep = got[0]
    assert rep["pairs"] == 40 and rep["left_out"] == 0 and rep["matches"] + rep["substitutions"] + rep["deletions"] == rep["ref_tokens"]
    assert got[1][37].tolist() == [0] * 6 and got[2][37] == [] and got[1][3, 3] == len(refs[3])       # an empty sequence is empty (no empty-line quirk)
    assert m.error_analysis(refs, hyps, top=2)["confusions"] == want[0]["confusions"][:2]
    none = m.error_analysis([], [], per_sample=True)
    assert none[0]["pairs"] == 0 and none[0]["confusions"] == [] and none[1].shape == (0, 6) and none[2] == [] and none[3] == []
    with pytest.raises(ValueError):
        m.error_analysis(refs, hyps[:3])


def test_the_driver_writes_the_report(results, lib, monkeypatch, tmp_path):
    from latex_ocr_amd.model import img2seq
    m, vocab, d = results
    sys.path.insert(0, ROOT)
    import evaluate_txt
    _stub_the_network(monkeypatch)
    monkeypatch.setattr(evaluate_txt, "Img2SeqModel", lambda cfg, out, voc: img2seq.Img2SeqModel(cfg, out, voc, lib=lib))
    seen = []
    real = img2seq.Img2SeqModel.error_analysis
    monkeypatch.setattr(img2seq.Img2SeqModel, "error_analysis", lambda self, refs, hyps, **kw: seen.append((refs, hyps)) or real(self, refs, hyps, **kw))
    without = evaluate_txt.main(["--results", d])
    assert not seen
    path = str(tmp_path / "errors.txt")
    assert evaluate_txt.main(["--results", d, "--errors", path]) == without and len(seen) == 1
    refs, hyps = seen[0]
    want = _host_loop(vocab, refs, hyps)[0]
    assert open(path).read() == format_error_report(want) and want["pairs"] == 3 and want["ref_tokens"] > 0
    assert evaluate_txt.main(["--results", d, "--errors", path, "--on-device"]) == without and open(path).read() == format_error_report(want)
