"""-m gpu: the text-metric counts on the MI355X.

1. lxo_text_stats on the case matrix of tests/text_stats_ref.py through liblxo.so, exactly as the hipsim file: rows and corpus row as integers, with
   and without the rows, accumulated over two halves; twice the same bytes; captured into a graph and replayed.
2. A strided device tensor [B, T, n] read in place through Engine.text_stats.
3. The ids of one real greedy decode of a tiny model (B = 8, 32 x 48, V = 11) scored on the device -- Engine.text_stats / text_metrics and
   Img2SeqModel.score_ids' arithmetic -- against the host functions on the cut lists."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from latex_ocr_amd import _abi
from latex_ocr_amd.engine import _p
from latex_ocr_amd.model.evaluation.text import bleu_score, edit_distance, exact_match_score, scores_from_counts, truncate_end
from text_stats_ref import CASE_NAMES, NC, check_text_case, corpus_of, named, pair_stats, run_text

V, H, W = 11, 32, 48
END, PAD = V - 1, V - 2


class Dev(object):
    """numpy <-> the GPU for the shared runners of tests/text_stats_ref.py"""
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


def _engine(dtype="f32", seed=0):
    """An engine without the encoder's side stream: nothing here trains, and a test module that takes streams from torch's pool moves every
    later module's streams to other hardware queues (tests/test_gpu_xdec.py's foreign-kernel test needs its third stream on a queue of its own)."""
    return with_env("LXO_ENC_OVERLAP", "0", lambda: Engine(V, dtype=dtype, seed=seed))


def _host(hyps, refs):
    return {"BLEU-4": bleu_score(refs, hyps) * 100, "ExactMatchScore": exact_match_score(refs, hyps) * 100, "EditDistance": edit_distance(refs, hyps) * 100}


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel --
@pytest.mark.parametrize("name", CASE_NAMES)
def test_stats_matrix(lib, name):
    c = named(name)
    _, corpus = check_text_case(lib, c, Dev)
    rc, none, alone = run_text(lib, c, Dev, want_stats=False, corpus=np.full(NC, -7, np.int64))      # without the rows: the waves add into the corpus
    assert rc == 0 and none is None and alone.tolist() == corpus.tolist()


def test_accumulate_and_repeat(lib):
    c = named("END, lengths")
    half = c["pairs"] // 2
    for want_stats in (True, False):
        rc, _, co = run_text(lib, c, Dev, want_stats=want_stats, corpus=np.full(NC, 99, np.int64), accumulate=0, hi=half)
        assert rc == 0 and co.tolist() == corpus_of(c["stats"][:half]).tolist()
        rc, _, co = run_text(lib, c, Dev, want_stats=want_stats, corpus=co, accumulate=1, lo=half)
        assert rc == 0 and co.tolist() == c["corpus"].tolist()
    for name in ("wave, ref 513", "limit x limit", "strided [B, T, n]"):
        c = named(name)
        a, b = run_text(lib, c, Dev, corpus=np.zeros(NC, np.int64)), run_text(lib, c, Dev, corpus=np.zeros(NC, np.int64))
        assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), name


def test_the_call_is_captured_into_a_graph():
    """the rows' launch and the reduction, then the zeroing launch and the launch that adds into the corpus itself, on the capturing stream: a replay
    gives the eager call's bytes, and on other ids what the host functions give on them"""
    c = named("wave, ref 129")
    eng = _engine()
    pairs, T = c["pairs"], c["T"]
    hyp = torch.from_numpy(c["hyp"]).cuda().view(pairs, T)
    ref, hl = torch.from_numpy(c["ref"]).cuda(), torch.from_numpy(c["hyp_len"]).cuda()
    args = ("graph", hyp, ref, hl, None, None, None)
    s0, c0 = eng._text_stats_device(*args, True, None, 1)           # eager first
    torch.cuda.synchronize()
    assert np.array_equal(s0.cpu().numpy(), c["stats"]) and c0.cpu().tolist() == c["corpus"].tolist()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s1, c1 = eng._text_stats_device(*args, True, None, 1)
        _, c2 = eng._text_stats_device(*args, False, None, 0)
    g.replay()
    torch.cuda.synchronize()
    assert s1.cpu().numpy().tobytes() == s0.cpu().numpy().tobytes() and c1.cpu().numpy().tobytes() == c0.cpu().numpy().tobytes() == c2.cpu().numpy().tobytes()
    other = np.random.default_rng(2).integers(0, 2, size=(pairs, T)).astype(np.int32)
    hyp.copy_(torch.from_numpy(other).cuda())
    g.replay()
    torch.cuda.synchronize()
    r = [int(x) for x in c["ref"][0]]
    want = np.array([pair_stats(other[p, :c["hyp_len"][p]], r) for p in range(pairs)], np.int32)
    assert np.array_equal(s1.cpu().numpy(), want) and c1.cpu().tolist() == c2.cpu().tolist() == corpus_of(want).tolist()


# ------------------------------------------------------------------------------------------------- 2. / 3. through the engine --
def test_strided_device_ids_are_read_in_place():
    eng = _engine()
    rng = np.random.default_rng(8)
    B, T, n = 3, 70, 4
    buf = torch.from_numpy(rng.integers(0, 3, size=(B, T + 3, n)).astype(np.int32)).cuda()      # (steps a decode did not run lie behind T)
    buf[0, 65, 1] = buf[1, 0, 2] = buf[2, 30, 0] = END
    ids = buf[:, :T]
    assert not ids.is_contiguous()
    refs, rl = pad_batch_formulas([list(rng.integers(0, 3, size=k)) for k in (66, 3, 40)], PAD, END)
    h = ids.cpu().numpy()
    cut = [(truncate_end(h[b, :, j], END), list(refs[b, :rl[b] - 1])) for b in range(B) for j in range(n)]
    want = np.array([pair_stats(x, y) for x, y in cut], np.int32)
    corpus = torch.zeros(NC, dtype=torch.int64, device="cuda")
    assert np.array_equal(eng.text_stats(ids, refs, ref_lengths=rl, id_end=END, corpus=corpus), want)
    assert corpus.cpu().tolist() == corpus_of(want).tolist()
    rows = torch.from_numpy(np.ascontiguousarray(h.transpose(0, 2, 1))).cuda()                 # [B, n, T] rows, as a permuted view
    assert np.array_equal(eng.text_stats(rows.permute(0, 2, 1), refs, ref_lengths=rl, id_end=END), want)
    assert eng.text_metrics(ids, refs, ref_lengths=rl, id_end=END) == _host([x for x, _ in cut], [y for _, y in cut])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_real_greedy_decode_scored_on_the_device(dtype):
    imgs, forms = synthetic.make_set(8, H, W, V, 2, 7, seed=21)
    eng = _engine(dtype, 5)
    assert eng.enc_side is None
    ids = eng.greedy_decode(pad_batch_images(imgs), END, max_iter=9)
    assert ids.shape[0] == 8 and ids.ndim == 2
    refs, rl = pad_batch_formulas(forms, PAD, END)
    hyps = [[int(x) for x in truncate_end(row, END)] for row in ids]
    cut_refs = [[int(x) for x in f] for f in forms]
    want = np.array([pair_stats(h, r) for h, r in zip(hyps, cut_refs)], np.int32)
    got = eng.text_stats(ids, refs, ref_lengths=rl, id_end=END)
    print("%s: decoded lengths %s, reference lengths %s, corpus row %s" % (dtype, want[:, 8].tolist(), want[:, 9].tolist(), corpus_of(want).tolist()))
    assert np.array_equal(got, want)
    assert eng.text_metrics(ids, refs, ref_lengths=rl, id_end=END) == _host(hyps, cut_refs) == scores_from_counts(corpus_of(want))
