"""-m gpu: the edit alignment on the MI355X.

1. lxo_edit_align on the case matrix of tests/edit_align_ref.py through liblxo.so, exactly as the hipsim file: maps, counts, corpus row and confusion
   matrix as integers between guard words, the validity checks; accumulated over two halves; twice the same bytes; captured into a graph and replayed
   on other ids.
2. A strided device tensor [B, T, n] read in place through Engine.edit_align.
3. The ids of one real greedy decode of a tiny model (B = 8, 32 x 48, V = 11) through Engine.edit_align and Img2SeqModel.error_analysis' arithmetic
   against the host align."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from latex_ocr_amd import _abi
from latex_ocr_amd.engine import _p
from latex_ocr_amd.model.evaluation.text import align, error_report, truncate_end
from edit_align_ref import CASE_NAMES, NC, align_ref, check_align_case, confusion_of, corpus_of, named, run_align

V, H, W = 11, 32, 48
END, PAD = V - 1, V - 2


class Dev(object):
    """numpy <-> the GPU for the shared runner of tests/edit_align_ref.py"""
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
    """An engine without the encoder's side stream, as tests/test_gpu_text_stats.py builds it (and for its reason)."""
    return with_env("LXO_ENC_OVERLAP", "0", lambda: Engine(V, dtype=dtype, seed=seed))


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel --
@pytest.mark.parametrize("name", CASE_NAMES)
def test_alignment_matrix(lib, name):
    check_align_case(lib, named(name), Dev)


def test_accumulate_and_repeat(lib):
    c = named("END, lengths")
    half, nconf = c["pairs"] // 2, (c["V"] + 1) ** 2
    conf1, out1 = confusion_of(c["cut"][:half], c["maps"][:half], c["V"])
    for want in (("hyp_align", "ref_align", "counts"), ()):
        rc, a = run_align(lib, c, Dev, want=want, corpus=np.full(NC, 99, np.int64), confusion=np.full(nconf, 99, np.int64), accumulate=0, hi=half)
        assert rc == 0 and a["corpus"].tolist() == corpus_of(c["counts"][:half], out1).tolist() and a["confusion"].tolist() == conf1.tolist()
        rc, b = run_align(lib, c, Dev, want=want, corpus=a["corpus"], confusion=a["confusion"], accumulate=1, lo=half)
        assert rc == 0 and b["corpus"].tolist() == c["corpus"].tolist() and b["confusion"].tolist() == c["confusion"].tolist()
    for name in ("ref 513", "limit x limit", "strided [B, T, n]", "exhaustive small"):
        c = named(name)
        nconf = (c["V"] + 1) ** 2
        a = run_align(lib, c, Dev, corpus=np.zeros(NC, np.int64), confusion=np.zeros(nconf, np.int64))
        b = run_align(lib, c, Dev, corpus=np.zeros(NC, np.int64), confusion=np.zeros(nconf, np.int64))
        assert a[0] == b[0] == 0 and all(a[1][k].tobytes() == b[1][k].tobytes() for k in a[1]), name


def test_the_call_is_captured_into_a_graph():
    """the zeroing and the pair launch on the capturing stream, with and without the per-pair outputs: a replay gives the eager call's bytes, and on
    other ids what the table reference gives on them"""
    c = named("ref 129")
    eng = _engine()
    pairs, T = c["pairs"], c["T"]
    hyp = torch.from_numpy(c["hyp"]).cuda().view(pairs, T)
    ref, hl = torch.from_numpy(c["ref"]).cuda(), torch.from_numpy(c["hyp_len"]).cuda()
    args = ("graph", hyp, ref, hl, None, None, None)
    conf = lambda: torch.zeros(c["V"] + 1, c["V"] + 1, dtype=torch.int64, device="cuda")
    e = eng._edit_align_device(*args, True, True, True, conf())     # eager first (it sizes the cached scratch)
    torch.cuda.synchronize()
    assert np.array_equal(e[0].cpu().numpy(), c["hyp_align"]) and np.array_equal(e[2].cpu().numpy(), c["counts"]) and e[3].cpu().tolist() == c["corpus"].tolist()
    co1, cf1, co2 = torch.zeros(NC, dtype=torch.int64, device="cuda"), conf(), torch.zeros(NC, dtype=torch.int64, device="cuda")
    co3, cf3 = torch.full((NC,), 99, dtype=torch.int64, device="cuda"), torch.full_like(cf1, 99)      # overwritten by the call itself (accumulate = 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        co1.zero_(); cf1.zero_(); co2.zero_()
        g1 = eng._edit_align_device(*args, True, True, co1, cf1)
        eng._edit_align_device(*args, False, False, co2, None)
        eng._ck(eng.lib.lxo_edit_align(_p(hyp), 1, T, 0, 1, T, _p(hl), _p(ref), 1, int(ref.shape[1]), None, None, pairs, pairs, -1, None, None, None, _p(co3), _p(cf3),
                                       c["V"], 0, _p(eng._align_scratch), eng._align_scratch.numel(), eng._stream()), "edit_align")
    g.replay()
    torch.cuda.synchronize()
    assert co3.cpu().tolist() == c["corpus"].tolist() and cf3.reshape(-1).cpu().tolist() == c["confusion"].tolist()
    g.replay()                                                      # overwritten again, not added to
    torch.cuda.synchronize()
    assert co3.cpu().tolist() == c["corpus"].tolist() and cf3.reshape(-1).cpu().tolist() == c["confusion"].tolist()
    for k in range(3):
        assert g1[k].cpu().numpy().tobytes() == e[k].cpu().numpy().tobytes(), k
    assert co1.cpu().tolist() == c["corpus"].tolist() and cf1.reshape(-1).cpu().tolist() == c["confusion"].tolist() and co2.cpu().tolist() == c["corpus"][:7].tolist() + [0]
    other = np.random.default_rng(2).integers(0, 2, size=(pairs, T)).astype(np.int32)
    hyp.copy_(torch.from_numpy(other).cuda())
    g.replay()
    torch.cuda.synchronize()
    r = [int(x) for x in c["ref"][0]]
    cut = [([int(x) for x in other[p, :c["hyp_len"][p]]], r) for p in range(pairs)]
    maps = [align_ref(h, r) for h, r in cut]
    counts = np.array([m[2] for m in maps], np.int32)
    conf2, out = confusion_of(cut, [(a, b) for a, b, _ in maps], c["V"])
    assert np.array_equal(g1[2].cpu().numpy(), counts) and co1.cpu().tolist() == corpus_of(counts, out).tolist() and cf1.reshape(-1).cpu().tolist() == conf2.tolist()
    assert co3.cpu().tolist() == co1.cpu().tolist() and torch.equal(cf3, cf1)
    ha = g1[0].cpu().numpy()
    assert all(ha[p, :len(m[0])].tolist() == m[0] and (ha[p, len(m[0]):] == -2).all() for p, m in enumerate(maps))


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
    cut = [([int(x) for x in truncate_end(h[b, :, j], END)], [int(x) for x in refs[b, :rl[b] - 1]]) for b in range(B) for j in range(n)]
    maps = [align_ref(x, y) for x, y in cut]
    al = eng.edit_align(ids, refs, ref_lengths=rl, id_end=END, corpus=True, confusion=True)
    assert np.array_equal(al.counts, [m[2] for m in maps])
    for p, (ha, ra, _) in enumerate(maps):
        assert al.hyp_align[p].tolist() == ha + [-2] * (T - len(ha)) and al.ref_align[p].tolist() == ra + [-2] * (refs.shape[1] - len(ra)), p
    conf, out = confusion_of(cut, [(a, b) for a, b, _ in maps], V)
    assert al.corpus.cpu().tolist() == corpus_of(al.counts, out).tolist() and al.confusion.reshape(-1).cpu().tolist() == conf.tolist()
    rows = torch.from_numpy(np.ascontiguousarray(h.transpose(0, 2, 1))).cuda()                 # [B, n, T] rows, as a permuted view
    al2 = eng.edit_align(rows.permute(0, 2, 1), refs, ref_lengths=rl, id_end=END)
    assert np.array_equal(al2.hyp_align, al.hyp_align) and np.array_equal(al2.ref_align, al.ref_align) and np.array_equal(al2.counts, al.counts)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_real_greedy_decode_aligned_on_the_device(dtype):
    imgs, forms = synthetic.make_set(8, H, W, V, 2, 7, seed=21)
    eng = _engine(dtype, 5)
    ids = eng.greedy_decode(pad_batch_images(imgs), END, max_iter=9)
    assert ids.shape[0] == 8 and ids.ndim == 2
    refs, rl = pad_batch_formulas(forms, PAD, END)
    hyps = [[int(x) for x in truncate_end(row, END)] for row in ids]
    cut_refs = [[int(x) for x in f] for f in forms]
    host = [align(h, r) for h, r in zip(hyps, cut_refs)]
    al = eng.edit_align(ids, refs, ref_lengths=rl, id_end=END, corpus=True, confusion=True)
    print("%s: decoded lengths %s, reference lengths %s, counts %s" % (dtype, al.counts[:, 4].tolist(), al.counts[:, 5].tolist(), al.counts[:, :4].sum(0).tolist()))
    assert np.array_equal(al.counts, [c for _, _, c in host])
    for p, (ha, ra, _) in enumerate(host):
        assert al.hyp_align[p, :len(ha)].tolist() == ha and al.ref_align[p, :len(ra)].tolist() == ra
        assert (al.hyp_align[p, len(ha):] == -2).all() and (al.ref_align[p, len(ra):] == -2).all()
    # error_analysis' arithmetic: its padded sides through the same device call, one corpus row and one matrix, against the host loop's report
    sides = []
    for seqs in (hyps, cut_refs):
        ln = np.array([len(s) for s in seqs], np.int32)
        a = np.zeros((len(seqs), max(int(ln.max()), 1)), np.int32)
        for i, s in enumerate(seqs):
            a[i, :len(s)] = s
        sides += [a, ln]
    _, _, _, corpus, confusion = eng._edit_align_device("error_analysis", sides[0], sides[2], sides[1], sides[3], None, None, False, False, True, True)
    conf, out = confusion_of(list(zip(hyps, cut_refs)), [(a, b) for a, b, _ in host], V)
    want = error_report(corpus_of([c for _, _, c in host], out), conf, {}, 20)
    assert error_report(corpus.cpu().numpy(), confusion.cpu().numpy(), {}, 20) == want == error_report(al.corpus.cpu().numpy(), al.confusion.cpu().numpy(), {}, 20)
    assert want["pairs"] == 8 and want["left_out"] == 0
