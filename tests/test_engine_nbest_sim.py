"""CPU (hipsim): the beam finished on the device, through the Python layers -- Engine.beam_decode(return_nbest=True) against the host route on the same
ids / parents / scores (utils/text.beam_backtrace, the END cut, np.diff: exact for the integers, bit for bit for the log-probs), its consensus
against tests/consensus_ref.py with the posterior as weights, its coverage penalty against coverage summed on the host from return_attention's maps,
the combinations with prefix / allowed / grammar, Engine.beam_finalize on arrays and strided tensors, the refusals, Img2SeqModel.nbest_batch and
predict.py's argument checks.  f32, 32 x 48, V = 11, beam 3, max_iter 4 .. 6."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import BeamPaths, Engine, NBest
from latex_ocr_amd.grammar import Grammar
from latex_ocr_amd.model.utils.image import encoder_out_hw, pad_batch_images
from latex_ocr_amd.model.utils.text import beam_backtrace, beam_parent_rows, beam_slots
from simlib import SIM_SO, build_sim
from beam_finalize_ref import finalize_reference, make_case, post_bound, rerank_reference, score_bound, stable_order
from consensus_ref import check_against_host

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, H, W = 11, 32, 48
END, K = 10, 3
CLS = np.array([1, -1, 2, -2, 1, -1, 0, 0, 0, 0, 0], np.int8)       # 0, 4 open kind 1; 1, 5 close it; 2 / 3 open / close kind 2


@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


@pytest.fixture(scope="module")
def eng(lib):
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=7)


def _images(n=2):
    imgs, _ = synthetic.make_set(n, H, W, V, 2, 4, seed=9)
    return pad_batch_images(imgs)


def host_route(ids, par, sc):
    """what the host does today: the back-trace of ids and scores, the END cut, the differences -> BeamPaths' five arrays"""
    B, n, k = ids.shape
    hyp, run = beam_backtrace(ids, par), beam_backtrace(sc, par)
    hit = hyp == END
    ln = np.where(hit.any(1), hit.argmax(1) + 1, n).astype(np.int32)
    live = np.arange(n)[None, :, None] < ln[:, None, :]
    tok = np.where(live, np.diff(run, axis=1, prepend=np.float32(0)), np.float32(0)).astype(np.float32)
    seq = np.take_along_axis(run, (ln - 1)[:, None, :], axis=1)[:, 0]
    src = beam_parent_rows(par).transpose(1, 0, 2).reshape(n, B * k).astype(np.int32)
    return np.where(live, hyp, END).astype(np.int32), ln, src, tok, seq


def check_nbest(nb, ids, par, sc, alpha=0.0):
    hyp, ln, _, tok, seq = host_route(ids, par, sc)
    assert isinstance(nb, NBest) and np.array_equal(nb.hyp, hyp) and nb.hyp.dtype == np.int32 and np.array_equal(nb.lengths, ln)
    assert nb.tok_logp.tobytes() == tok.tobytes() and nb.seq_logp.tobytes() == np.ascontiguousarray(seq).tobytes()
    ref, post, cp = rerank_reference(ln, seq, None, 0, alpha, 0.0, 1.0)
    assert (np.abs(nb.score - ref) <= score_bound(seq, ln, cp, alpha, 0.0)).all() and (np.abs(nb.post - post) <= post_bound(post)).all()
    assert np.array_equal(nb.order, stable_order(nb.score))
    if alpha == 0.0:
        assert nb.score.tobytes() == nb.seq_logp.tobytes()


@pytest.mark.parametrize("max_iter", [4, 6])
def test_nbest_is_the_host_route_on_the_same_decode(eng, max_iter):
    img = _images()
    ids, par, sc = eng.beam_decode(img, END, K, max_iter=max_iter, return_scores=True)
    out = eng.beam_decode(img, END, K, max_iter=max_iter, return_scores=True, return_nbest=True)
    assert len(out) == 4 and all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(out[:3], (ids, par, sc)))
    check_nbest(out[3], ids, par, sc)
    want = finalize_reference(ids, par, sc, ids.shape[1], K, END)   # and the definition itself
    assert np.array_equal(out[3].hyp, want["hyp"]) and out[3].tok_logp.tobytes() == want["tok_logp"].tobytes()
    # the leading outputs are those of the call without the flag, whatever it returns
    plain = eng.beam_decode(img, END, K, max_iter=max_iter)
    two = eng.beam_decode(img, END, K, max_iter=max_iter, return_nbest=True, length_penalty=0.6)
    assert isinstance(plain, np.ndarray) and len(two) == 2 and two[0].tobytes() == plain.tobytes() == ids.tobytes()
    check_nbest(two[1], ids, par, sc, alpha=0.6)
    wp = eng.beam_decode(img, END, K, max_iter=max_iter, return_parents=True, return_nbest=True)
    assert len(wp) == 3 and wp[1].tobytes() == par.tobytes() and wp[2].hyp.tobytes() == out[3].hyp.tobytes()


def test_the_consensus_over_the_beam(eng):
    img = _images()
    out = eng.beam_decode(img, END, K, max_iter=6, return_nbest=True, return_consensus=True)
    assert len(out) == 4
    nb, best, risk = out[1:]
    d = check_against_host(nb.hyp, END, best, risk, weights=nb.post)
    assert (d > 0).any()                                            # the hypotheses of an image differ somewhere
    b2, r2 = eng.consensus(nb.hyp, END, weights=nb.post)
    assert b2.tolist() == best.tolist() and r2.tobytes() == risk.tobytes()
    bleu = eng.beam_decode(img, END, K, max_iter=6, return_nbest=True, return_consensus=True, consensus_cost="bleu")
    b3, r3 = eng.consensus(nb.hyp, END, weights=nb.post, cost="bleu")
    assert bleu[2].tolist() == b3.tolist() and bleu[3].tobytes() == r3.tobytes() and bleu[1].hyp.tobytes() == nb.hyp.tobytes()


def test_the_coverage_penalty_reads_the_back_traced_maps(eng):
    img = _images()
    alpha_, beta, floor = 0.6, 0.3, 0.05
    ids, par, maps, sc = eng.beam_decode(img, END, K, max_iter=6, return_attention=True, return_scores=True)
    out = eng.beam_decode(img, END, K, max_iter=6, return_attention=True, return_scores=True, return_nbest=True, length_penalty=alpha_,
                          coverage_penalty=beta, cov_floor=floor)
    assert len(out) == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(out[:4], (ids, par, maps, sc)))
    nb = out[4]
    hyp, ln, _, tok, seq = host_route(ids, par, sc)
    assert np.array_equal(nb.hyp, hyp) and nb.seq_logp.tobytes() == np.ascontiguousarray(seq).tobytes()
    B, n = ids.shape[:2]
    Hp, Wp = encoder_out_hw(H, W)
    slots = beam_slots(par)
    cov = np.zeros((B, K, Hp * Wp), np.float32)
    for b in range(B):
        for i in range(K):
            for t in range(int(ln[b, i])):                          # ascending step, one f32 accumulator: attention_locate's coverage
                cov[b, i] += maps[b, t, par[b, t, slots[b, t, i]]].reshape(-1)
    ref, post, cp = rerank_reference(ln, seq, cov.reshape(B * K, -1), Hp * Wp, alpha_, beta, floor)
    assert (cp < 0).all() and (np.abs(nb.score - ref) <= score_bound(seq, ln, cp, alpha_, beta)).all()
    assert np.array_equal(nb.order, stable_order(nb.score)) and (np.abs(nb.post - post) <= post_bound(post)).all()
    # with the boxes: the device-built src gives what the host-built one gives, and the Locations stay last
    host = eng.beam_decode(img, END, K, max_iter=6, return_boxes=True, coverage=True)
    both = eng.beam_decode(img, END, K, max_iter=6, return_boxes=True, coverage=True, return_nbest=True, coverage_penalty=beta, cov_floor=floor)
    assert len(host) == 3 and len(both) == 4 and both[2].score.tobytes() == eng.beam_decode(img, END, K, max_iter=6, return_nbest=True, coverage_penalty=beta,
                                                                                            cov_floor=floor)[1].score.tobytes()
    for x, y in zip(host[2], both[3]):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(both[3].coverage.reshape(B, K, -1), cov)


def test_nbest_combines_with_prefix_allowed_and_grammar(eng):
    img = _images()
    g = Grammar(CLS, max_depth=2, budget=True, id_end=END)
    al = np.ones((2, V), bool)
    al[0, [6, 8]] = False
    al[1, 7] = False
    prefix, lens = np.array([[0, 2, 3, 0, 0, 0], [0] * 6], np.int32), np.array([3, 0], np.int32)
    for kw in (dict(prefix=prefix, prefix_lengths=lens), dict(allowed=al), dict(grammar=g), dict(grammar=g, allowed=al, prefix=prefix, prefix_lengths=lens)):
        ids, par, sc = eng.beam_decode(img, END, K, max_iter=6, return_scores=True, **kw)
        out = eng.beam_decode(img, END, K, max_iter=6, return_scores=True, return_nbest=True, return_consensus=True, **kw)
        assert len(out) == 6 and all(a.tobytes() == b.tobytes() for a, b in zip(out[:3], (ids, par, sc))), sorted(kw)
        check_nbest(out[3], ids, par, sc)
        check_against_host(out[3].hyp, END, out[4], out[5], weights=out[3].post)
        if "grammar" in kw:
            assert all(g.check(out[3].hyp[b, :, i], END) for b in range(2) for i in range(K))
        if "prefix" in kw:
            assert (out[3].hyp[0, :3] == prefix[0, :3, None]).all()
        if "allowed" in kw and "prefix" not in kw:
            assert not np.isin(out[3].hyp[0], [6, 8]).any() and not (out[3].hyp[1] == 7).any()
    dep = eng.beam_decode(img, END, K, max_iter=6, grammar=g, return_depth=True, return_nbest=True)
    assert len(dep) == 4 and isinstance(dep[3], NBest) and dep[2].dtype == np.int32


def test_beam_finalize_takes_arrays_tensors_and_views(eng):
    c = make_case("engine", 3, 5, 9, 12, "random", "mixed", 21)
    w, E = c["want"], c["id_end"]                                  # (the reference cases' own END)

    def same(got):
        assert isinstance(got, BeamPaths)
        for name, a in zip(("hyp", "len", "src", "tok_logp", "seq_logp"), got):
            assert (a is None and name in ("tok_logp", "seq_logp")) or a.tobytes() == w[name].tobytes(), name
    same(eng.beam_finalize(c["ids"], c["parents"], c["scores"], id_end=E, steps=9))
    same(eng.beam_finalize(c["ids"][:, :9], c["parents"][:, :9], c["scores"][:, :9], id_end=E))
    got = eng.beam_finalize(c["ids"], c["parents"], id_end=E, steps=9)
    assert got.tok_logp is None and got.seq_logp is None
    same(got)
    # slices of the decode buffers: read in place, ld_t = the buffer's steps
    t = [torch.from_numpy(c[n].copy()) for n in ("ids", "parents", "scores")]
    views = [x[:, :9] for x in t]
    assert not views[0].is_contiguous()
    same(eng.beam_finalize(*views, id_end=E))
    dev = eng.beam_finalize_dev(*views, id_end=E)
    assert isinstance(dev.hyp, torch.Tensor) and np.array_equal(dev.lengths.numpy(), w["len"])
    # rows [B, k, T] seen as [B, T, k]: no buffer of k-word rows, copied
    perm = [torch.from_numpy(np.ascontiguousarray(c[n][:, :9].transpose(0, 2, 1))).permute(0, 2, 1) for n in ("ids", "parents", "scores")]
    same(eng.beam_finalize(*perm, id_end=E))
    same(eng.beam_finalize(views[0], perm[1], views[2], id_end=E))          # mixed strides: copied too
    same(eng.beam_finalize(t[0].to(torch.int64), c["parents"], t[2].to(torch.float64), id_end=E, steps=9))


def test_refusals_before_any_launch(eng, monkeypatch):
    c = make_case("refuse", 2, 3, 5, 5, "random", "none", 22)
    ids, par, sc = c["ids"], c["parents"], c["scores"]
    calls = []
    monkeypatch.setattr(eng, "_ck", lambda rc, what: calls.append(what))
    bad = par.copy()
    bad[1, 2, 0] = 3
    neg = par.copy()
    neg[0, 0, 1] = -1
    for a in (dict(ids=ids[0]), dict(parents=par[:, :4]), dict(scores=sc[:1]), dict(id_end=None), dict(id_end=-1), dict(steps=0), dict(steps=6),
              dict(parents=bad), dict(parents=neg), dict(ids=np.zeros((1, 2, 17), np.int32), parents=np.zeros((1, 2, 17), np.int32), scores=None),
              dict(ids=np.zeros((1, 1025, 1), np.int32), parents=np.zeros((1, 1025, 1), np.int32), scores=None)):
        kw = dict(dict(ids=ids, parents=par, scores=sc, id_end=END), **a)
        with pytest.raises(ValueError):
            eng.beam_finalize(**kw)
    assert not calls
    bad[1, 2, 0] = 1
    bad[1, 4, 0] = 7                                                # behind `steps`: not looked at
    eng.beam_finalize(ids, bad, sc, id_end=END, steps=4)
    assert calls == ["beam_finalize"]
    img = _images()
    ws = eng.ws
    for kw in (dict(return_consensus=True), dict(length_penalty=0.5), dict(coverage_penalty=0.1), dict(return_nbest=True, length_penalty=-1.0),
               dict(return_nbest=True, coverage_penalty=float("nan")), dict(return_nbest=True, cov_floor=0.0), dict(return_nbest=True, cov_floor=1.5),
               dict(return_nbest=True, return_consensus=True, consensus_cost="wer"), dict(return_nbest=True, max_iter=1025)):
        with pytest.raises(ValueError):
            eng.beam_decode(img, END, K, **dict(dict(max_iter=4), **kw))
    assert calls == ["beam_finalize"] and eng.ws is ws


# ------------------------------------------------------------------------------------------------------------------ the model --
@pytest.fixture(scope="module")
def model(tmp_path_factory, lib):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    tmp = tmp_path_factory.mktemp("nbest")
    (tmp / "vocab.txt").write_text("\n".join(["a", "b", "c", "d", "e", "f", "g", "h"]) + "\n")          # + _UNK, _PAD, _END: 11 ids
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp / "vocab.txt")}))
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": 5, "decoding": "beam_search", "beam_size": K})
    m = Img2SeqModel(cfg, str(tmp) + "/out/", vocab, lib=lib)
    m.build_pred()
    m.engine = Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib, max_steps=7)
    return m


def test_nbest_batch(model):
    imgs, _ = synthetic.make_set(2, H, W, V, 2, 4, seed=9)
    assert model._vocab.id_end == END
    for kw in (dict(), dict(length_penalty=1.0, consensus=True), dict(length_penalty=0.6, coverage_penalty=0.2, consensus=True, consensus_cost="bleu")):
        res = model.nbest_batch(imgs, **kw)
        eo = model.engine.beam_decode(pad_batch_images(imgs), END, K, max_iter=6, return_nbest=True, length_penalty=kw.get("length_penalty", 0.0),
                                      coverage_penalty=kw.get("coverage_penalty", 0.0), return_consensus=bool(kw.get("consensus")),
                                      consensus_cost=kw.get("consensus_cost", "edit"))
        nb = eo[1]
        assert len(res) == 2
        for b, r in enumerate(res):
            hs = r["hypotheses"]
            assert [h["slot"] for h in hs] == nb.order[b].tolist() and [h["score"] for h in hs] == sorted((h["score"] for h in hs), reverse=True)
            for h in hs:
                i, n = h["slot"], h["length"]
                toks = [int(t) for t in nb.hyp[b, :n, i]]
                assert n == int(nb.lengths[b, i]) and h["text"] == " ".join(model._vocab.id_to_tok[t] for t in toks if t != END)
                assert h["logp"] == float(nb.seq_logp[b, i]) and h["score"] == float(nb.score[b, i]) and h["posterior"] == float(nb.post[b, i])
                assert h["token_logp"] == [float(x) for x in nb.tok_logp[b, :n, i]] and len(h["token_logp"]) == n
                assert ("risk" in h) == bool(kw.get("consensus")) and (not kw.get("consensus") or h["risk"] == float(eo[3][b, i]))
            assert abs(sum(h["posterior"] for h in hs) - 1.0) < 1e-6
            if kw.get("consensus"):
                assert hs[r["consensus"]]["slot"] == int(eo[2][b]) and r["expected_cost"] == hs[r["consensus"]]["risk"] == min(h["risk"] for h in hs)
            else:
                assert set(r) == {"hypotheses"}
    # the first hypothesis without penalties is predict_batch's best back-traced one where the two agree on the read-out
    model._config.decoding = "greedy"
    with pytest.raises(ValueError):
        model.nbest_batch(imgs)
    model._config.decoding = "beam_search"


def test_predict_refuses_what_nbest_does_not_combine_with(capsys):
    import predict
    for argv in (["--nbest", "--sample", "3", "x.png"], ["--length-penalty", "0.6", "x.png"], ["--nbest", "--length-penalty", "-1", "x.png"],
                 ["--nbest", "--consensus-cost", "bleu", "x.png"], ["--nbest", "--boxes", "x.png"]):
        with pytest.raises(SystemExit) as e:
            predict.main(argv)
        assert e.value.code == 2, argv
        capsys.readouterr()
