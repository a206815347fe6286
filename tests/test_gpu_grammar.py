"""-m gpu: decode under a delimiter grammar (lxo_greedy_decode_grammar / lxo_beam_decode_grammar / lxo_sample_decode_grammar; Engine
greedy_decode / beam_decode / sample_decode with grammar=; Img2SeqModel.predict_batch(grammar=); predict.py --balanced).

The weights of tests/test_gpu_constraint.py: the model writes 7s and then END at staggered steps.  Two class tables make that a grammar
problem: 7 declared an OPENER (the rows must close what they opened before END, a token 8 the model never writes by itself, and the budget
binds at the rows' staggered ends), and 7 declared a CLOSER (banned at depth 0: the model's dominant token is taken away).

f32: token for token against tests/grammar_ref.py, log-probs inside the 1e-5 of the f32 constrained tests, depths exact.  bf16 (launch per
step: the chain holds no grammar): the guarantee on every row, a replay of every emitted sequence through the host Grammar, and against the
f32 reference equal columns up to a row's first divergence, which must be a near-tie of the reference's logits over the step's set."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from test_gpu_benchcfg import count_set, V
from latex_ocr_amd.grammar import Grammar
import grammar_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END, B, MAX_ITER = V - 1, 4, 30
SMP = dict(temperature=1.0, top_k=8, top_p=0.95, seed=3)


def opener7():
    c = np.zeros(V, np.int8); c[7], c[8] = 1, -1
    return Grammar(c, max_depth=6, budget=True, id_end=END)


def closer7():
    c = np.zeros(V, np.int8); c[9], c[7] = 1, -1
    return Grammar(c, max_depth=6, budget=True, id_end=END)


TABLES = {"opener7": opener7, "closer7": closer7}


@pytest.fixture(scope="module")
def ctx():
    params = train_end_params(V)
    img = pad_batch_images(count_set(B, 41)[0])
    P = {k: torch.from_numpy(np.asarray(v).copy()) for k, v in params.items()}
    with torch.no_grad():
        enc = R.encoder(P, torch.from_numpy(img))
    return params, img, P, enc


def _engine(dtype, params):
    eng = Engine(V, dtype=dtype, seed=0)
    eng.load_params(params)
    return eng


def _replay(g, seqs, depths, what):
    """the guarantee and the replay: balanced and ended, every token in its S_t, depth_out the host's"""
    for i, (seq, dep) in enumerate(zip(seqs, depths)):
        assert g.check(seq, END), (what, i, list(seq))
        want, ok = g.replay(seq, MAX_ITER, END)
        assert ok, (what, i, list(seq))
        if dep is not None:
            assert list(dep) == want, (what, i, list(seq), list(dep), want)


@pytest.mark.parametrize("table", sorted(TABLES))
def test_greedy_f32_vs_reference(ctx, table):
    params, img, P, enc = ctx
    g = TABLES[table]()
    eng = _engine("f32", params)
    free = eng.greedy_decode(img, END, max_iter=MAX_ITER)
    ids, lp, dep = eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True)
    with torch.no_grad():
        rid, rlp, rdep, _ = grammar_ref.greedy_grammar(P, enc, END, g, MAX_ITER)
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    assert np.array_equal(dep, rdep)
    err = np.abs(lp - rlp).max()
    print("greedy f32 %s: %d steps (free %d), |logp - reference| max %.2e, deepest %d" % (table, ids.shape[1], free.shape[1], err, dep.max()))
    assert err < 1e-5
    _replay(g, ids, dep, "greedy f32 " + table)
    assert (free == 7).any() and not all(g.check(free[b], END) for b in range(B))      # the free decode is unbalanced: the grammar binds
    if table == "opener7":
        assert dep.max() >= 1 and (ids == 8).any()


@pytest.mark.parametrize("table", sorted(TABLES))
def test_beam_f32_vs_reference(ctx, table):
    params, img, P, enc = ctx
    g, k = TABLES[table](), 3
    eng = _engine("f32", params)
    free, fpar = eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_parents=True)
    ids, par, sc, dep = eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True)
    with torch.no_grad():
        rid, rpar, rsc, rdep = grammar_ref.beam_grammar(P, enc, END, k, g, MAX_ITER)
    assert ids.shape == rid.shape and np.array_equal(ids, rid) and np.array_equal(par, rpar)
    assert np.array_equal(dep, rdep)
    err = np.abs(sc - rsc).max()
    print("beam 3 f32 %s: %d steps (free %d), |scores - reference| max %.2e" % (table, ids.shape[1], free.shape[1], err))
    assert err < 1e-5 * max(1.0, float(np.abs(rsc).max()))
    for b in range(B):
        _replay(g, grammar_ref.backtrace(ids[b], par[b]), [None] * k, "beam f32 " + table)
    assert any(not g.check(s, END) for b in range(B) for s in grammar_ref.backtrace(free[b], fpar[b]))


@pytest.mark.parametrize("table", sorted(TABLES))
def test_sample_f32_vs_reference(ctx, table):
    params, img, P, enc = ctx
    g, n = TABLES[table](), 3
    eng = _engine("f32", params)
    free = eng.sample_decode(img, END, n, max_iter=MAX_ITER, **SMP)
    ids, lp, lq, dep = eng.sample_decode(img, END, n, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True, **SMP)
    with torch.no_grad():
        rid, rlp, rlq, rdep, _, _ = grammar_ref.sample_grammar(P, enc, END, n, g, MAX_ITER, SMP["temperature"], SMP["top_k"], SMP["top_p"], SMP["seed"])
    assert ids.shape == rid.shape and np.array_equal(ids, rid), (ids, rid)
    assert np.array_equal(dep, rdep)
    err = max(np.abs(lp - rlp).max(), np.abs(lq - rlq).max())
    print("sample 3 f32 %s: %d steps (free %d), |logp, logq - reference| max %.2e" % (table, ids.shape[1], free.shape[1], err))
    assert err < 1e-5
    for b in range(B):
        _replay(g, ids[b].T, dep[b].T, "sample f32 " + table)
    assert not all(g.check(free[b, :, j], END) for b in range(B) for j in range(n))


@pytest.mark.parametrize("table", sorted(TABLES))
def test_bf16_guarantee_replay_and_reference(ctx, table):
    params, img, P, enc = ctx
    g = TABLES[table]()
    eng = _engine("bf16", params)
    ids, lp, dep = eng.greedy_decode(img, END, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True)
    assert not eng.chain_status()[0]                                            # launch per step: the chain was not used
    _replay(g, ids, dep, "greedy bf16 " + table)
    assert np.isfinite(lp).all()
    with torch.no_grad():
        rid, _, _, rlogits = grammar_ref.greedy_grammar(P, enc, END, g, MAX_ITER)
    rlogits = np.where(np.isfinite(rlogits), rlogits, 0.0)                     # the reference's logits over S_t (a banned column is never a gap's operand)
    n_div = assert_flips_are_near_ties(ids, rid, rlogits, "grammar greedy bf16 " + table)
    T = min(ids.shape[1], rid.shape[1])
    m = np.cumprod(ids[:, :T] == rid[:, :T], axis=1).astype(bool)
    print("greedy bf16 %s: %d steps (reference %d), rows diverging %d, columns compared before the first divergence: %.4f of all"
          % (table, ids.shape[1], rid.shape[1], n_div, float(m.sum()) / float(B * max(ids.shape[1], rid.shape[1]))))
    k = 3
    bid, bpar, bsc, bdep = eng.beam_decode(img, END, k, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True)
    for b in range(B):
        _replay(g, grammar_ref.backtrace(bid[b], bpar[b]), [None] * k, "beam bf16 " + table)
        for t in range(bid.shape[1]):                                           # depth [t][j]: of the hypothesis in slot j at step t
            for j, seq in enumerate(grammar_ref.backtrace(bid[b, :t + 1], bpar[b, :t + 1])):
                assert bdep[b, t, j] == g.replay(seq, MAX_ITER, END)[0][-1], (b, t, j)
    assert np.isfinite(bsc).all()
    sid, slp, slq, sdep = eng.sample_decode(img, END, 3, max_iter=MAX_ITER, return_scores=True, grammar=g, return_depth=True, **SMP)
    for b in range(B):
        _replay(g, sid[b].T, sdep[b].T, "sample bf16 " + table)
    assert np.isfinite(slp).all() and np.isfinite(slq).all()


def test_grammar_refusals(ctx):
    params, img, _, _ = ctx
    eng = _engine("bf16", params)
    g = opener7()
    no_closer = np.ones(V, bool); no_closer[8] = False
    for kw in (dict(grammar=g, allowed=no_closer), dict(grammar=Grammar(np.zeros(V + 1, np.int8), id_end=END)), dict(return_depth=True),
               dict(grammar=g, prefix=np.full((B, 1), 8, np.int32))):
        with pytest.raises(ValueError):
            eng.greedy_decode(img, END, max_iter=MAX_ITER, **kw)
        with pytest.raises(ValueError):
            eng.beam_decode(img, END, 3, max_iter=MAX_ITER, **kw)
        with pytest.raises(ValueError):
            eng.sample_decode(img, END, 3, max_iter=MAX_ITER, **kw)
    assert not hasattr(eng, "_img") and eng.ws is None


# ---------------------------------------------------------------------------------------------------------------- the facade ----
@pytest.mark.parametrize("decoding", ["greedy", "beam_search"])
def test_predict_batch_and_predict_py_balanced(tmp_path, monkeypatch, decoding):
    from PIL import Image
    from latex_ocr_amd.model.utils.image import greyscale
    from test_gpu_constraint import _model
    monkeypatch.chdir(tmp_path)
    m, d = _model(str(tmp_path), decoding)
    vocab = m._vocab
    files = sorted(p for p in os.listdir("data/synthetic/test") if p.endswith(".png"))[:3]
    imgs = [greyscale(np.asarray(Image.open("data/synthetic/test/" + p).convert("RGB"))) for p in files]
    free = m.predict_batch(imgs)
    emitted = sorted({t for h in free for s in h for t in s.split()})
    assert emitted                                                           # the randomly initialised model writes something
    other = [t for t in vocab.tok_to_id if t not in emitted and vocab.tok_to_id[t] < vocab.n_tok - 3]
    pairs = [(emitted[0], other[0])]                                         # what the model writes opens; a token it does not write closes
    g = Grammar.from_pairs(vocab, pairs)
    ids_of = lambda s: [vocab.tok_to_id[t] for t in s.split()] + [vocab.id_end]
    assert not all(g.check(ids_of(s)) for h in free for s in h)              # the free hypotheses are unbalanced
    hyps, scores = m.predict_batch(imgs, return_scores=True, grammar=g)
    assert all(g.check(ids_of(s)) for h in hyps for s in h), hyps
    assert all(np.isfinite(scores[i][b][0]) for i in range(len(hyps)) for b in range(3))
    assert all(g.check(ids_of(s)) for h in m.predict_batch(imgs, grammar=g) for s in h)
    with pytest.raises(ValueError):
        m.predict_batch(imgs, grammar=True)                                  # Grammar.latex: the synthetic vocabulary has no delimiters
    m.save_session(1)
    run = lambda *extra: subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, *extra,
                                                  "data/synthetic/test/" + files[0], "data/synthetic/test/" + files[1]], cwd=str(tmp_path),
                                                 timeout=600, env=dict(os.environ, PYTHONPATH=ROOT)).decode()
    spec = "%s:%s" % pairs[0]
    lines = [l for l in run("--balanced", "--pairs", spec).splitlines() if "=>" in l]
    assert len(lines) == 2 and all(g.check(ids_of(l.split("=>")[1])) for l in lines), lines
    out = run("--pairs", spec)                                               # without the flag: the report
    ls = out.splitlines()
    said = [(ls[i].split("=>")[1], ls[i + 1].strip()) for i in range(len(ls) - 1) if "=>" in ls[i]]
    assert len(said) == 2 and all(r == "balanced: " + ("yes" if g.check(ids_of(h)) else "no") for h, r in said), out
