"""CPU (hipsim): teacher-forced scoring (lxo_score_tokens, Engine.score, Img2SeqModel.score_batch) -- the log-prob of every token of a
given formula, the model's top-1 token at every position and the per-sequence sums, read from the logits lxo_decoder_train_fwd leaves --
against log_softmax of oracle.decoder_train's logits, restated from the features the Sim's own decoder read (ws region "img", as
tests/test_decode_scores_sim.py does); against the training CE in bf16; and byte for byte: the call writes nothing but its outputs."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.model.utils.image import encoder_out_hw, pad_batch_images
from simharness import Sim, ptr
from simlib import SIM_SO, build_sim

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V = 11
H, W, T = 32, 48, 6
LENGTHS = np.array([6, 1, 3, 4], np.int32)          # one full row (length T), one of a single token
TOL = 1e-5
BF16_TOL = 1e-2                                    # per-token |logp bf16 - logp f32| (measured 3.1e-3 at this shape)


def _inputs(V_=V, B=4, seed=5):
    imgs, _ = synthetic.make_set(B, H, W, V_, 2, 4, seed=seed)
    rng = np.random.default_rng(seed)
    f = rng.integers(0, V_, size=(B, T)).astype(np.int32)
    return pad_batch_images(imgs), f


def _run(dtype, V_=V, lengths=LENGTHS, top1=True, seq=True, seed=0):
    img, f = _inputs(V_, len(lengths))
    B = len(lengths)
    S = Sim(B, H, W, T, V_, dtype=dtype, seed=seed, dims=SMALL)
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(img), None), "enc")
    S.ck(S.L.lxo_decoder_train_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(f), None), "dec")
    S.f, S.lengths = f, np.ascontiguousarray(lengths, np.int32)
    return S, _score(S, top1, seq)


def _score(S, top1=True, seq=True):
    B = S.f.shape[0]
    lp = np.full((B, T), 7.0, np.float32)
    t1 = np.full((B, T), 77, np.int32) if top1 else None
    sq = np.full(B, 7.0, np.float32) if seq else None
    S.ck(S.L.lxo_score_tokens(S.sref(), ptr(S.ws), ptr(S.f), ptr(S.lengths), ptr(lp), ptr(t1), ptr(sq), None), "score")
    return lp, t1, sq


def _features(S):
    Hp, Wp = encoder_out_hw(H, W)
    B = S.f.shape[0]
    if S.dtype == 1:
        return S.region("img", "ct")[:B * Hp * Wp * SMALL["C"]].reshape(B, Hp * Wp, SMALL["C"]).copy()
    return S.region("img", np.float32)[:B * Hp * Wp * SMALL["C"]].reshape(B, Hp * Wp, SMALL["C"]).copy()


def _oracle(S):
    """(log_softmax f64 [B, T, V], logits f64) of oracle.decoder_train from the features the Sim's decoder read"""
    import torch
    import torch.nn.functional as F
    from oracle import ref_model as R
    P = {k: torch.from_numpy(np.asarray(v)) for k, v in S.P.items()}
    lg = R.decoder_train(P, torch.from_numpy(_features(S)), torch.from_numpy(S.f.astype(np.int64))).double()
    return F.log_softmax(lg, dim=-1).numpy(), lg.numpy()


def _ordered_sum(x):
    s = np.float32(0.0)
    for v in x:
        s = np.float32(s + np.float32(v))
    return s


def _check_against_oracle(S, lp, t1, sq, tol):
    ref, lg = _oracle(S)
    B = S.f.shape[0]
    live = np.arange(T)[None, :] < S.lengths[:, None]
    tgt = np.take_along_axis(ref, S.f[..., None].astype(np.int64), -1)[..., 0]
    err = np.abs(lp - tgt)[live].max()
    print("logp vs oracle log_softmax: max |diff| %.2e" % err)
    assert err < tol
    assert (lp[~live] == 0).all() and (t1[~live] == -1).all()
    top2 = np.sort(lg, axis=-1)[..., -2:]
    clear = live & (top2[..., 1] - top2[..., 0] > 1e-4)
    assert clear.sum() > 0 and np.array_equal(t1[clear], lg.argmax(-1)[clear])
    assert ((t1[live] >= 0) & (t1[live] < S.V)).all()
    for b in range(B):
        assert sq[b].tobytes() == _ordered_sum(lp[b, :S.lengths[b]]).tobytes(), (b, sq[b], _ordered_sum(lp[b, :S.lengths[b]]))


def test_f32_scores_vs_oracle():
    S, (lp, t1, sq) = _run(0)
    _check_against_oracle(S, lp, t1, sq, TOL)


def test_general_kernel_form_large_vocabulary():
    """Vp > 1024: the strided three-pass form (score_kernel) instead of the row-in-registers one"""
    V_ = 1030
    S, (lp, t1, sq) = _run(0, V_=V_)
    assert (V_ + 31) // 32 * 32 > 1024
    _check_against_oracle(S, lp, t1, sq, TOL)


def test_bf16_scores():
    S32, (lp32, t32, _) = _run(0)
    S16, (lp16, t16, sq16) = _run(1)
    live = np.arange(T)[None, :] < LENGTHS[:, None]
    err = np.abs(lp16 - lp32)[live].max()
    print("bf16 vs f32 logp: max |diff| %.2e" % err)
    assert err < BF16_TOL
    assert (lp16[~live] == 0).all() and (t16[~live] == -1).all()
    for b in range(len(LENGTHS)):
        assert sq16[b].tobytes() == _ordered_sum(lp16[b, :LENGTHS[b]]).tobytes()
    # -sum logp over the live tokens = the CE kernel's sum CE on the same logits (its rows kernel, same expressions)
    S16.ck(S16.L.lxo_ce_loss_fwd_bwd(S16.sref(), ptr(S16.ws), ptr(S16.f), ptr(S16.lengths), ctypes.c_float(1.0 / int(LENGTHS.sum())), None), "ce")
    ce = float(S16.region("loss", np.float32)[0])
    tot = -float(np.sum(lp16[live], dtype=np.float64))
    print("bf16: -sum logp %.7f, CE sum %.7f" % (tot, ce))
    assert abs(tot - ce) <= 1e-5 * abs(ce)


@pytest.mark.parametrize("dtype", [0, 1])
def test_score_writes_nothing_but_its_outputs(dtype):
    S, first = _run(dtype)
    before = S.ws.copy()
    second = _score(S)
    assert np.array_equal(S.ws, before)                       # the whole workspace, byte for byte (d(logits), loss, det, ... untouched)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    lp, t1, sq = _score(S, top1=False, seq=False)              # optional outputs left out: the same log-probs
    assert lp.tobytes() == first[0].tobytes()
    assert np.array_equal(S.ws, before)


def test_failed_chain_word_poisons_every_output():
    S, _ = _run(1)
    w = S.region("xdec_sync", np.int32)
    w[_abi.LXO_XDEC_ERR_WORD] = 3                              # the forward chain's error word (what lxo_ce_loss_fwd_bwd turns into a NaN loss)
    lp, t1, sq = _score(S)
    assert np.isnan(lp).all() and (t1 == -1).all() and np.isnan(sq).all()


def test_null_logp_is_refused():
    S, _ = _run(0)
    rc = S.L.lxo_score_tokens(S.sref(), ptr(S.ws), ptr(S.f), ptr(S.lengths), None, None, None, None)
    assert rc != 0 and b"logp_out" in S.L.lxo_last_error()


# ---------------------------------------------------------------- host layer on the hipsim library --
@pytest.fixture(scope="module")
def lib():
    build_sim()
    return _abi.bind(ctypes.CDLL(SIM_SO))


def _engine(lib):
    from latex_ocr_amd.engine import Engine
    return Engine(V, dims=SMALL, dtype="f32", device="cpu", seed=3, lib=lib)


def test_engine_score(lib):
    eng = _engine(lib)
    img, f = _inputs(B=3)
    ln = np.array([6, 2, 5], np.int32)
    logp, top1, seq = eng.score(img, f, ln, return_top1=True)
    assert logp.shape == (3, T) and top1.shape == (3, T) and seq.shape == (3,) and logp.dtype == np.float32 and top1.dtype == np.int32
    live = np.arange(T)[None, :] < ln[:, None]
    assert (logp[live] < 0).all() and (logp[~live] == 0).all() and (top1[~live] == -1).all()
    lp2, seq2 = eng.score(img, f, ln)
    assert np.array_equal(lp2, logp) and np.array_equal(seq2, seq)
    ce, n = eng.evaluate_batch(img, f, ln)
    assert n == int(ln.sum()) and abs(-float(np.sum(seq, dtype=np.float64)) - ce) <= 1e-5 * abs(ce)
    for bad in (-1, V):
        g = f.copy(); g[1, 3] = bad
        with pytest.raises(ValueError):
            eng.score(img, g, ln)
    with pytest.raises(ValueError):
        eng.score(img, f, np.array([7, 1, 1], np.int32))       # a length beyond T
    assert np.array_equal(eng.score(img, f, ln)[0], logp)      # a refused call leaves nothing behind


def _model(lib, tmp_path):
    from latex_ocr_amd.model.img2seq import Img2SeqModel
    from latex_ocr_amd.model.utils.general import Config
    from latex_ocr_amd.model.utils.text import Vocab
    toks = ["a", "b", "c", "d", "e", "f", "g", "h"]             # + _UNK, _PAD, _END: 11 ids
    (tmp_path / "vocab.txt").write_text("\n".join(toks) + "\n")
    vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": str(tmp_path / "vocab.txt")}))
    assert vocab.n_tok == V
    cfg = Config({"attn_cell_config": {"dim_e": SMALL["E"], "dim_o": SMALL["O"], "num_units": SMALL["U"], "dim_embeddings": SMALL["D"]},
                  "compute_dtype": "f32", "device": "cpu", "max_length_formula": 20, "decoding": "greedy"})
    m = Img2SeqModel(cfg, str(tmp_path) + "/out/", vocab, lib=lib)
    m.build_pred()
    assert m.engine.lib is lib and m.engine.device.type == "cpu"
    m.engine = _engine(lib)            # C = 128, the encoder width the other sim tests interpret (configs give the facade 512 channels)
    return m, vocab


def test_model_score_batch(lib, tmp_path):
    m, vocab = _model(lib, tmp_path)
    imgs, _ = synthetic.make_set(3, H, W, V, 2, 4, seed=9)
    imgs = [imgs[0], imgs[1][:24, :40], imgs[2][:, :32]]                        # mixed sizes: padded as a training batch is
    strs = ["a b c", "d zz e f", "h"]                                          # "zz" is not in the vocabulary: id_unk
    ids = [vocab.form_prepro(s) for s in strs]
    assert ids[1][1] == vocab.id_unk
    out_s = m.score_batch(imgs, strs)
    out_i = m.score_batch(imgs, ids)
    assert out_s == out_i and len(out_s) == 3
    from latex_ocr_amd.model.utils.text import pad_batch_formulas
    f, ln = pad_batch_formulas(ids, vocab.id_pad, vocab.id_end)
    logp, top1, seq = m.engine.score(pad_batch_images(imgs), f, ln, return_top1=True)
    for b, (s, toks, first) in enumerate(out_s):
        n = len(ids[b]) + 1                                                    # the END the reference appends is scored too
        assert len(toks) == n and toks == [float(x) for x in logp[b, :n]] and s == float(seq[b])
        d = np.flatnonzero(top1[b, :n] != f[b, :n])
        assert first == (int(d[0]) if d.size else -1)
    with pytest.raises(ValueError):
        m.score_batch(imgs, strs[:2])
