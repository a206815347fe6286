"""CPU (hipsim): lxo_greedy_decode_scores / lxo_beam_decode_scores -- the token log-probs and hypothesis scores of the decode loops --
against the oracle: greedy log-probs = log_softmax of the oracle's logits at the ids; every beam score = the log-prob of the token path
that back-traces from its slot, restated by teacher-forcing that path through oracle.decoder_train.  The ids and parents stay those of the
calls without scores."""
import ctypes
import os

import numpy as np
import pytest

from simharness import Sim, ptr

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_small.npz"))
SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V, END, MAX_ITER, MS = 11, 10, 8, 9
# The interpreted encoder's output is not the same from one Sim to the next in a process (measured: up to 1e-2 apart at conv6 for the same
# image and weights), so the oracle restates the decode from the features the Sim's own decoder read (ws region "img"): what is compared
# is the decoder and the scores alone.
TOL = 1e-5


def _torch_params(S):
    import torch
    return {k: torch.from_numpy(np.asarray(v)) for k, v in S.P.items()}


def _sim(beam=1, gamma=1.0, prob=0.0):
    S = Sim(2, 32, 48, 1, V, dtype=0, seed=0, beam=beam, max_steps=MS, dims=SMALL)
    if beam > 1:
        S.shape.div_gamma, S.shape.div_prob, S.shape.div_seed = gamma, prob, 4
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(GOLD["img"]), None), "enc")
    from latex_ocr_amd.model.utils.image import encoder_out_hw
    Hp, Wp = encoder_out_hw(32, 48)
    S.enc = S.region("img", np.float32)[:2 * Hp * Wp * SMALL["C"]].reshape(2, Hp * Wp, SMALL["C"]).copy()     # f32: [B][R][C] features (+ positions)
    return S


def teacher_forced_logp(P, enc, paths):
    """log_softmax of oracle.decoder_train's logits at the tokens of `paths` (int [n, T]) fed back, from features enc [n, R, C]"""
    import torch
    import torch.nn.functional as F
    from oracle import ref_model as R
    f = torch.from_numpy(np.asarray(paths, np.int64))
    lg = R.decoder_train(P, torch.from_numpy(enc), f)
    return F.log_softmax(lg.double(), dim=-1).gather(-1, f[..., None])[..., 0].numpy()


def path_logprob(P, enc, path, id_end):
    """log-prob of the token sequence `path` (int [n]) under teacher forcing, summed up to and including its first END."""
    lp = teacher_forced_logp(P, enc[None], [path])[0]
    end = np.flatnonzero(np.asarray(path) == id_end)
    n = int(end[0]) + 1 if end.size else len(path)
    return float(lp[:n].sum())


def backtrace_path(ids, par, b, t, i):
    """tokens 0 .. t of the hypothesis in slot i at step t of image b"""
    out, slot = [], i
    for s in range(t, -1, -1):
        out.append(int(ids[b, s, slot]))
        slot = int(par[b, s, slot])
    return out[::-1]


def test_greedy_logp_is_log_softmax_of_the_oracle_logits():
    import torch
    from oracle import ref_model as R
    S = _sim()
    ids = np.zeros((2, MS), np.int32); lp = np.zeros((2, MS), np.float32); steps = ctypes.c_int(0)
    S.ck(S.L.lxo_greedy_decode_scores(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(ids), ptr(lp), None,
                                      ctypes.byref(steps), None), "greedy_scores")
    n = steps.value
    S2 = _sim()
    ids0 = np.zeros((2, MS), np.int32); steps0 = ctypes.c_int(0)
    S2.ck(S2.L.lxo_greedy_decode(S2.sref(), ptr(S2.params), ptr(S2.wpack), ptr(S2.ws), END, MAX_ITER, ptr(ids0), ctypes.byref(steps0), None), "greedy")
    assert steps0.value == n and np.array_equal(ids[:, :n], ids0[:, :n])
    rid = R.greedy_decode(_torch_params(S), torch.from_numpy(GOLD["img"]), END, max_iter=MAX_ITER)
    assert np.array_equal(ids[:, :n], rid.numpy())
    # the greedy loop's logits are those of teacher-forcing its own ids (the oracle's greedy_decode and decoder_train agree bit for bit)
    ref = teacher_forced_logp(_torch_params(S), S.enc, ids[:, :n])
    assert np.abs(lp[:, :n] - ref).max() < TOL, np.abs(lp[:, :n] - ref).max()


def test_greedy_scores_null_logp_is_refused():
    S = _sim()
    ids = np.zeros((2, MS), np.int32); steps = ctypes.c_int(0)
    assert S.L.lxo_greedy_decode_scores(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(ids), None, None,
                                        ctypes.byref(steps), None) != 0


def _beam(k, gamma=1.0, prob=0.0, scores=True):
    S = _sim(k, gamma, prob)
    ids = np.zeros((2, MS, k), np.int32); par = np.zeros((2, MS, k), np.int32); sc = np.zeros((2, MS, k), np.float32)
    steps = ctypes.c_int(0)
    if scores:
        S.ck(S.L.lxo_beam_decode_scores(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(ids), ptr(par), ptr(sc), None,
                                        ctypes.byref(steps), None), "beam_scores")
    else:
        S.ck(S.L.lxo_beam_decode(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), END, MAX_ITER, ptr(ids), ptr(par), ctypes.byref(steps), None), "beam")
    n = steps.value
    return S, ids[:, :n], par[:, :n], sc[:, :n]


@pytest.mark.parametrize("k,gamma,prob", [(2, 1.0, 0.0), (3, 1.0, 0.0), (3, 0.5, 1.0), (2, 0.3, 0.5)])
def test_beam_scores_keep_the_ids_and_parents(k, gamma, prob):
    _, ids, par, sc = _beam(k, gamma, prob)
    _, ids0, par0, _ = _beam(k, gamma, prob, scores=False)
    assert ids.shape == ids0.shape and np.array_equal(ids, ids0) and np.array_equal(par, par0)
    assert np.isfinite(sc).all() and (np.diff(sc, axis=2) <= 0).all()          # top_k: slots in descending score order


@pytest.mark.parametrize("k", [2, 3])
def test_beam_scores_are_the_teacher_forced_path_logprobs(k):
    S, ids, par, sc = _beam(k)
    P = _torch_params(S)
    T = ids.shape[1]
    for b in range(2):
        for t in range(T):
            for i in range(k):
                ref = path_logprob(P, S.enc[b], backtrace_path(ids, par, b, t, i), END)
                assert abs(sc[b, t, i] - ref) < TOL * max(1.0, abs(ref)), (b, t, i, sc[b, t, i], ref)
