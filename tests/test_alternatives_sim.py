"""CPU (hipsim): alternatives per position (lxo_score_alternatives: score_alt_rows_kernel<BF, KV, AL> and the strided score_alt_kernel<AL>)
-- the k best tokens, the given token's rank and the step's entropy -- on the CONSTRUCTED logits of tests/output_head_ref.py against the
float64 reference of tests/alternatives_ref.py: ids and ranks exactly, log-probs and entropies within bounds derived there; poisoned
padding; the bit identities with lxo_score_tokens; allowed sets; and the call's contract (writes nothing but its outputs, the failed-chain
word, refused arguments).  Then the sim's real decoder against oracle.decoder_train, and the host layers (Engine.score, Img2SeqModel)."""
import numpy as np
import pytest

from latex_ocr_amd import _abi
from alternatives_ref import check, pack_bits, reference
from output_head_ref import CASES, POISONS, VOCABS, make_case, padded, vpad
from simharness import Sim, ptr

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
H, W = 32, 48
B, T = 3, 4                        # 12 rows: three workgroups of four waves


def run_alt(S, f, ln, k, allow=None, allow_ld=0, rank=True, ent=True):
    """lxo_score_alternatives on what ws "logits" holds -> (ids [B, T, k], logp, rank, entropy); outputs start as sentinels"""
    nb, nt = f.shape
    ids = np.full((nb, nt, k), 77, np.int32)
    lp = np.full((nb, nt, k), 7.0, np.float32)
    rk = np.full((nb, nt), 77, np.int32) if rank else None
    en = np.full((nb, nt), 7.0, np.float32) if ent else None
    S.ck(S.L.lxo_score_alternatives(S.sref(), ptr(S.ws), ptr(f), ptr(ln), k, ptr(allow), allow_ld, ptr(ids), ptr(lp), ptr(rk), ptr(en), None), "alt")
    return ids, lp, rk, en


def score_tokens(S, f, ln):
    nb, nt = f.shape
    lp = np.full((nb, nt), 7.0, np.float32)
    t1 = np.full((nb, nt), 77, np.int32)
    S.ck(S.L.lxo_score_tokens(S.sref(), ptr(S.ws), ptr(f), ptr(ln), ptr(lp), ptr(t1), None, None), "score")
    return lp, t1


def check_identities(out, lp_tok, top1, f, ln, V):
    """against lxo_score_tokens on the same workspace: slot 0 is its top-1; a slot that holds the (clamped) target carries its logp, byte for
    byte, and the slot's index is the rank"""
    ids, lp, rk, _ = out
    nb, nt = f.shape
    live = np.arange(nt)[None, :] < ln[:, None]
    assert np.array_equal(ids[..., 0], top1)
    hit = (ids == np.clip(f.astype(np.int64), 0, V - 1)[..., None]) & live[..., None]
    b, t, j = np.nonzero(hit)
    assert lp[b, t, j].tobytes() == lp_tok[b, t].tobytes()
    assert np.array_equal(rk[b, t], j)
    assert ((rk[live] >= ids.shape[2]) == ~hit.any(-1)[live]).all()       # a target outside the k slots has a rank beyond them


_sims = {}


def _sim(V, dtype):
    if (V, dtype) not in _sims:
        _sims[(V, dtype)] = Sim(B, H, W, T, V, dtype=dtype, seed=0, dims=SMALL)
    return _sims[(V, dtype)]


def ks_of(V):
    return sorted({1, min(5, V), min(16, V)})


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", VOCABS)
def test_alternatives(V, dtype, case):
    S = _sim(V, dtype)
    Vp = vpad(V)
    x, f, ln = make_case(case, V, B, T, seed=1)
    S.write_region("logits", padded(x, Vp, None))
    lp_tok, top1 = score_tokens(S, f, ln)
    worst = [0.0, 0.0]
    for k in ks_of(V):
        ref = reference(x, f, ln, k)
        S.write_region("logits", padded(x, Vp, None))
        clean = run_alt(S, f, ln, k)
        e = check(ref, x, *clean)
        worst = [max(a, b) for a, b in zip(worst, e)]
        check_identities(clean, lp_tok, top1, f, ln, V)
        for poison in POISONS:
            S.write_region("logits", padded(x, Vp, poison))
            out = run_alt(S, f, ln, k)
            for a, b in zip(clean, out):
                assert a.tobytes() == b.tobytes(), (poison, k)                  # nothing read the padding
            pad = S.region("logits", np.float32)[:T * B * Vp].reshape(T * B, Vp)[:, V:Vp]
            assert (np.isnan(pad) if poison == "nan" else pad == np.float32(1e30)).all()    # ... and it was there to be read
    print("V=%d %s %s: worst |logp - ref| %.2e, entropy at %.3f of its bound" % (V, ("f32", "bf16")[dtype], case, worst[0], worst[1]))


def allowed_sets(x, f, ln, k, seed):
    """-> {name: bool [B, V] (or [1, V]: a shared set)}: about a quarter banned per row; one shared set; the target of every other position
    banned; a row with fewer than k allowed"""
    nb, V = f.shape[0], x.shape[1]
    rng = np.random.default_rng([seed, V, k])
    sets = {"random": rng.random((nb, V)) >= 0.25, "shared": rng.random((1, V)) >= 0.25}
    for a in sets.values():
        a[:, rng.integers(0, V)] = True                                         # never an empty row
    ban = np.ones((nb, V), bool)
    tgt = np.clip(f, 0, V - 1)
    for b in range(nb):
        ban[b, tgt[b, ::2]] = False
        if not ban[b].any():
            ban[b, (tgt[b, 0] + 1) % V] = True
    sets["target_banned"] = ban
    few = rng.random((nb, V)) >= 0.25
    few[nb - 1] = False
    few[nb - 1, rng.choice(V, size=max(1, min(k, V) - 2), replace=False)] = True      # fewer than k wherever k >= 2 (one where k = 1)
    few[0, rng.integers(0, V)] = True
    sets["few"] = few
    return sets


def check_allowed(run, x, f, ln, k):
    """run(allow words or None, allow_ld) -> outputs; every set of allowed_sets against the masked reference, all-ones byte-identical to no set"""
    nb, V = f.shape[0], x.shape[1]
    words = (V + 31) // 32
    plain = run(None, 0)
    for ones, ld in ((np.ones((nb, V), bool), words), (np.ones((1, V), bool), 0)):
        for a, b in zip(plain, run(pack_bits(ones), ld)):
            assert a.tobytes() == b.tobytes()
    worst = 0.0
    for name, al in allowed_sets(x, f, ln, k, seed=3).items():
        full = np.broadcast_to(al, (nb, V))
        ref = reference(x, f, ln, k, allowed=full)
        out = run(pack_bits(al), 0 if al.shape[0] == 1 else words)
        worst = max(worst, check(ref, x, *out)[1])
        live = ref["live"]
        if name == "target_banned":
            banned = live & ~np.take_along_axis(full, ref["tgt"], 1)
            assert banned.any() and (out[2][banned] == -1).all() and (out[2][live & ~banned] >= 0).all()
        if name == "few" and k >= 3:
            row = live[nb - 1]
            assert row.any() and (out[0][nb - 1][row][:, k - 2:] == -1).all() and np.isneginf(out[1][nb - 1][row][:, k - 2:]).all()
            assert (out[0][nb - 1][row][:, :k - 2] >= 0).all()
        sel = out[0][live]
        assert (np.take_along_axis(np.repeat(full[:, None], f.shape[1], 1)[live], np.maximum(sel, 0), 1) | (sel < 0)).all()      # no banned id
    return worst


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", (4, 33, 257, 512, 1000, 1025, 3000))
def test_allowed_sets(V, dtype):
    S = _sim(V, dtype)
    x, f, ln = make_case("normal", V, B, T, seed=2)
    S.write_region("logits", padded(x, vpad(V), "nan"))
    for k in ks_of(V):
        worst = check_allowed(lambda al, ld: run_alt(S, f, ln, k, al, ld), x, f, ln, k)
    print("V=%d %s: allowed sets, entropy at %.3f of its bound" % (V, ("f32", "bf16")[dtype], worst))


# ------------------------------------------------------------------------------------------------ the call's contract, real decoder --
from test_score_sim import V as V11, T as T6, _engine, _inputs, _model, _oracle, _run      # noqa: E402

LENGTHS = np.array([6, 3], np.int32)
_real = {}


def real(dtype):
    """the sim's real decoder after lxo_decoder_train_fwd on two images (one forward per dtype: the sim interprets the encoder at seconds per image)"""
    if dtype not in _real:
        _real[dtype] = _run(dtype, lengths=LENGTHS)[0]
    return _real[dtype]


@pytest.mark.parametrize("dtype", [0, 1])
def test_writes_nothing_but_its_outputs(dtype):
    S = real(dtype)
    before = S.ws.copy()
    first = run_alt(S, S.f, S.lengths, 3)
    second = run_alt(S, S.f, S.lengths, 3)
    assert np.array_equal(S.ws, before)                       # the whole workspace, byte for byte
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    ids, lp, rk, en = run_alt(S, S.f, S.lengths, 3, rank=False, ent=False)      # optional outputs left out: the same ids and log-probs
    assert rk is None and en is None and ids.tobytes() == first[0].tobytes() and lp.tobytes() == first[1].tobytes()
    run_alt(S, S.f, S.lengths, 3, pack_bits(np.ones((1, V11), bool)), 0)
    assert np.array_equal(S.ws, before)


def test_failed_chain_word_poisons_every_output():
    S = real(1)
    w = S.region("xdec_sync", np.int32)
    w[_abi.LXO_XDEC_ERR_WORD] = 3
    try:
        ids, lp, rk, en = run_alt(S, S.f, S.lengths, 4)
    finally:
        w[_abi.LXO_XDEC_ERR_WORD] = 0
    assert (ids == -1).all() and np.isnan(lp).all() and (rk == -1).all() and np.isnan(en).all()


def test_bad_arguments_are_refused():
    S = real(0)
    f, ln = S.f, S.lengths
    ids = np.full((2, T6, 3), 77, np.int32); lp = np.full((2, T6, 3), 7.0, np.float32)
    words = (V11 + 31) // 32
    L, s, w = S.L, S.sref(), ptr(S.ws)
    S40 = Sim(2, H, W, T6, 40, dtype=0, seed=0, dims=SMALL)      # V = 40: two words per row
    al = pack_bits(np.ones((2, 40), bool))
    calls = [("ids_out", lambda: L.lxo_score_alternatives(s, w, ptr(f), ptr(ln), 3, None, 0, None, ptr(lp), None, None, None)),
             ("logp_out", lambda: L.lxo_score_alternatives(s, w, ptr(f), ptr(ln), 3, None, 0, ptr(ids), None, None, None, None)),
             ("k", lambda: L.lxo_score_alternatives(s, w, ptr(f), ptr(ln), 0, None, 0, ptr(ids), ptr(lp), None, None, None)),
             ("k", lambda: L.lxo_score_alternatives(s, w, ptr(f), ptr(ln), 17, None, 0, ptr(ids), ptr(lp), None, None, None)),
             ("k", lambda: L.lxo_score_alternatives(s, w, ptr(f), ptr(ln), V11 + 1, None, 0, ptr(ids), ptr(lp), None, None, None)),
             ("allow", lambda: L.lxo_score_alternatives(s, w, ptr(f), ptr(ln), 3, None, words, ptr(ids), ptr(lp), None, None, None)),
             ("allow_ld", lambda: L.lxo_score_alternatives(S40.sref(), ptr(S40.ws), ptr(f), ptr(ln), 3, ptr(al), 1, ptr(ids), ptr(lp), None, None, None))]
    for name, call in calls:
        assert call() == -1 and name.encode() in L.lxo_last_error(), (name, L.lxo_last_error())
    assert (ids == 77).all() and (lp == 7.0).all()


def check_against_oracle(ref, ids, lp, rk, f, lengths, V, tol=1e-5):
    """ref = log_softmax f64 [B, T, V] of the oracle; no position excluded: a swap at a near-tie passes, a wrong candidate cannot"""
    nb, nt, k = ids.shape
    live = np.arange(nt)[None, :] < lengths[:, None]
    srt = -np.sort(-ref, axis=-1)
    worst = 0.0
    for b, t in zip(*np.nonzero(live)):
        i = ids[b, t]
        assert len(set(i.tolist())) == k and (i >= 0).all() and (i < V).all()
        e1, e2 = np.abs(lp[b, t] - ref[b, t, i]).max(), np.abs(lp[b, t] - srt[b, t, :k]).max()
        worst = max(worst, e1, e2)
        assert e1 < tol and e2 < tol, (b, t, e1, e2)
        rt = ref[b, t, f[b, t]]
        assert (ref[b, t] > rt + tol).sum() <= rk[b, t] <= (ref[b, t] >= rt - tol).sum() - 1, (b, t, rk[b, t])
    return worst


def test_real_decoder_vs_oracle():
    S = real(0)
    ref, _ = _oracle(S)
    live = np.arange(T6)[None, :] < S.lengths[:, None]
    h = -(np.exp(ref) * ref).sum(-1)
    for k in (1, 3, V11):
        ids, lp, rk, en = run_alt(S, S.f, S.lengths, k)
        worst = check_against_oracle(ref, ids, lp, rk, S.f, S.lengths, V11)
        assert np.abs(en - h)[live].max() < 1e-5 * (2 + h[live].max())
        print("k=%d: |logp - oracle| max %.2e, |H - oracle| max %.2e" % (k, worst, np.abs(en - h)[live].max()))


# ---------------------------------------------------------------- host layer on the hipsim library --
@pytest.fixture(scope="module")
def lib():
    from simharness import lib as sim_lib
    return sim_lib()


def forward_once(eng):
    """The sim interprets the encoder at seconds per image, and a test below asks for the same forward many times: skip a forward whose
    inputs are byte for byte the previous one's (lxo_score_tokens / lxo_score_alternatives leave the workspace as it is -- tested above);
    a decode in between makes the next forward run."""
    fwd, enc, last = eng.forward, eng._encode_only, [None]

    def forward(img, formula, **kw):
        key = (np.asarray(img).tobytes(), np.asarray(formula).tobytes(), np.asarray(formula).shape)
        if kw or key != last[0]:
            fwd(img, formula, **kw)
            last[0] = None if kw else key

    def encode_only(*a, **kw):
        last[0] = None
        return enc(*a, **kw)
    eng.forward, eng._encode_only = forward, encode_only
    return eng


def test_engine_score_alternatives(lib):
    from latex_ocr_amd.engine import Alternatives
    eng = forward_once(_engine(lib))
    img, f = _inputs(B=2)
    f = np.ascontiguousarray(f[:, :3])
    ln, nt = np.array([3, 2], np.int32), 3
    base = eng.score(img, f, ln, return_top1=True)
    same = eng.score(img, f, ln, return_top1=True, alternatives=0, allowed=None)
    assert len(same) == 3 and all(np.array_equal(a, b) for a, b in zip(base, same))
    out = eng.score(img, f, ln, return_top1=True, alternatives=4)
    assert len(out) == 4 and all(np.array_equal(a, b) for a, b in zip(base, out[:3]))
    alt = out[3]
    assert isinstance(alt, Alternatives) and alt.ids.shape == (2, nt, 4) and alt.logp.shape == (2, nt, 4) and alt.rank.shape == (2, nt) and alt.entropy.shape == (2, nt)
    assert alt.ids.dtype == np.int32 and alt.logp.dtype == np.float32 and alt.rank.dtype == np.int32 and alt.entropy.dtype == np.float32
    live = np.arange(nt)[None, :] < ln[:, None]
    assert np.array_equal(alt.ids[..., 0], base[1]) and (alt.ids[~live] == -1).all() and (alt.entropy[live] > 0).all()
    assert (np.diff(alt.logp[live], axis=-1) <= 0).all()
    two = eng.score(img, f, ln, alternatives=4)
    assert len(two) == 3 and all(np.array_equal(a, b) for a, b in zip(two[2], alt))
    # allowed sets: [V] and [B, V]; logp / top1 / seq stay the unconstrained values
    al = np.ones(V11, bool); al[base[1][0, 0]] = False
    con = eng.score(img, f, ln, return_top1=True, alternatives=4, allowed=al)
    assert all(np.array_equal(a, b) for a, b in zip(base, con[:3]))
    assert (con[3].ids[live] != base[1][0, 0]).all() and con[3].ids[0, 0, 0] == alt.ids[0, 0, 1]
    per = np.ones((2, V11), bool); per[1] = al
    rows = eng.score(img, f, ln, alternatives=4, allowed=per)[-1]
    assert np.array_equal(rows.ids[1], con[3].ids[1]) and np.array_equal(rows.ids[0], alt.ids[0]) and rows.logp[1].tobytes() == con[3].logp[1].tobytes()
    for bad in (dict(allowed=al), dict(alternatives=-1), dict(alternatives=17), dict(alternatives=V11 + 1), dict(alternatives=2, allowed=np.ones(V11 + 1, bool)),
                dict(alternatives=2, allowed=np.zeros(V11, bool))):
        with pytest.raises(ValueError):
            eng.score(img, f, ln, **bad)


def test_model_alternatives(lib, tmp_path):
    from latex_ocr_amd import synthetic
    m, vocab = _model(lib, tmp_path)
    forward_once(m.engine)
    m._config.max_length_formula = 3                                            # max_iter = 4: decodes of at most five steps
    imgs, _ = synthetic.make_set(2, 32, 48, V11, 2, 4, seed=9)
    strs = ["a b", "d zz e"]
    base = m.score_batch(imgs, strs)
    assert m.score_batch(imgs, strs, alternatives=0) == base
    out = m.score_batch(imgs, strs, alternatives=3)
    toks = set(vocab.tok_to_id)
    for (s, lps, first), full in zip(base, out):
        assert full[:3] == (s, lps, first) and len(full[3]) == len(lps)
        for t, e in enumerate(full[3]):
            assert set(e) == {"rank", "entropy", "alternatives"} and isinstance(e["rank"], int) and isinstance(e["entropy"], float)
            assert len(e["alternatives"]) == 3 and all(tok in toks and isinstance(lp, float) for tok, lp in e["alternatives"])
            if e["rank"] < 3:
                assert e["alternatives"][e["rank"]][1] == lps[t]                # the given token's slot carries its score
            assert (first == -1 or t < first) <= (e["rank"] == 0)
    ban = m.score_batch(imgs, strs, alternatives=3, banned=["a"])
    assert all(tok != "a" for r in ban for e in r[3] for tok, _ in e["alternatives"]) and ban[0][3][0]["rank"] == -1
    assert [r[:3] for r in ban] == base
    with pytest.raises(ValueError):
        m.score_batch(imgs, strs, banned=["a"])
    with pytest.raises(ValueError):
        m.score_batch(imgs, strs, alternatives=17)
    # decode, then the teacher-forced pass over what was emitted
    hyps, scores, alts = m.predict_batch(imgs, alternatives=2)
    assert len(alts) == len(hyps) == len(scores) == 1
    end = vocab.id_to_tok[vocab.id_end]
    for b in range(2):
        emitted = hyps[0][b].split() if hyps[0][b] else []
        n = len(scores[0][b][1])
        assert len(alts[0][b]) == n and n in (len(emitted), len(emitted) + 1) and n <= 5      # max_iter + 1 steps at the most
        path = emitted + [end] * (n - len(emitted))
        for t, e in enumerate(alts[0][b]):
            (t0, l0), (t1, l1) = e["alternatives"]
            if l0 - l1 > 1e-4:                                                  # away from a near-tie: slot 0 is the emitted token
                assert t0 == path[t] and e["rank"] == 0 and abs(l0 - scores[0][b][1][t]) < 1e-4
    with pytest.raises(ValueError):
        m.predict_batch(imgs, alternatives=17)
