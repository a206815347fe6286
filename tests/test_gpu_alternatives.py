"""-m gpu: alternatives per position (lxo_score_alternatives, Engine.score(alternatives=), Img2SeqModel, predict.py --alternatives).

1. CONSTRUCTED logits written into ws region "logits" (tests/output_head_ref.py's case matrix, tests/alternatives_ref.py's float64
   reference): ids and ranks exactly, log-probs and entropies within their bounds, poisoned padding, the bit identities with
   lxo_score_tokens, allowed sets, and row counts above the grid cap of the row loop.
2. The real decoder: f32 against the oracle without excluding a position; bf16 against the f32 run at a chain batch and a padded one;
   a batch above 64 against its pieces; the drivers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from alternatives_ref import check, pack_bits, reference
from latex_ocr_amd.engine import _p
from output_head_ref import CASES, POISONS, VOCABS, make_case, padded, vpad
from test_alternatives_sim import check_against_oracle, check_allowed, check_identities, ks_of
from test_gpu_score import BF16_BATCH_TOL, _results_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 32, 128

# ------------------------------------------------------------------------------------------------------------ 1. constructed logits --
_engines = {}


def _head_engine(V, dtype, B, T):
    eng = _engines.get((V, dtype))
    if eng is None:
        eng = _engines[(V, dtype)] = Engine(V, dtype=dtype, seed=0)
    eng.ensure(B, H, W, T)
    if dtype == "bf16":
        assert int(eng.region("xdec_sync", "i32")[512].item()) == 0            # the forward chain's error word the kernels read
    return eng


def write_logits(eng, x_p):
    eng.region("logits")[:x_p.size].copy_(torch.from_numpy(x_p.reshape(-1)))


def run_alt(eng, f, ln, k, allow=None, allow_ld=0):
    """lxo_score_alternatives on what ws "logits" holds -> (ids [B, T, k], logp, rank, entropy), host arrays"""
    B, T = f.shape
    dev = eng.device
    fd, ld = torch.from_numpy(f).to(dev), torch.from_numpy(ln).to(dev)
    al = torch.from_numpy(allow.view(np.int32)).to(dev) if allow is not None else None
    ids = torch.full((B, T, k), 77, dtype=torch.int32, device=dev)
    lp = torch.full((B, T, k), 7.0, dtype=torch.float32, device=dev)
    rk = torch.full((B, T), 77, dtype=torch.int32, device=dev)
    en = torch.full((B, T), 7.0, dtype=torch.float32, device=dev)
    eng._ck(eng.lib.lxo_score_alternatives(eng.sref(), _p(eng.ws), _p(fd), _p(ld), k, _p(al), allow_ld, _p(ids), _p(lp), _p(rk), _p(en),
                                           eng._stream()), "score_alternatives")
    return ids.cpu().numpy(), lp.cpu().numpy(), rk.cpu().numpy(), en.cpu().numpy()


def score_tokens(eng, f, ln):
    B, T = f.shape
    fd, ld = torch.from_numpy(f).to(eng.device), torch.from_numpy(ln).to(eng.device)
    lp = torch.full((B, T), 7.0, dtype=torch.float32, device=eng.device)
    t1 = torch.full((B, T), 77, dtype=torch.int32, device=eng.device)
    eng._ck(eng.lib.lxo_score_tokens(eng.sref(), _p(eng.ws), _p(fd), _p(ld), _p(lp), _p(t1), None, eng._stream()), "score_tokens")
    return lp.cpu().numpy(), t1.cpu().numpy()


def _case(V, dtype, case, B, T, ks, poisons=POISONS):
    eng = _head_engine(V, dtype, B, T)
    Vp = vpad(V)
    x, f, ln = make_case(case, V, B, T, seed=2)
    write_logits(eng, padded(x, Vp, None))
    lp_tok, top1 = score_tokens(eng, f, ln)
    worst = [0.0, 0.0]
    for k in ks:
        ref = reference(x, f, ln, k)
        write_logits(eng, padded(x, Vp, None))
        clean = run_alt(eng, f, ln, k)
        worst = [max(a, b) for a, b in zip(worst, check(ref, x, *clean))]
        check_identities(clean, lp_tok, top1, f, ln, V)
        for poison in poisons:
            write_logits(eng, padded(x, Vp, poison))
            out = run_alt(eng, f, ln, k)
            for a, b in zip(clean, out):
                assert a.tobytes() == b.tobytes(), (poison, k)                  # no output read the padding ...
            pad = eng.region("logits")[:T * B * Vp].cpu().numpy().reshape(T * B, Vp)[:, V:Vp]
            assert (np.isnan(pad) if poison == "nan" else pad == np.float32(1e30)).all()    # ... which was there to be read
    print("V=%d %s %s rows=%d: worst |logp - ref| %.2e, entropy at %.3f of its bound" % (V, dtype, case, B * T, worst[0], worst[1]))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", VOCABS)
def test_alternatives(V, dtype, case):
    _case(V, dtype, case, 8, 16, ks_of(V))                                      # 128 rows: 32 workgroups of four row-waves


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", [33, 512, 1025])
def test_allowed_sets(V, dtype):
    B, T = 8, 16
    eng = _head_engine(V, dtype, B, T)
    x, f, ln = make_case("normal", V, B, T, seed=3)
    write_logits(eng, padded(x, vpad(V), "nan"))
    for k in ks_of(V):
        worst = check_allowed(lambda al, ld: run_alt(eng, f, ln, k, al, ld), x, f, ln, k)
    print("V=%d %s: allowed sets, entropy at %.3f of its bound" % (V, dtype, worst))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", [33, 512, 3000])
def test_row_counts_above_the_grid_cap(V, dtype):
    """B = 64, T = 151: 9664 rows, above the 2048 workgroups x 4 rows of the row loop (512 x 4 of the strided one)"""
    _case(V, dtype, "normal", 64, 151, (5,), poisons=("nan",))


# ------------------------------------------------------------------------------------------------------------------ 2. real decoder --
def _live(lengths, T):
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def test_f32_vs_oracle():
    V = 33
    img, f, l = batch(4, H, W, V, 5, 12, seed=11)
    eng = Engine(V, dtype="f32", seed=3)
    P = oracle_params(eng)
    with torch.no_grad():
        lg = R.decoder_train(P, R.encoder(P, torch.from_numpy(img)), torch.from_numpy(f.astype(np.int64))).double()
    ref = F.log_softmax(lg, dim=-1).numpy()
    h = -(np.exp(ref) * ref).sum(-1)
    live = _live(l, f.shape[1])
    for k in (1, 5, 16):
        logp, top1, seq, alt = eng.score(img, f, l, return_top1=True, alternatives=k)
        assert alt.ids.shape == f.shape + (k,) and alt.rank.shape == f.shape and np.array_equal(alt.ids[..., 0], top1)
        worst = check_against_oracle(ref, alt.ids, alt.logp, alt.rank, f, l, V)
        eh = np.abs(alt.entropy - h)[live].max()
        print("f32 k=%d: |logp - oracle| max %.2e, |H - oracle| max %.2e" % (k, worst, eh))
        assert eh < 1e-5 * (2 + h[live].max())
        assert (alt.ids[~live] == -1).all() and (alt.logp[~live] == 0).all() and (alt.rank[~live] == -1).all() and (alt.entropy[~live] == 0).all()


@pytest.mark.parametrize("B", [8, 3])
def test_bf16_vs_f32(B):
    """bf16 against the f32 run of the same inputs and weights, slot by slot: order statistics move by no more than the values do, so a
    swap at a near-tie stays inside the per-token bar; B = 3 is filled up to a chain batch with dead rows that the result does not show"""
    from test_gpu_benchcfg import count_set, V
    imgs, forms = count_set(B, 909)
    img = pad_batch_images(imgs)
    f, l = pad_batch_formulas(forms, V - 2, V - 1)
    e32, e16 = Engine(V, dtype="f32", seed=2), Engine(V, dtype="bf16", seed=2)
    a32, a16 = e32.score(img, f, l, alternatives=5)[-1], e16.score(img, f, l, alternatives=5)[-1]
    assert e16.chain_used and e16.shape.B == 8 and (e16.shape.live_B == B if B != 8 else True)
    live = _live(l, f.shape[1])
    for a in a16:
        assert a.shape[:2] == (B, f.shape[1])
    err = np.abs(a16.logp - a32.logp)[live].max()
    eh = np.abs(a16.entropy - a32.entropy)[live].max()
    same = (a16.ids == a32.ids)[live].mean()
    print("bf16 vs f32 B=%d: |logp| max %.2e, |H| max %.2e, ids equal at %.4f of the slots" % (B, err, eh, same))
    assert err <= BF16_BATCH_TOL
    gap = np.abs(np.diff(a32.logp, axis=-1)).min(-1)                            # where no two f32 candidates are close the ids agree
    clear = live & (gap > 2 * BF16_BATCH_TOL)
    assert np.array_equal(a16.ids[clear][:, :4], a32.ids[clear][:, :4])
    assert (a16.ids[~live] == -1).all() and (a16.entropy[~live] == 0).all() and (a16.entropy[live] > 0).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_split_is_bit_identical_to_scoring_the_pieces(dtype):
    V = 33
    img, f, l = batch(70, H, W, V, 5, 12, seed=7)
    eng = Engine(V, dtype=dtype, seed=1, deterministic=True)
    al = np.random.default_rng(0).random((70, V)) >= 0.25
    for allowed in (None, al):
        whole = eng.score(img, f, l, return_top1=True, alternatives=3, allowed=allowed)
        a = eng.score(img[:64], f[:64], l[:64], return_top1=True, alternatives=3, allowed=None if allowed is None else allowed[:64])
        b = eng.score(img[64:], f[64:], l[64:], return_top1=True, alternatives=3, allowed=None if allowed is None else allowed[64:])
        for w, p0, p1 in zip(whole[:3] + tuple(whole[3]), a[:3] + tuple(a[3]), b[:3] + tuple(b[3])):
            assert w.shape[0] == 70 and w.tobytes() == np.concatenate([p0, p1]).tobytes()


def test_drivers(tmp_path, monkeypatch):
    from PIL import Image
    from latex_ocr_amd.model.utils.image import greyscale
    monkeypatch.chdir(tmp_path)
    m, d = _results_dir(str(tmp_path))
    png = sorted(p for p in os.listdir("data/synthetic/test") if p.endswith(".png"))[0]
    img = greyscale(np.asarray(Image.open("data/synthetic/test/" + png).convert("RGB")))
    hyps, scores, alts = m.predict_batch([img], alternatives=3)
    assert len(alts) == len(hyps) and all(len(alts[i][0]) == len(scores[i][0][1]) for i in range(len(hyps)))
    h2, s2, a2 = m.complete_batch([img], ["t1 t2"], alternatives=3)
    assert h2[0][0].split()[:2] == ["t1", "t2"] and len(a2[0][0]) == len(s2[0][0][1]) and len(a2[0][0][0]["alternatives"]) == 3
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--alternatives", "3",
                                   "data/synthetic/test/" + png], cwd=str(tmp_path), timeout=600, env=env).decode()
    rows = [x for x in out.splitlines() if " rank " in x and " entropy " in x]
    assert len(rows) == len(alts[0][0]) and "=>" in out, out
    for row, e in zip(rows, alts[0][0]):                                        # (another process: compared away from near-ties only)
        cand = row.split("|")[1].split()
        assert len(cand) == 6 and -1 <= int(row.split(" rank ")[1].split()[0]) < m._vocab.n_tok
        if e["alternatives"][0][1] - e["alternatives"][1][1] > 1e-3:
            assert cand[0] == e["alternatives"][0][0] and float(cand[1]) == pytest.approx(e["alternatives"][0][1], abs=1e-3)
    formula = "t1 t2 t3 zz t4"
    res = m.score_batch([img], [formula], alternatives=3)[0]
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "predict.py"), "--results", d, "--alternatives", "3", "--formula", formula,
                                   "data/synthetic/test/" + png], cwd=str(tmp_path), timeout=600, env=env).decode()
    rows = [x for x in out.splitlines() if " rank " in x and " entropy " in x]
    assert len(rows) == 6 == len(res[3]) and "first disagreement" in out
    for row, e, lp in zip(rows, res[3], res[1]):
        assert float(row.split(" logp ")[1].split()[0]) == pytest.approx(lp, abs=1e-3) and len(row.split("|")[1].split()) == 6
