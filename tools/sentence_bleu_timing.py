"""What the sentence-level BLEU cost costs (bf16, V = 500, 128 x 512; ids of a real sample_decode to the 152-step bound).

Alternating rounds of one process, medians of --reps with ranges, the shapes warmed up, host clock around --calls calls back to back that end in a
device synchronise.
 Arm 1, B = 64 images x n = 5 draws = 320 pairs against references of 95 .. 104 tokens:
  (a) lxo_sentence_bleu on the ids where the decode left them: one launch, no Levenshtein DP, the float tail in the kernel.
  (b) the same values from what there was before it: lxo_text_stats' rows (with its DP and its reduction launch spared: rows only) and a torch tail.
 Arm 2, B = 64 at n = 5 and n = 16:
  (a) lxo_consensus_bleu: B n (n - 1) / 2 waves, one count per unordered pair, the select launch.
  (b) the same result from a transposed contiguous copy of the ids, lxo_text_stats over all n^2 ordered pairs of an image through ref_index, the
      torch tail, a torch reduction and arg-min.
 Each (b) is compared with its (a) before anything is timed.  Prints one line per arm: median (min..max)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.engine import Engine, _p
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import pad_batch_formulas

V, B, H, W, MAX_ITER = 500, 64, 128, 512, 151
END, PAD = V - 1, V - 2
arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
reps, calls, sizes = arg("--reps", 5), arg("--calls", 200), [int(x) for x in (sys.argv[sys.argv.index("--n") + 1].split(",") if "--n" in sys.argv else ("5", "16"))]
B = arg("--batch", B)
NS = _abi.LXO_TEXT_STATS


def report(name, v, unit, base=None):
    v = sorted(v)
    print("%s: %s median of %d %.3f (%.3f..%.3f)%s" % (name, unit, len(v), v[len(v) // 2], v[0], v[-1],
                                                        "" if base is None else ", ratio to the first arm %.4f" % (v[len(v) // 2] / base)))
    return v[len(v) // 2]


def alternate(arms, unit):
    per = [[] for _ in arms]
    for r in range(reps):
        for i in (range(len(arms)) if r % 2 == 0 else reversed(range(len(arms)))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                arms[i][1]()
            torch.cuda.synchronize()
            per[i].append((time.perf_counter() - t0) * 1e6 / calls)
    base = None
    for (name, _), v in zip(arms, per):
        m = report(name, v, unit, base)
        base = m if base is None else base


def torch_tail(stats):
    """include/lxo.h's sentence BLEU from lxo_text_stats' rows, f32"""
    s = stats.to(torch.float32)
    p = torch.cat([s[:, 0:1] / s[:, 4:5], (s[:, 1:4] + 1) / (s[:, 5:8] + 1)], dim=1)
    h, r = s[:, 8], s[:, 9]
    bp = torch.where(h > r, torch.ones_like(h), torch.exp(1 - r / h.clamp(min=1)))
    b = bp * torch.exp(0.25 * torch.log(p.clamp(min=1e-30)).sum(dim=1))
    b = torch.where(stats[:, 0] == 0, torch.zeros_like(b), b)
    return torch.where(stats[:, 11] == 1, torch.ones_like(b), b)


eng = Engine(V, dtype="bf16", seed=0)
imgs, forms = synthetic.make_set(B, H, W, V, 95, 105, seed=5)
img = pad_batch_images(imgs)
refs, rl = pad_batch_formulas(forms, PAD, END)
refs_d, rl_d = torch.from_numpy(refs).cuda(), torch.from_numpy(rl).cuda()
unit = "us per call (%d calls back to back)" % calls

for n in sizes:
    ids, _, _, _, steps, _ = eng._sample_device(img, END, n, 1.0, 0, 1.0, 1, MAX_ITER)
    view = ids[:, :steps]
    geom = (n, int(view.stride(0)), int(view.stride(2)), int(view.stride(1)))
    if n == sizes[0]:
        pairs = B * n
        bleu = torch.empty(pairs, dtype=torch.float32, device="cuda")
        stats = torch.empty(pairs, NS, dtype=torch.int32, device="cuda")
        res = [None]

        def arm1_a():
            eng._ck(eng.lib.lxo_sentence_bleu(_p(view), geom[0], geom[1], geom[2], geom[3], steps, None, _p(refs_d), B, refs.shape[1], _p(rl_d), None, n, pairs,
                                              END, None, _p(bleu), None, eng._stream()), "sentence_bleu")

        def arm1_b():
            eng._ck(eng.lib.lxo_text_stats(_p(view), geom[0], geom[1], geom[2], geom[3], steps, None, _p(refs_d), B, refs.shape[1], _p(rl_d), None, n, pairs,
                                           END, _p(stats), None, 0, eng._stream()), "text_stats")
            res[0] = torch_tail(stats)

        for _ in range(3):
            arm1_a()
            arm1_b()
        torch.cuda.synchronize()
        print("arm 1: %d pairs, %d steps, hypotheses of %d .. %d tokens (mean %.1f), sBLEU %.4f .. %.4f; max |(a) - (b)| %.3e"
              % (pairs, steps, int(stats[:, 8].min()), int(stats[:, 8].max()), float(stats[:, 8].float().mean()), float(bleu.min()), float(bleu.max()),
                 float((bleu - res[0]).abs().max())))
        assert float((bleu - res[0]).abs().max()) <= 2e-5, "the composed arm's scores differ"
        alternate([("1 (a) lxo_sentence_bleu, %d pairs" % pairs, arm1_a), ("1 (b) lxo_text_stats rows + torch tail, %d pairs" % pairs, arm1_b)], unit)

    cost = torch.empty(B, n, n, dtype=torch.float32, device="cuda")
    risk = torch.empty(B, n, dtype=torch.float32, device="cuda")
    best = torch.empty(B, dtype=torch.int32, device="cuda")

    def arm2_a():
        eng._ck(eng.lib.lxo_consensus_bleu(_p(view), geom[1], geom[2], geom[3], B, n, steps, END, None, None, _p(cost), _p(risk), _p(best), eng._stream()),
                "consensus_bleu")

    pairs2 = B * n * n
    p = torch.arange(pairs2, device="cuda")
    ref_of = ((p // (n * n)) * n + p % n).to(torch.int32)            # pair (g, i, j): the reference is row g n + j
    stats2 = torch.empty(pairs2, NS, dtype=torch.int32, device="cuda")
    res2 = [None, None, None]

    def arm2_b():
        rows = view.permute(0, 2, 1).contiguous().view(B * n, steps)
        eng._ck(eng.lib.lxo_text_stats(_p(rows), n, steps, 0, 1, steps, None, _p(rows), B * n, steps, None, _p(ref_of), 1, pairs2, END, _p(stats2), None, 0,
                                       eng._stream()), "text_stats")
        res2[2] = (1 - torch_tail(stats2)).view(B, n, n)
        res2[0] = res2[2].sum(dim=2) / n
        res2[1] = res2[0].argmin(dim=1)

    for _ in range(3):
        arm2_a()
        arm2_b()
    torch.cuda.synchronize()
    agree = int((res2[1].to(torch.int32) == best).sum())
    print("arm 2, B = %d, n = %d: %d steps; (b) chooses as (a) on %d of %d images, max |cost difference| %.3e, max |risk difference| %.3e"
          % (B, n, steps, agree, B, float((res2[2] - cost).abs().max()), float((res2[0] - risk).abs().max())))
    assert float((res2[2] - cost).abs().max()) <= 2e-5, "the composed arm's costs differ"
    alternate([("2 (a) lxo_consensus_bleu, B = %d n = %d" % (B, n), arm2_a),
               ("2 (b) copy + lxo_text_stats over n^2 pairs + torch tail, reduction, arg-min, B = %d n = %d" % (B, n), arm2_b)], unit)
