"""What the text metrics cost on the device and on the host (bf16, V = 500, 128 x 512; 64 x 5 pairs of ids of a real sample_decode to the 152-step
bound, each draw against a reference of about 100 tokens).

Alternating rounds of one process, medians of --reps with ranges, the shapes warmed up:
 (a) Engine.text_metrics on host rows: two uploads, the launches, the one copy of 14 integers, scores_from_counts.
 (b) the host bleu_score + edit_distance + exact_match_score on the same cut lists.
 (c) Engine.edit_distance alone on the same pairs (host rows in, distances out): what there was before, and what the n-gram counting adds to.
Then the launches alone on device-resident ids, --calls calls back to back that end in a device synchronise: lxo_text_stats with the rows and the
reduction, lxo_text_stats into the corpus alone, lxo_edit_distance.  (a)'s dict is compared with (b)'s first.
--kernels-only runs just those launches a few times (for a kernel trace of its own).  Prints one line per arm: median (min..max)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine, _p
from latex_ocr_amd.model.evaluation.text import bleu_score, edit_distance, exact_match_score, truncate_end
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import pad_batch_formulas

V, B, N, H, W, MAX_ITER = 500, 64, 5, 128, 512, 151
END, PAD = V - 1, V - 2
arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
reps, calls = arg("--reps", 5), arg("--calls", 200)


def report(name, v, unit, base=None):
    v = sorted(v)
    print("%s: %s median of %d %.3f (%.3f..%.3f)%s" % (name, unit, len(v), v[len(v) // 2], v[0], v[-1],
                                                        "" if base is None else ", ratio to the first arm %.4f" % (v[len(v) // 2] / base)))
    return v[len(v) // 2]


def alternate(arms, timed, unit):
    per = [[] for _ in arms]
    for r in range(reps):
        for i in (range(len(arms)) if r % 2 == 0 else reversed(range(len(arms)))):
            per[i].append(timed(arms[i][1]))
    base = None
    for (name, _), v in zip(arms, per):
        m = report(name, v, unit, base)
        base = m if base is None else base


def timed_calls(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def timed_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


eng = Engine(V, dtype="bf16", seed=0)
imgs, forms = synthetic.make_set(B, H, W, V, 95, 105, seed=5)
ids, _, _, _, steps, _ = eng._sample_device(pad_batch_images(imgs), END, N, 1.0, 0, 1.0, 1, MAX_ITER)
view = ids[:, :steps]                                               # [B, steps, n] where the decode left it
ref, rl = pad_batch_formulas(forms, PAD, END)
ref_d, rl_d = torch.from_numpy(ref).cuda(), torch.from_numpy(rl).cuda()
pairs, Tr = B * N, int(ref.shape[1])
rows = np.ascontiguousarray(view.cpu().numpy().transpose(0, 2, 1)).reshape(pairs, steps)      # host rows [pairs, steps], pair b n + j
hyps = [[int(x) for x in truncate_end(r, END)] for r in rows]
refs = [[int(x) for x in forms[p // N]] for p in range(pairs)]
print("%d pairs: %d steps, hypothesis lengths %d..%d (mean %.1f), reference lengths %d..%d" % (pairs, steps, min(map(len, hyps)), max(map(len, hyps)),
      float(np.mean([len(h) for h in hyps])), min(map(len, refs)), max(map(len, refs))))

stats = torch.empty(pairs, 12, dtype=torch.int32, device="cuda")
corpus = torch.zeros(14, dtype=torch.int64, device="cuda")
dist = torch.empty(pairs, dtype=torch.int32, device="cuda")
geom = (N, int(view.stride(0)), int(view.stride(2)), int(view.stride(1)), steps)


def k_text(want_rows):
    eng._ck(eng.lib.lxo_text_stats(_p(view), *geom, None, _p(ref_d), B, Tr, _p(rl_d), None, N, pairs, END, _p(stats) if want_rows else None, _p(corpus), 0,
                                   eng._stream()), "text_stats")


def k_edit():
    eng._ck(eng.lib.lxo_edit_distance(_p(view), *geom, None, _p(ref_d), B, Tr, _p(rl_d), None, N, pairs, END, _p(dist), None, eng._stream()), "edit_distance")


for _ in range(3):
    k_text(True)
    k_text(False)
    k_edit()
torch.cuda.synchronize()
assert torch.equal(stats[:, 10], dist), "the distance column differs from lxo_edit_distance's"
if "--kernels-only" in sys.argv:
    sys.exit(0)

host = lambda: {"BLEU-4": bleu_score(refs, hyps) * 100, "ExactMatchScore": exact_match_score(refs, hyps) * 100, "EditDistance": edit_distance(refs, hyps) * 100}
dev = lambda: eng.text_metrics(rows, ref, ref_lengths=rl, id_end=END)
assert dev() == host(), "the device metrics differ from the host's"
print("scores: %s" % dev())
eng.edit_distance(rows, ref, ref_lengths=rl, id_end=END)
alternate([("(a) Engine.text_metrics, %d pairs" % pairs, dev), ("(b) host bleu_score + edit_distance + exact_match_score", host),
           ("(c) Engine.edit_distance, %d pairs" % pairs, lambda: eng.edit_distance(rows, ref, ref_lengths=rl, id_end=END))], timed_once,
          "ms per call (host arrays in, host values out)")
alternate([("lxo_edit_distance", k_edit), ("lxo_text_stats, rows + reduction", lambda: k_text(True)), ("lxo_text_stats, corpus alone", lambda: k_text(False))],
          timed_calls, "us per call (%d calls back to back, ids on the device)" % calls)
