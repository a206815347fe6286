"""What finishing a beam on the device costs (bf16, V = 500, B = 64, 128 x 512, beam 5, max_iter 151).

Alternating rounds of one process, medians of --reps with ranges, the shapes warmed up.
 1. The two launches alone on the buffers a real beam decode left, --calls calls back to back that end in a device synchronise: lxo_beam_finalize
    (all five outputs), lxo_beam_rerank (length penalty, no coverage), and both behind each other.
 2. beam_decode(return_scores=True, return_nbest=True) against the host route for the same outputs: beam_decode(return_scores=True), then
    utils/text.beam_backtrace on ids and scores, the END cut and the differences in numpy.
 3. With --consensus: beam_decode(return_nbest=True, return_consensus=True) against the host route of 2 followed by truncate_end + levenshtein
    over the k^2 pairs of every image and the posterior-weighted risk.
The device's hypotheses are compared with the host route's first.  Prints one line per arm: median (min..max)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.evaluation.text import levenshtein, truncate_end
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import beam_backtrace

V, B, H, W, K, MAX_ITER = 500, 64, 128, 512, 5, 151
END = V - 1
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
imgs, _ = synthetic.make_set(B, H, W, V, 95, 100, seed=5)
img = pad_batch_images(imgs)


def host_route():
    ids, par, sc = eng.beam_decode(img, END, K, max_iter=MAX_ITER, return_scores=True)
    hyp, run = beam_backtrace(ids, par), beam_backtrace(sc, par)
    n = ids.shape[1]
    hit = hyp == END
    ln = np.where(hit.any(1), hit.argmax(1) + 1, n).astype(np.int32)
    live = np.arange(n)[None, :, None] < ln[:, None, :]
    tok = np.where(live, np.diff(run, axis=1, prepend=np.float32(0)), np.float32(0))
    seq = np.take_along_axis(run, (ln - 1)[:, None, :], axis=1)[:, 0]
    return np.where(live, hyp, END), ln, tok, seq


def host_consensus():
    hyp, ln, tok, seq = host_route()
    e = np.exp(seq.astype(np.float64) - seq.max(1, keepdims=True))
    post = e / e.sum(1, keepdims=True)
    best = []
    for b in range(B):
        s = [truncate_end([int(x) for x in hyp[b, :, i]], END) for i in range(K)]
        d = np.array([[levenshtein(s[i], s[j]) / float(max(len(s[j]), 1)) if i != j else 0.0 for j in range(K)] for i in range(K)])
        best.append(int(np.argmin((d * post[b][None, :]).sum(1) / post[b].sum())))
    return hyp, best


for _ in range(2):
    out = eng.beam_decode(img, END, K, max_iter=MAX_ITER, return_scores=True, return_nbest=True)
    ref = host_route()
nb = out[3]
n = out[0].shape[1]
print("B %d, beam %d, steps run %d, hypothesis lengths %d..%d" % (B, K, n, nb.lengths.min(), nb.lengths.max()))
assert np.array_equal(nb.hyp, ref[0]) and np.array_equal(nb.lengths, ref[1]) and nb.tok_logp.tobytes() == ref[2].astype(np.float32).tobytes() \
    and nb.seq_logp.tobytes() == np.ascontiguousarray(ref[3]).tobytes(), "the device's n-best differs from the host route's"

ids, par, sc = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in out[:3])
fin = eng._beam_finalize(ids, par, sc, B, n, n, K, END)
alternate([("1a lxo_beam_finalize, five outputs", lambda: eng._beam_finalize(ids, par, sc, B, n, n, K, END)),
           ("1b lxo_beam_rerank, length penalty 0.6", lambda: eng._beam_rerank(fin.lengths, fin.seq_logp, None, 0.6, 0.0, 0.01)),
           ("1c both", lambda: eng._beam_rerank(*(eng._beam_finalize(ids, par, sc, B, n, n, K, END)[i] for i in (1, 4)), None, 0.6, 0.0, 0.01))],
          timed_calls, "us per call (%d calls back to back, the output tensors allocated per call)" % calls)
if "--kernels-only" in sys.argv:
    sys.exit(0)
alternate([("2a beam_decode(return_scores=True, return_nbest=True)", lambda: eng.beam_decode(img, END, K, max_iter=MAX_ITER, return_scores=True, return_nbest=True)),
           ("2b beam_decode(return_scores=True) + the host back-trace, END cut and differences", host_route),
           ("2c beam_decode(return_scores=True) alone", lambda: eng.beam_decode(img, END, K, max_iter=MAX_ITER, return_scores=True))], timed_once, "ms per call")
if "--consensus" in sys.argv:
    dev = eng.beam_decode(img, END, K, max_iter=MAX_ITER, return_nbest=True, return_consensus=True)
    same = np.mean(np.asarray(host_consensus()[1]) == dev[2])
    print("consensus choices equal to the host loop's (float64 risk; f32 near-ties may differ): %.3f of %d" % (same, B))
    alternate([("3a beam_decode(return_nbest=True, return_consensus=True)", lambda: eng.beam_decode(img, END, K, max_iter=MAX_ITER, return_nbest=True, return_consensus=True)),
               ("3b the host route + truncate_end + levenshtein over k^2 pairs", host_consensus)], timed_once, "ms per call")
