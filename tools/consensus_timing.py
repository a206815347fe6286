"""What the consensus choice among sampled transcriptions costs (bf16, V = 500, 128 x 512; ids of a real sample_decode to the 152-step bound).

At B = 64 images with n = 5 and with n = 16 draws, alternating rounds of one process, medians of --reps with ranges, the shapes warmed up, host
clock around --calls calls back to back that end in a device synchronise:
 (a) lxo_consensus on the ids where the decode left them: B n (n - 1) / 2 waves of DP, the select launch.
 (b) the same result from the entry points there were before it: a transposed contiguous copy of the ids, lxo_edit_distance over all n^2 ordered
     pairs of an image through ref_index, a torch reduction and arg-min.  Its distances and choices are compared with (a)'s first.
 (c) B = 10, n = 5 only: the host loop -- truncate_end and levenshtein over the unordered pairs, the risk in numpy -- on ids already on the host.
Then Engine.sample_decode(return_consensus=True) against the same call without it, whole calls, in the same rounds.
Prints one line per arm: median (min..max)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine, _p
from latex_ocr_amd.model.evaluation.text import levenshtein, truncate_end
from latex_ocr_amd.model.utils.image import pad_batch_images

V, B, H, W, MAX_ITER = 500, 64, 128, 512, 151
END = V - 1
arg = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
reps, calls, sizes = arg("--reps", 5), arg("--calls", 200), [int(x) for x in (sys.argv[sys.argv.index("--n") + 1].split(",") if "--n" in sys.argv else ("5", "16"))]
B = arg("--batch", B)


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


def host_consensus(ids):
    out = []
    for g in range(ids.shape[0]):
        s = [list(truncate_end(ids[g, :, j], END)) for j in range(ids.shape[2])]
        n = len(s)
        d = np.zeros((n, n))
        for i in range(n):
            for j in range(i + 1, n):
                d[i, j] = d[j, i] = levenshtein(s[i], s[j])
        risk = (d / np.array([max(len(x), 1) for x in s])[None, :]).sum(axis=1) / n
        out.append((int(np.argmin(risk)), risk))
    return out


eng = Engine(V, dtype="bf16", seed=0)
imgs, _ = synthetic.make_set(B, H, W, V, 95, 105, seed=5)
img = pad_batch_images(imgs)

for n in sizes:
    ids, _, _, _, steps, _ = eng._sample_device(img, END, n, 1.0, 0, 1.0, 1, MAX_ITER)
    view = ids[:, :steps]
    dist = torch.empty(B, n, n, dtype=torch.int32, device="cuda")
    risk = torch.empty(B, n, dtype=torch.float32, device="cuda")
    best = torch.empty(B, dtype=torch.int32, device="cuda")

    def arm_a():
        eng._ck(eng.lib.lxo_consensus(_p(view), int(view.stride(0)), int(view.stride(2)), int(view.stride(1)), B, n, steps, END, None, 1,
                                      _p(dist), _p(risk), _p(best), eng._stream()), "consensus")

    pairs = B * n * n
    p = torch.arange(pairs, device="cuda")
    ref_of = ((p // (n * n)) * n + p % n).to(torch.int32)            # pair (g, i, j): the reference is row g n + j
    d_b = torch.empty(pairs, dtype=torch.int32, device="cuda")
    c_b = torch.empty(pairs, dtype=torch.float32, device="cuda")
    res_b = [None, None]

    def arm_b():
        rows = view.permute(0, 2, 1).contiguous().view(B * n, steps)
        eng._ck(eng.lib.lxo_edit_distance(_p(rows), n, steps, 0, 1, steps, None, _p(rows), B * n, steps, None, _p(ref_of), 1, pairs, END,
                                          _p(d_b), _p(c_b), eng._stream()), "edit_distance")
        res_b[0] = c_b.view(B, n, n).sum(dim=2) / n
        res_b[1] = res_b[0].argmin(dim=1)

    for _ in range(3):
        arm_a()
        arm_b()
    torch.cuda.synchronize()
    lens = [len(truncate_end(ids[0, :steps, j].cpu().numpy(), END)) for j in range(n)]
    assert torch.equal(d_b.view(B, n, n), dist), "the composed arm's distances differ"
    agree = int((res_b[1].to(torch.int32) == best).sum())
    print("B = %d, n = %d: %d steps, lengths of image 0's draws %s, %d distinct distances; (b) chooses as (a) on %d of %d images, max |risk difference| %.3e"
          % (B, n, steps, lens, int(torch.unique(dist).numel()), agree, B, float((res_b[0] - risk).abs().max())))
    alternate([("(a) lxo_consensus, B = %d n = %d" % (B, n), arm_a), ("(b) copy + lxo_edit_distance over n^2 pairs + torch, B = %d n = %d" % (B, n), arm_b)],
              timed_calls, "us per call (%d calls back to back)" % calls)
    if n == 5:
        h = np.ascontiguousarray(ids[:10, :steps].cpu().numpy())
        want = host_consensus(h)
        assert [w[0] for w in want] == best[:10].cpu().tolist(), "the host loop chooses otherwise"
        sub = ids[:10, :steps]
        d10, r10, b10 = dist[:10].clone(), risk[:10].clone(), best[:10].clone()

        def arm_a10():
            eng._ck(eng.lib.lxo_consensus(_p(sub), int(sub.stride(0)), int(sub.stride(2)), int(sub.stride(1)), 10, n, steps, END, None, 1,
                                          _p(d10), _p(r10), _p(b10), eng._stream()), "consensus")
            return b10.cpu()
        arm_a10()
        alternate([("(c) host truncate_end + levenshtein loop, B = 10 n = 5", lambda: host_consensus(h)),
                   ("(a) lxo_consensus and its best copied out, B = 10 n = 5", arm_a10)], timed_once, "ms per call")

    kw = dict(n=n, temperature=1.0, seed=1, max_iter=MAX_ITER)
    eng.sample_decode(img, END, **kw)
    eng.sample_decode(img, END, return_consensus=True, **kw)
    alternate([("sample_decode, B = %d n = %d" % (B, n), lambda: eng.sample_decode(img, END, **kw)),
               ("sample_decode(return_consensus=True), B = %d n = %d" % (B, n), lambda: eng.sample_decode(img, END, return_consensus=True, **kw))],
              timed_once, "ms per call (images in, host arrays out)")
