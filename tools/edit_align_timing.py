"""What the edit alignment costs on the device and on the host (bf16, V = 500, 128 x 512; 64 x 5 pairs of ids of a real sample_decode to the 152-step
bound, each draw against a reference of about 100 tokens).

Alternating rounds of one process, medians of --reps with ranges, the shapes warmed up.  The launches on device-resident ids, --calls calls back to
back that end in a device synchronise:
 1. lxo_edit_distance alone: the kernel there was before, the baseline.
 2. lxo_edit_align with the counts only.
 3. with the two maps as well.
 4. with the maps and the confusion matrix at V = 500 (and the corpus row), added into.
Then, host lists in and the report out, once per round:
 5. the host align loop on the same lists with the sums and error_report.
 6. Img2SeqModel.error_analysis on the same lists.
The device's counts, maps and report are compared with the host's first.  Prints one line per arm: median (min..max)."""
import os, sys, time, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine, _p
from latex_ocr_amd.model.evaluation.text import align, error_report, truncate_end
from latex_ocr_amd.model.img2seq import Img2SeqModel
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

dist = torch.empty(pairs, dtype=torch.int32, device="cuda")
counts = torch.empty(pairs, 6, dtype=torch.int32, device="cuda")
ha, ra = torch.empty(pairs, steps, dtype=torch.int32, device="cuda"), torch.empty(pairs, Tr, dtype=torch.int32, device="cuda")
corpus, conf = torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(V + 1, V + 1, dtype=torch.int64, device="cuda")
need = int(eng.lib.lxo_edit_align_scratch_bytes(pairs, steps, Tr))
scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
geom = (N, int(view.stride(0)), int(view.stride(2)), int(view.stride(1)), steps)
print("scratch %d bytes (%d per pair)" % (need, need // pairs))


def k_edit():
    eng._ck(eng.lib.lxo_edit_distance(_p(view), *geom, None, _p(ref_d), B, Tr, _p(rl_d), None, N, pairs, END, _p(dist), None, eng._stream()), "edit_distance")


def k_align(maps, matrix):
    eng._ck(eng.lib.lxo_edit_align(_p(view), *geom, None, _p(ref_d), B, Tr, _p(rl_d), None, N, pairs, END, _p(ha) if maps else None, _p(ra) if maps else None,
                                   _p(counts), _p(corpus) if matrix else None, _p(conf) if matrix else None, V, 1, _p(scratch), need, eng._stream()), "edit_align")


def host_loop():
    al = [align(h, r) for h, r in zip(hyps, refs)]
    C = np.zeros((V + 1, V + 1), np.int64)
    for (h, r), (a, b, _) in zip(zip(hyps, refs), al):
        for i, j in enumerate(a):
            C[V if j < 0 else r[j], h[i]] += 1
        for j, i in enumerate(b):
            if i < 0:
                C[r[j], V] += 1
    c = np.array([x for _, _, x in al], np.int64)
    return error_report(list(c.sum(0)) + [len(al), 0], C, {}), al


model = Img2SeqModel.__new__(Img2SeqModel)                          # error_analysis reads the vocabulary's END, size and names and the engine, nothing else
model._vocab, model.engine = types.SimpleNamespace(id_end=END, n_tok=V, id_to_tok={}), eng

for _ in range(3):
    k_edit()
    k_align(False, False)
    k_align(True, False)
    k_align(True, True)
torch.cuda.synchronize()
assert torch.equal(counts[:, 1:4].sum(1).int(), dist), "S + I + D differs from lxo_edit_distance's"
want, al = host_loop()
assert np.array_equal(counts.cpu().numpy(), [x for _, _, x in al]), "the device counts differ from the host align's"
hm, rm = ha.cpu().numpy(), ra.cpu().numpy()
assert all(hm[p, :len(a)].tolist() == a and rm[p, :len(b)].tolist() == b for p, (a, b, _) in enumerate(al)), "the device maps differ from the host align's"
got = model.error_analysis(refs, hyps)
assert got == want, "error_analysis differs from the host loop"
print("report: S %d I %d D %d of %d reference tokens; SubRate %.2f InsRate %.2f DelRate %.2f" % (got["substitutions"], got["insertions"], got["deletions"],
      got["ref_tokens"], got["SubRate"], got["InsRate"], got["DelRate"]))
if "--kernels-only" in sys.argv:
    sys.exit(0)

alternate([("1 lxo_edit_distance", k_edit), ("2 lxo_edit_align, counts only", lambda: k_align(False, False)), ("3 lxo_edit_align, counts + maps", lambda: k_align(True, False)),
           ("4 lxo_edit_align, counts + maps + corpus + confusion at V = %d" % V, lambda: k_align(True, True))], timed_calls,
          "us per call (%d calls back to back, ids on the device)" % calls)
alternate([("5 host align loop + error_report, %d pairs" % pairs, host_loop), ("6 Img2SeqModel.error_analysis, %d pairs" % pairs, lambda: model.error_analysis(refs, hyps))],
          timed_once, "ms per call (host lists in, the report out)")
