"""What a minimum-risk batch costs with the candidates built on the host and on the device (bf16, V = 500, 128 x 512).

1. Img2SeqModel.mrt_batch on B = 10 images, n = 5 draws, the reference included (60 candidate rows, the chain batch of 64): the host arm
   (on_device=False: the ids copied out, truncate_end / levenshtein / pad_batch_formulas in Python, Engine.mrt_step) against the device arm
   (on_device=True: Engine.mrt_sample_step), host clock around whole calls, alternating rounds of one process; medians of --reps with ranges.
2. The candidate stage alone (lxo_mrt_candidates: three launches) on the ids of one sampled decode, between device events.
3. Engine.edit_distance on 384 pairs of about 100 tokens (host arrays in, host arrays out) against the host levenshtein on the same pairs.
Prints one line per arm: median (min..max)."""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import _p
from latex_ocr_amd.model.evaluation.text import levenshtein
from latex_ocr_amd.model.img2seq import Img2SeqModel
from latex_ocr_amd.model.utils.general import Config
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import Vocab, pad_batch_formulas

V, B, N = 500, 10, 5
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 2
launches = int(sys.argv[sys.argv.index("--launches") + 1]) if "--launches" in sys.argv else 50


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


tmp = tempfile.mkdtemp()
with open(os.path.join(tmp, "vocab.txt"), "w") as fh:
    fh.write("\n".join("t%d" % i for i in range(V - 3)) + "\n")                      # + _UNK, _PAD, _END: V ids
vocab = Vocab(Config({"unk": "_UNK", "pad": "_PAD", "end": "_END", "path_vocab": os.path.join(tmp, "vocab.txt")}))
assert vocab.n_tok == V
imgs, forms = synthetic.make_set(B, 128, 512, V, 95, 105, seed=5)                # references of about 100 tokens
forms = [[int(t) for t in f] for f in forms]


def model():
    m = Img2SeqModel(Config({"compute_dtype": "bf16", "max_length_formula": 150, "decoding": "greedy"}), os.path.join(tmp, "out") + "/", vocab)
    m.build_pred()
    return m


# ---- 1. mrt_batch, host arm against device arm
m_host, m_dev = model(), model()
kw = dict(n=N, alpha=0.005, temperature=1.0)
count = [0]


def batch_arm(m, on_device):
    def fn():
        count[0] += 1
        return m.mrt_batch(imgs, forms, 1e-4, seed=count[0], on_device=on_device, **kw)
    return fn


def timed_steps(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


arms = [("mrt_batch, candidates on the host", batch_arm(m_host, False)), ("mrt_batch, candidates on the device", batch_arm(m_dev, True))]
for _, fn in arms:
    out = fn()
print("rows per batch: %d of %d" % (sum(len(g) for g in out["candidates"]), B * (N + 1)))
alternate(arms, timed_steps, "ms per batch (images in, risk and candidates out)")
print("chains: host arm %s/%s, device arm %s/%s" % (m_host.engine.chain_used, m_host.engine.chain_used_bwd, m_dev.engine.chain_used, m_dev.engine.chain_used_bwd))

# ---- 2. the candidate stage alone
eng = m_dev.engine
img = pad_batch_images(imgs)
ref, rl = pad_batch_formulas(forms, vocab.id_pad, vocab.id_end)
ids, _, _, _, nsteps, _ = eng._sample_device(img, vocab.id_end, N, 1.0, 0, 1.0, 1, 151)
R, Tr = B * (N + 1), ref.shape[1]
Tc = max(nsteps + 1, Tr)
ref_d, rl_d = torch.from_numpy(ref).cuda(), torch.from_numpy(rl).cuda()
o = [torch.empty(s, dtype=torch.int32, device="cuda") for s in (R * Tc, R, R, B + 1, R)]


def candidates():
    eng._ck(eng.lib.lxo_mrt_candidates(_p(ids), B, int(ids.shape[1]), N, nsteps, _p(ref_d), Tr, _p(rl_d), vocab.id_end, vocab.id_pad, 1,
                                       _p(o[0]), _p(o[1]), _p(o[2].view(torch.float32)), _p(o[3]), _p(o[4]), eng._stream()), "mrt_candidates")


def timed_launches(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


for _ in range(5): candidates()
report("lxo_mrt_candidates, %d images x (%d draws of %d steps + the reference)" % (B, N, nsteps), [timed_launches(candidates) for _ in range(reps)],
       "us per call (%d calls back to back)" % launches)

# ---- 3. Engine.edit_distance against the host levenshtein
rng = np.random.default_rng(3)
pairs = 384
hyp = rng.integers(0, V - 3, size=(pairs, 100)).astype(np.int32)
refs = rng.integers(0, V - 3, size=(pairs, 100)).astype(np.int32)
hl, rll = rng.integers(90, 101, size=pairs).astype(np.int32), rng.integers(90, 101, size=pairs).astype(np.int32)


def timed_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


got = eng.edit_distance(hyp, refs, hl, rll)
want = [levenshtein(list(hyp[p, :hl[p]]), list(refs[p, :rll[p]])) for p in range(pairs)]
assert got.tolist() == want
alternate([("host levenshtein, %d pairs" % pairs, lambda: [levenshtein(list(hyp[p, :hl[p]]), list(refs[p, :rll[p]])) for p in range(pairs)]),
           ("Engine.edit_distance, %d pairs" % pairs, lambda: eng.edit_distance(hyp, refs, hl, rll))], timed_once, "ms per call (host arrays in and out)")
