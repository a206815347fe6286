"""What the weighted loss, label smoothing and the minimum-risk step cost, at the benchmark shape (B = 64, 128 x 512, V = 500, T = 101, bf16).

1. The loss launch (Engine.loss behind one forward: the memset, the CE kernel, the ordered reduction of its statistics) without weights --
   lxo_ce_loss_fwd_bwd, the yardstick --, with device row_weights (lxo_ce_loss_weighted), and with label_smoothing = 0.1 without weights and
   with the row_weights (lxo_ce_loss_smoothed), timed by device events over --launches back-to-back calls, in alternating rounds of one
   process; medians of --reps.
2. Engine.mrt_step (16 images x 4 candidates = the same 64 rows) and Engine.train_step(label_smoothing=0.1) against Engine.train_step on those
   rows, host clock around steps that end in the loss copy, the same way.
--soft K[,K...] (e.g. --soft 5,16) adds the soft-target arms: the loss launch with soft_weight = 0.5 and the k best tokens of a SECOND engine's
score_alternatives_dev as targets, with and without the row_weights, in the same alternating rounds as the label_smoothing arms (their baseline);
train_step(soft_targets=) and a whole distillation step (the teacher's forward and scoring + the student's step, what Img2SeqModel.distill_batch
runs with one teacher) beside train_step(label_smoothing=0.1); and the loss arms again at V = 1000 and V = 1025.  Without the flag: the lines above.
Prints one line per arm: median (min..max)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import pad_batch_formulas

V, B, G = 500, 64, 16
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
launches = int(sys.argv[sys.argv.index("--launches") + 1]) if "--launches" in sys.argv else 200
steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 5
soft_ks = [int(x) for x in sys.argv[sys.argv.index("--soft") + 1].split(",")] if "--soft" in sys.argv else []
imgs, forms = synthetic.make_set(B, 128, 512, V, 100, 101, seed=5)          # every formula 100 tokens: T = 101
img = pad_batch_images(imgs)
f, l = pad_batch_formulas(forms, V - 2, V - 1)
assert f.shape == (B, 101)
img_d, f_d, l_d = torch.from_numpy(img).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(l.astype(np.int32)).cuda()
n_tok = int(l.sum())
w_row = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 2.0, size=B).astype(np.float32)).cuda()


def report(name, v, unit, base=None):
    v = sorted(v)
    print("%s: %s median of %d %.2f (%.2f..%.2f)%s" % (name, unit, len(v), v[len(v) // 2], v[0], v[-1],
                                                        "" if base is None else ", ratio to the first arm %.4f" % (v[len(v) // 2] / base)))
    return v[len(v) // 2]


# ---- 1. the loss launch
eng = Engine(V, dtype="bf16", seed=0)
eng.forward(img_d, f_d)
arms = [("loss, no weights (lxo_ce_loss_fwd_bwd)", lambda: eng.loss(l_d, 1.0 / n_tok)),
        ("loss, row_weights (lxo_ce_loss_weighted)", lambda: eng.loss(l_d, 1.0 / n_tok, row_weights=w_row)),
        ("loss, label_smoothing 0.1 (lxo_ce_loss_smoothed)", lambda: eng.loss(l_d, 1.0 / n_tok, label_smoothing=0.1)),
        ("loss, label_smoothing 0.1 + row_weights (lxo_ce_loss_smoothed)", lambda: eng.loss(l_d, 1.0 / n_tok, row_weights=w_row, label_smoothing=0.1))]


def teacher_targets(teacher, k, im=None, fo=None, le=None):
    ids, logp = teacher.score_alternatives_dev(img_d if im is None else im, f_d if fo is None else fo, l_d if le is None else le, k)
    return ids, torch.exp(logp)


def soft_arms(e, targets, lens, ntok, wr):
    out = []
    for k, t in targets.items():
        out.append(("loss, soft_weight 0.5, k = %d (lxo_ce_loss_soft)" % k, lambda t=t: e.loss(lens, 1.0 / ntok, soft_targets=t, soft_weight=0.5)))
        out.append(("loss, soft_weight 0.5, k = %d + row_weights (lxo_ce_loss_soft)" % k,
                    lambda t=t: e.loss(lens, 1.0 / ntok, row_weights=wr, soft_targets=t, soft_weight=0.5)))
    return out


teach = Engine(V, dtype="bf16", seed=1) if soft_ks else None
soft_t = {k: teacher_targets(teach, k) for k in soft_ks}
arms += soft_arms(eng, soft_t, l_d, n_tok, w_row)


def timed_launches(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


for _, fn in arms:
    for _ in range(20): fn()
per = [[] for _ in arms]
for r in range(reps):
    for i in (range(len(arms)) if r % 2 == 0 else reversed(range(len(arms)))):
        per[i].append(timed_launches(arms[i][1]))
base = None
for (name, _), v in zip(arms, per):
    m = report(name, v, "us per call (%d calls back to back)" % launches, base)
    base = m if base is None else base

# ---- 2. mrt_step against train_step on the same 64 rows
gs = np.full(G, B // G)
cost = np.random.default_rng(2).uniform(0.0, 1.0, size=B).astype(np.float32)
e_ce, e_ls, e_mrt = Engine(V, dtype="bf16", seed=0), Engine(V, dtype="bf16", seed=0), Engine(V, dtype="bf16", seed=0)
img_rep = np.ascontiguousarray(img[np.repeat(np.arange(G), gs)])
arms = [("train_step, 64 rows", lambda: e_ce.train_step(img_rep, f, l, 1e-4)),
        ("train_step(label_smoothing=0.1), 64 rows", lambda: e_ls.train_step(img_rep, f, l, 1e-4, label_smoothing=0.1)),
        ("mrt_step, 16 images x 4 candidates", lambda: e_mrt.mrt_step(img[:G], f, l, gs, cost, 1e-4, 0.005))]
if soft_ks:
    k0 = soft_ks[0]
    e_sf, e_ds = Engine(V, dtype="bf16", seed=0), Engine(V, dtype="bf16", seed=0)
    rep_t = teacher_targets(teach, k0, img_rep, f, l)
    arms += [("train_step(soft_targets=, k = %d), 64 rows" % k0, lambda: e_sf.train_step(img_rep, f, l, 1e-4, soft_targets=rep_t, soft_weight=0.5)),
             ("distillation step, one teacher, k = %d (its forward and scoring + the student's step), 64 rows" % k0,
              lambda: e_ds.train_step(img_rep, f, l, 1e-4, soft_targets=teacher_targets(teach, k0, img_rep, f, l), soft_weight=0.5))]


def timed_steps(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


for _, fn in arms:
    for _ in range(3): fn()
per = [[] for _ in arms]
for r in range(reps):
    for i in (range(len(arms)) if r % 2 == 0 else reversed(range(len(arms)))):
        per[i].append(timed_steps(arms[i][1]))
base = None
for (name, _), v in zip(arms, per):
    m = report(name, v, "ms per step (host arrays in, loss out)", base)
    base = m if base is None else base
print("chains: train_step %s/%s, train_step(label_smoothing) %s/%s, mrt_step %s/%s" % (e_ce.chain_used, e_ce.chain_used_bwd, e_ls.chain_used,
                                                                                      e_ls.chain_used_bwd, e_mrt.chain_used, e_mrt.chain_used_bwd))

# ---- 3. the soft loss arms at the other two kernels: V = 1000 (the register row at KV = 16) and V = 1025 (the strided kernel)
for V3 in ((1000, 1025) if soft_ks else ()):
    imgs3, forms3 = synthetic.make_set(B, 128, 512, V3, 100, 101, seed=5)
    f3, l3 = pad_batch_formulas(forms3, V3 - 2, V3 - 1)
    i3, f3d, l3d = torch.from_numpy(pad_batch_images(imgs3)).cuda(), torch.from_numpy(f3).cuda(), torch.from_numpy(l3.astype(np.int32)).cuda()
    n3 = int(l3.sum())
    e3, t3 = Engine(V3, dtype="bf16", seed=0), Engine(V3, dtype="bf16", seed=1)
    tg3 = {k: teacher_targets(t3, k, i3, f3d, l3d) for k in soft_ks}
    e3.forward(i3, f3d)
    arms = [("V = %d: loss, label_smoothing 0.1 (lxo_ce_loss_smoothed)" % V3, lambda: e3.loss(l3d, 1.0 / n3, label_smoothing=0.1)),
            ("V = %d: loss, label_smoothing 0.1 + row_weights (lxo_ce_loss_smoothed)" % V3, lambda: e3.loss(l3d, 1.0 / n3, row_weights=w_row, label_smoothing=0.1))]
    arms += [("V = %d: %s" % (V3, n), fn) for n, fn in soft_arms(e3, tg3, l3d, n3, w_row)]
    for _, fn in arms:
        for _ in range(20): fn()
    per = [[] for _ in arms]
    for r in range(reps):
        for i in (range(len(arms)) if r % 2 == 0 else reversed(range(len(arms)))):
            per[i].append(timed_launches(arms[i][1]))
    base = None
    for (name, _), v in zip(arms, per):
        m = report(name, v, "us per call (%d calls back to back)" % launches, base)
        base = m if base is None else base
