"""Greedy / beam decode latency on synthetic 128x512 crops (random-init weights never emit END, so every run decodes
the full max_iter + 1 steps).  --scores: each decode once without and once with return_scores (token log-probs / hypothesis
scores), interleaved over --reps rounds, for the A/B of the scored calls.  --prefix N: the same A/B of the calls without a prefix and
with an N-token forced prefix on every row (prefix=, the decode still runs max_iter + 1 steps).  --ban N: the A/B of the calls without a
constraint and with N random tokens banned in every row (allowed= as [B, V]: a set per image).  --sample N: sampled decode with N draws per image
(Engine.sample_decode at temperature 1, then with top_k = 50 and top_p = 0.9) against beam N of the same tree, in alternating rounds; nothing else
runs then.  --grammar: greedy, beam 5 and sample 5 under a delimiter grammar (grammar=) against the same decode with a static set, both on the
launch-per-step kernels, in alternating rounds: the cost of the grammar kernel per step; nothing else runs then."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
V, B = 500, 64
imgs, _ = synthetic.make_set(B, 128, 512, V, 30, 101, seed=5)
img = torch.from_numpy(pad_batch_images(imgs)).cuda()
scores_ab = "--scores" in sys.argv
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
n_prefix = int(sys.argv[sys.argv.index("--prefix") + 1]) if "--prefix" in sys.argv else None
prefix = torch.randint(0, V - 1, (B, n_prefix or 1), generator=torch.Generator().manual_seed(3)).to(torch.int32) if n_prefix else None
n_ban = int(sys.argv[sys.argv.index("--ban") + 1]) if "--ban" in sys.argv else None
allowed = None
if n_ban:
    allowed = torch.ones(B, V, dtype=torch.bool)
    for b in range(B):
        allowed[b, torch.randperm(V - 1, generator=torch.Generator().manual_seed(7 + b))[:n_ban]] = False      # END (V - 1) stays allowed


def timed(fn, n=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): out = fn()
    torch.cuda.synchronize()
    out = out[0] if isinstance(out, tuple) else out
    return (time.perf_counter() - t0) / n, out.shape[1]


if "--sample" in sys.argv:
    n = int(sys.argv[sys.argv.index("--sample") + 1])
    eng = Engine(V, dtype="bf16", beam=n, max_steps=152)
    arms = [("beam %d" % n, lambda: eng.beam_decode(img, V - 1, n, max_iter=100)),
            ("sample %d" % n, lambda: eng.sample_decode(img, V - 1, n=n, seed=1, max_iter=100)),
            ("sample %d top_k 50 top_p 0.9" % n, lambda: eng.sample_decode(img, V - 1, n=n, top_k=50, top_p=0.9, seed=1, max_iter=100))]
    for _, fn in arms: fn()
    per = [[] for _ in arms]
    for r in range(reps):
        for i in (range(len(arms)) if r % 2 == 0 else reversed(range(len(arms)))):
            dt, steps = timed(arms[i][1])
            per[i].append(dt * 1e6 / steps)
    for (name, _), v in zip(arms, per):
        v = sorted(v)
        print("%s: %d steps, us per step median of %d %.2f (%.2f..%.2f), ratio to beam %.4f" % (name, steps, reps, v[reps // 2], v[0], v[-1], v[reps // 2] / sorted(per[0])[reps // 2]))
    sys.exit(0)

if "--grammar" in sys.argv:
    # the cost of the grammar kernel: greedy, beam 5 and sample 5 under a delimiter grammar against the same decode with a static set (every token
    # allowed, one row per image), both on the launch-per-step path (step_kernels forced: a grammar call never takes the persistent chain)
    import numpy as np
    from latex_ocr_amd.grammar import Grammar
    cls = np.zeros(V, np.int8)
    for q in range(1, 6):                                   # five kinds, four openers and four closers each
        cls[40 * q:40 * q + 4], cls[40 * q + 4:40 * q + 8] = q, -q
    gram = Grammar(cls, max_depth=32, budget=True, id_end=V - 1)
    every = torch.ones(B, V, dtype=torch.bool)
    for kind, n in (("greedy", 1), ("beam", 5), ("sample", 5)):
        eng = Engine(V, dtype="bf16", beam=n, max_steps=152)
        eng.step_kernels = 2
        call = {"greedy": lambda **kw: eng.greedy_decode(img, V - 1, max_iter=100, **kw),
                "beam": lambda **kw: eng.beam_decode(img, V - 1, n, max_iter=100, **kw),
                "sample": lambda **kw: eng.sample_decode(img, V - 1, n=n, seed=1, max_iter=100, **kw)}[kind]
        arms = [("static set", lambda: call(allowed=every)), ("grammar", lambda: call(allowed=every, grammar=gram))]
        for _, fn in arms: fn()
        per, steps = [[], []], [0, 0]
        for r in range(reps):
            for i in ((0, 1) if r % 2 == 0 else (1, 0)):
                dt, steps[i] = timed(arms[i][1])
                per[i].append(dt * 1e6 / steps[i])
        a, b = sorted(per[0]), sorted(per[1])
        print("%s %d: us per step (median of %d, min..max)  static set %.2f (%.2f..%.2f, %d steps)  grammar %.2f (%.2f..%.2f, %d steps)  difference %.2f us  ratio %.4f"
              % (kind, n, reps, a[reps // 2], a[0], a[-1], steps[0], b[reps // 2], b[0], b[-1], steps[1], b[reps // 2] - a[reps // 2], b[reps // 2] / a[reps // 2]))
    sys.exit(0)

for beam in (1, 5):
    eng = Engine(V, dtype="bf16", beam=beam, max_steps=152)
    if beam == 1:
        arms = {False: lambda: eng.greedy_decode(img, V - 1, max_iter=100), True: lambda: eng.greedy_decode(img, V - 1, max_iter=100, return_scores=True)}
    else:
        arms = {False: lambda: eng.beam_decode(img, V - 1, beam, max_iter=100), True: lambda: eng.beam_decode(img, V - 1, beam, max_iter=100, return_scores=True)}
    if n_prefix is not None:
        arms = {False: arms[False], True: (lambda: eng.greedy_decode(img, V - 1, max_iter=100, prefix=prefix)) if beam == 1 else
                (lambda: eng.beam_decode(img, V - 1, beam, max_iter=100, prefix=prefix))}
    if n_ban is not None:
        arms = {False: arms[False], True: (lambda: eng.greedy_decode(img, V - 1, max_iter=100, allowed=allowed)) if beam == 1 else
                (lambda: eng.beam_decode(img, V - 1, beam, max_iter=100, allowed=allowed))}
    if not scores_ab and n_prefix is None and n_ban is None:
        arms[False]()
        dt, steps = timed(arms[False])
        print("beam %d: %d steps, %.1f ms per batch of %d (%.1f us per step, %.0f img/s)" % (beam, steps, dt * 1e3, B, dt * 1e6 / steps, B / dt))
        continue
    arms[False](); arms[True]()
    per = {False: [], True: []}
    for r in range(reps):
        for sc in ((False, True) if r % 2 == 0 else (True, False)):
            dt, steps = timed(arms[sc])
            per[sc].append(dt * 1e6 / steps)
    a, b = sorted(per[False]), sorted(per[True])
    print("beam %d: us per step (median of %d, min..max)  %s %.2f (%.2f..%.2f)  %s %.2f (%.2f..%.2f)  ratio %.4f"
          % (beam, reps, "no constraint" if n_ban else "no prefix" if n_prefix else "ids only", a[reps // 2], a[0], a[-1],
             ("%d banned" % n_ban) if n_ban else ("prefix %d" % n_prefix) if n_prefix else "with scores", b[reps // 2], b[0], b[-1],
             b[reps // 2] / a[reps // 2]))
