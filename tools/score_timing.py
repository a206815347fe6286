"""Teacher-forced scoring (Engine.score: encoder + teacher-forced decoder + lxo_score_tokens) against Engine.evaluate_batch (the same forward
+ the CE kernel, which also writes d(logits)) on one batch: B = 64, 128 x 512 crops, V = 500, T = 101, bf16.  The two calls alternate over
--reps rounds (the order flips every round); each round times --n calls of each, host included (both end in a device-to-host copy).
--alternatives K adds a third arm to the same rounds, Engine.score(alternatives=K) (+ lxo_score_alternatives and its larger copy), and a
second output line that compares it with the score arm; without the flag the arms, their order and the output are unchanged."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import pad_batch_formulas
V, B = 500, 64
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
n = int(sys.argv[sys.argv.index("--n") + 1]) if "--n" in sys.argv else 10
imgs, forms = synthetic.make_set(B, 128, 512, V, 100, 101, seed=5)
img = pad_batch_images(imgs)
f, l = pad_batch_formulas(forms, V - 2, V - 1)
assert f.shape == (B, 101), f.shape
eng = Engine(V, dtype="bf16")
K = int(sys.argv[sys.argv.index("--alternatives") + 1]) if "--alternatives" in sys.argv else 0
arms = {"score": lambda: eng.score(img, f, l), "evaluate_batch": lambda: eng.evaluate_batch(img, f, l)}
order = ("score", "evaluate_batch")
if K:
    arms["alternatives"] = lambda: eng.score(img, f, l, alternatives=K)
    order += ("alternatives",)
for fn in arms.values():
    fn()
torch.cuda.synchronize()
per = {k: [] for k in arms}
for r in range(reps):
    for k in (order if r % 2 == 0 else order[::-1]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            arms[k]()
        torch.cuda.synchronize()
        per[k].append((time.perf_counter() - t0) / n * 1e3)
a, b = sorted(per["score"]), sorted(per["evaluate_batch"])
print("B=%d 128x512 V=%d T=%d bf16, chain used %s: ms per batch (median of %d rounds x %d calls, min..max)  score %.3f (%.3f..%.3f)  "
      "evaluate_batch %.3f (%.3f..%.3f)  ratio %.4f" % (B, V, f.shape[1], eng.chain_used, reps, n, a[reps // 2], a[0], a[-1],
                                                         b[reps // 2], b[0], b[-1], a[reps // 2] / b[reps // 2]))
if K:
    c = sorted(per["alternatives"])
    print("score(alternatives=%d) %.3f (%.3f..%.3f)  over score: %+.3f ms, ratio %.4f" % (K, c[reps // 2], c[0], c[-1], c[reps // 2] - a[reps // 2],
                                                                                        c[reps // 2] / a[reps // 2]))
