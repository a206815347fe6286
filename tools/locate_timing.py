"""What locating every token costs (bf16, V = 500, B = 64, 128 x 512, T = 101: 6464 maps of 14 x 62 cells in workspace region `alpha`).

Alternating rounds of one process, medians of --reps with ranges, the shapes warmed up.
 1. The lxo_attention_locate launch on region `alpha` of a real scoring pass, --calls calls back to back that end in a device synchronise: peak + box +
    stats; with the coverage as well; and the same outputs composed from torch operations on the device (marginals, cumsum, searchsorted, moments).
    The bytes of the one read of the maps over the time, as a fraction of the 8 TB/s peak.
 2. Engine.score against Engine.score(locate=True, coverage=True) and against the host route: score(return_attention=True) and the definition in
    numpy float64 on the copied maps.
 3. greedy_decode(return_attention=True) against greedy_decode(return_boxes=True, coverage=True).
The kernel's peak and box are compared with the torch composition's first.  Prints one line per arm: median (min..max)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import encoder_out_hw, pad_batch_images
from latex_ocr_amd.model.utils.text import pad_batch_formulas

V, B, H, W, MAX_ITER, MASS = 500, 64, 128, 512, 151, 0.9
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
    base, med = None, []
    for (name, _), v in zip(arms, per):
        m = report(name, v, unit, base)
        base = m if base is None else base
        med.append(m)
    return med


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
imgs, forms = synthetic.make_set(B, H, W, V, 95, 100, seed=5)
img = pad_batch_images(imgs)
f, ln = pad_batch_formulas(forms, PAD, END)
T = int(f.shape[1])
Hp, Wp = encoder_out_hw(H, W)
R, Rp = Hp * Wp, (Hp * Wp + 7) // 8 * 8
print("B %d, T %d, maps %d x %d (R %d, pitch %d), lengths %d..%d" % (B, T, Hp, Wp, R, Rp, ln.min(), ln.max()))
eng.score(img, f, ln)                                               # leaves region `alpha` [T][B][Rp] of the scoring pass in the workspace
alpha = eng.region("alpha", "f32", (T, B, Rp))
ln_d = torch.from_numpy(ln.astype(np.int32)).cuda()
read_bytes = int((np.arange(T)[None, :] < ln[:, None]).sum()) * R * 4


def k_locate(cov):
    return eng._locate(alpha, B * Rp, Rp, B, Hp, Wp, B, T, ln_d, None, MASS, cov)


def edges(C, lo, hi):
    return torch.searchsorted(C, lo, right=True), torch.searchsorted(C, hi, right=False)


def torch_locate():
    a = alpha[:, :, :R].permute(1, 0, 2).reshape(B, T, Hp, Wp)
    live = (torch.arange(T, device="cuda")[None, :] < ln_d[:, None])
    a = a * live[:, :, None, None]
    S = a.sum((2, 3))
    peak = a.reshape(B, T, R).argmax(2)
    px, py = a.sum(2), a.sum(3)
    tail = (0.5 * (1.0 - MASS)) * S
    x0, x1 = edges(px.cumsum(2), tail[..., None], (S - tail)[..., None])
    y0, y1 = edges(py.cumsum(2), tail[..., None], (S - tail)[..., None])
    xs, ys = torch.arange(Wp, device="cuda", dtype=torch.float32), torch.arange(Hp, device="cuda", dtype=torch.float32)
    inv = 1.0 / S.clamp_min(1e-30)
    cx, cy = (px * xs).sum(2) * inv, (py * ys).sum(2) * inv
    sx = ((px * (xs - cx[..., None]) ** 2).sum(2) * inv).sqrt()
    sy = ((py * (ys - cy[..., None]) ** 2).sum(2) * inv).sqrt()
    q = a * inv[..., None, None]
    ent = -(torch.xlogy(q, q)).sum((2, 3))
    inx = (xs >= x0) & (xs <= x1)
    iny = (ys >= y0) & (ys <= y1)
    inside = (a * inx[:, :, None, :] * iny[:, :, :, None]).sum((2, 3)) * inv
    share = a.reshape(B, T, R).gather(2, peak[..., None])[..., 0] * inv
    cov = a.sum(1)
    return peak, torch.cat([x0, y0, x1, y1], 2), torch.stack([S, cx, cy, sx, sy, ent, inside, share], 2), cov, live


def host_route():
    maps = eng.score(img, f, ln, return_attention=True)[-1].astype(np.float64)          # [B, T, Hp, Wp] on the host
    live = np.arange(T)[None, :] < ln[:, None]
    a = maps * live[:, :, None, None]
    S = a.sum((2, 3))
    peak = a.reshape(B, T, R).argmax(2)
    px, py = a.sum(2), a.sum(3)
    tail = (0.5 * (1.0 - MASS)) * S
    Cx, Cy = px.cumsum(2), py.cumsum(2)
    box = [(Cx > tail[..., None]).argmax(2), (Cy > tail[..., None]).argmax(2), (Cx >= (S - tail)[..., None]).argmax(2), (Cy >= (S - tail)[..., None]).argmax(2)]
    inv = 1.0 / np.maximum(S, 1e-300)
    xs, ys = np.arange(Wp), np.arange(Hp)
    cx, cy = (px * xs).sum(2) * inv, (py * ys).sum(2) * inv
    sx, sy = np.sqrt((px * (xs - cx[..., None]) ** 2).sum(2) * inv), np.sqrt((py * (ys - cy[..., None]) ** 2).sum(2) * inv)
    q = a * inv[..., None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(q > 0, q * np.log(q), 0.0).sum((2, 3))
    inx = (xs >= box[0][..., None]) & (xs <= box[2][..., None])
    iny = (ys >= box[1][..., None]) & (ys <= box[3][..., None])
    inside = (a * inx[:, :, None, :] * iny[:, :, :, None]).sum((2, 3)) * inv
    return peak, box, (S, cx, cy, sx, sy, ent, inside), a.sum(1)


for _ in range(3):
    loc = k_locate(True)
    ref = torch_locate()
torch.cuda.synchronize()
live = ref[4].cpu().numpy()
pk, bx = loc.peak.cpu().numpy(), loc.box.cpu().numpy()
assert (pk[live] == ref[0].cpu().numpy()[live]).all() and (pk[~live] == -1).all(), "the kernel's peaks differ from torch's arg-max"
same = (bx[live] == ref[1].cpu().numpy()[live]).all(1).mean()
print("boxes equal to the torch composition's (f32 cumsum, near-ties may differ): %.4f of %d; stats max |diff| %.2e; coverage max |diff| %.2e" % (
    same, live.sum(), float((loc.stats - ref[2])[torch.from_numpy(live).cuda()].abs().max()), float((loc.coverage.reshape(B, R) - ref[3].reshape(B, R)).abs().max())))
assert same > 0.99

med = alternate([("1a lxo_attention_locate: peak + box + stats", lambda: k_locate(False)), ("1b with the coverage", lambda: k_locate(True)),
                 ("1c the same outputs from torch operations", torch_locate)], timed_calls, "us per call (%d calls back to back)" % calls)
for name, m in zip(("1a", "1b"), med):
    print("%s: %.1f MB of maps read once in %.1f us = %.2f TB/s, %.1f %% of the 8 TB/s peak" % (name, read_bytes / 1e6, m, read_bytes / m / 1e6, read_bytes / m / 1e6 / 8 * 100))
if "--kernels-only" in sys.argv:
    sys.exit(0)
alternate([("2a Engine.score", lambda: eng.score(img, f, ln)), ("2b Engine.score(locate=True, coverage=True)", lambda: eng.score(img, f, ln, locate=True, coverage=True)),
           ("2c the host route: score(return_attention=True) + the definition in numpy float64", host_route)], timed_once, "ms per call")
alternate([("3a greedy_decode(return_attention=True)", lambda: eng.greedy_decode(img, END, max_iter=MAX_ITER, return_attention=True)),
           ("3b greedy_decode(return_boxes=True, coverage=True)", lambda: eng.greedy_decode(img, END, max_iter=MAX_ITER, return_boxes=True, coverage=True))],
          timed_once, "ms per call")
