"""Shared by tests/test_attention_locate_sim.py (hipsim) and tests/test_gpu_attention_locate.py (MI355X): the float64 restatement of
lxo_attention_locate's definition (include/lxo.h), the case matrix, the runner with guard words and the checkers.

WHAT IS HELD EXACTLY AND WHAT WITHIN A BOUND.  u = 2^-24 is the unit round-off of f32.  A sum of n non-negative f32 terms, added in any order,
errs by at most (n - 1) u times the sum to first order (each of the n - 1 additions rounds a partial sum that is at most the total).  A cumulative
marginal covers at most R cells, so TOL = R u S bounds the error of every f32 cumulative sum of a map, whatever the kernel's order.
  - DYADIC maps (cells integer multiples of 2^-12, total at most 2: every partial sum needs at most 13 bits) are summed exactly by f32 in any order:
    peak, box and stats[0] must EQUAL the reference.  is_dyadic() decides the class; no dyadic map is exempt from anything.
  - On every other map peak is still exact (a comparison of the f32 cells).  A box edge must be VALID under the float64 cumulative within TOL:
    C(x0) > tail - TOL and (x0 == 0 or C(x0 - 1) <= tail + TOL); C(x1) >= hi - TOL and (x1 == 0 or C(x1 - 1) < hi + TOL); and it must EQUAL the
    reference's edge wherever the reference's own margin -- the distance of the two cumulative values that decide the edge from the threshold --
    exceeds TOL.  (An edge at the last line is decided by the line before it alone: the last cumulative value is S by definition.)
  - stats against float64, with g = (R + 16) u (the sum's bound plus the handful of roundings around it):
      S: g S.   cx: g max(Wp - 1, 1), cy likewise (a ratio of two non-negative sums, scaled by the largest coordinate).
      sx, compared as variances v: the kernel's centroid is off by d <= e = 2 u Wp and each x - cx rounds by as much; about the true centroid the
        first moment vanishes, so d enters as d^2 only, and the per-term error of (x - cx) as 2 e E|x - cx| <= 2 e sqrt(v):
        |sx'^2 - v| <= 2 g v + 2 e sqrt(v) + e^2.   sy likewise with Hp.
      entropy H: q = a / S carries a relative error th <= (R + 2) u (S's, and the two roundings of a * (1 / S)), which moves -q ln q by at most
        th (-q ln q + q), summed th (H + 1); the device logf is within 2 ulp = 4 u of ln, 4 u H in all; the sum of the non-negative terms R u H:
        |H' - H| <= (2 R + 16) u (H + 1).
      inside (for the box the kernel returned): two non-negative sums, (2 R + 4) u.   peak_share: (R + 4) u times itself.
    The largest deviations met are kept in SEEN, as fractions of their bounds, for the record (profiles/attention_locate.txt).
  - coverage equals the ascending-t np.float32 sum bit for bit."""
import ctypes
import functools
import math

import numpy as np

from edit_distance_ref import Host

U = 2.0 ** -24
GUARD = 16
NS = 8                                                              # LXO_LOCATE_STATS
LIMIT = 9728                                                        # LXO_LOCATE_MAX_CELLS
MASSES = (1.0, 0.9, 0.5, 2.0 ** -20)
SHAPES = ((1, 1), (1, 7), (7, 1), (3, 5), (2, 65), (65, 2), (14, 62), (98, 98))
KINDS = ("one hot", "two peaks", "uniform", "dyadic", "zero", "nan", "softmax", "softmax flat")
CASE_NAMES = ["%dx%d %s" % (h, w, lay) for h, w in SHAPES for lay in ("TBR", "BTR")]
SEEN = {}


def is_dyadic(a32):
    a = a32.astype(np.float64)
    return bool(np.isfinite(a).all() and (a >= 0).all() and (a * 4096 == np.floor(a * 4096)).all() and a.sum() <= 2.0)


class MapRef(object):
    """one map in float64: the exactly rounded cumulative marginals (math.fsum of every prefix: monotone, and the last one is S), peak, moments"""

    def __init__(self, a32, Hp, Wp):
        self.a32, self.Hp, self.Wp = a32, Hp, Wp
        a = a32.astype(np.float64).reshape(Hp, Wp)
        self.a = a
        self.has = bool(np.isfinite(a).all() and math.fsum(a.ravel()) > 0)
        if not self.has:
            return
        self.S = math.fsum(a.ravel())
        self.dyadic = is_dyadic(a32)
        self.Cx = np.array([math.fsum(a[:, :x + 1].ravel()) for x in range(Wp)])
        self.Cy = np.array([math.fsum(a[:y + 1].ravel()) for y in range(Hp)])
        assert self.Cx[-1] == self.S == self.Cy[-1]
        self.peak = int(np.argmax(a32))                            # the first of equal maxima
        p = a / self.S
        xs, ys = np.arange(Wp, dtype=np.float64), np.arange(Hp, dtype=np.float64)
        self.cx, self.cy = float((p.sum(0) * xs).sum()), float((p.sum(1) * ys).sum())
        self.vx, self.vy = float((p.sum(0) * (xs - self.cx) ** 2).sum()), float((p.sum(1) * (ys - self.cy) ** 2).sum())
        nz = p[p > 0]
        self.H = float(-(nz * np.log(nz)).sum())
        self.peak_share = float(a.ravel()[self.peak] / self.S)

    def thresholds(self, mass):
        m = float(np.float32(mass))                                # the argument is a C float
        tail = (0.5 * (1.0 - m)) * self.S
        return tail, self.S - tail

    def edges(self, C, mass):
        """-> (e0, e1, margin of e0, margin of e1)"""
        tail, hi = self.thresholds(mass)
        e0, e1 = int(np.argmax(C > tail)), int(np.argmax(C >= hi))
        assert C[e0] > tail and C[e1] >= hi and e0 <= e1
        m0 = min(C[e0] - tail, tail - C[e0 - 1] if e0 else np.inf)
        m1 = min(C[e1] - hi if e1 < len(C) - 1 else np.inf, hi - C[e1 - 1] if e1 else np.inf)
        return e0, e1, m0, m1

    def box(self, mass):
        x0, x1, _, _ = self.edges(self.Cx, mass)
        y0, y1, _, _ = self.edges(self.Cy, mass)
        return [x0, y0, x1, y1]

    def inside(self, b):
        return float(self.a[b[1]:b[3] + 1, b[0]:b[2] + 1].sum() / self.S)


def _softmax(rng, R, scale):
    z = rng.standard_normal(R) * scale
    e = np.exp(z - z.max())
    return (e / e.sum()).astype(np.float32)


def _map(kind, rng, R):
    a = np.zeros(R, np.float32)
    if kind == "one hot":
        a[rng.integers(R)] = 1.0
    elif kind == "two peaks":                                       # equal maxima: the lower index is the peak; (one cell when there is only one)
        a[rng.choice(R, size=min(2, R), replace=False)] = 0.5
    elif kind == "uniform":                                         # dyadic while R <= 4096
        a[:] = 2.0 ** -math.ceil(math.log2(R)) if R > 1 else 1.0
    elif kind == "dyadic":                                          # 4096 units of 2^-12 thrown at random cells, many left empty when R is large
        a[:] = np.bincount(rng.integers(R, size=4096), minlength=R) * 2.0 ** -12
    elif kind == "nan":
        a = _softmax(rng, R, 1.0)
        a[rng.integers(R)] = np.nan
    elif kind == "softmax":
        a = _softmax(rng, R, 3.0)
    elif kind == "softmax flat":
        a = _softmax(rng, R, 0.5)
    else:
        assert kind == "zero"
    return a


@functools.lru_cache(maxsize=None)
def named(name):
    """-> the case: maps f32 [alpha_rows][steps][R], the buffer in its layout, len / src (or None), and a MapRef (or None) per position"""
    k = CASE_NAMES.index(name)
    (Hp, Wp), layout = SHAPES[k // 2], ("TBR", "BTR")[k % 2]
    R, steps, rows = Hp * Wp, len(KINDS), 3
    rng = np.random.default_rng(100 + k)
    alpha_rows = rows if layout == "TBR" else rows + 1
    maps = np.stack([np.stack([_map(kind, rng, R) for kind in KINDS]) for _ in range(alpha_rows)])
    if layout == "TBR":                                             # [steps][rows][Rp], the padding behind a map's R cells all NaN: it is never read
        Rp = R + 3
        buf = np.full((steps, alpha_rows, Rp), np.nan, np.float32)
        buf[:, :, :R] = maps.transpose(1, 0, 2)
        strides, ln, src = (alpha_rows * Rp, Rp), None, None
    else:                                                           # [rows][steps][R]; a length of 0, a full row, a cut one; src: a permutation per step, a -1, a row too far
        buf = maps.copy()
        strides = (R, steps * R)
        ln = np.array([steps, 0, steps - 2], np.int32)
        src = np.stack([rng.permutation(alpha_rows)[:rows] for _ in range(steps)]).astype(np.int32)
        src[1, 0], src[2, 2], src[3, 0] = -1, alpha_rows, 1 << 30
    refs = [[None] * steps for _ in range(rows)]
    cache = {}
    for i in range(rows):
        for t in range(steps):
            r = i if src is None else int(src[t, i])
            if (ln is None or t < ln[i]) and 0 <= r < alpha_rows:
                if (r, t) not in cache:
                    cache[r, t] = MapRef(maps[r, t], Hp, Wp)
                refs[i][t] = cache[r, t] if cache[r, t].has else None
    c = dict(name=name, Hp=Hp, Wp=Wp, R=R, rows=rows, steps=steps, alpha_rows=alpha_rows, maps=maps, buf=buf, strides=strides, len=ln, src=src, refs=refs)
    some = [m for row in refs for m in row if m is not None]
    assert any(m.dyadic for m in some) and (R == 1 or any(not m.dyadic for m in some))
    for (r, t), m in cache.items():                                 # the kinds built to be dyadic are
        if KINDS[t] in ("one hot", "two peaks", "dyadic") or (KINDS[t] == "uniform" and R <= 4096):
            assert m.has and m.dyadic, (name, KINDS[t])
    return c


def decided_share():
    """the share of the non-dyadic maps' edges, over the whole matrix, that the reference decides by more than TOL: the seeds are held to 0.95"""
    n = ok = 0
    for name in CASE_NAMES:
        c = named(name)
        tol = c["R"] * U
        for m in {id(m): m for row in c["refs"] for m in row if m is not None and not m.dyadic}.values():
            for mass in MASSES:
                for C in (m.Cx, m.Cy):
                    _, _, m0, m1 = m.edges(C, mass)
                    n += 2
                    ok += int(m0 > tol * m.S) + int(m1 > tol * m.S)
    return ok / n


def coverage_ref(c):
    """ascending t, one np.float32 accumulator per cell"""
    cov = np.zeros((c["rows"], c["R"]), np.float32)
    for i in range(c["rows"]):
        for t in range(c["steps"]):
            if c["refs"][i][t] is not None:
                cov[i] = cov[i] + c["refs"][i][t].a32
    assert cov.dtype == np.float32
    return cov


def _guarded(dev, shape, dtype):
    size = int(np.prod(shape))
    return dev.up(np.full(size + 2 * GUARD, -7, dtype)), size


def run_locate(lib, c, mass, dev=Host, want=("peak", "box", "stats", "coverage"), cov_ld=None, **over):
    """One lxo_attention_locate call on case c -> (rc, dict of the outputs asked for), every output between guard words that are checked.
    over: arguments replaced for the refusal tests (alpha=None, Hp=, ...)."""
    rows, steps, R = over.get("rows", c["rows"]), over.get("steps", c["steps"]), c["R"]
    cov_ld = R if cov_ld is None else cov_ld
    shapes = {"peak": ((c["rows"], c["steps"]), np.int32), "box": ((c["rows"], c["steps"], 4), np.int32), "stats": ((c["rows"], c["steps"], NS), np.float32),
              "coverage": ((c["rows"], max(cov_ld, R)), np.float32)}
    keep = [dev.up(c["buf"]), dev.up(c["len"]), dev.up(c["src"])]
    bufs = {k: _guarded(dev, *shapes[k]) for k in shapes if k in want}
    arg = lambda k: dev.ptr(bufs[k][0][GUARD:GUARD + bufs[k][1]]) if k in bufs else dev.ptr(None)
    a = dict(alpha=dev.ptr(keep[0]), ss=c["strides"][0], rs=c["strides"][1], alpha_rows=c["alpha_rows"], Hp=c["Hp"], Wp=c["Wp"], rows=rows, steps=steps,
             len=dev.ptr(keep[1]), src=dev.ptr(keep[2]), mass=mass, cov_ld=cov_ld)
    a.update({k: (dev.ptr(None) if v is None else v) for k, v in over.items()})
    rc = lib.lxo_attention_locate(a["alpha"], a["ss"], a["rs"], a["alpha_rows"], a["Hp"], a["Wp"], a["rows"], a["steps"], a["len"], a["src"], a["mass"],
                                  arg("peak"), arg("box"), arg("stats"), arg("coverage"), a["cov_ld"], dev.stream)
    got = {}
    for k, (buf, size) in bufs.items():
        h = dev.down(buf)
        assert (h[:GUARD] == -7).all() and (h[GUARD + size:] == -7).all(), (c["name"], k, "guard words")
        got[k] = h[GUARD:GUARD + size].reshape(shapes[k][0])
    return rc, got


def _seen(key, dev, bound):
    if bound > 0:
        SEEN[key] = max(SEEN.get(key, 0.0), dev / bound)


def check_position(c, m, mass, peak, box, st, where):
    """one position with a map against its MapRef"""
    R, Hp, Wp = c["R"], c["Hp"], c["Wp"]
    assert peak == m.peak, (where, "peak", peak, m.peak)
    ref_box = m.box(mass)
    x0, y0, x1, y1 = box
    assert 0 <= x0 <= x1 < Wp and 0 <= y0 <= y1 < Hp, (where, box)
    if m.dyadic:
        assert box == ref_box, (where, "box of a dyadic map", box, ref_box)
        assert st[0] == np.float32(m.S) and float(np.float32(m.S)) == m.S, (where, "S of a dyadic map", st[0], m.S)
    else:
        tol = R * U * m.S
        tail, hi = m.thresholds(mass)
        for C, e0, e1, axis in ((m.Cx, x0, x1, "x"), (m.Cy, y0, y1, "y")):
            assert C[e0] > tail - tol and (e0 == 0 or C[e0 - 1] <= tail + tol), (where, axis + "0 is not valid", e0)
            assert C[e1] >= hi - tol and (e1 == 0 or C[e1 - 1] < hi + tol), (where, axis + "1 is not valid", e1)
            r0, r1, m0, m1 = m.edges(C, mass)
            assert m0 <= tol or e0 == r0, (where, axis + "0", e0, r0, m0, tol)
            assert m1 <= tol or e1 == r1, (where, axis + "1", e1, r1, m1, tol)
    g, st = (R + 16) * U, [float(v) for v in st]
    checks = [("S", abs(st[0] - m.S), g * m.S), ("cx", abs(st[1] - m.cx), g * max(Wp - 1, 1)), ("cy", abs(st[2] - m.cy), g * max(Hp - 1, 1))]
    for key, got, v, n in (("sx", st[3], m.vx, Wp), ("sy", st[4], m.vy, Hp)):
        e = 2 * U * n
        checks.append((key, abs(got * got - v), 2 * g * v + 2 * e * math.sqrt(v) + e * e))
    ins = m.inside(box)
    checks += [("entropy", abs(st[5] - m.H), (2 * R + 16) * U * (m.H + 1)), ("inside", abs(st[6] - ins), (2 * R + 4) * U * ins),
               ("peak_share", abs(st[7] - m.peak_share), (R + 4) * U * m.peak_share)]
    for key, dev, bound in checks:
        print("%s %s: off by %.3e, bound %.3e" % (where, key, dev, bound))
        assert dev <= bound, (where, key, dev, bound)
        _seen(key, dev, bound)
    assert ins >= 2 * float(np.float32(mass)) - 1 - 4 * U, (where, "the box holds less than 2 mass - 1", ins)


def check_outputs(c, mass, got):
    for i in range(c["rows"]):
        for t in range(c["steps"]):
            m, where = c["refs"][i][t], "%s mass %g (%d, %d) %s" % (c["name"], mass, i, t, KINDS[t])
            if m is None:
                assert got["peak"][i, t] == -1 and (got["box"][i, t] == -1).all() and got["stats"][i, t].tobytes() == bytes(4 * NS), (where, "none")
            else:
                check_position(c, m, mass, int(got["peak"][i, t]), [int(v) for v in got["box"][i, t]], got["stats"][i, t], where)
    assert got["coverage"].tobytes() == coverage_ref(c).tobytes(), (c["name"], "coverage")


def check_locate_case(lib, c, dev=Host):
    """the whole case at every mass"""
    out = {}
    for mass in MASSES:
        rc, got = run_locate(lib, c, mass, dev)
        assert rc == 0, (c["name"], lib.lxo_last_error())
        check_outputs(c, mass, got)
        out[mass] = got
    return out
