"""CPU: the net of tests/test_gpu_gemm_paths.py without a GPU.  (1) tests/gemm_ref.py's runner on the hipsim interpreter, over the small cases
of every table; (2) the case tables against the dispatch mirror expected_kernel: every kernel instantiation the dense launchers can start
is named, every family has its tails, single-element extents, padded pitches and one-step / many-step reductions; (3) the checker itself:
a fake kernel that is the float64 reference with one defect at a time must fail, the undamaged one must pass; (4) a condition on the data:
every live element of every case has a finite reference and a bound above 0."""
import numpy as np
import pytest
import torch

import gemm_ref as G
from simlib import f32_to_bf16

# every instantiation lxo_launch_gemm_nt / _tn / _slab (csrc/gemm.hip) can start for dense operands, by family
FAMILY_KERNELS = {
    "nt": ["nt<f32,128x128>",
           "nt<bf16,A=bf16,C=bf16,BK=32>", "nt<bf16,A=bf16,C=f32,BK=32>", "nt<bf16,A=f32,C=f32,BK=32>",
           "nt<bf16,A=bf16,C=bf16,BK=64>", "nt<bf16,A=bf16,C=f32,BK=64>", "nt<bf16,A=f32,C=f32,BK=64>"],
    "nt64": ["nt<f32,64x64>", "nt<bf16,A=f32,C=f32,64x64>"],
    "skinny": ["skinny<f32>", "skinny<bf16>"],
    "nt_dma": ["nt_dma<f32 out>", "nt_dma<bf16 out>"],
    "slab": ["slab<f32>", "slab<bf16>"],
    "tn": ["tn<f32>", "tn<bf16,A=bf16,B=bf16>", "tn<bf16,A=f32,B=bf16>", "tn<bf16,A=bf16,B=f32>", "tn<bf16,A=f32,B=f32>"],
    "tn_tr": ["tn_tr"],
}
# where the switched tables go with LXO_GEMM_NT_DMA=0 LXO_GEMM_TN_TR=0
FALLBACK = {"nt_dma": ["nt<bf16,A=bf16,C=f32,BK=64>", "nt<bf16,A=bf16,C=bf16,BK=64>"], "tn_tr": ["tn<bf16,A=bf16,B=bf16>"]}
TILE = {"nt": (128, 128), "nt64": (64, 64), "skinny": (64, 32), "nt_dma": (128, 128), "slab": (64, 64), "tn": (128, 128), "tn_tr": (128, 128)}


# ------------------------------------------------------------------------------------------------------------------- interpreter --
class SimAdapter(object):
    """the library's HIP sources on the hipsim interpreter, on the NumPy buffers themselves"""

    def __init__(self):
        from simharness import lib
        self.L = lib()

    def run(self, c, bufs):
        def p(a):
            return 0 if a is None else a.ctypes.data
        rc = G.invoke(self.L, c, p(bufs["A"]), p(bufs["B"]), p(bufs["C"]), p(bufs["bias"]), None)
        return rc, bufs["C"]


@pytest.mark.parametrize("fam", G.FAMILIES)
def test_tables_on_the_interpreter(fam):
    cases = G.sim_subset(fam)
    assert cases
    if fam in G.KERNEL_FAMILIES:
        assert {G.expected_kernel(c) for c in cases} == set(FAMILY_KERNELS[fam]), "a kernel of the family has no case the interpreter runs"
    fails, worst, _ = G.run_table(SimAdapter(), fam, cases)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------- coverage --
def test_tables_name_every_kernel_under_both_switch_settings():
    every = {k for ks in FAMILY_KERNELS.values() for k in ks}
    assert len(every) == 21
    for fam in G.KERNEL_FAMILIES:
        names = {G.expected_kernel(c) for c in G.TABLES[fam]}
        assert names == set(FAMILY_KERNELS[fam]), (fam, sorted(names ^ set(FAMILY_KERNELS[fam])))
        off = {G.expected_kernel(c, G.ARMS_OFF) for c in G.TABLES[fam]}
        assert off == set(FALLBACK.get(fam, FAMILY_KERNELS[fam])), (fam, sorted(off))
        assert all(c["expect"] == "ok" for c in G.TABLES[fam])
    for sw in (G.DEFAULT_SWITCHES, G.ARMS_OFF):
        assert {G.expected_kernel(c, sw) for c in G.TABLES["refused"]} == {"refused(-2)", "refused(-3)"}
        assert {G.expected_kernel(c, sw) for c in G.TABLES["empty"]} == {"empty"}
    ids = [G.case_id(c) for t in G.TABLES.values() for c in t]
    assert len(ids) == len(set(ids)), "two cases with one id (and so one seed)"


@pytest.mark.parametrize("fam", G.KERNEL_FAMILIES)
def test_every_family_has_its_edges(fam):
    t = G.TABLES[fam]
    tm, tn = TILE[fam]

    def rows(c):
        return c["I"] if c["kind"] == "tn" else c["M"]

    def cols(c):
        return c["J"] if c["kind"] == "tn" else c["N"]
    assert any(rows(c) > tm and rows(c) % tm for c in t), "no M / I tail behind a full tile"
    assert any(cols(c) > tn and cols(c) % tn for c in t), "no N / J tail behind a full tile"
    assert any(rows(c) == 1 for c in t) and any(cols(c) == 1 for c in t), "no single-element extent"
    if fam in ("tn", "tn_tr"):
        assert any(c["M"] == 1 for c in t), "no single reduction row"
    for c in t:
        ext_a, ext_b = (c["I"], c["J"]) if c["kind"] == "tn" else (c["K"], c["K"])
        assert c["lda"] > ext_a and c["ldb"] > ext_b and c["ldc"] > cols(c), "a pitch equal to its extent: %s" % G.case_id(c)
        assert G.reduction(c) <= 1024
    for k in FAMILY_KERNELS[fam]:
        mine = [c for c in t if G.expected_kernel(c) == k]
        step = G.tile_step(k)
        one = [c for c in mine if G.reduction(c) == step and c.get("nsplit", 1) == 1]
        many = [c for c in mine if G.reduction(c) > step]
        assert many, "%s: no reduction of more than one step" % k
        assert one, "%s: no reduction of exactly one step (%d)" % (k, step)


def test_tn_tr_tables_deal_the_units_the_issue_names():
    t = G.TABLES["tn_tr"]
    assert {1, 3, 8, 9, 18} <= {G.tn_units(c) for c in t}
    # a middle range with rows and an empty last one; several empty ranges
    shapes = [[e > b for b, e in G.tn_ranges(c["M"], c["nsplit"])] for c in t]
    assert any(len(s) >= 3 and s[1] and not s[-1] for s in shapes)
    assert any(s.count(False) >= 2 for s in shapes)
    assert any([e > b for b, e in G.tn_ranges(c["M"], c["nsplit"])].count(False) >= 2 for c in G.TABLES["tn"] if c["dt"] == G.BF16)


def test_skinny_iterations_half_one_and_one_and_a_half():
    per_wave = {(c["dt"], c["K"] // 4) for c in G.TABLES["skinny"]}
    assert {(G.BF16, 64), (G.BF16, 128), (G.BF16, 192), (G.F32, 64), (G.F32, 128), (G.F32, 192)} <= per_wave


# ---------------------------------------------------------------------------------------------------------------- data condition --
@pytest.mark.parametrize("fam", G.KERNEL_FAMILIES)
def test_every_live_element_is_compared(fam):
    for c in G.TABLES[fam]:
        d = G.make_data(c)
        ref, bd = G.reference(c, d)
        n = (c["I"] * c["J"]) if c["kind"] == "tn" else c["M"] * c["N"] * (c["K"] // 128 if c["kind"] == "slab" else 1)
        assert ref.numel() == n == d["live"].size and n > 0, G.case_id(c)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bd).all()) and bool((bd > 0).all()), G.case_id(c)
        assert np.unique(d["live"]).size == n


# ---------------------------------------------------------------------------------------------------------------------- mutations --
class FakeAdapter(object):
    """a "kernel" that is the float64 reference (rounded once to the output type), with one defect"""

    def __init__(self, defect=None):
        self.defect = defect

    def run(self, c, bufs):
        d = G.make_data(c)                                  # the same values: the data of a case depends on the case alone
        out, _ = G.reference(c, d)
        out = out.clone()
        A, B, k = d["A"], d["B"], self.defect
        C = bufs["C"].copy()
        live = d["live"]
        if k == "rows swapped":
            out[[0, 1]] = out[[1, 0]]
        elif k == "last K-step dropped in one 32-row block":
            assert c["act"] == 0
            out[32:64] -= c["alpha"] * A[32:64, c["K"] - 32:] @ B[:c["N"], c["K"] - 32:].t()
        elif k == "padding NaN added":
            pad = bufs["A"][c["a_off"] + c["K"]]            # the first padding element of row 0
            out[0, 0] += float(pad if bufs["A"].dtype == np.float32 else G.bf16_to_f32(np.array([pad]))[0])
        elif k == "one range added twice":
            b, e = G.tn_ranges(c["M"], c["nsplit"])[1]
            out += A[b:e, :c["I"]].t() @ B[b:e, :c["J"]]
        elif k == "accumulate ignored":
            out -= d["C0"]
        o32 = out.to(torch.float32).numpy()
        if G.c_is_f32(c):
            stored = o32
        elif k == "bf16 truncated":
            stored = (o32.view(np.uint32) >> 16).astype(np.uint16)
        else:
            stored = f32_to_bf16(o32)
        keep = np.ones(live.shape, bool)
        if k == "tail column unwritten":
            keep[1, -1] = False
        C[live[keep]] = stored[keep]
        if k == "write into the padding":
            C[d["c_off"] + 2 * c["ldc"] + c["N"]] = C[live[0, 0]]
        return 0, C


NT_BF = G.nt_case("nt", G.BF16, 0, 0, 0, 129, 33, 96, 0, 0.25, 1, 0)
NT_SHORT = G.nt_case("nt", G.BF16, 0, 0, 0, 129, 33, 32, 0, 1.0, 0, 0)
NT_ACC = G.nt_case("nt", G.BF16, 0, 1, 0, 127, 33, 160, 0, 1.0, 1, 1)
TN_SPLIT = G.tn_case("tn", G.BF16, 1, 0, 130, 100, 50, 3, 1)
MUTATIONS = [("rows swapped", NT_BF), ("last K-step dropped in one 32-row block", NT_BF), ("tail column unwritten", NT_BF),
             ("write into the padding", NT_BF), ("padding NaN added", NT_BF), ("one range added twice", TN_SPLIT),
             ("accumulate ignored", NT_ACC), ("bf16 truncated", NT_SHORT)]


@pytest.mark.parametrize("defect,case", MUTATIONS, ids=[m[0].replace(" ", "_") for m in MUTATIONS])
def test_the_checker_catches(defect, case):
    good = G.run_case(FakeAdapter(), case)
    assert G.failure(good) is None, G.failure(good)
    bad = G.run_case(FakeAdapter(defect), case)
    print(G.failure(bad))
    assert G.failure(bad) is not None
    if defect == "write into the padding":
        assert bad["guards"] == 1 and bad["worst"] <= 1.0
    else:
        assert bad["guards"] == 0 and bad["worst"] > 1.0


@pytest.mark.parametrize("fam", G.FAMILIES)
def test_the_undamaged_fake_passes_and_wrong_return_codes_do_not(fam):
    class Rc(FakeAdapter):
        def run(self, c, bufs):
            return (0 if c["expect"] == "refused" else -2), bufs["C"]
    for c in G.TABLES[fam][::7] if fam in G.KERNEL_FAMILIES else G.TABLES[fam]:
        if c["expect"] == "ok":
            res = G.run_case(FakeAdapter(), c)
            assert G.failure(res) is None, G.failure(res)
        assert G.failure(G.run_case(Rc(), c)) is not None
