"""float64 reference, case tables and runner of the dense GEMM entry points (lxo_gemm_nt, lxo_gemm_tn, lxo_gemm_slab), for
tests/test_gpu_gemm_paths.py (MI355X) and tests/test_gemm_paths_sim.py (hipsim, coverage, mutation tests of the checker).  The reference is
torch float64 only and never calls the library; it follows tests/encoder_layers_ref.py and tests/decoder_steps_ref.py and uses their bars.

Operands are the values the kernel actually READS: a bf16 operand as stored, an f32 operand of a bf16 kernel rounded to bf16 (the kernels
convert on load with pack_bf2).  With S the float64 sum of the absolute values of an element's terms, an element is held to

    bf16-stored output        |got - ref| <= 2^-8 |ref| + 2^-14 S
    f32 output, bf16 mode     |got - ref| <= 2^-14 S              (every reduction here is <= 1024 long: n 2^-24 S <= 2^-14 S is derivable)
    dt == f32                 |got - ref| <= 2^-20 S
    ReLU                      the bound of its pre-activation
    act == 2                  tanh_dense's first-order bound (1 - v^2) absf S + EPS_T, + 2^-8 |v| where the result is stored as bf16

Data: Gaussian plus a ramp along one index of each operand (a transposed or permuted fragment cannot pass).  The ramps end at 0.5 against a
unit Gaussian, so an element's terms keep both signs and the f32 parity mode's bar (2^-20 S, not derivable as a worst case for 768 terms)
is held for the reason it is held in the model: the rounding errors of an fmaf chain over terms of both signs do not line up.  The NT weights
are scaled by K^-1/2, so that a tanh sees arguments of order 1.  Every operand is a view into a larger buffer in which all the kernel must
not read is NaN: the pitch padding (K..lda; round8(I)..lda for TN, whose kernels read whole 8-column chunks -- columns I..round8(I) hold a
large finite value that must never reach an output), two rows behind the last one and the elements in front of an offset pointer.  C is a
view into a buffer filled with a sentinel bit pattern: the row in front, the pitch padding N..ldc, two rows behind M and a slab's gap
M ldc..slab_stride must come back bit-identical.  Where the kernel overwrites (atomic == 0, NT without accumulate, slabs) the live part starts
as NaN."""
import ctypes
import zlib

import numpy as np
import torch

from encoder_layers_ref import bf16_round, bound, ratio, REL_BF16, ABS_BF16, ABS_F32
from decoder_steps_ref import mm, tanh_dense, EPS_T                                       # noqa: F401  (EPS_T: inside tanh_dense's bound)
from simlib import f32_to_bf16, bf16_to_f32

F32, BF16 = 0, 1
DEFAULT_SWITCHES = dict(nt_dma=1, tn_tr=1)
ARMS_OFF = dict(nt_dma=0, tn_tr=0)
SENT_F32, SENT_BF16 = 0xC2F6E979, 0xC2F7          # -123.456; -123.5
NAN_F32, NAN_BF16 = 0x7FC00000, 0x7FC0
JUNK = 1000.0                                      # TN columns I..round8(I): read by the 8-column chunks, never part of an output
FRONT_SLAB = 17


def round8(x):
    return (x + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------------------------- cases --
def nt_case(fam, dt, a_f32, c_f32, small, M, N, K, act=0, alpha=1.0, bias=True, acc=0, lda=None, ldb=None, ldc=None, off=0, expect="ok"):
    out_f32 = dt == F32 or bool(c_f32)
    return dict(kind="nt", fam=fam, dt=dt, a_f32=a_f32, c_f32=c_f32, small=small, M=M, N=N, K=K, act=act, alpha=float(alpha), bias=bool(bias),
                acc=acc, lda=K + 8 if lda is None else lda, ldb=K + 8 if ldb is None else ldb,
                ldc=(N + (3 if out_f32 else 5)) if ldc is None else ldc, a_off=off, b_off=off, expect=expect)


def slab_case(dt, M, N, K, lda=None, expect="ok"):
    ldc = N + 3
    return dict(kind="slab", fam="slab", dt=dt, a_f32=1, c_f32=1, small=1, M=M, N=N, K=K, act=0, alpha=1.0, bias=False, acc=0,
                lda=K + 4 if lda is None else lda, ldb=K + 8, ldc=ldc, a_off=0, b_off=0, slab_stride=max(M, 0) * ldc + 17, expect=expect)


def tn_case(fam, dt, a_f32, b_f32, M, I, J, nsplit=1, atomic=1, expect="ok"):
    return dict(kind="tn", fam=fam, dt=dt, a_f32=a_f32, b_f32=b_f32, M=M, I=I, J=J, nsplit=nsplit, atomic=atomic,
                lda=round8(max(I, 1)) + 8, ldb=round8(max(J, 1)) + 8, ldc=J + 3, a_off=0, b_off=0, expect=expect)


def case_id(c):
    d = "f32" if c["dt"] == F32 else "bf16"
    if c["kind"] == "tn":
        return "%s-%s-a%db%d-M%d-I%d-J%d-ns%d-at%d" % (c["fam"], d, c["a_f32"], c["b_f32"], c["M"], c["I"], c["J"], c["nsplit"], c["atomic"])
    s = "%s-%s-a%dc%d-M%d-N%d-K%d-lda%d" % (c["fam"], d, c["a_f32"], c["c_f32"], c["M"], c["N"], c["K"], c["lda"])
    if c["kind"] == "nt":
        s += "-act%d-al%g-b%d-acc%d-off%d" % (c["act"], c["alpha"], c["bias"], c["acc"], c["a_off"])
    return s


def a_is_f32(c):
    return c["dt"] == F32 or bool(c["a_f32"])


def b_is_f32(c):
    return c["dt"] == F32 or (c["kind"] == "tn" and bool(c["b_f32"]))


def c_is_f32(c):
    return c["kind"] != "nt" or c["dt"] == F32 or bool(c["c_f32"])


def reduction(c):
    return c["M"] if c["kind"] == "tn" else c["K"]


# ------------------------------------------------------------------------------------------------------------- dispatch mirror --
def _aligned16(c):
    return (c["a_off"] * (4 if a_is_f32(c) else 2)) % 16 == 0 and (c["b_off"] * (4 if b_is_f32(c) else 2)) % 16 == 0


def expected_kernel(c, sw=DEFAULT_SWITCHES):
    """Pure-Python mirror of lxo_launch_gemm_nt / _tn / _slab (csrc/gemm.hip) for the dense operands of the public entry points (no conv, no
    addend / relu_ref / out_pre / colsum, nbatch 1, no det_slab).  -> the kernel instantiation a case is meant for, "empty" or "refused(rc)".
    The operand bases are 16-byte aligned allocations; a_off / b_off are element offsets into them."""
    dt, bf = c["dt"], "f32" if c["dt"] == F32 else "bf16"
    if c["kind"] == "slab":
        # gemm.hip:752 -- K % 128, lda % 4
        if c["K"] % 128 != 0 or c["K"] <= 0 or c["lda"] % 4 != 0:
            return "refused(-2)"
        # gemm.hip:753 -- nothing to write
        if c["M"] <= 0 or c["N"] <= 0:
            return "empty"
        # gemm.hip:755-756
        return "slab<%s>" % bf
    if c["kind"] == "nt":
        a, cf, K = bool(c["a_f32"]), bool(c["c_f32"]), c["K"]
        # gemm.hip:684
        if c["M"] <= 0 or c["N"] <= 0:
            return "empty"
        # gemm.hip:685
        if K % 32 != 0 or K <= 0:
            return "refused(-2)"
        # gemm.hip:687-689 -- `plain` holds for every dense call of the public entry point
        if c["small"] and K % 256 == 0 and (dt == F32 or (a and cf)) and c["lda"] % 4 == 0:
            return "skinny<%s>" % bf
        # gemm.hip:690-694
        if dt == F32:
            return "nt<f32,64x64>" if c["small"] else "nt<f32,128x128>"
        # gemm.hip:700-703
        if c["small"]:
            return "nt<bf16,A=f32,C=f32,64x64>" if (a and cf) else "refused(-3)"
        # gemm.hip:704-709 and gemm_nt_dma.hip:113-115 (-2 = does not qualify: falls through to the register-staged kernel)
        k64 = K % 64 == 0
        if (not a and k64 and not c["acc"] and c["act"] == 0 and c["alpha"] == 1.0 and c["lda"] % 8 == 0 and c["ldb"] % 8 == 0 and _aligned16(c)
                and sw["nt_dma"] and c["M"] * c["lda"] * 2 < 2 ** 31 and c["N"] * c["ldb"] * 2 < 2 ** 31):
            return "nt_dma<%s out>" % ("f32" if cf else "bf16")
        # gemm.hip:710-713
        if a and not cf:
            return "refused(-3)"
        return "nt<bf16,A=%s,C=%s,BK=%d>" % ("f32" if a else "bf16", "f32" if cf else "bf16", 64 if k64 else 32)
    a, b = bool(c["a_f32"]), bool(c["b_f32"])
    # gemm.hip:717
    if c["I"] <= 0 or c["J"] <= 0 or c["M"] <= 0:
        return "empty"
    # gemm.hip:718
    if not c["atomic"] and c["nsplit"] != 1:
        return "refused(-2)"
    # gemm.hip:719-725 -- f32: one row range per tile whatever nsplit says
    if dt == F32:
        return "tn<f32>"
    # gemm.hip:740-745 and gemm_tn_tr.hip:176-178
    if not a and not b:
        if (sw["tn_tr"] and c["atomic"] and c["lda"] % 8 == 0 and c["ldb"] % 8 == 0 and round8(c["I"]) <= c["lda"] and round8(c["J"]) <= c["ldb"]
                and _aligned16(c) and c["M"] * c["lda"] * 2 < 2 ** 31 and c["M"] * c["ldb"] * 2 < 2 ** 31):
            return "tn_tr"
        return "tn<bf16,A=bf16,B=bf16>"
    # gemm.hip:746-748
    return "tn<bf16,A=%s,B=%s>" % ("f32" if a else "bf16", "f32" if b else "bf16")


def tile_step(kernel):
    """the reduction length one main-loop iteration of a kernel covers (skinny: of its four waves together; slab: one slab)"""
    if kernel.startswith("skinny"):
        return 512 if "bf16" in kernel else 256          # K / 4 per wave against 128 (bf16) / 64 (f32) per iteration
    if kernel.startswith("slab"):
        return 128
    if kernel.startswith("nt_dma") or kernel == "tn_tr" or kernel.startswith("tn<bf16"):
        return 64
    if kernel == "tn<f32>":
        return 32
    return 64 if "BK=64" in kernel else 32


def tn_ranges(M, nsplit, step=64):
    """the row ranges of the split kernels (gemm.hip:284-286, gemm_tn_tr.hip:45-46): [(mbeg, mend)], empty ones included"""
    per = ((M + nsplit - 1) // nsplit + step - 1) // step * step
    return [(s * per, min(M, s * per + per)) for s in range(nsplit)]


def tn_units(c):
    return ((c["I"] + 127) // 128) * ((c["J"] + 127) // 128) * c["nsplit"]


# ------------------------------------------------------------------------------------------------------------------------ tables --
# epilogues of the register-staged NT kernel; none of them leaves a bf16-A, K % 64 == 0 case eligible for the DMA kernel
#          act alpha  bias acc
_EPI = [(0, 0.25, 1, 0),      # plain fast path
        (1, 1.0, 0, 0),       # fast path with the ReLU floor
        (2, -1.5, 1, 0),      # general: tanh
        (0, 1.0, 1, 1),       # general: accumulate
        (1, 0.25, 1, 0),
        (0, -1.5, 0, 1),
        (2, 1.0, 0, 0)]


def _nt_table():
    out = []
    mn = [(M, N) for M in (1, 127, 129, 257) for N in (1, 33, 130)]
    i = 0
    for dt, a, cf in ((F32, 1, 1), (BF16, 0, 0), (BF16, 0, 1), (BF16, 1, 1)):
        for ks in ((32, 96, 160), (64, 192)):
            for M, N in mn:
                K = ks[i % len(ks)]
                act, alpha, bias, acc = _EPI[i % len(_EPI)]
                out.append(nt_case("nt", dt, a, cf, 0, M, N, K, act, alpha, bias, acc, lda=K + (8 if i % 2 else 24)))
                i += 1
    # the plain product with alpha == 1 where K % 64 != 0 keeps it away from the DMA kernel, and with f32 A where K % 64 == 0
    out.append(nt_case("nt", BF16, 0, 0, 0, 129, 33, 96, 0, 1.0, 0, 0))
    out.append(nt_case("nt", BF16, 0, 1, 0, 127, 130, 32, 0, 1.0, 1, 0))
    out.append(nt_case("nt", BF16, 1, 1, 0, 129, 130, 64, 0, 1.0, 1, 0))
    return out


def _nt64_table():
    out = []
    i = 0
    for dt in (F32, BF16):
        for M in (1, 63, 64, 65):
            for N in (1, 63, 65, 130):
                K = (128, 160)[i % 2]
                out.append(nt_case("nt64", dt, 1, 1, 1, M, N, K, 2, (1.0, 0.25, -1.5)[i % 3], i % 4 != 3, 0))
                i += 1
        out.append(nt_case("nt64", dt, 1, 1, 1, 65, 65, 32, 2, 1.0, 1, 0))          # one K-step
        out.append(nt_case("nt64", dt, 1, 1, 1, 65, 63, 160, 0, 0.25, 1, 1))        # the accumulate branch
    return out


def _skinny_table():
    out = []
    epi = [(0, 1.0, 1, 0), (2, 0.25, 1, 0), (0, -1.5, 0, 1), (2, 1.0, 0, 0), (0, 0.25, 1, 1), (1, 1.0, 1, 0)]
    i = 0
    for dt in (F32, BF16):
        for M in (1, 31, 33, 64, 65, 100):
            for N in (1, 31, 32, 33, 70):
                K = (256, 512, 768)[i % 3]
                act, alpha, bias, acc = epi[(i // 3) % len(epi)]
                out.append(nt_case("skinny", dt, 1, 1, 1, M, N, K, act, alpha, bias, acc, lda=K + 4, ldb=K + 8, ldc=N + 3))
                i += 1
        i += 1
    return out


def _dma_table():
    out = []
    i = 0
    for M in (1, 127, 128, 129, 300):
        for N in (1, 127, 129, 260):
            K = (64, 128, 192)[i % 3]
            out.append(nt_case("nt_dma", BF16, 0, i % 2, 0, M, N, K, 0, 1.0, (i // 2) % 2, 0, lda=K + 8, ldb=K + 16, off=8))
            i += 1
    return out


def _slab_table():
    out = []
    i = 0
    for M in (1, 63, 64, 65, 70):
        for N in (1, 63, 64, 65, 200):
            out.append(slab_case((F32, BF16)[i % 2], M, N, (128, 384)[(i // 2) % 2]))
            i += 1
    return out


_TN_I, _TN_J, _TN_M, _TN_NS = (1, 100, 128, 136, 257), (1, 50, 128, 200), (1, 63, 64, 65, 130, 1000), (1, 2, 3, 5)


def _tn_table():
    out = []
    i = 0
    for dt, a, b in ((F32, 1, 1), (BF16, 0, 0), (BF16, 1, 0), (BF16, 0, 1), (BF16, 1, 1)):
        both_bf = dt == BF16 and not a and not b
        for I in _TN_I:
            for J in _TN_J:
                M, ns = _TN_M[i % 6], _TN_NS[(i // 6 + i) % 4]
                atomic = 0 if (both_bf or i % 7 == 0) else 1          # bf16 x bf16 stays with the packing kernel only without atomics
                out.append(tn_case("tn", dt, a, b, M, I, J, 1 if not atomic else ns, atomic))
                i += 1
        i += 1
    out.append(tn_case("tn", F32, 1, 1, 32, 136, 50, 1, 1))                  # one 32-row step of the f32 kernel
    out.append(tn_case("tn", F32, 1, 1, 65, 100, 200, 1, 0))
    for a, b in ((1, 0), (0, 1), (1, 1)):
        out.append(tn_case("tn", BF16, a, b, 65, 136, 200, 5, 1))            # ranges 0..64, 64..65 and three empty ones
        out.append(tn_case("tn", BF16, a, b, 64, 100, 50, 1, 0))             # one 64-row step, plain stores
    seen = set()
    return [c for c in out if not (case_id(c) in seen or seen.add(case_id(c)))]          # the rotation already holds one of the explicit cases


def _tn_tr_table():
    out = []
    i = 0
    for I in _TN_I:
        for J in _TN_J:
            out.append(tn_case("tn_tr", BF16, 0, 0, _TN_M[i % 6], I, J, _TN_NS[(i // 6 + i) % 4], 1))
            i += 1
    #                  M    I    J   nsplit     tiles x nsplit = units
    for M, I, J, ns in ((64, 100, 50, 1),       # 1 x 1 = 1: one unit, one 64-row tile
                        (130, 257, 128, 1),     # 3 x 1 = 3
                        (1000, 128, 128, 3),    # 1 x 3 = 3
                        (130, 136, 200, 2),     # 4 x 2 = 8: exactly one unit per XCD run
                        (1000, 257, 128, 3),    # 3 x 3 = 9: runs of 2, the last XCD runs short
                        (1000, 257, 200, 3),    # 6 x 3 = 18: runs of 3, six XCDs used
                        (65, 257, 200, 3),      # 18 units; ranges 0..64, 64..65 and an empty last one
                        (65, 136, 50, 5),       # 10 units; three empty ranges
                        (130, 100, 200, 5)):    # ranges 0..64, 64..128, 128..130, two empty
        out.append(tn_case("tn_tr", BF16, 0, 0, M, I, J, ns, 1))
    return out


def _refused_table():
    return [nt_case("refused", BF16, 0, 0, 0, 65, 33, 40, expect="refused"),                      # NT: K % 32
            nt_case("refused", F32, 1, 1, 0, 65, 33, 48, expect="refused"),
            nt_case("refused", BF16, 1, 0, 1, 33, 33, 128, expect="refused"),                     # bf16 small with f32 A and bf16 C
            tn_case("refused", BF16, 1, 0, 130, 100, 50, 2, 0, expect="refused"),                 # atomic == 0 with two ranges
            tn_case("refused", F32, 1, 1, 130, 100, 50, 2, 0, expect="refused"),
            slab_case(BF16, 33, 65, 96, expect="refused"),                                        # slab: K % 128
            slab_case(F32, 33, 65, 128, lda=130, expect="refused")]                               # slab: lda % 4


def _empty_table():
    return [nt_case("empty", BF16, 0, 0, 0, 0, 33, 64, expect="empty"), nt_case("empty", BF16, 0, 1, 0, 65, 0, 64, expect="empty"),
            nt_case("empty", F32, 1, 1, 1, 0, 33, 256, expect="empty"), nt_case("empty", F32, 1, 1, 0, 65, 0, 32, expect="empty"),
            slab_case(BF16, 0, 65, 128, expect="empty"), slab_case(F32, 33, 0, 128, expect="empty"),
            tn_case("empty", BF16, 0, 0, 0, 100, 50, 2, 1, expect="empty"), tn_case("empty", BF16, 1, 0, 65, 0, 50, 1, 1, expect="empty"),
            tn_case("empty", F32, 1, 1, 65, 100, 0, 1, 0, expect="empty")]


TABLES = {"nt": _nt_table(), "nt64": _nt64_table(), "skinny": _skinny_table(), "nt_dma": _dma_table(), "slab": _slab_table(),
          "tn": _tn_table(), "tn_tr": _tn_tr_table(), "refused": _refused_table(), "empty": _empty_table()}
FAMILIES = list(TABLES)
KERNEL_FAMILIES = FAMILIES[:7]
SWITCHED = ("nt_dma", "tn_tr")           # the tables the LXO_GEMM_NT_DMA=0 LXO_GEMM_TN_TR=0 child runs again


def sim_subset(fam):
    """the cases the interpreter runs: M, N, I, J <= 140 and a reduction of at most 256"""
    return [c for c in TABLES[fam] if max(c.get("N", 0), c.get("I", 0), c.get("J", 0), c["M"]) <= 140 and reduction(c) <= 256]


# -------------------------------------------------------------------------------------------------------------------------- data --
def _alloc(n, dtype, fill_bits):
    """n elements of dtype (np.float32 / np.uint16) on a 64-byte boundary, every element the bit pattern fill_bits"""
    item = np.dtype(dtype).itemsize
    raw = np.empty(n * item + 64, np.uint8)
    o = (-raw.ctypes.data) % 64
    a = raw[o:o + n * item].view(np.uint32 if item == 4 else np.uint16)
    a[:] = fill_bits
    return a.view(dtype)


def _operand(vals, rows_alloc, pitch, off, as_f32, junk_to=0):
    """vals [rows, cols] float32 -> (buffer, the float64 values as stored): NaN in front of `off`, in the pitch padding and in the rows behind"""
    rows, cols = vals.shape
    buf = _alloc(off + rows_alloc * pitch, np.float32 if as_f32 else np.uint16, NAN_F32 if as_f32 else NAN_BF16)
    v = buf[off:].reshape(rows_alloc, pitch)
    stored = vals if as_f32 else f32_to_bf16(vals)
    v[:rows, :cols] = stored
    if junk_to > cols:
        v[:rows, cols:junk_to] = JUNK if as_f32 else f32_to_bf16(np.full((1,), JUNK, np.float32))[0]
    return buf, torch.from_numpy((stored if as_f32 else bf16_to_f32(stored)).astype(np.float64))


def make_data(c):
    """-> dict(bufs = {A, B, C, bias} NumPy buffers for the call, A / B / bias / C0 = float64 tensors of the values the kernel reads (an f32
    operand of a bf16 kernel rounded to bf16), c_off, live = flat indices of the live elements of C in the shape of the reference)"""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    cf32 = c_is_f32(c)
    cdt, sent, nan = (np.float32, SENT_F32, NAN_F32) if cf32 else (np.uint16, SENT_BF16, NAN_BF16)
    Ma = max(c["M"], 1)
    d = dict(bias=None, C0=None)
    if c["kind"] == "tn":
        I, J, ldc = c["I"], c["J"], c["ldc"]
        Ia, Ja = max(I, 1), max(J, 1)
        A = (rng.standard_normal((Ma, Ia)) + np.linspace(0.0, 0.5, Ia)[None, :]).astype(np.float32)
        B = (rng.standard_normal((Ma, Ja)) + np.linspace(0.0, 0.5, Ma)[:, None]).astype(np.float32)
        bA, d["A"] = _operand(A, Ma + 2, c["lda"], c["a_off"], a_is_f32(c), round8(Ia))
        bB, d["B"] = _operand(B, Ma + 2, c["ldb"], c["b_off"], b_is_f32(c), round8(Ja))
        c_off, rows, shape = ldc, Ia, (I, J)
        total = c_off + (Ia + 2) * ldc
        live = c_off + np.arange(I)[:, None] * ldc + np.arange(J)[None, :]
        fresh = not c["atomic"]
    else:
        N, K, ldc = c["N"], c["K"], c["ldc"]
        Na = max(N, 1)
        A = (rng.standard_normal((Ma, K)) + np.linspace(0.0, 0.5, K)[None, :]).astype(np.float32)
        B = ((rng.standard_normal((Na, K)) + np.linspace(0.0, 0.5, Na)[:, None]) / np.sqrt(K)).astype(np.float32)
        bA, d["A"] = _operand(A, Ma + 2, c["lda"], c["a_off"], a_is_f32(c))
        bB, d["B"] = _operand(B, Na + 2, c["ldb"], c["b_off"], b_is_f32(c))
        if c["kind"] == "slab":
            KS = max(K // 128, 1)
            c_off, total, shape = FRONT_SLAB, FRONT_SLAB + KS * c["slab_stride"] + FRONT_SLAB, (K // 128, c["M"], N)
            live = c_off + np.arange(K // 128)[:, None, None] * c["slab_stride"] + np.arange(c["M"])[None, :, None] * ldc + np.arange(N)[None, None, :]
        else:
            c_off, total, shape = ldc, ldc + (Ma + 2) * ldc, (c["M"], N)
            live = c_off + np.arange(c["M"])[:, None] * ldc + np.arange(N)[None, :]
        fresh = not c["acc"]
        if c["bias"]:
            bias = rng.standard_normal(Na).astype(np.float32)
            d["bias"] = torch.from_numpy(bias.astype(np.float64))
    if c["dt"] == BF16:          # what a bf16 kernel makes of an f32 operand
        d["A"], d["B"] = bf16_round(d["A"]), bf16_round(d["B"])
    C = _alloc(total, cdt, sent)
    live = live.reshape(shape).astype(np.int64)
    if c["expect"] == "ok":
        if fresh:
            C.view(np.uint32 if cf32 else np.uint16)[live.ravel()] = nan
        else:
            c0 = rng.standard_normal(shape).astype(np.float32)
            st = c0 if cf32 else f32_to_bf16(c0)
            C[live.ravel()] = st.ravel()
            d["C0"] = torch.from_numpy((st if cf32 else bf16_to_f32(st)).astype(np.float64))
    d["bufs"] = dict(A=bA, B=bB, C=C, bias=bias if c["kind"] == "nt" and c["bias"] else None)
    d["c_off"], d["live"] = c_off, live
    return d


# --------------------------------------------------------------------------------------------------------------------- reference --
def absf_of(c):
    return ABS_F32 if c["dt"] == F32 else ABS_BF16


def reference(c, d):
    """-> (ref, bound), float64, in the shape of d["live"]"""
    A, B, absf = d["A"][:c["M"]], d["B"], absf_of(c)
    rel = 0.0 if c_is_f32(c) else REL_BF16
    if c["kind"] == "tn":
        A, B = A[:, :c["I"]], B[:c["M"], :c["J"]]
        ref, S = mm(A.t(), B)
        if c["atomic"]:
            ref, S = ref + d["C0"], S + d["C0"].abs()
        return ref, bound(ref, S, 0.0, absf)
    B = B[:c["N"]]
    if c["kind"] == "slab":
        parts = [mm(A[:, k:k + 128], B[:, k:k + 128].t()) for k in range(0, c["K"], 128)]
        ref, S = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
        return ref, bound(ref, S, 0.0, absf)
    assert not (c["acc"] and c["act"]), "accumulate with an activation: the tables do not combine them"
    bias = d["bias"] if d["bias"] is not None else torch.zeros(c["N"], dtype=torch.float64)
    if c["act"] == 2:
        v, bd = tanh_dense(A, c["alpha"] * B.t(), bias, absf)
        return v, bd + rel * v.abs()
    pre, S = mm(A, B.t())
    pre, S = c["alpha"] * pre + bias, abs(c["alpha"]) * S + bias.abs()
    if c["acc"]:
        pre, S = pre + d["C0"], S + d["C0"].abs()
    bd = bound(pre, S, rel, absf)
    return (torch.relu(pre) if c["act"] == 1 else pre), bd


# ------------------------------------------------------------------------------------------------------------------------ runner --
def c_offset(c):
    """elements in front of C inside its buffer: one row of sentinels (slabs: FRONT_SLAB elements)"""
    return FRONT_SLAB if c["kind"] == "slab" else c["ldc"]


def invoke(L, c, pA, pB, pC, pbias, stream=None):
    """the entry point of a case on the base addresses (integers) of its buffers -> rc"""
    V = ctypes.c_void_p
    c_off = c_offset(c)
    A = V(pA + c["a_off"] * (4 if a_is_f32(c) else 2))
    B = V(pB + c["b_off"] * (4 if b_is_f32(c) else 2))
    C = V(pC + c_off * (4 if c_is_f32(c) else 2))
    if c["kind"] == "nt":
        return L.lxo_gemm_nt(c["dt"], c["a_f32"], c["c_f32"], c["small"], A, B, C, c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"],
                             V(pbias) if pbias else None, c["act"], ctypes.c_float(c["alpha"]), c["acc"], stream)
    if c["kind"] == "slab":
        return L.lxo_gemm_slab(c["dt"], A, B, C, c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"], ctypes.c_longlong(c["slab_stride"]), stream)
    return L.lxo_gemm_tn(c["dt"], c["a_f32"], c["b_f32"], A, B, C, c["M"], c["I"], c["J"], c["lda"], c["ldb"], c["ldc"], c["nsplit"], c["atomic"],
                         stream)


def _bits(a):
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def run_case(adapter, c, sw=DEFAULT_SWITCHES):
    """One call through adapter.run(case, bufs) -> (rc, C after the call).  -> dict: rc; kernel = expected_kernel; worst = the worst
    err / bound over the live elements and index = where; guards = number of elements outside the live part that changed (for a refused or
    empty call: anywhere) and guard_at = the first one's offset from C; crc of the live part's bits."""
    d = make_data(c)
    before = _bits(d["bufs"]["C"]).copy()
    rc, after = adapter.run(c, d["bufs"])
    after = _bits(np.ascontiguousarray(after).reshape(-1))
    res = dict(rc=rc, kernel=expected_kernel(c, sw), worst=0.0, index=None, guards=0, guard_at=None, crc=0, expect=c["expect"], id=case_id(c))
    changed = after != before
    if c["expect"] == "ok":
        changed[d["live"].ravel()] = False
    res["guards"] = int(changed.sum())
    if res["guards"]:
        res["guard_at"] = int(np.flatnonzero(changed)[0]) - d["c_off"]
    if c["expect"] != "ok" or rc != 0:
        return res
    raw = after[d["live"].ravel()]
    res["crc"] = zlib.crc32(raw.tobytes())
    got = raw.view(np.float32) if c_is_f32(c) else bf16_to_f32(raw)
    got = torch.from_numpy(got.astype(np.float64)).reshape(d["live"].shape)
    ref, bd = reference(c, d)
    res["worst"] = ratio(got, ref, bd)
    if got.numel():
        r = torch.where(torch.isfinite(got), (got - ref).abs() / bd, torch.full_like(ref, float("inf")))
        res["index"] = tuple(int(x) for x in np.unravel_index(int(r.argmax()), tuple(r.shape)))
    return res


def failure(res):
    """None where a result is what its case expects, else one line saying what is not"""
    e = res["expect"]
    if e == "refused":
        bad = res["rc"] == 0
    else:
        bad = res["rc"] != 0
    if not bad and res["guards"] == 0 and res["worst"] <= 1.0:
        return None
    return "%s [%s, expect %s]: rc %d, worst err/bound %.3g at %s, %d guard elements changed (first at C%+d)" % (
        res["id"], res["kernel"], e, res["rc"], res["worst"], res["index"], res["guards"], res["guard_at"] or 0)


def run_table(adapter, fam, cases=None, sw=DEFAULT_SWITCHES, out=print):
    """every case of a family's table; a call that fails where it should run ends the table (nothing more is started behind a failed launch).
    Prints one line per kernel with its worst ratio.  -> (failures, {kernel: (worst, case id)}, crc over the cases' outputs)"""
    fails, worst, crc = [], {}, 0
    for c in (TABLES[fam] if cases is None else cases):
        res = run_case(adapter, c, sw)
        f = failure(res)
        if f:
            fails.append(f)
        if c["expect"] != "refused" and res["rc"] != 0:
            break
        crc = zlib.crc32(b"%08x" % res["crc"], crc)
        if res["worst"] >= worst.get(res["kernel"], (-1.0, ""))[0]:
            worst[res["kernel"]] = (res["worst"], res["id"])
    for k in sorted(worst):
        out("%-8s %-32s worst err/bound %.4f  (%s)" % (fam, k, worst[k][0], worst[k][1]))
    return fails, worst, crc
