"""-m gpu: lxo_attention_locate on the MI355X through liblxo.so, on the case matrix of tests/attention_locate_ref.py exactly as the hipsim file runs
it: peak, box and S exact on the dyadic maps, edges valid within the f32 summation bound elsewhere, stats within their derived bounds, coverage
bit for bit, all between guard words; every output alone; runs repeated; the refusals; the call captured into a graph and replayed on other maps.
The largest deviations met, as fractions of their bounds, are printed for profiles/attention_locate.txt."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from latex_ocr_amd import _abi
from latex_ocr_amd.engine import _p
from attention_locate_ref import CASE_NAMES, LIMIT, SEEN, check_locate_case, check_outputs, coverage_ref, named, run_locate


class Dev(object):
    """numpy <-> the GPU for the shared runner of tests/attention_locate_ref.py"""
    stream = None

    @staticmethod
    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def ptr(a):
        return _p(a)

    @staticmethod
    def down(a):
        return a.cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_location_matrix(lib, name):
    check_locate_case(lib, named(name), Dev)
    print("largest deviation / bound so far: " + ", ".join("%s %.3e" % kv for kv in sorted(SEEN.items())))


def test_each_output_alone_and_runs_repeat(lib):
    for name in ("3x5 TBR", "2x65 BTR", "14x62 BTR", "98x98 TBR"):
        c = named(name)
        rc, full = run_locate(lib, c, 0.9, Dev)
        assert rc == 0
        for want in (("peak",), ("box",), ("stats",), ("coverage",), ("box", "coverage"), ("stats", "coverage")):
            rc, one = run_locate(lib, c, 0.9, Dev, want=want)
            assert rc == 0 and list(one) == list(want) and all(one[k].tobytes() == full[k].tobytes() for k in want), (name, want)
        rc, again = run_locate(lib, c, 0.9, Dev)
        assert rc == 0 and all(again[k].tobytes() == full[k].tobytes() for k in full), name
        rc, wide = run_locate(lib, c, 0.9, Dev, want=("coverage",), cov_ld=c["R"] + 5)
        assert rc == 0 and np.array_equal(wide["coverage"][:, :c["R"]], coverage_ref(c)) and (wide["coverage"][:, c["R"]:] == -7).all()


def test_refusals_launch_nothing(lib):
    c = named("3x5 BTR")
    cases = [(-1, dict(alpha=None)), (-1, dict(mass=0.0)), (-1, dict(mass=float("nan"))), (-1, dict(mass=1.5)), (-1, dict(ss=-1)), (-1, dict(rs=-1)),
             (-1, dict(rows=-1)), (-1, dict(steps=-1)), (-1, dict(alpha_rows=-1)), (-1, dict(cov_ld=c["R"] - 1)), (-5, dict(Hp=0)), (-5, dict(Wp=0)),
             (-5, dict(Hp=LIMIT + 1, Wp=1)), (-5, dict(Hp=98, Wp=100))]
    for code, kw in cases:
        cov_ld = kw.pop("cov_ld", None)
        rc, got = run_locate(lib, c, kw.pop("mass", 0.9), Dev, cov_ld=cov_ld, **kw)
        torch.cuda.synchronize()
        assert rc == code and lib.lxo_last_error() and all((v == -7).all() for v in got.values()), (code, kw)
    assert run_locate(lib, c, 0.9, Dev, want=())[0] == -1


def test_the_call_is_captured_into_a_graph(lib):
    """both launches on the capturing stream: a replay gives the eager call's bytes, and on other maps what the definition gives on them"""
    c, other = named("14x62 TBR"), named("14x62 BTR")
    R, rows, steps = c["R"], c["rows"], c["steps"]
    buf = torch.from_numpy(c["buf"]).cuda()
    rc, eager = run_locate(lib, c, 0.9, Dev)
    assert rc == 0
    peak = torch.full((rows, steps), -7, dtype=torch.int32, device="cuda")
    box = torch.full((rows, steps, 4), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((rows, steps, 8), -7, dtype=torch.float32, device="cuda")
    cov = torch.full((rows, R), -7, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = lib.lxo_attention_locate(_p(buf), c["strides"][0], c["strides"][1], c["alpha_rows"], c["Hp"], c["Wp"], rows, steps, None, None, 0.9,
                                      _p(peak), _p(box), _p(stats), _p(cov), R, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    got = dict(peak=peak.cpu().numpy(), box=box.cpu().numpy(), stats=stats.cpu().numpy(), coverage=cov.cpu().numpy())
    assert all(got[k].tobytes() == eager[k].tobytes() for k in got)
    # other maps in the same buffer, the same layout: the first alpha_rows rows of the BTR case's maps
    maps = other["maps"][:rows]
    nb = np.full(c["buf"].shape, np.nan, np.float32)
    nb[:, :, :R] = maps.transpose(1, 0, 2)
    buf.copy_(torch.from_numpy(nb).cuda())
    g.replay()
    torch.cuda.synchronize()
    from attention_locate_ref import MapRef
    refs = [[MapRef(maps[i, t], c["Hp"], c["Wp"]) for t in range(steps)] for i in range(rows)]
    c2 = dict(c, name="14x62 replayed", maps=maps, refs=[[m if m.has else None for m in row] for row in refs])
    check_outputs(c2, 0.9, dict(peak=peak.cpu().numpy(), box=box.cpu().numpy(), stats=stats.cpu().numpy(), coverage=cov.cpu().numpy()))
