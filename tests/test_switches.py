"""The library's environment switches live in ONE table (csrc/switches.hip).  A source scan keeps that table, DESIGN.md's table of it and
the tests that hold each arm in step, and keeps the removed switches out of the tree."""
import os, re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "latex_ocr_amd", "csrc")

# arms that no file under tests/ sets, each with its reason.  An arm that loses its test, or a new arm without one, fails test (c).
UNHELD = {
    "LXO_ATT_EXP": "no test sets it; taking it out would reach the `false` instantiations of the chains in xdec.hip: a decision of its own",
    "LXO_WGRAD_HALO": "no test sets it; its other arm is the kernel that lxo_launch_conv_wgrad's refusals (-2) fall back to, so it cannot go",
    "LXO_XDEC": "no test sets it; its other arm, the launch-per-step kernels, is what step_kernels = 2 and the shapes no chain takes run in the suite",
    "LXO_XDEC_DEC": "no test sets it; as LXO_XDEC, for the greedy-decode chain alone (batches that are not 8 / 16 / 32 / 64, f32)",
    "LXO_XDEC_BWD": "no test sets it; as LXO_XDEC, for the backward chain alone",
}
REMOVED = ("LXO_ATT_SPLIT", "LXO_ATT_BWD2", "LXO_ATT_BEAM_SHARED", "LXO_ATT_U", "LXO_XDEC_U", "LXO_ATT_WGS", "LXO_WG_MINBLK", "LXO_WG_STAGGER",
           "LXO_C1_CAP", "LXO_C1_CAPF", "LXO_POOLBWD_CAP", "LXO_ATT_PIPE", "LXO_ATT_ABL")


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _files(*tops):
    for top in tops:
        for d, dirs, names in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("build", "__pycache__", "golden")]
            for n in names:
                if n.endswith((".py", ".hip", ".h", ".cpp", ".sh", ".map", ".md", ".json")) or n == "Makefile":
                    yield os.path.join(d, n)


def _table():
    """{name: kind} of the rows of kSwitches"""
    rows = re.findall(r'^\s*\{"(LXO_\w+)",\s*(arm|value|live),\s*-?\d+\},', _read(os.path.join(CSRC, "switches.hip")), re.M)
    assert len(rows) == len(set(n for n, _ in rows)) and rows
    return dict(rows)


def test_getenv_in_one_file():
    hits = [os.path.basename(p) for p in _files(os.path.join("latex_ocr_amd", "csrc")) if "getenv(" in _read(p)]
    assert hits == ["switches.hip"], hits


def test_design_table_matches_source():
    doc = re.findall(r"^\| `(LXO_\w+)` \| (arm|value|live) \|", _read(os.path.join(ROOT, "DESIGN.md")), re.M)
    assert dict(doc) == _table() and len(doc) == len(_table())
    enum = re.search(r"enum LxoSwitch \{(.*?)\}", _read(os.path.join(CSRC, "switches.h")), re.S).group(1)
    ids = [x.strip() for x in enum.split(",") if x.strip()]
    assert ids == ["SW_" + n[4:] for n in _table()] + ["SW_COUNT"]          # the table is indexed by the enum: same order


def test_every_arm_is_held_or_listed():
    text = "\n".join(_read(p) for p in _files("tests") if p.endswith(".py") and os.path.abspath(p) != os.path.abspath(__file__))
    set_in_tests = set(re.findall(r"""["'](LXO_\w+)["']\s*[:,=]\s*["']0["']|\b(LXO_\w+)=["']0["']""", text))
    set_in_tests = {a or b for a, b in set_in_tests}
    arms = {n for n, k in _table().items() if k == "arm"}
    assert arms - set_in_tests == set(UNHELD), (sorted(arms - set_in_tests), sorted(UNHELD))


def test_removed_switches_are_gone():
    pat = re.compile(r"\b(%s)\b" % "|".join(REMOVED))
    hits = [(os.path.relpath(p, ROOT), m.group(1)) for p in _files("tests", "tools", "latex_ocr_amd")
            if os.path.abspath(p) != os.path.abspath(__file__) for m in [pat.search(_read(p))] if m]
    assert not hits, hits
