"""-m gpu: `bench.py --dump-outputs` on the headline workload (B = 64, 128x512, V = 500, bf16).  The timed engine runs the ordered-reduction
bf16 mode, so two runs of the same timed path -- two processes -- must write the same loss, weights and gradient bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_headline_dump_is_bit_identical_run_to_run(tmp_path):
    """The second run (--full) also takes the instrumented step (roofline entries) that follows the timed region -- one more training
    step on the same engine: its dump must still equal the plain run's, i.e. be taken before that step."""
    dumps = []
    env = dict(os.environ)
    env.pop("LXO_DETERMINISTIC", None)
    for run, extra in enumerate(([], ["--full", "--no-cpu-baseline", "--no-secondary", "--no-pmc"])):
        d = str(tmp_path / ("run%d" % run))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                            "--dump-outputs", d] + extra,
                           cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out = json.loads([x for x in r.stdout.decode().splitlines() if x.startswith("{")][-1])
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["deterministic"] is True
        assert ("roofline" in out) == (run == 1)                    # the instrumented step ran in the second run only
        if run == 0:                                                # a plain run measures the headline and nothing else
            assert not {"ms_per_step_by_phase", "secondary", "cpu_baseline", "pmc_traffic_per_launch"} & set(out), sorted(out)
        files = out["dump_outputs"]["files"]
        assert sorted(os.listdir(d)) == files == ["grads.npy", "loss.npy", "loss_stats.npy", "params.npy"]
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) < 64e6
        a = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
        assert all(np.isfinite(v).all() for v in a.values())
        dumps.append(a)
    diff = [k for k in dumps[0] if not np.array_equal(dumps[0][k], dumps[1][k])]
    assert not diff, "two runs of the same benchmark command dumped different %s" % diff
