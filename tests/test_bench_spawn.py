"""CPU, 2 ranks over gloo: `bench.py --gpus 2` launches its own ranks (torch.distributed.run), runs the data-parallel
training step (device-side token count, bucketed gradient all-reduce hooks) and rank 0 prints ONE JSON line whose
n_gpus equals --gpus.  --sim swaps RCCL for gloo and the gfx950 kernels for their hipsim build (TEST ONLY)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_spawns_two_ranks_and_reports_them():
    from simlib import build_sim
    build_sim()
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--sim", "--steps", "1", "--warmup", "0"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [x for x in r.stdout.decode().splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 4 and out["config"]["parallelism"] == "dp2"
    assert out["scaling"] == "weak" and out["steps"] == 1 and out["value"] > 0


def test_bench_dump_outputs_hold_the_last_timed_step(tmp_path):
    """--dump-outputs DIR writes the last timed step's loss, weights and gradient as float .npy files, under 64 MB.  Warm-up and timed
    steps are the same call and the hipsim build is deterministic, so 1 warm-up + 1 timed step and 0 + 2 must dump identical arrays --
    weights two Adam steps away from the initial ones -- and the result line counts the --steps it was given."""
    import numpy as np
    from simlib import build_sim
    from latex_ocr_amd.model import params as PP
    build_sim()
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["OMP_NUM_THREADS"] = "2"
    dumps = []
    for steps, warmup in ((1, 1), (2, 0)):
        d = str(tmp_path / ("steps%d" % steps))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sim", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", d],
                           cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out = json.loads([x for x in r.stdout.decode().splitlines() if x.startswith("{")][-1])
        assert out["steps"] == steps and out["ms_per_step"] > 0
        files = sorted(os.listdir(d))
        assert files == out["dump_outputs"]["files"] == ["grads.npy", "loss.npy", "loss_stats.npy", "params.npy"]
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) < 64e6
        a = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
        assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
        assert a["params"].size == a["grads"].size == out["dump_outputs"]["n_params"]
        assert a["loss"][0] == a["loss_stats"][0] / a["loss_stats"][1] and a["loss"][0] > 0
        dumps.append(a)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
    dims = dict(PP.DEFAULT_DIMS, C=128, E=128, U=128, O=128, D=16)          # bench.py --sim: V = 11, these dims, seed 0
    P0 = PP.init_params(11, 0, dims)
    init = np.concatenate([np.asarray(P0[k], np.float32).reshape(-1) for k, _, _ in PP.param_specs(11, dims)])
    assert init.size == dumps[0]["params"].size and not np.array_equal(init, dumps[0]["params"])
