"""bench.py --gpus N started the way the driver starts it (no external launcher): the parent spawns N fresh rank processes
(torch.distributed.run on 127.0.0.1) before touching any device, the ranks shard the batch through
ccsd_amd.distributed.load_sampling_fn_sharded, all-gather the samples, and rank 0's JSON line is the only thing on stdout.
Here the ranks run the product code over the host emulation of the kernels with gloo (`--emulate`, test only): the launcher,
sharding and reporting path is executed end to end on the GPU-less build box."""
import json
import os
import subprocess
import sys

from tests.emu_util import emu_library
from tests.helpers import ROOT


def test_bench_self_launches_two_ranks_on_the_emulation():
    emu_library()                                  # build once, before two ranks race for it
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--emulate", "--steps", "2", "--warmup", "1",
                        "--batch", "4", "--full"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["scaling"] == "weak"
    assert line["config"]["global_batch"] == 8 and line["config"]["finite"] is True
    assert line["value"] > 0 and abs(line["value"] - 8 / line["ms_per_step"]) < 1e-9
    for key in ("metric", "unit", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "roofline", "cpu_baseline"):
        assert key in line
    # per-rank split of the timed region (diagnosis of a scaling curve): PC-step time without the all-gather, and the all-gather
    pr = line["per_rank"]
    assert [r_["rank"] for r_ in pr] == [0, 1]
    for r_ in pr:
        assert r_["ms_per_step"] > 0 and r_["all_gather_ms"] >= 0 and r_["region_ms"] <= line["ms_per_step"] * line["steps"] * 1.001


def test_bench_worker_failure_is_reported():
    """A rank that dies makes the parent exit non-zero (no JSON line)."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--emulate", "--steps", "1", "--warmup", "1",
                        "--batch", "3", "--workload", "qm9_CC", "--event-stride", "1"],
                       capture_output=True, text=True, timeout=900, env=dict(env, CCSD_BENCH_FAIL_RANK="1"), cwd=ROOT)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.strip().startswith("{")]


def _plain_emulated_run(out_dir):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--emulate", "--steps", "2", "--warmup", "1",
                        "--batch", "4", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    """Without --full the line carries the headline figure only (no kernel-event pass, no CPU baseline); --dump-outputs writes
    the timed region's samples, and two runs with the same arguments write the same arrays."""
    import numpy as np

    emu_library()
    lines = [_plain_emulated_run(tmp_path / f"run{i}") for i in (0, 1)]
    for line in lines:
        assert line["steps"] == 2 and line["value"] > 0 and abs(line["value"] - 4 / line["ms_per_step"]) < 1e-9
        assert line["roofline"] is None and line["cpu_baseline"] is None
        assert not [k for k in line if k.startswith("roofline_")]
        assert line["dump_outputs"]["arrays"] == {"x": [4, 9, 4], "adj": [4, 9, 9], "rank2": [4, 36, 466]}
    for name in ("x", "adj", "rank2"):
        a, b = np.load(tmp_path / "run0" / f"{name}.npy"), np.load(tmp_path / "run1" / f"{name}.npy")
        assert a.dtype == np.float32 and np.isfinite(a).all()
        assert np.array_equal(a, b), name


def test_dump_outputs_samples_the_same_complexes_of_every_array_above_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    x, adj = torch.arange(10 * 3, dtype=torch.float32).view(10, 3), torch.arange(10 * 5, dtype=torch.float32).view(10, 5)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 4 * (3 + 5))          # room for 4 of the 10 complexes
    info = bench.dump_outputs(str(tmp_path), ["x", "adj"], [x, adj])
    assert info["complexes"] == 4 and info["of"] == 10
    gx, ga = np.load(tmp_path / "x.npy"), np.load(tmp_path / "adj.npy")
    rows = gx[:, 0] // 3
    assert gx.shape == (4, 3) and ga.shape == (4, 5) and np.all(np.diff(rows) > 0)
    assert np.array_equal(ga, adj.numpy()[rows.astype(int)])
    again = bench.dump_outputs(str(tmp_path / "again"), ["x", "adj"], [x, adj])
    assert again == dict(info, dir=str(tmp_path / "again")) and np.array_equal(np.load(tmp_path / "again" / "x.npy"), gx)
