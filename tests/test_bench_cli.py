"""bench.py's command line: the launcher contract (`--gpus N` must really start N ranks), --steps
and --dump-outputs.  The last test needs a GPU."""
import importlib.util
import os
import subprocess
import sys
import types

import pytest

from conftest import ROOT


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_flag_without_launcher_spawns_that_many_ranks(monkeypatch):
    bench = _load_bench()
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=7)

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1", "--no-pmc"])
    assert bench.main() == 7  # the children's exit code is passed on
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail == ["--gpus", "4", "--steps", "3", "--warmup", "1", "--no-pmc"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--no-pmc", "--no-cpu"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "refusing" in r.stderr and r.stdout.strip() == ""


def test_dump_outputs_is_passed_to_the_ranks(monkeypatch, tmp_path):
    bench = _load_bench()
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"] = cmd
        return types.SimpleNamespace(returncode=0)

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3", "--dump-outputs", "dump"])
    assert bench.main() == 0
    tail = seen["cmd"][seen["cmd"].index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail[tail.index("--dump-outputs") + 1] == str(tmp_path / "dump")  # the ranks may not share this cwd
    assert tail[tail.index("--steps") + 1] == "3"


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--no-pmc", "--no-cpu"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout.strip() == ""


def test_dump_outputs_stays_within_budget(tmp_path):
    """Whole arrays while they fit; beyond a rank's share of the budget, the same seeded sample of rows every time."""
    import numpy as np
    import torch
    bench = _load_bench()
    x = torch.arange(1000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "one"), "mvn_logpdf", x, 0, 1)
    got = np.load(tmp_path / "one" / "mvn_logpdf.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x.numpy())
    big = torch.arange(3_000_000, dtype=torch.float64)  # 24 MB per rank: more than 1/4 of the budget
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "mvn_logpdf", big, 3, 4)
    a, b = (np.load(tmp_path / d / "mvn_logpdf_rank3.npy") for d in ("a", "b"))
    assert np.array_equal(a, b) and 4 * os.path.getsize(tmp_path / "a" / "mvn_logpdf_rank3.npy") <= bench.DUMP_BUDGET_BYTES
    assert np.all(np.diff(a) > 0) and len(a) > 2_000_000  # rows in index order, the share filled


@pytest.mark.gpu
def test_dump_outputs_are_the_timed_steps_results(tmp_path):
    """--dump-outputs writes the log-densities of the timed launch: the same bits whatever --steps, and for the
    seeded inputs bench.py draws, the oracle's values."""
    import json

    import numpy as np
    import torch
    from oracle import oracle as O
    bench = _load_bench()
    dumps = []
    for steps in (3, 7):
        d = tmp_path / ("s%d" % steps)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", "1", "--no-pmc", "--no-cpu", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps
        assert sorted(os.listdir(d)) == ["mvn_logpdf.npy"]
        dumps.append(np.load(d / "mvn_logpdf.npy"))
    assert dumps[0].dtype == np.float64 and dumps[0].shape == (bench.N_PER_GPU,)
    assert np.array_equal(dumps[0], dumps[1])
    g = torch.Generator(device="cuda").manual_seed(1234)  # rank 0's batch, as bench.py draws it
    X = torch.randn(bench.N_PER_GPU, bench.D, dtype=torch.float64, device="cuda", generator=g)
    idx = np.arange(0, bench.N_PER_GPU, 487)
    Xh = X[torch.from_numpy(idx).cuda()].cpu().numpy()
    want = O.logpdf_hoisted(Xh, np.zeros(bench.D), bench.make_sigma(bench.D, 1))
    assert np.max(np.abs(dumps[0][idx] - want) / np.abs(want)) < 1e-6  # (the suite's RTOL)
