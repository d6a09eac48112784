"""bench.py's launch logic (CPU): `python bench.py --gpus N` with no launcher environment must start its own ranks (VERDICT round 5:
the bare command exited with rc 1 -- "launch with torch.distributed.run" -- before touching a GPU), keep working under torchrun, and
offer the single-process form.  No GPU work here: subprocess.run and the device count are doubled."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch):
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run_main(bench, monkeypatch, argv, env, visible):
    calls = []

    class Done:
        returncode = 0

    def fake_run(cmd, env=None, **kw):
        calls.append((cmd, env))
        return Done()

    import subprocess
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: visible)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MDTILE_BENCH_LAUNCHER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit) as ex:
        bench.main()
    return ex.value.code, calls


@pytest.mark.parametrize("visible", [1, 8])
def test_bare_command_spawns_its_own_ranks(bench, monkeypatch, visible):
    code, calls = _run_main(bench, monkeypatch, ["--gpus", "8", "--steps", "20", "--warmup", "5"], {}, visible)
    assert code == 0 and len(calls) == 1
    cmd, env = calls[0]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    tail = cmd[i + 1:]
    assert tail[:6] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    # one GPU for eight ranks: the flow still runs, every rank on cuda:0 over gloo; eight GPUs: nothing is added
    assert ("--debug-single-device" in tail) == (visible < 8)
    assert env["MASTER_ADDR"] == "127.0.0.1" and env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and "bench.py" in env["MDTILE_BENCH_LAUNCHER"]


def test_a_failing_child_fails_the_parent(bench, monkeypatch):
    import subprocess

    class Bad:
        returncode = 3

    monkeypatch.setattr(subprocess, "run", lambda *a, **k: Bad())
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert ex.value.code == 3


def test_mismatched_launcher_environment_is_refused_with_both_forms_named(bench, monkeypatch):
    code, calls = _run_main(bench, monkeypatch, ["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, 8)
    assert not calls and isinstance(code, str) and "python bench.py --gpus 4" in code and "torch.distributed.run" in code


def test_single_process_refuses_a_launcher_environment(bench, monkeypatch):
    code, calls = _run_main(bench, monkeypatch, ["--gpus", "4", "--single-process"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"}, 8)
    assert not calls and isinstance(code, str) and "ONE process" in code


def test_no_gpu_is_a_loud_error_not_a_cpu_run(bench, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert "MI355X" in str(ex.value.code)


def test_plain_run_leaves_out_the_untimed_passes(bench, monkeypatch):
    """A plain run drops every untimed pass; `--full` runs them all, and a --no-* option still drops its own pass from a --full run."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"])
    args = bench.parse()
    assert not args.full and all(getattr(args, k) for k in bench.FULL_PASSES)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--full", "--no-f32-pass"])
    args = bench.parse()
    assert args.full and args.no_f32_pass and not any(getattr(args, k) for k in bench.FULL_PASSES if k != "no_f32_pass")
