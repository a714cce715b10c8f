"""bench.py's rank plumbing without a GPU: `--gpus N` with no WORLD_SIZE starts exactly one
torch.distributed.run child (same arguments, 127.0.0.1 rendezvous) and exits with its code before any
HIP call; a WORLD_SIZE that disagrees with --gpus is refused."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_world_size_mismatch_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2 but --gpus 4" in r.stderr


def test_gpus_n_spawns_launcher(monkeypatch):
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    def no_cuda():
        raise AssertionError("HIP touched before the launcher")

    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.setattr(bench.torch.cuda, "is_available", no_cuda)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3", "--warmup", "1"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd
    assert "--master-addr=127.0.0.1" in cmd and cmd[-6:] == ["--gpus", "8", "--steps", "3", "--warmup", "1"]
    assert cmd[cmd.index("--nnodes=1") + 4].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_cpu_baseline_threads_ignore_torchrun_default(monkeypatch):
    """torch.distributed.run sets OMP_NUM_THREADS=1 in every rank when the variable was unset,
    so a CPU baseline reading torch.get_num_threads() at N>1 timed ONE thread. bench.host_threads()
    picks the host's cores itself."""
    import bench
    for k in ("MX_CPU_THREADS", "MX_HOST_THREADS", "OMP_NUM_THREADS", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    ncpu = len(os.sched_getaffinity(0))
    assert bench.host_threads() == ncpu
    monkeypatch.setenv("WORLD_SIZE", "8")
    monkeypatch.setenv("OMP_NUM_THREADS", "1")  # torchrun's default: not a request
    assert bench.host_threads() == ncpu
    monkeypatch.setenv("MX_HOST_THREADS", "16")  # the launching shell's setting, passed on by _launch_ranks
    assert bench.host_threads() == 16
    monkeypatch.setenv("MX_CPU_THREADS", "6")
    assert bench.host_threads() == 6
    monkeypatch.delenv("MX_CPU_THREADS")
    monkeypatch.delenv("MX_HOST_THREADS")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert bench.host_threads() == 3
    with bench._threads(2) as n:
        assert n == 2
    assert bench.torch.get_num_threads() != 2 or ncpu == 2


def test_dump_outputs_writes_float32_arrays_reproducibly(tmp_path):
    """--dump-outputs' writer on a small CPU module: every loss under its name, the trainable parameters
    and gradients as the same seeded sample on every call (a tensor above DUMP_SAMPLE elements is
    sampled, a smaller one kept whole, a frozen one left out), all float32."""
    import numpy as np
    import bench
    torch = bench.torch
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(80, 64), torch.nn.Linear(64, 3), torch.nn.Linear(3, 2))
    for p in m[2].parameters():
        p.requires_grad_(False)
    m(torch.randn(4, 80)).sum().backward()
    last = {"loss_a": torch.tensor(1.5, dtype=torch.float64), "loss_total": torch.tensor(2.25)}
    bench.dump_outputs(str(tmp_path / "a"), last, m)
    bench.dump_outputs(str(tmp_path / "b"), last, m)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grads_sample.npy", "loss_a.npy", "loss_total.npy", "params_sample.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    assert float(np.load(tmp_path / "a" / "loss_a.npy")) == 1.5
    ps = np.load(tmp_path / "a" / "params_sample.npy")
    assert 80 * 64 > bench.DUMP_SAMPLE and ps.size == bench.DUMP_SAMPLE + 64 + 64 * 3 + 3
    assert np.array_equal(ps[-3:], m[1].bias.detach().numpy())  # a small tensor whole, in order
    assert np.isin(ps[:bench.DUMP_SAMPLE], m[0].weight.detach().numpy()).all()
    assert np.load(tmp_path / "a" / "grads_sample.npy").shape == ps.shape


def test_tune_table_pins_the_conv_tuner(monkeypatch):
    """bench_tune.json seeds mx_det.conv's tuner cache with keys of the form the tuner builds (tuples,
    torch dtypes, bools) and candidates from its own lists; an entry already cached is left alone;
    MX_BENCH_TUNE_TABLE=0 loads nothing; keys survive the JSON round trip."""
    import bench
    from mx_det import conv as mc
    torch = bench.torch
    monkeypatch.setattr(mc, "_tune_cache", {})
    monkeypatch.setenv("MX_BENCH_TUNE_TABLE", "0")
    assert bench.load_tune_table() == 0 and mc._tune_cache == {}
    monkeypatch.delenv("MX_BENCH_TUNE_TABLE")
    n = bench.load_tune_table()
    assert n == len(mc._tune_cache) > 0
    kinds = set()
    for k, cfg in mc._tune_cache.items():
        assert isinstance(k, tuple) and isinstance(k[1], torch.dtype) and isinstance(k[9], tuple), k
        cands = ((mc._WG_CANDS_X3 if k[1] == torch.float32 else mc._WG_CANDS) if k[0] == "wgrad" else
                 (mc._FD_CANDS_X3 if k[1] == torch.float32 else mc._FD_CANDS))
        assert cfg in cands, (k, cfg)
        assert bench._tune_key(bench._tune_key(k, True), False) == k
        kinds.add(k[0])
    assert kinds == {"fwd", "dgrad", "wgrad"}
    k0 = next(iter(mc._tune_cache))
    mc._tune_cache[k0] = "kept"
    bench.load_tune_table()
    assert mc._tune_cache[k0] == "kept"


def test_launcher_passes_the_shell_thread_count(monkeypatch):
    import bench
    seen = {}
    monkeypatch.setattr(bench.subprocess, "call", lambda cmd, env=None: seen.update(env=env) or 0)
    monkeypatch.setenv("OMP_NUM_THREADS", "16")
    monkeypatch.delenv("MX_HOST_THREADS", raising=False)
    bench._launch_ranks(2)
    assert seen["env"]["MX_HOST_THREADS"] == "16"
