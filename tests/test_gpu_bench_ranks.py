"""bench.py's N>1 entry with ALL its legs (--full: headline, roofline + hbm_ops, bf16 variant, augment
variant, eval variants, CPU baseline) on one MI355X: `bench.py --gpus 2 --full` run directly starts the
torch.distributed.run child itself, both ranks on cuda:0 over gloo (MX_BENCH_REHEARSE=1; the real
N>1 run is one rank per GPU over RCCL). Every leg that all-reduces gradients must run on every rank,
or the ranks' collectives pair wrongly and the run hangs: the test asserts the run ends, with one JSON
line from rank 0 carrying n_gpus=2, roofline, hbm_ops and cpu_baseline. This process makes no GPU
call (the launcher is a child process). Reference: train_frcnn_augmented.py:120-216."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(200)
def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the headline fields only (no other leg ran),
    K timed steps, ms_per_step consistent with value; --dump-outputs leaves the last step's losses and the
    parameter / gradient samples as finite float32 arrays well under 64 MB. A second run with the same
    arguments (a new process: the conv tuner's choices are pinned by bench_tune.json) writes the same bits."""
    import numpy as np
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MX_BENCH_DP", "MX_BENCH_REHEARSE",
              "MX_BENCH_TUNE_TABLE", "MX_CONV_TUNE"):
        env.pop(k, None)

    def plain(out):
        r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                            "--warmup", "1", "--dump-outputs", str(out)], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=90)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-3000:]
        return json.loads(lines[0])

    rec = plain(tmp_path / "out")
    assert rec["config"]["conv_tuner"].startswith("bench_tune.json")
    assert rec["metric"] == "images/sec FRCNN-R50-FPN train @1333x800 bs=2/GPU" and rec["unit"] == "images/sec"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f32" and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] / 2000.0 - 1) < 1e-3
    for key in ("roofline", "hbm_ops", "cpu_baseline", "bf16_variant", "augment_variant", "eval_variant",
                "eval_restored_variant"):
        assert key not in rec, key
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["grads_sample.npy", "loss_box_reg.npy", "loss_classifier.npy", "loss_objectness.npy",
                     "loss_rpn_box_reg.npy", "loss_total.npy", "params_sample.npy"]
    arrs = {f: np.load(tmp_path / "out" / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) < 64 * 2 ** 20
    parts = sum(float(arrs[f]) for f in files if f.startswith("loss_") and f != "loss_total.npy")
    assert abs(parts - float(arrs["loss_total.npy"])) <= 1e-6 * abs(parts)  # an f32 sum of four terms: 3 * 2^-24
    assert arrs["params_sample.npy"].shape == arrs["grads_sample.npy"].shape and np.abs(arrs["grads_sample.npy"]).max() > 0
    plain(tmp_path / "again")
    assert sorted(os.listdir(tmp_path / "again")) == files
    for f in files:
        assert np.array_equal(arrs[f], np.load(tmp_path / "again" / f)), f


@pytest.mark.timeout(560)
def test_bench_two_ranks_default_flags():
    # the launching shell's OMP_NUM_THREADS (16 on the GPU boxes) is left as it is: the CPU baseline must
    # pick its thread count itself (bench.host_threads), not inherit torchrun's per-rank default of 1
    env = dict(os.environ, MX_BENCH_REHEARSE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
                        "--warmup", "2", "--full"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["parallelism"] == "dp2" and rec["config"]["global_batch"] == 4
    assert rec["value"] > 0 and rec["steps"] == 2 and rec["warmup"] == 2
    for key in ("roofline", "hbm_ops", "cpu_baseline", "bf16_variant", "augment_variant", "eval_variant",
                "eval_restored_variant"):
        assert key in rec, key
    assert rec["roofline"]["frac"] > 0 and "roi_align_fwd" in rec["hbm_ops"]
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["kind"] == "port"
    assert rec["cpu_baseline"]["cores"] > 1, rec["cpu_baseline"]
    assert "roofline" in rec["bf16_variant"]
