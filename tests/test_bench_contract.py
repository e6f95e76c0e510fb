"""bench.py driver contract on CPU: torch.distributed.run with 1, 4 and 8 gloo ranks (8 = the
driver's scaling run on a full MI355X node, here on gloo).

The driver runs ``python -m torch.distributed.run --nproc-per-node N bench.py --gpus N``
on one node; this rehearses the same launch (gloo instead of RCCL, tiny net, torch
backend) and checks the single JSON line rank 0 prints: whole-job value, weak-scaling
global batch, and the ``dpN`` parallelism tag.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("nproc", [1, 4, 8])
def test_bench_json_line_under_torchrun(nproc):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "2", "--warmup", "1",
           "--backend", "torch", "--batch", "2", "--filters", "8", "--layers", "3", "--pool", "16",
           "--min-warmup-s", "0.5"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1",
               PYTHONPATH=ROOT)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in out
    assert out["n_gpus"] == nproc and out["steps"] == 2 and out["warmup"] == 1
    assert out["scaling"] == "weak" and out["higher_is_better"] is True
    assert out["config"]["global_batch"] == 2 * nproc
    assert out["config"]["parallelism"] == "dp%d" % nproc
    assert out["value"] > 0
    # diagnostics of the multi-rank run: live process group, per-rank step times, exposed all-reduce
    assert out["world_size"] == nproc and len(out["rank_ms_per_step"]) == nproc
    assert out["dist_backend"] == ("gloo" if nproc > 1 else "none")
    assert "allreduce_exposed_ms_per_step" in out
    assert out["data"].startswith("synthetic: ")  # teacher-labelled pool (learnable labels)
    # at least --warmup steps and at least --min-warmup-s seconds, same count on every rank
    assert out["warmup_steps_run"] >= 1 and (out["warmup_steps_run"] - 1) % 10 == 0 and out["warmup_s"] >= 0.5
    # value is the whole-job rate: global positions over the (max-over-ranks) timed span
    assert abs(out["value"] - 2 * nproc * 2 / (out["ms_per_step"] * 2 / 1e3)) / out["value"] < 0.01


def _plain_bench(extra, env_extra=None, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "2",
           "--filters", "8", "--layers", "3", "--pool", "16", "--min-warmup-s", "0.5"] + extra
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1", PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_plain_launch_starts_the_ranks():
    """`python bench.py --gpus 4` with no torchrun: bench.py supervises 4 ranks itself and the one JSON
    line describes the 4-rank world (before round 6 it silently measured one rank)."""
    p = _plain_bench(["--gpus", "4", "--backend", "torch"])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["world_size"] == 4 and out["dist_backend"] == "gloo"
    assert out["config"]["global_batch"] == 8 and out["config"]["parallelism"] == "dp4"
    assert len(out["rank_ms_per_step"]) == 4


def test_bench_dump_outputs_repeat_and_full(tmp_path):
    """--dump-outputs DIR writes the last timed step's loss, metric, weights and gradients as float32
    .npy files, identical from run to run whatever the (time-based) number of warmup steps; --full is
    accepted and leaves the result line's headline keys in place."""
    import numpy as np

    dumps = []
    for name, extra in (("a", ["--min-warmup-s", "0.0"]), ("b", ["--full"])):
        d = str(tmp_path / name)
        p = _plain_bench(["--gpus", "1", "--backend", "torch", "--dump-outputs", d] + extra)
        assert p.returncode == 0, p.stderr[-3000:]
        out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["full"] is (name == "b")
        for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert key in out
        assert sorted(os.listdir(d)) == ["correct.npy", "grads.npy", "loss.npy", "params.npy"]
        dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)})
    a, b = dumps
    assert out["warmup_steps_run"] > 1  # run b warmed up for 0.5 s, run a for one step
    for f, x in a.items():
        assert x.dtype == np.float32 and np.isfinite(x).all()
        assert np.array_equal(x, b[f]), f
    assert a["params"].shape == a["grads"].shape and a["params"].size > 1000 and a["loss"].shape == (1,)
    assert np.abs(a["grads"]).max() > 0


@pytest.mark.gpu
def test_bench_restore_state_repeats_hip_steps(cuda_device):
    """What --dump-outputs relies on: after bench.restore_trainer_state the HIP trainer repeats the steps
    it took from the saved state bit for bit (master weights, their bf16 packs, schedule position)."""
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from alphago_amd.models.nets import PolicyNet
    from alphago_amd.train.engine import make_policy_trainer

    torch.manual_seed(0)
    B = 16
    tr = make_policy_trainer(PolicyNet(48, board=19, filters_per_layer=64, layers=3), B, 0.03, 1e-3,
                             backend="hip", device=cuda_device)
    g = torch.Generator(device=cuda_device)
    g.manual_seed(5)
    batches = [(torch.randint(0, 2, (B, 48, 19, 19), device=cuda_device, dtype=torch.uint8, generator=g),
                torch.randint(0, 361, (B,), device=cuda_device, dtype=torch.int32, generator=g),
                torch.randint(0, 8, (B,), device=cuda_device, dtype=torch.int32, generator=g)) for _ in range(3)]

    def steps():
        for b in batches:
            loss, corr = tr.step(*b)
        return loss.clone(), corr.clone(), tr.fp.flat.clone(), tr.fp.grad.clone()

    state = bench.trainer_state(tr)
    first = steps()
    later = steps()  # training goes on: different weights
    assert not torch.equal(first[2], later[2])
    bench.restore_trainer_state(tr, state)
    again = steps()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert tr.sched.iterations == 3


def test_bench_refuses_world_mismatch():
    """--gpus 2 inside a 4-rank torchrun world is refused (non-zero exit, no JSON line)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--backend", "torch", "--batch", "2", "--filters", "8", "--layers", "3", "--pool", "16"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1", PYTHONPATH=ROOT)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert "WORLD_SIZE=4" in p.stderr


def test_bench_refuses_missing_gpus():
    """The HIP backend with --gpus 2 and no visible GPU exits 2 with a message instead of running."""
    p = _plain_bench(["--gpus", "2", "--backend", "hip"], timeout=300)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert "GPU(s) are visible" in p.stderr
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_bench_supervisor_forwards_sigterm(tmp_path):
    """A plain `bench.py --gpus 2` stopped with SIGTERM stops its ranks too (no orphaned rank processes)."""
    import signal
    import time

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "torch", "--steps", "100000",
           "--warmup", "1", "--batch", "2", "--filters", "8", "--layers", "3", "--pool", "16", "--min-warmup-s", "0.5"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1", PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         start_new_session=True)
    time.sleep(25)  # ranks started and training
    pgid = os.getpgid(p.pid)
    p.send_signal(signal.SIGTERM)
    try:
        p.wait(timeout=60)
    finally:
        if p.poll() is None:
            os.killpg(pgid, signal.SIGKILL)
    assert p.returncode != 0
    time.sleep(2)
    # every process of the session (launcher + ranks) is gone
    alive = []
    for d in os.listdir("/proc"):
        if d.isdigit():
            try:
                if os.getpgid(int(d)) == pgid:
                    alive.append(int(d))
            except OSError:
                pass
    assert not alive, alive
