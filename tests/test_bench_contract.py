"""bench.py contract on CPU/gloo: `python bench.py --gpus N` is ONE command that starts N rank
processes itself (no external launcher), prints exactly one JSON line (rank 0's) and
propagates the first rank failure after stopping the others."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None, timeout=240):
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    env.pop("MASTER_PORT", None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def test_bench_self_spawns_ranks():
    r = _run(["--gpus", "2", "--model", "tiny", "--seq", "64", "--steps", "2", "--warmup", "1",
              "--dist-backend", "gloo"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["parallelism"] == "zero3-dp2"
    assert out["config"]["zero3_path"] == "sharded"
    assert out["config"]["global_batch"] == 2 * out["config"]["micro_batch"] * out["config"]["grad_accum"]
    assert out["value"] > 0 and out["vs_baseline"] is None  # tiny model: no baseline ratio


def test_bench_zero2_label():
    r = _run(["--gpus", "1", "--model", "tiny", "--seq", "64", "--steps", "1", "--warmup", "1", "--zero", "2"],
             extra_env={"WORLD_SIZE": "1"})
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads(r.stdout.decode().strip())
    assert out["config"]["zero3_path"] is None and out["config"]["parallelism"] == "zero2-dp1"
    assert out["metric"].startswith("tokens/sec tiny ZeRO-2")


def test_bench_dump_outputs_repeatable(tmp_path):
    """`--dump-outputs DIR` writes the last timed step's loss and parameter sample as float32 .npy
    files; the same arguments give the same seeded weights and batches, so two runs write the same
    arrays.  `--full` is accepted and `--steps` is the number of timed steps the record reports."""
    import numpy as np
    outs = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        r = _run(["--gpus", "1", "--model", "tiny", "--seq", "64", "--steps", "3", "--warmup", "1",
                  "--dump-outputs", str(d)] + extra,
                 extra_env={"WORLD_SIZE": "1", "HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"})  # CPU run
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        rec = json.loads(r.stdout.decode().strip())
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        assert "[hb] rank=0 timed step 2 queued" in r.stderr.decode()
        assert "timed step 3 queued" not in r.stderr.decode()
        assert sorted(p.name for p in d.iterdir()) == ["loss.npy", "params_sample.npy"]
        arrs = {p.name: np.load(p) for p in d.iterdir()}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
        assert arrs["loss.npy"].shape == (1,) and arrs["params_sample.npy"].size > 0
        assert abs(float(arrs["loss.npy"][0]) - rec["config"]["final_loss"]) <= 1e-3
        outs.append(arrs)
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k])


def test_bench_rank_failure_stops_all():
    r = _run(["--gpus", "2", "--model", "tiny", "--seq", "64", "--steps", "2", "--warmup", "1"],
             extra_env={"DSA_BENCH_FAIL_RANK": "1"}, timeout=120)
    assert r.returncode == 7
    assert r.stdout.decode().strip() == ""
    assert "rank 1 exited with status 7" in r.stderr.decode()


@pytest.mark.slow
def test_bench_pipeline_onebit_self_spawn():
    r = _run(["--gpus", "4", "--model", "tiny", "--seq", "64", "--steps", "1", "--warmup", "1", "--pipe", "2",
              "--optimizer", "onebitadam"], timeout=400)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads(r.stdout.decode().strip())
    assert out["n_gpus"] == 4 and out["config"]["parallelism"] == "pp2-dp2"


def test_bench_watchdog_ends_a_frozen_job():
    """rank 3 of a 4-rank gloo job freezes (SIGSTOP) at warmup step 1; the
    other ranks block in its collectives.  Their watchdogs (no heartbeat for
    DSA_BENCH_WATCHDOG_S) end them with their last heartbeat and stacks, and the parent stops
    every rank (the stopped one included) and exits non-zero well before any process-group
    timeout."""
    import time
    t0 = time.time()
    r = _run(["--gpus", "4", "--model", "tiny", "--seq", "64", "--steps", "2", "--warmup", "3",
              "--dist-backend", "gloo"],
             extra_env={"DSA_BENCH_STOP_RANK": "3", "DSA_BENCH_WATCHDOG_S": "20"}, timeout=200)
    took = time.time() - t0
    err = r.stderr.decode()
    assert r.returncode != 0, err[-3000:]
    assert took < 150, took
    assert "WATCHDOG" in err, err[-3000:]
    assert "last heartbeat" in err
    assert "[hb] rank=3" in err  # per-rank heartbeat lines
    assert r.stdout.decode().strip() == ""


def test_bench_heartbeats_per_step():
    r = _run(["--gpus", "2", "--model", "tiny", "--seq", "64", "--steps", "2", "--warmup", "1",
              "--dist-backend", "gloo"])
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    err = r.stderr.decode()
    for rank in (0, 1):
        assert f"[hb] rank={rank} warmup 0 done" in err
        assert f"[hb] rank={rank} timed step 1 queued" in err


def test_bench_world8_zero3():
    """the driver's N=8 contract at world 8 (tiny model, gloo), ZeRO-3 sharded
    path; the per-phase heartbeats and the collective counter the watchdog prints are present."""
    r = _run(["--gpus", "8", "--model", "tiny", "--seq", "64", "--steps", "1", "--warmup", "1",
              "--dist-backend", "gloo"], timeout=400)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-3000:]
    out = json.loads(r.stdout.decode().strip())
    assert out["n_gpus"] == 8 and out["config"]["parallelism"] == "zero3-dp8"
    assert out["config"]["global_batch"] == 8 * out["config"]["micro_batch"] * out["config"]["grad_accum"]
    for rank in range(8):
        assert f"[hb] rank={rank} warmup micro 0 bwd done" in err


@pytest.mark.slow
def test_bench_world8_pipe4_onebit():
    """BASELINE config 4 at its real rank count: PP4 x DP2 with 1-bit Adam over gloo."""
    r = _run(["--gpus", "8", "--model", "tiny", "--seq", "64", "--steps", "1", "--warmup", "3", "--pipe", "4",
              "--optimizer", "onebitadam", "--freeze-step", "1"], timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads(r.stdout.decode().strip())
    assert out["n_gpus"] == 8 and out["config"]["parallelism"] == "pp4-dp2"


def test_watchdog_prints_collective_progress():
    from deeperspeed_amd.utils import comm
    line = comm.progress()
    assert line.startswith("collectives issued=")


@pytest.mark.slow
def test_bench_config4_onebit_trains_after_freeze():
    """BASELINE config 4 (PP4 x DP2, 1-bit Adam) diverged in every rehearsal (loss
    11.6 -> 115-1,548) with freeze_step 2 at beta2 0.999.  With the bench's own optimizer block
    (bench.ONEBIT_*: beta2 0.95, freeze after 16 steps, warmup extended past the freeze) the
    compressed timed steps must train: finite, at most +5 % over the first compressed step, below
    the first warmup loss, and not flagged "diverged"."""
    r = _run(["--gpus", "8", "--model", "gpt-neox-125m", "--layers", "4", "--seq", "64", "--micro-batch", "1",
              "--grad-accum", "4", "--steps", "6", "--warmup", "2", "--pipe", "4", "--optimizer", "onebitadam"],
             timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads(r.stdout.decode().strip())
    c = out["config"]
    assert c["optimizer_params"]["freeze_step"] == 16 and c["optimizer_params"]["betas"] == [0.9, 0.95]
    assert c["warmup_steps_run"] == 17  # every timed step is a compressed one
    losses = c["timed_losses"]
    assert all(l == l and abs(l) < 1e4 for l in losses), losses
    assert losses[-1] <= 1.05 * losses[0], losses
    assert losses[-1] < c["first_warmup_loss"], (c["first_warmup_loss"], losses)
    assert out["diverged"] is False


def test_diverged_flag():
    src = open(os.path.join(ROOT, "bench.py")).read()
    # bench.py redirects fd 1 at import; evaluate only the pure helper
    ns = {}
    start = src.index("def diverged(")
    exec(src[start:src.index("\n\n\n", start)], {"DIVERGED_RATIO": 1.2}, ns)
    assert ns["diverged"](11.6, 115.0) and ns["diverged"](11.6, float("nan"))
    assert not ns["diverged"](11.6, 10.9) and not ns["diverged"](11.6, 13.0)
