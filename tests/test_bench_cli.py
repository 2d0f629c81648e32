"""`python3 bench.py --gpus N` as ONE command (`torchrun --nproc-per-node N`): started alone with N > 1 the
script launches its N ranks itself as a child `python -m torch.distributed.run`, before any GPU call, and relays the JSON line.

CPU part: the command the parent builds.  GPU part: the exact command line of the driver with `--gpus 2` on a one-GPU box under the
rehearsal switch (both ranks on device 0, tiles gathered over gloo) -- the protocol only, its numbers mean nothing."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_alone_with_gpus_above_one_it_starts_its_own_ranks(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    class Done:
        returncode = 7

    def fake_run(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return Done()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "5"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("MASTER_PORT", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                                   # the child's exit code is the parent's
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]      # the same arguments, unchanged
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_a_rank_count_that_does_not_match_the_launcher_is_refused(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "does not match WORLD_SIZE" in str(e.value.code)


@pytest.mark.gpu
def test_the_drivers_command_with_two_ranks_on_one_gpu():
    env = dict(os.environ, SDN_REHEARSE_ON_ONE_GPU="1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--size", "200",
           "--no-cpu-baseline", "--no-secondary", "--min-timed-s", "0"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, out.stdout[-3000:]                  # rank 0 prints ONE line
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 4 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["unit"] == "sampled-points/s" and rec["scaling"] in ("strong", "weak")


def test_dumped_outputs_are_float32_and_a_fixed_sample_above_the_cap(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    rng = np.random.default_rng(1)
    image, depth = rng.random((1000, 3), dtype=np.float32), rng.random(1000).astype(np.float64)
    bench.dump_outputs(str(tmp_path / "all"), {"image": image, "depth": depth})
    got_i, got_d = np.load(tmp_path / "all" / "image.npy"), np.load(tmp_path / "all" / "depth.npy")
    assert got_i.dtype == np.float32 and got_d.dtype == np.float32
    assert np.array_equal(got_i, image) and np.array_equal(got_d, depth.astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4000)          # 16 B per ray: 250 of the 1000 rays are kept
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"image": image, "depth": depth})
    a_i, a_d = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "a" / "depth.npy")
    assert a_i.shape == (250, 3) and a_d.shape == (250,) and a_i.nbytes + a_d.nbytes <= 4000
    assert np.array_equal(a_i, np.load(tmp_path / "b" / "image.npy")) and np.array_equal(a_d, np.load(tmp_path / "b" / "depth.npy"))
    rows = [int(np.flatnonzero((image == r).all(1))[0]) for r in a_i]      # the same rays in both arrays, in ray order
    assert rows == sorted(rows) and np.array_equal(a_d, depth[rows].astype(np.float32))


def test_dump_outputs_is_refused_outside_the_render_mode(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--mode", "train", "--dump-outputs", "x"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "render mode only" in str(e.value.code)


def _bench_line(args, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_a_plain_run_times_exactly_its_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    import numpy as np
    args = ["--gpus", "1", "--steps", "8", "--warmup", "1", "--size", "200"]
    rec = _bench_line(args + ["--dump-outputs", str(tmp_path / "a")])
    assert rec["steps"] == 8 and rec["frames_rendered"] == 8 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0 and abs(rec["ms_per_step"] * 8 - rec["timed_region_s"] * 1e3) < 1e-6
    assert rec["value"] > 0 and rec["unit"] == "sampled-points/s" and rec["higher_is_better"] is True and rec["dtype"] == "f16"
    for key in ("roofline", "kernel_times", "cpu_baseline", "latency_ms_one_loop_at_a_time", "reference_shaped", "grid_gather_rate"):
        assert key not in rec, key                                # --full only
    F = rec["config"]["frames_per_loop"]
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("image", "depth", "depth_valid")}
    assert all(a.dtype == np.float32 and a.shape[0] == F * 200 * 200 for a in got.values()) and got["image"].shape[1] == 3
    assert all(np.isfinite(a).all() for a in got.values()) and 0 < got["image"].mean() < 1
    assert 0 < got["depth_valid"].mean() < 1 and not got["depth"][got["depth_valid"] == 0].any()     # rays that miss the box: NaN -> 0
    _bench_line(args + ["--dump-outputs", str(tmp_path / "b")])
    for n, a in got.items():
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{n}.npy"), a)


@pytest.mark.gpu
def test_full_adds_the_per_kernel_and_side_measurements():
    rec = _bench_line(["--gpus", "1", "--steps", "8", "--warmup", "1", "--size", "200", "--full", "--no-cpu-baseline"])
    assert rec["steps"] == 8 and rec["frames_rendered"] == 8
    assert rec["roofline"]["kernel"] and rec["roofline"]["repeats"] >= 1 and rec["kernel_times"]
    assert rec["latency_ms_one_loop_at_a_time"] > 0 and rec["latency_ms_one_frame"] > 0
    assert rec["reference_shaped"]["ms_per_frame"] > 0 and rec["grid_gather_rate"] and "roofline_secondary" in rec
    assert "cpu_baseline" not in rec
