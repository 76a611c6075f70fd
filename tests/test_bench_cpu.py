"""bench.py's launch protocol without a GPU: ``--gpus 2`` starts its own two ranks (no external launcher), they
rendezvous over gloo on 127.0.0.1, time a stub step between barriers, take the MAX over ranks, and rank 0 prints
exactly one JSON line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--steps", "5", "--warmup", "2"] + extra,
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_self_launch_two_ranks():
    line = _run(["--gpus", "2"])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["steps"] == 5 and line["warmup"] == 2
    assert line["value"] > 0 and line["scaling"] == "weak" and line["higher_is_better"] is True
    # every rank's own rate, in rank order (a straggler GPU is visible in the driver's first scaling run)
    assert line["rank_order"] == [0, 1] and len(line["per_rank_value"]) == 2 and min(line["per_rank_value"]) > 0


def test_train_mode_protocol_two_ranks():
    """--mode train: the same launch / barrier / MAX protocol around a step that ends in the bucketed gradient all-reduce
    (shard.GradBucket); after the timed updates every rank holds the same parameters."""
    line = _run(["--gpus", "2", "--mode", "train"])
    assert line["mode"] == "train" and line["n_gpus"] == 2 and line["ranks_seen"] == 2
    assert abs(line["param_digest_spread"]) <= 1e-9
    assert line["value"] > 0
    # every rank's own rate in rank order, also in training mode (the driver's scaling run reads it)
    assert line["rank_order"] == [0, 1] and len(line["per_rank_value"]) == 2 and min(line["per_rank_value"]) > 0


def test_train_mode_under_the_drivers_launcher_two_ranks():
    """The driver's own launch line -- python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1
    ... bench.py --gpus 2 -- through the training protocol: one JSON line from rank 0, two per-rank values."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--stub", "--mode", "train",
                        "--gpus", "2", "--steps", "5", "--warmup", "2"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["mode"] == "train" and line["n_gpus"] == 2 and line["ranks_seen"] == 2
    assert line["rank_order"] == [0, 1] and len(line["per_rank_value"]) == 2 and min(line["per_rank_value"]) > 0
    assert abs(line["param_digest_spread"]) <= 1e-9


def test_four_ranks_train_protocol():
    """Four gloo ranks through the training protocol (bucketed all-reduce): every rank reports, the windows are timed on all
    of them (fastest / slowest rank of the reported window in the line), parameters agree afterwards.  (--full: the median
    of several windows.)"""
    line = _run(["--gpus", "4", "--mode", "train", "--full"])
    assert line["n_gpus"] == 4 and line["ranks_seen"] == 4 and abs(line["param_digest_spread"]) <= 1e-9
    assert line["rank_order"] == [0, 1, 2, 3] and len(line["per_rank_value"]) == 4
    t = line["timing"]
    assert t["windows"] >= 3 and t["windows"] % 2 == 1 and len(t["window_ms"]) == t["windows"] and t["steps_per_window"] == 5
    assert 0 < t["rank_ms_per_step_min"] <= t["rank_ms_per_step_max"]
    assert abs(line["ms_per_step"] * 5 - sorted(t["window_ms"])[t["windows"] // 2]) < 1e-2        # the median window is the one reported


def test_single_rank_needs_no_launcher():
    line = _run(["--gpus", "1"])
    assert line["n_gpus"] == 1 and line["ranks_seen"] == 1


def test_world_size_mismatch_is_an_error():
    env = {k: v for k, v in os.environ.items()}
    env.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert p.returncode != 0


def test_kernel_source_hash_tracks_the_sources(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    h = bench.kernel_source_hash()
    assert len(h) == 16 and h == bench.kernel_source_hash()


def test_plain_run_times_exactly_steps():
    """Without --full the timed region is ONE window of exactly --steps steps, and ms_per_step is that window / steps."""
    for extra in (["--gpus", "1"], ["--gpus", "2", "--mode", "train"]):
        line = _run(extra)
        t = line["timing"]
        assert t["windows"] == 1 and t["steps_per_window"] == 5 and len(t["window_ms"]) == 1
        assert abs(line["ms_per_step"] * 5 - t["window_ms"][0]) < 1e-2
        assert len(line["per_rank_value"]) == line["n_gpus"] and min(line["per_rank_value"]) > 0


def test_dump_outputs_is_reproducible(tmp_path):
    """--dump-outputs DIR: the last timed step's result as .npy, the same from run to run with the same arguments."""
    import numpy as np
    runs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        _run(["--gpus", "1", "--dump-outputs", str(d)])
        runs.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert list(runs[0]) == ["output.npy"] and runs[0]["output.npy"].dtype == np.float32
    assert runs[0]["output.npy"].shape == (64, 64)
    assert np.array_equal(runs[0]["output.npy"], runs[1]["output.npy"])


def test_dump_outputs_layout_and_budget(tmp_path):
    """Every distinct tensor once (the flattened last-stage entries alias stage4's), float32 unless float64, and above the
    budget a fixed sample of the large arrays, the same indices every time."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    depth = torch.rand(1, 64, 80, generator=g)
    outs = {"stage1": {"depth": torch.rand(1, 8, 10, generator=g), "attn_weight": torch.rand(1, 8, 8, 10, generator=g)},
            "stage4": {"depth": depth, "hypo": torch.rand(1, 4, 64, 80, generator=g).double()},
            "depth": depth, "count": torch.arange(6)}
    shapes = bench.dump_outputs(outs, str(tmp_path / "all"))
    assert shapes == {"stage1_depth": [1, 8, 10], "stage1_attn_weight": [1, 8, 8, 10], "stage4_depth": [1, 64, 80],
                      "stage4_hypo": [1, 4, 64, 80], "count": [6]}
    assert np.load(tmp_path / "all" / "stage4_hypo.npy").dtype == np.float64
    assert np.load(tmp_path / "all" / "count.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "all" / "stage4_depth.npy"), depth.numpy())
    budget = 16 << 10
    a = bench.dump_outputs(outs, str(tmp_path / "a"), budget=budget)
    b = bench.dump_outputs(outs, str(tmp_path / "b"), budget=budget)
    assert a == b and sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) - 128 for n in a) <= budget
    for n in a:
        assert np.array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy")))
    full = np.load(tmp_path / "all" / "stage4_hypo.npy").reshape(-1)
    part = np.load(tmp_path / "a" / "stage4_hypo.npy")
    assert part.size < full.size and np.isin(part, full).all()
